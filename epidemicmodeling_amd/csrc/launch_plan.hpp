// launch_plan.hpp -- what one call of epi_ekf_run_device / epi_sweep_run_device launches, decided in ONE place.  Plain C++17
// with no HIP in it: plan_launch() turns the descriptor, a few facts about the call's pointers and the SIMD count into a
// LaunchPlan -- the lane mapping, the forward / backward / monitor kernel variants with their LDS bytes, and the schedule as an
// ordered list of operations with their grids, step and chain ranges and streams.  epiekf.hip only follows the list (run_plan);
// tests/launch_plan_test.cpp checks the plan on a CPU.  Every comparison of a size with a threshold belongs here, and the
// function reads nothing but its argument.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/epiekf.h"

namespace epi {
struct ModelInfo { int m, flipped, lo_is_zero, phi_ge, obs_clamp, obs_fixed, generic; };
static const ModelInfo MODEL_TABLE[6] = {
    /* SIA3             */ {3, 0, 0, 0, 1, 0, 1},
    /* SIA6             */ {6, 0, 1, 0, 1, 0, 1},
    /* SIA3_BWD         */ {3, 1, 1, 0, 1, 0, 1},
    /* SIA6_BWD         */ {6, 1, 1, 0, 1, 0, 1},
    /* NEWCASE6         */ {6, 0, 1, 1, 1, 0, 0},
    /* NEWCASE6_CODEGEN */ {6, 0, 1, 1, 0, 1, 0},
};

// chains per wavefront / lanes per workgroup of the kernel families (the kernel headers say how each maps its lanes)
constexpr int kWave = 64;
constexpr int kQC = kWave / 4;   // ekf_quad.hpp: four lanes per chain
constexpr int kHG = 10;          // ekf_hex.hpp: six lanes per chain
constexpr int kW3G = 7;          // ekf_wave.hpp, 3-state models: nine lanes per chain
constexpr int kPipeLanes = 40;   // ekf_sym.hpp: lanes per workgroup of the LP = 1 forward variant
// the lane blocks eks_bwd_lane6 (ekf_lane6.hpp) is instantiated for: the balanced waves (balanced_lanes) of batches beyond one
// round of 64-lane waves -- 40 is the headline's; not 64 (lane6_ok below says why)
constexpr bool lane6_block(int blk) { return blk == 40 || blk == 48 || blk == 56; }
constexpr int pinv_chains(int m) { return m >= 6 ? 64 : 256; }   // chains per eks_pinv workgroup (pinv_wg<M>)
constexpr int kMonitorParDays = 8;       // days per ekf_monitor_par workgroup
// use the scan-free grid (ekf_monitor_par) while the batch has at most TWO 64-chain waves per SIMD (131 072 chains; round 6: the
// headline's 75 000 chains included -- forward stage + monitor 5.45-5.6 against 5.8-6.3 ms, the pass 0.3-0.5 ms shorter in each of
// four alternating runs, profiles/r06/ab_monitor_par.txt; round 5 had it at one)
constexpr int kMonitorParMaxWaves = 2;
// Forward pass in time segments (percent of T where each ends).  pinv(P(k|k-1)) needs nothing but the forward pass's
// output of day k and the smoother consumes X in REVERSE time order, so only the pinv grid of the last segment stands
// between the end of the forward pass and the start of the smoother: the last segments are short.
// (re-measured in round 3 with the cheaper pinv: four segments ending at 50 / 85 / 97 / 100 % give 3.06-3.11 ms against
// 3.12-3.16 for five ending at 40 / 70 / 90 / 98 / 100 % at 9 375 chains, level at 18 750: profiles/r03/time_cuts.txt)
constexpr int kTimeCuts[] = {0, 50, 85, 97, 100};
constexpr int kTimeSeg = (int)(sizeof(kTimeCuts) / sizeof(kTimeCuts[0])) - 1;
constexpr int kRpParts = 3;              // reverse-time pipeline: parts the observed days' smoother steps are cut into
constexpr int kHelperEvents = 16;        // events a helper stream owns; a plan uses n_events of them
constexpr int kMaxPlanOps = 32;

static inline int lane_block_of(const epi_batch_desc *d) { return (d->lane_block <= 0 || d->lane_block >= d->B) ? d->B : d->lane_block; }

// The innovation monitor leaves the forward kernels (ekf_monitor, ekf_quad.hpp) when R_v is a per-day series -- then rho
// feeds nothing back -- and two double-written L-sample windows per lane fit the default dynamic-LDS limit.
static inline bool monitor_hoisted(const epi_batch_desc *d)
{
    return MODEL_TABLE[d->model].generic && d->r_mode == 1 && d->q_mode == 0 && d->path_hint != 2 &&
           (size_t)4 * d->L * kWave * sizeof(double) <= 64u * 1024u;
}
// Which lane mapping runs the 6-state generic models (epi_batch_desc.shape).  Auto: four lanes per chain while every
// quad wavefront (16 chains) still gets a SIMD of its own, i.e. up to 16 384 chains on MI355X -- there the chains'
// per-day latency is what counts and the quad kernels' instruction stream is half as long (9 375 chains: 3.5 instead of
// 6.1 ms per pass); beyond that the quad waves (one per SIMD at ~290 registers) would run in rounds and one lane per
// chain, the shape with the least total work, wins (18 750 chains: 6.1 against 8.4 ms).  profiles/r02/batch_size_sweep.txt.
// Round 4: one WAVEFRONT per chain (ekf_wave.hpp) while every chain can have a SIMD of its own (B <= 1024 on MI355X): a lone
// wave's day costs ~0.6 us there against 2.1-2.2 us for a quad wave, at ~4 x the quad shape's total VALU work.  It needs the
// innovation monitor as its own kernel (R_v a per-day series) and a fixed Q_w; otherwise four lanes per chain.
static inline int shape_of(const epi_batch_desc *d, int n_simds)
{
    const ModelInfo &mi = MODEL_TABLE[d->model];
    if (!mi.generic) {
        // NewCaseEKFEstimatorWithOptimalNPI (round 5): one wavefront per chain (ekf_fwd_wave<0, 1, LC, 0>, eks_bwd_wave_nc) while every
        // chain can have a SIMD of its own -- the reference's own callers make ONE call per chain
        // (testScripts/testSIModelOptimalControl04EKS.m:168,302): 2.1 instead of 8.4 ms -- otherwise the dense one-lane kernels
        const bool ok = mi.m == 6 && !d->storage && d->q_mode == 0 && (size_t)6 * d->L * sizeof(double) <= 48u * 1024u;
        if (d->shape == EPI_SHAPE_WAVE) return ok ? EPI_SHAPE_WAVE : EPI_SHAPE_LANE;
        if (d->shape != EPI_SHAPE_AUTO) return EPI_SHAPE_LANE;
        return (ok && (long)d->B <= (long)n_simds) ? EPI_SHAPE_WAVE : EPI_SHAPE_LANE;
    }
    if (d->storage) return EPI_SHAPE_LANE;
    if (mi.m == 3) {
        // 3-state models: seven chains per wavefront, nine lanes each (ekf_fwd_wave3), for small batches; otherwise one lane
        // per chain.  There is no four-lane shape for them.  Measured (BASELINE config 3's chains x 400 days, ms per pass,
        // wave / lane): 300 chains 0.91 / 1.04, 2 000 1.09 / 1.20, 7 000 1.47 / 1.26, 20 000 3.08 / 1.80 -- a 3-state step is
        // bound by its scalar chain (state map, the 12-term NPI sum, two divisions: ~1.4 us per day in EITHER shape), the
        // 3 x 3 algebra the wave shape spreads over nine lanes is a small part of it.  Chosen up to 2 048 chains.
        const bool ok = monitor_hoisted(d);
        if (d->shape == EPI_SHAPE_WAVE) return ok ? EPI_SHAPE_WAVE : EPI_SHAPE_LANE;
        if (d->shape == EPI_SHAPE_LANE || d->shape == EPI_SHAPE_QUAD || d->shape == EPI_SHAPE_HEX) return EPI_SHAPE_LANE;
        return (ok && d->B <= 2048) ? EPI_SHAPE_WAVE : EPI_SHAPE_LANE;
    }
    // the hex shape needs the monitor as its own kernel (R_v a per-day series) and a fixed Q_w -- and at least a few days of
    // every array within the 2 GiB its addressing windows span (ekf_hex.hpp, hx_window): 288 B and 8 n_npi B per chain and day
    const bool hex_ok = monitor_hoisted(d) && (long)d->B <= (1L << 20) && (long)d->n_npi * d->Su <= (1L << 25);
    // the wave shape also runs the monitor inline (a scalar, possibly adaptive R_v: ekf_fwd_wave<FLIP, 1>, round 5)
    const bool wave_ok = hex_ok || (mi.generic && d->r_mode == 0 && d->q_mode == 0 && d->path_hint != 2 &&
                                    (size_t)6 * d->L * sizeof(double) <= 48u * 1024u);
    if (d->shape == EPI_SHAPE_WAVE) return wave_ok ? EPI_SHAPE_WAVE : EPI_SHAPE_QUAD;
    if (d->shape == EPI_SHAPE_HEX) return hex_ok ? EPI_SHAPE_HEX : EPI_SHAPE_QUAD;
    if (d->shape == EPI_SHAPE_QUAD || d->shape == EPI_SHAPE_LANE) return d->shape;
    // (round 5: with the hex shape there, one wavefront per chain wins only up to ~600 chains: 300 chains 1.59 against 1.81 ms per
    // call, 1 024 chains 2.15 against 1.84 -- profiles/r05/shape_latency.json; where the hex shape cannot run, up to one chain per SIMD)
    if (wave_ok && (long)d->B <= (hex_ok ? (long)n_simds * 5 / 8 : (long)n_simds)) return EPI_SHAPE_WAVE;
    // round 5: six lanes per chain, ten chains per wavefront (ekf_hex.hpp) up to TWO such wavefronts per SIMD (20 480 chains on
    // MI355X; beyond one per SIMD its kernels run two waves per SIMD, a third does not fit their registers): 9 375 chains -- the
    // shard of the headline sweep on one of 8 GPUs -- 2.6 ms against 3.2 (quad) and 4.9 (lane); 18 750 chains (one of 4 GPUs)
    // 5.1 against 5.6 (lane), 20 480 chains 5.5 against 5.7, 20 500 chains 6.5 against 5.8: profiles/r05/ab_hex_threshold.txt
    // (with the kernels' day offsets in the scalar offset; before that the shapes were level at 18 750)
    if (hex_ok && ((long)d->B + kHG - 1) / kHG <= 2 * (long)n_simds) return EPI_SHAPE_HEX;
    return ((long)d->B + kQC - 1) / kQC <= (long)n_simds ? EPI_SHAPE_QUAD : EPI_SHAPE_LANE;
}

// Lanes per wave for the one-chain-per-lane kernels.  `waves_per_simd` waves of such a kernel fit a SIMD (1 for the
// 6-state kernels, 2 for the 3-state ones).  6 states: if cn/64 waves exceed what is resident at once, the launch would run
// in rounds and the last round would leave most SIMDs idle while its few waves are limited by what ONE compute unit
// can pull from memory; narrower waves, a multiple of 8 lanes (64-byte segments), make every round equally full.
// 3 states: always full 64-lane waves.  Their arrays have 3 and 9 rows, so a wave writes 1.3 / 4 KB per array and step, and
// chunks that small only reach the HBM's rate when every row is a whole number of cache lines (64 lanes = 512 B):
// profiles/layout_probe/run_rows.py measures 4.7 / 5.2 TB/s for 3- / 9-row chunks of 56 lanes against 6.2 / 6.3 TB/s with 64
// (with 12 rows and more the width stops mattering), and BASELINE config 5 runs 20.6 -> 17.5 ms with full waves although its
// last round is a third full (profiles/r03/README.md).
static inline int balanced_lanes(int cn, int waves_per_simd, int n_simds)
{
    if (waves_per_simd >= 2) return kWave;
    const long cap = (long)n_simds * waves_per_simd;
    const long w64 = (cn + kWave - 1) / kWave;
    if (w64 <= cap) return kWave;
    const long rounds = (w64 + cap - 1) / cap;
    long lw = (cn + rounds * cap - 1) / (rounds * cap);
    lw = (lw + 7) / 8 * 8;
    return (int)(lw > kWave ? kWave : lw);
}

// ---- the plan
enum PlanStream { ON_MAIN = 0, ON_HELPER = 1 };
enum FwdKernel { FWD_NONE = 0, FWD_WAVE_NC, FWD_WAVE, FWD_WAVE3, FWD_HEX, FWD_QUAD, FWD_SYM };
enum BwdKernel { BWD_NONE = 0, BWD_WAVE_NC, BWD_WAVE, BWD_WAVE3, BWD_HEX, BWD_QUAD, BWD_LANE6, BWD_SYM };
enum MonKernel { MON_NONE = 0, MON_PAR, MON_SCAN };
// the template arguments a kernel family branches on
enum : unsigned {
    V_L21 = 1u,      // the window length the specialisations are compiled for
    V_BLK = 2u,      // hex: 10-chain layout blocks; quad: 16-chain blocks (forward: and L = 21)
    V_SOLO = 4u,     // hex / quad: every wave can have a SIMD of its own: keep it that way (hex smoother: prefetch; beyond: two waves per SIMD)
    V_INLINE = 8u,   // the forward kernel runs the innovation monitor itself (not hoisted)
    V_STOR = 16u,    // fp32 storage
    V_LP = 32u,      // sym forward: model constants in LDS, LDS sized by kPipeLanes lanes
    V_USD = 64u,     // sym forward, reduced outputs: the variant that fits two waves per SIMD
};
// FwdKernel / BwdKernel / MonKernel, V_* bits, chains one workgroup covers, dynamic LDS bytes
struct KernelPick { int kernel; unsigned bits; int wg_chains; unsigned lds; };
enum ScheduleBits : unsigned {        // 0: serial, one stage after the other on the caller's stream
    SCHED_OVERLAP = 1u,               // a full call on the packed kernels: a helper stream takes what is off the critical path
    SCHED_TIME_PIPE = 2u,             // forward kernel in time segments, the pinv grid of each beside the next
    SCHED_REVERSE_PIPE = 4u,          // smoother in time segments, the pinv grids of the earlier days beside the later days' smoother
    SCHED_FWD_RANGES = 8u,            // forward kernel and pinv grid in two chain ranges
    SCHED_BWD_ROUNDS = 16u,           // smoother in two chain ranges with the monitor between them
    SCHED_BWD_HORIZON = 32u,          // smoother cut where the horizon ends, the scoring tail beside the observed days
};
enum PlanOpKind { OP_FWD, OP_PINV, OP_BWD, OP_MONITOR, OP_TAIL, OP_RECORD, OP_WAIT };
struct PlanOp {
    int kind, stream;            // PlanOpKind; ON_MAIN: the caller's stream, ON_HELPER: the leased helper stream
    int a, b;    // OP_FWD: filter steps [a, b); OP_PINV: b array positions from pinv_pos0 + a on; OP_BWD: smoother steps a, a-1, ..., b; OP_RECORD / OP_WAIT: event a
    int c0, cn;                  // chain range
    unsigned grid, dense_grid;   // workgroups (x) of the picked kernel (OP_PINV: of eks_pinv) and of the dense one
    int xd;                      // OP_BWD, eks_bwd_lane6<., 40, XD>: X by LDS-DMA where every lane of the launch is alive
};
struct PlanIn {
    const epi_batch_desc *d;     // validated
    int n_simds;
    bool smooth, rerun;          // the call runs the smoother / the dense second pass of exact_nonfinite
    int hint, ws_upper;          // 0: ekf_precheck decides, 1: packed kernels, 2: dense kernels; KArgs.ws_upper
    bool want_rho, only;         // rho is an output (fp64 or fp32); this IS the dense second pass (KArgs.only is set)
    bool has_tail; int t_hist;   // the sweep's scoring tail
};
// The plan's input of ONE call, from the descriptor, the SIMD count and what the call's pointers say: are pinv_rank / status
// outputs, and the sweep's scoring tail with its t_hist.  run_device_impl (epiekf.hip) and the plan query of the tests
// (tests/plan_query.cpp) both come through here, so a test that asks which kernels a call launches asks the call's own question.
static inline PlanIn plan_call_input(const epi_batch_desc *d, int n_simds, bool has_pinv_rank, bool has_status, bool has_tail, int t_hist)
{
    const ModelInfo &mi = MODEL_TABLE[d->model];
    const bool f32 = d->storage == 1;
    const uint32_t sel = d->out_mask, om = f32 ? 0u : d->out_mask;   // selected in either storage; the fp64 outputs among them
    PlanIn in{}; in.d = d; in.n_simds = n_simds;
    // exact_nonfinite: 1 = always (runs the smoother to find the chains, whatever is selected); 0, the default = whenever the call
    // runs the smoother anyway; -1 = never
    const bool smooth_sel = (sel & (EPI_OUT_S_SMOOTH | EPI_OUT_P_SMOOTH)) || (mi.generic && (sel & EPI_OUT_U_OPT_SMOOTH)) ||
                            has_pinv_rank || has_status;
    in.rerun = mi.generic && (d->exact_nonfinite > 0 || (d->exact_nonfinite == 0 && smooth_sel)) && d->q_mode == 0 && d->phase == 0 && !f32;
    // (exact_nonfinite needs the smoother's guard to find the chains: it runs the smoother whatever is selected)
    in.smooth = smooth_sel || in.rerun;
    in.hint = (mi.generic && d->q_mode == 0) ? d->path_hint : 2;      // a time-varying Q_w is read per step by the dense kernels only
    // fp32 storage: every fp64 forward quantity the kernels see is workspace, upper triangles only
    in.ws_upper = ((om & EPI_OUT_P_MINUS) ? 0 : 1) | ((om & EPI_OUT_P_PLUS) ? 0 : 2);
    in.want_rho = (sel & EPI_OUT_RHO) != 0;
    in.has_tail = has_tail; in.t_hist = has_tail ? t_hist : 0;
    return in;
}
struct LaunchPlan {
    bool overflow;              // the lists below did not fit (never for a validated descriptor; launch_plan_test)
    int shape, chains_per_wave;  // EPI_SHAPE_*; chains a wave of that shape holds (what epi_ekf_preferred_lane_block answers)
    int lw, quad, wave, hex, mon_hoist;   // KArgs fields of the same names
    unsigned schedule;           // ScheduleBits
    int precheck;                // -1: none; dense_flag is cleared, then 0: nothing, 1: ekf_precheck over the batch, 2: set
    bool helper, dense;          // lease a helper stream; the dense kernels are enqueued (behind the packed ones with hint 0)
    KernelPick fwd, bwd, mon;
    unsigned dense_lds, mon_gx, mon_gy;   // ekf_fwd's LDS bytes; the monitor's grid
    bool rerun_after;            // then the dense second pass of exact_nonfinite (rerun_nonfinite_dense)
    int n_ops, n_events;
    PlanOp ops[kMaxPlanOps];
};

static inline LaunchPlan plan_launch(const PlanIn &in)
{
    const epi_batch_desc *d = in.d;
    const ModelInfo &mi = MODEL_TABLE[d->model];
    const int M = mi.m, B = d->B, T = d->T, L = d->L, phase = d->phase, blk = lane_block_of(d), nblk = (B + blk - 1) / blk;
    const long S = in.n_simds;
    const bool generic = mi.generic != 0, stor = d->storage == 1;
    LaunchPlan p{}; p.shape = shape_of(d, in.n_simds);
    p.lw = balanced_lanes(B, M == 6 ? 1 : 2, in.n_simds); p.wave = p.shape == EPI_SHAPE_WAVE;
    // (the dense second pass runs one lane per chain and its own monitor)
    p.quad = !in.only && p.shape == EPI_SHAPE_QUAD; p.hex = !in.only && p.shape == EPI_SHAPE_HEX; p.mon_hoist = !in.only && monitor_hoisted(d);
    p.chains_per_wave = p.shape == EPI_SHAPE_WAVE ? 1 : (p.shape == EPI_SHAPE_HEX ? kHG : (p.shape == EPI_SHAPE_QUAD ? kQC : p.lw));
    const bool lane = !p.wave && !p.quad && !p.hex, hoist = p.mon_hoist != 0;
    // hint 0: both variants are enqueued, the one ekf_precheck did not select returns at once
    p.dense = !generic || in.hint != 1;
    p.dense_lds = (unsigned)((size_t)3 * L * kWave * sizeof(double));
    const unsigned l21 = L == 21 ? V_L21 : 0u, inl = hoist ? 0u : V_INLINE;
    const unsigned win6 = (unsigned)((size_t)6 * L * sizeof(double));      // the wave shape's inline monitor windows
    const long fwd_waves = p.hex ? ((long)B + kHG - 1) / kHG : p.quad ? ((long)B + kQC - 1) / kQC : ((long)B + kWave - 1) / kWave;   // of the forward kernel
    const unsigned solo = fwd_waves <= S ? V_SOLO : 0u;
    // One lane per chain with fixed descriptors per addressing window (ekf_lane6.hpp): the layout block must be the lanes a
    // workgroup uses, and a compile-time constant
    // (not for 64-chain blocks: four workgroups' LDS columns would not fit a CU, and where three suffice -- one round of 64-lane
    // waves, the N = 2 shard of the headline sweep: 37 500 chains -- the kernel measured 3.84 against eks_bwd_sym's 3.5 ms:
    // such a batch is not issue-bound, profiles/r06/ab_n2_shard.txt)
    const bool lane6_ok = M == 6 && generic && lane && !stor && lane6_block(blk) && (long)blk * nblk <= (1L << 20);
    if (!generic && p.wave && !in.only) {      // NewCaseEKFEstimatorWithOptimalNPI, one wavefront per chain (monitor always inline)
        p.fwd = {FWD_WAVE_NC, l21, 1, win6};
        p.bwd = {BWD_WAVE_NC, 0u, 1, 0u};
        p.dense = false;
    } else if (generic && in.hint != 2) {
        if (p.wave && M == 6) {        // one wavefront per chain (ekf_wave.hpp); with a scalar R_v the monitor runs inline
            p.fwd = {FWD_WAVE, inl | l21, 1, hoist ? 0u : win6};
            p.bwd = {BWD_WAVE, 0u, 1, 0u};
        } else if (p.wave) {           // seven chains per wavefront, nine lanes each
            p.fwd = {FWD_WAVE3, 0u, kW3G, 0u};
            p.bwd = {BWD_WAVE3, 0u, kW3G, 0u};
        } else if (p.hex) {            // six lanes per chain, ten chains per wavefront (ekf_hex.hpp)
            p.fwd = {FWD_HEX, (blk == kHG ? V_BLK : 0u) | solo, kHG, 0u};
            p.bwd = {BWD_HEX, (blk == kHG ? V_BLK : 0u) | solo, kHG, 0u};
        } else if (p.quad) {
            // four lanes per chain, 16 chains per wavefront (ekf_quad.hpp): the specialisation for the layout and the
            // window length this shape is meant for, or the general one; with an inline monitor its windows are in LDS
            const unsigned qshm = (unsigned)(((size_t)(hoist ? 0 : 6 * L) + EPI_MAX_NPI) * kQC * sizeof(double));
            p.fwd = {FWD_QUAD, ((blk == kQC && L == 21) ? V_BLK : 0u) | inl | (hoist ? solo : 0u), kQC, qshm};
            p.bwd = {BWD_QUAD, blk == kQC ? V_BLK : 0u, kQC, 0u};
        } else {
            // narrow (balanced) waves: the variant with LDS-resident model constants and LDS sized by 40 lanes -- 298
            // instead of 408 VGPRs (a third of the AGPR traffic), still four workgroups per CU
            const size_t per_lane = ((size_t)3 * L + 4 * EPI_MAX_NPI) * sizeof(double);
            const bool lp = !stor && M == 6 && p.lw <= kPipeLanes && per_lane * kPipeLanes * 4 <= 160u * 1024u;
            // (Measured and not adopted, round 5: a 3-state forward kernel with a, u_max in LDS and a day's controls consumed on
            // arrival -- 166 registers, THREE clean waves per SIMD -- took 11.4-11.8 ms on BASELINE config 5 against 8.8-9.5 for the
            // 224-register kernel at two: the 24 LDS reads a day on the alpha map's dependent chain cost more than the third wave
            // returns, profiles/r05/ab_cfg5_three_waves.txt.)
            // hoisted: no windows in LDS, only the LP variant's model vectors; reduced outputs: the variant that fits two waves per SIMD
            const unsigned lds = hoist ? (lp ? (unsigned)((size_t)4 * EPI_MAX_NPI * kPipeLanes * sizeof(double)) : 0u)
                                       : (lp ? (unsigned)(per_lane * kPipeLanes) : p.dense_lds);
            p.fwd = {FWD_SYM, inl | (stor ? V_STOR : 0u) | (lp ? V_LP : 0u) | (lp && hoist && in.ws_upper == 3 ? V_USD : 0u), p.lw, lds};
            p.bwd = lane6_ok ? KernelPick{BWD_LANE6, 0u, blk, 0u} : KernelPick{BWD_SYM, stor ? V_STOR : 0u, p.lw, 0u};
        }
    }
    // the innovation monitor as its own launch (after the forward kernel that wrote the innovations)
    const bool mon = hoist && in.want_rho;
    if (mon) {
        const long mb = p.mon_gx = (unsigned)(((long)B + kWave - 1) / kWave);
        if (L == 21 && !((d->test_flags >> 1) & 1) && mb <= kMonitorParMaxWaves * S) {
            p.mon = {MON_PAR, V_L21, kWave, 0u};
            p.mon_gy = (unsigned)((T + kMonitorParDays - 1) / kMonitorParDays);
        } else {
            // time segments (each pays a 2L-2-step warm-up): enough of them that the grid gives every SIMD about eight of these
            // light waves (a lane's 100-step scan is latency-bound: 0.70 ms with two segments, 0.25 ms with eight at 75 000 chains),
            // none shorter than ~64 steps
            long nseg = (8 * S + mb - 1) / mb;
            const long max_seg = T / 64 > 1 ? T / 64 : 1;
            nseg = nseg < 1 ? 1 : (nseg > max_seg ? max_seg : nseg);
            p.mon = {MON_SCAN, l21, kWave, (unsigned)((size_t)4 * L * kWave * sizeof(double))};
            p.mon_gy = (unsigned)nseg;
        }
    }
    auto push = [&](int kind, int stream, int a, int b, int c0, int cn) {
        if (p.n_ops >= kMaxPlanOps) { p.overflow = true; return; }
        PlanOp &o = p.ops[p.n_ops++];
        o.kind = kind; o.stream = stream; o.a = a; o.b = b; o.c0 = c0; o.cn = cn;
        if (kind == OP_FWD || kind == OP_BWD) {
            const KernelPick &k = kind == OP_FWD ? p.fwd : p.bwd;
            o.grid = k.kernel ? (unsigned)((cn + k.wg_chains - 1) / k.wg_chains) : 0u;
            o.dense_grid = p.dense ? (unsigned)((cn + p.lw - 1) / p.lw) : 0u;
            o.xd = kind == OP_BWD && k.kernel == BWD_LANE6 && blk == 40 && cn % 40 == 0;
        } else if (kind == OP_PINV) {
            // x extent rounded up to a multiple of 8: the kernel re-orders its tiles so that every XCD gets a contiguous eighth per step
            unsigned tiles = (unsigned)((cn + pinv_chains(M) - 1) / pinv_chains(M));
            if (in.only && tiles > 8u) tiles = 8u;      // the second pass of exact_nonfinite walks the list of marked chains (see eks_pinv)
            o.grid = tiles >= 8u ? ((tiles + 7u) & ~7u) : tiles;
        }
    };
    auto fwd = [&](int k0, int k1, int c0, int cn) { push(OP_FWD, ON_MAIN, k0, k1, c0, cn); };
    auto bwd = [&](int from, int to, int c0, int cn) { push(OP_BWD, ON_MAIN, from, to, c0, cn); };
    // X = pinv(P(j|j-1)) of filter steps j_lo .. j_hi (the smoother needs j = 1 .. T-1); array position of step j: j, or T-1-j
    // for the time-flipped models
    auto pinv = [&](int s, int j_lo, int j_hi, int c0, int cn) { if (j_hi >= j_lo) push(OP_PINV, s, mi.flipped ? (T - 1 - j_hi) : (j_lo - 1), j_hi - j_lo + 1, c0, cn); };
    auto record = [&](int stream) { push(OP_RECORD, stream, p.n_events, 0, 0, 0); return p.n_events++; };
    auto wait = [&](int stream, int ev) { push(OP_WAIT, stream, ev, 0, 0, 0); };
    auto fork = [&](int from, int to) { wait(to, record(from)); };     // `to` continues after what `from` holds now
    auto finish = [&]() { p.overflow |= p.n_events > kHelperEvents; return p; };
    const bool fwd_phase = phase == 0 || phase == 1;
    // hint 0: fast path unless ekf_precheck finds a non-symmetric Ps_init / non-diagonal Q_w in the batch;
    // hint 1 / 2: the caller decided; the flag the kernels test is set accordingly
    p.precheck = (fwd_phase && generic && !in.only) ? (in.hint == 0 ? 1 : (in.hint == 2 ? 2 : 0)) : -1;
    if (!(generic && phase == 0 && in.smooth && in.hint == 1)) {
        // one stage after the other on the caller's stream (single stages for per-kernel timing, the forward pass alone,
        // batches that may take the dense kernels, the NewCase models, the dense second pass)
        if (fwd_phase) fwd(0, T, 0, B);
        if (fwd_phase && mon) push(OP_MONITOR, ON_MAIN, 0, 0, 0, B);
        if (!in.smooth) return finish();
        if (generic && (phase == 0 || phase == 2 || phase == 3)) pinv(ON_MAIN, 1, T - 1, 0, B);
        if (phase == 0 || phase == 2 || phase == 4) bwd(T - 2, 0, 0, B);
        if (phase == 0 && in.has_tail) push(OP_TAIL, ON_MAIN, 0, 0, 0, B);
        p.rerun_after = generic && in.rerun && phase == 0 && in.hint != 2;
        return finish();
    }
    // A full call on the packed kernels.  What does not lie on the critical path runs on a helper stream:
    //   * the innovation monitor (needs the forward pass only) beside the pinv grid and the smoother;
    //   * pipelined in TIME: a batch that does not fill the chip (the shards of the sweep on 2, 4, 8 GPUs) leaves SIMDs idle
    //     while its sequential forward waves crawl through the T days.  The forward kernel then runs in kTimeSeg launches (a
    //     later segment resumes from the S_MINUS / P_MINUS the previous one stored: same bits), and after each of them the
    //     eks_pinv grid of ITS days starts on the helper stream, beside the next forward segment.  Not for a batch that
    //     fills the chip (nothing idles: measured level, round 1);
    //   * the sweep's scoring tail: the horizon's u_opt_smooth is final after the smoother's first T - 1 - t_hist steps,
    //     so the recursion is cut there and scoring + Pareto filter run beside the rest of it.
    p.schedule = SCHED_OVERLAP; p.helper = true;
    const bool tail_cut = in.has_tail && in.t_hist >= 1 && in.t_hist <= T - 2;
    // (one wavefront per chain: the pinv grid of so few chains takes ~30 us, nothing to pipeline -- unless asked for)
    const bool force_split = (d->test_flags >> 2) & 1;                                                 // test hook
    const bool force_rp = (d->test_flags & 1) && p.hex && hoist && T >= 4 && d->time_pipe >= 0;         // test hook
    const bool tp = !force_rp && hoist && !stor && T >= 128 && d->time_pipe >= 0 &&
                    (d->time_pipe == 1 || (!p.wave && fwd_waves * 4 <= S * 3));
    // Pipelined in REVERSE time (round 5, the hex shape): the smoother consumes X = pinv(P(k+1|k)) from the last day backwards, so
    // only the pinv grid of the LAST days has to stand between the forward kernel and the smoother; the grids of the earlier days
    // run on the helper stream beside the smoother's first launches, and the smoother is cut where they end (the hand-over rows of
    // the horizon / observed-days split).  Beside the FORWARD kernel a pinv grid takes exactly what it saves (both want the vector
    // unit: forward segments 1.07 -> 1.50 ms); the smoother of this shape waits on memory most of the time.
    const bool rp = force_rp || (!tp && p.hex && hoist && T >= 128 && d->time_pipe >= 0);
    // (Round 6, measured and not adopted: the hex shape beyond one wavefront per SIMD -- 10 241 .. 20 480 chains, the shard of the headline
    // sweep on one of 4 GPUs -- as TWO chain ranges through the one-wave-per-SIMD kernels, pipelined across the ranges (the pinv grid of
    // the first beside the forward kernel of the second, the grid of the second beside the smoother of the first) instead of the
    // two-waves-per-SIMD kernels pipelined in reverse time: 5.20-5.28 against 4.58-4.80 ms at 18 750 chains, 3.75-3.80 against 3.06-3.09 at
    // 10 375 -- profiles/r06/ab_hex_rounds.txt.)
    bool helper_busy = false;
    if (rp) {
        p.schedule |= SCHED_REVERSE_PIPE;
        fwd(0, T, 0, B); fork(ON_MAIN, ON_HELPER);
        // smoother steps k = T-2 ... 0 in segments [hi, lo], descending: the horizon first when there is a scoring tail, the rest in
        // kRpParts parts; segment s needs X of filter steps lo+1 ... hi+1.  The first grid stays ahead of the smoother on the caller's stream
        int seg_hi[1 + kRpParts], seg_lo[1 + kRpParts], ev_pinv[1 + kRpParts] = {}, ns = 0, tail_seg = -1, top = T - 2;
        if (tail_cut) { seg_hi[ns] = top; seg_lo[ns] = in.t_hist; tail_seg = ns++; top = in.t_hist - 1; }
        const int parts = (top + 1 >= 96 || (force_rp && top + 1 >= 6)) ? kRpParts : 1;
        for (int q = 0; q < parts; q++) {
            const int lo = (int)((long)(top + 1) * (parts - 1 - q) / parts);
            seg_hi[ns] = top; seg_lo[ns] = lo; ns++;
            top = lo - 1;
        }
        for (int s = 0; s < ns; s++) {
            pinv(s == 0 ? ON_MAIN : ON_HELPER, seg_lo[s] + 1, seg_hi[s] + 1, 0, B);
            if (s > 0) ev_pinv[s] = record(ON_HELPER);
        }
        for (int s = 0; s < ns; s++) {
            if (s > 0) wait(ON_MAIN, ev_pinv[s]);
            bwd(seg_hi[s], seg_lo[s], 0, B);
            if (s == tail_seg) {            // the horizon's u_opt_smooth is final: scoring + Pareto filter behind the helper's pinv grids
                p.schedule |= SCHED_BWD_HORIZON;
                fork(ON_MAIN, ON_HELPER);
                push(OP_TAIL, ON_HELPER, 0, 0, 0, B);
            }
        }
        if (in.has_tail && tail_seg < 0) push(OP_TAIL, ON_MAIN, 0, 0, 0, B);
        if (mon) push(OP_MONITOR, ON_HELPER, 0, 0, 0, B);
        helper_busy = true;
    } else {
        // A one-lane batch that runs in ROUNDS of resident waves (more waves than SIMDs: the headline sweep): the chains of the forward
        // kernel's first round and the rest are two launches, and the pinv grid of the first range runs on the helper stream beside
        // the forward kernel of the second (whose 851 waves leave SIMDs and registers free at 75 000 chains; the forward kernel is
        // bound by its stores, the grid by the vector unit): 0.15 ms of the grid's 3.0 hidden (profiles/r06/ab_pinv_beside_fwd.txt).
        // epi_batch_desc.test_flags bit 2 cuts ANY one-lane batch of two waves or more in the middle the same way (test hook).
        const long waves = ((long)B + p.lw - 1) / p.lw;
        const long cA = force_split ? (waves / 2) * p.lw : S * p.lw;
        // (not when neither P(k|k-1) nor P(k|k) is an output: that forward kernel fits TWO waves per SIMD and the headline's 1 875 are
        // resident at once -- cut in two launches it took 1.1 ms longer, bench_cfg4_reduced 13.6 -> 14.7 ms)
        const bool fwd_ranges = M == 6 && lane && cA > 0 && cA < B && (force_split || (p.lw < kWave && in.ws_upper != 3));
        if (tp) {
            p.schedule |= SCHED_TIME_PIPE;
            for (int sg = 0; sg < kTimeSeg; sg++) {
                const int k0 = (int)((long)T * kTimeCuts[sg] / 100);
                const int k1 = (sg == kTimeSeg - 1) ? T : (int)((long)T * kTimeCuts[sg + 1] / 100);
                if (k1 <= k0) continue;
                fwd(k0, k1, 0, B);
                fork(ON_MAIN, ON_HELPER);
                // filter steps whose P(j|j-1) exists now and has not been inverted yet
                pinv(ON_HELPER, k0 + 1, k1 < T ? k1 : T - 1, 0, B);
            }
            fork(ON_HELPER, ON_MAIN);       // the smoother needs every pinv grid
            helper_busy = true;
        } else if (fwd_ranges) {
            p.schedule |= SCHED_FWD_RANGES;
            fwd(0, T, 0, (int)cA);
            fork(ON_MAIN, ON_HELPER);
            pinv(ON_HELPER, 1, T - 1, 0, (int)cA);
            fwd(0, T, (int)cA, B - (int)cA);
            if (mon) fork(ON_MAIN, ON_HELPER);
            pinv(ON_MAIN, 1, T - 1, (int)cA, B - (int)cA);      // beside the tail of the first range's grid
            fork(ON_HELPER, ON_MAIN);
        } else {
            fwd(0, T, 0, B);
            if (mon) fork(ON_MAIN, ON_HELPER);
            pinv(ON_MAIN, 1, T - 1, 0, B);
        }
        // A one-lane batch that runs in ROUNDS (more 64-chain waves than SIMDs: the headline sweep) on the fixed-descriptor smoother:
        // the chains of the smoother's first round of resident waves and the rest are two launches, and the monitor starts between
        // them -- beside the second launch, whose waves leave SIMDs free (851 waves on 1 024 SIMDs at 75 000 chains), instead of
        // beside the pinv grid, which is bound by the vector unit and simply takes 0.44 ms longer with the monitor next to it.
        const bool in_rounds = lane && fwd_waves > S;
        const bool cut = force_split && lane && nblk >= 2;        // test hook: the two launches at any size
        // (a first launch of 1 004 / 984 / 964 / 944 waves instead of the 1 024 that are resident at once: level, 14.41-14.88 ms per pass
        // whatever the cut; the monitor ahead of the first launch instead of between the two: +0.15 ms -- profiles/r06/ab_bwd_balance*.txt)
        const long first_round = cut ? (long)(nblk / 2) * blk : S * blk;
        const bool mon_late = !tp && (in_rounds || cut) && lane6_ok && mon && first_round < B;
        if (!mon_late && mon) { push(OP_MONITOR, ON_HELPER, 0, 0, 0, B); helper_busy = true; }
        // (Not for a one-lane batch that runs in ROUNDS of resident waves -- more 64-chain waves than SIMDs, the headline sweep: every
        // SIMD is taken by a 512-register wave, the tail finds no room beside the smoother and a second launch costs the smoother a
        // second pair of rounds: 15.1-15.9 against 15.6-16.2 ms per pass over four alternating runs, profiles/r06/ab_monitor_par.txt.)
        if (!in_rounds && !mon_late && tail_cut && !p.wave) {
            p.schedule |= SCHED_BWD_HORIZON;
            bwd(T - 2, in.t_hist, 0, B);                // the horizon days
            fork(ON_MAIN, ON_HELPER);
            push(OP_TAIL, ON_HELPER, 0, 0, 0, B); helper_busy = true;
            bwd(in.t_hist - 1, 0, 0, B);                // the observed days
        } else {
            if (mon_late) {
                p.schedule |= SCHED_BWD_ROUNDS;
                bwd(T - 2, 0, 0, (int)first_round);
                fork(ON_MAIN, ON_HELPER);
                push(OP_MONITOR, ON_HELPER, 0, 0, 0, B); helper_busy = true;
                bwd(T - 2, 0, (int)first_round, B - (int)first_round);
            } else bwd(T - 2, 0, 0, B);
            if (in.has_tail) push(OP_TAIL, ON_MAIN, 0, 0, 0, B);
        }
    }
    if (helper_busy) fork(ON_HELPER, ON_MAIN);
    p.rerun_after = in.rerun;
    return finish();
}

}  // namespace epi

// epiekf.hip -- kernels and C ABI of libepiekf.so (see include/epiekf.h).
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared epiekf.hip -o libepiekf.so
//
// Kernels
//   ekf_fwd<M,FLIP,GENERIC>  forward EKF loop, Tools/GenericExtendedKalmanFilter.m:98-186
//                            (GENERIC=0: Tools/NewCaseEKFEstimatorWithOptimalNPI.m:37-113)
//   eks_bwd<M,FLIP,GENERIC>  backward smoother loop, GenericEKF.m:189-230 (NewCase...m:115-139)
// Both keep one chain per lane (ekf_device.hpp); 64-thread workgroups so that the
// B/64 waves spread over the 1024 SIMDs of the chip as evenly as the batch allows.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>
#include "ekf_device.hpp"

namespace epi {

struct KArgs {
    int B, T, Sx, Su, n_npi, L, r_mode;
    int q_mode;   // 1: Q is [T][m*m][B], Q(:,:,k) of filter step k (GenericEKF.m:63-73); dense kernels only
    ModelFlags mf;
    const int32_t *x_series, *u_series;
    const double *x, *u, *R_series, *R_scalar, *prm;
    const double *s_init, *Ps_init, *s_final, *Ps_final, *Q;   // already swapped for flipped models
    // forward quantities (outputs or workspace; never NULL)
    double *S_MINUS, *S_PLUS, *P_MINUS, *P_PLUS;
    // bit 0 / bit 1: P_MINUS / P_PLUS is workspace, not a caller's output -- the packed kernels then store its upper
    // triangle only (what eks_pinv and eks_bwd_sym read back): 15 of 36 rows less to write per array and step
    int ws_upper;
    // optional outputs (NULL = not stored)
    double *u_opt, *u_opt_smooth, *S_SMOOTH, *P_SMOOTH, *K_GAIN, *innovations, *rho;
    int32_t *pinv_rank, *status;
    // smoother intermediates (workspace): X = pinv(P_MINUS(:,:,k+1)) stored at the position of step k+1,
    // rankbuf = kept rank | sweep-cap flag << 8 (or -1 where the non-finite guard of :211 fired)
    double *X;
    int32_t *rankbuf;
    int pinv_pos0;
    // generic models: word set by ekf_precheck when the batch must take the dense kernels (non-symmetric
    // Ps_init or non-diagonal Q_w); NULL = dense kernels always run (NewCase models)
    int *dense_flag;
    // chain range [c0, c0 + cn) this launch covers (a call may be split into chunks on two streams)
    int c0, cn;
    // chain-blocked layout of the output / workspace arrays (see Lay): lanes per block and blocks per time slice
    int blk, nblk;
    // lanes used per 64-thread workgroup (<= 64).  When the batch needs more than one round of resident waves,
    // the host narrows the waves so that the rounds are equally full (launch_chain): the sequential kernels are
    // bound by HBM / per-CU memory throughput, which scales with active lanes, not by wave count.
    int lw;
    int quad;   // 6-state generic models: four lanes per chain (ekf_quad.hpp) instead of one
    int wave;   // 6-state generic models: one WAVEFRONT per chain (ekf_wave.hpp)
    int hex;    // 6-state generic models: six lanes per chain, ten chains per wavefront (ekf_hex.hpp)
    int hexw;   // hex kernels: days per addressing window (0: as many as 2 GiB hold, see HexWin; the tests set a few days)
    // epi_batch_desc.storage = 1: the caller's outputs are fp32 arrays (same layouts, 4-byte elements); each selected
    // one is the fp64 result rounded once.  The four forward quantities the smoother reads back are then always fp64
    // workspace (S_MINUS ... P_PLUS above) and their fp32 copies are extra stores.  Packed (sym) kernels only.
    int stor;   // 1: fp32 storage (see F32 below)
    int k_begin, k_end;   // filter steps [k_begin, k_end) of this forward launch (k_end <= 0: up to T); eks_pinv: steps from pinv_step0
    int pinv_step0;
    // smoother steps of this backward launch (packed / quad kernels): k = bk_from, bk_from - 1, ..., bk_to.  bk_from = T - 2
    // starts from the terminal condition (:189-202); a later launch resumes from the S_SMOOTH / P_SMOOTH / status word the
    // previous one left in the hand-over workspace (hand_s [m][Bp], hand_p [m*m][Bp], hand_i [Bp]) -- the same bits
    int bk_from, bk_to;
    double *hand_s, *hand_p;
    int32_t *hand_i;
    int hand_pitch;       // Bp: chains the hand-over rows are sized for
    // epi_batch_desc.exact_nonfinite: after the packed kernels, chains whose covariance went non-finite (status bit 0) are
    // run again by the dense kernels, in place.  `only` [B] (workspace): the dense fwd / pinv / bwd launches of that second
    // pass return at once for every chain whose word is 0; only[B] counts the marked chains
    const int32_t *only;
    int32_t *only_buf;
    int mon_defer;   // 1: this launch does not enqueue ekf_monitor itself (the caller does, later)
    int mon_hoist;   // 1: the packed / quad forward kernels skip the innovation monitor, ekf_monitor replays it (r_mode 1)
    int mon_scan;    // test hook (epi_batch_desc.test_flags bit 1): the scan kernel ekf_monitor whatever the batch size
    struct F32 { float *u_opt, *u_opt_smooth, *S_MINUS, *S_PLUS, *S_SMOOTH, *P_MINUS, *P_PLUS, *P_SMOOTH, *K_GAIN, *innovations, *rho; } f;
};

// position in the caller's time axis of filter step k (flipped wrappers run the
// generic filter on time-reversed u/x and reverse every output: Backward*.m:19-40)
template <int FLIP> EPI_DEV int tpos(int k, int T) { return FLIP ? (T - 1 - k) : k; }

// Addressing.  Every array is [T][rows][B] (chain-minor), so an access is
//     slice base (wave-uniform: kernel argument + uniform time index)  +  row * B * 8 (uniform)  +  8 * chain (per lane).
// The per-step slice of an array is addressed through a buffer resource descriptor held in SGPRs
// (cdna_hip_programming.md T8/T20): `buffer_load/store_dwordx2 v_data, v_off, s[rsrc], s_rowoff offen` with ONE shared
// 32-bit per-lane byte offset, the row offset in an SGPR and hardware bounds checking -- no 64-bit per-lane address
// arithmetic and no VGPR pairs per access.  A slice must stay below 4 GiB: rows * B * 8 < 2^32  =>  B <= 2^23.
typedef __amdgpu_buffer_rsrc_t rsrc_t;
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
EPI_DEV rsrc_t mk_rsrc(const void *p, unsigned bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)p, /*stride*/ 0, bytes, 0x00020000);
}
EPI_DEV double bld(rsrc_t r, unsigned voff, unsigned soff)
{
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}
// Cache policy of the big streams (aux bit 1 = `nt` on gfx950).  Every output is written once and read back -- if at all --
// tens of GB later, so the stores are NON-TEMPORAL: they do not push the shared input series, the model constants and the
// smoother's own read stream out of L2 / Infinity Cache.  Measured on the headline sweep, alternating builds on one box
// (round 4): 17.4-18.0 -> 16.3-17.0 ms per pass (smoother 8.0 -> 7.3 ms, forward kernel -0.2 ms), reduced outputs 13.7 -> 13.4,
// nothing slower.  Non-temporal LOADS on every load: 20.3 ms (the shared series stop being cached) -- so only the streams a launch
// reads exactly once (the stored forward quantities and X in the smoothers, P_MINUS in the pinv grid) are loaded `nt` (bld_s):
// another 16.2-17.0 -> 15.8-16.1 ms, the next pass's forward kernel finding its shared inputs still in cache.
// Round 4, later: `nt` + `sc1` (aux 18: non-temporal AND written through at system scope, so the line does not stay dirty
// in L2) -- level with `nt` alone on boxes / placements where the pass runs at its best (15.5-15.9 ms) and 0.4-0.8 ms faster
// where the L2's tag pipeline stalls on the concurrently streamed arrays ("where the arrays lie"): forward kernel
// 7.05 -> 6.67 ms on one box, smoother 7.8 -> 7.0 ms on another, three boxes 16.1-16.9 -> 15.6-15.9 ms per pass.  `sc1` on the
// stream LOADS as well (aux 18) brings the slow mode back; `sc0 | sc1 | nt` (19) on them is level with `nt` alone.
constexpr int kStAux = 18;
constexpr int kSt32Aux = 18;      // the fp32-storage twins of the stores (BASELINE config 5)
// (`sc0 | sc1 | nt` = 19 on the stream loads: -0.24 +- 0.10 ms per headline pass against `nt` alone over 20 paired runs on four
// boxes, smoother -0.13, slow outliers 16.6-17.2 -> at most 16.8 ms; `sc1 | nt` = 18 brings the smoother's slow mode back)
constexpr int kLdStreamAux = 19;
EPI_DEV void bst(rsrc_t r, unsigned voff, unsigned soff, double v)
{
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, voff, soff, kStAux);
}
// non-temporal only: for layouts whose rows are not whole cache lines (the hex shape's ten-chain blocks, ekf_hex.hpp), where
// writing through (`sc1`) turns every partial line into a memory transaction of its own
EPI_DEV void bst_nt(rsrc_t r, unsigned voff, unsigned soff, double v)
{
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, voff, soff, 2);
}
// a load of data that this launch reads exactly once (stored forward quantities, X)
EPI_DEV double bld_s(rsrc_t r, unsigned voff, unsigned soff)
{
    return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, kLdStreamAux));
}
EPI_DEV double ldg(const double *__restrict__ row, unsigned voff)
{
    return *(const double *)((const char *)row + voff);
}
EPI_DEV void stg(double *__restrict__ row, unsigned voff, double v) { *(double *)((char *)row + voff) = v; }
EPI_DEV int ldg_i(const int32_t *__restrict__ row, unsigned voff4) { return *(const int32_t *)((const char *)row + voff4); }
EPI_DEV void stg_i(int32_t *__restrict__ row, unsigned voff4, int v) { *(int32_t *)((char *)row + voff4) = v; }

// Chain-blocked layout of the big per-(time, row, chain) arrays (the 11 outputs and the workspace).  Element
// (t, row, c) of an array with `rows` rows lives at double index
//     ((t * nblk + c / blk) * rows + row) * blk + c % blk,        nblk = ceil(B / blk).
// blk = B (nblk = 1) is the classic [T][rows][B].  blk = 8 makes the rows of eight neighbouring chains one contiguous
// rows * 64-byte block, so that the ~100 stores a wave issues per step fill whole DRAM pages instead of feeding ~100
// concurrent row streams (profiles/layout_probe: 5.5 ms instead of 7.7-8.5 ms for the forward kernel's 32 GB of
// stores).  Arrays with one row ([T][B]: innovations, rho, rank words) are simply [T][nblk * blk].
struct Lay { unsigned blk, nblk, cb, cr, c, bp; };
EPI_DEV Lay make_lay(const KArgs &a, int c)
{
    Lay l;
    l.blk = (unsigned)a.blk; l.nblk = (unsigned)a.nblk; l.c = (unsigned)c;
    l.cb = (unsigned)c / l.blk; l.cr = (unsigned)c - l.cb * l.blk; l.bp = l.blk * l.nblk;
    return l;
}
// buffer descriptor of time slice t of an array with `rows` rows, this lane's byte offset in it, and the row pitch
EPI_DEV rsrc_t lay_slice(const double *p, int t, unsigned rows, const Lay &l, unsigned &voff, unsigned &rowb)
{
    rowb = l.blk * 8u;
    voff = (l.cb * rows * l.blk + l.cr) * 8u;
    return mk_rsrc(p + (size_t)t * rows * l.bp, rows * l.bp * 8u);
}
// inputs that are per (time, row, chain) -- a time-varying Q_w -- keep the classic [T][rows][B]
EPI_DEV Lay lay_classic(int B, int c)
{
    Lay l;
    l.blk = (unsigned)B; l.nblk = 1u; l.c = (unsigned)c; l.cb = 0u; l.cr = (unsigned)c; l.bp = (unsigned)B;
    return l;
}
EPI_DEV Lay make_lay_classic(const KArgs &a, int c) { return lay_classic(a.B, c); }
EPI_DEV size_t lay_scalar(int t, const Lay &l) { return (size_t)t * l.bp + l.c; }   // index into a [T][nblk*blk] array

template <int M>
EPI_DEV void store_vec(double *__restrict__ dst, int t, const Lay &l, const double (&v)[M])
{
    if (!dst) return;
    unsigned voff, rowb;
    const rsrc_t r = lay_slice(dst, t, M, l, voff, rowb);
#pragma unroll
    for (int i = 0; i < M; i++) bst(r, voff, (unsigned)i * rowb, v[i]);
}
template <int M>
EPI_DEV void store_mat(double *__restrict__ dst, int t, const Lay &l, const double (&P)[M * M])
{
    if (!dst) return;
    unsigned voff, rowb;
    const rsrc_t r = lay_slice(dst, t, M * M, l, voff, rowb);
#pragma unroll
    for (int e = 0; e < M * M; e++) bst(r, voff, (unsigned)e * rowb, P[e]);
}
template <int M>
EPI_DEV void load_vec(const double *__restrict__ src, int t, const Lay &l, double (&v)[M])
{
    unsigned voff, rowb;
    const rsrc_t r = lay_slice(src, t, M, l, voff, rowb);
#pragma unroll
    for (int i = 0; i < M; i++) v[i] = bld_s(r, voff, (unsigned)i * rowb);
}
template <int M>
EPI_DEV void load_mat(const double *__restrict__ src, int t, const Lay &l, double (&P)[M * M])
{
    unsigned voff, rowb;
    const rsrc_t r = lay_slice(src, t, M * M, l, voff, rowb);
#pragma unroll
    for (int e = 0; e < M * M; e++) P[e] = bld_s(r, voff, (unsigned)e * rowb);
}
// full symmetric matrix from a packed upper-triangle array (M(M+1)/2 rows)
template <int M>
EPI_DEV void load_packed(const double *__restrict__ src, int t, const Lay &l, double (&P)[M * M])
{
    constexpr int NSX = M * (M + 1) / 2;
    unsigned voff, rowb;
    const rsrc_t r = lay_slice(src, t, NSX, l, voff, rowb);
#pragma unroll
    for (int j = 0; j < M; j++)
#pragma unroll
        for (int i = 0; i <= j; i++) {
            const double v = bld_s(r, voff, (unsigned)(i + j * (j + 1) / 2) * rowb);
            P[IXM(i, j)] = v;
            P[IXM(j, i)] = v;
        }
}
// the control series stay [T][n_npi][Su] (inputs, shared by the chains of a region)
EPI_DEV void load_u(const KArgs &a, int t, int su, double (&u)[kNpi])
{
    const unsigned voff = (unsigned)su * 8u, rowb = (unsigned)a.Su * 8u;
    const rsrc_t r = mk_rsrc(a.u + (size_t)t * a.n_npi * a.Su, (unsigned)a.n_npi * rowb);
    // rows k >= n_npi lie beyond the descriptor's range: the hardware bounds check returns 0.0 for them, which is the
    // padding value -- twelve unconditional loads instead of twelve scalar branches (the check includes the SGPR row
    // offset on gfx950: profiles/bounds_probe/probe.hip)
#pragma unroll
    for (int k = 0; k < kNpi; k++) u[k] = bld(r, voff, (unsigned)k * rowb);
}
EPI_DEV void store_u(double *__restrict__ dst, const KArgs &a, int t, const Lay &l, const double (&u)[kNpi])
{
    if (!dst) return;
    unsigned voff, rowb;
    const rsrc_t r = lay_slice(dst, t, (unsigned)a.n_npi, l, voff, rowb);
    if (a.n_npi == kNpi) {                    // the usual case: one scalar branch instead of twelve
#pragma unroll
        for (int k = 0; k < kNpi; k++) bst(r, voff, (unsigned)k * rowb, u[k]);
        return;
    }
#pragma unroll
    for (int k = 0; k < kNpi; k++)
        if (k < a.n_npi) bst(r, voff, (unsigned)k * rowb, u[k]);
}

// fp32-storage twins of the stores above (epi_batch_desc.storage = 1): same layout formulas with 4-byte elements, the
// value rounded once from the fp64 register
EPI_DEV rsrc_t lay_slice_f32(const float *p, int t, unsigned rows, const Lay &l, unsigned &voff, unsigned &rowb)
{
    rowb = l.blk * 4u;
    voff = (l.cb * rows * l.blk + l.cr) * 4u;
    return mk_rsrc(p + (size_t)t * rows * l.bp, rows * l.bp * 4u);
}
EPI_DEV void bst32(rsrc_t r, unsigned voff, unsigned soff, double v)
{
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, (float)v), r, voff, soff, kSt32Aux);
}
template <int N>
EPI_DEV void store_rows_f32(float *__restrict__ dst, int t, unsigned rows, const Lay &l, const double (&v)[N])
{
    if (!dst) return;
    unsigned voff, rowb;
    const rsrc_t r = lay_slice_f32(dst, t, rows, l, voff, rowb);
#pragma unroll
    for (int i = 0; i < N; i++)
        if ((unsigned)i < rows) bst32(r, voff, (unsigned)i * rowb, v[i]);
}
EPI_DEV void store_scalar_f32(float *__restrict__ dst, int t, const Lay &l, double v)
{
    if (dst) dst[lay_scalar(t, l)] = (float)v;
}

// ---------------------------------------------------------------------------
// forward pass
// ---------------------------------------------------------------------------
template <int M, int FLIP, int GENERIC>
__global__ __launch_bounds__(kWave) void ekf_fwd(const KArgs a)
{
    extern __shared__ double lds[];   // three sliding windows [3][L][64], one column per lane
    if (a.dense_flag && !*a.dense_flag) return;   // the symmetric fast path (ekf_fwd_sym) handles this batch
    const int lane = threadIdx.x;
    const int c = a.c0 + blockIdx.x * a.lw + lane;
    if (lane >= a.lw || c >= a.c0 + a.cn) return;
    if (a.only && !a.only[c]) return;             // second pass over the chains whose covariance went non-finite
    const int B = a.B, T = a.T, L = a.L;
    const int sx = a.x_series ? a.x_series[c] : c;
    const int su = a.u_series ? a.u_series[c] : c;
    const Lay lay = make_lay(a, c);

    ChainPrm p;
    load_prm<M>(p, a.prm, B, c, a.mf.lo_is_zero);
    const double v_bar = a.prm[(size_t)EPI_PRM_V_BAR * B + c];
    const double beta = a.prm[(size_t)EPI_PRM_BETA_EKF * B + c];
    const double gamma = a.prm[(size_t)EPI_PRM_GAMMA_EKF * B + c];

    double sk_minus[M], Pk_minus[M * M], Q[M * M];
#pragma unroll
    for (int i = 0; i < M; i++) sk_minus[i] = a.s_init[(size_t)i * B + c];
#pragma unroll
    for (int e = 0; e < M * M; e++) {
        Pk_minus[e] = a.Ps_init[(size_t)e * B + c];
        Q[e] = a.Q[(size_t)e * B + c];
    }
    double *winMean = lds + lane, *winCov = lds + (size_t)L * kWave + lane, *winCovN = lds + (size_t)2 * L * kWave + lane;
    for (int j = 0; j < L; j++) { winMean[j * kWave] = 0.0; winCov[j * kWave] = 0.0; winCovN[j * kWave] = 0.0; }
    int head = 0;

    const bool fixed_R = (a.r_mode == 0);            // GenericEKF.m:79-85
    const double R_v = fixed_R ? a.R_scalar[c] : 0.0;
    double R_next = R_v;                              // R(:,:,k+1) as left by step k (GENERIC) / running R (NewCase)

    for (int k = 0; k < T; k++) {
        const int t = tpos<FLIP>(k, T);
        // R_v is NOT time-flipped by the backward wrappers (Backward*.m:27 passes it through)
        const double Rk = fixed_R ? R_next : a.R_series[(size_t)k * a.Sx + sx];
        const double xk = a.x[(size_t)t * a.Sx + sx];
        double u_in[kNpi];
        load_u(a, t, su, u_in);
        if (GENERIC && a.q_mode)   // Q(:,:,k): like R_v, Q_w is not time-flipped by the backward wrappers
            load_mat<M>(a.Q, k, make_lay_classic(a, c), Q);

        store_vec<M>(a.S_MINUS, t, lay, sk_minus);       // :100-101
        store_mat<M>(a.P_MINUS, t, lay, Pk_minus);

        double C[M];
        obs_jacobian<M>(a.mf, sk_minus, C);               // :115
        const double xk_minus = predict_obs<M>(a.mf, sk_minus, v_bar);  // :116-119

        double innov, K[M], sk_plus[M], Pk_plus[M * M];
        const bool valid = !is_nan(xk);                   // :122
        if (valid) {
            innov = xk - xk_minus;
            double PCt[M], CP[M];
#pragma unroll
            for (int i = 0; i < M; i++) {
                double acc = Pk_minus[IXM(i, 0)] * C[0];
#pragma unroll
                for (int j = 1; j < M; j++) acc = fma(Pk_minus[IXM(i, j)], C[j], acc);
                PCt[i] = acc;
            }
#pragma unroll
            for (int j = 0; j < M; j++) {
                double acc = C[0] * Pk_minus[IXM(0, j)];
#pragma unroll
                for (int i = 1; i < M; i++) acc = fma(C[i], Pk_minus[IXM(i, j)], acc);
                CP[j] = acc;
            }
            double CPCt = CP[0] * C[0];
#pragma unroll
            for (int j = 1; j < M; j++) CPCt = fma(CP[j], C[j], CPCt);
            const double den = CPCt + gamma * Rk;          // :124 (D = 1, Hessian terms 0)
#pragma unroll
            for (int i = 0; i < M; i++) K[i] = PCt[i] / den;
            double IKC[M * M], T1[M * M];
#pragma unroll
            for (int j = 0; j < M; j++)
#pragma unroll
                for (int i = 0; i < M; i++) IKC[IXM(i, j)] = ((i == j) ? 1.0 : 0.0) - K[i] * C[j];
            mat_mul<M>(IKC, Pk_minus, T1);
            if (GENERIC) {
                double T2[M * M];
                mat_mul_bt<M>(T1, IKC, T2);                // Joseph form :127
#pragma unroll
                for (int j = 0; j < M; j++)
#pragma unroll
                    for (int i = 0; i < M; i++)
                        Pk_plus[IXM(i, j)] = (T2[IXM(i, j)] + (K[i] * Rk) * K[j]) / gamma;
            } else {
#pragma unroll
                for (int e = 0; e < M * M; e++) Pk_plus[e] = T1[e] / gamma;   // NewCase...m:64
            }
#pragma unroll
            for (int i = 0; i < M; i++) sk_plus[i] = sk_minus[i] + K[i] * innov;   // :129
        } else {                                           // :130-135
            innov = 0.0;
#pragma unroll
            for (int i = 0; i < M; i++) { K[i] = 0.0; sk_plus[i] = sk_minus[i]; }
#pragma unroll
            for (int e = 0; e < M * M; e++) Pk_plus[e] = Pk_minus[e];
        }
        if (GENERIC) symmetrize<M>(Pk_plus);               // :138
        state_hard_margins<M>(p, sk_plus);                 // :141

        // s(k+1|k), P(k+1|k)  :155-164
        double u_app[kNpi];
#pragma unroll
        for (int q = 0; q < kNpi; q++) u_app[q] = u_in[q];
        nlin_state_update<M, FLIP>(p, a.mf, u_app, sk_plus, sk_minus);
        store_u(a.u_opt, a, t, lay, u_app);
        {
            double A[M * M], T1[M * M], T2[M * M];
            state_jacobians<M, FLIP>(p, u_in, sk_plus, A);
            mat_mul<M>(A, Pk_plus, T1);
            mat_mul_bt<M>(T1, A, T2);
#pragma unroll
            for (int e = 0; e < M * M; e++) Pk_minus[e] = T2[e] + Q[e];   // B = I
        }
        if (GENERIC) symmetrize<M>(Pk_minus);              // :161
        state_hard_margins<M>(p, sk_minus);                // :164

        store_vec<M>(a.S_PLUS, t, lay, sk_plus);          // :167-169
        store_mat<M>(a.P_PLUS, t, lay, Pk_plus);
        store_vec<M>(a.K_GAIN, t, lay, K);
        if (a.innovations) a.innovations[lay_scalar(t, lay)] = innov;

        // innovation monitor :172-185 -- windows are newest-first and summed front to back
        const int cnt = (k + 1 < L) ? (k + 1) : L;
        head = (head == 0) ? (L - 1) : (head - 1);
        winMean[head * kWave] = innov;
        const double sum = ring_sum(winMean, head, L, innov);
        const double mu = sum / (double)cnt;
        const double cc = (innov - mu) * (innov - mu);
        const double ccn = GENERIC ? cc / (Rk + kEps) : cc / Rk;
        winCov[head * kWave] = cc;
        winCovN[head * kWave] = ccn;
        const double sumN = ring_sum(winCovN, head, L, ccn);
        // rho keeps FILTER-step order also for the time-flipped wrappers: GenericEKF.m:233 squeezes it to T x 1 and
        // Backward*.m:40 reverses a third dimension of size 1, i.e. nothing
        if (a.rho) a.rho[lay_scalar(k, lay)] = sumN / (double)cnt;
        if (fixed_R) {
            const bool adapt = GENERIC ? (beta != 1.0 && valid && k < T - 1) : (beta != 1.0 && valid);
            if (adapt) {
                const double sumC = ring_sum(winCov, head, L, cc);
                if (GENERIC) R_next = beta * Rk + (1.0 - beta) * (sumC / (double)cnt);   // :184
                else R_next = beta * Rk + (1.0 - beta) * sumC / (double)cnt;             // NewCase...m:111
            } else if (GENERIC) {
                R_next = R_v;   // R(k+1) keeps its initial value when step k does not write it
            }
        }
    }
}

// ---------------------------------------------------------------------------
// smoother gain, part 1: X = pinv(P_MINUS(:,:,k+1)) for every (chain, step) pair
// ---------------------------------------------------------------------------
// GenericEKF.m:209-215.  pinv of P(k+1|k) depends only on forward quantities, not on the backward
// recursion, so it is hoisted out of the sequential smoother loop: one lane per (chain, step) pair,
// (T-1)*B independent items.  This is where ~80 % of the path's flops are (cyclic Jacobi on a 6 x 6),
// and as a flat grid it load-balances over all 1024 SIMDs instead of B/64 long-lived waves.
// 6 x 6: one wavefront per workgroup.  The Jacobi iteration count is data dependent, and with 256-thread workgroups a
// SIMD's wave slot stays empty until all four waves of a workgroup have finished (measured 1.67 resident waves per SIMD
// instead of 1.9; 7.25 -> 6.6 ms on the headline sweep, 128 threads: 6.9 ms).  3 x 3: the waves are short and nearly
// uniform, and four times as many workgroups cost more than the slots they free (5.2 -> 5.9 ms on the 307 200-chain
// ensemble), so they keep 256 threads.
template <int M>
constexpr int pinv_wg() { return M >= 6 ? 64 : 256; }
// Three waves per SIMD (168 VGPRs): the third wave fills VALU issue slots two dependent fp64 chains leave idle (6.2 ->
// 5.9 ms on the headline sweep with 76 B/lane of scratch; 5.8 ms and no scratch once the Jacobi's b/z accumulators
// moved to LDS, 6 KB per wavefront).
// X = pinv(P(t1|t1-1)) of chain c: the work of one lane of the grid below
template <int M>
EPI_DEV void pinv_one(const KArgs &a, int c, int t1, double *plds)
{
    constexpr int WG = pinv_wg<M>();
    const Lay lay = make_lay(a, c);
    constexpr int NSX = M * (M + 1) / 2;
    double Pu[NSX];
    // P_MINUS is stored symmetrised (:161): only its upper triangle is read
    unsigned voff_p, rowb_p;
    const rsrc_t rp = lay_slice(a.P_MINUS, t1, M * M, lay, voff_p, rowb_p);
#pragma unroll
    for (int j = 0; j < M; j++)
#pragma unroll
        for (int i = 0; i <= j; i++) Pu[i + j * (j + 1) / 2] = bld_s(rp, voff_p, (unsigned)IXM(i, j) * rowb_p);
    bool bad = false;                                      // :211
#pragma unroll
    for (int i = 0; i < NSX; i++) bad = bad || is_nonfinite(Pu[i]);
    int32_t *rword = a.rankbuf + lay_scalar(t1, lay);
    if (bad) {
        *rword = -1;
        return;
    }
    // X is symmetric bit for bit: the workspace holds its packed upper triangle (M(M+1)/2 rows)
    double Xu[NSX];
    bool capped, indef;
    // one LDS column per lane: scratch of the full-rank route, and later the b/z accumulators of the two-sided fall-back
    int rank = sym_pinv_psd<M, WG>(Pu, Xu, &capped, &indef, plds + threadIdx.x);              // :215
    unsigned voff_x, rowb_x;
    const rsrc_t rx = lay_slice(a.X, t1, NSX, lay, voff_x, rowb_x);
    if (a.hex) {       // 80-byte rows: see bst_nt (eks_pinv of the 9 375-chain shard 0.84 ms written through, 0.49 ms not)
#pragma unroll
        for (int i = 0; i < NSX; i++) bst_nt(rx, voff_x, (unsigned)i * rowb_x, Xu[i]);
    } else {
#pragma unroll
        for (int i = 0; i < NSX; i++) bst(rx, voff_x, (unsigned)i * rowb_x, Xu[i]);
    }
    *rword = rank | (capped ? 0x100 : 0);
    if (__builtin_amdgcn_ballot_w64(indef) != 0ull) {
        // Not positive semi-definite up to rounding (never the case for a covariance the filter produced from a positive
        // semi-definite Ps_init): the two-sided Jacobi route on the matrix read again; the lanes concerned overwrite what
        // they stored above (nothing of the first route is live across this block).
        constexpr int BZS = (M >= 6) ? WG : 0;              // its b/z accumulators (one column per lane), see jacobi_eig
        double *bzs = plds;
        double P[M * M], X[M * M];
#pragma unroll
        for (int j = 0; j < M; j++)
#pragma unroll
            for (int i = 0; i <= j; i++) {
                const double v = bld(rp, voff_p, (unsigned)IXM(i, j) * rowb_p);
                P[IXM(i, j)] = v;
                P[IXM(j, i)] = v;
            }
        bool capped2;
        const int rank2 = sym_pinv_two_sided<M, BZS>(P, X, &capped2, bzs + threadIdx.x);
        if (indef) {
#pragma unroll
            for (int j = 0; j < M; j++)
#pragma unroll
                for (int i = 0; i <= j; i++) bst(rx, voff_x, (unsigned)(i + j * (j + 1) / 2) * rowb_x, X[IXM(i, j)]);
            *rword = rank2 | (capped2 ? 0x100 : 0);
        }
    }
}
template <int M, int LIST = 0>
__global__ __launch_bounds__(pinv_wg<M>(), 3) void eks_pinv(const KArgs a)
{
    // grid: x = pinv_wg<M>()-chain tiles of the chain range (rounded up to a multiple of 8), y = step; a workgroup shares one
    // step => uniform row bases
    // XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs (each with its own L2) in linear-id order, so
    // XCD c gets ids c, c + 8, ...  Within EVERY step give each XCD a contiguous eighth of the tiles: neighbouring tiles --
    // whose 64 chains share a partial cache line where they straddle a 40-chain layout block -- then meet in one L2, and all
    // XCDs still walk the steps together (the early, full-rank steps cost three times the late ones).
    const unsigned gx = gridDim.x;
    const unsigned long long lin = (unsigned long long)blockIdx.y * gx + blockIdx.x;      // (2^17 tiles x 2^16 steps exceed 32 bits)
    const unsigned per = gx >> 3;                              // tiles of a step per XCD (the grid's x extent is a multiple of 8)
    const unsigned xcd = (unsigned)(lin & 7ull);
    const unsigned long long k = lin >> 3;
    unsigned by = blockIdx.y, bx = blockIdx.x;                 // fewer than 8 tiles: the launch keeps the plain order
    if ((gx & 7u) == 0u) {
        by = (unsigned)(k / per);
        bx = xcd * per + (unsigned)(k - (unsigned long long)by * per);
    }
    constexpr int WG = pinv_wg<M>();
    constexpr int NSX = M * (M + 1) / 2;
    constexpr int LROWS = NSX > 2 * M ? NSX : 2 * M;
    // one LDS column per lane: scratch of the full-rank route, and later the b/z accumulators of the two-sided fall-back
    __shared__ double plds[LROWS * WG];
    // array positions of filter steps 2..T: 1..T-1, or 0..T-2 for the time-flipped models (pinv_pos0 = 0)
    const int t1 = a.pinv_pos0 + a.pinv_step0 + (int)by;
    if (LIST) {
        // Second pass over the chains whose covariance went non-finite (epi_batch_desc.exact_nonfinite, a.only): the launch is a
        // few tiles wide and walks the list mark_nonfinite left -- nothing to do, and next to nothing dispatched, when no chain
        // is marked.  (A kernel of its own: the loop around the 60 KB body costs the main grid 16 B of scratch per lane.)
        const int32_t *list = a.only + a.B + 1;
        const int count = a.only[a.B];
        for (int cl = (int)(bx * blockDim.x + threadIdx.x); cl < count; cl += (int)(gx * blockDim.x)) pinv_one<M>(a, list[cl], t1, plds);
        return;
    }
    const int cl = (int)(bx * blockDim.x + threadIdx.x);
    if (cl >= a.cn) return;
    pinv_one<M>(a, a.c0 + cl, t1, plds);
}

// ---------------------------------------------------------------------------
// backward pass (fixed-interval smoother)
// ---------------------------------------------------------------------------
template <int M, int FLIP, int GENERIC>
__global__ __launch_bounds__(kWave) void eks_bwd(const KArgs a)
{
    if (a.dense_flag && !*a.dense_flag) return;   // eks_bwd_sym handles this batch
    const int c = a.c0 + blockIdx.x * a.lw + threadIdx.x;
    if ((int)threadIdx.x >= a.lw || c >= a.c0 + a.cn) return;
    if (a.only && !a.only[c]) return;
    const int B = a.B, T = a.T;
    const int su = a.u_series ? a.u_series[c] : c;
    const Lay lay = make_lay(a, c);
    // the four 12-vectors of `params` in an LDS column per lane instead of 96 VGPRs (without this the 6-state kernel
    // spills: 512 registers + 84 B of scratch)
    // (three states: a and u_max only, VecLds2 -- 12 KB instead of 24 KB per workgroup, so that LDS does not cap the kernel
    // below the two waves per SIMD its registers allow)
    constexpr int NV = (M == 6) ? 4 : 2;
    __shared__ double vlds[NV * kNpi * kWave];
    LitePrm<typename std::conditional<M == 6, VecLds, VecLds2>::type> p;
    load_lite(p, a.prm, B, c, a.mf.lo_is_zero);
    p.v.base = vlds + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kNpi; k++) {
        vlds[(0 * kNpi + k) * kWave + threadIdx.x] = a.prm[(size_t)(EPI_PRM_A + k) * B + c];
        if constexpr (M == 6) {
            vlds[(1 * kNpi + k) * kWave + threadIdx.x] = a.prm[(size_t)(EPI_PRM_U_MIN + k) * B + c];
            vlds[(2 * kNpi + k) * kWave + threadIdx.x] = a.prm[(size_t)(EPI_PRM_U_MAX + k) * B + c];
            vlds[(3 * kNpi + k) * kWave + threadIdx.x] = a.prm[(size_t)(EPI_PRM_W_EFF + k) * B + c];
        } else {
            vlds[(1 * kNpi + k) * kWave + threadIdx.x] = a.prm[(size_t)(EPI_PRM_U_MAX + k) * B + c];
        }
    }

    // terminal conditions :189-202
    double Ss[M], Ps[M * M];
    const int tT = tpos<FLIP>(T - 1, T);
    load_vec<M>(a.S_PLUS, tT, lay, Ss);
    load_mat<M>(a.P_PLUS, tT, lay, Ps);
#pragma unroll
    for (int i = 0; i < M; i++) {
        double f = a.s_final[(size_t)i * B + c];
        if (!is_nan(f)) Ss[i] = f;
    }
    {
        double Pf[M * M];
#pragma unroll
        for (int e = 0; e < M * M; e++) Pf[e] = a.Ps_final[(size_t)e * B + c];
        if (GENERIC) {
#pragma unroll
            for (int e = 0; e < M * M; e++)
                if (!is_nan(Pf[e])) Ps[e] = Pf[e];
        } else {
            // P_SMOOTH(row, col, T) = Ps_final(row, col): cross-product sub-assignment, NewCase...m:125-127
            bool rows[M], cols[M];
#pragma unroll
            for (int i = 0; i < M; i++) { rows[i] = false; cols[i] = false; }
#pragma unroll
            for (int j = 0; j < M; j++)
#pragma unroll
                for (int i = 0; i < M; i++)
                    if (!is_nan(Pf[IXM(i, j)])) { rows[i] = true; cols[j] = true; }
#pragma unroll
            for (int j = 0; j < M; j++)
#pragma unroll
                for (int i = 0; i < M; i++)
                    if (rows[i] && cols[j]) Ps[IXM(i, j)] = Pf[IXM(i, j)];
        }
    }
    store_vec<M>(a.S_SMOOTH, tT, lay, Ss);
    store_mat<M>(a.P_SMOOTH, tT, lay, Ps);
    if (GENERIC && a.u_opt_smooth) {
        double z[kNpi];
#pragma unroll
        for (int k = 0; k < kNpi; k++) z[k] = 0.0;
        store_u(a.u_opt_smooth, a, tT, lay, z);      // column T is never written :95,204
    }
    if (a.pinv_rank) a.pinv_rank[lay_scalar(tT, lay)] = -1;

    int st_guard = 0, st_cap = 0, min_rank = M;
    for (int k = T - 2; k >= 0; k--) {
        const int t = tpos<FLIP>(k, T), t1 = tpos<FLIP>(k + 1, T);
        double Sp[M], Pp[M * M], Sm1[M], Pm1[M * M], u_in[kNpi];
        load_vec<M>(a.S_PLUS, t, lay, Sp);
        load_mat<M>(a.P_PLUS, t, lay, Pp);
        load_vec<M>(a.S_MINUS, t1, lay, Sm1);
        load_mat<M>(a.P_MINUS, t1, lay, Pm1);
        load_u(a, t, su, u_in);

        double J[M * M];
        int rank = -1;
        {
            double A[M * M], PAt[M * M];
            state_jacobians<M, FLIP>(p, u_in, Sp, A);          // :206
            mat_mul_bt<M>(Pp, A, PAt);                         // P_PLUS * A'
            if (GENERIC) {
                // pinv(P_MINUS(:,:,k+1)) was computed by eks_pinv (one lane per (chain, step) pair)
                const int rk = a.rankbuf[lay_scalar(t1, lay)];
                if (rk < 0) {                                  // non-finite P_MINUS guard :211-213
#pragma unroll
                    for (int e = 0; e < M * M; e++) J[e] = 0.0;
                    st_guard = 1;
                } else {
                    double X[M * M];
                    load_packed<M>(a.X, t1, lay, X);
                    mat_mul<M>(PAt, X, J);                     // :215
                    rank = rk & 0xff;
                    st_cap |= (rk >> 8) & 1;
                    min_rank = rank < min_rank ? rank : min_rank;
                }
            } else {
                mrdivide<M>(PAt, Pm1, J);                      // NewCase...m:132
            }
        }
        if (a.pinv_rank) a.pinv_rank[lay_scalar(t, lay)] = rank;

        double Sn[M];
        {
            double dv[M];
#pragma unroll
            for (int i = 0; i < M; i++) dv[i] = Ss[i] - Sm1[i];
#pragma unroll
            for (int i = 0; i < M; i++) {
                double acc = J[IXM(i, 0)] * dv[0];
#pragma unroll
                for (int j = 1; j < M; j++) acc = fma(J[IXM(i, j)], dv[j], acc);
                Sn[i] = Sp[i] + acc;                           // :218
            }
        }
        state_hard_margins<M>(p, Sn);                          // :221
        {
            double D[M * M], T1[M * M], T2[M * M];
#pragma unroll
            for (int e = 0; e < M * M; e++) D[e] = Pm1[e] - Ps[e];
            mat_mul<M>(J, D, T1);
            mat_mul_bt<M>(T1, J, T2);
#pragma unroll
            for (int e = 0; e < M * M; e++) Ps[e] = Pp[e] - T2[e];   // :223
        }
        if (GENERIC) symmetrize<M>(Ps);                        // :226
#pragma unroll
        for (int i = 0; i < M; i++) Ss[i] = Sn[i];
        store_vec<M>(a.S_SMOOTH, t, lay, Ss);
        store_mat<M>(a.P_SMOOTH, t, lay, Ps);
        if (GENERIC && a.u_opt_smooth) {                       // :229
            double sn_unused[M];
            nlin_state_update<M, FLIP>(p, a.mf, u_in, Ss, sn_unused);
            store_u(a.u_opt_smooth, a, t, lay, u_in);
        }
    }
    if (a.status) a.status[c] = st_guard | (st_cap << 1) | (min_rank << 8);
}

#include "ekf_sym.hpp"
#include "ekf_quad.hpp"
#include "ekf_wave.hpp"
#include "ekf_hex.hpp"
#include "ekf_lane6.hpp"

// ---------------------------------------------------------------------------
// forward simulators
// ---------------------------------------------------------------------------
// SimPrm, load_sim_prm, sialpha_step and npicost_accumulate live in ekf_device.hpp (npi_plan.hpp is compiled for the host with them)

__global__ __launch_bounds__(256) void sialpha_sim(const epi_sim_desc d, const int32_t *__restrict__ u_series,
                                                   const double *__restrict__ u, const double *__restrict__ sp,
                                                   const double *__restrict__ z, double *__restrict__ so,
                                                   double *__restrict__ io, double *__restrict__ ao,
                                                   double *__restrict__ J0, double *__restrict__ J1,
                                                   const double *__restrict__ J0_prefix,
                                                   const double *__restrict__ J1_prefix,
                                                   const int32_t *__restrict__ gate)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= d.B) return;
    if (gate && *gate == 0) return;       // second scoring pass after the dense re-run: nothing was re-run
    const int B = d.B;
    const int su = u_series ? u_series[c] : c;
    SimPrm p;
    double s, i, al;
    load_sim_prm(p, sp, B, c, s, i, al);
    // NPICost over [historic days, simulated days] (TrainPredictPrescribeNPI.m:481-493): the historic part of
    // the two sequential sums arrives as a per-chain prefix and the simulated days are added in order
    const bool pre = (d.prefix_days > 0) && J0_prefix && J1_prefix;
    double acc0 = pre ? J0_prefix[c] : 0.0, acc1 = pre ? J1_prefix[c] : 0.0;
    // u: [K][n_npi][Su], or chain-blocked ((t*nblk + su/blk)*n_npi + k)*blk + su%blk
    const int ublk = (d.u_block <= 0 || d.u_block >= d.Su) ? d.Su : d.u_block;
    const size_t unb = (size_t)(d.Su + ublk - 1) / ublk, ucb = (size_t)su / ublk, ucr = (size_t)su % ublk;
    for (int t = 0; t < d.K; t++) {
        double uk[kNpi];
#pragma unroll
        for (int k = 0; k < kNpi; k++) uk[k] = (k < d.n_npi) ? u[(((size_t)t * unb + ucb) * d.n_npi + k) * ublk + ucr] : 0.0;
        double z1 = 0.0, z2 = 0.0, z3 = 0.0;
        if (d.noise) {
            z1 = z[((size_t)t * 3 + 0) * B + c]; z2 = z[((size_t)t * 3 + 1) * B + c]; z3 = z[((size_t)t * 3 + 2) * B + c];
        }
        sialpha_step(p, uk, z1, z2, z3, s, i, al);
        if (so) so[(size_t)t * B + c] = s;
        if (io) io[(size_t)t * B + c] = i;
        if (ao) ao[(size_t)t * B + c] = al;
        if (d.with_cost) npicost_accumulate(p, uk, d.n_npi, t == 0 && !pre, s, i, al, acc0, acc1);
    }
    if (d.with_cost) {
        const size_t days = (size_t)d.K + (size_t)(pre ? d.prefix_days : 0);
        if (J0) J0[c] = acc0 / (double)days;
        if (J1) J1[c] = acc1 / (double)((size_t)d.n_npi * days);
    }
}

#include "noise.hpp"
// sialpha_sim with the three draws of (step t, chain c) generated: draws (t, 0 .. 2, c) of noise.hpp.  A body of its
// own, so that sialpha_sim keeps its text and its code
__global__ __launch_bounds__(256) void sialpha_sim_seeded(const epi_sim_desc d, const NoiseKey nk, const int32_t *__restrict__ u_series,
                                                          const double *__restrict__ u, const double *__restrict__ sp,
                                                          double *__restrict__ so, double *__restrict__ io, double *__restrict__ ao,
                                                          double *__restrict__ J0, double *__restrict__ J1,
                                                          const double *__restrict__ J0_prefix, const double *__restrict__ J1_prefix)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= d.B) return;
    const int B = d.B;
    const int su = u_series ? u_series[c] : c;
    SimPrm p;
    double s, i, al;
    load_sim_prm(p, sp, B, c, s, i, al);
    // NPICost over [historic days, simulated days] (TrainPredictPrescribeNPI.m:481-493): the historic part of
    // the two sequential sums arrives as a per-chain prefix and the simulated days are added in order
    const bool pre = (d.prefix_days > 0) && J0_prefix && J1_prefix;
    double acc0 = pre ? J0_prefix[c] : 0.0, acc1 = pre ? J1_prefix[c] : 0.0;
    // u: [K][n_npi][Su], or chain-blocked ((t*nblk + su/blk)*n_npi + k)*blk + su%blk
    const int ublk = (d.u_block <= 0 || d.u_block >= d.Su) ? d.Su : d.u_block;
    const size_t unb = (size_t)(d.Su + ublk - 1) / ublk, ucb = (size_t)su / ublk, ucr = (size_t)su % ublk;
    for (int t = 0; t < d.K; t++) {
        double uk[kNpi];
#pragma unroll
        for (int k = 0; k < kNpi; k++) uk[k] = (k < d.n_npi) ? u[(((size_t)t * unb + ucb) * d.n_npi + k) * ublk + ucr] : 0.0;
        double z1, z2, z3;
        epi_normal_three(nk, (uint32_t)t, (uint64_t)c, z1, z2, z3);
        sialpha_step(p, uk, z1, z2, z3, s, i, al);
        if (so) so[(size_t)t * B + c] = s;
        if (io) io[(size_t)t * B + c] = i;
        if (ao) ao[(size_t)t * B + c] = al;
        if (d.with_cost) npicost_accumulate(p, uk, d.n_npi, t == 0 && !pre, s, i, al, acc0, acc1);
    }
    if (d.with_cost) {
        const size_t days = (size_t)d.K + (size_t)(pre ? d.prefix_days : 0);
        if (J0) J0[c] = acc0 / (double)days;
        if (J1) J1[c] = acc1 / (double)((size_t)d.n_npi * days);
    }
}

#include "scenario_kernels.hpp"
#include "rt_expfit.hpp"
#include "preprocess.hpp"
#include "nnls.hpp"
#include "lookahead.hpp"
#include "rt_window.hpp"
#include "lasso.hpp"
#include "ens_summary.hpp"
#include "ens_score.hpp"
#include "path_functionals.hpp"
#include "curve_depth.hpp"
#include "ens_joint.hpp"
#include "ar_forecast.hpp"
// ar_simulate with the draw of (forecast day t, chain c) generated: draw (t, 0, c) of noise.hpp.  A body of its own: ar_forecast.hpp
// stays free of ekf_device.hpp (tests/ar_forecast_emu.cpp compiles it alone) and ar_simulate keeps its text and its code
__global__ __launch_bounds__(64) void ar_simulate_seeded(const ArSimArgs a, const NoiseKey nk)
{
    extern __shared__ double ar_lds[];
    const int lane = threadIdx.x, L = a.L, p = a.p, H = a.H;
    const long long blk = a.blk0 + (long long)blockIdx.x;
    const size_t R = (size_t)a.R, r = (size_t)(blk / a.bpr), B = R * (size_t)a.D;
    const int d = (int)(blk % a.bpr) * 64 + lane;
    const bool active = d < a.D;
    const size_t c = r * (size_t)a.D + (size_t)(active ? d : 0);
    double *y = ar_lds;                      // [L] the segment
    double *coef = y + ar_lds_seg(L);        // [32]
    double *ring = coef + 32;                // [p][64] past values of the recursion, one column per lane
    const double qnan = __builtin_nan("");
    int bad = 0;
    for (int t = lane; t < L; t += 64) {
        const double v = a.seg[(size_t)t * R + r];
        y[t] = v;
        bad |= !ar_finite(v);
    }
    int dead = 0;
    if (lane < p) {
        const double v = a.A[(size_t)lane * R + r];
        coef[lane] = v;
        dead = !ar_finite(v);
    }
    const double b0 = sqrt(a.nv[r]);
    dead |= !ar_finite(b0);
    bad = __ballot(bad) != 0;                // BAD_INPUT: every day is NaN
    dead = bad || __ballot(dead) != 0;       // no usable model: NaN from day L on
    __syncthreads();
    const double beta = a.beta[r], dt = a.dt;
    double s = a.s0[r], i = a.i0[r];
    size_t ser = 0;
    if (a.drive && active) ser = a.drive_series ? (size_t)a.drive_series[c] : c;
    double *o = a.S + c;
    // ---- the segment: alpha_hat = seg clamped, SI_Controlled.m:19-22 ----
    for (int t = 0; t < L; t++) {
        const double v = y[t];
        const double al = v < 0.0 ? 0.0 : v;
        if (active) {
            o[0] = bad ? qnan : s; o[B] = bad ? qnan : i; o[2 * B] = bad ? qnan : al;
        }
        o += 3 * B;
        const double sn = fmax(0.0, fmin(1.0, s - dt * al * s * i));
        const double in = fmax(0.0, fmin(1.0, i + dt * (al * s * i - beta * i)));
        s = sn; i = in;
    }
    // ---- the forecast: y(t) = b0 z(t) - sum a_k y(t-k), k ascending, the past from the segment first ----
    for (int j = 0; j < p; j++) ring[j * 64 + lane] = y[L - p + j];
    int head = 0;
    for (int t = 0; t < H; t++) {
        const double zt = epi_normal_draw(nk, (uint32_t)t, 0u, (uint64_t)c);
        double acc = b0 * zt;
        int idx = head;
        for (int k = 0; k < p; k++) {
            idx = idx == 0 ? p - 1 : idx - 1;
            acc = fma(-coef[k], ring[idx * 64 + lane], acc);
        }
        ring[head * 64 + lane] = acc;
        head = head + 1 == p ? 0 : head + 1;
        double v = acc;
        if (a.drive && active) v = acc + a.drive[(size_t)t * (size_t)a.Sd + ser];
        const double al = v < 0.0 ? 0.0 : v;
        if (active) {
            o[0] = dead ? qnan : s; o[B] = dead ? qnan : i; o[2 * B] = dead ? qnan : al;
        }
        o += 3 * B;
        if (t + 1 < H) {
            const double sn = fmax(0.0, fmin(1.0, s - dt * al * s * i));
            const double in = fmax(0.0, fmin(1.0, i + dt * (al * s * i - beta * i)));
            s = sn; i = in;
        }
    }
}
#include "two_filter.hpp"
#include "robust_fit.hpp"
#include "rate_map.hpp"
#include "mldivide.hpp"
#include "svr.hpp"
#include "loglik.hpp"
#include "innov_diag.hpp"
#include "npi_plan.hpp"
#include "smoother_draws.hpp"

struct SeirpRates { double ae, ai, kappa, rho, beta, mu, gamma; };
EPI_DEV void seirp_rhs(const SeirpRates &r, const double (&y)[5], double (&f)[5])
{
    // SEIRP.m:27-31
    f[0] = -r.ae * y[0] * y[1] - r.ai * y[0] * y[2] + r.gamma * y[3];
    f[1] = r.ae * y[0] * y[1] + r.ai * y[0] * y[2] - r.kappa * y[1] - r.rho * y[1];
    f[2] = r.kappa * y[1] - r.beta * y[2] - r.mu * y[2];
    f[3] = r.beta * y[2] + r.rho * y[1] - r.gamma * y[3];
    f[4] = r.mu * y[2];
}
__global__ __launch_bounds__(256) void seirp_sim(int B, int K, int par_steps, double dt, int saturated, int integrator,
                                                 const double *__restrict__ par, const double *__restrict__ init,
                                                 const double *__restrict__ sat, double *__restrict__ out)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= B) return;
    double y[5];
#pragma unroll
    for (int q = 0; q < 5; q++) { y[q] = init[(size_t)q * B + c]; out[(size_t)q * B + c] = y[q]; }
    double b0 = 0, bs = 0, m0 = 0, ms = 0, sg = 1, i_0 = 0;
    if (saturated) {
        b0 = sat[(size_t)0 * B + c]; bs = sat[(size_t)1 * B + c]; m0 = sat[(size_t)2 * B + c];
        ms = sat[(size_t)3 * B + c]; sg = sat[(size_t)4 * B + c]; i_0 = sat[(size_t)5 * B + c];
    }
    for (int t = 0; t < K - 1; t++) {
        const size_t pt = (par_steps == 1) ? 0 : (size_t)t;
        SeirpRates r;
        r.ae = par[(pt * 7 + 0) * B + c]; r.ai = par[(pt * 7 + 1) * B + c]; r.kappa = par[(pt * 7 + 2) * B + c];
        r.rho = par[(pt * 7 + 3) * B + c]; r.beta = par[(pt * 7 + 4) * B + c]; r.mu = par[(pt * 7 + 5) * B + c];
        r.gamma = par[(pt * 7 + 6) * B + c];
        if (saturated) {   // SEIRPSaturatedResource.m:27-29
            const double h = (epi_tanh((y[2] - i_0) / sg) + 1.0) / 2.0;
            r.beta = (bs - b0) * h + b0;
            r.mu = (ms - m0) * h + m0;
        }
        double yn[5];
        if (integrator == 0) {      // explicit Euler, the reference's integrator: (rhs)*dt + y
            double f[5];
            seirp_rhs(r, y, f);
#pragma unroll
            for (int q = 0; q < 5; q++) yn[q] = f[q] * dt + y[q];
        } else {                    // classical RK4 with the step's rates frozen (extension)
            double k1[5], k2[5], k3[5], k4[5], yt[5];
            seirp_rhs(r, y, k1);
#pragma unroll
            for (int q = 0; q < 5; q++) yt[q] = y[q] + 0.5 * dt * k1[q];
            seirp_rhs(r, yt, k2);
#pragma unroll
            for (int q = 0; q < 5; q++) yt[q] = y[q] + 0.5 * dt * k2[q];
            seirp_rhs(r, yt, k3);
#pragma unroll
            for (int q = 0; q < 5; q++) yt[q] = y[q] + dt * k3[q];
            seirp_rhs(r, yt, k4);
#pragma unroll
            for (int q = 0; q < 5; q++) yn[q] = y[q] + (dt / 6.0) * (k1[q] + 2.0 * k2[q] + 2.0 * k3[q] + k4[q]);
        }
#pragma unroll
        for (int q = 0; q < 5; q++) { y[q] = yn[q]; out[((size_t)(t + 1) * 5 + q) * B + c] = y[q]; }
    }
}

// Measurement utility: streams n doubles src -> dst with the SAME access shape as the filter kernels (one
// 8-byte element per lane, 512 B per wave instruction, grid-stride).  profiles/traffic_probe.py uses it to
// calibrate rocprofv3's FETCH_SIZE / WRITE_SIZE on a known byte count (MI355X_MICROARCH.md, HBM section).
__global__ __launch_bounds__(256) void calib_copy_f64(const double *__restrict__ src, double *__restrict__ dst, size_t n)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = src[i];
}

// epi_batch_desc.exact_nonfinite: only[c] = status bit 0 of chain c (the non-finite guard of GenericEKF.m:211 fired: its
// covariance overflowed at some day), only[B] = how many chains that is, only[B + 1 ...] = which (any order): the dense
// second pass's pinv grid walks that list instead of testing every (chain, step) pair
__global__ __launch_bounds__(256) void mark_nonfinite(const int32_t *__restrict__ status, int32_t *__restrict__ only, int B)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= B) return;
    const int v = status[c] & 1;
    only[c] = v;
    if (v) only[B + 1 + atomicAdd(only + B, 1)] = c;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static void set_err(char *err, const char *msg)
{
    if (err) { strncpy(err, msg, 255); err[255] = 0; }
}
static int hip_fail(char *err, hipError_t e, const char *what)
{
    char buf[256];
    snprintf(buf, sizeof buf, "HIP error in %s: %s", what, hipGetErrorString(e));
    set_err(err, buf);
    return EPI_ERR_HIP;
}

// [launch slices] -- host code only; tests/launch_slices_test.cpp compiles the lines between the two markers on their own
// A grid holds at most `cap` workgroups: launch(i0, ni) for every slice [i0, i0 + ni) of [0, items) in order, until one fails.
template <class F>
static hipError_t for_slices(int64_t items, int64_t cap, F &&launch)
{
    for (int64_t i0 = 0; i0 < items; i0 += cap) {
        const hipError_t e = launch(i0, (unsigned)(items - i0 < cap ? items - i0 : cap));
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
// A launch carries at most N counts by value: src[k0 .. k0 + kc) goes into the launch arguments' array, kc = min(K - k0, N).
template <int N>
static int copy_counts(int (&dst)[N], const int32_t *src, int k0, int K)
{
    const int kc = K - k0 < N ? K - k0 : N;
    for (int kk = 0; kk < kc; kk++) dst[kk] = src[k0 + kk];
    return kc;
}
// [/launch slices]

struct WsLayout { size_t s_minus, s_plus, p_minus, p_plus, x, rank, flag, innov, hand_s, hand_p, hand_i, only, status, total; };
static size_t padded_chains(const epi_batch_desc *d)
{
    const int blk = lane_block_of(d);
    return (size_t)((d->B + blk - 1) / blk) * blk;
}

// ---------------------------------------------------------------------------
// per-device state (the only state the library keeps besides the host entry points' context pool; both are freed by
// epi_host_pool_release): the SIMD count of each device, and idle helper streams
// ---------------------------------------------------------------------------
constexpr int kMaxDevices = 64;
// A helper stream of the LOWEST priority (its workgroups are placed after the caller's stream's) with the events one call
// needs to fork work onto it and join it back.  A call leases one for the time it takes to ENQUEUE its kernels; work of
// consecutive lessees simply queues up on the stream.
struct Helper { hipStream_t stream = nullptr; hipEvent_t ev[kHelperEvents] = {}; };
static std::mutex g_dev_mu;
static std::atomic<int> g_simds[kMaxDevices];
static std::vector<Helper *> g_helpers[kMaxDevices];
// helpers that were forked into a caller's stream CAPTURE: such a stream stays in capture mode until the caller ends the
// capture, which the library cannot see, so it is never leased again (another thread's hipEventRecord on it would fail or
// invalidate that capture); kept here until epi_host_pool_release
static std::vector<Helper *> g_retired_helpers[kMaxDevices];

static int current_device()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = 0;
    return dev;
}
static int simd_count(int dev)
{
    const int v = g_simds[dev].load(std::memory_order_relaxed);
    if (v > 0) return v;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
        (void)hipGetLastError();
        return 1024;                       // MI355X; not cached, so a later call asks the runtime again
    }
    g_simds[dev].store(cus * 4, std::memory_order_relaxed);
    return cus * 4;
}
static void helper_destroy(Helper *h)
{
    if (h->stream) { (void)hipStreamSynchronize(h->stream); (void)hipStreamDestroy(h->stream); }
    for (auto &ev : h->ev)
        if (ev) (void)hipEventDestroy(ev);
    delete h;
}
static hipError_t helper_acquire(int dev, Helper **out)
{
    {
        std::lock_guard<std::mutex> lk(g_dev_mu);
        if (!g_helpers[dev].empty()) { *out = g_helpers[dev].back(); g_helpers[dev].pop_back(); return hipSuccess; }
    }
    Helper *h = new Helper();
    int lo = 0, hi = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);      // lo = numerically largest = lowest priority
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&h->stream, hipStreamNonBlocking, lo);
    for (auto &ev : h->ev)
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) { helper_destroy(h); return e; }
    *out = h;
    return hipSuccess;
}
struct HelperLease {       // returns the helper to its device's idle list when the enqueueing call ends
    int dev; Helper *h = nullptr;
    bool captured = false;  // the caller's stream is being captured: the helper joined that capture and is retired instead
    explicit HelperLease(int d) : dev(d) {}
    ~HelperLease()
    {
        if (!h) return;
        std::lock_guard<std::mutex> lk(g_dev_mu);
        (captured ? g_retired_helpers[dev] : g_helpers[dev]).push_back(h);
    }
};
static void helpers_release_all()
{
    int prev = 0;
    const bool have_prev = hipGetDevice(&prev) == hipSuccess;
    for (int dev = 0; dev < kMaxDevices; dev++) {
        std::vector<Helper *> mine;
        {
            std::lock_guard<std::mutex> lk(g_dev_mu);
            mine.swap(g_helpers[dev]);
            mine.insert(mine.end(), g_retired_helpers[dev].begin(), g_retired_helpers[dev].end());
            g_retired_helpers[dev].clear();
        }
        if (mine.empty()) continue;
        (void)hipSetDevice(dev);
        for (Helper *h : mine) helper_destroy(h);
    }
    if (have_prev) (void)hipSetDevice(prev);
}

static WsLayout ws_layout(const epi_batch_desc *d)
{
    const int m = MODEL_TABLE[d->model].m;
    const size_t Bp = padded_chains(d);
    const size_t nS = (size_t)d->T * m * Bp * sizeof(double), nP = (size_t)d->T * m * m * Bp * sizeof(double);
    WsLayout w{};
    size_t off = 0;
    auto take = [&](bool need, size_t n) { size_t o = off; if (need) off += (n + 255) & ~(size_t)255; return o; };
    // fp32 storage: the forward quantities the smoother reads back are fp64 workspace whatever the caller selected
    const uint32_t om = d->storage ? (d->out_mask & ~(uint32_t)(EPI_OUT_S_MINUS | EPI_OUT_S_PLUS | EPI_OUT_P_MINUS | EPI_OUT_P_PLUS)) : d->out_mask;
    w.s_minus = take(!(om & EPI_OUT_S_MINUS), nS);
    w.s_plus = take(!(om & EPI_OUT_S_PLUS), nS);
    w.p_minus = take(!(om & EPI_OUT_P_MINUS), nP);
    w.p_plus = take(!(om & EPI_OUT_P_PLUS), nP);
    // smoother intermediates of the generic models: X = pinv(P_MINUS), packed upper triangle, and its rank word per (step, chain)
    const bool generic = MODEL_TABLE[d->model].generic;
    w.x = take(generic, (size_t)d->T * (m * (m + 1) / 2) * Bp * sizeof(double));
    w.rank = take(generic, (size_t)d->T * Bp * sizeof(int32_t));
    w.flag = take(generic, 256);
    // ekf_monitor reads the fp64 innovations: workspace when the caller does not take them as an fp64 output
    w.innov = take(monitor_hoisted(d) && (d->storage || !(d->out_mask & EPI_OUT_INNOVATIONS)), (size_t)d->T * Bp * sizeof(double));
    // hand-over rows between two backward launches (epi_sweep_run_device cuts the smoother where the horizon ends)
    w.hand_s = take(generic, (size_t)m * Bp * sizeof(double));
    w.hand_p = take(generic, (size_t)m * m * Bp * sizeof(double));
    w.hand_i = take(generic, Bp * sizeof(int32_t));
    // exact_nonfinite: the per-chain mask of the dense second pass (+ its counter) and a status array of the library's own
    // (the caller need not pass one)
    w.only = take(generic && d->exact_nonfinite >= 0, (2 * Bp + 1) * sizeof(int32_t));
    w.status = take(generic && d->exact_nonfinite >= 0, Bp * sizeof(int32_t));
    w.total = off;
    return w;
}

// ---------------------------------------------------------------------------
// launch logic
// ---------------------------------------------------------------------------
// the scoring tail of the Pareto sweep (epi_sweep_run_device): device pointers, validated by the entry point
struct Tail {
    int t_hist, R, P;
    const double *sp, *J0_prefix, *J1_prefix;
    double *J0, *J1;
    int32_t *on_front, *i_opt;
};
static_assert(pinv_wg<6>() == pinv_chains(6) && pinv_wg<3>() == pinv_chains(3), "launch_plan.hpp sizes the eks_pinv grid");

// Which kernels run, on which grids, in which order and on which stream is decided by plan_launch (launch_plan.hpp); what
// follows maps a plan's pick to the kernel it names and walks the plan's list.
template <class K, class... A>
static hipError_t launch(K kern, dim3 grid, int wg, size_t lds, hipStream_t st, const A &...args)
{
    if (lds > 64u * 1024u) {       // above the default dynamic-LDS limit
        const hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, grid, dim3(wg), lds, st, args...);
    return hipGetLastError();
}

// the innovation monitor as its own launch (after the forward kernel that wrote the innovations)
template <int FLIP>
static hipError_t launch_monitor(const KArgs &ka, const LaunchPlan &p, hipStream_t st)
{
    const dim3 grid(p.mon_gx, p.mon_gy);
    if (p.mon.kernel == MON_PAR) return launch(ekf_monitor_par<FLIP, 21, kMonitorParDays>, grid, kWave, 0, st, ka, ka.dense_flag);
    if (p.mon.bits & V_L21) return launch(ekf_monitor<FLIP, 21>, grid, kWave, p.mon.lds, st, ka, ka.dense_flag);
    return launch(ekf_monitor<FLIP, 0>, grid, kWave, p.mon.lds, st, ka, ka.dense_flag);
}

// forward kernel(s) over filter steps [o.a, o.b) of the chains [o.c0, o.c0 + o.cn)
template <int M, int FLIP, int GENERIC>
static hipError_t enqueue_fwd(KArgs ka, const LaunchPlan &p, const PlanOp &o, hipStream_t st)
{
    ka.k_begin = o.a; ka.k_end = o.b; ka.c0 = o.c0; ka.cn = o.cn;
    const unsigned v = p.fwd.bits;
    auto go = [&](auto kern) { return launch(kern, dim3(o.grid), kWave, p.fwd.lds, st, ka, (const int *)ka.dense_flag); };
    hipError_t e = hipSuccess;
    if constexpr (M == 6 && !GENERIC) {
        if (p.fwd.kernel == FWD_WAVE_NC) e = (v & V_L21) ? go(ekf_fwd_wave<0, 1, 21, 0>) : go(ekf_fwd_wave<0, 1, 0, 0>);
    }
    if constexpr (M == 6 && GENERIC) {
        if (p.fwd.kernel == FWD_WAVE)
            e = !(v & V_INLINE) ? go(ekf_fwd_wave<FLIP, 0>) : (v & V_L21) ? go(ekf_fwd_wave<FLIP, 1, 21>) : go(ekf_fwd_wave<FLIP, 1, 0>);
        if (p.fwd.kernel == FWD_HEX)
            e = (v & V_BLK) ? ((v & V_SOLO) ? go(ekf_fwd_hex<FLIP, kHG, 1>) : go(ekf_fwd_hex<FLIP, kHG, 0>))
                            : ((v & V_SOLO) ? go(ekf_fwd_hex<FLIP, 0, 1>) : go(ekf_fwd_hex<FLIP, 0, 0>));
        if (p.fwd.kernel == FWD_QUAD) {
            if (v & V_INLINE) e = (v & V_BLK) ? go(ekf_fwd_quad<FLIP, kQC, 21, 1, 0>) : go(ekf_fwd_quad<FLIP, 0, 0, 1, 0>);
            else if (v & V_SOLO) e = (v & V_BLK) ? go(ekf_fwd_quad<FLIP, kQC, 21, 0, 1>) : go(ekf_fwd_quad<FLIP, 0, 0, 0, 1>);
            else e = (v & V_BLK) ? go(ekf_fwd_quad<FLIP, kQC, 21, 0, 0>) : go(ekf_fwd_quad<FLIP, 0, 0, 0, 0>);
        }
    }
    if constexpr (M == 3 && GENERIC) {
        if (p.fwd.kernel == FWD_WAVE3) e = go(ekf_fwd_wave3<FLIP>);
    }
    if constexpr (GENERIC) {
        if (p.fwd.kernel == FWD_SYM) {
            if (v & V_INLINE) e = (v & V_STOR) ? go(ekf_fwd_sym<M, FLIP, 0, 1>) : (v & V_LP) ? go(ekf_fwd_sym<M, FLIP, 1>) : go(ekf_fwd_sym<M, FLIP, 0>);
            else if (v & V_STOR) e = go(ekf_fwd_sym<M, FLIP, 0, 1, 0>);
            else if (v & V_USD) e = go(ekf_fwd_sym<M, FLIP, 1, 0, 0, 1>);
            else e = (v & V_LP) ? go(ekf_fwd_sym<M, FLIP, 1, 0, 0>) : go(ekf_fwd_sym<M, FLIP, 0, 0, 0>);
        }
    }
    if (e == hipSuccess && p.dense) e = launch(ekf_fwd<M, FLIP, GENERIC>, dim3(o.dense_grid), kWave, p.dense_lds, st, ka);
    return e;
}

// X = pinv(P(j|j-1)) for the o.b array positions from pinv_pos0 + o.a on
template <int M>
static hipError_t enqueue_pinv(KArgs ka, const PlanOp &o, hipStream_t st)
{
    ka.c0 = o.c0; ka.cn = o.cn; ka.pinv_step0 = o.a;
    const dim3 grid(o.grid, (unsigned)o.b);
    return ka.only ? launch(eks_pinv<M, 1>, grid, pinv_wg<M>(), 0, st, ka) : launch(eks_pinv<M, 0>, grid, pinv_wg<M>(), 0, st, ka);
}

// backward recursion over smoother steps o.a ... o.b (the dense kernels only know the full range) of the chains [o.c0, o.c0 + o.cn)
template <int M, int FLIP, int GENERIC>
static hipError_t enqueue_bwd(KArgs ka, const LaunchPlan &p, const PlanOp &o, hipStream_t st)
{
    ka.bk_from = o.a; ka.bk_to = o.b; ka.c0 = o.c0; ka.cn = o.cn;
    const unsigned v = p.bwd.bits;
    auto go = [&](auto kern) { return launch(kern, dim3(o.grid), kWave, 0, st, ka, (const int *)ka.dense_flag); };
    hipError_t e = hipSuccess;
    if constexpr (M == 6 && !GENERIC) {
        if (p.bwd.kernel == BWD_WAVE_NC) e = launch(eks_bwd_wave_nc, dim3(o.grid), kWave, 0, st, ka);
    }
    if constexpr (M == 6 && GENERIC) {
        if (p.bwd.kernel == BWD_WAVE) e = go(eks_bwd_wave<FLIP>);
        if (p.bwd.kernel == BWD_HEX)
            e = (v & V_BLK) ? ((v & V_SOLO) ? go(eks_bwd_hex<FLIP, kHG, 2>) : go(eks_bwd_hex<FLIP, kHG, 0>))
                            : ((v & V_SOLO) ? go(eks_bwd_hex<FLIP, 0, 1>) : go(eks_bwd_hex<FLIP, 0, 0>));
        if (p.bwd.kernel == BWD_QUAD) e = (v & V_BLK) ? go(eks_bwd_quad<FLIP, kQC>) : go(eks_bwd_quad<FLIP, 0>);
        if (p.bwd.kernel == BWD_LANE6)
            e = p.bwd.wg_chains == 40 ? (o.xd ? go(eks_bwd_lane6<FLIP, 40, 1>) : go(eks_bwd_lane6<FLIP, 40, 0>))
                                      : (p.bwd.wg_chains == 48 ? go(eks_bwd_lane6<FLIP, 48, 0>) : go(eks_bwd_lane6<FLIP, 56, 0>));
    }
    if constexpr (M == 3 && GENERIC) {
        if (p.bwd.kernel == BWD_WAVE3) e = go(eks_bwd_wave3<FLIP>);
    }
    if constexpr (GENERIC) {
        if (p.bwd.kernel == BWD_SYM) e = (v & V_STOR) ? go(eks_bwd_sym<M, FLIP, 1>) : go(eks_bwd_sym<M, FLIP>);
    }
    if (e == hipSuccess && p.dense) e = launch(eks_bwd<M, FLIP, GENERIC>, dim3(o.dense_grid), kWave, 0, st, ka);
    return e;
}

// scoring of the sweep's horizon (TrainPredictPrescribeNPI.m:481-493) from the u_opt_smooth the smoother just wrote,
// then the Pareto filter and optimum per region (:624-633) when the call holds whole regions
static hipError_t enqueue_tail(const KArgs &ka, const Tail &t, hipStream_t st, const int32_t *gate = nullptr)
{
    epi_sim_desc sd{};
    sd.abi_version = EPIEKF_ABI_VERSION; sd.B = ka.B; sd.K = ka.T - t.t_hist; sd.Su = ka.B; sd.n_npi = ka.n_npi;
    sd.noise = 0; sd.with_cost = 1; sd.prefix_days = t.t_hist; sd.u_block = ka.blk >= ka.B ? 0 : ka.blk;
    // day t_hist of u_opt_smooth: a time slice is n_npi rows of nblk * blk chains in either layout
    const double *u_h = ka.u_opt_smooth + (size_t)t.t_hist * ka.n_npi * ((size_t)ka.nblk * ka.blk);
    hipLaunchKernelGGL(sialpha_sim, dim3((ka.B + 255) / 256), dim3(256), 0, st, sd, (const int32_t *)nullptr, u_h, t.sp,
                       (const double *)nullptr, (double *)nullptr, (double *)nullptr, (double *)nullptr, t.J0, t.J1,
                       t.J0_prefix, t.J1_prefix, gate);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || (!t.on_front && !t.i_opt)) return e;
    hipLaunchKernelGGL(pareto_front, dim3(t.R), dim3(256), (size_t)2 * t.P * sizeof(double), st, t.P, t.J0, t.J1, t.on_front, t.i_opt, gate);
    return hipGetLastError();
}

// the plan's operations in the plan's order; `h` is the leased helper stream when the plan asks for one
template <int M, int FLIP, int GENERIC>
static hipError_t run_plan(const KArgs &ka, const LaunchPlan &p, const Tail *tail, hipStream_t st, Helper *h)
{
    if (p.overflow || (p.helper && !h)) return hipErrorInvalidValue;
    for (int i = 0; i < p.n_ops; i++) {
        const PlanOp &o = p.ops[i];
        hipStream_t s = o.stream == ON_HELPER ? h->stream : st;
        hipError_t e = hipSuccess;
        switch (o.kind) {
        case OP_FWD: e = enqueue_fwd<M, FLIP, GENERIC>(ka, p, o, s); break;
        case OP_PINV: e = enqueue_pinv<M>(ka, o, s); break;
        case OP_BWD: e = enqueue_bwd<M, FLIP, GENERIC>(ka, p, o, s); break;
        case OP_MONITOR: e = launch_monitor<FLIP>(ka, p, s); break;
        case OP_TAIL: e = enqueue_tail(ka, *tail, s); break;
        case OP_RECORD: e = hipEventRecord(h->ev[o.a], s); break;
        case OP_WAIT: e = hipStreamWaitEvent(s, h->ev[o.a], 0); break;
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// epi_batch_desc.exact_nonfinite.  The packed / quad kernels skip products with structural zeros, which is exact for finite
// operands; once a chain's covariance has overflowed, a skipped `Inf * 0` leaves a finite number where the dense evaluation
// (the reference's, and MATLAB's BLAS) has NaN.  Up to the first overflow both evaluations hold the same bits, so the
// non-finite guard of :211 fires for such a chain in either (status bit 0).  Those chains -- and only those -- are run again
// from the start by the dense kernels, which mirror the reference term for term, writing over their outputs in place; then
// the scoring tail is repeated if any chain was re-run.  Costs three launches that return at once when no chain is marked
// (the pinv grid's ~(B/64)(T-1) empty workgroups: ~0.15 ms at 75 000 x 520).
template <int M, int FLIP>
static hipError_t rerun_nonfinite_dense(const KArgs &ka, const PlanIn &in, const Tail *tail, hipStream_t st)
{
    hipError_t e = hipMemsetAsync(ka.only_buf + ka.B, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mark_nonfinite, dim3((ka.B + 255) / 256), dim3(256), 0, st, (const int32_t *)ka.status, ka.only_buf, ka.B);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    PlanIn ind = in;
    ind.hint = 2; ind.only = true; ind.smooth = true; ind.rerun = false; ind.has_tail = false;
    const LaunchPlan pd = plan_launch(ind);
    KArgs kd = ka;
    kd.only = ka.only_buf; kd.dense_flag = nullptr; kd.quad = pd.quad; kd.hex = pd.hex; kd.mon_hoist = pd.mon_hoist;
    if ((e = run_plan<M, FLIP, 1>(kd, pd, nullptr, st, nullptr)) != hipSuccess) return e;
    if (tail) e = enqueue_tail(ka, *tail, st, ka.only_buf + ka.B);
    return e;
}

template <int M, int FLIP, int GENERIC>
static hipError_t launch_chain(const KArgs &ka, const PlanIn &in, const LaunchPlan &p, const Tail *tail, int dev, hipStream_t st)
{
    hipError_t e = hipSuccess;
    if (p.precheck >= 0) {
        if ((e = hipMemsetAsync(ka.dense_flag, 0, sizeof(int), st)) != hipSuccess) return e;
        if (p.precheck == 1) hipLaunchKernelGGL((ekf_precheck<M>), dim3((ka.B + 255) / 256), dim3(256), 0, st, ka, ka.dense_flag, 0);
        if (p.precheck == 2) hipLaunchKernelGGL((ekf_precheck<M>), dim3(1), dim3(64), 0, st, ka, ka.dense_flag, 1);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    HelperLease lease(dev);
    if (p.helper) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess) (void)hipGetLastError();    // the legacy default stream cannot be queried while another stream captures
        lease.captured = cs != hipStreamCaptureStatusNone;
        if ((e = helper_acquire(dev, &lease.h)) != hipSuccess) return e;
    }
    e = run_plan<M, FLIP, GENERIC>(ka, p, tail, st, lease.h);
    if constexpr (GENERIC) {
        if (e == hipSuccess && p.rerun_after) e = rerun_nonfinite_dense<M, FLIP>(ka, in, tail, st);
    }
    return e;
}

// the one thing the plan takes from the device: its SIMD count
static PlanIn plan_input(const epi_batch_desc *d, int dev) { PlanIn in{}; in.d = d; in.n_simds = simd_count(dev); return in; }

}  // namespace epi

using namespace epi;

extern "C" {

int epi_abi_version(void) { return EPIEKF_ABI_VERSION; }

const char *epi_status_string(int status)
{
    switch (status) {
    case EPI_OK: return "ok";
    case EPI_ERR_UNDEFINED_ORDER: return "Undefined order";
    case EPI_ERR_Q_MISMATCH: return "Process noise covariance noise mismatch";
    case EPI_ERR_R_MISMATCH: return "Observation noise covariance noise mismatch";
    case EPI_ERR_OBS_TYPE: return "unknown observation type";
    case EPI_ERR_BAD_ARG: return "bad argument";
    case EPI_ERR_WORKSPACE: return "workspace too small";
    case EPI_ERR_HIP: return "HIP runtime error";
    case EPI_ERR_UNSUPPORTED: return "unsupported";
    default: return "unknown status";
    }
}

int epi_model_dim(int model) { return (model >= 0 && model < 6) ? MODEL_TABLE[model].m : -1; }

int epi_ekf_validate(const epi_batch_desc *d, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->model < 0 || d->model > 5) { set_err(err, "unknown model"); return EPI_ERR_BAD_ARG; }
    if (d->B < 1 || d->T < 1 || d->Sx < 1 || d->Su < 1 || d->L < 1) { set_err(err, "B, T, Sx, Su, L must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->T > 65536) { set_err(err, "T is limited to 65536 (grid y dimension of eks_pinv)"); return EPI_ERR_BAD_ARG; }
    if (d->B > (1 << 23) || d->Sx > (1 << 23) || d->Su > (1 << 23)) { set_err(err, "B, Sx, Su are limited to 2^23 (a per-step array slice is addressed through one 4 GiB buffer descriptor)"); return EPI_ERR_BAD_ARG; }
    if (d->n_npi < 1 || d->n_npi > EPI_MAX_NPI) { set_err(err, "n_npi out of range 1..12"); return EPI_ERR_BAD_ARG; }
    if (d->order != 1 && d->order != 2) { set_err(err, epi_status_string(EPI_ERR_UNDEFINED_ORDER)); return EPI_ERR_UNDEFINED_ORDER; }
    const ModelInfo &mi = MODEL_TABLE[d->model];
    if (!mi.obs_fixed && d->obs_type != EPI_OBS_NEWCASES && d->obs_type != EPI_OBS_TOTALCASES) {
        set_err(err, epi_status_string(EPI_ERR_OBS_TYPE)); return EPI_ERR_OBS_TYPE;
    }
    if (d->q_mode != 0 && d->q_mode != 1) { set_err(err, epi_status_string(EPI_ERR_Q_MISMATCH)); return EPI_ERR_Q_MISMATCH; }
    if (!mi.generic && d->q_mode != 0) {   // NewCase...m:30  Q = Q_w is added to an m x m matrix as it is
        set_err(err, epi_status_string(EPI_ERR_Q_MISMATCH)); return EPI_ERR_Q_MISMATCH;
    }
    if (d->r_mode != 0 && d->r_mode != 1) { set_err(err, epi_status_string(EPI_ERR_R_MISMATCH)); return EPI_ERR_R_MISMATCH; }
    if (!mi.generic && d->r_mode != 0) {   // NewCase...m:31  R = R_v is used as a scalar
        set_err(err, epi_status_string(EPI_ERR_R_MISMATCH)); return EPI_ERR_R_MISMATCH;
    }
    // three fp64 windows of L samples per lane must fit the CU's 160 KiB LDS
    if (d->phase < 0 || d->phase > 4) { set_err(err, "phase must be 0..4"); return EPI_ERR_BAD_ARG; }
    if (d->path_hint < 0 || d->path_hint > 2) { set_err(err, "path_hint must be 0, 1 or 2"); return EPI_ERR_BAD_ARG; }
    if (d->time_pipe < -1 || d->time_pipe > 1) { set_err(err, "time_pipe must be -1 (off), 0 (auto) or 1 (on)"); return EPI_ERR_BAD_ARG; }
    if (d->lane_block < 0) { set_err(err, "lane_block must be >= 0"); return EPI_ERR_BAD_ARG; }
    if (d->shape < 0 || d->shape > 4) { set_err(err, "shape must be 0 (auto), 1 (one lane per chain), 2 (four lanes per chain), 3 (one wavefront per chain) or 4 (six lanes per chain)"); return EPI_ERR_BAD_ARG; }
    if (d->storage < 0 || d->storage > 1) { set_err(err, "storage must be 0 (fp64) or 1 (fp32)"); return EPI_ERR_BAD_ARG; }
    if (d->exact_nonfinite < -1 || d->exact_nonfinite > 1) { set_err(err, "exact_nonfinite must be 0 (default: on), 1 (on) or -1 (off)"); return EPI_ERR_BAD_ARG; }
    if (d->placement_tries < 0 || d->placement_tries > EPI_PLACEMENT_MAX_TRIES) { set_err(err, "placement_tries must be 0 .. EPI_PLACEMENT_MAX_TRIES"); return EPI_ERR_BAD_ARG; }
    if (d->test_window < 0 || d->test_window == 1) { set_err(err, "test_window must be 0 (production) or >= 2"); return EPI_ERR_BAD_ARG; }
    if (d->test_flags < 0 || d->test_flags > 7) { set_err(err, "test_flags must be 0 (production) .. 7"); return EPI_ERR_BAD_ARG; }
    if (padded_chains(d) > ((size_t)1 << 23)) { set_err(err, "B rounded up to lane_block exceeds 2^23"); return EPI_ERR_BAD_ARG; }
    if ((size_t)3 * d->L * kWave * sizeof(double) > 160u * 1024u) { set_err(err, "inv_monitor_len too large for LDS (max 106)"); return EPI_ERR_UNSUPPORTED; }
    return EPI_OK;
}

size_t epi_ekf_workspace_bytes(const epi_batch_desc *d)
{
    if (epi_ekf_validate(d, nullptr) != EPI_OK) return 0;
    return ws_layout(d).total;
}

int epi_ekf_preferred_lane_block(const epi_batch_desc *d)
{
    epi_batch_desc probe;
    if (!d) return 0;
    probe = *d; probe.lane_block = 0;
    if (epi_ekf_validate(&probe, nullptr) != EPI_OK) return 0;
    const int lw = plan_launch(plan_input(d, current_device())).chains_per_wave;
    return lw < d->B ? lw : d->B;
}

static int run_device_impl(const epi_batch_desc *d, const epi_inputs *in, const epi_outputs *out,
                           void *workspace, size_t workspace_bytes, const Tail *tail, void *stream, char *err)
{
    int rc = epi_ekf_validate(d, err);
    if (rc != EPI_OK) return rc;
    if (!in || !out) { set_err(err, "NULL inputs/outputs"); return EPI_ERR_BAD_ARG; }
    const ModelInfo &mi = MODEL_TABLE[d->model];
    if (!in->x || !in->u || !in->prm || !in->s_init || !in->Ps_init || !in->s_final || !in->Ps_final || !in->Q) {
        set_err(err, "NULL input array"); return EPI_ERR_BAD_ARG;
    }
    if (d->r_mode == 0 && !in->R_scalar) { set_err(err, "r_mode 0 needs R_scalar"); return EPI_ERR_BAD_ARG; }
    if (d->r_mode == 1 && !in->R_series) { set_err(err, "r_mode 1 needs R_series"); return EPI_ERR_BAD_ARG; }
    if (!in->x_series && d->Sx != d->B) { set_err(err, "identity x_series needs Sx == B"); return EPI_ERR_BAD_ARG; }
    if (!in->u_series && d->Su != d->B) { set_err(err, "identity u_series needs Su == B"); return EPI_ERR_BAD_ARG; }
    const WsLayout wl = ws_layout(d);
    if (wl.total > 0 && (!workspace || workspace_bytes < wl.total)) {
        set_err(err, epi_status_string(EPI_ERR_WORKSPACE)); return EPI_ERR_WORKSPACE;
    }
    const bool f32 = d->storage == 1;
    if (f32 && (!mi.generic || d->q_mode != 0 || d->path_hint != 1)) {
        set_err(err, "storage = 1 (fp32) runs the packed kernels of the generic models only: fixed Q_w and path_hint = 1 "
                     "(epi_ekf_precheck_device said the batch qualifies)");
        return EPI_ERR_UNSUPPORTED;
    }
    // fp32 storage: every fp64 output pointer the kernels see is either workspace (forward quantities) or NULL
    const uint32_t om = f32 ? 0u : d->out_mask;
    const uint32_t om32 = f32 ? d->out_mask : 0u;
    auto sel = [&](uint32_t bit, double *p) -> double * { return (om & bit) ? p : nullptr; };
    auto sel32 = [&](uint32_t bit, double *p) -> float * { return (om32 & bit) ? (float *)p : nullptr; };
    char *ws = (char *)workspace;
    KArgs ka{};
    ka.B = d->B; ka.T = d->T; ka.Sx = d->Sx; ka.Su = d->Su; ka.n_npi = d->n_npi; ka.L = d->L; ka.r_mode = d->r_mode; ka.q_mode = d->q_mode;
    ka.blk = lane_block_of(d); ka.nblk = (d->B + ka.blk - 1) / ka.blk;
    ka.mon_scan = (d->test_flags >> 1) & 1;
    ka.hexw = d->test_window;      // test hook (0 in production): days per addressing window, see epi_batch_desc.test_window
    ka.stor = f32 ? 1 : 0;
    ka.bk_from = d->T - 2; ka.bk_to = 0;
    ka.c0 = 0; ka.cn = d->B;
    ka.mf.lo_is_zero = mi.lo_is_zero; ka.mf.phi_ge = mi.phi_ge; ka.mf.obs_clamp = mi.obs_clamp;
    ka.mf.obs_type = mi.obs_fixed ? EPI_OBS_NEWCASES : d->obs_type;
    ka.x_series = in->x_series; ka.u_series = in->u_series;
    ka.x = in->x; ka.u = in->u; ka.R_series = in->R_series; ka.R_scalar = in->R_scalar; ka.prm = in->prm; ka.Q = in->Q;
    if (!mi.flipped) {
        ka.s_init = in->s_init; ka.Ps_init = in->Ps_init; ka.s_final = in->s_final; ka.Ps_final = in->Ps_final;
    } else {   // Backward*.m:21-24
        ka.s_init = in->s_final; ka.Ps_init = in->Ps_final; ka.s_final = in->s_init; ka.Ps_final = in->Ps_init;
    }
    const bool has_uos = mi.generic;
    ka.S_MINUS = (om & EPI_OUT_S_MINUS) ? out->S_MINUS : (double *)(ws + wl.s_minus);
    ka.S_PLUS = (om & EPI_OUT_S_PLUS) ? out->S_PLUS : (double *)(ws + wl.s_plus);
    ka.P_MINUS = (om & EPI_OUT_P_MINUS) ? out->P_MINUS : (double *)(ws + wl.p_minus);
    ka.P_PLUS = (om & EPI_OUT_P_PLUS) ? out->P_PLUS : (double *)(ws + wl.p_plus);
    // what the plan is asked for this call (plan_call_input, launch_plan.hpp): smoother or not, the dense second pass, ws_upper
    const int dev = current_device();
    const PlanIn pin = plan_call_input(d, plan_input(d, dev).n_simds, out->pinv_rank != nullptr, out->status != nullptr, tail != nullptr,
                                       tail ? tail->t_hist : 0);
    ka.ws_upper = pin.ws_upper;
    // fp32 storage, 3 states: the packed smoother recomputes s(k+1|k) from s(k|k) (ekf_sym.hpp, RC), nothing reads an
    // fp64 S_MINUS back -- the forward kernel then stores the caller's fp32 copy only
    if (f32 && mi.m == 3) ka.S_MINUS = nullptr;
    ka.u_opt = sel(EPI_OUT_U_OPT, out->u_opt);
    ka.u_opt_smooth = has_uos ? sel(EPI_OUT_U_OPT_SMOOTH, out->u_opt_smooth) : nullptr;
    ka.S_SMOOTH = sel(EPI_OUT_S_SMOOTH, out->S_SMOOTH);
    ka.P_SMOOTH = sel(EPI_OUT_P_SMOOTH, out->P_SMOOTH);
    ka.K_GAIN = sel(EPI_OUT_K_GAIN, out->K_GAIN);
    ka.innovations = sel(EPI_OUT_INNOVATIONS, out->innovations);
    ka.rho = sel(EPI_OUT_RHO, out->rho);
    ka.f.u_opt = sel32(EPI_OUT_U_OPT, out->u_opt);
    ka.f.u_opt_smooth = has_uos ? sel32(EPI_OUT_U_OPT_SMOOTH, out->u_opt_smooth) : nullptr;
    ka.f.S_MINUS = sel32(EPI_OUT_S_MINUS, out->S_MINUS); ka.f.S_PLUS = sel32(EPI_OUT_S_PLUS, out->S_PLUS);
    ka.f.S_SMOOTH = sel32(EPI_OUT_S_SMOOTH, out->S_SMOOTH);
    ka.f.P_MINUS = sel32(EPI_OUT_P_MINUS, out->P_MINUS); ka.f.P_PLUS = sel32(EPI_OUT_P_PLUS, out->P_PLUS);
    ka.f.P_SMOOTH = sel32(EPI_OUT_P_SMOOTH, out->P_SMOOTH);
    ka.f.K_GAIN = sel32(EPI_OUT_K_GAIN, out->K_GAIN); ka.f.innovations = sel32(EPI_OUT_INNOVATIONS, out->innovations);
    ka.f.rho = sel32(EPI_OUT_RHO, out->rho);
    ka.pinv_rank = out->pinv_rank; ka.status = out->status;
    if (mi.generic && d->exact_nonfinite >= 0) {
        ka.only_buf = (int32_t *)(ws + wl.only);
        if (!ka.status && pin.rerun) ka.status = (int32_t *)(ws + wl.status);
    }
    const LaunchPlan plan = plan_launch(pin);
    ka.quad = plan.quad; ka.wave = plan.wave; ka.hex = plan.hex; ka.mon_hoist = plan.mon_hoist; ka.lw = plan.lw;
    if (ka.mon_hoist && !ka.innovations && (ka.rho || ka.f.rho)) ka.innovations = (double *)(ws + wl.innov);
    ka.X = mi.generic ? (double *)(ws + wl.x) : nullptr;
    ka.rankbuf = mi.generic ? (int32_t *)(ws + wl.rank) : nullptr;
    ka.pinv_pos0 = mi.flipped ? 0 : 1;
    ka.dense_flag = mi.generic ? (int *)(ws + wl.flag) : nullptr;
    if (mi.generic) {
        ka.hand_s = (double *)(ws + wl.hand_s); ka.hand_p = (double *)(ws + wl.hand_p); ka.hand_i = (int32_t *)(ws + wl.hand_i);
        ka.hand_pitch = (int)padded_chains(d);
    }
    {
        struct { uint32_t bit; const void *p; const char *n; } chk[] = {
            {EPI_OUT_U_OPT, out->u_opt, "u_opt"}, {EPI_OUT_S_MINUS, out->S_MINUS, "S_MINUS"},
            {EPI_OUT_S_PLUS, out->S_PLUS, "S_PLUS"}, {EPI_OUT_S_SMOOTH, out->S_SMOOTH, "S_SMOOTH"},
            {EPI_OUT_P_MINUS, out->P_MINUS, "P_MINUS"}, {EPI_OUT_P_PLUS, out->P_PLUS, "P_PLUS"},
            {EPI_OUT_P_SMOOTH, out->P_SMOOTH, "P_SMOOTH"}, {EPI_OUT_K_GAIN, out->K_GAIN, "K_GAIN"},
            {EPI_OUT_INNOVATIONS, out->innovations, "innovations"}, {EPI_OUT_RHO, out->rho, "rho"}};
        for (auto &q : chk)
            if (((om | om32) & q.bit) && !q.p) { char b[128]; snprintf(b, sizeof b, "output %s selected but NULL", q.n); set_err(err, b); return EPI_ERR_BAD_ARG; }
        if (has_uos && ((om | om32) & EPI_OUT_U_OPT_SMOOTH) && !out->u_opt_smooth) { set_err(err, "output u_opt_smooth selected but NULL"); return EPI_ERR_BAD_ARG; }
    }
    hipStream_t st = (hipStream_t)stream;
    if (tail && (!ka.u_opt_smooth || d->phase != 0)) { set_err(err, "the sweep's scoring tail needs a full call (phase 0) with fp64 u_opt_smooth selected"); return EPI_ERR_BAD_ARG; }
    hipError_t e;
    switch (d->model) {
    case EPI_MODEL_SIA3: e = launch_chain<3, 0, 1>(ka, pin, plan, tail, dev, st); break;
    case EPI_MODEL_SIA6: e = launch_chain<6, 0, 1>(ka, pin, plan, tail, dev, st); break;
    case EPI_MODEL_SIA3_BWD: e = launch_chain<3, 1, 1>(ka, pin, plan, tail, dev, st); break;
    case EPI_MODEL_SIA6_BWD: e = launch_chain<6, 1, 1>(ka, pin, plan, tail, dev, st); break;
    default: e = launch_chain<6, 0, 0>(ka, pin, plan, tail, dev, st); break;
    }
    if (e != hipSuccess) return hip_fail(err, e, "kernel launch");
    return EPI_OK;
}

int epi_ekf_run_device(const epi_batch_desc *d, const epi_inputs *in, const epi_outputs *out,
                       void *workspace, size_t workspace_bytes, void *stream, char *err)
{
    return run_device_impl(d, in, out, workspace, workspace_bytes, nullptr, stream, err);
}

static int sweep_args_ok(const epi_batch_desc *d, const epi_sweep_desc *sd, const double *sp, const double *J0_prefix,
                         const double *J1_prefix, double *J0, double *J1, int32_t *on_front, int32_t *i_opt, char *err)
{
    if (!d || !sd || sd->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "bad sweep descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->model != EPI_MODEL_SIA6) { set_err(err, "the cost-weight sweep runs SIAlphaModelEKFOptControlled (EPI_MODEL_SIA6)"); return EPI_ERR_UNSUPPORTED; }
    if (sd->t_hist < 1 || sd->t_hist >= d->T) { set_err(err, "t_hist must leave at least one horizon day: 1 <= t_hist < T"); return EPI_ERR_BAD_ARG; }
    if (!sp || !J0_prefix || !J1_prefix || !J0 || !J1) { set_err(err, "NULL scoring array"); return EPI_ERR_BAD_ARG; }
    if (on_front || i_opt) {
        if (sd->R < 1 || sd->P < 1 || (int64_t)sd->R * sd->P != (int64_t)d->B) { set_err(err, "the Pareto filter needs whole regions: B == R * P"); return EPI_ERR_BAD_ARG; }
        if (sd->P > 8192) { set_err(err, "more than 8192 points per region"); return EPI_ERR_UNSUPPORTED; }
    }
    if (d->storage != 0 || !(d->out_mask & EPI_OUT_U_OPT_SMOOTH)) { set_err(err, "the sweep scores the fp64 u_opt_smooth output: select it (storage 0)"); return EPI_ERR_BAD_ARG; }
    return EPI_OK;
}

int epi_sweep_run_device(const epi_batch_desc *d, const epi_inputs *in, const epi_outputs *out, void *workspace,
                         size_t workspace_bytes, const epi_sweep_desc *sd, const double *sp, const double *J0_prefix,
                         const double *J1_prefix, double *J0, double *J1, int32_t *on_front, int32_t *i_opt, void *stream,
                         char *err)
{
    int rc = sweep_args_ok(d, sd, sp, J0_prefix, J1_prefix, J0, J1, on_front, i_opt, err);
    if (rc != EPI_OK) return rc;
    Tail t{};
    t.t_hist = sd->t_hist; t.R = sd->R; t.P = sd->P;
    t.sp = sp; t.J0_prefix = J0_prefix; t.J1_prefix = J1_prefix; t.J0 = J0; t.J1 = J1; t.on_front = on_front; t.i_opt = i_opt;
    if ((on_front || i_opt) && (size_t)2 * sd->P * sizeof(double) > 64u * 1024u) {
        hipError_t e = hipFuncSetAttribute((const void *)pareto_front, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)2 * sd->P * sizeof(double)));
        if (e != hipSuccess) return hip_fail(err, e, "hipFuncSetAttribute");
    }
    epi_batch_desc full = *d;
    full.phase = 0;
    return run_device_impl(&full, in, out, workspace, workspace_bytes, &t, stream, err);
}

// (forward + monitor, pinv grid, smoother) milliseconds of this call on THESE arrays, enqueued stage by stage (phases 1, 3, 4)
// between HIP events on `stream`: the mean over as many rounds as fill `min_ms` of device time (at least one), after one untimed
// round.  Synchronous.  What a device-pointer caller compares allocations with ("Placement"): the same arrays give the
// same times run after run, another allocation of the same arrays may be 5-15 % off.
int epi_ekf_time_stages_device(const epi_batch_desc *d, const epi_inputs *in, const epi_outputs *out, void *workspace,
                               size_t workspace_bytes, void *stream, double min_ms, double *ms, char *err)
{
    if (!d || !ms) { set_err(err, "NULL descriptor / result array"); return EPI_ERR_BAD_ARG; }
    epi_batch_desc s = *d;
    hipStream_t st = (hipStream_t)stream;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int i = 0; i < 4 && e == hipSuccess; i++) e = hipEventCreate(&ev[i]);
    auto done = [&](int rc) { for (auto &x : ev) if (x) (void)hipEventDestroy(x); return rc; };
    if (e != hipSuccess) return done(hip_fail(err, e, "hipEventCreate"));
    const int phases[3] = {1, 3, 4};
    double acc[3] = {0.0, 0.0, 0.0}, total = 0.0;
    int rounds = 0;
    for (int r = -1; r < 4096 && (r < 1 || total < min_ms); r++) {       // r = -1: the untimed round
        (void)hipEventRecord(ev[0], st);
        for (int q = 0; q < 3; q++) {
            s.phase = phases[q];
            const int rc = epi_ekf_run_device(&s, in, out, workspace, workspace_bytes, stream, err);
            if (rc != EPI_OK) { (void)hipStreamSynchronize(st); return done(rc); }
            (void)hipEventRecord(ev[q + 1], st);
        }
        if ((e = hipStreamSynchronize(st)) != hipSuccess) return done(hip_fail(err, e, "kernel execution"));
        if (r < 0) continue;
        for (int q = 0; q < 3; q++) {
            float t = 0.0f;
            (void)hipEventElapsedTime(&t, ev[q], ev[q + 1]);
            acc[q] += t; total += t;
        }
        rounds++;
    }
    for (int q = 0; q < 3; q++) ms[q] = acc[q] / (double)rounds;
    return done(EPI_OK);
}

int epi_ekf_precheck_device(const epi_batch_desc *d, const epi_inputs *in, void *stream, int *fast_ok, char *err)
{
    int rc = epi_ekf_validate(d, err);
    if (rc != EPI_OK) return rc;
    if (!in || !fast_ok || !in->Ps_init || !in->Ps_final || !in->Q || !in->s_init || !in->s_final) { set_err(err, "NULL argument"); return EPI_ERR_BAD_ARG; }
    const ModelInfo &mi = MODEL_TABLE[d->model];
    *fast_ok = 0;
    if (!mi.generic || d->q_mode != 0) return EPI_OK;   // NewCase models never symmetrise; Q(:,:,k): dense kernels only
    KArgs ka{};
    ka.B = d->B;
    ka.Ps_init = mi.flipped ? in->Ps_final : in->Ps_init;
    ka.Ps_final = mi.flipped ? in->Ps_init : in->Ps_final;
    ka.s_init = mi.flipped ? in->s_final : in->s_init;
    ka.Q = in->Q;
    int *flag = nullptr;
    hipError_t e = hipMalloc((void **)&flag, sizeof(int));
    if (e != hipSuccess) return hip_fail(err, e, "hipMalloc");
    hipStream_t st = (hipStream_t)stream;
    int host_flag = 1;
    if ((e = hipMemsetAsync(flag, 0, sizeof(int), st)) == hipSuccess) {
        if (mi.m == 3) hipLaunchKernelGGL((ekf_precheck<3>), dim3((d->B + 255) / 256), dim3(256), 0, st, ka, flag, 0);
        else hipLaunchKernelGGL((ekf_precheck<6>), dim3((d->B + 255) / 256), dim3(256), 0, st, ka, flag, 0);
        if ((e = hipGetLastError()) == hipSuccess)
            e = hipMemcpyAsync(&host_flag, flag, sizeof(int), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    (void)hipFree(flag);
    if (e != hipSuccess) return hip_fail(err, e, "precheck");
    *fast_ok = host_flag ? 0 : 1;
    return EPI_OK;
}

// ---------------------------------------------------------------------------
// host-pointer entry points: pooled contexts
// ---------------------------------------------------------------------------
// A context owns what a host call needs on one device -- a stream, a device arena and a pinned staging buffer -- and
// outlives the call (idle contexts wait in a per-device pool), so that the 250 calls per region of the unchanged
// reference caller (TrainPredictPrescribeNPI.m:421-460) do not pay 50 hipMalloc/hipFree and 50 synchronous copies each.
}   // extern "C"
#include "host_stage.hpp"
namespace epi {
// ekf_precheck's rules on HOST arrays ([rows][pitch] doubles, columns [lo, lo + n)): may these chains take the packed
// kernels?  Ps_init and Ps_final bit-wise symmetric (values and NaN pattern), Q_w diagonal, s_init / Ps_init / diag(Q_w)
// finite.  The host entry points have the arrays in host memory, so the check costs no device round trip.
static bool host_precheck(int m, bool flipped, const epi_inputs *in, size_t pitch, size_t lo, size_t n)
{
    const double *Pi = flipped ? in->Ps_final : in->Ps_init, *Pf = flipped ? in->Ps_init : in->Ps_final;
    const double *si = flipped ? in->s_final : in->s_init, *Q = in->Q;
    auto nonfinite = [](double v) { return !(v - v == 0.0); };
    auto same = [](double a, double b) { return a == b || (a != a && b != b); };
    for (int j = 0; j < m; j++)
        for (int i = 0; i <= j; i++) {
            const double *pu = Pi + (size_t)(i + m * j) * pitch + lo, *pl = Pi + (size_t)(j + m * i) * pitch + lo;
            const double *fu = Pf + (size_t)(i + m * j) * pitch + lo, *fl = Pf + (size_t)(j + m * i) * pitch + lo;
            const double *qu = Q + (size_t)(i + m * j) * pitch + lo, *ql = Q + (size_t)(j + m * i) * pitch + lo;
            for (size_t c = 0; c < n; c++) {
                if (nonfinite(pu[c])) return false;
                if (i == j) { if (nonfinite(qu[c])) return false; continue; }
                if (!same(pu[c], pl[c]) || !same(fu[c], fl[c]) || !(qu[c] == 0.0) || !(ql[c] == 0.0)) return false;
            }
        }
    for (int i = 0; i < m; i++)
        for (size_t c = 0; c < n; c++)
            if (nonfinite(si[(size_t)i * pitch + lo + c])) return false;
    return true;
}

// chains [lo, lo + n) of a host call on one context.  Per-chain arrays are [rows][B] in the caller's memory: the block is a
// strided piece of each row.
static int run_host_block(HostCtx *cx, const epi_batch_desc *d0, const epi_inputs *in, const epi_outputs *out, int lo, int n, char *err)
{
    if (n <= 0) return EPI_OK;
    epi_batch_desc d = *d0;
    const size_t Bfull = (size_t)d0->B;
    d.B = n;
    // A host call returns what the dense evaluation returns, overflowed chains included (exact_nonfinite) -- but the call ends
    // with a synchronising download anyway, so the per-chain status words come back with it and the dense second pass is
    // enqueued only when one of them has bit 0 set: the common call pays nothing for it (the device-side variant costs five
    // launches that return at once, ~40 us of a 1.5 ms one-chain call).
    d.exact_nonfinite = -1;
    const bool id_x = !in->x_series, id_u = !in->u_series;      // identity series: one series per chain, sliced with the chains
    if (id_x) d.Sx = n;
    if (id_u) d.Su = n;
    const ModelInfo &mi = MODEL_TABLE[d.model];
    const int m = mi.m, mm = m * m;
    const size_t T = (size_t)d.T;
    HostIO io;
    epi_inputs din{};
    epi_outputs dout{};
    // inputs
    const size_t o_xs = in->x_series ? io.add_in(in->x_series, 1, 4, Bfull, lo, n) : 0;
    const size_t o_us = in->u_series ? io.add_in(in->u_series, 1, 4, Bfull, lo, n) : 0;
    const size_t o_x = id_x ? io.add_in(in->x, T, 8, Bfull, lo, n) : io.add_in(in->x, T, 8, d0->Sx, 0, d0->Sx);
    const size_t o_u = id_u ? io.add_in(in->u, T * d.n_npi, 8, Bfull, lo, n) : io.add_in(in->u, T * d.n_npi, 8, d0->Su, 0, d0->Su);
    size_t o_rs = 0, o_rc = 0;
    if (d.r_mode == 1) o_rs = id_x ? io.add_in(in->R_series, T, 8, Bfull, lo, n) : io.add_in(in->R_series, T, 8, d0->Sx, 0, d0->Sx);
    else o_rc = io.add_in(in->R_scalar, 1, 8, Bfull, lo, n);
    const size_t o_prm = io.add_in(in->prm, EPI_PRM_COUNT, 8, Bfull, lo, n);
    const size_t o_si = io.add_in(in->s_init, m, 8, Bfull, lo, n), o_pi = io.add_in(in->Ps_init, mm, 8, Bfull, lo, n);
    const size_t o_sf = io.add_in(in->s_final, m, 8, Bfull, lo, n), o_pf = io.add_in(in->Ps_final, mm, 8, Bfull, lo, n);
    const size_t o_q = io.add_in(in->Q, (d.q_mode ? T : (size_t)1) * mm, 8, Bfull, lo, n);
    if (!io.inputs_present()) { set_err(err, "NULL input array"); return EPI_ERR_BAD_ARG; }
    // the caller's arrays are in host memory: decide here which kernels run (what epi_ekf_precheck_device answers for
    // device arrays), so that a host call enqueues one variant only and gets the overlapped launch
    if (d.path_hint == 0 && mi.generic && d.q_mode == 0)
        d.path_hint = host_precheck(m, mi.flipped != 0, in, Bfull, (size_t)lo, (size_t)n) ? 1 : 2;
    // outputs
    struct O { uint32_t bit; double *epi_outputs::*arr; size_t rows; };
    const size_t rU = T * d.n_npi, rS = T * m, rP = T * mm, r1 = T;
    const O olist[] = {{EPI_OUT_U_OPT, &epi_outputs::u_opt, rU}, {EPI_OUT_U_OPT_SMOOTH, &epi_outputs::u_opt_smooth, rU},
                       {EPI_OUT_S_MINUS, &epi_outputs::S_MINUS, rS}, {EPI_OUT_S_PLUS, &epi_outputs::S_PLUS, rS},
                       {EPI_OUT_S_SMOOTH, &epi_outputs::S_SMOOTH, rS}, {EPI_OUT_P_MINUS, &epi_outputs::P_MINUS, rP},
                       {EPI_OUT_P_PLUS, &epi_outputs::P_PLUS, rP}, {EPI_OUT_P_SMOOTH, &epi_outputs::P_SMOOTH, rP},
                       {EPI_OUT_K_GAIN, &epi_outputs::K_GAIN, rS}, {EPI_OUT_INNOVATIONS, &epi_outputs::innovations, r1},
                       {EPI_OUT_RHO, &epi_outputs::rho, r1}};
    std::vector<size_t> o_out;
    for (auto &o : olist)
        o_out.push_back(((d.out_mask & o.bit) && out->*o.arr) ? io.add_out(out->*o.arr, o.rows, 8, Bfull, lo, n) : HostIO::kAbsent);
    const size_t o_rank = out->pinv_rank ? io.add_out(out->pinv_rank, T, 4, Bfull, lo, n) : HostIO::kAbsent;
    // does this call run the smoother (which is where an overflowed chain is recognised)?
    const uint32_t smooth_bits = EPI_OUT_S_SMOOTH | EPI_OUT_P_SMOOTH | (mi.generic ? (uint32_t)EPI_OUT_U_OPT_SMOOTH : 0u);
    bool smooths = out->pinv_rank != nullptr || out->status != nullptr;
    for (auto &o : olist) smooths = smooths || ((d.out_mask & o.bit & smooth_bits) && out->*o.arr);
    const bool watch = smooths && mi.generic && d.q_mode == 0 && d.storage == 0 && d.phase == 0;
    std::vector<int32_t> own_status;
    int32_t *hstat = out->status ? out->status + lo : nullptr;
    size_t o_stat = HostIO::kAbsent;
    if (out->status) o_stat = io.add_out(out->status, 1, 4, Bfull, lo, n);
    else if (watch) { own_status.assign((size_t)n, 0); hstat = own_status.data(); o_stat = io.add_out(own_status.data(), 1, 4, (size_t)n, 0, n); }
    epi_batch_desc dmax = d;
    dmax.exact_nonfinite = watch ? 1 : -1;           // the workspace is sized for the second pass
    const size_t wsb = epi_ekf_workspace_bytes(&dmax);
    const size_t o_ws = io.reserve(wsb);
    // the device-side view of the call for the arena at `base`
    auto bind = [&](char *base) {
        din.x_series = in->x_series ? (const int32_t *)(base + o_xs) : nullptr;
        din.u_series = in->u_series ? (const int32_t *)(base + o_us) : nullptr;
        din.x = (const double *)(base + o_x); din.u = (const double *)(base + o_u);
        din.R_series = d.r_mode == 1 ? (const double *)(base + o_rs) : nullptr;
        din.R_scalar = d.r_mode == 1 ? nullptr : (const double *)(base + o_rc);
        din.prm = (const double *)(base + o_prm);
        din.s_init = (const double *)(base + o_si); din.Ps_init = (const double *)(base + o_pi);
        din.s_final = (const double *)(base + o_sf); din.Ps_final = (const double *)(base + o_pf);
        din.Q = (const double *)(base + o_q);
        size_t k = 0;
        for (auto &o : olist) dout.*o.arr = HostIO::at<double>(base, o_out[k++]);
        dout.pinv_rank = HostIO::at<int32_t>(base, o_rank);
        dout.status = HostIO::at<int32_t>(base, o_stat);
    };
    int rc = run_call(cx, io, d0->placement_tries, lo == 0 ? out->placement : nullptr, err, [&](char *base, hipStream_t st) {
        bind(base);
        return epi_ekf_run_device(&d, &din, &dout, wsb ? base + o_ws : nullptr, wsb, st, err);
    });
    if (rc != EPI_OK || !watch) return rc;
    bool any = false;
    for (int c = 0; c < n; c++) any = any || (hstat[c] & 1);
    if (any) {                                        // rare: a covariance overflowed -- the dense second pass, then the outputs again
        char *base = cx->arena;
        bind(base);
        rc = epi_ekf_run_device(&dmax, &din, &dout, wsb ? base + o_ws : nullptr, wsb, cx->stream, err);
        if (rc != EPI_OK) { (void)hipStreamSynchronize(cx->stream); return rc; }
        const hipError_t e = io.download(cx, base);
        if (e != hipSuccess) return hip_fail(err, e, "kernel execution / download (dense second pass)");
    }
    return EPI_OK;
}
static int host_args_ok(const epi_batch_desc *d, const epi_inputs *in, const epi_outputs *out, char *err)
{
    int rc = epi_ekf_validate(d, err);
    if (rc != EPI_OK) return rc;
    if (!in || !out) { set_err(err, "NULL inputs/outputs"); return EPI_ERR_BAD_ARG; }
    if (lane_block_of(d) != d->B) { set_err(err, "the host entry points take the classic layout only (lane_block = 0)"); return EPI_ERR_UNSUPPORTED; }
    if (d->storage != 0) { set_err(err, "the host entry points return fp64 arrays (storage = 0)"); return EPI_ERR_UNSUPPORTED; }
    if (!in->x_series && d->Sx != d->B) { set_err(err, "identity x_series needs Sx == B"); return EPI_ERR_BAD_ARG; }
    if (!in->u_series && d->Su != d->B) { set_err(err, "identity u_series needs Su == B"); return EPI_ERR_BAD_ARG; }
    return EPI_OK;
}

// One worker thread per device for the *_multi entry points (created on first use, parked on a condition variable between
// calls, joined by epi_host_pool_release): a call hands every block of chains / regions to the worker of its device and
// waits; blocks that name the same device run one after the other.
struct DevWorker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::function<void()>> q;
    bool stop = false;
    void loop()
    {
        for (;;) {
            std::function<void()> job;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || !q.empty(); });
                if (q.empty()) return;
                job = std::move(q.front());
                q.pop_front();
            }
            job();
        }
    }
};
static std::mutex g_worker_mu;
static DevWorker *g_workers[kMaxDevices];
static void worker_submit(int device, std::function<void()> job)
{
    DevWorker *w;
    {
        std::lock_guard<std::mutex> lk(g_worker_mu);
        if (!g_workers[device]) {
            g_workers[device] = new DevWorker();
            g_workers[device]->th = std::thread([p = g_workers[device]] { p->loop(); });
        }
        w = g_workers[device];
    }
    { std::lock_guard<std::mutex> lk(w->mu); w->q.push_back(std::move(job)); }
    w->cv.notify_one();
}
static void workers_release_all()
{
    for (int dev = 0; dev < kMaxDevices; dev++) {
        DevWorker *w;
        { std::lock_guard<std::mutex> lk(g_worker_mu); w = g_workers[dev]; g_workers[dev] = nullptr; }
        if (!w) continue;
        { std::lock_guard<std::mutex> lk(w->mu); w->stop = true; }
        w->cv.notify_one();
        w->th.join();
        delete w;
    }
}
// runs job(r) for r = 0 .. n-1 on the workers of devices dev_of(r) and waits for all of them
static void run_on_devices(int n, const std::function<int(int)> &dev_of, const std::function<void(int)> &job)
{
    if (n == 1) { job(0); return; }          // one block: the calling thread does it (and keeps its current device: with_ctx)
    std::mutex mu;
    std::condition_variable cv;
    int left = n;
    for (int r = 0; r < n; r++)
        worker_submit(dev_of(r), [&, r] {
            job(r);
            std::lock_guard<std::mutex> lk(mu);
            if (--left == 0) cv.notify_one();
        });
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return left == 0; });
}
}   // namespace epi
// ---- the launches of svr.hpp (epi_svr_run_device) ----
template <int NR, bool GAU>
static hipError_t sv_launch_items(const SvArgs &g, unsigned blocks, size_t shm, hipStream_t st)
{
    hipError_t e;
    if (shm > 64u * 1024u &&            // above the default dynamic-LDS limit
        (e = hipFuncSetAttribute((const void *)svr_items<NR, GAU>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm)) != hipSuccess)
        return e;
    hipLaunchKernelGGL((svr_items<NR, GAU>), dim3(blocks), dim3(kSvThreads), shm, st, g);
    return hipGetLastError();
}

// the rows-per-lane instantiation for the launch's largest row count
template <bool GAU>
static hipError_t sv_dispatch(const SvArgs &g, int nmax, unsigned blocks, size_t shm, hipStream_t st)
{
    if (nmax <= kSvThreads) return sv_launch_items<1, GAU>(g, blocks, shm, st);
    if (nmax <= 2 * kSvThreads) return sv_launch_items<2, GAU>(g, blocks, shm, st);
    return sv_launch_items<4, GAU>(g, blocks, shm, st);
}

extern "C" {

int epi_ekf_run_host(const epi_batch_desc *d, const epi_inputs *in, const epi_outputs *out, int device, char *err)
{
    int rc = host_args_ok(d, in, out, err);
    if (rc != EPI_OK) return rc;
    return with_ctx(device, err, [&](HostCtx *cx) { return run_host_block(cx, d, in, out, 0, d->B, err); });
}

static int multi_devices_ok(int n_devices, const int *device_ids, char *err)
{
    if (n_devices < 1 || n_devices > kMaxDevices) { set_err(err, "n_devices must be 1..64"); return EPI_ERR_BAD_ARG; }
    for (int r = 0; r < n_devices; r++) {
        const int dev = device_ids ? device_ids[r] : r;
        if (dev < 0 || dev >= kMaxDevices) { set_err(err, "device id out of range 0..63"); return EPI_ERR_BAD_ARG; }
    }
    return EPI_OK;
}

int epi_ekf_run_host_multi(const epi_batch_desc *d, const epi_inputs *in, const epi_outputs *out, int n_devices,
                           const int *device_ids, char *err)
{
    int rc = host_args_ok(d, in, out, err);
    if (rc != EPI_OK) return rc;
    if ((rc = multi_devices_ok(n_devices, device_ids, err)) != EPI_OK) return rc;
    const int per = (d->B + n_devices - 1) / n_devices;
    std::vector<int> rcs((size_t)n_devices, EPI_OK);
    std::vector<std::vector<char>> errs((size_t)n_devices, std::vector<char>(256, 0));
    auto dev_of = [&](int r) { return device_ids ? device_ids[r] : r; };
    run_on_devices(n_devices, dev_of, [&](int r) {
        const int lo = r * per < d->B ? r * per : d->B, n = (lo + per <= d->B ? per : d->B - lo);
        if (n <= 0) return;
        char *er = errs[(size_t)r].data();
        rcs[(size_t)r] = with_ctx(dev_of(r), er, [&](HostCtx *cx) { return run_host_block(cx, d, in, out, lo, n, er); });
    });
    for (int r = 0; r < n_devices; r++)
        if (rcs[(size_t)r] != EPI_OK) { set_err(err, errs[(size_t)r].data()); return rcs[(size_t)r]; }
    return EPI_OK;
}

// regions [r0, r0 + Rd) of the sweep on one context (see epi_sweep_prescribe_host)
static int prescribe_block(HostCtx *cx, const epi_prescribe_desc *pd, const epi_prescribe_inputs *in, const epi_prescribe_outputs *out,
                           int r0, int Rd, char *err)
{
    if (Rd <= 0) return EPI_OK;
    const size_t R = (size_t)pd->R, P = (size_t)pd->P, T = (size_t)pd->T, n = (size_t)pd->n_npi;
    const size_t Bd = (size_t)Rd * P, Bfull = R * P, c0 = (size_t)r0 * P;
    const bool extras = pd->out_mask != 0;
    // the filter's descriptor for this block: chain c = region * P + ll reads series `region`
    epi_batch_desc d{};
    d.abi_version = EPIEKF_ABI_VERSION; d.model = EPI_MODEL_SIA6; d.B = (int32_t)Bd; d.T = pd->T; d.Sx = Rd; d.Su = Rd;
    d.n_npi = pd->n_npi; d.L = pd->L; d.order = pd->order; d.obs_type = pd->obs_type; d.r_mode = 1; d.q_mode = 0;
    d.out_mask = pd->out_mask | EPI_OUT_U_OPT_SMOOTH | (out->S_opt ? EPI_OUT_S_SMOOTH : 0u);
    d.shape = pd->shape; d.time_pipe = pd->time_pipe;
    d.exact_nonfinite = 1;
    {
        epi_inputs hin{};
        hin.s_init = in->s_init; hin.Ps_init = in->Ps_init; hin.s_final = in->s_final; hin.Ps_final = in->Ps_final; hin.Q = in->Q;
        d.path_hint = host_precheck(6, false, &hin, R, (size_t)r0, (size_t)Rd) ? 1 : 2;
    }
    // per-chain extras come back in the classic layout; without them the filter writes the layout it runs fastest in
    d.lane_block = extras ? 0 : epi_ekf_preferred_lane_block(&d);
    if (d.lane_block >= d.B) d.lane_block = 0;
    int rc = epi_ekf_validate(&d, err);
    if (rc != EPI_OK) return rc;
    const size_t blk = d.lane_block ? (size_t)d.lane_block : Bd, nblk = (Bd + blk - 1) / blk, Bp = nblk * blk;

    HostIO io;
    const size_t o_x = io.add_in(in->x, T, 8, R, r0, Rd), o_u = io.add_in(in->u, T * n, 8, R, r0, Rd);
    const size_t o_rs = io.add_in(in->R_series, T, 8, R, r0, Rd), o_eps = io.add_in(in->eps, 1, 8, P, 0, P);
    // the per-region rows, contiguous and in the order of the per-chain rows sweep_expand writes
    io.off = (io.off + 255) & ~(size_t)255;
    io.align = 8;
    struct Row { const double *host; size_t rows; };
    const Row rows[] = {{in->prm, EPI_PRM_COUNT}, {in->s_init, 6}, {in->Ps_init, 36}, {in->s_final, 6}, {in->Ps_final, 36},
                        {in->Q, 36}, {in->sp, EPI_SIM_PRM_COUNT}, {in->J0_prefix, 1}, {in->J1_prefix, 1}};
    size_t o_reg = 0, nrows = 0;
    for (auto &rw : rows) {
        const size_t o = io.add_in(rw.host, rw.rows, 8, R, r0, Rd);
        if (nrows == 0) o_reg = o;
        nrows += rw.rows;
    }
    io.align = 256;
    io.off = (io.off + 255) & ~(size_t)255; io.in_bytes = io.off;
    if (!io.inputs_present()) { set_err(err, "NULL input array"); return EPI_ERR_BAD_ARG; }
    // outputs, in one run of the arena so that a small call downloads them with one copy
    const size_t o_j0 = io.add_out(out->J0, 1, 8, Bfull, c0, Bd), o_j1 = io.add_out(out->J1, 1, 8, Bfull, c0, Bd);
    const size_t o_of = io.add_out(out->on_front, 1, 4, Bfull, c0, Bd), o_io = io.add_out(out->i_opt, 1, 4, R, r0, Rd);
    const size_t o_uo = io.add_out(out->u_opt, T * n, 8, R, r0, Rd), o_so = io.add_out(out->S_opt, T * 6, 8, R, r0, Rd);
    struct O { uint32_t bit; double *epi_outputs::*arr; size_t rows; };
    const epi_outputs &ex = out->extras;
    const O olist[] = {{EPI_OUT_U_OPT, &epi_outputs::u_opt, T * n}, {EPI_OUT_U_OPT_SMOOTH, &epi_outputs::u_opt_smooth, T * n},
                       {EPI_OUT_S_MINUS, &epi_outputs::S_MINUS, T * 6}, {EPI_OUT_S_PLUS, &epi_outputs::S_PLUS, T * 6},
                       {EPI_OUT_S_SMOOTH, &epi_outputs::S_SMOOTH, T * 6}, {EPI_OUT_P_MINUS, &epi_outputs::P_MINUS, T * 36},
                       {EPI_OUT_P_PLUS, &epi_outputs::P_PLUS, T * 36}, {EPI_OUT_P_SMOOTH, &epi_outputs::P_SMOOTH, T * 36},
                       {EPI_OUT_K_GAIN, &epi_outputs::K_GAIN, T * 6}, {EPI_OUT_INNOVATIONS, &epi_outputs::innovations, T},
                       {EPI_OUT_RHO, &epi_outputs::rho, T}};
    std::vector<size_t> o_ex;
    for (auto &o : olist) {
        if ((pd->out_mask & o.bit) && !(ex.*o.arr)) { set_err(err, "extras: output selected but NULL"); return EPI_ERR_BAD_ARG; }
        o_ex.push_back((pd->out_mask & o.bit) ? io.add_out(ex.*o.arr, o.rows, 8, Bfull, c0, Bd) : HostIO::kAbsent);
    }
    // device-only: expanded per-chain rows, the series map, filter outputs that do not leave the device, workspace
    const size_t o_chain = io.reserve(nrows * Bd * 8), o_ser = io.reserve(Bd * 4);
    const size_t o_uos = (pd->out_mask & EPI_OUT_U_OPT_SMOOTH) ? HostIO::kAbsent : io.reserve(T * n * Bp * 8);
    const size_t o_ss = ((pd->out_mask & EPI_OUT_S_SMOOTH) || !out->S_opt) ? HostIO::kAbsent : io.reserve(T * 6 * Bp * 8);
    const size_t wsb = epi_ekf_workspace_bytes(&d);
    const size_t o_ws = io.reserve(wsb);
    return run_call(cx, io, pd->placement_tries, r0 == 0 ? out->placement : nullptr, err, [&](char *base, hipStream_t st) -> int {
        double *chain = (double *)(base + o_chain);
        int32_t *series = (int32_t *)(base + o_ser);
        hipLaunchKernelGGL(sweep_expand, dim3((unsigned)((Bd + 255) / 256), 8), dim3(256), 0, st, (int)nrows, Rd, (int)P,
                           (int)EPI_PRM_EPSILON, (const double *)(base + o_reg), (const double *)(base + o_eps), chain, series);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(err, e, "sweep_expand launch");
        epi_inputs din{};
        din.x_series = series; din.u_series = series;
        din.x = (const double *)(base + o_x); din.u = (const double *)(base + o_u); din.R_series = (const double *)(base + o_rs);
        size_t row = 0;
        auto take = [&](size_t nr) { const double *p = chain + row * Bd; row += nr; return p; };
        din.prm = take(EPI_PRM_COUNT); din.s_init = take(6); din.Ps_init = take(36); din.s_final = take(6); din.Ps_final = take(36);
        din.Q = take(36);
        const double *sp = take(EPI_SIM_PRM_COUNT), *j0p = take(1), *j1p = take(1);
        epi_outputs dd{};
        size_t k = 0;
        for (auto &o : olist) dd.*o.arr = HostIO::at<double>(base, o_ex[k++]);
        if (!dd.u_opt_smooth) dd.u_opt_smooth = (double *)(base + o_uos);
        if (!dd.S_SMOOTH && out->S_opt) dd.S_SMOOTH = (double *)(base + o_ss);
        epi_sweep_desc sd{};
        sd.abi_version = EPIEKF_ABI_VERSION; sd.R = Rd; sd.P = (int32_t)P; sd.t_hist = pd->t_hist;
        const int r = epi_sweep_run_device(&d, &din, &dd, wsb ? base + o_ws : nullptr, wsb, &sd, sp, j0p, j1p, (double *)(base + o_j0),
                                           (double *)(base + o_j1), (int32_t *)(base + o_of), (int32_t *)(base + o_io), st, err);
        if (r != EPI_OK) return r;
        struct G { double *host; const double *src; size_t off; int rows; };
        const G gs[] = {{out->u_opt, dd.u_opt_smooth, o_uo, (int)n}, {out->S_opt, dd.S_SMOOTH, o_so, 6}};
        for (auto &g : gs) {
            if (!g.host) continue;
            const size_t cnt = T * (size_t)g.rows * (size_t)Rd;
            hipLaunchKernelGGL(sweep_gather_opt, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, (int)T, g.rows, Rd, (int)P,
                               (int)blk, (int)nblk, (const int32_t *)(base + o_io), g.src, (double *)(base + g.off));
            if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "sweep_gather_opt launch");
        }
        return EPI_OK;
    });
}

int epi_sweep_prescribe_host(const epi_prescribe_desc *d, const epi_prescribe_inputs *in, const epi_prescribe_outputs *out,
                             int n_devices, const int *device_ids, char *err)
{
    if (!d || !in || !out || d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "bad prescribe descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->R < 1 || d->P < 1 || (int64_t)d->R * d->P > ((int64_t)1 << 23)) { set_err(err, "R, P must be >= 1 and R * P <= 2^23"); return EPI_ERR_BAD_ARG; }
    if (d->P > 8192) { set_err(err, "more than 8192 points per region"); return EPI_ERR_UNSUPPORTED; }
    if (d->t_hist < 1 || d->t_hist >= d->T) { set_err(err, "t_hist must leave at least one horizon day: 1 <= t_hist < T"); return EPI_ERR_BAD_ARG; }
    if (d->out_mask & ~(uint32_t)EPI_OUT_ALL) { set_err(err, "unknown bits in out_mask"); return EPI_ERR_BAD_ARG; }
    if (d->placement_tries < 0 || d->placement_tries > EPI_PLACEMENT_MAX_TRIES) { set_err(err, "placement_tries must be 0 .. EPI_PLACEMENT_MAX_TRIES"); return EPI_ERR_BAD_ARG; }
    int rc = multi_devices_ok(n_devices, device_ids, err);
    if (rc != EPI_OK) return rc;
    const int per = (d->R + n_devices - 1) / n_devices;
    std::vector<int> rcs((size_t)n_devices, EPI_OK);
    std::vector<std::vector<char>> errs((size_t)n_devices, std::vector<char>(256, 0));
    auto dev_of = [&](int r) { return device_ids ? device_ids[r] : r; };
    run_on_devices(n_devices, dev_of, [&](int r) {
        const int lo = r * per < d->R ? r * per : d->R, n = (lo + per <= d->R ? per : d->R - lo);
        if (n <= 0) return;
        char *er = errs[(size_t)r].data();
        rcs[(size_t)r] = with_ctx(dev_of(r), er, [&](HostCtx *cx) { return prescribe_block(cx, d, in, out, lo, n, er); });
    });
    for (int r = 0; r < n_devices; r++)
        if (rcs[(size_t)r] != EPI_OK) { set_err(err, errs[(size_t)r].data()); return rcs[(size_t)r]; }
    return EPI_OK;
}

void epi_host_pool_release(void)
{
    workers_release_all();
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (HostCtx *c : g_pool) delete c;
        g_pool.clear();
    }
    helpers_release_all();
}

int epi_calib_copy_f64_device(const double *src, double *dst, size_t n, void *stream, char *err)
{
    if (!src || !dst || n == 0) { set_err(err, "bad calibration arguments"); return EPI_ERR_BAD_ARG; }
    hipLaunchKernelGGL(calib_copy_f64, dim3(256 * 8), dim3(256), 0, (hipStream_t)stream, src, dst, n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(err, e, "calib_copy_f64 launch");
    return EPI_OK;
}

// the seeded calls' common checks: a valid noise descriptor and no z beside it
static int noise_key(const epi_noise_desc *noise, const void *z, NoiseKey *nk, char *err)
{
    int rc = epi_noise_validate(noise, err);
    if (rc != EPI_OK) return rc;
    if (z) { set_err(err, "a seeded call takes no z: the draws have one source"); return EPI_ERR_BAD_ARG; }
    nk->seed_lo = noise->seed_lo; nk->seed_hi = noise->seed_hi; nk->stream = noise->stream;
    return EPI_OK;
}

// nk: NULL (the draws are read from z) or the seeded call's key
static int sialpha_launch(const epi_sim_desc *d, const int32_t *u_series, const double *u, const double *sp,
                          const double *z, const NoiseKey *nk, double *s, double *i, double *alpha, double *J0, double *J1,
                          const double *J0_prefix, const double *J1_prefix, void *stream, char *err)
{
    if (!d || d->abi_version != EPIEKF_ABI_VERSION || d->B < 1 || d->K < 1 || d->Su < 1 || d->n_npi < 1 ||
        d->n_npi > EPI_MAX_NPI || !u || !sp || (!nk && d->noise && !z) || (!u_series && d->Su != d->B) || d->prefix_days < 0 ||
        (d->prefix_days > 0 && (!J0_prefix || !J1_prefix))) {
        set_err(err, "bad simulator descriptor"); return EPI_ERR_BAD_ARG;
    }
    const int blocks = (d->B + 255) / 256;
    if (nk)
        hipLaunchKernelGGL(sialpha_sim_seeded, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *d, *nk, u_series, u, sp, s, i, alpha,
                           J0, J1, J0_prefix, J1_prefix);
    else
        hipLaunchKernelGGL(sialpha_sim, dim3(blocks), dim3(256), 0, (hipStream_t)stream, *d, u_series, u, sp, z, s, i, alpha,
                           J0, J1, J0_prefix, J1_prefix, (const int32_t *)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(err, e, "sialpha_sim launch");
    return EPI_OK;
}

int epi_sialpha_sim_device(const epi_sim_desc *d, const int32_t *u_series, const double *u, const double *sp,
                           const double *z, double *s, double *i, double *alpha, double *J0, double *J1,
                           void *stream, char *err)
{
    if (d && d->prefix_days != 0) { set_err(err, "prefix_days needs epi_sialpha_score_device"); return EPI_ERR_BAD_ARG; }
    return sialpha_launch(d, u_series, u, sp, z, nullptr, s, i, alpha, J0, J1, nullptr, nullptr, stream, err);
}

int epi_sialpha_sim_device_seeded(const epi_sim_desc *d, const epi_noise_desc *noise, const int32_t *u_series, const double *u,
                                  const double *sp, const double *z, double *s, double *i, double *alpha, double *J0, double *J1,
                                  void *stream, char *err)
{
    NoiseKey nk;
    int rc = noise_key(noise, z, &nk, err);
    if (rc != EPI_OK) return rc;
    if (d && d->prefix_days != 0) { set_err(err, "prefix_days needs epi_sialpha_score_device_seeded"); return EPI_ERR_BAD_ARG; }
    return sialpha_launch(d, u_series, u, sp, nullptr, &nk, s, i, alpha, J0, J1, nullptr, nullptr, stream, err);
}

int epi_sialpha_score_device(const epi_sim_desc *d, const int32_t *u_series, const double *u, const double *sp,
                             const double *z, const double *J0_prefix, const double *J1_prefix, double *s, double *i,
                             double *alpha, double *J0, double *J1, void *stream, char *err)
{
    return sialpha_launch(d, u_series, u, sp, z, nullptr, s, i, alpha, J0, J1, J0_prefix, J1_prefix, stream, err);
}

int epi_sialpha_score_device_seeded(const epi_sim_desc *d, const epi_noise_desc *noise, const int32_t *u_series, const double *u,
                                    const double *sp, const double *z, const double *J0_prefix, const double *J1_prefix, double *s,
                                    double *i, double *alpha, double *J0, double *J1, void *stream, char *err)
{
    NoiseKey nk;
    int rc = noise_key(noise, z, &nk, err);
    if (rc != EPI_OK) return rc;
    return sialpha_launch(d, u_series, u, sp, nullptr, &nk, s, i, alpha, J0, J1, J0_prefix, J1_prefix, stream, err);
}

static int random_npi_mc_launch(const epi_mc_desc *d, const double *sp, const double *u_min, const double *z, const NoiseKey *nk,
                                const double *J0_prefix, const double *J1_prefix, double *u_out, double *J0, double *J1,
                                void *stream, char *err)
{
    if (!d || d->abi_version != EPIEKF_ABI_VERSION || d->R < 1 || d->n_scen < 1 || d->K < 1 || d->n_npi < 1 ||
        d->n_npi > EPI_MAX_NPI || !sp || !u_min || !J0 || !J1 || (!nk && d->noise && !z) || d->prefix_days < 0 ||
        (d->prefix_days > 0 && (!J0_prefix || !J1_prefix)) || (int64_t)d->R * d->n_scen > (int64_t)1 << 30) {
        set_err(err, "bad Monte-Carlo scenario descriptor"); return EPI_ERR_BAD_ARG;
    }
    const int B = d->R * d->n_scen;
    if (nk)
        hipLaunchKernelGGL(random_npi_mc_seeded, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, *d, *nk, sp, u_min,
                           J0_prefix, J1_prefix, u_out, J0, J1);
    else
        hipLaunchKernelGGL(random_npi_mc, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, *d, sp, u_min, z,
                           J0_prefix, J1_prefix, u_out, J0, J1);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(err, e, "random_npi_mc launch");
    return EPI_OK;
}

int epi_random_npi_mc_device(const epi_mc_desc *d, const double *sp, const double *u_min, const double *z,
                             const double *J0_prefix, const double *J1_prefix, double *u_out, double *J0, double *J1,
                             void *stream, char *err)
{
    return random_npi_mc_launch(d, sp, u_min, z, nullptr, J0_prefix, J1_prefix, u_out, J0, J1, stream, err);
}

int epi_random_npi_mc_device_seeded(const epi_mc_desc *d, const epi_noise_desc *noise, const double *sp, const double *u_min,
                                    const double *z, const double *J0_prefix, const double *J1_prefix, double *u_out, double *J0,
                                    double *J1, void *stream, char *err)
{
    NoiseKey nk;
    int rc = noise_key(noise, z, &nk, err);
    if (rc != EPI_OK) return rc;
    return random_npi_mc_launch(d, sp, u_min, nullptr, &nk, J0_prefix, J1_prefix, u_out, J0, J1, stream, err);
}

int epi_pareto_front_device(int32_t R, int32_t P, const double *J0, const double *J1, int32_t *on_front,
                            int32_t *i_opt, void *stream, char *err)
{
    if (R < 1 || P < 1 || !J0 || !J1 || (!on_front && !i_opt)) { set_err(err, "bad Pareto-front arguments"); return EPI_ERR_BAD_ARG; }
    if (P > 8192) { set_err(err, "more than 8192 points per region"); return EPI_ERR_UNSUPPORTED; }
    const size_t shmem = (size_t)2 * P * sizeof(double);
    if (shmem > 64u * 1024u) {
        hipError_t e = hipFuncSetAttribute((const void *)pareto_front, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
        if (e != hipSuccess) return hip_fail(err, e, "hipFuncSetAttribute");
    }
    // one 256-lane workgroup per region, in slices: a launch's thread count is a 32-bit number in the HIP runtime and wraps
    // silently beyond it (2^24 regions and more in one launch)
    constexpr int64_t kSlice = (int64_t)1 << 22;
    for (int64_t r0 = 0; r0 < R; r0 += kSlice) {
        const int64_t nr = R - r0 < kSlice ? R - r0 : kSlice;
        hipLaunchKernelGGL(pareto_front, dim3((unsigned)nr), dim3(256), shmem, (hipStream_t)stream, P, J0 + r0 * P, J1 + r0 * P,
                           on_front ? on_front + r0 * P : nullptr, i_opt ? i_opt + r0 : nullptr, (const int32_t *)nullptr);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(err, e, "pareto_front launch");
    }
    return EPI_OK;
}

int epi_npi_cost_device(int32_t B, int32_t T, int32_t n_npi, int32_t Su, int32_t weights_per_day,
                        const int32_t *u_series, const double *newcases, const double *inputs, const double *weights,
                        double *J0, double *J1, void *stream, char *err)
{
    if (B < 1 || T < 1 || n_npi < 1 || Su < 1 || !newcases || !inputs || !weights || !J0 || !J1 || (!u_series && Su != B)) {
        set_err(err, "bad NPICost arguments"); return EPI_ERR_BAD_ARG;
    }
    hipLaunchKernelGGL(npi_cost, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, T, n_npi, Su,
                       weights_per_day, u_series, newcases, inputs, weights, J0, J1);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(err, e, "npi_cost launch");
    return EPI_OK;
}

int epi_si_controlled_device(int32_t B, int32_t K, int32_t Sa, double dt, const int32_t *alpha_series, const double *alpha,
                             const double *prm, double *s, double *i, void *stream, char *err)
{
    if (B < 1 || K < 1 || Sa < 1 || !prm || !s || !i || (K > 1 && !alpha) || (!alpha_series && Sa != B)) {
        set_err(err, "bad SI_Controlled arguments"); return EPI_ERR_BAD_ARG;
    }
    hipLaunchKernelGGL(si_controlled, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, K, Sa, dt, alpha_series,
                       alpha, prm, s, i);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(err, e, "si_controlled launch");
    return EPI_OK;
}

int epi_sir_sim_device(int32_t B, int32_t K, double dt, const double *prm, double *out, void *stream, char *err)
{
    if (B < 1 || K < 1 || !prm || !out) { set_err(err, "bad SIR arguments"); return EPI_ERR_BAD_ARG; }
    hipLaunchKernelGGL(sir_sim, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, K, dt, prm, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(err, e, "sir_sim launch");
    return EPI_OK;
}

// ---- host-pointer variants of the simulators and the cost (what a MEX gateway binds: matlab/epiekf_sim_mex.cpp) ----

static int sialpha_sim_host(const epi_sim_desc *d, const epi_noise_desc *noise, const int32_t *u_series, const double *u, const double *sp,
                            const double *z, double *s, double *i, double *alpha, double *J0, double *J1, int device,
                            char *err)
{
    if (!d || d->B < 1 || d->K < 1 || d->Su < 1 || d->n_npi < 1 || !u || !sp) { set_err(err, "bad simulator descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->u_block != 0) { set_err(err, "u_block is a device-side layout"); return EPI_ERR_BAD_ARG; }
    const size_t B = d->B, K = d->K;
    HostIO io;
    const size_t o_us = io.in(u_series, B * 4), o_u = io.in(u, K * d->n_npi * (size_t)d->Su * 8);
    const size_t o_sp = io.in(sp, (size_t)EPI_SIM_PRM_COUNT * B * 8), o_z = io.in(z, K * 3 * B * 8);
    const size_t o_s = io.out(s, K * B * 8), o_i = io.out(i, K * B * 8), o_a = io.out(alpha, K * B * 8);
    const size_t o_0 = io.out(J0, B * 8), o_1 = io.out(J1, B * 8);
    auto enqueue = [&](char *base, hipStream_t st) {
        auto f64 = [&](size_t o) { return HostIO::at<double>(base, o); };
        const int32_t *dus = HostIO::at<const int32_t>(base, o_us);
        if (noise)
            return epi_sialpha_sim_device_seeded(d, noise, dus, f64(o_u), f64(o_sp), nullptr, f64(o_s), f64(o_i), f64(o_a), f64(o_0),
                                                 f64(o_1), st, err);
        return epi_sialpha_sim_device(d, dus, f64(o_u), f64(o_sp), f64(o_z), f64(o_s), f64(o_i), f64(o_a), f64(o_0), f64(o_1), st, err);
    };
    return run_host(device, io, err, enqueue);
}

int epi_sialpha_sim_host(const epi_sim_desc *d, const int32_t *u_series, const double *u, const double *sp,
                         const double *z, double *s, double *i, double *alpha, double *J0, double *J1, int device,
                         char *err)
{
    return sialpha_sim_host(d, nullptr, u_series, u, sp, z, s, i, alpha, J0, J1, device, err);
}

int epi_sialpha_sim_host_seeded(const epi_sim_desc *d, const epi_noise_desc *noise, const int32_t *u_series, const double *u,
                                const double *sp, const double *z, double *s, double *i, double *alpha, double *J0, double *J1,
                                int device, char *err)
{
    NoiseKey nk;
    int rc = noise_key(noise, z, &nk, err);                // before anything is staged
    if (rc != EPI_OK) return rc;
    return sialpha_sim_host(d, noise, u_series, u, sp, nullptr, s, i, alpha, J0, J1, device, err);
}

int epi_seirp_sim_host(int32_t B, int32_t K, int32_t par_steps, double dt, int32_t saturated, int32_t integrator,
                       const double *par, const double *init, const double *sat, double *out, int device, char *err)
{
    if (B < 1 || K < 1 || par_steps < 1 || !par || !init || !out) { set_err(err, "bad SEIRP arguments"); return EPI_ERR_BAD_ARG; }
    HostIO io;
    const size_t o_p = io.in(par, (size_t)par_steps * 7 * B * 8), o_i = io.in(init, (size_t)5 * B * 8), o_s = io.in(sat, (size_t)6 * B * 8);
    const size_t o_out = io.out(out, (size_t)K * 5 * B * 8);
    auto enqueue = [&](char *base, hipStream_t st) {
        auto f64 = [&](size_t o) { return HostIO::at<double>(base, o); };
        return epi_seirp_sim_device(B, K, par_steps, dt, saturated, integrator, f64(o_p), f64(o_i), f64(o_s), f64(o_out), st, err);
    };
    return run_host(device, io, err, enqueue);
}

int epi_si_controlled_host(int32_t B, int32_t K, int32_t Sa, double dt, const int32_t *alpha_series, const double *alpha,
                           const double *prm, double *s, double *i, int device, char *err)
{
    if (B < 1 || K < 1 || Sa < 1) { set_err(err, "bad SI_Controlled arguments"); return EPI_ERR_BAD_ARG; }
    HostIO io;
    const size_t o_as = io.in(alpha_series, (size_t)B * 4), o_a = io.in(alpha, (size_t)(K > 1 ? K - 1 : 1) * Sa * 8);
    const size_t o_p = io.in(prm, (size_t)3 * B * 8);
    const size_t o_s = io.out(s, (size_t)K * B * 8), o_i = io.out(i, (size_t)K * B * 8);
    auto enqueue = [&](char *base, hipStream_t st) {
        auto f64 = [&](size_t o) { return HostIO::at<double>(base, o); };
        return epi_si_controlled_device(B, K, Sa, dt, HostIO::at<const int32_t>(base, o_as), f64(o_a), f64(o_p), f64(o_s), f64(o_i), st, err);
    };
    return run_host(device, io, err, enqueue);
}

int epi_npi_cost_host(int32_t B, int32_t T, int32_t n_npi, int32_t Su, int32_t weights_per_day, const int32_t *u_series,
                      const double *newcases, const double *inputs, const double *weights, double *J0, double *J1,
                      int device, char *err)
{
    if (B < 1 || T < 1 || n_npi < 1 || Su < 1) { set_err(err, "bad NPICost arguments"); return EPI_ERR_BAD_ARG; }
    HostIO io;
    const size_t o_us = io.in(u_series, (size_t)B * 4), o_n = io.in(newcases, (size_t)T * B * 8);
    const size_t o_u = io.in(inputs, (size_t)T * n_npi * Su * 8);
    const size_t o_w = io.in(weights, (size_t)(weights_per_day ? T : 1) * n_npi * B * 8);
    const size_t o_0 = io.out(J0, (size_t)B * 8), o_1 = io.out(J1, (size_t)B * 8);
    auto enqueue = [&](char *base, hipStream_t st) {
        auto f64 = [&](size_t o) { return HostIO::at<double>(base, o); };
        return epi_npi_cost_device(B, T, n_npi, Su, weights_per_day, HostIO::at<const int32_t>(base, o_us), f64(o_n), f64(o_u), f64(o_w),
                                   f64(o_0), f64(o_1), st, err);
    };
    return run_host(device, io, err, enqueue);
}

int epi_sir_sim_host(int32_t B, int32_t K, double dt, const double *prm, double *out, int device, char *err)
{
    if (B < 1 || K < 1) { set_err(err, "bad SIR arguments"); return EPI_ERR_BAD_ARG; }
    HostIO io;
    const size_t o_p = io.in(prm, (size_t)6 * B * 8), o_out = io.out(out, (size_t)K * 3 * B * 8);
    auto enqueue = [&](char *base, hipStream_t st) {
        return epi_sir_sim_device(B, K, dt, HostIO::at<const double>(base, o_p), HostIO::at<double>(base, o_out), st, err);
    };
    return run_host(device, io, err, enqueue);
}

int epi_preprocess_host(const epi_pre_desc *d, const double *cases, const double *deaths, const double *population,
                        const double *ip, const epi_pre_outputs *out, int device, char *err)
{
    if (!d || !out || d->S < 1 || d->T < 1 || d->n_npi < 0 || d->n_npi > EPI_MAX_NPI) { set_err(err, "bad preprocessing descriptor"); return EPI_ERR_BAD_ARG; }
    const size_t TS = (size_t)d->T * d->S * 8;
    HostIO io;
    const size_t o_c = io.in(cases, TS), o_d = io.in(deaths, TS), o_p = io.in(population, (size_t)d->S * 8);
    const size_t o_ip = io.in(ip, TS * (size_t)d->n_npi);
    using PO = epi_pre_outputs;
    struct O { double *PO::*arr; size_t bytes; };
    const O outs[9] = {{&PO::new_refined, TS}, {&PO::new_smoothed, TS}, {&PO::zero_lag, TS}, {&PO::x_new, TS}, {&PO::x_total, TS},
                       {&PO::R_v, TS}, {&PO::fatality, TS}, {&PO::I0, (size_t)d->S * 8}, {&PO::ip_filled, TS * (size_t)d->n_npi}};
    size_t o_out[9];
    for (int k = 0; k < 9; k++) o_out[k] = io.out(out->*outs[k].arr, outs[k].bytes);
    const size_t wsb = epi_preprocess_workspace_bytes(d);
    const size_t o_ws = wsb ? io.reserve(wsb) : HostIO::kAbsent;
    auto enqueue = [&](char *base, hipStream_t st) {
        auto f64 = [&](size_t o) { return HostIO::at<double>(base, o); };
        epi_pre_outputs dout{};
        for (int k = 0; k < 9; k++) dout.*outs[k].arr = f64(o_out[k]);
        return epi_preprocess_device(d, f64(o_c), f64(o_d), f64(o_p), f64(o_ip), &dout, HostIO::at<void>(base, o_ws), wsb, st, err);
    };
    return run_host(device, io, err, enqueue);
}

int epi_nnls_affine_fit_host(const epi_nnls_desc *d, const double *X, const double *y, double *a, double *b,
                             double *min_err, int32_t *iters, int32_t *flag, int device, char *err)
{
    if (!d || d->S < 1 || d->D < 1 || d->n < 1 || d->n > EPI_MAX_NPI) { set_err(err, "bad NNLS descriptor"); return EPI_ERR_BAD_ARG; }
    const size_t S = d->S;
    HostIO io;
    const size_t o_X = io.in(X, (size_t)d->D * d->n * S * 8), o_y = io.in(y, (size_t)d->D * S * 8);
    const size_t o_a = io.out(a, (size_t)d->n * S * 8), o_b = io.out(b, S * 8), o_m = io.out(min_err, S * 8);
    const size_t o_i = io.out(iters, S * 4), o_f = io.out(flag, S * 4);
    auto enqueue = [&](char *base, hipStream_t st) {
        auto f64 = [&](size_t o) { return HostIO::at<double>(base, o); };
        return epi_nnls_affine_fit_device(d, f64(o_X), f64(o_y), f64(o_a), f64(o_b), f64(o_m), HostIO::at<int32_t>(base, o_i),
                                          HostIO::at<int32_t>(base, o_f), st, err);
    };
    return run_host(device, io, err, enqueue);
}

static int random_npi_mc_host(const epi_mc_desc *d, const epi_noise_desc *noise, const double *sp, const double *u_min, const double *z,
                              const double *J0_prefix, const double *J1_prefix, double *u_out, double *J0, double *J1,
                              int device, char *err)
{
    if (!d || d->R < 1 || d->n_scen < 1 || d->K < 1 || d->n_npi < 1 || d->n_npi > EPI_MAX_NPI ||
        (int64_t)d->R * d->n_scen > (int64_t)1 << 30) { set_err(err, "bad Monte-Carlo scenario descriptor"); return EPI_ERR_BAD_ARG; }
    const size_t R = d->R, B = R * (size_t)d->n_scen, K = d->K;
    HostIO io;
    const size_t o_sp = io.in(sp, (size_t)EPI_SIM_PRM_COUNT * R * 8), o_um = io.in(u_min, (size_t)d->n_npi * R * 8);
    const size_t o_z = io.in(z, K * 3 * B * 8), o_p0 = io.in(J0_prefix, R * 8), o_p1 = io.in(J1_prefix, R * 8);
    const size_t o_u = io.out(u_out, K * (size_t)d->n_npi * B * 8), o_0 = io.out(J0, B * 8), o_1 = io.out(J1, B * 8);
    auto enqueue = [&](char *base, hipStream_t st) {
        auto f64 = [&](size_t o) { return HostIO::at<double>(base, o); };
        if (noise)
            return epi_random_npi_mc_device_seeded(d, noise, f64(o_sp), f64(o_um), nullptr, f64(o_p0), f64(o_p1), f64(o_u), f64(o_0),
                                                   f64(o_1), st, err);
        return epi_random_npi_mc_device(d, f64(o_sp), f64(o_um), f64(o_z), f64(o_p0), f64(o_p1), f64(o_u), f64(o_0), f64(o_1), st, err);
    };
    return run_host(device, io, err, enqueue);
}

int epi_random_npi_mc_host(const epi_mc_desc *d, const double *sp, const double *u_min, const double *z,
                           const double *J0_prefix, const double *J1_prefix, double *u_out, double *J0, double *J1,
                           int device, char *err)
{
    return random_npi_mc_host(d, nullptr, sp, u_min, z, J0_prefix, J1_prefix, u_out, J0, J1, device, err);
}

int epi_random_npi_mc_host_seeded(const epi_mc_desc *d, const epi_noise_desc *noise, const double *sp, const double *u_min,
                                  const double *z, const double *J0_prefix, const double *J1_prefix, double *u_out, double *J0,
                                  double *J1, int device, char *err)
{
    NoiseKey nk;
    int rc = noise_key(noise, z, &nk, err);                // before anything is staged
    if (rc != EPI_OK) return rc;
    return random_npi_mc_host(d, noise, sp, u_min, nullptr, J0_prefix, J1_prefix, u_out, J0, J1, device, err);
}

int epi_rt_expfit_validate(const epi_rt_desc *d, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->B < 1 || d->T < 1 || d->Sx < 1 || d->L < 1) { set_err(err, "B, T, Sx, L must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->B > (1 << 23) || d->Sx > (1 << 23)) { set_err(err, "B, Sx are limited to 2^23"); return EPI_ERR_BAD_ARG; }
    if (d->order != 1 && d->order != 2) { set_err(err, epi_status_string(EPI_ERR_UNDEFINED_ORDER)); return EPI_ERR_UNDEFINED_ORDER; }
    if ((size_t)3 * d->L * kWave * sizeof(double) > 160u * 1024u) { set_err(err, "inv_monitor_len too large for LDS (max 106)"); return EPI_ERR_UNSUPPORTED; }
    return EPI_OK;
}

int epi_rt_expfit_run_device(const epi_rt_desc *d, const int32_t *x_series, const double *x, const double *rp,
                             const epi_rt_outputs *out, void *stream, char *err)
{
    int rc = epi_rt_expfit_validate(d, err);
    if (rc != EPI_OK) return rc;
    if (!x || !rp || !out) { set_err(err, "NULL input array"); return EPI_ERR_BAD_ARG; }
    if (!x_series && d->Sx != d->B) { set_err(err, "identity x_series needs Sx == B"); return EPI_ERR_BAD_ARG; }
    if (!out->S_MINUS || !out->S_PLUS || !out->P_MINUS || !out->P_PLUS) {
        set_err(err, "S_MINUS, S_PLUS, P_MINUS, P_PLUS are required outputs"); return EPI_ERR_BAD_ARG;
    }
    RtArgs a{};
    a.B = d->B; a.T = d->T; a.Sx = d->Sx; a.L = d->L; a.order = d->order;
    a.x_series = x_series; a.x = x; a.rp = rp;
    a.S_MINUS = out->S_MINUS; a.S_PLUS = out->S_PLUS; a.P_MINUS = out->P_MINUS; a.P_PLUS = out->P_PLUS;
    a.K_GAIN = out->K_GAIN; a.S_SMOOTH = out->S_SMOOTH; a.P_SMOOTH = out->P_SMOOTH;
    a.innovations = out->innovations; a.rho = out->rho;
    const size_t shmem = (size_t)3 * d->L * kWave * sizeof(double);
    hipError_t e;
    if (shmem > 64u * 1024u &&
        (e = hipFuncSetAttribute((const void *)rt_expfit_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem)) != hipSuccess)
        return hip_fail(err, e, "hipFuncSetAttribute");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rt_expfit_fwd, dim3((d->B + kWave - 1) / kWave), dim3(kWave), shmem, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "rt_expfit_fwd launch");
    if (a.S_SMOOTH || a.P_SMOOTH) {
        hipLaunchKernelGGL(rt_expfit_bwd, dim3((d->B + 255) / 256), dim3(256), 0, st, a);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "rt_expfit_bwd launch");
    }
    return EPI_OK;
}

int epi_rt_expfit_run_host(const epi_rt_desc *d, const int32_t *x_series, const double *x, const double *rp,
                           const epi_rt_outputs *out, int device, char *err)
{
    int rc = epi_rt_expfit_validate(d, err);
    if (rc != EPI_OK) return rc;
    if (!x || !rp || !out) { set_err(err, "NULL input array"); return EPI_ERR_BAD_ARG; }
    const size_t B = d->B, T = d->T;
    HostIO io;
    const size_t o_xs = io.in(x_series, B * 4), o_x = io.in(x, T * d->Sx * 8), o_rp = io.in(rp, (size_t)EPI_RT_PRM_COUNT * B * 8);
    struct O { double *epi_rt_outputs::*arr; size_t bytes; bool required; };
    const size_t n2 = T * 2 * B * 8, n4 = T * 4 * B * 8, n1 = T * B * 8;
    const O outs[] = {{&epi_rt_outputs::S_MINUS, n2, true}, {&epi_rt_outputs::S_PLUS, n2, true}, {&epi_rt_outputs::P_MINUS, n4, true},
                      {&epi_rt_outputs::P_PLUS, n4, true}, {&epi_rt_outputs::K_GAIN, n2, false}, {&epi_rt_outputs::S_SMOOTH, n2, false},
                      {&epi_rt_outputs::P_SMOOTH, n4, false}, {&epi_rt_outputs::innovations, n1, false}, {&epi_rt_outputs::rho, n1, false}};
    size_t o_out[9];
    for (int k = 0; k < 9; k++)   // forward quantities the caller does not want still feed the smoother: a device copy, no download
        o_out[k] = outs[k].required ? io.add_out(out->*outs[k].arr, 1, 1, outs[k].bytes, 0, outs[k].bytes) : io.out(out->*outs[k].arr, outs[k].bytes);
    auto enqueue = [&](char *base, hipStream_t st) {
        epi_rt_outputs dout{};
        for (int k = 0; k < 9; k++) dout.*outs[k].arr = HostIO::at<double>(base, o_out[k]);
        return epi_rt_expfit_run_device(d, HostIO::at<const int32_t>(base, o_xs), HostIO::at<const double>(base, o_x),
                                        HostIO::at<const double>(base, o_rp), &dout, st, err);
    };
    return run_host(device, io, err, enqueue);
}

static int pre_validate(const epi_pre_desc *d, int *W2, int *nfact, char *err)
{
    if (!d || d->abi_version != EPIEKF_ABI_VERSION || d->S < 1 || d->n_npi < 0 || d->n_npi > EPI_MAX_NPI || d->first_num_days < 0) {
        set_err(err, "bad preprocessing descriptor"); return EPI_ERR_BAD_ARG;
    }
    if (d->W < 1 || d->W > kPreMaxTaps) { set_err(err, "SmoothingWinLen out of range 1..32"); return EPI_ERR_BAD_ARG; }
    if (d->T < 2) { set_err(err, "Insufficient data"); return EPI_ERR_BAD_ARG; }            // :168
    int w2 = (int)floor((double)d->W / 2 + 0.5);                                            // MATLAB round()
    if (w2 < 1) w2 = 1;
    const int nf = (3 * (w2 - 1) > 1) ? 3 * (w2 - 1) : 1;
    if (d->T <= nf) {
        char b[96]; snprintf(b, sizeof b, "Data length must be larger than %d samples.", nf);
        set_err(err, b); return EPI_ERR_BAD_ARG;
    }
    *W2 = w2; *nfact = nf;
    return EPI_OK;
}

size_t epi_preprocess_workspace_bytes(const epi_pre_desc *d)
{
    int W2, nfact;
    if (pre_validate(d, &W2, &nfact, nullptr) != EPI_OK) return 0;
    return ((size_t)3 * d->T + 2 * (size_t)nfact) * (size_t)d->S * sizeof(double);
}

int epi_preprocess_device(const epi_pre_desc *d, const double *cases, const double *deaths, const double *population,
                          const double *ip, const epi_pre_outputs *out, void *workspace, size_t workspace_bytes,
                          void *stream, char *err)
{
    int W2 = 0, nfact = 0;
    int rc = pre_validate(d, &W2, &nfact, err);
    if (rc != EPI_OK) return rc;
    if (!cases || !population || !out) { set_err(err, "NULL input array"); return EPI_ERR_BAD_ARG; }
    if (out->ip_filled && (!ip || d->n_npi < 1)) { set_err(err, "ip_filled selected without ip"); return EPI_ERR_BAD_ARG; }
    if (out->fatality && !deaths) { set_err(err, "fatality selected without deaths"); return EPI_ERR_BAD_ARG; }
    if (!workspace || workspace_bytes < epi_preprocess_workspace_bytes(d)) {
        set_err(err, epi_status_string(EPI_ERR_WORKSPACE)); return EPI_ERR_WORKSPACE;
    }
    PreArgs a{};
    a.T = d->T; a.S = d->S; a.W = d->W; a.W2 = W2; a.nfact = nfact; a.first_num_days = d->first_num_days;
    a.min_cases = d->min_cases;
    a.cases = cases; a.deaths = deaths; a.population = population;
    a.new_refined = out->new_refined; a.new_smoothed = out->new_smoothed; a.zero_lag = out->zero_lag;
    a.x_new = out->x_new; a.x_total = out->x_total; a.R_v = out->R_v; a.fatality = out->fatality; a.I0 = out->I0;
    a.ws = (double *)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(preprocess_regions, dim3((d->S + 63) / 64), dim3(64), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(err, e, "preprocess_regions launch");
    if (out->ip_filled) {
        const int cols = d->n_npi * d->S;
        hipLaunchKernelGGL(npi_fill, dim3((cols + 255) / 256), dim3(256), 0, st, d->T, cols, ip, out->ip_filled);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "npi_fill launch");
    }
    return EPI_OK;
}

int epi_nnls_affine_fit_device(const epi_nnls_desc *d, const double *X, const double *y, double *a, double *b,
                               double *min_err, int32_t *iters, int32_t *flag, void *stream, char *err)
{
    if (!d || d->abi_version != EPIEKF_ABI_VERSION || d->S < 1 || d->D < 1 || d->n < 1 || d->n > kNnMax || d->max_iters < 0 ||
        !X || !y || !a) {
        set_err(err, "bad NNLS descriptor"); return EPI_ERR_BAD_ARG;
    }
    const size_t shmem = ((size_t)kNnDoubles * sizeof(double) + (size_t)kNnInts * sizeof(int)) * kNnLanes;
    hipError_t e = hipFuncSetAttribute((const void *)nnls_affine_fit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    if (e != hipSuccess) return hip_fail(err, e, "hipFuncSetAttribute");
    NnArgs g{};
    g.S = d->S; g.D = d->D; g.n = d->n; g.max_iters = d->max_iters;
    g.X = X; g.y = y; g.a = a; g.b = b; g.min_err = min_err; g.iters = iters; g.flag = flag;
    hipLaunchKernelGGL(nnls_affine_fit, dim3((d->S + kNnLanes - 1) / kNnLanes), dim3(kNnLanes), shmem, (hipStream_t)stream, g);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "nnls_affine_fit launch");
    return EPI_OK;
}

int epi_seirp_sim_device(int32_t B, int32_t K, int32_t par_steps, double dt, int32_t saturated, int32_t integrator,
                         const double *par, const double *init, const double *sat, double *out, void *stream, char *err)
{
    if (B < 1 || K < 1 || !par || !init || !out || (saturated && !sat) || (par_steps != 1 && par_steps < K - 1) ||
        (integrator != 0 && integrator != 1)) {
        set_err(err, "bad SEIRP arguments"); return EPI_ERR_BAD_ARG;
    }
    const int blocks = (B + 255) / 256;
    hipLaunchKernelGGL(seirp_sim, dim3(blocks), dim3(256), 0, (hipStream_t)stream, B, K, par_steps, dt, saturated, integrator, par, init, sat, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(err, e, "seirp_sim launch");
    return EPI_OK;
}


// ---- the forecast look-ahead error study (Tools/ForecastQualityAssessment.m:359-393, 428-449; include/epiekf.h) ----
// Lane mapping of the study's filter when the descriptor leaves it open (shape 0).  At the study's batch sizes one lane per
// chain wins: 236 regions x 91 starts (21 476 chains) x 366 days 1.36 ms per call against 2.49 with seven chains per
// wavefront, 300 regions (27 300 chains) 1.53 against 3.41 (profiles/lookahead/bench.json); small studies keep the filter's
// own small-batch choice.
static int la_shape(const epi_lookahead_desc *d)
{
    if (d->shape != 0) return d->shape;
    return (int64_t)d->R * d->F <= 2048 ? EPI_SHAPE_WAVE : EPI_SHAPE_LANE;
}

// the filter call of the study: chain c = r * F + (s - 1), observations materialised per chain, controls shared per region
static epi_batch_desc la_batch_desc(const epi_lookahead_desc *d, int path_hint)
{
    epi_batch_desc b{};
    b.abi_version = EPIEKF_ABI_VERSION; b.model = EPI_MODEL_SIA3;
    b.B = d->R * d->F; b.T = d->LL; b.Sx = b.B; b.Su = d->R;
    b.n_npi = d->n_npi; b.L = d->L; b.order = d->order; b.obs_type = d->obs_type; b.r_mode = d->r_mode; b.q_mode = 0;
    b.out_mask = EPI_OUT_S_PLUS | EPI_OUT_S_SMOOTH;
    b.path_hint = path_hint; b.shape = la_shape(d); b.placement_tries = d->placement_tries;
    return b;
}

struct LaWs { size_t x, rs, rsc, prm, si, psi, sf, psf, q, us, sp, ss, ekf, ekf_bytes, total; };
static LaWs la_ws_layout(const epi_lookahead_desc *d)
{
    const size_t B = (size_t)d->R * d->F, T = (size_t)d->LL;
    LaWs w{};
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += (n + 255) & ~(size_t)255; return o; };
    w.x = take(T * B * 8);
    w.rs = take(d->r_mode == 1 ? T * B * 8 : 0); w.rsc = take(d->r_mode == 0 ? B * 8 : 0);
    w.prm = take((size_t)EPI_PRM_COUNT * B * 8);
    w.si = take(3 * B * 8); w.psi = take(9 * B * 8); w.sf = take(3 * B * 8); w.psf = take(9 * B * 8); w.q = take(9 * B * 8);
    w.us = take(B * 4);
    w.sp = take(T * 3 * B * 8); w.ss = take(T * 3 * B * 8);      // used when the caller does not take S_PLUS / S_SMOOTH
    const epi_batch_desc b = la_batch_desc(d, 0);                  // path_hint 0 needs the most workspace
    w.ekf_bytes = epi_ekf_workspace_bytes(&b);
    w.ekf = take(w.ekf_bytes);
    w.total = off;
    return w;
}

int epi_lookahead_validate(const epi_lookahead_desc *d, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->model != EPI_MODEL_SIA3) {
        set_err(err, "the look-ahead study runs SIAlphaModelEKF (EPI_MODEL_SIA3) only"); return EPI_ERR_UNSUPPORTED;
    }
    if (d->R < 1 || d->LL < 1) { set_err(err, "R and LL must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->F < 1) { set_err(err, "F (num_forecast_days) must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->F > d->LL) { set_err(err, "F (num_forecast_days) must not exceed LL: a start masks at most every day"); return EPI_ERR_BAD_ARG; }
    if (d->F > kLaMaxF) { set_err(err, "F (num_forecast_days) is limited to 1024 (a table column is staged in LDS)"); return EPI_ERR_BAD_ARG; }
    if (d->M < 1) { set_err(err, "M (MaxLookAheadDays) must be >= 1"); return EPI_ERR_BAD_ARG; }
    if ((int64_t)d->R * d->F > ((int64_t)1 << 23)) { set_err(err, "R * F chains are limited to 2^23"); return EPI_ERR_BAD_ARG; }
    if ((int64_t)d->R * d->M > (int64_t)0x7fffffff) { set_err(err, "M * R table columns exceed the grid"); return EPI_ERR_BAD_ARG; }
    if (d->shape != 0 && d->shape != EPI_SHAPE_LANE && d->shape != EPI_SHAPE_WAVE) {
        set_err(err, "shape must be 0 (the study decides), 1 (one lane per chain) or 3 (seven chains per wavefront)"); return EPI_ERR_BAD_ARG;
    }
    const epi_batch_desc b = la_batch_desc(d, 0);
    return epi_ekf_validate(&b, err);
}

size_t epi_lookahead_workspace_bytes(const epi_lookahead_desc *d)
{
    if (epi_lookahead_validate(d, nullptr) != EPI_OK) return 0;
    return la_ws_layout(d).total;
}

static int la_args_ok(const epi_lookahead_desc *d, const epi_lookahead_inputs *in, const epi_lookahead_outputs *out, char *err)
{
    int rc = epi_lookahead_validate(d, err);
    if (rc != EPI_OK) return rc;
    if (!in || !out) { set_err(err, "NULL inputs/outputs"); return EPI_ERR_BAD_ARG; }
    if (!in->x || !in->u || !in->prm || !in->s_init || !in->Ps_init || !in->s_final || !in->Ps_final || !in->Q) {
        set_err(err, "NULL input array"); return EPI_ERR_BAD_ARG;
    }
    if (!in->truth || !in->population) { set_err(err, "NULL truth / population"); return EPI_ERR_BAD_ARG; }
    if (d->r_mode == 0 && !in->R_scalar) { set_err(err, "r_mode 0 needs R_scalar"); return EPI_ERR_BAD_ARG; }
    if (d->r_mode == 1 && !in->R_series) { set_err(err, "r_mode 1 needs R_series"); return EPI_ERR_BAD_ARG; }
    if (!out->est_plus || !out->est_smooth || !out->mean_plus || !out->median_plus || !out->std_plus || !out->mean_smooth ||
        !out->median_smooth || !out->std_smooth) {
        set_err(err, "NULL output table / statistic"); return EPI_ERR_BAD_ARG;
    }
    return EPI_OK;
}

// expand -> filter + smoother -> error tables -> statistics, all on `st`
static int la_enqueue(const epi_lookahead_desc *d, const epi_lookahead_inputs *in, const epi_lookahead_outputs *out,
                      void *workspace, size_t workspace_bytes, int path_hint, hipStream_t st, char *err)
{
    int rc = la_args_ok(d, in, out, err);
    if (rc != EPI_OK) return rc;
    const LaWs wl = la_ws_layout(d);
    if (!workspace || workspace_bytes < wl.total) { set_err(err, epi_status_string(EPI_ERR_WORKSPACE)); return EPI_ERR_WORKSPACE; }
    char *ws = (char *)workspace;
    const int B = d->R * d->F;
    LaArgs a{};
    a.R = d->R; a.LL = d->LL; a.F = d->F; a.M = d->M; a.n_npi = d->n_npi; a.r_mode = d->r_mode;
    a.x = in->x; a.R_series = in->R_series; a.R_scalar = in->R_scalar; a.prm = in->prm; a.s_init = in->s_init; a.Ps_init = in->Ps_init;
    a.s_final = in->s_final; a.Ps_final = in->Ps_final; a.Q = in->Q; a.truth = in->truth; a.population = in->population;
    a.cx = (double *)(ws + wl.x); a.cR_series = d->r_mode == 1 ? (double *)(ws + wl.rs) : nullptr;
    a.cR_scalar = d->r_mode == 0 ? (double *)(ws + wl.rsc) : nullptr;
    a.cprm = (double *)(ws + wl.prm); a.cs_init = (double *)(ws + wl.si); a.cPs_init = (double *)(ws + wl.psi);
    a.cs_final = (double *)(ws + wl.sf); a.cPs_final = (double *)(ws + wl.psf); a.cQ = (double *)(ws + wl.q);
    a.u_series = (int32_t *)(ws + wl.us);
    a.S_PLUS = out->S_PLUS ? out->S_PLUS : (double *)(ws + wl.sp);
    a.S_SMOOTH = out->S_SMOOTH ? out->S_SMOOTH : (double *)(ws + wl.ss);
    a.est_plus = out->est_plus; a.est_smooth = out->est_smooth;
    a.mean_plus = out->mean_plus; a.median_plus = out->median_plus; a.std_plus = out->std_plus;
    a.mean_smooth = out->mean_smooth; a.median_smooth = out->median_smooth; a.std_smooth = out->std_smooth;
    const int nrows = d->LL * (d->r_mode == 1 ? 2 : 1) + kLaChainRows;
    hipLaunchKernelGGL(lookahead_expand, dim3((unsigned)((B + 255) / 256), (unsigned)(nrows < 4096 ? nrows : 4096)), dim3(256), 0, st, a, nrows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(err, e, "lookahead_expand launch");
    const epi_batch_desc b = la_batch_desc(d, path_hint);
    epi_inputs din{};
    din.x_series = nullptr; din.u_series = a.u_series;
    din.x = a.cx; din.u = in->u; din.R_series = a.cR_series; din.R_scalar = a.cR_scalar; din.prm = a.cprm;
    din.s_init = a.cs_init; din.Ps_init = a.cPs_init; din.s_final = a.cs_final; din.Ps_final = a.cPs_final; din.Q = a.cQ;
    epi_outputs dout{};
    dout.S_PLUS = (double *)a.S_PLUS; dout.S_SMOOTH = (double *)a.S_SMOOTH; dout.status = out->status;
    rc = epi_ekf_run_device(&b, &din, &dout, ws + wl.ekf, wl.ekf_bytes, st, err);
    if (rc != EPI_OK) return rc;
    const size_t n_err = (size_t)d->F * d->M * d->R;
    for (size_t e0 = 0; e0 < n_err; e0 += kLaLaunchElements) {   // in slices: see LaArgs
        a.e0 = e0;
        const size_t ne = n_err - e0 < kLaLaunchElements ? n_err - e0 : kLaLaunchElements;
        hipLaunchKernelGGL(lookahead_errors, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, a);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "lookahead_errors launch");
    }
    const int64_t n_col = (int64_t)d->M * d->R;                  // <= 2^31 - 1 (epi_lookahead_validate)
    for (int64_t col0 = 0; col0 < n_col; col0 += kLaLaunchColumns) {
        a.col0 = (int)col0;
        const int64_t nc = n_col - col0 < kLaLaunchColumns ? n_col - col0 : kLaLaunchColumns;
        hipLaunchKernelGGL(lookahead_stats, dim3((unsigned)nc, 2), dim3(kWave), 0, st, a);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "lookahead_stats launch");
    }
    return EPI_OK;
}

int epi_lookahead_run_device(const epi_lookahead_desc *d, const epi_lookahead_inputs *in, const epi_lookahead_outputs *out,
                             void *workspace, size_t workspace_bytes, void *stream, char *err)
{
    return la_enqueue(d, in, out, workspace, workspace_bytes, 0, (hipStream_t)stream, err);
}

int epi_lookahead_run_host(const epi_lookahead_desc *d, const epi_lookahead_inputs *in, const epi_lookahead_outputs *out,
                           int device, char *err)
{
    int rc = la_args_ok(d, in, out, err);
    if (rc != EPI_OK) return rc;
    const size_t R = (size_t)d->R, T = (size_t)d->LL, F = (size_t)d->F, M = (size_t)d->M, B = R * F, n = (size_t)d->n_npi;
    HostIO io;
    const size_t o_x = io.add_in(in->x, T, 8, R, 0, R), o_u = io.add_in(in->u, T * n, 8, R, 0, R);
    const size_t o_rs = d->r_mode == 1 ? io.add_in(in->R_series, T, 8, R, 0, R) : io.add_in(in->R_scalar, 1, 8, R, 0, R);
    const size_t o_prm = io.add_in(in->prm, EPI_PRM_COUNT, 8, R, 0, R), o_si = io.add_in(in->s_init, 3, 8, R, 0, R);
    const size_t o_psi = io.add_in(in->Ps_init, 9, 8, R, 0, R), o_sf = io.add_in(in->s_final, 3, 8, R, 0, R);
    const size_t o_psf = io.add_in(in->Ps_final, 9, 8, R, 0, R), o_q = io.add_in(in->Q, 9, 8, R, 0, R);
    const size_t o_tr = io.add_in(in->truth, T, 8, R, 0, R), o_pop = io.add_in(in->population, 1, 8, R, 0, R);
    using LO = epi_lookahead_outputs;
    double *LO::*const stats[6] = {&LO::mean_plus, &LO::median_plus, &LO::std_plus, &LO::mean_smooth, &LO::median_smooth, &LO::std_smooth};
    const size_t o_ep = io.add_out(out->est_plus, F * M, 8, R, 0, R), o_es = io.add_out(out->est_smooth, F * M, 8, R, 0, R);
    size_t o_st[6];
    for (int k = 0; k < 6; k++) o_st[k] = io.add_out(out->*stats[k], M, 8, R, 0, R);
    const size_t o_sp = out->S_PLUS ? io.add_out(out->S_PLUS, T * 3, 8, B, 0, B) : HostIO::kAbsent;
    const size_t o_ss = out->S_SMOOTH ? io.add_out(out->S_SMOOTH, T * 3, 8, B, 0, B) : HostIO::kAbsent;
    const size_t o_status = out->status ? io.add_out(out->status, 1, 4, B, 0, B) : HostIO::kAbsent;
    const size_t wsb = epi_lookahead_workspace_bytes(d);
    const size_t o_ws = io.reserve(wsb);
    // the inputs are per region: the packed kernels' conditions are checked on the host, once per region
    epi_inputs hin{};
    hin.s_init = in->s_init; hin.Ps_init = in->Ps_init; hin.s_final = in->s_final; hin.Ps_final = in->Ps_final; hin.Q = in->Q;
    const int path_hint = host_precheck(3, false, &hin, R, 0, R) ? 1 : 2;
    auto enqueue = [&](char *base, hipStream_t st) {
        auto dp = [&](size_t o) { return HostIO::at<const double>(base, o); };
        epi_lookahead_inputs din{};
        din.x = dp(o_x); din.u = dp(o_u);
        din.R_series = d->r_mode == 1 ? dp(o_rs) : nullptr; din.R_scalar = d->r_mode == 0 ? dp(o_rs) : nullptr;
        din.prm = dp(o_prm); din.s_init = dp(o_si); din.Ps_init = dp(o_psi); din.s_final = dp(o_sf); din.Ps_final = dp(o_psf);
        din.Q = dp(o_q); din.truth = dp(o_tr); din.population = dp(o_pop);
        epi_lookahead_outputs dout{};
        dout.est_plus = HostIO::at<double>(base, o_ep); dout.est_smooth = HostIO::at<double>(base, o_es);
        for (int k = 0; k < 6; k++) dout.*stats[k] = HostIO::at<double>(base, o_st[k]);
        dout.S_PLUS = HostIO::at<double>(base, o_sp); dout.S_SMOOTH = HostIO::at<double>(base, o_ss);
        dout.status = HostIO::at<int32_t>(base, o_status);
        return la_enqueue(d, &din, &dout, base + o_ws, wsb, path_hint, st, err);
    };
    return with_ctx(device, err, [&](HostCtx *cx) { return run_call(cx, io, d->placement_tries, nullptr, err, enqueue); });
}

// ---- the sliding-window growth-rate estimators (Tools/Rt_ExpFitLogLinReg.m, Rt_ExpFitGenRatios.m, Rt_ExpFitNonlinLS.m) ----
int epi_rtwin_validate(const epi_rtwin_desc *d, const double *new_cases, const epi_rtwin_outputs *out, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->R < 1 || d->L < 1) { set_err(err, "R and L must be >= 1"); return EPI_ERR_BAD_ARG; }
    if ((int64_t)d->R * d->L > (int64_t)0x7fffffff) { set_err(err, "R * L is limited to 2^31 - 1"); return EPI_ERR_BAD_ARG; }
    if (d->methods == 0) { set_err(err, "methods is empty: ask for LogLinReg (1), GenRatios (2) and / or NonlinLS (4)"); return EPI_ERR_BAD_ARG; }
    if (d->methods & ~(EPI_RTWIN_LOGLINREG | EPI_RTWIN_GENRATIOS | EPI_RTWIN_NONLINLS)) { set_err(err, "unknown method bit"); return EPI_ERR_BAD_ARG; }
    if (d->causal != 0 && d->causal != 1) { set_err(err, "causal must be 0 or 1"); return EPI_ERR_BAD_ARG; }
    if ((d->methods & EPI_RTWIN_GENRATIOS) && (d->generation_period < 1 || d->generation_period > d->L)) {
        set_err(err, "generation_period must lie in 1 .. L"); return EPI_ERR_BAD_ARG;
    }
    if (!new_cases || !out) { set_err(err, "NULL new_cases / outputs"); return EPI_ERR_BAD_ARG; }
    if (d->wlen < 2 || d->wlen > kRtwMaxSamples) {
        set_err(err, "wlen is limited to 2 .. 31 (a window is held in registers)"); return EPI_ERR_UNSUPPORTED;
    }
    return EPI_OK;
}

static RtwArgs rtw_args(const epi_rtwin_desc *d, const double *x, const epi_rtwin_outputs *o)
{
    RtwArgs a{};
    a.R = d->R; a.L = d->L; a.wlen = d->wlen; a.causal = d->causal; a.gp = d->generation_period;
    const int h = d->wlen / 2;
    a.nw = d->causal ? d->wlen : 2 * h + 1;
    a.off = d->causal ? -(d->wlen - 1) : -h;
    a.lo = -a.off;
    a.hi = d->L - (a.nw - 1 + a.off);
    a.time_unit = d->time_unit;
    double sn = 0.0, sn2 = 0.0;
    for (int i = 0; i < a.nw; i++) {
        a.n[i] = (double)(i + a.off);
        a.t[i] = a.n[i] / d->time_unit;
        sn = sn + a.n[i];
        sn2 = sn2 + a.n[i] * a.n[i];
    }
    a.En = sn / (double)a.nw; a.En2 = sn2 / (double)a.nw;
    a.Det = a.En2 - a.En * a.En;
    a.c_ma = 1.0 / (double)d->wlen;
    a.x = x;
    a.llr_Rt = o->llr_Rt; a.llr_A = o->llr_A; a.llr_Lambda = o->llr_Lambda; a.llr_ExpFit = o->llr_ExpFit;
    a.gr_Rt = o->gr_Rt; a.gr_Lambda = o->gr_Lambda; a.gr_RtSmoothed = o->gr_RtSmoothed; a.gr_LambdaSmoothed = o->gr_LambdaSmoothed;
    a.nls_Rt = o->nls_Rt; a.nls_A = o->nls_A; a.nls_Lambda = o->nls_Lambda; a.nls_ExpFit = o->nls_ExpFit;
    a.nls_status = o->nls_status; a.nls_iters = o->nls_iters;
    return a;
}

int epi_rtwin_run_device(const epi_rtwin_desc *d, const double *new_cases, const epi_rtwin_outputs *out, void *stream, char *err)
{
    int rc = epi_rtwin_validate(d, new_cases, out, err);
    if (rc != EPI_OK) return rc;
    const RtwArgs a = rtw_args(d, new_cases, out);
    hipStream_t st = (hipStream_t)stream;
    const int64_t n = (int64_t)d->L * d->R;
    hipError_t e;
    if ((d->methods & EPI_RTWIN_LOGLINREG) && (a.llr_Rt || a.llr_A || a.llr_Lambda || a.llr_ExpFit)) {
        hipLaunchKernelGGL(rtw_loglin, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "rtw_loglin launch");
    }
    if ((d->methods & EPI_RTWIN_GENRATIOS) && (a.gr_Rt || a.gr_Lambda || a.gr_RtSmoothed || a.gr_LambdaSmoothed)) {
        hipLaunchKernelGGL(rtw_genratios, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "rtw_genratios launch");
    }
    if ((d->methods & EPI_RTWIN_NONLINLS) &&
        (a.nls_Rt || a.nls_A || a.nls_Lambda || a.nls_ExpFit || a.nls_status || a.nls_iters)) {
        const size_t lds = (size_t)4 * a.nw * 64 * sizeof(double);
        hipLaunchKernelGGL(rtw_nonlin, dim3((unsigned)((n + 63) / 64)), dim3(64), lds, st, a);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "rtw_nonlin launch");
    }
    return EPI_OK;
}

int epi_rtwin_run_host(const epi_rtwin_desc *d, const double *new_cases, const epi_rtwin_outputs *out, int device, char *err)
{
    int rc = epi_rtwin_validate(d, new_cases, out, err);
    if (rc != EPI_OK) return rc;
    const size_t R = (size_t)d->R, T = (size_t)d->L;
    HostIO io;
    const size_t o_x = io.add_in(new_cases, T, 8, R, 0, R);
    using RO = epi_rtwin_outputs;
    const HostIO::Opt<RO, double> f64[12] = {{&RO::llr_Rt, T}, {&RO::llr_A, T}, {&RO::llr_Lambda, T}, {&RO::llr_ExpFit, T},
                                             {&RO::gr_Rt, T}, {&RO::gr_Lambda, T}, {&RO::gr_RtSmoothed, T}, {&RO::gr_LambdaSmoothed, T},
                                             {&RO::nls_Rt, T}, {&RO::nls_A, T}, {&RO::nls_Lambda, T}, {&RO::nls_ExpFit, T}};
    const HostIO::Opt<RO, int32_t> i32[2] = {{&RO::nls_status, T}, {&RO::nls_iters, T}};
    size_t o_f[12], o_i[2];
    io.add_opt(*out, f64, o_f, R);
    io.add_opt(*out, i32, o_i, R);
    auto enqueue = [&](char *base, hipStream_t st) {
        epi_rtwin_outputs dout{};
        HostIO::bind_opt(dout, f64, o_f, base);
        HostIO::bind_opt(dout, i32, o_i, base);
        return epi_rtwin_run_device(d, (const double *)(base + o_x), &dout, st, err);
    };
    return run_host(device, io, err, enqueue);
}

// ---- REGRESSION_TYPE = 'LASSO': lasso(X, y, 'CV', K) per region (TrainPredictPrescribeNPI.m:254-290) ----
int epi_lasso_validate(const epi_lasso_desc *d, const double *X, const double *y, const int32_t *fold,
                       const epi_lasso_outputs *out, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->R < 1) { set_err(err, "R must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->D < 2) { set_err(err, "D must be >= 2"); return EPI_ERR_BAD_ARG; }
    if (d->n < 1) { set_err(err, "n must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->num_lambda < 1) { set_err(err, "num_lambda must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->K < 0 || d->K == 1) { set_err(err, "K must be 0 (path only) or >= 2"); return EPI_ERR_BAD_ARG; }
    if (d->K > d->D) { set_err(err, "K must not exceed D (every fold needs a day)"); return EPI_ERR_BAD_ARG; }
    if (!(d->lambda_ratio > 0.0 && d->lambda_ratio < 1.0)) { set_err(err, "lambda_ratio must lie in (0, 1)"); return EPI_ERR_BAD_ARG; }
    if (!(d->rel_tol > 0.0 && d->rel_tol <= 1.7976931348623157e308)) { set_err(err, "rel_tol must be > 0 and finite"); return EPI_ERR_BAD_ARG; }
    if (d->max_iter < 1) { set_err(err, "max_iter must be >= 1"); return EPI_ERR_BAD_ARG; }
    if ((int64_t)d->R * d->D * d->n > (int64_t)0x7fffffff) { set_err(err, "R * D * n is limited to 2^31 - 1"); return EPI_ERR_BAD_ARG; }
    if (!X || !y || !out) { set_err(err, "NULL X / y / outputs"); return EPI_ERR_BAD_ARG; }
    if (d->K >= 2 && !fold) { set_err(err, "NULL fold (K >= 2)"); return EPI_ERR_BAD_ARG; }
    if (!out->status) { set_err(err, "NULL status output"); return EPI_ERR_BAD_ARG; }
    if (d->K >= 2 && (!out->a || !out->b)) { set_err(err, "NULL a / b output (K >= 2)"); return EPI_ERR_BAD_ARG; }
    if (d->n > kLsMaxN) { set_err(err, "n is limited to 12"); return EPI_ERR_UNSUPPORTED; }
    if (d->D > kLsMaxD) { set_err(err, "D is limited to 256 (a region's window and residuals are held in LDS)"); return EPI_ERR_UNSUPPORTED; }
    if (d->K > kLsMaxK) { set_err(err, "K is limited to 63 (the folds and the full fit share one wavefront)"); return EPI_ERR_UNSUPPORTED; }
    if (d->num_lambda > kLsMaxNL) { set_err(err, "num_lambda is limited to 100"); return EPI_ERR_UNSUPPORTED; }
    return EPI_OK;
}

int epi_lasso_run_device(const epi_lasso_desc *d, const double *X, const double *y, const int32_t *fold,
                         const epi_lasso_outputs *out, void *stream, char *err)
{
    int rc = epi_lasso_validate(d, X, y, fold, out, err);
    if (rc != EPI_OK) return rc;
    LsArgs g{};
    g.R = d->R; g.D = d->D; g.n = d->n; g.K = d->K; g.NL = d->num_lambda; g.max_iter = d->max_iter;
    g.ratio = d->lambda_ratio; g.rel_tol = d->rel_tol;
    g.X = X; g.y = y; g.fold = fold;
    g.a = out->a; g.b = out->b; g.lambda = out->lambda; g.B = out->B; g.intercept = out->intercept; g.mse = out->mse; g.se = out->se;
    g.df = out->df; g.iters = out->iters; g.idx_min = out->idx_min_mse; g.idx_1se = out->idx_1se; g.status = out->status;
    const size_t shmem = lasso_lds_bytes(d->D, d->n, d->num_lambda);
    hipError_t e = hipFuncSetAttribute((const void *)lasso_cv, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem);
    if (e != hipSuccess) return hip_fail(err, e, "hipFuncSetAttribute");
    for (int64_t r0 = 0; r0 < d->R; r0 += kLsLaunchRegions) {    // one 64-lane workgroup per region, in slices (lasso.hpp)
        g.r0 = (int)r0;
        const int64_t nr = d->R - r0 < kLsLaunchRegions ? d->R - r0 : kLsLaunchRegions;
        hipLaunchKernelGGL(lasso_cv, dim3((unsigned)nr), dim3(64), shmem, (hipStream_t)stream, g);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "lasso_cv launch");
    }
    return EPI_OK;
}

int epi_lasso_run_host(const epi_lasso_desc *d, const double *X, const double *y, const int32_t *fold,
                       const epi_lasso_outputs *out, int device, char *err)
{
    int rc = epi_lasso_validate(d, X, y, fold, out, err);
    if (rc != EPI_OK) return rc;
    const size_t R = (size_t)d->R, D = (size_t)d->D, n = (size_t)d->n, NL = (size_t)d->num_lambda;
    if (d->K >= 2) {                     // the partition is on the host here: an argument error, not a region status
        std::vector<int> cnt((size_t)d->K);
        for (size_t r = 0; r < R; r++) {
            std::fill(cnt.begin(), cnt.end(), 0);
            for (size_t i = 0; i < D; i++) {
                const int32_t f = fold[i * R + r];
                if (f < 0 || f >= d->K) { set_err(err, "fold value outside 0 .. K-1"); return EPI_ERR_BAD_ARG; }
                cnt[(size_t)f]++;
            }
            for (int f = 0; f < d->K; f++)
                if (cnt[(size_t)f] == 0) { set_err(err, "empty fold"); return EPI_ERR_BAD_ARG; }
        }
    }
    HostIO io;
    const size_t o_X = io.add_in(X, D * n, 8, R, 0, R), o_y = io.add_in(y, D, 8, R, 0, R);
    const size_t o_f = d->K >= 2 ? io.add_in(fold, D, 4, R, 0, R) : HostIO::kAbsent;
    using LO = epi_lasso_outputs;
    const HostIO::Opt<LO, double> f64[7] = {{&LO::a, n}, {&LO::b, 1}, {&LO::lambda, NL}, {&LO::B, NL * n}, {&LO::intercept, NL},
                                            {&LO::mse, NL}, {&LO::se, NL}};
    const HostIO::Opt<LO, int32_t> i32[5] = {{&LO::df, NL}, {&LO::iters, NL}, {&LO::idx_min_mse, 1}, {&LO::idx_1se, 1}, {&LO::status, 1}};
    size_t o_d[7], o_i[5];
    io.add_opt(*out, f64, o_d, R);
    io.add_opt(*out, i32, o_i, R);
    auto enqueue = [&](char *base, hipStream_t st) {
        epi_lasso_outputs dout{};
        HostIO::bind_opt(dout, f64, o_d, base);
        HostIO::bind_opt(dout, i32, o_i, base);
        return epi_lasso_run_device(d, (const double *)(base + o_X), (const double *)(base + o_y), HostIO::at<const int32_t>(base, o_f),
                                    &dout, st, err);
    };
    return run_host(device, io, err, enqueue);
}

// ---- REGRESSION_TYPE = 'NONNEGATIVELS-ELEMENT-WISE': a robust bounded affine fit per (NPI, region) (TrainPredictPrescribeNPI.m:279-292) ----
int epi_robfit_validate(const epi_robfit_desc *d, const double *X, const double *y, const epi_robfit_outputs *out, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->R < 1) { set_err(err, "R must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->D < 3) { set_err(err, "D must be >= 3"); return EPI_ERR_BAD_ARG; }
    if (d->n < 1) { set_err(err, "n must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->robust != 0 && d->robust != 1) { set_err(err, "robust must be 0 or 1"); return EPI_ERR_BAD_ARG; }
    if (d->max_iter < 1 || d->max_iter > 100000) { set_err(err, "max_iter must lie in 1 .. 100000"); return EPI_ERR_BAD_ARG; }
    if (d->lower_a != d->lower_a || d->upper_a != d->upper_a) { set_err(err, "lower_a / upper_a must not be NaN"); return EPI_ERR_BAD_ARG; }
    if (d->lower_a > d->upper_a) { set_err(err, "lower_a must not exceed upper_a"); return EPI_ERR_BAD_ARG; }
    if ((int64_t)d->R * d->D * d->n > (int64_t)0x7fffffff) { set_err(err, "R * D * n is limited to 2^31 - 1"); return EPI_ERR_BAD_ARG; }
    if (!X || !y || !out) { set_err(err, "NULL X / y / outputs"); return EPI_ERR_BAD_ARG; }
    if (!out->a && !out->b_item && !out->sigma && !out->iters && !out->status && !out->weights && !out->b) { set_err(err, "every output is NULL"); return EPI_ERR_BAD_ARG; }
    if (d->n > kRfMaxN) { set_err(err, "n is limited to 12"); return EPI_ERR_UNSUPPORTED; }
    if (d->D > kRfMaxD) { set_err(err, "D is limited to 1024 (a wavefront holds an item's days in registers)"); return EPI_ERR_UNSUPPORTED; }
    return EPI_OK;
}

static hipError_t rf_dispatch(const RfArgs &g, unsigned blocks, bool intercept, hipStream_t st)
{
    if (g.D <= 64) return rf_launch<1>(g, blocks, intercept, st);   // registers per lane: P / 64, P the power of two >= D
    if (g.D <= 128) return rf_launch<2>(g, blocks, intercept, st);
    if (g.D <= 256) return rf_launch<4>(g, blocks, intercept, st);
    if (g.D <= 512) return rf_launch<8>(g, blocks, intercept, st);
    return rf_launch<16>(g, blocks, intercept, st);
}

int epi_robfit_run_device(const epi_robfit_desc *d, const double *X, const double *y, const epi_robfit_outputs *out,
                          void *stream, char *err)
{
    int rc = epi_robfit_validate(d, X, y, out, err);
    if (rc != EPI_OK) return rc;
    RfArgs g{};
    g.R = d->R; g.D = d->D; g.n = d->n; g.robust = d->robust; g.max_iter = d->max_iter; g.lower = d->lower_a; g.upper = d->upper_a;
    g.X = X; g.y = y;
    g.a = out->a; g.b_item = out->b_item; g.sigma = out->sigma; g.iters = out->iters; g.status = out->status;
    g.weights = out->weights; g.b = out->b;
    const hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (out->a || out->b_item || out->sigma || out->iters || out->status || out->weights) {
        const int64_t items = (int64_t)d->n * d->R;
        e = for_slices(items, kRfLaunchItems, [&](int64_t i0, unsigned ni) {    // one 64-lane workgroup per item, in slices (robust_fit.hpp)
            g.item0 = (long long)i0;
            return rf_dispatch(g, ni, false, st);
        });
        if (e != hipSuccess) return hip_fail(err, e, "robfit_items launch");
    }
    if (out->b) {
        e = for_slices(d->R, kRfLaunchItems, [&](int64_t r0, unsigned nr) {     // one 64-lane workgroup per region, behind the items
            g.item0 = (long long)r0;
            return rf_dispatch(g, nr, true, st);
        });
        if (e != hipSuccess) return hip_fail(err, e, "robfit_intercept launch");
    }
    return EPI_OK;
}

int epi_robfit_run_host(const epi_robfit_desc *d, const double *X, const double *y, const epi_robfit_outputs *out,
                        int device, char *err)
{
    int rc = epi_robfit_validate(d, X, y, out, err);
    if (rc != EPI_OK) return rc;
    const size_t R = (size_t)d->R, D = (size_t)d->D, n = (size_t)d->n;
    HostIO io;
    const size_t o_X = io.add_in(X, D * n, 8, R, 0, R), o_y = io.add_in(y, D, 8, R, 0, R);
    using RO = epi_robfit_outputs;
    const HostIO::Opt<RO, double> f64[5] = {{&RO::a, n}, {&RO::b_item, n}, {&RO::sigma, n}, {&RO::weights, D * n}, {&RO::b, 1}};
    const HostIO::Opt<RO, int32_t> i32[2] = {{&RO::iters, n}, {&RO::status, n}};
    size_t o_d[5], o_i[2];
    io.add_opt(*out, f64, o_d, R);
    io.add_opt(*out, i32, o_i, R);
    auto enqueue = [&](char *base, hipStream_t st) {
        epi_robfit_outputs dout{};
        HostIO::bind_opt(dout, f64, o_d, base);
        HostIO::bind_opt(dout, i32, o_i, base);
        return epi_robfit_run_device(d, (const double *)(base + o_X), (const double *)(base + o_y), &dout, st, err);
    };
    return run_host(device, io, err, enqueue);
}

// ---- the NPI-to-growth-rate predictor per (train end, region) (test04FullFeatureExtMLpipeline.m:292-404, :418-431, :576-642) ----
int epi_ratemap_validate(const epi_ratemap_desc *d, const epi_ratemap_inputs *in, const epi_ratemap_outputs *out, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->T < 1) { set_err(err, "T must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->n < 1) { set_err(err, "n must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->R < 1) { set_err(err, "R must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->E < 0) { set_err(err, "E must be >= 0"); return EPI_ERR_BAD_ARG; }
    if (d->K < 1) { set_err(err, "K must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->n_lags < 0) { set_err(err, "n_lags must be >= 0"); return EPI_ERR_BAD_ARG; }
    if (d->fit != 0 && d->fit != 1) { set_err(err, "fit must be 0 or 1"); return EPI_ERR_BAD_ARG; }
    if (d->effect_lag < 0) { set_err(err, "effect_lag must be >= 0"); return EPI_ERR_BAD_ARG; }
    if (!(d->ridge >= 0.0) || d->ridge == (double)INFINITY) { set_err(err, "ridge must be finite and >= 0"); return EPI_ERR_BAD_ARG; }
    if (!(d->lambda_threshold >= 0.0)) { set_err(err, "lambda_threshold must be >= 0"); return EPI_ERR_BAD_ARG; }
    if (!(fabs(d->reduction_effect) < (double)INFINITY)) { set_err(err, "reduction_effect must be finite"); return EPI_ERR_BAD_ARG; }
    if (d->n > kRmMaxN) { set_err(err, "n is limited to 24"); return EPI_ERR_UNSUPPORTED; }
    if (d->n_lags > kRmMaxLags) { set_err(err, "n_lags is limited to 3"); return EPI_ERR_UNSUPPORTED; }
    if (d->E > kRmMaxE) { set_err(err, "E is limited to 8"); return EPI_ERR_UNSUPPORTED; }
    const int64_t F = (int64_t)d->n * (1 + d->n_lags) + d->E;
    if (F > kRmMaxF) { set_err(err, "F = n (1 + n_lags) + E is limited to 96 (the triangle of G is factored in LDS)"); return EPI_ERR_UNSUPPORTED; }
    for (int l = 0; l < d->n_lags; l++)
        if (d->lags[l] < 1 || d->lags[l] >= d->T) { set_err(err, "every lag must lie in 1 .. T - 1"); return EPI_ERR_BAD_ARG; }
    const int64_t lim = (int64_t)1 << 31, T = d->T, R = d->R, K = d->K;
    if (K * R >= lim) { set_err(err, "K * R must stay below 2^31"); return EPI_ERR_BAD_ARG; }
    if (T * d->n * R >= lim || T * d->E * R >= lim || K * F * R >= lim || (double)K * (double)T * (double)R >= (double)lim) {
        set_err(err, "every array's element count must stay below 2^31"); return EPI_ERR_BAD_ARG;
    }
    if (!in || !out) { set_err(err, "NULL inputs / outputs"); return EPI_ERR_BAD_ARG; }
    if (!in->ip || !in->new_smoothed || !in->n_train) { set_err(err, "NULL ip / new_smoothed / n_train"); return EPI_ERR_BAD_ARG; }
    if (d->E > 0 && !in->extra) { set_err(err, "E > 0 needs extra"); return EPI_ERR_BAD_ARG; }
    if (d->fit && !in->y) { set_err(err, "fit = 1 needs y"); return EPI_ERR_BAD_ARG; }
    if (!d->fit && !in->lambda_in) { set_err(err, "fit = 0 needs lambda_in"); return EPI_ERR_BAD_ARG; }
    if (!out->map && !out->x_mx && !out->y_filled && !out->lambda_hat && !out->new_cases_est && !out->tracker && !out->status) {
        set_err(err, "every output is NULL"); return EPI_ERR_BAD_ARG;
    }
    if (!d->fit && out->map) { set_err(err, "map needs fit = 1"); return EPI_ERR_BAD_ARG; }
    if (out->y_filled && !in->y) { set_err(err, "y_filled needs y"); return EPI_ERR_BAD_ARG; }
    for (int k = 0; k < d->K; k++)
        if (in->n_train[k] < 1 || in->n_train[k] > d->T) { set_err(err, "every n_train must lie in 1 .. T"); return EPI_ERR_BAD_ARG; }
    return EPI_OK;
}

static hipError_t rm_dispatch(const RmArgs &g, unsigned blocks, hipStream_t st)
{
    const int per_lane = ((g.F + 1) * (g.F + 2) / 2 - 1 + kRmThreads - 1) / kRmThreads;    // entries of G and c a lane owns
    if (!g.fit || per_lane <= 1) return rm_launch_items<1>(g, blocks, st);
    if (per_lane <= 2) return rm_launch_items<2>(g, blocks, st);
    if (per_lane <= 5) return rm_launch_items<5>(g, blocks, st);
    if (per_lane <= 10) return rm_launch_items<10>(g, blocks, st);
    return rm_launch_items<19>(g, blocks, st);
}

int epi_ratemap_run_device(const epi_ratemap_desc *d, const epi_ratemap_inputs *in, const epi_ratemap_outputs *out,
                           void *stream, char *err)
{
    int rc = epi_ratemap_validate(d, in, out, err);
    if (rc != EPI_OK) return rc;
    RmArgs g{};
    g.T = d->T; g.n = d->n; g.R = d->R; g.E = d->E; g.n_lags = d->n_lags; g.fit = d->fit; g.effect_lag = d->effect_lag;
    g.F = d->n * (1 + d->n_lags) + d->E;
    for (int l = 0; l < d->n_lags; l++) g.lags[l] = d->lags[l];
    g.ridge = d->ridge; g.thr = d->lambda_threshold; g.red = d->reduction_effect;
    g.ip = in->ip; g.y = in->y; g.ns = in->new_smoothed; g.extra = in->extra; g.lambda_in = in->lambda_in;
    g.map = out->map; g.x_mx = out->x_mx; g.y_filled = out->y_filled; g.lambda_hat = out->lambda_hat; g.est = out->new_cases_est;
    g.tracker = out->tracker; g.status = out->status;
    const hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    if (out->x_mx || out->y_filled || out->tracker) {
        e = for_slices(d->R, kRmLaunchItems, [&](int64_t r0, unsigned nr) {     // one workgroup per region
            g.item0 = (long long)r0;
            hipLaunchKernelGGL(ratemap_region, dim3(nr), dim3(kRmThreads), 0, st, g);
            return hipGetLastError();
        });
        if (e != hipSuccess) return hip_fail(err, e, "ratemap_region launch");
    }
    if (out->map || out->lambda_hat || out->new_cases_est || out->status) {
        for (int k0 = 0; k0 < d->K; k0 += kRmTrainEnds) {              // a launch carries up to 64 train ends by value
            const int kc = copy_counts(g.nt, in->n_train, k0, d->K);
            g.k0 = k0;
            e = for_slices((int64_t)kc * d->R, kRmLaunchItems, [&](int64_t i0, unsigned ni) {   // one workgroup per item, in slices (rate_map.hpp)
                g.item0 = (long long)i0;
                return rm_dispatch(g, ni, st);
            });
            if (e != hipSuccess) return hip_fail(err, e, "ratemap_items launch");
        }
    }
    return EPI_OK;
}

int epi_ratemap_run_host(const epi_ratemap_desc *d, const epi_ratemap_inputs *in, const epi_ratemap_outputs *out,
                         int device, char *err)
{
    int rc = epi_ratemap_validate(d, in, out, err);
    if (rc != EPI_OK) return rc;
    const size_t T = (size_t)d->T, n = (size_t)d->n, R = (size_t)d->R, E = (size_t)d->E, K = (size_t)d->K;
    const size_t F = n * (size_t)(1 + d->n_lags) + E, none = HostIO::kAbsent;
    HostIO io;
    const size_t o_ip = io.add_in(in->ip, T * n, 8, R, 0, R), o_ns = io.add_in(in->new_smoothed, T, 8, R, 0, R);
    const size_t o_y = in->y ? io.add_in(in->y, T, 8, R, 0, R) : none;
    const size_t o_ex = d->E > 0 ? io.add_in(in->extra, T * E, 8, R, 0, R) : none;
    const size_t o_li = d->fit ? none : io.add_in(in->lambda_in, K * T, 8, R, 0, R);
    using MO = epi_ratemap_outputs;
    const HostIO::Opt<MO, double> f64[6] = {{&MO::map, K * F}, {&MO::x_mx, F}, {&MO::y_filled, T}, {&MO::lambda_hat, K * T},
                                            {&MO::new_cases_est, K * T}, {&MO::tracker, T}};
    const HostIO::Opt<MO, int32_t> i32[1] = {{&MO::status, K}};
    size_t o_d[6], o_i[1];
    io.add_opt(*out, f64, o_d, R);
    io.add_opt(*out, i32, o_i, R);
    auto enqueue = [&](char *base, hipStream_t st) {
        epi_ratemap_inputs din{};
        din.ip = (const double *)(base + o_ip); din.new_smoothed = (const double *)(base + o_ns);
        din.y = HostIO::at<const double>(base, o_y); din.extra = HostIO::at<const double>(base, o_ex);
        din.lambda_in = HostIO::at<const double>(base, o_li);
        din.n_train = in->n_train;                                     // host memory in both entry points
        epi_ratemap_outputs dout{};
        HostIO::bind_opt(dout, f64, o_d, base);
        HostIO::bind_opt(dout, i32, o_i, base);
        return epi_ratemap_run_device(d, &din, &dout, st, err);
    };
    return run_host(device, io, err, enqueue);
}

// ---- MATLAB's rectangular backslash per (row count, region) (test01FitExponential.m:159, test03 :169, test05 :185) ----
int epi_mldiv_validate(const epi_mldiv_desc *d, const epi_mldiv_inputs *in, const epi_mldiv_outputs *out, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->D < 1) { set_err(err, "D must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->F < 1) { set_err(err, "F must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->R < 1) { set_err(err, "R must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->K < 1) { set_err(err, "K must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (!(d->tol_scale >= 0.0) || d->tol_scale == (double)INFINITY) { set_err(err, "tol_scale must be finite and >= 0"); return EPI_ERR_BAD_ARG; }
    if (d->F > kMlMaxF) { set_err(err, "F is limited to 96"); return EPI_ERR_UNSUPPORTED; }
    const int64_t lim = (int64_t)1 << 31, D = d->D, F = d->F, R = d->R, K = d->K;
    if (K * R >= lim) { set_err(err, "K * R must stay below 2^31"); return EPI_ERR_BAD_ARG; }
    if (D * F * R >= lim || K * F * R >= lim || (double)K * (double)D * (double)R >= (double)lim) {
        set_err(err, "every array's element count must stay below 2^31"); return EPI_ERR_BAD_ARG;
    }
    if (!in || !out) { set_err(err, "NULL inputs / outputs"); return EPI_ERR_BAD_ARG; }
    if (!in->X || !in->y || !in->n_rows) { set_err(err, "NULL X / y / n_rows"); return EPI_ERR_BAD_ARG; }
    if (!out->m && !out->rank && !out->perm && !out->rdiag && !out->resid && !out->fitted && !out->status) {
        set_err(err, "every output is NULL"); return EPI_ERR_BAD_ARG;
    }
    for (int k = 0; k < d->K; k++)
        if (in->n_rows[k] < 1 || in->n_rows[k] > d->D) { set_err(err, "every n_rows must lie in 1 .. D"); return EPI_ERR_BAD_ARG; }
    for (int k = 0; k < d->K; k++)
        if ((int64_t)in->n_rows[k] * (F + 1) > kMlMaxElems) {
            set_err(err, "max(n_rows) * (F + 1) is limited to 20000 (the item's matrix is factored in LDS)"); return EPI_ERR_UNSUPPORTED;
        }
    return EPI_OK;
}

int epi_mldiv_run_device(const epi_mldiv_desc *d, const epi_mldiv_inputs *in, const epi_mldiv_outputs *out,
                         void *stream, char *err)
{
    int rc = epi_mldiv_validate(d, in, out, err);
    if (rc != EPI_OK) return rc;
    MlArgs g{};
    g.D = d->D; g.F = d->F; g.R = d->R; g.tol_scale = d->tol_scale;
    g.X = in->X; g.y = in->y;
    g.m = out->m; g.rank = out->rank; g.perm = out->perm; g.rdiag = out->rdiag; g.resid = out->resid; g.fitted = out->fitted;
    g.status = out->status;
    const hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    for (int k0 = 0; k0 < d->K; k0 += kMlRowCounts) {                  // a launch carries up to 64 row counts by value
        const int kc = copy_counts(g.nr, in->n_rows, k0, d->K);
        g.k0 = k0;
        int nmax = 1;
        for (int kk = 0; kk < kc; kk++) nmax = g.nr[kk] > nmax ? g.nr[kk] : nmax;
        const size_t shm = ml_lds_bytes(nmax, d->F);
        if (shm > 64u * 1024u &&        // above the default dynamic-LDS limit
            (e = hipFuncSetAttribute((const void *)mldivide_items, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm)) != hipSuccess)
            return hip_fail(err, e, "hipFuncSetAttribute");
        e = for_slices((int64_t)kc * d->R, kMlLaunchItems, [&](int64_t i0, unsigned ni) {       // one workgroup per item, in slices (mldivide.hpp)
            g.item0 = (long long)i0;
            hipLaunchKernelGGL(mldivide_items, dim3(ni), dim3(kMlThreads), shm, st, g);
            return hipGetLastError();
        });
        if (e != hipSuccess) return hip_fail(err, e, "mldivide_items launch");
    }
    return EPI_OK;
}

int epi_mldiv_run_host(const epi_mldiv_desc *d, const epi_mldiv_inputs *in, const epi_mldiv_outputs *out,
                       int device, char *err)
{
    int rc = epi_mldiv_validate(d, in, out, err);
    if (rc != EPI_OK) return rc;
    const size_t D = (size_t)d->D, F = (size_t)d->F, R = (size_t)d->R, K = (size_t)d->K;
    HostIO io;
    const size_t o_X = io.add_in(in->X, D * F, 8, R, 0, R), o_y = io.add_in(in->y, D, 8, R, 0, R);
    using MO = epi_mldiv_outputs;
    const HostIO::Opt<MO, double> f64[4] = {{&MO::m, K * F}, {&MO::rdiag, K * F}, {&MO::resid, K}, {&MO::fitted, K * D}};
    const HostIO::Opt<MO, int32_t> i32[3] = {{&MO::rank, K}, {&MO::perm, K * F}, {&MO::status, K}};
    size_t o_d[4], o_i[3];
    io.add_opt(*out, f64, o_d, R);
    io.add_opt(*out, i32, o_i, R);
    auto enqueue = [&](char *base, hipStream_t st) {
        epi_mldiv_inputs din{};
        din.X = (const double *)(base + o_X); din.y = (const double *)(base + o_y);
        din.n_rows = in->n_rows;                                       // host memory in both entry points
        epi_mldiv_outputs dout{};
        HostIO::bind_opt(dout, f64, o_d, base);
        HostIO::bind_opt(dout, i32, o_i, base);
        return epi_mldiv_run_device(d, &din, &dout, st, err);
    };
    return run_host(device, io, err, enqueue);
}

// ---- support-vector regression per (row count, region) (test05DirectNewCasesLearning.m:198-268, test04 :435-445, test03 :242-262) ----
int epi_svr_validate(const epi_svr_desc *d, const epi_svr_inputs *in, const epi_svr_outputs *out, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->D < 1) { set_err(err, "D must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->F < 1) { set_err(err, "F must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->R < 1) { set_err(err, "R must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->K < 1) { set_err(err, "K must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->kernel != EPI_SVR_LINEAR && d->kernel != EPI_SVR_GAUSSIAN) { set_err(err, "kernel must be EPI_SVR_LINEAR or EPI_SVR_GAUSSIAN"); return EPI_ERR_BAD_ARG; }
    if (d->max_iter < 1 || d->max_iter > 10000000) { set_err(err, "max_iter must lie in 1 .. 10000000"); return EPI_ERR_BAD_ARG; }
    if (!(d->tol > 0.0) || d->tol == (double)INFINITY) { set_err(err, "tol must be finite and > 0"); return EPI_ERR_BAD_ARG; }
    if (d->F > kSvMaxF) { set_err(err, "F is limited to 96"); return EPI_ERR_UNSUPPORTED; }
    const int64_t lim = (int64_t)1 << 31, D = d->D, F = d->F, R = d->R, K = d->K;
    if (K * R >= lim) { set_err(err, "K * R must stay below 2^31"); return EPI_ERR_BAD_ARG; }
    if (D * F * R >= lim || K * F * R >= lim || (double)K * (double)D * (double)R >= (double)lim) {
        set_err(err, "every array's element count must stay below 2^31"); return EPI_ERR_BAD_ARG;
    }
    if (!in || !out) { set_err(err, "NULL inputs / outputs"); return EPI_ERR_BAD_ARG; }
    if (!in->X || !in->y || !in->n_rows) { set_err(err, "NULL X / y / n_rows"); return EPI_ERR_BAD_ARG; }
    if (!in->box || !in->epsilon || !in->kernel_scale) { set_err(err, "NULL box / epsilon / kernel_scale"); return EPI_ERR_BAD_ARG; }
    if (!out->beta && !out->bias && !out->w && !out->fitted && !out->n_iter && !out->gap && !out->n_sv && !out->status) {
        set_err(err, "every output is NULL"); return EPI_ERR_BAD_ARG;
    }
    if (out->w && d->kernel != EPI_SVR_LINEAR) { set_err(err, "w exists for the linear kernel only"); return EPI_ERR_BAD_ARG; }
    for (int k = 0; k < d->K; k++)
        if (in->n_rows[k] < 1 || in->n_rows[k] > d->D) { set_err(err, "every n_rows must lie in 1 .. D"); return EPI_ERR_BAD_ARG; }
    for (int k = 0; k < d->K; k++) {
        if (in->n_rows[k] > kSvMaxRows) { set_err(err, "n_rows is limited to 1024 (four rows a lane)"); return EPI_ERR_UNSUPPORTED; }
        if ((int64_t)in->n_rows[k] * ((F | 1) + 1) > kSvMaxElems) {
            set_err(err, "max(n_rows) * ((F | 1) + 1) is limited to 20000 (the item's rows stay in LDS)"); return EPI_ERR_UNSUPPORTED;
        }
    }
    return EPI_OK;
}

int epi_svr_run_device(const epi_svr_desc *d, const epi_svr_inputs *in, const epi_svr_outputs *out,
                       void *stream, char *err)
{
    int rc = epi_svr_validate(d, in, out, err);
    if (rc != EPI_OK) return rc;
    SvArgs g{};
    g.D = d->D; g.F = d->F; g.R = d->R; g.max_iter = d->max_iter; g.tol = d->tol;
    g.X = in->X; g.y = in->y; g.box = in->box; g.eps = in->epsilon; g.scale = in->kernel_scale;
    g.beta = out->beta; g.bias = out->bias; g.w = out->w; g.fitted = out->fitted; g.gap = out->gap;
    g.n_iter = out->n_iter; g.n_sv = out->n_sv; g.status = out->status;
    const bool gau = d->kernel == EPI_SVR_GAUSSIAN;
    const hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    for (int k0 = 0; k0 < d->K; k0 += kSvRowCounts) {                  // a launch carries up to 64 row counts by value
        const int kc = copy_counts(g.nr, in->n_rows, k0, d->K);
        g.k0 = k0;
        int nmax = 1, nmin = d->D;
        for (int kk = 0; kk < kc; kk++) {
            nmax = g.nr[kk] > nmax ? g.nr[kk] : nmax;
            nmin = g.nr[kk] < nmin ? g.nr[kk] : nmin;
        }
        const size_t doubles = sv_lds_doubles(nmax, nmin, d->D, d->F, gau);
        g.lds = (int)doubles;
        e = for_slices((int64_t)kc * d->R, kSvLaunchItems, [&](int64_t i0, unsigned ni) {       // one workgroup per item, in slices (svr.hpp)
            g.item0 = (long long)i0;
            return gau ? sv_dispatch<true>(g, nmax, ni, doubles * sizeof(double), st) : sv_dispatch<false>(g, nmax, ni, doubles * sizeof(double), st);
        });
        if (e != hipSuccess) return hip_fail(err, e, "svr_items launch");
    }
    return EPI_OK;
}

int epi_svr_run_host(const epi_svr_desc *d, const epi_svr_inputs *in, const epi_svr_outputs *out,
                     int device, char *err)
{
    int rc = epi_svr_validate(d, in, out, err);
    if (rc != EPI_OK) return rc;
    const size_t D = (size_t)d->D, F = (size_t)d->F, R = (size_t)d->R, K = (size_t)d->K;
    HostIO io;
    const size_t o_X = io.add_in(in->X, D * F, 8, R, 0, R), o_y = io.add_in(in->y, D, 8, R, 0, R);
    const size_t o_b = io.add_in(in->box, 1, 8, R, 0, R), o_e = io.add_in(in->epsilon, 1, 8, R, 0, R), o_s = io.add_in(in->kernel_scale, 1, 8, R, 0, R);
    using SO = epi_svr_outputs;
    const HostIO::Opt<SO, double> f64[5] = {{&SO::beta, K * D}, {&SO::bias, K}, {&SO::w, K * F}, {&SO::fitted, K * D}, {&SO::gap, K}};
    const HostIO::Opt<SO, int32_t> i32[3] = {{&SO::n_iter, K}, {&SO::n_sv, K}, {&SO::status, K}};
    size_t o_d[5], o_i[3];
    io.add_opt(*out, f64, o_d, R);
    io.add_opt(*out, i32, o_i, R);
    auto enqueue = [&](char *base, hipStream_t st) {
        epi_svr_inputs din{};
        din.X = (const double *)(base + o_X); din.y = (const double *)(base + o_y);
        din.box = (const double *)(base + o_b); din.epsilon = (const double *)(base + o_e); din.kernel_scale = (const double *)(base + o_s);
        din.n_rows = in->n_rows;                                       // host memory in both entry points
        epi_svr_outputs dout{};
        HostIO::bind_opt(dout, f64, o_d, base);
        HostIO::bind_opt(dout, i32, o_i, base);
        return epi_svr_run_device(d, &din, &dout, st, err);
    };
    return run_host(device, io, err, enqueue);
}

// ---- Monte-Carlo ensemble statistics over the draws of every region (BASELINE config 5) ----
int epi_ens_validate(const epi_ens_desc *d, const void *src, const double *population, const epi_ens_outputs *out, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->T < 1) { set_err(err, "T must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->rows < 1) { set_err(err, "rows must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->R < 1) { set_err(err, "R must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->D < 1 || d->D > kEnsMaxD) { set_err(err, "D must lie in 1 .. 4096 (a wavefront holds the draws of an item in registers)"); return EPI_ERR_BAD_ARG; }
    if (d->n_q < 1 || d->n_q > kEnsMaxQ) { set_err(err, "n_q must lie in 1 .. 16"); return EPI_ERR_BAD_ARG; }
    for (int k = 0; k < d->n_q; k++)
        if (!(d->q[k] >= 0.0 && d->q[k] <= 1.0)) { set_err(err, "every q must be finite and lie in [0, 1]"); return EPI_ERR_BAD_ARG; }
    if ((int64_t)d->R * d->D > (int64_t)0x7fffffff) { set_err(err, "R * D is limited to 2^31 - 1"); return EPI_ERR_BAD_ARG; }
    if (d->storage != 0 && d->storage != 1) { set_err(err, "storage must be 0 (double) or 1 (float)"); return EPI_ERR_BAD_ARG; }
    if (d->derive_newcases != 0 && d->derive_newcases != 1) { set_err(err, "derive_newcases must be 0 or 1"); return EPI_ERR_BAD_ARG; }
    if (d->derive_newcases && d->rows < 3) { set_err(err, "derive_newcases needs at least 3 rows"); return EPI_ERR_BAD_ARG; }
    if (d->derive_newcases && !population) { set_err(err, "NULL population (derive_newcases)"); return EPI_ERR_BAD_ARG; }
    if (!src || !out) { set_err(err, "NULL src / outputs"); return EPI_ERR_BAD_ARG; }
    if (!out->count) { set_err(err, "NULL count output"); return EPI_ERR_BAD_ARG; }
    return EPI_OK;
}

int epi_ens_run_device(const epi_ens_desc *d, const void *src, const double *population, const epi_ens_outputs *out,
                       void *stream, char *err)
{
    int rc = epi_ens_validate(d, src, population, out, err);
    if (rc != EPI_OK) return rc;
    EnsArgs g{};
    g.T = d->T; g.rows = d->rows; g.rows_out = d->rows + d->derive_newcases; g.R = d->R; g.D = d->D; g.n_q = d->n_q;
    g.f32 = d->storage; g.derive = d->derive_newcases;
    g.src = src; g.population = population;
    for (int k = 0; k < d->n_q; k++) g.q[k] = d->q[k];
    g.mean = out->mean; g.std = out->std; g.mn = out->min; g.mx = out->max; g.quant = out->quantiles; g.count = out->count;
    const int64_t items = (int64_t)d->T * g.rows_out * d->R;
    const hipStream_t st = (hipStream_t)stream;
    const hipError_t e = for_slices(items, kEnsLaunchItems, [&](int64_t i0, unsigned ni) {      // one 64-lane workgroup per item, in slices (ens_summary.hpp)
        g.item0 = (long long)i0;
        if (d->D <= 64) return ens_launch<1>(g, ni, st);           // registers per lane: P / 64, P the power of two >= D
        if (d->D <= 128) return ens_launch<2>(g, ni, st);
        if (d->D <= 256) return ens_launch<4>(g, ni, st);
        if (d->D <= 512) return ens_launch<8>(g, ni, st);
        if (d->D <= 1024) return ens_launch<16>(g, ni, st);
        if (d->D <= 2048) return ens_launch<32>(g, ni, st);
        return ens_launch<64>(g, ni, st);
    });
    if (e != hipSuccess) return hip_fail(err, e, "ens_summary launch");
    return EPI_OK;
}

int epi_ens_run_host(const epi_ens_desc *d, const void *src, const double *population, const epi_ens_outputs *out,
                     int device, char *err)
{
    int rc = epi_ens_validate(d, src, population, out, err);
    if (rc != EPI_OK) return rc;
    const size_t R = (size_t)d->R, B = R * (size_t)d->D, T = (size_t)d->T, ro = (size_t)(d->rows + d->derive_newcases);
    HostIO io;
    const size_t o_src = io.add_in(src, T * (size_t)d->rows, d->storage ? 4 : 8, B, 0, B);
    const size_t o_pop = d->derive_newcases ? io.add_in(population, 1, 8, R, 0, R) : HostIO::kAbsent;
    using EO = epi_ens_outputs;
    const HostIO::Opt<EO, double> f64[5] = {{&EO::mean, T * ro}, {&EO::std, T * ro}, {&EO::min, T * ro}, {&EO::max, T * ro},
                                            {&EO::quantiles, T * ro * (size_t)d->n_q}};
    size_t o_d[5];
    io.add_opt(*out, f64, o_d, R);
    const size_t o_cnt = io.add_out(out->count, T * ro, 4, R, 0, R);
    auto enqueue = [&](char *base, hipStream_t st) {
        epi_ens_outputs dout{};
        HostIO::bind_opt(dout, f64, o_d, base);
        dout.count = (int32_t *)(base + o_cnt);
        return epi_ens_run_device(d, base + o_src, HostIO::at<const double>(base, o_pop), &dout, st, err);
    };
    return run_host(device, io, err, enqueue);
}

// ---- the autoregressive alpha forecaster, R regions x D draws (Tools/PrescribeNPI.m:204-215) ----
int epi_arfc_validate(const epi_arfc_desc *d, const epi_arfc_inputs *in, const epi_arfc_outputs *out, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->R < 1) { set_err(err, "R must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->D < 1) { set_err(err, "D must be >= 1"); return EPI_ERR_BAD_ARG; }
    if ((int64_t)d->R * d->D > (int64_t)0x7fffffff) { set_err(err, "R * D is limited to 2^31 - 1"); return EPI_ERR_BAD_ARG; }
    if (d->p < 1 || d->p > kArMaxP) { set_err(err, "p must lie in 1 .. 32"); return EPI_ERR_BAD_ARG; }
    if (d->L < d->p + 1) { set_err(err, "L must be at least p + 1"); return EPI_ERR_BAD_ARG; }
    if (d->L - d->p > kArMaxRows) { set_err(err, "L - p is limited to 256 (the stacked matrix of a region lives in LDS)"); return EPI_ERR_BAD_ARG; }
    if (2 * (d->L - d->p) < d->p + 1) { set_err(err, "2 (L - p) must be at least p + 1 (more equations than unknowns)"); return EPI_ERR_BAD_ARG; }
    if (d->H < 1) { set_err(err, "H must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->fit != 0 && d->fit != 1) { set_err(err, "fit must be 0 or 1"); return EPI_ERR_BAD_ARG; }
    if (d->nv_mode != 0 && d->nv_mode != 1) { set_err(err, "nv_mode must be 0 or 1"); return EPI_ERR_BAD_ARG; }
    if (!(fabs(d->dt) < (double)INFINITY)) { set_err(err, "dt must be finite"); return EPI_ERR_BAD_ARG; }
    if (!in || !out) { set_err(err, "NULL inputs / outputs"); return EPI_ERR_BAD_ARG; }
    if (!in->seg || !in->beta || !in->s0 || !in->i0) { set_err(err, "NULL seg / beta / s0 / i0"); return EPI_ERR_BAD_ARG; }
    if (d->fit == 0 && (!in->A || !in->noise_var)) { set_err(err, "fit = 0 needs A and noise_var"); return EPI_ERR_BAD_ARG; }
    if (d->fit == 1 && (!out->A_out || !out->noise_var_out)) { set_err(err, "fit = 1 needs A_out and noise_var_out (the fit hands its model to the simulation through them)"); return EPI_ERR_BAD_ARG; }
    if (in->drive && d->Sd < 1) { set_err(err, "Sd must be >= 1 with a drive"); return EPI_ERR_BAD_ARG; }
    if (in->drive && !in->drive_series && (int64_t)d->Sd != (int64_t)d->R * d->D) { set_err(err, "drive without drive_series needs Sd == R * D"); return EPI_ERR_BAD_ARG; }
    if (!out->S) { set_err(err, "NULL S output"); return EPI_ERR_BAD_ARG; }
    return EPI_OK;
}

// nk: NULL (the draws are read from in->z) or the seeded call's key
static int arfc_run_device(const epi_arfc_desc *d, const NoiseKey *nk, const epi_arfc_inputs *in, const epi_arfc_outputs *out, void *stream,
                           char *err)
{
    int rc = epi_arfc_validate(d, in, out, err);
    if (rc != EPI_OK) return rc;
    const hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    const double *A = in->A, *nv = in->noise_var;
    if (d->fit) {
        ArFitArgs f{};
        f.L = d->L; f.p = d->p; f.R = d->R; f.nv_mode = d->nv_mode;
        f.seg = in->seg; f.A = out->A_out; f.nv = out->noise_var_out; f.status = out->status;
        const size_t shm = ar_fit_lds_bytes(d->L, d->p);
        // always the worst case (p = 32, L = 288), never this call's size: concurrent callers with different (L, p) then set the
        // same value, so the attribute cannot change between another thread's set and its launch
        if ((e = hipFuncSetAttribute((const void *)ar_fit, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)ar_fit_lds_bytes(kArMaxP + kArMaxRows, kArMaxP))) != hipSuccess)
            return hip_fail(err, e, "hipFuncSetAttribute");
        for (int64_t r0 = 0; r0 < d->R; r0 += kArLaunchBlocks) {           // one 64-lane workgroup per region, in slices
            f.r0 = (long long)r0;
            const unsigned nb = (unsigned)(d->R - r0 < kArLaunchBlocks ? d->R - r0 : kArLaunchBlocks);
            hipLaunchKernelGGL(ar_fit, dim3(nb), dim3(64), shm, st, f);
            if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "ar_fit launch");
        }
        A = out->A_out; nv = out->noise_var_out;
    } else {
        const size_t R = (size_t)d->R;
        if (out->A_out && (e = hipMemcpyAsync(out->A_out, in->A, (size_t)d->p * R * sizeof(double), hipMemcpyDeviceToDevice, st)) != hipSuccess)
            return hip_fail(err, e, "copy of A");
        if (out->noise_var_out && (e = hipMemcpyAsync(out->noise_var_out, in->noise_var, R * sizeof(double), hipMemcpyDeviceToDevice, st)) != hipSuccess)
            return hip_fail(err, e, "copy of noise_var");
        if (out->status) {
            hipLaunchKernelGGL(ar_given_status, dim3((unsigned)((d->R + 63) / 64)), dim3(64), 0, st, d->L, d->R, in->seg, out->status);
            if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "ar_given_status launch");
        }
    }
    ArSimArgs g{};
    g.L = d->L; g.p = d->p; g.H = d->H; g.R = d->R; g.D = d->D; g.Sd = d->Sd; g.bpr = ar_blocks_per_region(d->D); g.dt = d->dt;
    g.seg = in->seg; g.beta = in->beta; g.s0 = in->s0; g.i0 = in->i0; g.A = A; g.nv = nv; g.z = in->z; g.drive = in->drive;
    g.drive_series = in->drive_series; g.S = out->S;
    const size_t shm = ar_sim_lds_bytes(d->L, d->p);
    const int64_t blocks = (int64_t)d->R * g.bpr;
    for (int64_t b0 = 0; b0 < blocks; b0 += kArLaunchBlocks) {
        g.blk0 = (long long)b0;
        const unsigned nb = (unsigned)(blocks - b0 < kArLaunchBlocks ? blocks - b0 : kArLaunchBlocks);
        if (nk) hipLaunchKernelGGL(ar_simulate_seeded, dim3(nb), dim3(64), shm, st, g, *nk);
        else hipLaunchKernelGGL(ar_simulate, dim3(nb), dim3(64), shm, st, g);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "ar_simulate launch");
    }
    return EPI_OK;
}

int epi_arfc_run_device(const epi_arfc_desc *d, const epi_arfc_inputs *in, const epi_arfc_outputs *out, void *stream, char *err)
{
    return arfc_run_device(d, nullptr, in, out, stream, err);
}

int epi_arfc_run_device_seeded(const epi_arfc_desc *d, const epi_noise_desc *noise, const epi_arfc_inputs *in, const epi_arfc_outputs *out,
                               void *stream, char *err)
{
    NoiseKey nk;
    int rc = noise_key(noise, in ? in->z : nullptr, &nk, err);
    if (rc != EPI_OK) return rc;
    return arfc_run_device(d, &nk, in, out, stream, err);
}

static int arfc_run_host(const epi_arfc_desc *d, const epi_noise_desc *noise, const epi_arfc_inputs *in, const epi_arfc_outputs *out, int device,
                         char *err)
{
    int rc = epi_arfc_validate(d, in, out, err);
    if (rc != EPI_OK) return rc;
    const size_t R = (size_t)d->R, B = R * (size_t)d->D, K = (size_t)d->L + (size_t)d->H, none = HostIO::kAbsent;
    HostIO io;
    const size_t o_seg = io.add_in(in->seg, (size_t)d->L, 8, R, 0, R);
    const size_t o_beta = io.add_in(in->beta, 1, 8, R, 0, R), o_s0 = io.add_in(in->s0, 1, 8, R, 0, R), o_i0 = io.add_in(in->i0, 1, 8, R, 0, R);
    const size_t o_z = in->z ? io.add_in(in->z, (size_t)d->H, 8, B, 0, B) : none;
    const size_t o_drv = in->drive ? io.add_in(in->drive, (size_t)d->H, 8, (size_t)d->Sd, 0, (size_t)d->Sd) : none;
    const size_t o_ser = in->drive && in->drive_series ? io.add_in(in->drive_series, 1, 4, B, 0, B) : none;
    const size_t o_A = d->fit ? none : io.add_in(in->A, (size_t)d->p, 8, R, 0, R);
    const size_t o_nv = d->fit ? none : io.add_in(in->noise_var, 1, 8, R, 0, R);
    const size_t o_S = io.add_out(out->S, K * 3, 8, B, 0, B);
    const size_t o_Ao = io.add_out(out->A_out, (size_t)d->p, 8, R, 0, R);          // device copies exist even when not wanted
    const size_t o_nvo = io.add_out(out->noise_var_out, 1, 8, R, 0, R);
    const size_t o_st = io.add_out(out->status, 1, 4, R, 0, R);
    auto enqueue = [&](char *base, hipStream_t st) {
        auto dp = [&](size_t o) { return HostIO::at<const double>(base, o); };
        epi_arfc_inputs din{};
        din.seg = dp(o_seg); din.beta = dp(o_beta); din.s0 = dp(o_s0); din.i0 = dp(o_i0); din.z = dp(o_z); din.drive = dp(o_drv);
        din.drive_series = HostIO::at<const int32_t>(base, o_ser);
        din.A = dp(o_A); din.noise_var = dp(o_nv);
        epi_arfc_outputs dout{};
        dout.S = (double *)(base + o_S); dout.A_out = (double *)(base + o_Ao); dout.noise_var_out = (double *)(base + o_nvo);
        dout.status = (int32_t *)(base + o_st);
        return noise ? epi_arfc_run_device_seeded(d, noise, &din, &dout, st, err) : epi_arfc_run_device(d, &din, &dout, st, err);
    };
    return run_host(device, io, err, enqueue);
}

int epi_arfc_run_host(const epi_arfc_desc *d, const epi_arfc_inputs *in, const epi_arfc_outputs *out, int device, char *err)
{
    return arfc_run_host(d, nullptr, in, out, device, err);
}

int epi_arfc_run_host_seeded(const epi_arfc_desc *d, const epi_noise_desc *noise, const epi_arfc_inputs *in, const epi_arfc_outputs *out,
                             int device, char *err)
{
    NoiseKey nk;
    int rc = noise_key(noise, in ? in->z : nullptr, &nk, err);   // before anything is staged: no z is copied
    if (rc != EPI_OK) return rc;
    return arfc_run_host(d, noise, in, out, device, err);
}

// ---- the forward-backward filter fusion, one item per (chain, day) (Tools/TrainPredictPrescribeNPI.m:464-478) ----
int epi_fuse_validate(const epi_fuse_desc *d, const epi_fuse_inputs *in, const epi_fuse_outputs *out, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->m != 3 && d->m != 6) { set_err(err, "m must be 3 or 6"); return EPI_ERR_BAD_ARG; }
    if (d->B < 1) { set_err(err, "B must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->T < 1) { set_err(err, "T must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->lane_block < 0 || d->lane_block > d->B) { set_err(err, "lane_block must lie in 0 .. B (0 or B: the classic [T][rows][B])"); return EPI_ERR_BAD_ARG; }
    if (d->storage != 0 && d->storage != 1) { set_err(err, "storage must be 0 (double) or 1 (float)"); return EPI_ERR_BAD_ARG; }
    if (d->form != 0 && d->form != 1) { set_err(err, "form must be 0 (the reference as written) or 1 (the information form)"); return EPI_ERR_BAD_ARG; }
    if (d->p_solver != 0 && d->p_solver != 1) { set_err(err, "p_solver must be 0 (S \\ C) or 1 (pinv(S) * C)"); return EPI_ERR_BAD_ARG; }
    if (d->form == 1 && d->p_solver != 0) { set_err(err, "p_solver must be 0 with form = 1"); return EPI_ERR_BAD_ARG; }
    if (d->reserved != 0) { set_err(err, "reserved must be 0"); return EPI_ERR_BAD_ARG; }
    if (!in || !out) { set_err(err, "NULL inputs / outputs"); return EPI_ERR_BAD_ARG; }
    if (!in->sf || !in->Pf || !in->sb || !in->Pb) { set_err(err, "NULL sf / Pf / sb / Pb"); return EPI_ERR_BAD_ARG; }
    if (!out->s_out && !out->P_out && !out->d2) { set_err(err, "no output requested: at least one of s_out / P_out / d2"); return EPI_ERR_BAD_ARG; }
    return EPI_OK;
}

int epi_fuse_run_device(const epi_fuse_desc *d, const epi_fuse_inputs *in, const epi_fuse_outputs *out, void *stream, char *err)
{
    int rc = epi_fuse_validate(d, in, out, err);
    if (rc != EPI_OK) return rc;
    const hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    FuseArgs g{};
    g.B = d->B; g.T = d->T; g.f32 = d->storage; g.form = d->form; g.p_solver = d->p_solver;
    fuse_geometry(d->B, d->lane_block, &g.blk, &g.nblk);
    g.sf = in->sf; g.Pf = in->Pf; g.sb = in->sb; g.Pb = in->Pb;
    g.s_out = out->s_out; g.P_out = out->P_out; g.d2 = out->d2; g.rank = out->rank; g.status = out->status;
    if (out->status && (e = hipMemsetAsync(out->status, 0, (size_t)d->B * sizeof(int32_t), st)) != hipSuccess)
        return hip_fail(err, e, "hipMemsetAsync of status");
    const int wgs = d->m == 6 ? pinv_wg<6>() : pinv_wg<3>();
    g.tiles = (unsigned)(((int64_t)d->B + wgs - 1) / wgs);
    const long long groups = (long long)g.tiles * d->T;
    for (long long w0 = 0; w0 < groups; w0 += kFuseLaunchGroups) {     // in slices (two_filter.hpp)
        g.wg0 = w0;
        const unsigned nb = (unsigned)(groups - w0 < kFuseLaunchGroups ? groups - w0 : kFuseLaunchGroups);
        if (d->m == 6) hipLaunchKernelGGL(two_filter<6>, dim3(nb), dim3(pinv_wg<6>()), 0, st, g);
        else hipLaunchKernelGGL(two_filter<3>, dim3(nb), dim3(pinv_wg<3>()), 0, st, g);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "two_filter launch");
    }
    return EPI_OK;
}

int epi_fuse_run_host(const epi_fuse_desc *d, const epi_fuse_inputs *in, const epi_fuse_outputs *out, int device, char *err)
{
    int rc = epi_fuse_validate(d, in, out, err);
    if (rc != EPI_OK) return rc;
    const size_t B = (size_t)d->B, T = (size_t)d->T, m = (size_t)d->m, none = HostIO::kAbsent;
    int gblk, gnblk;
    fuse_geometry(d->B, d->lane_block, &gblk, &gnblk);
    const size_t Bp = (size_t)gnblk * (size_t)gblk, es = d->storage ? 4 : 8;       // a day of a blocked array holds rows * Bp elements
    HostIO io;
    const size_t o_sf = io.add_in(in->sf, T * m, es, Bp, 0, Bp), o_Pf = io.add_in(in->Pf, T * m * m, es, Bp, 0, Bp);
    const size_t o_sb = io.add_in(in->sb, T * m, es, Bp, 0, Bp), o_Pb = io.add_in(in->Pb, T * m * m, es, Bp, 0, Bp);
    const size_t o_s = out->s_out ? io.add_out(out->s_out, T * m, es, Bp, 0, Bp) : none;
    const size_t o_P = out->P_out ? io.add_out(out->P_out, T * m * m, es, Bp, 0, Bp) : none;
    const size_t o_d2 = out->d2 ? io.add_out(out->d2, T, 8, B, 0, B) : none;
    const size_t o_rk = out->rank ? io.add_out(out->rank, T, 4, B, 0, B) : none;
    const size_t o_st = out->status ? io.add_out(out->status, 1, 4, B, 0, B) : none;
    auto enqueue = [&](char *base, hipStream_t st) -> int {
        // the padding lanes of a blocked output are never written by the kernel: the host entry returns them as zeros, not as
        // arena bytes (include/epiekf.h says so)
        hipError_t e;
        if (Bp != B) {
            if (o_s != none && (e = hipMemsetAsync(base + o_s, 0, T * m * Bp * es, st)) != hipSuccess) return hip_fail(err, e, "hipMemsetAsync of s_out");
            if (o_P != none && (e = hipMemsetAsync(base + o_P, 0, T * m * m * Bp * es, st)) != hipSuccess) return hip_fail(err, e, "hipMemsetAsync of P_out");
        }
        epi_fuse_inputs din{};
        din.sf = base + o_sf; din.Pf = base + o_Pf; din.sb = base + o_sb; din.Pb = base + o_Pb;
        epi_fuse_outputs dout{};
        dout.s_out = HostIO::at<char>(base, o_s); dout.P_out = HostIO::at<char>(base, o_P);
        dout.d2 = HostIO::at<double>(base, o_d2);
        dout.rank = HostIO::at<int32_t>(base, o_rk); dout.status = HostIO::at<int32_t>(base, o_st);
        return epi_fuse_run_device(d, &din, &dout, st, err);
    };
    return run_host(device, io, err, enqueue);
}

// ---- the Gaussian innovation log-likelihood of every chain, from the arrays a filter run left (loglik.hpp) ----
// the workspace: the block sums [nb32][B] (term, q: double; n, bad: int32), the per-chain loglik / n_valid / status the selection
// reads when the caller does not want them, and for r_mode 0 R(k) [T][B]; every piece starts at a multiple of 256 bytes
struct LlWs { size_t term, q, n, bad, ll, nv, st, rk, bytes; };
static LlWs ll_workspace(const epi_loglik_desc *d)
{
    const size_t B = (size_t)d->B, nb = ((size_t)d->T + kLlBlock - 1) / kLlBlock;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    LlWs w{};
    size_t o = 0;
    w.term = o; o += up(nb * B * 8);
    w.q = o; o += up(nb * B * 8);
    w.n = o; o += up(nb * B * 4);
    w.bad = o; o += up(nb * B * 4);
    w.ll = o; o += up(B * 8);
    w.nv = o; o += up(B * 4);
    w.st = o; o += up(B * 4);
    w.rk = o; if (d->r_mode == 0) o += up((size_t)d->T * B * 8);
    w.bytes = o;
    return w;
}

int epi_loglik_validate(const epi_loglik_desc *d, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->model < 0 || d->model > EPI_MODEL_NEWCASE6_CODEGEN) { set_err(err, "unknown model"); return EPI_ERR_BAD_ARG; }
    const ModelInfo &mi = MODEL_TABLE[d->model];
    if (!mi.obs_fixed && d->obs_type != EPI_OBS_NEWCASES && d->obs_type != EPI_OBS_TOTALCASES) {
        set_err(err, "unknown observation type");
        return EPI_ERR_OBS_TYPE;
    }
    if (d->B < 1) { set_err(err, "B must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->T < 1) { set_err(err, "T must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->L < 1) { set_err(err, "L must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->Sx < 1) { set_err(err, "Sx must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->r_mode != 0 && d->r_mode != 1) { set_err(err, "r_mode must be 0 (R_scalar) or 1 (R_series)"); return EPI_ERR_BAD_ARG; }
    if (d->k0 < 0 || d->k1 < 0 || d->k1 > d->T || d->k0 >= (d->k1 ? d->k1 : d->T)) {
        set_err(err, "the window must satisfy 0 <= k0 < k1 <= T (k1 = 0: T)");
        return EPI_ERR_BAD_ARG;
    }
    if (d->G < 0 || (d->G > 0 && d->B % d->G != 0)) { set_err(err, "G must be 0 or divide B"); return EPI_ERR_BAD_ARG; }
    if (d->lane_block < 0 || d->lane_block > d->B) { set_err(err, "lane_block must lie in 0 .. B (0 or B: the classic [T][rows][B])"); return EPI_ERR_BAD_ARG; }
    if (d->storage != 0 && d->storage != 1) { set_err(err, "storage must be 0 (double) or 1 (float)"); return EPI_ERR_BAD_ARG; }
    if (d->reserved != 0) { set_err(err, "reserved must be 0"); return EPI_ERR_BAD_ARG; }
    if (d->r_mode == 0 && (size_t)2 * d->L * kWave * sizeof(double) > 64u * 1024u) { set_err(err, "L too large for the replay's windows in LDS (max 64)"); return EPI_ERR_UNSUPPORTED; }
    if (((int64_t)d->B + 255) / 256 * 256 * (((int64_t)d->T + kLlBlock - 1) / kLlBlock) >= ((int64_t)1 << 31) || ((int64_t)d->T + kLlBlock - 1) / kLlBlock > 65535) {
        set_err(err, "B * ceil(T / 32) is limited to 2^31 - 1 (one launch covers every block of every chain)");
        return EPI_ERR_UNSUPPORTED;
    }
    return EPI_OK;
}

int epi_loglik_workspace_bytes(const epi_loglik_desc *d, size_t *bytes, char *err)
{
    int rc = epi_loglik_validate(d, err);
    if (rc != EPI_OK) return rc;
    if (!bytes) { set_err(err, "NULL bytes"); return EPI_ERR_BAD_ARG; }
    *bytes = ll_workspace(d).bytes;
    return EPI_OK;
}

// the pointer checks, shared by the device and the host entry
static int ll_check_arrays(const epi_loglik_desc *d, const epi_loglik_inputs *in, const epi_loglik_outputs *out, char *err)
{
    if (!in || !out) { set_err(err, "NULL inputs / outputs"); return EPI_ERR_BAD_ARG; }
    if (!in->S_MINUS || !in->P_MINUS || !in->innovations || !in->x || !in->prm) { set_err(err, "NULL S_MINUS / P_MINUS / innovations / x / prm"); return EPI_ERR_BAD_ARG; }
    if (d->r_mode == 1 && !in->R_series) { set_err(err, "r_mode 1 needs R_series"); return EPI_ERR_BAD_ARG; }
    if (d->r_mode == 0 && !in->R_scalar) { set_err(err, "r_mode 0 needs R_scalar"); return EPI_ERR_BAD_ARG; }
    if (!in->x_series && d->Sx != d->B) { set_err(err, "x_series is NULL: Sx must equal B"); return EPI_ERR_BAD_ARG; }
    if (!out->loglik && !out->nis_mean && !out->S && !out->nis && !out->R_used) {
        set_err(err, "no output requested: at least one of loglik / nis_mean / S / nis / R_used");
        return EPI_ERR_BAD_ARG;
    }
    if ((out->best || out->best_loglik) && d->G <= 0) { set_err(err, "best / best_loglik need G > 0"); return EPI_ERR_BAD_ARG; }
    return EPI_OK;
}

int epi_loglik_run_device(const epi_loglik_desc *d, const epi_loglik_inputs *in, const epi_loglik_outputs *out, void *ws,
                          size_t ws_bytes, void *stream, char *err)
{
    int rc = epi_loglik_validate(d, err);
    if (rc != EPI_OK) return rc;
    if ((rc = ll_check_arrays(d, in, out, err)) != EPI_OK) return rc;
    const LlWs w = ll_workspace(d);
    if (!ws || ws_bytes < w.bytes) { set_err(err, "workspace too small (epi_loglik_workspace_bytes)"); return EPI_ERR_WORKSPACE; }
    const hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    const ModelInfo &mi = MODEL_TABLE[d->model];
    char *base = (char *)ws;
    LlArgs a{};
    a.B = d->B; a.T = d->T; a.L = d->L; a.Sx = d->Sx; a.r_mode = d->r_mode; a.f32 = d->storage; a.flip = mi.flipped;
    a.generic = mi.generic; a.obs_type = mi.obs_fixed ? EPI_OBS_NEWCASES : d->obs_type;
    a.k0 = d->k0; a.k1 = d->k1 ? d->k1 : d->T; a.G = d->G; a.m = mi.m; a.nb32 = (d->T + kLlBlock - 1) / kLlBlock;
    ll_geometry(d->B, d->lane_block, &a.blk, &a.nblk);
    a.S_MINUS = in->S_MINUS; a.P_MINUS = in->P_MINUS; a.innov = in->innovations;
    a.x = in->x; a.R_series = in->R_series; a.R_scalar = in->R_scalar; a.prm = in->prm; a.x_series = in->x_series;
    a.Rk = out->R_used ? out->R_used : (d->r_mode == 0 ? (double *)(base + w.rk) : nullptr);
    a.part_term = (double *)(base + w.term); a.part_q = (double *)(base + w.q);
    a.part_n = (int32_t *)(base + w.n); a.part_bad = (int32_t *)(base + w.bad);
    a.loglik = out->loglik ? out->loglik : (double *)(base + w.ll);
    a.nis_mean = out->nis_mean;
    a.n_valid = out->n_valid ? out->n_valid : (int32_t *)(base + w.nv);
    a.status = out->status ? out->status : (int32_t *)(base + w.st);
    a.S = out->S; a.nis = out->nis; a.best = out->best; a.best_loglik = out->best_loglik;
    const unsigned tiles = (unsigned)(((int64_t)d->B + 255) / 256);
    if (d->r_mode == 0) {
        hipLaunchKernelGGL(ll_replay, dim3((unsigned)(((int64_t)d->B + kWave - 1) / kWave)), dim3(kWave),
                           (size_t)2 * d->L * kWave * sizeof(double), st, a);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "ll_replay launch");
    }
    const bool sums = out->loglik || out->nis_mean || out->n_valid || out->status || out->best || out->best_loglik;
    if (sums || out->S || out->nis || (d->r_mode == 1 && out->R_used)) {
        hipLaunchKernelGGL(ll_blocks, dim3(tiles, (unsigned)a.nb32), dim3(256), 0, st, a);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "ll_blocks launch");
    }
    if (sums) {
        hipLaunchKernelGGL(ll_chains, dim3(tiles), dim3(256), 0, st, a);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "ll_chains launch");
    }
    if (out->best || out->best_loglik) {
        hipLaunchKernelGGL(ll_select, dim3((unsigned)(((int64_t)(d->B / d->G) + 255) / 256)), dim3(256), 0, st, a);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "ll_select launch");
    }
    return EPI_OK;
}

int epi_loglik_run_host(const epi_loglik_desc *d, const epi_loglik_inputs *in, const epi_loglik_outputs *out, int device, char *err)
{
    int rc = epi_loglik_validate(d, err);
    if (rc != EPI_OK) return rc;
    if ((rc = ll_check_arrays(d, in, out, err)) != EPI_OK) return rc;
    const size_t B = (size_t)d->B, T = (size_t)d->T, Sx = (size_t)d->Sx, m = (size_t)MODEL_TABLE[d->model].m, none = HostIO::kAbsent;
    int gblk, gnblk;
    ll_geometry(d->B, d->lane_block, &gblk, &gnblk);
    const size_t Bp = (size_t)gnblk * (size_t)gblk, es = d->storage ? 4 : 8;
    HostIO io;
    const size_t o_sm = io.add_in(in->S_MINUS, T * m, es, Bp, 0, Bp), o_pm = io.add_in(in->P_MINUS, T * m * m, es, Bp, 0, Bp);
    const size_t o_in = io.add_in(in->innovations, T, es, Bp, 0, Bp), o_x = io.add_in(in->x, T, 8, Sx, 0, Sx);
    const size_t o_rs = d->r_mode == 1 ? io.add_in(in->R_series, T, 8, Sx, 0, Sx) : none;
    const size_t o_rv = d->r_mode == 0 ? io.add_in(in->R_scalar, 1, 8, B, 0, B) : none;
    const size_t o_xs = in->x_series ? io.add_in(in->x_series, 1, 4, B, 0, B) : none;
    const size_t o_prm = io.add_in(in->prm, (size_t)EPI_PRM_COUNT, 8, B, 0, B);
    const size_t Rg = d->G > 0 ? B / (size_t)d->G : 0;
    const size_t o_ll = out->loglik ? io.add_out(out->loglik, 1, 8, B, 0, B) : none;
    const size_t o_nm = out->nis_mean ? io.add_out(out->nis_mean, 1, 8, B, 0, B) : none;
    const size_t o_nv = out->n_valid ? io.add_out(out->n_valid, 1, 4, B, 0, B) : none;
    const size_t o_st = out->status ? io.add_out(out->status, 1, 4, B, 0, B) : none;
    const size_t o_S = out->S ? io.add_out(out->S, T, 8, B, 0, B) : none;
    const size_t o_ni = out->nis ? io.add_out(out->nis, T, 8, B, 0, B) : none;
    const size_t o_ru = out->R_used ? io.add_out(out->R_used, T, 8, B, 0, B) : none;
    const size_t o_b = out->best ? io.add_out(out->best, 1, 4, Rg, 0, Rg) : none;
    const size_t o_bl = out->best_loglik ? io.add_out(out->best_loglik, 1, 8, Rg, 0, Rg) : none;
    const size_t wsb = ll_workspace(d).bytes;
    const size_t o_ws = io.reserve(wsb);
    auto enqueue = [&](char *base, hipStream_t st) -> int {
        epi_loglik_inputs din{};
        din.S_MINUS = base + o_sm; din.P_MINUS = base + o_pm; din.innovations = base + o_in;
        din.x = HostIO::at<const double>(base, o_x); din.R_series = HostIO::at<const double>(base, o_rs);
        din.R_scalar = HostIO::at<const double>(base, o_rv); din.x_series = HostIO::at<const int32_t>(base, o_xs);
        din.prm = HostIO::at<const double>(base, o_prm);
        epi_loglik_outputs dout{};
        dout.loglik = HostIO::at<double>(base, o_ll); dout.nis_mean = HostIO::at<double>(base, o_nm);
        dout.n_valid = HostIO::at<int32_t>(base, o_nv); dout.status = HostIO::at<int32_t>(base, o_st);
        dout.S = HostIO::at<double>(base, o_S); dout.nis = HostIO::at<double>(base, o_ni); dout.R_used = HostIO::at<double>(base, o_ru);
        dout.best = HostIO::at<int32_t>(base, o_b); dout.best_loglik = HostIO::at<double>(base, o_bl);
        return epi_loglik_run_device(d, &din, &dout, base + o_ws, wsb, st, err);
    };
    return run_host(device, io, err, enqueue);
}

// ---- the direct optimal-NPI planner: one lane per (region, cost weight) chain (npi_plan.hpp) ----
// the workspace: the second plan [H][n][B], the states of side 1 (and of side 0 when the caller does not want them) [H][3][B],
// the vertex / held masks [H][B] uint32; every piece starts at a multiple of 256 bytes
struct PlanWs { size_t u1, x1, x0, mask, bytes; };
static PlanWs plan_workspace(const epi_plan_desc *d, bool want_states)
{
    const size_t B = (size_t)d->R * (size_t)d->P, H = (size_t)d->H;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    PlanWs w{};
    size_t o = 0;
    w.u1 = o; o += up(H * (size_t)d->n_npi * B * 8);
    w.x1 = o; o += up(H * 3 * B * 8);
    w.x0 = o; if (!want_states) o += up(H * 3 * B * 8);
    w.mask = o; o += up(H * B * 4);
    w.bytes = o;
    return w;
}

int epi_plan_validate(const epi_plan_desc *d, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->R < 1 || d->P < 1) { set_err(err, "R and P must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->H < 1) { set_err(err, "H must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->n_npi < 1 || d->n_npi > kNpi) { set_err(err, "n_npi must lie in 1 .. 12"); return EPI_ERR_BAD_ARG; }
    if (d->prefix_days < 0) { set_err(err, "prefix_days must be >= 0"); return EPI_ERR_BAD_ARG; }
    if (d->max_iter < 1 || d->max_iter > kPlanMaxIter) { set_err(err, "max_iter must lie in 1 .. 255"); return EPI_ERR_BAD_ARG; }
    if (d->max_halvings < 0 || d->max_halvings > kPlanMaxHalvings) { set_err(err, "max_halvings must lie in 0 .. 30"); return EPI_ERR_BAD_ARG; }
    if (!(d->tol >= 0.0 && d->tol <= 1.7976931348623157e308)) { set_err(err, "tol must be finite and >= 0"); return EPI_ERR_BAD_ARG; }
    const int64_t B = (int64_t)d->R * d->P, lim = (int64_t)1 << 31, rows = d->n_npi > 3 ? d->n_npi : 3;
    if (B >= lim || (int64_t)d->H * rows >= lim || (int64_t)d->H * rows * B >= lim || (int64_t)d->max_iter * B >= lim) {
        set_err(err, "R * P, H * max(n_npi, 3) * R * P and max_iter * R * P are limited to 2^31 - 1 (the call is one launch)");
        return EPI_ERR_UNSUPPORTED;
    }
    return EPI_OK;
}

int epi_plan_workspace_bytes(const epi_plan_desc *d, size_t *bytes, char *err)
{
    int rc = epi_plan_validate(d, err);
    if (rc != EPI_OK) return rc;
    if (!bytes) { set_err(err, "NULL bytes"); return EPI_ERR_BAD_ARG; }
    *bytes = plan_workspace(d, false).bytes;               // the larger of the two cases: the caller may size it before choosing outputs
    return EPI_OK;
}

// the pointer checks, shared by the device and the host entry
static int plan_check_arrays(const epi_plan_desc *d, const epi_plan_inputs *in, const epi_plan_outputs *out, char *err)
{
    if (!in || !out) { set_err(err, "NULL inputs / outputs"); return EPI_ERR_BAD_ARG; }
    if (!in->sp || !in->u_min || !in->eps) { set_err(err, "NULL sp / u_min / eps"); return EPI_ERR_BAD_ARG; }
    if (d->prefix_days > 0 && (!in->J0_prefix || !in->J1_prefix)) { set_err(err, "prefix_days > 0 needs J0_prefix and J1_prefix"); return EPI_ERR_BAD_ARG; }
    if (!out->plan || !out->J0 || !out->J1 || !out->F || !out->gap || !out->iters || !out->halvings || !out->status) {
        set_err(err, "NULL plan / J0 / J1 / F / gap / iters / halvings / status");
        return EPI_ERR_BAD_ARG;
    }
    return EPI_OK;
}

int epi_plan_run_device(const epi_plan_desc *d, const epi_plan_inputs *in, const epi_plan_outputs *out, void *ws, size_t ws_bytes,
                        void *stream, char *err)
{
    int rc = epi_plan_validate(d, err);
    if (rc != EPI_OK) return rc;
    if ((rc = plan_check_arrays(d, in, out, err)) != EPI_OK) return rc;
    const PlanWs w = plan_workspace(d, out->states != nullptr);
    if (!ws || ws_bytes < w.bytes) { set_err(err, "workspace too small (epi_plan_workspace_bytes)"); return EPI_ERR_WORKSPACE; }
    char *base = (char *)ws;
    PlanArgs a{};
    a.R = d->R; a.P = d->P; a.H = d->H; a.n = d->n_npi; a.max_iter = d->max_iter; a.max_halvings = d->max_halvings;
    a.prefix_days = d->prefix_days; a.tol = d->tol;
    a.sp = in->sp; a.u_min = in->u_min; a.eps = in->eps; a.u_fixed = in->u_fixed; a.u_init = in->u_init;
    a.J0_prefix = in->J0_prefix; a.J1_prefix = in->J1_prefix;
    a.ub[0] = out->plan; a.ub[1] = (double *)(base + w.u1);
    a.xb[0] = out->states ? out->states : (double *)(base + w.x0); a.xb[1] = (double *)(base + w.x1);
    a.want_states = out->states != nullptr;
    a.mask = (uint32_t *)(base + w.mask);
    a.J0 = out->J0; a.J1 = out->J1; a.F = out->F; a.gap = out->gap;
    a.iters = out->iters; a.halvings = out->halvings; a.status = out->status;
    a.mu = out->mu; a.F_trace = out->F_trace;
    const int64_t B = (int64_t)d->R * d->P;
    hipLaunchKernelGGL(plan_solve, dim3((unsigned)((B + kWave - 1) / kWave)), dim3(kWave), 0, (hipStream_t)stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(err, e, "plan_solve launch");
    return EPI_OK;
}

int epi_plan_run_host(const epi_plan_desc *d, const epi_plan_inputs *in, const epi_plan_outputs *out, int device, char *err)
{
    int rc = epi_plan_validate(d, err);
    if (rc != EPI_OK) return rc;
    if ((rc = plan_check_arrays(d, in, out, err)) != EPI_OK) return rc;
    const size_t R = (size_t)d->R, P = (size_t)d->P, B = R * P, H = (size_t)d->H, n = (size_t)d->n_npi, none = HostIO::kAbsent;
    const bool pre = d->prefix_days > 0;
    HostIO io;
    const size_t o_sp = io.add_in(in->sp, (size_t)EPI_SIM_PRM_COUNT, 8, R, 0, R), o_um = io.add_in(in->u_min, n, 8, R, 0, R);
    const size_t o_eps = io.add_in(in->eps, 1, 8, P, 0, P);
    const size_t o_uf = in->u_fixed ? io.add_in(in->u_fixed, H * n, 8, R, 0, R) : none;
    const size_t o_ui = in->u_init ? io.add_in(in->u_init, H * n, 8, B, 0, B) : none;
    const size_t o_j0p = pre ? io.add_in(in->J0_prefix, 1, 8, R, 0, R) : none, o_j1p = pre ? io.add_in(in->J1_prefix, 1, 8, R, 0, R) : none;
    const size_t o_plan = io.add_out(out->plan, H * n, 8, B, 0, B);
    const size_t o_j0 = io.add_out(out->J0, 1, 8, B, 0, B), o_j1 = io.add_out(out->J1, 1, 8, B, 0, B);
    const size_t o_F = io.add_out(out->F, 1, 8, B, 0, B), o_gap = io.add_out(out->gap, 1, 8, B, 0, B);
    const size_t o_it = io.add_out(out->iters, 1, 4, B, 0, B), o_hv = io.add_out(out->halvings, 1, 4, B, 0, B);
    const size_t o_st = io.add_out(out->status, 1, 4, B, 0, B);
    const size_t o_x = out->states ? io.add_out(out->states, H * 3, 8, B, 0, B) : none;
    const size_t o_mu = out->mu ? io.add_out(out->mu, H * 3, 8, B, 0, B) : none;
    const size_t o_ft = out->F_trace ? io.add_out(out->F_trace, (size_t)d->max_iter, 8, B, 0, B) : none;
    const size_t wsb = plan_workspace(d, out->states != nullptr).bytes;
    const size_t o_ws = io.reserve(wsb);
    auto enqueue = [&](char *base, hipStream_t st) -> int {
        epi_plan_inputs din{};
        din.sp = HostIO::at<const double>(base, o_sp); din.u_min = HostIO::at<const double>(base, o_um);
        din.eps = HostIO::at<const double>(base, o_eps); din.u_fixed = HostIO::at<const double>(base, o_uf);
        din.u_init = HostIO::at<const double>(base, o_ui);
        din.J0_prefix = HostIO::at<const double>(base, o_j0p); din.J1_prefix = HostIO::at<const double>(base, o_j1p);
        epi_plan_outputs dout{};
        dout.plan = HostIO::at<double>(base, o_plan); dout.J0 = HostIO::at<double>(base, o_j0); dout.J1 = HostIO::at<double>(base, o_j1);
        dout.F = HostIO::at<double>(base, o_F); dout.gap = HostIO::at<double>(base, o_gap);
        dout.iters = HostIO::at<int32_t>(base, o_it); dout.halvings = HostIO::at<int32_t>(base, o_hv);
        dout.status = HostIO::at<int32_t>(base, o_st);
        dout.states = HostIO::at<double>(base, o_x); dout.mu = HostIO::at<double>(base, o_mu); dout.F_trace = HostIO::at<double>(base, o_ft);
        return epi_plan_run_device(d, &din, &dout, base + o_ws, wsb, st, err);
    };
    return run_host(device, io, err, enqueue);
}

// ---- joint posterior draws of the smoothed paths: sdraw_gain, then sdraw_paths (smoother_draws.hpp) ----
// the workspace: one record of kSdRec doubles per (day, chain)
int epi_sdraw_validate(const epi_sdraw_desc *d, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->model < 0 || d->model > EPI_MODEL_NEWCASE6_CODEGEN) { set_err(err, "unknown model"); return EPI_ERR_BAD_ARG; }
    const ModelInfo &mi = MODEL_TABLE[d->model];
    if (mi.m != 3) {
        set_err(err, "smoother draws need the 3-state SIAlphaModelEKF: the 6-state costate block has no meaningful factor in fp64");
        return EPI_ERR_UNSUPPORTED;
    }
    if (mi.flipped) { set_err(err, "smoother draws do not take the time-flipped models"); return EPI_ERR_UNSUPPORTED; }
    if (d->B < 1) { set_err(err, "B must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->T < 1) { set_err(err, "T must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->D < 1) { set_err(err, "D must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->k0 < 0 || d->k0 >= d->T) { set_err(err, "k0 must lie in 0 .. T-1"); return EPI_ERR_BAD_ARG; }
    if (d->clamp != 0 && d->clamp != 1) { set_err(err, "clamp must be 0 or 1"); return EPI_ERR_BAD_ARG; }
    if (d->lane_block < 0 || d->lane_block > d->B) { set_err(err, "lane_block must lie in 0 .. B (0 or B: the classic [T][rows][B])"); return EPI_ERR_BAD_ARG; }
    if (d->storage != 0 && d->storage != 1) { set_err(err, "storage must be 0 (double) or 1 (float)"); return EPI_ERR_BAD_ARG; }
    if (d->z_f32 != 0 && d->z_f32 != 1) { set_err(err, "z_f32 must be 0 (double) or 1 (float)"); return EPI_ERR_BAD_ARG; }
    if (d->out_f32 != 0 && d->out_f32 != 1) { set_err(err, "out_f32 must be 0 (double) or 1 (float)"); return EPI_ERR_BAD_ARG; }
    if (d->test_launch_groups < 0) { set_err(err, "test_launch_groups must be >= 0"); return EPI_ERR_BAD_ARG; }
    return EPI_OK;
}

int epi_sdraw_workspace_bytes(const epi_sdraw_desc *d, size_t *bytes, char *err)
{
    int rc = epi_sdraw_validate(d, err);
    if (rc != EPI_OK) return rc;
    if (!bytes) { set_err(err, "NULL bytes"); return EPI_ERR_BAD_ARG; }
    *bytes = (size_t)d->T * (size_t)d->B * (size_t)kSdRec * sizeof(double);
    return EPI_OK;
}

static int sdraw_check_arrays(const epi_sdraw_inputs *in, const epi_sdraw_outputs *out, char *err)
{
    if (!in || !out) { set_err(err, "NULL inputs / outputs"); return EPI_ERR_BAD_ARG; }
    if (!in->S_PLUS || !in->P_PLUS || !in->S_MINUS || !in->P_MINUS || !in->prm) { set_err(err, "NULL S_PLUS / P_PLUS / S_MINUS / P_MINUS / prm"); return EPI_ERR_BAD_ARG; }
    if (!out->X && !out->rank && !out->status && !out->J && !out->L) { set_err(err, "no output requested: at least one of X / rank / status / J / L"); return EPI_ERR_BAD_ARG; }
    return EPI_OK;
}

// nk: NULL (the draws are read from in->z, if any) or the seeded call's key
static int sdraw_run_device(const epi_sdraw_desc *d, const NoiseKey *nk, const epi_sdraw_inputs *in, const epi_sdraw_outputs *out, void *ws,
                            size_t ws_bytes, void *stream, char *err)
{
    int rc = epi_sdraw_validate(d, err);
    if (rc != EPI_OK) return rc;
    if ((rc = sdraw_check_arrays(in, out, err)) != EPI_OK) return rc;
    const size_t need = (size_t)d->T * (size_t)d->B * (size_t)kSdRec * sizeof(double);
    if (!ws || ws_bytes < need) { set_err(err, "workspace too small (epi_sdraw_workspace_bytes)"); return EPI_ERR_WORKSPACE; }
    const hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    SdArgs g{};
    g.B = d->B; g.T = d->T; g.D = d->D; g.k0 = d->k0; g.clamp = d->clamp; g.f32 = d->storage;
    sdraw_geometry(d->B, d->lane_block, &g.blk, &g.nblk);
    g.S_PLUS = in->S_PLUS; g.P_PLUS = in->P_PLUS; g.S_MINUS = in->S_MINUS; g.P_MINUS = in->P_MINUS;
    g.prm = in->prm; g.s_term = in->s_term; g.P_term = in->P_term; g.z = in->z;
    g.X = out->X; g.ws = (double *)ws; g.J = out->J; g.L = out->L; g.rank = out->rank; g.status = out->status;
    if (out->status && (e = hipMemsetAsync(out->status, 0, (size_t)d->B * sizeof(int32_t), st)) != hipSuccess)
        return hip_fail(err, e, "hipMemsetAsync of status");
    const long long cap = d->test_launch_groups > 0 ? (long long)d->test_launch_groups : kSdLaunchGroups;
    g.tiles = (unsigned)(((int64_t)d->B + pinv_wg<3>() - 1) / pinv_wg<3>());
    const long long groups = (long long)g.tiles * d->T;          // every day, also those below k0: J, L and rank cover [T]
    for (long long w0 = 0; w0 < groups; w0 += cap) {                  // in slices, as two_filter's
        g.wg0 = w0;
        const unsigned nb = (unsigned)(groups - w0 < cap ? groups - w0 : cap);
        hipLaunchKernelGGL(sdraw_gain<3>, dim3(nb), dim3(pinv_wg<3>()), 0, st, g);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "sdraw_gain launch");
    }
    if (!out->X) return EPI_OK;
    const long long pg = (long long)(((int64_t)d->B * d->D + kSdPathWg - 1) / kSdPathWg);
    using PathKernel = void (*)(const SdArgs);
    static const PathKernel kernels[3][2] = {{sdraw_paths<0, 0>, sdraw_paths<0, 1>}, {sdraw_paths<1, 0>, sdraw_paths<1, 1>},
                                             {sdraw_paths<2, 0>, sdraw_paths<2, 1>}};
    const PathKernel kern = kernels[!in->z ? 0 : (d->z_f32 ? 2 : 1)][d->out_f32];
    for (long long w0 = 0; w0 < pg; w0 += cap) {
        g.wg0 = w0;
        const unsigned nb = (unsigned)(pg - w0 < cap ? pg - w0 : cap);
        if (nk && d->out_f32) hipLaunchKernelGGL(sdraw_paths_seeded<1>, dim3(nb), dim3(kSdPathWg), 0, st, g, *nk);
        else if (nk) hipLaunchKernelGGL(sdraw_paths_seeded<0>, dim3(nb), dim3(kSdPathWg), 0, st, g, *nk);
        else hipLaunchKernelGGL(kern, dim3(nb), dim3(kSdPathWg), 0, st, g);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "sdraw_paths launch");
    }
    return EPI_OK;
}

int epi_sdraw_run_device(const epi_sdraw_desc *d, const epi_sdraw_inputs *in, const epi_sdraw_outputs *out, void *ws, size_t ws_bytes,
                         void *stream, char *err)
{
    return sdraw_run_device(d, nullptr, in, out, ws, ws_bytes, stream, err);
}

int epi_sdraw_run_device_seeded(const epi_sdraw_desc *d, const epi_noise_desc *noise, const epi_sdraw_inputs *in, const epi_sdraw_outputs *out,
                                void *ws, size_t ws_bytes, void *stream, char *err)
{
    NoiseKey nk;
    int rc = noise_key(noise, in ? in->z : nullptr, &nk, err);
    if (rc != EPI_OK) return rc;
    return sdraw_run_device(d, &nk, in, out, ws, ws_bytes, stream, err);
}

static int sdraw_run_host(const epi_sdraw_desc *d, const epi_noise_desc *noise, const epi_sdraw_inputs *in, const epi_sdraw_outputs *out,
                          int device, char *err)
{
    int rc = epi_sdraw_validate(d, err);
    if (rc != EPI_OK) return rc;
    if ((rc = sdraw_check_arrays(in, out, err)) != EPI_OK) return rc;
    const size_t B = (size_t)d->B, T = (size_t)d->T, N = B * (size_t)d->D, Tk = T - (size_t)d->k0, none = HostIO::kAbsent;
    int gblk, gnblk;
    sdraw_geometry(d->B, d->lane_block, &gblk, &gnblk);
    const size_t Bp = (size_t)gnblk * (size_t)gblk, es = d->storage ? 4 : 8;
    HostIO io;
    const size_t o_sp = io.add_in(in->S_PLUS, T * 3, es, Bp, 0, Bp), o_pp = io.add_in(in->P_PLUS, T * 9, es, Bp, 0, Bp);
    const size_t o_sm = io.add_in(in->S_MINUS, T * 3, es, Bp, 0, Bp), o_pm = io.add_in(in->P_MINUS, T * 9, es, Bp, 0, Bp);
    const size_t o_prm = io.add_in(in->prm, (size_t)EPI_PRM_COUNT, 8, B, 0, B);
    const size_t o_z = in->z ? io.add_in(in->z, Tk * 3, d->z_f32 ? 4 : 8, N, 0, N) : none;
    const size_t o_st = in->s_term ? io.add_in(in->s_term, 3, 8, B, 0, B) : none, o_pt = in->P_term ? io.add_in(in->P_term, 9, 8, B, 0, B) : none;
    const size_t o_X = out->X ? io.add_out(out->X, Tk * 3, d->out_f32 ? 4 : 8, N, 0, N) : none;
    const size_t o_rk = out->rank ? io.add_out(out->rank, T, 4, B, 0, B) : none, o_ss = out->status ? io.add_out(out->status, 1, 4, B, 0, B) : none;
    const size_t o_J = out->J ? io.add_out(out->J, T * 9, 8, B, 0, B) : none, o_L = out->L ? io.add_out(out->L, T * 9, 8, B, 0, B) : none;
    const size_t wsb = T * B * (size_t)kSdRec * sizeof(double);
    const size_t o_ws = io.reserve(wsb);
    auto enqueue = [&](char *base, hipStream_t st) -> int {
        epi_sdraw_inputs din{};
        din.S_PLUS = base + o_sp; din.P_PLUS = base + o_pp; din.S_MINUS = base + o_sm; din.P_MINUS = base + o_pm;
        din.prm = HostIO::at<const double>(base, o_prm); din.z = HostIO::at<const char>(base, o_z);
        din.s_term = HostIO::at<const double>(base, o_st); din.P_term = HostIO::at<const double>(base, o_pt);
        epi_sdraw_outputs dout{};
        dout.X = HostIO::at<char>(base, o_X); dout.rank = HostIO::at<int32_t>(base, o_rk); dout.status = HostIO::at<int32_t>(base, o_ss);
        dout.J = HostIO::at<double>(base, o_J); dout.L = HostIO::at<double>(base, o_L);
        return noise ? epi_sdraw_run_device_seeded(d, noise, &din, &dout, base + o_ws, wsb, st, err)
                     : epi_sdraw_run_device(d, &din, &dout, base + o_ws, wsb, st, err);
    };
    return run_host(device, io, err, enqueue);
}

int epi_sdraw_run_host(const epi_sdraw_desc *d, const epi_sdraw_inputs *in, const epi_sdraw_outputs *out, int device, char *err)
{
    return sdraw_run_host(d, nullptr, in, out, device, err);
}

int epi_sdraw_run_host_seeded(const epi_sdraw_desc *d, const epi_noise_desc *noise, const epi_sdraw_inputs *in, const epi_sdraw_outputs *out,
                              int device, char *err)
{
    NoiseKey nk;
    int rc = noise_key(noise, in ? in->z : nullptr, &nk, err);   // before anything is staged: no z is copied
    if (rc != EPI_OK) return rc;
    return sdraw_run_host(d, noise, in, out, device, err);
}

// ---- standard-normal draws from a seed: noise_fill (noise.hpp) ----
int epi_noise_validate(const epi_noise_desc *d, char *err)
{
    if (!d) { set_err(err, "NULL noise descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->stream >= (1u << 30)) { set_err(err, "stream must be below 2^30"); return EPI_ERR_BAD_ARG; }
    return EPI_OK;
}

static int noise_fill_check(const epi_noise_desc *d, int64_t t0, int64_t nt, int32_t rows, int64_t lane0, int64_t n_lanes, int32_t out_f32,
                            const void *out, int32_t test_launch_groups, char *err)
{
    int rc = epi_noise_validate(d, err);
    if (rc != EPI_OK) return rc;
    if (rows != 1 && rows != 3) { set_err(err, "rows must be 1 or 3"); return EPI_ERR_BAD_ARG; }
    if (nt < 1 || n_lanes < 1) { set_err(err, "nt and n_lanes must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (t0 < 0 || t0 > ((int64_t)1 << 32) || nt > ((int64_t)1 << 32) - t0) { set_err(err, "t0 .. t0 + nt must lie in 0 .. 2^32 (t is one counter word)"); return EPI_ERR_BAD_ARG; }
    if (lane0 < 0 || n_lanes - 1 > INT64_MAX - lane0) { set_err(err, "lane0 .. lane0 + n_lanes must lie in 0 .. 2^63"); return EPI_ERR_BAD_ARG; }
    if (n_lanes > ((int64_t)1 << 62) / (3 * nt)) { set_err(err, "more than 2^62 elements"); return EPI_ERR_BAD_ARG; }
    if (out_f32 != 0 && out_f32 != 1) { set_err(err, "out_f32 must be 0 (double) or 1 (float)"); return EPI_ERR_BAD_ARG; }
    if (test_launch_groups < 0) { set_err(err, "test_launch_groups must be >= 0"); return EPI_ERR_BAD_ARG; }
    if (!out) { set_err(err, "NULL out"); return EPI_ERR_BAD_ARG; }
    return EPI_OK;
}

int epi_noise_fill_device(const epi_noise_desc *d, int64_t t0, int64_t nt, int32_t rows, int64_t lane0, int64_t n_lanes, int32_t out_f32,
                          void *out, int32_t test_launch_groups, void *stream, char *err)
{
    int rc = noise_fill_check(d, t0, nt, rows, lane0, n_lanes, out_f32, out, test_launch_groups, err);
    if (rc != EPI_OK) return rc;
    NoiseFillArgs a{};
    a.nk.seed_lo = d->seed_lo; a.nk.seed_hi = d->seed_hi; a.nk.stream = d->stream;
    a.rows = rows; a.f32 = out_f32; a.t0 = (uint32_t)t0; a.lane0 = (uint64_t)lane0; a.n_lanes = (uint64_t)n_lanes;
    a.items = (uint64_t)nt * (uint64_t)((rows + 1) / 2) * (uint64_t)n_lanes;
    a.out = out;
    const long long cap = test_launch_groups > 0 ? (long long)test_launch_groups : kNoiseLaunchGroups;
    const long long groups = (long long)((a.items + kNoiseWg - 1) / kNoiseWg);
    for (long long w0 = 0; w0 < groups; w0 += cap) {                  // in slices, as sdraw's
        a.wg0 = w0;
        const unsigned nb = (unsigned)(groups - w0 < cap ? groups - w0 : cap);
        hipLaunchKernelGGL(noise_fill, dim3(nb), dim3(kNoiseWg), 0, (hipStream_t)stream, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(err, e, "noise_fill launch");
    }
    return EPI_OK;
}

int epi_noise_fill_host(const epi_noise_desc *d, int64_t t0, int64_t nt, int32_t rows, int64_t lane0, int64_t n_lanes, int32_t out_f32,
                        void *out, int device, char *err)
{
    int rc = noise_fill_check(d, t0, nt, rows, lane0, n_lanes, out_f32, out, 0, err);
    if (rc != EPI_OK) return rc;
    HostIO io;
    const size_t o_out = io.add_out(out, (size_t)nt * (size_t)rows, out_f32 ? 4 : 8, (size_t)n_lanes, 0, (size_t)n_lanes);
    auto enqueue = [&](char *base, hipStream_t st) -> int {
        return epi_noise_fill_device(d, t0, nt, rows, lane0, n_lanes, out_f32, base + o_out, 0, st, err);
    };
    return run_host(device, io, err, enqueue);
}

// ---- probabilistic forecast scores of the ensembles: escore_items, then escore_regions (ens_score.hpp) ----
static int escore_check_desc(const epi_escore_desc *d, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->T < 1) { set_err(err, "T must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->rows < 1) { set_err(err, "rows must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->R < 1) { set_err(err, "R must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->Rt < 1) { set_err(err, "Rt must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->D < 1 || d->D > kEnsMaxD) { set_err(err, "D must lie in 1 .. 4096 (a wavefront holds the draws of an item in registers)"); return EPI_ERR_BAD_ARG; }
    if ((int64_t)d->R * d->D > (int64_t)0x7fffffff) { set_err(err, "R * D is limited to 2^31 - 1"); return EPI_ERR_BAD_ARG; }
    if (d->n_a < 0 || d->n_a > kEsMaxA) { set_err(err, "n_a must lie in 0 .. 8"); return EPI_ERR_BAD_ARG; }
    if (d->n_bins < 0 || d->n_bins > kEsMaxBins) { set_err(err, "n_bins must lie in 0 .. 32"); return EPI_ERR_BAD_ARG; }
    for (int k = 0; k < d->n_a; k++) {
        if (!(d->alpha[k] > 0.0 && d->alpha[k] < 1.0)) { set_err(err, "every alpha must lie in (0, 1)"); return EPI_ERR_BAD_ARG; }
        if (k && !(d->alpha[k] < d->alpha[k - 1])) { set_err(err, "alpha must be strictly descending"); return EPI_ERR_BAD_ARG; }
    }
    if (d->k0 < 0 || d->k1 < d->k0 || d->k1 > d->T) { set_err(err, "k0, k1 must satisfy 0 <= k0 <= k1 <= T"); return EPI_ERR_BAD_ARG; }
    if (d->storage != 0 && d->storage != 1) { set_err(err, "storage must be 0 (double) or 1 (float)"); return EPI_ERR_BAD_ARG; }
    if (d->derive_newcases != 0 && d->derive_newcases != 1) { set_err(err, "derive_newcases must be 0 or 1"); return EPI_ERR_BAD_ARG; }
    if (d->derive_newcases && d->rows < 3) { set_err(err, "derive_newcases needs at least 3 rows"); return EPI_ERR_BAD_ARG; }
    if (d->test_launch_items < 0) { set_err(err, "test_launch_items must be >= 0"); return EPI_ERR_BAD_ARG; }
    return EPI_OK;
}

static bool escore_wants_regions(const epi_escore_outputs *o)
{
    return o->crps_mean || o->wis_mean || o->ae_mean || o->n_scored || o->cover_frac || o->pit_hist;
}

int epi_escore_validate(const epi_escore_desc *d, const epi_escore_inputs *in, const epi_escore_outputs *out, char *err)
{
    int rc = escore_check_desc(d, err);
    if (rc != EPI_OK) return rc;
    if (!in || !out) { set_err(err, "NULL inputs / outputs"); return EPI_ERR_BAD_ARG; }
    if (!in->src) { set_err(err, "NULL src"); return EPI_ERR_BAD_ARG; }
    if (!in->truth) { set_err(err, "NULL truth"); return EPI_ERR_BAD_ARG; }
    if (d->derive_newcases && !in->population) { set_err(err, "NULL population (derive_newcases)"); return EPI_ERR_BAD_ARG; }
    if (!in->truth_series && d->Rt != d->R) { set_err(err, "without truth_series, truth must hold R columns (Rt = R)"); return EPI_ERR_BAD_ARG; }
    if (out->pit_hist && d->n_bins < 1) { set_err(err, "pit_hist needs n_bins >= 1"); return EPI_ERR_BAD_ARG; }
    if (!(out->crps || out->wis || out->ae || out->width || out->rank || out->ties || out->cover || out->count || escore_wants_regions(out))) {
        set_err(err, "no output requested");
        return EPI_ERR_BAD_ARG;
    }
    return EPI_OK;
}

// the workspace: crps, wis, ae (doubles), then rank, ties, cover, count (int32), each one element per item
static size_t escore_ws_bytes(const epi_escore_desc *d)
{
    return (size_t)d->T * (size_t)(d->rows + d->derive_newcases) * (size_t)d->R * (3 * sizeof(double) + 4 * sizeof(int32_t));
}

int epi_escore_workspace_bytes(const epi_escore_desc *d, size_t *bytes, char *err)
{
    int rc = escore_check_desc(d, err);
    if (rc != EPI_OK) return rc;
    if (!bytes) { set_err(err, "NULL bytes"); return EPI_ERR_BAD_ARG; }
    *bytes = escore_ws_bytes(d);
    return EPI_OK;
}

int epi_escore_run_device(const epi_escore_desc *d, const epi_escore_inputs *in, const epi_escore_outputs *out, void *ws,
                          size_t ws_bytes, void *stream, char *err)
{
    int rc = epi_escore_validate(d, in, out, err);
    if (rc != EPI_OK) return rc;
    const bool regions = escore_wants_regions(out);
    if (regions && (!ws || ws_bytes < escore_ws_bytes(d))) { set_err(err, "workspace too small (epi_escore_workspace_bytes)"); return EPI_ERR_WORKSPACE; }
    EsArgs g{};
    g.T = d->T; g.rows = d->rows; g.rows_out = d->rows + d->derive_newcases; g.R = d->R; g.D = d->D; g.Rt = d->Rt;
    g.n_a = d->n_a; g.n_bins = d->n_bins; g.f32 = d->storage; g.derive = d->derive_newcases; g.k0 = d->k0; g.k1 = d->k1;
    g.src = in->src; g.population = in->population; g.truth = in->truth; g.truth_series = in->truth_series; g.first_day = in->first_day;
    for (int k = 0; k < d->n_a; k++) {                               // the probabilities, once, in double
        g.alpha[k] = d->alpha[k];
        g.q_lo[k] = d->alpha[k] / 2.0;
        g.q_hi[k] = 1.0 - d->alpha[k] / 2.0;
    }
    const int64_t items = (int64_t)d->T * g.rows_out * d->R;
    g.crps = out->crps; g.wis = out->wis; g.ae = out->ae; g.width = out->width;
    g.rank = out->rank; g.ties = out->ties; g.cover = out->cover; g.count = out->count;
    if (regions) {                                                   // what the region pass reads and the caller did not ask for
        double *wd = (double *)ws;
        int32_t *wi = (int32_t *)(wd + 3 * (size_t)items);
        if (!g.crps && out->crps_mean) g.crps = wd;
        if (!g.wis && out->wis_mean) g.wis = wd + (size_t)items;
        if (!g.ae && out->ae_mean) g.ae = wd + 2 * (size_t)items;
        if (!g.rank) g.rank = wi;
        if (!g.ties && out->pit_hist) g.ties = wi + (size_t)items;
        if (!g.cover && out->cover_frac) g.cover = wi + 2 * (size_t)items;
        if (!g.count && out->pit_hist) g.count = wi + 3 * (size_t)items;
    }
    g.crps_mean = out->crps_mean; g.wis_mean = out->wis_mean; g.ae_mean = out->ae_mean; g.n_scored = out->n_scored;
    g.cover_frac = out->cover_frac; g.pit_hist = out->pit_hist;
    const hipStream_t st = (hipStream_t)stream;
    const int64_t cap = d->test_launch_items > 0 ? (int64_t)d->test_launch_items : kEnsLaunchItems;
    hipError_t e = hipSuccess;
    for (int64_t i0 = 0; i0 < items && e == hipSuccess; i0 += cap) {  // one 64-lane workgroup per item, in slices, as sdraw's (ens_score.hpp)
        g.item0 = (long long)i0;
        const unsigned ni = (unsigned)(items - i0 < cap ? items - i0 : cap);
        if (d->D <= 64) e = escore_launch<1>(g, ni, st);              // registers per lane: P / 64, P the power of two >= D
        else if (d->D <= 128) e = escore_launch<2>(g, ni, st);
        else if (d->D <= 256) e = escore_launch<4>(g, ni, st);
        else if (d->D <= 512) e = escore_launch<8>(g, ni, st);
        else if (d->D <= 1024) e = escore_launch<16>(g, ni, st);
        else if (d->D <= 2048) e = escore_launch<32>(g, ni, st);
        else e = escore_launch<64>(g, ni, st);
    }
    if (e != hipSuccess) return hip_fail(err, e, "escore_items launch");
    if (!regions) return EPI_OK;
    const int64_t lanes = (int64_t)g.rows_out * d->R;                // < 2^31 * 4097 / D: one launch (R * D <= INT32_MAX, rows' small)
    hipLaunchKernelGGL(escore_regions, dim3((unsigned)((lanes + kEsRegionWg - 1) / kEsRegionWg)), dim3(kEsRegionWg), 0, st, g);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "escore_regions launch");
    return EPI_OK;
}

int epi_escore_run_host(const epi_escore_desc *d, const epi_escore_inputs *in, const epi_escore_outputs *out, int device, char *err)
{
    int rc = epi_escore_validate(d, in, out, err);
    if (rc != EPI_OK) return rc;
    const size_t R = (size_t)d->R, B = R * (size_t)d->D, T = (size_t)d->T, ro = (size_t)(d->rows + d->derive_newcases), Rt = (size_t)d->Rt;
    const size_t na = (size_t)d->n_a, nb = (size_t)d->n_bins, none = HostIO::kAbsent;
    HostIO io;
    const size_t o_src = io.add_in(in->src, T * (size_t)d->rows, d->storage ? 4 : 8, B, 0, B);
    const size_t o_pop = d->derive_newcases ? io.add_in(in->population, 1, 8, R, 0, R) : none;
    const size_t o_tr = io.add_in(in->truth, T * ro, 8, Rt, 0, Rt);
    const size_t o_ts = in->truth_series ? io.add_in(in->truth_series, 1, 4, R, 0, R) : none;
    const size_t o_fd = in->first_day ? io.add_in(in->first_day, 1, 4, R, 0, R) : none;
    using EO = epi_escore_outputs;
    const HostIO::Opt<EO, double> f64[8] = {{&EO::crps, T * ro}, {&EO::wis, T * ro}, {&EO::ae, T * ro}, {&EO::width, T * na * ro},
                                            {&EO::crps_mean, ro}, {&EO::wis_mean, ro}, {&EO::ae_mean, ro}, {&EO::cover_frac, na * ro}};
    const HostIO::Opt<EO, int32_t> i32[6] = {{&EO::rank, T * ro}, {&EO::ties, T * ro}, {&EO::cover, T * ro}, {&EO::count, T * ro},
                                             {&EO::n_scored, ro}, {&EO::pit_hist, nb * ro}};
    size_t o_d[8], o_i[6];
    io.add_opt(*out, f64, o_d, R);
    io.add_opt(*out, i32, o_i, R);
    const size_t wsb = escore_ws_bytes(d);
    const size_t o_ws = escore_wants_regions(out) ? io.reserve(wsb) : none;
    auto enqueue = [&](char *base, hipStream_t st) -> int {
        epi_escore_inputs din{};
        din.src = base + o_src; din.population = HostIO::at<const double>(base, o_pop); din.truth = (const double *)(base + o_tr);
        din.truth_series = HostIO::at<const int32_t>(base, o_ts); din.first_day = HostIO::at<const int32_t>(base, o_fd);
        epi_escore_outputs dout{};
        HostIO::bind_opt(dout, f64, o_d, base);
        HostIO::bind_opt(dout, i32, o_i, base);
        return epi_escore_run_device(d, &din, &dout, HostIO::at<char>(base, o_ws), wsb, st, err);
    };
    return run_host(device, io, err, enqueue);
}

// ---- path functionals of the ensembles: pathfn_paths, pathfn_combine over time segments, pathfn_regions (path_functionals.hpp) ----
// The segment rule (profiles/path_functionals/segments.json): a path grid of fewer wavefronts than the device has
// SIMDs (kPfSegWaves) is cut into kPfSegMost segments of whole 32-day blocks; at 1 200 wavefronts the cut gains nothing, at 4 800 it
// costs a third.
constexpr long long kPfSegWaves = 1024;
constexpr int kPfSegMost = 8;

static void pathfn_geometry(const epi_pathfn_desc *d, int *nseg, int *seg_days, int *nblk)
{
    const int W = d->k1 - d->k0, nb = (W + kPfBlock - 1) / kPfBlock;
    long long want = d->test_segments;
    if (want <= 0) {
        const long long groups = d->derive_newcases ? (long long)d->rows - 2 : (long long)d->rows;
        const long long waves = (((long long)d->R * d->D + 63) / 64) * groups;
        want = waves >= kPfSegWaves ? 1 : kPfSegMost;
    }
    if (want > nb) want = nb;
    const int per = (int)((nb + want - 1) / want);                    // blocks of a segment
    *nseg = (nb + per - 1) / per;                                     // no empty segment
    *seg_days = per * kPfBlock;
    *nblk = nb;
}

static int pathfn_check_desc(const epi_pathfn_desc *d, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->T < 1) { set_err(err, "T must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->rows < 1 || d->rows > 4096) { set_err(err, "rows must lie in 1 .. 4096"); return EPI_ERR_BAD_ARG; }
    if (d->R < 1) { set_err(err, "R must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->D < 1) { set_err(err, "D must be >= 1"); return EPI_ERR_BAD_ARG; }
    if ((int64_t)d->R * d->D > (int64_t)0x7fffffff) { set_err(err, "R * D is limited to 2^31 - 1"); return EPI_ERR_BAD_ARG; }
    if (d->n_thr < 0 || d->n_thr > kPfMaxThr) { set_err(err, "n_thr must lie in 0 .. 8"); return EPI_ERR_BAD_ARG; }
    if (d->k0 < 0 || d->k1 <= d->k0 || d->k1 > d->T) { set_err(err, "k0, k1 must satisfy 0 <= k0 < k1 <= T"); return EPI_ERR_BAD_ARG; }
    if (d->storage != 0 && d->storage != 1) { set_err(err, "storage must be 0 (double) or 1 (float)"); return EPI_ERR_BAD_ARG; }
    if (d->derive_newcases != 0 && d->derive_newcases != 1) { set_err(err, "derive_newcases must be 0 or 1"); return EPI_ERR_BAD_ARG; }
    if (d->derive_newcases && d->rows < 3) { set_err(err, "derive_newcases needs at least 3 rows"); return EPI_ERR_BAD_ARG; }
    const int nb = (d->k1 - d->k0 + kPfBlock - 1) / kPfBlock;
    if (d->test_segments < 0 || d->test_segments > (nb < kPfMaxSeg ? nb : kPfMaxSeg)) {
        set_err(err, "test_segments must lie in 0 .. min(ceil((k1 - k0) / 32), 1024): a segment is whole 32-day blocks");
        return EPI_ERR_BAD_ARG;
    }
    if (d->test_launch_groups < 0) { set_err(err, "test_launch_groups must be >= 0"); return EPI_ERR_BAD_ARG; }
    return EPI_OK;
}

static bool pathfn_wants_regions(const epi_pathfn_outputs *o)
{
    return o->n_paths || o->peak_day_hist || o->n_cross || o->cross_day_hist;
}

int epi_pathfn_validate(const epi_pathfn_desc *d, const epi_pathfn_inputs *in, const epi_pathfn_outputs *out, char *err)
{
    int rc = pathfn_check_desc(d, err);
    if (rc != EPI_OK) return rc;
    if (!in || !out) { set_err(err, "NULL inputs / outputs"); return EPI_ERR_BAD_ARG; }
    if (!in->src) { set_err(err, "NULL src"); return EPI_ERR_BAD_ARG; }
    if (d->derive_newcases && !in->population) { set_err(err, "NULL population (derive_newcases)"); return EPI_ERR_BAD_ARG; }
    if (d->n_thr > 0 && !in->thr) { set_err(err, "NULL thr (n_thr > 0)"); return EPI_ERR_BAD_ARG; }
    if (d->n_thr == 0 && (out->first_cross || out->days_above || out->longest_run || out->n_cross || out->cross_day_hist)) {
        set_err(err, "first_cross, days_above, longest_run, n_cross and cross_day_hist need n_thr >= 1");
        return EPI_ERR_BAD_ARG;
    }
    if ((out->peak_day_hist || out->cross_day_hist) && d->k1 - d->k0 > kPfMaxW) {
        set_err(err, "a histogram holds at most 4096 days (k1 - k0): its bins live in LDS");
        return EPI_ERR_BAD_ARG;
    }
    if (!(out->peak_value || out->peak_day || out->min_value || out->min_day || out->total || out->first_cross || out->days_above ||
          out->longest_run || out->n_valid || pathfn_wants_regions(out))) {
        set_err(err, "no output requested");
        return EPI_ERR_BAD_ARG;
    }
    return EPI_OK;
}

// the workspace in doubles, then int32: peak_day [M], first_cross [n_thr][M]; with segments p_mx, p_mn [nseg][M], p_bsum [nblk][M],
// then p_int [nseg][3][M], p_thr [nseg][5][n_thr][M]
static size_t pathfn_ws_bytes(const epi_pathfn_desc *d)
{
    int nseg, seg_days, nblk;
    pathfn_geometry(d, &nseg, &seg_days, &nblk);
    const size_t M = (size_t)(d->rows + d->derive_newcases) * (size_t)d->R * (size_t)d->D, nt = (size_t)d->n_thr;
    size_t n = (1 + nt) * M * sizeof(double);
    if (nseg > 1) n += (2 * (size_t)nseg + (size_t)nblk) * M * sizeof(double) + (size_t)nseg * (3 + 5 * nt) * M * sizeof(int32_t);
    return n;
}

int epi_pathfn_workspace_bytes(const epi_pathfn_desc *d, size_t *bytes, char *err)
{
    int rc = pathfn_check_desc(d, err);
    if (rc != EPI_OK) return rc;
    if (!bytes) { set_err(err, "NULL bytes"); return EPI_ERR_BAD_ARG; }
    *bytes = pathfn_ws_bytes(d);
    return EPI_OK;
}

int epi_pathfn_run_device(const epi_pathfn_desc *d, const epi_pathfn_inputs *in, const epi_pathfn_outputs *out, void *ws,
                          size_t ws_bytes, void *stream, char *err)
{
    int rc = epi_pathfn_validate(d, in, out, err);
    if (rc != EPI_OK) return rc;
    PfArgs g{};
    pathfn_geometry(d, &g.nseg, &g.seg_days, &g.nblk);
    const bool regions = pathfn_wants_regions(out);
    if ((regions || g.nseg > 1) && (!ws || ws_bytes < pathfn_ws_bytes(d))) { set_err(err, "workspace too small (epi_pathfn_workspace_bytes)"); return EPI_ERR_WORKSPACE; }
    g.T = d->T; g.rows = d->rows; g.rows_out = d->rows + d->derive_newcases; g.R = d->R; g.D = d->D; g.n_thr = d->n_thr;
    g.derive = d->derive_newcases; g.k0 = d->k0; g.k1 = d->k1;
    g.src = in->src; g.population = in->population; g.thr = in->thr; g.first_day = in->first_day;
    g.peak_value = out->peak_value; g.peak_day = out->peak_day; g.min_value = out->min_value; g.min_day = out->min_day;
    g.total = out->total; g.first_cross = out->first_cross; g.days_above = out->days_above; g.longest_run = out->longest_run;
    g.n_valid = out->n_valid; g.n_paths = out->n_paths; g.peak_day_hist = out->peak_day_hist; g.n_cross = out->n_cross;
    g.cross_day_hist = out->cross_day_hist;
    const size_t N = (size_t)d->R * (size_t)d->D, M = (size_t)g.rows_out * N, nt = (size_t)d->n_thr;
    double *wd = (double *)ws;
    if (!g.peak_day && (out->n_paths || out->peak_day_hist)) g.peak_day = wd;     // what the region pass reads and the caller did not ask for
    if (!g.first_cross && (out->n_cross || out->cross_day_hist)) g.first_cross = wd + M;
    if (g.nseg > 1) {
        g.p_mx = wd + (1 + nt) * M;
        g.p_mn = g.p_mx + (size_t)g.nseg * M;
        g.p_bsum = g.p_mn + (size_t)g.nseg * M;
        g.p_int = (int32_t *)(g.p_bsum + (size_t)g.nblk * M);
        g.p_thr = g.p_int + (size_t)g.nseg * 3 * M;
    }
    const hipStream_t st = (hipStream_t)stream;
    const long long cap = d->test_launch_groups > 0 ? (long long)d->test_launch_groups : kPfLaunchGroups;
    const long long pg = (long long)((N + kPfPathWg - 1) / kPfPathWg);
    using PathKernel = void (*)(const PfArgs);
    // NT: the compile-time bound on n_thr, in the buckets 0, 2 and 8 (their registers)
#define EPI_PF_ROW(F, NT) {{pathfn_paths<F, NT, 1, 0>, pathfn_paths<F, NT, 1, 1>}, {pathfn_paths<F, NT, 4, 0>, pathfn_paths<F, NT, 4, 1>}}
    static const PathKernel paths[2][3][2][2] = {{EPI_PF_ROW(0, 0), EPI_PF_ROW(0, 2), EPI_PF_ROW(0, 8)},
                                                 {EPI_PF_ROW(1, 0), EPI_PF_ROW(1, 2), EPI_PF_ROW(1, 8)}};   // [storage][bucket][NR = 4][segments]
#undef EPI_PF_ROW
    static const PathKernel combine[3] = {pathfn_combine<0>, pathfn_combine<2>, pathfn_combine<8>};
    const int bucket = d->n_thr == 0 ? 0 : (d->n_thr <= 2 ? 1 : 2), seg = g.nseg > 1 ? 1 : 0;
    hipError_t e = hipSuccess;
    // the path grid, in launches of its own loop (as sdraw's): grid.y the segments, grid.z the row groups
    auto launch_paths = [&](PathKernel kern, int row0, int nz) {
        const long long per = cap / ((long long)g.nseg * nz) > 0 ? cap / ((long long)g.nseg * nz) : 1;
        g.row0 = row0;
        for (long long w0 = 0; w0 < pg && e == hipSuccess; w0 = w0 + per) {
            g.group0 = w0;
            const unsigned nb = (unsigned)(pg - w0 < per ? pg - w0 : per);
            hipLaunchKernelGGL(kern, dim3(nb, (unsigned)g.nseg, (unsigned)nz), dim3(kPfPathWg), 0, st, g);
            e = hipGetLastError();
        }
    };
    if (d->derive_newcases) {
        launch_paths(paths[d->storage][bucket][1][seg], 0, 1);
        if (e == hipSuccess && d->rows > 3) launch_paths(paths[d->storage][bucket][0][seg], 3, d->rows - 3);
    } else {
        launch_paths(paths[d->storage][bucket][0][seg], 0, d->rows);
    }
    if (e != hipSuccess) return hip_fail(err, e, "pathfn_paths launch");
    if (g.nseg > 1) {
        const long long per = cap / g.rows_out > 0 ? cap / g.rows_out : 1;
        for (long long w0 = 0; w0 < pg; w0 = w0 + per) {
            g.group0 = w0;
            const unsigned nb = (unsigned)(pg - w0 < per ? pg - w0 : per);
            hipLaunchKernelGGL(combine[bucket], dim3(nb, (unsigned)g.rows_out), dim3(kPfPathWg), 0, st, g);
            if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "pathfn_combine launch");
        }
    }
    if (!regions) return EPI_OK;
    const long long rg = (long long)((out->n_cross || out->cross_day_hist) ? 1 + d->n_thr : 1) * g.rows_out * d->R;
    for (long long w0 = 0; w0 < rg; w0 = w0 + cap) {
        g.group0 = w0;
        const unsigned nb = (unsigned)(rg - w0 < cap ? rg - w0 : cap);
        hipLaunchKernelGGL(pathfn_regions, dim3(nb), dim3(kPfRegionWg), 0, st, g);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "pathfn_regions launch");
    }
    return EPI_OK;
}

int epi_pathfn_run_host(const epi_pathfn_desc *d, const epi_pathfn_inputs *in, const epi_pathfn_outputs *out, int device, char *err)
{
    int rc = epi_pathfn_validate(d, in, out, err);
    if (rc != EPI_OK) return rc;
    const size_t R = (size_t)d->R, N = R * (size_t)d->D, T = (size_t)d->T, ro = (size_t)(d->rows + d->derive_newcases);
    const size_t nt = (size_t)d->n_thr, W = (size_t)(d->k1 - d->k0), none = HostIO::kAbsent;
    HostIO io;
    const size_t o_src = io.add_in(in->src, T * (size_t)d->rows, d->storage ? 4 : 8, N, 0, N);
    const size_t o_pop = d->derive_newcases ? io.add_in(in->population, 1, 8, R, 0, R) : none;
    const size_t o_thr = nt ? io.add_in(in->thr, nt * ro, 8, R, 0, R) : none;
    const size_t o_fd = in->first_day ? io.add_in(in->first_day, 1, 4, R, 0, R) : none;
    using PO = epi_pathfn_outputs;
    const HostIO::Opt<PO, double> f64[8] = {{&PO::peak_value, ro}, {&PO::peak_day, ro}, {&PO::min_value, ro}, {&PO::min_day, ro},
                                            {&PO::total, ro}, {&PO::first_cross, nt * ro}, {&PO::days_above, nt * ro},
                                            {&PO::longest_run, nt * ro}};
    const HostIO::Opt<PO, int32_t> i32p[1] = {{&PO::n_valid, ro}};
    const HostIO::Opt<PO, int32_t> i32r[4] = {{&PO::n_paths, ro}, {&PO::peak_day_hist, W * ro}, {&PO::n_cross, nt * ro},
                                              {&PO::cross_day_hist, W * nt * ro}};
    size_t o_d[8], o_p[1], o_r[4];
    io.add_opt(*out, f64, o_d, N);
    io.add_opt(*out, i32p, o_p, N);
    io.add_opt(*out, i32r, o_r, R);
    int nseg, seg_days, nblk;
    pathfn_geometry(d, &nseg, &seg_days, &nblk);
    const size_t wsb = pathfn_ws_bytes(d);
    const size_t o_ws = (pathfn_wants_regions(out) || nseg > 1) ? io.reserve(wsb) : none;
    auto enqueue = [&](char *base, hipStream_t st) -> int {
        epi_pathfn_inputs din{};
        din.src = base + o_src; din.population = HostIO::at<const double>(base, o_pop); din.thr = HostIO::at<const double>(base, o_thr);
        din.first_day = HostIO::at<const int32_t>(base, o_fd);
        epi_pathfn_outputs dout{};
        HostIO::bind_opt(dout, f64, o_d, base);
        HostIO::bind_opt(dout, i32p, o_p, base);
        HostIO::bind_opt(dout, i32r, o_r, base);
        return epi_pathfn_run_device(d, &din, &dout, HostIO::at<char>(base, o_ws), wsb, st, err);
    };
    return run_host(device, io, err, enqueue);
}

// ---- joint scores of the ensembles: ejoint_members, ejoint_pairs, ejoint_vario, ejoint_final (ens_joint.hpp) ----
static int ejoint_check_desc(const epi_ejoint_desc *d, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->T < 1) { set_err(err, "T must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->rows < 1) { set_err(err, "rows must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->R < 1) { set_err(err, "R must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->Rt < 1) { set_err(err, "Rt must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->D < 1 || d->D > kEnsMaxD) { set_err(err, "D must lie in 1 .. 4096 (a wavefront holds the draws of an item in registers)"); return EPI_ERR_BAD_ARG; }
    if ((int64_t)d->R * d->D > (int64_t)0x7fffffff) { set_err(err, "R * D is limited to 2^31 - 1"); return EPI_ERR_BAD_ARG; }
    if (d->k0 < 0 || d->k1 < d->k0 || d->k1 > d->T) { set_err(err, "k0, k1 must satisfy 0 <= k0 <= k1 <= T"); return EPI_ERR_BAD_ARG; }
    if (d->storage != 0 && d->storage != 1) { set_err(err, "storage must be 0 (double) or 1 (float)"); return EPI_ERR_BAD_ARG; }
    if (d->derive_newcases != 0 && d->derive_newcases != 1) { set_err(err, "derive_newcases must be 0 or 1"); return EPI_ERR_BAD_ARG; }
    if (d->derive_newcases && d->rows < 3) { set_err(err, "derive_newcases needs at least 3 rows"); return EPI_ERR_BAD_ARG; }
    if (d->vs_order < 0 || d->vs_order > 2) { set_err(err, "vs_order must be 0 (no variogram score), 1 (p = 0.5) or 2 (p = 1)"); return EPI_ERR_BAD_ARG; }
    if (d->max_lag < 0) { set_err(err, "max_lag must be >= 0 (0: every lag)"); return EPI_ERR_BAD_ARG; }
    if (d->test_launch_tiles < 0) { set_err(err, "test_launch_tiles must be >= 0"); return EPI_ERR_BAD_ARG; }
    const int64_t items = (int64_t)(d->rows + d->derive_newcases) * d->R, nb = (d->D + 63) / 64, tiles = nb * (nb + 1) / 2, wcap = d->k1 - d->k0;
    if (items > (int64_t)0x7fffffff) { set_err(err, "(rows + derive_newcases) * R is limited to 2^31 - 1"); return EPI_ERR_BAD_ARG; }
    if (items * (tiles > wcap ? tiles : wcap) > ((int64_t)1 << 40)) {
        set_err(err, "(rows + derive_newcases) * R * max(tiles, k1 - k0) is limited to 2^40 (the workspace holds a double for each)");
        return EPI_ERR_BAD_ARG;
    }
    return EPI_OK;
}

int epi_ejoint_validate(const epi_ejoint_desc *d, const epi_ejoint_inputs *in, const epi_ejoint_outputs *out, char *err)
{
    int rc = ejoint_check_desc(d, err);
    if (rc != EPI_OK) return rc;
    if (!in || !out) { set_err(err, "NULL inputs / outputs"); return EPI_ERR_BAD_ARG; }
    if (!in->src) { set_err(err, "NULL src"); return EPI_ERR_BAD_ARG; }
    if (!in->truth) { set_err(err, "NULL truth"); return EPI_ERR_BAD_ARG; }
    if (d->derive_newcases && !in->population) { set_err(err, "NULL population (derive_newcases)"); return EPI_ERR_BAD_ARG; }
    if (!in->truth_series && d->Rt != d->R) { set_err(err, "without truth_series, truth must hold R columns (Rt = R)"); return EPI_ERR_BAD_ARG; }
    if (out->vs && d->vs_order == 0) { set_err(err, "vs needs vs_order 1 (p = 0.5) or 2 (p = 1)"); return EPI_ERR_BAD_ARG; }
    if (!(out->es || out->truth_term || out->spread_term || out->vs || out->n_members || out->n_days || out->member_dist)) {
        set_err(err, "no output requested");
        return EPI_ERR_BAD_ARG;
    }
    return EPI_OK;
}

static size_t ejoint_ws_bytes(const epi_ejoint_desc *d)
{
    const size_t nb = (size_t)(d->D + 63) / 64;
    return ejoint_ws_size((size_t)(d->rows + d->derive_newcases) * (size_t)d->R, nb, nb * (nb + 1) / 2, (size_t)(d->k1 - d->k0));
}

int epi_ejoint_workspace_bytes(const epi_ejoint_desc *d, size_t *bytes, char *err)
{
    int rc = ejoint_check_desc(d, err);
    if (rc != EPI_OK) return rc;
    if (!bytes) { set_err(err, "NULL bytes"); return EPI_ERR_BAD_ARG; }
    *bytes = ejoint_ws_bytes(d);
    return EPI_OK;
}

int epi_ejoint_run_device(const epi_ejoint_desc *d, const epi_ejoint_inputs *in, const epi_ejoint_outputs *out, void *ws,
                          size_t ws_bytes, void *stream, char *err)
{
    int rc = epi_ejoint_validate(d, in, out, err);
    if (rc != EPI_OK) return rc;
    if (!ws || ws_bytes < ejoint_ws_bytes(d)) { set_err(err, "workspace too small (epi_ejoint_workspace_bytes)"); return EPI_ERR_WORKSPACE; }
    EjArgs g{};
    g.T = d->T; g.rows = d->rows; g.rows_out = d->rows + d->derive_newcases; g.R = d->R; g.D = d->D; g.Rt = d->Rt;
    g.f32 = d->storage; g.derive = d->derive_newcases; g.k0 = d->k0; g.k1 = d->k1; g.vs_order = d->vs_order; g.max_lag = d->max_lag;
    g.nb = (d->D + 63) / 64; g.tiles = g.nb * (g.nb + 1) / 2; g.wcap = d->k1 - d->k0;
    g.src = in->src; g.population = in->population; g.truth = in->truth; g.truth_series = in->truth_series; g.first_day = in->first_day;
    const size_t items = (size_t)g.rows_out * (size_t)d->R;
    const bool pairs = out->es || out->spread_term, vario = out->vs != nullptr;
    ejoint_carve(g, ws, items, pairs, vario);
    g.es = out->es; g.truth_term = out->truth_term; g.spread_term = out->spread_term; g.vs = out->vs;
    g.n_members = out->n_members; g.n_days = out->n_days; g.member_dist = out->member_dist;
    const hipStream_t st = (hipStream_t)stream;
    const long long cap = d->test_launch_tiles > 0 ? (long long)d->test_launch_tiles : (long long)kEnsLaunchItems;
    auto run = [&](int which, long long units) {                      // one 64-lane workgroup per unit, in launches below 2^31 threads
        return ejoint_for_units(units, cap, [&](long long u0, long long nu) {
            g.unit0 = u0; g.units = nu;
            return (int)ejoint_launch(which, g, (unsigned)nu, st);
        });
    };
    int e = run(0, (long long)items);
    if (e) return hip_fail(err, (hipError_t)e, "ejoint_members launch");
    if (pairs && (e = run(2, (long long)items * g.tiles))) return hip_fail(err, (hipError_t)e, "ejoint_pairs launch");
    if (vario && g.wcap > 0 && (e = run(1, (long long)items * g.wcap))) return hip_fail(err, (hipError_t)e, "ejoint_vario launch");
    if (out->es || out->truth_term || out->spread_term || out->vs || out->n_members || out->n_days) {
        hipLaunchKernelGGL(ejoint_final, dim3((unsigned)((items + kEjFinalWg - 1) / kEjFinalWg)), dim3(kEjFinalWg), 0, st, g);
        const hipError_t f = hipGetLastError();
        if (f != hipSuccess) return hip_fail(err, f, "ejoint_final launch");
    }
    return EPI_OK;
}

int epi_ejoint_run_host(const epi_ejoint_desc *d, const epi_ejoint_inputs *in, const epi_ejoint_outputs *out, int device, char *err)
{
    int rc = epi_ejoint_validate(d, in, out, err);
    if (rc != EPI_OK) return rc;
    const size_t R = (size_t)d->R, B = R * (size_t)d->D, T = (size_t)d->T, ro = (size_t)(d->rows + d->derive_newcases), Rt = (size_t)d->Rt;
    const size_t none = HostIO::kAbsent;
    HostIO io;
    const size_t o_src = io.add_in(in->src, T * (size_t)d->rows, d->storage ? 4 : 8, B, 0, B);
    const size_t o_pop = d->derive_newcases ? io.add_in(in->population, 1, 8, R, 0, R) : none;
    const size_t o_tr = io.add_in(in->truth, T * ro, 8, Rt, 0, Rt);
    const size_t o_ts = in->truth_series ? io.add_in(in->truth_series, 1, 4, R, 0, R) : none;
    const size_t o_fd = in->first_day ? io.add_in(in->first_day, 1, 4, R, 0, R) : none;
    using EO = epi_ejoint_outputs;
    const HostIO::Opt<EO, double> f64[4] = {{&EO::es, ro}, {&EO::truth_term, ro}, {&EO::spread_term, ro}, {&EO::vs, ro}};
    const HostIO::Opt<EO, int32_t> i32[2] = {{&EO::n_members, ro}, {&EO::n_days, ro}};
    size_t o_d[4], o_i[2];
    io.add_opt(*out, f64, o_d, R);
    io.add_opt(*out, i32, o_i, R);
    const size_t o_md = out->member_dist ? io.add_out(out->member_dist, ro, 8, B, 0, B) : none;
    const size_t wsb = ejoint_ws_bytes(d);
    const size_t o_ws = io.reserve(wsb);
    auto enqueue = [&](char *base, hipStream_t st) -> int {
        epi_ejoint_inputs din{};
        din.src = base + o_src; din.population = HostIO::at<const double>(base, o_pop); din.truth = (const double *)(base + o_tr);
        din.truth_series = HostIO::at<const int32_t>(base, o_ts); din.first_day = HostIO::at<const int32_t>(base, o_fd);
        epi_ejoint_outputs dout{};
        HostIO::bind_opt(dout, f64, o_d, base);
        HostIO::bind_opt(dout, i32, o_i, base);
        dout.member_dist = HostIO::at<double>(base, o_md);
        return epi_ejoint_run_device(d, &din, &dout, HostIO::at<char>(base, o_ws), wsb, st, err);
    };
    return run_host(device, io, err, enqueue);
}

// ---- whiteness diagnostics of the innovations of every chain (innov_diag.hpp) ----
// the workspace: the per-block records of the two passes [nb32][B], the lagged products [nb32][H][B] and the per-chain words of
// pass 1; every piece starts at a multiple of 256 bytes
struct IdWs { size_t d8[10], i4[7], c8[2], c4[2], rc, bytes; };
static IdWs id_workspace(const epi_idiag_desc *d)
{
    const size_t B = (size_t)d->B, nb = ((size_t)d->T + kIdBlock - 1) / kIdBlock;
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    IdWs w{};
    size_t o = 0;
    for (size_t &p : w.d8) { p = o; o += up(nb * B * 8); }     // p_sum p_q pre_q r_m2 r_m3 r_m4 r_f r_l r_max r_cs
    for (size_t &p : w.i4) { p = o; o += up(nb * B * 4); }     // p_n p_bad pre_n r_nf r_nl r_maxk r_csk
    for (size_t &p : w.c8) { p = o; o += up(B * 8); }          // c_mean c_q
    for (size_t &p : w.c4) { p = o; o += up(B * 4); }          // c_n c_bad
    w.rc = o; o += up(nb * (size_t)d->n_lags * B * 8);
    w.bytes = o;
    return w;
}

int epi_idiag_validate(const epi_idiag_desc *d, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->B < 1) { set_err(err, "B must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->T < 1) { set_err(err, "T must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->lane_block < 0 || d->lane_block > d->B) { set_err(err, "lane_block must lie in 0 .. B (0 or B: the classic [T][B])"); return EPI_ERR_BAD_ARG; }
    if (d->storage != 0 && d->storage != 1) { set_err(err, "storage must be 0 (double) or 1 (float)"); return EPI_ERR_BAD_ARG; }
    if (d->flip != 0 && d->flip != 1) { set_err(err, "flip must be 0 or 1"); return EPI_ERR_BAD_ARG; }
    if (d->k0 < 0 || d->k1 > d->T || d->k0 > d->k1) { set_err(err, "the window must satisfy 0 <= k0 <= k1 <= T"); return EPI_ERR_BAD_ARG; }
    if (d->n_lags < 0) { set_err(err, "n_lags must be >= 0"); return EPI_ERR_BAD_ARG; }
    if (d->reserved != 0) { set_err(err, "reserved must be 0"); return EPI_ERR_BAD_ARG; }
    if (d->n_lags > kIdMaxLags) { set_err(err, "n_lags is limited to 64 (the rows a block's lags reach ahead are held in LDS)"); return EPI_ERR_UNSUPPORTED; }
    if (d->T >= (1 << 21)) { set_err(err, "T is limited to 2^21 - 1"); return EPI_ERR_UNSUPPORTED; }
    if (((int64_t)d->B + 255) / 256 * 256 * (((int64_t)d->T + kIdBlock - 1) / kIdBlock) >= ((int64_t)1 << 31)) {
        set_err(err, "B * ceil(T / 32) is limited to 2^31 - 1 (one launch covers every block of every chain)");
        return EPI_ERR_UNSUPPORTED;
    }
    return EPI_OK;
}

int epi_idiag_workspace_bytes(const epi_idiag_desc *d, size_t *bytes, char *err)
{
    int rc = epi_idiag_validate(d, err);
    if (rc != EPI_OK) return rc;
    if (!bytes) { set_err(err, "NULL bytes"); return EPI_ERR_BAD_ARG; }
    *bytes = id_workspace(d).bytes;
    return EPI_OK;
}

static int id_check_arrays(const epi_idiag_inputs *in, const epi_idiag_outputs *out, char *err)
{
    if (!in || !out) { set_err(err, "NULL inputs / outputs"); return EPI_ERR_BAD_ARG; }
    if (!in->e) { set_err(err, "NULL e"); return EPI_ERR_BAD_ARG; }
    bool any = out->acf != nullptr;
    for (double *const p : {out->mean, out->var, out->skew, out->kurt, out->jb, out->nis_sum, out->nis_mean, out->lb_q, out->het,
                            out->cusumsq_max, out->max_abs}) any = any || p;
    for (int32_t *const p : {out->n, out->lb_lags, out->het_n1, out->het_n2, out->cusumsq_step, out->max_abs_step, out->status}) any = any || p;
    if (!any) { set_err(err, "no output requested"); return EPI_ERR_BAD_ARG; }
    return EPI_OK;
}

int epi_idiag_run_device(const epi_idiag_desc *d, const epi_idiag_inputs *in, const epi_idiag_outputs *out, void *ws,
                         size_t ws_bytes, void *stream, char *err)
{
    int rc = epi_idiag_validate(d, err);
    if (rc != EPI_OK) return rc;
    if ((rc = id_check_arrays(in, out, err)) != EPI_OK) return rc;
    const IdWs w = id_workspace(d);
    if (!ws || ws_bytes < w.bytes) { set_err(err, "workspace too small (epi_idiag_workspace_bytes)"); return EPI_ERR_WORKSPACE; }
    const hipStream_t st = (hipStream_t)stream;
    hipError_t e;
    char *base = (char *)ws;
    IdArgs a{};
    a.B = d->B; a.T = d->T; a.H = d->n_lags; a.lags = (out->acf || out->lb_q) ? d->n_lags : 0; a.f32 = d->storage; a.flip = d->flip;
    a.k0 = d->k0; a.k1 = d->k1; a.nb32 = (d->T + kIdBlock - 1) / kIdBlock; a.h3 = (int)((2 * (int64_t)(d->k1 - d->k0) + 3) / 6);
    int blk, nblk;
    ll_geometry(d->B, d->lane_block, &blk, &nblk);
    a.bp = (size_t)blk * (size_t)nblk;
    a.e = in->e; a.S = in->S;
    auto D = [&](int k) { return (double *)(base + w.d8[k]); };
    auto I = [&](int k) { return (int32_t *)(base + w.i4[k]); };
    a.p_sum = D(0); a.p_q = D(1); a.pre_q = D(2); a.r_m2 = D(3); a.r_m3 = D(4); a.r_m4 = D(5); a.r_f = D(6); a.r_l = D(7);
    a.r_max = D(8); a.r_cs = D(9);
    a.p_n = I(0); a.p_bad = I(1); a.pre_n = I(2); a.r_nf = I(3); a.r_nl = I(4); a.r_maxk = I(5); a.r_csk = I(6);
    a.c_mean = (double *)(base + w.c8[0]); a.c_q = (double *)(base + w.c8[1]);
    a.c_n = (int32_t *)(base + w.c4[0]); a.c_bad = (int32_t *)(base + w.c4[1]);
    a.r_c = (double *)(base + w.rc);
    a.mean = out->mean; a.var = out->var; a.skew = out->skew; a.kurt = out->kurt; a.jb = out->jb; a.nis_sum = out->nis_sum;
    a.nis_mean = out->nis_mean; a.lb_q = out->lb_q; a.het = out->het; a.cusumsq_max = out->cusumsq_max; a.max_abs = out->max_abs;
    a.n = out->n; a.lb_lags = out->lb_lags; a.het_n1 = out->het_n1; a.het_n2 = out->het_n2; a.cusumsq_step = out->cusumsq_step;
    a.max_abs_step = out->max_abs_step; a.status = out->status; a.acf = out->acf;
    const unsigned t256 = (unsigned)(((int64_t)d->B + 255) / 256), t64 = (unsigned)(((int64_t)d->B + kWave - 1) / kWave);
    hipLaunchKernelGGL(id_blocks1, dim3(t256 * (unsigned)a.nb32), dim3(256), 0, st, a, t256);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "id_blocks1 launch");
    hipLaunchKernelGGL(id_chains1, dim3(t256), dim3(256), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "id_chains1 launch");
    hipLaunchKernelGGL(id_blocks2, dim3(t64 * (unsigned)a.nb32), dim3(kWave), (size_t)(kIdBlock + a.lags) * kWave * sizeof(double), st, a, t64);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "id_blocks2 launch");
    hipLaunchKernelGGL(id_chains2, dim3(t256), dim3(256), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(err, e, "id_chains2 launch");
    return EPI_OK;
}

int epi_idiag_run_host(const epi_idiag_desc *d, const epi_idiag_inputs *in, const epi_idiag_outputs *out, int device, char *err)
{
    int rc = epi_idiag_validate(d, err);
    if (rc != EPI_OK) return rc;
    if ((rc = id_check_arrays(in, out, err)) != EPI_OK) return rc;
    const size_t B = (size_t)d->B, T = (size_t)d->T, none = HostIO::kAbsent;
    int gblk, gnblk;
    ll_geometry(d->B, d->lane_block, &gblk, &gnblk);
    const size_t Bp = (size_t)gnblk * (size_t)gblk;
    static const HostIO::Opt<epi_idiag_outputs, double> f64[] = {
        {&epi_idiag_outputs::mean, 1}, {&epi_idiag_outputs::var, 1}, {&epi_idiag_outputs::skew, 1}, {&epi_idiag_outputs::kurt, 1},
        {&epi_idiag_outputs::jb, 1}, {&epi_idiag_outputs::nis_sum, 1}, {&epi_idiag_outputs::nis_mean, 1}, {&epi_idiag_outputs::lb_q, 1},
        {&epi_idiag_outputs::het, 1}, {&epi_idiag_outputs::cusumsq_max, 1}, {&epi_idiag_outputs::max_abs, 1}};
    static const HostIO::Opt<epi_idiag_outputs, int32_t> i32[] = {
        {&epi_idiag_outputs::n, 1}, {&epi_idiag_outputs::lb_lags, 1}, {&epi_idiag_outputs::het_n1, 1}, {&epi_idiag_outputs::het_n2, 1},
        {&epi_idiag_outputs::cusumsq_step, 1}, {&epi_idiag_outputs::max_abs_step, 1}, {&epi_idiag_outputs::status, 1}};
    HostIO io;
    const size_t o_e = io.add_in(in->e, T, d->storage ? 4 : 8, Bp, 0, Bp);
    const size_t o_S = in->S ? io.add_in(in->S, T, 8, B, 0, B) : none;
    size_t o_d[11], o_i[7];
    io.add_opt(*out, f64, o_d, B);
    io.add_opt(*out, i32, o_i, B);
    const size_t o_acf = (out->acf && d->n_lags > 0) ? io.add_out(out->acf, (size_t)d->n_lags, 8, B, 0, B) : none;
    const size_t wsb = id_workspace(d).bytes;
    const size_t o_ws = io.reserve(wsb);
    const bool only_empty_acf = out->acf && d->n_lags == 0;
    auto enqueue = [&](char *base, hipStream_t st) -> int {
        epi_idiag_inputs din{};
        din.e = base + o_e; din.S = HostIO::at<const double>(base, o_S);
        epi_idiag_outputs dout{};
        HostIO::bind_opt(dout, f64, o_d, base);
        HostIO::bind_opt(dout, i32, o_i, base);
        dout.acf = only_empty_acf ? (double *)(base + o_ws) : HostIO::at<double>(base, o_acf);   // H = 0: nothing is written
        return epi_idiag_run_device(d, &din, &dout, base + o_ws, wsb, st, err);
    };
    return run_host(device, io, err, enqueue);
}

// ---- curve statistics of the ensembles: cdepth_days, cdepth_combine, cdepth_rank, cdepth_envelope, cdepth_fence, cdepth_outliers
// (curve_depth.hpp) ----
// One wavefront per 32-day block unless test_segments asks for fewer, longer segments: the depth pass is compute-bound on the
// sort, so more wavefronts are only more parallelism.
static void cdepth_geometry(const epi_cdepth_desc *d, int *nseg, int *seg_days, int *nblk)
{
    const int W = d->k1 - d->k0, nb = (W + kCdBlock - 1) / kCdBlock;
    long long want = d->test_segments > 0 ? d->test_segments : kCdMaxSeg;
    if (want > nb) want = nb;
    const int per = (int)((nb + want - 1) / want);                    // blocks of a segment
    *nseg = (nb + per - 1) / per;                                     // no empty segment
    *seg_days = per * kCdBlock;
    *nblk = nb;
}

static int cdepth_check_desc(const epi_cdepth_desc *d, char *err)
{
    if (!d) { set_err(err, "NULL descriptor"); return EPI_ERR_BAD_ARG; }
    if (d->abi_version != EPIEKF_ABI_VERSION) { set_err(err, "ABI version mismatch"); return EPI_ERR_BAD_ARG; }
    if (d->T < 1) { set_err(err, "T must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->rows < 1 || d->rows > 4096) { set_err(err, "rows must lie in 1 .. 4096"); return EPI_ERR_BAD_ARG; }
    if (d->R < 1) { set_err(err, "R must be >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->D < 1 || d->D > kCdMaxD) { set_err(err, "D must lie in 1 .. 4096 (a wavefront holds the draws of an item in registers)"); return EPI_ERR_BAD_ARG; }
    if ((int64_t)d->R * d->D > (int64_t)0x7fffffff) { set_err(err, "R * D is limited to 2^31 - 1"); return EPI_ERR_BAD_ARG; }
    if (d->k0 < 0 || d->k1 <= d->k0 || d->k1 > d->T) { set_err(err, "k0, k1 must satisfy 0 <= k0 < k1 <= T"); return EPI_ERR_BAD_ARG; }
    if (d->storage != 0 && d->storage != 1) { set_err(err, "storage must be 0 (double) or 1 (float)"); return EPI_ERR_BAD_ARG; }
    if (d->derive_newcases != 0 && d->derive_newcases != 1) { set_err(err, "derive_newcases must be 0 or 1"); return EPI_ERR_BAD_ARG; }
    if (d->derive_newcases && d->rows < 3) { set_err(err, "derive_newcases needs at least 3 rows"); return EPI_ERR_BAD_ARG; }
    if (d->n_alpha < 0 || d->n_alpha > kCdMaxAlpha) { set_err(err, "n_alpha must lie in 0 .. 8"); return EPI_ERR_BAD_ARG; }
    for (int k = 0; k < d->n_alpha; k++) {
        if (!(d->alpha[k] > 0.0 && d->alpha[k] <= 1.0)) { set_err(err, "every alpha must lie in (0, 1]"); return EPI_ERR_BAD_ARG; }
        if (k > 0 && !(d->alpha[k] > d->alpha[k - 1])) { set_err(err, "alpha must be strictly ascending"); return EPI_ERR_BAD_ARG; }
    }
    if (!(d->fence_factor >= 0.0)) { set_err(err, "fence_factor must be >= 0 (0: no boxplot)"); return EPI_ERR_BAD_ARG; }
    if (d->fence_factor > 0.0 && !(d->fence_frac > 0.0 && d->fence_frac <= 1.0)) { set_err(err, "fence_frac must lie in (0, 1]"); return EPI_ERR_BAD_ARG; }
    const int nb = (d->k1 - d->k0 + kCdBlock - 1) / kCdBlock;
    if (d->test_segments < 0 || d->test_segments > (nb < kCdMaxSeg ? nb : kCdMaxSeg)) {
        set_err(err, "test_segments must lie in 0 .. min(ceil((k1 - k0) / 32), 1024): a segment is whole 32-day blocks");
        return EPI_ERR_BAD_ARG;
    }
    if (d->test_launch_groups < 0) { set_err(err, "test_launch_groups must be >= 0"); return EPI_ERR_BAD_ARG; }
    return EPI_OK;
}

static bool cdepth_wants_fence(const epi_cdepth_outputs *o) { return o->out_days || o->n_outliers || o->whisk_lo || o->whisk_hi; }
static bool cdepth_wants_env(const epi_cdepth_outputs *o) { return o->env_lo || o->env_hi || o->median_curve || cdepth_wants_fence(o); }
static bool cdepth_wants_rank(const epi_cdepth_outputs *o) { return o->depth_rank || o->n_ranked || o->median_path || cdepth_wants_env(o); }

int epi_cdepth_validate(const epi_cdepth_desc *d, const epi_cdepth_inputs *in, const epi_cdepth_outputs *out, char *err)
{
    int rc = cdepth_check_desc(d, err);
    if (rc != EPI_OK) return rc;
    if (!in || !out) { set_err(err, "NULL inputs / outputs"); return EPI_ERR_BAD_ARG; }
    if (!in->src) { set_err(err, "NULL src"); return EPI_ERR_BAD_ARG; }
    if (d->derive_newcases && !in->population) { set_err(err, "NULL population (derive_newcases)"); return EPI_ERR_BAD_ARG; }
    if (d->n_alpha == 0 && (out->env_lo || out->env_hi)) { set_err(err, "env_lo and env_hi need n_alpha >= 1"); return EPI_ERR_BAD_ARG; }
    if (d->fence_factor == 0.0 && cdepth_wants_fence(out)) {
        set_err(err, "out_days, n_outliers, whisk_lo and whisk_hi need fence_factor > 0");
        return EPI_ERR_BAD_ARG;
    }
    if (!(out->depth || out->mhi || out->band_count || out->pair_total || out->n_valid || cdepth_wants_rank(out))) {
        set_err(err, "no output requested");
        return EPI_ERR_BAD_ARG;
    }
    return EPI_OK;
}

// the workspace: doubles depth [M], fence_lo, fence_hi [T][plane]; then 32-bit rec [nblk][4][M], depth_rank, out_days [M], n_ranked,
// median_path [plane]
static size_t cdepth_ws_bytes(const epi_cdepth_desc *d)
{
    int nseg, seg_days, nblk;
    cdepth_geometry(d, &nseg, &seg_days, &nblk);
    const size_t ro = (size_t)(d->rows + d->derive_newcases), M = ro * (size_t)d->R * (size_t)d->D, plane = ro * (size_t)d->R;
    return (M + 2 * (size_t)d->T * plane) * sizeof(double) + ((size_t)nblk * 4 * M + 2 * M + 2 * plane) * sizeof(int32_t);
}

int epi_cdepth_workspace_bytes(const epi_cdepth_desc *d, size_t *bytes, char *err)
{
    int rc = cdepth_check_desc(d, err);
    if (rc != EPI_OK) return rc;
    if (!bytes) { set_err(err, "NULL bytes"); return EPI_ERR_BAD_ARG; }
    *bytes = cdepth_ws_bytes(d);
    return EPI_OK;
}

int epi_cdepth_run_device(const epi_cdepth_desc *d, const epi_cdepth_inputs *in, const epi_cdepth_outputs *out, void *ws,
                          size_t ws_bytes, void *stream, char *err)
{
    int rc = epi_cdepth_validate(d, in, out, err);
    if (rc != EPI_OK) return rc;
    if (!ws || ws_bytes < cdepth_ws_bytes(d)) { set_err(err, "workspace too small (epi_cdepth_workspace_bytes)"); return EPI_ERR_WORKSPACE; }
    CdArgs g{};
    cdepth_geometry(d, &g.nseg, &g.seg_days, &g.nblk);
    g.T = d->T; g.rows = d->rows; g.rows_out = d->rows + d->derive_newcases; g.R = d->R; g.D = d->D; g.derive = d->derive_newcases;
    g.k0 = d->k0; g.k1 = d->k1; g.n_alpha = d->n_alpha; g.fence_factor = d->fence_factor;
    g.src = in->src; g.population = in->population; g.first_day = in->first_day;
    const bool rank = cdepth_wants_rank(out), env = cdepth_wants_env(out), fence = cdepth_wants_fence(out);
    for (int k = 0; k < d->n_alpha; k++) g.frac[k] = d->alpha[k];
    g.nk = d->n_alpha;
    if (fence) g.frac[g.nk++] = d->fence_frac;
    const size_t N = (size_t)d->R * (size_t)d->D, M = (size_t)g.rows_out * N, plane = (size_t)g.rows_out * (size_t)d->R;
    double *wd = (double *)ws;
    g.depth = out->depth ? out->depth : wd;                           // what a later pass reads and the caller did not ask for
    g.fence_lo = wd + M;
    g.fence_hi = g.fence_lo + (size_t)d->T * plane;
    g.rec = (uint32_t *)(g.fence_hi + (size_t)d->T * plane);
    int32_t *wi = (int32_t *)(g.rec + (size_t)g.nblk * 4 * M);
    g.depth_rank = out->depth_rank ? out->depth_rank : wi;
    g.out_days = out->out_days ? out->out_days : wi + M;
    g.n_ranked = out->n_ranked ? out->n_ranked : wi + 2 * M;
    g.median_path = out->median_path ? out->median_path : wi + 2 * M + plane;
    g.mhi = out->mhi; g.band_count = out->band_count; g.pair_total = out->pair_total; g.n_valid = out->n_valid;
    g.n_outliers = out->n_outliers; g.env_lo = out->env_lo; g.env_hi = out->env_hi; g.median_curve = out->median_curve;
    g.whisk_lo = out->whisk_lo; g.whisk_hi = out->whisk_hi;
    const hipStream_t st = (hipStream_t)stream;
    const long long cap = d->test_launch_groups > 0 ? (long long)d->test_launch_groups : kCdLaunchGroups;
    using Kernel = void (*)(const CdArgs);
    hipError_t e = hipSuccess;
    // a grid of `groups` workgroups in x and ny in y, in launches of at most `cap` workgroups
    auto launch = [&](Kernel kern, long long groups, int ny, int wg) {
        const long long per = cap / ny > 0 ? cap / ny : 1;
        for (long long w0 = 0; w0 < groups && e == hipSuccess; w0 = w0 + per) {
            g.group0 = w0;
            const unsigned nb = (unsigned)(groups - w0 < per ? groups - w0 : per);
            hipLaunchKernelGGL(kern, dim3(nb, (unsigned)ny), dim3(wg), 0, st, g);
            e = hipGetLastError();
        }
    };
    // NV: registers per lane of the item, P / 64, P the power of two >= max(D, 64), as epi_ens_run_device's
#define EPI_CD_DAYS(NV) {cdepth_days<0, NV>, cdepth_days<1, NV>}
    static const Kernel days[7][2] = {EPI_CD_DAYS(1), EPI_CD_DAYS(2), EPI_CD_DAYS(4), EPI_CD_DAYS(8), EPI_CD_DAYS(16), EPI_CD_DAYS(32),
                                      EPI_CD_DAYS(64)};
#undef EPI_CD_DAYS
    int nv = 0;
    while ((64 << nv) < d->D) nv++;
    const long long lanes = (long long)((N + kCdLaneWg - 1) / kCdLaneWg);
    launch(days[nv][d->storage], (long long)plane, g.nseg, 64);
    if (e != hipSuccess) return hip_fail(err, e, "cdepth_days launch");
    launch(cdepth_combine, lanes, g.rows_out, kCdLaneWg);
    if (e != hipSuccess) return hip_fail(err, e, "cdepth_combine launch");
    if (!rank) return EPI_OK;
    launch(cdepth_rank, lanes, g.rows_out, kCdLaneWg);
    if (e != hipSuccess) return hip_fail(err, e, "cdepth_rank launch");
    if (!env) return EPI_OK;
    g.mode = 0;
    launch(d->storage ? cdepth_envelope<1> : cdepth_envelope<0>, (long long)d->T * (long long)plane, 1, 64);
    if (e != hipSuccess) return hip_fail(err, e, "cdepth_envelope launch");
    if (!fence) return EPI_OK;
    launch(d->storage ? cdepth_fence<1> : cdepth_fence<0>, lanes, g.rows_out, kCdLaneWg);
    if (e != hipSuccess) return hip_fail(err, e, "cdepth_fence launch");
    if (out->n_outliers) {
        launch(cdepth_outliers, (long long)((plane + kCdLaneWg - 1) / kCdLaneWg), 1, kCdLaneWg);
        if (e != hipSuccess) return hip_fail(err, e, "cdepth_outliers launch");
    }
    if (out->whisk_lo || out->whisk_hi) {
        g.mode = 1;
        launch(d->storage ? cdepth_envelope<1> : cdepth_envelope<0>, (long long)d->T * (long long)plane, 1, 64);
        if (e != hipSuccess) return hip_fail(err, e, "cdepth_envelope (whiskers) launch");
    }
    return EPI_OK;
}

int epi_cdepth_run_host(const epi_cdepth_desc *d, const epi_cdepth_inputs *in, const epi_cdepth_outputs *out, int device, char *err)
{
    int rc = epi_cdepth_validate(d, in, out, err);
    if (rc != EPI_OK) return rc;
    const size_t R = (size_t)d->R, N = R * (size_t)d->D, T = (size_t)d->T, ro = (size_t)(d->rows + d->derive_newcases);
    const size_t na = (size_t)d->n_alpha, none = HostIO::kAbsent;
    HostIO io;
    const size_t o_src = io.add_in(in->src, T * (size_t)d->rows, d->storage ? 4 : 8, N, 0, N);
    const size_t o_pop = d->derive_newcases ? io.add_in(in->population, 1, 8, R, 0, R) : none;
    const size_t o_fd = in->first_day ? io.add_in(in->first_day, 1, 4, R, 0, R) : none;
    using CO = epi_cdepth_outputs;
    const HostIO::Opt<CO, double> f64p[4] = {{&CO::depth, ro}, {&CO::mhi, ro}, {&CO::band_count, ro}, {&CO::pair_total, ro}};
    const HostIO::Opt<CO, int32_t> i32p[3] = {{&CO::n_valid, ro}, {&CO::depth_rank, ro}, {&CO::out_days, ro}};
    const HostIO::Opt<CO, int32_t> i32r[3] = {{&CO::n_ranked, ro}, {&CO::median_path, ro}, {&CO::n_outliers, ro}};
    const HostIO::Opt<CO, double> f64r[5] = {{&CO::env_lo, T * na * ro}, {&CO::env_hi, T * na * ro}, {&CO::median_curve, T * ro},
                                             {&CO::whisk_lo, T * ro}, {&CO::whisk_hi, T * ro}};
    size_t o_dp[4], o_ip[3], o_ir[3], o_dr[5];
    io.add_opt(*out, f64p, o_dp, N);
    io.add_opt(*out, i32p, o_ip, N);
    io.add_opt(*out, i32r, o_ir, R);
    io.add_opt(*out, f64r, o_dr, R);
    const size_t wsb = cdepth_ws_bytes(d);
    const size_t o_ws = io.reserve(wsb);
    auto enqueue = [&](char *base, hipStream_t st) -> int {
        epi_cdepth_inputs din{};
        din.src = base + o_src; din.population = HostIO::at<const double>(base, o_pop); din.first_day = HostIO::at<const int32_t>(base, o_fd);
        epi_cdepth_outputs dout{};
        HostIO::bind_opt(dout, f64p, o_dp, base);
        HostIO::bind_opt(dout, i32p, o_ip, base);
        HostIO::bind_opt(dout, i32r, o_ir, base);
        HostIO::bind_opt(dout, f64r, o_dr, base);
        return epi_cdepth_run_device(d, &din, &dout, HostIO::at<char>(base, o_ws), wsb, st, err);
    };
    return run_host(device, io, err, enqueue);
}

}  // extern "C"

// plan_query.cpp -- which kernel instances ONE call of epi_ekf_run_device / epi_sweep_run_device launches, by name, and every
// instance ANY call can launch.  Plain C++17, no HIP: it includes csrc/launch_plan.hpp, asks plan_launch the question
// run_device_impl asks (through the same plan_call_input) and maps the plan's picks to the names of the kernels -- the ladders of
// enqueue_fwd, enqueue_bwd, launch_monitor and enqueue_pinv in csrc/epiekf.hip restated.  tests/plan_probe.py builds it as a
// shared object (g++, no sanitizer) and loads it with ctypes; tests/test_kernel_ledger.py holds the names against the kernels a
// host-only compile of epiekf.hip lists, so a ladder that changes without this file fails there.
//
// A name is what `nm -C` prints for the kernel's host stub, without "epi::" and the argument list: "ekf_fwd_sym<6, 0, 1, 0, 0, 0>".
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <set>
#include <string>
#include <vector>
#include "launch_plan.hpp"

using namespace epi;

namespace {

std::string fmt(const char *f, ...)
{
    char b[96];
    va_list ap;
    va_start(ap, f);
    vsnprintf(b, sizeof b, f, ap);
    va_end(ap);
    return b;
}

// enqueue_fwd<M, FLIP, GENERIC>: "" where the ladder launches nothing for this pick
std::string fwd_name(int M, int F, int G, const KernelPick &k)
{
    const unsigned v = k.bits;
    if (M == 6 && !G && k.kernel == FWD_WAVE_NC) return (v & V_L21) ? "ekf_fwd_wave<0, 1, 21, 0>" : "ekf_fwd_wave<0, 1, 0, 0>";
    if (M == 6 && G) {
        if (k.kernel == FWD_WAVE)
            return !(v & V_INLINE) ? fmt("ekf_fwd_wave<%d, 0, 0, 1>", F) : (v & V_L21) ? fmt("ekf_fwd_wave<%d, 1, 21, 1>", F) : fmt("ekf_fwd_wave<%d, 1, 0, 1>", F);
        if (k.kernel == FWD_HEX) return fmt("ekf_fwd_hex<%d, %d, %d>", F, (v & V_BLK) ? kHG : 0, (v & V_SOLO) ? 1 : 0);
        if (k.kernel == FWD_QUAD) {
            const char *blk = (v & V_BLK) ? "16, 21" : "0, 0";
            if (v & V_INLINE) return fmt("ekf_fwd_quad<%d, %s, 1, 0>", F, blk);
            return fmt("ekf_fwd_quad<%d, %s, 0, %d>", F, blk, (v & V_SOLO) ? 1 : 0);
        }
    }
    if (M == 3 && G && k.kernel == FWD_WAVE3) return fmt("ekf_fwd_wave3<%d>", F);
    if (G && k.kernel == FWD_SYM) {
        // ekf_fwd_sym<M, FLIP, LP, STOR = 0, MON = 1, USD = 0>
        if (v & V_INLINE) return (v & V_STOR) ? fmt("ekf_fwd_sym<%d, %d, 0, 1, 1, 0>", M, F) : fmt("ekf_fwd_sym<%d, %d, %d, 0, 1, 0>", M, F, (v & V_LP) ? 1 : 0);
        if (v & V_STOR) return fmt("ekf_fwd_sym<%d, %d, 0, 1, 0, 0>", M, F);
        if (v & V_USD) return fmt("ekf_fwd_sym<%d, %d, 1, 0, 0, 1>", M, F);
        return fmt("ekf_fwd_sym<%d, %d, %d, 0, 0, 0>", M, F, (v & V_LP) ? 1 : 0);
    }
    return "";
}

// enqueue_bwd<M, FLIP, GENERIC>
std::string bwd_name(int M, int F, int G, const KernelPick &k, int xd)
{
    const unsigned v = k.bits;
    if (M == 6 && !G && k.kernel == BWD_WAVE_NC) return "eks_bwd_wave_nc";
    if (M == 6 && G) {
        if (k.kernel == BWD_WAVE) return fmt("eks_bwd_wave<%d>", F);
        // eks_bwd_hex<FLIP, BLK, PF>: the prefetch sets of the one-wave-per-SIMD variants are 2 (10-chain blocks) and 1 (classic)
        if (k.kernel == BWD_HEX) return (v & V_BLK) ? fmt("eks_bwd_hex<%d, %d, %d>", F, kHG, (v & V_SOLO) ? 2 : 0) : fmt("eks_bwd_hex<%d, 0, %d>", F, (v & V_SOLO) ? 1 : 0);
        if (k.kernel == BWD_QUAD) return fmt("eks_bwd_quad<%d, %d>", F, (v & V_BLK) ? kQC : 0);
        if (k.kernel == BWD_LANE6)
            return k.wg_chains == 40 ? fmt("eks_bwd_lane6<%d, 40, %d>", F, xd ? 1 : 0) : fmt("eks_bwd_lane6<%d, %d, 0>", F, k.wg_chains == 48 ? 48 : 56);
    }
    if (M == 3 && G && k.kernel == BWD_WAVE3) return fmt("eks_bwd_wave3<%d>", F);
    if (G && k.kernel == BWD_SYM) return fmt("eks_bwd_sym<%d, %d, %d>", M, F, (v & V_STOR) ? 1 : 0);
    return "";
}

// launch_monitor<FLIP>
std::string mon_name(int F, const KernelPick &k)
{
    if (k.kernel == MON_PAR) return fmt("ekf_monitor_par<%d, 21, %d>", F, kMonitorParDays);
    return fmt("ekf_monitor<%d, %d>", F, (k.bits & V_L21) ? 21 : 0);
}

struct Launch { std::string role, name; };

// run_plan<M, FLIP, GENERIC> over the plan's list: (role, name) in launch order
void walk(const LaunchPlan &p, int M, int F, int G, bool only, const char *prefix, std::vector<Launch> &out)
{
    auto add = [&](const char *role, const std::string &n) { if (!n.empty()) out.push_back({std::string(prefix) + role, n}); };
    for (int i = 0; i < p.n_ops; i++) {
        const PlanOp &o = p.ops[i];
        if (o.kind == OP_FWD) {
            add("fwd", fwd_name(M, F, G, p.fwd));
            if (p.dense) add("dense_fwd", fmt("ekf_fwd<%d, %d, %d>", M, F, G));
        } else if (o.kind == OP_BWD) {
            add("bwd", bwd_name(M, F, G, p.bwd, o.xd));
            if (p.dense) add("dense_bwd", fmt("eks_bwd<%d, %d, %d>", M, F, G));
        } else if (o.kind == OP_PINV) add("pinv", fmt("eks_pinv<%d, %d>", M, only ? 1 : 0));
        else if (o.kind == OP_MONITOR) add("mon", mon_name(F, p.mon));
    }
}

// what walk() reads of a plan, packed: two plans of a model with the same word launch the same names
uint64_t name_key(const LaunchPlan &p)
{
    uint64_t k = (uint64_t)p.fwd.kernel | (uint64_t)p.fwd.bits << 3 | (uint64_t)p.bwd.kernel << 10 | (uint64_t)p.bwd.bits << 13 |
                 (uint64_t)p.bwd.wg_chains << 20 | (uint64_t)p.mon.kernel << 27 | (uint64_t)p.mon.bits << 29 | (uint64_t)p.dense << 36;
    for (int i = 0; i < p.n_ops; i++) k |= (uint64_t)1 << (37 + p.ops[i].kind) | (p.ops[i].kind == OP_BWD ? (uint64_t)1 << (44 + p.ops[i].xd) : 0);
    return k;
}

// launch_chain: the plan's list, then the dense second pass of exact_nonfinite (rerun_nonfinite_dense) where the plan asks for it.
// seen: the names of a (model, plan word, second plan word) already taken are not spelled out again (the enumeration).
LaunchPlan launches(const PlanIn &in, std::vector<Launch> &out, std::set<std::vector<uint64_t>> *seen = nullptr)
{
    const ModelInfo &mi = MODEL_TABLE[in.d->model];
    const int M = mi.m, G = mi.generic, F = G ? mi.flipped : 0;       // (the NewCase models run launch_chain<6, 0, 0>)
    const LaunchPlan p = plan_launch(in);
    const bool second = G && p.rerun_after;
    LaunchPlan p2{};
    if (second) {
        PlanIn ind = in;
        ind.hint = 2; ind.only = true; ind.smooth = true; ind.rerun = false; ind.has_tail = false;
        p2 = plan_launch(ind);
    }
    if (seen && !seen->insert({(uint64_t)in.d->model, name_key(p), second ? name_key(p2) : ~(uint64_t)0}).second) return p;
    walk(p, M, F, G, false, "", out);
    if (second) walk(p2, M, F, 1, true, "second_", out);
    return p;
}

// epi_ekf_validate + run_device_impl's checks, as far as the grid below can miss them
bool valid(const epi_batch_desc &d)
{
    const ModelInfo &mi = MODEL_TABLE[d.model];
    if (!mi.generic && (d.r_mode != 0 || d.q_mode != 0)) return false;
    if (d.storage == 1 && (!mi.generic || d.q_mode != 0 || d.path_hint != 1)) return false;
    if ((size_t)3 * d.L * kWave * sizeof(double) > 160u * 1024u) return false;
    return d.B >= 1 && d.T >= 1 && d.B <= (1 << 23);
}

}  // namespace

extern "C" {

// The launches of one call.  facts[0..5] = shape, lw, schedule bits, the forward kernel's dynamic LDS bytes, operations in the
// plan, overflow.  buf receives "role name\n" per launch in launch order (roles: fwd, bwd, mon, pinv, dense_fwd, dense_bwd; the
// second pass of exact_nonfinite with "second_" in front).  Returns the bytes written, -1 if buf is too small.
int epi_plan_query(const epi_batch_desc *d, int has_pinv_rank, int has_status, int n_simds, int has_tail, int t_hist, int32_t *facts,
                   char *buf, size_t cap)
{
    std::vector<Launch> l;
    const LaunchPlan p = launches(plan_call_input(d, n_simds, has_pinv_rank != 0, has_status != 0, has_tail != 0, t_hist), l);
    facts[0] = p.shape; facts[1] = p.lw; facts[2] = (int32_t)p.schedule; facts[3] = (int32_t)p.fwd.lds; facts[4] = p.n_ops; facts[5] = p.overflow;
    std::string s;
    for (const Launch &x : l) s += x.role + " " + x.name + "\n";
    if (s.size() + 1 > cap) return -1;
    memcpy(buf, s.c_str(), s.size() + 1);
    return (int)s.size();
}

// Every instance name a plan can produce on n_simds SIMDs, one per line, sorted: all six models; B at both sides of every
// threshold of the plan up to 2 * 64 * S + 1; T 6 / 40 / 130; L 21 / 5 / 50 (50: the monitor no longer hoisted); both r_mode; all
// shapes; blocks 0 / 8 / 10 / 16 / 40 / 48 / 56; both storages; P_MINUS and P_PLUS selected or not (ws_upper 0 / 3); hint 1 / 2; rho
// selected or not; test_flags 0..7; time_pipe -1 / 0 / 1; the sweep's tail (6-state forward model).  plans: how many were made.
int epi_plan_enumerate(int n_simds, int64_t *plans, char *buf, size_t cap)
{
    const long S = n_simds;
    const long Bs[] = {1, 7, 64, 80, 130, S * 5 / 8 + 1, S + 1, 2049, kHG * S, kHG * S + 1, kQC * S + 1, 2 * kHG * S + 1, 64 * S, 64 * S + 1, 2 * 64 * S + 1};
    const int Ts[] = {6, 40, 130}, Ls[] = {21, 5, 50}, blks[] = {0, 8, 10, 16, 40, 48, 56};
    std::set<std::string> names;
    std::set<std::vector<uint64_t>> seen;
    std::vector<Launch> l;
    int64_t n = 0;
    epi_batch_desc d{};
    d.abi_version = EPIEKF_ABI_VERSION; d.n_npi = EPI_MAX_NPI; d.order = 1;
    for (d.model = 0; d.model < 6; d.model++)
    for (long B : Bs) for (int T : Ts) for (int L : Ls)
    for (d.r_mode = 0; d.r_mode < 2; d.r_mode++)
    for (d.shape = 0; d.shape <= 4; d.shape++)
    for (int blk : blks)
    for (d.storage = 0; d.storage < 2; d.storage++)
    for (int upper = 0; upper < 2; upper++)
    for (d.path_hint = 1; d.path_hint <= 2; d.path_hint++)
    for (int rho = 0; rho < 2; rho++)
    for (d.test_flags = 0; d.test_flags < 8; d.test_flags++)
    for (d.time_pipe = -1; d.time_pipe <= 1; d.time_pipe++) {
        d.B = d.Sx = d.Su = (int)B; d.T = T; d.L = L; d.lane_block = blk;
        d.out_mask = (EPI_OUT_ALL & ~(uint32_t)(EPI_OUT_P_MINUS | EPI_OUT_P_PLUS | EPI_OUT_RHO)) | (upper ? 0u : (uint32_t)(EPI_OUT_P_MINUS | EPI_OUT_P_PLUS)) |
                     (rho ? (uint32_t)EPI_OUT_RHO : 0u);
        if (!valid(d)) continue;
        const int tails = (d.model == EPI_MODEL_SIA6 && d.storage == 0) ? 2 : 1;
        for (int tail = 0; tail < tails; tail++) {
            l.clear();
            if (launches(plan_call_input(&d, n_simds, true, true, tail != 0, T / 2), l, &seen).overflow) return -2;
            for (const Launch &x : l) names.insert(x.name);
            n++;
        }
    }
    *plans = n;
    std::string s;
    for (const std::string &x : names) s += x + "\n";
    if (s.size() + 1 > cap) return -1;
    memcpy(buf, s.c_str(), s.size() + 1);
    return (int)names.size();
}

}  // extern "C"

// The direct optimal-NPI planner: for every (region, cost weight) chain the Pontryagin problem of the prescription path solved
// in its stable direction -- states forward, adjoint backward from zero -- by Frank-Wolfe steps with backtracking; included by
// epiekf.hip (entry point epi_plan_run_device, include/epiekf.h).  DESIGN.md §4.15 pins the arithmetic; tests/npi_plan_ref.c
// restates it and the GPU suite holds the two to the same bits.
//
//   plan_solve   one lane per chain c = region * P + l (cost weight fastest); the whole iteration loop of a chain runs in this
//                one launch.  A lane leaves the loop when its chain stops; a wavefront lives as long as its slowest lane.
//
// Per chain and day the lane keeps in HBM, chain-minor so that a wavefront's day is one contiguous run per row:
//   ub[2]  [H][n][B]  the current plan and the trial plan; which of the two is current flips with every accepted step
//   xb[2]  [H][3][B]  the post-update states (s, i, alpha) of the current and of the trial plan
//   mask   [H][B]     bits 0..11: the vertex u* of the last adjoint pass (set: u_max, clear: u_min); bits 16..27: entry is held
// ub[0] is the caller's `plan`, xb[0] the caller's `states` where wanted: a chain that stops on side 1 copies its columns over.
// Whether a clamp was inactive on a day is a pure function of the stored post-update state (strictly inside its bounds), so the
// adjoint pass recomputes the three flags from xb instead of reading a fourth row.
//
// The forward pass is sialpha_step with zero noise followed by npicost_accumulate, the two functions of the scoring tail.
// Addressing is plain 64-bit element offsets, so no array size limits it and the same source compiles for the host.
//
// Host-compilation contract: the kernel's body is the EPI_DEV function plan_lane of its chain index; tests/npi_plan_emu.cpp
// compiles it with the host compiler and calls it one lane at a time.
#pragma once

constexpr int kPlanMaxIter = 255, kPlanMaxHalvings = 30;
constexpr int kPlanStopCap = 1, kPlanStopSearch = 2, kPlanStopNonfinite = 4;   // bits of status

struct PlanArgs {
    int R, P, H, n, max_iter, max_halvings, prefix_days;
    double tol;
    const double *sp, *u_min, *eps, *u_fixed, *u_init, *J0_prefix, *J1_prefix;
    double *ub[2], *xb[2];
    uint32_t *mask;
    double *J0, *J1, *F, *gap;
    int32_t *iters, *halvings, *status;
    double *mu, *F_trace;                                  // [H][3][B], [max_iter][B] or NULL
    int want_states;                                       // xb[0] is the caller's
};

struct PlanSums { double F, j0, j1; };

// One forward pass over the horizon from the end-of-history state.  TRIAL 0: the starting plan (held entries from u_fixed, free
// ones from u_init or u_min) is formed, written to side 0 and the held bits to mask.  TRIAL 1: the trial plan u + theta (u* - u)
// of side `src` is formed, written to the other side.  Either way the day's states go to the written side.
template <int TRIAL>
EPI_DEV PlanSums plan_forward(const PlanArgs &a, const SimPrm &p, const double (&umin)[kNpi], size_t c, size_t r, int src, double theta,
                              double eps, double ome, double s, double i, double al, bool pre)
{
    const size_t B = (size_t)a.R * (size_t)a.P, R = (size_t)a.R, n = (size_t)a.n;
    const int dst = TRIAL ? 1 - src : 0;
    const double *us = a.ub[src];
    double *ud = a.ub[dst], *xd = a.xb[dst];
    double acc0 = 0.0, acc1 = 0.0;
    double j0 = pre ? a.J0_prefix[r] : 0.0, j1 = pre ? a.J1_prefix[r] : 0.0;
    // the trial pass loads day t + 1 (plan and mask word of the side it reads) before it computes and stores day t: the two
    // sides are different buffers, and a lane's day otherwise waits a full memory round trip for every load it starts
    double un[kNpi];
    uint32_t mn = 0;
    auto load_day = [&](int t) {
        mn = a.mask[(size_t)t * B + c];
#pragma unroll
        for (int k = 0; k < kNpi; k++) un[k] = (k < a.n) ? us[((size_t)t * n + k) * B + c] : 0.0;
    };
    if (TRIAL) load_day(0);
    for (int t = 0; t < a.H; t++) {
        double uk[kNpi];
        if (TRIAL) {
            const uint32_t m = mn;
            double u[kNpi];
#pragma unroll
            for (int k = 0; k < kNpi; k++) u[k] = un[k];
            if (t + 1 < a.H) load_day(t + 1);
#pragma unroll
            for (int k = 0; k < kNpi; k++) {
                uk[k] = 0.0;
                if (k < a.n) {
                    const double ustar = ((m >> k) & 1u) ? p.um[k] : umin[k];
                    uk[k] = ((m >> (16 + k)) & 1u) ? u[k] : u[k] + theta * (ustar - u[k]);
                }
            }
        } else {
            uint32_t held = 0;
#pragma unroll
            for (int k = 0; k < kNpi; k++) {
                uk[k] = 0.0;
                if (k < a.n) {
                    const double uf = a.u_fixed ? a.u_fixed[((size_t)t * n + k) * R + r] : __builtin_nan("");
                    if (!is_nan(uf)) { uk[k] = uf; held |= 1u << (16 + k); }
                    else uk[k] = a.u_init ? a.u_init[((size_t)t * n + k) * B + c] : umin[k];
                }
            }
            a.mask[(size_t)t * B + c] = held;
        }
#pragma unroll
        for (int k = 0; k < kNpi; k++)
            if (k < a.n) ud[((size_t)t * n + k) * B + c] = uk[k];
        sialpha_step(p, uk, 0.0, 0.0, 0.0, s, i, al);
        xd[((size_t)t * 3 + 0) * B + c] = s;
        xd[((size_t)t * 3 + 1) * B + c] = i;
        xd[((size_t)t * 3 + 2) * B + c] = al;
        npicost_accumulate(p, uk, a.n, t == 0, s, i, al, acc0, acc1);
        if (pre) npicost_accumulate(p, uk, a.n, false, s, i, al, j0, j1);
    }
    PlanSums o;
    o.F = ome * acc0 + eps * acc1;
    o.j0 = pre ? j0 : acc0;
    o.j1 = pre ? j1 : acc1;
    return o;
}

// One adjoint pass over side `cur`, days descending: mu, the gradient, the vertex bits and the gap.
EPI_DEV double plan_adjoint(const PlanArgs &a, const SimPrm &p, const double (&umin)[kNpi], size_t c, int cur, double eps, double ome)
{
    const size_t B = (size_t)a.R * (size_t)a.P, n = (size_t)a.n;
    const double *x = a.xb[cur], *u = a.ub[cur];
    const double dt = p.dt;
    double gap = 0.0;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0;                   // D(t+1) mu(t+1)
    // day t - 1 (states, plan, mask word) is loaded before day t is computed and its mask word stored: other addresses
    double xn[3], un[kNpi];
    uint32_t mn = 0;
    auto load_day = [&](int t) {
        mn = a.mask[(size_t)t * B + c];
#pragma unroll
        for (int j = 0; j < 3; j++) xn[j] = x[((size_t)t * 3 + j) * B + c];
#pragma unroll
        for (int k = 0; k < kNpi; k++) un[k] = (k < a.n) ? u[((size_t)t * n + k) * B + c] : 0.0;
    };
    load_day(a.H - 1);
    for (int t = a.H - 1; t >= 0; t--) {
        const double s = xn[0], i = xn[1], al = xn[2];
        const uint32_t held = mn >> 16;
        double ut[kNpi];
#pragma unroll
        for (int k = 0; k < kNpi; k++) ut[k] = un[k];
        if (t > 0) load_day(t - 1);
        double mu0 = ome * (i * al), mu1 = ome * (s * al), mu2 = ome * (s * i);
        if (t < a.H - 1) {
            // the state block of state_jacobians at x(t), its structural zeros skipped; A' v, row index ascending
            const double A00 = 1.0 - dt * al * i, A01 = -dt * al * s, A02 = -dt * s * i;
            const double A10 = dt * i * al, A11 = 1.0 + dt * (s * al - p.beta), A12 = dt * s * i;
            const double A22 = 1.0 - dt * p.gamma;
            const double m0 = fma(A10, v1, A00 * v0);
            const double m1 = fma(A11, v1, A01 * v0);
            const double m2 = fma(A22, v2, fma(A12, v1, A02 * v0));
            mu0 = mu0 + m0; mu1 = mu1 + m1; mu2 = mu2 + m2;
        }
        const bool d0 = 0.0 < s && s < 1.0, d1 = 0.0 < i && i < 1.0, d2 = p.alpha_min < al && al < p.alpha_max;
        if (a.mu) {
            a.mu[((size_t)t * 3 + 0) * B + c] = mu0;
            a.mu[((size_t)t * 3 + 1) * B + c] = mu1;
            a.mu[((size_t)t * 3 + 2) * B + c] = mu2;
        }
        uint32_t bits = 0;
#pragma unroll
        for (int k = 0; k < kNpi; k++)
            if (k < a.n) {
                const double ew = eps * p.w[k];
                const double g = d2 ? ew - dt * p.ga[k] * mu2 : ew;
                const bool up = !(g > 0.0);
                if (up) bits |= 1u << k;
                if (!((held >> k) & 1u)) {
                    const double ustar = up ? p.um[k] : umin[k];
                    gap = gap + g * (ut[k] - ustar);
                }
            }
        a.mask[(size_t)t * B + c] = (held << 16) | bits;
        v0 = d0 ? mu0 : 0.0; v1 = d1 ? mu1 : 0.0; v2 = d2 ? mu2 : 0.0;
    }
    return gap;
}

EPI_DEV void plan_lane(const PlanArgs &a, int ci)
{
    const size_t c = (size_t)ci, B = (size_t)a.R * (size_t)a.P, r = c / (size_t)a.P, l = c - r * (size_t)a.P, n = (size_t)a.n;
    SimPrm p;
    double s0, i0, al0;
    load_sim_prm(p, a.sp, a.R, (int)r, s0, i0, al0);
    double umin[kNpi];
#pragma unroll
    for (int k = 0; k < kNpi; k++) umin[k] = (k < a.n) ? a.u_min[(size_t)k * (size_t)a.R + r] : 0.0;
    const double eps = a.eps[l], ome = 1.0 - eps;
    const bool pre = a.prefix_days > 0;
    const double qnan = __builtin_nan("");

    int cur = 0, iters = 0, halv = 0, st = 0;
    PlanSums f = plan_forward<0>(a, p, umin, c, r, 0, 0.0, eps, ome, s0, i0, al0, pre);
    double gap = qnan;
    for (;;) {
        if (is_nonfinite(f.F)) { st |= kPlanStopNonfinite; break; }
        if (a.F_trace) a.F_trace[(size_t)iters * B + c] = f.F;
        iters++;
        gap = plan_adjoint(a, p, umin, c, cur, eps, ome);
        if (gap <= a.tol * fabs(f.F)) break;
        if (iters == a.max_iter) { st |= kPlanStopCap; break; }
        bool accepted = false;
        double theta = 1.0;
        for (int j = 0; j <= a.max_halvings; j++) {
            const PlanSums ft = plan_forward<1>(a, p, umin, c, r, cur, theta, eps, ome, s0, i0, al0, pre);
            if (ft.F < f.F) { f = ft; cur = 1 - cur; accepted = true; break; }
            halv++;
            theta = theta * 0.5;
        }
        if (!accepted) { st |= kPlanStopSearch; break; }
    }
    if (st & kPlanStopNonfinite) {                         // no adjoint belongs to this plan
        gap = qnan;
        if (a.mu)
            for (size_t e = 0; e < (size_t)a.H * 3; e++) a.mu[e * B + c] = qnan;
    }
    if (a.F_trace)
        for (int q = iters; q < a.max_iter; q++) a.F_trace[(size_t)q * B + c] = qnan;
    if (cur == 1) {
        for (size_t e = 0; e < (size_t)a.H * n; e++) a.ub[0][e * B + c] = a.ub[1][e * B + c];
        if (a.want_states)
            for (size_t e = 0; e < (size_t)a.H * 3; e++) a.xb[0][e * B + c] = a.xb[1][e * B + c];
    }
    const size_t days = (size_t)a.H + (size_t)(pre ? a.prefix_days : 0);
    a.J0[c] = f.j0 / (double)days;
    a.J1[c] = f.j1 / (double)(n * days);
    a.F[c] = f.F;
    a.gap[c] = gap;
    a.iters[c] = iters;
    a.halvings[c] = halv;
    a.status[c] = st;
}

#ifndef EPI_PLAN_HOST
__global__ __launch_bounds__(kWave) void plan_solve(const PlanArgs a)
{
    const long long c = (long long)blockIdx.x * kWave + threadIdx.x;
    if (c >= (long long)a.R * a.P) return;
    plan_lane(a, (int)c);
}
#endif

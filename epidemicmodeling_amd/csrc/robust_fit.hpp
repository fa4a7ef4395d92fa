// REGRESSION_TYPE = 'NONNEGATIVELS-ELEMENT-WISE' (TrainPredictPrescribeNPI.m:279-292, :340-353): for every NPI k and region r
// on its own a robust affine fit y ~ a x + b of alpha against that NPI, the slope bounded; the region's intercept is
// mean(y - X a).  Included by epiekf.hip (entry point epi_robfit_run_device, include/epiekf.h).  DESIGN.md §4.10 pins the
// arithmetic (bisquare iteratively reweighted least squares, residuals adjusted by leverage, scale from the median absolute
// deviation); tests/robust_fit_ref.c and tests/robust_fit_ref.py restate it and the suites hold all three to the same bits.
//
// robfit_items: one wavefront per item (k, r).  Day d lives in register d / 64 of lane d % 64, a lane holds NV = P / 64 days,
// P the power of two >= max(D, 64) (NV = 1 .. 16).  x, y, the leverage factor and the weights stay in registers for the whole
// iteration; every sum over days is the pairwise tree of ens_summary.hpp with +0.0 in the places D .. P-1, the median comes
// from its register bitonic sort (+Inf in those places).  Every quantity that steers the loop (a, b, the scale, the stop test)
// is the result of a tree or of a pick and therefore the same in all 64 lanes: the loop condition is wave-uniform.  No LDS, no
// barrier, no atomics, no host synchronisation.
// robfit_intercept: one wavefront per region, launched behind robfit_items on the same stream.  It reads the slopes that
// launch wrote; when the caller asked for no slope array it fits the region's n items itself, one after the other.
#pragma once
#include "ens_summary.hpp"             // ens_tree, ens_sort, ens_pick

constexpr int kRfMaxD = 1024, kRfMaxN = 12;
constexpr int kRfNonfinite = 1, kRfConst = 2, kRfSlopeLost = 4, kRfMaxiter = 8, kRfBound = 16;   // epi_robfit_status_bits
// items per launch: a launch's thread count (workgroups x 64 lanes) is a 32-bit number in the HIP runtime (lasso.hpp)
constexpr int64_t kRfLaunchItems = (int64_t)1 << 25;

struct RfArgs {
    int R, D, n, robust, max_iter;
    long long item0;                       // first item (robfit_items) or region (robfit_intercept) of this launch
    double lower, upper;
    const double *X, *y;                   // [D][n][R], [D][R]
    double *a, *b_item, *sigma;            // [n][R]
    int32_t *iters, *status;               // [n][R]
    double *weights;                       // [D][n][R]
    double *b;                             // [R]
};

struct RfFit { double a, b, sigma; int iters, status; };

// the weighted bounded solve of §4.10 over the item's days; the padding places hold +0.0 in every sum
template <int NV>
EPI_DEV void rf_wls(const double (&x)[NV], const double (&y)[NV], const double (&w)[NV], int lane, int D, bool cst, double lower,
                    double upper, double &a, double &b, int &flags)
{
    double s[NV];
#pragma unroll
    for (int j = 0; j < NV; j++) s[j] = j * 64 + lane < D ? w[j] : 0.0;
    const double sw = ens_tree<NV>(s);
#pragma unroll
    for (int j = 0; j < NV; j++) s[j] = j * 64 + lane < D ? w[j] * x[j] : 0.0;
    const double mx = ens_tree<NV>(s) / sw;
#pragma unroll
    for (int j = 0; j < NV; j++) s[j] = j * 64 + lane < D ? w[j] * y[j] : 0.0;
    const double my = ens_tree<NV>(s) / sw;
#pragma unroll
    for (int j = 0; j < NV; j++) s[j] = j * 64 + lane < D ? (w[j] * (x[j] - mx)) * (x[j] - mx) : 0.0;
    const double sxx = ens_tree<NV>(s);
#pragma unroll
    for (int j = 0; j < NV; j++) s[j] = j * 64 + lane < D ? (w[j] * (x[j] - mx)) * (y[j] - my) : 0.0;
    const double sxy = ens_tree<NV>(s);
#pragma unroll
    for (int j = 0; j < NV; j++) s[j] = j * 64 + lane < D ? (w[j] * x[j]) * x[j] : 0.0;
    const double swxx = ens_tree<NV>(s);
    flags = 0;
    a = 0.0;
    if (!cst && sxx > 2.220446049250313e-16 * swxx) {          // the slope is identified
        const double raw = sxy / sxx;
        a = raw;
        if (a < lower) a = lower;
        if (a > upper) a = upper;
        if (a != raw) flags = kRfBound;
    } else if (!cst) {
        flags = kRfSlopeLost;
    }
    b = my - a * mx;
}

// the fit of item (k, r); every member of the result is the same in all lanes.  store: write the item's outputs
template <int NV>
EPI_DEV RfFit rf_item(const RfArgs &g, int k, size_t r, int lane, bool store)
{
    const int D = g.D;
    const size_t R = (size_t)g.R, n = (size_t)g.n, oi = (size_t)k * R + r;
    const double qnan = __builtin_nan("");
    double x[NV], y[NV], adj[NV], w[NV], s[NV];
    bool finite = true;
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const int d = j * 64 + lane;
        x[j] = d < D ? g.X[((size_t)d * n + (size_t)k) * R + r] : 0.0;
        y[j] = d < D ? g.y[(size_t)d * R + r] : 0.0;
        finite = finite && fabs(x[j]) < (double)INFINITY && fabs(y[j]) < (double)INFINITY;
    }
    RfFit f;
    if (__ballot(!finite) != 0) {
        f.a = f.b = f.sigma = qnan; f.iters = 0; f.status = kRfNonfinite;
        if (store) {
            if (lane == 0) {
                if (g.a) g.a[oi] = qnan;
                if (g.b_item) g.b_item[oi] = qnan;
                if (g.sigma) g.sigma[oi] = qnan;
                if (g.iters) g.iters[oi] = 0;
                if (g.status) g.status[oi] = kRfNonfinite;
            }
            if (g.weights) {
#pragma unroll
                for (int j = 0; j < NV; j++) {
                    const int d = j * 64 + lane;
                    if (d < D) g.weights[((size_t)d * n + (size_t)k) * R + r] = qnan;
                }
            }
        }
        return f;
    }
    // ---- constant column: max == min, exact ----
    double lo = (double)INFINITY, hi = -(double)INFINITY;
#pragma unroll
    for (int j = 0; j < NV; j++) {
        if (j * 64 + lane < D) { lo = fmin(lo, x[j]); hi = fmax(hi, x[j]); }
    }
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) { lo = fmin(lo, __shfl_xor(lo, h)); hi = fmax(hi, __shfl_xor(hi, h)); }
    const bool cst = lo == hi;
    const double Dd = (double)D;
    // ---- leverage of the unweighted design [x 1], once ----
#pragma unroll
    for (int j = 0; j < NV; j++) s[j] = x[j];
    const double xbar = ens_tree<NV>(s) / Dd;
#pragma unroll
    for (int j = 0; j < NV; j++) s[j] = j * 64 + lane < D ? (x[j] - xbar) * (x[j] - xbar) : 0.0;
    const double sxx0 = ens_tree<NV>(s);
#pragma unroll
    for (int j = 0; j < NV; j++) {
        double h = 1.0 / Dd;
        if (!cst) {
            h = 1.0 / Dd + ((x[j] - xbar) * (x[j] - xbar)) / sxx0;
            if (!(h < 0.9999)) h = 0.9999;
        }
        adj[j] = 1.0 / sqrt(1.0 - h);
    }
    // ---- tiny = 1e-6 std(y), D - 1 normalisation ----
#pragma unroll
    for (int j = 0; j < NV; j++) s[j] = y[j];
    const double ybar = ens_tree<NV>(s) / Dd;
#pragma unroll
    for (int j = 0; j < NV; j++) s[j] = j * 64 + lane < D ? (y[j] - ybar) * (y[j] - ybar) : 0.0;
    double tiny = 1e-6 * sqrt(ens_tree<NV>(s) / (Dd - 1.0));
    if (tiny == 0.0) tiny = 1.0;
    // ---- the start: ordinary bounded least squares ----
#pragma unroll
    for (int j = 0; j < NV; j++) w[j] = 1.0;
    int flags;
    rf_wls<NV>(x, y, w, lane, D, cst, g.lower, g.upper, f.a, f.b, flags);
    f.sigma = qnan;
    f.iters = 0;
    int hit_cap = 0;
    if (g.robust) {
        const int m = D - 1;                 // the sorted |radj| without its smallest member: places 1 .. D-1
        for (;;) {
#pragma unroll
            for (int j = 0; j < NV; j++) {
                w[j] = (y[j] - (f.a * x[j] + f.b)) * adj[j];                  // radj
                s[j] = j * 64 + lane < D ? fabs(w[j]) : (double)INFINITY;
            }
            ens_sort<NV>(s, lane);
            double med;
            if (m & 1) {
                med = ens_pick<NV>(s, 1 + (m - 1) / 2);
            } else {
                const double ml = ens_pick<NV>(s, m / 2), mh = ens_pick<NV>(s, m / 2 + 1);
                med = (ml + mh) / 2.0;
            }
            const double sg = med / 0.6745;
            f.sigma = sg > tiny ? sg : tiny;
            const double den = f.sigma * 4.685;
#pragma unroll
            for (int j = 0; j < NV; j++) {
                const double u = w[j] / den, t = 1.0 - u * u;
                w[j] = fabs(u) < 1.0 ? t * t : 0.0;
            }
            const double a0 = f.a, b0 = f.b;
            rf_wls<NV>(x, y, w, lane, D, cst, g.lower, g.upper, f.a, f.b, flags);
            f.iters++;
            const double se = 1.4901161193847656e-08;                        // sqrt(eps) = 2^-26
            if (fabs(f.a - a0) <= se * fmax(fabs(f.a), fabs(a0)) && fabs(f.b - b0) <= se * fmax(fabs(f.b), fabs(b0))) break;
            if (f.iters == g.max_iter) { hit_cap = kRfMaxiter; break; }
        }
    }
    f.status = (cst ? kRfConst : 0) | flags | hit_cap;
    if (store) {
        if (lane == 0) {
            if (g.a) g.a[oi] = f.a;
            if (g.b_item) g.b_item[oi] = f.b;
            if (g.sigma) g.sigma[oi] = f.sigma;
            if (g.iters) g.iters[oi] = f.iters;
            if (g.status) g.status[oi] = f.status;
        }
        if (g.weights) {
#pragma unroll
            for (int j = 0; j < NV; j++) {
                const int d = j * 64 + lane;
                if (d < D) g.weights[((size_t)d * n + (size_t)k) * R + r] = w[j];
            }
        }
    }
    return f;
}

template <int NV>
__global__ __launch_bounds__(64) void robfit_items(const RfArgs g)
{
    const long long item = g.item0 + (long long)blockIdx.x;              // item = k * R + r
    (void)rf_item<NV>(g, (int)(item / g.R), (size_t)(item % g.R), (int)threadIdx.x, true);
}

// b[r] = (1 / D) sum_d (y_d - sum_k X[d][k][r] a_k): the inner sum from 0 in ascending k, the outer sum the same tree
template <int NV>
__global__ __launch_bounds__(64) void robfit_intercept(const RfArgs g)
{
    const int lane = threadIdx.x, D = g.D;
    const size_t R = (size_t)g.R, n = (size_t)g.n, r = (size_t)(g.item0 + (long long)blockIdx.x);
    double s[NV];
#pragma unroll
    for (int j = 0; j < NV; j++) s[j] = 0.0;
    for (int k = 0; k < g.n; k++) {
        const double ak = g.a ? g.a[(size_t)k * R + r] : rf_item<NV>(g, k, r, lane, false).a;
#pragma unroll
        for (int j = 0; j < NV; j++) {
            const int d = j * 64 + lane;
            if (d < D) s[j] = s[j] + g.X[((size_t)d * n + (size_t)k) * R + r] * ak;
        }
    }
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const int d = j * 64 + lane;
        s[j] = d < D ? g.y[(size_t)d * R + r] - s[j] : 0.0;
    }
    const double b = (1.0 / (double)D) * ens_tree<NV>(s);
    if (lane == 0) g.b[r] = b;
}

template <int NV>
inline hipError_t rf_launch(const RfArgs &g, unsigned blocks, bool intercept, hipStream_t st)
{
    if (intercept) hipLaunchKernelGGL(robfit_intercept<NV>, dim3(blocks), dim3(64), 0, st, g);
    else hipLaunchKernelGGL(robfit_items<NV>, dim3(blocks), dim3(64), 0, st, g);
    return hipGetLastError();
}

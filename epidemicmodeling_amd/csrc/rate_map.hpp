// The NPI-to-growth-rate predictor of testScripts/test04FullFeatureExtMLpipeline.m (:292-404 the ridge-regularised linear
// map from the intervention plans and their lagged copies to the growth rate, :418-431 the policy tracker, :576-642 the clip
// and the rebuild of the new cases), one item per (train end k, region r).  Included by epiekf.hip (entry point
// epi_ratemap_run_device, include/epiekf.h).  DESIGN.md §4.11 pins the arithmetic; tests/rate_map_ref.c and
// tests/rate_map_ref.py restate it and the suites hold all three to the same bits.
//
// ratemap_items<NE>: one workgroup of 256 lanes per item.  The lower triangle of G = X'X and, as one more row, c = X'y are
// (F+1)(F+2)/2 - 1 entries; lane l owns the entries l, l + 256, ... (NE of them, in registers) and runs each entry's chain
// over the training days ascending.  The days are staged kRmDays at a time in LDS, normalised once.  The triangle then goes
// to LDS, where the Cholesky factorisation (column by column, row F riding along as the forward substitution) and the back
// substitution run in place.  The test days' predictions are one fma chain per day and lane; the running sum of the clipped
// rates is one lane's sequential pass over a staged block of 256 days.  No atomics, no scratch, no host synchronisation.
// The normalisation and the target fill depend on the region alone; an item computes them again (T F + T loads) rather than
// wait for another launch.
// ratemap_region: one workgroup per region for the three outputs that belong to the region: x_mx (a lane per column),
// y_filled and the policy tracker (one lane each, in waves of their own: both are sequential in the day).
#pragma once

constexpr int kRmMaxN = 24, kRmMaxLags = 3, kRmMaxE = 8, kRmMaxF = 96;
constexpr int kRmLeadingNan = 1, kRmNotPd = 2, kRmNonfinite = 4;      // epi_ratemap_status_bits
constexpr int kRmThreads = 256, kRmDays = 8, kRmTrainEnds = 64;
// workgroups per launch: a launch's thread count (workgroups x 256 lanes) is a 32-bit number in the HIP runtime (lasso.hpp)
constexpr int64_t kRmLaunchItems = (int64_t)1 << 22;

struct RmArgs {
    int T, n, R, E, n_lags, fit, effect_lag, F;
    int lags[kRmMaxLags];
    int k0;                                // the first train end of this launch
    long long item0;                       // the first item of this launch within its train ends: item = kk * R + r
    int nt[kRmTrainEnds];                  // n_train[k0 + kk]
    double ridge, thr, red;
    const double *ip, *y, *ns, *extra, *lambda_in;     // [T][n][R], [T][R], [T][R], [T][E][R], [K][T][R]
    double *map, *x_mx, *y_filled, *lambda_hat, *est, *tracker;
    int32_t *status;
};

EPI_DEV bool rm_finite(double v) { return fabs(v) < (double)INFINITY; }

// column f of [IP, lagged(lag1), .., extra] on day t (0-based) of region r, before the normalisation
EPI_DEV double rm_feat(const RmArgs &g, size_t r, int t, int f)
{
    const int nb = g.n * (1 + g.n_lags);
    if (f >= nb) return g.extra[((size_t)t * (size_t)g.E + (size_t)(f - nb)) * (size_t)g.R + r];
    const int b = f / g.n, p = f % g.n;
    const int lag = b == 0 ? 0 : g.lags[b - 1];
    if (t < lag) return 0.0;
    return g.ip[((size_t)(t - lag) * (size_t)g.n + (size_t)p) * (size_t)g.R + r];
}

// max(abs(column)) over all T days, NaN ignored (an all-NaN column gives NaN), 0 -> 1
EPI_DEV double rm_col_max(const RmArgs &g, size_t r, int f)
{
    double m = -1.0;
    for (int t = 0; t < g.T; t++) {
        const double a = fabs(rm_feat(g, r, t, f));
        if (a > m) m = a;
    }
    if (m < 0.0) return __builtin_nan("");
    return m == 0.0 ? 1.0 : m;
}

// doubles of dynamic LDS a workgroup of ratemap_items needs
inline size_t rm_lds_doubles(int F)
{
    return (size_t)(F + 1) * (F + 2) / 2 + (size_t)kRmDays * (F + 1) + 2 * (size_t)F + kRmThreads + 2;
}

extern __shared__ double rm_lds[];

template <int NE>
__global__ __launch_bounds__(kRmThreads) void ratemap_items(const RmArgs g)
{
    const int tid = threadIdx.x, T = g.T, F = g.F, W = F + 1;
    const long long item = g.item0 + (long long)blockIdx.x;
    const int kk = (int)(item / g.R), nt = g.nt[kk];
    const size_t R = (size_t)g.R, r = (size_t)(item % g.R), k = (size_t)(g.k0 + kk);
    const size_t o = k * (size_t)T * R + r;                       // lambda_hat / est / lambda_in of day t: o + t R
    const int nent = W * (W + 1) / 2 - 1;                          // the triangle of G, then row F = c
    double *A = rm_lds, *rows = A + nent + 1, *mxs = rows + kRmDays * W, *ms = mxs + F, *buf = ms + F;
    double *diag = rows;                                           // L's diagonal, once the staged days are consumed
    int *flag = (int *)(buf + kRmThreads);                         // [0]: a non-finite result
    const double qnan = __builtin_nan("");
    if (tid < 2) flag[tid] = 0;
    int fail = 0;
    if (g.fit) {
        if (tid < F) mxs[tid] = rm_col_max(g, r, tid);
        const double y0 = g.y[r];
        if (y0 != y0) fail = kRmLeadingNan;                        // the same in every lane
    }
    __syncthreads();
    if (g.fit && !fail) {
        // ---- G and c: every entry one chain over the training days ascending ----
        double acc[NE];
        int ei[NE], ej[NE];
#pragma unroll
        for (int q = 0; q < NE; q++) {
            const int e = tid + q * kRmThreads;
            int i = 0, j = 0;
            if (e < nent) {
                i = (int)((sqrt(8.0 * (double)e + 1.0) - 1.0) * 0.5);
                while (i * (i + 1) / 2 > e) i--;
                while ((i + 1) * (i + 2) / 2 <= e) i++;
                j = e - i * (i + 1) / 2;
            }
            ei[q] = i; ej[q] = j; acc[q] = 0.0;
        }
        double yprev = 0.0;
        for (int t0 = 0; t0 < nt; t0 += kRmDays) {
            const int nd = nt - t0 < kRmDays ? nt - t0 : kRmDays;
            for (int idx = tid; idx < nd * F; idx += kRmThreads) {
                const int d = idx / F, f = idx % F;
                rows[d * W + f] = rm_feat(g, r, t0 + d, f) / mxs[f];
            }
            if (tid == 0) {                                        // the target fill is sequential in the day
                for (int d = 0; d < nd; d++) {
                    double v = g.y[(size_t)(t0 + d) * R + r];
                    if (t0 + d > 0 && !rm_finite(v)) v = yprev;
                    yprev = v;
                    rows[d * W + F] = v;
                    if (g.lambda_hat) g.lambda_hat[o + (size_t)(t0 + d) * R] = v;
                    if (!rm_finite(v)) flag[0] = 1;
                }
            }
            __syncthreads();
            for (int d = 0; d < nd; d++) {
#pragma unroll
                for (int q = 0; q < NE; q++) {
                    const double a = rows[d * W + ei[q]], b = rows[d * W + ej[q]];
                    acc[q] = t0 + d == 0 ? a * b : fma(a, b, acc[q]);
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < NE; q++) {
            const int e = tid + q * kRmThreads;
            if (e < nent) A[e] = ei[q] == ej[q] ? acc[q] + g.ridge : acc[q];
        }
        __syncthreads();
        // ---- unblocked lower Cholesky, column by column; lane i owns row i, row F (c) becomes the forward substitution ----
        for (int j = 0; j < F; j++) {
            const double *Lj = A + (size_t)j * (j + 1) / 2;
            double piv = Lj[j];
            if (j > 0) {
                double d = Lj[0] * Lj[0];
                for (int q = 1; q < j; q++) d = fma(Lj[q], Lj[q], d);
                piv = piv - d;
            }
            if (!(piv > 0.0) || piv == (double)INFINITY) { fail = kRmNotPd; break; }     // the same in every lane
            const double ljj = sqrt(piv);
            double v = 0.0;
            if (tid > j && tid <= F) {
                const double *Li = A + (size_t)tid * (tid + 1) / 2;
                v = Li[j];
                if (j > 0) {
                    double d = Li[0] * Lj[0];
                    for (int q = 1; q < j; q++) d = fma(Li[q], Lj[q], d);
                    v = v - d;
                }
                v = v / ljj;
            }
            if (tid > j && tid <= F) A[(size_t)tid * (tid + 1) / 2 + j] = v;   // column j: read by no lane during step j
            if (tid == j) diag[j] = ljj;                                       // G(j,j) stays where every lane reads it
            __syncthreads();
        }
        if (!fail) {
            // ---- back substitution by columns: lane i's remainder loses L(k,i) m_k for k descending ----
            double s = tid < F ? A[(size_t)F * (F + 1) / 2 + tid] : 0.0;
            for (int q = F - 1; q >= 0; q--) {
                if (tid == q) ms[q] = s / diag[q];
                __syncthreads();
                if (tid < q) s = fma(-A[(size_t)q * (q + 1) / 2 + tid], ms[q], s);
            }
            if (tid < F) {
                const double m = ms[tid];
                if (g.map) g.map[(k * (size_t)F + (size_t)tid) * R + r] = m;
                if (!rm_finite(m)) flag[0] = 1;
            }
        }
    }
    if (fail) {                                                    // LEADING_NAN or NOT_PD: NaN outputs, that status alone
        __syncthreads();                                           // lane 0's training days of lambda_hat are behind us
        if (tid < F && g.map) g.map[(k * (size_t)F + (size_t)tid) * R + r] = qnan;
        for (int t = tid; t < T; t += kRmThreads) {
            if (g.lambda_hat) g.lambda_hat[o + (size_t)t * R] = qnan;
            if (g.est) g.est[o + (size_t)t * R] = qnan;
        }
        if (tid == 0 && g.status) g.status[k * R + r] = fail;
        return;
    }
    // ---- the training days: new_smoothed as it is; without a fit lambda_in as it is ----
    for (int t = tid; t < nt; t += kRmThreads) {
        const double v = g.ns[(size_t)t * R + r];
        if (g.est) g.est[o + (size_t)t * R] = v;
        if (!rm_finite(v)) flag[0] = 1;
        if (!g.fit) {
            const double l = g.lambda_in[o + (size_t)t * R];
            if (g.lambda_hat) g.lambda_hat[o + (size_t)t * R] = l;
            if (!rm_finite(l)) flag[0] = 1;
        }
    }
    // ---- the test days in blocks of 256: predict and clip (a lane per day), running sum (lane 0), exp (a lane per day) ----
    const double anchor = g.ns[(size_t)(nt - 1) * R + r];
    double cum = 0.0;
    for (int t0 = nt; t0 < T; t0 += kRmThreads) {
        const int t = t0 + tid, nd = T - t0 < kRmThreads ? T - t0 : kRmThreads;
        if (t < T) {
            double v;
            if (g.fit) {
                v = (rm_feat(g, r, t, 0) / mxs[0]) * ms[0];
                for (int f = 1; f < F; f++) v = fma(rm_feat(g, r, t, f) / mxs[f], ms[f], v);
            } else {
                v = g.lambda_in[o + (size_t)t * R];
            }
            if (v > g.thr) v = g.thr;
            else if (v < -g.thr) v = -g.thr;
            if (g.lambda_hat) g.lambda_hat[o + (size_t)t * R] = v;
            if (!rm_finite(v)) flag[0] = 1;
            buf[tid] = v;
        }
        __syncthreads();
        if (tid == 0) {
            for (int d = 0; d < nd; d++) {
                cum = cum + buf[d];
                buf[d] = cum;
            }
        }
        __syncthreads();
        if (t < T) {
            const double v = anchor * epi_exp(buf[tid]);
            if (g.est) g.est[o + (size_t)t * R] = v;
            if (!rm_finite(v)) flag[0] = 1;
        }
        __syncthreads();
    }
    __syncthreads();
    if (tid == 0 && g.status) g.status[k * R + r] = flag[0] ? kRmNonfinite : 0;
}

// x_mx, y_filled and the policy tracker of region item0 + blockIdx.x
__global__ __launch_bounds__(kRmThreads) void ratemap_region(const RmArgs g)
{
    const int tid = threadIdx.x, T = g.T, n = g.n;
    const size_t R = (size_t)g.R, r = (size_t)(g.item0 + (long long)blockIdx.x);
    if (g.x_mx && tid < g.F) g.x_mx[(size_t)tid * R + r] = rm_col_max(g, r, tid);
    if (g.y_filled && tid == 128) {
        double prev = 0.0;
        for (int t = 0; t < T; t++) {
            double v = g.y[(size_t)t * R + r];
            if (t > 0 && !rm_finite(v)) v = prev;
            prev = v;
            g.y_filled[(size_t)t * R + r] = v;
        }
    }
    if (g.tracker && tid == 192) {
        // day ii's event acts from day min(ii + effect_lag, T-1) on; that start never decreases with ii, so a running sum over
        // the events in order gives every day the additions of the reference's loop in the reference's order
        double run = 0.0, prev = 0.0;
        int ii = 1;
        for (int d = 0; d < T; d++) {
            for (; ii < T && (ii + g.effect_lag < T - 1 ? ii + g.effect_lag : T - 1) <= d; ii++) {
                if (ii == 1) {
                    prev = g.ip[r];
                    for (int p = 1; p < n; p++) prev = prev + g.ip[(size_t)p * R + r];
                    prev = prev / (double)n;
                }
                double cur = g.ip[((size_t)ii * (size_t)n) * R + r];
                for (int p = 1; p < n; p++) cur = cur + g.ip[((size_t)ii * (size_t)n + (size_t)p) * R + r];
                cur = cur / (double)n;
                if (cur > prev) run = run - g.red;
                else if (cur < prev) run = run + g.red;
                prev = cur;
            }
            g.tracker[(size_t)d * R + r] = run;
        }
    }
}

template <int NE>
inline hipError_t rm_launch_items(const RmArgs &g, unsigned blocks, hipStream_t st)
{
    hipLaunchKernelGGL(ratemap_items<NE>, dim3(blocks), dim3(kRmThreads), rm_lds_doubles(g.F) * sizeof(double), st, g);
    return hipGetLastError();
}

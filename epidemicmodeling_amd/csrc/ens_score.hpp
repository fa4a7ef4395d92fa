// Probabilistic forecast scores of the Monte-Carlo ensembles: an array of B = R * D chains (region-major, what ens_summary.hpp
// takes) and a truth -> the ensemble CRPS, the weighted interval score, the absolute error of the median, interval coverage and
// the rank of the truth of every (day, row, region), and per (row, region) their means over a window of days with the rank (PIT)
// histogram; included by epiekf.hip after ens_summary.hpp (entry point epi_escore_run_device, include/epiekf.h).  DESIGN.md
// §4.17 pins the arithmetic; tests/escore_ref.py and tests/escore_ref.c restate it and the GPU suite holds them to the same bits.
//
//   escore_items    one wavefront per item (day t, row, region r) in the shape of ens_summary<NV>: element e in register e / 64 of
//                   lane e % 64, NV = P / 64.  rank, ties and n by ballot on the unsorted members; then the members are sorted IN
//                   the array they were loaded into (ens_sort), the 2 n_a + 1 quantiles are picked (ens_pick) into scalars, and the
//                   same array is overwritten with the CRPS terms by sorted position and summed (ens_tree): one NV-double array
//                   lives at a time.  No LDS, no barrier, no atomics.
//   escore_regions  one lane per (row, region), regions fastest: the days k0 <= t < k1 in ascending order from 0.0.  No cross-lane
//                   operation.
//
// Host-compilation contract (loglik.hpp): the body of escore_regions is the EPI_DEV function escore_region_lane of its indices;
// tests/escore_emu.cpp compiles it with the host compiler (EPI_ESCORE_HOST: without the wavefront kernel) and calls it lane by
// lane.
#pragma once

constexpr int kEsMaxA = 8, kEsMaxBins = 32;

struct EsArgs {
    int T, rows, rows_out, R, D, Rt, n_a, n_bins, f32, derive, k0, k1;
    long long item0;                        // first item of this launch
    const void *src;                        // [T][rows][R * D], double or float
    const double *population;               // [R] (derive)
    const double *truth;                    // [T][rows_out][Rt]
    const int32_t *truth_series;            // [R] or NULL (r itself)
    const int32_t *first_day;               // [R] or NULL (0)
    double alpha[kEsMaxA], q_lo[kEsMaxA], q_hi[kEsMaxA];
    double *crps, *wis, *ae;                // [T][rows_out][R]: outputs or workspace or NULL
    double *width;                          // [T][n_a][rows_out][R]
    int32_t *rank, *ties, *cover, *count;   // [T][rows_out][R]
    double *crps_mean, *wis_mean, *ae_mean; // [rows_out][R]
    int32_t *n_scored;                      // [rows_out][R]
    double *cover_frac;                     // [n_a][rows_out][R]
    int32_t *pit_hist;                      // [n_bins][rows_out][R]
};

// ---- the region pass: means over the window, coverage fractions, the histogram of the non-randomised mid-rank ----
// The day's loads do not depend on whether the day is scored (an unscored day's values are loaded and dropped by a select), so
// the loads of several days are in flight together; the bin counters are registers picked by a compare, not by an index.
EPI_DEV void escore_region_lane(const EsArgs &a, int row, int r)
{
    const size_t R = (size_t)a.R, RO = (size_t)a.rows_out, col = (size_t)row * R + (size_t)r, plane = RO * R;
    const int fd = a.first_day ? a.first_day[r] : 0;
    const double qnan = __builtin_nan("");
    double sc = 0.0, sw = 0.0, sa = 0.0;
    int ns = 0, cov[kEsMaxA], hist[kEsMaxBins];
    for (int k = 0; k < kEsMaxA; k++) cov[k] = 0;
    for (int b = 0; b < kEsMaxBins; b++) hist[b] = 0;
    const long long nb = (long long)a.n_bins;
#pragma unroll 4
    for (int t = a.k0 > fd ? a.k0 : fd; t < a.k1; t++) {
        const size_t o = (size_t)t * plane + col;
        const int rank = a.rank[o];
        const bool on = rank >= 0;
        ns += on ? 1 : 0;
        if (a.crps_mean) { const double v = a.crps[o]; sc = on ? sc + v : sc; }
        if (a.wis_mean) { const double v = a.wis[o]; sw = on ? sw + v : sw; }
        if (a.ae_mean) { const double v = a.ae[o]; sa = on ? sa + v : sa; }
        if (a.cover_frac) {
            const int c = a.cover[o];                                // 0 for an unscored item
            for (int k = 0; k < kEsMaxA; k++) cov[k] += (c >> k) & 1;
        }
        if (a.pit_hist) {
            const long long num = (2ll * rank + a.ties[o] + 1ll) * nb, den = 2ll * ((long long)a.count[o] + 1ll);    // count >= 0: den >= 2
            long long q = num / den;
            if (q > nb - 1) q = nb - 1;
            const int b = on ? (int)q : -1;
            for (int k = 0; k < kEsMaxBins; k++) hist[k] += b == k ? 1 : 0;
        }
    }
    if (a.n_scored) a.n_scored[col] = ns;
    if (a.crps_mean) a.crps_mean[col] = ns ? sc / (double)ns : qnan;
    if (a.wis_mean) a.wis_mean[col] = ns ? sw / (double)ns : qnan;
    if (a.ae_mean) a.ae_mean[col] = ns ? sa / (double)ns : qnan;
    if (a.cover_frac)
        for (int k = 0; k < kEsMaxA; k++)
            if (k < a.n_a) a.cover_frac[(size_t)k * plane + col] = ns ? (double)cov[k] / (double)ns : qnan;
    if (a.pit_hist)
        for (int k = 0; k < kEsMaxBins; k++)
            if (k < a.n_bins) a.pit_hist[(size_t)k * plane + col] = hist[k];
}

#ifndef EPI_ESCORE_HOST
EPI_DEV double es_load(const EsArgs &a, size_t o)
{
    return a.f32 ? (double)((const float *)a.src)[o] : ((const double *)a.src)[o];
}

// the quantile at p of the sorted members x(1 .. n), n >= 1: the expression of ens_summary (MATLAB's quantile)
template <int NV>
EPI_DEV double es_quantile(const double (&w)[NV], int n, double p, double x1, double xn)
{
    const double h = (double)n * p + 0.5;
    const double kf = floor(h), g = h - kf;
    if (kf < 1.0) return x1;
    if (kf >= (double)n) return xn;
    const int ki = (int)kf;                                          // 1 .. n-1
    const double xk = ens_pick<NV>(w, ki - 1), xk1 = ens_pick<NV>(w, ki);
    return xk + g * (xk1 - xk);
}

template <int NV>
__global__ __launch_bounds__(64) void escore_items(const EsArgs a)
{
    const int lane = threadIdx.x, D = a.D;
    const long long item = a.item0 + (long long)blockIdx.x;
    const int row = (int)(item % a.rows_out);
    const long long tr = item / a.rows_out;
    const int r = (int)(tr % a.R);
    const size_t t = (size_t)(tr / a.R), B = (size_t)a.R * (size_t)D;
    const double qnan = __builtin_nan("");
    double w[NV];
    // ---- the item's members (absent = NaN), as ens_summary loads them ----
    if (row < a.rows) {
        const size_t o = (t * (size_t)a.rows + (size_t)row) * B + (size_t)r * (size_t)D;
#pragma unroll
        for (int j = 0; j < NV; j++) {
            const int e = j * 64 + lane;
            w[j] = e < D ? es_load(a, o + (size_t)e) : qnan;
        }
    } else {                            // the derived row: ((N_r v0) v1) v2 of rows 0, 1, 2
        const size_t o = t * (size_t)a.rows * B + (size_t)r * (size_t)D;
        const double N = a.population[r];
#pragma unroll
        for (int j = 0; j < NV; j++) {
            const int e = j * 64 + lane;
            w[j] = e < D ? ((N * es_load(a, o + (size_t)e)) * es_load(a, o + B + (size_t)e)) * es_load(a, o + 2 * B + (size_t)e) : qnan;
        }
    }
    const int ts = a.truth_series ? a.truth_series[r] : r;
    const double y = a.truth[(t * (size_t)a.rows_out + (size_t)row) * (size_t)a.Rt + (size_t)ts];
    // ---- n, rank, ties: ballots over the unsorted members (a NaN compares false) ----
    int n = 0, rank = 0, ties = 0;
#pragma unroll
    for (int j = 0; j < NV; j++) {
        n += __popcll(__ballot(w[j] == w[j]));
        rank += __popcll(__ballot(w[j] < y));
        ties += __popcll(__ballot(w[j] == y));
    }
    const size_t plane = (size_t)a.rows_out * (size_t)a.R;
    const size_t oo = t * plane + (size_t)row * (size_t)a.R + (size_t)r;
    if (n == 0 || y != y) {
        if (lane == 0) {
            if (a.count) a.count[oo] = n;
            if (a.rank) a.rank[oo] = -1;
            if (a.ties) a.ties[oo] = -1;
            if (a.cover) a.cover[oo] = 0;
            if (a.crps) a.crps[oo] = qnan;
            if (a.wis) a.wis[oo] = qnan;
            if (a.ae) a.ae[oo] = qnan;
            if (a.width)
                for (int k = 0; k < a.n_a; k++) a.width[(t * (size_t)a.n_a + (size_t)k) * plane + (size_t)row * (size_t)a.R + (size_t)r] = qnan;
        }
        return;
    }
    if (lane == 0) {
        if (a.count) a.count[oo] = n;
        if (a.rank) a.rank[oo] = rank;
        if (a.ties) a.ties[oo] = ties;
    }
    if (!(a.crps || a.wis || a.ae || a.cover || a.width)) return;
    // ---- the members ascending, the absent ones +Inf behind them ----
#pragma unroll
    for (int j = 0; j < NV; j++) w[j] = w[j] == w[j] ? w[j] : (double)INFINITY;
    ens_sort<NV>(w, lane);
    // ---- the median and the central intervals: ae, wis, cover, width ----
    if (a.wis || a.ae || a.cover || a.width) {
        const double x1 = ens_pick<NV>(w, 0), xn = ens_pick<NV>(w, n - 1);
        const double med = es_quantile<NV>(w, n, 0.5, x1, xn);
        const double ae = fabs(y - med);
        double acc = 0.5 * ae;
        int cover = 0;
        for (int k = 0; k < a.n_a; k++) {
            const double l = es_quantile<NV>(w, n, a.q_lo[k], x1, xn), u = es_quantile<NV>(w, n, a.q_hi[k], x1, xn);
            const double wd = u - l, c = 2.0 / a.alpha[k];
            const double dl = l - y, du = y - u;
            const double is = (wd + c * (dl > 0.0 ? dl : 0.0)) + c * (du > 0.0 ? du : 0.0);
            acc = acc + (a.alpha[k] / 2.0) * is;
            cover |= (l <= y && y <= u) ? 1 << k : 0;
            if (lane == 0 && a.width) a.width[(t * (size_t)a.n_a + (size_t)k) * plane + (size_t)row * (size_t)a.R + (size_t)r] = wd;
        }
        if (lane == 0) {
            if (a.ae) a.ae[oo] = ae;
            if (a.wis) a.wis[oo] = acc / ((double)a.n_a + 0.5);
            if (a.cover) a.cover[oo] = cover;
        }
    }
    if (!a.crps) return;
    // ---- crps = (2 / n^2) sum_i (x(i) - y) (n [y < x(i)] - i + 0.5), the terms by sorted position through the tree ----
    const double nd = (double)n;
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const int e = j * 64 + lane;                                  // sorted position i - 1
        const double coef = ((y < w[j] ? nd : 0.0) - (double)(e + 1)) + 0.5;
        w[j] = e < n ? (w[j] - y) * coef : 0.0;
    }
    const double sum = ens_tree<NV>(w);
    if (lane == 0) a.crps[oo] = (2.0 / (nd * nd)) * sum;
}

template <int NV>
inline hipError_t escore_launch(const EsArgs &g, unsigned items, hipStream_t st)
{
    hipLaunchKernelGGL(escore_items<NV>, dim3(items), dim3(64), 0, st, g);
    return hipGetLastError();
}

constexpr int kEsRegionWg = 256;
__global__ __launch_bounds__(kEsRegionWg) void escore_regions(const EsArgs a)
{
    const long long i = (long long)blockIdx.x * kEsRegionWg + threadIdx.x;
    if (i >= (long long)a.rows_out * a.R) return;
    escore_region_lane(a, (int)(i / a.R), (int)(i % a.R));
}
#endif

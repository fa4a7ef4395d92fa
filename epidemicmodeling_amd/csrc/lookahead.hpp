// Tools/ForecastQualityAssessment.m:359-393, 428-449 -- the forecast look-ahead error study around the 3-state filter;
// included by epiekf.hip (entry point epi_lookahead_run_device).
//
// Chain c = r * F + (s - 1) is region r with its last s observations masked.  lookahead_expand materialises the masked batch
// (x, R_v and the per-chain parameter columns) in the workspace so that the unchanged filter kernels run it; the filter and
// smoother write S_PLUS / S_SMOOTH [LL][3][R * F]; lookahead_errors turns them into the two error tables and lookahead_stats
// reduces each table column.  Operation order is MATLAB's, one IEEE rounding per written operation (-ffp-contract=off).
#pragma once

constexpr int kLaLaunchColumns = 1 << 25;             // lookahead_stats: columns (64-lane workgroups) per launch
constexpr size_t kLaLaunchElements = (size_t)1 << 31; // lookahead_errors: table elements (lanes) per launch
struct LaArgs {
    int R, LL, F, M, n_npi, r_mode;
    // first table column of a lookahead_stats launch and first table element of a lookahead_errors launch: both grids are
    // launched in slices, a launch's thread count being a 32-bit number in the HIP runtime (beyond it the count wraps silently)
    int col0;
    size_t e0;
    // per-region inputs
    const double *x, *R_series, *R_scalar, *prm, *s_init, *Ps_init, *s_final, *Ps_final, *Q, *truth, *population;
    // per-chain copies (workspace)
    double *cx, *cR_series, *cR_scalar, *cprm, *cs_init, *cPs_init, *cs_final, *cPs_final, *cQ;
    int32_t *u_series;
    // filter outputs [LL][3][R * F]
    const double *S_PLUS, *S_SMOOTH;
    // results
    double *est_plus, *est_smooth;                              // [F][M][R]
    double *mean_plus, *median_plus, *std_plus, *mean_smooth, *median_smooth, *std_smooth;   // [M][R]
};

// rows of the per-chain arrays lookahead_expand writes, after the LL rows of x and (r_mode 1) the LL rows of R_series
constexpr int kLaChainRows = EPI_PRM_COUNT + 3 + 9 + 3 + 9 + 9 + 1;   // prm, s_init, Ps_init, s_final, Ps_final, Q, R_scalar

// grid (ceil(B / 256), rows): row y < LL is day y of x (NaN from day LL - s on; u_series with it on day 0), then the days of
// R_series, then the per-chain columns, all copied from column r
__global__ __launch_bounds__(256) void lookahead_expand(const LaArgs a, int nrows)
{
    const int B = a.R * a.F;
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= B) return;
    const int r = c / a.F, s = c - r * a.F + 1;
    const size_t Bs = (size_t)B, Rs = (size_t)a.R;
    for (int y = blockIdx.y; y < nrows; y += gridDim.y) {
        if (y < a.LL) {                                           // observations_PARTIAL(LL - start + 1 : LL) = nan  (:384-385)
            a.cx[(size_t)y * Bs + c] = (y >= a.LL - s) ? __builtin_nan("") : a.x[(size_t)y * Rs + r];
            if (y == 0) a.u_series[c] = r;                        // every chain of a region reads its controls
            continue;
        }
        int k = y - a.LL;
        if (a.r_mode == 1) {
            if (k < a.LL) { a.cR_series[(size_t)k * Bs + c] = a.R_series[(size_t)k * Rs + r]; continue; }
            k -= a.LL;
        }
        const double *src; double *dst; int row;
        if (k < EPI_PRM_COUNT) { src = a.prm; dst = a.cprm; row = k; }
        else if ((k -= EPI_PRM_COUNT) < 3) { src = a.s_init; dst = a.cs_init; row = k; }
        else if ((k -= 3) < 9) { src = a.Ps_init; dst = a.cPs_init; row = k; }
        else if ((k -= 9) < 3) { src = a.s_final; dst = a.cs_final; row = k; }
        else if ((k -= 3) < 9) { src = a.Ps_final; dst = a.cPs_final; row = k; }
        else if ((k -= 9) < 9) { src = a.Q; dst = a.cQ; row = k; }
        else { if (a.r_mode != 0) continue; src = a.R_scalar; dst = a.cR_scalar; row = 0; }
        dst[(size_t)row * Bs + c] = src[(size_t)row * Rs + r];
    }
}

// one lane per (start s, look-ahead day j, region r), r fastest: EstError_*(s, j) of :387-391
__global__ __launch_bounds__(256) void lookahead_errors(const LaArgs a)
{
    const size_t n = (size_t)a.F * a.M * a.R;
    const size_t e = a.e0 + (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int r = (int)(e % a.R);
    const int j = (int)((e / a.R) % a.M) + 1;
    const int s = (int)(e / ((size_t)a.R * a.M)) + 1;
    double ep = 0.0, es = 0.0;                                    // EstError_* = zeros(num_forecast_days, MaxLookAheadDays)
    if (j <= s) {                                                 // j <= min(s, M): last_index - LL + start = min(s, M)
        const size_t B = (size_t)a.R * a.F, c = (size_t)r * a.F + (s - 1);
        const int t = a.LL - s + j - 1;
        const double N = a.population[r], tr = a.truth[(size_t)t * a.R + r];
        const double *P = a.S_PLUS + (size_t)t * 3 * B + c, *S = a.S_SMOOTH + (size_t)t * 3 * B + c;
        const double est_p = ((N * P[0]) * P[B]) * P[2 * B];     // N_population * S(1,:).*S(2,:).*S(3,:)  (:387-388)
        const double est_s = ((N * S[0]) * S[B]) * S[2 * B];
        ep = (100.0 * fabs(tr - est_p)) / tr;                     // 100 * abs(truth - est) ./ truth  (:389-390)
        es = (100.0 * fabs(tr - est_s)) / tr;
    }
    a.est_plus[e] = ep;
    a.est_smooth[e] = es;
}

constexpr int kLaMaxF = 1024;   // rows of a table column staged in LDS (epi_lookahead_validate: F <= 1024)

EPI_DEV double la_sign(double v) { return (double)((v > 0.0) - (v < 0.0)); }

// one wavefront per (look-ahead day j, region r) column and table (blockIdx.y: 0 = PLUS, 1 = SMOOTH): mean / median / std over
// rows s = M .. F (:428-449: mean(EstError(MaxLookAheadDays:end, :), 1) etc.).  The median is exact: every value's position in
// the stable ascending order is counted against all others, the two middle positions are picked.
__global__ __launch_bounds__(kWave) void lookahead_stats(const LaArgs a)
{
    __shared__ double v[kLaMaxF];
    __shared__ double mid[2];
    __shared__ int has_nan;
    const int col = a.col0 + (int)blockIdx.x;                     // col = j0 * R + r
    const int lane = threadIdx.x;
    const bool smooth = blockIdx.y == 1;
    const double *tbl = smooth ? a.est_smooth : a.est_plus;
    double *o_mean = smooth ? a.mean_smooth : a.mean_plus, *o_med = smooth ? a.median_smooth : a.median_plus;
    double *o_std = smooth ? a.std_smooth : a.std_plus;
    const int n = a.F - a.M + 1;
    if (n <= 0) {                                                 // MATLAB over an empty range: NaN
        if (lane == 0) { o_mean[col] = __builtin_nan(""); o_med[col] = __builtin_nan(""); o_std[col] = __builtin_nan(""); }
        return;
    }
    const size_t MR = (size_t)a.M * a.R;
    if (lane == 0) has_nan = 0;
    __syncthreads();
    int nan_here = 0;
    for (int i = lane; i < n; i += kWave) {
        const double x = tbl[(size_t)(a.M - 1 + i) * MR + col];
        v[i] = x;
        nan_here |= x != x;
    }
    if (nan_here) has_nan = 1;
    __syncthreads();
    if (lane == 0) {
        double sum = 0.0;
        for (int i = 0; i < n; i++) sum += v[i];
        const double mean = sum / (double)n;
        double sq = 0.0;
        for (int i = 0; i < n; i++) { const double d = v[i] - mean; sq += d * d; }
        o_mean[col] = mean;
        o_std[col] = n == 1 ? 0.0 : sqrt(sq / (double)(n - 1));
    }
    if (has_nan) {
        if (lane == 0) o_med[col] = __builtin_nan("");
        return;
    }
    const int lo = (n - 1) / 2, hi = n / 2;
    for (int i = lane; i < n; i += kWave) {
        const double x = v[i];
        int rank = 0;
        for (int k = 0; k < n; k++) {
            const double y = v[k];
            rank += (y < x) || (y == x && k < i);
        }
        if (rank == lo) mid[0] = x;
        if (rank == hi) mid[1] = x;
    }
    __syncthreads();
    if (lane == 0) {
        // MATLAB's median midpoint as we read it (the reference's toolbox source is not available to check against, nor is a
        // MATLAB to run): a + (b - a) / 2, or (a + b) / 2 when a and b differ in sign or either is infinite
        const double x0 = mid[0], x1 = mid[1];
        double med = x0;
        if (hi != lo) med = (la_sign(x0) != la_sign(x1) || isinf(x0) || isinf(x1)) ? (x0 + x1) / 2.0 : x0 + (x1 - x0) / 2.0;
        o_med[col] = med;
    }
}

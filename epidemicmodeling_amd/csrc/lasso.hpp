// REGRESSION_TYPE = 'LASSO' between the EKF rounds: lasso(X, y, 'CV', K) for every region (Tools/TrainPredictPrescribeNPI.m:
// 254-290, ForecastQualityAssessment.m:256-292); included by epiekf.hip (entry point epi_lasso_run_device, include/epiekf.h).
// DESIGN.md §4.5 is our reading of lasso, point by point; tests/lasso_ref.c restates it in C and the GPU suite holds the
// two to the same bits.
//
// One wavefront per region.  Lane f < K fits fold f's training set, lane K the whole window (K = 0: lane 0, path only);
// the other lanes only take part in the barriers.  Every lane runs its own warm-started coordinate-descent path along the
// lambda sequence that lane K derives from the full-data sums; the lanes meet once per lambda, when the folds' held-out
// SSEs are reduced in fold order into MSE(k) and SE(k).
//
// LDS (dynamic, D <= 256, n <= 12, NL <= 100: at most 162 208 B of the 160 KiB):
//   X [D][n] and y [D] of the region (read by every lane at the same address: broadcast), fold [D],
//   r [D][64] the residual of every lane, sample-major (lane-consecutive doubles: conflict-free),
//   the per-fold SSE and SSE / |fold| of the current lambda, lambda [NL] (descending), MSE / SE [NL] (ascending).
// The per-column state (mu, sigma, colsq, b, B) is held in registers: every loop over the columns is fully unrolled to
// kLsMaxN, so each array is indexed by constants and nothing goes to scratch.  Xs(i,j) = (X(i,j) - mu_j) / sigma_j is
// recomputed where it is used (no per-lane copy of the standardized block fits in LDS); the recomputation rounds the same
// way every time.
#pragma once

constexpr int kLsMaxN = 12, kLsMaxD = 256, kLsMaxK = 63, kLsMaxNL = 100;

struct LsArgs {
    int R, D, n, K, NL, max_iter;
    int r0;                        // first region of this launch (the regions are launched in slices, see kLsLaunchRegions)
    double ratio, rel_tol;
    const double *X, *y;           // [D][n][R], [D][R]
    const int32_t *fold;           // [D][R] (K >= 2)
    double *a, *b, *lambda, *B, *intercept, *mse, *se;
    int32_t *df, *iters, *idx_min, *idx_1se, *status;
};

// regions per launch: a launch's thread count (workgroups x 64 lanes) is a 32-bit number in the HIP runtime, beyond it the count
// wraps silently (2^26 + 1000 regions in one launch ran 1 000 of them and returned hipSuccess)
constexpr int kLsLaunchRegions = 1 << 25;

inline size_t lasso_lds_bytes(int D, int n, int NL)
{
    return ((size_t)D * n + D + (size_t)D * 64 + 128 + 3 * (size_t)NL + 8) * sizeof(double) + (size_t)D * sizeof(int);
}

struct LsLane {                    // the fit of one lane: its sample set and its iterate
    double N, muY, mu[kLsMaxN], sigma[kLsMaxN], colsq[kLsMaxN], b[kLsMaxN];
    int cnt, cst, active;
};

// one coordinate update of column j at lambda lam: rj = r + Xs_j b_j, rho = Xs_j' rj / N,
// b_j = sign(rho) max(|rho| - lam, 0) / colsq_j, r = rj - Xs_j b_j
EPI_DEV double lasso_update(const double *sX, double *sr, const int *sfold, int D, int n, int j, int lane, bool full,
                            double mu, double sg, double cq, double N, double bj, double lam)
{
    double rho = 0.0;
    for (int i = 0; i < D; i++) {
        if (full || sfold[i] != lane) {
            const double xs = (sX[i * n + j] - mu) / sg;
            const double rj = sr[i * 64 + lane] + xs * bj;
            sr[i * 64 + lane] = rj;
            rho = rho + xs * rj;
        }
    }
    rho = rho / N;
    double t = fabs(rho) - lam;
    t = t > 0.0 ? t : 0.0;
    const double bn = (rho > 0.0 ? t : (rho < 0.0 ? -t : 0.0)) / cq;
    for (int i = 0; i < D; i++) {
        if (full || sfold[i] != lane) {
            const double xs = (sX[i * n + j] - mu) / sg;
            sr[i * 64 + lane] = sr[i * 64 + lane] - xs * bn;
        }
    }
    return bn;
}

// coordinate descent at one lambda from the lane's current iterate; returns the cycles run, sets hit at max_iter
EPI_DEV int lasso_descend(LsLane &L, const double *sX, double *sr, const int *sfold, int D, int n, int lane, bool full,
                          double lam, double rel_tol, int max_iter, bool &hit)
{
    int it = 0;
    for (;;) {
        while (L.active) {
            if (it >= max_iter) { hit = true; return it; }
            double dmax = 0.0;
#pragma unroll
            for (int j = 0; j < kLsMaxN; j++) {
                if (j < n && (L.active >> j & 1)) {
                    const double bold = L.b[j];
                    L.b[j] = lasso_update(sX, sr, sfold, D, n, j, lane, full, L.mu[j], L.sigma[j], L.colsq[j], L.N, bold, lam);
                    const double d = fabs(L.b[j] - bold) / (1.0 + fabs(bold));
                    if (d > dmax) dmax = d;
                }
            }
            it++;
            if (dmax < rel_tol) break;
        }
        if (it >= max_iter) { hit = true; return it; }
        int grew = 0;
#pragma unroll
        for (int j = 0; j < kLsMaxN; j++) {
            if (j < n && !((L.active | L.cst) >> j & 1)) {
                L.b[j] = lasso_update(sX, sr, sfold, D, n, j, lane, full, L.mu[j], L.sigma[j], L.colsq[j], L.N, L.b[j], lam);
                if (L.b[j] != 0.0) grew |= 1 << j;
            }
        }
        it++;
        if (!grew) return it;
        L.active |= grew;
    }
}

// B = b ./ sigma (constant columns 0), Intercept = muY - sum_j mu_j B_j (sequential); returns df
EPI_DEV int lasso_coefs(const LsLane &L, int n, double (&Bv)[kLsMaxN], double &icpt)
{
    double s = 0.0;
    int df = 0;
#pragma unroll
    for (int j = 0; j < kLsMaxN; j++) {
        if (j < n) {
            Bv[j] = (L.cst >> j & 1) ? 0.0 : L.b[j] / L.sigma[j];
            s = s + L.mu[j] * Bv[j];
            df += Bv[j] != 0.0;
        }
    }
    icpt = L.muY - s;
    return df;
}

__global__ __launch_bounds__(64) void lasso_cv(const LsArgs a)
{
    extern __shared__ double ls_lds[];
    const int D = a.D, n = a.n, K = a.K, NL = a.NL, R = a.R;
    const int reg = a.r0 + (int)blockIdx.x, lane = threadIdx.x;
    const bool cv = K >= 2;
    double *sX = ls_lds, *sy = sX + (size_t)D * n, *sr = sy + D, *ssse = sr + (size_t)D * 64, *smf = ssse + 64;
    double *slam = smf + 64, *smse = slam + NL, *sse = smse + NL, *smisc = sse + NL;
    int *sfold = (int *)(smisc + 8);
    for (int e = lane; e < D * n; e += 64) sX[e] = a.X[(size_t)e * R + reg];
    for (int i = lane; i < D; i += 64) {
        sy[i] = a.y[(size_t)i * R + reg];
        sfold[i] = cv ? a.fold[(size_t)i * R + reg] : 0;
    }
    __syncthreads();
    int nonfin = 0, badf = 0;
    for (int e = lane; e < D * n; e += 64) nonfin |= is_nonfinite(sX[e]) ? 1 : 0;
    for (int i = lane; i < D; i += 64) {
        nonfin |= is_nonfinite(sy[i]) ? 1 : 0;
        if (cv && (sfold[i] < 0 || sfold[i] >= K)) badf = 1;
    }
    if (cv && lane < K) {
        int c = 0;
        for (int i = 0; i < D; i++) c += sfold[i] == lane;
        if (c == 0) badf = 1;
    }
    badf = __syncthreads_or(badf);
    nonfin = __syncthreads_or(nonfin);
    const double qnan = __builtin_nan("");
    if (badf || nonfin) {
        if (lane == 0) {
            for (int k = 0; k < NL; k++) {
                const size_t o = (size_t)k * R + reg;
                if (a.lambda) a.lambda[o] = qnan;
                if (a.intercept) a.intercept[o] = qnan;
                if (a.mse) a.mse[o] = qnan;
                if (a.se) a.se[o] = qnan;
                if (a.df) a.df[o] = 0;
                if (a.iters) a.iters[o] = 0;
                if (a.B) for (int j = 0; j < n; j++) a.B[((size_t)k * n + j) * R + reg] = qnan;
            }
            if (a.a) for (int j = 0; j < n; j++) a.a[(size_t)j * R + reg] = qnan;
            if (a.b) a.b[reg] = qnan;
            if (a.idx_min) a.idx_min[reg] = -1;
            if (a.idx_1se) a.idx_1se[reg] = -1;
            a.status[reg] = badf ? EPI_LASSO_BAD_FOLDS : EPI_LASSO_NONFINITE;
        }
        return;
    }
    const bool live = lane <= K, full = lane == K;
    // ---- the lane's sample set: mu, sigma, colsq, mean(y) and the residual r = y - mean(y) ----
    LsLane L;
    L.cnt = 0; L.cst = 0; L.active = 0; L.N = 1.0; L.muY = 0.0;
#pragma unroll
    for (int j = 0; j < kLsMaxN; j++) { L.mu[j] = 0.0; L.sigma[j] = 1.0; L.colsq[j] = 1.0; L.b[j] = 0.0; }
    if (live) {
        for (int i = 0; i < D; i++) L.cnt += (full || sfold[i] != lane) ? 1 : 0;
        L.N = (double)L.cnt;
#pragma unroll
        for (int j = 0; j < kLsMaxN; j++) {
            if (j < n) {
                double s = 0.0, mx = -(double)INFINITY, mn = (double)INFINITY;
                for (int i = 0; i < D; i++)
                    if (full || sfold[i] != lane) {
                        const double v = sX[i * n + j];
                        s = s + v;
                        if (v > mx) mx = v;
                        if (v < mn) mn = v;
                    }
                L.mu[j] = s / L.N;
                if (mx == mn) {
                    L.cst |= 1 << j;
                } else {
                    s = 0.0;
                    for (int i = 0; i < D; i++)
                        if (full || sfold[i] != lane) { const double d = sX[i * n + j] - L.mu[j]; s = s + d * d; }
                    L.sigma[j] = sqrt(s / L.N);
                    s = 0.0;
                    for (int i = 0; i < D; i++)
                        if (full || sfold[i] != lane) { const double xs = (sX[i * n + j] - L.mu[j]) / L.sigma[j]; s = s + xs * xs; }
                    L.colsq[j] = s / L.N;
                }
            }
        }
        double s = 0.0;
        for (int i = 0; i < D; i++) if (full || sfold[i] != lane) s = s + sy[i];
        L.muY = s / L.N;
        for (int i = 0; i < D; i++) sr[i * 64 + lane] = (full || sfold[i] != lane) ? sy[i] - L.muY : 0.0;
    }
    // ---- the lambda sequence from the full fit ----
    if (full) {
        double lmax = 0.0, ymx = -(double)INFINITY, ymn = (double)INFINITY;
#pragma unroll
        for (int j = 0; j < kLsMaxN; j++) {
            if (j < n && !(L.cst >> j & 1)) {
                double s = 0.0;
                for (int i = 0; i < D; i++) s = s + (sX[i * n + j] - L.mu[j]) / L.sigma[j] * sr[i * 64 + lane];
                const double v = fabs(s) / L.N;
                if (v > lmax) lmax = v;
            }
        }
        for (int i = 0; i < D; i++) { if (sy[i] > ymx) ymx = sy[i]; if (sy[i] < ymn) ymn = sy[i]; }
        const bool null_model = L.cst == (1 << n) - 1 || ymx == ymn || !(lmax > 0.0);
        smisc[0] = null_model ? 1.0 : 0.0;
        if (null_model) {
            for (int k = 0; k < NL; k++) slam[k] = 0.0;
        } else if (NL == 1) {
            slam[0] = lmax;
        } else {
            const double l0 = epi_log(lmax), l1 = epi_log(lmax * a.ratio);
            const double st = (l1 - l0) / (double)(NL - 1);
            for (int k = 0; k < NL; k++) slam[k] = epi_exp(l0 + (double)k * st);
        }
    }
    __syncthreads();
    const bool null_model = smisc[0] != 0.0;
    // ---- the path, largest lambda first ----
    bool hit = false;
    int im = -1;
    double best = (double)INFINITY, Bv[kLsMaxN], av[kLsMaxN], bv = qnan;
#pragma unroll
    for (int j = 0; j < kLsMaxN; j++) av[j] = qnan;
    for (int k = 0; k < NL; k++) {
        const int kk = NL - 1 - k;
        if (live) {
            int it = 0;
            if (!null_model) it = lasso_descend(L, sX, sr, sfold, D, n, lane, full, slam[k], a.rel_tol, a.max_iter, hit);
            double icpt;
            const int dfk = lasso_coefs(L, n, Bv, icpt);
            if (full) {
                const size_t o = (size_t)kk * R + reg;
                if (a.lambda) a.lambda[o] = slam[k];
                if (a.B) {
#pragma unroll
                    for (int j = 0; j < kLsMaxN; j++) if (j < n) a.B[((size_t)kk * n + j) * R + reg] = Bv[j];
                }
                if (a.intercept) a.intercept[o] = icpt;
                if (a.df) a.df[o] = dfk;
                if (a.iters) a.iters[o] = it;
            } else {                                    // SSE over the held-out days
                double s = 0.0;
                for (int i = 0; i < D; i++) {
                    if (sfold[i] != lane) continue;
                    double xb = 0.0;
#pragma unroll
                    for (int j = 0; j < kLsMaxN; j++) if (j < n) xb = xb + sX[i * n + j] * Bv[j];
                    const double e = (sy[i] - icpt) - xb;
                    s = s + e * e;
                }
                ssse[lane] = s;
                smf[lane] = s / (double)(D - L.cnt);
            }
        }
        if (cv) {
            __syncthreads();
            if (full) {
                double s = 0.0, m = 0.0, v = 0.0;
                for (int f = 0; f < K; f++) s = s + ssse[f];
                for (int f = 0; f < K; f++) m = m + smf[f];
                m = m / (double)K;
                for (int f = 0; f < K; f++) { const double d = smf[f] - m; v = v + d * d; }
                const double msek = s / (double)D, sek = sqrt(v / (double)(K - 1)) / sqrt((double)K);
                smse[kk] = msek; sse[kk] = sek;
                const size_t o = (size_t)kk * R + reg;
                if (a.mse) a.mse[o] = msek;
                if (a.se) a.se[o] = sek;
                if (msek <= best) {                     // descending lambda: ties go to the smaller index
                    double icpt;
                    best = msek; im = kk;
                    lasso_coefs(L, n, av, icpt);
                    bv = icpt;
                }
            }
            __syncthreads();
        }
    }
    const int any_hit = __syncthreads_or(hit ? 1 : 0);
    if (full) {
        if (cv) {
            int i1 = -1;
            if (im >= 0) {
                const double thr = smse[im] + sse[im];
                for (int k = NL - 1; k >= 0; k--) if (smse[k] <= thr) { i1 = k; break; }
            }
            if (a.idx_min) a.idx_min[reg] = im;
            if (a.idx_1se) a.idx_1se[reg] = i1;
#pragma unroll
            for (int j = 0; j < kLsMaxN; j++) if (j < n) a.a[(size_t)j * R + reg] = av[j];
            a.b[reg] = bv;
        }
        a.status[reg] = null_model ? EPI_LASSO_NULL_MODEL : any_hit ? EPI_LASSO_MAXITER : EPI_LASSO_OK;
    }
}

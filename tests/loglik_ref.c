/* The bit-exact C yardstick of the innovation log-likelihood (csrc/loglik.hpp is held to it bit for bit).
 * An independent restatement: one chain at a time, one sequential walk over the filter steps, classic [T][rows][B] doubles
 * (tests/loglik_ref.py rounds them once for float storage), the two windows of the replay as plain histories.
 * Build: cc -O2 -ffp-contract=off -mfma -fPIC -shared (no contraction by the compiler; fma() where the definition says fma). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

double llr_fma(double a, double b, double c) { return fma(a, b, c); }

/* the library's log with a fixed operation order (csrc/ekf_device.hpp, epi_log), restated */
double llr_log(double x)
{
    if (x != x) return x;
    if (x < 0.0) return NAN;
    if (x == 0.0) return -INFINITY;
    if (x == INFINITY) return x;
    int e;
    double m = frexp(x, &e);
    if (m < 0.70710678118654752440) { m = m + m; e = e - 1; }
    const double f = m - 1.0, k = (double)e;
    const double s = f / (2.0 + f);
    const double z = s * s, w = z * z;
    const double t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01));
    const double t2 = z * (6.666666666666735130e-01 + w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)));
    const double R = t2 + t1;
    const double hfsq = 0.5 * f * f;
    return k * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + k * 1.90821492927058770002e-10)) - f);
}

static int finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }

/* sum of the newest L samples of h[0..k], newest first; samples before the start count as 0.0 (the filter's zero-filled windows) */
static double window_sum(const double *h, int k, int L)
{
    double s = h[k];
    for (int j = 1; j < L; j++) s = s + (k - j >= 0 ? h[k - j] : 0.0);
    return s;
}

/* m: states; flip: a *_BWD model; generic: not a NewCase model; newcases: the resolved observation type is NEWCASES.
 * gamma, beta [B]; PCt [T][3][B] (P- C' of the valid days, by day, for the gain identity; NaN elsewhere) may be NULL, like every output */
void llr_run(int m, int flip, int generic, int newcases, int B, int T, int L, int Sx, int r_mode, int k0, int k1, int rounded,
             const double *S_MINUS, const double *P_MINUS, const double *innov, const double *x, const double *R_series,
             const double *R_scalar, const int32_t *x_series, const double *gamma, const double *beta,
             double *loglik, double *nis_mean, int32_t *n_valid, int32_t *status, double *S_out, double *nis, double *R_used, double *PCt)
{
    double *he = malloc(sizeof(double) * (size_t)T), *hc = malloc(sizeof(double) * (size_t)T);
    for (int c = 0; c < B; c++) {
        const int sx = x_series ? x_series[c] : c;
        double Rnext = r_mode ? 0.0 : R_scalar[c];
        double tot_t = 0.0, tot_q = 0.0, blk_t = 0.0, blk_q = 0.0;
        int tot_n = 0, blk_n = 0, bad = 0;
        for (int k = 0; k < T; k++) {
            const int t = flip ? T - 1 - k : k;
            const size_t o = (size_t)t * B + c;
            const double xk = x[(size_t)t * Sx + sx];
            const int observed = !(xk != xk);
            const double Rk = r_mode ? R_series[(size_t)k * Sx + sx] : Rnext;
            if (R_used) R_used[o] = Rk;
            if (!r_mode) {                                   /* GenericExtendedKalmanFilter.m:172-185, NewCase...m:111 */
                const int cnt = k + 1 < L ? k + 1 : L;
                he[k] = innov[o];
                const double mu = window_sum(he, k, L) / (double)cnt;
                hc[k] = (he[k] - mu) * (he[k] - mu);
                if (generic) {
                    if (beta[c] != 1.0 && observed && k < T - 1) Rnext = beta[c] * Rk + (1.0 - beta[c]) * (window_sum(hc, k, L) / (double)cnt);
                    else Rnext = R_scalar[c];
                } else if (beta[c] != 1.0 && observed) {
                    Rnext = beta[c] * Rk + (1.0 - beta[c]) * window_sum(hc, k, L) / (double)cnt;
                }
            }
            if (k % 32 == 0) { blk_t = 0.0; blk_q = 0.0; blk_n = 0; }
            double S = NAN, q = NAN, pct[3] = {NAN, NAN, NAN};
            if (observed && k >= k0 && k < k1) {
                const double *s = S_MINUS + (size_t)t * m * B + c, *P = P_MINUS + (size_t)t * m * m * B + c;
                double C[3];
                if (newcases) { C[0] = s[(size_t)B] * s[(size_t)2 * B]; C[1] = s[0] * s[(size_t)2 * B]; C[2] = s[0] * s[(size_t)B]; }
                else { C[0] = -1.0; C[1] = 0.0; C[2] = 0.0; }
#define PE(i, j) P[(size_t)((i) + m * (j)) * B]
                double CP[3];
                for (int i = 0; i < 3; i++) pct[i] = fma(PE(i, 2), C[2], fma(PE(i, 1), C[1], PE(i, 0) * C[0]));
                for (int j = 0; j < 3; j++) CP[j] = fma(C[2], PE(2, j), fma(C[1], PE(1, j), C[0] * PE(0, j)));
#undef PE
                const double CPCt = fma(CP[2], C[2], fma(CP[1], C[1], CP[0] * C[0]));
                S = CPCt + gamma[c] * Rk;
                const double e = innov[o];
                if (finite_d(S) && S >= 2.2250738585072014e-308 && finite_d(e)) {
                    q = e * e / S;
                    blk_t = blk_t + (llr_log(S) + q);
                    blk_q = blk_q + q;
                    blk_n = blk_n + 1;
                } else {
                    bad = 1;
                }
            }
            if (S_out) S_out[o] = S;
            if (nis) nis[o] = q;
            if (PCt) for (int i = 0; i < 3; i++) PCt[((size_t)t * 3 + i) * B + c] = pct[i];
            if (k % 32 == 31 || k == T - 1) { tot_t = tot_t + blk_t; tot_q = tot_q + blk_q; tot_n = tot_n + blk_n; }
        }
        if (loglik) loglik[c] = -0.5 * (tot_t + (double)tot_n * 1.8378770664093453);
        if (nis_mean) nis_mean[c] = tot_q / (double)tot_n;
        if (n_valid) n_valid[c] = tot_n;
        if (status) status[c] = bad | ((rounded && !r_mode && beta[c] != 1.0) ? 4 : 0);
    }
    free(he);
    free(hc);
}

/* best [R], best_loglik [R] of R regions x G candidates, region-major */
void llr_select(int R, int G, const double *loglik, const int32_t *n_valid, const int32_t *status, int32_t *best, double *best_loglik)
{
    for (int r = 0; r < R; r++) {
        int b = -1;
        double v = NAN;
        for (int g = 0; g < G; g++) {
            const int c = r * G + g;
            if ((status[c] & 1) || n_valid[c] <= 0) continue;
            if (b < 0 || loglik[c] > v) { b = g; v = loglik[c]; }
        }
        best[r] = b;
        best_loglik[r] = v;
    }
}

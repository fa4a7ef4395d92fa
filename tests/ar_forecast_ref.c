/* Independent C restatement of DESIGN.md section 4.8 (the autoregressive alpha forecaster), the bit-exact yardstick of
 * csrc/ar_forecast.hpp.  Built by the tests with gcc -O2 -ffp-contract=off: every operation below is one IEEE double
 * operation, and fma() is the one fused operation the design names.  Plain serial C: no lanes, no LDS. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define ARF_OK 0
#define ARF_RANK_DEFICIENT 1
#define ARF_BAD_INPUT 2

/* the pinned sum of section 4.8: term(i) for rows i = first .. count-1; chain i mod 64 accumulates its rows in ascending
 * order with fma from +0.0; the 64 chains are then combined at distances 32, 16, .. 1: c[l] = c[l] + c[l ^ h] */
static double combine(double *c)
{
    double n[64];
    for (int h = 32; h >= 1; h >>= 1) {
        for (int l = 0; l < 64; l++) n[l] = c[l] + c[l ^ h];
        memcpy(c, n, sizeof n);
    }
    return c[0];
}

static double pinned_dot(const double *u, const double *v, int first, int count)
{
    double c[64];
    for (int l = 0; l < 64; l++) c[l] = 0.0;
    for (int i = first; i < count; i++) c[i & 63] = fma(u[i], v[i], c[i & 63]);
    return combine(c);
}

static int all_finite(const double *y, int L)
{
    for (int t = 0; t < L; t++)
        if (!isfinite(y[t])) return 0;
    return 1;
}

/* one region: y [L] -> a [p] (a_1 .. a_p), *nv; returns the status.  On a status other than ARF_OK a and *nv are NaN. */
int arf_fit(const double *y, int L, int p, int nv_mode, double *a, double *nv)
{
    const int n = L - p, M = 2 * n;
    for (int k = 0; k < p; k++) a[k] = NAN;
    *nv = NAN;
    if (!all_finite(y, L)) return ARF_BAD_INPUT;
    /* columns 0 .. p-1 = the regressors of a_1 .. a_p, column p = the left-hand sides; col[c] has M rows */
    double **col = (double **)malloc((size_t)(p + 1) * sizeof *col);
    for (int c = 0; c <= p; c++) col[c] = (double *)malloc((size_t)M * sizeof(double));
    for (int t = p; t < L; t++) {                      /* 0-based t: forward row t - p, backward row n + t - p */
        for (int k = 1; k <= p; k++) {
            col[k - 1][t - p] = y[t - k];
            col[k - 1][n + t - p] = y[t - p + k];
        }
        col[p][t - p] = y[t];
        col[p][n + t - p] = y[t - p];
    }
    double big = 0.0;
    for (int c = 0; c < p; c++) big = fmax(big, sqrt(pinned_dot(col[c], col[c], 0, M)));
    const double tol = ((double)(M > p ? M : p) * 2.220446049250313e-16) * big;
    double rdiag[32];
    int status = ARF_OK;
    for (int j = 0; j < p && status == ARF_OK; j++) {
        const double norm = sqrt(pinned_dot(col[j], col[j], j, M));
        if (!(norm > tol)) { status = ARF_RANK_DEFICIENT; break; }
        const double xjj = col[j][j];
        rdiag[j] = xjj >= 0.0 ? -norm : norm;
        const double dd = norm * (norm + fabs(xjj));
        col[j][j] = xjj - rdiag[j];                    /* the reflector v, rows j .. M-1 of column j */
        for (int c = j + 1; c <= p; c++) {
            const double f = pinned_dot(col[j], col[c], j, M) / dd;
            for (int i = j; i < M; i++) col[c][i] = col[c][i] - f * col[j][i];
        }
    }
    if (status == ARF_OK) {
        for (int j = p - 1; j >= 0; j--) {
            double s = -col[p][j];
            for (int k = j + 1; k < p; k++) s = s - col[k][j] * a[k];
            a[j] = s / rdiag[j];
        }
        double cf[64], cb[64];
        for (int l = 0; l < 64; l++) cf[l] = cb[l] = 0.0;
        for (int i = 0; i < n; i++) {
            const int t = p + i;
            double ef = y[t], eb = y[i];
            for (int k = 1; k <= p; k++) {
                ef = fma(a[k - 1], y[t - k], ef);
                eb = fma(a[k - 1], y[i + k], eb);
            }
            cf[i & 63] = fma(ef, ef, cf[i & 63]);
            cb[i & 63] = fma(eb, eb, cb[i & 63]);
        }
        const double frss = combine(cf), brss = combine(cb);
        *nv = nv_mode == 0 ? (frss + brss) / (double)(2 * n) : frss / (double)n;
    }
    for (int c = 0; c <= p; c++) free(col[c]);
    free(col);
    return status;
}

/* one chain: y [L], a [p], nv, z [H] or NULL, drive [H] or NULL -> S [K][3] (s, i, alpha_hat), K = L + H */
void arf_chain(const double *y, int L, int p, int H, const double *a, double nv, double beta, double s0, double i0, double dt,
               const double *z, const double *drive, double *S)
{
    const int K = L + H;
    const int bad = !all_finite(y, L);
    int dead = bad;
    const double b0 = sqrt(nv);
    if (!isfinite(b0)) dead = 1;
    for (int k = 0; k < p; k++)
        if (!isfinite(a[k])) dead = 1;
    double *w = (double *)malloc((size_t)K * sizeof(double));      /* the unclamped series: seg, then the recursion */
    double *al = (double *)malloc((size_t)K * sizeof(double));
    memcpy(w, y, (size_t)L * sizeof(double));
    for (int t = 0; t < H; t++) {
        double acc = b0 * (z ? z[t] : 0.0);
        for (int k = 1; k <= p; k++) acc = fma(-a[k - 1], w[L + t - k], acc);
        w[L + t] = acc;
    }
    for (int t = 0; t < K; t++) {
        double v = w[t];
        if (t >= L && drive) v = v + drive[t - L];
        al[t] = v < 0.0 ? 0.0 : v;                                 /* AlphaHatARX(AlphaHatARX < 0) = 0 */
    }
    double s = s0, i = i0;
    for (int t = 0; t < K; t++) {
        const int nan_day = bad || (dead && t >= L);
        S[3 * t + 0] = nan_day ? NAN : s;
        S[3 * t + 1] = nan_day ? NAN : i;
        S[3 * t + 2] = nan_day ? NAN : al[t];
        if (t < K - 1) {                                           /* Tools/SI_Controlled.m:20-21 */
            const double sn = fmax(0.0, fmin(1.0, s - dt * al[t] * s * i));
            const double in = fmax(0.0, fmin(1.0, i + dt * (al[t] * s * i - beta * i)));
            s = sn; i = in;
        }
    }
    free(w);
    free(al);
}

/* the whole batch in the library's layouts: seg [L][R], beta / s0 / i0 [R], z [H][B] or NULL, drive [H][Sd] or NULL,
 * series [B] or NULL, A_in [p][R] / nv_in [R] (fit = 0) -> S [K][3][B], A_out [p][R], nv_out [R], status [R] */
void arf_run(const double *seg, const double *beta, const double *s0, const double *i0, const double *z, const double *drive,
             const int32_t *series, const double *A_in, const double *nv_in, int R, int D, int L, int p, int H, int Sd, int fit,
             int nv_mode, double dt, double *S, double *A_out, double *nv_out, int32_t *status)
{
    const size_t B = (size_t)R * (size_t)D, K = (size_t)L + (size_t)H;
    double *y = (double *)malloc((size_t)L * sizeof(double)), *zc = (double *)malloc((size_t)H * sizeof(double));
    double *dc = (double *)malloc((size_t)H * sizeof(double)), *Sc = (double *)malloc(K * 3 * sizeof(double));
    double a[32], nv;
    for (int r = 0; r < R; r++) {
        for (int t = 0; t < L; t++) y[t] = seg[(size_t)t * R + r];
        int st;
        if (fit) {
            st = arf_fit(y, L, p, nv_mode, a, &nv);
        } else {
            for (int k = 0; k < p; k++) a[k] = A_in[(size_t)k * R + r];
            nv = nv_in[r];
            st = all_finite(y, L) ? ARF_OK : ARF_BAD_INPUT;
        }
        for (int k = 0; k < p; k++) A_out[(size_t)k * R + r] = a[k];
        nv_out[r] = nv;
        status[r] = st;
        for (int d = 0; d < D; d++) {
            const size_t c = (size_t)r * D + d;
            if (z) for (int t = 0; t < H; t++) zc[t] = z[(size_t)t * B + c];
            if (drive) {
                const size_t ser = series ? (size_t)series[c] : c;
                for (int t = 0; t < H; t++) dc[t] = drive[(size_t)t * Sd + ser];
            }
            arf_chain(y, L, p, H, a, nv, beta[r], s0[r], i0[r], dt, z ? zc : NULL, drive ? dc : NULL, Sc);
            for (size_t t = 0; t < K; t++)
                for (int j = 0; j < 3; j++) S[(t * 3 + j) * B + c] = Sc[3 * t + j];
        }
    }
    free(y); free(zc); free(dc); free(Sc);
}

/* The probabilistic forecast scores of epi_escore_run_* (include/epiekf.h) as a sequential C restatement: one
 * IEEE double operation per written operation (built with -ffp-contract=off), in the order the definition gives.  q_lo, q_hi are
 * handed in: they are formed once by the caller, as the library forms them.  Driven by tests/escore_ref.py (EscoreC). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

static int cmp_double(const void *a, const void *b)
{
    const double x = *(const double *)a, y = *(const double *)b;
    return (x > y) - (x < y);
}

/* the quantile of epi_ens_run_* on the ascending x[0 .. n-1], n >= 1 */
static double quantile(const double *x, int n, double p)
{
    const double h = (double)n * p + 0.5;
    const double kf = floor(h), g = h - kf;
    if (kf < 1.0) return x[0];
    if (kf >= (double)n) return x[n - 1];
    const int k = (int)kf;
    return x[k - 1] + g * (x[k] - x[k - 1]);
}

/* the pairwise sum over P positions, P a power of two: a[i] = a[i] + a[i + h], h = P/2 .. 1 */
static double tree(double *a, int P)
{
    for (int h = P / 2; h >= 1; h /= 2)
        for (int i = 0; i < h; i++) a[i] = a[i] + a[i + h];
    return a[0];
}

static double pos(double d) { return d > 0.0 ? d : 0.0; }

void escore_ref(int T, int rows, int R, int D, int Rt, int n_a, int n_bins, int f32, int derive, int k0, int k1, const void *src,
                const double *population, const double *truth, const int32_t *truth_series, const int32_t *first_day,
                const double *alpha, const double *q_lo, const double *q_hi, double *crps, double *wis, double *ae, double *width,
                int32_t *rank, int32_t *ties, int32_t *cover, int32_t *count, double *crps_mean, double *wis_mean, double *ae_mean,
                int32_t *n_scored, double *cover_frac, int32_t *pit_hist)
{
    const int ro = rows + derive;
    const size_t B = (size_t)R * (size_t)D, plane = (size_t)ro * (size_t)R;
    int P = 64;
    while (P < D) P *= 2;
    double *x = malloc(sizeof(double) * (size_t)P), *term = malloc(sizeof(double) * (size_t)P);
#define SRC(o) (f32 ? (double)((const float *)src)[o] : ((const double *)src)[o])
    for (int t = 0; t < T; t++)
        for (int row = 0; row < ro; row++)
            for (int r = 0; r < R; r++) {
                const size_t oo = (size_t)t * plane + (size_t)row * (size_t)R + (size_t)r;
                const int ts = truth_series ? truth_series[r] : r;
                const double y = truth[((size_t)t * (size_t)ro + (size_t)row) * (size_t)Rt + (size_t)ts];
                int n = 0, rk = 0, ti = 0;
                for (int e = 0; e < D; e++) {
                    double v;
                    if (row < rows) {
                        v = SRC(((size_t)t * (size_t)rows + (size_t)row) * B + (size_t)r * (size_t)D + (size_t)e);
                    } else {
                        const size_t o = (size_t)t * (size_t)rows * B + (size_t)r * (size_t)D + (size_t)e;
                        v = ((population[r] * SRC(o)) * SRC(o + B)) * SRC(o + 2 * B);
                    }
                    if (v == v) x[n++] = v;
                    rk += v < y;
                    ti += v == y;
                }
                count[oo] = n;
                if (n == 0 || y != y) {
                    rank[oo] = ties[oo] = -1;
                    cover[oo] = 0;
                    crps[oo] = wis[oo] = ae[oo] = NAN;
                    for (int k = 0; k < n_a; k++) width[((size_t)t * (size_t)n_a + (size_t)k) * plane + (size_t)row * (size_t)R + (size_t)r] = NAN;
                    continue;
                }
                rank[oo] = rk;
                ties[oo] = ti;
                qsort(x, (size_t)n, sizeof(double), cmp_double);
                const double med = quantile(x, n, 0.5);
                const double a_e = fabs(y - med);
                double acc = 0.5 * a_e;
                int cv = 0;
                for (int k = 0; k < n_a; k++) {
                    const double l = quantile(x, n, q_lo[k]), u = quantile(x, n, q_hi[k]);
                    const double wd = u - l, c = 2.0 / alpha[k];
                    const double is = (wd + c * pos(l - y)) + c * pos(y - u);
                    acc = acc + (alpha[k] / 2.0) * is;
                    if (l <= y && y <= u) cv |= 1 << k;
                    width[((size_t)t * (size_t)n_a + (size_t)k) * plane + (size_t)row * (size_t)R + (size_t)r] = wd;
                }
                ae[oo] = a_e;
                wis[oo] = acc / ((double)n_a + 0.5);
                cover[oo] = cv;
                const double nd = (double)n;
                for (int e = 0; e < P; e++) {
                    const double coef = e < n ? ((y < x[e] ? nd : 0.0) - (double)(e + 1)) + 0.5 : 0.0;
                    term[e] = e < n ? (x[e] - y) * coef : 0.0;
                }
                crps[oo] = (2.0 / (nd * nd)) * tree(term, P);
            }
#undef SRC
    for (int row = 0; row < ro; row++)
        for (int r = 0; r < R; r++) {
            const size_t col = (size_t)row * (size_t)R + (size_t)r;
            const int fd = first_day ? first_day[r] : 0;
            double sc = 0.0, sw = 0.0, sa = 0.0;
            int ns = 0, cov[8] = {0};
            for (int b = 0; b < n_bins; b++) pit_hist[(size_t)b * plane + col] = 0;
            for (int t = k0; t < k1; t++) {
                const size_t o = (size_t)t * plane + col;
                if (t < fd || rank[o] < 0) continue;
                ns++;
                sc = sc + crps[o];
                sw = sw + wis[o];
                sa = sa + ae[o];
                for (int k = 0; k < n_a; k++) cov[k] += (cover[o] >> k) & 1;
                if (n_bins) {
                    int64_t b = ((2 * (int64_t)rank[o] + ties[o] + 1) * n_bins) / (2 * ((int64_t)count[o] + 1));
                    if (b > n_bins - 1) b = n_bins - 1;
                    pit_hist[(size_t)b * plane + col] += 1;
                }
            }
            n_scored[col] = ns;
            crps_mean[col] = ns ? sc / (double)ns : NAN;
            wis_mean[col] = ns ? sw / (double)ns : NAN;
            ae_mean[col] = ns ? sa / (double)ns : NAN;
            for (int k = 0; k < n_a; k++) cover_frac[(size_t)k * plane + col] = ns ? (double)cov[k] / (double)ns : NAN;
        }
    free(x);
    free(term);
}

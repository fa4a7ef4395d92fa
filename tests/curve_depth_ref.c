/* Sequential C restatement of the curve statistics (include/epiekf_cdepth.h): one (row, region) after the other,
 * every count by comparing every pair of members, one double operation per written operation (built with -ffp-contract=off).
 * Driven by tests/curve_depth_ref.py.  Every output array is written; without alpha / with fence_factor = 0 the envelopes / the
 * boxplot's outputs hold NaN and 0. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

static double value(const void *src, int f32, size_t o)
{
    return f32 ? (double)((const float *)src)[o] : ((const double *)src)[o];
}

/* of zeros of both signs the min is -0.0 and the max +0.0 */
static double min2(double x, double y) { return y < x || (y == x && signbit(y)) ? y : x; }
static double max2(double x, double y) { return y > x || (y == x && !signbit(y)) ? y : x; }

static int deepest(double f, int n)
{
    int m = (int)ceil(f * (double)n);
    if (m < 1) m = 1;
    return m < n ? m : n;
}

static int64_t choose2(int64_t n) { return n * (n - 1) / 2; }

/* min / max over the members d with keep[d] that are not NaN on the day v[0 .. D); returns whether there is one */
static int envelope(const double *v, const char *keep, int D, double *lo, double *hi)
{
    int any = 0;
    for (int d = 0; d < D; d++) {
        if (!keep[d] || isnan(v[d])) continue;
        *lo = any ? min2(*lo, v[d]) : v[d];
        *hi = any ? max2(*hi, v[d]) : v[d];
        any = 1;
    }
    return any;
}

int cdepth_ref(int T, int rows, int R, int D, int n_alpha, int f32, int derive, int k0, int k1, const void *src, const double *population,
               const int32_t *first_day, const double *alpha, double fence_factor, double fence_frac, double *depth, double *mhi,
               double *band_count, double *pair_total, int32_t *n_valid, int32_t *depth_rank, int32_t *out_days, int32_t *n_ranked,
               int32_t *median_path, int32_t *n_outliers, double *env_lo, double *env_hi, double *median_curve, double *whisk_lo,
               double *whisk_hi)
{
    const size_t N = (size_t)R * (size_t)D, ro = (size_t)(rows + derive), plane = ro * (size_t)R;
    double *v = (double *)malloc((size_t)T * (size_t)D * sizeof(double));
    double *flo = (double *)malloc((size_t)T * sizeof(double)), *fhi = (double *)malloc((size_t)T * sizeof(double));
    int64_t *acc = (int64_t *)malloc((size_t)D * 4 * sizeof(int64_t));
    char *keep = (char *)malloc((size_t)D);
    if (!v || !flo || !fhi || !acc || !keep) return 1;
    for (size_t q = 0; q < ro; q++)
        for (size_t r = 0; r < (size_t)R; r++) {
            const size_t base = q * N + r * (size_t)D, col = q * (size_t)R + r;
            int lo = first_day ? first_day[r] : 0;
            if (lo < k0) lo = k0;
            for (int t = 0; t < T; t++)
                for (int d = 0; d < D; d++) {
                    const size_t p = r * (size_t)D + (size_t)d;
                    double x;
                    if (q < (size_t)rows) {
                        x = value(src, f32, ((size_t)t * (size_t)rows + q) * N + p);
                    } else {
                        const size_t o = (size_t)t * (size_t)rows * N + p;
                        x = population[r] * value(src, f32, o);
                        x = x * value(src, f32, o + N);
                        x = x * value(src, f32, o + 2 * N);
                    }
                    v[(size_t)t * (size_t)D + (size_t)d] = x;
                }
            /* ---- depth ---- */
            for (int d = 0; d < D; d++) {
                acc[4 * d] = acc[4 * d + 1] = acc[4 * d + 2] = acc[4 * d + 3] = 0;
                n_valid[base + (size_t)d] = 0;
            }
            for (int t = lo; t < k1; t++) {
                const double *x = v + (size_t)t * (size_t)D;
                int64_t n = 0;
                for (int e = 0; e < D; e++) n += !isnan(x[e]);
                for (int d = 0; d < D; d++) {
                    if (isnan(x[d])) continue;
                    int64_t below = 0, above = 0;
                    for (int e = 0; e < D; e++) {
                        if (isnan(x[e])) continue;
                        below += x[e] < x[d];
                        above += x[e] > x[d];
                    }
                    acc[4 * d] += choose2(n) - choose2(below) - choose2(above);
                    acc[4 * d + 1] += choose2(n);
                    acc[4 * d + 2] += n - above;
                    acc[4 * d + 3] += n;
                    n_valid[base + (size_t)d]++;
                }
            }
            for (int d = 0; d < D; d++) {
                const size_t m = base + (size_t)d;
                band_count[m] = (double)acc[4 * d];
                pair_total[m] = (double)acc[4 * d + 1];
                depth[m] = acc[4 * d + 1] ? (double)acc[4 * d] / (double)acc[4 * d + 1] : NAN;
                mhi[m] = n_valid[m] ? (double)acc[4 * d + 2] / (double)acc[4 * d + 3] : NAN;
            }
            /* ---- ranks ---- */
            int nr = 0, mp = -1;
            for (int d = 0; d < D; d++) {
                const double x = depth[base + (size_t)d];
                int rank = 0;
                if (isnan(x)) {
                    rank = -1;
                } else {
                    nr++;
                    for (int e = 0; e < D; e++) {
                        const double y = depth[base + (size_t)e];
                        rank += y > x || (e < d && y == x);
                    }
                    if (rank == 0) mp = d;
                }
                depth_rank[base + (size_t)d] = rank;
            }
            n_ranked[col] = nr;
            median_path[col] = mp;
            /* ---- central regions and the deepest curve ---- */
            for (int t = 0; t < T; t++) {
                const double *x = v + (size_t)t * (size_t)D;
                const int in = t >= lo && t < k1;
                for (int k = 0; k < n_alpha; k++) {
                    const int mk = deepest(alpha[k], nr);
                    double l = NAN, h = NAN;
                    for (int d = 0; d < D; d++) keep[d] = depth_rank[base + (size_t)d] >= 0 && depth_rank[base + (size_t)d] < mk;
                    if (!(in && envelope(x, keep, D, &l, &h))) l = h = NAN;
                    env_lo[((size_t)t * (size_t)n_alpha + (size_t)k) * plane + col] = l;
                    env_hi[((size_t)t * (size_t)n_alpha + (size_t)k) * plane + col] = h;
                }
                median_curve[(size_t)t * plane + col] = in && mp >= 0 ? x[mp] : NAN;
                flo[t] = fhi[t] = NAN;
                if (fence_factor > 0.0 && in) {
                    const int mf = deepest(fence_frac, nr);
                    for (int d = 0; d < D; d++) keep[d] = depth_rank[base + (size_t)d] >= 0 && depth_rank[base + (size_t)d] < mf;
                    if (!envelope(x, keep, D, &flo[t], &fhi[t])) flo[t] = fhi[t] = NAN;
                }
            }
            /* ---- the functional boxplot ---- */
            int nout = 0;
            for (int d = 0; d < D; d++) {
                int out = 0;
                if (fence_factor > 0.0)
                    for (int t = lo; t < k1; t++) {
                        const double x = v[(size_t)t * (size_t)D + (size_t)d];
                        const double w = fhi[t] - flo[t];
                        const double fw = fence_factor * w;
                        const double lo_f = flo[t] - fw, hi_f = fhi[t] + fw;
                        out += !isnan(x) && (x < lo_f || x > hi_f);
                    }
                out_days[base + (size_t)d] = out;
                nout += depth_rank[base + (size_t)d] >= 0 && out > 0;
                keep[d] = depth_rank[base + (size_t)d] >= 0 && out == 0;
            }
            n_outliers[col] = nout;
            for (int t = 0; t < T; t++) {
                double l = NAN, h = NAN;
                if (!(fence_factor > 0.0 && t >= lo && t < k1 && envelope(v + (size_t)t * (size_t)D, keep, D, &l, &h))) l = h = NAN;
                whisk_lo[(size_t)t * plane + col] = l;
                whisk_hi[(size_t)t * plane + col] = h;
            }
        }
    free(v); free(flo); free(fhi); free(acc); free(keep);
    return 0;
}

/* Sequential C restatement of the path functionals (include/epiekf.h): one path and row after the other, its
 * days ascending, one double operation per written operation (built with -ffp-contract=off).  Driven by tests/pathfn_ref.py. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

static double value(const void *src, int f32, size_t o)
{
    return f32 ? (double)((const float *)src)[o] : ((const double *)src)[o];
}

void pathfn_ref(int T, int rows, int R, int D, int n_thr, int f32, int derive, int k0, int k1, const void *src, const double *population,
                const double *thr, const int32_t *first_day, double *peak_value, double *peak_day, double *min_value, double *min_day,
                double *total, double *first_cross, double *days_above, double *longest_run, int32_t *n_valid, int32_t *n_paths,
                int32_t *peak_day_hist, int32_t *n_cross, int32_t *cross_day_hist)
{
    const size_t N = (size_t)R * (size_t)D, ro = (size_t)(rows + derive), M = ro * N, plane = ro * (size_t)R;
    const int W = k1 - k0;
    (void)T;
    for (size_t i = 0; i < plane; i++) n_paths[i] = 0;
    for (size_t i = 0; i < (size_t)W * plane; i++) peak_day_hist[i] = 0;
    for (size_t i = 0; i < (size_t)n_thr * plane; i++) n_cross[i] = 0;
    for (size_t i = 0; i < (size_t)W * (size_t)n_thr * plane; i++) cross_day_hist[i] = 0;
    for (size_t q = 0; q < ro; q++)
        for (size_t p = 0; p < N; p++) {
            const size_t r = p / (size_t)D, m = q * N + p, col = q * (size_t)R + r;
            int lo = first_day ? first_day[r] : 0;
            if (lo < k0) lo = k0;
            double mx = 0.0, mn = 0.0, tot = 0.0;
            int mxd = -1, mnd = -1, nv = 0;
            int first[8], cnt[8], cur[8], best[8];
            for (int j = 0; j < n_thr; j++) { first[j] = -1; cnt[j] = cur[j] = best[j] = 0; }
            for (int tb = k0; tb < k1; tb += 32) {
                double bs = 0.0;
                for (int t = tb; t < tb + 32 && t < k1; t++) {
                    double v;
                    if (q < (size_t)rows) {
                        v = value(src, f32, ((size_t)t * (size_t)rows + q) * N + p);
                    } else {
                        const size_t o = (size_t)t * (size_t)rows * N + p;
                        v = population[r] * value(src, f32, o);
                        v = v * value(src, f32, o + N);
                        v = v * value(src, f32, o + 2 * N);
                    }
                    const int ok = t >= lo && !isnan(v);
                    if (ok) {
                        if (nv == 0 || v > mx) { mx = v; mxd = t; }
                        if (nv == 0 || v < mn) { mn = v; mnd = t; }
                        nv++;
                        bs = bs + v;
                    }
                    for (int j = 0; j < n_thr; j++) {
                        if (ok && v >= thr[((size_t)j * ro + q) * (size_t)R + r]) {
                            if (first[j] < 0) first[j] = t;
                            cnt[j]++;
                            cur[j]++;
                            if (cur[j] > best[j]) best[j] = cur[j];
                        } else {
                            cur[j] = 0;
                        }
                    }
                }
                tot = tot + bs;
            }
            n_valid[m] = nv;
            peak_value[m] = nv ? mx : NAN;
            peak_day[m] = nv ? (double)mxd : NAN;
            min_value[m] = nv ? mn : NAN;
            min_day[m] = nv ? (double)mnd : NAN;
            total[m] = nv ? tot : NAN;
            if (nv) {
                n_paths[col]++;
                peak_day_hist[(size_t)(mxd - k0) * plane + col]++;
            }
            for (int j = 0; j < n_thr; j++) {
                const size_t mj = (size_t)j * M + m;
                const int asked = nv && !isnan(thr[((size_t)j * ro + q) * (size_t)R + r]);
                first_cross[mj] = asked && first[j] >= 0 ? (double)first[j] : NAN;
                days_above[mj] = asked ? (double)cnt[j] : NAN;
                longest_run[mj] = asked ? (double)best[j] : NAN;
                if (asked && first[j] >= 0) {
                    n_cross[(size_t)j * plane + col]++;
                    cross_day_hist[((size_t)(first[j] - k0) * (size_t)n_thr + (size_t)j) * plane + col]++;
                }
            }
        }
}

/* The joint scores of epi_ejoint_run_* (include/epiekf.h) as a sequential C restatement: one IEEE double
 * operation per written operation (built with -ffp-contract=off), in the order the definition gives.  Driven by
 * tests/ejoint_ref.py (EjointC) and linked into tests/ejoint_emu.cpp's program. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

/* the pairwise sum over P positions, P a power of two: a[i] = a[i] + a[i + h], h = P/2 .. 1 */
static double tree(double *a, int P)
{
    for (int h = P / 2; h >= 1; h /= 2)
        for (int i = 0; i < h; i++) a[i] = a[i] + a[i + h];
    return a[0];
}

static double gfun(double a, int vs_order) { return vs_order == 1 ? sqrt(fabs(a)) : fabs(a); }

void ejoint_ref(int T, int rows, int R, int D, int Rt, int f32, int derive, int k0, int k1, int vs_order, int max_lag, const void *src,
                const double *population, const double *truth, const int32_t *truth_series, const int32_t *first_day, double *es,
                double *truth_term, double *spread_term, double *vs, int32_t *n_members, int32_t *n_days, double *member_dist)
{
    const int ro = rows + derive, nb = (D + 63) / 64, wcap = k1 - k0;
    const size_t B = (size_t)R * (size_t)D;
    int P = 64;
    while (P < D) P *= 2;
    (void)T;
    double *x = malloc(sizeof(double) * (size_t)(wcap > 0 ? wcap : 1) * (size_t)D), *y = malloc(sizeof(double) * (size_t)(wcap > 0 ? wcap : 1));
    double *a = malloc(sizeof(double) * (size_t)P);
    int *days = malloc(sizeof(int) * (size_t)(wcap > 0 ? wcap : 1)), *ok = malloc(sizeof(int) * (size_t)nb * 64);
#define SRC(o) (f32 ? (double)((const float *)src)[o] : ((const double *)src)[o])
#define X(w, e) x[(size_t)(w) * (size_t)D + (size_t)(e)]
    for (int row = 0; row < ro; row++)
        for (int r = 0; r < R; r++) {
            const size_t col = (size_t)row * (size_t)R + (size_t)r;
            const int ts = truth_series ? truth_series[r] : r, fd = first_day ? first_day[r] : 0;
            int W = 0;
            for (int t = k0 > fd ? k0 : fd; t < k1; t++) {
                const double yt = truth[((size_t)t * (size_t)ro + (size_t)row) * (size_t)Rt + (size_t)ts];
                if (yt != yt) continue;
                for (int e = 0; e < D; e++) {
                    if (row < rows) {
                        X(W, e) = SRC(((size_t)t * (size_t)rows + (size_t)row) * B + (size_t)r * (size_t)D + (size_t)e);
                    } else {
                        const size_t o = (size_t)t * (size_t)rows * B + (size_t)r * (size_t)D + (size_t)e;
                        X(W, e) = ((population[r] * SRC(o)) * SRC(o + B)) * SRC(o + 2 * B);
                    }
                }
                y[W] = yt;
                days[W++] = t;
            }
            int n = 0;
            for (int e = 0; e < nb * 64; e++) {
                ok[e] = e < D;
                for (int w = 0; w < W && e < D; w++)
                    if (X(w, e) != X(w, e)) ok[e] = 0;
                n += ok[e];
            }
            n_members[col] = n;
            n_days[col] = W;
            if (n == 0 || W == 0) {
                es[col] = truth_term[col] = spread_term[col] = vs[col] = NAN;
                for (int e = 0; e < D; e++) member_dist[col * (size_t)D + (size_t)e] = NAN;
                continue;
            }
            const double nd = (double)n;
            for (int e = 0; e < P; e++) a[e] = 0.0;
            for (int e = 0; e < D; e++) {
                double d2 = 0.0;
                for (int w = 0; w < W; w++) {
                    const double d = X(w, e) - y[w];
                    d2 = d2 + d * d;
                }
                const double ei = sqrt(d2);
                member_dist[col * (size_t)D + (size_t)e] = ok[e] ? ei : NAN;
                a[e] = ok[e] ? ei : 0.0;
            }
            const double tt = tree(a, P);
            truth_term[col] = tt / nd;
            double ps = 0.0;
            for (int I = 0; I < nb; I++)
                for (int J = I; J < nb; J++) {
                    double s[64];
                    for (int i = 0; i < 64; i++) {
                        const int ei = I * 64 + i;
                        s[i] = 0.0;
                        for (int j = 0; j < 64; j++) {
                            const int ej = J * 64 + j;
                            double c = 0.0;
                            if (ok[ei] && ok[ej] && (I != J || j > i)) {
                                double d2 = 0.0;
                                for (int w = 0; w < W; w++) {
                                    const double d = X(w, ei) - X(w, ej);
                                    d2 = d2 + d * d;
                                }
                                c = sqrt(d2);
                            }
                            s[i] = s[i] + c;
                        }
                    }
                    ps = ps + tree(s, 64);
                }
            spread_term[col] = ps / (nd * nd);
            es[col] = truth_term[col] - spread_term[col];
            double v_all = 0.0;
            for (int s = 0; s < W && vs_order; s++) {
                double v = 0.0;
                for (int t = s + 1; t < W; t++) {
                    if (max_lag > 0 && days[t] - days[s] > max_lag) break;
                    for (int e = 0; e < P; e++) a[e] = e < D && ok[e] ? gfun(X(s, e) - X(t, e), vs_order) : 0.0;
                    const double m = tree(a, P) / nd;
                    const double term = gfun(y[s] - y[t], vs_order) - m;
                    v = v + term * term;
                }
                v_all = v_all + v;
            }
            vs[col] = vs_order ? v_all : NAN;
        }
#undef X
#undef SRC
    free(x);
    free(y);
    free(a);
    free(days);
    free(ok);
}

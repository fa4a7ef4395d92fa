/* Plain-C restatement of DESIGN.md §4.10 (the element-wise robust regression), one item after the other: the operation order
 * the kernel (csrc/robust_fit.hpp) and tests/robust_fit_ref.py share bit for bit.  Build: gcc -O2 -ffp-contract=off.
 * Every sum over days is the pairwise tree a[i] += a[i + h], h = P/2 .. 1, over the D terms padded with +0.0 to P, the power
 * of two >= max(D, 64); the median comes from a full ascending sort.  Every output may be NULL. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

enum { NONFINITE = 1, CONST = 2, SLOPE_LOST = 4, MAXITER = 8, BOUND = 16 };
#define MAXP 1024

static double tree(const double *v, int D)
{
    double a[MAXP];
    int P = 64;
    while (P < D) P <<= 1;
    for (int i = 0; i < P; i++) a[i] = i < D ? v[i] : 0.0;
    for (int h = P / 2; h >= 1; h >>= 1)
        for (int i = 0; i < h; i++) a[i] = a[i] + a[i + h];
    return a[0];
}

static int cmp(const void *p, const void *q)
{
    const double u = *(const double *)p, v = *(const double *)q;
    return (u > v) - (u < v);
}

static void wls(const double *x, const double *y, const double *w, int D, int cst, double lower, double upper, double *a, double *b,
                int *flags)
{
    double s[MAXP];
    for (int d = 0; d < D; d++) s[d] = w[d];
    const double sw = tree(s, D);
    for (int d = 0; d < D; d++) s[d] = w[d] * x[d];
    const double mx = tree(s, D) / sw;
    for (int d = 0; d < D; d++) s[d] = w[d] * y[d];
    const double my = tree(s, D) / sw;
    for (int d = 0; d < D; d++) s[d] = (w[d] * (x[d] - mx)) * (x[d] - mx);
    const double sxx = tree(s, D);
    for (int d = 0; d < D; d++) s[d] = (w[d] * (x[d] - mx)) * (y[d] - my);
    const double sxy = tree(s, D);
    for (int d = 0; d < D; d++) s[d] = (w[d] * x[d]) * x[d];
    const double swxx = tree(s, D);
    *flags = 0;
    *a = 0.0;
    if (!cst && sxx > 2.220446049250313e-16 * swxx) {
        const double raw = sxy / sxx;
        double v = raw;
        if (v < lower) v = lower;
        if (v > upper) v = upper;
        if (v != raw) *flags = BOUND;
        *a = v;
    } else if (!cst) {
        *flags = SLOPE_LOST;
    }
    *b = my - *a * mx;
}

/* one item; w [D] receives the final weights */
static void item(const double *x, const double *y, int D, int robust, int max_iter, double lower, double upper, double *a, double *b,
                 double *sigma, int32_t *iters, int32_t *status, double *w)
{
    double s[MAXP], adj[MAXP], radj[MAXP];
    int finite = 1;
    for (int d = 0; d < D; d++) finite = finite && fabs(x[d]) < INFINITY && fabs(y[d]) < INFINITY;
    if (!finite) {
        *a = *b = *sigma = NAN; *iters = 0; *status = NONFINITE;
        for (int d = 0; d < D; d++) w[d] = NAN;
        return;
    }
    double lo = x[0], hi = x[0];
    for (int d = 1; d < D; d++) { if (x[d] < lo) lo = x[d]; if (x[d] > hi) hi = x[d]; }
    const int cst = lo == hi;
    const double Dd = (double)D;
    const double xbar = tree(x, D) / Dd;
    for (int d = 0; d < D; d++) s[d] = (x[d] - xbar) * (x[d] - xbar);
    const double sxx0 = tree(s, D);
    for (int d = 0; d < D; d++) {
        double h = 1.0 / Dd;
        if (!cst) {
            h = 1.0 / Dd + ((x[d] - xbar) * (x[d] - xbar)) / sxx0;
            if (!(h < 0.9999)) h = 0.9999;
        }
        adj[d] = 1.0 / sqrt(1.0 - h);
    }
    const double ybar = tree(y, D) / Dd;
    for (int d = 0; d < D; d++) s[d] = (y[d] - ybar) * (y[d] - ybar);
    double tiny = 1e-6 * sqrt(tree(s, D) / (Dd - 1.0));
    if (tiny == 0.0) tiny = 1.0;
    for (int d = 0; d < D; d++) w[d] = 1.0;
    int flags, cap = 0;
    wls(x, y, w, D, cst, lower, upper, a, b, &flags);
    *sigma = NAN;
    *iters = 0;
    if (robust) {
        const int m = D - 1;
        for (;;) {
            for (int d = 0; d < D; d++) { radj[d] = (y[d] - (*a * x[d] + *b)) * adj[d]; s[d] = fabs(radj[d]); }
            qsort(s, (size_t)D, sizeof(double), cmp);
            const double med = (m & 1) ? s[1 + (m - 1) / 2] : (s[m / 2] + s[m / 2 + 1]) / 2.0;
            const double sg = med / 0.6745;
            *sigma = sg > tiny ? sg : tiny;
            const double den = *sigma * 4.685;
            for (int d = 0; d < D; d++) {
                const double u = radj[d] / den, t = 1.0 - u * u;
                w[d] = fabs(u) < 1.0 ? t * t : 0.0;
            }
            const double a0 = *a, b0 = *b;
            wls(x, y, w, D, cst, lower, upper, a, b, &flags);
            ++*iters;
            const double se = 1.4901161193847656e-08;
            if (fabs(*a - a0) <= se * fmax(fabs(*a), fabs(a0)) && fabs(*b - b0) <= se * fmax(fabs(*b), fabs(b0))) break;
            if (*iters == max_iter) { cap = MAXITER; break; }
        }
    }
    *status = (cst ? CONST : 0) | flags | cap;
}

/* X [D][n][R], y [D][R]; a, b_item, sigma, iters, status [n][R]; weights [D][n][R]; b [R] */
void robfit_run(const double *X, const double *y, int R, int D, int n, int robust, int max_iter, double lower, double upper, double *a,
                double *b_item, double *sigma, int32_t *iters, int32_t *status, double *weights, double *b)
{
    double x[MAXP], yy[MAXP], w[MAXP], s[MAXP], ak[16];
    for (int r = 0; r < R; r++) {
        for (int d = 0; d < D; d++) yy[d] = y[(size_t)d * R + r];
        for (int k = 0; k < n; k++) {
            double bi, sg;
            int32_t it, st;
            for (int d = 0; d < D; d++) x[d] = X[((size_t)d * n + k) * R + r];
            item(x, yy, D, robust, max_iter, lower, upper, &ak[k], &bi, &sg, &it, &st, w);
            const size_t o = (size_t)k * R + r;
            if (a) a[o] = ak[k];
            if (b_item) b_item[o] = bi;
            if (sigma) sigma[o] = sg;
            if (iters) iters[o] = it;
            if (status) status[o] = st;
            if (weights)
                for (int d = 0; d < D; d++) weights[((size_t)d * n + k) * R + r] = w[d];
        }
        if (b) {
            for (int d = 0; d < D; d++) {
                double t = 0.0;
                for (int k = 0; k < n; k++) t = t + X[((size_t)d * n + k) * R + r] * ak[k];
                s[d] = yy[d] - t;
            }
            b[r] = (1.0 / (double)D) * tree(s, D);
        }
    }
}

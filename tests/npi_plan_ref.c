/* Sequential C restatement of the direct optimal-NPI planner (include/epiekf.h, epi_plan_*): the yardstick the
 * kernel csrc/npi_plan.hpp is held to bit for bit.  One chain at a time, plain arrays of one chain ([H][n] plans, [H][3]
 * states), no layout tricks; compiled with -ffp-contract=off so that every written operation rounds once and fma() is the
 * only fused one.  tests/npi_plan_ref.py loads it and restates it once more in NumPy.
 *
 * npr_run      the whole call, arrays laid out as the C ABI's
 * npr_score    F, sum0, sum1 and the states of one given plan of one region (the forward pass alone)
 * npr_fma      fma() for the NumPy reading */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { S0 = 0, I0, AL0, AMIN, AMAX, GAMMA, BB, BETA, S_STD, I_STD, A_STD, DT, ROW_A = 12, ROW_UMAX = 24, ROW_W = 36, ROWS = 48 };

double npr_fma(double a, double b, double c) { return fma(a, b, c); }

typedef struct {
    double s0, i0, al0, amin, amax, gamma, b, beta, s_std, i_std, a_std, dt;
    double ga[12], umax[12], w[12], umin[12];
    int n;
} region_t;

static void load_region(region_t *g, const double *sp, const double *u_min, int R, int r, int n)
{
    const double *col = sp + r;
#define ROW(f) col[(size_t)(f) * R]
    g->s0 = ROW(S0); g->i0 = ROW(I0); g->al0 = ROW(AL0); g->amin = ROW(AMIN); g->amax = ROW(AMAX); g->gamma = ROW(GAMMA);
    g->b = ROW(BB); g->beta = ROW(BETA); g->s_std = ROW(S_STD); g->i_std = ROW(I_STD); g->a_std = ROW(A_STD); g->dt = ROW(DT);
    for (int k = 0; k < 12; k++) {
        g->ga[k] = g->gamma * ROW(ROW_A + k);
        g->umax[k] = ROW(ROW_UMAX + k);
        g->w[k] = ROW(ROW_W + k);
        g->umin[k] = k < n ? u_min[(size_t)k * R + r] : 0.0;
    }
#undef ROW
    g->n = n;
}

/* the forward pass: u [H][n] of one chain -> x [H][3]; sums[0..1] from the first term, sums[2..3] continued from the prefix */
static double forward(const region_t *g, int H, const double *u, double eps, double ome, int pre, double j0p, double j1p, double *x,
                      double *sums)
{
    double s = g->s0, i = g->i0, al = g->al0, acc0 = 0.0, acc1 = 0.0, j0 = j0p, j1 = j1p;
    const int n = g->n;
    for (int t = 0; t < H; t++) {
        double uk[12];
        for (int k = 0; k < 12; k++) uk[k] = k < n ? u[(size_t)t * n + k] : 0.0;
        double dot = g->ga[0] * (g->umax[0] - uk[0]);
        for (int k = 1; k < 12; k++) dot = fma(g->ga[k], g->umax[k] - uk[k], dot);
        const double sn = fmax(0.0, fmin(1.0, s - g->dt * (al * s * i + 0.0 * g->s_std)));
        const double in = fmax(0.0, fmin(1.0, i + g->dt * (al * s * i - g->beta * i + 0.0 * g->i_std)));
        const double an = fmax(g->amin, fmin(g->amax, al + g->dt * (-g->gamma * al + g->gamma * g->b + dot + 0.0 * g->a_std)));
        s = sn; i = in; al = an;
        x[t * 3 + 0] = s; x[t * 3 + 1] = i; x[t * 3 + 2] = al;
        const double nc = s * i * al;
        acc0 = t == 0 ? nc : acc0 + nc;
        if (pre) j0 = j0 + nc;
        for (int k = 0; k < n; k++) {
            const double term = g->w[k] * uk[k];
            acc1 = (t == 0 && k == 0) ? term : acc1 + term;
            if (pre) j1 = j1 + term;
        }
    }
    sums[0] = acc0; sums[1] = acc1; sums[2] = pre ? j0 : acc0; sums[3] = pre ? j1 : acc1;
    return ome * acc0 + eps * acc1;
}

/* the adjoint pass: mu [H][3], g [H][n], up [H][n] (1: the vertex is u_max); returns the gap over the free entries */
static double adjoint(const region_t *q, int H, const double *x, const double *u, const unsigned char *held, double eps, double ome,
                      double *mu, double *grad, unsigned char *up)
{
    const int n = q->n;
    const double dt = q->dt;
    double gap = 0.0, v[3] = {0.0, 0.0, 0.0};
    for (int t = H - 1; t >= 0; t--) {
        const double s = x[t * 3], i = x[t * 3 + 1], al = x[t * 3 + 2];
        double m[3];
        m[0] = ome * (i * al); m[1] = ome * (s * al); m[2] = ome * (s * i);
        if (t < H - 1) {
            double A[3][3];
            A[0][0] = 1.0 - dt * al * i; A[0][1] = -dt * al * s;                 A[0][2] = -dt * s * i;
            A[1][0] = dt * i * al;       A[1][1] = 1.0 + dt * (s * al - q->beta); A[1][2] = dt * s * i;
            A[2][0] = 0.0;               A[2][1] = 0.0;                          A[2][2] = 1.0 - dt * q->gamma;
            const double a0 = fma(A[1][0], v[1], A[0][0] * v[0]);
            const double a1 = fma(A[1][1], v[1], A[0][1] * v[0]);
            const double a2 = fma(A[2][2], v[2], fma(A[1][2], v[1], A[0][2] * v[0]));
            m[0] = m[0] + a0; m[1] = m[1] + a1; m[2] = m[2] + a2;
        }
        const int d0 = 0.0 < s && s < 1.0, d1 = 0.0 < i && i < 1.0, d2 = q->amin < al && al < q->amax;
        mu[t * 3] = m[0]; mu[t * 3 + 1] = m[1]; mu[t * 3 + 2] = m[2];
        for (int k = 0; k < n; k++) {
            const double ew = eps * q->w[k];
            const double g = d2 ? ew - dt * q->ga[k] * m[2] : ew;
            const int hi = !(g > 0.0);
            grad[(size_t)t * n + k] = g;
            up[(size_t)t * n + k] = (unsigned char)hi;
            if (!held[(size_t)t * n + k]) gap = gap + g * (u[(size_t)t * n + k] - (hi ? q->umax[k] : q->umin[k]));
        }
        v[0] = d0 ? m[0] : 0.0; v[1] = d1 ? m[1] : 0.0; v[2] = d2 ? m[2] : 0.0;
    }
    return gap;
}

static int nonfinite(double v) { return !(fabs(v) <= 1.7976931348623157e308); }

void npr_run(int R, int P, int H, int n, int prefix_days, int max_iter, int max_halvings, double tol, const double *sp,
             const double *u_min, const double *eps_grid, const double *u_fixed, const double *u_init, const double *J0_prefix,
             const double *J1_prefix, double *plan, double *J0, double *J1, double *F, double *gap_out, int32_t *iters_out,
             int32_t *halvings_out, int32_t *status, double *states, double *mu_out, double *F_trace, double *grad_out)
{
    const size_t B = (size_t)R * P, Hn = (size_t)H * n, H3 = (size_t)H * 3;
    double *u = malloc(Hn * 8), *ut = malloc(Hn * 8), *x = malloc(H3 * 8), *xt = malloc(H3 * 8), *mu = malloc(H3 * 8), *grad = malloc(Hn * 8);
    unsigned char *held = malloc(Hn), *up = malloc(Hn);
    const int pre = prefix_days > 0;
    for (size_t c = 0; c < B; c++) {
        const int r = (int)(c / P), l = (int)(c % P);
        region_t g;
        load_region(&g, sp, u_min, R, r, n);
        const double eps = eps_grid[l], ome = 1.0 - eps;
        const double j0p = pre ? J0_prefix[r] : 0.0, j1p = pre ? J1_prefix[r] : 0.0;
        for (int t = 0; t < H; t++)
            for (int k = 0; k < n; k++) {
                const size_t e = (size_t)t * n + k;
                const double uf = u_fixed ? u_fixed[e * R + r] : NAN;
                held[e] = (unsigned char)!isnan(uf);
                u[e] = held[e] ? uf : (u_init ? u_init[e * B + c] : g.umin[k]);
            }
        double sums[4], sums_t[4];
        double Fc = forward(&g, H, u, eps, ome, pre, j0p, j1p, x, sums), gap = NAN;
        int iters = 0, halv = 0, st = 0;
        for (size_t e = 0; e < H3; e++) mu[e] = NAN;
        for (size_t e = 0; e < Hn; e++) grad[e] = NAN;
        for (;;) {
            if (nonfinite(Fc)) { st |= 4; break; }
            if (F_trace) F_trace[(size_t)iters * B + c] = Fc;
            iters++;
            gap = adjoint(&g, H, x, u, held, eps, ome, mu, grad, up);
            if (gap <= tol * fabs(Fc)) break;
            if (iters == max_iter) { st |= 1; break; }
            int accepted = 0;
            double theta = 1.0;
            for (int j = 0; j <= max_halvings; j++) {
                for (int t = 0; t < H; t++)
                    for (int k = 0; k < n; k++) {
                        const size_t e = (size_t)t * n + k;
                        const double ustar = up[e] ? g.umax[k] : g.umin[k];
                        ut[e] = held[e] ? u[e] : u[e] + theta * (ustar - u[e]);
                    }
                const double Ft = forward(&g, H, ut, eps, ome, pre, j0p, j1p, xt, sums_t);
                if (Ft < Fc) {
                    Fc = Ft;
                    memcpy(u, ut, Hn * 8); memcpy(x, xt, H3 * 8); memcpy(sums, sums_t, sizeof sums);
                    accepted = 1;
                    break;
                }
                halv++;
                theta = theta * 0.5;
            }
            if (!accepted) { st |= 2; break; }
        }
        if (st & 4) {
            gap = NAN;
            for (size_t e = 0; e < H3; e++) mu[e] = NAN;
            for (size_t e = 0; e < Hn; e++) grad[e] = NAN;
        }
        if (F_trace)
            for (int q = iters; q < max_iter; q++) F_trace[(size_t)q * B + c] = NAN;
        const size_t days = (size_t)H + (size_t)(pre ? prefix_days : 0);
        for (size_t e = 0; e < Hn; e++) plan[e * B + c] = u[e];
        if (states) for (size_t e = 0; e < H3; e++) states[e * B + c] = x[e];
        if (mu_out) for (size_t e = 0; e < H3; e++) mu_out[e * B + c] = mu[e];
        if (grad_out) for (size_t e = 0; e < Hn; e++) grad_out[e * B + c] = grad[e];
        J0[c] = sums[2] / (double)days;
        J1[c] = sums[3] / (double)((size_t)n * days);
        F[c] = Fc; gap_out[c] = gap; iters_out[c] = iters; halvings_out[c] = halv; status[c] = st;
    }
    free(u); free(ut); free(x); free(xt); free(mu); free(grad); free(held); free(up);
}

/* one plan u [H][n] of region r at cost weight eps: out = {F, sum0, sum1, J0, J1}, x [H][3] */
void npr_score(int R, int r, int H, int n, int prefix_days, double eps, const double *sp, const double *u_min, const double *u,
               const double *J0_prefix, const double *J1_prefix, double *out, double *x)
{
    region_t g;
    load_region(&g, sp, u_min, R, r, n);
    const int pre = prefix_days > 0;
    double sums[4];
    out[0] = forward(&g, H, u, eps, 1.0 - eps, pre, pre ? J0_prefix[r] : 0.0, pre ? J1_prefix[r] : 0.0, x, sums);
    out[1] = sums[0]; out[2] = sums[1];
    const size_t days = (size_t)H + (size_t)(pre ? prefix_days : 0);
    out[3] = sums[2] / (double)days;
    out[4] = sums[3] / (double)((size_t)n * days);
}

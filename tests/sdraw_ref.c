/* The bit-exact C yardstick of the smoother draws (include/epiekf.h: epi_sdraw_*): a sequential restatement, one
 * chain, one day, one draw at a time, in the classic layout with double inputs (tests/sdraw_ref.py rounds them first for float
 * storage).  The pseudo-inverse is the oracle's orc_sym_pinv (linked from oracle/libekf_oracle.so); products that the smoother
 * hands to its BLAS use fma() as the oracle does, everything else is written operations (-ffp-contract=off). */
#include <math.h>
#include <stdint.h>
#include <stddef.h>

int orc_sym_pinv(int m, const double *A, double *X);

#define IX(i, j) ((i) + 3 * (j))
#define SDR_EPS 2.220446049250313e-16

double sdr_fma(double a, double b, double c) { return fma(a, b, c); }
void sdr_fma_vec(int n, double a, const double *b, const double *c, double *out)
{
    for (int i = 0; i < n; i++) out[i] = fma(a, b[i], c[i]);
}

static int nonfinite(double v) { return isnan(v) || isinf(v); }

/* right-looking Cholesky with diagonal pivoting and dpstf2's stop; F = the factor with its rows back in the original order */
int sdr_pchol(const double *S, double *F)
{
    double a[9], l[9];
    int piv[3] = {0, 1, 2}, rank = 0;
    for (int e = 0; e < 9; e++) { a[e] = S[e]; l[e] = 0.0; F[e] = 0.0; }
    double dmax = a[IX(0, 0)];
    for (int i = 1; i < 3; i++)
        if (a[IX(i, i)] > dmax) dmax = a[IX(i, i)];
    const double stop = 3.0 * SDR_EPS * dmax;
    for (int j = 0; j < 3; j++) {
        int pv = j;
        for (int q = j + 1; q < 3; q++)
            if (a[IX(q, q)] > a[IX(pv, pv)]) pv = q;
        const double best = a[IX(pv, pv)];
        if (!(best > stop) || !(best > 0.0)) break;
        if (pv != j) {
            double t;
            for (int c = 0; c < 3; c++) { t = a[IX(j, c)]; a[IX(j, c)] = a[IX(pv, c)]; a[IX(pv, c)] = t; }
            for (int r = 0; r < 3; r++) { t = a[IX(r, j)]; a[IX(r, j)] = a[IX(r, pv)]; a[IX(r, pv)] = t; }
            for (int c = 0; c < 3; c++) { t = l[IX(j, c)]; l[IX(j, c)] = l[IX(pv, c)]; l[IX(pv, c)] = t; }
            int ti = piv[j]; piv[j] = piv[pv]; piv[pv] = ti;
        }
        const double ajj = sqrt(best);
        l[IX(j, j)] = ajj;
        for (int i = j + 1; i < 3; i++) l[IX(i, j)] = a[IX(i, j)] / ajj;
        for (int c = j + 1; c < 3; c++)
            for (int i = j + 1; i < 3; i++) a[IX(i, c)] = a[IX(i, c)] - l[IX(i, j)] * l[IX(c, j)];
        rank = j + 1;
    }
    for (int i = 0; i < 3; i++)
        for (int c = 0; c < 3; c++) F[IX(piv[i], c)] = l[IX(i, c)];
    return rank;
}

static void clamp3(double *v, double slo, double ilo, double amin, double amax)
{
    const double c0 = fmin(1.0, fmax(slo, v[0])), c1 = fmin(1.0, fmax(ilo, v[1])), c2 = fmin(amax, fmax(amin, v[2]));
    v[0] = isnan(v[0]) ? v[0] : c0;
    v[1] = isnan(v[1]) ? v[1] : c1;
    v[2] = isnan(v[2]) ? v[2] : c2;
}

/* prm7: dt, beta, gamma, s_min, i_min, alpha_min, alpha_max, each [B].  The gains and factors of every (chain, day) */
void sdr_gain(int B, int T, const double *S_PLUS, const double *P_PLUS, const double *P_MINUS, const double *const *prm7,
              const double *P_term, int32_t *rank, int32_t *status, double *Jout, double *Lout)
{
    const double qnan = NAN;
    for (int c = 0; c < B; c++) {
        const double dt = prm7[0][c], beta = prm7[1][c], gamma = prm7[2][c];
        int st = 0;
        for (int k = 0; k < T; k++) {
            const int last = (k == T - 1);
            double Sp[3], Pp[9], Pm[9], J[9], F[9], Sig[9];
            for (int i = 0; i < 3; i++) Sp[i] = S_PLUS[((size_t)k * 3 + i) * B + c];
            for (int e = 0; e < 9; e++) Pp[e] = (last && P_term) ? P_term[(size_t)e * B + c] : P_PLUS[((size_t)k * 9 + e) * B + c];
            int badp = 0, badm = 0;
            for (int e = 0; e < 9; e++) badp |= nonfinite(Pp[e]);
            for (int i = 0; i < 3; i++) badp |= nonfinite(Sp[i]);
            for (int e = 0; e < 9; e++) J[e] = 0.0;
            for (int e = 0; e < 9; e++) Pm[e] = 0.0;
            if (!last) {
                for (int e = 0; e < 9; e++) Pm[e] = P_MINUS[((size_t)(k + 1) * 9 + e) * B + c];
                for (int e = 0; e < 9; e++) badm |= nonfinite(Pm[e]);
                if (!badm) {
                    double A[9] = {0}, PAt[9], Ps[9], Xp[9];
                    A[IX(0, 0)] = 1.0 - dt * Sp[2] * Sp[1];
                    A[IX(0, 1)] = -dt * Sp[2] * Sp[0];
                    A[IX(0, 2)] = -dt * Sp[0] * Sp[1];
                    A[IX(1, 0)] = dt * Sp[1] * Sp[2];
                    A[IX(1, 1)] = 1.0 + dt * (Sp[0] * Sp[2] - beta);
                    A[IX(1, 2)] = dt * Sp[0] * Sp[1];
                    A[IX(2, 2)] = 1.0 - dt * gamma;
                    for (int j = 0; j < 3; j++)
                        for (int i = 0; i < 3; i++) {
                            double acc = Pp[IX(i, 0)] * A[IX(j, 0)];
                            for (int q = 1; q < 3; q++) acc = fma(Pp[IX(i, q)], A[IX(j, q)], acc);
                            PAt[IX(i, j)] = acc;
                        }
                    for (int j = 0; j < 3; j++)                        /* the upper triangle of P_MINUS, mirrored */
                        for (int i = 0; i <= j; i++) { Ps[IX(i, j)] = Pm[IX(i, j)]; Ps[IX(j, i)] = Pm[IX(i, j)]; }
                    orc_sym_pinv(3, Ps, Xp);
                    for (int j = 0; j < 3; j++)
                        for (int i = 0; i < j; i++) Xp[IX(j, i)] = Xp[IX(i, j)];
                    for (int j = 0; j < 3; j++)
                        for (int i = 0; i < 3; i++) {
                            double acc = PAt[IX(i, 0)] * Xp[IX(0, j)];
                            for (int q = 1; q < 3; q++) acc = fma(PAt[IX(i, q)], Xp[IX(q, j)], acc);
                            J[IX(i, j)] = acc;
                        }
                } else {
                    for (int e = 0; e < 9; e++) Pm[e] = 0.0;
                }
            }
            int rk = -1;
            if (badp) {
                for (int e = 0; e < 9; e++) { J[e] = qnan; F[e] = qnan; }
            } else {
                double T1[9];
                for (int j = 0; j < 3; j++)
                    for (int i = 0; i < 3; i++) {
                        double acc = J[IX(i, 0)] * Pm[IX(0, j)];
                        for (int q = 1; q < 3; q++) acc = acc + J[IX(i, q)] * Pm[IX(q, j)];
                        T1[IX(i, j)] = acc;
                    }
                for (int j = 0; j < 3; j++)
                    for (int i = 0; i < 3; i++) {
                        double acc = T1[IX(i, 0)] * J[IX(j, 0)];
                        for (int q = 1; q < 3; q++) acc = acc + T1[IX(i, q)] * J[IX(j, q)];
                        Sig[IX(i, j)] = Pp[IX(i, j)] - acc;
                    }
                for (int j = 0; j < 3; j++)
                    for (int i = j + 1; i < 3; i++) {
                        const double v = (Sig[IX(i, j)] + Sig[IX(j, i)]) / 2.0;
                        Sig[IX(i, j)] = v;
                        Sig[IX(j, i)] = v;
                    }
                for (int i = 0; i < 3; i++) Sig[IX(i, i)] = (Sig[IX(i, i)] + Sig[IX(i, i)]) / 2.0;
                rk = sdr_pchol(Sig, F);
            }
            if (badp || badm) st |= 1;
            if (!badp && rk < 3) st |= 2;
            if (rank) rank[(size_t)k * B + c] = rk;
            for (int e = 0; e < 9; e++) {
                if (Jout) Jout[((size_t)k * 9 + e) * B + c] = J[e];
                if (Lout) Lout[((size_t)k * 9 + e) * B + c] = F[e];
            }
        }
        if (status) status[c] = st;
    }
}

/* z_mode 0: no noise, 1: double z, 2: float z.  The recursion of the paths from J, L [T][9][B] (what sdr_gain returned) */
void sdr_paths(int B, int T, int D, int k0, int clamp, int z_mode, int out_f32, const double *S_PLUS, const double *S_MINUS,
               const double *const *prm7, const void *z, const double *s_term, const double *J, const double *L, void *X)
{
    const size_t N = (size_t)B * (size_t)D;
    for (int c = 0; c < B; c++)
        for (int d = 0; d < D; d++) {
            const size_t p = (size_t)c * D + d;
            double x[3] = {0.0, 0.0, 0.0};
            for (int k = T - 1; k >= k0; k--) {
                const double *Jk = J, *Lk = L;
                double v[3];
                if (k == T - 1) {
                    for (int i = 0; i < 3; i++) v[i] = s_term ? s_term[(size_t)i * B + c] : S_PLUS[((size_t)k * 3 + i) * B + c];
                } else {
                    double dv[3];
                    for (int i = 0; i < 3; i++) dv[i] = x[i] - S_MINUS[((size_t)(k + 1) * 3 + i) * B + c];
                    for (int i = 0; i < 3; i++) {
                        double acc = Jk[((size_t)k * 9 + IX(i, 0)) * B + c] * dv[0];
                        for (int j = 1; j < 3; j++) acc = fma(Jk[((size_t)k * 9 + IX(i, j)) * B + c], dv[j], acc);
                        v[i] = S_PLUS[((size_t)k * 3 + i) * B + c] + acc;
                    }
                }
                if (z_mode) {
                    double zz[3];
                    for (int i = 0; i < 3; i++) {
                        const size_t o = ((size_t)(k - k0) * 3 + i) * N + p;
                        zz[i] = z_mode == 2 ? (double)((const float *)z)[o] : ((const double *)z)[o];
                    }
                    for (int i = 0; i < 3; i++) {
                        double nz = Lk[((size_t)k * 9 + IX(i, 0)) * B + c] * zz[0];
                        for (int j = 1; j < 3; j++) nz = nz + Lk[((size_t)k * 9 + IX(i, j)) * B + c] * zz[j];
                        v[i] = v[i] + nz;
                    }
                }
                if (clamp) clamp3(v, prm7[3][c], prm7[4][c], prm7[5][c], prm7[6][c]);
                for (int i = 0; i < 3; i++) {
                    const size_t o = ((size_t)(k - k0) * 3 + i) * N + p;
                    x[i] = v[i];
                    if (out_f32) ((float *)X)[o] = (float)v[i];
                    else ((double *)X)[o] = v[i];
                }
            }
        }
}

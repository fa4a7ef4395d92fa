/* The bit-exact C yardstick of the innovation whiteness diagnostics (csrc/innov_diag.hpp is held to it bit for
 * bit).  An independent restatement: one chain at a time, sequential walks over the filter steps with the standardised series
 * kept as a plain history, classic [T][B] doubles (tests/innov_diag_ref.py rounds e once for float storage and unblocks it).
 * Build: cc -O2 -ffp-contract=off -fPIC -shared (no contraction by the compiler: every product is rounded before it is added). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

static int finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }

/* e [T][B], S [T][B] or NULL; every output [B] (acf [H][B]) and may be NULL */
void idr_run(int B, int T, int H, int flip, int k0, int k1, const double *e, const double *S,
             double *mean_o, double *var_o, double *skew_o, double *kurt_o, double *jb_o, double *nis_sum_o, double *nis_mean_o,
             double *lb_q_o, double *het_o, double *cusumsq_max_o, double *max_abs_o,
             int32_t *n_o, int32_t *lb_lags_o, int32_t *het_n1_o, int32_t *het_n2_o, int32_t *cusumsq_step_o, int32_t *max_abs_step_o,
             int32_t *status_o, double *acf_o)
{
    double *nu = malloc(sizeof(double) * (size_t)T), *d = malloc(sizeof(double) * (size_t)T);
    char *ok = malloc((size_t)T);
    const int W = k1 - k0, h3 = (int)((2 * (long long)W + 3) / 6);
    for (int c = 0; c < B; c++) {
        int status = 0, n = 0, blk_n = 0;
        double sum1 = 0.0, q = 0.0, blk_s = 0.0, blk_q = 0.0;
        /* pass 1 */
        for (int k = 0; k < T; k++) {
            const size_t o = (size_t)(flip ? T - 1 - k : k) * B + c;
            ok[k] = 0;
            nu[k] = 0.0;
            if (k % 32 == 0) { blk_s = 0.0; blk_q = 0.0; blk_n = 0; }
            if (k >= k0 && k < k1) {
                const double ek = e[o];
                if (S) {
                    const double s = S[o];
                    if (s != s) { /* the day does not count */ }
                    else if (finite_d(s) && s >= 2.2250738585072014e-308 && finite_d(ek)) { ok[k] = 1; nu[k] = ek / sqrt(s); }
                    else status |= 1;
                } else {
                    if (ek != ek) { }
                    else if (finite_d(ek)) { ok[k] = 1; nu[k] = ek; }
                    else status |= 1;
                }
                if (ok[k]) {
                    blk_s = blk_s + nu[k];
                    blk_q = blk_q + nu[k] * nu[k];
                    blk_n = blk_n + 1;
                }
            }
            if (k % 32 == 31 || k == T - 1) { sum1 = sum1 + blk_s; q = q + blk_q; n = n + blk_n; }
        }
        if (n == 0) {
            status |= 2;
            if (mean_o) mean_o[c] = NAN;
            if (var_o) var_o[c] = NAN;
            if (skew_o) skew_o[c] = NAN;
            if (kurt_o) kurt_o[c] = NAN;
            if (jb_o) jb_o[c] = NAN;
            if (nis_sum_o) nis_sum_o[c] = NAN;
            if (nis_mean_o) nis_mean_o[c] = NAN;
            if (lb_q_o) lb_q_o[c] = NAN;
            if (het_o) het_o[c] = NAN;
            if (cusumsq_max_o) cusumsq_max_o[c] = NAN;
            if (max_abs_o) max_abs_o[c] = NAN;
            if (n_o) n_o[c] = 0;
            if (lb_lags_o) lb_lags_o[c] = 0;
            if (het_n1_o) het_n1_o[c] = 0;
            if (het_n2_o) het_n2_o[c] = 0;
            if (cusumsq_step_o) cusumsq_step_o[c] = -1;
            if (max_abs_step_o) max_abs_step_o[c] = -1;
            if (status_o) status_o[c] = status;
            if (acf_o) for (int h = 0; h < H; h++) acf_o[(size_t)h * B + c] = NAN;
            continue;
        }
        const double mean = sum1 / (double)n;
        /* pass 2: the moments, the thirds, the largest value, the CUSUM of squares */
        double m2 = 0.0, m3 = 0.0, m4 = 0.0, f = 0.0, l = 0.0, b2 = 0.0, b3 = 0.0, b4 = 0.0, bf = 0.0, bl = 0.0;
        double done_q = 0.0, run = 0.0, cs_max = 0.0, a_max = 0.0;
        int nf = 0, nl = 0, j = 0, cs_step = -1, a_step = -1;
        for (int k = 0; k < T; k++) {
            if (k % 32 == 0) { b2 = b3 = b4 = bf = bl = 0.0; run = 0.0; }
            d[k] = 0.0;
            if (ok[k]) {
                const double dk = nu[k] - mean, sq = nu[k] * nu[k];
                d[k] = dk;
                b2 = b2 + dk * dk;
                b3 = b3 + (dk * dk) * dk;
                b4 = b4 + (dk * dk) * (dk * dk);
                if (k < k0 + h3) { bf = bf + sq; nf = nf + 1; }
                if (k >= k1 - h3) { bl = bl + sq; nl = nl + 1; }
                run = run + sq;
                j = j + 1;
                const double cs = fabs((done_q + run) / q - (double)j / (double)n);
                if (cs_step < 0 || cs > cs_max || (cs != cs && cs_max == cs_max)) { cs_max = cs; cs_step = k; }
                const double av = fabs(nu[k]);
                if (a_step < 0 || av > a_max || (av != av && a_max == a_max)) { a_max = av; a_step = k; }
            }
            if (k % 32 == 31 || k == T - 1) {
                m2 = m2 + b2; m3 = m3 + b3; m4 = m4 + b4; f = f + bf; l = l + bl;
                done_q = done_q + run;
            }
        }
        const int deg = m2 == 0.0 || !finite_d(m2);
        const int Hu = H < n - 1 ? H : n - 1;
        if (deg) status |= 4;
        if (Hu < H) status |= 8;
        const double dn = (double)n, var = m2 / dn, sd = sqrt(var);
        const double skew = (m3 / dn) / (var * sd), kurt = (m4 / dn) / (var * var);
        const double jb = (dn / 6.0) * (skew * skew + ((kurt - 3.0) * (kurt - 3.0)) / 4.0);
        /* the lagged products, lag by lag */
        double lbsum = 0.0;
        for (int h = 1; h <= H; h++) {
            double ac = NAN;
            if (h <= Hu && !deg) {
                double ch = 0.0, bc = 0.0;
                for (int k = 0; k < T; k++) {
                    if (k % 32 == 0) bc = 0.0;
                    if (ok[k] && k + h < k1 && ok[k + h]) bc = bc + d[k] * d[k + h];
                    if (k % 32 == 31 || k == T - 1) ch = ch + bc;
                }
                ac = ch / m2;
                lbsum = lbsum + (ac * ac) / (double)(n - h);
            }
            if (acf_o) acf_o[(size_t)(h - 1) * B + c] = ac;
        }
        double lb = (dn * (double)(n + 2)) * lbsum;
        if (deg || (Hu < H && Hu == 0)) lb = NAN;
        if (mean_o) mean_o[c] = mean;
        if (var_o) var_o[c] = var;
        if (skew_o) skew_o[c] = deg ? NAN : skew;
        if (kurt_o) kurt_o[c] = deg ? NAN : kurt;
        if (jb_o) jb_o[c] = deg ? NAN : jb;
        if (nis_sum_o) nis_sum_o[c] = q;
        if (nis_mean_o) nis_mean_o[c] = q / dn;
        if (lb_q_o) lb_q_o[c] = lb;
        if (het_o) het_o[c] = (nf == 0 || nl == 0) ? NAN : (l / (double)nl) / (f / (double)nf);
        if (cusumsq_max_o) cusumsq_max_o[c] = cs_max;
        if (max_abs_o) max_abs_o[c] = a_max;
        if (n_o) n_o[c] = n;
        if (lb_lags_o) lb_lags_o[c] = Hu;
        if (het_n1_o) het_n1_o[c] = nf;
        if (het_n2_o) het_n2_o[c] = nl;
        if (cusumsq_step_o) cusumsq_step_o[c] = cs_step;
        if (max_abs_step_o) max_abs_step_o[c] = a_step;
        if (status_o) status_o[c] = status;
    }
    free(nu);
    free(d);
    free(ok);
}

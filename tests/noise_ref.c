/* The seeded standard-normal draws of include/epiekf.h, restated in plain C, one draw at a time: Philox4x32-10,
 * the 52-bit open uniform, Wichura's AS241 (PPND16) with the library's logarithm.  No code is shared with csrc/noise.hpp; compiled
 * with -ffp-contract=off, so that every written operation rounds once.  tests/noise_ref.py loads it. */
#include <math.h>
#include <stdint.h>

void nzr_philox(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    uint32_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]}, k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; r++) {
        const uint64_t a = (uint64_t)0xD2511F53u * c[0], b = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(b >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(a >> 32) ^ c[3] ^ k1;
        c[1] = (uint32_t)b; c[3] = (uint32_t)a; c[0] = n0; c[2] = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    for (int i = 0; i < 4; i++) out[i] = c[i];
}

/* the library's logarithm on (0, 1): x = 2^e m, m in [sqrt(1/2), sqrt(2)), the fdlibm polynomial, no fma */
static double nzr_log(double x)
{
    int e;
    double m = frexp(x, &e);
    if (m < 0.70710678118654752440) { m = m + m; e = e - 1; }
    const double f = m - 1.0, k = (double)e, s = f / (2.0 + f), z = s * s, w = z * z;
    const double t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01));
    const double t2 = z * (6.666666666666735130e-01 + w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 +
                                                                                           w * 1.479819860511658591e-01)));
    const double R = t2 + t1, hfsq = 0.5 * f * f;
    return k * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + k * 1.90821492927058770002e-10)) - f);
}

double nzr_uniform(uint32_t wa, uint32_t wb)
{
    const uint64_t n = ((uint64_t)(wa >> 6) << 26) + (uint64_t)(wb >> 6);
    return ((double)n + 0.5) * ldexp(1.0, -52);
}

static double horner(const double *c, double r)
{
    double acc = c[0];
    for (int k = 1; k < 8; k++) acc = acc * r + c[k];
    return acc;
}

double nzr_icdf(double u)
{
    static const double a[8] = {2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
                                1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0};
    static const double b[8] = {5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
                                5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0};
    static const double c[8] = {7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
                                3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0};
    static const double d[8] = {1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
                                6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0};
    static const double e[8] = {2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
                                2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0};
    static const double f[8] = {2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
                                1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0};
    const double q = u - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        return (horner(a, r) * q) / horner(b, r);
    }
    double r = sqrt(-nzr_log(q < 0.0 ? u : 1.0 - u)), x;
    if (r <= 5.0) { r = r - 1.6; x = horner(c, r) / horner(d, r); }
    else { r = r - 5.0; x = horner(e, r) / horner(f, r); }
    return q < 0.0 ? -x : x;
}

double nzr_draw(uint32_t seed_lo, uint32_t seed_hi, uint32_t stream, uint32_t t, uint32_t row, uint64_t lane)
{
    const uint32_t ctr[4] = {(uint32_t)(lane & 0xffffffffu), (uint32_t)(lane >> 32), t, 0x80000000u | (stream << 1) | (row >> 1)};
    const uint32_t key[2] = {seed_lo, seed_hi};
    uint32_t w[4];
    nzr_philox(ctr, key, w);
    const uint32_t j = row & 1u;
    return nzr_icdf(nzr_uniform(w[2 * j], w[2 * j + 1]));
}

/* out [nt][rows][n_lanes]: the window [t0, t0 + nt) x rows x [lane0, lane0 + n_lanes) */
void nzr_fill(uint32_t seed_lo, uint32_t seed_hi, uint32_t stream, uint32_t t0, int nt, int rows, uint64_t lane0, int64_t n_lanes, double *out)
{
    for (int t = 0; t < nt; t++)
        for (int row = 0; row < rows; row++)
            for (int64_t l = 0; l < n_lanes; l++)
                out[((int64_t)t * rows + row) * n_lanes + l] = nzr_draw(seed_lo, seed_hi, stream, t0 + (uint32_t)t, (uint32_t)row, lane0 + (uint64_t)l);
}

void nzr_icdf_vec(int64_t n, const double *u, double *z)
{
    for (int64_t k = 0; k < n; k++) z[k] = nzr_icdf(u[k]);
}

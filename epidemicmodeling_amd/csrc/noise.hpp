// Standard-normal draws from a seed, generated where they are used; included (inside namespace epi) by epiekf.hip, scenario_kernels.hpp
// and smoother_draws.hpp, entry points epi_noise_fill_device and the *_seeded calls (include/epiekf.h).  DESIGN.md
// §4.21 pins the definition; tests/noise_ref.c and tests/noise_ref.py restate it and the GPU suite holds the fill kernel to their
// bits.
//
//   philox4x32_10      the counter-based generator (Salmon et al., SC'11) the random NPI plans are drawn from, moved here unchanged
//   epi_normal_pair    rows 2 q and 2 q + 1 of (t, lane): ONE Philox block, key (seed_lo, seed_hi), counter (lane lo, lane hi, t,
//                      0x80000000 | stream << 1 | q); words (0, 1) make the even row's uniform, (2, 3) the odd row's
//   epi_normal_draw    one row of it (the other half of the block is discarded)
//   noise_fill         one lane per (t, row pair, lane) of a window of the logical array [nt][rows][lanes], writing the pair
//
// u = (n + 0.5) 2^-52 with n = (w_a >> 6) 2^26 + (w_b >> 6): exact in double and strictly inside (0, 1), so the logarithm of the
// tails never sees 0 and |z| <= 8.2096 (u = 2^-53).  z = the inverse normal CDF of u by Wichura's AS241 (PPND16): every polynomial
// is Horner in written operations (acc = acc * r + c; the library is built without contraction), the tails take r = sqrt(-epi_log(min(u,
// 1 - u))) with the library's epi_log and the correctly rounded sqrt, the quotient is one division.
//
// Cost: a block is 20 64-bit products of 32-bit words, a variate 14 fp64 multiplies and 14 additions, a division, and in the tails
// a logarithm and a root -- none of them full-rate instructions on CDNA.  15 % of the draws lie in the tails, so a 64-lane wave takes
// the central and the near-tail path almost always: the coefficients are SELECTED per lane and one Horner pair runs for all three
// branches; only the logarithm and the root sit behind a branch.  Measured: generating costs more than reading
// 24 bytes would -- sdraw_paths 4.0 ms against 2.2 ms at 300 x 1 024 x 520 -- and saves the array.
//
// Host-compilation contract: standard C++ over ekf_device.hpp (epi_log); the kernel itself is compiled by hipcc only.
#pragma once

// Philox4x32-10 (Salmon et al., SC'11): counter-based, so the draw of (region, scenario, NPI, day) does not depend
// on launch geometry and the CPU oracle reproduces it exactly.  MATLAB's randi stream itself cannot be matched
// (and is not part of the function's contract); the mapping plan -> (J0, J1) is what parity is checked on.
EPI_DEV void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4])
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// what a kernel carries of an epi_noise_desc
struct NoiseKey { uint32_t seed_lo, seed_hi, stream; };

constexpr long long kNoiseLaunchGroups = 1ll << 22;      // workgroups of 256 per launch: a launch's thread count is a 32-bit number
constexpr int kNoiseWg = 256;

EPI_DEV double epi_uniform_open(uint32_t wa, uint32_t wb)
{
    return ((double)(wa >> 6) * 67108864.0 + ((double)(wb >> 6) + 0.5)) * 2.220446049250313e-16;     // every step exact
}

// AS241 PPND16: the coefficient of r^k (k = 7 .. 0) of the numerator and the denominator, central / near tail / far tail
EPI_DEV double epi_normal_icdf(double u)
{
    constexpr double NA[8] = {2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
                              1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0};
    constexpr double DA[8] = {5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
                              5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0};
    constexpr double NC[8] = {7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
                              3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0};
    constexpr double DC[8] = {1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
                              6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0};
    constexpr double NE[8] = {2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
                              2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0};
    constexpr double DE[8] = {2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
                              1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0};
    const double q = u - 0.5;
    const bool central = fabs(q) <= 0.425;
    double r = 0.180625 - q * q;
    bool far = false;
    if (!central) {
        const double rt = sqrt(-epi_log(q < 0.0 ? u : 1.0 - u));
        far = rt > 5.0;
        r = far ? rt - 5.0 : rt - 1.6;
    }
    double num = central ? NA[0] : (far ? NE[0] : NC[0]), den = central ? DA[0] : (far ? DE[0] : DC[0]);
#pragma unroll
    for (int k = 1; k < 8; k++) {
        num = num * r + (central ? NA[k] : (far ? NE[k] : NC[k]));
        den = den * r + (central ? DA[k] : (far ? DE[k] : DC[k]));
    }
    num = central ? num * q : (q < 0.0 ? -num : num);
    return num / den;
}

// rows 2 q (z0) and 2 q + 1 (z1) of (t, lane)
EPI_DEV void epi_normal_pair(const NoiseKey &nk, uint32_t t, uint32_t q, uint64_t lane, double &z0, double &z1)
{
    uint32_t w[4];
    philox4x32_10((uint32_t)lane, (uint32_t)(lane >> 32), t, 0x80000000u | (nk.stream << 1) | q, nk.seed_lo, nk.seed_hi, w);
    z0 = epi_normal_icdf(epi_uniform_open(w[0], w[1]));
    z1 = epi_normal_icdf(epi_uniform_open(w[2], w[3]));
}

EPI_DEV double epi_normal_draw(const NoiseKey &nk, uint32_t t, uint32_t row, uint64_t lane)
{
    uint32_t w[4];
    philox4x32_10((uint32_t)lane, (uint32_t)(lane >> 32), t, 0x80000000u | (nk.stream << 1) | (row >> 1), nk.seed_lo, nk.seed_hi, w);
    return (row & 1u) ? epi_normal_icdf(epi_uniform_open(w[2], w[3])) : epi_normal_icdf(epi_uniform_open(w[0], w[1]));
}

// the three rows of a state-noise day: the pair (0, 1) and row 2
EPI_DEV void epi_normal_three(const NoiseKey &nk, uint32_t t, uint64_t lane, double &z0, double &z1, double &z2)
{
    epi_normal_pair(nk, t, 0u, lane, z0, z1);
    z2 = epi_normal_draw(nk, t, 2u, lane);
}

struct NoiseFillArgs {
    NoiseKey nk;
    int rows, f32;
    uint32_t t0;
    uint64_t lane0, n_lanes, items;                      // items = nt * pairs * n_lanes
    long long wg0;                                       // first workgroup of this launch
    void *out;                                           // [nt][rows][n_lanes] double or float
};

// item = (t * pairs + q) * n_lanes + l: the lanes of a wave write consecutive words of one row (and of the next)
EPI_DEV void noise_fill_lane(const NoiseFillArgs &a, uint64_t item)
{
    const uint64_t pairs = (uint64_t)(a.rows + 1) / 2, l = item % a.n_lanes, tq = item / a.n_lanes;
    const uint32_t q = (uint32_t)(tq % pairs);
    const uint64_t t = tq / pairs;
    const bool two = (int)(2 * q + 1) < a.rows;
    double z0, z1;
    epi_normal_pair(a.nk, a.t0 + (uint32_t)t, q, a.lane0 + l, z0, z1);
    const size_t o = (size_t)((t * (uint64_t)a.rows + 2 * q) * a.n_lanes + l);
    if (a.f32) {
        __builtin_nontemporal_store((float)z0, (float *)a.out + o);
        if (two) __builtin_nontemporal_store((float)z1, (float *)a.out + (o + (size_t)a.n_lanes));
    } else {
        __builtin_nontemporal_store(z0, (double *)a.out + o);
        if (two) __builtin_nontemporal_store(z1, (double *)a.out + (o + (size_t)a.n_lanes));
    }
}

#ifdef __HIPCC__
__global__ __launch_bounds__(kNoiseWg) void noise_fill(const NoiseFillArgs a)
{
    const uint64_t item = (uint64_t)(a.wg0 + (long long)blockIdx.x) * (uint64_t)kNoiseWg + threadIdx.x;
    if (item >= a.items) return;
    noise_fill_lane(a, item);
}
#endif

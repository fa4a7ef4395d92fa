// Monte-Carlo ensemble statistics: an output array of B = R * D chains (region-major: chain = r * D + d) -> mean, std, min,
// max, quantiles and the member count over the D draws of every (day, row, region); included by epiekf.hip (entry point
// epi_ens_run_device, include/epiekf.h).  DESIGN.md §4.7 pins the arithmetic; tests/ens_summary_ref.py restates it in
// NumPy and the GPU suite holds the two to the same values.
//
// One wavefront per item (day t, row, region r).  Element e of the item lives in register e / 64 of lane e % 64, so the
// loads are coalesced (64 consecutive values per instruction) and a lane holds NV = P / 64 values, P the power of two
// >= max(D, 64) (the kernel is instantiated for NV = 1 .. 64).  Elements D .. P-1 and NaN members are "absent": +0.0 in
// the two pairwise sums, +Inf in the sort.  No LDS, no barrier, no atomics, no host synchronisation.
//   sums   a[i] += a[i + h], h = P/2 .. 1: h >= 64 pairs registers of one lane, h < 64 pairs lanes (shuffle).  Padding D
//          to 64 when D < 64 adds +0.0 terms only: the value of the sum is that of the tree over the smaller P.
//   sort   bitonic network over the P elements, ascending: distance >= 64 is a compare-exchange of two registers,
//          distance < 64 a shuffle and a min or a max.  x(1 .. n) are then elements 0 .. n-1.
//   order statistics are read with a register select (the register index is wave-uniform) and one shuffle.
#pragma once

constexpr int kEnsMaxD = 4096, kEnsMaxQ = 16;

// items per launch: a launch's thread count (workgroups x 64 lanes) is a 32-bit number in the HIP runtime (lasso.hpp)
constexpr int64_t kEnsLaunchItems = (int64_t)1 << 25;

struct EnsArgs {
    int T, rows, rows_out, R, D, n_q, f32, derive;
    long long item0;               // first item of this launch
    const void *src;               // [T][rows][R * D], double or float
    const double *population;      // [R] (derive)
    double q[kEnsMaxQ];
    double *mean, *std, *mn, *mx;  // [T][rows_out][R]
    double *quant;                 // [T][n_q][rows_out][R]
    int32_t *count;                // [T][rows_out][R]
};

EPI_DEV double ens_load(const EnsArgs &a, size_t o)
{
    return a.f32 ? (double)((const float *)a.src)[o] : ((const double *)a.src)[o];
}

// a[0] of the pairwise tree over the wavefront's P = 64 NV elements, in every lane
template <int NV>
EPI_DEV double ens_tree(double (&s)[NV])
{
#pragma unroll
    for (int h = NV / 2; h >= 1; h >>= 1) {
#pragma unroll
        for (int j = 0; j < h; j++) s[j] = s[j] + s[j + h];
    }
    double t = s[0];
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) t = t + __shfl_xor(t, h);      // lane i < h: a[i] + a[i + h]
    return __shfl(t, 0);
}

// ascending bitonic sort of the P elements (no NaN among them)
template <int NV>
EPI_DEV void ens_sort(double (&w)[NV], int lane)
{
#pragma unroll
    for (int k = 2; k <= NV * 64; k <<= 1) {
#pragma unroll
        for (int d = k >> 1; d >= 1; d >>= 1) {
            if (d >= 64) {
                const int jd = d >> 6;
#pragma unroll
                for (int j = 0; j < NV; j++) {
                    if (j & jd) continue;
                    const double lo = fmin(w[j], w[j | jd]), hi = fmax(w[j], w[j | jd]);
                    const bool asc = ((j << 6) & k) == 0;
                    w[j] = asc ? lo : hi;
                    w[j | jd] = asc ? hi : lo;
                }
            } else {
#pragma unroll
                for (int j = 0; j < NV; j++) {
                    const double p = __shfl_xor(w[j], d);
                    const bool asc = k >= 64 ? ((j << 6) & k) == 0 : (lane & k) == 0;
                    const bool low = ((lane & d) == 0) == asc;
                    w[j] = low ? fmin(w[j], p) : fmax(w[j], p);
                }
            }
        }
    }
}

// element e (wave-uniform) of the sorted item, in every lane
template <int NV>
EPI_DEV double ens_pick(const double (&w)[NV], int e)
{
    const int je = e >> 6;
    double x = w[0];
#pragma unroll
    for (int j = 1; j < NV; j++) x = j == je ? w[j] : x;
    return __shfl(x, e & 63);
}

template <int NV>
__global__ __launch_bounds__(64) void ens_summary(const EnsArgs a)
{
    const int lane = threadIdx.x, D = a.D;
    const long long item = a.item0 + (long long)blockIdx.x;
    const int row = (int)(item % a.rows_out);
    const long long tr = item / a.rows_out;
    const int r = (int)(tr % a.R);
    const size_t t = (size_t)(tr / a.R), B = (size_t)a.R * (size_t)D;
    const double qnan = __builtin_nan("");
    double v[NV], w[NV];
    // ---- the item's members (absent = NaN) ----
    if (row < a.rows) {
        const size_t o = (t * (size_t)a.rows + (size_t)row) * B + (size_t)r * (size_t)D;
#pragma unroll
        for (int j = 0; j < NV; j++) {
            const int e = j * 64 + lane;
            v[j] = e < D ? ens_load(a, o + (size_t)e) : qnan;
        }
    } else {                            // the derived row: ((N_r v0) v1) v2 of rows 0, 1, 2
        const size_t o = t * (size_t)a.rows * B + (size_t)r * (size_t)D;
        const double N = a.population[r];
#pragma unroll
        for (int j = 0; j < NV; j++) {
            const int e = j * 64 + lane;
            v[j] = e < D ? ((N * ens_load(a, o + (size_t)e)) * ens_load(a, o + B + (size_t)e)) * ens_load(a, o + 2 * B + (size_t)e) : qnan;
        }
    }
    int n = 0;
#pragma unroll
    for (int j = 0; j < NV; j++) n += __popcll(__ballot(v[j] == v[j]));
    // ---- mean and std: two pairwise trees over the members in draw order ----
#pragma unroll
    for (int j = 0; j < NV; j++) w[j] = v[j] == v[j] ? v[j] : 0.0;
    const double mean = ens_tree<NV>(w) / (double)n;
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const double dev = v[j] == v[j] ? v[j] - mean : 0.0;
        w[j] = dev * dev;
    }
    double sd = sqrt(ens_tree<NV>(w) / (double)(n - 1));
    if (n == 1) sd = 0.0;
    const size_t oo = (t * (size_t)a.rows_out + (size_t)row) * (size_t)a.R + (size_t)r;
    if (lane == 0) {
        a.count[oo] = n;
        if (a.mean) a.mean[oo] = n ? mean : qnan;
        if (a.std) a.std[oo] = n ? sd : qnan;
    }
    if (!(a.mn || a.mx || a.quant)) return;
    if (n == 0) {
        if (lane == 0) {
            if (a.mn) a.mn[oo] = qnan;
            if (a.mx) a.mx[oo] = qnan;
            if (a.quant)
                for (int k = 0; k < a.n_q; k++) a.quant[((t * (size_t)a.n_q + (size_t)k) * (size_t)a.rows_out + (size_t)row) * (size_t)a.R + (size_t)r] = qnan;
        }
        return;
    }
    // ---- order statistics ----
#pragma unroll
    for (int j = 0; j < NV; j++) w[j] = v[j] == v[j] ? v[j] : (double)INFINITY;
    ens_sort<NV>(w, lane);
    const double x1 = ens_pick<NV>(w, 0), xn = ens_pick<NV>(w, n - 1);
    if (lane == 0) {
        if (a.mn) a.mn[oo] = x1;
        if (a.mx) a.mx[oo] = xn;
    }
    if (!a.quant) return;
    for (int k = 0; k < a.n_q; k++) {
        const double h = (double)n * a.q[k] + 0.5;
        const double kf = floor(h), g = h - kf;
        double res;
        if (kf < 1.0) {
            res = x1;
        } else if (kf >= (double)n) {
            res = xn;
        } else {
            const int ki = (int)kf;                                  // 1 .. n-1
            const double xk = ens_pick<NV>(w, ki - 1), xk1 = ens_pick<NV>(w, ki);
            res = xk + g * (xk1 - xk);
        }
        if (lane == 0) a.quant[((t * (size_t)a.n_q + (size_t)k) * (size_t)a.rows_out + (size_t)row) * (size_t)a.R + (size_t)r] = res;
    }
}

template <int NV>
inline hipError_t ens_launch(const EnsArgs &g, unsigned items, hipStream_t st)
{
    hipLaunchKernelGGL(ens_summary<NV>, dim3(items), dim3(64), 0, st, g);
    return hipGetLastError();
}

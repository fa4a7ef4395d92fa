// Curve statistics of the Monte-Carlo ensembles: an array of N = R * D joint paths (region-major, what ens_summary.hpp takes) ->
// per path and row the modified band depth (bands of two curves, rank form), the modified hypograph index and the depth rank
// within its region; per (day, row, region) the envelopes of the deepest fractions of the CURVES, the deepest curve itself and
// the functional boxplot's whiskers; per path its days outside the fences.  Included by epiekf.hip after path_functionals.hpp
// (entry point epi_cdepth_run_device, include/epiekf_cdepth.h).  DESIGN.md §4.23 pins the definition; tests/curve_depth_ref.py and
// tests/curve_depth_ref.c restate it and the GPU suite holds the device to the same bits.  Everything but the two final divisions
// and the fences is integer counts, min and max: no order of the work changes a bit.
//
//   cdepth_days<F32, NV>  (the hot path) one wavefront per (row, region, time segment); a segment is whole 32-day blocks.  Per day
//                   the members are loaded in the ens_summary register layout (element e in register e / 64 of lane e % 64,
//                   NV = P / 64 registers, P the power of two >= max(D, 64)), sorted with ens_sort (absent = +Inf) and the
//                   sorted copy is placed in LDS; every lane then reads its members AGAIN (the line is in cache; keeping them
//                   beside the sort would double the registers at NV = 64) and finds `below` and `above` with two branch-free
//                   binary searches of log2 P steps in LDS.  c_t, C(n_t), n_t - above and n_t are added into per-member
//                   32-bit accumulators in registers (the lane owns member (j, lane) on every day: no LDS adds at all); after
//                   32 days (32 C(4096, 2) < 2^31) they go to the workspace as the block's record.
//   cdepth_combine  one lane per (path, row): adds the block records as 64-bit integers, divides once for depth and mhi.
//   cdepth_rank     one lane per (path, row): counts the deeper paths and the equal ones of lower index over its region's D
//                   depths (every lane of a region reads the same address: one cache line per 8 steps); the lane of draw 0
//                   writes n_ranked, the lane of rank 0 median_path.
//   cdepth_envelope<F32>  one wavefront per (day, row, region): one read of the item, the members masked by depth_rank < m_k for
//                   every fraction at once (the fence's fraction rides along as one more), wave min / max by shuffles.  With
//                   mode 1 the mask is "ranked and out_days == 0": the whiskers.
//   cdepth_fence<F32>  one lane per (path, row) streaming the days against the fence envelope, as pathfn_paths streams them.
//   cdepth_outliers one lane per (row, region): the ranked paths with out_days > 0.
// No global atomics, no host synchronisation, no allocation.  Every element offset is 64-bit.
//
// Host-compilation contract (loglik.hpp): the bodies of cdepth_combine, cdepth_rank, cdepth_fence and cdepth_outliers are the
// EPI_DEV functions cdepth_*_lane of their indices; tests/curve_depth_emu.cpp compiles them with the host compiler
// (EPI_CDEPTH_HOST: without the kernels) and calls them lane by lane.
#pragma once

constexpr int kCdMaxAlpha = 8;                            // central regions of one call
constexpr int kCdMaxFrac = kCdMaxAlpha + 1;               // and the fence's fraction
constexpr int kCdBlock = 32;                              // days of one block record: 32 C(4096, 2) < 2^31
constexpr int kCdMaxD = 4096;
constexpr int kCdChunk = 8;                               // members a lane reads again at a time in the depth pass
constexpr int kCdLaneWg = 256;
constexpr int kCdMaxSeg = 1024;
constexpr long long kCdLaunchGroups = 1ll << 22;          // workgroups per launch: a launch's thread count is a 32-bit number

struct CdArgs {
    int T, rows, rows_out, R, D, derive, k0, k1;
    int nseg, seg_days, nblk;               // segments, days of a segment (a multiple of kCdBlock), blocks of the window
    int n_alpha, nk, mode;                  // envelope pass: nk fractions in frac (n_alpha, + 1 with the fence's); mode 1: the whiskers
    long long group0;                       // first workgroup of this launch
    double frac[kCdMaxFrac];
    double fence_factor;
    const void *src;                        // [T][rows][N], double or float
    const double *population;               // [R] (derive)
    const int32_t *first_day;               // [R] or NULL (0)
    uint32_t *rec;                          // [nblk][4][M]: band, pairs, le | valid days << 24, members (M = rows_out * N)
    double *depth, *mhi, *band_count, *pair_total;   // [rows_out][N] (depth: output or workspace)
    int32_t *n_valid;                       // [rows_out][N]
    int32_t *depth_rank, *out_days;         // [rows_out][N], output or workspace
    int32_t *n_ranked, *median_path;        // [rows_out][R], output or workspace
    int32_t *n_outliers;                    // [rows_out][R]
    double *env_lo, *env_hi;                // [T][n_alpha][rows_out][R]
    double *median_curve;                   // [T][rows_out][R]
    double *fence_lo, *fence_hi;            // [T][rows_out][R], workspace
    double *whisk_lo, *whisk_hi;            // [T][rows_out][R]
};

template <int F32>
EPI_DEV double cd_ld(const void *p, size_t o)
{
    return F32 ? (double)((const float *)p)[o] : ((const double *)p)[o];
}

// the value of path p on day t in row q (q = a.rows: the derived row)
template <int F32>
EPI_DEV double cd_member(const CdArgs &a, int t, int q, size_t p)
{
    const size_t N = (size_t)a.R * (size_t)a.D, o = (size_t)t * (size_t)a.rows * N + p;
    if (q < a.rows) return cd_ld<F32>(a.src, o + (size_t)q * N);
    return ((a.population[p / (size_t)a.D] * cd_ld<F32>(a.src, o)) * cd_ld<F32>(a.src, o + N)) * cd_ld<F32>(a.src, o + 2 * N);
}

// min and max of two values that are not NaN; of zeros of both signs the min is -0.0 and the max +0.0, whatever the order
EPI_DEV double cd_min(double x, double y) { return y < x || (y == x && __builtin_signbit(y)) ? y : x; }
EPI_DEV double cd_max(double x, double y) { return y > x || (y == x && !__builtin_signbit(y)) ? y : x; }

EPI_DEV int cd_first_day(const CdArgs &a, int r)
{
    const int fd = a.first_day ? a.first_day[r] : 0;
    return a.k0 > fd ? a.k0 : fd;
}

// m of a fraction: min(n, max(1, (int)ceil(f n)))
EPI_DEV int cd_deepest(double f, int n)
{
    int m = (int)ceil(f * (double)n);
    m = m < 1 ? 1 : m;
    return m < n ? m : n;
}

// ---- one (path, row): the block records added as 64-bit integers ----
EPI_DEV void cdepth_combine_lane(const CdArgs &a, size_t p, int q)
{
    const size_t N = (size_t)a.R * (size_t)a.D, M = (size_t)a.rows_out * N, m = (size_t)q * N + p;
    unsigned long long band = 0, pairs = 0, le = 0, mem = 0;
    int nv = 0;
    for (int b = 0; b < a.nblk; b++) {
        const uint32_t *rc = a.rec + (size_t)b * 4 * M + m;
        band += rc[0];
        pairs += rc[M];
        le += rc[2 * M] & 0xffffffu;
        nv += (int)(rc[2 * M] >> 24);
        mem += rc[3 * M];
    }
    const double qnan = __builtin_nan("");
    if (a.depth) a.depth[m] = pairs ? (double)band / (double)pairs : qnan;
    if (a.mhi) a.mhi[m] = nv ? (double)le / (double)mem : qnan;
    if (a.band_count) a.band_count[m] = (double)band;
    if (a.pair_total) a.pair_total[m] = (double)pairs;
    if (a.n_valid) a.n_valid[m] = nv;
}

// ---- one (path, row): its rank among the D depths of its region ----
EPI_DEV void cdepth_rank_lane(const CdArgs &a, size_t p, int q)
{
    const size_t N = (size_t)a.R * (size_t)a.D, m = (size_t)q * N + p;
    const int r = (int)(p / (size_t)a.D), d = (int)(p % (size_t)a.D);
    const double *dep = a.depth + (size_t)q * N + (size_t)r * (size_t)a.D;
    const double x = dep[d];
    int gt = 0, eq = 0, nr = 0;
    for (int e = 0; e < a.D; e++) {
        const double y = dep[e];
        nr += y == y ? 1 : 0;
        gt += y > x ? 1 : 0;
        eq += e < d && y == x ? 1 : 0;
    }
    const int rank = x == x ? gt + eq : -1;
    const size_t col = (size_t)q * (size_t)a.R + (size_t)r;
    a.depth_rank[m] = rank;
    if (d == 0) {
        a.n_ranked[col] = nr;
        if (nr == 0) a.median_path[col] = -1;
    }
    if (rank == 0) a.median_path[col] = d;
}

// ---- one (path, row): its days outside the fences ----
template <int F32>
EPI_DEV void cdepth_fence_lane(const CdArgs &a, size_t p, int q)
{
    const size_t N = (size_t)a.R * (size_t)a.D, plane = (size_t)a.rows_out * (size_t)a.R;
    const int r = (int)(p / (size_t)a.D);
    const size_t col = (size_t)q * (size_t)a.R + (size_t)r;
    int out = 0;
    for (int t = cd_first_day(a, r); t < a.k1; t++) {
        const double v = cd_member<F32>(a, t, q, p);
        const double lo = a.fence_lo[(size_t)t * plane + col], hi = a.fence_hi[(size_t)t * plane + col];
        const double w = hi - lo;
        const double fw = a.fence_factor * w;
        const double lo_f = lo - fw, hi_f = hi + fw;
        out += v == v && (v < lo_f || v > hi_f) ? 1 : 0;
    }
    a.out_days[(size_t)q * N + p] = out;
}

// ---- one (row, region): the ranked paths with a day outside the fences ----
EPI_DEV void cdepth_outliers_lane(const CdArgs &a, size_t col)
{
    const size_t N = (size_t)a.R * (size_t)a.D;
    const size_t q = col / (size_t)a.R, r = col % (size_t)a.R, base = q * N + r * (size_t)a.D;
    int n = 0;
    for (int d = 0; d < a.D; d++) n += a.depth_rank[base + (size_t)d] >= 0 && a.out_days[base + (size_t)d] > 0 ? 1 : 0;
    a.n_outliers[col] = n;
}

#ifndef EPI_CDEPTH_HOST
// days t0 <= t < t1 of segment s
EPI_DEV void cd_segment(const CdArgs &a, int s, int &t0, int &t1)
{
    const long long b = (long long)a.k0 + (long long)s * a.seg_days, e = b + a.seg_days;
    t0 = (int)(b < a.k1 ? b : a.k1);
    t1 = (int)(e < a.k1 ? e : a.k1);
}

// workgroup (x: (row, region), y: segment), one wavefront
template <int F32, int NV>
__global__ __launch_bounds__(64) void cdepth_days(const CdArgs a)
{
    constexpr int P = NV * 64;
    __shared__ double srt[P];
    const int lane = threadIdx.x, D = a.D;
    const long long item = a.group0 + (long long)blockIdx.x;
    const int r = (int)(item % a.R), q = (int)(item / a.R);
    const size_t N = (size_t)a.R * (size_t)D, M = (size_t)a.rows_out * N, p0 = (size_t)r * (size_t)D;
    const int lo = cd_first_day(a, r);
    int t0, t1;
    cd_segment(a, (int)blockIdx.y, t0, t1);
    for (int tb = t0; tb < t1; tb += kCdBlock) {
        uint32_t band[NV], pairs[NV], lenv[NV], mem[NV];
#pragma unroll
        for (int j = 0; j < NV; j++) band[j] = pairs[j] = lenv[j] = mem[j] = 0;
        const int te = tb + kCdBlock < t1 ? tb + kCdBlock : t1;
        for (int t = tb > lo ? tb : lo; t < te; t++) {
            double w[NV];
            int n = 0;
#pragma unroll
            for (int j = 0; j < NV; j++) {
                const int e = j * 64 + lane;
                const double x = e < D ? cd_member<F32>(a, t, q, p0 + (size_t)e) : __builtin_nan("");
                n += __popcll(__ballot(x == x));
                w[j] = x == x ? x : (double)INFINITY;
            }
            ens_sort<NV>(w, lane);
            __syncthreads();                                           // the searches of the day before are done
#pragma unroll
            for (int j = 0; j < NV; j++) srt[j * 64 + lane] = w[j];
            __syncthreads();
            if (n == 0) continue;                                      // wave-uniform
            const uint32_t cn = (uint32_t)n * (uint32_t)(n - 1) / 2;
            // the members again, CH registers at a time: the fence keeps the compiler from hoisting all NV loads above the
            // searches, which at NV >= 32 spilled the accumulators to scratch
            constexpr int CH = NV < kCdChunk ? NV : kCdChunk;
#pragma unroll
            for (int j0 = 0; j0 < NV; j0 += CH) {
                double xs[CH];
#pragma unroll
                for (int i = 0; i < CH; i++) {
                    const int e = (j0 + i) * 64 + lane;
                    xs[i] = e < D ? cd_member<F32>(a, t, q, p0 + (size_t)e) : __builtin_nan("");
                }
#pragma unroll
                for (int i = 0; i < CH; i++) {
                const int j = j0 + i;
                const double x = xs[i];
                // below = #{sorted < x}, ub = #{sorted <= x} among the n values in front (behind them +Inf): the count of a
                // prefix of the P sorted elements, one bit of it per step; a count of P itself is looked at apart
                int lb = 0, ub = 0;
#pragma unroll
                for (int st = P / 2; st >= 1; st >>= 1) {
                    lb += srt[lb + st - 1] < x ? st : 0;
                    ub += srt[ub + st - 1] <= x ? st : 0;
                }
                ub = srt[P - 1] <= x ? P : ub;
                ub = ub < n ? ub : n;                                  // a member at +Inf: the absent ones are not above it
                const uint32_t below = (uint32_t)lb, above = (uint32_t)(n - ub);
                const uint32_t c = cn - below * (below - 1) / 2 - above * (above - 1) / 2;      // C(0) = 0 * 0xffffffff / 2 = 0
                const bool ok = x == x;
                band[j] += ok ? c : 0u;
                pairs[j] += ok ? cn : 0u;
                lenv[j] += ok ? (uint32_t)ub + (1u << 24) : 0u;
                mem[j] += ok ? (uint32_t)n : 0u;
                }
                __asm__ volatile("" ::: "memory");
            }
        }
        uint32_t *rc = a.rec + (size_t)((tb - a.k0) / kCdBlock) * 4 * M + (size_t)q * N + p0;
#pragma unroll
        for (int j = 0; j < NV; j++) {
            const int e = j * 64 + lane;
            if (e < D) {
                rc[(size_t)e] = band[j];
                rc[M + (size_t)e] = pairs[j];
                rc[2 * M + (size_t)e] = lenv[j];
                rc[3 * M + (size_t)e] = mem[j];
            }
        }
    }
}

__global__ __launch_bounds__(kCdLaneWg) void cdepth_combine(const CdArgs a)
{
    const size_t p = ((size_t)a.group0 + (size_t)blockIdx.x) * kCdLaneWg + threadIdx.x;
    if (p >= (size_t)a.R * (size_t)a.D) return;
    cdepth_combine_lane(a, p, (int)blockIdx.y);
}

__global__ __launch_bounds__(kCdLaneWg) void cdepth_rank(const CdArgs a)
{
    const size_t p = ((size_t)a.group0 + (size_t)blockIdx.x) * kCdLaneWg + threadIdx.x;
    if (p >= (size_t)a.R * (size_t)a.D) return;
    cdepth_rank_lane(a, p, (int)blockIdx.y);
}

template <int F32>
__global__ __launch_bounds__(kCdLaneWg) void cdepth_fence(const CdArgs a)
{
    const size_t p = ((size_t)a.group0 + (size_t)blockIdx.x) * kCdLaneWg + threadIdx.x;
    if (p >= (size_t)a.R * (size_t)a.D) return;
    cdepth_fence_lane<F32>(a, p, (int)blockIdx.y);
}

__global__ __launch_bounds__(kCdLaneWg) void cdepth_outliers(const CdArgs a)
{
    const size_t col = ((size_t)a.group0 + (size_t)blockIdx.x) * kCdLaneWg + threadIdx.x;
    if (col >= (size_t)a.rows_out * (size_t)a.R) return;
    cdepth_outliers_lane(a, col);
}

// workgroup = item (day t, row q, region r), one wavefront; mode 0: fraction k keeps the members with 0 <= depth_rank < m_k;
// mode 1: one "fraction", the ranked members with out_days == 0
template <int F32>
__global__ __launch_bounds__(64) void cdepth_envelope(const CdArgs a)
{
    const int lane = threadIdx.x, D = a.D;
    const long long item = a.group0 + (long long)blockIdx.x;
    const int r = (int)(item % a.R), q = (int)((item / a.R) % a.rows_out), t = (int)(item / ((long long)a.R * a.rows_out));
    const size_t N = (size_t)a.R * (size_t)D, plane = (size_t)a.rows_out * (size_t)a.R, col = (size_t)q * (size_t)a.R + (size_t)r;
    const size_t base = (size_t)q * N + (size_t)r * (size_t)D;
    const bool in = t >= cd_first_day(a, r) && t < a.k1;
    const int nk = a.mode ? 1 : a.nk, nr = a.n_ranked[col];
    const double qnan = __builtin_nan("");
    int m[kCdMaxFrac];
    double mn[kCdMaxFrac], mx[kCdMaxFrac];
    unsigned any = 0;
#pragma unroll
    for (int k = 0; k < kCdMaxFrac; k++) {
        m[k] = k >= nk ? 0 : (a.mode ? 1 : cd_deepest(a.frac[k], nr));
        mn[k] = (double)INFINITY;
        mx[k] = -(double)INFINITY;
    }
    if (in) {
        for (int e = lane; e < D; e += 64) {
            const int rank = a.depth_rank[base + (size_t)e];
            const int key = rank < 0 ? 0x7fffffff : (a.mode ? (a.out_days[base + (size_t)e] == 0 ? 0 : 0x7fffffff) : rank);
            const double v = cd_member<F32>(a, t, q, (size_t)r * (size_t)D + (size_t)e);
            if (v != v) continue;
#pragma unroll
            for (int k = 0; k < kCdMaxFrac; k++) {
                if (key < m[k]) {
                    mn[k] = cd_min(mn[k], v);
                    mx[k] = cd_max(mx[k], v);
                    any |= 1u << k;
                }
            }
        }
    }
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) {
        any |= (unsigned)__shfl_xor((int)any, h);
#pragma unroll
        for (int k = 0; k < kCdMaxFrac; k++) {
            mn[k] = cd_min(mn[k], __shfl_xor(mn[k], h));
            mx[k] = cd_max(mx[k], __shfl_xor(mx[k], h));
        }
    }
    if (lane != 0) return;
    const size_t oo = (size_t)t * plane + col;
    if (a.mode) {
        if (a.whisk_lo) a.whisk_lo[oo] = any & 1u ? mn[0] : qnan;
        if (a.whisk_hi) a.whisk_hi[oo] = any & 1u ? mx[0] : qnan;
        return;
    }
#pragma unroll
    for (int k = 0; k < kCdMaxFrac; k++) {
        if (k >= nk) continue;
        const bool has = (any >> k) & 1u;
        if (k < a.n_alpha) {
            const size_t ok = ((size_t)t * (size_t)a.n_alpha + (size_t)k) * plane + col;
            if (a.env_lo) a.env_lo[ok] = has ? mn[k] : qnan;
            if (a.env_hi) a.env_hi[ok] = has ? mx[k] : qnan;
        } else {
            a.fence_lo[oo] = has ? mn[k] : qnan;
            a.fence_hi[oo] = has ? mx[k] : qnan;
        }
    }
    if (a.median_curve) {
        const int mp = a.median_path[col];
        a.median_curve[oo] = in && mp >= 0 ? cd_member<F32>(a, t, q, (size_t)r * (size_t)D + (size_t)mp) : qnan;
    }
}
#endif

// Joint (multivariate) scores of the Monte-Carlo ensembles: an array of B = R * D chains (region-major, what ens_summary.hpp
// takes) and a truth -> per (row, region) over a window of days the energy score and the variogram score of the D paths;
// included by epiekf.hip after ens_summary.hpp (entry point epi_ejoint_run_device, include/epiekf.h).  DESIGN.md §4.20 pins the
// arithmetic; tests/ejoint_ref.py and tests/ejoint_ref.c restate it and the GPU suite holds them to the same bits.
//
// An item is one (row, region r), item = row * R + r; its days are the t of the window from first_day[r] on whose truth is not
// NaN, its members the draws without a NaN on any of those days.
// The wavefront kernels are templates of the storage type S (double or float), so that a day's loads are issued together and no
// branch on the storage sits at a load.
//   ejoint_members  one wavefront per item in the shape of ens_summary<NV> (member e in register e / 64 of lane e % 64): walks the
//                   window once, writes the item's day list, n, W, the mask of present members (one 64-bit word per block of 64
//                   members), the e_i (member_dist) and tree(e): the pre-pass the other two kernels read their masks from.
//   ejoint_pairs    the hot path: one wavefront per (item, tile I <= J) of 64 x 64 members.  Lane i holds member I * 64 + i and
//                   the 64 accumulators d2(i, j) in registers across the day loop; a day's 64 values of block J are formed once
//                   (one per lane: float conversion and derived row included), written to an LDS image and read by every lane
//                   at one address (a broadcast read).  The next day's values are loaded raw before the day's 3 * 64 fp64
//                   operations and formed a day later, so the loads fly under the arithmetic.  sqrt runs once per pair after
//                   the loop; the tile sum goes to the slot [item][tile] of the
//                   workspace from lane 0.  The grid is item-major and remapped so that the blocks that share an L2 (block id
//                   modulo 8) get consecutive tiles: an item's re-reads stay in one L2.  The map is a bijection of the launch's
//                   blocks and every block writes its own slot, so it decides the speed only.
//   ejoint_vario    one wavefront per (item, day s of the item) in the shape of ens_summary<NV>: x_s stays in registers, the
//                   later days t are walked with one ens_tree per pair of days; writes v_s to the workspace.
//   ejoint_final    one lane per (row, region): adds the tile sums and the v_s in the pinned order and forms the outputs.
// No atomics anywhere.  All element offsets are 64-bit.
//
// Host-compilation contract (loglik.hpp): the body of ejoint_final is the EPI_DEV function ejoint_final_lane of its indices, and
// the unit and workspace arithmetic of the launches (ejoint_tile_of, ejoint_swizzle, ejoint_for_units, ejoint_carve) is plain C++; tests/ejoint_emu.cpp
// compiles them with the host compiler (EPI_EJOINT_HOST: without the wavefront kernels) and runs them lane by lane.
#pragma once

struct EjArgs {
    int T, rows, rows_out, R, D, Rt, f32, derive, k0, k1, vs_order, max_lag;
    int nb, tiles, wcap;                    // blocks of 64 members, nb (nb + 1) / 2 tiles, k1 - k0 days of the window
    long long unit0, units;                 // first unit (item, tile or day) of this launch, units in it
    const void *src;                        // [T][rows][R * D], double or float
    const double *population;               // [R] (derive)
    const double *truth;                    // [T][rows_out][Rt]
    const int32_t *truth_series;            // [R] or NULL (r itself)
    const int32_t *first_day;               // [R] or NULL (0)
    // the workspace
    int32_t *n_mem, *n_day;                 // [items]
    int32_t *days;                          // [items][wcap]: the item's days, ascending
    unsigned long long *mask;               // [items][nb]: bit i of word I = member I * 64 + i is present
    double *tsum;                           // [items]: tree(e)
    double *tile;                           // [items][tiles] or NULL (no pair sum asked for)
    double *vrow;                           // [items][wcap] or NULL (no variogram score asked for)
    // the outputs, each may be NULL
    double *es, *truth_term, *spread_term, *vs;   // [rows_out][R]
    int32_t *n_members, *n_days;            // [rows_out][R]
    double *member_dist;                    // [rows_out][R * D]
};

// tile number -> (I, J), I <= J < nb, in the order I ascending, then J ascending from I
EPI_DEV void ejoint_tile_of(int tile, int nb, int &I, int &J)
{
    I = 0;
    while (tile >= nb - I) { tile -= nb - I; I++; }
    J = I + tile;
}

// block b of a launch of n blocks -> the unit it works on: the blocks b, b + 8, b + 16, .. get consecutive units (a bijection
// of 0 .. n-1 for every n)
EPI_DEV long long ejoint_swizzle(long long b, long long n)
{
    const long long q = n / 8, rm = n % 8, x = b % 8;
    return (x < rm ? x * (q + 1) : rm * (q + 1) + (x - rm) * q) + b / 8;
}

// ---- the final pass ----
EPI_DEV void ejoint_final_lane(const EjArgs &a, int row, int r)
{
    const size_t col = (size_t)row * (size_t)a.R + (size_t)r;
    const int n = a.n_mem[col], W = a.n_day[col];
    const bool def = n > 0 && W > 0;
    const double qnan = __builtin_nan(""), nd = (double)n;
    if (a.n_members) a.n_members[col] = n;
    if (a.n_days) a.n_days[col] = W;
    if (a.es || a.truth_term || a.spread_term) {
        double tt = qnan, sp = qnan;
        if (def) {
            tt = a.tsum[col] / nd;
            if (a.tile) {
                double ps = 0.0;
                const double *ti = a.tile + col * (size_t)a.tiles;
                for (int k = 0; k < a.tiles; k++) ps = ps + ti[k];
                sp = ps / (nd * nd);
            }
        }
        if (a.truth_term) a.truth_term[col] = tt;
        if (a.spread_term) a.spread_term[col] = sp;
        if (a.es) a.es[col] = tt - sp;
    }
    if (a.vs) {
        double v = 0.0;
        if (def) {
            const double *vr = a.vrow + col * (size_t)a.wcap;
            for (int s = 0; s < W; s++) v = v + vr[s];
        }
        a.vs[col] = def ? v : qnan;
    }
}

#ifndef EPI_EJOINT_HOST
// the item's P = 64 NV positions on day t (position e in x[e / 64] of lane e % 64; beyond D: +0.0): the stored values, or the
// derived row ((N_r v0) v1) v2 of rows 0, 1, 2.  S = double or float, the storage; the loads of up to 16 registers are issued
// together, before the first of their values is formed and handed to use(j, value), j the register
template <int NV, typename S, typename F>
EPI_DEV void ej_day(const EjArgs &a, int row, int t, int r, int lane, F use)
{
    constexpr int CH = NV < 16 ? NV : 16;
    const S *src = (const S *)a.src;
    const size_t B = (size_t)a.R * (size_t)a.D, c = (size_t)r * (size_t)a.D + (size_t)lane;
    if (row < a.rows) {
        const S *p = src + ((size_t)t * (size_t)a.rows + (size_t)row) * B + c;
#pragma unroll
        for (int j0 = 0; j0 < NV; j0 += CH) {
            S v[CH];
#pragma unroll
            for (int j = 0; j < CH; j++) v[j] = (j0 + j) * 64 + lane < a.D ? p[(j0 + j) * 64] : (S)0;
#pragma unroll
            for (int j = 0; j < CH; j++) use(j0 + j, (double)v[j]);
        }
    } else {
        const S *p = src + (size_t)t * (size_t)a.rows * B + c;
        const double N = a.population[r];
#pragma unroll
        for (int j0 = 0; j0 < NV; j0 += CH) {
            S v0[CH], v1[CH], v2[CH];
#pragma unroll
            for (int j = 0; j < CH; j++) {
                const bool in = (j0 + j) * 64 + lane < a.D;
                v0[j] = in ? p[(j0 + j) * 64] : (S)0;
                v1[j] = in ? p[B + (j0 + j) * 64] : (S)0;
                v2[j] = in ? p[2 * B + (j0 + j) * 64] : (S)0;
            }
#pragma unroll
            for (int j = 0; j < CH; j++) use(j0 + j, (j0 + j) * 64 + lane < a.D ? ((N * (double)v0[j]) * (double)v1[j]) * (double)v2[j] : 0.0);
        }
    }
}

EPI_DEV double ej_truth(const EjArgs &a, int row, int t, int ts)
{
    return a.truth[((size_t)t * (size_t)a.rows_out + (size_t)row) * (size_t)a.Rt + (size_t)ts];
}

template <int NV, typename S>
__global__ __launch_bounds__(64) void ejoint_members(const EjArgs a)
{
    const int lane = threadIdx.x, D = a.D;
    const long long item = a.unit0 + (long long)blockIdx.x;
    const int row = (int)(item / a.R), r = (int)(item % a.R);
    const int ts = a.truth_series ? a.truth_series[r] : r;
    const int fd = a.first_day ? a.first_day[r] : 0;
    const double qnan = __builtin_nan("");
    double d2[NV];
    bool ok[NV];
#pragma unroll
    for (int j = 0; j < NV; j++) {
        d2[j] = 0.0;
        ok[j] = j * 64 + lane < D;
    }
    int32_t *days = a.days + (size_t)item * (size_t)a.wcap;
    int W = 0;
#pragma unroll 1
    for (int t = a.k0 > fd ? a.k0 : fd; t < a.k1; t++) {
        const double y = ej_truth(a, row, t, ts);
        if (y != y) continue;                                         // wave-uniform
        if (lane == 0) days[W] = t;
        W++;
        ej_day<NV, S>(a, row, t, r, lane, [&](int j, double x) {
            ok[j] = ok[j] && x == x;
            const double d = x - y;
            d2[j] = d2[j] + d * d;
        });
    }
    int n = 0;
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const unsigned long long m = __ballot(ok[j]);
        n += __popcll(m);
        if (lane == 0 && j < a.nb) a.mask[(size_t)item * (size_t)a.nb + (size_t)j] = m;
    }
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const int e = j * 64 + lane;
        const double v = sqrt(d2[j]);
        if (a.member_dist && e < D) a.member_dist[(size_t)item * (size_t)D + (size_t)e] = ok[j] && W > 0 ? v : qnan;
        d2[j] = ok[j] ? v : 0.0;
    }
    const double sum = ens_tree<NV>(d2);
    if (lane == 0) {
        a.n_mem[item] = n;
        a.n_day[item] = W;
        a.tsum[item] = sum;
    }
}

// a member's stored values on one day as they were loaded (S = double or float): forming the member (the float conversion, the
// derived row's product) waits for the loads, so it is done a day later, when they have flown under that day's arithmetic
template <typename S>
struct EjRaw { S v0, v1, v2; };

template <typename S>
EPI_DEV EjRaw<S> ej_raw(const EjArgs &a, bool in, int row, int t, int r, int e)
{
    EjRaw<S> q{(S)0, (S)0, (S)0};                                     // a position beyond D: +0.0
    if (!in) return q;
    const S *src = (const S *)a.src;
    const size_t B = (size_t)a.R * (size_t)a.D, c = (size_t)r * (size_t)a.D + (size_t)e;
    if (row < a.rows) {
        q.v0 = src[((size_t)t * (size_t)a.rows + (size_t)row) * B + c];
    } else {
        const size_t o = (size_t)t * (size_t)a.rows * B + c;
        q.v0 = src[o]; q.v1 = src[o + B]; q.v2 = src[o + 2 * B];
    }
    return q;
}

template <typename S>
EPI_DEV double ej_formed(const EjArgs &a, const EjRaw<S> &q, int row, double N)
{
    if (row < a.rows) return (double)q.v0;
    return ((N * (double)q.v0) * (double)q.v1) * (double)q.v2;
}

template <typename S>
__global__ __launch_bounds__(64) void ejoint_pairs(const EjArgs a)
{
    __shared__ double img[2][64];
    const int lane = threadIdx.x, D = a.D;
    const long long u = a.unit0 + ejoint_swizzle((long long)blockIdx.x, a.units);
    const long long item = u / a.tiles;
    const int tile = (int)(u % a.tiles);
    const int n = a.n_mem[item], W = a.n_day[item];
    if (n == 0 || W == 0) return;                                     // the final pass does not read the slots of such an item
    int I, J;
    ejoint_tile_of(tile, a.nb, I, J);
    const int row = (int)(item / a.R), r = (int)(item % a.R);
    const int ei = I * 64 + lane, ej = J * 64 + lane;
    const bool ini = ei < D, inj = ej < D;
    const double N = row < a.rows ? 0.0 : a.population[r];
    const int32_t *days = a.days + (size_t)item * (size_t)a.wcap;
    double acc[64];
#pragma unroll
    for (int j = 0; j < 64; j++) acc[j] = 0.0;
    EjRaw<S> qi = ej_raw<S>(a, ini, row, days[0], r, ei), qj = ej_raw<S>(a, inj, row, days[0], r, ej);
#pragma unroll 1
    for (int w = 0; w < W; w++) {
        double *im = img[w & 1];                                      // two images: a day's write never meets the day before's reads
        const double xc = ej_formed<S>(a, qi, row, N);
        im[lane] = ej_formed<S>(a, qj, row, N);
        __syncthreads();
        if (w + 1 < W) {                                              // the next day's loads fly under this day's arithmetic
            const int t = days[w + 1];
            qi = ej_raw<S>(a, ini, row, t, r, ei);
            qj = ej_raw<S>(a, inj, row, t, r, ej);
        }
#pragma unroll
        for (int j = 0; j < 64; j++) {
            const double d = xc - im[j];
            acc[j] = acc[j] + d * d;
        }
    }
    const unsigned long long mi = a.mask[(size_t)item * (size_t)a.nb + (size_t)I], mj = a.mask[(size_t)item * (size_t)a.nb + (size_t)J];
    const bool pi = (mi >> lane) & 1ull;
    double s[1] = {0.0};
#pragma unroll
    for (int j = 0; j < 64; j++) {
        const bool on = pi && ((mj >> j) & 1ull) && (I != J || j > lane);
        const double v = sqrt(acc[j]);
        s[0] = s[0] + (on ? v : 0.0);
    }
    const double sum = ens_tree<1>(s);
    if (lane == 0) a.tile[(size_t)item * (size_t)a.tiles + (size_t)tile] = sum;
}

template <int NV, typename S>
__global__ __launch_bounds__(64) void ejoint_vario(const EjArgs a)
{
    const int lane = threadIdx.x, D = a.D;
    const long long u = a.unit0 + (long long)blockIdx.x;
    const long long item = u / a.wcap;
    const int s = (int)(u % a.wcap);
    const int n = a.n_mem[item], W = a.n_day[item];
    if (n == 0 || W == 0 || s >= W) return;                           // the final pass reads v_s for s < W only
    const int row = (int)(item / a.R), r = (int)(item % a.R);
    const int ts = a.truth_series ? a.truth_series[r] : r;
    const int32_t *days = a.days + (size_t)item * (size_t)a.wcap;
    const int t0 = days[s];
    const double y0 = ej_truth(a, row, t0, ts), nd = (double)n;
    double x0[NV], g[NV];
    bool ok[NV];
    ej_day<NV, S>(a, row, t0, r, lane, [&](int j, double x) { x0[j] = x; });
#pragma unroll
    for (int j = 0; j < NV; j++) {
        ok[j] = j < a.nb ? (a.mask[(size_t)item * (size_t)a.nb + (size_t)j] >> lane) & 1ull : false;
    }
    double v = 0.0;
#pragma unroll 1
    for (int w = s + 1; w < W; w++) {
        const int t = days[w];
        if (a.max_lag > 0 && t - t0 > a.max_lag) break;
        ej_day<NV, S>(a, row, t, r, lane, [&](int j, double x) {
            double d = fabs(x0[j] - x);
            if (a.vs_order == 1) d = sqrt(d);
            g[j] = ok[j] ? d : 0.0;
        });
        const double m = ens_tree<NV>(g) / nd;
        double gy = fabs(y0 - ej_truth(a, row, t, ts));
        if (a.vs_order == 1) gy = sqrt(gy);
        const double term = gy - m;
        v = v + term * term;
    }
    if (lane == 0) a.vrow[(size_t)item * (size_t)a.wcap + (size_t)s] = v;
}

constexpr int kEjFinalWg = 256;
__global__ __launch_bounds__(kEjFinalWg) void ejoint_final(const EjArgs a)
{
    const long long i = (long long)blockIdx.x * kEjFinalWg + threadIdx.x;
    if (i >= (long long)a.rows_out * a.R) return;
    ejoint_final_lane(a, (int)(i / a.R), (int)(i % a.R));
}

// which: 0 = ejoint_members, 1 = ejoint_vario (both hold the item's P = 64 NV positions in registers)
template <int NV>
inline hipError_t ejoint_launch_nv(int which, const EjArgs &g, unsigned blocks, hipStream_t st)
{
    if (which == 0 && g.f32) hipLaunchKernelGGL((ejoint_members<NV, float>), dim3(blocks), dim3(64), 0, st, g);
    else if (which == 0) hipLaunchKernelGGL((ejoint_members<NV, double>), dim3(blocks), dim3(64), 0, st, g);
    else if (g.f32) hipLaunchKernelGGL((ejoint_vario<NV, float>), dim3(blocks), dim3(64), 0, st, g);
    else hipLaunchKernelGGL((ejoint_vario<NV, double>), dim3(blocks), dim3(64), 0, st, g);
    return hipGetLastError();
}

inline hipError_t ejoint_launch(int which, const EjArgs &g, unsigned blocks, hipStream_t st)
{
    if (which == 2) {
        if (g.f32) hipLaunchKernelGGL(ejoint_pairs<float>, dim3(blocks), dim3(64), 0, st, g);
        else hipLaunchKernelGGL(ejoint_pairs<double>, dim3(blocks), dim3(64), 0, st, g);
        return hipGetLastError();
    }
    if (g.D <= 64) return ejoint_launch_nv<1>(which, g, blocks, st);  // registers per lane: P / 64, P the power of two >= D
    if (g.D <= 128) return ejoint_launch_nv<2>(which, g, blocks, st);
    if (g.D <= 256) return ejoint_launch_nv<4>(which, g, blocks, st);
    if (g.D <= 512) return ejoint_launch_nv<8>(which, g, blocks, st);
    if (g.D <= 1024) return ejoint_launch_nv<16>(which, g, blocks, st);
    if (g.D <= 2048) return ejoint_launch_nv<32>(which, g, blocks, st);
    return ejoint_launch_nv<64>(which, g, blocks, st);
}
#endif

// the workspace, in this order: tsum [items], tile [items][tiles], vrow [items][wcap] (doubles), mask [items][nb] (64-bit words),
// n_mem, n_day [items], days [items][wcap] (int32); laid out for every call alike, whichever outputs are asked for
inline size_t ejoint_ws_size(size_t items, size_t nb, size_t tiles, size_t wcap)
{
    return items * ((1 + tiles + wcap + nb) * 8 + (2 + wcap) * 4);
}

// g.nb, g.tiles, g.wcap are set; pairs / vario: the tile sums / the v_s are asked for (else their pointers stay NULL)
inline void ejoint_carve(EjArgs &g, void *ws, size_t items, bool pairs, bool vario)
{
    double *wd = (double *)ws;
    g.tsum = wd; wd += items;
    g.tile = pairs ? wd : nullptr; wd += items * (size_t)g.tiles;
    g.vrow = vario ? wd : nullptr; wd += items * (size_t)g.wcap;
    g.mask = (unsigned long long *)wd; wd += items * (size_t)g.nb;
    g.n_mem = (int32_t *)wd; g.n_day = g.n_mem + items; g.days = g.n_day + items;
}

// the launches of one kernel over `units` units, at most `cap` in each: launch(first unit, units of the launch) until one fails
template <typename F>
inline int ejoint_for_units(long long units, long long cap, F launch)
{
    for (long long u0 = 0; u0 < units; u0 += cap) {
        const int e = launch(u0, units - u0 < cap ? units - u0 : cap);
        if (e) return e;
    }
    return 0;
}

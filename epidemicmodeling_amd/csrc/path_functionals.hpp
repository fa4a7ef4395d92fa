// Path functionals of the Monte-Carlo ensembles: an array of N = R * D joint paths (region-major, what ens_summary.hpp takes) ->
// per path and row the peak (value and first day), the minimum, the blocked total, and per threshold the first crossing, the days
// above and the longest run above; per (row, region) the histograms of the peak day and of the first crossing over the paths.
// Included by epiekf.hip after ens_score.hpp (entry point epi_pathfn_run_device, include/epiekf.h).  DESIGN.md §4.18 pins the
// arithmetic; tests/pathfn_ref.py and tests/pathfn_ref.c restate it and the GPU suite holds them to the same bits.
//
//   pathfn_paths<F32, NT, NR, SEG>  one lane per path, consecutive paths on consecutive lanes (a wave's day-row is one 512 B run of
//                   doubles); grid.y the time segments, grid.z the row groups.  NR = 4: rows 0, 1, 2 and the derived row
//                   ((N v0) v1) v2 in ONE lane, each value loaded once; NR = 1: one row, which nothing ties to another (every
//                   value is still read once, and the independent rows are further waves).  The loads do not depend on the
//                   running state: they are issued non-temporally kPfPrefetch days ahead through a register ring with
//                   compile-time indices.  NT bounds n_thr at compile time; every state is a scalar of an unrolled loop (no
//                   indexed register array, no scratch).  Every element offset is 64-bit.
//   pathfn_combine<NT>  (more than one segment) one lane per (path, row): folds the segments' partial records ascending.  Every
//                   quantity combines exactly: max / min with the first index, integer counts, runs as (prefix, suffix, best,
//                   length), and the total as the block sums added in block order ACROSS segment borders.
//   pathfn_regions  one workgroup per (histogram, row, region): integer bins in LDS (LDS integer adds), then written out.  No
//                   global atomics of any kind.
//
// Host-compilation contract (loglik.hpp): the bodies of pathfn_paths and pathfn_combine are the EPI_DEV functions pathfn_path_lane
// and pathfn_combine_lane of their indices; tests/pathfn_emu.cpp compiles them with the host compiler (EPI_PATHFN_HOST: without
// the kernels) and calls them lane by lane.
#pragma once

constexpr int kPfMaxThr = 8;                              // thresholds of one call
constexpr int kPfBlock = 32;                              // days of one block of the total (part of the definition)
constexpr int kPfPrefetch = 8, kPfPrefetchWide = 4;       // days the loads run ahead of their use (NT <= 2, NT > 2); divide kPfBlock
constexpr int kPfPathWg = 256, kPfRegionWg = 256;
constexpr int kPfMaxW = 4096;                             // bins of one histogram in LDS
constexpr int kPfMaxSeg = 1024;
constexpr long long kPfLaunchGroups = 1ll << 22;          // workgroups per launch: a launch's thread count is a 32-bit number

struct PfArgs {
    int T, rows, rows_out, R, D, n_thr, derive, k0, k1;
    int nseg, seg_days, nblk;               // segments, days of a segment (a multiple of kPfBlock), blocks of the window
    int row0;                               // NR = 1: the row of grid.z = 0
    long long group0;                       // first workgroup of this launch
    const void *src;                        // [T][rows][N], double or float
    const double *population;               // [R] (derive)
    const double *thr;                      // [n_thr][rows_out][R]
    const int32_t *first_day;               // [R] or NULL (0)
    double *peak_value, *peak_day, *min_value, *min_day, *total;   // [rows_out][N]: outputs (peak_day: or workspace) or NULL
    double *first_cross, *days_above, *longest_run;                // [n_thr][rows_out][N]
    int32_t *n_valid;                       // [rows_out][N]
    int32_t *n_paths, *peak_day_hist;       // [rows_out][R], [W][rows_out][R]
    int32_t *n_cross, *cross_day_hist;      // [n_thr][rows_out][R], [W][n_thr][rows_out][R]
    // the segments' partial records (nseg > 1), M = rows_out * N elements per plane
    double *p_mx, *p_mn;                    // [nseg][M]
    double *p_bsum;                         // [nblk][M]
    int32_t *p_int;                         // [nseg][3][M]: peak day, min day, valid days
    int32_t *p_thr;                         // [nseg][5][n_thr][M]: first, count, prefix run, suffix run, best run
};

struct PfRow { double mx, mn; int mxd, mnd, nv; };
struct PfThr { int first, cnt, cur, best, pre; };

template <int F32>
EPI_DEV double pf_ld(const void *p, size_t o)
{
    return F32 ? (double)__builtin_nontemporal_load((const float *)p + o) : __builtin_nontemporal_load((const double *)p + o);
}

// days t0 <= t < t1 of segment s
EPI_DEV void pf_segment(const PfArgs &a, int s, int &t0, int &t1)
{
    const long long b = (long long)a.k0 + (long long)s * a.seg_days, e = b + a.seg_days;
    t0 = (int)(b < a.k1 ? b : a.k1);
    t1 = (int)(e < a.k1 ? e : a.k1);
}

// ---- what a (path, row) and a (path, row, threshold) end as ----
EPI_DEV void pf_store_row(const PfArgs &a, size_t m, const PfRow &r, double tot)
{
    const double qnan = __builtin_nan("");
    const bool any = r.nv > 0;
    if (a.peak_value) a.peak_value[m] = any ? r.mx : qnan;
    if (a.peak_day) a.peak_day[m] = any ? (double)r.mxd : qnan;
    if (a.min_value) a.min_value[m] = any ? r.mn : qnan;
    if (a.min_day) a.min_day[m] = any ? (double)r.mnd : qnan;
    if (a.total) a.total[m] = any ? tot : qnan;
    if (a.n_valid) a.n_valid[m] = r.nv;
}

EPI_DEV void pf_store_thr(const PfArgs &a, size_t mj, bool asked, int first, int cnt, int best)
{
    const double qnan = __builtin_nan("");
    if (a.first_cross) a.first_cross[mj] = asked && first >= 0 ? (double)first : qnan;
    if (a.days_above) a.days_above[mj] = asked ? (double)cnt : qnan;
    if (a.longest_run) a.longest_run[mj] = asked ? (double)best : qnan;
}

// ---- one path, one segment, one row group: q0 the row (NR = 1); NR = 4: rows 0, 1, 2 and the derived row a.rows ----
// SEG 0: the whole window in one segment (a.nseg = 1), the prefix runs are not kept
template <int F32, int NT, int NR, int SEG>
EPI_DEV void pathfn_path_lane(const PfArgs &a, size_t p, int s, int q0)
{
    constexpr int PF = NT > 2 ? kPfPrefetchWide : kPfPrefetch, NL = NR == 4 ? 3 : 1;     // NL: rows loaded
    static_assert(kPfBlock % PF == 0, "a block is whole chunks of the ring");
    const size_t N = (size_t)a.R * (size_t)a.D, rows = (size_t)a.rows;
    const int r = (int)(p / (size_t)a.D);
    const int fd = a.first_day ? a.first_day[r] : 0;
    const int lo = a.k0 > fd ? a.k0 : fd;
    int t0, t1;
    pf_segment(a, s, t0, t1);
    const double qnan = __builtin_nan("");
    const double Np = NR == 4 ? a.population[r] : 0.0;
    int q[NR];
#pragma unroll
    for (int i = 0; i < NR; i++) q[i] = NR == 4 ? (i < 3 ? i : a.rows) : q0;
    double thr[NR][NT > 0 ? NT : 1];
    PfThr ts[NR][NT > 0 ? NT : 1];
    PfRow rs[NR];
    double tot[NR];
#pragma unroll
    for (int i = 0; i < NR; i++) {
        rs[i].mx = rs[i].mn = 0.0;
        rs[i].mxd = rs[i].mnd = -1;
        rs[i].nv = 0;
        tot[i] = 0.0;
#pragma unroll
        for (int j = 0; j < NT; j++) {
            thr[i][j] = j < a.n_thr ? a.thr[((size_t)j * (size_t)a.rows_out + (size_t)q[i]) * (size_t)a.R + (size_t)r] : qnan;
            ts[i][j].first = -1;
            ts[i][j].cnt = ts[i][j].cur = ts[i][j].best = 0;
            ts[i][j].pre = -1;
        }
    }
    // the ring: the values of day t0 + c PF + i sit in slot i; a day past the segment is the segment's last day, loaded and dropped
    const size_t base = (size_t)(NR == 4 ? 0 : q0) * N + p, day = rows * N;
    double ring[PF][NL];
    if (t0 < t1) {
#pragma unroll
        for (int i = 0; i < PF; i++) {
            const int tt = t0 + i < t1 ? t0 + i : t1 - 1;
#pragma unroll
            for (int l = 0; l < NL; l++) ring[i][l] = pf_ld<F32>(a.src, (size_t)tt * day + base + (size_t)l * N);
        }
    }
    for (int tb = t0; tb < t1; tb += kPfBlock) {
        double bs[NR];
#pragma unroll
        for (int i = 0; i < NR; i++) bs[i] = 0.0;
        for (int c = 0; c < kPfBlock; c += PF) {
            if (tb + c >= t1) break;
#pragma unroll
            for (int k = 0; k < PF; k++) {
                const int t = tb + c + k;
                double v[NR];
#pragma unroll
                for (int l = 0; l < NL; l++) v[l] = ring[k][l];
                if (NR == 4) v[3] = ((Np * v[0]) * v[1]) * v[2];
                const int tn = t + PF < t1 ? t + PF : t1 - 1;          // t1 >= 1 here
#pragma unroll
                for (int l = 0; l < NL; l++) ring[k][l] = pf_ld<F32>(a.src, (size_t)tn * day + base + (size_t)l * N);
                const bool in = t < t1 && t >= lo;
#pragma unroll
                for (int i = 0; i < NR; i++) {
                    const double x = v[i];
                    const bool ok = in && x == x;
                    const bool gt = ok && (rs[i].nv == 0 || x > rs[i].mx), lt = ok && (rs[i].nv == 0 || x < rs[i].mn);
                    rs[i].mx = gt ? x : rs[i].mx;
                    rs[i].mxd = gt ? t : rs[i].mxd;
                    rs[i].mn = lt ? x : rs[i].mn;
                    rs[i].mnd = lt ? t : rs[i].mnd;
                    rs[i].nv += ok ? 1 : 0;
                    bs[i] = ok ? bs[i] + x : bs[i];
#pragma unroll
                    for (int j = 0; j < NT; j++) {
                        PfThr &h = ts[i][j];
                        const bool ab = ok && x >= thr[i][j];
                        const bool live = t < t1;                       // a day past the segment is no day: it breaks no run
                        h.first = ab && h.first < 0 ? t : h.first;
                        h.cnt += ab ? 1 : 0;
                        if (SEG) h.pre = live && !ab && h.pre < 0 ? h.cur : h.pre;
                        h.cur = ab ? h.cur + 1 : (live ? 0 : h.cur);
                        h.best = h.cur > h.best ? h.cur : h.best;
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NR; i++) {
            tot[i] = tot[i] + bs[i];
            if (SEG) a.p_bsum[(size_t)((tb - a.k0) / kPfBlock) * ((size_t)a.rows_out * N) + (size_t)q[i] * N + p] = bs[i];
        }
    }
    const size_t M = (size_t)a.rows_out * N;
#pragma unroll
    for (int i = 0; i < NR; i++) {
        const size_t m = (size_t)q[i] * N + p;
        if (SEG) {
            a.p_mx[(size_t)s * M + m] = rs[i].mx;
            a.p_mn[(size_t)s * M + m] = rs[i].mn;
            int32_t *pi = a.p_int + (size_t)s * 3 * M + m;
            pi[0] = rs[i].mxd; pi[M] = rs[i].mnd; pi[2 * M] = rs[i].nv;
#pragma unroll
            for (int j = 0; j < NT; j++) {
                if (j >= a.n_thr) continue;
                const PfThr &h = ts[i][j];
                int32_t *pt = a.p_thr + ((size_t)s * 5 * (size_t)a.n_thr + (size_t)j) * M + m;
                const size_t f = (size_t)a.n_thr * M;
                pt[0] = h.first; pt[f] = h.cnt; pt[2 * f] = h.pre < 0 ? h.cur : h.pre; pt[3 * f] = h.cur; pt[4 * f] = h.best;
            }
        } else {
            pf_store_row(a, m, rs[i], tot[i]);
#pragma unroll
            for (int j = 0; j < NT; j++) {
                if (j >= a.n_thr) continue;
                const bool asked = rs[i].nv > 0 && thr[i][j] == thr[i][j];
                pf_store_thr(a, (size_t)j * M + m, asked, ts[i][j].first, ts[i][j].cnt, ts[i][j].best);
            }
        }
    }
}

// ---- one (path, row): the segments' records folded ascending ----
template <int NT>
EPI_DEV void pathfn_combine_lane(const PfArgs &a, size_t p, int q)
{
    const size_t N = (size_t)a.R * (size_t)a.D, M = (size_t)a.rows_out * N, m = (size_t)q * N + p;
    const int r = (int)(p / (size_t)a.D);
    PfRow c;
    c.mx = c.mn = 0.0;
    c.mxd = c.mnd = -1;
    c.nv = 0;
    int first[NT > 0 ? NT : 1], cnt[NT > 0 ? NT : 1], cur[NT > 0 ? NT : 1], best[NT > 0 ? NT : 1];
#pragma unroll
    for (int j = 0; j < NT; j++) { first[j] = -1; cnt[j] = cur[j] = best[j] = 0; }
    for (int s = 0; s < a.nseg; s++) {
        int t0, t1;
        pf_segment(a, s, t0, t1);
        const int len = t1 - t0;
        const int32_t *pi = a.p_int + (size_t)s * 3 * M + m;
        const int nv = pi[2 * M];
        const double mx = a.p_mx[(size_t)s * M + m], mn = a.p_mn[(size_t)s * M + m];
        const bool gt = nv > 0 && (c.nv == 0 || mx > c.mx), lt = nv > 0 && (c.nv == 0 || mn < c.mn);
        c.mx = gt ? mx : c.mx;
        c.mxd = gt ? pi[0] : c.mxd;
        c.mn = lt ? mn : c.mn;
        c.mnd = lt ? pi[M] : c.mnd;
        c.nv += nv;
#pragma unroll
        for (int j = 0; j < NT; j++) {
            if (j >= a.n_thr) continue;
            const int32_t *pt = a.p_thr + ((size_t)s * 5 * (size_t)a.n_thr + (size_t)j) * M + m;
            const size_t f = (size_t)a.n_thr * M;
            const int f_s = pt[0], pre = pt[2 * f], suf = pt[3 * f], b_s = pt[4 * f];
            first[j] = first[j] < 0 ? f_s : first[j];
            cnt[j] += pt[f];
            const int joined = cur[j] + pre;
            best[j] = joined > best[j] ? joined : best[j];
            best[j] = b_s > best[j] ? b_s : best[j];
            cur[j] = pre == len ? joined : suf;                       // a segment above on every day extends the run through it
        }
    }
    double tot = 0.0;
    for (int b = 0; b < a.nblk; b++) tot = tot + a.p_bsum[(size_t)b * M + m];
    pf_store_row(a, m, c, tot);
#pragma unroll
    for (int j = 0; j < NT; j++) {
        if (j >= a.n_thr) continue;
        const double th = a.thr[((size_t)j * (size_t)a.rows_out + (size_t)q) * (size_t)a.R + (size_t)r];
        pf_store_thr(a, (size_t)j * M + m, c.nv > 0 && th == th, first[j], cnt[j], best[j]);
    }
}

#ifndef EPI_PATHFN_HOST
template <int F32, int NT, int NR, int SEG>
__global__ __launch_bounds__(kPfPathWg) void pathfn_paths(const PfArgs a)
{
    const size_t p = ((size_t)a.group0 + (size_t)blockIdx.x) * kPfPathWg + threadIdx.x;
    if (p >= (size_t)a.R * (size_t)a.D) return;
    pathfn_path_lane<F32, NT, NR, SEG>(a, p, (int)blockIdx.y, a.row0 + (int)blockIdx.z);
}

template <int NT>
__global__ __launch_bounds__(kPfPathWg) void pathfn_combine(const PfArgs a)
{
    const size_t p = ((size_t)a.group0 + (size_t)blockIdx.x) * kPfPathWg + threadIdx.x;
    if (p >= (size_t)a.R * (size_t)a.D) return;
    pathfn_combine_lane<NT>(a, p, (int)blockIdx.y);
}

// workgroup (h, q, r): h = 0 the peak day, h >= 1 the first crossing of threshold h - 1; a NaN day is a path that has none
__global__ __launch_bounds__(kPfRegionWg) void pathfn_regions(const PfArgs a)
{
    __shared__ int32_t bins[kPfMaxW + 1];
    const int W = a.k1 - a.k0;
    const long long g = a.group0 + (long long)blockIdx.x;
    const int r = (int)(g % a.R), q = (int)((g / a.R) % a.rows_out), h = (int)(g / ((long long)a.R * a.rows_out));
    const size_t N = (size_t)a.R * (size_t)a.D, M = (size_t)a.rows_out * N, plane = (size_t)a.rows_out * (size_t)a.R;
    const size_t col = (size_t)q * (size_t)a.R + (size_t)r;
    int32_t *cnt_out = h == 0 ? a.n_paths : a.n_cross;
    int32_t *hist_out = h == 0 ? a.peak_day_hist : a.cross_day_hist;
    if (!cnt_out && !hist_out) return;
    const int nb = hist_out ? W : 0;                                   // n_paths / n_cross alone need no bins: any W (validate bounds a histogram's)
    for (int b = threadIdx.x; b < nb; b += kPfRegionWg) bins[b] = 0;
    if (threadIdx.x == 0) bins[kPfMaxW] = 0;
    __syncthreads();
    const double *day = h == 0 ? a.peak_day + (size_t)q * N + (size_t)r * (size_t)a.D
                               : a.first_cross + (size_t)(h - 1) * M + (size_t)q * N + (size_t)r * (size_t)a.D;
    for (int d = threadIdx.x; d < a.D; d += kPfRegionWg) {
        const double t = day[d];
        if (t == t) {
            int b = (int)t - a.k0;
            b = b < 0 ? 0 : (b >= W ? W - 1 : b);                      // k0 <= t < k1 by construction: the LDS index stays inside
            if (hist_out) atomicAdd(&bins[b], 1);
            atomicAdd(&bins[kPfMaxW], 1);
        }
    }
    __syncthreads();
    if (h == 0) {
        if (cnt_out && threadIdx.x == 0) cnt_out[col] = bins[kPfMaxW];
        if (hist_out)
            for (int b = threadIdx.x; b < W; b += kPfRegionWg) hist_out[(size_t)b * plane + col] = bins[b];
    } else {
        const size_t j = (size_t)(h - 1);
        if (cnt_out && threadIdx.x == 0) cnt_out[j * plane + col] = bins[kPfMaxW];
        if (hist_out)
            for (int b = threadIdx.x; b < W; b += kPfRegionWg) hist_out[((size_t)b * (size_t)a.n_thr + j) * plane + col] = bins[b];
    }
}
#endif

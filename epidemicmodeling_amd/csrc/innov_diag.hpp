// Whiteness diagnostics of the innovations of every chain: serial correlation (autocorrelations, Ljung-Box), moments (skewness,
// kurtosis, Jarque-Bera), the NIS sum, a first-third / last-third variance ratio, the CUSUM of squares and the largest value,
// from the innovations as the runner wrote them (classic or chain-blocked, double or float) and the per-day innovation
// variance S that epi_loglik_run_device writes (or none: the series is taken as standardised); included by epiekf.hip (entry
// point epi_idiag_run_device, include/epiekf.h).  DESIGN.md §4.22 pins the arithmetic; tests/innov_diag_ref.c restates it and
// the GPU suite holds the two to the same bits.
//
//   id_blocks1  one lane per (chain, block of 32 filter steps): nu = e / sqrt(S) of every step that counts; the block's count,
//               sum of nu and of nu nu from 0.0 in ascending k, and whether a bad day lies in it.
//   id_chains1  one lane per chain adds the block records in ascending order from 0.0: n, the mean, q = the NIS sum, and per
//               block the q and the count of the complete earlier blocks (the CUSUM's prefix).
//   id_blocks2  one lane per (chain, block): d = nu - mean of the block's rows and of the H rows after them go into the lane's
//               own column of an LDS tile [32 + H][64] (a row is read by the 64 lanes as one conflict-free run of doubles; no
//               lane reads another's column, so no barrier), the block's 32 also stay in registers; the central moments, the
//               two thirds, the largest value, the CUSUM of squares, and per lag h the block's sum of d(k) d(k+h) -- the
//               term belongs to k's block -- with the second factor read from LDS.
//   id_chains2  one lane per chain adds the block records in ascending order and forms every output.
//
// Because the order of every sum is fixed by the 32-step blocks, the time-parallel kernels give the bits of a sequential walk.
// Chains are the fastest index everywhere, so a wavefront's load of one row is one contiguous run; non-temporal loads through
// 64-bit element offsets.  No register array is indexed dynamically (the 32 rows of a block are unrolled), so neither block
// kernel uses scratch.
//
// Host-compilation contract (as loglik.hpp): each kernel's body is an EPI_DEV function of its own indices (id_*_lane);
// tests/innov_diag_emu.cpp compiles them with the host compiler and calls them one lane at a time, the LDS column being a plain
// array of stride 1.  The __global__ wrappers below them only compute the indices.
#pragma once

constexpr int kIdBlock = 32;                              // filter steps per summation block (part of the definition)
constexpr int kIdMaxLags = 64;
constexpr int kIdBadDay = 1, kIdEmpty = 2, kIdDegenerate = 4, kIdFewLags = 8;   // bits of status

struct IdArgs {
    int B, T, H, lags, f32, flip, k0, k1, nb32, h3;       // lags: H if an output needs the lagged products, else 0
    size_t bp;                                            // elements per day of e: nblk * blk (ll_geometry)
    const void *e;
    const double *S;                                      // [T][B] by day, or NULL
    double *p_sum, *p_q;                                  // pass 1, [nb32][B]
    int32_t *p_n, *p_bad;
    double *pre_q;                                        // [nb32][B]: q and count of the complete earlier blocks
    int32_t *pre_n;
    double *c_mean, *c_q;                                 // [B]
    int32_t *c_n, *c_bad;
    double *r_m2, *r_m3, *r_m4, *r_f, *r_l, *r_max, *r_cs;   // pass 2, [nb32][B]
    int32_t *r_nf, *r_nl, *r_maxk, *r_csk;
    double *r_c;                                          // [nb32][H][B]
    double *mean, *var, *skew, *kurt, *jb, *nis_sum, *nis_mean, *lb_q, *het, *cusumsq_max, *max_abs;   // [B] or NULL
    int32_t *n, *lb_lags, *het_n1, *het_n2, *cusumsq_step, *max_abs_step, *status;
    double *acf;                                          // [H][B] or NULL
};

// filter step k (k0 <= k < k1) of chain c: 0 and *nu if the step counts, 1 if it is skipped silently, 2 if it is a bad day
EPI_DEV int id_nu(const IdArgs &a, int c, int k, double *nu)
{
    const size_t t = (size_t)(a.flip ? (a.T - 1 - k) : k);
    const double e = ll_ld(a.e, t * a.bp + c, a.f32);
    if (a.S) {
        const double S = __builtin_nontemporal_load(a.S + (t * (size_t)a.B + c));
        if (is_nan(S)) return 1;
        if (is_nonfinite(S) || S < kLlDblMin || is_nonfinite(e)) return 2;
        *nu = e / sqrt(S);
        return 0;
    }
    if (is_nan(e)) return 1;
    if (is_nonfinite(e)) return 2;
    *nu = e;
    return 0;
}

// the running largest value and its lowest step: `v` at step k replaces `best` when no step is held yet, when it is larger, or when
// it is the first NaN (a NaN, once held, stays: the blocks then combine to what a sequential walk gives)
EPI_DEV bool id_beats(double v, double best, int step) { return step < 0 || v > best || (is_nan(v) && !is_nan(best)); }

// ---- pass 1: one block of 32 filter steps of one chain ----
EPI_DEV void id_block1_lane(const IdArgs &a, int c, int b32)
{
    double sum = 0.0, q = 0.0;
    int n = 0, bad = 0;
    const int kb = b32 * kIdBlock;
    for (int r = 0; r < kIdBlock; r++) {
        const int k = kb + r;
        if (k < a.k0 || k >= a.k1) continue;
        double nu = 0.0;
        const int what = id_nu(a, c, k, &nu);
        if (what == 0) {
            const double nn = nu * nu;
            sum = sum + nu;
            q = q + nn;
            n = n + 1;
        } else if (what == 2) {
            bad = 1;
        }
    }
    const size_t po = (size_t)b32 * (size_t)a.B + c;
    a.p_sum[po] = sum;
    a.p_q[po] = q;
    a.p_n[po] = n;
    a.p_bad[po] = bad;
}

// ---- pass 1: the blocks of one chain, in order ----
EPI_DEV void id_chain1_lane(const IdArgs &a, int c)
{
    double sum = 0.0, q = 0.0;
    int n = 0, bad = 0;
    for (int b = 0; b < a.nb32; b++) {
        const size_t po = (size_t)b * (size_t)a.B + c;
        a.pre_q[po] = q;
        a.pre_n[po] = n;
        sum = sum + a.p_sum[po];
        q = q + a.p_q[po];
        n = n + a.p_n[po];
        bad = bad | a.p_bad[po];
    }
    a.c_mean[c] = sum / (double)n;
    a.c_q[c] = q;
    a.c_n[c] = n;
    a.c_bad[c] = bad;
}

// ---- pass 2: one block of one chain; col: this lane's column of [32 + H] doubles with element stride `stride` ----
EPI_DEV void id_block2_lane(const IdArgs &a, int c, int b32, double *col, int stride)
{
    const size_t po = (size_t)b32 * (size_t)a.B + c;
    const int n = a.c_n[c];
    const double mean = a.c_mean[c], qtot = a.c_q[c], dn = (double)n, pq = a.pre_q[po];
    const int kb = b32 * kIdBlock, f_end = a.k0 + a.h3, l_beg = a.k1 - a.h3;
    double dk[kIdBlock];
    uint32_t m0 = 0;
    uint64_t mhi = 0;
    double m2 = 0.0, m3 = 0.0, m4 = 0.0, f = 0.0, l = 0.0, mx = 0.0, cs = 0.0, run = 0.0;
    int nf = 0, nl = 0, mxk = -1, csk = -1, j = a.pre_n[po];
#pragma unroll
    for (int r = 0; r < kIdBlock; r++) {
        const int k = kb + r;
        double d = 0.0;
        if (k >= a.k0 && k < a.k1) {
            double nu = 0.0;
            if (id_nu(a, c, k, &nu) == 0) {
                m0 |= 1u << r;
                d = nu - mean;
                const double dd = d * d, nn = nu * nu;
                const double d3 = dd * d, d4 = dd * dd;
                m2 = m2 + dd;
                m3 = m3 + d3;
                m4 = m4 + d4;
                run = run + nn;
                j = j + 1;
                const double prefix = pq + run;
                const double acs = fabs(prefix / qtot - (double)j / dn);
                if (id_beats(acs, cs, csk)) { cs = acs; csk = k; }
                const double an = fabs(nu);
                if (id_beats(an, mx, mxk)) { mx = an; mxk = k; }
                if (k < f_end) { f = f + nn; nf = nf + 1; }
                if (k >= l_beg) { l = l + nn; nl = nl + 1; }
            }
        }
        dk[r] = d;
        col[(size_t)r * stride] = d;
    }
    a.r_m2[po] = m2; a.r_m3[po] = m3; a.r_m4[po] = m4;
    a.r_f[po] = f; a.r_l[po] = l; a.r_nf[po] = nf; a.r_nl[po] = nl;
    a.r_max[po] = mx; a.r_maxk[po] = mxk;
    a.r_cs[po] = cs; a.r_csk[po] = csk;
    if (a.lags <= 0) return;
    for (int r = kIdBlock; r < kIdBlock + a.lags; r++) {    // the rows the lags reach ahead
        const int k = kb + r;
        double d = 0.0;
        if (k >= a.k0 && k < a.k1) {
            double nu = 0.0;
            if (id_nu(a, c, k, &nu) == 0) {
                mhi |= (uint64_t)1 << (r - kIdBlock);
                d = nu - mean;
            }
        }
        col[(size_t)r * stride] = d;
    }
    const uint64_t mlo = (mhi << 32) | (uint64_t)m0;       // rows 0 .. 63
    for (int h = 1; h <= a.lags; h++) {
        const uint32_t mh = h < 32 ? (uint32_t)(mlo >> h) : (uint32_t)(mhi >> (h - 32));   // rows h .. h + 31
        const uint32_t both = m0 & mh;
        const double *ahead = col + (size_t)h * stride;
        double acc = 0.0;
#pragma unroll
        for (int r = 0; r < kIdBlock; r++) {
            const double p = dk[r] * ahead[(size_t)r * stride];
            const double s = acc + p;
            acc = ((both >> r) & 1u) ? s : acc;
        }
        a.r_c[((size_t)b32 * (size_t)a.H + (size_t)(h - 1)) * (size_t)a.B + c] = acc;
    }
}

// ---- pass 2: the blocks of one chain, in order, and every output ----
EPI_DEV void id_chain2_lane(const IdArgs &a, int c)
{
    const size_t B = (size_t)a.B;
    const double qnan = __builtin_nan("");
    const int n = a.c_n[c];
    const double q = a.c_q[c], mean = a.c_mean[c], dn = (double)n;
    double m2 = 0.0, m3 = 0.0, m4 = 0.0, f = 0.0, l = 0.0, mx = 0.0, cs = 0.0;
    int nf = 0, nl = 0, mxk = -1, csk = -1;
    for (int b = 0; b < a.nb32; b++) {
        const size_t po = (size_t)b * B + c;
        m2 = m2 + a.r_m2[po];
        m3 = m3 + a.r_m3[po];
        m4 = m4 + a.r_m4[po];
        f = f + a.r_f[po];
        l = l + a.r_l[po];
        nf = nf + a.r_nf[po];
        nl = nl + a.r_nl[po];
        const int bk = a.r_maxk[po], ck = a.r_csk[po];
        const double bm = a.r_max[po], cm = a.r_cs[po];
        if (bk >= 0 && id_beats(bm, mx, mxk)) { mx = bm; mxk = bk; }
        if (ck >= 0 && id_beats(cm, cs, csk)) { cs = cm; csk = ck; }
    }
    int st = a.c_bad[c];
    if (n == 0) {
        st = st | kIdEmpty;
        if (a.mean) a.mean[c] = qnan;
        if (a.var) a.var[c] = qnan;
        if (a.skew) a.skew[c] = qnan;
        if (a.kurt) a.kurt[c] = qnan;
        if (a.jb) a.jb[c] = qnan;
        if (a.nis_sum) a.nis_sum[c] = qnan;
        if (a.nis_mean) a.nis_mean[c] = qnan;
        if (a.lb_q) a.lb_q[c] = qnan;
        if (a.het) a.het[c] = qnan;
        if (a.cusumsq_max) a.cusumsq_max[c] = qnan;
        if (a.max_abs) a.max_abs[c] = qnan;
        if (a.n) a.n[c] = 0;
        if (a.lb_lags) a.lb_lags[c] = 0;
        if (a.het_n1) a.het_n1[c] = 0;
        if (a.het_n2) a.het_n2[c] = 0;
        if (a.cusumsq_step) a.cusumsq_step[c] = -1;
        if (a.max_abs_step) a.max_abs_step[c] = -1;
        if (a.status) a.status[c] = st;
        if (a.acf)
            for (int h = 1; h <= a.H; h++) a.acf[(size_t)(h - 1) * B + c] = qnan;
        return;
    }
    const bool deg = (m2 == 0.0) || is_nonfinite(m2);
    const int Hu = a.H < n - 1 ? a.H : n - 1;
    if (deg) st = st | kIdDegenerate;
    if (Hu < a.H) st = st | kIdFewLags;
    const double var = m2 / dn;
    const double sd = sqrt(var);
    const double skew = (m3 / dn) / (var * sd), kurt = (m4 / dn) / (var * var);
    const double k3 = kurt - 3.0;
    const double jb = (dn / 6.0) * (skew * skew + (k3 * k3) / 4.0);
    double lbsum = 0.0;
    for (int h = 1; h <= a.lags; h++) {
        double ac = qnan;
        if (h <= Hu && !deg) {
            double ch = 0.0;
            for (int b = 0; b < a.nb32; b++) ch = ch + a.r_c[((size_t)b * (size_t)a.H + (size_t)(h - 1)) * B + c];
            ac = ch / m2;
            lbsum = lbsum + (ac * ac) / (double)(n - h);
        }
        if (a.acf) a.acf[(size_t)(h - 1) * B + c] = ac;
    }
    double lb = (dn * (double)(n + 2)) * lbsum;
    if (deg || (Hu < a.H && Hu == 0)) lb = qnan;
    if (a.mean) a.mean[c] = mean;
    if (a.var) a.var[c] = var;
    if (a.skew) a.skew[c] = deg ? qnan : skew;
    if (a.kurt) a.kurt[c] = deg ? qnan : kurt;
    if (a.jb) a.jb[c] = deg ? qnan : jb;
    if (a.nis_sum) a.nis_sum[c] = q;
    if (a.nis_mean) a.nis_mean[c] = q / dn;
    if (a.lb_q) a.lb_q[c] = lb;
    if (a.het) a.het[c] = (nf == 0 || nl == 0) ? qnan : (l / (double)nl) / (f / (double)nf);
    if (a.cusumsq_max) a.cusumsq_max[c] = cs;
    if (a.max_abs) a.max_abs[c] = mx;
    if (a.n) a.n[c] = n;
    if (a.lb_lags) a.lb_lags[c] = Hu;
    if (a.het_n1) a.het_n1[c] = nf;
    if (a.het_n2) a.het_n2[c] = nl;
    if (a.cusumsq_step) a.cusumsq_step[c] = csk;
    if (a.max_abs_step) a.max_abs_step[c] = mxk;
    if (a.status) a.status[c] = st;
}

#ifndef EPI_IDIAG_HOST
// the grids are flat: workgroup w covers the chains of tile w % tiles of block w / tiles (ceil(T / 32) may pass 65535)
__global__ __launch_bounds__(256) void id_blocks1(const IdArgs a, const unsigned tiles)
{
    const long long c = (long long)(blockIdx.x % tiles) * 256 + threadIdx.x;
    if (c >= a.B) return;
    id_block1_lane(a, (int)c, (int)(blockIdx.x / tiles));
}
__global__ __launch_bounds__(256) void id_chains1(const IdArgs a)
{
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.B) return;
    id_chain1_lane(a, (int)c);
}
__global__ __launch_bounds__(kWave) void id_blocks2(const IdArgs a, const unsigned tiles)
{
    extern __shared__ double lds[];                        // [32 + lags][64], one column per lane
    const long long c = (long long)(blockIdx.x % tiles) * kWave + threadIdx.x;
    if (c >= a.B) return;
    id_block2_lane(a, (int)c, (int)(blockIdx.x / tiles), lds + threadIdx.x, kWave);
}
__global__ __launch_bounds__(256) void id_chains2(const IdArgs a)
{
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.B) return;
    id_chain2_lane(a, (int)c);
}
#endif

// The two fitrsvm rows of the reference's predictor block (testScripts/test05DirectNewCasesLearning.m:198-268,
// test04FullFeatureExtMLpipeline.m:435-445, test03ExpfitVsIPRegression.m:242-262): the epsilon-insensitive support-vector
// regression QP, linear or Gaussian kernel, solved by LIBSVM's sequential minimal optimisation in its 2n-variable form; one item
// per (row count k, region r).  Included by epiekf.hip (entry point epi_svr_run_device, include/epiekf.h).  DESIGN.md §4.13 pins
// the arithmetic; tests/svr_ref.c and tests/svr_ref.py restate it and the suites hold all three to the same bits.
//
// svr_items<NR, GAU>: one workgroup of 256 lanes per item.  The used rows of X lie in LDS for the whole solve, row-major with
// the odd stride S = F | 1 doubles, so that the rows a wave reads side by side start in different bank pairs.  Lane l owns the
// data rows l, l + 256, .. (NR of them): their two gradient entries, alpha, alpha* and K(k,k) stay in registers.  An iteration
// is: the maximal violator i and M(alpha) by a lane-local scan, a wave reduction by shuffles and a merge of the four waves'
// slots in LDS (the winner's owner adds alpha_i and K(i,i) to its wave's slot); column i from LDS; the second-order choice of
// j the same way (its owner adds -s_j G_j, alpha_j, K(j,j) and K(i,j)); column j; the analytic pair step in every lane; the
// two fma updates.  Two barriers per iteration: the two slot regions alternate, so a region is rewritten only after the other
// region's barrier.  Maximum and minimum are exact and ties go to the lowest variable index, so the lane order cannot matter.
// Every branch around a barrier is uniform.  No atomics, no scratch, no host synchronisation.
#pragma once

constexpr int kSvMaxF = 96, kSvThreads = 256, kSvWaves = kSvThreads / 64, kSvRowCounts = 64;
constexpr int kSvMaxRows = 4 * kSvThreads;  // n_rows <= 1024: at most NR = 4 data rows per lane
constexpr int kSvMaxElems = 20000;          // max(n_rows) (S + 1): the staged rows and the beta column beside them
constexpr int kSvSlot = 6, kSvRed = 2 * kSvWaves * kSvSlot;
// doubles before beta: the slots [2][4][6], w [96], the lanes' counts (256 ints), 2 flags; rounded up
constexpr int kSvAux = 280;
constexpr int kSvLdsDoubles = 20480;        // 160 KiB
constexpr int kSvNotConverged = 1, kSvBadInput = 2, kSvNonfinite = 4;              // epi_svr_status_bits
constexpr double kSvTau = 1e-12;            // LIBSVM's TAU: what a non-positive curvature is replaced by
// workgroups per launch: a launch's thread count (workgroups x 256 lanes) is a 32-bit number in the HIP runtime (lasso.hpp)
constexpr int64_t kSvLaunchItems = (int64_t)1 << 22;

struct SvArgs {
    int D, F, R;
    int k0;                                // the first row count of this launch
    long long item0;                       // the first item of this launch within its row counts: item = kk * R + r
    int nr[kSvRowCounts];                  // n_rows[k0 + kk]
    int max_iter;
    int lds;                               // doubles of dynamic LDS the launch was given
    double tol;
    const double *X, *y;                   // [D][F][R], [D][R]
    const double *box, *eps, *scale;       // [R]
    double *beta, *bias, *w, *fitted, *gap;
    int32_t *n_iter, *n_sv, *status;
};

EPI_DEV bool sv_finite(double v) { return fabs(v) < (double)INFINITY; }

#ifndef SV_HOST_WAVE
// the best (largest value, then lowest index) pair of the wave, in every lane
EPI_DEV void sv_wave_best(double &v, int &i)
{
    for (int m = 32; m; m >>= 1) {
        const double v2 = __shfl_xor(v, m);
        const int i2 = __shfl_xor(i, m);
        if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
    }
}
EPI_DEV double sv_wave_max(double v)
{
    for (int m = 32; m; m >>= 1) {
        const double v2 = __shfl_xor(v, m);
        if (v2 > v) v = v2;
    }
    return v;
}
#endif

// K(a, b) over f ascending; a has the element stride sa (a row of X in HBM has R), b is a row in LDS
template <bool GAU>
EPI_DEV double sv_kval(const double *a, size_t sa, const double *b, int F, double s2)
{
    if (GAU) {
        double t = a[0] - b[0], d = t * t;
        for (int f = 1; f < F; f++) {
            t = a[(size_t)f * sa] - b[f];
            d = fma(t, t, d);
        }
        return epi_exp(-(d / s2));
    }
    double acc = a[0] * b[0];
    for (int f = 1; f < F; f++) acc = fma(a[(size_t)f * sa], b[f], acc);
    return acc;
}

// the merge of the four waves' slots: value, index (the lowest on a tie)
EPI_DEV int sv_merge(const double *slot, double &best)
{
    int w = 0;
    for (int q = 1; q < kSvWaves; q++) {
        const double v = slot[q * kSvSlot], bv = slot[w * kSvSlot];
        if (v > bv || (v == bv && slot[q * kSvSlot + 1] < slot[w * kSvSlot + 1])) w = q;
    }
    best = slot[w * kSvSlot];
    return w;
}

// doubles of dynamic LDS a launch needs: the largest item, and for the Gaussian kernel room for up to 256 prediction rows
inline size_t sv_lds_doubles(int nmax, int nmin, int D, int F, bool gau)
{
    const size_t S = (size_t)(F | 1);
    size_t v = (size_t)kSvAux + (size_t)nmax * (S + 1);
    if (gau && D > nmin) v += (size_t)(D - nmin < kSvThreads ? D - nmin : kSvThreads) * S;
    return v < (size_t)kSvLdsDoubles ? v : (size_t)kSvLdsDoubles;
}

extern __shared__ double sv_lds[];

template <int NR, bool GAU>
__global__ __launch_bounds__(kSvThreads) void svr_items(const SvArgs g)
{
    const int tid = threadIdx.x, lane = tid % 64, wave = tid / 64, D = g.D, F = g.F, S = F | 1;
    const long long item = g.item0 + (long long)blockIdx.x;
    const int kk = (int)(item / g.R), n = g.nr[kk];
    const size_t R = (size_t)g.R, r = (size_t)(item % g.R), k = (size_t)(g.k0 + kk);
    double *red = sv_lds, *wl = red + kSvRed, *bet = sv_lds + kSvAux, *Xs = bet + n, *chunk = Xs + (size_t)n * S;
    int *cnt = (int *)(wl + kSvMaxF), *flag = cnt + kSvThreads;        // [0]: a bad input; [1]: a non-finite result
    const double qnan = __builtin_nan(""), inf = (double)INFINITY;
    const double C = g.box[r], e = g.eps[r], s = g.scale[r], s2 = s * s;
    if (tid < 2) flag[tid] = 0;
    __syncthreads();
    // ---- the used rows of X into LDS; y of the lane's rows into registers ----
    for (int idx = tid; idx < n * F; idx += kSvThreads) {
        const int i = idx / F, f = idx % F;
        const double v = g.X[((size_t)i * (size_t)F + (size_t)f) * R + r];
        Xs[i * S + f] = v;
        if (!sv_finite(v)) flag[0] = 1;
    }
    double Gp[NR], Gm[NR], ap[NR], am[NR], kd[NR];
    for (int q = 0; q < NR; q++) {
        const int row = tid + q * kSvThreads;
        const double yv = row < n ? g.y[(size_t)row * R + r] : 0.0;
        if (!sv_finite(yv)) flag[0] = 1;
        Gp[q] = e - yv;                                                // the linear term of alpha and of alpha*
        Gm[q] = e + yv;
        ap[q] = am[q] = 0.0;
    }
    __syncthreads();
    if (flag[0] || !(C > 0.0 && C < inf) || !(e >= 0.0 && e < inf) || !(s > 0.0 && s < inf)) {     // BAD_INPUT: uniform
        for (int t = tid; t < D; t += kSvThreads) {
            if (g.beta) g.beta[(k * (size_t)D + (size_t)t) * R + r] = qnan;
            if (g.fitted) g.fitted[(k * (size_t)D + (size_t)t) * R + r] = qnan;
        }
        if (g.w && tid < F) g.w[(k * (size_t)F + (size_t)tid) * R + r] = qnan;
        if (tid == 0) {
            if (g.bias) g.bias[k * R + r] = qnan;
            if (g.gap) g.gap[k * R + r] = qnan;
            if (g.n_iter) g.n_iter[k * R + r] = 0;
            if (g.n_sv) g.n_sv[k * R + r] = 0;
            if (g.status) g.status[k * R + r] = kSvBadInput;
        }
        return;
    }
    for (int q = 0; q < NR; q++) {
        const int row = tid + q * kSvThreads;
        kd[q] = row < n ? sv_kval<GAU>(Xs + row * S, 1, Xs + row * S, F, s2) : 0.0;
    }
    // ---- sequential minimal optimisation: variable v < n is alpha_v (sign +1), v >= n is alpha*_(v-n) (sign -1) ----
    int it = 0;
    double gmax, gmin, gap;
    for (;;) {
        // the maximal violator of the up set, and M(alpha) over the low set (as the maximum of the negated values)
        double lv = -inf, la = 0.0, lk = 0.0, lnm = -inf;
        int li = -1;
        for (int q = 0; q < NR; q++) {
            const int row = tid + q * kSvThreads;
            const double val = -Gp[q];
            if (row < n && ap[q] < C && val > lv) { lv = val; li = row; la = ap[q]; lk = kd[q]; }
            if (row < n && ap[q] > 0.0 && -val > lnm) lnm = -val;
        }
        for (int q = 0; q < NR; q++) {
            const int row = tid + q * kSvThreads;
            const double val = Gm[q];
            if (row < n && am[q] > 0.0 && val > lv) { lv = val; li = row + n; la = am[q]; lk = kd[q]; }
            if (row < n && am[q] < C && -val > lnm) lnm = -val;
        }
        double wv = lv;
        int wi = li;
        sv_wave_best(wv, wi);
        const double wm = sv_wave_max(lnm);
        double *sa = red + wave * kSvSlot;
        if (lane == 0) { sa[0] = wv; sa[1] = (double)wi; sa[4] = wm; }
        if (wi >= 0 && wi == li) { sa[2] = la; sa[3] = lk; }
        __syncthreads();
        int win = sv_merge(red, gmax);
        const int i = (int)red[win * kSvSlot + 1];
        const double ai0 = red[win * kSvSlot + 2], kii = red[win * kSvSlot + 3];
        double nm = red[4];
        for (int q = 1; q < kSvWaves; q++) nm = red[q * kSvSlot + 4] > nm ? red[q * kSvSlot + 4] : nm;
        gmin = -nm;
        gap = gmax - gmin;
        if (!(gap >= g.tol) || it == g.max_iter) break;
        const bool si = i < n;
        const int ki = si ? i : i - n;
        // column i, and the second-order choice of j over the low set (the largest b^2 / a, ties to the lowest index)
        double Qi[NR], Qj[NR];
        for (int q = 0; q < NR; q++) {
            const int row = tid + q * kSvThreads;
            Qi[q] = row < n ? sv_kval<GAU>(Xs + row * S, 1, Xs + ki * S, F, s2) : 0.0;
        }
        double lval = 0.0;
        lv = -inf; li = -1; la = 0.0; lk = 0.0;
        double lq = 0.0;
        for (int sgn = 0; sgn < 2; sgn++)
            for (int q = 0; q < NR; q++) {
                const int row = tid + q * kSvThreads;
                const double val = sgn == 0 ? -Gp[q] : Gm[q], b = gmax - val;
                const bool low = sgn == 0 ? ap[q] > 0.0 : am[q] < C;
                if (row < n && low && b > 0.0) {
                    double a = (kii + kd[q]) - 2.0 * Qi[q];
                    if (!(a > 0.0)) a = kSvTau;
                    const double o = (b * b) / a;
                    if (o > lv) { lv = o; li = sgn == 0 ? row : row + n; lval = val; la = sgn == 0 ? ap[q] : am[q]; lk = kd[q]; lq = Qi[q]; }
                }
            }
        wv = lv;
        wi = li;
        sv_wave_best(wv, wi);
        double *sb = red + (kSvWaves + wave) * kSvSlot;
        if (lane == 0) { sb[0] = wv; sb[1] = (double)wi; }
        if (wi >= 0 && wi == li) { sb[2] = lval; sb[3] = la; sb[4] = lk; sb[5] = lq; }
        __syncthreads();
        double obj;
        win = kSvWaves + sv_merge(red + kSvWaves * kSvSlot, obj);
        const int j = (int)red[win * kSvSlot + 1];
        if (j < 0) break;                                              // no descent pair (only with non-finite gradients)
        const double valj = red[win * kSvSlot + 2], aj0 = red[win * kSvSlot + 3], kjj = red[win * kSvSlot + 4], kij = red[win * kSvSlot + 5];
        const bool sj = j < n;
        const int kj = sj ? j : j - n;
        for (int q = 0; q < NR; q++) {
            const int row = tid + q * kSvThreads;
            Qj[q] = row < n ? sv_kval<GAU>(Xs + row * S, 1, Xs + kj * S, F, s2) : 0.0;
        }
        // the analytic step on (alpha_i, alpha_j) with LIBSVM's clipping to the box, in every lane
        const double Gi = si ? -gmax : gmax, Gj = sj ? -valj : valj;
        double quad = (kii + kjj) - 2.0 * kij;
        if (!(quad > 0.0)) quad = kSvTau;
        double ai = ai0, aj = aj0;
        if (si != sj) {
            const double delta = (-Gi - Gj) / quad, diff = ai - aj;
            ai = ai + delta;
            aj = aj + delta;
            if (diff > 0.0) { if (aj < 0.0) { aj = 0.0; ai = diff; } }
            else { if (ai < 0.0) { ai = 0.0; aj = -diff; } }
            if (diff > 0.0) { if (ai > C) { ai = C; aj = C - diff; } }
            else { if (aj > C) { aj = C; ai = C + diff; } }
        } else {
            const double delta = (Gi - Gj) / quad, sum = ai + aj;
            ai = ai - delta;
            aj = aj + delta;
            if (sum > C) { if (ai > C) { ai = C; aj = sum - C; } }
            else { if (aj < 0.0) { aj = 0.0; ai = sum; } }
            if (sum > C) { if (aj > C) { aj = C; ai = sum - C; } }
            else { if (ai < 0.0) { ai = 0.0; aj = sum; } }
        }
        const double dai = ai - ai0, daj = aj - aj0;
        for (int q = 0; q < NR; q++) {
            const int row = tid + q * kSvThreads;
            Gp[q] = fma(si ? Qi[q] : -Qi[q], dai, Gp[q]);
            Gp[q] = fma(sj ? Qj[q] : -Qj[q], daj, Gp[q]);
            Gm[q] = fma(si ? -Qi[q] : Qi[q], dai, Gm[q]);
            Gm[q] = fma(sj ? -Qj[q] : Qj[q], daj, Gm[q]);
            if (row == ki) { if (si) ap[q] = ai; else am[q] = ai; }
            if (row == kj) { if (sj) ap[q] = aj; else am[q] = aj; }
        }
        it++;
    }
    // ---- the bias: LIBSVM's rule ----
    int nf = 0, ns = 0;
    for (int q = 0; q < NR; q++)
        if (tid + q * kSvThreads < n) {
            nf += (ap[q] > 0.0 && ap[q] < C) + (am[q] > 0.0 && am[q] < C);
            ns += ap[q] - am[q] != 0.0;
        }
    cnt[tid] = nf | (ns << 16);
    __syncthreads();
    int n_free = 0, n_sv = 0;
    for (int l = 0; l < kSvThreads; l++) { n_free += cnt[l] & 0xffff; n_sv += cnt[l] >> 16; }
    double bias;
    if (n_free > 0) {                                                  // -(the mean of y_i G_i over the free variables), v ascending
        for (int half = 0; half < 2; half++) {
            for (int q = 0; q < NR; q++) {
                const int row = tid + q * kSvThreads;
                const double a = half == 0 ? ap[q] : am[q];
                if (row < n) bet[row] = a > 0.0 && a < C ? (half == 0 ? Gp[q] : -Gm[q]) : 0.0;     // + 0 leaves the sum as it is
            }
            __syncthreads();
            if (tid == 0) {
                double sm = half == 0 ? 0.0 : red[0];
                for (int i = 0; i < n; i++) sm = sm + bet[i];
                red[0] = sm;
            }
            __syncthreads();
        }
        bias = -(red[0] / (double)n_free);
    } else {
        bias = (gmax + gmin) * 0.5;                                    // the midpoint of the two bounds
    }
    if (!sv_finite(bias) || !sv_finite(gap)) flag[1] = 1;
    // ---- beta = alpha - alpha* on the rows used, +0 beyond them ----
    for (int q = 0; q < NR; q++) {
        const int row = tid + q * kSvThreads;
        if (row < n) {
            const double b = ap[q] - am[q];
            bet[row] = b;
            if (g.beta) g.beta[(k * (size_t)D + (size_t)row) * R + r] = b;
            if (!sv_finite(b)) flag[1] = 1;
        }
    }
    if (g.beta)
        for (int t = n + tid; t < D; t += kSvThreads) g.beta[(k * (size_t)D + (size_t)t) * R + r] = 0.0;
    __syncthreads();
    if (!GAU) {
        // ---- w = sum_i beta_i x_i, a lane per column; fitted = x_t . w + bias over ALL D rows ----
        if (tid < F) {
            double acc = bet[0] * Xs[tid];
            for (int i = 1; i < n; i++) acc = fma(bet[i], Xs[i * S + tid], acc);
            wl[tid] = acc;
            if (g.w) g.w[(k * (size_t)F + (size_t)tid) * R + r] = acc;
            if (!sv_finite(acc)) flag[1] = 1;
        }
        __syncthreads();
        for (int t = tid; t < D; t += kSvThreads) {
            const double *x = g.X + (size_t)t * (size_t)F * R + r;
            double v = x[0] * wl[0];
            for (int f = 1; f < F; f++) v = fma(x[(size_t)f * R], wl[f], v);
            v = v + bias;
            if (g.fitted) g.fitted[(k * (size_t)D + (size_t)t) * R + r] = v;
            if (!sv_finite(v)) flag[1] = 1;
        }
    } else {
        // ---- fitted = sum_i beta_i K(x_t, x_i) + bias: the rows used from LDS, the rows beyond them staged `cap` at a time ----
        for (int t = tid; t < n; t += kSvThreads) {
            const double *x = Xs + t * S;
            double acc = bet[0] * sv_kval<true>(x, 1, Xs, F, s2);
            for (int i = 1; i < n; i++) acc = fma(bet[i], sv_kval<true>(x, 1, Xs + i * S, F, s2), acc);
            acc = acc + bias;
            if (g.fitted) g.fitted[(k * (size_t)D + (size_t)t) * R + r] = acc;
            if (!sv_finite(acc)) flag[1] = 1;
        }
        int cap = (g.lds - kSvAux - n * (S + 1)) / S;
        cap = cap < kSvThreads ? cap : kSvThreads;
        for (int c0 = n; c0 < D && cap > 0; c0 += cap) {
            const int rows = D - c0 < cap ? D - c0 : cap;
            __syncthreads();
            for (int idx = tid; idx < rows * F; idx += kSvThreads) {
                const int i = idx / F, f = idx % F;
                chunk[i * S + f] = g.X[((size_t)(c0 + i) * (size_t)F + (size_t)f) * R + r];
            }
            __syncthreads();
            if (tid < rows) {
                const double *x = chunk + tid * S;
                double acc = bet[0] * sv_kval<true>(x, 1, Xs, F, s2);
                for (int i = 1; i < n; i++) acc = fma(bet[i], sv_kval<true>(x, 1, Xs + i * S, F, s2), acc);
                acc = acc + bias;
                if (g.fitted) g.fitted[(k * (size_t)D + (size_t)(c0 + tid)) * R + r] = acc;
                if (!sv_finite(acc)) flag[1] = 1;
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        if (g.bias) g.bias[k * R + r] = bias;
        if (g.gap) g.gap[k * R + r] = gap;
        if (g.n_iter) g.n_iter[k * R + r] = it;
        if (g.n_sv) g.n_sv[k * R + r] = n_sv;
        if (g.status) g.status[k * R + r] = (gap < g.tol ? 0 : kSvNotConverged) | (flag[1] ? kSvNonfinite : 0);
    }
}

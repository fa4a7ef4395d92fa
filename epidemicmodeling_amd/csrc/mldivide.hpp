// MATLAB's rectangular backslash m = X \ y of test01FitExponential.m:159, test03ExpfitVsIPRegression.m:169 and
// test05DirectNewCasesLearning.m:185 (IPtoRateMap = X(1:train,:) \ y(1:train)): Householder QR with column pivoting on X
// itself, MATLAB's rank rule, the basic solution; one item per (row count k, region r).  Included by epiekf.hip (entry point
// epi_mldiv_run_device, include/epiekf.h).  DESIGN.md §4.12 pins the arithmetic; tests/mldivide_ref.c and
// tests/mldivide_ref.py restate it and the suites hold all three to the same bits.
//
// mldivide_items: one workgroup of 256 lanes per item.  The item's [n_rows][F+1] work matrix [X y] lives in LDS, column-major,
// for the whole factorisation; the columns are never moved, col[] holds the pivot order.  Every sum over rows is kMlP = 8
// interleaved fma chains (row i in chain i mod 8): lane (slot, p) = (tid / 8, tid % 8) runs chain p of the column in its slot,
// the partials meet in LDS and are added in ascending order, and the same lane then updates the rows i = p mod 8 of that
// column, so a column belongs to one group of 8 lanes through a Householder step.  Columns beyond 32 slots take further rounds.
// Every lane reads the pivot, tau and the rank from LDS itself: every branch around a barrier is uniform.  The reflector is
// never stored: v_i = a_i * scale is formed where it is used, and Q'y is the y column riding along.  No atomics, no scratch,
// no host synchronisation.
#pragma once

constexpr int kMlMaxF = 96, kMlP = 8, kMlThreads = 256, kMlSlots = kMlThreads / kMlP, kMlRowCounts = 64;
constexpr int kMlMaxElems = 20000;         // max(n_rows) (F + 1): 160 000 bytes of the 160 KiB of LDS
constexpr int kMlAux = 480;                // doubles before the matrix: vn1[96], vn2[96], partials[256], col[97] bytes, 2 flags
constexpr int kMlRankDeficient = 1, kMlNonfiniteInput = 2, kMlNonfinite = 4;      // epi_mldiv_status_bits
constexpr double kMlEps = 2.220446049250313e-16, kMlTol3z = 1.4901161193847656e-08;   // 2^-52, 2^-26
constexpr double kMlTiny = 0x1p-900;       // a column whose squares sum to less has no reflector (their rounding would break Q'Q = I)
// workgroups per launch: a launch's thread count (workgroups x 256 lanes) is a 32-bit number in the HIP runtime (lasso.hpp)
constexpr int64_t kMlLaunchItems = (int64_t)1 << 22;

struct MlArgs {
    int D, F, R;
    int k0;                                // the first row count of this launch
    long long item0;                       // the first item of this launch within its row counts: item = kk * R + r
    int nr[kMlRowCounts];                  // n_rows[k0 + kk]
    double tol_scale;
    const double *X, *y;                   // [D][F][R], [D][R]
    double *m, *rdiag, *resid, *fitted;
    int32_t *rank, *perm, *status;
};

EPI_DEV bool ml_finite(double v) { return fabs(v) < (double)INFINITY; }

// chain p of the sum over the rows lo .. n-1 of a_i b_i (a_i * scale, rounded, with `scaled`): the rows i = p mod 8 ascending
EPI_DEV double ml_chain(const double *a, const double *b, int lo, int n, int p, double scale, bool scaled)
{
    double s = 0.0;
    for (int i = lo + (p - lo % kMlP + kMlP) % kMlP; i < n; i += kMlP) s = fma(scaled ? a[i] * scale : a[i], b[i], s);
    return s;
}

EPI_DEV double ml_combine(const double *part)
{
    double t = part[0];
    for (int p = 1; p < kMlP; p++) t = t + part[p];
    return t;
}

// bytes of dynamic LDS a workgroup needs for n rows
inline size_t ml_lds_bytes(int n, int F) { return ((size_t)kMlAux + (size_t)n * (size_t)(F + 1)) * sizeof(double); }

extern __shared__ double ml_lds[];

__global__ __launch_bounds__(kMlThreads) void mldivide_items(const MlArgs g)
{
    const int tid = threadIdx.x, D = g.D, F = g.F, W = F + 1, p = tid % kMlP, slot = tid / kMlP;
    const long long item = g.item0 + (long long)blockIdx.x;
    const int kk = (int)(item / g.R), n = g.nr[kk], mn = n < F ? n : F;
    const size_t R = (size_t)g.R, r = (size_t)(item % g.R), k = (size_t)(g.k0 + kk);
    double *vn1 = ml_lds, *vn2 = vn1 + kMlMaxF, *part = vn2 + kMlMaxF, *A = ml_lds + kMlAux;
    unsigned char *col = (unsigned char *)(part + kMlThreads);         // col[q]: the original column at pivot position q; col[F] = F
    int *flag = (int *)(ml_lds + kMlAux - 2);                          // [0]: a non-finite input, later result; [1]: a norm to recompute
    const double qnan = __builtin_nan("");
    if (tid < 2) flag[tid] = 0;
    if (tid <= F) col[tid] = (unsigned char)tid;
    __syncthreads();
    // ---- [X y] of the used rows into LDS: column f at A + f n, y at A + F n ----
    for (int idx = tid; idx < n * W; idx += kMlThreads) {
        const int i = idx / W, f = idx % W;
        const double v = f < F ? g.X[((size_t)i * (size_t)F + (size_t)f) * R + r] : g.y[(size_t)i * R + r];
        A[(size_t)f * n + i] = v;
        if (!ml_finite(v)) flag[0] = 1;
    }
    __syncthreads();
    if (flag[0]) {                                                     // NONFINITE_INPUT: the same in every lane
        if (tid < F) {
            const size_t o = (k * (size_t)F + (size_t)tid) * R + r;
            if (g.m) g.m[o] = qnan;
            if (g.rdiag) g.rdiag[o] = qnan;
            if (g.perm) g.perm[o] = tid;
        }
        if (g.fitted)
            for (int t = tid; t < D; t += kMlThreads) g.fitted[(k * (size_t)D + (size_t)t) * R + r] = qnan;
        if (tid == 0) {
            if (g.resid) g.resid[k * R + r] = qnan;
            if (g.rank) g.rank[k * R + r] = -1;
            if (g.status) g.status[k * R + r] = kMlNonfiniteInput;
        }
        return;
    }
    // ---- the column norms ----
    for (int f0 = 0; f0 < F; f0 += kMlSlots) {
        const int f = f0 + slot;
        if (f < F) part[tid] = ml_chain(A + (size_t)f * n, A + (size_t)f * n, 0, n, p, 0.0, false);
        __syncthreads();
        if (f < F && p == 0) vn1[f] = vn2[f] = sqrt(ml_combine(part + tid));
        __syncthreads();
    }
    // ---- Householder QR with column pivoting ----
    for (int j = 0; j < mn; j++) {
        int best = j;
        double bv = vn1[col[j]];
        for (int q = j + 1; q < F; q++) {
            const double v = vn1[col[q]];
            if (v > bv || (v == bv && col[q] < col[best])) { best = q; bv = v; }
        }
        const int c = col[best];
        const double *ac = A + (size_t)c * n;
        if (tid < kMlP) part[tid] = ml_chain(ac, ac, j + 1, n, tid, 0.0, false);
        __syncthreads();
        const double alpha = ac[j], ss = ml_combine(part), t2 = fma(alpha, alpha, ss);
        double beta = alpha, tau = 0.0, scale = 0.0;
        if (ss != 0.0 && t2 >= kMlTiny) {
            beta = -copysign(sqrt(t2), alpha);
            tau = (beta - alpha) / beta;
            scale = 1.0 / (alpha - beta);
        }
        if (tid == 0) {
            col[best] = col[j];
            col[j] = (unsigned char)c;
            flag[1] = 0;
        }
        __syncthreads();
        if (tid == 0) A[(size_t)c * n + j] = beta;                     // R(j,j); the rounds below read column c below row j only
        if (tau != 0.0) {
            for (int q0 = j + 1; q0 <= F; q0 += kMlSlots) {            // the remaining columns and y, 32 a round
                const int q = q0 + slot;
                double *ak = A + (size_t)(q <= F ? col[q] : 0) * n;
                double aj = 0.0;                                       // read before the barrier: one lane of the group rewrites it
                if (q <= F) {
                    aj = ak[j];
                    part[tid] = ml_chain(ac, ak, j + 1, n, p, scale, true);
                }
                __syncthreads();
                if (q <= F) {
                    const double w = aj + ml_combine(part + slot * kMlP), tw = tau * w;
                    for (int i = j + 1 + (p - (j + 1) % kMlP + kMlP) % kMlP; i < n; i += kMlP) ak[i] = fma(-tw, ac[i] * scale, ak[i]);
                    if (p == j % kMlP) ak[j] = aj - tw;
                }
                __syncthreads();
            }
        }
        // the partial norms, downdated as in dlaqp2: a lane per remaining column
        if (tid < F - j - 1) {
            const int kq = col[j + 1 + tid];
            const double v1 = vn1[kq];
            if (v1 != 0.0) {
                const double t = fabs(A[(size_t)kq * n + j]) / v1;
                double temp = 1.0 - t * t;
                if (temp < 0.0) temp = 0.0;
                const double u = v1 / vn2[kq], temp2 = temp * (u * u);
                if (temp2 <= kMlTol3z) { vn2[kq] = -1.0; flag[1] = 1; }    // below the safeguard: computed again below
                else vn1[kq] = v1 * sqrt(temp);
            }
        }
        __syncthreads();
        if (flag[1]) {                                                 // the same in every lane
            for (int q0 = j + 1; q0 < F; q0 += kMlSlots) {
                const int q = q0 + slot, kq = q < F ? col[q] : 0;
                const bool again = q < F && vn2[kq] < 0.0;
                if (again) part[tid] = ml_chain(A + (size_t)kq * n, A + (size_t)kq * n, j + 1, n, p, 0.0, false);
                __syncthreads();
                if (again && p == 0) vn1[kq] = vn2[kq] = sqrt(ml_combine(part + tid));
                __syncthreads();
            }
        }
    }
    // ---- MATLAB's rank rule, read by every lane from R's diagonal in LDS ----
    const double tol = g.tol_scale * (double)(n > F ? n : F) * kMlEps * fabs(A[(size_t)col[0] * n]);
    int rank = 0;
    while (rank < mn && fabs(A[(size_t)col[rank] * n + rank]) > tol) rank++;
    // ---- the basic solution: back substitution by columns, lane i's remainder loses R(i,q) m_q for q descending ----
    const double *z = A + (size_t)F * n;
    double s = tid < rank ? z[tid] : 0.0;
    for (int q = rank - 1; q >= 0; q--) {
        const double *aq = A + (size_t)col[q] * n;
        if (tid == q) part[q] = s / aq[q];
        __syncthreads();
        if (tid < q) s = fma(-aq[tid], part[q], s);
    }
    if (tid < F) vn1[tid] = 0.0;                                       // vn1 becomes m in the original column order
    __syncthreads();
    if (tid < rank) vn1[col[tid]] = part[tid];
    __syncthreads();
    if (tid < kMlP) part[tid] = ml_chain(z, z, rank, n, tid, 0.0, false);
    if (tid < F) {
        const size_t o = (k * (size_t)F + (size_t)tid) * R + r;
        const double mv = vn1[tid], rd = tid < mn ? A[(size_t)col[tid] * n + tid] : 0.0;
        if (g.m) g.m[o] = mv;
        if (g.rdiag) g.rdiag[o] = rd;
        if (g.perm) g.perm[o] = col[tid];
        if (!ml_finite(mv) || !ml_finite(rd)) flag[0] = 1;
    }
    // ---- X m over ALL D rows: the rows beyond n_rows are the prediction ----
    for (int t = tid; t < D; t += kMlThreads) {
        const double *x = g.X + (size_t)t * (size_t)F * R + r;
        double v = x[0] * vn1[0];
        for (int f = 1; f < F; f++) v = fma(x[(size_t)f * R], vn1[f], v);
        if (g.fitted) g.fitted[(k * (size_t)D + (size_t)t) * R + r] = v;
        if (!ml_finite(v)) flag[0] = 1;
    }
    __syncthreads();
    if (tid == 0) {
        const double res = sqrt(ml_combine(part));
        if (g.resid) g.resid[k * R + r] = res;
        if (g.rank) g.rank[k * R + r] = rank;
        if (g.status) g.status[k * R + r] = (rank < mn ? kMlRankDeficient : 0) | (flag[0] || !ml_finite(res) ? kMlNonfinite : 0);
    }
}

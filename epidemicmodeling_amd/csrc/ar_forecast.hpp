// The autoregressive alpha forecaster (Tools/PrescribeNPI.m:204-215: ar -> filtic -> filter -> clamp -> SI_Controlled) for R
// regions x D Monte-Carlo draws, chain = r * D + d; included by epiekf.hip (entry point epi_arfc_run_device,
// include/epiekf.h).  DESIGN.md §4.8 pins the arithmetic; tests/ar_forecast_ref.c restates it in C and the GPU suite holds
// the two to the same bits.
//
// ar_fit       one wavefront per region.  The stacked forward-backward matrix [X | b] (M = 2 (L - p) rows, p + 1 columns)
//              is built from the segment in LDS, column-major (a lane's rows are 64 apart: conflict-free), and reduced by
//              Householder reflections.  Every column sum is the PINNED SUM: lane l runs one fma chain over the rows
//              i = l, l + 64, ... (ascending, from +0.0), the 64 chains are combined by t = t + shfl_xor(t, h), h = 32 .. 1
//              (IEEE addition commutes, so every lane ends with the same bits).  A lane only ever writes its own rows;
//              the pivot element and R's rows cross lanes through LDS behind a barrier.
// ar_simulate  one lane per chain, 64-lane workgroups that never straddle a region: the region's segment, A and b0 are
//              read once per workgroup; the p past values live in a per-lane LDS ring [p][64] (a runtime-indexed register
//              array would go to scratch).  z / drive loads and S stores are coalesced over the chains.
#pragma once

constexpr int kArMaxP = 32, kArMaxRows = 256;      // p, L - p
constexpr int kArOk = 0, kArRankDeficient = 1, kArBadInput = 2;
// workgroups per launch: a launch's thread count (workgroups x 64 lanes) is a 32-bit number in the HIP runtime (lasso.hpp)
constexpr int64_t kArLaunchBlocks = (int64_t)1 << 25;

struct ArFitArgs {
    int L, p, R, nv_mode;
    long long r0;                  // first region of this launch
    const double *seg;             // [L][R]
    double *A, *nv;                // [p][R], [R]
    int32_t *status;               // [R] or NULL
};

struct ArSimArgs {
    int L, p, H, R, D, Sd, bpr;    // bpr = workgroups per region
    long long blk0;                // first workgroup of this launch
    double dt;
    const double *seg, *beta, *s0, *i0;   // [L][R], [R] x 3
    const double *A, *nv;          // [p][R], [R]
    const double *z, *drive;       // [H][B] or NULL, [H][Sd] or NULL
    const int32_t *drive_series;   // [B] or NULL
    double *S;                     // [L + H][3][B]
};

// workgroups per region of ar_simulate: ceil(D / 64), in 64 bits (D + 63 leaves int for D > 2^31 - 64, which validate accepts
// with R = 1); the result is at most 2^25 and fits ArSimArgs::bpr
inline int ar_blocks_per_region(int D) { return (int)(((int64_t)D + 63) / 64); }

EPI_DEV size_t ar_lds_seg(int L) { return ((size_t)L + 7) & ~(size_t)7; }
inline size_t ar_fit_lds_bytes(int L, int p) { return ((((size_t)L + 7) & ~(size_t)7) + 64 + (size_t)(p + 1) * 2 * (size_t)(L - p)) * sizeof(double); }
inline size_t ar_sim_lds_bytes(int L, int p) { return ((((size_t)L + 7) & ~(size_t)7) + 32 + (size_t)p * 64) * sizeof(double); }

EPI_DEV bool ar_finite(double v) { return fabs(v) < (double)INFINITY; }

// the butterfly of the pinned sum: every lane returns the same bits
EPI_DEV double ar_combine(double t)
{
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) t = t + __shfl_xor(t, h);
    return t;
}

__global__ __launch_bounds__(64) void ar_fit(const ArFitArgs a)
{
    extern __shared__ double ar_lds[];
    const int lane = threadIdx.x, L = a.L, p = a.p, n = L - p, M = 2 * n;
    const size_t R = (size_t)a.R, r = (size_t)(a.r0 + (long long)blockIdx.x);
    double *y = ar_lds;                      // [L] the segment
    double *coef = y + ar_lds_seg(L);        // [32] a_1 .. a_p
    double *diag = coef + 32;                // [32] r_jj
    double *X = diag + 32;                   // [p + 1][M], column p = b
    const double qnan = __builtin_nan("");
    int bad = 0;
    for (int t = lane; t < L; t += 64) {
        const double v = a.seg[(size_t)t * R + r];
        y[t] = v;
        bad |= !ar_finite(v);
    }
    bad = __ballot(bad) != 0;
    __syncthreads();
    int status = bad ? kArBadInput : kArOk;
    double nv = qnan;
    if (!bad) {
        // forward rows t = p .. L-1 (row t - p): y(t) + sum a_k y(t-k); backward rows (row n + t - p): y(t-p) + sum a_k y(t-p+k)
        for (int i = lane; i < M; i += 64) {
            const bool fwd = i < n;
            const int base = fwd ? p + i : i - n;
            for (int k = 1; k <= p; k++) X[(size_t)(k - 1) * M + i] = y[fwd ? base - k : base + k];
            X[(size_t)p * M + i] = y[base];
        }
        // the rank rule's scale: the largest 2-norm of an original column
        double big = 0.0;
        for (int c = 0; c < p; c++) {
            const double *xc = X + (size_t)c * M;
            double acc = 0.0;
            for (int i = lane; i < M; i += 64) acc = fma(xc[i], xc[i], acc);
            big = fmax(big, sqrt(ar_combine(acc)));
        }
        const double tol = ((double)(M > p ? M : p) * 2.220446049250313e-16) * big;
        for (int j = 0; j < p; j++) {
            __syncthreads();                 // row j of column j was written by lane j % 64 in the previous update
            double *xj = X + (size_t)j * M;
            double acc = 0.0;
            for (int i = lane; i < M; i += 64)
                if (i >= j) acc = fma(xj[i], xj[i], acc);
            const double norm = sqrt(ar_combine(acc));
            if (!(norm > tol)) { status = kArRankDeficient; break; }     // wave-uniform
            const double xjj = xj[j];
            const double rjj = xjj >= 0.0 ? -norm : norm;
            const double vj = xjj - rjj;
            const double dd = norm * (norm + fabs(xjj));                 // v'v / 2
            __syncthreads();
            if (lane == (j & 63)) xj[j] = vj;                            // the reflector stays in column j, rows j ..
            if (lane == 0) diag[j] = rjj;
            __syncthreads();
            for (int c = j + 1; c <= p; c++) {
                double *xc = X + (size_t)c * M;
                double w = 0.0;
                for (int i = lane; i < M; i += 64)
                    if (i >= j) w = fma(xj[i], xc[i], w);
                const double f = ar_combine(w) / dd;
                for (int i = lane; i < M; i += 64)
                    if (i >= j) xc[i] = xc[i] - f * xj[i];
            }
        }
        __syncthreads();
        if (status == kArOk) {
            // R a = -c, back-substitution; every lane computes the same values and writes the same words
            for (int j = p - 1; j >= 0; j--) {
                double s = -X[(size_t)p * M + j];
                for (int k = j + 1; k < p; k++) s = s - X[(size_t)k * M + j] * coef[k];
                coef[j] = s / diag[j];
            }
            // residual sums over the original rows, forward and backward separately
            double af = 0.0, ab = 0.0;
            for (int i = lane; i < n; i += 64) {
                const int t = p + i;
                double ef = y[t], eb = y[i];
                for (int k = 1; k <= p; k++) {
                    ef = fma(coef[k - 1], y[t - k], ef);
                    eb = fma(coef[k - 1], y[i + k], eb);
                }
                af = fma(ef, ef, af);
                ab = fma(eb, eb, ab);
            }
            const double frss = ar_combine(af), brss = ar_combine(ab);
            nv = a.nv_mode == 0 ? (frss + brss) / (double)(2 * n) : frss / (double)n;
        }
    }
    if (lane < p) a.A[(size_t)lane * R + r] = status == kArOk ? coef[lane] : qnan;
    if (lane == 0) {
        a.nv[r] = nv;
        if (a.status) a.status[r] = status;
    }
}

// the status of the given-model mode (no fit runs): one lane per region
__global__ __launch_bounds__(64) void ar_given_status(int L, int R, const double *__restrict__ seg, int32_t *__restrict__ status)
{
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= R) return;
    int bad = 0;
    for (int t = 0; t < L; t++) bad |= !ar_finite(seg[(size_t)t * (size_t)R + (size_t)r]);
    status[r] = bad ? kArBadInput : kArOk;
}

__global__ __launch_bounds__(64) void ar_simulate(const ArSimArgs a)
{
    extern __shared__ double ar_lds[];
    const int lane = threadIdx.x, L = a.L, p = a.p, H = a.H;
    const long long blk = a.blk0 + (long long)blockIdx.x;
    const size_t R = (size_t)a.R, r = (size_t)(blk / a.bpr), B = R * (size_t)a.D;
    const int d = (int)(blk % a.bpr) * 64 + lane;
    const bool active = d < a.D;
    const size_t c = r * (size_t)a.D + (size_t)(active ? d : 0);
    double *y = ar_lds;                      // [L] the segment
    double *coef = y + ar_lds_seg(L);        // [32]
    double *ring = coef + 32;                // [p][64] past values of the recursion, one column per lane
    const double qnan = __builtin_nan("");
    int bad = 0;
    for (int t = lane; t < L; t += 64) {
        const double v = a.seg[(size_t)t * R + r];
        y[t] = v;
        bad |= !ar_finite(v);
    }
    int dead = 0;
    if (lane < p) {
        const double v = a.A[(size_t)lane * R + r];
        coef[lane] = v;
        dead = !ar_finite(v);
    }
    const double b0 = sqrt(a.nv[r]);
    dead |= !ar_finite(b0);
    bad = __ballot(bad) != 0;                // BAD_INPUT: every day is NaN
    dead = bad || __ballot(dead) != 0;       // no usable model: NaN from day L on
    __syncthreads();
    const double beta = a.beta[r], dt = a.dt;
    double s = a.s0[r], i = a.i0[r];
    size_t ser = 0;
    if (a.drive && active) ser = a.drive_series ? (size_t)a.drive_series[c] : c;
    double *o = a.S + c;
    // ---- the segment: alpha_hat = seg clamped, SI_Controlled.m:19-22 ----
    for (int t = 0; t < L; t++) {
        const double v = y[t];
        const double al = v < 0.0 ? 0.0 : v;
        if (active) {
            o[0] = bad ? qnan : s; o[B] = bad ? qnan : i; o[2 * B] = bad ? qnan : al;
        }
        o += 3 * B;
        const double sn = fmax(0.0, fmin(1.0, s - dt * al * s * i));
        const double in = fmax(0.0, fmin(1.0, i + dt * (al * s * i - beta * i)));
        s = sn; i = in;
    }
    // ---- the forecast: y(t) = b0 z(t) - sum a_k y(t-k), k ascending, the past from the segment first ----
    for (int j = 0; j < p; j++) ring[j * 64 + lane] = y[L - p + j];
    int head = 0;
    for (int t = 0; t < H; t++) {
        const double zt = (a.z && active) ? a.z[(size_t)t * B + c] : 0.0;
        double acc = b0 * zt;
        int idx = head;
        for (int k = 0; k < p; k++) {
            idx = idx == 0 ? p - 1 : idx - 1;
            acc = fma(-coef[k], ring[idx * 64 + lane], acc);
        }
        ring[head * 64 + lane] = acc;
        head = head + 1 == p ? 0 : head + 1;
        double v = acc;
        if (a.drive && active) v = acc + a.drive[(size_t)t * (size_t)a.Sd + ser];
        const double al = v < 0.0 ? 0.0 : v;
        if (active) {
            o[0] = dead ? qnan : s; o[B] = dead ? qnan : i; o[2 * B] = dead ? qnan : al;
        }
        o += 3 * B;
        if (t + 1 < H) {
            const double sn = fmax(0.0, fmin(1.0, s - dt * al * s * i));
            const double in = fmax(0.0, fmin(1.0, i + dt * (al * s * i - beta * i)));
            s = sn; i = in;
        }
    }
}

// The Gaussian innovation log-likelihood of every chain from the arrays a filter run left in HBM (S_MINUS, P_MINUS, innovations
// as the runner wrote them: classic or chain-blocked, double or float); included by epiekf.hip (entry point
// epi_loglik_run_device, include/epiekf.h).  DESIGN.md §4.14 pins the arithmetic; tests/loglik_ref.c restates it and the GPU
// suite holds the two to the same bits.
//
//   ll_replay   (r_mode 0 only) one lane per chain walks the T filter steps and replays the filter's adaptive R(k) from the
//               stored innovations and the NaN mask of x (ekf_fwd's recursion: two L-sample rings in LDS, summed newest first);
//               R(k) goes to R_used or to the workspace, indexed by day.
//   ll_blocks   one lane per (chain, block of 32 filter steps): S = C P- C' + gamma R(k) in the dense filter's operation order
//               restricted to the upper-left 3 x 3 of P-, the per-day outputs, and the block's sums added in ascending k from 0.0.
//   ll_chains   one lane per chain adds the block sums in ascending block order from 0.0 and forms loglik / nis_mean.
//   ll_select   one lane per region: the lowest candidate index of the largest loglik among the usable candidates.
//
// Because the order of every sum is fixed by the 32-step blocks, the time-parallel kernels give the bits of a sequential walk.
// Chains are the fastest index everywhere, so a wavefront's load of one row of one day is one contiguous run; every element is
// read once (non-temporal loads) through a 64-bit element offset, so no array size limits the addressing.
//
// Host-compilation contract: each kernel's body is an EPI_DEV function of its own indices (ll_*_lane); tests/loglik_emu.cpp
// compiles them with the host compiler and calls them one lane at a time.  The __global__ wrappers below them only compute the
// indices.
#pragma once

constexpr int kLlBlock = 32;                              // filter steps per summation block (part of the definition)
constexpr double kLlLog2Pi = 1.8378770664093453;          // log(2 pi)
constexpr double kLlDblMin = 2.2250738585072014e-308;

struct LlArgs {
    int B, T, L, Sx, r_mode, f32, flip, generic, obs_type, k0, k1, G;
    int blk, nblk;                                        // layout of S_MINUS / P_MINUS / innovations (ll_geometry)
    int m, nb32;                                          // states of the model; ceil(T / 32)
    const void *S_MINUS, *P_MINUS, *innov;
    const double *x, *R_series, *R_scalar, *prm;
    const int32_t *x_series;
    double *Rk;                                           // [T][B] by day: R_used or workspace (r_mode 0), R_used or NULL (r_mode 1)
    double *part_term, *part_q;                           // [nb32][B]
    int32_t *part_n, *part_bad;                           // [nb32][B]
    double *loglik, *nis_mean;                            // [B] (ll_select reads loglik, n_valid, status: workspace if not wanted)
    int32_t *n_valid, *status;
    double *S, *nis;                                      // [T][B] or NULL
    int32_t *best;                                        // [B / G]
    double *best_loglik;
};

// the layout block and the blocks per day from the descriptor's B and lane_block (two_filter.hpp's rule: blk = B, the classic
// layout, for lane_block 0 or >= B; in 64 bits, so that B + blk - 1 cannot leave int)
inline void ll_geometry(int B, int lane_block, int *blk, int *nblk)
{
    const int64_t b = (lane_block <= 0 || lane_block >= B) ? (int64_t)B : (int64_t)lane_block;
    *blk = (int)b;
    *nblk = (int)(((int64_t)B + b - 1) / b);
}

EPI_DEV double ll_ld(const void *p, size_t o, int f32)
{
    return f32 ? (double)__builtin_nontemporal_load((const float *)p + o) : __builtin_nontemporal_load((const double *)p + o);
}

// ---- the filter's adaptive R replayed (epiekf.hip, ekf_fwd: the innovation monitor and R(k+1)) ----
// win: this lane's column of two zeroed rings [2][L] with element stride `stride`
EPI_DEV void ll_replay_lane(const LlArgs &a, int c, double *win, int stride)
{
    const int T = a.T, L = a.L;
    const size_t B = (size_t)a.B, bp = (size_t)a.blk * (size_t)a.nblk;
    const int sx = a.x_series ? a.x_series[c] : c;
    const double beta = a.prm[(size_t)EPI_PRM_BETA_EKF * B + c];
    const double R_v = a.R_scalar[c];
    double *winMean = win, *winCov = win + (size_t)L * stride;
    for (int j = 0; j < L; j++) { winMean[j * stride] = 0.0; winCov[j * stride] = 0.0; }
    int head = 0;
    double R_next = R_v;
    for (int k = 0; k < T; k++) {
        const int t = a.flip ? (T - 1 - k) : k;
        const double Rk = R_next;
        a.Rk[(size_t)t * B + c] = Rk;
        const bool valid = !is_nan(a.x[(size_t)t * a.Sx + sx]);
        const double innov = ll_ld(a.innov, (size_t)t * bp + c, a.f32);
        const int cnt = (k + 1 < L) ? (k + 1) : L;
        head = (head == 0) ? (L - 1) : (head - 1);
        winMean[head * stride] = innov;
        const double sum = ring_sum(winMean, head, L, innov, stride);
        const double mu = sum / (double)cnt;
        const double cc = (innov - mu) * (innov - mu);
        winCov[head * stride] = cc;
        const bool adapt = a.generic ? (beta != 1.0 && valid && k < T - 1) : (beta != 1.0 && valid);
        if (adapt) {
            const double sumC = ring_sum(winCov, head, L, cc, stride);
            if (a.generic) R_next = beta * Rk + (1.0 - beta) * (sumC / (double)cnt);
            else R_next = beta * Rk + (1.0 - beta) * sumC / (double)cnt;
        } else if (a.generic) {
            R_next = R_v;
        }
    }
}

// ---- one block of 32 filter steps of one chain ----
EPI_DEV void ll_block_lane(const LlArgs &a, int c, int b32)
{
    const int T = a.T, M = a.m;
    const size_t B = (size_t)a.B, blk = (size_t)a.blk, cb = (size_t)c / blk, cr = (size_t)c - cb * blk;
    const size_t bp = blk * (size_t)a.nblk;
    const int sx = a.x_series ? a.x_series[c] : c;
    const double gamma = a.prm[(size_t)EPI_PRM_GAMMA_EKF * B + c];
    const double qnan = __builtin_nan("");
    double sum_term = 0.0, sum_q = 0.0;
    int n = 0, bad = 0;
    const int kb = b32 * kLlBlock, ke = (kb + kLlBlock < T) ? kb + kLlBlock : T;
    for (int k = kb; k < ke; k++) {
        const int t = a.flip ? (T - 1 - k) : k;
        const size_t o = (size_t)t * B + c;
        const double xk = a.x[(size_t)t * a.Sx + sx];
        double Rk;
        if (a.r_mode) {
            Rk = a.R_series[(size_t)k * a.Sx + sx];        // R_v is not time-flipped by the backward wrappers
            if (a.Rk) a.Rk[o] = Rk;
        } else {
            Rk = a.Rk[o];
        }
        const bool valid = !is_nan(xk) && k >= a.k0 && k < a.k1;
        double S = qnan, q = qnan;
        if (valid) {
            const size_t slot = (size_t)t * (size_t)a.nblk + cb;
            const size_t ov = slot * (size_t)M * blk + cr, om = slot * (size_t)(M * M) * blk + cr;
            double s[3], P[9], C[3];
#pragma unroll
            for (int i = 0; i < 3; i++) s[i] = ll_ld(a.S_MINUS, ov + (size_t)i * blk, a.f32);
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
                for (int i = 0; i < 3; i++) P[i + 3 * j] = ll_ld(a.P_MINUS, om + (size_t)(i + M * j) * blk, a.f32);
            const double e = ll_ld(a.innov, (size_t)t * bp + c, a.f32);
            if (a.obs_type == EPI_OBS_NEWCASES) {          // obs_jacobian, rows 0..2
                C[0] = s[1] * s[2];
                C[1] = s[0] * s[2];
                C[2] = s[0] * s[1];
            } else {
                C[0] = -1.0; C[1] = 0.0; C[2] = 0.0;
            }
            double CP[3];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                double acc = C[0] * P[0 + 3 * j];
                acc = fma(C[1], P[1 + 3 * j], acc);
                acc = fma(C[2], P[2 + 3 * j], acc);
                CP[j] = acc;
            }
            double CPCt = CP[0] * C[0];
            CPCt = fma(CP[1], C[1], CPCt);
            CPCt = fma(CP[2], C[2], CPCt);
            S = CPCt + gamma * Rk;
            const bool good = !is_nonfinite(S) && !(S < kLlDblMin) && !is_nonfinite(e);
            if (good) {
                q = e * e / S;
                const double term = epi_log(S) + q;
                sum_term = sum_term + term;
                sum_q = sum_q + q;
                n = n + 1;
            } else {
                bad = 1;
            }
        }
        if (a.S) a.S[o] = S;
        if (a.nis) a.nis[o] = q;
    }
    const size_t po = (size_t)b32 * B + c;
    a.part_term[po] = sum_term;
    a.part_q[po] = sum_q;
    a.part_n[po] = n;
    a.part_bad[po] = bad;
}

// ---- the blocks of one chain, in order ----
EPI_DEV void ll_chain_lane(const LlArgs &a, int c)
{
    const size_t B = (size_t)a.B;
    double sum_term = 0.0, sum_q = 0.0;
    int n = 0, bad = 0;
    for (int b = 0; b < a.nb32; b++) {
        const size_t po = (size_t)b * B + c;
        sum_term = sum_term + a.part_term[po];
        sum_q = sum_q + a.part_q[po];
        n = n + a.part_n[po];
        bad = bad | a.part_bad[po];
    }
    int st = bad;
    if (a.f32 && !a.r_mode && a.prm[(size_t)EPI_PRM_BETA_EKF * B + c] != 1.0) st = st | 4;   // R replayed from rounded innovations
    a.loglik[c] = -0.5 * (sum_term + (double)n * kLlLog2Pi);
    if (a.nis_mean) a.nis_mean[c] = sum_q / (double)n;
    a.n_valid[c] = n;
    a.status[c] = st;
}

// ---- the candidates of one region ----
EPI_DEV void ll_select_lane(const LlArgs &a, int r)
{
    int best = -1;
    double bl = __builtin_nan("");
    for (int g = 0; g < a.G; g++) {
        const size_t c = (size_t)r * (size_t)a.G + g;
        if ((a.status[c] & 1) || a.n_valid[c] <= 0) continue;
        const double v = a.loglik[c];
        if (best < 0 || v > bl) { best = g; bl = v; }
    }
    if (a.best) a.best[r] = best;
    if (a.best_loglik) a.best_loglik[r] = bl;
}

#ifndef EPI_LOGLIK_HOST
__global__ __launch_bounds__(kWave) void ll_replay(const LlArgs a)
{
    extern __shared__ double lds[];                        // two rings [2][L][64], one column per lane
    const long long c = (long long)blockIdx.x * kWave + threadIdx.x;
    if (c >= a.B) return;
    ll_replay_lane(a, (int)c, lds + threadIdx.x, kWave);
}
__global__ __launch_bounds__(256) void ll_blocks(const LlArgs a)
{
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.B) return;
    ll_block_lane(a, (int)c, (int)blockIdx.y);
}
__global__ __launch_bounds__(256) void ll_chains(const LlArgs a)
{
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.B) return;
    ll_chain_lane(a, (int)c);
}
__global__ __launch_bounds__(256) void ll_select(const LlArgs a)
{
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.B / a.G) return;
    ll_select_lane(a, (int)r);
}
#endif

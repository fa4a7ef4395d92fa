// Joint posterior draws of the smoothed paths by backward simulation, from the arrays a 3-state filter run left in HBM (S_PLUS,
// P_PLUS, S_MINUS, P_MINUS as the runner wrote them: classic or chain-blocked, double or float); included by epiekf.hip (entry
// point epi_sdraw_run_device, include/epiekf.h).  DESIGN.md §4.16 pins the arithmetic; tests/sdraw_ref.c restates it and the GPU
// suite holds the two to the same bits.
//
//   sdraw_gain   time-parallel, a flat grid shaped like two_filter's: one lane per (chain, day), a workgroup = pinv_wg<3>()
//                neighbouring chains of ONE day.  Day k < T-1: A = StateJacobians(S+_k), J = (P+_k A') pinv(P-_{k+1}) in the
//                smoother's own operation order (mat_mul_bt, sym_pinv_psd, mat_mul: J has the bits eks_bwd forms), the guard of
//                GenericExtendedKalmanFilter.m:211, Sigma = P+ - J P- J' symmetrised, F = its pivoted Cholesky factor with the rows
//                put back in the original order.  Day T-1: J = 0, F = the factor of the terminal covariance.  Per (chain, day) it
//                leaves 24 doubles in the workspace [T][B][24]: J (9), F (9), S+_k (3), S-_{k+1} (3), so that sdraw_paths reads
//                one contiguous 192-byte record and never sees the input layout or storage.
//   sdraw_paths  one lane per path p = chain * D + draw: the recursion x_k = clamp((S+ + J (x_{k+1} - S-)) + F z_k) from T-1 down to
//                k0.  The record's address is the same for every lane of a chain (D / 64 re-reads, served by L2); the lane's three
//                z of a day are read once (non-temporal) kSdPrefetch days ahead of their use, the three outputs are written once
//                (non-temporal).  Every offset is 64-bit.
//
// Products: J and the mean update accumulate with fma() exactly where the smoother does (ekf_device.hpp's contract, the oracle's
// order); everything this call adds (Sigma, the factor, F z) is written operations: acc = a_0 b_0; acc = acc + a_k b_k, k ascending.
//
// Host-compilation contract: the body of each kernel is an EPI_DEV function of its own indices (sdraw_gain_lane, sdraw_path_lane);
// tests/sdraw_emu.cpp compiles them with the host compiler and calls them one lane at a time.
#pragma once
#include "noise.hpp"

constexpr int kSdRec = 24;                                // doubles per (day, chain) record: J 9, F 9, S+ 3, S-(k+1) 3
constexpr int kSdPrefetch = 4;                            // days the z loads run ahead of their use (measured)
constexpr long long kSdLaunchGroups = 1ll << 22;          // workgroups per launch: a launch's thread count is a 32-bit number
constexpr int kSdPathWg = 256;
constexpr int kSdNonfinite = 1, kSdRankDeficient = 2;     // bits of status

struct SdPrm { double dt, beta, gamma, epsilon, slo, ilo, alpha_min, alpha_max; };

struct SdArgs {
    int B, T, D, k0, clamp, blk, nblk, f32;
    unsigned tiles;                                       // sdraw_gain: workgroups per day
    long long wg0;                                        // first workgroup of this launch (both kernels)
    const void *S_PLUS, *P_PLUS, *S_MINUS, *P_MINUS;      // [T][nblk][3 | 9][blk], double or float
    const double *prm, *s_term, *P_term;                  // [EPI_PRM_COUNT][B]; [3][B], [9][B] or NULL
    const void *z;                                        // [T - k0][3][B * D] double or float, or NULL
    void *X;                                              // [T - k0][3][B * D] double or float
    double *ws;                                           // [T][B][kSdRec]
    double *J, *L;                                        // [T][9][B] or NULL
    int32_t *rank, *status;                               // [T][B], [B] or NULL
};

inline void sdraw_geometry(int B, int lane_block, int *blk, int *nblk)
{
    const int64_t b = (lane_block <= 0 || lane_block >= B) ? (int64_t)B : (int64_t)lane_block;
    *blk = (int)b;
    *nblk = (int)(((int64_t)B + b - 1) / b);
}

EPI_DEV double sd_ld(const void *p, size_t o, int f32)
{
    return f32 ? (double)__builtin_nontemporal_load((const float *)p + o) : __builtin_nontemporal_load((const double *)p + o);
}

// The lower factor of the symmetric 3 x 3 S by a right-looking Cholesky with diagonal pivoting (the first largest remaining
// diagonal entry), stopped as LAPACK's dpstf2 documents: when that pivot is <= 3 eps max diag(S) or not positive (a NaN pivot
// included).  The remaining columns stay zero and the rows return to the original order: F F' = S up to rounding, F is a
// row-permuted lower triangle.  Returns the rank.  Compile-time indices only (selects, no indexed registers).
EPI_DEV int sd_pchol(const double (&S)[9], double (&F)[9])
{
    constexpr int M = 3;
    double a[9], l[9];
    int piv[3] = {0, 1, 2};
#pragma unroll
    for (int e = 0; e < 9; e++) { a[e] = S[e]; l[e] = 0.0; }
    double dmax = a[IXM(0, 0)];
    dmax = (a[IXM(1, 1)] > dmax) ? a[IXM(1, 1)] : dmax;
    dmax = (a[IXM(2, 2)] > dmax) ? a[IXM(2, 2)] : dmax;
    const double stop = 3.0 * kEps * dmax;
    int rank = 0;
    bool live = true;
#pragma unroll
    for (int j = 0; j < M; j++) {
        int pv = j;
        double best = a[IXM(j, j)];
#pragma unroll
        for (int q = j + 1; q < M; q++)
            if (a[IXM(q, q)] > best) { best = a[IXM(q, q)]; pv = q; }
#pragma unroll
        for (int q = j + 1; q < M; q++) {                 // the symmetric interchange j <-> q of a, the rows of l, the order
            const bool sw = (pv == q);
#pragma unroll
            for (int c = 0; c < M; c++) {
                const double u = a[IXM(j, c)], v = a[IXM(q, c)];
                a[IXM(j, c)] = sw ? v : u;
                a[IXM(q, c)] = sw ? u : v;
            }
#pragma unroll
            for (int r = 0; r < M; r++) {
                const double u = a[IXM(r, j)], v = a[IXM(r, q)];
                a[IXM(r, j)] = sw ? v : u;
                a[IXM(r, q)] = sw ? u : v;
            }
#pragma unroll
            for (int c = 0; c < M; c++) {
                const double u = l[IXM(j, c)], v = l[IXM(q, c)];
                l[IXM(j, c)] = sw ? v : u;
                l[IXM(q, c)] = sw ? u : v;
            }
            const int pu = piv[j], pq = piv[q];
            piv[j] = sw ? pq : pu;
            piv[q] = sw ? pu : pq;
        }
        live = live && (best > stop) && (best > 0.0);     // false for a NaN pivot
        const double ajj = sqrt(live ? best : 1.0);
        l[IXM(j, j)] = live ? ajj : 0.0;
        rank = live ? j + 1 : rank;
#pragma unroll
        for (int i = j + 1; i < M; i++) l[IXM(i, j)] = live ? a[IXM(i, j)] / ajj : 0.0;
#pragma unroll
        for (int c = j + 1; c < M; c++)
#pragma unroll
            for (int i = j + 1; i < M; i++) a[IXM(i, c)] = a[IXM(i, c)] - l[IXM(i, j)] * l[IXM(c, j)];
    }
#pragma unroll
    for (int r = 0; r < M; r++)                           // row piv[i] of F = row i of l
#pragma unroll
        for (int c = 0; c < M; c++) {
            double v = l[IXM(0, c)];
            v = (piv[1] == r) ? l[IXM(1, c)] : v;
            v = (piv[2] == r) ? l[IXM(2, c)] : v;
            F[IXM(r, c)] = v;
        }
    return rank;
}

// ---- one (chain, day) item: cl may lie past the batch (the lane then works on the last chain and stores nothing) ----
template <int WG>
EPI_DEV void sdraw_gain_lane(const SdArgs &a, size_t t, size_t cl, double *lds)
{
    constexpr int M = 3, NS = 6;
    auto sx = [](int i, int j) constexpr { return i <= j ? i + j * (j + 1) / 2 : j + i * (i + 1) / 2; };
    const bool live = cl < (size_t)a.B;
    const size_t c = live ? cl : (size_t)a.B - 1;
    const size_t B = (size_t)a.B, blk = (size_t)a.blk, cb = c / blk, cr = c - cb * blk;
    const bool last = (t + 1 == (size_t)a.T);              // wave-uniform: a workgroup is one day
    const size_t t1 = last ? t : t + 1;
    const size_t slot = t * (size_t)a.nblk + cb, slot1 = t1 * (size_t)a.nblk + cb;
    const size_t ov = slot * (size_t)M * blk + cr, om = slot * (size_t)(M * M) * blk + cr;
    const size_t ov1 = slot1 * (size_t)M * blk + cr, om1 = slot1 * (size_t)(M * M) * blk + cr;
    const int f32 = a.f32;
    const double qnan = __builtin_nan("");

    double Sp[M], Sm1[M], Pp[M * M], Pm[M * M];
#pragma unroll
    for (int i = 0; i < M; i++) {
        Sp[i] = sd_ld(a.S_PLUS, ov + (size_t)i * blk, f32);
        Sm1[i] = sd_ld(a.S_MINUS, ov1 + (size_t)i * blk, f32);
    }
#pragma unroll
    for (int e = 0; e < M * M; e++) {
        Pp[e] = (last && a.P_term) ? a.P_term[(size_t)e * B + c] : sd_ld(a.P_PLUS, om + (size_t)e * blk, f32);
        Pm[e] = sd_ld(a.P_MINUS, om1 + (size_t)e * blk, f32);
    }
    bool badp = false, badm = false;                       // a non-finite S+ / P+ entry: NaN record; the guard :211 on P-(k+1)
#pragma unroll
    for (int e = 0; e < M * M; e++) { badp = badp || is_nonfinite(Pp[e]); badm = badm || is_nonfinite(Pm[e]); }
#pragma unroll
    for (int i = 0; i < M; i++) badp = badp || is_nonfinite(Sp[i]);
    badm = badm && !last;
    const bool zeroJ = badm || last;
    // the lanes that form no gain run the routines on the zero matrix (they return at once), as two_filter's do
    double Pu[NS], Xu[NS];
#pragma unroll
    for (int j = 0; j < M; j++)
#pragma unroll
        for (int i = 0; i <= j; i++) Pu[sx(i, j)] = zeroJ ? 0.0 : Pm[IXM(i, j)];   // P_MINUS is stored symmetrised: its upper triangle
    bool capped, indef;
    sym_pinv_psd<M, WG>(Pu, Xu, &capped, &indef, lds);
    if (__builtin_amdgcn_ballot_w64(indef) != 0ull) {
        // not positive semi-definite up to rounding: the two-sided Jacobi route, exactly as eks_pinv takes it
        double P2[M * M], X2[M * M];
#pragma unroll
        for (int j = 0; j < M; j++)
#pragma unroll
            for (int i = 0; i <= j; i++) { P2[IXM(i, j)] = Pu[sx(i, j)]; P2[IXM(j, i)] = Pu[sx(i, j)]; }
        bool capped2;
        sym_pinv_two_sided<M, 0>(P2, X2, &capped2, lds);
#pragma unroll
        for (int j = 0; j < M; j++)
#pragma unroll
            for (int i = 0; i <= j; i++) Xu[sx(i, j)] = indef ? X2[IXM(i, j)] : Xu[sx(i, j)];
    }
    double J[M * M], Sig[M * M], F[M * M];
    {
        SdPrm p;
        p.dt = a.prm[(size_t)EPI_PRM_DT * B + c]; p.beta = a.prm[(size_t)EPI_PRM_BETA * B + c];
        p.gamma = a.prm[(size_t)EPI_PRM_GAMMA * B + c]; p.epsilon = 0.0;
        double A[M * M], PAt[M * M], X[M * M];
        jacobian_entries<M, 0>(p, Sp, 0.0, A);             // SIAlphaModelEKF.m:62-76
        mat_mul_bt<M>(Pp, A, PAt);                         // P_PLUS * A'
#pragma unroll
        for (int j = 0; j < M; j++)
#pragma unroll
            for (int i = 0; i < M; i++) X[IXM(i, j)] = Xu[sx(i, j)];
        mat_mul<M>(PAt, X, J);                             // :215
#pragma unroll
        for (int e = 0; e < M * M; e++) J[e] = zeroJ ? 0.0 : J[e];
    }
    {
        // Sigma = P+ - (J P-) J', written products; the guard's and the last day's J = 0 meets a zeroed P-
        double T1[M * M];
#pragma unroll
        for (int j = 0; j < M; j++)
#pragma unroll
            for (int i = 0; i < M; i++) {
                double acc = J[IXM(i, 0)] * (zeroJ ? 0.0 : Pm[IXM(0, j)]);
#pragma unroll
                for (int k = 1; k < M; k++) acc = acc + J[IXM(i, k)] * (zeroJ ? 0.0 : Pm[IXM(k, j)]);
                T1[IXM(i, j)] = acc;
            }
#pragma unroll
        for (int j = 0; j < M; j++)
#pragma unroll
            for (int i = 0; i < M; i++) {
                double acc = T1[IXM(i, 0)] * J[IXM(j, 0)];
#pragma unroll
                for (int k = 1; k < M; k++) acc = acc + T1[IXM(i, k)] * J[IXM(j, k)];
                Sig[IXM(i, j)] = Pp[IXM(i, j)] - acc;
            }
        symmetrize<M>(Sig);
#pragma unroll
        for (int e = 0; e < M * M; e++) Sig[e] = badp ? 0.0 : Sig[e];
    }
    int rank = sd_pchol(Sig, F);
    if (!live) return;
    double *w = a.ws + (t * B + c) * (size_t)kSdRec;
#pragma unroll
    for (int e = 0; e < M * M; e++) {
        const double je = badp ? qnan : J[e], fe = badp ? qnan : F[e];
        w[e] = je;
        w[9 + e] = fe;
        if (a.J) a.J[(t * 9 + (size_t)e) * B + c] = je;
        if (a.L) a.L[(t * 9 + (size_t)e) * B + c] = fe;
    }
#pragma unroll
    for (int i = 0; i < M; i++) {
        w[18 + i] = (last && a.s_term) ? a.s_term[(size_t)i * B + c] : Sp[i];
        w[21 + i] = Sm1[i];
    }
    rank = badp ? -1 : rank;
    if (a.rank) a.rank[t * B + c] = rank;
    const int bits = ((badp || badm) ? kSdNonfinite : 0) | ((!badp && rank < M) ? kSdRankDeficient : 0);
    if (a.status && bits) atomicOr(a.status + c, bits);
}

// ---- one path: ZM 0 no noise (the deterministic path), 1 double z, 2 float z, 3 z generated from nk (draw (k - k0, row, p)
// of noise.hpp, at the point of use: there is no load latency to run ahead of, and the queue's registers stay free); OF 1 float X.
// nk is an argument of its own (read with ZM 3 only), so that SdArgs and the kernels that take nothing else stay as they were ----
template <int ZM>
EPI_DEV void sd_ldz(const SdArgs &a, size_t N, size_t p, int k, double (&z)[3], const NoiseKey &nk)
{
    if (ZM == 0) return;
    if (ZM == 3) { epi_normal_three(nk, (uint32_t)(k - a.k0), (uint64_t)p, z[0], z[1], z[2]); return; }
    const size_t o = (size_t)(k - a.k0) * 3 * N + p;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        if (ZM == 2) z[i] = (double)__builtin_nontemporal_load((const float *)a.z + (o + (size_t)i * N));
        else z[i] = __builtin_nontemporal_load((const double *)a.z + (o + (size_t)i * N));
    }
}

template <int ZM, int OF>
EPI_DEV void sdraw_path_lane(const SdArgs &a, size_t p, const NoiseKey &nk = NoiseKey{})
{
    constexpr int M = 3, PF = kSdPrefetch;
    const size_t B = (size_t)a.B, N = B * (size_t)a.D, c = p / (size_t)a.D;
    const int T = a.T, k0 = a.k0;
    SdPrm pr;
    pr.slo = a.prm[(size_t)EPI_PRM_S_MIN * B + c]; pr.ilo = a.prm[(size_t)EPI_PRM_I_MIN * B + c];
    pr.alpha_min = a.prm[(size_t)EPI_PRM_ALPHA_MIN * B + c]; pr.alpha_max = a.prm[(size_t)EPI_PRM_ALPHA_MAX * B + c];
    double zq[PF][3];
#pragma unroll
    for (int q = 0; q < PF; q++) {
#pragma unroll
        for (int i = 0; i < 3; i++) zq[q][i] = 0.0;
        if (ZM != 3 && T - 1 - q >= k0) sd_ldz<ZM>(a, N, p, T - 1 - q, zq[q], nk);
    }
    double x[M] = {0.0, 0.0, 0.0};
    for (int kb = T - 1; kb >= k0; kb -= PF) {
#pragma unroll
        for (int q = 0; q < PF; q++) {
            const int k = kb - q;
            if (k < k0) break;
            const double *w = a.ws + ((size_t)k * B + c) * (size_t)kSdRec;
            double v[M];
            if (k == T - 1) {
#pragma unroll
                for (int i = 0; i < M; i++) v[i] = w[18 + i];
            } else {
                double dv[M];
#pragma unroll
                for (int i = 0; i < M; i++) dv[i] = x[i] - w[21 + i];
#pragma unroll
                for (int i = 0; i < M; i++) {
                    double acc = w[IXM(i, 0)] * dv[0];
#pragma unroll
                    for (int j = 1; j < M; j++) acc = fma(w[IXM(i, j)], dv[j], acc);
                    v[i] = w[18 + i] + acc;                 // :218
                }
            }
            if (ZM != 0) {
                if (ZM == 3) sd_ldz<ZM>(a, N, p, k, zq[q], nk);
#pragma unroll
                for (int i = 0; i < M; i++) {
                    double nz = w[9 + IXM(i, 0)] * zq[q][0];
#pragma unroll
                    for (int j = 1; j < M; j++) nz = nz + w[9 + IXM(i, j)] * zq[q][j];
                    v[i] = v[i] + nz;
                }
                if (ZM != 3 && k - PF >= k0) sd_ldz<ZM>(a, N, p, k - PF, zq[q], nk);
            }
            if (a.clamp) {                                 // :221 on every draw; a NaN draw stays NaN
                double cl[M];
#pragma unroll
                for (int i = 0; i < M; i++) cl[i] = v[i];
                state_hard_margins<M>(pr, cl);
#pragma unroll
                for (int i = 0; i < M; i++) v[i] = is_nan(v[i]) ? v[i] : cl[i];
            }
            const size_t o = (size_t)(k - k0) * 3 * N + p;
#pragma unroll
            for (int i = 0; i < M; i++) {
                x[i] = v[i];
                if (OF) __builtin_nontemporal_store((float)v[i], (float *)a.X + (o + (size_t)i * N));
                else __builtin_nontemporal_store(v[i], (double *)a.X + (o + (size_t)i * N));
            }
        }
    }
}

#ifndef EPI_SDRAW_HOST
template <int M>
__global__ __launch_bounds__(pinv_wg<M>()) void sdraw_gain(const SdArgs a)
{
    constexpr int WG = pinv_wg<M>();
    __shared__ double plds[M * (M + 1) / 2 * WG];           // one column per lane: sym_pinv_psd's scratch
    const long long wg = a.wg0 + (long long)blockIdx.x;
    const size_t t = (size_t)(wg / (long long)a.tiles);
    const size_t cl = (size_t)(wg % (long long)a.tiles) * (size_t)WG + threadIdx.x;
    sdraw_gain_lane<WG>(a, t, cl, plds + threadIdx.x);
}
template <int ZM, int OF>
__global__ __launch_bounds__(kSdPathWg) void sdraw_paths(const SdArgs a)
{
    const size_t p = (size_t)(a.wg0 + (long long)blockIdx.x) * (size_t)kSdPathWg + threadIdx.x;
    if (p >= (size_t)a.B * (size_t)a.D) return;
    sdraw_path_lane<ZM, OF>(a, p);
}
template <int OF>
__global__ __launch_bounds__(kSdPathWg) void sdraw_paths_seeded(const SdArgs a, const NoiseKey nk)
{
    const size_t p = (size_t)(a.wg0 + (long long)blockIdx.x) * (size_t)kSdPathWg + threadIdx.x;
    if (p >= (size_t)a.B * (size_t)a.D) return;
    sdraw_path_lane<3, OF>(a, p, nk);
}
#endif

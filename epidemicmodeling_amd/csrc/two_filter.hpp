// The forward-backward filter fusion of Tools/TrainPredictPrescribeNPI.m:464-478 ("Backward filtering (under test)"): per
// (chain, day) two estimates (sf, Pf), (sb, Pb) -> one, in the reference's form (form 0) or the information form (form 1);
// included by epiekf.hip (entry point epi_fuse_run_device, include/epiekf.h).  DESIGN.md §4.9 pins the arithmetic;
// tests/two_filter_ref.py restates it in Python over the oracle's orc_sym_pinv / orc_mrdivide and the GPU suite holds the
// two to the same bits.
//
// A flat grid shaped like eks_pinv's: one lane per item, a workgroup = pinv_wg<M>() neighbouring chains of ONE day, workgroup
// w of the call = day w / tiles, chain tile w % tiles.  The pseudo-inverse routines and mrdivide use wavefront ballots and
// wave-uniform loops, so EVERY lane of a wavefront runs the whole body: a lane past the end of the batch works on the last
// chain of the day (a valid item) and only skips its stores.
//
// Products are written operations (this file never calls fma() in one): acc = a_0 b_0; acc = acc + a_k b_k, k ascending.
// Register pressure (6 x 6: Pf, Pb, S, X and a product are 150 doubles) is met by sequencing: upper triangles -> S -> X, then
// Pf / Pb are read AGAIN column by column for the products (the second read of a line comes from L2); X stays in registers.
#pragma once

// workgroups per launch: a launch's thread count (workgroups x lanes) is a 32-bit number in the HIP runtime (lasso.hpp)
constexpr long long kFuseLaunchGroups = 1ll << 23;

struct FuseArgs {
    int B, T, blk, nblk, f32, form, p_solver;
    unsigned tiles;                 // workgroups per day
    long long wg0;                  // first workgroup of this launch
    const void *sf, *Pf, *sb, *Pb;  // [T][nblk][m | m*m][blk], double or float
    void *s_out, *P_out;            // the same layout and element type, or NULL
    double *d2;                     // [T][B] or NULL
    int32_t *rank, *status;         // [T][B], [B], or NULL
};

// the layout block and the blocks per day from the descriptor's B and lane_block: blk = B (classic) for lane_block 0 or >= B,
// nblk = ceil(B / blk), in 64 bits (B + blk - 1 leaves int for the classic layout with B > 2^30); both results fit an int
inline void fuse_geometry(int B, int lane_block, int *blk, int *nblk)
{
    const int64_t b = (lane_block <= 0 || lane_block >= B) ? (int64_t)B : (int64_t)lane_block;
    *blk = (int)b;
    *nblk = (int)(((int64_t)B + b - 1) / b);
}

// the first pass over Pf / Pb (the upper triangles, for S): every element of it is read again by the products: cached
EPI_DEV double fuse_ld(const void *p, size_t o, int f32)
{
    return f32 ? (double)((const float *)p)[o] : ((const double *)p)[o];
}
// the product pass (and sf / sb, read once): non-temporal, the cache policy of the once-read streams.  For all
// but one path this is the last read of the element; form 0 with p_solver 0 reads the upper triangle of Pf a third time, again
// non-temporally, to form S for the LU solve (the line is then served by L2 or by memory: results do not depend on it)
EPI_DEV double fuse_ld_nt(const void *p, size_t o, int f32)
{
    return f32 ? (double)__builtin_nontemporal_load((const float *)p + o) : __builtin_nontemporal_load((const double *)p + o);
}
// outputs are written once and not read back by this call: non-temporal, rounded once for float storage
EPI_DEV void fuse_st(void *p, size_t o, int f32, double v)
{
    if (f32) __builtin_nontemporal_store((float)v, (float *)p + o);
    else __builtin_nontemporal_store(v, (double *)p + o);
}

template <int M>
__global__ __launch_bounds__(pinv_wg<M>()) void two_filter(const FuseArgs a)
{
    constexpr int WG = pinv_wg<M>();
    constexpr int NS = M * (M + 1) / 2;
    constexpr int LROWS = NS > 2 * M ? NS : 2 * M;
    // one LDS column per lane: scratch of sym_pinv_psd's full-rank route, then the b/z accumulators of the two-sided route
    __shared__ double plds[LROWS * WG];
    auto sx = [](int i, int j) constexpr { return i <= j ? i + j * (j + 1) / 2 : j + i * (i + 1) / 2; };
    const long long wg = a.wg0 + (long long)blockIdx.x;
    const size_t t = (size_t)(wg / (long long)a.tiles);
    const size_t cl = (size_t)(wg % (long long)a.tiles) * (size_t)WG + threadIdx.x;
    const bool live = cl < (size_t)a.B;
    const size_t c = live ? cl : (size_t)a.B - 1;           // tail lanes: a valid item, no stores
    const size_t blk = (size_t)a.blk, cb = c / blk, cr = c - cb * blk;
    const size_t slot = t * (size_t)a.nblk + cb;
    const size_t ov = slot * (size_t)M * blk + cr;          // row r of this item's vector: ov + r * blk
    const size_t om = slot * (size_t)(M * M) * blk + cr;    // entry e = i + M j of its matrix: om + e * blk
    const int f32 = a.f32;
    const double qnan = __builtin_nan("");

    // ---- S = Pf + Pb from the upper triangles, the non-finite guard, X = pinv(S) ----
    double Su[NS], sfv[M], sbv[M];
#pragma unroll
    for (int j = 0; j < M; j++)
#pragma unroll
        for (int i = 0; i <= j; i++)
            Su[sx(i, j)] = fuse_ld(a.Pf, om + (size_t)IXM(i, j) * blk, f32) + fuse_ld(a.Pb, om + (size_t)IXM(i, j) * blk, f32);
#pragma unroll
    for (int i = 0; i < M; i++) {
        sfv[i] = fuse_ld_nt(a.sf, ov + (size_t)i * blk, f32);
        sbv[i] = fuse_ld_nt(a.sb, ov + (size_t)i * blk, f32);
    }
    bool bad = false;
#pragma unroll
    for (int i = 0; i < NS; i++) bad = bad || is_nonfinite(Su[i]);
#pragma unroll
    for (int i = 0; i < M; i++) bad = bad || is_nonfinite(sfv[i]) || is_nonfinite(sbv[i]);
    // a non-finite item does not evaluate the pseudo-inverse: its lane runs the routines on the zero matrix (they return at
    // once) and every output is overwritten with NaN below
#pragma unroll
    for (int i = 0; i < NS; i++) Su[i] = bad ? 0.0 : Su[i];
    double Xu[NS];
    bool capped, indef;
    int rank = sym_pinv_psd<M, WG>(Su, Xu, &capped, &indef, plds + threadIdx.x);
    if (__builtin_amdgcn_ballot_w64(indef) != 0ull) {
        // not positive semi-definite up to rounding: the two-sided Jacobi route on S formed again, exactly as eks_pinv does
        constexpr int BZS = (M >= 6) ? WG : 0;
        double S[M * M], X[M * M];
#pragma unroll
        for (int j = 0; j < M; j++)
#pragma unroll
            for (int i = 0; i <= j; i++) {
                const double v = fuse_ld(a.Pf, om + (size_t)IXM(i, j) * blk, f32) + fuse_ld(a.Pb, om + (size_t)IXM(i, j) * blk, f32);
                S[IXM(i, j)] = bad ? 0.0 : v;
                S[IXM(j, i)] = bad ? 0.0 : v;
            }
        bool capped2;
        const int rank2 = sym_pinv_two_sided<M, BZS>(S, X, &capped2, plds + threadIdx.x);
#pragma unroll
        for (int j = 0; j < M; j++)
#pragma unroll
            for (int i = 0; i <= j; i++) Xu[sx(i, j)] = indef ? X[IXM(i, j)] : Xu[sx(i, j)];
        rank = indef ? rank2 : rank;
        capped = indef ? capped2 : capped;
    }

    // ---- d2 = e' (X e), e = sf - sb ----
    if (a.d2) {
        double e[M], d2 = 0.0;
#pragma unroll
        for (int i = 0; i < M; i++) e[i] = sfv[i] - sbv[i];
#pragma unroll
        for (int i = 0; i < M; i++) {
            double acc = Xu[sx(i, 0)] * e[0];
#pragma unroll
            for (int k = 1; k < M; k++) acc = acc + Xu[sx(i, k)] * e[k];
            d2 = (i == 0) ? e[0] * acc : d2 + e[i] * acc;
        }
        if (live) a.d2[t * (size_t)a.B + c] = bad ? qnan : d2;
    }
    if (live) {
        if (a.rank) a.rank[t * (size_t)a.B + c] = bad ? -1 : rank;
        const int bits = (bad ? 1 : 0) | ((!bad && capped) ? 2 : 0);
        if (a.status && bits) atomicOr(a.status + c, bits);
    }
    if (!a.s_out && !a.P_out) return;                       // wave-uniform

    double s[M];
    if (a.form == 1) {
        // s = Pb (X sf) + Pf (X sb);  Y = X Pb;  P = Pf Y;  P = (P + P') / 2
        double t1[M], t2[M], ya[M], yb[M];
#pragma unroll
        for (int i = 0; i < M; i++) {
            double acc1 = Xu[sx(i, 0)] * sfv[0], acc2 = Xu[sx(i, 0)] * sbv[0];
#pragma unroll
            for (int k = 1; k < M; k++) {
                acc1 = acc1 + Xu[sx(i, k)] * sfv[k];
                acc2 = acc2 + Xu[sx(i, k)] * sbv[k];
            }
            t1[i] = acc1;
            t2[i] = acc2;
        }
        double Y[M * M];
#pragma unroll
        for (int j = 0; j < M; j++) {                       // column j of Pb: term k = j of Pb t1, and column j of Y
            double pb[M];
#pragma unroll
            for (int i = 0; i < M; i++) pb[i] = fuse_ld_nt(a.Pb, om + (size_t)IXM(i, j) * blk, f32);
#pragma unroll
            for (int i = 0; i < M; i++) ya[i] = (j == 0) ? pb[i] * t1[0] : ya[i] + pb[i] * t1[j];
#pragma unroll
            for (int i = 0; i < M; i++) {
                double acc = Xu[sx(i, 0)] * pb[0];
#pragma unroll
                for (int k = 1; k < M; k++) acc = acc + Xu[sx(i, k)] * pb[k];
                Y[IXM(i, j)] = acc;
            }
        }
        double P[M * M];
#pragma unroll
        for (int k = 0; k < M; k++) {                       // column k of Pf: term k of Pf t2 and of every entry of Pf Y
            double pf[M];
#pragma unroll
            for (int i = 0; i < M; i++) pf[i] = fuse_ld_nt(a.Pf, om + (size_t)IXM(i, k) * blk, f32);
#pragma unroll
            for (int i = 0; i < M; i++) yb[i] = (k == 0) ? pf[i] * t2[0] : yb[i] + pf[i] * t2[k];
#pragma unroll
            for (int j = 0; j < M; j++)
#pragma unroll
                for (int i = 0; i < M; i++) P[IXM(i, j)] = (k == 0) ? pf[i] * Y[IXM(0, j)] : P[IXM(i, j)] + pf[i] * Y[IXM(k, j)];
        }
#pragma unroll
        for (int i = 0; i < M; i++) s[i] = ya[i] + yb[i];
        symmetrize<M>(P);                                   // GenericExtendedKalmanFilter.m:138
        if (a.P_out && live) {
#pragma unroll
            for (int e = 0; e < M * M; e++) fuse_st(a.P_out, om + (size_t)e * blk, f32, bad ? qnan : P[e]);
        }
    } else {
        // w = Pb sf + Pf sb;  s = X w;  C = Pf Pb;  P = S \ C (p_solver 0) or X C (p_solver 1), not symmetrised
        double ya[M], yb[M], Pbm[M * M], Cm[M * M];
#pragma unroll
        for (int j = 0; j < M; j++)
#pragma unroll
            for (int i = 0; i < M; i++) Pbm[IXM(i, j)] = fuse_ld_nt(a.Pb, om + (size_t)IXM(i, j) * blk, f32);
#pragma unroll
        for (int i = 0; i < M; i++) {
            double acc = Pbm[IXM(i, 0)] * sfv[0];
#pragma unroll
            for (int k = 1; k < M; k++) acc = acc + Pbm[IXM(i, k)] * sfv[k];
            ya[i] = acc;
        }
#pragma unroll
        for (int k = 0; k < M; k++) {
            double pf[M];
#pragma unroll
            for (int i = 0; i < M; i++) pf[i] = fuse_ld_nt(a.Pf, om + (size_t)IXM(i, k) * blk, f32);
#pragma unroll
            for (int i = 0; i < M; i++) yb[i] = (k == 0) ? pf[i] * sbv[0] : yb[i] + pf[i] * sbv[k];
#pragma unroll
            for (int j = 0; j < M; j++)
#pragma unroll
                for (int i = 0; i < M; i++) Cm[IXM(i, j)] = (k == 0) ? pf[i] * Pbm[IXM(0, j)] : Cm[IXM(i, j)] + pf[i] * Pbm[IXM(k, j)];
        }
        double w[M];
#pragma unroll
        for (int i = 0; i < M; i++) w[i] = ya[i] + yb[i];
#pragma unroll
        for (int i = 0; i < M; i++) {
            double acc = Xu[sx(i, 0)] * w[0];
#pragma unroll
            for (int k = 1; k < M; k++) acc = acc + Xu[sx(i, k)] * w[k];
            s[i] = acc;
        }
        if (a.P_out) {                                      // wave-uniform
            double P[M * M];
            if (a.p_solver == 1) {
#pragma unroll
                for (int j = 0; j < M; j++)
#pragma unroll
                    for (int i = 0; i < M; i++) {
                        double acc = Xu[sx(i, 0)] * Cm[IXM(0, j)];
#pragma unroll
                        for (int k = 1; k < M; k++) acc = acc + Xu[sx(i, k)] * Cm[IXM(k, j)];
                        P[IXM(i, j)] = acc;
                    }
            } else {
                // S \ C = (C' / S')': MATLAB's general square path (dgetf2 + dgetrs) through the existing mrdivide; S is formed
                // again, from the same two loads and the same add as above (non-finite items: the zero matrix, see `bad`)
                double S[M * M], Ct[M * M], R[M * M];
#pragma unroll
                for (int j = 0; j < M; j++)
#pragma unroll
                    for (int i = 0; i <= j; i++) {
                        const double v = fuse_ld_nt(a.Pf, om + (size_t)IXM(i, j) * blk, f32) + Pbm[IXM(i, j)];
                        S[IXM(i, j)] = bad ? 0.0 : v;
                        S[IXM(j, i)] = bad ? 0.0 : v;
                    }
#pragma unroll
                for (int j = 0; j < M; j++)
#pragma unroll
                    for (int i = 0; i < M; i++) Ct[IXM(i, j)] = Cm[IXM(j, i)];
                mrdivide<M>(Ct, S, R);                      // S' = S bit for bit
#pragma unroll
                for (int j = 0; j < M; j++)
#pragma unroll
                    for (int i = 0; i < M; i++) P[IXM(i, j)] = R[IXM(j, i)];
            }
            if (live) {
#pragma unroll
                for (int e = 0; e < M * M; e++) fuse_st(a.P_out, om + (size_t)e * blk, f32, bad ? qnan : P[e]);
            }
        }
    }
    if (a.s_out && live) {
#pragma unroll
        for (int i = 0; i < M; i++) fuse_st(a.s_out, ov + (size_t)i * blk, f32, bad ? qnan : s[i]);
    }
}

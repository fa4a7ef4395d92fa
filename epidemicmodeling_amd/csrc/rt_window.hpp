// Tools/Rt_ExpFitLogLinReg.m, Tools/Rt_ExpFitGenRatios.m, Tools/Rt_ExpFitNonlinLS.m -- the sliding-window growth-rate
// estimators over R series of L days; included by epiekf.hip (entry point epi_rtwin_run_device, include/epiekf.h).
//
// Every array is [L][R] (day-major, region-minor: the new_smoothed layout of epi_preprocess_device), and every kernel puts
// the region index fastest, so a wavefront's window reads are coalesced rows.
//
//   rtw_loglin    : one lane per (day, region).  Closed-form least-squares line through epi_log of the window.
//   rtw_genratios : one lane per (day, region).  log(x(t) / x(t - gp)) / gp and its `filter(ones(1,wlen), wlen, .)` moving
//                   average; the lane recomputes the wlen - 1 earlier ratios itself (bits do not depend on that choice).
//   rtw_nonlin    : one lane per (day, region).  nlinfit's Levenberg-Marquardt fit of A exp(lambda t) to the window (DESIGN
//                   §4.4 lists our reading point by point).  The window, the Jacobian and the residual live in LDS (see
//                   RtwWin): nothing goes to scratch.
//
// log is epi_log and exp is epi_exp (both in ekf_device.hpp): both have a fixed operation order, so tests/rt_window_ref.c
// reproduces every bit, and the LM branches (accept / reject / converge) take the same path on both sides.
#pragma once

constexpr int kRtwMaxSamples = 31;            // wlen 2..31: a centred window holds at most 2 floor(31/2) + 1 = 31 samples
constexpr int kRtwMaxIter = 250;              // optimset MaxIter
constexpr double kRtwTol = 1e-6;              // optimset TolX = TolFun
constexpr double kRtwEps = 2.220446049250313e-16;
constexpr double kRtwSqrtEps = 1.4901161193847656e-08;     // sqrt(eps)
constexpr double kRtwDiffStep = 6.055454452393343e-06;     // eps^(1/3), nlinfit's DerivStep

struct RtwArgs {
    int R, L, wlen, causal, gp, nw, off, lo, hi;   // nw samples per window, sample i of window mm is day mm + off + i;
                                                   // windows mm = lo .. hi - 1 (0-based)
    double time_unit, En, En2, Det, c_ma;          // c_ma = 1 / wlen (filter's b / a(1))
    double n[32], t[32];                           // n_i and t_i = n_i / time_unit, i < nw
    const double *x;
    double *llr_Rt, *llr_A, *llr_Lambda, *llr_ExpFit;
    double *gr_Rt, *gr_Lambda, *gr_RtSmoothed, *gr_LambdaSmoothed;
    double *nls_Rt, *nls_A, *nls_Lambda, *nls_ExpFit;
    int32_t *nls_status, *nls_iters;
};

// ---- Rt_ExpFitLogLinReg -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rtw_loglin(const RtwArgs a)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)a.L * a.R) return;
    const int mm = (int)(idx / a.R), reg = (int)(idx - (int64_t)mm * a.R);
    double ALog = 0.0, r = 0.0;
    if (mm >= a.lo && mm < a.hi) {
        double s = 0.0, ns = 0.0;
        for (int i = 0; i < a.nw; i++) {
            const double seg = epi_log(a.x[(size_t)(mm + a.off + i) * a.R + reg]);
            s = s + seg;
            ns = ns + a.n[i] * seg;
        }
        const double ms = s / (double)a.nw, mns = ns / (double)a.nw;
        ALog = (ms * a.En2 - mns * a.En) / a.Det;
        r = (mns - ms * a.En) / a.Det;
    }
    const double A = epi_exp(ALog), Rt = epi_exp(r);
    const size_t o = (size_t)idx;
    if (a.llr_Rt) a.llr_Rt[o] = Rt;
    if (a.llr_A) a.llr_A[o] = A;
    if (a.llr_Lambda) a.llr_Lambda[o] = r / a.time_unit;
    if (a.llr_ExpFit) a.llr_ExpFit[o] = A * Rt;
}

// ---- Rt_ExpFitGenRatios -------------------------------------------------------------------------------------------
EPI_DEV double rtw_ratio(const RtwArgs &a, int t, int reg)
{
    const double gp = (double)a.gp;
    if (t < a.gp) return 0.0 / gp;
    return epi_log(a.x[(size_t)t * a.R + reg] / a.x[(size_t)(t - a.gp) * a.R + reg]) / gp;
}

__global__ __launch_bounds__(256) void rtw_genratios(const RtwArgs a)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)a.L * a.R) return;
    const int t = (int)(idx / a.R), reg = (int)(idx - (int64_t)t * a.R);
    const double lam = rtw_ratio(a, t, reg), c = a.c_ma;
    // filter(ones(1,wlen), wlen, .): c x(n) + (c x(n-1) + (... + c x(n-wlen+1))), the order of pre_causal_ma
    double acc = 0.0;
    for (int k = a.wlen - 1; k >= 1; k--) {
        const double p = (t - k >= 0) ? c * rtw_ratio(a, t - k, reg) : 0.0;
        acc = p + acc;
    }
    const double lams = c * lam + acc;
    const size_t o = (size_t)idx;
    if (a.gr_Rt) a.gr_Rt[o] = epi_exp(lam * a.time_unit);
    if (a.gr_Lambda) a.gr_Lambda[o] = lam;
    if (a.gr_RtSmoothed) a.gr_RtSmoothed[o] = epi_exp(lams * a.time_unit);
    if (a.gr_LambdaSmoothed) a.gr_LambdaSmoothed[o] = lams;
}

// ---- Rt_ExpFitNonlinLS --------------------------------------------------------------------------------------------
EPI_DEV bool rtw_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// The window y, the Jacobian columns J0, J1 and the residual rv live in LDS, sample i of lane l at [i * 64 + l] (conflict-
// free): held in registers across the fully unrolled loops they spilled to scratch (the unrolled epi_exp evaluations and
// their constants take the registers), so every loop here runs over the runtime window length instead.  Cost: 2 KB of LDS
// per 64-lane block (one wavefront) and window sample, which bounds the occupancy: 14 KB at wlen 7, so 11 wavefronts per CU
// (the 94 VGPRs would allow 20); 62 KB at a centred wlen of 31, so 2.  The flat (day, region) index puts two days in one
// wavefront when R is not a multiple of 64; lanes stay independent, so results do not depend on it.
struct RtwWin {
    double *y, *J0, *J1, *rv;    // + threadIdx.x; element i at [i * 64]
    const double *t;             // [nw], shared by the block
    int nw;
    uint32_t keep;               // bit i: sample i is not NaN
    int nobs;
};

// sse of the model at (b0, b1) over the kept samples; *model_ok: the model is finite at every sample (FunValCheck)
EPI_DEV double rtw_sse(const RtwWin &w, double b0, double b1, bool *model_ok)
{
    double sse = 0.0;
    bool ok = true;
    for (int i = 0; i < w.nw; i++) {
        const double f = b0 * epi_exp(b1 * w.t[i]);
        ok = ok && rtw_finite(f);
        if (w.keep >> i & 1u) { const double rr = w.y[i * 64] - f; sse = sse + rr * rr; }
    }
    *model_ok = ok;
    return sse;
}

// the LM step: [J; diag(sqrt(lam * d))] \ [r; 0; 0] by Householder QR, larger-norm column first.  Rows i < nw of the
// window (a dropped NaN sample is a zero row), then damping row A = [sA, 0] and row B = [0, sB]; sums run in that order.
EPI_DEV void rtw_lm_step(const RtwWin &w, double d0, double d1, double lam, double *s0, double *s1)
{
    const double sA = sqrt(lam * d0), sB = sqrt(lam * d1);
    const double n0sq = d0 + sA * sA, n1sq = d1 + sB * sB;
    const bool piv = n1sq > n0sq;
    const double *P = piv ? w.J1 : w.J0, *Q = piv ? w.J0 : w.J1, *rv = w.rv;
    const double pA = piv ? 0.0 : sA, pB = piv ? sB : 0.0, qA = piv ? sA : 0.0, qB = piv ? 0.0 : sB;
    const double np = sqrt(piv ? n1sq : n0sq);
    if (np == 0.0) { *s0 = 0.0; *s1 = 0.0; return; }
    // first reflector (leading row 0)
    const double alpha = P[0] >= 0.0 ? -np : np;
    const double v0 = P[0] - alpha;
    double vv = v0 * v0, vq = v0 * Q[0], vb = v0 * rv[0];
    for (int i = 1; i < w.nw; i++) {
        const double p = P[i * 64];
        vv = vv + p * p; vq = vq + p * Q[i * 64]; vb = vb + p * rv[i * 64];
    }
    vv = vv + pA * pA; vv = vv + pB * pB;
    vq = vq + pA * qA; vq = vq + pB * qB;
    const double fq = (2.0 * vq) / vv, fb = (2.0 * vb) / vv;
    const double R11 = alpha, R12 = Q[0] - fq * v0, c1 = rv[0] - fb * v0;
    // second reflector (leading row 1) on q' = q - fq v, b' = b - fb v
    const double qpA = qA - fq * pA, qpB = qB - fq * pB, bpA = 0.0 - fb * pA, bpB = 0.0 - fb * pB;
    double nq2 = 0.0;
    for (int i = 1; i < w.nw; i++) { const double qp = Q[i * 64] - fq * P[i * 64]; nq2 = nq2 + qp * qp; }
    nq2 = nq2 + qpA * qpA; nq2 = nq2 + qpB * qpB;
    const double nq = sqrt(nq2);
    const double tol = (double)(w.nobs + 2) * kRtwEps * fabs(R11);
    double xq = 0.0;                                         // rank 1: the basic solution leaves the second column out
    if (nq > tol) {
        const double q1 = Q[64] - fq * P[64], b1 = rv[64] - fb * P[64];
        const double alpha2 = q1 >= 0.0 ? -nq : nq;
        const double w1 = q1 - alpha2;
        double ww = w1 * w1, wb = w1 * b1;
        for (int i = 2; i < w.nw; i++) {
            const double qp = Q[i * 64] - fq * P[i * 64], bp = rv[i * 64] - fb * P[i * 64];
            ww = ww + qp * qp; wb = wb + qp * bp;
        }
        ww = ww + qpA * qpA; ww = ww + qpB * qpB;
        wb = wb + qpA * bpA; wb = wb + qpB * bpB;
        const double g = (2.0 * wb) / ww;
        xq = (b1 - g * w1) / alpha2;
    }
    const double xp = (c1 - R12 * xq) / R11;
    *s0 = piv ? xq : xp;
    *s1 = piv ? xp : xq;
}

// one window: returns the status, writes A, r and the iteration count
EPI_DEV int rtw_fit(const RtwWin &w, double xm, double *A_out, double *r_out, int *iters_out)
{
    int iter = 0;
    const double nan = __builtin_nan("");
    *A_out = nan; *r_out = nan; *iters_out = 0;
    if (w.nobs < 2) return EPI_RTWIN_MODEL_ERROR;            // nlinfit: not enough observations
    double b0 = xm, b1 = 0.0, lam = 0.01;
    bool ok;
    double sse = rtw_sse(w, b0, b1, &ok);
    if (!ok || !rtw_finite(sse)) return EPI_RTWIN_MODEL_ERROR;
    int cause = 0;
    while (iter < kRtwMaxIter) {
        iter++;
        const double a0 = b0, a1 = b1, sseold = sse;
        // forward-difference Jacobian and residual at beta
        const double nb = sqrt(a0 * a0 + a1 * a1);
        const double nbz = nb + (nb == 0.0 ? 1.0 : 0.0);
        const double h0 = kRtwDiffStep * (a0 != 0.0 ? fabs(a0) : nbz), h1 = kRtwDiffStep * (a1 != 0.0 ? fabs(a1) : nbz);
        const double p0 = a0 + h0, p1 = a1 + h1;
        double d0 = 0.0, d1 = 0.0;
        for (int i = 0; i < w.nw; i++) {
            double j0 = 0.0, j1 = 0.0, r = 0.0;
            if (w.keep >> i & 1u) {
                const double ti = w.t[i];
                const double e = epi_exp(a1 * ti);
                const double f = a0 * e;
                r = w.y[i * 64] - f;
                j0 = (p0 * e - f) / h0;
                j1 = (a0 * epi_exp(p1 * ti) - f) / h1;
                d0 = d0 + j0 * j0;
                d1 = d1 + j1 * j1;
            }
            w.J0[i * 64] = j0; w.J1[i * 64] = j1; w.rv[i * 64] = r;
        }
        if (!rtw_finite(d0) || !rtw_finite(d1)) { *iters_out = iter; return EPI_RTWIN_MODEL_ERROR; }
        double s0, s1;
        rtw_lm_step(w, d0, d1, lam, &s0, &s1);
        b0 = a0 + s0; b1 = a1 + s1;
        sse = rtw_sse(w, b0, b1, &ok);
        if (!rtw_finite(sse)) { *iters_out = iter; return EPI_RTWIN_MODEL_ERROR; }
        if (sse < sseold) {
            lam = fmax(lam / 10.0, kRtwEps);
        } else {
            while (sse > sseold) {
                lam = lam * 10.0;
                if (lam > 1e16) { cause = EPI_RTWIN_STALL; break; }
                rtw_lm_step(w, d0, d1, lam, &s0, &s1);
                b0 = a0 + s0; b1 = a1 + s1;
                sse = rtw_sse(w, b0, b1, &ok);
                if (!rtw_finite(sse)) { *iters_out = iter; return EPI_RTWIN_MODEL_ERROR; }
            }
        }
        if (cause) break;
        if (sqrt(s0 * s0 + s1 * s1) < kRtwTol * (kRtwSqrtEps + sqrt(b0 * b0 + b1 * b1))) { cause = EPI_RTWIN_TOLX; break; }
        if (fabs(sse - sseold) <= kRtwTol * sse) { cause = EPI_RTWIN_TOLFUN; break; }
    }
    if (iter >= kRtwMaxIter) cause = EPI_RTWIN_MAXITER;
    *A_out = b0; *r_out = b1; *iters_out = iter;
    return cause;
}

// dynamic LDS: 4 nw * 64 doubles (y, J0, J1, rv) per 64-lane block
__global__ __launch_bounds__(64) void rtw_nonlin(const RtwArgs a)
{
    extern __shared__ double rtw_lds[];
    __shared__ double s_t[kRtwMaxSamples];
    const int64_t idx = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (threadIdx.x < (unsigned)a.nw) s_t[threadIdx.x] = a.t[threadIdx.x];
    __syncthreads();
    if (idx >= (int64_t)a.L * a.R) return;
    const int mm = (int)(idx / a.R), reg = (int)(idx - (int64_t)mm * a.R);
    const double xm = a.x[(size_t)idx];
    double A, r;
    int status, iters = 0;
    if (mm < a.lo || mm >= a.hi) {
        A = a.causal ? 0.0 : xm;                              // causal: filter([zeros(1,wlen-1),1], 1, x) before day wlen
        r = 0.0;
        status = EPI_RTWIN_OUTSIDE;
    } else {
        RtwWin w;
        const size_t col = (size_t)a.nw * 64;
        w.y = rtw_lds + threadIdx.x; w.J0 = w.y + col; w.J1 = w.J0 + col; w.rv = w.J1 + col;
        w.t = s_t; w.nw = a.nw; w.keep = 0; w.nobs = 0;
        int nz = 0;
        for (int i = 0; i < a.nw; i++) {
            const double v = a.x[(size_t)(mm + a.off + i) * a.R + reg];
            w.y[i * 64] = v;
            nz += v != 0.0;                                     // NaN ~= 0
            if (v == v) { w.keep |= 1u << i; w.nobs++; }        // nlinfit drops NaN observations
        }
        if (nz < a.wlen) {
            A = xm; r = 0.0; status = EPI_RTWIN_SKIPPED;
        } else {
            status = rtw_fit(w, xm, &A, &r, &iters);
        }
    }
    const size_t o = (size_t)idx;
    const double Rt = epi_exp(r);
    if (a.nls_Rt) a.nls_Rt[o] = Rt;
    if (a.nls_A) a.nls_A[o] = A;
    if (a.nls_Lambda) a.nls_Lambda[o] = r / a.time_unit;
    if (a.nls_ExpFit) a.nls_ExpFit[o] = A * Rt;
    if (a.nls_status) a.nls_status[o] = status;
    if (a.nls_iters) a.nls_iters[o] = iters;
}

/* The structures of the innovation whiteness diagnostics (epi_idiag_validate / _workspace_bytes / _run_device / _run_host, declared
 * in epiekf.h, which includes this file). */
#ifndef EPIEKF_IDIAG_H
#define EPIEKF_IDIAG_H
#include <stddef.h>
#include <stdint.h>

/* Whiteness diagnostics of the innovations of every chain.
 * Not a script of the reference: its monitor rho is a 21-day running normalised innovation variance per day
 * (Tools/GenericExtendedKalmanFilter.m:172-185); this is the per-chain test of whether a filter run is statistically consistent.
 * Definition (pinned; restated in tests/innov_diag_ref.c).  Chain c, filter step k, row t = k (flip: T-1-k):
 *   counts   k0 <= k < k1, e finite and, with S given, S a normal positive finite number.  S = NaN (the likelihood's "day does
 *              not count"; without S: e = NaN) is skipped silently; any other non-countable value in the window sets bit 0
 *   nu       = e / sqrt(S), or e without S
 *   sums     in blocks of 32 filter steps aligned at k = 0: each block from 0.0 in ascending k, the blocks from 0.0 in ascending
 *              order; every product is rounded before it is added; a term is added only when every step it names counts
 *   pass 1   n, sum1 = sum nu, q = sum nu nu;  mean = sum1 / n;  nis_sum = q;  nis_mean = q / n
 *   pass 2   d = nu - mean;  m2 = sum d d, m3 = sum (d d) d, m4 = sum (d d)(d d);  c_h = sum d(k) d(k+h), h = 1..H, the term in
 *              k's block;  max_abs = max |nu| at max_abs_step = the lowest such k;  with W = k1 - k0, h3 = (2W + 3) / 6 in integers:
 *              f, het_n1 = sum nu nu and count over [k0, k0 + h3), l, het_n2 over [k1 - h3, k1);  CUSUM of squares per counted k:
 *              cs = prefix / q - j / n, prefix = (q of the complete earlier blocks) + (the block's running sum of nu nu through k),
 *              j = the counted steps <= k;  cusumsq_max = max |cs| at cusumsq_step = the lowest such k
 *   var = m2 / n, sd = sqrt(var), skew = (m3 / n) / (var sd), kurt = (m4 / n) / (var var),
 *   jb = (n / 6.0) (skew skew + ((kurt - 3.0)(kurt - 3.0)) / 4.0),  acf[h-1] = c_h / m2,  lb_lags = Hu = min(H, n - 1),
 *   lb_q = (n (n + 2)) sum_{h = 1..Hu ascending from 0.0} (acf_h acf_h) / (n - h),  het = (l / het_n2) / (f / het_n1)
 *   status   bit 0: a bad day;  bit 1: n = 0 -- every double output NaN, the counts 0, the steps -1, no other bit but bit 0;
 *              bit 2: m2 zero or not finite -- acf, skew, kurt, jb, lb_q NaN;  bit 3: Hu < H -- acf rows beyond Hu NaN, lb_q NaN
 *              for Hu = 0.  het is NaN when het_n1 or het_n2 is 0
 * Layout: e as epi_ekf_run_* left the innovations: element (t, c) at t * nblk * blk + c, blk = lane_block (0 or B: the classic
 *   [T][B]), doubles (storage 0) or floats (storage 1, widened on load; all arithmetic is double).  Padding lanes are never
 *   read.  S [T][B] doubles by day, as epi_loglik_run_device writes it, or NULL.  Every output may be NULL, one is required. */
typedef struct epi_idiag_desc {
    int32_t abi_version;
    int32_t B, T;                /* chains, days */
    int32_t lane_block;          /* 0 or B: classic; else chains per layout block of e */
    int32_t storage;             /* 0 = double, 1 = float (e) */
    int32_t flip;                /* 0: row t = k;  1: row t = T-1-k (the *_BWD models) */
    int32_t k0, k1;              /* window of filter steps, 0 <= k0 <= k1 <= T */
    int32_t n_lags;              /* H, 0 .. 64 */
    int32_t reserved;            /* 0 */
} epi_idiag_desc;
typedef struct epi_idiag_inputs {
    const void *e;
    const double *S;             /* or NULL */
} epi_idiag_inputs;
typedef struct epi_idiag_outputs {
    double *mean, *var, *skew, *kurt, *jb, *nis_sum, *nis_mean, *lb_q, *het, *cusumsq_max, *max_abs;   /* [B] */
    int32_t *n, *lb_lags, *het_n1, *het_n2, *cusumsq_step, *max_abs_step, *status;                    /* [B] */
    double *acf;                                                                                       /* [H][B] */
} epi_idiag_outputs;
#endif

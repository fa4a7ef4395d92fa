/* The structures of the curve statistics of the ensembles (epi_cdepth_validate / _workspace_bytes / _run_device / _run_host,
 * declared in epiekf.h, which includes this file). */
#ifndef EPIEKF_CDEPTH_H
#define EPIEKF_CDEPTH_H
#include <stddef.h>
#include <stdint.h>

/* Curve statistics of the Monte-Carlo ensembles: modified band depth, central envelopes, functional boxplot.
 * Not a script of the reference.  The depth is the modified band depth with bands of two curves (Lopez-Pintado and Romo 2009) in
 * the rank form of Sun, Genton and Nychka (2012), the fences are the functional boxplot's (Sun and Genton 2011).
 * src [T][rows][N], N = R * D, region-major (path p = r * D + d), double or float widened once, and the derived row
 * ((N_r v0) v1) v2 as row `rows`, exactly as epi_pathfn_run_* take them; rows' = rows + derive_newcases.
 * Definition (pinned; restated in tests/curve_depth_ref.py and tests/curve_depth_ref.c).
 * Day t of region r and row q: lo_r = max(k0, first_day[r]) (first_day 0 without the array); the day is a day of the item when
 *   lo_r <= t < k1.  A member d is VALID on it when its value v_d is not NaN; +Inf and -Inf are values.  n_t = the valid members,
 *   below = #{e valid : v_e < v_d}, above = #{e valid : v_e > v_d}, C(n) = n (n - 1) / 2,
 *   c_t(d) = C(n_t) - C(below) - C(above): the pairs of valid members whose closed band holds v_d.
 * Per path and row over the days of the item on which the path is valid (exact integers):
 *   band_count = sum c_t(d), pair_total = sum C(n_t), le_count = sum (n_t - above), member_total = sum n_t, n_valid = the days;
 *   depth = band_count / pair_total (NaN when pair_total = 0), mhi = le_count / member_total (NaN when n_valid = 0): one
 *   division of the two integers as doubles each.  band_count and pair_total are written as doubles (below 2^53).
 * Per (row, region): a path is RANKED when depth is not NaN; n_ranked their number;
 *   depth_rank(d) = #{e : depth_e > depth_d} + #{e < d : depth_e == depth_d} (0 the deepest), -1 for an unranked path;
 *   median_path = the d of rank 0, -1 without a ranked path.
 * Central regions, alpha[k] in (0, 1] strictly ascending: m_k = min(n_ranked, max(1, (int)ceil(alpha[k] * (double)n_ranked)));
 *   env_lo / env_hi [t][k] = the min / max over the paths with 0 <= depth_rank < m_k that are valid on day t of the item, NaN
 *   without one.  Of zeros of both signs the min is -0.0 and the max +0.0.  median_curve[t] = the value of median_path on day
 *   t of the item (NaN without a median path).
 * Functional boxplot (fence_factor > 0): lo, hi the envelope of the m_f deepest paths, m_f from fence_frac as m_k from alpha;
 *   w = hi - lo; lo_f = lo - fence_factor * w; hi_f = hi + fence_factor * w (one rounding per written operation, no fma);
 *   out_days(d) = #{valid days of d with v < lo_f or v > hi_f} (a NaN fence: both false); n_outliers = #{ranked paths with
 *   out_days > 0}; whisk_lo / whisk_hi [t] = the min / max over the ranked paths with out_days = 0 that are valid on day t.
 * Per-day outputs hold NaN on the days outside [lo_r, k1).  Every output may be NULL, one is required. */
typedef struct epi_cdepth_desc {
    int32_t abi_version;
    int32_t T, rows, R;          /* days, rows of src (1 .. 4096), regions: each >= 1 */
    int32_t D;                   /* draws per region, 1 .. 4096; R * D <= INT32_MAX */
    int32_t n_alpha;             /* central regions, 0 .. 8 */
    int32_t storage;             /* element type of src: 0 = double, 1 = float */
    int32_t derive_newcases;     /* 0, or 1: append the row ((N * row0) * row1) * row2 */
    int32_t k0, k1;              /* the window, 0 <= k0 < k1 <= T */
    int32_t test_segments;       /* 0: one wavefront per 32-day block; > 0: time segments wanted, at most min(ceil(W / 32), 1024) */
    int32_t test_launch_groups;  /* 0; > 0: workgroups per launch (the tests cut small calls into several launches with it) */
    double alpha[8];             /* the first n_alpha: each in (0, 1], strictly ascending */
    double fence_factor;         /* 0: no boxplot; > 0: the fences' factor (1.5 is the customary one) */
    double fence_frac;           /* in (0, 1] when fence_factor > 0 (0.5 is the customary one) */
} epi_cdepth_desc;
typedef struct epi_cdepth_inputs {
    const void *src;                     /* [T][rows][R * D] */
    const double *population;            /* [R] (derive_newcases) or NULL */
    const int32_t *first_day;            /* [R] or NULL */
} epi_cdepth_inputs;
typedef struct epi_cdepth_outputs {
    double *depth, *mhi, *band_count, *pair_total;      /* [rows'][N] */
    int32_t *n_valid, *depth_rank, *out_days;           /* [rows'][N] */
    int32_t *n_ranked, *median_path, *n_outliers;       /* [rows'][R] */
    double *env_lo, *env_hi;                            /* [T][n_alpha][rows'][R] */
    double *median_curve, *whisk_lo, *whisk_hi;         /* [T][rows'][R] */
} epi_cdepth_outputs;
#endif

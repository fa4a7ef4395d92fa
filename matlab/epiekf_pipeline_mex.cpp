// epiekf_pipeline_mex.cpp -- MEX gateway for the stages of Tools/TrainPredictPrescribeNPI.m around the filter, each for ALL
// regions in one call (include/epiekf.h: the *_host entry points).  The REGION index is the FIRST dimension of every array,
// so MATLAB's column-major arrays are the ABI's region-minor arrays without any transposition.
//
//   out = epiekf_pipeline_mex('prescribe', x, u, R_v, prm, s_init, Ps_init, s_final, Ps_final, Q_w, epsilons, sp, J0_prefix,
//                             J1_prefix, t_hist, L, order, obs_type, devices)
//       the cost-weight sweep of every region -- SIAlphaModelEKFOptControlled for each epsilon, the scenario scoring and the
//       Pareto front (Tools/TrainPredictPrescribeNPI.m:421-493, 624-633) -- on the GPUs listed in `devices` (zero-based ids,
//       [] = device 0).  x, R_v  R x T (NaN over the horizon);  u  R x n_npi x T (NaN = choose optimally);  prm  R x 61
//       (epiekf_pack_params per region; its epsilon entry is ignored);  s_init, s_final  R x 6;  Ps_init, Ps_final, Q_w
//       R x 36 (vec'd matrices);  epsilons  P x 1 = human_npi_cost_factor;  sp  R x 48 (EPI_SIM_* columns: s/i/alpha_historic
//       (end), model constants, NPI_MAXES, npi_weights);  J0_prefix, J1_prefix  R x 1 (sequential historic sums of NPICost).
//       out.J0, out.J1  P x R (column r = J0_opt_control of region r);  out.on_front  P x R (logical as double);
//       out.I_opt  R x 1 (ONE-based);  out.u_opt  R x n_npi x T = opt_control_input_smooth of the optimum;  out.S_opt
//       R x 6 x T = its S_SMOOTH.
//   out = epiekf_pipeline_mex('preprocess', cases, deaths, population, ip, W, first_num_days, min_cases)
//       :142-198, 201-202, 240.  cases, deaths ([] = none)  S x T cumulative counts;  population  S x 1;  ip ([] = none)
//       S x n_npi x T.  Fields new_refined, new_smoothed, zero_lag, x_new, x_total, R_v, fatality (S x T), I0 (S x 1),
//       ip_filled (S x n_npi x T).
//   [a, b, min_err, iters] = epiekf_pipeline_mex('nnls', X, y, max_iters)
//       :251-276 ('NONNEGATIVELS').  X  S x n x D = NPI_MAXES - InterventionPlans over the window;  y  S x D;  a  S x n;
//       b, min_err, iters  S x 1.
//   [a, b, lambda, mse, se, idx, idx1se, B, intercept, df] = epiekf_pipeline_mex('lasso', X, y, K, fold)
//       :254-290 ('LASSO'): lasso(X, y, 'CV', K) per region with MATLAB's defaults, the partition given.
//       X  R x n x D (as for 'nnls');  y  R x D;  fold  R x D with values 1 .. K (fold(r, t) = k: day t is in the test set
//       of fold k; [] when K = 0: the path only).  a  R x n = B(:, IndexMinMSE);  b  R x 1 = Intercept(IndexMinMSE);
//       lambda, mse, se, intercept, df  R x NumLambda (ascending lambda, MATLAB's order);  idx, idx1se  R x 1
//       (IndexMinMSE, Index1SE, ONE-based);  B  R x n x NumLambda.  A region whose X / y holds Inf or NaN gets NaN outputs
//       and idx = idx1se = 0; with K = 0, a, b, mse and se are NaN and idx = idx1se = 0.  (No lasso.m is shipped: it would shadow the Statistics Toolbox function.)
//   [a, b, b_item, sigma, iters, status, weights] = epiekf_pipeline_mex('robustfit', X, y, robust, lower, upper, max_iter)
//       :279-292 ('NONNEGATIVELS-ELEMENT-WISE'): for every NPI on its own fit(X(:,k), y, 'a*x+b', 'Robust','on',
//       'Lower',[lower -inf]) as bisquare iteratively reweighted least squares, then b = mean(y - X*a).
//       X  R x n x D (as for 'nnls');  y  R x D;  robust  0 or 1;  lower, upper  the slope's bounds (the reference: 0, Inf);
//       max_iter  1 .. 100000 (50).  a, b_item, sigma, iters, status  R x n (status: bits 1 non-finite, 2 constant column,
//       4 slope lost, 8 iteration cap, 16 bound active);  b  R x 1;  weights  R x n x D (only when requested).
//   [lambda_hat, new_cases_est, map, status, x_mx, y_filled, tracker] = epiekf_pipeline_mex('ratemap', ip, y, new_smoothed, extra,
//           lambda_in, n_train, lags, ridge, lambda_threshold, reduction_effect, effect_lag)
//       The NPI-to-growth-rate predictor of testScripts/test04FullFeatureExtMLpipeline.m (:292-404, :418-431, :576-642) for R
//       regions x K train ends.  ip  R x n x T, N/A-filled;  y ([] with lambda_in)  R x T, the growth rate;
//       new_smoothed  R x T;  extra ([] = none)  R x E x T caller-made columns;  lambda_in ([] = fit the linear map)  R x T x K:
//       taken as lambda_hat, clipped and rebuilt;  n_train  K train ends (numTimeStepsTrain, 1 .. T);  lags  0 .. 3 lags
//       (the reference: [3 5 7]);  ridge (1e-6), lambda_threshold (0.1), reduction_effect (0.01), effect_lag (3).
//       lambda_hat, new_cases_est  R x T x K;  map  R x F x K, F = n (1 + numel(lags)) + E ([] without a fit);  status  R x K
//       (bits 1 leading NaN target, 2 not positive definite, 4 non-finite);  x_mx  R x F;  y_filled  R x T ([] without y);
//       tracker  R x T.
//   [m, rank, perm, rdiag, resid, fitted, status] = epiekf_pipeline_mex('mldivide', X, y, n_rows, tol_scale)
//       MATLAB's rectangular backslash X(1:n_rows(k),:) \ y(1:n_rows(k)) of test01FitExponential.m:159, test03 :169 and test05
//       :185 for R regions x K row counts: Householder QR with column pivoting, the rank by
//       abs(R(j,j)) > tol_scale * max(n_rows, F) * eps * abs(R(1,1)) (tol_scale 1: lscov's rule), the basic solution.
//       X  R x F x D (F <= 96, max(n_rows) * (F + 1) <= 20000);  y  R x D;  n_rows  K row counts 1 .. D ([] = D);  tol_scale (1).
//       m, rdiag  R x F x K;  perm  R x F x K, 1-based column numbers in pivot order;  rank, resid, status  R x K (status: bits
//       1 rank deficient, 2 non-finite input, 4 non-finite result);  fitted  R x D x K, X * m over all D rows.
//   [beta, bias, w, fitted, n_iter, gap, n_sv, status] = epiekf_pipeline_mex('svr', X, y, n_rows, kernel, box, epsilon, kernel_scale, tol, max_iter)
//       The fitrsvm rows of test05DirectNewCasesLearning.m:198-268, test04 :435-445 and test03 :242-262 for R regions x K row
//       counts: epsilon-insensitive support-vector regression by LIBSVM's sequential minimal optimisation.
//       X  R x F x D (F <= 96, n_rows <= 1024, max(n_rows) * (bitor(F, 1) + 1) <= 20000);  y  R x D;  n_rows  K row counts 1 .. D
//       ([] = D);  kernel  0 linear, 1 Gaussian;  box, epsilon, kernel_scale  a scalar or R values;  tol ([] = 1e-3);  max_iter
//       ([] = 100000).  beta, fitted  R x D x K;  w  R x F x K ([] for the Gaussian kernel);  bias, n_iter, gap, n_sv, status
//       R x K (status: bits 1 not converged, 2 bad input, 4 non-finite result).
//   [mean, std, min, max, quantiles, count] = epiekf_pipeline_mex('ens_summary', src, D, q, population)
//       Monte-Carlo ensemble statistics (BASELINE config 5).  src  B x rows x T (or B x T), B = R * D chains,
//       region-major (chain = (r-1) * D + d): a filter output such as S_SMOOTH;  D  draws per region;  q  1 .. 16
//       probabilities in [0, 1] (quantile(x, q)'s rule);  population ([] = none)  R x 1: appends the row
//       ((N * row1) * row2) * row3.  NaN members are excluded.  mean, std, min, max, count  R x rows' x T;  quantiles
//       R x rows' x n_q x T.
//   [S, A, noise_var, status] = epiekf_pipeline_mex('ar_forecast', seg, prm, dt, p, H, D, z, drive, drive_series, A, noise_var, nv_mode)
//       The autoregressive alpha forecaster of Tools/PrescribeNPI.m:204-241 for R regions x D draws:
//       ar(seg, p) -> filtic -> filter(sqrt(nv), A, z, zi) (+ drive) -> negatives to 0 -> SI_Controlled.  seg  R x L;  prm  R x 3
//       (beta, s0, i0);  z ([] = zeros)  B x H standard-normal draws, B = R * D, chain = (r-1) * D + d;  drive ([] = none)
//       Sd x H, added before the clamp;  drive_series ([] : Sd == B)  B x 1, ONE-based;  A, noise_var ([] , [] = fit the
//       model)  R x p and R x 1: get(ar_sys, 'A')(2:end) and get(ar_sys, 'NoiseVariance') -- which normalisation MATLAB's
//       NoiseVariance uses is not pinned by the reference, nv_mode (0 or 1) chooses ours when the model is fitted.
//       S  B x 3 x (L + H), rows (s, i, alpha_hat): what 'ens_summary' takes;  A  R x p (a_1 .. a_p);  noise_var, status
//       R x 1 (0 ok, 1 rank-deficient: NaN from day L + 1 on, 2 non-finite seg: NaN).  An optional 14th input `seed` (see 'noise')
//       with z = []: the draws 'noise'(H, 1, B, seed) are generated inside the kernel.
//   [S_FRW_BCK, P_FRW_BCK, d2, rank] = epiekf_pipeline_mex('fuse', S_f, P_f, S_b, P_b, form, p_solver)
//       The "Backward filtering (under test)" fusion of :464-478 for one chain.  S_f, S_b  m x T and P_f, P_b
//       m x m x T (m = 3 or 6): the outputs of a forward filter and of its reverse-time twin as they come back (un-flipped);
//       forward S_PLUS / P_PLUS with backward S_MINUS / P_MINUS counts day t's observation once, PLUS with PLUS is the
//       reference's choice.  form  0 = the reference's two lines as written (p_solver 0: S \ C by LU, 1: pinv(S) * C),
//       1 = the information form Pf X Pb, symmetrised (p_solver 0); both required.  S_FRW_BCK  m x T;  P_FRW_BCK  m x m x T;
//       d2  1 x T, (S_f - S_b)' pinv(P_f + P_b) (S_f - S_b);  rank  1 x T, the rank pinv kept (-1: a non-finite day, NaN).
//   [loglik, nis_mean, n_valid, status, S, nis, R_used] = epiekf_pipeline_mex('loglik', model_id, S_MINUS, P_MINUS, innovations, x, R_v, prm, L, obs_type, k_first, k_last)
//       The Gaussian innovation log-likelihood of one chain from a filter run's outputs, the arguments in the
//       order of epi_loglik_inputs.  model_id, obs_type  as epiekf_mex takes them;  S_MINUS  m x T;  P_MINUS  m x m x T;
//       innovations, x  1 x T;  R_v  1 x T (a series, by filter step) or a scalar (the filter's adaptive R is replayed);  prm
//       the filter's parameter vector (EPI_PRM_COUNT entries);  L  inv_monitor_len;  k_first, k_last ([] = 1, T)  the filter steps
//       that count, ONE-based and inclusive.  loglik, nis_mean, n_valid, status  scalars;  S, nis, R_used  1 x T by day (NaN where
//       the day does not count).
//   [plan, J0, J1, F, gap, iters, halvings, status, states, mu, F_trace] = epiekf_pipeline_mex('plan', sp, u_min, eps, H, u_fixed, u_init, J0_prefix, J1_prefix, prefix_days, max_iter, max_halvings, tol)
//       The direct optimal-NPI planner: for every (region, cost weight) the horizon's plan from the states run
//       forward and the adjoint run backward, Frank-Wolfe steps with backtracking; a stationary point with its gap.  sp  R x 48;
//       u_min  R x n_npi;  eps  P cost weights;  H  days;  u_fixed ([] = all free)  R x n_npi x H, NaN = free;  u_init ([] =
//       u_min)  (P*R) x n_npi x H;  J0_prefix, J1_prefix ([] with prefix_days 0)  R x 1.  Chain (r-1) * P + l.  plan  (P*R) x
//       n_npi x H;  J0 .. status  P x R (status 0: gap <= tol |F|; bit 0: max_iter passes; bit 1: no descending step; bit 2:
//       F not finite);  states, mu  (P*R) x 3 x H and F_trace  (P*R) x max_iter (NaN beyond iters), only when requested.
//   [X, rank, status, J, L] = epiekf_pipeline_mex('sdraw', S_PLUS, P_PLUS, S_MINUS, P_MINUS, prm, D, z, s_term, P_term, k_first, clamp)
//       Joint posterior draws of the smoothed path of ONE 3-state chain by backward simulation.  S_PLUS, S_MINUS
//       3 x T;  P_PLUS, P_MINUS  3 x 3 x T;  prm  the filter's parameter vector (EPI_PRM_COUNT entries);  D  draws;  z ([] = no
//       noise: with the clamp the path is S_SMOOTH)  D x 3 x (T - k_first + 1) standard-normal inputs;  s_term, P_term ([] = S_PLUS,
//       P_PLUS of day T)  3 x 1, 3 x 3;  k_first ([] = 1)  the first day returned, ONE-based;  clamp ([] = 1).  X  D x 3 x
//       (T - k_first + 1);  rank  1 x T (-1: a NaN record);  status  scalar (bit 0: a non-finite input entry met, bit 1: a rank
//       below 3);  J, L  3 x 3 x T, only when requested.  An optional 13th input `seed` (see 'noise') with z = []: "D draws,
//       seed 7" -- the draws 'noise'(T - k_first + 1, 3, D, seed) are generated inside the kernel and no z is made or copied.
//   [crps, wis, ae, width, rank, ties, cover, count, crps_mean, wis_mean, ae_mean, n_scored, cover_frac, pit_hist] = epiekf_pipeline_mex('escore', src, truth, D, alpha, n_bins, population, truth_series, first_day, k_first, k_last)
//       Probabilistic forecast scores of a Monte-Carlo ensemble against a truth.  src, D, population  as
//       'ens_summary' takes them;  truth  Rt x rows' x T (or Rt x T for a B x T src);  alpha ([] = none)  up to 8 levels of
//       central intervals in (0, 1), strictly descending;  n_bins  0 .. 32 bins of the rank histogram;  truth_series ([] : Rt == R)
//       R x 1, ONE-based column of truth of every region;  first_day ([] = 1)  R x 1, ONE-based first day a region is scored
//       from;  k_first, k_last ([] = 1, T)  the days the per-region outputs run over, ONE-based and inclusive.  crps, wis, ae,
//       rank, ties, cover, count  R x rows' x T (rank, ties -1 and NaN scores: not scored);  width  R x rows' x n_a x T;
//       crps_mean, wis_mean, ae_mean, n_scored  R x rows';  cover_frac  R x rows' x n_a;  pit_hist  R x rows' x n_bins.
//   [es, vs, truth_term, spread_term, n_members, n_days, member_dist] = epiekf_pipeline_mex('jscore', src, truth, D, vs_p, max_lag, population, truth_series, first_day, k_first, k_last)
//       Joint scores of a Monte-Carlo ensemble's paths against a truth: the energy score and the variogram score of every (row,
//       region) over a window of days.  src, truth, D, population, truth_series, first_day, k_first, k_last  as
//       'escore' takes them;  vs_p ([] or 0 = no variogram score)  0.5 or 1;  max_lag ([] = 0: every pair of days)  the largest
//       distance in days of a pair in the variogram score.  es, vs (NaN without vs_p), truth_term, spread_term, n_members,
//       n_days  R x rows';  member_dist  B x rows' (NaN: an absent member).
//   [depth, mhi, depth_rank, median_path, median_curve, env_lo, env_hi, whisk_lo, whisk_hi, out_days, n_outliers, n_ranked, band_count, pair_total, n_valid] = epiekf_pipeline_mex('cdepth', src, D, alpha, fence_factor, fence_frac, population, first_day, k_first, k_last)
//       Curve statistics of a Monte-Carlo ensemble: modified band depth, central envelopes, functional boxplot.
//       src, D, population, first_day, k_first, k_last  as 'pathfn' takes them;  alpha ([] = [0.5 0.9])  up to 8 fractions in (0, 1],
//       ascending;  fence_factor ([] = 1.5; 0 = no boxplot), fence_frac ([] = 0.5).  depth, mhi, band_count, pair_total, n_valid,
//       out_days  B x rows';  depth_rank  B x rows', ONE-based (1 = the deepest path of its region, 0 = unranked);  median_path,
//       n_outliers, n_ranked  R x rows' (median_path ONE-based within the region, 0 = none);  median_curve, whisk_lo, whisk_hi
//       R x rows' x T;  env_lo, env_hi  R x rows' x n_alpha x T.  Days outside the window are NaN; without a boxplot out_days,
//       n_outliers are 0 and the whiskers NaN.
//   [peak_value, peak_day, min_value, min_day, total, first_cross, days_above, longest_run, n_valid, n_paths, peak_day_hist, n_cross, cross_day_hist] = epiekf_pipeline_mex('pathfn', src, D, thr, population, first_day, k_first, k_last)
//       Functionals of every joint path of a Monte-Carlo ensemble.  src, D, population  as 'ens_summary' takes
//       them;  thr ([] = none)  R x rows' x n_thr (R x n_thr for a B x T src), at most 8 thresholds, NaN = not asked;  first_day
//       ([] = 1)  R x 1, ONE-based first day of every region;  k_first, k_last ([] = 1, T)  the window, ONE-based and inclusive.
//       peak_value, min_value, total, n_valid  B x rows';  peak_day, min_day  B x rows', ONE-based days;  first_cross (ONE-based,
//       NaN: never), days_above, longest_run  B x rows' x n_thr;  n_paths  R x rows';  peak_day_hist  R x rows' x W (W = k_last -
//       k_first + 1, at most 4096);  n_cross  R x rows' x n_thr;  cross_day_hist  R x rows' x n_thr x W.
//   [stats, acf] = epiekf_pipeline_mex('idiag', e, S, n_lags, k_first, k_last, flip)
//       Whiteness diagnostics of one chain's innovations (the statistics only -- p-values are left to the
//       caller's chi2cdf).  e  1 x T innovations;  S  1 x T innovation variances by day (the 'loglik' command's S; NaN = the day
//       does not count) or [] (e is taken as standardised);  n_lags  0 .. 64;  k_first, k_last ([] = 1, T)  the filter steps that
//       count, ONE-based and inclusive;  flip  0, or 1 for a backward model (filter step k is day T+1-k).  stats  18 x 1 in the
//       order of epi_idiag_outputs: mean, var, skew, kurt, jb, nis_sum, nis_mean, lb_q, het, cusumsq_max, max_abs, n, lb_lags,
//       het_n1, het_n2, cusumsq_step, max_abs_step (both ONE-based; 0: none), status;  acf  n_lags x 1.
//   [J0, J1, u] = epiekf_pipeline_mex('mc', sp, u_min, n_scen, K, seed, z, J0_prefix, J1_prefix, prefix_days)
//       :496-521.  sp  R x 48;  u_min  R x n_npi;  z ([] = noise-free)  (n_scen*R) x 3 x K;  J0, J1  R x n_scen;
//       u  (n_scen*R) x n_npi x K (only when requested).  An optional 11th input `noise_seed` (see 'noise'; it may equal seed)
//       with z = []: the state noise 'noise'(K, 3, n_scen*R, noise_seed) is generated inside the kernel.
//   z = epiekf_pipeline_mex('noise', nt, rows, lanes, seed, t0, lane0)
//       Standard-normal draws from a seed: the window [t0, t0 + nt) x rows x [lane0, lane0 + lanes) of the
//       array the seed stands for (t0, lane0 ZERO-based offsets, [] or absent = 0), z  lanes x rows x nt.  rows 1 or 3.  seed  a
//       double scalar (an integer in 0 .. 2^53) or [seed, stream] with stream < 2^30.  A command given `seed` equals the same
//       command given z = 'noise'(...) of its z's shape, bit for bit.  |z| <= 8.21.
// Build on a MATLAB host:  mex -I../include epiekf_pipeline_mex.cpp -L../epidemicmodeling_amd -lepiekf
#include <stdio.h>
#include <string.h>
#include <limits>
#include <vector>
#include "mex.h"
#include "epiekf.h"

static void fail_if(int rc, const char *err)
{
    if (rc != EPI_OK) mexErrMsgIdAndTxt("epiekf:error", "%s (%s)", err, epi_status_string(rc));
}
static const double *opt(const mxArray *a) { return mxIsEmpty(a) ? NULL : mxGetPr(a); }
// the optional seed argument at position k: absent or [] = none (false); a double scalar or [seed, stream]
static bool seed_arg(int nrhs, const mxArray *prhs[], int k, epi_noise_desc *nd)
{
    if (nrhs <= k || mxIsEmpty(prhs[k])) return false;
    const mwSize n = mxGetNumberOfElements(prhs[k]);
    if (!mxGetPr(prhs[k]) || n > 2) mexErrMsgTxt("seed must be a double scalar or [seed, stream]");
    const double sd = mxGetPr(prhs[k])[0], st = n == 2 ? mxGetPr(prhs[k])[1] : 0.0;
    if (!(sd >= 0.0 && sd <= 9007199254740992.0) || (double)(uint64_t)sd != sd) mexErrMsgTxt("seed must be an integer in 0 .. 2^53");
    if (!(st >= 0.0 && st < 4294967296.0) || (double)(uint64_t)st != st) mexErrMsgTxt("stream must be a non-negative integer");
    memset(nd, 0, sizeof *nd);
    nd->abi_version = EPIEKF_ABI_VERSION; nd->seed_lo = (uint32_t)((uint64_t)sd & 0xFFFFFFFFu); nd->seed_hi = (uint32_t)((uint64_t)sd >> 32);
    nd->stream = (uint32_t)st;                             // 2^30 and above reach the library's own check
    return true;
}
static void want(const mxArray *a, mwSize rows, mwSize cols, const char *what)
{
    if (mxGetM(a) != rows || mxGetN(a) != cols) mexErrMsgIdAndTxt("epiekf:arg", "%s must be %d x %d", what, (int)rows, (int)cols);
}
static mxArray *dbl3(mwSize a, mwSize b, mwSize c)
{
    const mwSize d[3] = {a, b, c};
    return mxCreateNumericArray(3, d, mxDOUBLE_CLASS, mxREAL);
}

static void prescribe(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    (void)nlhs;
    // (an optional 20th input: epi_prescribe_desc.placement_tries -- the first sweep of a size keeps the fastest of that many device arenas)
    if (nrhs != 19 && nrhs != 20) mexErrMsgTxt("epiekf_pipeline_mex('prescribe', ...): 19 inputs expected (+ optional placement_tries)");
    const mxArray *x = prhs[1], *u = prhs[2];
    if (mxGetNumberOfDimensions(u) != 3) mexErrMsgTxt("u must be R x n_npi x T");
    const mwSize *du = mxGetDimensions(u);
    const mwSize R = du[0], n = du[1], T = du[2], P = mxGetNumberOfElements(prhs[10]);
    want(x, R, T, "x"); want(prhs[3], R, T, "R_v"); want(prhs[4], R, EPI_PRM_COUNT, "prm");
    want(prhs[5], R, 6, "s_init"); want(prhs[6], R, 36, "Ps_init"); want(prhs[7], R, 6, "s_final"); want(prhs[8], R, 36, "Ps_final");
    want(prhs[9], R, 36, "Q_w"); want(prhs[11], R, EPI_SIM_PRM_COUNT, "sp");
    if (mxGetNumberOfElements(prhs[12]) != R || mxGetNumberOfElements(prhs[13]) != R) mexErrMsgTxt("J0_prefix, J1_prefix must have one entry per region");
    if (P < 1) mexErrMsgTxt("epsilons is empty");
    epi_prescribe_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION; d.R = (int32_t)R; d.P = (int32_t)P; d.T = (int32_t)T; d.t_hist = (int32_t)mxGetScalar(prhs[14]);
    d.n_npi = (int32_t)n; d.L = (int32_t)mxGetScalar(prhs[15]); d.order = (int32_t)mxGetScalar(prhs[16]); d.obs_type = (int32_t)mxGetScalar(prhs[17]);
    if (nrhs == 20) d.placement_tries = (int32_t)mxGetScalar(prhs[19]);
    epi_prescribe_inputs in;
    memset(&in, 0, sizeof in);
    in.x = mxGetPr(x); in.u = mxGetPr(u); in.R_series = mxGetPr(prhs[3]); in.prm = mxGetPr(prhs[4]);
    in.s_init = mxGetPr(prhs[5]); in.Ps_init = mxGetPr(prhs[6]); in.s_final = mxGetPr(prhs[7]); in.Ps_final = mxGetPr(prhs[8]);
    in.Q = mxGetPr(prhs[9]); in.eps = mxGetPr(prhs[10]); in.sp = mxGetPr(prhs[11]); in.J0_prefix = mxGetPr(prhs[12]); in.J1_prefix = mxGetPr(prhs[13]);
    std::vector<int> devs;
    for (mwSize k = 0; k < mxGetNumberOfElements(prhs[18]); k++) devs.push_back((int)mxGetPr(prhs[18])[k]);
    if (devs.empty()) devs.push_back(0);
    const char *names[] = {"J0", "J1", "on_front", "I_opt", "u_opt", "S_opt"};
    mxArray *f[6] = {mxCreateDoubleMatrix(P, R, mxREAL), mxCreateDoubleMatrix(P, R, mxREAL), mxCreateDoubleMatrix(P, R, mxREAL),
                     mxCreateDoubleMatrix(R, 1, mxREAL), dbl3(R, n, T), dbl3(R, 6, T)};
    std::vector<int32_t> on((size_t)(R * P)), iopt((size_t)R);
    epi_prescribe_outputs out;
    memset(&out, 0, sizeof out);
    out.J0 = mxGetPr(f[0]); out.J1 = mxGetPr(f[1]); out.on_front = on.data(); out.i_opt = iopt.data();
    out.u_opt = mxGetPr(f[4]); out.S_opt = mxGetPr(f[5]);
    char err[256] = {0};
    const int rc = epi_sweep_prescribe_host(&d, &in, &out, (int)devs.size(), devs.data(), err);
    if (rc != EPI_OK) { for (mxArray *a : f) mxDestroyArray(a); fail_if(rc, err); }
    for (size_t k = 0; k < on.size(); k++) mxGetPr(f[2])[k] = (double)on[k];
    for (size_t k = 0; k < iopt.size(); k++) mxGetPr(f[3])[k] = (double)iopt[k] + 1.0;      // MATLAB indices start at one
    plhs[0] = mxCreateStructMatrix(1, 1, 6, names);
    for (int k = 0; k < 6; k++) mxSetFieldByNumber(plhs[0], 0, k, f[k]);
}

static void preprocess(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    (void)nlhs;
    if (nrhs != 8) mexErrMsgTxt("epiekf_pipeline_mex('preprocess', cases, deaths, population, ip, W, first_num_days, min_cases): 8 inputs expected");
    const mwSize S = mxGetM(prhs[1]), T = mxGetN(prhs[1]);
    const bool has_d = !mxIsEmpty(prhs[2]), has_ip = !mxIsEmpty(prhs[4]);
    if (has_d) want(prhs[2], S, T, "deaths");
    if (mxGetNumberOfElements(prhs[3]) != S) mexErrMsgTxt("population must have one entry per region");
    mwSize n = 0;
    if (has_ip) {
        if (mxGetNumberOfDimensions(prhs[4]) != 3 || mxGetDimensions(prhs[4])[0] != S || mxGetDimensions(prhs[4])[2] != T) mexErrMsgTxt("ip must be S x n_npi x T");
        n = mxGetDimensions(prhs[4])[1];
    }
    epi_pre_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION; d.S = (int32_t)S; d.T = (int32_t)T; d.n_npi = (int32_t)n; d.W = (int32_t)mxGetScalar(prhs[5]);
    d.first_num_days = (int32_t)mxGetScalar(prhs[6]); d.min_cases = mxGetScalar(prhs[7]);
    const char *names[] = {"new_refined", "new_smoothed", "zero_lag", "x_new", "x_total", "R_v", "fatality", "I0", "ip_filled"};
    mxArray *f[9];
    for (int k = 0; k < 7; k++) f[k] = (k == 6 && !has_d) ? mxCreateDoubleMatrix(0, 0, mxREAL) : mxCreateDoubleMatrix(S, T, mxREAL);
    f[7] = mxCreateDoubleMatrix(S, 1, mxREAL);
    f[8] = has_ip ? dbl3(S, n, T) : mxCreateDoubleMatrix(0, 0, mxREAL);
    epi_pre_outputs out;
    memset(&out, 0, sizeof out);
    out.new_refined = mxGetPr(f[0]); out.new_smoothed = mxGetPr(f[1]); out.zero_lag = mxGetPr(f[2]); out.x_new = mxGetPr(f[3]);
    out.x_total = mxGetPr(f[4]); out.R_v = mxGetPr(f[5]); out.fatality = has_d ? mxGetPr(f[6]) : NULL; out.I0 = mxGetPr(f[7]);
    out.ip_filled = has_ip ? mxGetPr(f[8]) : NULL;
    char err[256] = {0};
    const int rc = epi_preprocess_host(&d, mxGetPr(prhs[1]), opt(prhs[2]), mxGetPr(prhs[3]), opt(prhs[4]), &out, /*device=*/0, err);
    if (rc != EPI_OK) { for (mxArray *a : f) mxDestroyArray(a); fail_if(rc, err); }
    plhs[0] = mxCreateStructMatrix(1, 1, 9, names);
    for (int k = 0; k < 9; k++) mxSetFieldByNumber(plhs[0], 0, k, f[k]);
}

static void nnls(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs != 4) mexErrMsgTxt("epiekf_pipeline_mex('nnls', X, y, max_iters): 4 inputs expected");
    if (mxGetNumberOfDimensions(prhs[1]) != 3) mexErrMsgTxt("X must be S x n x D");
    const mwSize *dx = mxGetDimensions(prhs[1]);
    const mwSize S = dx[0], n = dx[1], D = dx[2];
    want(prhs[2], S, D, "y");
    epi_nnls_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION; d.S = (int32_t)S; d.D = (int32_t)D; d.n = (int32_t)n; d.max_iters = (int32_t)mxGetScalar(prhs[3]);
    mxArray *a = mxCreateDoubleMatrix(S, n, mxREAL), *b = mxCreateDoubleMatrix(S, 1, mxREAL), *me = mxCreateDoubleMatrix(S, 1, mxREAL);
    mxArray *it = mxCreateDoubleMatrix(S, 1, mxREAL);
    std::vector<int32_t> iters((size_t)S);
    char err[256] = {0};
    const int rc = epi_nnls_affine_fit_host(&d, mxGetPr(prhs[1]), mxGetPr(prhs[2]), mxGetPr(a), mxGetPr(b), mxGetPr(me), iters.data(), NULL, /*device=*/0, err);
    if (rc != EPI_OK) { mxDestroyArray(a); mxDestroyArray(b); mxDestroyArray(me); mxDestroyArray(it); fail_if(rc, err); }
    for (size_t k = 0; k < iters.size(); k++) mxGetPr(it)[k] = (double)iters[k];
    mxArray *o[4] = {a, b, me, it};
    for (int k = 0; k < 4; k++)
        if (k < nlhs || k == 0) plhs[k] = o[k]; else mxDestroyArray(o[k]);
}

static void lasso(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs != 5) mexErrMsgTxt("epiekf_pipeline_mex('lasso', X, y, K, fold): 5 inputs expected");
    if (mxGetNumberOfDimensions(prhs[1]) != 3) mexErrMsgTxt("X must be R x n x D");
    const mwSize *dx = mxGetDimensions(prhs[1]);
    const mwSize R = dx[0], n = dx[1], D = dx[2];
    want(prhs[2], R, D, "y");
    const int K = (int)mxGetScalar(prhs[3]);
    std::vector<int32_t> fold;
    if (K >= 2) {
        want(prhs[4], R, D, "fold");
        const double *f = mxGetPr(prhs[4]);
        fold.resize((size_t)(R * D));
        for (size_t k = 0; k < fold.size(); k++) fold[k] = (int32_t)f[k] - 1;       // MATLAB's 1 .. K -> 0 .. K-1
    }
    epi_lasso_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION; d.R = (int32_t)R; d.D = (int32_t)D; d.n = (int32_t)n; d.K = K;
    d.num_lambda = 100; d.lambda_ratio = 1e-4; d.rel_tol = 1e-4; d.max_iter = 100000;        // lasso's defaults
    const mwSize NL = (mwSize)d.num_lambda;
    const bool cv = K >= 2;
    mxArray *a = mxCreateDoubleMatrix(R, n, mxREAL), *b = mxCreateDoubleMatrix(R, 1, mxREAL);
    mxArray *lam = mxCreateDoubleMatrix(R, NL, mxREAL), *mse = mxCreateDoubleMatrix(R, NL, mxREAL), *se = mxCreateDoubleMatrix(R, NL, mxREAL);
    mxArray *idx = mxCreateDoubleMatrix(R, 1, mxREAL), *idx1 = mxCreateDoubleMatrix(R, 1, mxREAL);
    mxArray *B = dbl3(R, n, NL), *icpt = mxCreateDoubleMatrix(R, NL, mxREAL), *df = mxCreateDoubleMatrix(R, NL, mxREAL);
    mxArray *o[10] = {a, b, lam, mse, se, idx, idx1, B, icpt, df};
    std::vector<int32_t> dfv((size_t)(NL * R)), im((size_t)R), i1((size_t)R), st((size_t)R);
    epi_lasso_outputs out;
    memset(&out, 0, sizeof out);
    out.lambda = mxGetPr(lam); out.B = mxGetPr(B); out.intercept = mxGetPr(icpt); out.df = dfv.data(); out.status = st.data();
    if (cv) {
        out.a = mxGetPr(a); out.b = mxGetPr(b); out.mse = mxGetPr(mse); out.se = mxGetPr(se);
        out.idx_min_mse = im.data(); out.idx_1se = i1.data();
    }
    // the ABI's [NL][R] and [NL][n][R] are MATLAB's R x NL and R x n x NL: no transposition
    char err[256] = {0};
    const int rc = epi_lasso_run_host(&d, mxGetPr(prhs[1]), mxGetPr(prhs[2]), cv ? fold.data() : NULL, &out, /*device=*/0, err);
    if (rc != EPI_OK) { for (mxArray *m : o) mxDestroyArray(m); fail_if(rc, err); }
    for (size_t k = 0; k < dfv.size(); k++) mxGetPr(df)[k] = (double)dfv[k];
    if (!cv)                                                                        // no cross-validation: a, b, mse, se are NaN
        for (mxArray *m : {a, b, mse, se})
            for (size_t k = 0; k < mxGetNumberOfElements(m); k++) mxGetPr(m)[k] = std::numeric_limits<double>::quiet_NaN();
    for (mwSize r = 0; r < R; r++) {
        mxGetPr(idx)[r] = cv ? (double)(im[r] + 1) : 0.0;
        mxGetPr(idx1)[r] = cv ? (double)(i1[r] + 1) : 0.0;
    }
    for (int k = 0; k < 10; k++)
        if (k < nlhs || k == 0) plhs[k] = o[k]; else mxDestroyArray(o[k]);
}

static void robustfit(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs != 7) mexErrMsgTxt("epiekf_pipeline_mex('robustfit', X, y, robust, lower, upper, max_iter): 7 inputs expected");
    if (mxGetNumberOfDimensions(prhs[1]) != 3) mexErrMsgTxt("X must be R x n x D");
    const mwSize *dx = mxGetDimensions(prhs[1]);
    const mwSize R = dx[0], n = dx[1], D = dx[2];
    want(prhs[2], R, D, "y");
    epi_robfit_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION; d.R = (int32_t)R; d.D = (int32_t)D; d.n = (int32_t)n;
    d.robust = (int32_t)mxGetScalar(prhs[3]); d.lower_a = mxGetScalar(prhs[4]); d.upper_a = mxGetScalar(prhs[5]);
    d.max_iter = (int32_t)mxGetScalar(prhs[6]);
    const bool want_w = nlhs >= 7;
    mxArray *a = mxCreateDoubleMatrix(R, n, mxREAL), *b = mxCreateDoubleMatrix(R, 1, mxREAL), *bi = mxCreateDoubleMatrix(R, n, mxREAL);
    mxArray *sg = mxCreateDoubleMatrix(R, n, mxREAL), *it = mxCreateDoubleMatrix(R, n, mxREAL), *st = mxCreateDoubleMatrix(R, n, mxREAL);
    mxArray *w = want_w ? dbl3(R, n, D) : mxCreateDoubleMatrix(0, 0, mxREAL);
    mxArray *o[7] = {a, b, bi, sg, it, st, w};
    std::vector<int32_t> itv((size_t)(R * n)), stv((size_t)(R * n));
    epi_robfit_outputs out;
    memset(&out, 0, sizeof out);
    out.a = mxGetPr(a); out.b = mxGetPr(b); out.b_item = mxGetPr(bi); out.sigma = mxGetPr(sg); out.iters = itv.data(); out.status = stv.data();
    if (want_w) out.weights = mxGetPr(w);
    // the ABI's [n][R] and [D][n][R] are MATLAB's R x n and R x n x D: no transposition
    char err[256] = {0};
    const int rc = epi_robfit_run_host(&d, mxGetPr(prhs[1]), mxGetPr(prhs[2]), &out, /*device=*/0, err);
    if (rc != EPI_OK) { for (mxArray *m : o) mxDestroyArray(m); fail_if(rc, err); }
    for (size_t k = 0; k < itv.size(); k++) { mxGetPr(it)[k] = (double)itv[k]; mxGetPr(st)[k] = (double)stv[k]; }
    for (int k = 0; k < 7; k++)
        if (k < nlhs || k == 0) plhs[k] = o[k]; else mxDestroyArray(o[k]);
}

static void ratemap(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs != 12)
        mexErrMsgTxt("epiekf_pipeline_mex('ratemap', ip, y, new_smoothed, extra, lambda_in, n_train, lags, ridge, lambda_threshold, "
                     "reduction_effect, effect_lag): 12 inputs expected");
    const mwSize nd = mxGetNumberOfDimensions(prhs[1]);
    const mwSize *dx = mxGetDimensions(prhs[1]);
    if (nd > 3 || mxIsEmpty(prhs[1])) mexErrMsgTxt("ip must be R x n x T");
    const mwSize R = dx[0], n = dx[1], T = nd == 3 ? dx[2] : 1;
    const bool fit = mxIsEmpty(prhs[5]), have_y = !mxIsEmpty(prhs[2]);
    if (have_y) want(prhs[2], R, T, "y");
    want(prhs[3], R, T, "new_smoothed");
    const mwSize K = mxGetNumberOfElements(prhs[6]), NL = mxGetNumberOfElements(prhs[7]);
    if (K < 1) mexErrMsgTxt("n_train must hold at least one train end");
    if (NL > 3) mexErrMsgTxt("lags holds at most 3 lags");
    mwSize E = 0;
    if (!mxIsEmpty(prhs[4])) {
        const mwSize ne = mxGetNumberOfDimensions(prhs[4]);
        const mwSize *de = mxGetDimensions(prhs[4]);
        if (ne > 3 || de[0] != R || (ne == 3 ? de[2] : 1) != T) mexErrMsgTxt("extra must be R x E x T");
        E = de[1];
    }
    if (!fit) {
        const mwSize nl = mxGetNumberOfDimensions(prhs[5]);
        const mwSize *dl = mxGetDimensions(prhs[5]);
        if (nl > 3 || dl[0] != R || dl[1] != T || (nl == 3 ? dl[2] : 1) != K) mexErrMsgTxt("lambda_in must be R x T x K");
    }
    epi_ratemap_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION; d.T = (int32_t)T; d.n = (int32_t)n; d.R = (int32_t)R; d.E = (int32_t)E; d.K = (int32_t)K;
    d.n_lags = (int32_t)NL; d.fit = fit ? 1 : 0;
    for (mwSize l = 0; l < NL; l++) d.lags[l] = (int32_t)mxGetPr(prhs[7])[l];
    d.ridge = mxGetScalar(prhs[8]); d.lambda_threshold = mxGetScalar(prhs[9]); d.reduction_effect = mxGetScalar(prhs[10]);
    d.effect_lag = (int32_t)mxGetScalar(prhs[11]);
    std::vector<int32_t> nt((size_t)K), stv((size_t)(R * K));
    for (mwSize k = 0; k < K; k++) nt[k] = (int32_t)mxGetPr(prhs[6])[k];
    const mwSize F = n * (1 + NL) + E;
    mxArray *lh = dbl3(R, T, K), *es = dbl3(R, T, K), *mp = fit ? dbl3(R, F, K) : mxCreateDoubleMatrix(0, 0, mxREAL);
    mxArray *st = mxCreateDoubleMatrix(R, K, mxREAL), *xm = mxCreateDoubleMatrix(R, F, mxREAL);
    mxArray *yf = have_y ? mxCreateDoubleMatrix(R, T, mxREAL) : mxCreateDoubleMatrix(0, 0, mxREAL), *tr = mxCreateDoubleMatrix(R, T, mxREAL);
    mxArray *o[7] = {lh, es, mp, st, xm, yf, tr};
    epi_ratemap_inputs in;
    memset(&in, 0, sizeof in);
    in.ip = mxGetPr(prhs[1]); in.y = opt(prhs[2]); in.new_smoothed = mxGetPr(prhs[3]); in.extra = opt(prhs[4]); in.lambda_in = opt(prhs[5]);
    in.n_train = nt.data();
    epi_ratemap_outputs out;
    memset(&out, 0, sizeof out);
    out.lambda_hat = mxGetPr(lh); out.new_cases_est = mxGetPr(es); out.status = stv.data();
    if (fit) out.map = mxGetPr(mp);
    if (nlhs >= 5) out.x_mx = mxGetPr(xm);
    if (nlhs >= 6 && have_y) out.y_filled = mxGetPr(yf);
    if (nlhs >= 7) out.tracker = mxGetPr(tr);
    // the ABI's [K][T][R], [K][F][R], [F][R] and [T][R] are MATLAB's R x T x K, R x F x K, R x F and R x T: no transposition
    char err[256] = {0};
    const int rc = epi_ratemap_run_host(&d, &in, &out, /*device=*/0, err);
    if (rc != EPI_OK) { for (mxArray *m : o) mxDestroyArray(m); fail_if(rc, err); }
    for (size_t k = 0; k < stv.size(); k++) mxGetPr(st)[k] = (double)stv[k];
    for (int k = 0; k < 7; k++)
        if (k < nlhs || k == 0) plhs[k] = o[k]; else mxDestroyArray(o[k]);
}

static void mldivide(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs != 5) mexErrMsgTxt("epiekf_pipeline_mex('mldivide', X, y, n_rows, tol_scale): 5 inputs expected");
    const mwSize nd = mxGetNumberOfDimensions(prhs[1]);
    const mwSize *dx = mxGetDimensions(prhs[1]);
    if (nd > 3 || mxIsEmpty(prhs[1])) mexErrMsgTxt("X must be R x F x D");
    const mwSize R = dx[0], F = dx[1], D = nd == 3 ? dx[2] : 1;
    want(prhs[2], R, D, "y");
    const mwSize K = mxIsEmpty(prhs[3]) ? 1 : mxGetNumberOfElements(prhs[3]);
    epi_mldiv_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION; d.D = (int32_t)D; d.F = (int32_t)F; d.R = (int32_t)R; d.K = (int32_t)K;
    d.tol_scale = mxIsEmpty(prhs[4]) ? 1.0 : mxGetScalar(prhs[4]);
    std::vector<int32_t> nr((size_t)K, (int32_t)D), rkv((size_t)(R * K)), stv((size_t)(R * K)), pmv((size_t)(R * F * K));
    if (!mxIsEmpty(prhs[3]))
        for (mwSize k = 0; k < K; k++) nr[k] = (int32_t)mxGetPr(prhs[3])[k];
    mxArray *m = dbl3(R, F, K), *rk = mxCreateDoubleMatrix(R, K, mxREAL), *pm = dbl3(R, F, K), *rd = dbl3(R, F, K);
    mxArray *rs = mxCreateDoubleMatrix(R, K, mxREAL), *fi = dbl3(R, D, K), *st = mxCreateDoubleMatrix(R, K, mxREAL);
    mxArray *o[7] = {m, rk, pm, rd, rs, fi, st};
    epi_mldiv_inputs in;
    memset(&in, 0, sizeof in);
    in.X = mxGetPr(prhs[1]); in.y = mxGetPr(prhs[2]); in.n_rows = nr.data();
    epi_mldiv_outputs out;
    memset(&out, 0, sizeof out);
    out.m = mxGetPr(m);
    if (nlhs >= 2) out.rank = rkv.data();
    if (nlhs >= 3) out.perm = pmv.data();
    if (nlhs >= 4) out.rdiag = mxGetPr(rd);
    if (nlhs >= 5) out.resid = mxGetPr(rs);
    if (nlhs >= 6) out.fitted = mxGetPr(fi);
    if (nlhs >= 7) out.status = stv.data();
    // the ABI's [K][F][R], [K][D][R] and [K][R] are MATLAB's R x F x K, R x D x K and R x K: no transposition
    char err[256] = {0};
    const int rc = epi_mldiv_run_host(&d, &in, &out, /*device=*/0, err);
    if (rc != EPI_OK) { for (mxArray *a : o) mxDestroyArray(a); fail_if(rc, err); }
    for (size_t k = 0; k < stv.size(); k++) { mxGetPr(rk)[k] = (double)rkv[k]; mxGetPr(st)[k] = (double)stv[k]; }
    for (size_t k = 0; k < pmv.size(); k++) mxGetPr(pm)[k] = (double)pmv[k] + 1.0;       // MATLAB's column numbers
    for (int k = 0; k < 7; k++)
        if (k < nlhs || k == 0) plhs[k] = o[k]; else mxDestroyArray(o[k]);
}

static void svr(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs != 10) mexErrMsgTxt("epiekf_pipeline_mex('svr', X, y, n_rows, kernel, box, epsilon, kernel_scale, tol, max_iter): 10 inputs expected");
    const mwSize nd = mxGetNumberOfDimensions(prhs[1]);
    const mwSize *dx = mxGetDimensions(prhs[1]);
    if (nd > 3 || mxIsEmpty(prhs[1])) mexErrMsgTxt("X must be R x F x D");
    const mwSize R = dx[0], F = dx[1], D = nd == 3 ? dx[2] : 1;
    want(prhs[2], R, D, "y");
    const mwSize K = mxIsEmpty(prhs[3]) ? 1 : mxGetNumberOfElements(prhs[3]);
    epi_svr_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION; d.D = (int32_t)D; d.F = (int32_t)F; d.R = (int32_t)R; d.K = (int32_t)K;
    d.kernel = mxIsEmpty(prhs[4]) ? EPI_SVR_LINEAR : (int32_t)mxGetScalar(prhs[4]);
    d.tol = mxIsEmpty(prhs[8]) ? 1e-3 : mxGetScalar(prhs[8]);
    d.max_iter = mxIsEmpty(prhs[9]) ? 100000 : (int32_t)mxGetScalar(prhs[9]);
    std::vector<double> reg[3];
    static const char *const names[3] = {"box", "epsilon", "kernel_scale"};
    for (int q = 0; q < 3; q++) {                                       // a scalar is broadcast over the regions
        const mxArray *a = prhs[5 + q];
        const mwSize ne = mxGetNumberOfElements(a);
        if (ne != 1 && ne != R) {
            char msg[64];
            snprintf(msg, sizeof msg, "%s must be a scalar or R values", names[q]);
            mexErrMsgTxt(msg);
        }
        reg[q].resize((size_t)R);
        for (mwSize r = 0; r < R; r++) reg[q][r] = mxGetPr(a)[ne == 1 ? 0 : r];
    }
    const bool lin = d.kernel == EPI_SVR_LINEAR;
    std::vector<int32_t> nr((size_t)K, (int32_t)D), niv((size_t)(R * K)), nsv((size_t)(R * K)), stv((size_t)(R * K));
    if (!mxIsEmpty(prhs[3]))
        for (mwSize k = 0; k < K; k++) nr[k] = (int32_t)mxGetPr(prhs[3])[k];
    mxArray *be = dbl3(R, D, K), *bi = mxCreateDoubleMatrix(R, K, mxREAL), *w = lin ? dbl3(R, F, K) : mxCreateDoubleMatrix(0, 0, mxREAL);
    mxArray *fi = dbl3(R, D, K), *ni = mxCreateDoubleMatrix(R, K, mxREAL), *gp = mxCreateDoubleMatrix(R, K, mxREAL);
    mxArray *ns = mxCreateDoubleMatrix(R, K, mxREAL), *st = mxCreateDoubleMatrix(R, K, mxREAL);
    mxArray *o[8] = {be, bi, w, fi, ni, gp, ns, st};
    epi_svr_inputs in;
    memset(&in, 0, sizeof in);
    in.X = mxGetPr(prhs[1]); in.y = mxGetPr(prhs[2]); in.n_rows = nr.data();
    in.box = reg[0].data(); in.epsilon = reg[1].data(); in.kernel_scale = reg[2].data();
    epi_svr_outputs out;
    memset(&out, 0, sizeof out);
    out.beta = mxGetPr(be);
    if (nlhs >= 2) out.bias = mxGetPr(bi);
    if (nlhs >= 3 && lin) out.w = mxGetPr(w);
    if (nlhs >= 4) out.fitted = mxGetPr(fi);
    if (nlhs >= 5) out.n_iter = niv.data();
    if (nlhs >= 6) out.gap = mxGetPr(gp);
    if (nlhs >= 7) out.n_sv = nsv.data();
    if (nlhs >= 8) out.status = stv.data();
    // the ABI's [K][D][R], [K][F][R] and [K][R] are MATLAB's R x D x K, R x F x K and R x K: no transposition
    char err[256] = {0};
    const int rc = epi_svr_run_host(&d, &in, &out, /*device=*/0, err);
    if (rc != EPI_OK) { for (mxArray *a : o) mxDestroyArray(a); fail_if(rc, err); }
    for (size_t k = 0; k < stv.size(); k++) { mxGetPr(ni)[k] = (double)niv[k]; mxGetPr(ns)[k] = (double)nsv[k]; mxGetPr(st)[k] = (double)stv[k]; }
    for (int k = 0; k < 8; k++)
        if (k < nlhs || k == 0) plhs[k] = o[k]; else mxDestroyArray(o[k]);
}

static void ens_summary(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs != 5) mexErrMsgTxt("epiekf_pipeline_mex('ens_summary', src, D, q, population): 5 inputs expected");
    const mwSize nd = mxGetNumberOfDimensions(prhs[1]);
    if (nd > 3 || mxIsEmpty(prhs[1]) || !mxGetPr(prhs[1])) mexErrMsgTxt("src must be a double array B x rows x T (or B x T)");
    const mwSize *ds = mxGetDimensions(prhs[1]);
    const mwSize B = ds[0], rows = nd == 3 ? ds[1] : 1, T = nd == 3 ? ds[2] : ds[1];
    const double Dd = mxGetScalar(prhs[2]);
    if (!(Dd >= 1.0 && Dd <= 4096.0) || (double)(mwSize)Dd != Dd || B % (mwSize)Dd != 0) mexErrMsgTxt("D must be an integer in 1 .. 4096 that divides the number of chains");
    const mwSize D = (mwSize)Dd, R = B / D, nq = mxGetNumberOfElements(prhs[3]);
    if (nq < 1 || nq > 16) mexErrMsgTxt("q must hold 1 .. 16 probabilities");
    const bool derive = !mxIsEmpty(prhs[4]);
    if (derive && mxGetNumberOfElements(prhs[4]) != R) mexErrMsgTxt("population must have one entry per region");
    epi_ens_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION; d.T = (int32_t)T; d.rows = (int32_t)rows; d.R = (int32_t)R; d.D = (int32_t)D;
    d.n_q = (int32_t)nq; d.storage = 0; d.derive_newcases = derive ? 1 : 0;
    for (mwSize k = 0; k < nq; k++) d.q[k] = mxGetPr(prhs[3])[k];
    const mwSize ro = rows + (derive ? 1 : 0);
    const mwSize d4[4] = {R, ro, nq, T};
    mxArray *o[6] = {dbl3(R, ro, T), dbl3(R, ro, T), dbl3(R, ro, T), dbl3(R, ro, T), mxCreateNumericArray(4, d4, mxDOUBLE_CLASS, mxREAL),
                     dbl3(R, ro, T)};
    std::vector<int32_t> cnt((size_t)(R * ro * T));
    epi_ens_outputs out;
    memset(&out, 0, sizeof out);
    out.mean = mxGetPr(o[0]); out.std = mxGetPr(o[1]); out.min = mxGetPr(o[2]); out.max = mxGetPr(o[3]); out.quantiles = mxGetPr(o[4]);
    out.count = cnt.data();
    // the ABI's [T][rows'][R] and [T][n_q][rows'][R] are MATLAB's R x rows' x T and R x rows' x n_q x T: no transposition
    char err[256] = {0};
    const int rc = epi_ens_run_host(&d, mxGetPr(prhs[1]), derive ? mxGetPr(prhs[4]) : NULL, &out, /*device=*/0, err);
    if (rc != EPI_OK) { for (mxArray *m : o) mxDestroyArray(m); fail_if(rc, err); }
    for (size_t k = 0; k < cnt.size(); k++) mxGetPr(o[5])[k] = (double)cnt[k];
    for (int k = 0; k < 6; k++)
        if (k < nlhs || k == 0) plhs[k] = o[k]; else mxDestroyArray(o[k]);
}

static void escore(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs != 11) mexErrMsgTxt("epiekf_pipeline_mex('escore', src, truth, D, alpha, n_bins, population, truth_series, first_day, k_first, k_last): 11 inputs expected");
    const mwSize nd = mxGetNumberOfDimensions(prhs[1]);
    if (nd > 3 || mxIsEmpty(prhs[1]) || !mxGetPr(prhs[1])) mexErrMsgTxt("src must be a double array B x rows x T (or B x T)");
    const mwSize *ds = mxGetDimensions(prhs[1]);
    const mwSize B = ds[0], rows = nd == 3 ? ds[1] : 1, T = nd == 3 ? ds[2] : ds[1];
    const double Dd = mxGetScalar(prhs[3]);
    if (!(Dd >= 1.0 && Dd <= 4096.0) || (double)(mwSize)Dd != Dd || B % (mwSize)Dd != 0) mexErrMsgTxt("D must be an integer in 1 .. 4096 that divides the number of chains");
    const mwSize D = (mwSize)Dd, R = B / D, na = mxGetNumberOfElements(prhs[4]);
    if (na > 8) mexErrMsgTxt("alpha must hold at most 8 levels");
    if (mxIsEmpty(prhs[5]) || !mxGetPr(prhs[5]) || mxGetNumberOfElements(prhs[5]) != 1) mexErrMsgTxt("n_bins must be a double scalar");
    const double nbd = mxGetScalar(prhs[5]);
    if (!(nbd >= 0.0 && nbd <= 32.0) || (double)(mwSize)nbd != nbd) mexErrMsgTxt("n_bins must be an integer in 0 .. 32");
    const mwSize nb = (mwSize)nbd;
    const bool derive = !mxIsEmpty(prhs[6]);
    if (derive && mxGetNumberOfElements(prhs[6]) != R) mexErrMsgTxt("population must have one entry per region");
    const mwSize ro = rows + (derive ? 1 : 0);
    const mwSize ndt = mxGetNumberOfDimensions(prhs[2]);
    if (ndt > 3 || mxIsEmpty(prhs[2]) || !mxGetPr(prhs[2])) mexErrMsgTxt("truth must be a double array Rt x rows' x T (or Rt x T)");
    const mwSize *dt = mxGetDimensions(prhs[2]);
    const mwSize Rt = dt[0];
    if (nd == 3 ? !((ndt == 3 && dt[1] == ro && dt[2] == T) || (ndt == 2 && T == 1 && dt[1] == ro)) : !(ndt == 2 && dt[1] == T && ro == 1))
        mexErrMsgTxt("truth must be Rt x rows' x T (Rt x T for a B x T src), rows' = rows + 1 with a population");
    std::vector<int32_t> ser, fd;
    if (!mxIsEmpty(prhs[7])) {
        if (mxGetNumberOfElements(prhs[7]) != R) mexErrMsgTxt("truth_series must have one entry per region");
        ser.resize((size_t)R);
        for (mwSize r = 0; r < R; r++) {
            const double v = mxGetPr(prhs[7])[r];
            if (!(v >= 1.0 && v <= (double)Rt) || (double)(mwSize)v != v) mexErrMsgTxt("truth_series must hold ONE-based columns of truth");
            ser[(size_t)r] = (int32_t)v - 1;
        }
    } else if (Rt != R) {
        mexErrMsgTxt("truth must hold one column per region (or pass truth_series)");
    }
    if (!mxIsEmpty(prhs[8])) {
        if (mxGetNumberOfElements(prhs[8]) != R) mexErrMsgTxt("first_day must have one entry per region");
        fd.resize((size_t)R);
        for (mwSize r = 0; r < R; r++) {
            const double v = mxGetPr(prhs[8])[r];
            if (!(v >= 1.0 && v <= 2147483647.0) || (double)(mwSize)v != v) mexErrMsgTxt("first_day must hold ONE-based days");
            fd[(size_t)r] = (int32_t)v - 1;
        }
    }
    double kf = 1.0, kl = (double)T;
    if (!mxIsEmpty(prhs[9])) kf = mxGetScalar(prhs[9]);
    if (!mxIsEmpty(prhs[10])) kl = mxGetScalar(prhs[10]);
    if (!(kf >= 1.0 && kf <= (double)T && kl >= kf - 1.0 && kl <= (double)T) || (double)(mwSize)kf != kf || (double)(mwSize)kl != kl)
        mexErrMsgTxt("k_first, k_last must be integers with 1 <= k_first <= T and k_first - 1 <= k_last <= T");
    epi_escore_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION; d.T = (int32_t)T; d.rows = (int32_t)rows; d.R = (int32_t)R; d.D = (int32_t)D; d.Rt = (int32_t)Rt;
    d.n_a = (int32_t)na; d.n_bins = (int32_t)nb; d.storage = 0; d.derive_newcases = derive ? 1 : 0;
    d.k0 = (int32_t)kf - 1; d.k1 = (int32_t)kl;
    for (mwSize k = 0; k < na; k++) d.alpha[k] = mxGetPr(prhs[4])[k];
    epi_escore_inputs in;
    memset(&in, 0, sizeof in);
    in.src = mxGetPr(prhs[1]); in.population = derive ? mxGetPr(prhs[6]) : NULL; in.truth = mxGetPr(prhs[2]);
    in.truth_series = ser.empty() ? NULL : ser.data(); in.first_day = fd.empty() ? NULL : fd.data();
    // the ABI's [T][rows'][R], [T][n_a][rows'][R], [rows'][R], [n][rows'][R] are MATLAB's R x rows' x T, R x rows' x n_a x T,
    // R x rows', R x rows' x n: no transposition
    const mwSize d4[4] = {R, ro, na, T};
    mxArray *o[14] = {dbl3(R, ro, T), dbl3(R, ro, T), dbl3(R, ro, T), mxCreateNumericArray(4, d4, mxDOUBLE_CLASS, mxREAL),
                      dbl3(R, ro, T), dbl3(R, ro, T), dbl3(R, ro, T), dbl3(R, ro, T),
                      mxCreateDoubleMatrix(R, ro, mxREAL), mxCreateDoubleMatrix(R, ro, mxREAL), mxCreateDoubleMatrix(R, ro, mxREAL),
                      mxCreateDoubleMatrix(R, ro, mxREAL), dbl3(R, ro, na), dbl3(R, ro, nb)};
    const size_t items = (size_t)(R * ro * T), cols = (size_t)(R * ro);
    std::vector<int32_t> ibuf(4 * items + cols + cols * (size_t)nb + 1);
    int32_t *irank = ibuf.data(), *ities = irank + items, *icover = ities + items, *icount = icover + items, *ins = icount + items,
            *ipit = ins + cols;
    epi_escore_outputs out;
    memset(&out, 0, sizeof out);
    out.crps = mxGetPr(o[0]); out.wis = mxGetPr(o[1]); out.ae = mxGetPr(o[2]); out.width = na ? mxGetPr(o[3]) : NULL;
    out.rank = irank; out.ties = ities; out.cover = icover; out.count = icount;
    out.crps_mean = mxGetPr(o[8]); out.wis_mean = mxGetPr(o[9]); out.ae_mean = mxGetPr(o[10]); out.n_scored = ins;
    out.cover_frac = na ? mxGetPr(o[12]) : NULL; out.pit_hist = nb ? ipit : NULL;
    char err[256] = {0};
    const int rc = epi_escore_run_host(&d, &in, &out, /*device=*/0, err);
    if (rc != EPI_OK) { for (mxArray *m : o) mxDestroyArray(m); fail_if(rc, err); }
    const int32_t *isrc[4] = {irank, ities, icover, icount};
    for (int j = 0; j < 4; j++)
        for (size_t k = 0; k < items; k++) mxGetPr(o[4 + j])[k] = (double)isrc[j][k];
    for (size_t k = 0; k < cols; k++) mxGetPr(o[11])[k] = (double)ins[k];
    for (size_t k = 0; k < cols * (size_t)nb; k++) mxGetPr(o[13])[k] = (double)ipit[k];
    for (int k = 0; k < 14; k++)
        if (k < nlhs || k == 0) plhs[k] = o[k]; else mxDestroyArray(o[k]);
}

static void jscore(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs != 11) mexErrMsgTxt("epiekf_pipeline_mex('jscore', src, truth, D, vs_p, max_lag, population, truth_series, first_day, k_first, k_last): 11 inputs expected");
    const mwSize nd = mxGetNumberOfDimensions(prhs[1]);
    if (nd > 3 || mxIsEmpty(prhs[1]) || !mxGetPr(prhs[1])) mexErrMsgTxt("src must be a double array B x rows x T (or B x T)");
    const mwSize *ds = mxGetDimensions(prhs[1]);
    const mwSize B = ds[0], rows = nd == 3 ? ds[1] : 1, T = nd == 3 ? ds[2] : ds[1];
    const double Dd = mxGetScalar(prhs[3]);
    if (!(Dd >= 1.0 && Dd <= 4096.0) || (double)(mwSize)Dd != Dd || B % (mwSize)Dd != 0) mexErrMsgTxt("D must be an integer in 1 .. 4096 that divides the number of chains");
    const mwSize D = (mwSize)Dd, R = B / D;
    const double p = mxIsEmpty(prhs[4]) ? 0.0 : mxGetScalar(prhs[4]);
    if (p != 0.0 && p != 0.5 && p != 1.0) mexErrMsgTxt("vs_p must be [] or 0 (no variogram score), 0.5 or 1");
    const double lag = mxIsEmpty(prhs[5]) ? 0.0 : mxGetScalar(prhs[5]);
    if (!(lag >= 0.0 && lag <= 2147483647.0) || (double)(mwSize)lag != lag) mexErrMsgTxt("max_lag must be an integer >= 0");
    const bool derive = !mxIsEmpty(prhs[6]);
    if (derive && mxGetNumberOfElements(prhs[6]) != R) mexErrMsgTxt("population must have one entry per region");
    const mwSize ro = rows + (derive ? 1 : 0);
    const mwSize ndt = mxGetNumberOfDimensions(prhs[2]);
    if (ndt > 3 || mxIsEmpty(prhs[2]) || !mxGetPr(prhs[2])) mexErrMsgTxt("truth must be a double array Rt x rows' x T (or Rt x T)");
    const mwSize *dt = mxGetDimensions(prhs[2]);
    const mwSize Rt = dt[0];
    if (nd == 3 ? !((ndt == 3 && dt[1] == ro && dt[2] == T) || (ndt == 2 && T == 1 && dt[1] == ro)) : !(ndt == 2 && dt[1] == T && ro == 1))
        mexErrMsgTxt("truth must be Rt x rows' x T (Rt x T for a B x T src), rows' = rows + 1 with a population");
    std::vector<int32_t> ser, fd;
    if (!mxIsEmpty(prhs[7])) {
        if (mxGetNumberOfElements(prhs[7]) != R) mexErrMsgTxt("truth_series must have one entry per region");
        ser.resize((size_t)R);
        for (mwSize r = 0; r < R; r++) {
            const double v = mxGetPr(prhs[7])[r];
            if (!(v >= 1.0 && v <= (double)Rt) || (double)(mwSize)v != v) mexErrMsgTxt("truth_series must hold ONE-based columns of truth");
            ser[(size_t)r] = (int32_t)v - 1;
        }
    } else if (Rt != R) {
        mexErrMsgTxt("truth must hold one column per region (or pass truth_series)");
    }
    if (!mxIsEmpty(prhs[8])) {
        if (mxGetNumberOfElements(prhs[8]) != R) mexErrMsgTxt("first_day must have one entry per region");
        fd.resize((size_t)R);
        for (mwSize r = 0; r < R; r++) {
            const double v = mxGetPr(prhs[8])[r];
            if (!(v >= 1.0 && v <= 2147483647.0) || (double)(mwSize)v != v) mexErrMsgTxt("first_day must hold ONE-based days");
            fd[(size_t)r] = (int32_t)v - 1;
        }
    }
    double kf = 1.0, kl = (double)T;
    if (!mxIsEmpty(prhs[9])) kf = mxGetScalar(prhs[9]);
    if (!mxIsEmpty(prhs[10])) kl = mxGetScalar(prhs[10]);
    if (!(kf >= 1.0 && kf <= (double)T && kl >= kf - 1.0 && kl <= (double)T) || (double)(mwSize)kf != kf || (double)(mwSize)kl != kl)
        mexErrMsgTxt("k_first, k_last must be integers with 1 <= k_first <= T and k_first - 1 <= k_last <= T");
    epi_ejoint_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION; d.T = (int32_t)T; d.rows = (int32_t)rows; d.R = (int32_t)R; d.D = (int32_t)D; d.Rt = (int32_t)Rt;
    d.storage = 0; d.derive_newcases = derive ? 1 : 0; d.k0 = (int32_t)kf - 1; d.k1 = (int32_t)kl;
    d.vs_order = p == 0.5 ? 1 : (p == 1.0 ? 2 : 0); d.max_lag = (int32_t)lag;
    epi_ejoint_inputs in;
    memset(&in, 0, sizeof in);
    in.src = mxGetPr(prhs[1]); in.population = derive ? mxGetPr(prhs[6]) : NULL; in.truth = mxGetPr(prhs[2]);
    in.truth_series = ser.empty() ? NULL : ser.data(); in.first_day = fd.empty() ? NULL : fd.data();
    // the ABI's [rows'][R] and [rows'][R * D] are MATLAB's R x rows' and B x rows': no transposition
    mxArray *o[7];
    for (int k = 0; k < 6; k++) o[k] = mxCreateDoubleMatrix(R, ro, mxREAL);
    o[6] = mxCreateDoubleMatrix(B, ro, mxREAL);
    const size_t cols = (size_t)(R * ro);
    std::vector<int32_t> ibuf(2 * cols + 1);
    epi_ejoint_outputs out;
    memset(&out, 0, sizeof out);
    out.es = mxGetPr(o[0]); out.vs = d.vs_order ? mxGetPr(o[1]) : NULL; out.truth_term = mxGetPr(o[2]); out.spread_term = mxGetPr(o[3]);
    out.n_members = ibuf.data(); out.n_days = ibuf.data() + cols; out.member_dist = mxGetPr(o[6]);
    char err[256] = {0};
    const int rc = epi_ejoint_run_host(&d, &in, &out, /*device=*/0, err);
    if (rc != EPI_OK) { for (mxArray *m : o) mxDestroyArray(m); fail_if(rc, err); }
    for (size_t k = 0; k < cols; k++) {
        if (!d.vs_order) mxGetPr(o[1])[k] = std::numeric_limits<double>::quiet_NaN();
        mxGetPr(o[4])[k] = (double)ibuf[k];
        mxGetPr(o[5])[k] = (double)ibuf[cols + k];
    }
    for (int k = 0; k < 7; k++)
        if (k < nlhs || k == 0) plhs[k] = o[k]; else mxDestroyArray(o[k]);
}

static void pathfn(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs != 8) mexErrMsgTxt("epiekf_pipeline_mex('pathfn', src, D, thr, population, first_day, k_first, k_last): 8 inputs expected");
    const mwSize nd = mxGetNumberOfDimensions(prhs[1]);
    if (nd > 3 || mxIsEmpty(prhs[1]) || !mxGetPr(prhs[1])) mexErrMsgTxt("src must be a double array B x rows x T (or B x T)");
    const mwSize *ds = mxGetDimensions(prhs[1]);
    const mwSize B = ds[0], rows = nd == 3 ? ds[1] : 1, T = nd == 3 ? ds[2] : ds[1];
    const double Dd = mxGetScalar(prhs[2]);
    if (!(Dd >= 1.0 && Dd <= 2147483647.0) || (double)(mwSize)Dd != Dd || B % (mwSize)Dd != 0) mexErrMsgTxt("D must be a positive integer that divides the number of chains");
    const mwSize D = (mwSize)Dd, R = B / D;
    const bool derive = !mxIsEmpty(prhs[4]);
    if (derive && mxGetNumberOfElements(prhs[4]) != R) mexErrMsgTxt("population must have one entry per region");
    const mwSize ro = rows + (derive ? 1 : 0);
    mwSize nt = 0;
    if (!mxIsEmpty(prhs[3])) {
        if (!mxGetPr(prhs[3])) mexErrMsgTxt("thr must be a double array R x rows' x n_thr (R x n_thr for a B x T src)");
        const mwSize ndt = mxGetNumberOfDimensions(prhs[3]);
        const mwSize *dt = mxGetDimensions(prhs[3]);
        if (ndt > 3 || dt[0] != R || (nd == 3 ? dt[1] != ro : (ndt == 3 || ro != 1)))
            mexErrMsgTxt("thr must be R x rows' x n_thr (R x n_thr for a B x T src), rows' = rows + 1 with a population");
        nt = nd == 3 ? (ndt == 3 ? dt[2] : 1) : dt[1];
        if (nt > 8) mexErrMsgTxt("thr must hold at most 8 thresholds");
    }
    std::vector<int32_t> fd;
    if (!mxIsEmpty(prhs[5])) {
        if (mxGetNumberOfElements(prhs[5]) != R) mexErrMsgTxt("first_day must have one entry per region");
        fd.resize((size_t)R);
        for (mwSize r = 0; r < R; r++) {
            const double v = mxGetPr(prhs[5])[r];
            if (!(v >= 1.0 && v <= 2147483647.0) || (double)(mwSize)v != v) mexErrMsgTxt("first_day must hold ONE-based days");
            fd[(size_t)r] = (int32_t)v - 1;
        }
    }
    double kf = 1.0, kl = (double)T;
    if (!mxIsEmpty(prhs[6])) kf = mxGetScalar(prhs[6]);
    if (!mxIsEmpty(prhs[7])) kl = mxGetScalar(prhs[7]);
    if (!(kf >= 1.0 && kf <= (double)T && kl >= kf && kl <= (double)T) || (double)(mwSize)kf != kf || (double)(mwSize)kl != kl)
        mexErrMsgTxt("k_first, k_last must be integers with 1 <= k_first <= k_last <= T");
    const mwSize W = (mwSize)kl - (mwSize)kf + 1;
    if (W > 4096) mexErrMsgTxt("the window must hold at most 4096 days (the histograms)");
    epi_pathfn_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION; d.T = (int32_t)T; d.rows = (int32_t)rows; d.R = (int32_t)R; d.D = (int32_t)D; d.n_thr = (int32_t)nt;
    d.storage = 0; d.derive_newcases = derive ? 1 : 0; d.k0 = (int32_t)kf - 1; d.k1 = (int32_t)kl;
    epi_pathfn_inputs in;
    memset(&in, 0, sizeof in);
    in.src = mxGetPr(prhs[1]); in.population = derive ? mxGetPr(prhs[4]) : NULL; in.thr = nt ? mxGetPr(prhs[3]) : NULL;
    in.first_day = fd.empty() ? NULL : fd.data();
    // the ABI's [rows'][N], [n_thr][rows'][N], [rows'][R], [W][rows'][R], [W][n_thr][rows'][R] are MATLAB's B x rows', B x rows' x
    // n_thr, R x rows', R x rows' x W, R x rows' x n_thr x W: no transposition
    const mwSize d4[4] = {R, ro, nt, W};
    mxArray *o[13] = {mxCreateDoubleMatrix(B, ro, mxREAL), mxCreateDoubleMatrix(B, ro, mxREAL), mxCreateDoubleMatrix(B, ro, mxREAL),
                      mxCreateDoubleMatrix(B, ro, mxREAL), mxCreateDoubleMatrix(B, ro, mxREAL), dbl3(B, ro, nt), dbl3(B, ro, nt),
                      dbl3(B, ro, nt), mxCreateDoubleMatrix(B, ro, mxREAL), mxCreateDoubleMatrix(R, ro, mxREAL), dbl3(R, ro, W),
                      dbl3(R, ro, nt), mxCreateNumericArray(4, d4, mxDOUBLE_CLASS, mxREAL)};
    const size_t M = (size_t)(B * ro), cols = (size_t)(R * ro);
    const size_t ni[5] = {M, cols, cols * (size_t)W, cols * (size_t)nt, cols * (size_t)nt * (size_t)W};
    std::vector<int32_t> ibuf(ni[0] + ni[1] + ni[2] + ni[3] + ni[4] + 1);
    int32_t *ip[5];
    ip[0] = ibuf.data();
    for (int j = 1; j < 5; j++) ip[j] = ip[j - 1] + ni[j - 1];
    epi_pathfn_outputs out;
    memset(&out, 0, sizeof out);
    out.peak_value = mxGetPr(o[0]); out.peak_day = mxGetPr(o[1]); out.min_value = mxGetPr(o[2]); out.min_day = mxGetPr(o[3]);
    out.total = mxGetPr(o[4]);
    if (nt) { out.first_cross = mxGetPr(o[5]); out.days_above = mxGetPr(o[6]); out.longest_run = mxGetPr(o[7]); out.n_cross = ip[3]; out.cross_day_hist = ip[4]; }
    out.n_valid = ip[0]; out.n_paths = ip[1]; out.peak_day_hist = ip[2];
    char err[256] = {0};
    const int rc = epi_pathfn_run_host(&d, &in, &out, /*device=*/0, err);
    if (rc != EPI_OK) { for (mxArray *m : o) mxDestroyArray(m); fail_if(rc, err); }
    for (size_t k = 0; k < M; k++) { mxGetPr(o[1])[k] += 1.0; mxGetPr(o[3])[k] += 1.0; }      // ONE-based days (NaN stays NaN)
    for (size_t k = 0; k < M * (size_t)nt; k++) mxGetPr(o[5])[k] += 1.0;
    const int oi[5] = {8, 9, 10, 11, 12};
    for (int j = 0; j < 5; j++)
        for (size_t k = 0; k < ni[j]; k++) mxGetPr(o[oi[j]])[k] = (double)ip[j][k];
    for (int k = 0; k < 13; k++)
        if (k < nlhs || k == 0) plhs[k] = o[k]; else mxDestroyArray(o[k]);
}

static void cdepth(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs != 10) mexErrMsgTxt("epiekf_pipeline_mex('cdepth', src, D, alpha, fence_factor, fence_frac, population, first_day, k_first, k_last): 10 inputs expected");
    const mwSize nd = mxGetNumberOfDimensions(prhs[1]);
    if (nd > 3 || mxIsEmpty(prhs[1]) || !mxGetPr(prhs[1])) mexErrMsgTxt("src must be a double array B x rows x T (or B x T)");
    const mwSize *ds = mxGetDimensions(prhs[1]);
    const mwSize B = ds[0], rows = nd == 3 ? ds[1] : 1, T = nd == 3 ? ds[2] : ds[1];
    const double Dd = mxGetScalar(prhs[2]);
    if (!(Dd >= 1.0 && Dd <= 2147483647.0) || (double)(mwSize)Dd != Dd || B % (mwSize)Dd != 0) mexErrMsgTxt("D must be a positive integer that divides the number of chains");
    const mwSize D = (mwSize)Dd, R = B / D;
    const bool derive = !mxIsEmpty(prhs[6]);
    if (derive && mxGetNumberOfElements(prhs[6]) != R) mexErrMsgTxt("population must have one entry per region");
    const mwSize ro = rows + (derive ? 1 : 0);
    epi_cdepth_desc d;
    memset(&d, 0, sizeof d);
    mwSize na = 2;
    d.alpha[0] = 0.5; d.alpha[1] = 0.9;
    if (!mxIsEmpty(prhs[3])) {
        na = mxGetNumberOfElements(prhs[3]);
        if (!mxGetPr(prhs[3]) || na > 8) mexErrMsgTxt("alpha must hold at most 8 fractions");
        for (mwSize k = 0; k < na; k++) d.alpha[k] = mxGetPr(prhs[3])[k];
    }
    d.fence_factor = mxIsEmpty(prhs[4]) ? 1.5 : mxGetScalar(prhs[4]);
    d.fence_frac = mxIsEmpty(prhs[5]) ? 0.5 : mxGetScalar(prhs[5]);
    const bool fence = d.fence_factor > 0.0;
    std::vector<int32_t> fd;
    if (!mxIsEmpty(prhs[7])) {
        if (mxGetNumberOfElements(prhs[7]) != R) mexErrMsgTxt("first_day must have one entry per region");
        fd.resize((size_t)R);
        for (mwSize r = 0; r < R; r++) {
            const double v = mxGetPr(prhs[7])[r];
            if (!(v >= 1.0 && v <= 2147483647.0) || (double)(mwSize)v != v) mexErrMsgTxt("first_day must hold ONE-based days");
            fd[(size_t)r] = (int32_t)v - 1;
        }
    }
    double kf = 1.0, kl = (double)T;
    if (!mxIsEmpty(prhs[8])) kf = mxGetScalar(prhs[8]);
    if (!mxIsEmpty(prhs[9])) kl = mxGetScalar(prhs[9]);
    if (!(kf >= 1.0 && kf <= (double)T && kl >= kf && kl <= (double)T) || (double)(mwSize)kf != kf || (double)(mwSize)kl != kl)
        mexErrMsgTxt("k_first, k_last must be integers with 1 <= k_first <= k_last <= T");
    d.abi_version = EPIEKF_ABI_VERSION; d.T = (int32_t)T; d.rows = (int32_t)rows; d.R = (int32_t)R; d.D = (int32_t)D; d.n_alpha = (int32_t)na;
    d.storage = 0; d.derive_newcases = derive ? 1 : 0; d.k0 = (int32_t)kf - 1; d.k1 = (int32_t)kl;
    epi_cdepth_inputs in;
    memset(&in, 0, sizeof in);
    in.src = mxGetPr(prhs[1]); in.population = derive ? mxGetPr(prhs[6]) : NULL; in.first_day = fd.empty() ? NULL : fd.data();
    // the ABI's [rows'][N], [rows'][R], [T][rows'][R], [T][n_alpha][rows'][R] are MATLAB's B x rows', R x rows', R x rows' x T,
    // R x rows' x n_alpha x T: no transposition
    const mwSize d4[4] = {R, ro, na, T};
    mxArray *o[15] = {mxCreateDoubleMatrix(B, ro, mxREAL), mxCreateDoubleMatrix(B, ro, mxREAL), mxCreateDoubleMatrix(B, ro, mxREAL),
                      mxCreateDoubleMatrix(R, ro, mxREAL), dbl3(R, ro, T), mxCreateNumericArray(4, d4, mxDOUBLE_CLASS, mxREAL),
                      mxCreateNumericArray(4, d4, mxDOUBLE_CLASS, mxREAL), dbl3(R, ro, T), dbl3(R, ro, T), mxCreateDoubleMatrix(B, ro, mxREAL),
                      mxCreateDoubleMatrix(R, ro, mxREAL), mxCreateDoubleMatrix(R, ro, mxREAL), mxCreateDoubleMatrix(B, ro, mxREAL),
                      mxCreateDoubleMatrix(B, ro, mxREAL), mxCreateDoubleMatrix(B, ro, mxREAL)};
    const size_t M = (size_t)(B * ro), cols = (size_t)(R * ro);
    std::vector<int32_t> ibuf(3 * M + 3 * cols + 1, 0);
    int32_t *rank = ibuf.data(), *od = rank + M, *nv = od + M, *mp = nv + M, *no = mp + cols, *nr = no + cols;
    epi_cdepth_outputs out;
    memset(&out, 0, sizeof out);
    out.depth = mxGetPr(o[0]); out.mhi = mxGetPr(o[1]); out.depth_rank = rank; out.median_path = mp; out.median_curve = mxGetPr(o[4]);
    if (na) { out.env_lo = mxGetPr(o[5]); out.env_hi = mxGetPr(o[6]); }
    if (fence) { out.whisk_lo = mxGetPr(o[7]); out.whisk_hi = mxGetPr(o[8]); out.out_days = od; out.n_outliers = no; }
    out.n_ranked = nr; out.band_count = mxGetPr(o[12]); out.pair_total = mxGetPr(o[13]); out.n_valid = nv;
    char err[256] = {0};
    const int rc = epi_cdepth_run_host(&d, &in, &out, /*device=*/0, err);
    if (rc != EPI_OK) { for (mxArray *m : o) mxDestroyArray(m); fail_if(rc, err); }
    for (size_t k = 0; k < M; k++) {
        mxGetPr(o[2])[k] = (double)rank[k] + 1.0;                               // ONE-based, 0 = unranked
        mxGetPr(o[9])[k] = (double)od[k];
        mxGetPr(o[14])[k] = (double)nv[k];
    }
    for (size_t k = 0; k < cols; k++) {
        mxGetPr(o[3])[k] = (double)mp[k] + 1.0;                                 // ONE-based, 0 = none
        mxGetPr(o[10])[k] = (double)no[k];
        mxGetPr(o[11])[k] = (double)nr[k];
    }
    if (!fence)
        for (size_t k = 0; k < cols * (size_t)T; k++) mxGetPr(o[7])[k] = mxGetPr(o[8])[k] = std::numeric_limits<double>::quiet_NaN();
    for (int k = 0; k < 15; k++)
        if (k < nlhs || k == 0) plhs[k] = o[k]; else mxDestroyArray(o[k]);
}

static void ar_forecast(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs != 13 && nrhs != 14) mexErrMsgTxt("epiekf_pipeline_mex('ar_forecast', seg, prm, dt, p, H, D, z, drive, drive_series, A, noise_var, nv_mode): 13 inputs expected (a 14th: seed)");
    epi_noise_desc nd;
    const bool seeded = seed_arg(nrhs, prhs, 13, &nd);
    if (seeded && !mxIsEmpty(prhs[7])) mexErrMsgTxt("seed and z together: the draws have one source");
    if (mxIsEmpty(prhs[1]) || mxGetNumberOfDimensions(prhs[1]) != 2) mexErrMsgTxt("seg must be R x L");
    const mwSize R = mxGetM(prhs[1]), L = mxGetN(prhs[1]);
    want(prhs[2], R, 3, "prm");
    for (int k = 3; k <= 6; k++)
        if (mxIsEmpty(prhs[k]) || !mxGetPr(prhs[k]) || mxGetNumberOfElements(prhs[k]) != 1) mexErrMsgTxt("dt, p, H and D must be double scalars");
    if (mxIsEmpty(prhs[12]) || !mxGetPr(prhs[12]) || mxGetNumberOfElements(prhs[12]) != 1) mexErrMsgTxt("nv_mode must be a double scalar (0 or 1)");
    const double pd = mxGetScalar(prhs[4]), Hd = mxGetScalar(prhs[5]), Dd = mxGetScalar(prhs[6]), nvd = mxGetScalar(prhs[12]);
    if (nvd != 0.0 && nvd != 1.0) mexErrMsgTxt("nv_mode must be 0 or 1");
    if (!(pd >= 0.0 && pd <= 1e6 && Hd >= 0.0 && Hd <= 1e9 && Dd >= 1.0 && Dd <= 2147483647.0) || (double)(mwSize)pd != pd || (double)(mwSize)Hd != Hd || (double)(mwSize)Dd != Dd)
        mexErrMsgTxt("p, H and D must be integers (D >= 1)");
    const mwSize p = (mwSize)pd, H = (mwSize)Hd, D = (mwSize)Dd;
    if ((double)R * (double)D > 2147483647.0) mexErrMsgTxt("R * D is limited to 2^31 - 1");
    const mwSize B = R * D, K = L + H;
    if (!mxIsEmpty(prhs[7])) want(prhs[7], B, H, "z");
    mwSize Sd = 0;
    if (!mxIsEmpty(prhs[8])) {
        if (mxGetN(prhs[8]) != H) mexErrMsgTxt("drive must be Sd x H");
        Sd = mxGetM(prhs[8]);
    }
    std::vector<int32_t> ser;
    if (!mxIsEmpty(prhs[9])) {
        if (!Sd) mexErrMsgTxt("drive_series without drive");
        if (mxGetNumberOfElements(prhs[9]) != B) mexErrMsgTxt("drive_series must have one entry per chain");
        ser.resize((size_t)B);
        for (mwSize c = 0; c < B; c++) {
            const double v = mxGetPr(prhs[9])[c];
            if (!(v >= 1.0 && v <= (double)Sd) || (double)(mwSize)v != v) mexErrMsgTxt("drive_series value outside 1 .. Sd");
            ser[(size_t)c] = (int32_t)v - 1;
        }
    }
    const bool given = !mxIsEmpty(prhs[10]) || !mxIsEmpty(prhs[11]);
    if (given) {
        if (mxIsEmpty(prhs[10]) || mxIsEmpty(prhs[11])) mexErrMsgTxt("A and noise_var are given together or not at all");
        want(prhs[10], R, p, "A");
        if (mxGetNumberOfElements(prhs[11]) != R) mexErrMsgTxt("noise_var must have one entry per region");
    }
    epi_arfc_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION; d.R = (int32_t)R; d.D = (int32_t)D; d.L = (int32_t)L; d.p = (int32_t)p; d.H = (int32_t)H;
    d.fit = given ? 0 : 1; d.nv_mode = (int32_t)nvd; d.Sd = (int32_t)Sd; d.dt = mxGetScalar(prhs[3]);
    epi_arfc_inputs in;
    memset(&in, 0, sizeof in);
    const double *prm = mxGetPr(prhs[2]);
    in.seg = mxGetPr(prhs[1]); in.beta = prm; in.s0 = prm + R; in.i0 = prm + 2 * R;
    in.z = opt(prhs[7]); in.drive = opt(prhs[8]); in.drive_series = ser.empty() ? NULL : ser.data();
    in.A = given ? mxGetPr(prhs[10]) : NULL; in.noise_var = given ? mxGetPr(prhs[11]) : NULL;
    // the ABI's [K][3][B], [p][R] are MATLAB's B x 3 x K, R x p: no transposition
    mxArray *o[4] = {dbl3(B, 3, K ? K : 1), mxCreateDoubleMatrix(R, p ? p : 1, mxREAL), mxCreateDoubleMatrix(R, 1, mxREAL), mxCreateDoubleMatrix(R, 1, mxREAL)};
    std::vector<int32_t> st((size_t)R);
    epi_arfc_outputs out;
    memset(&out, 0, sizeof out);
    out.S = mxGetPr(o[0]); out.A_out = mxGetPr(o[1]); out.noise_var_out = mxGetPr(o[2]); out.status = st.data();
    char err[256] = {0};
    const int rc = seeded ? epi_arfc_run_host_seeded(&d, &nd, &in, &out, /*device=*/0, err) : epi_arfc_run_host(&d, &in, &out, /*device=*/0, err);
    if (rc != EPI_OK) { for (mxArray *m : o) mxDestroyArray(m); fail_if(rc, err); }
    for (size_t k = 0; k < st.size(); k++) mxGetPr(o[3])[k] = (double)st[k];
    for (int k = 0; k < 4; k++)
        if (k < nlhs || k == 0) plhs[k] = o[k]; else mxDestroyArray(o[k]);
}

static void fuse(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs != 7) mexErrMsgTxt("epiekf_pipeline_mex('fuse', S_f, P_f, S_b, P_b, form, p_solver): 7 inputs expected");
    for (int k = 1; k <= 4; k++)
        if (mxIsEmpty(prhs[k]) || !mxGetPr(prhs[k])) mexErrMsgTxt("S_f, P_f, S_b and P_b must be non-empty double arrays");
    if (mxGetNumberOfDimensions(prhs[1]) != 2) mexErrMsgTxt("S_f must be m x T");
    const mwSize m = mxGetM(prhs[1]), T = mxGetN(prhs[1]);
    if (m != 3 && m != 6) mexErrMsgTxt("m must be 3 or 6");
    want(prhs[3], m, T, "S_b");
    for (int k = 2; k <= 4; k += 2) {
        // m x m x T; MATLAB drops a trailing singleton: m x m for T = 1
        const mwSize nd = mxGetNumberOfDimensions(prhs[k]);
        const mwSize *dm = mxGetDimensions(prhs[k]);
        if (nd < 2 || nd > 3 || dm[0] != m || dm[1] != m || (nd == 3 ? dm[2] : 1) != T)
            mexErrMsgTxt(k == 2 ? "P_f must be m x m x T" : "P_b must be m x m x T");
    }
    for (int k = 5; k <= 6; k++)
        if (mxIsEmpty(prhs[k]) || !mxGetPr(prhs[k]) || mxGetNumberOfElements(prhs[k]) != 1) mexErrMsgTxt("form and p_solver must be double scalars");
    const double fd = mxGetScalar(prhs[5]), pd = mxGetScalar(prhs[6]);
    if ((fd != 0.0 && fd != 1.0) || (pd != 0.0 && pd != 1.0)) mexErrMsgTxt("form and p_solver must be 0 or 1");
    epi_fuse_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION; d.m = (int32_t)m; d.B = 1; d.T = (int32_t)T; d.form = (int32_t)fd; d.p_solver = (int32_t)pd;
    epi_fuse_inputs in;
    memset(&in, 0, sizeof in);
    in.sf = mxGetPr(prhs[1]); in.Pf = mxGetPr(prhs[2]); in.sb = mxGetPr(prhs[3]); in.Pb = mxGetPr(prhs[4]);
    // the ABI's [T][m][1], [T][m*m][1] (entry (i, j) in row i + m j) are MATLAB's m x T, m x m x T: no transposition
    mxArray *o[4] = {mxCreateDoubleMatrix(m, T, mxREAL), dbl3(m, m, T), mxCreateDoubleMatrix(1, T, mxREAL), mxCreateDoubleMatrix(1, T, mxREAL)};
    std::vector<int32_t> rk((size_t)T);
    epi_fuse_outputs out;
    memset(&out, 0, sizeof out);
    out.s_out = mxGetPr(o[0]); out.P_out = mxGetPr(o[1]); out.d2 = mxGetPr(o[2]); out.rank = rk.data();
    char err[256] = {0};
    const int rc = epi_fuse_run_host(&d, &in, &out, /*device=*/0, err);
    if (rc != EPI_OK) { for (mxArray *a : o) mxDestroyArray(a); fail_if(rc, err); }
    for (size_t k = 0; k < rk.size(); k++) mxGetPr(o[3])[k] = (double)rk[k];
    for (int k = 0; k < 4; k++)
        if (k < nlhs || k == 0) plhs[k] = o[k]; else mxDestroyArray(o[k]);
}

static void loglik(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs != 12) mexErrMsgTxt("epiekf_pipeline_mex('loglik', model_id, S_MINUS, P_MINUS, innovations, x, R_v, prm, L, obs_type, k_first, k_last): 12 inputs expected");
    for (int k = 1; k <= 9; k++)
        if (mxIsEmpty(prhs[k]) || !mxGetPr(prhs[k])) mexErrMsgTxt("model_id ... obs_type must be non-empty double arrays");
    const int model = (int)mxGetScalar(prhs[1]);
    const int mm = epi_model_dim(model);
    if (mm < 0) mexErrMsgTxt("unknown model id");
    const mwSize m = (mwSize)mm;
    if (mxGetNumberOfDimensions(prhs[2]) != 2 || mxGetM(prhs[2]) != m) mexErrMsgTxt("S_MINUS must be m x T");
    const mwSize T = mxGetN(prhs[2]);
    {
        const mwSize nd = mxGetNumberOfDimensions(prhs[3]);
        const mwSize *dm = mxGetDimensions(prhs[3]);
        if (nd < 2 || nd > 3 || dm[0] != m || dm[1] != m || (nd == 3 ? dm[2] : 1) != T) mexErrMsgTxt("P_MINUS must be m x m x T");
    }
    if (mxGetNumberOfElements(prhs[4]) != T || mxGetNumberOfElements(prhs[5]) != T) mexErrMsgTxt("innovations and x must be 1 x T");
    const mwSize nr = mxGetNumberOfElements(prhs[6]);
    if (nr != 1 && nr != T) mexErrMsgTxt("R_v must be 1 x T or a scalar");
    if (mxGetNumberOfElements(prhs[7]) != EPI_PRM_COUNT) mexErrMsgTxt("prm must hold EPI_PRM_COUNT entries");
    double kf = 1.0, kl = (double)T;
    if (!mxIsEmpty(prhs[10])) kf = mxGetScalar(prhs[10]);
    if (!mxIsEmpty(prhs[11])) kl = mxGetScalar(prhs[11]);
    if (!(kf >= 1.0 && kl >= kf && kl <= (double)T) || kf != (double)(int32_t)kf || kl != (double)(int32_t)kl)
        mexErrMsgTxt("k_first, k_last must be integers with 1 <= k_first <= k_last <= T");
    epi_loglik_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION; d.model = model; d.B = 1; d.T = (int32_t)T; d.L = (int32_t)mxGetScalar(prhs[8]);
    d.obs_type = (int32_t)mxGetScalar(prhs[9]); d.r_mode = (nr == T && T > 1) ? 1 : 0; d.Sx = 1;
    d.k0 = (int32_t)kf - 1; d.k1 = (int32_t)kl;
    epi_loglik_inputs in;
    memset(&in, 0, sizeof in);
    // the ABI's [T][m][1], [T][m*m][1] (entry (i, j) in row i + m j) are MATLAB's m x T, m x m x T: no transposition
    in.S_MINUS = mxGetPr(prhs[2]); in.P_MINUS = mxGetPr(prhs[3]); in.innovations = mxGetPr(prhs[4]); in.x = mxGetPr(prhs[5]);
    if (d.r_mode) in.R_series = mxGetPr(prhs[6]); else in.R_scalar = mxGetPr(prhs[6]);
    in.prm = mxGetPr(prhs[7]);
    mxArray *o[7];
    for (int k = 0; k < 7; k++) o[k] = mxCreateDoubleMatrix(1, k < 4 ? 1 : T, mxREAL);
    int32_t nv = 0, st = 0;
    epi_loglik_outputs out;
    memset(&out, 0, sizeof out);
    out.loglik = mxGetPr(o[0]); out.nis_mean = mxGetPr(o[1]); out.n_valid = &nv; out.status = &st;
    out.S = mxGetPr(o[4]); out.nis = mxGetPr(o[5]); out.R_used = mxGetPr(o[6]);
    char err[256] = {0};
    const int rc = epi_loglik_run_host(&d, &in, &out, /*device=*/0, err);
    if (rc != EPI_OK) { for (mxArray *a : o) mxDestroyArray(a); fail_if(rc, err); }
    mxGetPr(o[2])[0] = (double)nv; mxGetPr(o[3])[0] = (double)st;
    for (int k = 0; k < 7; k++)
        if (k < nlhs || k == 0) plhs[k] = o[k]; else mxDestroyArray(o[k]);
}

static void plan(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs != 13) mexErrMsgTxt("epiekf_pipeline_mex('plan', sp, u_min, eps, H, u_fixed, u_init, J0_prefix, J1_prefix, prefix_days, max_iter, max_halvings, tol): 13 inputs expected");
    for (int k = 1; k <= 4; k++)
        if (mxIsEmpty(prhs[k]) || !mxGetPr(prhs[k])) mexErrMsgTxt("sp, u_min, eps, H must be non-empty double arrays");
    for (int k = 9; k <= 12; k++)
        if (mxIsEmpty(prhs[k]) || !mxGetPr(prhs[k])) mexErrMsgTxt("prefix_days, max_iter, max_halvings, tol must be scalars");
    const mwSize R = mxGetM(prhs[1]), n = mxGetN(prhs[2]), P = mxGetNumberOfElements(prhs[3]);
    want(prhs[1], R, EPI_SIM_PRM_COUNT, "sp");
    if (mxGetM(prhs[2]) != R) mexErrMsgTxt("u_min must be R x n_npi");
    epi_plan_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION; d.R = (int32_t)R; d.P = (int32_t)P; d.H = (int32_t)mxGetScalar(prhs[4]); d.n_npi = (int32_t)n;
    d.prefix_days = (int32_t)mxGetScalar(prhs[9]); d.max_iter = (int32_t)mxGetScalar(prhs[10]);
    d.max_halvings = (int32_t)mxGetScalar(prhs[11]); d.tol = mxGetScalar(prhs[12]);
    char err[256] = {0};
    fail_if(epi_plan_validate(&d, err), err);
    const mwSize B = R * P, H = (mwSize)d.H;
    if (!mxIsEmpty(prhs[5]) && mxGetNumberOfElements(prhs[5]) != R * n * H) mexErrMsgTxt("u_fixed must be R x n_npi x H");
    if (!mxIsEmpty(prhs[6]) && mxGetNumberOfElements(prhs[6]) != B * n * H) mexErrMsgTxt("u_init must be (P*R) x n_npi x H");
    if (d.prefix_days > 0 && (mxGetNumberOfElements(prhs[7]) != R || mxGetNumberOfElements(prhs[8]) != R)) mexErrMsgTxt("J0_prefix, J1_prefix must have one entry per region");
    epi_plan_inputs in;
    memset(&in, 0, sizeof in);
    in.sp = mxGetPr(prhs[1]); in.u_min = mxGetPr(prhs[2]); in.eps = mxGetPr(prhs[3]); in.u_fixed = opt(prhs[5]); in.u_init = opt(prhs[6]);
    in.J0_prefix = d.prefix_days > 0 ? mxGetPr(prhs[7]) : NULL; in.J1_prefix = d.prefix_days > 0 ? mxGetPr(prhs[8]) : NULL;
    mxArray *o[11];
    o[0] = dbl3(B, n, H);
    for (int k = 1; k < 8; k++) o[k] = mxCreateDoubleMatrix(P, R, mxREAL);
    o[8] = nlhs > 8 ? dbl3(B, 3, H) : NULL;
    o[9] = nlhs > 9 ? dbl3(B, 3, H) : NULL;
    o[10] = nlhs > 10 ? mxCreateDoubleMatrix(B, (mwSize)d.max_iter, mxREAL) : NULL;
    std::vector<int32_t> it(B), hv(B), st(B);
    epi_plan_outputs out;
    memset(&out, 0, sizeof out);
    out.plan = mxGetPr(o[0]); out.J0 = mxGetPr(o[1]); out.J1 = mxGetPr(o[2]); out.F = mxGetPr(o[3]); out.gap = mxGetPr(o[4]);
    out.iters = it.data(); out.halvings = hv.data(); out.status = st.data();
    out.states = o[8] ? mxGetPr(o[8]) : NULL; out.mu = o[9] ? mxGetPr(o[9]) : NULL; out.F_trace = o[10] ? mxGetPr(o[10]) : NULL;
    const int rc = epi_plan_run_host(&d, &in, &out, /*device=*/0, err);
    if (rc != EPI_OK) { for (mxArray *a : o) if (a) mxDestroyArray(a); fail_if(rc, err); }
    for (size_t c = 0; c < (size_t)B; c++) { mxGetPr(o[5])[c] = (double)it[c]; mxGetPr(o[6])[c] = (double)hv[c]; mxGetPr(o[7])[c] = (double)st[c]; }
    for (int k = 0; k < 11; k++)
        if (k < nlhs || k == 0) plhs[k] = o[k]; else if (o[k]) mxDestroyArray(o[k]);
}

static void sdraw(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs != 12 && nrhs != 13) mexErrMsgTxt("epiekf_pipeline_mex('sdraw', S_PLUS, P_PLUS, S_MINUS, P_MINUS, prm, D, z, s_term, P_term, k_first, clamp): 12 inputs expected (a 13th: seed)");
    epi_noise_desc nd;
    const bool seeded = seed_arg(nrhs, prhs, 12, &nd);
    if (seeded && !mxIsEmpty(prhs[7])) mexErrMsgTxt("seed and z together: the draws have one source");
    for (int k = 1; k <= 6; k++)
        if (mxIsEmpty(prhs[k]) || !mxGetPr(prhs[k])) mexErrMsgTxt("S_PLUS ... D must be non-empty double arrays");
    if (mxGetNumberOfDimensions(prhs[1]) != 2 || mxGetM(prhs[1]) != 3) mexErrMsgTxt("S_PLUS must be 3 x T");
    const mwSize T = mxGetN(prhs[1]);
    if (mxGetNumberOfDimensions(prhs[3]) != 2 || mxGetM(prhs[3]) != 3 || mxGetN(prhs[3]) != T) mexErrMsgTxt("S_MINUS must be 3 x T");
    for (int k = 2; k <= 4; k += 2) {
        const mwSize nd = mxGetNumberOfDimensions(prhs[k]);
        const mwSize *dm = mxGetDimensions(prhs[k]);
        if (nd < 2 || nd > 3 || dm[0] != 3 || dm[1] != 3 || (nd == 3 ? dm[2] : 1) != T) mexErrMsgTxt("P_PLUS, P_MINUS must be 3 x 3 x T");
    }
    if (mxGetNumberOfElements(prhs[5]) != EPI_PRM_COUNT) mexErrMsgTxt("prm must hold EPI_PRM_COUNT entries");
    double kf = 1.0;
    if (!mxIsEmpty(prhs[10])) kf = mxGetScalar(prhs[10]);
    if (!(kf >= 1.0 && kf <= (double)T) || kf != (double)(int32_t)kf) mexErrMsgTxt("k_first must be an integer with 1 <= k_first <= T");
    epi_sdraw_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION; d.model = EPI_MODEL_SIA3; d.B = 1; d.T = (int32_t)T; d.D = (int32_t)mxGetScalar(prhs[6]);
    d.k0 = (int32_t)kf - 1; d.clamp = mxIsEmpty(prhs[11]) ? 1 : (int32_t)mxGetScalar(prhs[11]);
    char err[256] = {0};
    fail_if(epi_sdraw_validate(&d, err), err);
    const mwSize D = (mwSize)d.D, Tk = T - (mwSize)d.k0;
    if (!mxIsEmpty(prhs[7]) && mxGetNumberOfElements(prhs[7]) != D * 3 * Tk) mexErrMsgTxt("z must be D x 3 x (T - k_first + 1)");
    if (!mxIsEmpty(prhs[8]) && mxGetNumberOfElements(prhs[8]) != 3) mexErrMsgTxt("s_term must be 3 x 1");
    if (!mxIsEmpty(prhs[9]) && mxGetNumberOfElements(prhs[9]) != 9) mexErrMsgTxt("P_term must be 3 x 3");
    epi_sdraw_inputs in;
    memset(&in, 0, sizeof in);
    // the ABI's [T][3][1], [T][9][1] (entry (i, j) in row i + 3 j) are MATLAB's 3 x T, 3 x 3 x T; [T'][3][D] is D x 3 x T'
    in.S_PLUS = mxGetPr(prhs[1]); in.P_PLUS = mxGetPr(prhs[2]); in.S_MINUS = mxGetPr(prhs[3]); in.P_MINUS = mxGetPr(prhs[4]);
    in.prm = mxGetPr(prhs[5]); in.z = opt(prhs[7]); in.s_term = opt(prhs[8]); in.P_term = opt(prhs[9]);
    mxArray *o[5];
    o[0] = dbl3(D, 3, Tk);
    o[1] = mxCreateDoubleMatrix(1, T, mxREAL);
    o[2] = mxCreateDoubleMatrix(1, 1, mxREAL);
    o[3] = nlhs > 3 ? dbl3(3, 3, T) : NULL;
    o[4] = nlhs > 4 ? dbl3(3, 3, T) : NULL;
    std::vector<int32_t> rk(T);
    int32_t st = 0;
    epi_sdraw_outputs out;
    memset(&out, 0, sizeof out);
    out.X = mxGetPr(o[0]); out.rank = rk.data(); out.status = &st;
    out.J = o[3] ? mxGetPr(o[3]) : NULL; out.L = o[4] ? mxGetPr(o[4]) : NULL;
    const int rc = seeded ? epi_sdraw_run_host_seeded(&d, &nd, &in, &out, /*device=*/0, err) : epi_sdraw_run_host(&d, &in, &out, /*device=*/0, err);
    if (rc != EPI_OK) { for (mxArray *a : o) if (a) mxDestroyArray(a); fail_if(rc, err); }
    for (size_t k = 0; k < (size_t)T; k++) mxGetPr(o[1])[k] = (double)rk[k];
    mxGetPr(o[2])[0] = (double)st;
    for (int k = 0; k < 5; k++)
        if (k < nlhs || k == 0) plhs[k] = o[k]; else if (o[k]) mxDestroyArray(o[k]);
}

static void idiag(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs != 7) mexErrMsgTxt("epiekf_pipeline_mex('idiag', e, S, n_lags, k_first, k_last, flip): 7 inputs expected");
    if (mxIsEmpty(prhs[1]) || !mxGetPr(prhs[1]) || mxIsEmpty(prhs[3]) || !mxGetPr(prhs[3]) || mxIsEmpty(prhs[6]) || !mxGetPr(prhs[6]))
        mexErrMsgTxt("e, n_lags and flip must be non-empty double arrays");
    const mwSize T = mxGetNumberOfElements(prhs[1]);
    const bool hasS = !mxIsEmpty(prhs[2]);
    if (hasS && (!mxGetPr(prhs[2]) || mxGetNumberOfElements(prhs[2]) != T)) mexErrMsgTxt("S must be 1 x T or []");
    const double nl = mxGetScalar(prhs[3]), fl = mxGetScalar(prhs[6]);
    if (nl != (double)(int32_t)nl) mexErrMsgTxt("n_lags must be an integer");
    if (fl != 0.0 && fl != 1.0) mexErrMsgTxt("flip must be 0 or 1");
    double kf = 1.0, kl = (double)T;
    if (!mxIsEmpty(prhs[4])) kf = mxGetScalar(prhs[4]);
    if (!mxIsEmpty(prhs[5])) kl = mxGetScalar(prhs[5]);
    if (!(kf >= 1.0 && kl >= kf - 1.0 && kl <= (double)T) || kf != (double)(int32_t)kf || kl != (double)(int32_t)kl)
        mexErrMsgTxt("k_first, k_last must be integers with 1 <= k_first <= k_last + 1 <= T + 1");
    epi_idiag_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION; d.B = 1; d.T = (int32_t)T; d.flip = (int32_t)fl; d.k0 = (int32_t)kf - 1; d.k1 = (int32_t)kl;
    d.n_lags = (int32_t)nl;
    char err[256] = {0};
    fail_if(epi_idiag_validate(&d, err), err);                 // before n_lags sizes anything
    epi_idiag_inputs in;
    memset(&in, 0, sizeof in);
    in.e = mxGetPr(prhs[1]); in.S = hasS ? mxGetPr(prhs[2]) : nullptr;
    mxArray *o[2] = {mxCreateDoubleMatrix(18, 1, mxREAL), mxCreateDoubleMatrix((mwSize)d.n_lags, 1, mxREAL)};
    double *st = mxGetPr(o[0]);
    int32_t iv[7] = {0, 0, 0, 0, 0, 0, 0};
    epi_idiag_outputs out;
    memset(&out, 0, sizeof out);
    out.mean = st + 0; out.var = st + 1; out.skew = st + 2; out.kurt = st + 3; out.jb = st + 4; out.nis_sum = st + 5;
    out.nis_mean = st + 6; out.lb_q = st + 7; out.het = st + 8; out.cusumsq_max = st + 9; out.max_abs = st + 10;
    out.n = iv + 0; out.lb_lags = iv + 1; out.het_n1 = iv + 2; out.het_n2 = iv + 3; out.cusumsq_step = iv + 4;
    out.max_abs_step = iv + 5; out.status = iv + 6;
    out.acf = d.n_lags > 0 ? mxGetPr(o[1]) : nullptr;
    const int rc = epi_idiag_run_host(&d, &in, &out, /*device=*/0, err);
    if (rc != EPI_OK) { for (mxArray *a : o) mxDestroyArray(a); fail_if(rc, err); }
    for (int k = 0; k < 7; k++) st[11 + k] = (double)(iv[k] + ((k == 4 || k == 5) ? 1 : 0));      // the two steps ONE-based
    for (int k = 0; k < 2; k++)
        if (k < nlhs || k == 0) plhs[k] = o[k]; else mxDestroyArray(o[k]);
}

static void mc(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs != 10 && nrhs != 11) mexErrMsgTxt("epiekf_pipeline_mex('mc', sp, u_min, n_scen, K, seed, z, J0_prefix, J1_prefix, prefix_days): 10 inputs expected (an 11th: noise_seed)");
    epi_noise_desc nd;
    const bool seeded = seed_arg(nrhs, prhs, 10, &nd);
    if (seeded && !mxIsEmpty(prhs[6])) mexErrMsgTxt("noise_seed and z together: the draws have one source");
    const mwSize R = mxGetM(prhs[1]), n = mxGetN(prhs[2]);
    want(prhs[1], R, EPI_SIM_PRM_COUNT, "sp");
    if (mxGetM(prhs[2]) != R) mexErrMsgTxt("u_min must be R x n_npi");
    epi_mc_desc d;
    memset(&d, 0, sizeof d);
    d.abi_version = EPIEKF_ABI_VERSION; d.R = (int32_t)R; d.n_scen = (int32_t)mxGetScalar(prhs[3]); d.K = (int32_t)mxGetScalar(prhs[4]); d.n_npi = (int32_t)n;
    const double seed = mxGetScalar(prhs[5]);
    d.seed_lo = (uint32_t)((uint64_t)seed & 0xFFFFFFFFu); d.seed_hi = (uint32_t)((uint64_t)seed >> 32);
    d.noise = mxIsEmpty(prhs[6]) ? 0 : 1; d.prefix_days = (int32_t)mxGetScalar(prhs[9]);
    if (d.n_scen < 1 || d.K < 1) mexErrMsgTxt("n_scen and K must be positive");
    const mwSize B = R * (mwSize)d.n_scen;
    if (d.noise && mxGetNumberOfElements(prhs[6]) != B * 3 * (mwSize)d.K) mexErrMsgTxt("z must be (n_scen*R) x 3 x K");
    if (d.prefix_days > 0 && (mxGetNumberOfElements(prhs[7]) != R || mxGetNumberOfElements(prhs[8]) != R)) mexErrMsgTxt("J0_prefix, J1_prefix must have one entry per region");
    mxArray *j0 = mxCreateDoubleMatrix(R, (mwSize)d.n_scen, mxREAL), *j1 = mxCreateDoubleMatrix(R, (mwSize)d.n_scen, mxREAL);
    mxArray *uo = nlhs > 2 ? dbl3(B, n, (mwSize)d.K) : NULL;
    char err[256] = {0};
    const double *j0p = d.prefix_days > 0 ? mxGetPr(prhs[7]) : NULL, *j1p = d.prefix_days > 0 ? mxGetPr(prhs[8]) : NULL;
    const int rc = seeded ? epi_random_npi_mc_host_seeded(&d, &nd, mxGetPr(prhs[1]), mxGetPr(prhs[2]), NULL, j0p, j1p, uo ? mxGetPr(uo) : NULL,
                                                          mxGetPr(j0), mxGetPr(j1), /*device=*/0, err)
                          : epi_random_npi_mc_host(&d, mxGetPr(prhs[1]), mxGetPr(prhs[2]), opt(prhs[6]), j0p, j1p, uo ? mxGetPr(uo) : NULL,
                                                   mxGetPr(j0), mxGetPr(j1), /*device=*/0, err);
    if (rc != EPI_OK) { mxDestroyArray(j0); mxDestroyArray(j1); mxDestroyArray(uo); fail_if(rc, err); }
    plhs[0] = j0;
    if (nlhs > 1) plhs[1] = j1; else mxDestroyArray(j1);
    if (nlhs > 2) plhs[2] = uo;
}

static void noise(int, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    if (nrhs < 5 || nrhs > 7) mexErrMsgTxt("epiekf_pipeline_mex('noise', nt, rows, lanes, seed, t0, lane0): 5 to 7 inputs expected");
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};              // nt, rows, lanes, t0, lane0
    const int at[5] = {1, 2, 3, 5, 6};
    for (int k = 0; k < 5; k++) {
        if (at[k] >= nrhs || (k >= 3 && mxIsEmpty(prhs[at[k]]))) continue;
        if (!mxGetPr(prhs[at[k]]) || mxGetNumberOfElements(prhs[at[k]]) != 1) mexErrMsgTxt("nt, rows, lanes, t0 and lane0 must be double scalars");
        v[k] = mxGetScalar(prhs[at[k]]);
        if (!(v[k] >= 0.0 && v[k] <= 9007199254740992.0) || (double)(int64_t)v[k] != v[k]) mexErrMsgTxt("nt, rows, lanes, t0 and lane0 must be non-negative integers");
    }
    epi_noise_desc nd;
    if (!seed_arg(nrhs, prhs, 4, &nd)) mexErrMsgTxt("seed must be a double scalar or [seed, stream]");
    char err[256] = {0};
    if (v[0] < 1.0 || v[2] < 1.0) mexErrMsgTxt("nt and lanes must be >= 1");
    if (v[1] != 1.0 && v[1] != 3.0) mexErrMsgTxt("rows must be 1 or 3");
    if (v[0] * v[1] * v[2] > 2147483647.0) mexErrMsgTxt("nt * rows * lanes is limited to 2^31 - 1: ask for a window");
    // the ABI's [nt][rows][lanes] is MATLAB's lanes x rows x nt
    mxArray *z = dbl3((mwSize)v[2], (mwSize)v[1], (mwSize)v[0]);
    const int rc = epi_noise_fill_host(&nd, (int64_t)v[3], (int64_t)v[0], (int32_t)v[1], (int64_t)v[4], (int64_t)v[2], 0, mxGetPr(z), /*device=*/0, err);
    if (rc != EPI_OK) { mxDestroyArray(z); fail_if(rc, err); }
    plhs[0] = z;
}

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[])
{
    char cmd[16] = {0};
    if (nrhs < 1 || mxGetString(prhs[0], cmd, sizeof cmd) != 0) mexErrMsgTxt("epiekf_pipeline_mex: first argument is the command string");
    mexAtExit(epi_host_pool_release);       // `clear mex` hands the library's pooled contexts, helper streams and worker threads back
    if (strcmp(cmd, "prescribe") == 0) prescribe(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "preprocess") == 0) preprocess(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "nnls") == 0) nnls(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "lasso") == 0) lasso(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "robustfit") == 0) robustfit(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "ratemap") == 0) ratemap(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "mldivide") == 0) mldivide(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "svr") == 0) svr(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "ens_summary") == 0) ens_summary(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "ar_forecast") == 0) ar_forecast(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "fuse") == 0) fuse(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "loglik") == 0) loglik(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "idiag") == 0) idiag(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "plan") == 0) plan(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "sdraw") == 0) sdraw(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "escore") == 0) escore(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "pathfn") == 0) pathfn(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "cdepth") == 0) cdepth(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "jscore") == 0) jscore(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "mc") == 0) mc(nlhs, plhs, nrhs, prhs);
    else if (strcmp(cmd, "noise") == 0) noise(nlhs, plhs, nrhs, prhs);
    else mexErrMsgTxt("epiekf_pipeline_mex: unknown command");
}

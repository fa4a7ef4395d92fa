"""The device stages of Tools/TrainPredictPrescribeNPI.m chained for ALL regions at once:

    data-set columns --preprocess--> x, R_v, u, I0                                   (:142-198, 201-202, 240)
      --SIAlphaModelEKF, zero input--> alpha estimate                                 (:203-248)
      --lsqnonneg + intercept loop--> a, b                                            (:251-276)
      --SIAlphaModelEKF, real inputs--> alpha estimate                                (:296-305)
      --lsqnonneg + intercept loop--> a2, b2                                          (:306-330)
      --SIAlphaModelEKF, last plan held over the horizon--> s/i/alpha_historic        (:351-362)
      --SIAlphaModelEKFOptControlled sweep over the cost weights--> u_opt_smooth      (:421-460)
      --SIalpha_Controlled + NPICost--> (J0, J1) per cost weight                      (:481-493)
      --Pareto front + optimum--> prescription per region                             (:624-633)

The reference walks the regions (and, inside, the 250 cost weights) in serial MATLAB loops; here every stage is one
batched call into libepiekf.so.  Only per-region vectors (I0, a, b, end-of-history state, cost prefixes) cross the
host between stages; the filter outputs stay in HBM.  `prescribe()` returns every intermediate so that the tests can
re-derive each stage from the previous one with the CPU oracle."""
from __future__ import annotations

import numpy as np
import torch

from . import batch, layout as L, synth


def filter_setup(I0, N, dt=1.0):
    """s_init, Q_w, Ps_init of the 3-state filter per region (TrainPredictPrescribeNPI.m:229-237) -> [3,S],[9,S],[9,S]."""
    S = N.shape[0]
    stds = np.stack([10.0 * I0 / N, 30.0 * I0 / N, np.full(S, 1e-2)])
    Q = np.zeros((9, S)); P0 = np.zeros((9, S))
    for d in range(3):
        Q[d * 3 + d] = dt ** 2 * stds[d] ** 2
        P0[d * 3 + d] = dt ** 2 * (10 * stds[d]) ** 2
    s_init = np.stack([(N - I0) / N, I0 / N, np.full(S, synth.ALPHA0)])
    return s_init, Q, P0


def _prm3(N, a, b, n_npi):
    S = N.shape[0]
    prm = synth._base_prm(S)
    prm[L.PRM_S_MIN] = synth.MIN_CASES / N
    prm[L.PRM_I_MIN] = synth.MIN_CASES / N
    prm[L.PRM_B] = b
    prm[L.PRM_A:L.PRM_A + n_npi] = a
    return prm


def workload3(x, R, u, N, I0, a, b):
    """SIAlphaModelEKF over all regions: x, R [T,S], u [T,n,S]; a [n,S], b [S]."""
    T, S = x.shape
    s_init, Q, P0 = filter_setup(I0, N)
    return synth.Workload(model="SIAlphaModelEKF", T=T, n_npi=u.shape[1], x=np.ascontiguousarray(x), u=np.ascontiguousarray(u),
                          R_series=np.ascontiguousarray(R), R_scalar=None, x_series=None, u_series=None,
                          prm=_prm3(N, a, b, u.shape[1]), s_init=s_init, Ps_init=P0, s_final=np.full((3, S), np.nan),
                          Ps_final=np.full((9, S), np.nan), Q=Q)


def sweep_region_inputs(N, I0, a, b, n, w_eff=1.0):
    """Per-REGION arguments of the 6-state sweep (TrainPredictPrescribeNPI.m:423-453): prm [61,S] (EPSILON row left 0),
    s_init [6,S], Ps_init, s_final, Ps_final, Q [36,S].  The cost weight is the only thing that differs between the P
    chains of a region."""
    S = N.shape[0]
    s3, Q3, P3 = filter_setup(I0, N)
    prm = _prm3(N, a, b, n)
    prm[L.PRM_W_EFF:L.PRM_W_EFF + n] = w_eff
    s_init = np.zeros((6, S)); s_init[:3] = s3
    Q = np.zeros((36, S)); P0 = np.zeros((36, S))
    for d in range(3):
        Q[d * 6 + d] = Q3[d * 3 + d]; P0[d * 6 + d] = P3[d * 3 + d]
    for d in range(3, 6):
        Q[d * 6 + d] = synth.Q_LAMBDA ** 2; P0[d * 6 + d] = 10.0 * synth.Q_LAMBDA ** 2
    s_final = np.full((6, S), np.nan); s_final[3:] = 0.0
    Ps_final = np.zeros((36, S))
    for i in range(3):
        for j in range(3):
            Ps_final[i + 6 * j] = np.nan
    for d in range(3, 6):
        Ps_final[d * 6 + d] = 1e-8
    return dict(prm=prm, s_init=s_init, Ps_init=P0, s_final=s_final, Ps_final=Ps_final, Q=Q)


def workload6(x, R, u, N, I0, a, b, eps_grid, w_eff=1.0):
    """SIAlphaModelEKFOptControlled sweep: chain c = region * n_eps + e (:421-460).  x, R [T,S] with NaN over the
    horizon, u [T,n,S] with NaN over the horizon."""
    T, S = x.shape
    n, P = u.shape[1], eps_grid.shape[0]
    rr = np.repeat(np.arange(S), P)
    reg = sweep_region_inputs(N, I0, a, b, n, w_eff)
    prm = reg["prm"][:, rr]
    prm[L.PRM_EPSILON] = np.tile(eps_grid, S)
    return synth.Workload(model="SIAlphaModelEKFOptControlled", T=T, n_npi=n, x=np.ascontiguousarray(x),
                          u=np.ascontiguousarray(u), R_series=np.ascontiguousarray(R), R_scalar=None,
                          x_series=rr.astype(np.int32), u_series=rr.astype(np.int32), prm=prm, s_init=reg["s_init"][:, rr],
                          Ps_init=reg["Ps_init"][:, rr], s_final=reg["s_final"][:, rr], Ps_final=reg["Ps_final"][:, rr],
                          Q=reg["Q"][:, rr])


def scoring_region_inputs(hist_end, a, b, u_max, wts):
    """Per-region scoring block sp [48,S] (EPI_SIM_* rows) of the sweep's tail (:481): end-of-history state, model
    constants, NPI_MAXES, NPICost weights."""
    n, S = a.shape
    sp = np.zeros((batch.SIM_PRM_COUNT, S))
    sp[0:3] = hist_end
    sp[3], sp[4], sp[5] = synth.ALPHA_MIN, synth.ALPHA_MAX, synth.MODEL_GAMMA
    sp[6], sp[7], sp[11] = b, synth.MODEL_BETA, 1.0
    sp[batch.SIM_A:batch.SIM_A + n] = a
    sp[batch.SIM_U_MAX:batch.SIM_U_MAX + n] = u_max[:, None]
    sp[batch.SIM_W:batch.SIM_W + n] = wts
    return sp


def _alpha_smooth(w, device):
    dw = batch.DeviceWorkload(w, device)
    r = batch.EkfRunner(dw, outputs=["S_SMOOTH"])
    r.run()
    torch.cuda.synchronize(dw.device)
    return r.out["S_SMOOTH"].cpu().numpy()                 # [T, 3, S]


REGRESSIONS = ("nonnegls", "lasso", "elementwise")


def _regress(X, y, regression, cv_folds, cv_seed, device):
    """One regression between the EKF rounds (TrainPredictPrescribeNPI.m:251-290): 'nonnegls' = lsqnonneg + the intercept
    loop (batch.nnls_affine_fit), 'lasso' = lasso(X, y, 'CV', cv_folds) with folds from cv_seed (batch.lasso_cv; a, b at
    IndexMinMSE, and the path's lambda, mse, se, idx_min_mse, idx_1se, status ... alongside), 'elementwise' = the robust
    bounded fit of every NPI on its own and b = mean(y - X a) (:279-292, batch.robust_affine_fit; b_item, sigma, iters,
    status alongside)."""
    if regression == "nonnegls":
        res = batch.nnls_affine_fit(X, y, device=device)
    elif regression == "elementwise":
        res = batch.robust_affine_fit(X, y, device=device)
    else:
        res = batch.lasso_cv(X, y, K=cv_folds, seed=cv_seed, device=device)
    return {k: v.cpu().numpy() for k, v in res.items()}


def _front_half(cases, deaths, N, ip, num_regression_days, W, device, regression="nonnegls", cv_folds=50, cv_seed=0):
    """Preprocessing, EKF round 1, regression, round 2, regression (TrainPredictPrescribeNPI.m:142-330,
    ForecastQualityAssessment.m:160-356) over the days given.  regression selects REGRESSION_TYPE: "nonnegls" (the
    default), "lasso" or "elementwise"; with "lasso" round 1 draws its folds from cv_seed and round 2 from cv_seed + 1 (the reference
    draws a fresh partition per lasso call).  Returns pre, alpha_round1, fit1, alpha_round2, fit2, X_reg."""
    if regression not in REGRESSIONS:
        raise ValueError(f"regression must be one of {REGRESSIONS}")
    T, S = cases.shape
    n = ip.shape[1]
    u_max = synth.IP_MAXES[:n]
    out = {}
    pre = {k: v.cpu().numpy() for k, v in batch.preprocess(cases, N, deaths, ip, W=W, min_cases=synth.MIN_CASES,
                                                            first_num_days=7, device=device).items()}
    out["pre"] = pre
    x, R, u, I0 = pre["x_new"], pre["R_v"], pre["ip_filled"], pre["I0"]
    # round 1: zero input, a = 0, b = 0 -> alpha estimate -> regression
    S1 = _alpha_smooth(workload3(x, R, np.zeros_like(u), N, I0, np.zeros((n, S)), np.zeros(S)), device)
    D = min(num_regression_days, T)
    X = np.ascontiguousarray(u_max[None, :, None] - u[T - D:])
    fit1 = _regress(X, np.ascontiguousarray(S1[T - D:, 2]), regression, cv_folds, cv_seed, device)
    # round 2: real inputs -> refined alpha -> second regression
    S2 = _alpha_smooth(workload3(x, R, u, N, I0, fit1["a"], fit1["b"]), device)
    fit2 = _regress(X, np.ascontiguousarray(S2[T - D:, 2]), regression, cv_folds, cv_seed + 1, device)
    out.update(alpha_round1=S1[:, 2], fit1=fit1, alpha_round2=S2[:, 2], fit2=fit2, X_reg=X)
    return out


def prescribe(cases, deaths, population, ip, horizon=30, n_eps=50, num_regression_days=60, npi_weights=None,
              W=7, device="cuda:0", regression="nonnegls", cv_folds=50, cv_seed=0, planner="sweep", plan_max_iter=64,
              plan_max_halvings=30, plan_tol=1e-9):
    """Run the chain above.  cases/deaths [T,S] cumulative counts (NaN = missing), population [S], ip [T,n,S] (NaN = N/A).
    regression = "nonnegls" (REGRESSION_TYPE 'NONNEGATIVELS', the default) or "lasso" ('LASSO': lasso(X, y, 'CV', cv_folds),
    folds drawn from cv_seed in round 1 and cv_seed + 1 in round 2; the coefficients may be negative) or "elementwise"
    (REGRESSION_TYPE 'NONNEGATIVELS-ELEMENT-WISE': a robust fit of alpha against every NPI on its own, slope >= 0,
    DESIGN.md §4.10; it needs num_regression_days >= 3).
    planner = "sweep" (the default: the reference's 6-state SIAlphaModelEKFOptControlled sweep, whose smoothed costates pick
    the plan) or "direct": the plan of every (region, cost weight) comes from batch.npi_plan (states forward,
    adjoint backward, up to plan_max_iter Frank-Wolfe steps to gap <= plan_tol |F|), scored by NPICost over [historic, horizon]
    like the sweep's and put through the same Pareto selection.  Over a long history the sweep's plan is rounding noise
    (DESIGN.md §2); the direct planner's is not.
    Returns a dict with every intermediate and `prescription` [horizon, n, S]: the smoothed optimal plan of each region's
    Pareto optimum (`I_opt`), plus `front` [S, n_eps] and (J0, J1) [S, n_eps].  With planner = "direct" there are no sweep
    keys (`sweep`, `x_sweep`, `R_sweep`, `u_sweep`, `sweep_region`); instead `plan` [horizon, n, S * n_eps] (a device tensor),
    `plan_F`, `plan_gap` [S, n_eps] float64, `plan_iters`, `plan_halvings`, `plan_status` [S, n_eps] int32 (batch.npi_plan)."""
    if planner not in ("sweep", "direct"):
        raise ValueError('planner must be "sweep" or "direct"')
    T, S = cases.shape
    n = ip.shape[1]
    N = np.asarray(population, dtype=np.float64)
    u_max = synth.IP_MAXES[:n]
    out = _front_half(cases, deaths, N, ip, num_regression_days, W, device, regression, cv_folds, cv_seed)
    pre, fit2, X = out["pre"], out["fit2"], out["X_reg"]
    x, R, u, I0 = pre["x_new"], pre["R_v"], pre["ip_filled"], pre["I0"]
    # forecast set-up (:333-341): R_v padded with its mean, observations and (for the sweep) controls NaN over the horizon
    R_mean = R.sum(axis=0) / T
    xh = np.concatenate([x, np.full((horizon, S), np.nan)]); Rh = np.concatenate([R, np.repeat(R_mean[None], horizon, 0)])
    u_fixed = np.concatenate([u, np.repeat(u[-1:], horizon, 0)])                       # last plan held (:351-353)
    Sf = _alpha_smooth(workload3(xh, Rh, u_fixed, N, I0, fit2["a"], fit2["b"]), device)
    hist = Sf[:T]                                                                      # s/i/alpha_historic (:355-357)
    out.update(R_mean=R_mean, historic=hist)
    eps_grid = synth.epsilon_grid(n_eps)
    if planner == "direct":
        return _prescribe_direct(out, hist, u, u_fixed, fit2, u_max, npi_weights, eps_grid, horizon, I0, X, device, plan_max_iter,
                                 plan_max_halvings, plan_tol)
    # Pareto sweep over the cost weights
    u_nan = np.concatenate([u, np.full((horizon, n, S), np.nan)])
    w6 = workload6(xh, Rh, u_nan, N, I0, fit2["a"], fit2["b"], eps_grid)
    dw = batch.DeviceWorkload(w6, device)
    runner = batch.EkfRunner(dw, outputs=["u_opt_smooth", "S_SMOOTH"], lane_block="auto")   # chain-blocked outputs
    runner.run()
    uos = runner.out["u_opt_smooth"]                                                   # stays in HBM (blocked layout)
    # scoring (:481-493): simulate the horizon from the end-of-history state, NPICost over [historic, horizon]
    wts = np.ones((n, S)) if npi_weights is None else np.asarray(npi_weights, dtype=np.float64)
    rr = np.repeat(np.arange(S), n_eps)
    sp_region = scoring_region_inputs(hist[T - 1], fit2["a"], fit2["b"], u_max, wts)
    sp = sp_region[:, rr]
    J0p_region = np.cumsum(hist[:, 0] * hist[:, 1] * hist[:, 2], axis=0)[-1]           # sequential historic sums
    J1p_region = np.cumsum((wts[None] * u).reshape(T * n, S), axis=0)[-1]
    J0p, J1p = J0p_region[rr], J1p_region[rr]
    out.update(sp_region=sp_region, J0_prefix_region=J0p_region, J1_prefix_region=J1p_region, x_sweep=xh, R_sweep=Rh, u_sweep=u_nan,
               sweep_region=sweep_region_inputs(N, I0, fit2["a"], fit2["b"], n), I0=I0, u_fixed=u_fixed, X_reg=X)
    sc = batch.score_sweep(uos, T, sp, J0p, J1p, B=S * n_eps)
    front, i_opt = batch.pareto_front(sc["J0"], sc["J1"], S)
    torch.cuda.synchronize(dw.device)
    i_opt_h = i_opt.cpu().numpy()
    chains = np.arange(S) * n_eps + i_opt_h
    if uos.dim() == 4:            # blocked [T+H, nblk, n, blk]: pick (block, lane) of every optimum chain
        cb = torch.as_tensor(chains // runner.blk, device=uos.device); cr = torch.as_tensor(chains % runner.blk, device=uos.device)
        best = uos[T:][:, cb, :, cr].permute(1, 2, 0)          # index dims come first: [S, H, n] -> [H, n, S]
    else:
        best = uos[T:].index_select(2, torch.as_tensor(chains, device=uos.device))
    out.update(eps_grid=eps_grid, sp=sp, J0_prefix=J0p, J1_prefix=J1p,
               J0=sc["J0"].cpu().numpy().reshape(S, n_eps), J1=sc["J1"].cpu().numpy().reshape(S, n_eps),
               front=front.cpu().numpy(), i_opt=i_opt_h, sweep=w6,
               prescription=best.cpu().numpy())
    return out


def _prescribe_direct(out, hist, u, u_fixed, fit2, u_max, npi_weights, eps_grid, horizon, I0, X, device, max_iter, max_halvings, tol):
    """prescribe's tail with planner = "direct": batch.npi_plan from the end-of-history state, then the sweep's own Pareto
    selection over the call's (J0, J1)"""
    T, n, S = u.shape
    n_eps = eps_grid.shape[0]
    wts = np.ones((n, S)) if npi_weights is None else np.asarray(npi_weights, dtype=np.float64)
    sp_region = scoring_region_inputs(hist[T - 1], fit2["a"], fit2["b"], u_max, wts)
    J0p_region = np.cumsum(hist[:, 0] * hist[:, 1] * hist[:, 2], axis=0)[-1]           # sequential historic sums
    J1p_region = np.cumsum((wts[None] * u).reshape(T * n, S), axis=0)[-1]
    u_min = np.repeat(synth.IP_MINS[:n, None], S, axis=1)
    res = batch.npi_plan(sp_region, u_min, eps_grid, horizon, J0_prefix=J0p_region, J1_prefix=J1p_region, prefix_days=T,
                         max_iter=max_iter, max_halvings=max_halvings, tol=tol, device=device)
    front, i_opt = batch.pareto_front(res["J0"], res["J1"], S)
    torch.cuda.synchronize(res["plan"].device)
    i_opt_h = i_opt.cpu().numpy()
    chains = np.arange(S) * n_eps + i_opt_h
    best = res["plan"].index_select(2, torch.as_tensor(chains, device=res["plan"].device))
    rr = np.repeat(np.arange(S), n_eps)
    host = lambda k: res[k].cpu().numpy().reshape(S, n_eps)
    out.update(sp_region=sp_region, J0_prefix_region=J0p_region, J1_prefix_region=J1p_region, I0=I0, u_fixed=u_fixed, X_reg=X,
               eps_grid=eps_grid, sp=sp_region[:, rr], J0_prefix=J0p_region[rr], J1_prefix=J1p_region[rr], J0=host("J0"), J1=host("J1"),
               front=front.cpu().numpy(), i_opt=i_opt_h, prescription=best.cpu().numpy(), plan=res["plan"], plan_F=host("F"),
               plan_gap=host("gap"), plan_iters=host("iters"), plan_halvings=host("halvings"), plan_status=host("status"))
    return out


def forecast_quality(cases, deaths, population, ip, num_forecast_days, max_lookahead=60, num_regression_days=60, W=7,
                     device="cuda:0", chains=False, shape=0, regression="nonnegls", cv_folds=50, cv_seed=0):
    """The forecast look-ahead error study of Tools/ForecastQualityAssessment.m for ALL regions in one device call.

    cases / deaths [LL, S] cumulative counts (NaN = missing), population [S], ip [LL, n, S] (NaN = N/A) over the WHOLE window;
    the first LL - num_forecast_days days are the training window.  The front half (preprocessing, EKF round 1, NNLS, round 2,
    NNLS: :160-356) runs on the training window exactly as in prescribe(); the whole window is preprocessed too, giving the
    `_ENTIRE` quantities (:102-132): new_smoothed = NewCasesSmoothed_ENTIRE (the truth), x_new the observations, ip_filled the
    controls.  R_v of the training window is padded with its mean (:362).  Then every region is filtered once per start
    s = 1 .. num_forecast_days with its last s observations hidden (:380-393) and the error tables and their statistics over
    the starts max_lookahead .. num_forecast_days (:428-449) are computed (batch.lookahead).  regression, cv_folds and
    cv_seed select REGRESSION_TYPE as in prescribe() ("elementwise": REGRESSION_TYPE 'NONNEGATIVELS-ELEMENT-WISE').
    Returns a dict: the front half's intermediates (pre, alpha_round1, fit1, alpha_round2, fit2, X_reg), pre_entire, R_full,
    workload (the per-region synth.Workload of the study), truth, and est_plus / est_smooth [F, M, S],
    mean / median / std_{plus,smooth} [M, S] (+ S_PLUS / S_SMOOTH / status of every chain with chains=True)."""
    LL, S = cases.shape
    F = int(num_forecast_days)
    T = LL - F
    if F < 1 or T < 2:
        raise ValueError("num_forecast_days must be >= 1 and leave a training window of at least 2 days")
    N = np.asarray(population, dtype=np.float64)
    out = _front_half(cases[:T], None if deaths is None else deaths[:T], N, ip[:T], num_regression_days, W, device,
                      regression, cv_folds, cv_seed)
    fit2, I0, R = out["fit2"], out["pre"]["I0"], out["pre"]["R_v"]
    ent = {k: v.cpu().numpy() for k, v in batch.preprocess(cases, N, deaths, ip, W=W, min_cases=synth.MIN_CASES,
                                                            first_num_days=7, device=device).items()}
    R_mean = R.sum(axis=0) / T
    R_full = np.concatenate([R, np.repeat(R_mean[None], F, 0)])
    w = workload3(ent["x_new"], R_full, ent["ip_filled"], N, I0, fit2["a"], fit2["b"])
    truth = ent["new_smoothed"]
    res = batch.lookahead(w, truth, N, F, max_lookahead, device=device, chains=chains, shape=shape)
    out.update(pre_entire=ent, R_mean=R_mean, R_full=R_full, workload=w, truth=truth, **res)
    return out


# testScripts/test04FullFeatureExtMLpipeline.m:203-219: the exponential-fit EKF's settings in the feature-extraction pipeline
GROWTH_EKF = dict(w_bar=[0.0, 0.0], v_bar=0.0, Q_w=np.diag([250.0 ** 2, 3.0e-3 ** 2]), R_v=10.0 ** 2, beta=0.9, gamma=0.995,
                  inv_monitor_len=21, params=[1.0, 0.9, 0.1])


def growth_rate_ekf_workload(new_smoothed, order, forecast_days=0, s_init_lambda=None):
    """Rt_ExpFitEKF for every column of new_smoothed [T, S] with test04's settings (:197-219) as one synth.RtWorkload: the
    last `forecast_days` days hidden (NaN), s_init = [first sample; Lambda_GeoGenRatios(1)] per column (s_init_lambda [S],
    default 0: GenRatios' first value is always 0), Ps_init = 100 Q_w."""
    x = np.array(new_smoothed, dtype=np.float64, ndmin=2)
    T, S = x.shape
    if forecast_days > 0:
        x[T - int(forecast_days):] = np.nan
    e = GROWTH_EKF
    Q_w = e["Q_w"]
    rp = np.zeros((synth.RT_PRM_COUNT, S))                  # EPI_RT_* rows of include/epiekf.h
    rp[0:3] = np.asarray(e["params"])[:, None]
    rp[3:5] = np.asarray(e["w_bar"])[:, None]
    rp[5], rp[6], rp[7], rp[8] = e["v_bar"], e["R_v"], e["beta"], e["gamma"]
    rp[9] = x[0]
    rp[10] = 0.0 if s_init_lambda is None else np.asarray(s_init_lambda, dtype=np.float64)
    rp[11:15] = (100.0 * Q_w).reshape(-1, order="F")[:, None]
    rp[15:19] = Q_w.reshape(-1, order="F")[:, None]
    return synth.RtWorkload(x=np.ascontiguousarray(x), rp=rp, x_series=None, L=e["inv_monitor_len"], order=int(order))


def growth_rates(cases, population, wlen=7, generation_period=3, causal=1, forecast_days=0, time_unit=1.0, device="cuda:0"):
    """The growth-rate features of testScripts/test04FullFeatureExtMLpipeline.m (:160-219) for ALL regions:

      cumulative cases --batch.preprocess (W = wlen)--> new_smoothed   (test04's MOVINGAVERAGE-CAUSAL branch, :175)
      --batch.rt_window--> LogLinReg, GenRatios, NonlinLS in one call  (:185-195)
      --batch.RtRunner, orders 1 and 2--> Rt_ExpFitEKF of every region, one call per order   (:197-219)

    The daily counts come from this project's cleaning (preprocess: diff, negatives clamped to 0, a missing last day filled
    with the last valid one, other gaps 0); test04's own cleaning differs only in how several missing trailing days are
    filled.  cases [T, S] cumulative counts (NaN = missing), population [S].  Returns a dict: new_smoothed [T, S], the
    rt_window outputs [T, S] (llr_*, gr_*, nls_*), and per EKF order k ekf{k}_S_PLUS / ekf{k}_S_SMOOTH [T, 2, S]."""
    N = np.asarray(population, dtype=np.float64)
    pre = batch.preprocess(cases, N, W=wlen, min_cases=synth.MIN_CASES, first_num_days=7, outputs=("new_smoothed",),
                           device=device)
    ns = pre["new_smoothed"]
    rw = batch.rt_window(ns, wlen, time_unit, causal, generation_period, ("LogLinReg", "GenRatios", "NonlinLS"), device=device)
    out = {"new_smoothed": ns.cpu().numpy()}
    out.update({k: v.cpu().numpy() for k, v in rw.items()})
    for order in (1, 2):
        w = growth_rate_ekf_workload(out["new_smoothed"], order, forecast_days, out["gr_Lambda"][0])
        r = batch.rt_expfit(w, device=device, outputs=("S_PLUS", "S_SMOOTH"))
        out[f"ekf{order}_S_PLUS"], out[f"ekf{order}_S_SMOOTH"] = r["S_PLUS"], r["S_SMOOTH"]
    return out


GROWTH_TARGETS = ("llr_Lambda", "gr_Lambda", "gr_LambdaSmoothed", "nls_Lambda")
GROWTH_SOLVERS = ("ridge", "backslash", "svr", "svr_gaussian")


def backslash_features(ip_filled, lags, extra=None):
    """[ip_filled, its copies lagged by each of `lags` (zero on their first lag days), extra] as one device tensor [T, F, S]:
    rate_map's feature matrix before the normalisation"""
    T = ip_filled.shape[0]
    blocks = [ip_filled]
    for lag in lags:
        b = torch.zeros_like(ip_filled)
        b[int(lag):] = ip_filled[:T - int(lag)]
        blocks.append(b)
    if extra is not None:
        blocks.append(extra)
    return torch.cat(blocks, dim=1).contiguous()


def growth_forecast(cases, population, ip, predict_ahead=None, n_train=None, lags=(3, 5, 7), target="llr_Lambda", extra=None,
                    ridge=1e-6, lambda_threshold=0.1, reduction_effect=0.01, effect_lag=3, wlen=7, generation_period=3, causal=1,
                    time_unit=1.0, device="cuda:0", solver="ridge", normalise=False, tol_scale=1.0, box=None, epsilon=None,
                    kernel_scale=None, svr_tol=1e-3, svr_max_iter=100000):
    """The phase-I predictor of testScripts/test04FullFeatureExtMLpipeline.m (:160-195 the features, :292-404 the linear map,
    :418-431 the policy tracker, :576-642 the clip and the rebuild) for ALL regions and every train / test split:

      cumulative cases, plans --batch.preprocess (W = wlen)--> new_smoothed, ip_filled
      --batch.rt_window--> the growth-rate estimates; `target` picks the regressand (the script: Lambda_LogLinReg, :299)
      --batch.rate_map--> map, lambda_hat, new_cases_est per (train end, region), tracker per region

    cases [T, S] cumulative counts (NaN = missing), population [S], ip [T, n, S] (NaN = N/A).  Give predict_ahead (days, one
    number or a list: numTimeStepsTrain = T - predict_ahead, :293) or n_train (train ends 1 .. T).  extra [T, E, S]: further
    caller-made columns (test05's ones, test01's cumsum columns).
    Returns a dict: new_smoothed, ip_filled, the rt_window outputs, n_train [K], every batch.rate_map output, and the error of
    new_cases_est against new_smoothed over the test days: err [K, T, S] (NaN on the training days), mae and rmse [K, S]
    (NaN for an item without test days or with a failure status).

    solver="backslash" is the predictor of test01FitExponential.m:159, test03ExpfitVsIPRegression.m:169 and
    test05DirectNewCasesLearning.m:185 instead: IPtoRateMap = X(1:train,:) \\ y(1:train) on the raw columns (normalise=True
    divides every column by rate_map's x_mx first), no ridge, by batch.mldivide (tol_scale: its rank tolerance);
    lambda_in = [y(1:n_train); X(n_train+1:T,:) m] then goes through batch.rate_map's clip, rebuild and tracker.  The dict
    gains map [K, F, S] (in the units of the columns used), rank, perm, resid and mldivide_status.

    solver="svr" / "svr_gaussian" are the fitrsvm rows of test05 :198-262, test04 :435-445 and test03 :242-262: batch.svr with
    the linear / the Gaussian kernel on the same feature matrix (normalise as above), box / epsilon / kernel_scale scalars or
    arrays [S], None for _lib.svr_defaults of y_filled(1:max(n_train)); svr_tol and svr_max_iter are its stopping rule.  The
    fitted rates go through the clip and the rebuild like the backslash's.  The dict gains beta [K, T, S], bias, n_iter, gap,
    n_sv and svr_status [K, S], and map [K, F, S] for the linear kernel."""
    if target not in GROWTH_TARGETS:
        raise ValueError(f"target must be one of {GROWTH_TARGETS}")
    if solver not in GROWTH_SOLVERS:
        raise ValueError(f"solver must be one of {GROWTH_SOLVERS}")
    if (predict_ahead is None) == (n_train is None):
        raise ValueError("give predict_ahead or n_train, not both")
    T = np.shape(cases)[0]
    nt = np.atleast_1d(np.asarray(n_train if predict_ahead is None else T - np.atleast_1d(np.asarray(predict_ahead)))).astype(np.int64)
    N = np.asarray(population, dtype=np.float64)
    pre = batch.preprocess(cases, N, ip=ip, W=wlen, min_cases=synth.MIN_CASES, first_num_days=7,
                           outputs=("new_smoothed", "ip_filled"), device=device)
    ns, ipf = pre["new_smoothed"], pre["ip_filled"]
    rw = batch.rt_window(ns, wlen, time_unit, causal, generation_period, ("LogLinReg", "GenRatios", "NonlinLS"), device=device)
    if solver == "ridge":
        rm = batch.rate_map(ipf, ns, nt, y=rw[target], extra=extra, lags=lags, ridge=ridge, lambda_threshold=lambda_threshold,
                            reduction_effect=reduction_effect, effect_lag=effect_lag, device=device)
    else:
        if extra is not None:
            extra = torch.as_tensor(np.ascontiguousarray(extra), dtype=torch.float64).to(ipf.device)
        rm = batch.rate_map(ipf, ns, nt, y=rw[target], extra=extra, lags=lags, reduction_effect=reduction_effect,
                            effect_lag=effect_lag, outputs=("x_mx", "y_filled", "tracker"), device=device)
        X = backslash_features(ipf, lags, extra)
        if normalise:
            X = X / rm["x_mx"][None]
        if solver == "backslash":
            ml = batch.mldivide(X, rm["y_filled"], n_rows=nt, tol_scale=tol_scale, outputs=("m", "rank", "perm", "resid", "fitted", "status"),
                                device=device)
            extras = {"map": ml["m"], "rank": ml["rank"], "perm": ml["perm"], "resid": ml["resid"], "mldivide_status": ml["status"]}
        else:
            kernel = "linear" if solver == "svr" else "gaussian"
            ml = batch.svr(X, rm["y_filled"], n_rows=nt, kernel=kernel, box=box, epsilon=epsilon, kernel_scale=kernel_scale, tol=svr_tol,
                           max_iter=svr_max_iter, device=device)
            extras = {k: ml[k] for k in ("beta", "bias", "n_iter", "gap", "n_sv")}
            extras["svr_status"] = ml["status"]
            if kernel == "linear":
                extras["map"] = ml["w"]
        train = torch.arange(T, device=ipf.device)[None, :, None] < torch.as_tensor(nt, device=ipf.device)[:, None, None]
        lambda_in = torch.where(train, rm["y_filled"][None], ml["fitted"])
        rm.update(batch.rate_map(ipf, ns, nt, lambda_in=lambda_in, lambda_threshold=lambda_threshold, outputs=("lambda_hat", "new_cases_est", "status"),
                                 device=device))
        rm.update(extras)
    out = {"new_smoothed": ns.cpu().numpy(), "ip_filled": ipf.cpu().numpy(), "n_train": nt.astype(np.int32), "target": target}
    out.update({k: v.cpu().numpy() for k, v in rw.items()})
    out.update({k: v.cpu().numpy() for k, v in rm.items()})
    return _forecast_errors(out, nt, T)


def _forecast_errors(out, nt, T):
    """err [K, T, S] (NaN on the training days), mae and rmse [K, S] of out["new_cases_est"] against out["new_smoothed"]"""
    test = np.arange(T)[None, :, None] >= nt[:, None, None]                  # [K, T, 1]
    err = np.where(test, out["new_cases_est"] - out["new_smoothed"][None], np.nan)
    cnt = (T - nt).astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        out["err"] = err
        out["mae"] = np.where(cnt > 0, np.where(test, np.abs(err), 0.0).sum(axis=1) / cnt, np.nan)
        out["rmse"] = np.where(cnt > 0, np.sqrt(np.where(test, err * err, 0.0).sum(axis=1) / cnt), np.nan)
    return out


def growth_forecast_mean(results, lambda_threshold=0.1, device="cuda:0"):
    """The script's LambdaHatTotal = mean([LambdaHatARX; LambdaHatLinear; LambdaHatSVM; LambdaHatSVMGAU]) of
    test05DirectNewCasesLearning.m:268 (test04 :623-624): the mean of the lambda_hat [K, T, S] of several growth_forecast
    results (any solvers; the same cases, plans and n_train), added in the order given and divided by their number, then
    through batch.rate_map's clip and rebuild (fit = 0).  Returns new_smoothed, ip_filled, n_train, lambda_mean (before the
    clip), lambda_hat, new_cases_est, status, err, mae, rmse."""
    results = list(results)
    if not results:
        raise ValueError("no result given")
    first = results[0]
    nt = np.asarray(first["n_train"]).astype(np.int64)
    for res in results[1:]:
        if np.shape(res["lambda_hat"]) != np.shape(first["lambda_hat"]) or not np.array_equal(res["n_train"], first["n_train"]):
            raise ValueError("the results must share their shapes and n_train")
    total = np.array(first["lambda_hat"], dtype=np.float64)
    for res in results[1:]:
        total = total + res["lambda_hat"]
    mean = total / float(len(results))
    rm = batch.rate_map(first["ip_filled"], first["new_smoothed"], nt, lambda_in=mean, lambda_threshold=lambda_threshold,
                        outputs=("lambda_hat", "new_cases_est", "status"), device=device)
    out = {"new_smoothed": np.asarray(first["new_smoothed"]), "ip_filled": np.asarray(first["ip_filled"]), "n_train": nt.astype(np.int32),
           "lambda_mean": mean}
    out.update({k: v.cpu().numpy() for k, v in rm.items()})
    return _forecast_errors(out, nt, mean.shape[1])


def monte_carlo_eks(w, n_regions, q=(0.025, 0.25, 0.5, 0.75, 0.975), population=None, storage="f32", outputs=("S_SMOOTH",),
                    device="cuda:0"):
    """BASELINE config 5 end to end: the Monte-Carlo smoother on a region-major workload (chain = region * n_draws + draw,
    synth.make_cfg5) and, for every output array named in `outputs`, its distribution over the draws of each region
    (batch.ensemble_summary: mean, std, min, max, quantiles at `q`, count per day, row and region).  The chains stay in
    HBM (`storage`: "f32" as config 5 stores them, or "f64"); only the summaries are returned, as device tensors.
    population [n_regions] appends the new-case row ((N * s) * i) * alpha to the summary of a 3-row output.
    Returns {output name: dict of batch.ensemble_summary} and "runner", the EkfRunner that holds the chains."""
    n_regions = int(n_regions)
    if w.B % n_regions:
        raise ValueError("the workload does not hold the same number of draws for every region")
    D = w.B // n_regions
    dw = batch.DeviceWorkload(w, device)
    r = batch.EkfRunner(dw, outputs=list(outputs), storage=storage)
    r.run()
    res = {name: batch.ensemble_summary(r.out[name], n_regions, D, q=q,
                                        population=population if r.out[name].dim() == 3 and r.out[name].shape[1] >= 3 else None)
           for name in outputs}
    res["runner"] = r
    return res


def ar_forecast(cases, deaths, population, ip, horizon=90, ar_order=24, history=120, n_draws=256, plan=None,
                q=(0.025, 0.25, 0.5, 0.75, 0.975), seed=0, regression="nonnegls", nv_mode=0, num_regression_days=60, W=7,
                cv_folds=50, cv_seed=0, device="cuda:0", rng="torch"):
    """The autoregressive alpha forecast of Tools/PrescribeNPI.m:204-241 as a Monte-Carlo fan chart for ALL regions: the front
    half (preprocessing, EKF round 1, regression, round 2, regression), then ar(alpha(end-history+1:end), ar_order) ->
    filtic -> filter over n_draws noise realisations per region -> negatives to 0 -> SI_Controlled from ((N - I0) / N, I0 / N)
    over [segment, forecast] (batch.ar_forecast, one device call), then the distribution over the draws of s, i, alpha_hat and
    the new cases ((N s) i) alpha per day and region (batch.ensemble_summary, one more; nothing is copied back in between).
    The noise is torch.randn on the device from `seed`; with rng="device" it is generated inside the simulation kernel from
    `seed`, no z array exists and the returned z is None.  plan [horizon, n, S] (None = no exogenous term) adds
    gamma * ((u_max - u)' a + b) of the second regression to the continuation before the clamp: the regressor is the one the
    regression was trained on (X = u_max - u), where PrescribeNPI.m:237 multiplies the raw plan.
    Returns the front half's intermediates, seg [history, S], `forecast` (the dict of batch.ar_forecast: S [history + horizon,
    3, S * n_draws], A, noise_var, status), `summary` (the dict of batch.ensemble_summary, rows s, i, alpha_hat, new cases),
    z and drive."""
    T, S = cases.shape
    n = ip.shape[1]
    history, horizon, n_draws = int(history), int(horizon), int(n_draws)
    if history > T:
        raise ValueError("history exceeds the number of days given")
    N = np.asarray(population, dtype=np.float64)
    out = _front_half(cases, deaths, N, ip, num_regression_days, W, device, regression, cv_folds, cv_seed)
    I0, fit2 = out["pre"]["I0"], out["fit2"]
    seg = np.ascontiguousarray(out["alpha_round2"][T - history:])
    dev = torch.device(device)
    z = None
    if not _check_rng(rng):
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        z = torch.randn((horizon, S * n_draws), dtype=torch.float64, device=dev, generator=gen)
    drive = ser = None
    if plan is not None:
        plan = np.asarray(plan, dtype=np.float64)
        if plan.shape != (horizon, n, S):
            raise ValueError("plan must be [horizon, n, S]")
        x = synth.IP_MAXES[:n][None, :, None] - plan
        drive = synth.MODEL_GAMMA * ((x * fit2["a"][None]).sum(axis=1) + fit2["b"][None])          # [horizon, S]
        ser = np.repeat(np.arange(S, dtype=np.int32), n_draws)
    fc = batch.ar_forecast(seg, np.full(S, synth.MODEL_BETA), (N - I0) / N, I0 / N, 1.0, ar_order, horizon, n_draws, z=z,
                           drive=drive, drive_series=ser, nv_mode=nv_mode, device=device, seed=int(seed) if z is None else None)
    summary = batch.ensemble_summary(fc["S"], S, n_draws, q=q, population=N)
    out.update(seg=seg, forecast=fc, summary=summary, z=z, drive=drive)
    return out


def two_filter_smooth(w, form=1, backward="minus", storage="f64", device="cuda:0", lane_block="auto", p_solver=0):
    """The "Backward filtering (under test)" step of Tools/TrainPredictPrescribeNPI.m:464-478 on the device: run the forward
    filter of `w` (a synth.Workload of SIAlphaModelEKF or SIAlphaModelEKFOptControlled), run its reverse-time twin
    (synth.as_backward: the SIAlphaModelBackwardEKF[OptControlled] model with the same fifteen arguments, as the commented
    reference call passes them; the library flips the time axis internally and returns its outputs un-flipped), and fuse the
    two per (chain, day) with batch.two_filter -- from the runners' chain-blocked arrays as they lie, nothing is copied back
    or unblocked in between.
    backward = "minus" (default) fuses forward S_PLUS / P_PLUS with backward S_MINUS / P_MINUS, so that day t's observation is
    counted once; "plus" takes the backward S_PLUS / P_PLUS, the reference's choice.  form = 1 (default) is the information
    form of the two-filter smoother; form = 0 with backward = "plus" is the reference's formula as written (see
    batch.two_filter for why that is not the default).  storage "f32": both runs store float32 and the fusion reads and
    writes float32.
    Returns {"forward": EkfRunner, "backward": EkfRunner, "fused": dict of batch.two_filter (s, P in the runners' layout,
    d2, rank, status), "lane_block": blk, "B": chains}.  No host synchronisation."""
    if backward not in ("minus", "plus"):
        raise ValueError('backward must be "minus" or "plus"')
    if w.model not in ("SIAlphaModelEKF", "SIAlphaModelEKFOptControlled"):
        raise ValueError("w must be a forward workload of the 3- or 6-state SI-alpha model")
    wb = synth.as_backward(w)
    names_f = ["S_PLUS", "P_PLUS"]
    names_b = ["S_MINUS", "P_MINUS"] if backward == "minus" else ["S_PLUS", "P_PLUS"]
    rf = batch.EkfRunner(batch.DeviceWorkload(w, device), names_f, lane_block=lane_block, storage=storage)
    # one layout for both runs: the backward runner takes the forward one's block size
    rb = batch.EkfRunner(batch.DeviceWorkload(wb, device), names_b, lane_block=0 if rf.blk == w.B else rf.blk, storage=storage)
    rf.run()
    rb.run()
    fused = batch.two_filter(rf.out[names_f[0]], rf.out[names_f[1]], rb.out[names_b[0]], rb.out[names_b[1]], form=form,
                             p_solver=p_solver, lane_block=0 if rf.blk == w.B else rf.blk, B=w.B)
    return {"forward": rf, "backward": rb, "fused": fused, "lane_block": rf.blk, "B": w.B}


def filter_likelihood(w, k0=0, k1=None, storage="f64", lane_block="auto", shape=0, device="cuda:0", G=0, outputs=None):
    """Run the filter of `w` (a synth.Workload of any of the six models) and score every chain with
    batch.innovation_likelihood: an EkfRunner with the outputs S_MINUS, P_MINUS, innovations, then the likelihood call on
    runner.out[...] as they lie -- chain-blocked or classic, float64 or float32 (storage "f32"); nothing is unblocked or
    copied back in between.  k0, k1: the window of filter steps that counts (k1 = None: T).  G, outputs: as
    batch.innovation_likelihood.  Returns (runner, dict of device tensors).  No host synchronisation."""
    dw = batch.DeviceWorkload(w, device)
    r = batch.EkfRunner(dw, ["S_MINUS", "P_MINUS", "innovations"], lane_block=lane_block, shape=shape, storage=storage)
    r.run()
    res = batch.innovation_likelihood(r.out["S_MINUS"], r.out["P_MINUS"], r.out["innovations"], dw.x, dw.prm, w.model,
                                      R_series=dw.R_series, R_scalar=dw.R_scalar, x_series=dw.x_series, L=w.L, obs_type=w.obs_type,
                                      k0=k0, k1=k1, lane_block=0 if r.blk == w.B else r.blk, B=w.B, G=G, outputs=outputs)
    return r, res


def likelihood_grid(w, q_scale=(1.0,), r_scale=(1.0,), gamma_ekf=None, beta_ekf=None):
    """The workload of R x G chains, region-major, that runs every chain ("region") of `w` under G candidate noise settings:
    G = the Cartesian product q_scale x r_scale x gamma_ekf x beta_ekf in that order, the last axis fastest.  Q_w is scaled per
    chain by q_scale; R_v by r_scale (R_scalar per chain; R_series -- and x beside it -- once per r_scale value, addressed
    through x_series); the prm rows GAMMA_EKF / BETA_EKF are replaced per chain (None: every region keeps its own, the table
    holds NaN there); u is shared through u_series.  Returns (workload, table [G, 4] of (q_scale, r_scale, gamma_ekf,
    beta_ekf) per candidate)."""
    import itertools
    if np.ndim(w.Q) != 2:
        raise ValueError("likelihood_grid scales a constant Q_w [m*m, B]")
    qs, rs = [float(v) for v in np.atleast_1d(q_scale)], [float(v) for v in np.atleast_1d(r_scale)]
    gs = [np.nan] if gamma_ekf is None else [float(v) for v in np.atleast_1d(gamma_ekf)]
    bs = [np.nan] if beta_ekf is None else [float(v) for v in np.atleast_1d(beta_ekf)]
    combos = list(itertools.product(range(len(qs)), range(len(rs)), range(len(gs)), range(len(bs))))
    G, R = len(combos), w.B
    table = np.array([[qs[a], rs[b], gs[c], bs[d]] for a, b, c, d in combos], dtype=np.float64).reshape(G, 4)
    reg = np.repeat(np.arange(R), G)                      # the region of every chain
    cand = np.tile(np.arange(G), R)
    rep = lambda a: np.ascontiguousarray(a[..., reg])
    prm = rep(w.prm)
    if gamma_ekf is not None:
        prm[L.PRM_GAMMA_EKF] = table[cand, 2]
    if beta_ekf is not None:
        prm[L.PRM_BETA_EKF] = table[cand, 3]
    xs0 = np.arange(R) if w.x_series is None else np.asarray(w.x_series, dtype=np.int64)
    us0 = np.arange(R) if w.u_series is None else np.asarray(w.u_series, dtype=np.int64)
    ri = np.array([b for _, b, _, _ in combos], dtype=np.int64)[cand]      # index into r_scale of every chain
    if w.R_series is not None:
        x = np.ascontiguousarray(np.concatenate([w.x] * len(rs), axis=1))
        R_series = np.ascontiguousarray(np.concatenate([w.R_series * v for v in rs], axis=1))
        x_series, R_scalar = (ri * w.Sx + xs0[reg]).astype(np.int32), None
    else:
        x, R_series = w.x, None
        x_series, R_scalar = xs0[reg].astype(np.int32), np.ascontiguousarray(w.R_scalar[reg] * table[cand, 1])
    gw = synth.Workload(model=w.model, T=w.T, n_npi=w.n_npi, x=x, u=w.u, R_series=R_series, R_scalar=R_scalar, x_series=x_series,
                        u_series=us0[reg].astype(np.int32), prm=prm, s_init=rep(w.s_init), Ps_init=rep(w.Ps_init),
                        s_final=rep(w.s_final), Ps_final=rep(w.Ps_final), Q=np.ascontiguousarray(rep(w.Q) * table[cand, 0]),
                        L=w.L, order=w.order, obs_type=w.obs_type, meta=dict(w.meta))
    return gw, table


def tune_filter(w, q_scale=(1.0,), r_scale=(1.0,), gamma_ekf=None, beta_ekf=None, burn_in=0, storage="f64", lane_block="auto",
                shape=0, device="cuda:0", min_lb_p=None, n_lags=10):
    """Choose the filter's noise settings per region by likelihood: likelihood_grid(w, ...) run as one batch of R x G chains by
    filter_likelihood with k0 = burn_in (the first burn_in filter steps, where Ps_init still dominates, do not count), and per
    region the candidate with the largest log-likelihood.
    What this is: the Gaussian innovation likelihood of the EKF's linearisation, sum over the observed days of
    -1/2 (log S + e^2 / S + log 2 pi) with S the innovation variance the filter itself divided by.  What it is not: with the
    state clamps and a fading memory gamma != 1 the innovations are not those of an exact Gaussian model, so the number is a
    score for comparing candidates of ONE region on the same data and window -- not a calibrated probability, and not
    comparable between regions or windows.
    Returns {"loglik" [R, G], "n_valid" [R, G], "status" [R, G], "best" [R] int32 (-1: no usable candidate), "best_loglik" [R],
    "chosen" [R, 4] (q_scale, r_scale, gamma_ekf, beta_ekf of the best candidate; NaN for best = -1 and for an axis left at
    None), "table" [G, 4], "runner", "workload"}, tensors on the device.  No host synchronisation.
    min_lb_p (None: the above, unchanged): a largest likelihood says nothing about whether the candidate's innovations are
    white.  With a value, every candidate's innovations also go through batch.innovation_diagnostics (n_lags lags, the same
    window) and "best" / "best_loglik" / "chosen" are taken among the usable candidates whose Ljung-Box p-value lb_p >=
    min_lb_p (-1 / NaN where none qualifies); "best_any" [R] keeps the choice by likelihood alone and "lb_p" [R, G] is returned."""
    gw, table = likelihood_grid(w, q_scale, r_scale, gamma_ekf, beta_ekf)
    G, R = table.shape[0], w.B
    if min_lb_p is not None:
        return _tune_filter_white(gw, table, R, burn_in, storage, lane_block, shape, device, float(min_lb_p), n_lags)
    r, res = filter_likelihood(gw, k0=burn_in, storage=storage, lane_block=lane_block, shape=shape, device=device, G=G)
    tab = torch.as_tensor(table, dtype=torch.float64).to(res["best"].device)
    best = res["best"].to(torch.int64)
    chosen = tab[best.clamp(min=0)]
    chosen = torch.where((best < 0)[:, None], torch.full_like(chosen, float("nan")), chosen)
    return {"loglik": res["loglik"].view(R, G), "n_valid": res["n_valid"].view(R, G), "status": res["status"].view(R, G),
            "best": res["best"], "best_loglik": res["best_loglik"], "chosen": chosen, "table": tab, "runner": r, "workload": gw}


def diagnostic_pvalues(stats):
    """The p-values of batch.innovation_diagnostics' statistics under the hypothesis of white Gaussian innovations of unit
    variance, with torch on the tensors' own device (plumbing: not part of the pinned arithmetic of DESIGN.md §4.22):
        lb_p  = P(chi2(lb_lags) >= lb_q) = gammaincc(lb_lags / 2, lb_q / 2)       serial correlation (Ljung-Box)
        jb_p  = P(chi2(2) >= jb) = exp(-jb / 2)                                   normality (Jarque-Bera)
        nis_p = 2 min(P(chi2(n) <= nis_sum), P(chi2(n) >= nis_sum))               the NIS consistency test, two-sided
    NaN where the statistic is NaN or has no degrees of freedom.  het gets none: under the hypothesis it is F(het_n2, het_n1)
    distributed, and torch has no F distribution.  `stats` needs the keys of the p-values wanted; returns a dict of those."""
    out = {}
    nan = float("nan")
    if "lb_q" in stats and "lb_lags" in stats:
        dof = stats["lb_lags"].to(torch.float64)
        p = torch.special.gammaincc(0.5 * dof.clamp(min=1.0), 0.5 * stats["lb_q"])
        out["lb_p"] = torch.where(dof > 0, p, torch.full_like(p, nan))
    if "jb" in stats:
        out["jb_p"] = torch.exp(-0.5 * stats["jb"])
    if "nis_sum" in stats and "n" in stats:
        dof = stats["n"].to(torch.float64)
        a, x = 0.5 * dof.clamp(min=1.0), 0.5 * stats["nis_sum"]
        p = 2.0 * torch.minimum(torch.special.gammainc(a, x), torch.special.gammaincc(a, x))
        out["nis_p"] = torch.where(dof > 0, p, torch.full_like(p, nan))
    return out


def filter_diagnostics(w, n_lags=10, burn_in=0, k1=None, storage="f64", lane_block="auto", shape=0, device="cuda:0", outputs=None):
    """Is the filter run of `w` statistically consistent?  An EkfRunner with the outputs S_MINUS, P_MINUS, innovations, then
    batch.innovation_likelihood for the per-day innovation variance S, then batch.innovation_diagnostics on the innovations and S
    as they lie (chain-blocked or classic, float64 or float32; nothing is unblocked or copied back), over the filter steps
    burn_in <= k < k1 (k1 = None: T).  outputs: as batch.innovation_diagnostics (None: all).  Returns (runner, dict of device
    tensors): the statistics, diagnostic_pvalues' "lb_p", "jb_p", "nis_p" where their statistics were asked for, and the
    likelihood's "loglik".  No host synchronisation."""
    r, lik = filter_likelihood(w, k0=burn_in, k1=k1, storage=storage, lane_block=lane_block, shape=shape, device=device,
                               outputs=("loglik", "S"))
    res = batch.innovation_diagnostics(r.out["innovations"], lik["S"], n_lags=n_lags, k0=burn_in, k1=k1, flip="Backward" in w.model,
                                       lane_block=0 if r.blk == w.B else r.blk, B=w.B, outputs=outputs)
    res.update(diagnostic_pvalues(res))
    res["loglik"] = lik["loglik"]
    return r, res


def _tune_filter_white(gw, table, R, burn_in, storage, lane_block, shape, device, min_lb_p, n_lags):
    """tune_filter with min_lb_p: the grid run once, the likelihood with S, the diagnostics, and the choice among the candidates
    that pass the Ljung-Box test"""
    G = table.shape[0]
    r, res = filter_likelihood(gw, k0=burn_in, storage=storage, lane_block=lane_block, shape=shape, device=device, G=G,
                               outputs=("loglik", "n_valid", "status", "S", "best", "best_loglik"))
    dg = batch.innovation_diagnostics(r.out["innovations"], res["S"], n_lags=n_lags, k0=burn_in, flip="Backward" in gw.model,
                                      lane_block=0 if r.blk == gw.B else r.blk, B=gw.B, outputs=("lb_q", "lb_lags"))
    lb_p = diagnostic_pvalues(dg)["lb_p"].view(R, G)
    ll, nv, st = res["loglik"].view(R, G), res["n_valid"].view(R, G), res["status"].view(R, G)
    ok = ((st & 1) == 0) & (nv > 0) & (lb_p >= min_lb_p) & ~torch.isnan(ll)
    score = torch.where(ok, ll, torch.full_like(ll, float("-inf")))
    best = torch.where(ok.any(dim=1), torch.argmax(score, dim=1), torch.full((R,), -1, dtype=torch.int64, device=ll.device))
    best_ll = torch.where(best >= 0, ll.gather(1, best.clamp(min=0)[:, None])[:, 0], torch.full((R,), float("nan"), dtype=ll.dtype, device=ll.device))
    tab = torch.as_tensor(table, dtype=torch.float64).to(ll.device)
    chosen = tab[best.clamp(min=0)]
    chosen = torch.where((best < 0)[:, None], torch.full_like(chosen, float("nan")), chosen)
    return {"loglik": ll, "n_valid": nv, "status": st, "best": best.to(torch.int32), "best_loglik": best_ll, "chosen": chosen,
            "table": tab, "runner": r, "workload": gw, "best_any": res["best"], "lb_p": lb_p}


def _check_rng(rng, z=None):
    if rng not in ("torch", "device"):
        raise ValueError('rng must be "torch" or "device"')
    if rng == "device" and z is not None:
        raise ValueError('rng="device" and z together: the draws have one source')
    return rng == "device"


def smoothed_fan(w, n_draws, q=(0.025, 0.25, 0.5, 0.75, 0.975), population=None, seed=0, k0=0, storage="f64", clamp=True,
                 device="cuda:0", lane_block="auto", z=None, rng="torch", noise_stream=0, curves=None):
    """The fan chart of the EKF/EKS itself: run the smoother of `w` (a synth.Workload of SIAlphaModelEKF), draw n_draws joint
    posterior paths per chain by backward simulation (batch.smoother_draws on the runner's arrays as they lie; the terminal law is
    the smoothed last day, so s_final / Ps_final of the workload are honoured) and summarise them over the draws of each chain
    (batch.ensemble_summary: mean, std, min, max, quantiles at `q`; population [B] appends the new-case row ((N s) i) alpha).
    The noise is torch.randn on the device from `seed` (or `z` [T - k0, 3, B * n_draws], to repeat a call on given draws); k0 is
    the first day returned.  Nothing is copied back in between.
    rng="device": the noise is generated inside the draw kernel from (`seed`, noise_stream) and no z array
    exists -- the fan's memory halves; the returned z is None, and batch.normal_draws(T - k0, 3, B * n_draws, seed, noise_stream)
    is the array that, passed as z, gives the same bits.  Another generator than torch's: other draws of the same law.
    curves: None (the default: nothing below runs), True or a dict of curve_boxplot's keywords: summary["curves"] is then
    curve_boxplot of the drawn paths (the deepest path, the envelopes of the deepest fractions of the paths, the whiskers).
    Returns (runner, X [T - k0, 3, B * n_draws], the summary dict, z).  No host synchronisation."""
    if w.model != "SIAlphaModelEKF":
        raise ValueError("smoothed_fan needs a workload of the 3-state SIAlphaModelEKF")
    seeded = _check_rng(rng, z)
    n_draws, k0 = int(n_draws), int(k0)
    dev = torch.device(device)
    dw = batch.DeviceWorkload(w, device)
    r = batch.EkfRunner(dw, ["S_PLUS", "P_PLUS", "S_MINUS", "P_MINUS", "S_SMOOTH", "P_SMOOTH"], lane_block=lane_block, storage=storage)
    r.run()
    if z is None and not seeded:
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
        z = torch.randn((w.T - k0, 3, w.B * n_draws), dtype=torch.float64, device=dev, generator=gen)
    blk = 0 if r.blk == w.B else r.blk
    ss, ps = r.out["S_SMOOTH"][-1], r.out["P_SMOOTH"][-1]          # the last day: [3, B] / [9, B], or [nblk, rows, blk]
    if blk:
        ss = ss.permute(1, 0, 2).reshape(3, -1)[:, :w.B]
        ps = ps.permute(1, 0, 2).reshape(9, -1)[:, :w.B]
    res = batch.smoother_draws(r.out["S_PLUS"], r.out["P_PLUS"], r.out["S_MINUS"], r.out["P_MINUS"], dw.prm, n_draws, z=z,
                               s_term=ss.to(torch.float64), P_term=ps.to(torch.float64), k0=k0, clamp=clamp, lane_block=blk, B=w.B,
                               seed=int(seed) if seeded else None, noise_stream=noise_stream if seeded else 0)
    summary = batch.ensemble_summary(res["X"], w.B, n_draws, q=q, population=population)
    summary["rank"], summary["status"] = res["rank"], res["status"]
    if curves is not None and curves is not False:
        summary["curves"] = curve_boxplot(res["X"], w.B, n_draws, population=population, **(curves if isinstance(curves, dict) else {}))
    return r, res["X"], summary, z


def forecast_fan(cases, deaths, population, ip, horizon, n_draws=256, plan=None, q=(0.025, 0.25, 0.5, 0.75, 0.975), seed=0, k0=None,
                 storage="f64", clamp=True, regression="nonnegls", num_regression_days=60, W=7, cv_folds=50, cv_seed=0, device="cuda:0",
                 rng="torch", curves=None):
    """The forecast of Tools/TrainPredictPrescribeNPI.m:356-377 as a fan chart of the smoother's own joint law: the front half
    (preprocessing, EKF round 1, regression, round 2, regression), then the forecast filter -- the observations padded with NaN
    over `horizon` days, R_v padded with its mean (:360), the NPIs of `plan` [horizon, n, S] or, with plan = None, the last day's
    held (the reference's "fixed" forecast, :373-375) -- and smoothed_fan on it.  k0: the first day returned (default: the start
    of the horizon).  rng: smoothed_fan's ("device": no z array, z is None).  Returns the front half's intermediates, `workload` (the forecast filter's), `runner`, X [T + horizon - k0,
    3, S * n_draws], `summary` (rows s, i, alpha, new cases) and z.  curves: smoothed_fan's (None: nothing changes)."""
    T, S = cases.shape
    n = ip.shape[1]
    horizon = int(horizon)
    if horizon < 1:
        raise ValueError("horizon must be >= 1")
    N = np.asarray(population, dtype=np.float64)
    out = _front_half(cases, deaths, N, ip, num_regression_days, W, device, regression, cv_folds, cv_seed)
    pre, fit2 = out["pre"], out["fit2"]
    x, R, u = pre["x_new"], pre["R_v"], pre["ip_filled"]
    if plan is None:
        tail = np.repeat(u[-1:], horizon, axis=0)
    else:
        tail = np.asarray(plan, dtype=np.float64)
        if tail.shape != (horizon, n, S):
            raise ValueError("plan must be [horizon, n, S]")
    xf = np.concatenate([x, np.full((horizon, S), np.nan)])
    Rf = np.concatenate([R, np.repeat(R.mean(axis=0, keepdims=True), horizon, axis=0)])
    uf = np.concatenate([u, tail])
    wf = workload3(xf, Rf, uf, N, pre["I0"], fit2["a"], fit2["b"])
    r, X, summary, z = smoothed_fan(wf, n_draws, q=q, population=N, seed=seed, k0=T if k0 is None else int(k0), storage=storage,
                                    clamp=clamp, device=device, rng=rng, curves=curves)
    out.update(workload=wf, runner=r, X=X, summary=summary, z=z)
    return out


def fan_quality(cases, deaths, population, ip, num_forecast_days, starts, n_draws=256, alpha=(0.5, 0.05), n_bins=10, seed=0,
                storage="f64", clamp=True, num_regression_days=60, W=7, device="cuda:0", regression="nonnegls", cv_folds=50, cv_seed=0,
                z=None, joint=False, vs_p=0.5, max_lag=0, rng="torch"):
    """The look-ahead study of forecast_quality done with fans: instead of one point estimate per day, every forecast is the
    smoother's joint posterior law, scored against the truth by the ensemble CRPS, the weighted interval score, interval coverage
    and the rank histogram (batch.ensemble_score).

    cases / deaths [LL, S], population [S], ip [LL, n, S] over the WHOLE window; the first LL - num_forecast_days days are the
    training window, on which the front half runs exactly as in forecast_quality.  starts: the forecast starts, each in 1 ..
    num_forecast_days; chain c = region * len(starts) + j is region's forecast filter with its last starts[j] observations hidden
    (ForecastQualityAssessment.m:380-393), so its origin -- the first day it has not seen -- is day LL - starts[j].  One 3-state
    filter runs over all chains, smoothed_fan draws n_draws paths per chain from the earliest origin on, and the new-case row
    ((N s) i) alpha of every chain is scored against new_smoothed of the whole window (the truth of forecast_quality) from the
    chain's origin on.  Nothing is copied back between these steps.
    Returns the front half's intermediates, pre_entire, R_full, truth [LL, S], workload (the chains'), runner, X, z, origin [B],
    k0, `scores` (the dict of batch.ensemble_score over the days k0 .. LL-1: rows s, i, alpha carry no truth and are NaN / -1,
    row 3 is the new cases; its per-region outputs are the per-chain aggregates), and by lead time l = day - origin, averaged over
    the starts that reach it, crps_by_lead, wis_by_lead [max(starts), S] and cover_by_lead [n_a, max(starts), S] (torch
    reductions over the per-item scores).
    joint=True adds, from the same paths and origins, `joint_scores`: the dict of batch.ensemble_joint_score
    over the same days, whose row 3 scores every chain's new-case paths as paths from its origin on -- es (the energy score), vs
    (the variogram score of order vs_p over pairs of days at most max_lag apart) and n_days, each [4, B] -- and es, vs, n_days
    [B], that row.  The default returns exactly the keys above.  rng: smoothed_fan's ("device": no z array, z is None)."""
    LL, S = cases.shape
    F = int(num_forecast_days)
    T = LL - F
    if F < 1 or T < 2:
        raise ValueError("num_forecast_days must be >= 1 and leave a training window of at least 2 days")
    st = [int(v) for v in np.atleast_1d(np.asarray(starts))]
    if not st or min(st) < 1 or max(st) > F:
        raise ValueError("starts must hold forecast starts in 1 .. num_forecast_days")
    J, D = len(st), int(n_draws)
    N = np.asarray(population, dtype=np.float64)
    out = _front_half(cases[:T], None if deaths is None else deaths[:T], N, ip[:T], num_regression_days, W, device,
                      regression, cv_folds, cv_seed)
    fit2, I0, R = out["fit2"], out["pre"]["I0"], out["pre"]["R_v"]
    ent = {k: v.cpu().numpy() for k, v in batch.preprocess(cases, N, deaths, ip, W=W, min_cases=synth.MIN_CASES,
                                                            first_num_days=7, device=device).items()}
    R_mean = R.sum(axis=0) / T
    R_full = np.concatenate([R, np.repeat(R_mean[None], F, 0)])
    rr = np.repeat(np.arange(S), J)                        # the region of every chain
    origin = (LL - np.tile(np.asarray(st), S)).astype(np.int32)
    x = ent["x_new"][:, rr].copy()
    x[np.arange(LL)[:, None] >= origin[None, :]] = np.nan  # the last starts[j] observations hidden
    w = workload3(x, R_full[:, rr], ent["ip_filled"][:, :, rr], N[rr], I0[rr], fit2["a"][:, rr], fit2["b"][rr])
    k0 = int(origin.min())
    dev = torch.device(device)
    r, X, _, z = smoothed_fan(w, D, q=(0.5,), population=None, seed=seed, k0=k0, storage=storage, clamp=clamp, device=device, z=z,
                              rng=rng)
    truth = ent["new_smoothed"]
    tw = np.full((LL - k0, 4, S), np.nan)
    tw[:, 3] = truth[k0:]
    fd = torch.as_tensor(origin - k0, device=dev)
    scores = batch.ensemble_score(X, torch.as_tensor(tw, device=dev), S * J, D, alpha=alpha, n_bins=n_bins, population=N[rr],
                                  truth_series=torch.as_tensor(rr.astype(np.int32), device=dev), first_day=fd)
    # by lead time: item (origin_c - k0 + l, row 3, c) of every chain that reaches lead l, averaged over the starts of a region
    H = max(st)
    lead = torch.arange(H, device=dev)[:, None]
    day = fd.to(torch.int64)[None, :] + lead                                   # [H, B]
    reach = day < (LL - k0)
    dayc = day.clamp(max=LL - k0 - 1)
    ok = reach & (scores["rank"][:, 3].gather(0, dayc) >= 0)
    cnt = ok.view(H, S, J).sum(dim=2).to(torch.float64)

    def by_lead(v):                                                              # v [LL - k0, B]
        g = torch.where(ok, v.gather(0, dayc).to(torch.float64), torch.zeros((), dtype=torch.float64, device=dev))
        return g.view(H, S, J).sum(dim=2) / cnt
    n_a = scores["width"].shape[1]
    cover = scores["cover"][:, 3]
    out.update(pre_entire=ent, R_mean=R_mean, R_full=R_full, truth=truth, workload=w, runner=r, X=X, z=z, origin=origin, k0=k0,
               starts=st, scores=scores, crps_by_lead=by_lead(scores["crps"][:, 3]), wis_by_lead=by_lead(scores["wis"][:, 3]),
               cover_by_lead=torch.stack([by_lead((cover >> k) & 1) for k in range(n_a)]) if n_a else
               torch.empty((0, H, S), dtype=torch.float64, device=dev))
    if joint:
        js = batch.ensemble_joint_score(X, torch.as_tensor(tw, device=dev), S * J, D, vs_p=vs_p, max_lag=max_lag, population=N[rr],
                                        truth_series=torch.as_tensor(rr.astype(np.int32), device=dev), first_day=fd,
                                        outputs=("es", "vs", "n_days") if vs_p else ("es", "n_days"))
        out.update(joint_scores=js, es=js["es"][3], n_days=js["n_days"][3], **({"vs": js["vs"][3]} if vs_p else {}))
    return out


OUTLOOK_SUMMARISED = ("peak_value", "peak_day", "total", "days_above", "longest_run")


def path_outlook(X, R, D, thresholds=None, population=None, q=(0.025, 0.25, 0.5, 0.75, 0.975), k0=0, k1=None, first_day=None):
    """What the joint draws were made for: when the peak is, how high, how many cases over the window, and with what probability a
    threshold is exceeded by day t and for how long.  X [T, rows, R * D] are joint paths where they lie (smoothed_fan's or
    forecast_fan's X, monte_carlo_eks', ar_forecast's); batch.path_functionals reads them once, and
    batch.ensemble_summary turns each per-path functional into its law over the D draws of every region: nothing is copied back.
    thresholds [n_thr, rows', R] (NaN: not asked for that row and region; None: no threshold), population [R] appends the new-case
    row, the window is k0 <= t < k1 from first_day[r] on.
    Returns `functionals` (the dict of batch.path_functionals), for each of peak_value, peak_day, total [rows', R] and -- with
    thresholds -- days_above, longest_run [n_thr, rows', R] the dict of batch.ensemble_summary over the draws (mean, std, min, max,
    count: the number of paths that have the functional; quantiles at q [rows', n_q, R] and [n_thr, n_q, rows', R]), p_peak_by_day [W, rows', R] (the probability that the
    peak lies on or before day k0 + w) and p_cross_by_day [W, n_thr, rows', R] (that threshold j has been reached by day k0 + w):
    the cumulative sums of the two histograms over n_paths (torch reductions)."""
    fn = batch.path_functionals(X, R, D, thresholds=thresholds, population=population, first_day=first_day, k0=k0, k1=k1)
    out = {"functionals": fn}
    for k in OUTLOOK_SUMMARISED:
        if k in fn:                                         # [rows', B] is a [T, B] source, [n_thr, rows', B] a [T, rows, B] one
            out[k] = batch.ensemble_summary(fn[k] if fn[k].dim() > 1 else fn[k].unsqueeze(0), R, D, q=q)
    n_paths = fn["n_paths"].to(torch.float64)
    out["p_peak_by_day"] = fn["peak_day_hist"].cumsum(dim=0).to(torch.float64) / n_paths
    if "cross_day_hist" in fn:
        out["p_cross_by_day"] = fn["cross_day_hist"].cumsum(dim=0).to(torch.float64) / n_paths
    return out


def curve_boxplot(X, R, D, alpha=(0.5, 0.9), fence_factor=1.5, fence_frac=0.5, population=None, q=(0.025, 0.25, 0.5, 0.75, 0.975), k0=0,
                  k1=None, first_day=None):
    """The functional boxplot of joint paths where they lie: which path is the typical one and what band the central fractions of
    the PATHS cover -- a band made of curves, which keeps a peak that the members reach on different days, where the per-day
    quantiles of ensemble_summary flatten it.  X [T, rows, R * D] (smoothed_fan's or forecast_fan's X, monte_carlo_eks',
    ar_forecast's); batch.curve_statistics ranks the paths of every (row, region) by modified band depth;
    population [R] appends the new-case row; the window is k0 <= t < k1 from first_day[r] on.
    Returns `statistics` (the dict of batch.curve_statistics), median_curve [T, rows', R] (the deepest path), env_lo, env_hi [T,
    n_alpha, rows', R] (the envelope of the alpha deepest paths), whisk_lo, whisk_hi [T, rows', R] (the envelope of the paths that
    stay inside the fences), n_outliers, n_ranked [rows', R], and `depth`: the dict of batch.ensemble_summary of the depths over
    the draws of every region (quantiles at q [rows', n_q, R]).  Nothing is copied back."""
    st = batch.curve_statistics(X, R, D, alpha=alpha, fence_factor=fence_factor, fence_frac=fence_frac, population=population,
                                first_day=first_day, k0=k0, k1=k1)
    out = {"statistics": st}
    out.update({k: st[k] for k in ("median_curve", "env_lo", "env_hi", "whisk_lo", "whisk_hi", "n_outliers", "n_ranked") if k in st})
    out["depth"] = batch.ensemble_summary(st["depth"] if st["depth"].dim() > 1 else st["depth"].unsqueeze(0), R, D, q=q)
    return out


def forecast_outlook(cases, deaths, population, ip, horizon, thresholds=None, n_draws=256, plan=None, q=(0.025, 0.25, 0.5, 0.75, 0.975),
                     seed=0, storage="f64", clamp=True, regression="nonnegls", num_regression_days=60, W=7, cv_folds=50, cv_seed=0,
                     device="cuda:0", rng="torch", curves=None):
    """forecast_fan, then path_outlook over the horizon: per region the law of the peak day and height of the forecast, of the
    cases over the horizon, and of the days above `thresholds` [n_thr, 4, S] (rows s, i, alpha, new cases; NaN: not asked).
    rng, curves: smoothed_fan's (curves = None: nothing changes).  Returns forecast_fan's dict with `outlook` (path_outlook's; day 0 of its histograms is the first day of the
    horizon)."""
    out = forecast_fan(cases, deaths, population, ip, horizon, n_draws=n_draws, plan=plan, q=q, seed=seed, storage=storage, clamp=clamp,
                       regression=regression, num_regression_days=num_regression_days, W=W, cv_folds=cv_folds, cv_seed=cv_seed,
                       device=device, rng=rng, curves=curves)
    S = cases.shape[1]
    out["outlook"] = path_outlook(out["X"], S, int(n_draws), thresholds, population=np.asarray(population, dtype=np.float64), q=q)
    return out

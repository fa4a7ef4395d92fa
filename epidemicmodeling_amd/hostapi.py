"""NumPy-in / NumPy-out bindings of the HOST-pointer entry points that take a whole stage of
Tools/TrainPredictPrescribeNPI.m for all regions at once -- what a MEX gateway binds (matlab/epiekf_pipeline_mex.cpp).
No torch here: the arrays are plain host memory and the library stages them through the device(s) itself."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _call, _lib
from . import layout as L


class HostBackend:
    """The host entry points' side of a family call (_call): inputs become contiguous NumPy arrays, which it keeps alive,
    outputs are NumPy arrays, the library stages both through device `device` and returns when the results are back."""
    kind, checks_folds = "run_host", False

    def __init__(self, device):
        self.device, self.keep = int(device), []

    def _put(self, v, dtype):
        if v is not None:
            v = np.ascontiguousarray(v, dtype=dtype)
            self.keep.append(v)
        return v

    def f64(self, v):
        return self._put(v, np.float64)

    def i32(self, v):
        return self._put(v, np.int32)

    def f32(self, v):
        return self._put(v, np.float32)

    def empty(self, shape, dtype):
        return np.empty(shape, dtype=dtype)

    def ptr(self, a):
        return None if a is None else a.ctypes.data

    def resident(self, v):
        return False

    def host(self, v):
        return v

    def tail(self):
        return self.device


def _f(a, keep):
    """the flat-argument calls' inputs: the address of `a` as a contiguous float64 array, kept alive in `keep`"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64)
    keep.append(a)
    return a.ctypes.data


def sweep_prescribe(x, u, R_series, region, eps, sp, J0_prefix, J1_prefix, t_hist, L_win=21, order=1, obs_type="NEWCASES",
                    devices=(0,), extras=(), shape=0, time_pipe=0, want_S=True, placement_tries=0):
    """epi_sweep_prescribe_host: the cost-weight sweep of ALL regions (TrainPredictPrescribeNPI.m:421-493, 624-633).

    x, R_series [T, R]; u [T, n, R]; region: dict prm [61, R], s_init [6, R], Ps_init / s_final(6) / Ps_final / Q [36, R];
    eps [P]; sp [48, R]; J0_prefix, J1_prefix [R].  Returns dict J0, J1 [R, P], on_front bool [R, P], i_opt [R] (0-based),
    u_opt [T, n, R], S_opt [T, 6, R] and the per-chain extras named in `extras` ([T, rows, R * P]).
    placement_tries > 1 (epi_prescribe_desc.placement_tries): a call that allocates a new device arena keeps the fastest of that
    many candidates; the report of the first device's block comes back as out["placement"] = {tries, chosen, ms}."""
    keep = []
    T, R = np.shape(x)
    n, P = np.shape(u)[1], len(eps)
    d = _lib.PrescribeDesc()
    d.abi_version, d.R, d.P, d.T, d.t_hist, d.n_npi = _lib.ABI_VERSION, R, P, T, int(t_hist), n
    d.L, d.order, d.obs_type = int(L_win), int(order), L.OBS_IDS.get(obs_type, 99) if isinstance(obs_type, str) else int(obs_type)
    d.shape, d.time_pipe, d.placement_tries = int(shape), int(time_pipe), int(placement_tries)
    ins = _lib.PrescribeInputs()
    ins.x, ins.u, ins.R_series, ins.eps = _f(x, keep), _f(u, keep), _f(R_series, keep), _f(eps, keep)
    for k in ("prm", "s_init", "Ps_init", "s_final", "Ps_final", "Q"):
        setattr(ins, k, _f(region[k], keep))
    ins.sp, ins.J0_prefix, ins.J1_prefix = _f(sp, keep), _f(J0_prefix, keep), _f(J1_prefix, keep)
    out = {"J0": np.empty((R, P)), "J1": np.empty((R, P)), "on_front": np.empty((R, P), dtype=np.int32),
           "i_opt": np.empty((R,), dtype=np.int32), "u_opt": np.empty((T, n, R))}
    if want_S:
        out["S_opt"] = np.empty((T, 6, R))
    outs = _lib.PrescribeOutputs()
    for k in ("J0", "J1", "on_front", "i_opt", "u_opt", "S_opt"):
        setattr(outs, k, out[k].ctypes.data if k in out else None)
    mask = 0
    rows = {"u_opt": n, "u_opt_smooth": n, "S_MINUS": 6, "S_PLUS": 6, "S_SMOOTH": 6, "P_MINUS": 36, "P_PLUS": 36, "P_SMOOTH": 36, "K_GAIN": 6}
    ex = {}
    for name in extras:
        mask |= L.OUT_BITS[name]
        ex[name] = np.empty((T, rows[name], R * P) if name in rows else (T, R * P))
        setattr(outs.extras, name, ex[name].ctypes.data)
    d.out_mask = mask
    rep = _lib.PlacementReport()
    outs.placement = C.addressof(rep)
    ids = (C.c_int * len(devices))(*devices)
    err = C.create_string_buffer(256)
    rc = _lib.lib().epi_sweep_prescribe_host(C.byref(d), C.byref(ins), C.byref(outs), len(devices), ids, err)
    _lib.check(rc, err)
    out["on_front"] = out["on_front"].astype(bool)
    out.update(ex)
    out["placement"] = {"tries": int(rep.tries), "chosen": int(rep.chosen), "ms": [float(rep.ms[i]) for i in range(rep.tries)]}
    return out


def preprocess(cases, population, deaths=None, ip=None, W=7, min_cases=1.0, first_num_days=7, device=0):
    """epi_preprocess_host (TrainPredictPrescribeNPI.m:142-198, 201-202, 240): cases / deaths [T, S], population [S],
    ip [T, n, S].  Returns the dict of batch.preprocess as NumPy arrays."""
    keep = []
    T, S = np.shape(cases)
    d = _lib.PreDesc()
    d.abi_version, d.S, d.T, d.n_npi = _lib.ABI_VERSION, S, T, 0 if ip is None else np.shape(ip)[1]
    d.W, d.first_num_days, d.min_cases = int(W), int(first_num_days), float(min_cases)
    names = [k for k in _lib.PRE_OUT_NAMES if not (k == "fatality" and deaths is None) and not (k == "ip_filled" and ip is None)]
    out = {k: np.empty((S,) if k == "I0" else (np.shape(ip) if k == "ip_filled" else (T, S))) for k in names}
    outs = _lib.PreOutputs()
    for k in _lib.PRE_OUT_NAMES:
        setattr(outs, k, out[k].ctypes.data if k in out else None)
    err = C.create_string_buffer(256)
    rc = _lib.lib().epi_preprocess_host(C.byref(d), _f(cases, keep), _f(deaths, keep), _f(population, keep), _f(ip, keep), C.byref(outs),
                                        int(device), err)
    _lib.check(rc, err)
    return out


def nnls_affine_fit(X, y, max_iters=100, device=0):
    """epi_nnls_affine_fit_host (TrainPredictPrescribeNPI.m:251-276): X [D, n, S], y [D, S] -> dict a [n, S], b, min_err,
    iters, flag [S]."""
    keep = []
    D, n, S = np.shape(X)
    d = _lib.NnlsDesc()
    d.abi_version, d.S, d.D, d.n, d.max_iters = _lib.ABI_VERSION, S, D, n, int(max_iters)
    out = {"a": np.empty((n, S)), "b": np.empty(S), "min_err": np.empty(S), "iters": np.empty(S, dtype=np.int32),
           "flag": np.empty(S, dtype=np.int32)}
    err = C.create_string_buffer(256)
    rc = _lib.lib().epi_nnls_affine_fit_host(C.byref(d), _f(X, keep), _f(y, keep), *(out[k].ctypes.data for k in ("a", "b", "min_err", "iters", "flag")),
                                             int(device), err)
    _lib.check(rc, err)
    return out


def normal_draws(nt, rows, lanes, seed, stream=0, t0=0, lane0=0, dtype=np.float64, device=0):
    """epi_noise_fill_host: batch.normal_draws as a NumPy array [nt, rows, lanes] (synchronous), the same bits"""
    if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError("dtype must be float64 or float32")
    return _call.normal_draws(HostBackend(device), nt, rows, lanes, seed, stream, t0, lane0, np.dtype(dtype) == np.dtype(np.float32))


def random_npi_mc(sp, u_min, n_scen, K, seed=0, z=None, J0_prefix=None, J1_prefix=None, prefix_days=0, store_u=False, device=0,
                  noise_seed=None, noise_stream=0):
    """epi_random_npi_mc_host (TrainPredictPrescribeNPI.m:496-521): sp [48, R], u_min [n, R] -> dict J0, J1 [n_scen, R]
    (+ u [K, n, n_scen * R]).  noise_seed= / noise_stream=: as batch.random_npi_mc (no z is copied)."""
    noise = _lib.noise_of(noise_seed, noise_stream, z)
    keep = []
    n, R = np.shape(u_min)
    d = _lib.McDesc()
    d.abi_version, d.R, d.n_scen, d.K, d.n_npi = _lib.ABI_VERSION, R, int(n_scen), int(K), n
    d.noise, d.prefix_days = int(z is not None), int(prefix_days)
    d.seed_lo, d.seed_hi = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    out = {"J0": np.empty((n_scen, R)), "J1": np.empty((n_scen, R))}
    if store_u:
        out["u"] = np.empty((K, n, n_scen * R))
    err = C.create_string_buffer(256)
    tail = (_f(sp, keep), _f(u_min, keep), _f(z, keep), _f(J0_prefix, keep), _f(J1_prefix, keep),
            out["u"].ctypes.data if store_u else None, out["J0"].ctypes.data, out["J1"].ctypes.data, int(device), err)
    if noise is None:
        rc = _lib.lib().epi_random_npi_mc_host(C.byref(d), *tail)
    else:
        rc = _lib.lib().epi_random_npi_mc_host_seeded(C.byref(d), C.byref(noise), *tail)
    _lib.check(rc, err)
    return out


def sir(alpha, beta, gamma, s0, i0, r0, K, dt, device=0):
    """testScripts/testSIR01.m:15-36 (BASELINE config 1): the 3-compartment SIR with return flow, forward Euler.  Scalars or
    arrays of B parameter sets; returns (s, i, r), each [K, B] (the first sample is the initial state)."""
    prm = np.ascontiguousarray(np.stack(np.broadcast_arrays(*[np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (alpha, beta, gamma, s0, i0, r0)])))
    B = prm.shape[1]
    out = np.empty((int(K), 3, B))
    err = C.create_string_buffer(256)
    rc = _lib.lib().epi_sir_sim_host(B, int(K), float(dt), prm.ctypes.data, out.ctypes.data, int(device), err)
    _lib.check(rc, err)
    return out[:, 0], out[:, 1], out[:, 2]


def rt_window(new_cases, wlen, time_unit=1.0, causal=1, generation_period=None, methods=("LogLinReg", "GenRatios", "NonlinLS"),
              device=0):
    """epi_rtwin_run_host: the three sliding-window growth-rate estimators over new_cases [L, R] (NumPy in and out,
    synchronous).  Returns the dict of batch.rt_window as NumPy arrays."""
    return _call.rt_window(HostBackend(device), new_cases, wlen, time_unit, causal, generation_period, methods)


def lasso_cv(X, y, K=50, folds=None, seed=0, num_lambda=100, lambda_ratio=1e-4, rel_tol=1e-4, max_iter=100000, device=0):
    """epi_lasso_run_host: lasso(X, y, 'CV', K) for every region (NumPy in and out, synchronous).  X [D, n, R], y [D, R],
    folds [D, R] (default batch.lasso_folds(D, K, R, seed)).  Returns the dict of batch.lasso_cv as NumPy arrays."""
    return _call.lasso_cv(HostBackend(device), X, y, K, folds, seed, num_lambda, lambda_ratio, rel_tol, max_iter)


def robust_affine_fit(X, y, robust=True, lower=0.0, upper=float("inf"), max_iter=50, outputs=None, device=0):
    """epi_robfit_run_host: the element-wise robust regression of batch.robust_affine_fit on NumPy arrays (synchronous).
    X [D, n, R], y [D, R].  Returns the dict of batch.robust_affine_fit as NumPy arrays."""
    return _call.robust_affine_fit(HostBackend(device), X, y, robust, lower, upper, max_iter, outputs)


def rate_map(ip, new_smoothed, n_train, y=None, extra=None, lambda_in=None, lags=(3, 5, 7), ridge=1e-6, lambda_threshold=0.1,
             reduction_effect=0.01, effect_lag=3, outputs=None, device=0):
    """epi_ratemap_run_host: the NPI-to-growth-rate predictor of batch.rate_map on NumPy arrays (synchronous).
    ip [T, n, R], new_smoothed [T, R], y [T, R] or lambda_in [K, T, R], extra [T, E, R].  Returns the dict of batch.rate_map
    as NumPy arrays."""
    return _call.rate_map(HostBackend(device), ip, new_smoothed, n_train, y, extra, lambda_in, lags, ridge, lambda_threshold,
                          reduction_effect, effect_lag, outputs)


def mldivide(X, y, n_rows=None, tol_scale=1.0, outputs=None, device=0):
    """epi_mldiv_run_host: MATLAB's rectangular backslash of batch.mldivide on NumPy arrays (synchronous).
    X [D, F, R], y [D, R].  Returns the dict of batch.mldivide as NumPy arrays."""
    return _call.mldivide(HostBackend(device), X, y, n_rows, tol_scale, outputs)


def svr(X, y, n_rows=None, kernel="linear", box=None, epsilon=None, kernel_scale=None, tol=1e-3, max_iter=100000, outputs=None,
        device=0):
    """epi_svr_run_host: the support-vector regression of batch.svr on NumPy arrays (synchronous).
    X [D, F, R], y [D, R]; box, epsilon, kernel_scale scalars or arrays [R], None for _lib.svr_defaults of y(1:max(n_rows)).
    Returns the dict of batch.svr as NumPy arrays."""
    return _call.svr(HostBackend(device), X, y, n_rows, kernel, box, epsilon, kernel_scale, tol, max_iter, outputs)


def ensemble_summary(src, R, D, q=_lib.ENS_DEFAULT_Q, population=None, outputs=None, device=0):
    """epi_ens_run_host: the Monte-Carlo ensemble statistics of batch.ensemble_summary on NumPy arrays (synchronous).
    src [T, rows, B] or [T, B], float32 or float64 (anything else is converted to float64), B = R * D region-major.
    Returns the dict of batch.ensemble_summary as NumPy arrays."""
    src = np.asarray(src)
    if src.dtype not in (np.float32, np.float64):
        src = src.astype(np.float64)
    src = np.ascontiguousarray(src)
    if src.ndim not in (2, 3):
        raise ValueError("src must be [T, rows, B] or [T, B]")
    R, D = int(R), int(D)
    if src.shape[-1] != R * D:
        raise ValueError(f"src holds {src.shape[-1]} chains, R * D = {R * D}")
    T, rows = src.shape[0], (1 if src.ndim == 2 else src.shape[1])
    be = HostBackend(device)
    pop = be.f64(population)
    if pop is not None and pop.shape != (R,):
        raise ValueError("population must be [R]")
    d = _lib.make_ens_desc(T, rows, R, D, q, storage=1 if src.dtype == np.float32 else 0, derive_newcases=int(population is not None))
    names = [k for k in _lib.ENS_OUT_NAMES if k != "count"] if outputs is None else list(outputs)
    bad = [k for k in names if k not in _lib.ENS_OUT_NAMES]
    if bad:
        raise ValueError(f"unknown outputs {bad}")
    shapes = _lib.ens_shapes(T, rows, R, d.n_q, d.derive_newcases)
    out = _call.run_family("ens", be, d, [be.ptr(src), be.ptr(pop)], shapes, names + ["count"])
    if src.ndim == 2:
        out = {k: v.reshape(v.shape[:-2] + v.shape[-1:]) for k, v in out.items()}
    return out


def ar_forecast(seg, beta, s0, i0, dt, p, H, D, z=None, drive=None, drive_series=None, A=None, noise_var=None, nv_mode=0,
                device=0, seed=None, noise_stream=0):
    """epi_arfc_run_host: the autoregressive alpha forecaster of batch.ar_forecast on NumPy arrays (synchronous).
    seg [L, R], beta / s0 / i0 [R], z [H, R * D] or None, drive [H, Sd] or None with drive_series [R * D] or None, A [p, R]
    and noise_var [R] (both or neither).  seed= / noise_stream=: as batch.ar_forecast (no z is copied).  Returns the dict of
    batch.ar_forecast as NumPy arrays."""
    noise = _lib.noise_of(seed, noise_stream, z)
    if (A is None) != (noise_var is None):
        raise ValueError("A and noise_var are given together (the given-model mode) or not at all")
    be = HostBackend(device)
    seg = np.ascontiguousarray(seg, dtype=np.float64)
    if seg.ndim != 2:
        raise ValueError("seg must be [L, R]")
    Ls, R = seg.shape
    p, H, D = int(p), int(H), int(D)
    B = R * D
    for name, v, shape in (("beta", beta, (R,)), ("s0", s0, (R,)), ("i0", i0, (R,)), ("z", z, (H, B)), ("A", A, (p, R)),
                           ("noise_var", noise_var, (R,)), ("drive_series", drive_series, (B,))):
        if v is not None and np.shape(v) != shape:
            raise ValueError(f"{name} must have shape {shape}")
    Sd = 0
    if drive is not None:
        drive = np.ascontiguousarray(drive, dtype=np.float64)
        if drive.ndim != 2 or drive.shape[0] != H:
            raise ValueError("drive must be [H, Sd]")
        Sd = drive.shape[1]
    elif drive_series is not None:
        raise ValueError("drive_series without drive")
    ser = None
    if drive_series is not None:
        ser = np.ascontiguousarray(drive_series, dtype=np.int32)
        if ser.min() < 0 or ser.max() >= Sd:
            raise ValueError("drive_series must hold entries in 0 .. Sd-1")
    d = _lib.make_arfc_desc(R, D, Ls, p, H, dt, fit=int(A is None), nv_mode=nv_mode, Sd=Sd)
    ins = _lib.ArfcInputs()
    for k, v in zip(_lib.ARFC_IN_NAMES, (seg, beta, s0, i0, z, drive, None, A, noise_var)):
        setattr(ins, k, be.ptr(be.f64(v)))
    ins.drive_series = be.ptr(ser)
    out = _call.run_family("arfc", be, d, [C.byref(ins)], _lib.arfc_shapes(R, D, Ls, p, H), _lib.ARFC_OUT_NAMES, noise=noise)
    return {"S": out["S"], "A": out["A_out"], "noise_var": out["noise_var_out"], "status": out["status"]}


def two_filter(sf, Pf, sb, Pb, form=1, p_solver=0, outputs=("s", "P", "d2", "rank", "status"), device=0):
    """epi_fuse_run_host: the forward-backward filter fusion of batch.two_filter on NumPy arrays (synchronous).  sf, sb
    [T, m, B], Pf, Pb [T, m*m, B] (m = 3 or 6; all float32 = float storage, anything else is taken as float64); the arrays
    of a single chain may drop the last axis.  Returns the dict of batch.two_filter as NumPy arrays."""
    dt = np.float32 if all(np.asarray(v).dtype == np.float32 for v in (sf, Pf, sb, Pb)) else np.float64
    arrs = [np.ascontiguousarray(v, dtype=dt) for v in (sf, Pf, sb, Pb)]
    single = arrs[0].ndim == 2
    if single:
        arrs = [v[:, :, None] for v in arrs]
    arrs = [np.ascontiguousarray(v) for v in arrs]
    sf, Pf, sb, Pb = arrs
    if sf.ndim != 3 or Pf.ndim != 3:
        raise ValueError("sf must be [T, m, B] and Pf [T, m*m, B]")
    T, m, B = sf.shape
    if m not in (3, 6) or Pf.shape != (T, m * m, B) or sb.shape != sf.shape or Pb.shape != Pf.shape:
        raise ValueError("m must be 3 or 6, Pf [T, m*m, B], and sb / Pb shaped as sf / Pf")
    for k in outputs:
        if k not in ("s", "P", "d2", "rank", "status"):
            raise ValueError(f"unknown output {k!r}")
    d = _lib.make_fuse_desc(m, B, T, form, p_solver=p_solver, lane_block=0, storage=int(dt == np.float32))
    shapes = _lib.fuse_shapes(m, B, T, 0)
    abi = {"s": "s_out", "P": "P_out", "d2": "d2", "rank": "rank", "status": "status"}
    ins = _lib.FuseInputs()
    for k, v in zip(_lib.FUSE_IN_NAMES, arrs):
        setattr(ins, k, v.ctypes.data)
    out = _call.run_family("fuse", HostBackend(device), d, [C.byref(ins)], shapes, [abi[k] for k in outputs],
                           f32=("s_out", "P_out") if dt == np.float32 else ())
    out = {k: out[abi[k]] for k in outputs}
    if single:
        out = {k: (v if k == "status" else v[..., 0]) for k, v in out.items()}
    return out


def innovation_likelihood(S_MINUS, P_MINUS, innovations, x, prm, model, R_series=None, R_scalar=None, x_series=None, L=21,
                          obs_type="NEWCASES", k0=0, k1=None, lane_block=0, B=None, G=0, outputs=None, device=0):
    """epi_loglik_run_host: batch.innovation_likelihood on NumPy arrays (synchronous): the same arguments, and the same keys,
    order, dtypes and bits.  S_MINUS, P_MINUS, innovations all float32 = float storage, anything else is taken as float64."""
    return _call.innovation_likelihood(HostBackend(device), *(np.asarray(v) for v in (S_MINUS, P_MINUS, innovations)), x, prm,
                                       model, R_series, R_scalar, x_series, L, obs_type, k0, k1, lane_block, B, G, outputs)


def npi_plan(sp, u_min, eps, horizon, u_fixed=None, u_init=None, J0_prefix=None, J1_prefix=None, prefix_days=0, max_iter=64,
             max_halvings=30, tol=1e-9, outputs=None, device=0):
    """epi_plan_run_host: batch.npi_plan on NumPy arrays (synchronous): the same arguments, and the same keys, order, dtypes
    and bits."""
    return _call.npi_plan(HostBackend(device), sp, u_min, eps, horizon, u_fixed, u_init, J0_prefix, J1_prefix, prefix_days, max_iter,
                          max_halvings, tol, outputs)


def smoother_draws(S_PLUS, P_PLUS, S_MINUS, P_MINUS, prm, D, z=None, s_term=None, P_term=None, k0=0, clamp=True, lane_block=0, B=None,
                   out_dtype=None, outputs=("X", "rank", "status"), device=0, seed=None, noise_stream=0):
    """epi_sdraw_run_host: batch.smoother_draws on NumPy arrays (synchronous): the same arguments, and the same keys, order,
    dtypes and bits.  The four filter arrays all float32 = float storage, anything else is taken as float64; z float32 or
    float64; out_dtype np.float64 (default) or np.float32.  seed= / noise_stream=: no z is made or copied."""
    z = None if z is None else np.asarray(z)
    return _call.smoother_draws(HostBackend(device), *(np.asarray(v) for v in (S_PLUS, P_PLUS, S_MINUS, P_MINUS)), prm, D, z, s_term,
                                P_term, k0, clamp, lane_block, B, None if out_dtype is None else np.dtype(out_dtype), outputs, 0, seed,
                                noise_stream)


def ensemble_score(src, truth, R, D, alpha=_lib.ESCORE_DEFAULT_ALPHA, n_bins=0, population=None, truth_series=None, first_day=None,
                   k0=0, k1=None, outputs=None, device=0, test_launch_items=0):
    """epi_escore_run_host: batch.ensemble_score on NumPy arrays (synchronous): the same arguments, and the same keys, order,
    dtypes and bits.  A float32 src = float storage, anything else is taken as float64."""
    src = np.asarray(src)
    if src.ndim == 4:
        raise ValueError("src is a chain-blocked array [T, nblk, rows, blk]; ensemble_score takes the classic layout [T, rows, B]")
    src = np.ascontiguousarray(src, dtype=np.float32 if src.dtype == np.float32 else np.float64)
    return _call.ensemble_score(HostBackend(device), src, truth, R, D, alpha, n_bins, population, truth_series, first_day, k0, k1,
                                outputs, test_launch_items)


def path_functionals(src, R, D, thresholds=None, population=None, first_day=None, k0=0, k1=None, outputs=None, device=0,
                     test_segments=0, test_launch_groups=0):
    """epi_pathfn_run_host: batch.path_functionals on NumPy arrays (synchronous): the same arguments, and the same keys, order,
    dtypes and bits.  A float32 src = float storage, anything else is taken as float64."""
    src = np.asarray(src)
    if src.ndim == 4:
        raise ValueError("src is a chain-blocked array [T, nblk, rows, blk]; path_functionals takes the classic layout [T, rows, B]")
    src = np.ascontiguousarray(src, dtype=np.float32 if src.dtype == np.float32 else np.float64)
    return _call.path_functionals(HostBackend(device), src, R, D, thresholds, population, first_day, k0, k1, outputs,
                                  test_segments, test_launch_groups)


def curve_statistics(src, R, D, alpha=_lib.CDEPTH_DEFAULT_ALPHA, fence_factor=_lib.CDEPTH_DEFAULT_FENCE_FACTOR,
                     fence_frac=_lib.CDEPTH_DEFAULT_FENCE_FRAC, population=None, first_day=None, k0=0, k1=None, outputs=None, device=0,
                     test_segments=0, test_launch_groups=0):
    """epi_cdepth_run_host: batch.curve_statistics on NumPy arrays (synchronous): the same arguments, and the same keys, order,
    dtypes and bits.  A float32 src = float storage, anything else is taken as float64."""
    src = np.asarray(src)
    if src.ndim == 4:
        raise ValueError("src is a chain-blocked array [T, nblk, rows, blk]; ensemble_summary takes the classic layout [T, rows, B]")
    src = np.ascontiguousarray(src, dtype=np.float32 if src.dtype == np.float32 else np.float64)
    return _call.curve_statistics(HostBackend(device), src, R, D, alpha, fence_factor, fence_frac, population, first_day, k0, k1,
                                  outputs, test_segments, test_launch_groups)


def ensemble_joint_score(src, truth, R, D, vs_p=None, max_lag=0, population=None, truth_series=None, first_day=None, k0=0, k1=None,
                         outputs=None, device=0, test_launch_tiles=0):
    """epi_ejoint_run_host: batch.ensemble_joint_score on NumPy arrays (synchronous): the same arguments, and the same keys, order,
    dtypes and bits.  A float32 src = float storage, anything else is taken as float64."""
    src = np.asarray(src)
    if src.ndim == 4:
        raise ValueError("src is a chain-blocked array [T, nblk, rows, blk]; ensemble_score takes the classic layout [T, rows, B]")
    src = np.ascontiguousarray(src, dtype=np.float32 if src.dtype == np.float32 else np.float64)
    return _call.ensemble_joint_score(HostBackend(device), src, truth, R, D, vs_p, max_lag, population, truth_series, first_day, k0, k1,
                                      outputs, test_launch_tiles)


def innovation_diagnostics(innovations, S=None, n_lags=10, k0=0, k1=None, flip=False, lane_block=0, B=None, outputs=None, device=0):
    """epi_idiag_run_host: batch.innovation_diagnostics on NumPy arrays (synchronous): the same arguments, and the same keys,
    order, dtypes and bits.  float32 innovations = float storage, anything else is taken as float64."""
    return _call.innovation_diagnostics(HostBackend(device), np.asarray(innovations), None if S is None else np.asarray(S), n_lags,
                                        k0, k1, flip, lane_block, B, outputs)

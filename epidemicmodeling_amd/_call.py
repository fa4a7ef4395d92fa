"""The one call path of the batched family calls (_lib.FAMILIES), shared by batch (torch tensors on a stream) and hostapi
(NumPy arrays, a device ordinal).  No torch here: what differs between the two entry points is asked of a backend,

    f64(v) / i32(v) / f32(v)
                       the input as a contiguous float64 / int32 / float32 array where the call reads it (None stays None); the
                       backend keeps it alive
    empty(shape, dt)   an uninitialised output, dt one of np.float64 / np.int32 / np.float32
    ptr(a)             the address of such an array (None stays None)
    kind, tail()       "run_device" and the stream, or "run_host" and the device ordinal
    resident(v)        v already lies where the call reads it (a torch tensor for the device entry; never for the host's)
    host(v)            v as something NumPy reads
    checks_folds       lasso_cv checks a host-side partition before the call

batch.DeviceBackend and hostapi.HostBackend.  Every family's call ends in run_family; the six families whose two entry
points are the same function have their body here, written against a backend."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import layout as L


def run_family(fam, be, desc, args, shapes, names, f32=(), noise=None):
    """Allocate the outputs `names` of family `fam` (a key of _lib.FAMILIES) from `shapes` -- int32 where the family says so,
    float32 for those in `f32`, else float64 --, bind them (the others stay NULL), call epi_<fam>_<be.kind>(desc, *args,
    outputs, be.tail(), err) and check its status.  Returns the dict of outputs in the order of the family's names.  noise: a
    _lib.NoiseDesc, for the seeded sibling epi_<fam>_<be.kind>_seeded(desc, noise, ...)."""
    f = _lib.FAMILIES[fam]
    out = {k: be.empty(shapes[k], np.int32 if k in f.out_i32 else (np.float32 if k in f32 else np.float64))
           for k in f.out_names if k in names}
    outs = f.args[-1]._type_()                      # the family's outputs structure
    for k, v in out.items():
        setattr(outs, k, be.ptr(v))
    err = C.create_string_buffer(256)
    if noise is None:
        rc = getattr(_lib.lib(), f"epi_{fam}_{be.kind}")(C.byref(desc), *args, C.byref(outs), be.tail(), err)
    else:
        rc = getattr(_lib.lib(), f"epi_{fam}_{be.kind}_seeded")(C.byref(desc), C.byref(noise), *args, C.byref(outs), be.tail(), err)
    _lib.check(rc, err)
    return out


def normal_draws(be, nt, rows, lanes, seed, stream=0, t0=0, lane0=0, f32=False, test_launch_groups=0):
    """The window [t0, t0 + nt) x rows x [lane0, lane0 + lanes) of the seeded standard-normal array (epi_noise_fill_*, DESIGN.md
    §4.21) as the backend's array [nt, rows, lanes], float64 or float32"""
    nt, rows, lanes = int(nt), int(rows), int(lanes)
    if rows not in (1, 3):
        raise ValueError("rows must be 1 or 3")
    if nt < 1 or lanes < 1:
        raise ValueError("nt and lanes must be >= 1")
    d = _lib.make_noise_desc(seed, stream)
    args = (C.byref(d), int(t0), nt, rows, int(lane0), lanes, int(bool(f32)))
    err = C.create_string_buffer(256)
    h = _lib.lib()
    out = be.empty((nt, rows, lanes), np.float32 if f32 else np.float64)
    if be.kind == "run_device":
        rc = h.epi_noise_fill_device(*args, be.ptr(out), int(test_launch_groups), be.tail(), err)
    else:
        rc = h.epi_noise_fill_host(*args, be.ptr(out), be.tail(), err)
    _lib.check(rc, err)
    return out


def _rtwin_names(methods, status=True):
    bits = _lib.rtwin_methods(methods)
    names = []
    if bits & 1:
        names += [n for n in _lib.RTWIN_OUT_F64 if n.startswith("llr_")]
    if bits & 2:
        names += [n for n in _lib.RTWIN_OUT_F64 if n.startswith("gr_")]
    if bits & 4:
        names += [n for n in _lib.RTWIN_OUT_F64 if n.startswith("nls_")] + (list(_lib.RTWIN_OUT_I32) if status else [])
    return bits, names


def rt_window(be, new_cases, wlen, time_unit, causal, generation_period, methods):
    x = be.f64(new_cases)
    if x.ndim != 2:
        raise ValueError("new_cases must be [L, R]")
    L_, R = x.shape
    bits, names = _rtwin_names(methods)
    d = _lib.make_rtwin_desc(R, L_, wlen, time_unit, causal, generation_period, bits)
    return run_family("rtwin", be, d, [be.ptr(x)], dict.fromkeys(names, (L_, R)), names)


def lasso_folds(D, K, R, seed=0):
    """A cross-validation partition for lasso_cv: fold [D, R] int32 in 0 .. K-1.  Every region gets its own random
    permutation of the D days (np.random.default_rng(seed), regions in order); the fold sizes are those of cvpartition's
    KFold: the first D mod K folds get ceil(D / K) days, the rest floor(D / K).  Deterministic for a given seed."""
    D, K, R = int(D), int(K), int(R)
    if not 2 <= K <= D:
        raise ValueError("lasso_folds needs 2 <= K <= D")
    rng = np.random.default_rng(seed)
    sizes = np.full(K, D // K)
    sizes[:D % K] += 1
    label = np.repeat(np.arange(K, dtype=np.int32), sizes)
    fold = np.empty((D, R), dtype=np.int32)
    for r in range(R):
        fold[rng.permutation(D), r] = label
    return fold


def check_lasso_folds(fold, K):
    """ValueError unless fold [D, R] holds only 0 .. K-1 and leaves no fold empty in any region"""
    f = np.asarray(fold)
    if f.ndim != 2 or f.min() < 0 or f.max() >= K:
        raise ValueError("folds must be [D, R] with values in 0 .. K-1")
    for r in range(f.shape[1]):
        if np.bincount(f[:, r], minlength=K).min() == 0:
            raise ValueError(f"region {r}: a fold is empty")


def lasso_cv(be, X, y, K, folds, seed, num_lambda, lambda_ratio, rel_tol, max_iter):
    X, y = be.f64(X), be.f64(y)
    if X.ndim != 3 or y.ndim != 2 or y.shape != (X.shape[0], X.shape[2]):
        raise ValueError("X must be [D, n, R] and y [D, R]")
    D, n, R = X.shape
    K = int(K)
    f = None
    if K >= 2:
        if folds is None:
            folds = lasso_folds(D, K, R, seed)
        if be.checks_folds and not be.resident(folds):
            check_lasso_folds(folds, K)
        f = be.i32(folds)
    d = _lib.make_lasso_desc(R, D, n, K, num_lambda, lambda_ratio, rel_tol, max_iter)
    shapes = _lib.lasso_shapes(R, D, n, K, num_lambda)
    out = run_family("lasso", be, d, [be.ptr(X), be.ptr(y), be.ptr(f)], shapes, shapes)
    return {k: out[k] for k in shapes}              # the path's outputs first, the cross-validation's behind them


def robust_affine_fit(be, X, y, robust, lower, upper, max_iter, outputs):
    X, y = be.f64(X), be.f64(y)
    if X.ndim != 3 or y.ndim != 2 or y.shape != (X.shape[0], X.shape[2]):
        raise ValueError("X must be [D, n, R] and y [D, R]")
    D, n, R = X.shape
    names = _lib.robfit_out_names(outputs)
    d = _lib.make_robfit_desc(R, D, n, int(bool(robust)), max_iter, lower, upper)
    return run_family("robfit", be, d, [be.ptr(X), be.ptr(y)], _lib.robfit_shapes(R, D, n), names)


def rate_map(be, ip, new_smoothed, n_train, y, extra, lambda_in, lags, ridge, lambda_threshold, reduction_effect, effect_lag,
             outputs):
    ip, ns, y, extra, lambda_in = be.f64(ip), be.f64(new_smoothed), be.f64(y), be.f64(extra), be.f64(lambda_in)
    if ip.ndim != 3 or ns.ndim != 2 or ns.shape != (ip.shape[0], ip.shape[2]):
        raise ValueError("ip must be [T, n, R] and new_smoothed [T, R]")
    T, n, R = ip.shape
    nt = _lib.ratemap_n_train(n_train)
    K = int(nt.size)
    fit = lambda_in is None
    if fit and y is None:
        raise ValueError("y (to fit) or lambda_in (to skip the fit) is needed")
    if (y is not None and y.shape != (T, R)) or (extra is not None and (extra.ndim != 3 or extra.shape[0] != T or extra.shape[2] != R)) \
            or (lambda_in is not None and lambda_in.shape != (K, T, R)):
        raise ValueError("y must be [T, R], extra [T, E, R] and lambda_in [K, T, R]")
    E = 0 if extra is None else int(extra.shape[1])
    names = _lib.ratemap_out_names(outputs, fit, y is not None)
    d = _lib.make_ratemap_desc(T, n, R, E, K, lags, int(fit), effect_lag, ridge, lambda_threshold, reduction_effect)
    ins = _lib.RatemapInputs()
    ins.ip, ins.y, ins.new_smoothed, ins.extra, ins.lambda_in = be.ptr(ip), be.ptr(y), be.ptr(ns), be.ptr(extra), be.ptr(lambda_in)
    ins.n_train = nt.ctypes.data
    return run_family("ratemap", be, d, [C.byref(ins)], _lib.ratemap_shapes(T, n, R, E, K, d.n_lags), names)


def mldivide(be, X, y, n_rows, tol_scale, outputs):
    X, y = be.f64(X), be.f64(y)
    if X.ndim != 3 or y.ndim != 2 or y.shape != (X.shape[0], X.shape[2]):
        raise ValueError("X must be [D, F, R] and y [D, R]")
    D, F, R = X.shape
    nr = _lib.mldiv_n_rows(n_rows, D)
    K = int(nr.size)
    names = _lib.mldiv_out_names(outputs)
    d = _lib.make_mldiv_desc(D, F, R, K, tol_scale)
    ins = _lib.MldivInputs()
    ins.X, ins.y, ins.n_rows = be.ptr(X), be.ptr(y), nr.ctypes.data
    return run_family("mldiv", be, d, [C.byref(ins)], _lib.mldiv_shapes(D, F, R, K), names)


def svr(be, X, y, n_rows, kernel, box, epsilon, kernel_scale, tol, max_iter, outputs):
    X, y = be.f64(X), be.f64(y)
    if X.ndim != 3 or y.ndim != 2 or y.shape != (X.shape[0], X.shape[2]):
        raise ValueError("X must be [D, F, R] and y [D, R]")
    D, F, R = X.shape
    nr = _lib.mldiv_n_rows(n_rows, D)
    K = int(nr.size)
    names = _lib.svr_out_names(outputs, kernel)
    d = _lib.make_svr_desc(D, F, R, K, kernel, tol, max_iter)
    if box is None or epsilon is None or kernel_scale is None:
        dflt = _lib.svr_defaults(be.host(y[:max(1, min(int(nr.max()), D))]), kernel)
        box, epsilon = dflt["box"] if box is None else box, dflt["epsilon"] if epsilon is None else epsilon
        kernel_scale = dflt["kernel_scale"] if kernel_scale is None else kernel_scale

    def reg(v, name):                               # an array [R] that is already resident is taken as it is
        return be.f64(v if be.resident(v) and v.shape == (R,) else _lib.svr_region_array(be.host(v), R, name))

    ins = _lib.SvrInputs()
    ins.X, ins.y, ins.n_rows = be.ptr(X), be.ptr(y), nr.ctypes.data
    ins.box, ins.epsilon, ins.kernel_scale = be.ptr(reg(box, "box")), be.ptr(reg(epsilon, "epsilon")), be.ptr(reg(kernel_scale, "kernel_scale"))
    return run_family("svr", be, d, [C.byref(ins)], _lib.svr_shapes(D, F, R, K), names)


def run_with_workspace(prefix, be, desc, ins, outs, out_names, out_i32, shapes, names, out_f32=(), noise=None):
    """The call helper of the calls whose device entry takes a workspace (epi_<prefix>_workspace_bytes / _run_device /
    _run_host), which are no families: allocate the outputs `names`, and for the device entry the workspace, through the
    backend; bind them into the outputs structure `outs`, call and check the status.  Returns the dict of outputs in the ABI's
    order.  out_f32: the outputs the descriptor asks for as float32.  noise: a _lib.NoiseDesc, for the seeded siblings
    epi_<prefix>_run_device_seeded / _run_host_seeded(desc, noise, ...)."""
    h = _lib.lib()
    out = {k: be.empty(shapes[k], np.int32 if k in out_i32 else (np.float32 if k in out_f32 else np.float64))
           for k in out_names if k in names}
    for k, v in out.items():
        setattr(outs, k, be.ptr(v))
    err = C.create_string_buffer(256)
    if be.kind == "run_device":
        n = C.c_size_t(0)
        _lib.check(getattr(h, f"epi_{prefix}_workspace_bytes")(C.byref(desc), C.byref(n), err), err)
        ws = be.empty(((max(n.value, 8) + 7) // 8,), np.float64)
        tail = (C.byref(ins), C.byref(outs), be.ptr(ws), n.value, be.tail(), err)
    else:
        tail = (C.byref(ins), C.byref(outs), be.tail(), err)
    if noise is None:
        rc = getattr(h, f"epi_{prefix}_{be.kind}")(C.byref(desc), *tail)
    else:
        rc = getattr(h, f"epi_{prefix}_{be.kind}_seeded")(C.byref(desc), C.byref(noise), *tail)
    _lib.check(rc, err)
    return out


def run_loglik(be, desc, ins, shapes, names):
    """The innovation likelihood's call: run_with_workspace with its names"""
    return run_with_workspace("loglik", be, desc, ins, _lib.LoglikOutputs(), _lib.LOGLIK_OUT_NAMES, _lib.LOGLIK_OUT_I32, shapes, names)


def innovation_likelihood(be, S_MINUS, P_MINUS, innovations, x, prm, model, R_series, R_scalar, x_series, L_, obs_type, k0, k1,
                          lane_block, B, G, outputs):
    f32 = all(str(v.dtype).endswith("float32") for v in (S_MINUS, P_MINUS, innovations))
    put = be.f32 if f32 else be.f64
    sm, pm, inn = put(S_MINUS), put(P_MINUS), put(innovations)
    if model not in L.MODEL_DIM:
        raise ValueError(f"unknown model {model!r}")
    m, blk = L.MODEL_DIM[model], int(lane_block)
    if sm.ndim == 3 and pm.ndim == 3:
        T, rows, nB = sm.shape
        if 0 < blk < nB:
            raise ValueError("lane_block given with classic [T, rows, B] arrays")
        if B is not None and int(B) != nB:
            raise ValueError("B does not match the arrays")
        B, blk, Bp = nB, 0, nB
    elif sm.ndim == 4 and pm.ndim == 4:
        T, nblk, rows, bl = sm.shape
        if bl != blk:
            raise ValueError("chain-blocked arrays [T, nblk, rows, blk] need lane_block = blk")
        B = nblk * blk if B is None else int(B)
        if nblk != (B + blk - 1) // blk or blk >= B:
            raise ValueError("B does not match nblk blocks of lane_block chains")
        Bp = nblk * blk
    else:
        raise ValueError("S_MINUS / P_MINUS must be [T, m, B] / [T, m*m, B] or [T, nblk, m, blk] / [T, nblk, m*m, blk]")
    if rows != m or tuple(pm.shape) != tuple(sm.shape[:-2]) + (m * m, sm.shape[-1]):
        raise ValueError(f"{model} has m = {m}: S_MINUS must hold m rows and P_MINUS m*m")
    if tuple(inn.shape) != (T, Bp):
        raise ValueError("innovations must be [T, B] ([T, nblk * blk] for chain-blocked arrays)")
    x, prm = be.f64(x), be.f64(prm)
    if x.ndim != 2 or x.shape[0] != T:
        raise ValueError("x must be [T, Sx]")
    Sx = int(x.shape[1])
    if tuple(prm.shape) != (L.PRM_COUNT, B):
        raise ValueError("prm must be [PRM_COUNT, B]")
    if (R_series is None) == (R_scalar is None):
        raise ValueError("exactly one of R_series / R_scalar is needed")
    R_series, R_scalar, x_series = be.f64(R_series), be.f64(R_scalar), be.i32(x_series)
    if R_series is not None and tuple(R_series.shape) != (T, Sx):
        raise ValueError("R_series must be [T, Sx]")
    if R_scalar is not None and tuple(R_scalar.shape) != (B,):
        raise ValueError("R_scalar must be [B]")
    if x_series is not None and tuple(x_series.shape) != (B,):
        raise ValueError("x_series must be [B]")
    if x_series is None and Sx != B:
        raise ValueError("without x_series, x must be [T, B]")
    names = _lib.loglik_out_names(outputs, G)
    d = _lib.make_loglik_desc(model, B, T, L_, obs_type, int(R_series is not None), Sx, blk, int(f32), k0, k1, G)
    err = C.create_string_buffer(256)
    _lib.check(_lib.lib().epi_loglik_validate(C.byref(d), err), err)      # before anything is allocated from G
    ins = _lib.LoglikInputs()
    for k, v in zip(_lib.LOGLIK_IN_NAMES, (sm, pm, inn, x, R_series, R_scalar, x_series, prm)):
        setattr(ins, k, be.ptr(v))
    return run_loglik(be, d, ins, _lib.loglik_shapes(B, T, G), names)


def npi_plan(be, sp, u_min, eps, horizon, u_fixed, u_init, J0_prefix, J1_prefix, prefix_days, max_iter, max_halvings, tol, outputs):
    sp, u_min, eps = be.f64(sp), be.f64(u_min), be.f64(eps)
    if sp.ndim != 2 or sp.shape[0] != _lib.PLAN_SIM_PRM_COUNT:
        raise ValueError("sp must be [48, R] (pipeline.scoring_region_inputs)")
    R = int(sp.shape[1])
    if u_min.ndim != 2 or u_min.shape[1] != R:
        raise ValueError("u_min must be [n, R]")
    if eps.ndim != 1:
        raise ValueError("eps must be [P]")
    n, P, H = int(u_min.shape[0]), int(eps.shape[0]), int(horizon)
    u_fixed, u_init, J0_prefix, J1_prefix = be.f64(u_fixed), be.f64(u_init), be.f64(J0_prefix), be.f64(J1_prefix)
    if u_fixed is not None and tuple(u_fixed.shape) != (H, n, R):
        raise ValueError("u_fixed must be [H, n, R]")
    if u_init is not None and tuple(u_init.shape) != (H, n, R * P):
        raise ValueError("u_init must be [H, n, R * P]")
    if int(prefix_days) > 0 and (J0_prefix is None or J1_prefix is None):
        raise ValueError("prefix_days > 0 needs J0_prefix and J1_prefix")
    for v in (J0_prefix, J1_prefix):
        if v is not None and tuple(v.shape) != (R,):
            raise ValueError("J0_prefix / J1_prefix must be [R]")
    names = _lib.plan_out_names(outputs)
    d = _lib.make_plan_desc(R, P, H, n, prefix_days, max_iter, max_halvings, tol)
    err = C.create_string_buffer(256)
    _lib.check(_lib.lib().epi_plan_validate(C.byref(d), err), err)        # before anything is allocated from the sizes
    ins = _lib.PlanInputs()
    for k, v in zip(_lib.PLAN_IN_NAMES, (sp, u_min, eps, u_fixed, u_init, J0_prefix, J1_prefix)):
        setattr(ins, k, be.ptr(v))
    return run_with_workspace("plan", be, d, ins, _lib.PlanOutputs(), _lib.PLAN_OUT_NAMES, _lib.PLAN_OUT_I32,
                              _lib.plan_shapes(R, P, H, n, max_iter), names)


def _is_f32(v):
    return str(v.dtype).endswith("float32")


def smoother_draws(be, S_PLUS, P_PLUS, S_MINUS, P_MINUS, prm, D, z, s_term, P_term, k0, clamp, lane_block, B, out_dtype, outputs,
                   test_launch_groups=0, seed=None, stream=0):
    noise = _lib.noise_of(seed, stream, z)
    big = (S_PLUS, P_PLUS, S_MINUS, P_MINUS)
    f32 = all(_is_f32(v) for v in big)
    put = be.f32 if f32 else be.f64
    sp, pp, sm, pm = (put(v) for v in big)
    blk = int(lane_block)
    if all(v.ndim == 3 for v in (sp, pp, sm, pm)):
        T, rows, nB = sp.shape
        if 0 < blk < nB:
            raise ValueError("lane_block given with classic [T, rows, B] arrays")
        if B is not None and int(B) != nB:
            raise ValueError("B does not match the arrays")
        B, blk = nB, 0
    elif all(v.ndim == 4 for v in (sp, pp, sm, pm)):
        T, nblk, rows, bl = sp.shape
        if bl != blk:
            raise ValueError("chain-blocked arrays [T, nblk, rows, blk] need lane_block = blk")
        B = nblk * blk if B is None else int(B)
        if nblk != (B + blk - 1) // blk or blk >= B:
            raise ValueError("B does not match nblk blocks of lane_block chains")
    else:
        raise ValueError("S_PLUS / P_PLUS / S_MINUS / P_MINUS must be [T, rows, B] or [T, nblk, rows, blk]")
    if rows != 3 or tuple(sm.shape) != tuple(sp.shape) or tuple(pp.shape) != tuple(sp.shape[:-2]) + (9, sp.shape[-1]) \
            or tuple(pm.shape) != tuple(pp.shape):
        raise ValueError("smoother draws need the 3-state model: S_PLUS, S_MINUS must hold 3 rows and P_PLUS, P_MINUS 9")
    prm = be.f64(prm)
    if tuple(prm.shape) != (L.PRM_COUNT, B):
        raise ValueError("prm must be [PRM_COUNT, B]")
    T, D, k0 = int(T), int(D), int(k0)
    z_f32 = z is not None and _is_f32(z)
    if out_dtype is None:
        out_f32 = False
    elif str(out_dtype).endswith("float32"):
        out_f32 = True
    elif str(out_dtype).endswith("float64"):
        out_f32 = False
    else:
        raise ValueError("out_dtype must be float64 or float32")
    d = _lib.make_sdraw_desc(B, T, D, k0, clamp, blk, int(f32), int(z_f32), int(out_f32), test_launch_groups=test_launch_groups)
    err = C.create_string_buffer(256)
    _lib.check(_lib.lib().epi_sdraw_validate(C.byref(d), err), err)       # before anything is allocated from the sizes
    if z is not None:
        z = be.f32(z) if z_f32 else be.f64(z)
        if tuple(z.shape) != (T - k0, 3, B * D):
            raise ValueError("z must be [T - k0, 3, B * D]")
    s_term, P_term = be.f64(s_term), be.f64(P_term)
    if s_term is not None and tuple(s_term.shape) != (3, B):
        raise ValueError("s_term must be [3, B]")
    if P_term is not None and tuple(P_term.shape) != (9, B):
        raise ValueError("P_term must be [9, B]")
    names = _lib.out_names(_lib.SDRAW_OUT_NAMES, outputs, _lib.SDRAW_DEFAULT)
    ins = _lib.SdrawInputs()
    for k, v in zip(_lib.SDRAW_IN_NAMES, (sp, pp, sm, pm, prm, z, s_term, P_term)):
        setattr(ins, k, be.ptr(v))
    return run_with_workspace("sdraw", be, d, ins, _lib.SdrawOutputs(), _lib.SDRAW_OUT_NAMES, _lib.SDRAW_OUT_I32,
                              _lib.sdraw_shapes(B, T, D, k0), names, out_f32=("X",) if out_f32 else (), noise=noise)


def _scored_inputs(be, src, truth, R, D, population, truth_series, first_day):
    """The checks ensemble_score and ensemble_joint_score share on src [T, rows, R * D] or [T, R * D], truth [T, rows', Rt],
    population, truth_series and first_day; returns (R, D, T, rows, Rt, population, truth, truth_series, first_day) as the
    backend's arrays"""
    if src.ndim not in (2, 3):
        raise ValueError("src must be [T, rows, B] or [T, B]")
    R, D = int(R), int(D)
    if src.shape[-1] != R * D:
        raise ValueError(f"src holds {src.shape[-1]} chains, R * D = {R * D}")
    T, rows = int(src.shape[0]), (1 if src.ndim == 2 else int(src.shape[1]))
    pop = be.f64(population)
    if pop is not None and tuple(pop.shape) != (R,):
        raise ValueError("population must be [R]")
    ro = rows + int(pop is not None)
    truth = be.f64(truth)
    if truth.ndim == 2 and src.ndim == 2:
        truth = truth.reshape(T, 1, truth.shape[-1]) if truth.shape[0] == T else truth
    if truth.ndim != 3 or tuple(truth.shape[:2]) != (T, ro):
        raise ValueError(f"truth must be [T, rows', Rt] = [{T}, {ro}, Rt] ([T, Rt] for a [T, B] src)")
    Rt = int(truth.shape[2])
    ts, fd = be.i32(truth_series), be.i32(first_day)
    if ts is None and Rt != R:
        raise ValueError(f"truth holds {Rt} columns, R = {R}: pass truth_series [R]")
    if ts is not None:
        if tuple(ts.shape) != (R,):
            raise ValueError("truth_series must be [R]")
        if not be.resident(truth_series):
            h = np.asarray(truth_series)
            if h.min() < 0 or h.max() >= Rt:
                raise ValueError("truth_series must hold entries in 0 .. Rt-1")
    if fd is not None and tuple(fd.shape) != (R,):
        raise ValueError("first_day must be [R]")
    return R, D, T, rows, Rt, pop, truth, ts, fd


def ensemble_score(be, src, truth, R, D, alpha, n_bins, population, truth_series, first_day, k0, k1, outputs, test_launch_items=0):
    """src: contiguous [T, rows, R * D] or [T, R * D], float32 or float64, where the call reads it"""
    R, D, T, rows, Rt, pop, truth, ts, fd = _scored_inputs(be, src, truth, R, D, population, truth_series, first_day)
    d = _lib.make_escore_desc(T, rows, R, D, Rt, alpha, n_bins, storage=int(_is_f32(src)), derive_newcases=int(pop is not None),
                              k0=k0, k1=k1, test_launch_items=test_launch_items)
    names = _lib.escore_out_names(outputs, n_bins)
    ins = _lib.EscoreInputs()
    for k, v in zip(_lib.ESCORE_IN_NAMES, (src, pop, truth, ts, fd)):
        setattr(ins, k, be.ptr(v))
    probe = _lib.EscoreOutputs()
    for k in names:
        setattr(probe, k, 1)                            # validate looks only at which outputs are asked for
    err = C.create_string_buffer(256)
    _lib.check(_lib.lib().epi_escore_validate(C.byref(d), C.byref(ins), C.byref(probe), err), err)   # before anything is allocated
    out = run_with_workspace("escore", be, d, ins, _lib.EscoreOutputs(), _lib.ESCORE_OUT_NAMES, _lib.ESCORE_OUT_I32,
                             _lib.escore_shapes(T, rows, R, d.n_a, d.n_bins, d.derive_newcases), names)
    if src.ndim == 2:
        out = {k: v.reshape(tuple(v.shape[:-2]) + tuple(v.shape[-1:])) for k, v in out.items()}
    return out


def path_functionals(be, src, R, D, thresholds, population, first_day, k0, k1, outputs, test_segments=0, test_launch_groups=0):
    """src: contiguous [T, rows, R * D] or [T, R * D], float32 or float64, where the call reads it"""
    if src.ndim not in (2, 3):
        raise ValueError("src must be [T, rows, B] or [T, B]")
    R, D = int(R), int(D)
    if src.shape[-1] != R * D:
        raise ValueError(f"src holds {src.shape[-1]} chains, R * D = {R * D}")
    T, rows = int(src.shape[0]), (1 if src.ndim == 2 else int(src.shape[1]))
    pop = be.f64(population)
    if pop is not None and tuple(pop.shape) != (R,):
        raise ValueError("population must be [R]")
    ro = rows + int(pop is not None)
    thr = be.f64(thresholds)
    n_thr = 0
    if thr is not None:
        if thr.ndim == 2 and src.ndim == 2:
            thr = thr.reshape(thr.shape[0], 1, thr.shape[1])
        if thr.ndim != 3 or tuple(thr.shape[1:]) != (ro, R):
            raise ValueError(f"thresholds must be [n_thr, rows', R] = [n_thr, {ro}, {R}] ([n_thr, R] for a [T, B] src)")
        n_thr = int(thr.shape[0])
        if n_thr == 0:
            thr = None
    fd = be.i32(first_day)
    if fd is not None and tuple(fd.shape) != (R,):
        raise ValueError("first_day must be [R]")
    d = _lib.make_pathfn_desc(T, rows, R, D, n_thr, storage=int(_is_f32(src)), derive_newcases=int(pop is not None), k0=k0, k1=k1,
                              test_segments=test_segments, test_launch_groups=test_launch_groups)
    names = _lib.pathfn_out_names(outputs, n_thr)
    ins = _lib.PathfnInputs()
    for k, v in zip(_lib.PATHFN_IN_NAMES, (src, pop, thr, fd)):
        setattr(ins, k, be.ptr(v))
    probe = _lib.PathfnOutputs()
    for k in names:
        setattr(probe, k, 1)                            # validate looks only at which outputs are asked for
    err = C.create_string_buffer(256)
    _lib.check(_lib.lib().epi_pathfn_validate(C.byref(d), C.byref(ins), C.byref(probe), err), err)   # before anything is allocated
    out = run_with_workspace("pathfn", be, d, ins, _lib.PathfnOutputs(), _lib.PATHFN_OUT_NAMES, _lib.PATHFN_OUT_I32,
                             _lib.pathfn_shapes(rows, R, D, n_thr, d.k1 - d.k0, d.derive_newcases), names)
    if src.ndim == 2:
        out = {k: v.reshape(tuple(v.shape[:-2]) + tuple(v.shape[-1:])) for k, v in out.items()}
    return out


def curve_statistics(be, src, R, D, alpha, fence_factor, fence_frac, population, first_day, k0, k1, outputs, test_segments=0,
                     test_launch_groups=0):
    """src: contiguous [T, rows, R * D] or [T, R * D], float32 or float64, where the call reads it"""
    if src.ndim not in (2, 3):
        raise ValueError("src must be [T, rows, B] or [T, B]")
    R, D = int(R), int(D)
    if src.shape[-1] != R * D:
        raise ValueError(f"src holds {src.shape[-1]} chains, R * D = {R * D}")
    T, rows = int(src.shape[0]), (1 if src.ndim == 2 else int(src.shape[1]))
    pop = be.f64(population)
    if pop is not None and tuple(pop.shape) != (R,):
        raise ValueError("population must be [R]")
    fd = be.i32(first_day)
    if fd is not None and tuple(fd.shape) != (R,):
        raise ValueError("first_day must be [R]")
    fence_factor = 0.0 if fence_factor is None else float(fence_factor)
    d = _lib.make_cdepth_desc(T, rows, R, D, alpha, fence_factor, fence_frac if fence_factor > 0.0 else 0.0, storage=int(_is_f32(src)),
                              derive_newcases=int(pop is not None), k0=k0, k1=k1, test_segments=test_segments,
                              test_launch_groups=test_launch_groups)
    names = _lib.cdepth_out_names(outputs, d.n_alpha, fence_factor)
    ins = _lib.CdepthInputs()
    for k, v in zip(_lib.CDEPTH_IN_NAMES, (src, pop, fd)):
        setattr(ins, k, be.ptr(v))
    probe = _lib.CdepthOutputs()
    for k in names:
        setattr(probe, k, 1)                            # validate looks only at which outputs are asked for
    err = C.create_string_buffer(256)
    _lib.check(_lib.lib().epi_cdepth_validate(C.byref(d), C.byref(ins), C.byref(probe), err), err)   # before anything is allocated
    out = run_with_workspace("cdepth", be, d, ins, _lib.CdepthOutputs(), _lib.CDEPTH_OUT_NAMES, _lib.CDEPTH_OUT_I32,
                             _lib.cdepth_shapes(T, rows, R, D, d.n_alpha, d.derive_newcases), names)
    if src.ndim == 2:
        out = {k: v.reshape(tuple(v.shape[:-2]) + tuple(v.shape[-1:])) for k, v in out.items()}
    return out


def ensemble_joint_score(be, src, truth, R, D, vs_p, max_lag, population, truth_series, first_day, k0, k1, outputs, test_launch_tiles=0):
    """src: contiguous [T, rows, R * D] or [T, R * D], float32 or float64, where the call reads it"""
    R, D, T, rows, Rt, pop, truth, ts, fd = _scored_inputs(be, src, truth, R, D, population, truth_series, first_day)
    if vs_p not in _lib.EJOINT_VS_ORDERS:
        raise ValueError("vs_p must be None, 0.5 or 1: the variogram score is pinned for these two exponents only")
    d = _lib.make_ejoint_desc(T, rows, R, D, Rt, _lib.EJOINT_VS_ORDERS[vs_p], max_lag, storage=int(_is_f32(src)),
                              derive_newcases=int(pop is not None), k0=k0, k1=k1, test_launch_tiles=test_launch_tiles)
    names = _lib.ejoint_out_names(outputs, d.vs_order)
    ins = _lib.EjointInputs()
    for k, v in zip(_lib.EJOINT_IN_NAMES, (src, pop, truth, ts, fd)):
        setattr(ins, k, be.ptr(v))
    probe = _lib.EjointOutputs()
    for k in names:
        setattr(probe, k, 1)                            # validate looks only at which outputs are asked for
    err = C.create_string_buffer(256)
    _lib.check(_lib.lib().epi_ejoint_validate(C.byref(d), C.byref(ins), C.byref(probe), err), err)   # before anything is allocated
    out = run_with_workspace("ejoint", be, d, ins, _lib.EjointOutputs(), _lib.EJOINT_OUT_NAMES, _lib.EJOINT_OUT_I32,
                             _lib.ejoint_shapes(rows, R, D, d.derive_newcases), names)
    if src.ndim == 2:
        out = {k: v.reshape(tuple(v.shape[:-2]) + tuple(v.shape[-1:])) for k, v in out.items()}
    return out


def innovation_diagnostics(be, innovations, S, n_lags, k0, k1, flip, lane_block, B, outputs):
    f32 = str(innovations.dtype).endswith("float32")
    e = (be.f32 if f32 else be.f64)(innovations)
    if e.ndim != 2:
        raise ValueError("innovations must be [T, B] ([T, nblk * blk] for chain-blocked arrays)")
    T, Bp = (int(v) for v in e.shape)
    blk = int(lane_block)
    if blk < 0:
        raise ValueError("lane_block must be >= 0")
    if B is None:
        if blk > 0 and S is None:
            raise ValueError("chain-blocked innovations without S need B")
        B = Bp if blk == 0 else int(S.shape[-1])
    B = int(B)
    if blk <= 0 or blk >= B:
        blk = 0
    if Bp != (B if blk == 0 else (B + blk - 1) // blk * blk):
        raise ValueError("innovations must be [T, B] ([T, nblk * blk] for chain-blocked arrays)")
    S = be.f64(S)
    if S is not None and tuple(S.shape) != (T, B):
        raise ValueError("S must be [T, B]")
    names = _lib.idiag_out_names(outputs)
    d = _lib.make_idiag_desc(B, T, n_lags, k0, k1, int(bool(flip)), blk, int(f32))
    err = C.create_string_buffer(256)
    _lib.check(_lib.lib().epi_idiag_validate(C.byref(d), err), err)      # before anything is allocated from n_lags
    ins = _lib.IdiagInputs()
    ins.e, ins.S = be.ptr(e), be.ptr(S)
    return run_with_workspace("idiag", be, d, ins, _lib.IdiagOutputs(), _lib.IDIAG_OUT_NAMES, _lib.IDIAG_OUT_I32,
                              _lib.idiag_shapes(B, d.n_lags), names)

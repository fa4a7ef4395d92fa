"""Shared helpers for the test-suite: Workload <-> MATLAB-shaped arguments, comparisons."""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from epidemicmodeling_amd import layout as L  # noqa: E402
from oracle import ekf_numpy as enp  # noqa: E402
from oracle import oracle_lib as olib  # noqa: E402

OUT_NAMES = ["u_opt", "u_opt_smooth", "S_MINUS", "S_PLUS", "S_SMOOTH", "P_MINUS", "P_PLUS", "P_SMOOTH",
             "K_GAIN", "innovations", "rho"]


def chain_args(w, c):
    """MATLAB-shaped arguments of chain `c` of Workload `w` for oracle/ekf_numpy.run_model."""
    m = w.m
    sx = int(w.x_series[c]) if w.x_series is not None else c
    su = int(w.u_series[c]) if w.u_series is not None else c
    p = enp.Params(
        dt=w.prm[L.PRM_DT, c], beta=w.prm[L.PRM_BETA, c], gamma=w.prm[L.PRM_GAMMA, c],
        sigma=w.prm[L.PRM_SIGMA, c], b=w.prm[L.PRM_B, c], epsilon=w.prm[L.PRM_EPSILON, c],
        s_min=w.prm[L.PRM_S_MIN, c], i_min=w.prm[L.PRM_I_MIN, c],
        alpha_min=w.prm[L.PRM_ALPHA_MIN, c], alpha_max=w.prm[L.PRM_ALPHA_MAX, c],
        a=w.prm[L.PRM_A:L.PRM_A + w.n_npi, c].copy(), u_min=w.prm[L.PRM_U_MIN:L.PRM_U_MIN + w.n_npi, c].copy(),
        u_max=w.prm[L.PRM_U_MAX:L.PRM_U_MAX + w.n_npi, c].copy(),
        w=w.prm[L.PRM_W_EFF:L.PRM_W_EFF + w.n_npi, c].copy(), obs_type=w.obs_type)
    u = np.ascontiguousarray(w.u[:, :, su].T)            # n_npi x T
    x = w.x[:, sx].copy()
    R_v = w.R_series[:, sx].copy() if w.R_series is not None else float(w.R_scalar[c])
    Pi = w.Ps_init[:, c].reshape(m, m, order="F")
    Pf = w.Ps_final[:, c].reshape(m, m, order="F")
    if np.ndim(w.Q) == 3:                                # time-varying: [T][m*m][B] -> m x m x T
        Q = np.ascontiguousarray(w.Q[:, :, c].T).reshape(m, m, -1, order="F")
    else:
        Q = w.Q[:, c].reshape(m, m, order="F")
    return (u, x, p, w.s_init[:, c].copy(), Pi, w.s_final[:, c].copy(), Pf, np.zeros(m),
            float(w.prm[L.PRM_V_BAR, c]), Q, R_v, float(w.prm[L.PRM_BETA_EKF, c]),
            float(w.prm[L.PRM_GAMMA_EKF, c]), w.L, w.order)


def numpy_chain(w, c):
    """Run chain c through the NumPy restatement; returns dict name -> MATLAB-shaped array."""
    out = enp.run_model(w.model, *chain_args(w, c))
    if w.model.startswith("NewCase"):
        names = ["u_opt", "S_MINUS", "S_PLUS", "S_SMOOTH", "P_MINUS", "P_PLUS", "P_SMOOTH", "K_GAIN",
                 "innovations", "rho"]
        return dict(zip(names, out))
    d = dict(zip(OUT_NAMES, out[:11]))
    d["pinv_rank"] = out[11]
    return d


def oracle_batch(w, n_threads=0, outputs=None):
    """Run Workload `w` through the C oracle's batched driver."""
    return olib.run_batch(w.model, w.T, w.n_npi, w.L, w.order, w.obs_type, w.x, w.u, w.prm, w.s_init,
                          w.Ps_init, w.s_final, w.Ps_final, w.Q, R_series=w.R_series, R_scalar=w.R_scalar,
                          x_series=w.x_series, u_series=w.u_series, n_threads=n_threads, outputs=outputs)


def batch_chain(out, name, c, m):
    """Chain c of batched output `name` reshaped to the MATLAB shape."""
    a = out[name]
    if a.ndim == 2:
        return a[:, c]
    v = a[:, :, c]                      # [T, rows]
    if name.startswith("P_"):
        return v.T.reshape(m, m, -1, order="F")
    if name == "K_GAIN":
        return v.T.reshape(m, 1, -1)
    return v.T


def oracle_guard_fired(ref, model):
    """[B] bool from an oracle result: did the non-finite guard of GenericEKF.m:211 fire at any executed smoother step
    (pinv_rank == -1 there)?  That is bit 0 of the library's per-chain `status`.  The smoother never executes the last
    column (the first one for the time-flipped wrappers), whose rank word is -1 by convention."""
    rk = ref["pinv_rank"]
    ex = rk[1:] if "Backward" in model else rk[:-1]
    return (ex == -1).any(axis=0)


def rel_err(a, b):
    """max |a-b| / max(|b|) over finite entries, with NaN/Inf patterns required to match."""
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    fa, fb = np.isfinite(a), np.isfinite(b)
    if not np.array_equal(fa, fb):
        return np.inf
    if not fa.any():
        return 0.0
    scale = np.max(np.abs(b[fb]))
    if scale == 0:
        return float(np.max(np.abs(a[fa])))
    return float(np.max(np.abs(a[fa] - b[fb])) / scale)


def rowwise_rel_err(a, b):
    """Per-row (first axis) relative error, max over rows: each state component is compared
    against its own magnitude (s ~ 1, i ~ 1e-6, lambda ~ 1e20 must not mask each other)."""
    a = np.asarray(a); b = np.asarray(b)
    return max(rel_err(a[i], b[i]) for i in range(a.shape[0]))


def rowwise_abs_rel_err(a, b, floor=1e-12):
    """Per-row error relative to that row's own magnitude, with an absolute floor so that rows that are
    numerically zero (costates at epsilon -> 1) do not turn rounding noise into O(1) 'relative' error."""
    a = np.asarray(a); b = np.asarray(b)
    worst = 0.0
    for i in range(a.shape[0]):
        fa, fb = np.isfinite(a[i]), np.isfinite(b[i])
        if not np.array_equal(fa, fb):
            return np.inf
        if not fa.any():
            continue
        scale = max(np.max(np.abs(b[i][fb])), floor)
        worst = max(worst, float(np.max(np.abs(a[i][fa] - b[i][fb])) / scale))
    return worst


def load_golden(name):
    """tests/golden/<name>.npz -> (Workload, dict of expected outputs)."""
    from epidemicmodeling_amd import synth
    d = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    g = lambda k: d["in_" + k] if ("in_" + k) in d.files else None
    w = synth.Workload(model=str(d["in_model"]), T=int(d["in_T"]), n_npi=int(d["in_n_npi"]), x=d["in_x"], u=d["in_u"],
                       R_series=g("R_series"), R_scalar=g("R_scalar"), x_series=g("x_series"), u_series=g("u_series"),
                       prm=d["in_prm"], s_init=d["in_s_init"], Ps_init=d["in_Ps_init"], s_final=d["in_s_final"],
                       Ps_final=d["in_Ps_final"], Q=d["in_Q"], L=int(d["in_L"]), order=int(d["in_order"]),
                       obs_type=str(d["in_obs_type"]))
    exp = {k[4:]: d[k] for k in d.files if k.startswith("out_")}
    return w, exp


GOLDEN_CASES = ["sia3_cfg3", "sia6_cfg4", "sia6_row3_adaptiveR", "newcase6_row4", "newcase6_codegen_row4",
                "sia3_backward", "sia6_backward"]


def with_time_varying_q(w, seed=0):
    """Same workload with Q_w as an m x m x T array per chain (GenericExtendedKalmanFilter.m:63-73):
    Q [T][m*m][B], each page the fixed Q scaled by a slowly varying positive factor."""
    import copy
    rng = np.random.default_rng(seed)
    w2 = copy.copy(w)
    scale = 1.0 + 0.5 * np.sin(np.arange(w.T) / 7.0)[:, None, None] + 0.1 * rng.random((w.T, 1, w.B))
    w2.Q = np.ascontiguousarray(w.Q[None, :, :] * scale)
    return w2


def with_npis(w, n):
    """Copy of Workload `w` with its first `n` NPIs only: u [T][n][Su] (contiguous), and the per-NPI parameter rows a, u_min,
    u_max and w zeroed beyond `n` (the padding the library expects of an n_npi < 12 batch)."""
    import copy
    w2 = copy.copy(w)
    w2.n_npi = int(n)
    w2.u = np.ascontiguousarray(w.u[:, :n, :])
    w2.prm = w.prm.copy()
    for f in (L.PRM_A, L.PRM_U_MIN, L.PRM_U_MAX, L.PRM_W_EFF):
        w2.prm[f + n:f + 12] = 0.0
    return w2


def make_regression_problem(S=40, D=120, n=12, seed=0):
    """Regression windows like TrainPredictPrescribeNPI.m:251-253: X = NPI_MAXES - InterventionPlans (small integers,
    step-like in time, some NPIs never changed => constant / collinear columns, some always at the maximum => zero
    columns), y = smoothed alpha.  Returns X [D, n, S], y [D, S]."""
    from epidemicmodeling_amd import synth
    rng = np.random.default_rng(seed)
    umax = synth.IP_MAXES[:n]
    lvl = np.floor(rng.random((D, n, S)) * (umax[None, :, None] + 1))
    keep = rng.random((D, n, S)) < 0.04
    keep[0] = True
    idx = np.maximum.accumulate(np.where(keep, np.arange(D)[:, None, None], 0), axis=0)
    ip = np.take_along_axis(lvl, idx, axis=0)                    # piecewise-constant policies
    if n > 2:
        ip[:, 2, ::3] = 1.0                                       # never changed
    if n > 5:
        ip[:, 5, ::3] = 2.0                                       # never changed (collinear with the one above)
    if n > 7:
        ip[:, 7, ::4] = umax[7]                                   # always at the maximum: zero column of X
    X = umax[None, :, None] - ip
    a_true = np.maximum(rng.normal(0.0, 0.02, (n, S)), 0.0)
    y = np.einsum("dns,ns->ds", X, a_true) + 0.08 + 0.004 * rng.standard_normal((D, S))
    y[:, 1::7] -= 0.2                                             # regions whose mean residual is negative
    return np.ascontiguousarray(X), np.ascontiguousarray(y)


def lapack_reading_worker(job):
    """Worker of a process pool (spawn context: the children never touch the GPU): chains `cs` of Workload `w` through
    oracle/ekf_numpy.py -- the independent reading of the .m files that uses LAPACK's SVD for pinv, the closest thing to
    MATLAB's own built-in available here.  Returns the quantities the HIP-vs-LAPACK report compares."""
    w, cs = job[0], job[1]
    one_ulp = len(job) > 2 and job[2]          # also: the same reading with every observation moved by one ulp ("*_1ulp")
    if one_ulp:
        w2 = w.select(np.arange(w.B))
        w2.x = np.nextafter(w.x, np.inf)
    out = []
    for c in cs:
        nd = numpy_chain(w, int(c))
        r = {k: np.asarray(nd[k]) for k in ("S_MINUS", "S_PLUS", "S_SMOOTH", "u_opt_smooth", "pinv_rank") if k in nd}
        if one_ulp:
            n2 = numpy_chain(w2, int(c))
            r.update({k + "_1ulp": np.asarray(n2[k]) for k in ("S_MINUS", "S_PLUS")})
        out.append(r)
    return out


def host_call(w, devices=None, outputs=None, extras=True, shape=0, out=None, timing=None, placement_tries=0, report=None, device=0):
    """Workload `w` through the HOST-pointer C ABI (classic layout, numpy arrays [T][rows][B]): epi_ekf_run_host on `device`,
    or -- devices = list of device ids -- epi_ekf_run_host_multi with one chain block per entry.  Returns dict of arrays.
    `out`: the dict a previous call returned (its arrays are written again instead of allocating and NaN-filling new ones);
    `timing`: a list that gets the seconds the C call itself took appended; `placement_tries` / `report` (a list that gets
    {"tries", "chosen", "ms"} appended): epi_batch_desc.placement_tries and the epi_placement_report the call fills."""
    import ctypes as C
    import time
    from epidemicmodeling_amd import _lib
    names = [n for n in (outputs or OUT_NAMES) if not (w.model.startswith("NewCase") and n == "u_opt_smooth")]
    m, n_npi, B, T = w.m, w.n_npi, w.B, w.T
    rows = {"u_opt": n_npi, "u_opt_smooth": n_npi, "S_MINUS": m, "S_PLUS": m, "S_SMOOTH": m, "P_MINUS": m * m, "P_PLUS": m * m,
            "P_SMOOTH": m * m, "K_GAIN": m}
    if out is None:
        out = {k: np.full((T, rows[k], B) if k in rows else (T, B), np.nan) for k in names}
    mask = 0
    for k in names:
        mask |= L.OUT_BITS[k]
    Sx = w.x.shape[1]; Su = w.u.shape[2]
    d = _lib.make_desc(w.model, B, T, Sx, Su, n_npi, w.L, w.order, w.obs_type, 1 if w.R_series is not None else 0, mask,
                       1 if np.ndim(w.Q) == 3 else 0)
    d.shape = shape
    d.placement_tries = int(placement_tries)
    ins, outs = _lib.Inputs(), _lib.Outputs()
    rep = _lib.PlacementReport()
    outs.placement = C.addressof(rep)
    keep = []
    def ptr(a, dt=np.float64):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dt); keep.append(a)
        return a.ctypes.data
    ins.x_series, ins.u_series = ptr(w.x_series, np.int32), ptr(w.u_series, np.int32)
    ins.x, ins.u, ins.R_series, ins.R_scalar, ins.prm = ptr(w.x), ptr(w.u), ptr(w.R_series), ptr(w.R_scalar), ptr(w.prm)
    ins.s_init, ins.Ps_init, ins.s_final, ins.Ps_final, ins.Q = ptr(w.s_init), ptr(w.Ps_init), ptr(w.s_final), ptr(w.Ps_final), ptr(w.Q)
    for k in names:
        setattr(outs, k, out[k].ctypes.data)
    if extras:
        if "pinv_rank" not in out:
            out["pinv_rank"] = np.full((T, B), -7, dtype=np.int32); out["status"] = np.full((B,), -7, dtype=np.int32)
        outs.pinv_rank, outs.status = out["pinv_rank"].ctypes.data, out["status"].ctypes.data
    err = C.create_string_buffer(256)
    t0 = time.perf_counter()
    if devices is None:
        rc = _lib.lib().epi_ekf_run_host(C.byref(d), C.byref(ins), C.byref(outs), int(device), err)
    else:
        ids = (C.c_int * len(devices))(*devices)
        rc = _lib.lib().epi_ekf_run_host_multi(C.byref(d), C.byref(ins), C.byref(outs), len(devices), ids, err)
    if timing is not None:
        timing.append(time.perf_counter() - t0)
    _lib.check(rc, err)
    if report is not None:
        report.append({"tries": int(rep.tries), "chosen": int(rep.chosen), "ms": [float(rep.ms[i]) for i in range(rep.tries)]})
    return out


def flat_call(sym, args, device=0, gpu=None):
    """One of the flat-argument calls (simulators, small fits) in either form: epi_<sym>_host(args..., device, err) on NumPy
    arrays or, with `gpu` (a torch device), epi_<sym>_device(args..., stream, err) on copies there.  args: ctypes descriptors
    (by reference; a NoiseDesc among them selects the _seeded symbol), numbers, None, NumPy arrays (inputs),
    (name, shape[, dtype]) for an output array, (StructClass, {field: shape}) for a struct of optional float64 outputs.
    Outputs are NaN / -1 filled beforehand.  Returns {name: NumPy array}."""
    import ctypes as C
    import torch
    from epidemicmodeling_amd import _lib
    h, keep, out, call = _lib.lib(), [], {}, []

    def put(a):
        a = np.ascontiguousarray(a) if gpu is None else torch.as_tensor(np.ascontiguousarray(a)).to(gpu)
        keep.append(a)
        return a.ctypes.data if gpu is None else a.data_ptr()

    def new(name, shape, dtype=np.float64):
        fill = np.nan if dtype == np.float64 else -1
        out[name] = a = np.full(shape, fill, dtype=dtype) if gpu is None else \
            torch.full(shape, fill, dtype=torch.float64 if dtype == np.float64 else torch.int32, device=gpu)
        return a.ctypes.data if gpu is None else a.data_ptr()

    for a in args:
        if isinstance(a, C.Structure):
            call.append(C.byref(a))
        elif isinstance(a, np.ndarray):
            call.append(put(a))
        elif isinstance(a, tuple) and isinstance(a[0], str):
            call.append(new(*a))
        elif isinstance(a, tuple):
            s = a[0]()
            for k, shape in a[1].items():
                setattr(s, k, new(k, shape))
            keep.append(s)
            call.append(C.byref(s))
        else:
            call.append(a)
    seeded = "_seeded" if any(isinstance(a, _lib.NoiseDesc) for a in args) else ""
    err = C.create_string_buffer(256)
    if gpu is None:
        rc = getattr(h, f"epi_{sym}_host{seeded}")(*call, int(device), err)
    else:
        if sym == "preprocess":                      # the device form takes its workspace from the caller
            wsb = int(h.epi_preprocess_workspace_bytes(C.byref(args[0])))
            keep.append(torch.empty(max(wsb // 8, 1), dtype=torch.float64, device=gpu))
            call += [keep[-1].data_ptr(), wsb]
        rc = getattr(h, f"epi_{sym}_device{seeded}")(*call, C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream), err)
        torch.cuda.synchronize(gpu)
    _lib.check(rc, err)
    return {k: (v if gpu is None else v.cpu().numpy()) for k, v in out.items()}


FLAT_SEED, FLAT_STREAM = 0x5EEDF00D12345, 3


def flat_call_cases():
    """name -> (sym, args of the host form, args of the device form) for flat_call: the nine host functions of the simulators
    and small fits, each with every optional array present ("/full") and with every optional array absent ("/bare"), and
    the two seeded forms.  B = 5 chains, K = 6 days, 2 NPIs; Monte-Carlo 3 regions x 4 scenarios x 5 days; preprocessing
    and NNLS 3 regions x 24 days / 16 rows x 3 columns; Rt_ExpFitEKF 24 days, window 5.  The device form differs where the host form
    may decline an output the device form requires (rt_expfit/bare)."""
    from epidemicmodeling_amd import _lib, synth
    rng = np.random.default_rng(11)
    B, K, n, Su = 5, 6, 2, 3
    i32 = np.int32

    def sim_prm(cols):
        sp = np.zeros((48, cols))
        sp[0], sp[1], sp[2], sp[4], sp[5], sp[7], sp[11] = 0.99, 0.01, 0.3 + 0.1 * rng.random(cols), 100.0, 1 / 7, synth.MODEL_BETA, 1.0
        sp[8:11] = 1e-3
        sp[12:12 + n], sp[24:24 + n], sp[36:36 + n] = 0.01, synth.IP_MAXES[:n, None], 1.0
        return sp

    def sim_desc(Su_, noise, with_cost):
        d = _lib.SimDesc()
        d.abi_version, d.B, d.K, d.Su, d.n_npi, d.noise, d.with_cost = _lib.ABI_VERSION, B, K, Su_, n, noise, with_cost
        return d

    def mc_desc(noise, prefix_days):
        d = _lib.McDesc()
        d.abi_version, d.R, d.n_scen, d.K, d.n_npi, d.noise, d.prefix_days, d.seed_lo = _lib.ABI_VERSION, 3, 4, 5, n, noise, prefix_days, 77
        return d

    cases = {}
    sp, series = sim_prm(B), (np.arange(B) % Su).astype(i32)
    u_shared, u_own, z = rng.random((K, n, Su)) * 2, rng.random((K, n, B)) * 2, rng.standard_normal((K, 3, B))
    traj = [(k, (K, B)) for k in ("s", "i", "alpha")]
    cost = [("J0", (B,)), ("J1", (B,))]
    cases["sialpha_sim/full"] = ("sialpha_sim", [sim_desc(Su, 1, 1), series, u_shared, sp, z] + traj + cost)
    cases["sialpha_sim/bare"] = ("sialpha_sim", [sim_desc(B, 0, 0), None, u_own, sp, None] + traj + [None, None])
    noise = _lib.make_noise_desc(FLAT_SEED, FLAT_STREAM)
    cases["sialpha_sim/seeded"] = ("sialpha_sim", [sim_desc(Su, 0, 1), noise, series, u_shared, sp, None] + traj + cost)

    spr, u_min, zr = sim_prm(3), np.zeros((n, 3)), rng.standard_normal((5, 3, 12))
    J = [("J0", (4, 3)), ("J1", (4, 3))]
    cases["random_npi_mc/full"] = ("random_npi_mc", [mc_desc(1, 7), spr, u_min, zr, rng.random(3), rng.random(3), ("u", (5, n, 12))] + J)
    cases["random_npi_mc/bare"] = ("random_npi_mc", [mc_desc(0, 0), spr, u_min, None, None, None, None] + J)
    cases["random_npi_mc/seeded"] = ("random_npi_mc", [mc_desc(0, 0), noise, spr, u_min, None, None, None, ("u", (5, n, 12))] + J)

    par, init = 0.05 + 0.2 * rng.random((K, 7, B)), np.tile(np.array([[0.98], [0.01], [0.01], [0.0], [0.0]]), (1, B))
    sat = np.tile(np.array([[0.2], [0.1], [0.01], [0.02], [0.01], [0.02]]), (1, B)) * (1 + 0.1 * rng.random((6, B)))
    cases["seirp_sim/full"] = ("seirp_sim", [B, K, K, 0.5, 1, 0, par, init, sat, ("out", (K, 5, B))])
    cases["seirp_sim/bare"] = ("seirp_sim", [B, K, K, 0.5, 0, 0, par, init, None, ("out", (K, 5, B))])

    prm = np.stack([np.full(B, 1 / 7), 0.99 - 0.01 * rng.random(B), 0.01 * (1 + rng.random(B))])
    si = [("s", (K, B)), ("i", (K, B))]
    cases["si_controlled/full"] = ("si_controlled", [B, K, 2, 1.0, (np.arange(B) % 2).astype(i32), 0.2 + 0.1 * rng.random((K - 1, 2)), prm] + si)
    cases["si_controlled/bare"] = ("si_controlled", [B, K, B, 1.0, None, 0.2 + 0.1 * rng.random((K - 1, B)), prm] + si)

    nc = rng.random((K, B)) * 100
    cases["npi_cost/full"] = ("npi_cost", [B, K, n, Su, 1, series, nc, u_shared, rng.random((K, n, B))] + cost)
    cases["npi_cost/bare"] = ("npi_cost", [B, K, n, B, 0, None, nc, u_own, rng.random((n, B))] + cost)

    sir = np.stack([0.3 + 0.1 * rng.random(B), np.full(B, 0.1), np.full(B, 0.01), np.full(B, 0.99), np.full(B, 0.01), np.zeros(B)])
    cases["sir_sim/full"] = ("sir_sim", [B, K, 0.5, sir, ("out", (K, 3, B))])

    raw = synth.make_raw_counts(3, 24, seed=4, n_npi=n)

    def pre_desc(n_npi):
        d = _lib.PreDesc()
        d.abi_version, d.S, d.T, d.n_npi, d.W, d.first_num_days, d.min_cases = _lib.ABI_VERSION, 3, 24, n_npi, 7, 7, 1.0
        return d

    pre_all = {k: (3,) if k == "I0" else ((24, n, 3) if k == "ip_filled" else (24, 3)) for k in _lib.PRE_OUT_NAMES}
    cases["preprocess/full"] = ("preprocess", [pre_desc(n), raw["cases"], raw["deaths"], raw["population"], raw["ip"], (_lib.PreOutputs, pre_all)])
    cases["preprocess/bare"] = ("preprocess", [pre_desc(0), raw["cases"], None, raw["population"], None,
                                               (_lib.PreOutputs, {"x_new": (24, 3), "I0": (3,)})])

    nd = _lib.NnlsDesc()
    nd.abi_version, nd.S, nd.D, nd.n, nd.max_iters = _lib.ABI_VERSION, 3, 16, 3, 100
    X, y = rng.integers(0, 4, size=(16, 3, 3)).astype(np.float64), rng.random((16, 3))
    cases["nnls_affine_fit/full"] = ("nnls_affine_fit", [nd, X, y, ("a", (3, 3)), ("b", (3,)), ("min_err", (3,)), ("iters", (3,), i32),
                                                         ("flag", (3,), i32)])
    cases["nnls_affine_fit/bare"] = ("nnls_affine_fit", [nd, X, y, ("a", (3, 3)), None, None, None, None])

    def rt(w, names):
        d = _lib.RtDesc()
        d.abi_version, d.B, d.T, d.Sx, d.L, d.order = _lib.ABI_VERSION, w.B, w.T, w.x.shape[1], w.L, w.order
        rows = {"S_MINUS": 2, "S_PLUS": 2, "P_MINUS": 4, "P_PLUS": 4, "K_GAIN": 2, "S_SMOOTH": 2, "P_SMOOTH": 4}
        return [d, w.x_series, w.x, w.rp, (_lib.RtOutputs, {k: (w.T, rows[k], w.B) if k in rows else (w.T, w.B) for k in names})]

    forward = ("S_MINUS", "S_PLUS", "P_MINUS", "P_PLUS")
    cases["rt_expfit_run/full"] = ("rt_expfit_run", rt(synth.make_rt(2, 24, n_draws=2, L=5), _lib.RT_OUT_NAMES))
    w = synth.make_rt(3, 24, L=5, order=2)
    cases["rt_expfit_run/bare"] = ("rt_expfit_run", rt(w, ("S_SMOOTH",)), rt(w, forward + ("S_SMOOTH",)))
    return {k: (v[0], v[1], v[-1]) for k, v in cases.items()}


REFEREE_CASES = ["ref_cfg4_dead_400_120", "ref_cfg4_live_400_120", "ref_cfg4_live_60_120", "ref_row3_adaptiveR_30_120",
                 "ref_cfg3_400", "ref_sia3_backward_120", "ref_sia6_backward_40", "ref_newcase_sweep_400_120",
                 "ref_sia6_backward_150", "ref_sia3_totalcases_200", "ref_cfg4_varying_q_90_30", "ref_cfg3_terminal_120"]
REFEREE_GATE_CAP = 1e-2      # an output whose frozen gate exceeds this is rounding-dominated in fp64: reported, not gated


def referee_inner_gate(fx, base):
    """Round 5 (verdict r04 item 5): the frozen gates are 10 x the larger of the C oracle's and the LAPACK reading's distance from
    the exact result, i.e. set by LAPACK's error -- 5 to 7 decades looser than where the library stands (the smoothed epidemic
    states of `ref_cfg4_dead_400_120` 4.5e-13 against a gate of 2.7e-8): kernel and C oracle could lose five digits TOGETHER
    and stay green.  The inner gate is 100 x the distance the C oracle stood at when the fixture was frozen (at least 1e-12);
    None where that exceeds REFEREE_GATE_CAP (rounding-dominated outputs)."""
    t = max(100.0 * float(fx["dist_C_" + base]), 1e-12)
    return t if t <= REFEREE_GATE_CAP else None


def load_referee(name):
    """tests/golden/<name>.npz (tests/golden/make_golden_referee.py) -> (Workload, dict): `ref_*` the reference's formulas
    in 160-digit arithmetic rounded once (MATLAB shapes + a trailing chain axis), `lap_*` the frozen LAPACK reading,
    `dist_C_* / dist_lap_* / tol_*` the distances measured when the fixture was frozen and the gates derived from them."""
    w, _ = load_golden(name)
    d = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    return w, {k: d[k] for k in d.files if not k.startswith("in_")}


def referee_compare(w, got, fx, what):
    """Outputs `got` (batched [T][rows][B] arrays of the chains of fixture `fx`) against the frozen referee and LAPACK
    vectors.  Returns (failures, report): every output whose frozen gate is <= REFEREE_GATE_CAP must lie within the gate
    of the exact result and within 2 x the gate of the LAPACK reading; pinv ranks must equal the exact ranks outside the
    steps the referee lists as ambiguous (a singular value within 10 x of the cut-off); where the smoothed costates are
    rounding-dominated the free controls may differ from the exact plan in no more entries than the LAPACK reading's did."""
    m, B = w.m, w.B
    fails, rep = [], {}
    rows = lambda a: a[None] if a.ndim == 1 else a.reshape(-1, a.shape[-1])
    for key in sorted(k for k in fx if k.startswith("ref_")):
        n = key[4:]
        if n in ("pinv_rank", "near_cutoff"):
            continue
        diag = n.endswith("_diag")
        base = n[:-5] if diag else n
        if base not in got:
            continue
        worst, worst_lap = 0.0, 0.0
        for c in range(B):
            g = batch_chain(got, base, c, m)
            if diag:
                g = np.stack([g[i, i] for i in range(m)])
            worst = max(worst, rowwise_abs_rel_err(rows(g), rows(fx[key][..., c])))
            if "lap_" + n in fx:
                worst_lap = max(worst_lap, rowwise_abs_rel_err(rows(g), rows(fx["lap_" + n][..., c])))
        tol = float(fx["tol_" + base])
        gated = tol <= REFEREE_GATE_CAP
        rep[n] = {"vs_exact": worst, "vs_lapack_reading": worst_lap if "lap_" + n in fx else None, "gate": tol if gated else None,
                  "frozen_distance_C": float(fx["dist_C_" + base]), "frozen_distance_lapack": float(fx["dist_lap_" + base])}
        if gated and not worst <= tol:
            fails.append((what, n, "vs exact", worst, tol))
        inner = referee_inner_gate(fx, base)
        rep[n]["inner_gate"] = inner
        if inner is not None and not worst <= inner:
            fails.append((what, n, "vs exact, inner gate (100 x the C oracle's frozen distance)", worst, inner))
        if gated and "lap_" + n in fx and not worst_lap <= 2.0 * tol:
            fails.append((what, n, "vs LAPACK reading", worst_lap, 2.0 * tol))
    # the epidemic states of S_SMOOTH have a gate of their own (the costates beside them may be rounding-dominated)
    if "ref_S_SMOOTH" in fx and "S_SMOOTH" in got:
        worst = max(rowwise_abs_rel_err(batch_chain(got, "S_SMOOTH", c, m)[:3], fx["ref_S_SMOOTH"][:3, :, c]) for c in range(B))
        tol = float(fx["tol_S_SMOOTH_states"])
        inner = referee_inner_gate(fx, "S_SMOOTH_states")
        rep["S_SMOOTH_states"] = {"vs_exact": worst, "gate": tol, "inner_gate": inner}
        if not worst <= tol:
            fails.append((what, "S_SMOOTH(1:3)", "vs exact", worst, tol))
        if inner is not None and not worst <= inner:
            fails.append((what, "S_SMOOTH(1:3)", "vs exact, inner gate (100 x the C oracle's frozen distance)", worst, inner))
    if "ref_pinv_rank" in fx and "pinv_rank" in got:
        T = w.T
        amb = {(int(c), (T - 1 - int(k)) if "Backward" in w.model else int(k)) for c, k, _ in fx["ref_near_cutoff"]}
        mm = [(c, int(k)) for c in range(B) for k in np.flatnonzero(got["pinv_rank"][:, c] != fx["ref_pinv_rank"][:, c])]
        out = [x for x in mm if x not in amb]
        rep["pinv_rank"] = {"mismatch_steps": len(mm), "outside_ambiguous_steps": len(out), "ambiguous_steps": len(amb)}
        if out:
            fails.append((what, "pinv_rank", "differs from the exact rank away from the cut-off", out[:5], 0))
    if "flips_lap" in fx and "u_opt_smooth" in got:
        flips = []
        for c in range(B):
            su = int(w.u_series[c]) if w.u_series is not None else c
            fm = np.isnan(w.u[:, :, su].T)
            fm[:, 0 if "Backward" in w.model else -1] = False
            flips.append(int(np.sum(batch_chain(got, "u_opt_smooth", c, m)[fm] != fx["ref_u_opt_smooth"][..., c][fm])))
        rep["control_flips_vs_exact"] = {"this": flips, "frozen_C": fx["flips_C"].tolist(), "frozen_lapack": fx["flips_lap"].tolist(),
                                         "free_controls": fx["free_controls"].tolist()}
        if float(fx["tol_u_opt_smooth"]) <= REFEREE_GATE_CAP:
            if sum(flips) != 0:
                fails.append((what, "u_opt_smooth", "differs from the exact plan", sum(flips), 0))
        elif sum(flips) > max(int(fx["flips_lap"].sum()), int(fx["flips_C"].sum())):
            fails.append((what, "u_opt_smooth", "more flips vs the exact plan than either frozen fp64 reading", sum(flips),
                          max(int(fx["flips_lap"].sum()), int(fx["flips_C"].sum()))))
    return fails, rep


# ---------------------------------------------------------------- poisoned output arenas for optional-output tests
class GuardArena:
    """Every output of a call in ONE byte arena, each segment with `guard` bytes before and after it, all of it filled with
    the byte POISON.  The caller passes ptr(name) for the outputs it requests and NULL for the rest; afterwards untouched(
    requested) says whether every byte outside the requested segments (guards and unrequested neighbours) is still POISON.
    specs: [(name, shape, numpy dtype)].  device: a torch device string for device memory, None for host memory."""
    POISON = 0xA7

    def __init__(self, specs, device=None, guard=256):
        self.specs, self.device, self.seg = specs, device, {}
        off = guard
        for name, shape, dt in specs:
            nb = int(np.prod(shape)) * np.dtype(dt).itemsize
            self.seg[name] = (off, nb, tuple(shape), np.dtype(dt))
            off += (nb + 255) // 256 * 256 + guard
        if device is None:
            self.buf = np.full(off, self.POISON, dtype=np.uint8)
            self.base = self.buf.ctypes.data
        else:
            import torch
            self.buf = torch.full((off,), self.POISON, dtype=torch.uint8, device=device)
            self.base = self.buf.data_ptr()

    def ptr(self, name):
        return self.base + self.seg[name][0]

    def _bytes(self):
        if self.device is None:
            return self.buf.copy()
        import torch
        torch.cuda.synchronize(self.device)
        return self.buf.cpu().numpy()

    def get(self, name):
        off, nb, shape, dt = self.seg[name]
        return self._bytes()[off:off + nb].view(dt).reshape(shape)

    def untouched(self, requested):
        b = self._bytes()
        keep = np.ones(b.size, dtype=bool)
        for name in requested:
            off, nb, _, _ = self.seg[name]
            keep[off:off + nb] = False
        return bool((b[keep] == self.POISON).all())


# ---------------------------------------------------------------- batches at the edges of the kernels' 32-bit addressing
# (tests/test_gpu_addressing_limits.py).  Chains are independent, so a sampled chain of a batch far too large for the oracle
# must equal, bit for bit, the oracle's run of that chain alone -- provided the chains differ, so that an offset that wraps or
# lands in a neighbouring block cannot read a twin.  Every per-chain input is therefore a closed form of the chain index that
# torch evaluates on the device for the whole batch and NumPy re-evaluates for the sample: integer hashing, gathers, and
# integer x power-of-two products (exact in fp64), nothing whose device and host bits could differ.
POISON64 = 0x7FF80000DEADBEEF       # a quiet NaN with a payload no arithmetic produces: "this word was never stored"
POISON32 = 0x7FC0BEEF
POISON_RANK, POISON_STATUS = -7, -1


def chain_hash(c, k):
    """32-bit hash of chain index c (int64 array, NumPy or torch: the same integer operations on both) in stream k.  Every
    intermediate stays below 2^63."""
    h = (c * 2654435761 + (k * 40503 + 12345)) & 0xFFFFFFFF
    h = h ^ (h >> 15)
    h = (h * 73244475) & 0xFFFFFFFF
    h = h ^ (h >> 13)
    h = (h * 73244475) & 0xFFFFFFFF
    return h ^ (h >> 16)


class FormulaBatch:
    """B chains of a generic model derived from a small `base` Workload with one chain per region (S regions, identity series):
    chain c takes region r(c) = chain_hash(c, 1) mod S -- its parameters, covariances and end-point -- and, of its own,
        epsilon(c) = (1 + (chain_hash(c, 2) >> 9)) 2^-24       in (0, 1/2]
        i0(c)      = 2^-20 + (c + 1) 2^-43,   s0(c) = 1 - i0(c)   (injective in c: no two chains share their inputs)
    x_mode / u_mode: "regions" = the S series of the base, chain c reads series r(c) (Sx = S); "one" = a single shared series
    (Sx = 1, region 0's); "own" = one series per chain (Sx = B, identity: column c is a copy of region r(c)'s).
    u_mode = "table" (with Su): a table of Su control series by formula -- integer NPI levels table_level(day, k, s) on the
    days region 0 has controls, free (NaN) where it has none -- of which chain c reads series table_series(c): 0, Su - 1 and
    the middle ones for c mod 8 < 4, a hashed one otherwise.
    A base with a scalar R_v (the NewCase models) passes R_scalar of region r(c).
    plant(chain, row, value) overrides one entry of Ps_init (a covariance that overflows in mid-run)."""

    def __init__(self, base, B, x_mode="regions", u_mode="regions", Su=None):
        assert base.x_series is None and base.u_series is None and base.Sx == base.B and base.Su == base.B
        assert np.ndim(base.Q) == 2
        self.base, self.B, self.S, self.x_mode, self.u_mode = base, int(B), base.B, x_mode, u_mode
        self.m = base.m
        self.Su_table = None if Su is None else int(Su)
        self.planted = []

    def table_series(self, c):
        Su = self.Su_table
        fixed = (c % 8 == 0) * 0 + (c % 8 == 1) * (Su - 1) + (c % 8 == 2) * (Su // 2) + (c % 8 == 3) * (Su // 2 - 1)
        return fixed * (c % 8 < 4) + (chain_hash(c, 6) % Su) * (c % 8 >= 4)

    def table_level(self, t, k, s, umax):
        """Integer NPI level of day t, NPI k, series s (int64 arrays that broadcast; umax the integer maxima, same shape as k)."""
        n = self.base.n_npi
        return chain_hash((t * n + k) * self.Su_table + s, 5) % (umax + 1)

    def plant(self, chain, row, value):
        self.planted.append((int(chain), int(row), float(value)))

    # -- the closed forms: c is an int64 array of chain indices, NumPy or torch
    def region(self, c):
        return chain_hash(c, 1) % self.S

    @staticmethod
    def epsilon_bits(c):
        return (chain_hash(c, 2) >> 9) + 1            # x 2^-24

    @staticmethod
    def i0_bits(c):
        return c + 1 + (1 << 23)                      # x 2^-43

    def _series_index(self, mode, r):
        return {"regions": r, "one": r * 0, "own": None}[mode]

    def host_workload(self, idx):
        """synth.Workload of the chains `idx`, by NumPy."""
        from epidemicmodeling_amd import synth
        b = self.base
        c = np.asarray(idx, dtype=np.int64)
        r = self.region(c)
        prm = np.ascontiguousarray(b.prm[:, r])
        prm[L.PRM_EPSILON] = self.epsilon_bits(c).astype(np.float64) * 2.0 ** -24
        s_init = np.ascontiguousarray(b.s_init[:, r])
        s_init[1] = self.i0_bits(c).astype(np.float64) * 2.0 ** -43
        s_init[0] = 1.0 - s_init[1]
        Ps_init = np.ascontiguousarray(b.Ps_init[:, r])
        for ch, row, v in self.planted:
            Ps_init[row, c == ch] = v

        def series(mode, a):
            if mode == "own":
                return np.ascontiguousarray(a[..., r]), None
            if mode == "one":
                return np.ascontiguousarray(a[..., :1]), np.zeros(c.size, dtype=np.int32)
            return a, r.astype(np.int32)
        x, xs = series(self.x_mode, b.x)
        Rs = None if b.R_series is None else series(self.x_mode, b.R_series)[0]
        Rsc = None if b.R_scalar is None else np.ascontiguousarray(b.R_scalar[r])
        if self.u_mode == "table":
            used, us = np.unique(self.table_series(c), return_inverse=True)
            umax = b.prm[L.PRM_U_MAX:L.PRM_U_MAX + b.n_npi, 0].astype(np.int64)
            tt, kk = np.arange(b.T, dtype=np.int64)[:, None, None], np.arange(b.n_npi, dtype=np.int64)[None, :, None]
            u = self.table_level(tt, kk, used[None, None, :], umax[None, :, None]).astype(np.float64)
            u[np.isnan(b.u[:, 0, 0])] = np.nan
            us = us.astype(np.int32)
        else:
            u, us = series(self.u_mode, b.u)
        return synth.Workload(model=b.model, T=b.T, n_npi=b.n_npi, x=x, u=u, R_series=Rs, R_scalar=Rsc, x_series=xs, u_series=us,
                              prm=prm, s_init=s_init, Ps_init=Ps_init, s_final=np.ascontiguousarray(b.s_final[:, r]),
                              Ps_final=np.ascontiguousarray(b.Ps_final[:, r]), Q=np.ascontiguousarray(b.Q[:, r]), L=b.L,
                              order=b.order, obs_type=b.obs_type)

    def device_workload(self, device):
        """batch.DeviceWorkload of all B chains, evaluated by torch on the device (nothing of size B exists on the host)."""
        import torch
        from epidemicmodeling_amd import batch
        b = self.base
        dev = torch.device(device)
        f = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(dev)
        c = torch.arange(self.B, dtype=torch.int64, device=dev)
        r = self.region(c)
        dw = batch.DeviceWorkload.__new__(batch.DeviceWorkload)
        dw.device = dev
        dw.model, dw.T, dw.n_npi, dw.L, dw.order, dw.obs_type = b.model, b.T, b.n_npi, b.L, b.order, b.obs_type
        dw.m, dw.B = b.m, self.B
        dw.prm = f(b.prm).index_select(1, r)
        dw.prm[L.PRM_EPSILON] = self.epsilon_bits(c).to(torch.float64) * 2.0 ** -24
        dw.s_init = f(b.s_init).index_select(1, r)
        dw.s_init[1] = self.i0_bits(c).to(torch.float64) * 2.0 ** -43
        dw.s_init[0] = 1.0 - dw.s_init[1]
        dw.Ps_init = f(b.Ps_init).index_select(1, r)
        for ch, row, v in self.planted:
            dw.Ps_init[row, ch] = v
        dw.s_final, dw.Ps_final, dw.Q = (f(a).index_select(1, r) for a in (b.s_final, b.Ps_final, b.Q))

        def series(mode, a):
            t = f(a)
            if mode == "own":
                return t.index_select(t.dim() - 1, r), None
            if mode == "one":
                return t[..., :1].contiguous(), torch.zeros(self.B, dtype=torch.int32, device=dev)
            return t, r.to(torch.int32)
        dw.x, dw.x_series = series(self.x_mode, b.x)
        dw.R_series = None if b.R_series is None else series(self.x_mode, b.R_series)[0]
        dw.R_scalar = None if b.R_scalar is None else f(b.R_scalar).index_select(0, r)
        if self.u_mode == "table":
            Su = self.Su_table
            umax = torch.as_tensor(b.prm[L.PRM_U_MAX:L.PRM_U_MAX + b.n_npi, 0].astype(np.int64), device=dev)
            kk, ss = torch.arange(b.n_npi, dtype=torch.int64, device=dev)[:, None], torch.arange(Su, dtype=torch.int64, device=dev)[None, :]
            dw.u = torch.empty((b.T, b.n_npi, Su), dtype=torch.float64, device=dev)
            for t in range(b.T):                                 # a day at a time: the hash's temporaries stay small
                if np.isnan(b.u[t, 0, 0]):
                    dw.u[t] = float("nan")
                else:
                    dw.u[t] = self.table_level(t, kk, ss, umax[:, None]).to(torch.float64)
            dw.u_series = self.table_series(c).to(torch.int32)
        else:
            dw.u, dw.u_series = series(self.u_mode, b.u)
        dw.Sx, dw.Su = dw.x.shape[1], dw.u.shape[2]
        dw.r_mode, dw.q_mode = (1 if b.R_series is not None else 0), 0
        return dw

    def inputs_of(self, dw, idx):
        """The per-chain inputs of chains `idx` as the device holds them, in host_workload's form (for the bit-for-bit check of
        the two evaluations before a run)."""
        import torch
        sel = torch.as_tensor(np.asarray(idx, dtype=np.int64), device=dw.device)
        g = lambda t: t.index_select(t.dim() - 1, sel).cpu().numpy()
        d = {k: g(getattr(dw, k)) for k in ("prm", "s_init", "Ps_init", "s_final", "Ps_final", "Q")}
        if dw.R_scalar is not None:
            d["R_scalar"] = g(dw.R_scalar)
        if self.x_mode != "own":
            d["x_series"] = g(dw.x_series)
        if self.u_mode not in ("own", "table"):
            d["u_series"] = g(dw.u_series)
        if self.x_mode == "own":
            d["x"] = g(dw.x)
            if dw.R_series is not None:
                d["R_series"] = g(dw.R_series)
        if self.u_mode == "own":
            d["u"] = g(dw.u)
        if self.u_mode == "table":               # the series each sampled chain reads, whole
            us = g(dw.u_series).astype(np.int64)
            d["u_of_chain"] = dw.u.index_select(2, torch.as_tensor(us, device=dw.device)).cpu().numpy()
        return d


def chain_offsets(c, rows, B, blk):
    """Byte offsets [rows, n] of chains c within ONE day of a `rows`-row fp64 array: blocked layout [nblk][rows][blk] when
    blk < B, else classic [rows][B]."""
    c = np.asarray(c, dtype=np.int64)
    row = np.arange(rows, dtype=np.int64)[:, None]
    if blk >= B:
        return (row * B + c[None]) * 8
    return ((c // blk)[None] * rows * blk + row * blk + (c % blk)[None]) * 8


def extreme_sample(B, blk, units=(), n_spread=200, rows=(36, 21), itemsize=8):
    """The chains a test at an addressing limit compares against the oracle: 0, 1, B-2, B-1; both sides of the boundary
    nearest to B/2 and to B of every unit in `units` (layout block, wavefront, workgroup, chain range); for each row count in
    `rows`, both sides of the chain where the byte offset within a day slice first reaches 2^31 and 2^32 (any row), when the
    slice is that large; n_spread more by linspace.  Returns (idx, classes): classes maps a name to the chains of that class."""
    cls = {"ends": [0, 1, B - 2, B - 1]}
    for u in sorted(set(int(v) for v in units if 1 < v < B)):
        near = []
        for target in (B // 2, B):
            k = max(1, min((B - 1) // u, int(round(target / u))))
            near += [k * u - 1, k * u, k * u + 1]
        cls["unit%d" % u] = near
    for r in rows:
        for bit in (31, 32):
            lim = (1 << bit) // (itemsize)             # element index within the day slice
            if blk >= B:                                # classic: element = row * B + c; the first row that reaches it
                hits = [lim - row * B for row in range(r) if 0 <= lim - row * B < B]
            else:                                       # blocked: element = cb * r * blk + row * blk + cr
                cb = lim // (r * blk)
                hits = [cb * blk + d for d in (0, blk - 1)] + [(cb + 1) * blk]
                hits = [h for h in hits if h < B]
                if lim >= ((B + blk - 1) // blk) * r * blk:
                    hits = []
            if hits:
                cls["rows%d_bit%d" % (r, bit)] = sorted({h + d for h in hits for d in (-1, 0, 1)})
    cls["spread"] = np.linspace(0, B - 1, n_spread).astype(np.int64).tolist()
    idx = np.unique(np.concatenate([np.asarray(v, dtype=np.int64) for v in cls.values()]))
    idx = idx[(idx >= 0) & (idx < B)]
    return idx, {k: [int(x) for x in v if 0 <= x < B] for k, v in cls.items()}


def poison_runner(r):
    """Every output, the workspace and the extras of an EkfRunner filled with the poison patterns."""
    import torch
    for t in list(r.out.values()) + [r.ws]:
        if t.dtype == torch.float32:
            t.view(torch.int32).fill_(POISON32)
        else:
            t.view(torch.int64).fill_(POISON64)
    if r.pinv_rank is not None:
        r.pinv_rank.fill_(POISON_RANK)
        r.status.fill_(POISON_STATUS)


def surviving_poison(r):
    """{name: count} of the words of every selected output (pinv_rank and status included) that still hold the poison pattern
    after a run, over the WHOLE batch -- the lanes a blocked layout pads the last block with are not outputs and not counted."""
    import torch
    B, blk, nblk = r.dw.B, r.blk, r.nblk
    left = {}
    tensors = dict(r.out)
    if r.pinv_rank is not None:
        tensors["pinv_rank"], tensors["status"] = r.pinv_rank, r.status
    for name, t in tensors.items():
        n = 0
        if name == "status":
            n = int((t == POISON_STATUS).sum())
        else:
            for day in range(t.shape[0]):
                s = t[day]
                if s.dtype == torch.int32:
                    hit = s == POISON_RANK
                elif s.dtype == torch.float32:
                    hit = s.view(torch.int32) == POISON32
                else:
                    hit = s.view(torch.int64) == POISON64
                if blk < B and s.dim() == 3:                    # [nblk, rows, blk]
                    n += int(hit[:nblk - 1].sum()) + int(hit[nblk - 1, :, :B - (nblk - 1) * blk].sum())
                else:                                           # [rows, B] or [B (padded)]
                    n += int(hit[..., :B].sum())
        if n:
            left[name] = n
    return left


def sampled_output(r, name, idx):
    """[T, rows, n] ([T, n]) NumPy array of chains idx of output `name` (or "pinv_rank"), gathered on the device from the
    layout run() wrote -- the offsets restated here (chain_offsets), without a copy of the whole array."""
    import torch
    t = r.pinv_rank if name == "pinv_rank" else r.out[name]
    dev = t.device
    B, blk = r.dw.B, r.blk
    T = t.shape[0]
    if t.dim() == 2:
        return t.index_select(1, torch.as_tensor(np.asarray(idx, dtype=np.int64), device=dev)).cpu().numpy()
    rows = t.shape[-2]
    pos = chain_offsets(idx, rows, B, blk) // 8
    got = t.reshape(T, -1).index_select(1, torch.as_tensor(pos.reshape(-1), device=dev))
    return got.reshape(T, rows, len(idx)).cpu().numpy()


# ---------------------------------------------------------------- the calls around the filter at their launch and offset limits
# (tests/test_gpu_addressing_limits.py part B, tests/test_gpu_call_limits.py)
def poisoned(shape, dtype, device):
    """A device tensor filled with the poison pattern of its type: POISON64 (float64), POISON32 (float32), POISON_RANK (integers)."""
    import torch
    t = torch.empty(shape, dtype=dtype, device=device)
    if dtype == torch.float64:
        t.view(torch.int64).fill_(POISON64)
    elif dtype == torch.float32:
        t.view(torch.int32).fill_(POISON32)
    else:
        t.fill_(POISON_RANK)
    return t


def holds_poison(t):
    """Does any word of `t` (a tensor poisoned() made) still hold its poison pattern?"""
    import torch
    if t.dtype == torch.float64:
        return bool((t.view(torch.int64) == POISON64).any())
    if t.dtype == torch.float32:
        return bool((t.view(torch.int32) == POISON32).any())
    return bool((t == POISON_RANK).any())


def need_free(device, need):
    """Fail the test, with the numbers, if fewer than `need` bytes of device memory are free; reset the peak statistics."""
    import pytest
    import torch
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info(device)
    if free < need:
        pytest.fail(f"needs ~{need / 2**30:.1f} GiB of device memory, {free / 2**30:.1f} of {total / 2**30:.1f} GiB are free")
    torch.cuda.reset_peak_memory_stats(device)


def formula_rows(L_, R, device, fn, dtype):
    """[L_, R] tensor whose row t is fn(t * R + arange(R)), a row at a time (the hash's temporaries stay small)."""
    import torch
    out = torch.empty((L_, R), dtype=dtype, device=device)
    c = torch.arange(R, dtype=torch.int64, device=device)
    for t in range(L_):
        out[t] = fn(c + t * R).to(dtype)
    return out


def crossing_regions(rows, R, bits=(31, 32), itemsize=8):
    """Columns of a [rows, R] array on both sides of the element whose byte offset first reaches 2^bit."""
    reg = []
    for b in bits:
        e = (1 << b) // itemsize
        if e < rows * R:
            reg += [(e % R) + d for d in (-2, -1, 0, 1)]
    return [q for q in reg if 0 <= q < R]


def boundary_items(unit, count):
    """Items k * unit - 2 .. k * unit + 1 around every launch-slice boundary k * unit < count of a call that starts `unit` items
    per launch."""
    return [k * unit + d for k in range(1, (count - 1) // unit + 1) for d in (-2, -1, 0, 1) if 0 <= k * unit + d < count]


def as_f64(a):
    """an integer array of the formulas (NumPy or torch) as float64"""
    return a.astype(np.float64) if isinstance(a, np.ndarray) else a.double()


def hash_pos(c, k):
    """1 .. 2^20 from stream k of the hash"""
    return (chain_hash(c, k) >> 12) + 1


def hash_sgn(c, k):
    """-2^19 .. 2^19 - 1"""
    return (chain_hash(c, k) >> 12) - (1 << 19)


def bits_equal(g, w):
    """bit for bit, any NaN equal to any NaN; integers: the same values"""
    g, w = np.asarray(g), np.asarray(w)
    if g.shape != w.shape or g.dtype != w.dtype:
        return False
    if g.dtype.kind != "f":
        return bool(np.array_equal(g, w))
    u = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
    ng, nw = np.isnan(g), np.isnan(w)
    return bool(np.array_equal(ng, nw) and np.array_equal(g.view(u)[~ng], w.view(u)[~nw]))


def both_sides(sample, items, of=lambda i: i):
    """every launch-boundary item's region / day is in the sample"""
    return bool(items) and {int(of(i)) for i in items} <= sample


def poison_words(t, int_poison):
    """how many words of output `t` still hold the poison pattern of its type (count_nonzero: no int64 copy of the mask)"""
    import torch
    if t.dtype == torch.float64:
        hit = t.view(torch.int64) == POISON64
    elif t.dtype == torch.float32:
        hit = t.view(torch.int32) == POISON32
    else:
        hit = t == int_poison
    return int(torch.count_nonzero(hit))


def passed_bits(nbytes, bits=(31, 32, 33)):
    """which of the byte offsets 2^bit lie inside an array of nbytes bytes"""
    return [b for b in bits if nbytes > (1 << b)]


def region_columns(reg, D):
    """the columns reg[j] * D .. reg[j] * D + D - 1 of an array [rows, R * D], region after region"""
    reg = np.asarray(reg, dtype=np.int64)
    return (reg[:, None] * D + np.arange(D, dtype=np.int64)[None]).reshape(-1)


def formula_sample(rows, N, cols, fn, dtype=np.float64):
    """[rows, len(cols)]: what formula_rows(rows, N, ...) holds in the columns `cols`, evaluated by NumPy"""
    cols = np.asarray(cols, dtype=np.int64)
    return np.asarray(fn(np.arange(rows, dtype=np.int64)[:, None] * N + cols[None])).astype(dtype)


def replaced(cond, value, v):
    """v with the constant `value` where cond holds (NumPy or torch: the formulas' non-finite entries)"""
    if isinstance(v, np.ndarray):
        return np.where(cond, value, v)
    import torch
    return torch.where(cond, torch.full_like(v, value), v)


def poisoned_words(count, device):
    """a workspace of `count` doubles, every 64-bit word POISON64"""
    import torch
    t = torch.empty(int(count), dtype=torch.float64, device=device)
    t.view(torch.int64).fill_(POISON64)
    return t


def selected(t, sel):
    """the columns `sel` (a device index tensor) of the last axis of t, as NumPy"""
    return t.index_select(t.dim() - 1, sel).cpu().numpy()


def report_limits(what, t_call, t_case, device):
    """the [limits] line of a case: the library call alone, the whole case since time.perf_counter() gave `t_case`, peak memory"""
    import time
    import torch
    peak = torch.cuda.max_memory_allocated(device)
    print(f"[limits] {what}: call {t_call:.2f} s, case {time.perf_counter() - t_case:.1f} s, peak {peak / 2**30:.1f} GiB")


# ---------------------------------------------------------------- the pieces the cases of tests/test_gpu_newer_call_limits.py share
LIMIT_BITS = (31, 32, 33)


def dyadic10(k):
    """a formula: stream k of the hash as a dyadic value"""
    return lambda c: as_f64(hash_pos(c, k)) * 2.0 ** -10                # (0, 1024], 20 significant bits: exact in float too


def with_nan(fn, k, every):
    """fn, with a NaN where stream k of the hash is a multiple of `every`"""
    return lambda c: replaced(chain_hash(c, k) % every == 0, float("nan"), fn(c))


def assert_passes(nbytes, passes):
    """nbytes: {name: bytes} of EVERY array of the call; passes: {name: bits} -- every array not named stays below 2^31"""
    assert {k: passed_bits(v, LIMIT_BITS) for k, v in nbytes.items()} == {k: list(passes.get(k, ())) for k in nbytes}, \
        {k: passed_bits(v, LIMIT_BITS) for k, v in nbytes.items() if passed_bits(v, LIMIT_BITS)}


def crossing_sample(rows, N, itemsize, nbytes_passes, of=lambda c: c):
    """the regions of of(column), -1 .. +1, on both sides of every 2^bit crossing of an array seen as [rows, N]"""
    cols = crossing_regions(rows, N, bits=LIMIT_BITS, itemsize=itemsize)
    assert len(cols) == 4 * len(nbytes_passes), (rows, N, itemsize, cols)
    return sorted({of(c) + d for c in cols for d in (-1, 0, 1)})


def region_sample(R, n_spread, *more):
    """sorted sampled regions: 0, 1, R - 2, R - 1, a spread, and the lists `more`, each of which must lie inside 0 .. R - 1 or
    is clipped to it; asserts that the ends and the spread are held"""
    reg, cls = extreme_sample(R, R, n_spread=n_spread, rows=())
    reg = np.unique(np.concatenate([reg] + [np.asarray(m, dtype=np.int64) for m in more]).astype(np.int64))
    reg = reg[(reg >= 0) & (reg < R)]
    S = set(reg.tolist())
    assert {0, 1, R - 2, R - 1} <= S and set(cls["spread"]) <= S
    return reg, S


def assert_no_poison(out):
    """rule 2: no word of any tensor of `out` (made by poisoned() / poisoned_words()) still holds its poison pattern"""
    left = {k: poison_words(t, POISON_RANK) for k, t in out.items()}
    assert not any(left.values()), ("outputs that still hold the poison pattern (words)", left)


def compare_sample(out, want, sel, reg):
    """rule 3: the columns of every output that belong to the sampled regions against the restatement"""
    assert set(out) <= set(want), (sorted(out), sorted(want))
    for k, t in out.items():
        got, w = selected(t, sel[k] if isinstance(sel, dict) else sel), want[k]
        if not bits_equal(got, w):
            assert got.shape == w.shape and got.dtype == w.dtype, (k, got.shape, w.shape, got.dtype, w.dtype)
            bad = ~((got == w) | ((got != got) & (w != w)))
            cols = np.flatnonzero(bad.reshape(-1, bad.shape[-1]).any(axis=0))
            n = got.shape[-1] // reg.size
            raise AssertionError((k, "regions", reg[np.unique(cols // n)][:12].tolist(), "words", int(bad.sum())))


def timed_device_call(entry, dev, *args):
    """the device entry `entry` of the library with `args`, the current stream and an error buffer: seconds of the call"""
    import ctypes as C
    import time
    import torch
    from epidemicmodeling_amd import _lib
    err = C.create_string_buffer(256)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    rc = getattr(_lib.lib(), entry)(*args, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), err)
    _lib.check(rc, err)
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def cycled_population(R, dev):
    """[R] on the device and the 16 values it cycles through (the ens_summary limits case does the same)"""
    import torch
    from epidemicmodeling_amd import synth
    N16 = synth.make_regions(16)["N"].astype(np.float64)
    return torch.as_tensor(N16, device=dev).index_select(0, torch.arange(R, dtype=torch.int64, device=dev) % 16), N16


def scaled_rows(fn, rows_out, scale_row, scale):
    """fn over an array [n, rows_out, R] flattened to [n * rows_out, R], the rows `scale_row` of every n times `scale` (a power of
    two: exact) -- the truths and thresholds of the derived row live at N_r v^3"""
    def on_device(n, R, dev):
        import torch
        t = formula_rows(n * rows_out, R, dev, fn, torch.float64).reshape(n, rows_out, R)
        t[:, scale_row] *= scale
        return t

    def on_host(n, R, reg):
        t = formula_sample(n * rows_out, R, reg, fn).reshape(n, rows_out, reg.size)
        t[:, scale_row] *= scale
        return t
    return on_device, on_host


# ---------------------------------------------------------------- whole-batch comparisons of the full-size runs
# ("Every chain of the full-size runs").  The equality is the suite's np.array_equal(..., equal_nan=True): NaN equals
# NaN whatever its payload, +0 equals -0, nothing else is equal that is not the same number.  words_equal() is that rule element
# by element on torch tensors, so that it can be evaluated where the data lies (tests/test_whole_batch_helpers.py holds it
# against NumPy's).
def words_equal(a, b):
    """bool tensor: a[i] and b[i] are the same number, or both NaN (integers: the same value)."""
    import torch
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    eq = a == b
    if a.dtype.is_floating_point:
        eq |= torch.isnan(a) & torch.isnan(b)
    return eq


def _runner_tensors(r, names=None, status=False):
    """{name: tensor}: names=None -- every output the runner holds (in OUT_NAMES order) and pinv_rank; else exactly `names`.
    status=True adds the per-chain status words."""
    if names is None:
        d = {n: r.out[n] for n in OUT_NAMES if n in r.out}
        if r.pinv_rank is not None:
            d["pinv_rank"] = r.pinv_rank
    else:
        d = {n: (r.pinv_rank if n == "pinv_rank" else r.out[n]) for n in names}
    assert d and all(t is not None for t in d.values()), (names, list(r.out))
    if status and r.status is not None:
        d["status"] = r.status
    return d


def chain_slice(t, lo, hi, B, blk):
    """[T', rows, hi - lo] ([T', hi - lo]) of chains [lo, hi) of an output in the runner's layout -- classic [T', rows, B] /
    [T', B (padded)] or blocked [T', nblk, rows, blk]; lo a multiple of blk when blocked.  Only the blocks that hold the range
    are unblocked (a copy of that slice, never of the array)."""
    if t.dim() == 2 or blk >= B:
        return t[..., lo:hi]
    assert lo % blk == 0, (lo, blk)
    s = t[:, lo // blk:(hi + blk - 1) // blk]
    T, nb, rows, _ = s.shape
    return s.permute(0, 2, 1, 3).reshape(T, rows, nb * blk)[:, :, :hi - lo]


def chain_ranges(B, blk, chunk):
    """[(lo, hi)] that cover chains 0 .. B-1 exactly once, at most `chunk` chains each (one layout block where a block is larger),
    every lo a multiple of the layout block `blk` (blk >= B: classic layout, any start)."""
    step = int(chunk) if blk >= B else max(blk, int(chunk) // blk * blk)
    assert step >= 1
    return [(lo, min(B, lo + step)) for lo in range(0, B, step)]


def describe_mismatch(name, got, ref, lo, day0, blk, B, what, first=6):
    """The failure message of a whole-batch comparison.  got / ref: NumPy arrays [T', rows, n] ([T', n]) of chains lo .. lo+n-1
    and days day0 .. day0+T'-1 that differ somewhere."""
    g3, r3 = (a[:, None, :] if a.ndim == 2 else a for a in (got, ref))
    with np.errstate(invalid="ignore"):
        bad = ~((g3 == r3) | ((g3 != g3) & (r3 != r3)))
    chains = np.flatnonzero(bad.any(axis=(0, 1)))
    cells = np.argwhere(bad.transpose(2, 0, 1))              # (chain, day, row), chain-major
    lines = []
    for c, d, row in cells[:first]:
        lines.append("(chain %d, day %d, row %d): got %r, expected %r" % (lo + c, day0 + d, row, g3[d, row, c].item(), r3[d, row, c].item()))
    msg = "%s: %s differs in %d chain(s) of [%d, %d), %d word(s)" % (what, name, chains.size, lo, lo + g3.shape[2], int(bad.sum()))
    if blk < B:
        badc, n = bad.any(axis=(0, 1)), g3.shape[2]
        blocks = np.unique((lo + chains) // blk)
        whole = [int(b) for b in blocks if b * blk >= lo and min(B, (b + 1) * blk) <= lo + n
                 and badc[b * blk - lo:min(B, (b + 1) * blk) - lo].all()]
        msg += "; layout blocks (chain // %d): %s%s" % (blk, blocks[:12].tolist(), " ..." if blocks.size > 12 else "")
        msg += ("; EVERY chain of block(s) %s" % whole[:12]) if whole else "; no block differs in all its chains"
    days = day0 + np.flatnonzero(bad.any(axis=(1, 2)))
    msg += "; days %d .. %d (%d of them)" % (days.min(), days.max(), days.size)
    return msg + "\n  " + "\n  ".join(lines)


def all_chains_equal_oracle(r, w, names=None, chunk=2400, what=""):
    """EVERY chain of runner `r`'s outputs (and pinv_rank) against the C oracle's run of Workload `w`, bit for bit: the batch is
    walked in chain ranges that start on layout blocks and cover 0 .. B-1 exactly once; per range the oracle runs those chains
    alone, its arrays go to where the outputs lie and are compared there with words_equal (fp32 storage: against the oracle's
    result rounded once).  Host memory is bounded by the range (2 400 six-state chains x 520 days x all outputs: 1.6 GB).  The
    first range that differs fails the call -- no further range is run -- with the output, the number of differing chains, the
    first (chain, day, row) with both values and the layout blocks they fall in.  The number of chains compared is asserted to be
    w.B: no chain may be left out.  Returns {"chains", "ranges", "oracle_s", "transfer_s", "compare_s"} (and prints it)."""
    import time
    import torch
    B, blk = r.dw.B, r.blk
    assert B == w.B, (B, w.B)
    tensors = _runner_tensors(r, names)
    stat = {"chains": 0, "ranges": 0, "oracle_s": 0.0, "transfer_s": 0.0, "compare_s": 0.0}
    dev = next(iter(tensors.values())).device
    sync = (lambda: torch.cuda.synchronize(dev)) if dev.type == "cuda" else (lambda: None)
    seen_to = 0
    for lo, hi in chain_ranges(B, blk, chunk):
        assert lo == seen_to and hi > lo and (blk >= B or lo % blk == 0), (lo, hi, seen_to, blk)
        t0 = time.perf_counter()
        ref = oracle_batch(w.select(np.arange(lo, hi)))
        stat["oracle_s"] += time.perf_counter() - t0
        for name, t in tensors.items():
            assert name in ref, name
            e = ref[name].astype(np.float32) if t.dtype == torch.float32 else ref[name]
            t0 = time.perf_counter()
            exp = torch.from_numpy(np.ascontiguousarray(e)).to(dev)
            sync()
            t1 = time.perf_counter()
            got = chain_slice(t, lo, hi, B, blk)
            assert got.shape == exp.shape and got.shape[-1] == hi - lo, (name, got.shape, exp.shape)
            same = bool(words_equal(got, exp).all())
            t2 = time.perf_counter()
            stat["transfer_s"] += t1 - t0
            stat["compare_s"] += t2 - t1
            if not same:
                raise AssertionError(describe_mismatch(name, got.cpu().numpy(), e, lo, 0, blk, B, what or "against the oracle"))
            del exp, got
        stat["chains"] += hi - lo
        stat["ranges"] += 1
        seen_to = hi
    assert stat["chains"] == w.B and seen_to == w.B, (stat["chains"], w.B)
    print("all_chains_equal_oracle%s: %d of %d chains in %d ranges equal the oracle in %s; oracle %.1f s, transfers %.1f s, compare %.1f s"
          % (" [" + what + "]" if what else "", stat["chains"], w.B, stat["ranges"], ", ".join(tensors), stat["oracle_s"],
             stat["transfer_s"], stat["compare_s"]))
    return stat


def snapshot_outputs(r):
    """Clones of every output of a runner, pinv_rank and status, where they lie (what device_outputs_equal compares against)."""
    return {n: t.clone() for n, t in _runner_tensors(r, status=True).items()}


def snapshot_views(r):
    """The same dict of the runner's own tensors, not clones (to hold ANOTHER runner against, e.g. fp32 storage against fp64)."""
    return dict(_runner_tensors(r, status=True))


def device_outputs_equal(r, saved, days=8, rounded=False, what=""):
    """Every word of every output of runner `r` (pinv_rank and status too) against `saved` -- clones taken earlier
    (snapshot_outputs), or another runner's tensors of the same layout -- with words_equal, evaluated where the tensors lie, `days`
    days at a time (the temporaries stay small).  The lanes a blocked layout pads its last block with are not outputs and not
    compared.  rounded=True: `saved` holds fp64 results and `r` fp32 storage; each saved word is rounded once first.  The first
    output that differs fails the call, in all_chains_equal_oracle's terms.  Returns {"chains", "words", "compare_s"}."""
    import time
    import torch
    B, blk = r.dw.B, r.blk
    tensors = _runner_tensors(r, status=True)
    assert set(tensors) == set(saved), (sorted(tensors), sorted(saved))
    dev = next(iter(tensors.values())).device
    t0 = time.perf_counter()
    words = 0
    for name, t in tensors.items():
        s = saved[name]
        assert s.shape == t.shape and s.device == t.device and s.data_ptr() != t.data_ptr(), name
        assert s.dtype == t.dtype or (rounded and t.dtype == torch.float32 and s.dtype == torch.float64), (name, s.dtype, t.dtype)
        if name == "status":
            a, b = t[None, :B], s[None, :B]               # one "day"
        else:
            a, b = t, s
        for d0 in range(0, a.shape[0], days):
            ga, gb = (chain_slice(x[d0:d0 + days], 0, B, B, blk) for x in (a, b))
            if gb.dtype != ga.dtype:
                gb = gb.to(ga.dtype)
            assert ga.shape[-1] == B
            words += ga.numel()
            if not bool(words_equal(ga, gb).all()):
                bad = (~words_equal(ga, gb)).reshape(ga.shape[0], -1, B).any(dim=1).any(dim=0)
                c0 = int(torch.nonzero(bad)[0])
                lo = c0 if blk >= B else c0 // blk * blk
                hi = min(B, lo + max(blk if blk < B else 0, 2400))
                raise AssertionError(describe_mismatch(name, ga[..., lo:hi].cpu().numpy(), gb[..., lo:hi].cpu().numpy(), lo, d0, blk, B,
                                                       (what or "against the saved outputs") + " (%d chain(s) of the batch differ in these days)"
                                                       % int(bad.sum())))
            del ga, gb
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    stat = {"chains": B, "words": words, "compare_s": time.perf_counter() - t0}
    print("device_outputs_equal%s: %d chains, %d words in %s equal; %.1f s"
          % (" [" + what + "]" if what else "", B, words, ", ".join(tensors), stat["compare_s"]))
    return stat

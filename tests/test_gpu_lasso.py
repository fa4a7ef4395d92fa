"""The cross-validated LASSO on the device (epi_lasso_run_device / _host, batch.lasso_cv and the pipeline's
regression="lasso"): every output, status, iteration count and index bit-identical to the C restatement
tests/lasso_ref.c."""
import ctypes as C

import numpy as np
import pytest

from tests.lasso_ref import LassoRef, ST_BAD_FOLDS, ST_MAXITER, ST_NONFINITE, ST_NULL_MODEL, ST_OK
from tests.test_lasso_host import make_problem

pytestmark = pytest.mark.gpu

I32_FILL = -12345


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return LassoRef(tmp_path_factory.mktemp("lasso_ref_gpu"))


def _run_device(X, y, fold, K, NL, ratio=1e-4, rel_tol=1e-4, max_iter=100000, device="cuda:0"):
    """epi_lasso_run_device on NaN-filled outputs (int outputs filled with I32_FILL)"""
    import torch
    from epidemicmodeling_amd import _lib
    dev = torch.device(device)
    D, n, R = X.shape
    Xd = torch.as_tensor(np.ascontiguousarray(X), device=dev)
    yd = torch.as_tensor(np.ascontiguousarray(y), device=dev)
    fd = None if K < 2 else torch.as_tensor(np.ascontiguousarray(fold, dtype=np.int32), device=dev)
    out = {}
    for k, sh in _lib.lasso_shapes(R, D, n, K, NL).items():
        if k in _lib.LASSO_OUT_I32:
            out[k] = torch.full(sh, I32_FILL, dtype=torch.int32, device=dev)
        else:
            out[k] = torch.full(sh, float("nan"), dtype=torch.float64, device=dev)
    outs = _lib.LassoOutputs()
    for k in _lib.LASSO_OUT_NAMES:
        setattr(outs, k, None if k not in out else C.c_void_p(out[k].data_ptr()))
    d = _lib.make_lasso_desc(R, D, n, K, NL, ratio, rel_tol, max_iter)
    err = C.create_string_buffer(256)
    st = torch.cuda.current_stream(dev)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = _lib.lib().epi_lasso_run_device(C.byref(d), ptr(Xd), ptr(yd), ptr(fd), C.byref(outs), C.c_void_p(st.cuda_stream), err)
    _lib.check(rc, err)
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same(got, want):
    assert set(got) == set(want), (set(got), set(want))
    for k in want:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, k
        if w.dtype == np.float64:
            nan = np.isnan(w)
            assert np.array_equal(np.isnan(g), nan), k
            assert np.array_equal(g[~nan].view(np.int64), w[~nan].view(np.int64)), k      # bit for bit, -0 / +0 included
        else:
            assert np.array_equal(g, w.astype(g.dtype)), k


CASES = [  # R, n, D, K, NL, max_iter
    (1, 5, 60, 10, 100, 100000),
    (63, 12, 60, 50, 100, 100000),
    (64, 1, 2, 2, 1, 100000),
    (65, 5, 256, 63, 100, 100000),
    (236, 12, 60, 50, 100, 100000),
    (65, 12, 60, 0, 100, 100000),
    (64, 5, 60, 10, 20, 3),
    (63, 12, 256, 2, 1, 100000),
    (236, 1, 60, 0, 1, 100000),
]


@pytest.mark.parametrize("R, n, D, K, NL, max_iter", CASES)
def test_bit_identical_to_reference(gpu_device, ref, R, n, D, K, NL, max_iter):
    X, y, fold = make_problem(R, D, n, K, seed=R * 7 + n + D + K)
    got = _run_device(X, y, fold, K, NL, max_iter=max_iter, device=gpu_device)
    want = ref.run(X, y, fold, K, NL, max_iter=max_iter)
    _same(got, want)
    st = set(got["status"].tolist())
    if R >= 5 and K >= 2:
        assert {ST_NULL_MODEL, ST_NONFINITE} <= st
    if max_iter == 3:
        assert ST_MAXITER in st
    if R >= 63 and NL == 100 and D == 60:
        assert ST_OK in st and (got["df"] > 0).any()


def test_bad_folds_on_the_device(gpu_device, ref):
    X, y, fold = make_problem(8, 40, 5, 6, seed=5, specials=False)
    fold[fold[:, 2] == 5, 2] = 0            # region 2: fold 5 empty
    fold[7, 6] = 9                          # region 6: value outside 0 .. K-1
    got = _run_device(X, y, fold, 6, 30, device=gpu_device)
    assert got["status"][2] == ST_BAD_FOLDS and got["status"][6] == ST_BAD_FOLDS
    assert (np.delete(got["status"], [2, 6]) == ST_OK).all()
    _same(got, ref.run(X, y, fold, 6, 30))


def test_batch_and_host_entries_equal_the_device_entry(gpu_device, ref):
    import torch
    from epidemicmodeling_amd import batch, hostapi
    X, y, fold = make_problem(70, 60, 12, 50, seed=9)
    dev = _run_device(X, y, fold, 50, 100, device=gpu_device)
    b = {k: v.cpu().numpy() for k, v in batch.lasso_cv(X, y, K=50, folds=fold, device=gpu_device).items()}
    torch.cuda.synchronize()
    h = hostapi.lasso_cv(X, y, K=50, folds=fold)
    _same(b, dev)
    _same(h, dev)
    # the default partition is lasso_folds(D, K, R, seed)
    _same(hostapi.lasso_cv(X, y, K=50, seed=3), hostapi.lasso_cv(X, y, K=50, folds=batch.lasso_folds(60, 50, 70, 3)))


def _lasso_region_fits(ref, X, alpha, D, K, seed):
    y = np.ascontiguousarray(alpha[-D:])
    return ref.run(X, y, __import__("epidemicmodeling_amd").batch.lasso_folds(D, K, X.shape[2], seed), K, 100)


def _check_front_half(ref, out, raw, N, T, D, K, seed, H):
    """re-derive preprocessing, both EKF rounds and both LASSO fits from the previous stage (oracle + tests/lasso_ref)"""
    from epidemicmodeling_amd import pipeline, synth
    from oracle import oracle_lib as olib
    S = N.shape[0]
    pre = out["pre"]
    for r in range(S):
        p = olib.preprocess_region(raw["cases"][:T, r], raw["deaths"][:T, r], N[r])
        assert np.array_equal(pre["x_new"][:, r], p["x_new"]) and np.array_equal(pre["R_v"][:, r], p["R_v"])
    x, R, u, I0 = pre["x_new"], pre["R_v"], pre["ip_filled"], pre["I0"]
    n = u.shape[1]
    o1 = H.oracle_batch(pipeline.workload3(x, R, np.zeros_like(u), N, I0, np.zeros((n, S)), np.zeros(S)), outputs=["S_SMOOTH"])
    assert np.array_equal(out["alpha_round1"], o1["S_SMOOTH"][:, 2])
    X = synth.IP_MAXES[None, :n, None] - u[T - D:]
    assert np.array_equal(out["X_reg"], X)
    f1 = _lasso_region_fits(ref, X, out["alpha_round1"], D, K, seed)
    _same({k: out["fit1"][k] for k in f1}, f1)
    o2 = H.oracle_batch(pipeline.workload3(x, R, u, N, I0, out["fit1"]["a"], out["fit1"]["b"]), outputs=["S_SMOOTH"])
    assert np.array_equal(out["alpha_round2"], o2["S_SMOOTH"][:, 2])
    f2 = _lasso_region_fits(ref, X, out["alpha_round2"], D, K, seed + 1)
    _same({k: out["fit2"][k] for k in f2}, f2)
    for k in ("lambda", "mse", "se", "idx_min_mse", "idx_1se", "status"):
        assert k in out["fit1"] and k in out["fit2"]
    return f2


def test_prescription_pipeline_with_lasso_stage_by_stage(gpu_device, ref):
    """pipeline.prescribe(regression="lasso") on the region set of test_prescription_pipeline_stage_by_stage: every stage
    re-derived from the previous one (the filter oracle; tests/lasso_ref for both regressions) and the run reaches a
    prescription.  LASSO coefficients may be negative (the clamp of TrainPredictPrescribeNPI.m:261 is commented out):
    the 3-state EKF, the 6-state sweep and the scoring take them unchanged."""
    from tests import helpers as H
    from epidemicmodeling_amd import pipeline, synth
    S, T, H_, n_eps, D, K, seed = 7, 150, 25, 12, 50, 10, 4
    raw = synth.make_raw_counts(S, T, seed=31)
    raw["cases"][:, -1] = np.cumsum(np.full(T, 40.0))
    out = pipeline.prescribe(raw["cases"], raw["deaths"], raw["population"], raw["ip"], horizon=H_, n_eps=n_eps,
                             num_regression_days=D, device=gpu_device, regression="lasso", cv_folds=K, cv_seed=seed)
    N = raw["population"]
    _check_front_half(ref, out, raw, N, T, D, K, seed, H)
    os_ = H.oracle_batch(out["sweep"], outputs=["u_opt_smooth"])
    chains = np.arange(S) * n_eps + out["i_opt"]
    assert np.array_equal(out["prescription"], os_["u_opt_smooth"][T:][:, :, chains])
    n = raw["ip"].shape[1]
    assert out["prescription"].shape == (H_, n, S) and np.isfinite(out["prescription"]).all()
    assert np.isin(out["fit2"]["status"], [ST_OK, ST_NULL_MODEL]).all() and (out["fit2"]["status"] == ST_OK).any()
    # the default is untouched: NNLS results are what they were
    nn = pipeline.prescribe(raw["cases"], raw["deaths"], raw["population"], raw["ip"], horizon=H_, n_eps=n_eps,
                            num_regression_days=D, device=gpu_device)
    assert (nn["fit2"]["a"] >= 0).all() and "lambda" not in nn["fit2"]


def test_forecast_quality_with_lasso_stage_by_stage(gpu_device, ref):
    from tests import helpers as H
    from epidemicmodeling_amd import pipeline, synth
    S, LL, F, M, D, K, seed = 6, 140, 20, 10, 60, 50, 0
    raw = synth.make_raw_counts(S, LL, seed=17)
    raw["cases"][:, -1] = np.cumsum(np.full(LL, 40.0))
    out = pipeline.forecast_quality(raw["cases"], raw["deaths"], raw["population"], raw["ip"], F, max_lookahead=M,
                                    num_regression_days=D, device=gpu_device, regression="lasso")
    T = LL - F
    N = raw["population"]
    _check_front_half(ref, out, raw, N, T, D, K, seed, H)
    # the study downstream runs on the LASSO fit of round 2 exactly as it does on the NNLS fit
    w = out["workload"]
    n = raw["ip"].shape[1]
    from epidemicmodeling_amd import layout as L
    assert np.array_equal(w.prm[L.PRM_A:L.PRM_A + n], out["fit2"]["a"]) and np.array_equal(w.prm[L.PRM_B], out["fit2"]["b"])
    from tests import lookahead_ref as LR
    from tests.test_gpu_lookahead import ARRAYS, _same as same_tables
    same_tables(out, LR.expected(w, out["truth"], np.asarray(N, dtype=np.float64), F, M), ARRAYS)


# ---------------------------------------------------------------- every limit at once
LIMIT_CASES = [  # R, n, D, K, NL, max_iter
    (3, 12, 256, 63, 100, 100000),          # 63 fold lanes x 12 columns x 100 lambdas over 256 days: the LDS maximum
    (65, 12, 63, 63, 100, 100000),          # K = D: single-day folds, each fold lane trains on D - 1 days
    (3, 12, 256, 63, 100, 1),               # max_iter = 1 at the maximum shape
]


@pytest.mark.parametrize("R, n, D, K, NL, max_iter", LIMIT_CASES)
def test_bit_identical_at_the_limits(gpu_device, ref, R, n, D, K, NL, max_iter):
    if D == 256 and n == 12 and NL == 100:
        # lasso_lds_bytes (csrc/lasso.hpp): (D n + D + 64 D + 128 + 3 NL + 8) doubles + D ints, inside the 160 KiB of a CU
        assert (D * n + D + D * 64 + 128 + 3 * NL + 8) * 8 + D * 4 == 162208 <= 160 * 1024
    X, y, fold = make_problem(R, D, n, K, seed=R * 7 + n + D + K + max_iter)
    got = _run_device(X, y, fold, K, NL, max_iter=max_iter, device=gpu_device)
    _same(got, ref.run(X, y, fold, K, NL, max_iter=max_iter))
    if max_iter == 1:
        assert ST_MAXITER in set(got["status"].tolist())
    else:
        assert ST_OK in set(got["status"].tolist())


def _constant_on_one_training_set(R, D, K, f_const, seed):
    """make_problem without specials, then in every region: column 0 constant on the training set of fold f_const (it
    varies only on that fold's days), and day 0 moved into fold f_const (so that the column's first day is held out)."""
    from epidemicmodeling_amd import batch
    X, y, _ = make_problem(R, D, 6, 0, seed, specials=False)
    fold = batch.lasso_folds(D, K, R, seed)
    rng = np.random.default_rng(seed)
    for r in range(R):
        f0 = fold[0, r]
        if f0 != f_const:                     # swap day 0 with a day of fold f_const: fold sizes stay as they were
            i = np.flatnonzero(fold[:, r] == f_const)[0]
            fold[i, r], fold[0, r] = f0, f_const
        hold = fold[:, r] == f_const
        X[:, 0, r] = 3.0
        X[hold, 0, r] = 3.0 + rng.uniform(0.5, 2.0, hold.sum())
        y[:, r] += 0.05 * X[:, 0, r]
    return X, y, fold


@pytest.mark.parametrize("D, K", [(40, 5), (63, 63), (256, 63)])
def test_constant_column_on_the_last_folds_training_set(gpu_device, ref, D, K):
    """A column that is constant on the training set of fold K - 1 only (make_problem's special builds it for fold 0):
    that lane must drop the column, the other lanes and the full fit keep it."""
    X, y, fold = _constant_on_one_training_set(4, D, K, K - 1, seed=D + K)
    for r in range(4):
        train = fold[:, r] != K - 1
        assert X[train, 0, r].max() == X[train, 0, r].min() and X[:, 0, r].max() != X[:, 0, r].min()
    got = _run_device(X, y, fold, K, 100, device=gpu_device)
    _same(got, ref.run(X, y, fold, K, 100))
    assert np.isfinite(got["mse"]).all() and (got["status"] == ST_OK).all()


# ---------------------------------------------------------------- optional outputs: each alone, in a poisoned arena
LASSO_OPTIONAL = ("lambda", "B", "intercept", "df", "mse", "se", "iters", "idx_min_mse", "idx_1se")


@pytest.mark.parametrize("K", [0, 7])
@pytest.mark.parametrize("entry", ["device", "host"])
def test_each_output_alone(gpu_device, ref, K, entry):
    """epi_lasso_outputs may hold NULL for every output but status (and a, b when K >= 2).  Each optional output alone, and
    mse + se without B, comes back equal to the all-outputs run bit for bit; every byte outside the requested outputs keeps
    its poison (guards and never-requested neighbours)."""
    import torch
    from epidemicmodeling_amd import _lib
    from tests import helpers as H
    R, D, n, NL = 9, 50, 6, 20
    X, y, fold = make_problem(R, D, n, K, seed=31 + K)
    full = ref.run(X, y, fold, K, NL)
    shapes = _lib.lasso_shapes(R, D, n, K, NL)
    specs = [(k, shapes[k], np.int32 if k in _lib.LASSO_OUT_I32 else np.float64) for k in _lib.LASSO_OUT_NAMES if k in shapes]
    required = ("status", "a", "b") if K >= 2 else ("status",)
    subsets = [(k,) for k in LASSO_OPTIONAL if k in shapes] + ([("mse", "se", "lambda"), ("a", "b")] if K >= 2 else [("B", "df")])
    Xc, yc = np.ascontiguousarray(X), np.ascontiguousarray(y)
    fc = None if K < 2 else np.ascontiguousarray(fold, dtype=np.int32)
    if entry == "device":
        Xd, yd = torch.as_tensor(Xc, device=gpu_device), torch.as_tensor(yc, device=gpu_device)
        fd = None if fc is None else torch.as_tensor(fc, device=gpu_device)
    d = _lib.make_lasso_desc(R, D, n, K, NL)
    for sub in subsets:
        req = tuple(dict.fromkeys(required + sub))
        ar = H.GuardArena(specs, device=gpu_device if entry == "device" else None)
        outs = _lib.LassoOutputs()
        for k in _lib.LASSO_OUT_NAMES:
            setattr(outs, k, C.c_void_p(ar.ptr(k)) if k in req else None)
        err = C.create_string_buffer(256)
        if entry == "device":
            st = torch.cuda.current_stream(torch.device(gpu_device))
            rc = _lib.lib().epi_lasso_run_device(C.byref(d), C.c_void_p(Xd.data_ptr()), C.c_void_p(yd.data_ptr()),
                                                 None if fd is None else C.c_void_p(fd.data_ptr()), C.byref(outs),
                                                 C.c_void_p(st.cuda_stream), err)
        else:
            rc = _lib.lib().epi_lasso_run_host(C.byref(d), C.c_void_p(Xc.ctypes.data), C.c_void_p(yc.ctypes.data),
                                               None if fc is None else C.c_void_p(fc.ctypes.data), C.byref(outs), 0, err)
        _lib.check(rc, err)
        _same({k: ar.get(k) for k in req}, {k: full[k] for k in req})
        assert ar.untouched(req), sub


# ---------------------------------------------------------------- the device path against the optimality conditions
def test_device_path_meets_the_kkt_conditions_at_the_maximum_shape(gpu_device, ref):
    """test_lasso_host.py::test_path_meets_the_kkt_conditions on the GPU's B path at D = 256, n = 12, NL = 100 (with 63 fold
    lanes beside the full fit), with the same bound: at every lambda g = Xs' (Y0 - Xs b) / N equals lambda sign(b_j) where
    b_j != 0 and lies in [-lambda, lambda] where b_j = 0, up to RelTol sum_k |G_jk| (1 + |b_k|) (1 + RelTol) plus 1e-12 of the
    scale of g."""
    from tests.test_lasso_host import _standardized
    R, D, n, K = 4, 256, 12, 63
    X, y, fold = make_problem(R, D, n, K, seed=77, specials=False)
    got = _run_device(X, y, fold, K, 100, device=gpu_device)
    rel_tol = 1e-4
    for r in range(R):
        assert got["status"][r] == ST_OK
        Xs, Y0, sig, cst = _standardized(X[:, :, r], y[:, r])
        G = Xs.T @ Xs / D
        for k in range(100):
            lam = got["lambda"][k, r]
            b = got["B"][k, :, r] * sig
            g = Xs.T @ (Y0 - Xs @ b) / D
            bound = rel_tol * np.abs(G) @ ((1 + np.abs(b)) * (1 + rel_tol)) + 1e-12 * (np.abs(Xs).T @ np.abs(Y0) / D + lam)
            act = (b != 0) & ~cst
            assert np.all(np.abs(g[act] - lam * np.sign(b[act])) <= bound[act]), (r, k)
            zero = (b == 0) & ~cst
            assert np.all(np.abs(g[zero]) <= lam + bound[zero]), (r, k)


def test_device_cv_half_agrees_with_sklearn(gpu_device, ref):
    """The CV half against code this project did not write: every fold of every region refitted at every lambda with
    sklearn.linear_model.Lasso on the fold's own standardization, the held-out MSE and SE recomputed
    (tests/lasso_ref.py::sklearn_cv, whose docstring derives the gates from the KKT bound of the RelTol stopping rule and
    the strong convexity of each fold's objective).  The GPU's mse / se must lie within those gates, and idx_min_mse /
    idx_1se must be sklearn's wherever the MSE margin exceeds them.  RelTol 1e-8 makes the gates tight enough to decide
    indices."""
    pytest.importorskip("sklearn")
    from tests.lasso_ref import cv_indices_agree, sklearn_cv
    R, D, n, K, rel_tol = 6, 40, 6, 5, 1e-8
    X, y, fold = make_problem(R, D, n, K, seed=12, specials=False)
    got = _run_device(X, y, fold, K, 100, rel_tol=rel_tol, device=gpu_device)
    _same(got, ref.run(X, y, fold, K, 100, rel_tol=rel_tol))
    decided = gated = 0
    for r in range(R):
        assert got["status"][r] == ST_OK
        mse, se, g_mse, g_se = sklearn_cv(X[:, :, r], y[:, r], fold[:, r], K, got["lambda"][:, r], rel_tol)
        ok = ~np.isnan(g_mse)
        gated += ok.sum()
        assert np.all(np.abs(got["mse"][ok, r] - mse[ok]) <= g_mse[ok]), r
        assert np.all(np.abs(got["se"][ok, r] - se[ok]) <= g_se[ok]), r
        if ok.all():
            decided += cv_indices_agree(got["mse"][:, r], got["se"][:, r], g_mse, g_se, int(got["idx_min_mse"][r]),
                                        int(got["idx_1se"][r]), mse, se)
    assert gated >= 300 and decided > 0

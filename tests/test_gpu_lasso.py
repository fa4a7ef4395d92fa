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

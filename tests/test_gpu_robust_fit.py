"""The element-wise robust regression on the device (epi_robfit_run_device / _host, batch.robust_affine_fit and the pipeline's
regression="elementwise"): every output bit-identical to the C restatement tests/robust_fit_ref.c, any NaN equal to any NaN."""
import ctypes as C
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import robust_fit_ref as RF

pytestmark = pytest.mark.gpu

INF = np.inf
F64_POISON, I32_POISON, GUARD = -7777.25, -12345, 64

# the issue's shapes, plus D = 300: without it no shape runs the NV = 8 instantiation (256 < D <= 512)
SHAPES = list(itertools.product((3, 4, 63, 64, 65, 129, 300, 1024), (1, 12), (1, 5, 70)))
# both sides of every `<=` of rf_dispatch (64 | 128 | 256 | 512): 64 / 65 and 129 are above, these are the rest
SHAPES += [(D, 1, 5) for D in (128, 256, 257, 512, 513)]
MAIN = (1, 50, 0.0, INF)                                        # robust, max_iter, lower, upper: the reference's call
ROTA = [(1, 1, 0.0, INF), (1, 3, -INF, INF), (0, 50, 0.0, INF), (0, 50, -INF, INF), (1, 50, -INF, INF), (1, 3, 0.0, INF),
        (1, 1, -INF, INF), (1, 50, 0.02, 0.02), (0, 3, -INF, INF), (0, 1, 0.0, INF)]


def _settings(i):
    """every shape runs the reference's call and one of the other settings in turn"""
    return [MAIN, ROTA[i % len(ROTA)]]


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return RF.RobfitRef(tmp_path_factory.mktemp("robfit_ref_gpu"))


@functools.lru_cache(maxsize=None)
def _problem(D, n, R):
    X, y = RF.make_case(1000 * D + 10 * n + R, D, n, R)
    RF.plant(X, y)
    return X, y                                                  # shared: no test writes to them


_WANT = {}


def _want(ref, D, n, R, setting):
    """the C restatement's outputs, computed once per (shape, setting) and shared (read-only)"""
    key = (D, n, R, setting)
    if key not in _WANT:
        X, y = _problem(D, n, R)
        robust, max_iter, lower, upper = setting
        w = ref.run(X, y, robust=robust, lower=lower, upper=upper, max_iter=max_iter)
        for v in w.values():
            v.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


def _run_device(X, y, setting, names=RF.OUT_NAMES, device="cuda:0", calls=1):
    """epi_robfit_run_device `calls` times back to back on one stream, no synchronisation in between, each into its own
    poison-filled outputs with GUARD poisoned elements behind each; the guards are checked here"""
    import torch
    from epidemicmodeling_amd import _lib
    dev = torch.device(device)
    D, n, R = X.shape
    robust, max_iter, lower, upper = setting
    Xd = torch.as_tensor(np.ascontiguousarray(X), device=dev)
    yd = torch.as_tensor(np.ascontiguousarray(y), device=dev)
    shapes = _lib.robfit_shapes(R, D, n)
    d = _lib.make_robfit_desc(R, D, n, robust, max_iter, lower, upper)
    st = torch.cuda.current_stream(dev)
    bufs = []
    for _ in range(calls):
        buf = {}
        for k in names:
            m = int(np.prod(shapes[k]))
            if k in _lib.ROBFIT_OUT_I32:
                buf[k] = torch.full((m + GUARD,), I32_POISON, dtype=torch.int32, device=dev)
            else:
                buf[k] = torch.full((m + GUARD,), F64_POISON, dtype=torch.float64, device=dev)
        outs = _lib.RobfitOutputs()
        for k in _lib.ROBFIT_OUT_NAMES:
            setattr(outs, k, C.c_void_p(buf[k].data_ptr()) if k in buf else None)
        err = C.create_string_buffer(256)
        rc = _lib.lib().epi_robfit_run_device(C.byref(d), C.c_void_p(Xd.data_ptr()), C.c_void_p(yd.data_ptr()), C.byref(outs),
                                              C.c_void_p(st.cuda_stream), err)
        _lib.check(rc, err)
        bufs.append(buf)
    torch.cuda.synchronize(dev)
    res = []
    for buf in bufs:
        o = {}
        for k, v in buf.items():
            h = v.cpu().numpy()
            m = h.size - GUARD
            assert (h[m:] == (I32_POISON if k in _lib.ROBFIT_OUT_I32 else F64_POISON)).all(), f"{k}: written behind its end"
            o[k] = h[:m].reshape(shapes[k])
        res.append(o)
    return res if calls > 1 else res[0]


def _same(got, want, names=None):
    names = list(want) if names is None else names
    assert set(got) == set(names), (set(got), names)
    for k in names:
        assert RF.same_bits(np.asarray(got[k]), np.asarray(want[k])), k
        if np.asarray(got[k]).dtype == np.float64:
            assert not (np.asarray(got[k]) == F64_POISON).any(), f"{k}: an element was not written"


@pytest.mark.parametrize("i, shape", list(enumerate(SHAPES)), ids=[f"D{D}-n{n}-R{R}" for D, n, R in SHAPES])
def test_bit_identical_to_restatement(gpu_device, ref, i, shape):
    D, n, R = shape
    X, y = _problem(D, n, R)
    for setting in _settings(i):
        _same(_run_device(X, y, setting, device=gpu_device), _want(ref, D, n, R, setting))


def test_the_cases_reach_every_path(ref):
    """what the parametrised test above really covers, from the restatement's outputs: every status bit, every NV, iteration
    counts below and at the cap, both robust settings, every max_iter and both bounds settings"""
    bits, nvs, below, at, seen = 0, set(), False, False, set()
    for i, (D, n, R) in enumerate(SHAPES):
        nvs.add(max(64, 1 << (D - 1).bit_length()) // 64)
        for setting in _settings(i):
            w = _want(ref, D, n, R, setting)
            bits |= int(np.bitwise_or.reduce(w["status"].ravel()))
            seen.add(setting)
            if setting[0]:
                live = w["status"] != RF.NONFINITE
                below |= bool((w["iters"][live] < setting[1]).any())
                at |= bool((w["iters"][live] == setting[1]).any())
            else:
                assert (w["iters"] == 0).all()
    assert bits == RF.NONFINITE | RF.CONST | RF.SLOPE_LOST | RF.MAXITER | RF.BOUND
    assert nvs == {1, 2, 4, 8, 16} and below and at
    days = {D for D, _, _ in SHAPES}
    nv = lambda D: max(64, 1 << (D - 1).bit_length()) // 64
    for edge in (64, 128, 256, 512):                             # rf_dispatch: a shape on each threshold and one beyond it
        assert edge in days and edge + 1 in days and nv(edge + 1) == 2 * nv(edge), edge
    assert 3 in days and 1024 in days                            # validate's ends: 3 .. kRfMaxD
    assert {s[0] for s in seen} == {0, 1} and {s[1] for s in seen} == {1, 3, 50}
    assert {(0.0, INF), (-INF, INF)} <= {s[2:] for s in seen}
    X, y = _problem(5, 12, 70)
    kinds = RF.plant(X.copy(), y.copy())
    assert kinds == ["exact", "negative", "const", "outlier", "slope_lost", "nonfinite", "clip"]
    w = _want(ref, 5, 12, 70, MAIN)
    assert w["status"][0, 4] & RF.SLOPE_LOST and w["status"][11, 5] == RF.NONFINITE and np.isnan(w["b"][5])
    w = _want(ref, 65, 12, 70, MAIN)
    assert w["status"][0, 0] == 0 and w["a"][0, 0] == 0.5 and (w["weights"][:, 0, 0] == 1.0).all()      # the exact line
    assert w["status"][0, 1] & RF.BOUND and w["a"][0, 1] == 0.0                                        # the negative slope
    assert w["status"][11, 2] & RF.CONST and w["weights"][65 // 2, 0, 3] == 0.0                        # constant; the outlier


@pytest.mark.parametrize("D, n, R, setting", [(65, 12, 5, MAIN), (4, 1, 70, MAIN), (300, 1, 5, ROTA[2])])
@pytest.mark.parametrize("entry", ["device", "host"])
def test_each_output_alone(gpu_device, ref, entry, D, n, R, setting):
    from epidemicmodeling_amd import hostapi
    X, y = _problem(D, n, R)
    want = _want(ref, D, n, R, setting)
    robust, max_iter, lower, upper = setting
    for k in RF.OUT_NAMES:
        if entry == "device":
            got = _run_device(X, y, setting, names=(k,), device=gpu_device)
        else:
            got = hostapi.robust_affine_fit(X, y, robust=robust, lower=lower, upper=upper, max_iter=max_iter, outputs=(k,))
        _same(got, want, [k])


def test_batch_and_host_entries_equal_the_device_entry(gpu_device, ref):
    import torch
    from epidemicmodeling_amd import batch, hostapi
    D, n, R = 129, 12, 70
    X, y = _problem(D, n, R)
    want = _want(ref, D, n, R, MAIN)
    dev = _run_device(X, y, MAIN, device=gpu_device)
    b = batch.robust_affine_fit(X, y, outputs=RF.OUT_NAMES, device=gpu_device)
    torch.cuda.synchronize()
    b = {k: v.cpu().numpy() for k, v in b.items()}
    h = hostapi.robust_affine_fit(X, y, outputs=RF.OUT_NAMES)
    _same(dev, want)
    _same(b, dev)
    _same(h, dev)
    # the default leaves the weights out; robust=False is the least-squares start
    assert set(hostapi.robust_affine_fit(X, y)) == set(RF.OUT_NAMES) - {"weights"}
    D, n, R = 64, 12, 5
    X, y = _problem(D, n, R)
    _same(hostapi.robust_affine_fit(X, y, robust=False, lower=-INF, outputs=RF.OUT_NAMES), _want(ref, D, n, R, ROTA[3]))


def test_two_calls_back_to_back_on_one_stream(gpu_device, ref):
    D, n, R = 63, 12, 70
    X, y = _problem(D, n, R)
    first, second = _run_device(X, y, MAIN, device=gpu_device, calls=2)
    _same(first, _want(ref, D, n, R, MAIN))
    _same(second, first)


def _check_front_half(ref, out, raw, N, T, D, H):
    """re-derive preprocessing, both EKF rounds and both regressions from the previous stage (the filter oracle and the
    restatement applied to that stage's X_reg and alpha)"""
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
    names = [k for k in RF.OUT_NAMES if k != "weights"]
    f1 = ref.run(X, np.ascontiguousarray(out["alpha_round1"][-D:]))
    _same(out["fit1"], f1, names)
    o2 = H.oracle_batch(pipeline.workload3(x, R, u, N, I0, out["fit1"]["a"], out["fit1"]["b"]), outputs=["S_SMOOTH"])
    assert np.array_equal(out["alpha_round2"], o2["S_SMOOTH"][:, 2])
    f2 = ref.run(X, np.ascontiguousarray(out["alpha_round2"][-D:]))
    _same(out["fit2"], f2, names)
    assert (out["fit2"]["a"] >= 0).all() and np.isfinite(out["fit2"]["b"]).all()
    return f2


def test_prescription_pipeline_with_elementwise_stage_by_stage(gpu_device, ref):
    """pipeline.prescribe(regression="elementwise") on the region set of the LASSO pipeline test: every stage re-derived from
    the previous one, and the sweep consumes exactly the a, b of the second regression."""
    from tests import helpers as H
    from epidemicmodeling_amd import pipeline, synth
    S, T, H_, n_eps, D = 7, 150, 25, 12, 50
    raw = synth.make_raw_counts(S, T, seed=31)
    raw["cases"][:, -1] = np.cumsum(np.full(T, 40.0))
    out = pipeline.prescribe(raw["cases"], raw["deaths"], raw["population"], raw["ip"], horizon=H_, n_eps=n_eps,
                             num_regression_days=D, device=gpu_device, regression="elementwise")
    N = raw["population"]
    _check_front_half(ref, out, raw, N, T, D, H)
    os_ = H.oracle_batch(out["sweep"], outputs=["u_opt_smooth"])
    chains = np.arange(S) * n_eps + out["i_opt"]
    assert np.array_equal(out["prescription"], os_["u_opt_smooth"][T:][:, :, chains])
    n = raw["ip"].shape[1]
    assert out["prescription"].shape == (H_, n, S) and np.isfinite(out["prescription"]).all()
    # the stages behind the regression are built from exactly that a, b
    a2, b2 = out["fit2"]["a"], out["fit2"]["b"]
    reg = pipeline.sweep_region_inputs(N, out["I0"], a2, b2, n)
    assert set(reg) == set(out["sweep_region"]) and all(np.array_equal(out["sweep_region"][k], v, equal_nan=True) for k, v in reg.items())
    assert np.array_equal(out["sp_region"], pipeline.scoring_region_inputs(out["historic"][T - 1], a2, b2, synth.IP_MAXES[:n], np.ones((n, S))))
    w6 = pipeline.workload6(out["x_sweep"], out["R_sweep"], out["u_sweep"], N, out["I0"], a2, b2, out["eps_grid"])
    assert np.array_equal(out["sweep"].prm, w6.prm, equal_nan=True)
    with pytest.raises(ValueError, match="regression must be one of"):
        pipeline.prescribe(raw["cases"], raw["deaths"], raw["population"], raw["ip"], regression="element-wise", device=gpu_device)


def test_forecast_quality_with_elementwise_stage_by_stage(gpu_device, ref):
    from tests import helpers as H
    from epidemicmodeling_amd import pipeline, synth
    S, LL, F, M, D = 6, 140, 20, 10, 60
    raw = synth.make_raw_counts(S, LL, seed=17)
    raw["cases"][:, -1] = np.cumsum(np.full(LL, 40.0))
    out = pipeline.forecast_quality(raw["cases"], raw["deaths"], raw["population"], raw["ip"], F, max_lookahead=M,
                                    num_regression_days=D, device=gpu_device, regression="elementwise")
    T = LL - F
    N = raw["population"]
    _check_front_half(ref, out, raw, N, T, D, H)
    w = out["workload"]
    n = raw["ip"].shape[1]
    from epidemicmodeling_amd import layout as L
    assert np.array_equal(w.prm[L.PRM_A:L.PRM_A + n], out["fit2"]["a"]) and np.array_equal(w.prm[L.PRM_B], out["fit2"]["b"])
    from tests import lookahead_ref as LR
    from tests.test_gpu_lookahead import ARRAYS, _same as same_tables
    same_tables(out, LR.expected(w, out["truth"], np.asarray(N, dtype=np.float64), F, M), ARRAYS)


def test_prescribe_example_with_elementwise(gpu_device):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "prescribe_from_csv.py"), "--regression", "elementwise"],
                       capture_output=True, text=True, timeout=600, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "(regression: elementwise)" in r.stdout

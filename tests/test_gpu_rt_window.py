"""The sliding-window growth-rate estimators on the device (epi_rtwin_run_device / _host): every output, status and
iteration count bit-identical to the C restatement tests/rt_window_ref.c."""
import numpy as np
import pytest

from tests.rt_window_ref import RtWindowRef, ST_MAXITER, ST_MODEL_ERROR, ST_STALL
from tests.test_rt_window_host import hard_series

pytestmark = pytest.mark.gpu

ALL = ("LogLinReg", "GenRatios", "NonlinLS")


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return RtWindowRef(tmp_path_factory.mktemp("rtwin_ref_gpu"))


def _cases(R, L, seed):
    """noisy exponentials with zeros, NaN, Inf and the hard pieces that hit the iteration limit / stall"""
    rng = np.random.default_rng(seed)
    t = np.arange(L)[:, None]
    x = rng.uniform(5, 500, R) * np.exp(rng.uniform(-0.05, 0.08, R) * t + 0.3 * np.sin(t / rng.uniform(4, 12, R)))
    x *= 1.0 + 0.05 * rng.standard_normal((L, R))
    x = np.abs(x)
    m = rng.random((L, R))
    x[m < 0.02] = 0.0
    x[(m >= 0.02) & (m < 0.03)] = np.nan
    x[(m >= 0.03) & (m < 0.033)] = np.inf
    h = hard_series()
    for r in range(0, R, 3):
        n = min(L, len(h))
        x[:n, r] = np.roll(h, 7 * r)[:n]
    return x


def _want(ref, x, wlen, tu, causal, gp, methods):
    full = ref.all(x, wlen, tu, causal, gp if gp is not None else 1)
    keys = []
    if "LogLinReg" in methods:
        keys += [k for k in full if k.startswith("llr_")]
    if "GenRatios" in methods:
        keys += [k for k in full if k.startswith("gr_")]
    if "NonlinLS" in methods:
        keys += [k for k in full if k.startswith("nls_")]
    return {k: full[k] for k in keys}


def _same(got, want):
    assert set(got) == set(want)
    for k in want:
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else got[k]
        assert g.dtype == want[k].dtype, k
        if g.dtype == np.float64:
            # bit for bit, -0 / +0 included; only a NaN's payload and sign are free (x86 and the GPU make different NaNs)
            nan = np.isnan(want[k])
            assert np.array_equal(np.isnan(g), nan), k
            assert np.array_equal(g[~nan].view(np.int64), want[k][~nan].view(np.int64)), k
        else:
            assert np.array_equal(g, want[k]), k


@pytest.mark.parametrize("R", [1, 63, 64, 65])
@pytest.mark.parametrize("wlen, causal", [(7, 1), (7, 0), (6, 0), (6, 1), (2, 1), (31, 0), (14, 1)])
def test_bit_identical_to_reference(hip_lib, gpu_device, ref, R, wlen, causal):
    from epidemicmodeling_amd import batch
    import torch
    x = _cases(R, 90, R * 100 + wlen + causal)
    got = batch.rt_window(x, wlen, 1.5, causal, 4, ALL, device=gpu_device)
    torch.cuda.synchronize()
    _same(got, _want(ref, x, wlen, 1.5, causal, 4, ALL))


def test_statuses_covered(hip_lib, gpu_device, ref):
    from epidemicmodeling_amd import batch
    x = _cases(65, 120, 3)
    got = batch.rt_window(x, 7, 1.0, 1, 3, ("NonlinLS",), device=gpu_device)
    st = set(np.unique(got["nls_status"].cpu().numpy()).tolist())
    assert {0, 5, ST_MODEL_ERROR} <= st and (ST_MAXITER in st or ST_STALL in st) and ({1, 2} & st)
    _same(got, _want(ref, x, 7, 1.0, 1, 3, ("NonlinLS",)))


@pytest.mark.parametrize("methods", [("LogLinReg",), ("GenRatios",), ("NonlinLS",), ("LogLinReg", "GenRatios"),
                                     ("LogLinReg", "NonlinLS"), ("GenRatios", "NonlinLS")])
def test_method_subsets(hip_lib, gpu_device, ref, methods):
    from epidemicmodeling_amd import batch
    x = _cases(40, 50, 11)
    got = batch.rt_window(x, 5, 2.0, 0, 50 if "GenRatios" in methods else None, methods, device=gpu_device)
    _same(got, _want(ref, x, 5, 2.0, 0, 50, methods))


def test_short_series_and_gp_equal_L(hip_lib, gpu_device, ref):
    from epidemicmodeling_amd import batch
    x = _cases(5, 4, 2)
    got = batch.rt_window(x, 7, 1.0, 1, 4, ALL, device=gpu_device)
    _same(got, _want(ref, x, 7, 1.0, 1, 4, ALL))


def test_host_entry_equals_device_entry(hip_lib, gpu_device):
    from epidemicmodeling_amd import batch, hostapi
    x = _cases(70, 60, 5)
    dev = batch.rt_window(x, 7, 1.0, 1, 3, ALL, device=gpu_device)
    host = hostapi.rt_window(x, 7, 1.0, 1, 3, ALL, device=0)
    _same(dev, host)


def test_tools_mirrors_equal_a_batch_column(hip_lib, gpu_device):
    from epidemicmodeling_amd import batch, tools
    x = _cases(6, 80, 9)
    x[:, 4] = np.abs(x[:, 4])
    x[~np.isfinite(x[:, 4]), 4] = 1.0
    b = {k: v.cpu().numpy() for k, v in batch.rt_window(x, 7, 1.0, 0, 3, ALL, device=gpu_device).items()}
    col = x[:, 4]
    Rt, A, Lam, Fit = tools.Rt_ExpFitLogLinReg(col, 7, 1.0, 0)
    assert Rt.shape == (1, 80)
    for g, k in zip((Rt, A, Lam, Fit), ("llr_Rt", "llr_A", "llr_Lambda", "llr_ExpFit")):
        assert np.array_equal(g[0], b[k][:, 4], equal_nan=True)
    for g, k in zip(tools.Rt_ExpFitGenRatios(col, 7, 3, 1.0), ("gr_Rt", "gr_Lambda", "gr_RtSmoothed", "gr_LambdaSmoothed")):
        assert np.array_equal(g[0], b[k][:, 4], equal_nan=True)
    assert not np.any(b["nls_status"][:, 4] == ST_MODEL_ERROR)
    for g, k in zip(tools.Rt_ExpFitNonlinLS(col, 7, 1.0, 0), ("nls_Rt", "nls_A", "nls_Lambda", "nls_ExpFit")):
        assert np.array_equal(g[0], b[k][:, 4], equal_nan=True)
    bad = col.copy()
    bad[40] = np.inf
    with pytest.raises(RuntimeError, match="nlinfit"):
        tools.Rt_ExpFitNonlinLS(bad, 7, 1.0, 0)


def test_article_size_sample(hip_lib, gpu_device, ref):
    from epidemicmodeling_amd import batch
    x = _cases(236, 366, 1)
    got = {k: v.cpu().numpy() for k, v in batch.rt_window(x, 7, 1.0, 1, 3, ALL, device=gpu_device).items()}
    cols = np.arange(0, 236, 17)
    want = ref.all(np.ascontiguousarray(x[:, cols]), 7, 1.0, 1, 3)
    _same({k: v[:, cols] for k, v in got.items()}, want)


def test_growth_rates_pipeline_equals_its_stages(hip_lib, gpu_device):
    from epidemicmodeling_amd import batch, pipeline, synth, tools
    rng = np.random.default_rng(4)
    T, S = 90, 5
    daily = rng.uniform(10, 200, (T, S)) * np.exp(0.02 * np.arange(T))[:, None]
    cases = np.cumsum(daily, axis=0)
    cases[30, 1] = np.nan
    N = rng.uniform(1e6, 1e7, S)
    out = pipeline.growth_rates(cases, N, wlen=7, generation_period=3, causal=1, device=gpu_device)
    pre = batch.preprocess(cases, N, W=7, min_cases=synth.MIN_CASES, first_num_days=7, device=gpu_device)
    ns = pre["new_smoothed"].cpu().numpy()
    assert np.array_equal(out["new_smoothed"], ns)
    rw = {k: v.cpu().numpy() for k, v in batch.rt_window(ns, 7, 1.0, 1, 3, ALL, device=gpu_device).items()}
    for k in rw:
        assert np.array_equal(out[k], rw[k], equal_nan=True), k
    # the EKF stage (one batched call per order) equals tools.Rt_ExpFitEKF on each region with test04's settings (:197-219)
    Q_w = np.diag([250.0 ** 2, 3.0e-3 ** 2])
    for order in (1, 2):
        for s in range(S):
            r = tools.Rt_ExpFitEKF(ns[:, s].reshape(1, -1), [ns[0, s], 0.0], [1.0, 0.9, 0.1], [0.0, 0.0], 0.0, 100.0 * Q_w, Q_w,
                                   100.0, 0.9, 0.995, 21, order)
            assert np.array_equal(out[f"ekf{order}_S_PLUS"][:, :, s], r[1].T, equal_nan=True)
            assert np.array_equal(out[f"ekf{order}_S_SMOOTH"][:, :, s], r[5].T, equal_nan=True)
    hidden = pipeline.growth_rates(cases, N, wlen=7, generation_period=3, causal=1, forecast_days=10, device=gpu_device)
    r = tools.Rt_ExpFitEKF(np.concatenate([ns[:80, 2], np.full(10, np.nan)]).reshape(1, -1), [ns[0, 2], 0.0], [1.0, 0.9, 0.1],
                           [0.0, 0.0], 0.0, 100.0 * Q_w, Q_w, 100.0, 0.9, 0.995, 21, 1)
    assert np.array_equal(hidden["ekf1_S_SMOOTH"][:, :, 2], r[5].T, equal_nan=True)


def test_example_script_runs(hip_lib, gpu_device, tmp_path):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "growth.csv"
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "growth_rates_from_csv.py"), str(out)],
                       capture_output=True, text=True, timeout=600, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr
    text = out.read_text().splitlines()
    assert text[0].startswith("region,day,new_smoothed,llr_Lambda") and len(text) > 10

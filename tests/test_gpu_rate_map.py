"""The NPI-to-growth-rate predictor on the device (epi_ratemap_run_device / _host, batch.rate_map, hostapi.rate_map and
pipeline.growth_forecast): every output and status bit-identical to the C restatement tests/rate_map_ref.c, any NaN equal to
any NaN.  Outputs are pre-filled with NaN poison (status with an integer one), so an element the kernels did not write shows
as a NaN the restatement does not have; GUARD poisoned elements lie behind every output."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rate_map_ref as RM

pytestmark = pytest.mark.gpu

I32_POISON, GUARD = -12345, 64
# every NaN the restatement produces is the default quiet NaN; the poison carries a payload, so the two can be told apart
POISON_BITS = np.int64(0x7FF8DEADBEEF0001)


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return RM.RatemapRef(tmp_path_factory.mktemp("ratemap_ref_gpu"))


_WANT = {}


def _want(ref, i, fit=1):
    """the C restatement's outputs, computed once per case and shared (read-only)"""
    if (i, fit) not in _WANT:
        w = ref.run(RM.problem(i, fit), [k for k in RM.OUT_NAMES if fit or k != "map"])
        for v in w.values():
            v.setflags(write=False)
        _WANT[(i, fit)] = w
    return _WANT[(i, fit)]


def _desc(p):
    from epidemicmodeling_amd import _lib
    T, n, R = p["ip"].shape
    E = 0 if p["extra"] is None else p["extra"].shape[1]
    d = _lib.make_ratemap_desc(T, n, R, E, len(p["n_train"]), p["lags"], p["fit"], p["effect_lag"], p["ridge"], p["thr"], p["red"])
    return d, _lib.ratemap_shapes(T, n, R, E, len(p["n_train"]), len(p["lags"]))


def _run_device(p, names, device="cuda:0", calls=1):
    """epi_ratemap_run_device `calls` times back to back on one stream, no synchronisation in between, each into its own
    poison-filled outputs with GUARD poisoned elements behind each; the guards are checked here"""
    import torch
    from epidemicmodeling_amd import _lib
    dev = torch.device(device)
    d, shapes = _desc(p)
    up = lambda a: None if a is None else torch.as_tensor(np.array(a, dtype=np.float64), device=dev)   # a copy: the cases are read-only
    t = {k: up(p[k]) for k in ("ip", "y", "new_smoothed", "extra", "lambda_in")}
    if not p["fit"] and "y_filled" not in names:
        t["y"] = None
    nt = np.ascontiguousarray(p["n_train"], dtype=np.int32)
    ins = _lib.RatemapInputs()
    for k, v in t.items():
        setattr(ins, k, None if v is None else C.c_void_p(v.data_ptr()))
    ins.n_train = nt.ctypes.data
    st = torch.cuda.current_stream(dev)
    bufs = []
    for _ in range(calls):
        buf = {}
        for k in names:
            m = int(np.prod(shapes[k]))
            if k in _lib.RATEMAP_OUT_I32:
                buf[k] = torch.full((m + GUARD,), I32_POISON, dtype=torch.int32, device=dev)
            else:
                buf[k] = torch.full((m + GUARD,), int(POISON_BITS), dtype=torch.int64, device=dev)
        outs = _lib.RatemapOutputs()
        for k in _lib.RATEMAP_OUT_NAMES:
            setattr(outs, k, C.c_void_p(buf[k].data_ptr()) if k in buf else None)
        err = C.create_string_buffer(256)
        rc = _lib.lib().epi_ratemap_run_device(C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(st.cuda_stream), err)
        _lib.check(rc, err)
        bufs.append(buf)
    torch.cuda.synchronize(dev)
    res = []
    for buf in bufs:
        o = {}
        for k, v in buf.items():
            h = v.cpu().numpy()
            m = h.size - GUARD
            assert (h[m:] == (I32_POISON if k in _lib.RATEMAP_OUT_I32 else POISON_BITS)).all(), f"{k}: written behind its end"
            assert not (h[:m] == (I32_POISON if k in _lib.RATEMAP_OUT_I32 else POISON_BITS)).any(), f"{k}: an element was not written"
            o[k] = h[:m].reshape(shapes[k]) if k in _lib.RATEMAP_OUT_I32 else h[:m].view(np.float64).reshape(shapes[k])
        res.append(o)
    return res if calls > 1 else res[0]


def _same(got, want, names=None):
    names = list(want) if names is None else list(names)
    assert set(got) == set(names), (set(got), names)
    for k in names:
        assert RM.same_bits(np.asarray(got[k]), np.asarray(want[k])), k


IDS = ["T%d-n%d-lags%d-E%d-K%d-R%d" % (c[0], c[1], len(c[2]), c[3], c[4], c[5]) for c, _ in RM.CASES]


@pytest.mark.parametrize("i", range(len(RM.CASES)), ids=IDS)
def test_bit_identical_to_restatement(gpu_device, ref, i):
    _same(_run_device(RM.problem(i), RM.OUT_NAMES, device=gpu_device), _want(ref, i))


@pytest.mark.parametrize("i", (1, 3, 6))
def test_without_a_fit(gpu_device, ref, i):
    names = [k for k in RM.OUT_NAMES if k != "map"]
    _same(_run_device(RM.problem(i, 0), names, device=gpu_device), _want(ref, i, 0))
    # and without y: lambda_in alone feeds the clip and the rebuild
    names = [k for k in names if k != "y_filled"]
    _same(_run_device(RM.problem(i, 0), names, device=gpu_device), _want(ref, i, 0), names)


def test_each_output_alone(gpu_device, ref):
    for i in (1, 4):
        want = _want(ref, i)
        for k in RM.OUT_NAMES:
            _same(_run_device(RM.problem(i), [k], device=gpu_device), want, [k])


def test_two_calls_back_to_back_on_one_stream(gpu_device, ref):
    a, b = _run_device(RM.problem(3), RM.OUT_NAMES, device=gpu_device, calls=2)
    _same(a, _want(ref, 3))
    _same(b, _want(ref, 3))


@pytest.mark.parametrize("i", (1, 2, 5))
def test_device_batch_and_host_entries_are_equal(gpu_device, ref, i):
    from epidemicmodeling_amd import batch, hostapi
    p, want = RM.problem(i), _want(ref, i)
    kw = dict(y=p["y"], extra=p["extra"], lags=p["lags"], ridge=p["ridge"], lambda_threshold=p["thr"], reduction_effect=p["red"],
              effect_lag=p["effect_lag"])
    _same({k: v.cpu().numpy() for k, v in batch.rate_map(p["ip"], p["new_smoothed"], p["n_train"], device=gpu_device, **kw).items()}, want)
    _same(hostapi.rate_map(p["ip"], p["new_smoothed"], p["n_train"], **kw), want)
    p0, want0 = RM.problem(i, 0), _want(ref, i, 0)
    got = hostapi.rate_map(p0["ip"], p0["new_smoothed"], p0["n_train"], lambda_in=p0["lambda_in"], lags=p0["lags"],
                           outputs=("lambda_hat", "new_cases_est", "status"))
    _same(got, want0, ("lambda_hat", "new_cases_est", "status"))


def test_growth_forecast_pipeline_equals_its_stages(gpu_device, ref):
    from epidemicmodeling_amd import batch, pipeline, synth
    rng = np.random.default_rng(11)
    T, S, n = 90, 5, 4
    daily = rng.uniform(10, 200, (T, S)) * np.exp(0.02 * np.arange(T))[:, None]
    cases = np.cumsum(daily, axis=0)
    cases[30, 1] = np.nan
    N = rng.uniform(1e6, 1e7, S)
    ip = np.repeat(rng.integers(0, 4, size=(T // 10, n, S)), 10, axis=0).astype(np.float64)
    ip[40:43, 1, 2] = np.nan                                                 # N/A days: preprocess fills them
    out = pipeline.growth_forecast(cases, N, ip, predict_ahead=(14, 30), lags=(3, 5, 7), target="llr_Lambda", device=gpu_device)
    assert list(out["n_train"]) == [76, 60]
    pre = batch.preprocess(cases, N, ip=ip, W=7, min_cases=synth.MIN_CASES, first_num_days=7, device=gpu_device)
    ns, ipf = pre["new_smoothed"].cpu().numpy(), pre["ip_filled"].cpu().numpy()
    assert np.array_equal(out["new_smoothed"], ns) and np.array_equal(out["ip_filled"], ipf) and not np.isnan(ipf).any()
    rw = batch.rt_window(ns, 7, 1.0, 1, 3, ("LogLinReg", "GenRatios", "NonlinLS"), device=gpu_device)
    y = rw["llr_Lambda"].cpu().numpy()
    assert np.array_equal(out["llr_Lambda"], y, equal_nan=True)
    p = dict(ip=ipf, y=y, new_smoothed=ns, extra=None, lambda_in=None, n_train=(76, 60), lags=(3, 5, 7), fit=1, effect_lag=3,
             ridge=1e-6, thr=0.1, red=0.01)
    want = ref.run(p)
    _same({k: out[k] for k in RM.OUT_NAMES}, want)
    _same(RM.np_rate_map(p, ref.fma, ref.exp), want)
    for k, nt in enumerate((76, 60)):
        e = want["new_cases_est"][k, nt:] - ns[nt:]
        assert np.array_equal(out["err"][k, nt:], e, equal_nan=True) and np.isnan(out["err"][k, :nt]).all()
        assert np.allclose(out["mae"][k], np.abs(e).mean(axis=0), rtol=1e-13, equal_nan=True)
        assert np.allclose(out["rmse"][k], np.sqrt((e * e).mean(axis=0)), rtol=1e-13, equal_nan=True)
    # another regressand and a caller-made ones column (test05's)
    out2 = pipeline.growth_forecast(cases, N, ip, n_train=[80], lags=(3,), target="gr_LambdaSmoothed", extra=np.ones((T, 1, S)),
                                    device=gpu_device)
    p2 = dict(p, y=rw["gr_LambdaSmoothed"].cpu().numpy(), extra=np.ones((T, 1, S)), n_train=(80,), lags=(3,))
    _same({k: out2[k] for k in RM.OUT_NAMES}, ref.run(p2))


def test_example_script_runs(gpu_device, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "forecast.csv"
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "growth_forecast_from_csv.py"), str(out)],
                       capture_output=True, text=True, timeout=300, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr
    text = out.read_text().splitlines()
    assert text[0].startswith("region,days_ahead,day,new_smoothed,lambda_hat,new_cases_est,status") and len(text) > 10

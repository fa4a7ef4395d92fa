"""The sliding-window growth-rate estimators without a GPU: descriptor validation through the C ABI, and the C restatement
(tests/rt_window_ref.c, the GPU suite's yardstick) against NumPy / SciPy readings of the three .m files."""
import ctypes as C

import numpy as np
import pytest

from tests.rt_window_ref import (RtWindowRef, np_genratios, np_loglinreg, ST_MODEL_ERROR, ST_OUTSIDE, ST_SKIPPED, ST_TOLFUN,
                                 ST_TOLX, ST_MAXITER, ST_STALL)


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return RtWindowRef(tmp_path_factory.mktemp("rtwin_ref"))


def _ulps(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    d = np.abs(a - b) / np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), 5e-324)
    return np.where(same, 0.0, d)


def _series(rng, L, growth=0.05, noise=0.05, a0=50.0):
    t = np.arange(L)
    return a0 * np.exp(growth * t + 0.3 * np.sin(t / 9.0)) * (1.0 + noise * rng.standard_normal(L))


# ---- validation ---------------------------------------------------------------------------------------------------
def _validate(**kw):
    from epidemicmodeling_amd import _lib
    args = dict(R=4, L_=30, wlen=7, time_unit=1.0, causal=1, generation_period=3, methods=7)
    args.update({k: v for k, v in kw.items() if k in args})
    d = _lib.make_rtwin_desc(**args)
    for k in ("abi_version",):
        if k in kw:
            setattr(d, k, kw[k])
    x = np.ones((30, 4))
    outs = _lib.RtwinOutputs()
    err = C.create_string_buffer(256)
    xp = None if kw.get("null_x") else x.ctypes.data
    rc = _lib.lib().epi_rtwin_validate(C.byref(d), xp, None if kw.get("null_out") else C.byref(outs), err)
    rc_host = _lib.lib().epi_rtwin_run_host(C.byref(d), xp, None if kw.get("null_out") else C.byref(outs), 0,
                                            C.create_string_buffer(256))
    return rc, err.value.decode(), rc_host


@pytest.mark.parametrize("kw, rc, msg", [
    (dict(abi_version=5), -5, "ABI"),
    (dict(R=0), -5, "R and L"),
    (dict(L_=0), -5, "R and L"),
    (dict(causal=2), -5, "causal"),
    (dict(generation_period=0), -5, "generation_period"),
    (dict(generation_period=31), -5, "generation_period"),
    (dict(methods=0), -5, "methods"),
    (dict(null_x=True), -5, "NULL"),
    (dict(null_out=True), -5, "NULL"),
    (dict(wlen=1), -8, "wlen"),
    (dict(wlen=32), -8, "wlen"),
])
def test_validate_rejects(hip_lib, kw, rc, msg):
    got, text, host = _validate(**kw)
    assert got == rc and msg in text
    assert host == rc                     # the host entry validates before it touches a device


def test_validate_accepts(hip_lib):
    assert _validate()[0] == 0
    assert _validate(generation_period=0, methods=5)[0] == 0      # gp only matters for GenRatios
    assert _validate(generation_period=30)[0] == 0                # gp == L
    assert _validate(wlen=2)[0] == 0 and _validate(wlen=31)[0] == 0


def test_python_layer_reports_validation(hip_lib):
    from epidemicmodeling_amd import hostapi, _lib
    with pytest.raises(_lib.EpiError, match="wlen"):
        hostapi.rt_window(np.ones((10, 2)), 40, generation_period=3)


# ---- the C restatement against the .m readings ---------------------------------------------------------------------
def test_log_is_within_an_ulp(ref):
    rng = np.random.default_rng(1)
    xs = np.concatenate([np.exp(rng.uniform(-700, 700, 4000)), rng.uniform(0.5, 2.0, 4000), [1.0, 2.0, 0.5, 1e-310, 7.0]])
    got = np.array([ref.log(v) for v in xs])
    assert _ulps(got, np.log(xs)).max() <= 1.0
    assert ref.log(0.0) == -np.inf and np.isnan(ref.log(-1.0)) and np.isnan(ref.log(np.nan)) and ref.log(np.inf) == np.inf
    assert ref.log(1.0) == 0.0


@pytest.mark.parametrize("wlen", [2, 3, 6, 7, 14, 31])
@pytest.mark.parametrize("causal", [0, 1])
def test_loglinreg_matches_numpy(ref, wlen, causal):
    rng = np.random.default_rng(wlen + 10 * causal)
    x = _series(rng, 80)
    got = ref.loglinreg(x, wlen, 1.5, causal)
    want = np_loglinreg(x, wlen, 1.5, causal)
    for k in want:                                # NumPy's mean sums pairwise: a few ulp of the sums, amplified by 1 / Det
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=1e-13)
    # the slope is np.polyfit's on the log
    h = wlen // 2
    mm = 40
    seg = np.log(x[mm - wlen + 1:mm + 1]) if causal else np.log(x[mm - h:mm + h + 1])
    n = np.arange(-wlen + 1, 1) if causal else np.arange(-h, h + 1)
    slope, icpt = np.polyfit(n, seg, 1)
    assert got["Lambda"][mm] * 1.5 == pytest.approx(slope, rel=1e-10)
    assert np.log(got["A"][mm]) == pytest.approx(icpt, rel=1e-10, abs=1e-12)


def test_loglinreg_edges(ref):
    x = np.array([1.0, 2.0, 0.0, 4.0, 8.0, np.nan, 3.0, 5.0, 6.0, 7.0])
    got = ref.loglinreg(x, 3, 1.0, 1)
    want = np_loglinreg(x, 3, 1.0, 1)
    for k in want:
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(want[k]))
        fin = ~np.isnan(want[k])
        np.testing.assert_allclose(got[k][fin], want[k][fin], rtol=1e-12, atol=1e-13)
    assert np.all(got["Rt"][:2] == 1.0) and np.all(got["A"][:2] == 1.0) and np.all(got["Lambda"][:2] == 0.0)
    short = ref.loglinreg(np.arange(1.0, 4.0), 7, 1.0, 1)                  # L < wlen: no window
    assert np.all(short["Rt"] == 1.0) and np.all(short["Lambda"] == 0.0)


@pytest.mark.parametrize("wlen, gp", [(2, 1), (7, 3), (7, 7), (13, 5), (31, 2)])
def test_genratios_matches_numpy(ref, wlen, gp):
    rng = np.random.default_rng(wlen * gp)
    x = _series(rng, 60)
    x[[10, 25]] = 0.0
    x[33] = np.nan
    got = ref.genratios(x, wlen, gp, 0.5)
    want = np_genratios(x, wlen, gp, 0.5)
    for k in want:
        np.testing.assert_array_equal(np.isnan(got[k]), np.isnan(want[k]))
        np.testing.assert_array_equal(np.isinf(got[k]), np.isinf(want[k]))
        fin = np.isfinite(want[k])
        np.testing.assert_allclose(got[k][fin], want[k][fin], rtol=1e-13, atol=1e-15)
    assert np.all(got["Lambda"][:gp] == 0.0)


def test_genratios_gp_equals_L(ref):
    got = ref.genratios(np.arange(1.0, 8.0), 3, 7, 1.0)
    assert np.all(got["Lambda"] == 0.0) and np.all(got["Rt"] == 1.0) and np.all(got["RtSmoothed"] == 1.0)


def _lm_scipy(seg, t, x0):
    from scipy.optimize import least_squares
    keep = ~np.isnan(seg)
    f = lambda b: b[0] * np.exp(b[1] * t[keep]) - seg[keep]
    return least_squares(f, x0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15).x


@pytest.mark.parametrize("wlen, causal, tu", [(7, 1, 1.0), (7, 0, 1.0), (6, 0, 2.0), (14, 1, 7.0), (31, 0, 1.0), (2, 1, 1.0)])
def test_nonlinls_matches_scipy_lm(ref, wlen, causal, tu):
    rng = np.random.default_rng(100 + wlen)
    x = _series(rng, 70, noise=0.03)
    got = ref.nonlinls(x, wlen, tu, causal)
    h = wlen // 2
    n = np.arange(-wlen + 1, 1) if causal else np.arange(-h, h + 1)
    days = range(wlen - 1, 70) if causal else range(h, 70 - h)
    for mm in list(days)[::5]:
        seg = x[mm - wlen + 1:mm + 1] if causal else x[mm - h:mm + h + 1]
        t = n / tu
        b = _lm_scipy(seg, t, [x[mm], 0.0])
        assert got["status"][mm] in (ST_TOLX, ST_TOLFUN)
        # TolFun = 1e-6 stops on a relative SSE change: the SSE is the optimum's to ~1e-6, the parameters to ~1e-5
        sse = ((seg - got["A"][mm] * np.exp(got["Lambda"][mm] * tu * t)) ** 2).sum()
        sse_opt = ((seg - b[0] * np.exp(b[1] * t)) ** 2).sum()
        assert sse <= sse_opt * (1 + 2e-6) + 1e-15 * (seg ** 2).sum()
        assert got["A"][mm] == pytest.approx(b[0], rel=3e-5)
        assert got["Lambda"][mm] * tu == pytest.approx(b[1], rel=3e-4, abs=1e-6)
    np.testing.assert_array_equal(got["Rt"], np.array([ref.exp(v) for v in got["Lambda"] * tu]))


@pytest.mark.parametrize("causal", [0, 1])
def test_nonlinls_recovers_exact_exponentials(ref, causal):
    t = np.arange(60)
    x = 20.0 * np.exp(0.04 * t)
    got = ref.nonlinls(x, 7, 1.0, causal)
    inside = got["status"] != ST_OUTSIDE
    assert inside.sum() > 40
    np.testing.assert_allclose(got["Lambda"][inside], 0.04, rtol=1e-8)
    np.testing.assert_allclose(got["A"][inside], x[inside], rtol=1e-8)


def test_nonlinls_quirks(ref):
    x = np.array([3.0, 4.0, 5.0, 0.0, 7.0, 8.0, 9.0, 10.0, 11.0, 12.0, 13.0, 14.0])
    c = ref.nonlinls(x, 3, 1.0, 1)
    assert np.all(c["A"][:2] == 0.0) and np.all(c["status"][:2] == ST_OUTSIDE)     # causal leading A = 0
    assert np.all(c["status"][3:6] == ST_SKIPPED)                                    # a zero in the window: skip
    assert np.all(c["A"][3:6] == x[3:6]) and np.all(c["Lambda"][3:6] == 0.0) and np.all(c["iters"][3:6] == 0)
    assert np.all(np.isin(c["status"][6:], (ST_TOLX, ST_TOLFUN)))
    z = ref.nonlinls(x, 4, 1.0, 0)                                                   # even wlen centred: 5 samples
    assert np.all(z["A"][:2] == x[:2]) and z["status"][0] == ST_OUTSIDE               # centred: A starts as x
    assert np.isin(z["status"][3], (ST_TOLX, ST_TOLFUN))                              # one zero in 5 samples: fitted
    o = ref.nonlinls(x, 3, 1.0, 0)
    assert o["status"][3] == ST_SKIPPED                                               # odd wlen: one zero skips
    # NaN counts as non-zero and is then dropped
    y = 10.0 * np.exp(0.1 * np.arange(12))
    y[5] = np.nan
    g = ref.nonlinls(y, 5, 1.0, 1)
    assert g["status"][6] in (ST_TOLX, ST_TOLFUN) and g["Lambda"][6] == pytest.approx(0.1, rel=1e-8)
    assert g["status"][5] == ST_MODEL_ERROR and np.isnan(g["A"][5])                  # x(mm) = NaN starts the model at NaN
    # Inf: model error, NaN outputs
    w = y.copy(); w[5] = 10.0; w[8] = np.inf
    e = ref.nonlinls(w, 3, 1.0, 1)
    assert np.all(e["status"][8:11] == ST_MODEL_ERROR) and np.all(np.isnan(e["Rt"][8:11]))
    # L < wlen: nothing fitted
    s = ref.nonlinls(np.arange(1.0, 4.0), 7, 1.0, 1)
    assert np.all(s["status"] == ST_OUTSIDE) and np.all(s["A"] == 0.0)
    # fewer than 2 samples after dropping NaN
    q = ref.nonlinls(np.array([1.0, np.nan, np.nan, 2.0]), 2, 1.0, 1)
    assert q["status"][2] == ST_MODEL_ERROR


def test_nonlinls_limits_reached(ref):
    """windows that hit the iteration limit or stall exist and report it (inputs of the GPU bit-exactness suite)"""
    from tests.test_rt_window_host import hard_series
    x = hard_series()
    got = ref.nonlinls(x, 7, 1.0, 1)
    st = set(np.unique(got["status"]).tolist())
    assert ST_MAXITER in st or ST_STALL in st


def hard_series():
    """a series whose windows include near-flat, oscillating and huge-dynamic-range pieces"""
    rng = np.random.default_rng(7)
    parts = [np.full(20, 5.0), 1e6 * np.exp(-2.0 * np.arange(20)), 1.0 + (np.arange(20) % 2) * 1e3,
             np.exp(rng.uniform(-30, 30, 30)), 100.0 * np.exp(0.3 * np.arange(20)) * (1 + 0.5 * rng.standard_normal(20))]
    return np.abs(np.concatenate(parts)) + 1e-3

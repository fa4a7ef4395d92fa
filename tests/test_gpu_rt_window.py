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


# ---------------------------------------------------------------- window shapes at the limits
def _nw(wlen, causal):
    return wlen if causal else 2 * (wlen // 2) + 1


@pytest.mark.parametrize("wlen, causal", [(31, 1), (30, 0), (30, 1), (3, 0)])
@pytest.mark.parametrize("dL", [None, -1, 0, 1])
def test_window_lengths_around_the_series_length(hip_lib, gpu_device, ref, wlen, causal, dL):
    """L in {1, nw - 1, nw, nw + 1} for the longest causal window (31 samples), both parities of a 30-day window and the
    shortest centred one; generation_period 1 and L, time units 7 and 0.25, R = 1 and R = 65 (a second wavefront)."""
    from epidemicmodeling_amd import batch
    import torch
    L = 1 if dL is None else _nw(wlen, causal) + dL
    for R in (1, 65):
        x = _cases(R, L, 1000 * wlen + 10 * L + causal)
        for gp, tu in ((1, 7.0), (L, 0.25)):
            got = batch.rt_window(x, wlen, tu, causal, gp, ALL, device=gpu_device)
            torch.cuda.synchronize()
            _same(got, _want(ref, x, wlen, tu, causal, gp, ALL))
            if L >= _nw(wlen, causal):
                assert (got["nls_status"].cpu().numpy() != 0).any()


# ---------------------------------------------------------------- optional outputs: each alone, in a poisoned arena
SUBSETS = [(n,) for n in ("llr_Rt", "llr_A", "llr_Lambda", "llr_ExpFit", "gr_Rt", "gr_Lambda", "gr_RtSmoothed",
                          "gr_LambdaSmoothed", "nls_Rt", "nls_A", "nls_Lambda", "nls_ExpFit", "nls_status", "nls_iters")]
SUBSETS += [("llr_ExpFit", "nls_iters"), ("gr_Lambda", "nls_status"), ("llr_A", "gr_RtSmoothed", "nls_ExpFit")]


@pytest.mark.parametrize("entry", ["device", "host"])
def test_each_output_alone(hip_lib, gpu_device, entry):
    """epi_rtwin_outputs may hold NULL for any output.  With all three methods on, each output alone (and a few mixed subsets)
    comes back equal to the all-outputs run bit for bit; every byte of the arena outside the requested outputs (guards and
    the never-requested neighbours) keeps its poison.  The dispatcher decides per method from an OR of the pointers."""
    import ctypes as C
    from epidemicmodeling_amd import _lib, batch
    import torch
    from tests import helpers as H
    R, L, wlen = 67, 40, 7
    x = np.ascontiguousarray(_cases(R, L, 21))
    full = {k: v.cpu().numpy() for k, v in batch.rt_window(x, wlen, 1.5, 1, 3, ALL, device=gpu_device).items()}
    specs = [(n, (L, R), np.int32 if n in _lib.RTWIN_OUT_I32 else np.float64) for n in _lib.RTWIN_OUT_NAMES]
    d = _lib.make_rtwin_desc(R, L, wlen, 1.5, 1, 3, 7)
    xd = torch.as_tensor(x, device=gpu_device)
    for req in SUBSETS:
        ar = H.GuardArena(specs, device=gpu_device if entry == "device" else None)
        outs = _lib.RtwinOutputs()
        for n in _lib.RTWIN_OUT_NAMES:
            setattr(outs, n, C.c_void_p(ar.ptr(n)) if n in req else None)
        err = C.create_string_buffer(256)
        if entry == "device":
            st = torch.cuda.current_stream(torch.device(gpu_device))
            rc = _lib.lib().epi_rtwin_run_device(C.byref(d), C.c_void_p(xd.data_ptr()), C.byref(outs), C.c_void_p(st.cuda_stream),
                                                 err)
        else:
            rc = _lib.lib().epi_rtwin_run_host(C.byref(d), C.c_void_p(x.ctypes.data), C.byref(outs), 0, err)
        _lib.check(rc, err)
        _same({n: ar.get(n) for n in req}, {n: full[n] for n in req})
        assert ar.untouched(req), req


# ---------------------------------------------------------------- LogLinReg and GenRatios against 50-digit arithmetic
def _gamma(k):
    u = 2.0 ** -53
    return k * u / (1 - k * u)


@pytest.mark.parametrize("wlen, causal", [(2, 1), (2, 0), (31, 1), (31, 0)])
def test_loglinreg_and_genratios_against_high_precision(hip_lib, gpu_device, wlen, causal):
    """The window regression and the generation ratios evaluated in 50-digit arithmetic (mpmath) from the fp64 inputs.
    Bound (u = 2^-53, gamma_k = k u / (1 - k u)): epi_log is within 1 ulp <= 2 u |seg_i| of log x_i.  r = sum c_i seg_i with
    c_i = (n_i - En) / (nw Det) moves by at most sum |c_i| 2 u |seg_i| through the logs; the kernel's sums s and ns carry
    gamma_nw sum |seg_i| and gamma_nw sum |n_i seg_i| (n_i are exact integers), the means one rounding each, the products and
    the difference in the numerator one each, En / En2 / Det (exact sums of integers, a division each and a difference) a
    relative gamma_3 (En2 + En^2) / Det, and the last division one: the error of r is bounded by
      (E_log + gamma_nw+2 (sum |n_i seg_i| + |En| sum |seg_i|) / nw) / Det + (gamma_3 (En2 + En^2) / Det + 2 u) |r|
    and ALog likewise with (En2, En) in place of (1, En) on (ms, mns).  Lambda = r / time_unit adds one rounding.  A = exp(ALog)
    (epi_exp within 1 ulp): relative error |dALog| + 2 u.  GenRatios: lambda = log(x_t / x_t-gp) / gp: the quotient's rounding
    moves the log by u, the log adds 1 ulp and the division one rounding: |d lambda| <= u / gp + 3 u |lambda|; the moving
    average of wlen terms c lambda (c = 1 / wlen rounded) adds gamma_wlen+2 sum |lambda| / wlen on top of the propagated errors
    of its terms."""
    pytest.importorskip("mpmath")
    from epidemicmodeling_amd import batch
    x = _smooth_cases(wlen, causal)
    got = {k: v.cpu().numpy() for k, v in batch.rt_window(x, wlen, 0.25, causal, 4, ("LogLinReg", "GenRatios"),
                                                           device=gpu_device).items()}
    _check_against_high_precision(got, x, wlen, causal, 4, 0.25)


def _smooth_cases(wlen, causal):
    rng = np.random.default_rng(wlen * 3 + causal)
    R, L = 5, 70
    t = np.arange(L)[:, None]
    x = rng.uniform(5, 5e4, R) * np.exp(rng.uniform(-0.1, 0.1, R) * t) * (1 + 0.3 * rng.random((L, R)))
    return np.ascontiguousarray(x)


def _check_against_high_precision(got, x, wlen, causal, gp, tu):
    import mpmath as mp
    mp.mp.dps = 50
    u = 2.0 ** -53
    L, R = x.shape
    nw = _nw(wlen, causal)
    off = -(wlen - 1) if causal else -(wlen // 2)
    n = np.arange(nw) + off
    En, En2 = mp.mpf(int(n.sum())) / nw, mp.mpf(int((n * n).sum())) / nw
    Det = En2 - En ** 2
    fDet = float(Det)
    checked = 0
    for r_ in range(R):
        lg = [mp.log(mp.mpf(float(v))) for v in x[:, r_]]
        for mm in range(-off, L - (nw - 1 + off)):
            seg = [lg[mm + off + i] for i in range(nw)]
            ms = mp.fsum(seg) / nw
            mns = mp.fsum(mp.mpf(int(n[i])) * seg[i] for i in range(nw)) / nw
            r = (mns - ms * En) / Det
            ALog = (ms * En2 - mns * En) / Det
            sabs = float(mp.fsum(abs(s) for s in seg))
            nsabs = float(mp.fsum(abs(int(n[i]) * seg[i]) for i in range(nw)))
            cdet = _gamma(3) * float(En2 + En ** 2) / fDet
            e_log_r = sum(abs(float(n[i] - En)) / (nw * fDet) * 2 * u * abs(float(seg[i])) for i in range(nw))
            e_r = (e_log_r + _gamma(nw + 2) * (nsabs + abs(float(En)) * sabs) / nw / fDet) + (cdet + 2 * u) * abs(float(r))
            e_log_a = sum(abs(float(En2 - n[i] * En)) / (nw * fDet) * 2 * u * abs(float(seg[i])) for i in range(nw))
            e_a = (e_log_a + _gamma(nw + 2) * (float(En2) * sabs + abs(float(En)) * nsabs) / nw / fDet) + (cdet + 2 * u) * abs(float(ALog))
            lam = got["llr_Lambda"][mm, r_]
            assert abs(lam - float(r / tu)) <= (e_r / tu) * (1 + 1e-6) + u * abs(lam), (r_, mm)
            A = got["llr_A"][mm, r_]
            exA = mp.exp(ALog)
            assert abs(mp.mpf(float(A)) - exA) <= exA * (e_a * (1 + 1e-6) + 2 * u) * (1 + 1e-6), (r_, mm)
            checked += 1
        # GenRatios
        lam_ex = [mp.mpf(0)] * gp + [mp.log(mp.mpf(float(x[t_, r_])) / mp.mpf(float(x[t_ - gp, r_]))) / gp for t_ in range(gp, L)]
        e_lam = [0.0] * gp + [u / gp + 3 * u * abs(float(v)) for v in lam_ex[gp:]]
        for t_ in range(L):
            g = got["gr_Lambda"][t_, r_]
            assert abs(g - float(lam_ex[t_])) <= e_lam[t_] * (1 + 1e-6) + 1e-300, (r_, t_)
            terms = [lam_ex[t_ - k] for k in range(wlen) if t_ - k >= 0]
            sm = mp.fsum(terms) / wlen
            e_sm = (sum(e_lam[t_ - k] for k in range(wlen) if t_ - k >= 0) / wlen
                    + _gamma(wlen + 2) * float(mp.fsum(abs(v) for v in terms)) / wlen)
            gs = got["gr_LambdaSmoothed"][t_, r_]
            assert abs(gs - float(sm)) <= e_sm * (1 + 1e-6) + 1e-300, (r_, t_)
    assert checked > 0

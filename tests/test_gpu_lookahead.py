"""GPU suite of the forecast look-ahead error study (Tools/ForecastQualityAssessment.m:359-393, 428-449) as one device call
(epi_lookahead_run_device / _host, batch.lookahead, pipeline.forecast_quality): bit for bit against the C oracle's chains
and the restatement of tests/lookahead_ref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as H
from tests import lookahead_ref as LR

pytestmark = pytest.mark.gpu

ARRAYS = ("est_plus", "est_smooth", "mean_plus", "median_plus", "std_plus", "mean_smooth", "median_smooth", "std_smooth")


def _case(R, LL, zeros=True):
    from epidemicmodeling_amd import synth
    w = synth.make_cfg3(R, LL)
    N = synth.make_regions(R)["N"].astype(np.float64)
    # NewCasesSmoothed_ENTIRE stand-in: the synthetic regions' new cases, shifted off zero (their epidemics die out)
    truth = w.x * N[None, :] + 50.0
    if zeros:                                                 # zero truth days in the tail: Inf (and 0/0 = NaN) entries
        truth[LL - 1, 0] = 0.0
        truth[LL - 3, R - 1] = 0.0
    return w, np.ascontiguousarray(truth), N


def _same(got, exp, names, cols=None):
    for n in names:
        g = got[n] if cols is None else got[n][..., cols]
        assert g.shape == exp[n].shape, (n, g.shape, exp[n].shape)
        assert np.array_equal(g, exp[n], equal_nan=True), (n, np.nanmax(np.abs(g - exp[n])))


def test_lookahead_small_study_bit_identical(gpu_device):
    from epidemicmodeling_amd import batch, synth
    w, truth, N = _case(6, 150)
    got = batch.lookahead(w, truth, N, 25, 10, device=gpu_device, chains=True)
    exp = LR.expected(w, truth, N, 25, 10)
    _same(got, exp, ARRAYS + ("S_PLUS", "S_SMOOTH"))
    assert np.isinf(got["est_plus"][:, :, 0]).any()
    # the same chains as the test scaffolding's ensemble run through the filter entry
    ens = batch.run_workload(synth.make_mask_ensemble(6, 150, 25), outputs=["S_PLUS", "S_SMOOTH"], device=gpu_device)
    assert np.array_equal(got["S_PLUS"], ens["S_PLUS"], equal_nan=True)
    assert np.array_equal(got["S_SMOOTH"], ens["S_SMOOTH"], equal_nan=True)
    assert (got["status"] == ens["status"]).all()
    # both lane mappings of the 3-state filter give the same study
    for shape in (1, 3):
        alt = batch.lookahead(w, truth, N, 25, 10, device=gpu_device, shape=shape)
        _same(alt, exp, ARRAYS)


@pytest.mark.parametrize("R,LL,F,M,kind", [(3, 60, 5, 10, "F<M"), (3, 60, 1, 10, "F=1"), (3, 60, 12, 1, "M=1"),
                                           (2, 40, 40, 8, "F=LL"), (3, 60, 14, 6, "TOTALCASES"), (3, 60, 9, 4, "R_scalar"),
                                           (3, 60, 11, 5, "no zeros")])
def test_lookahead_edge_cases(gpu_device, R, LL, F, M, kind):
    from epidemicmodeling_amd import batch
    w, truth, N = _case(R, LL, zeros=kind != "no zeros")
    if kind == "TOTALCASES":
        w.obs_type = "TOTALCASES"
        w.x = np.ascontiguousarray(np.nancumsum(w.x, axis=0))
    if kind == "R_scalar":
        w.R_scalar = np.ascontiguousarray(np.nanmean(w.R_series, axis=0))
        w.R_series = None
    got = batch.lookahead(w, truth, N, F, M, device=gpu_device, chains=True)
    exp = LR.expected(w, truth, N, F, M)
    _same(got, exp, ARRAYS + ("S_PLUS", "S_SMOOTH"))
    if F < M:
        assert all(np.isnan(got[n]).all() for n in ARRAYS[2:])
    if F == LL:                                   # the last start hides every observation: a pure prediction
        assert np.isnan(got["est_plus"][F - 1]).sum() < got["est_plus"][F - 1].size


def test_lookahead_host_entry_matches_device_entry(gpu_device):
    from epidemicmodeling_amd import _lib, batch
    w, truth, N = _case(5, 120)
    dev = batch.lookahead(w, truth, N, 30, 12, device=gpu_device, chains=True)
    host = batch.lookahead_host(w, truth, N, 30, 12, device=0, chains=True)
    _same(host, dev, ARRAYS + ("S_PLUS", "S_SMOOTH", "status"))
    host2 = batch.lookahead_host(w, truth, N, 30, 12, device=0, placement_tries=2)
    _same(host2, dev, ARRAYS)
    with pytest.raises(_lib.EpiError, match="must not exceed LL"):
        batch.lookahead_host(w, truth, N, 121, 12, device=0)
    with pytest.raises(_lib.EpiError, match="MaxLookAheadDays"):
        batch.lookahead_host(w, truth, N, 30, 0, device=0)


def test_forecast_quality_pipeline(gpu_device):
    from epidemicmodeling_amd import pipeline, synth
    raw = synth.make_raw_counts(n_regions=8, T=200, seed=3)
    F, M = 30, 20
    fq = pipeline.forecast_quality(raw["cases"], raw["deaths"], raw["population"], raw["ip"], F, max_lookahead=M,
                                   device=gpu_device, chains=True)
    T = 200 - F
    pr = pipeline.prescribe(raw["cases"][:T], raw["deaths"][:T], raw["population"], raw["ip"][:T], horizon=10, n_eps=4,
                            device=gpu_device)
    for k in ("alpha_round1", "alpha_round2", "X_reg"):
        assert np.array_equal(fq[k], pr[k], equal_nan=True), k
    for k in ("fit1", "fit2", "pre"):
        for kk in pr[k]:
            assert np.array_equal(fq[k][kk], pr[k][kk], equal_nan=True), (k, kk)
    assert np.array_equal(fq["R_mean"], pr["R_mean"], equal_nan=True)
    w = fq["workload"]
    assert w.T == 200 and np.array_equal(w.x, fq["pre_entire"]["x_new"], equal_nan=True)
    assert np.array_equal(w.R_series[:T], pr["pre"]["R_v"], equal_nan=True)
    exp = LR.expected(w, fq["truth"], np.asarray(raw["population"], dtype=np.float64), F, M)
    _same(fq, exp, ARRAYS + ("S_PLUS", "S_SMOOTH"))


def test_lookahead_article_size_sampled(gpu_device):
    """236 regions x 366 days, F = 91, M = 60 (testScripts/testIEEEJSTSP2021ArticleResults.m:72): every chain of 16 regions
    against the oracle and the restatement."""
    from epidemicmodeling_amd import batch
    R, LL, F, M = 236, 366, 91, 60
    w, truth, N = _case(R, LL)
    got = batch.lookahead(w, truth, N, F, M, device=gpu_device, chains=True)
    idx = np.sort(np.concatenate([[0, R - 1], np.random.default_rng(11).choice(np.arange(1, R - 1), 14, replace=False)]))
    exp = LR.expected(LR.regions(w, idx), truth[:, idx], N[idx], F, M, n_threads=16)
    _same(got, exp, ARRAYS, cols=idx)
    chains = (idx[:, None] * F + np.arange(F)[None, :]).ravel()
    for n in ("S_PLUS", "S_SMOOTH"):
        assert np.array_equal(got[n][:, :, chains], exp[n], equal_nan=True), n


def test_forecast_quality_example_runs(tmp_path, gpu_device):
    root = H.ROOT
    out = tmp_path / "errors.csv"
    res = subprocess.run([sys.executable, os.path.join(root, "examples", "forecast_quality_from_csv.py"), str(out)],
                         capture_output=True, text=True, timeout=600, cwd=root)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = out.read_text().splitlines()
    assert lines[0].split(",")[:6] == ["region", "lookahead_day", "mean_plus", "median_plus", "std_plus", "mean_smooth"]
    assert len(lines) > 1


# ---------------------------------------------------------------- the validated limits: n = F - M + 1 up to kLaMaxF = 1024
def _est(S, N, t, c):
    """((N * s) * i) * alpha of chain c on day t, in the kernel's operation order"""
    return ((N * S[t, 0, c]) * S[t, 1, c]) * S[t, 2, c]


def _limit_case(LL, F, M):
    """Five regions whose columns of the tables hold the values the median's ranking and midpoint must get right, over
    n = F - M + 1 rows.  The chains do not depend on truth or population, so they are run once and the truth is derived
    from them.  Returns (w, truth, N, expected)."""
    from epidemicmodeling_amd import synth
    R = 5
    w = synth.make_cfg3(R, LL)
    N = synth.make_regions(R)["N"].astype(np.float64)
    ch = H.oracle_batch(LR.mask_ensemble(w, F), n_threads=16, outputs=["S_PLUS", "S_SMOOTH"])
    SP = ch["S_PLUS"]
    truth = w.x * N[None, :] + 50.0
    n = F - M + 1
    rows = np.arange(M, F + 1)                                   # the starts s of the rows the statistics read
    # region 0: zero truth days (+Inf entries) on every third row of column j = M, and a NaN truth day behind row index
    # min(70, n - 1) of column j = 1 (median NaN, mean / std still written)
    truth[LL - rows[::3] + M - 1, 0] = 0.0
    truth[LL - (M + min(70, n - 1)), 0] = np.nan
    # region 1: population 0 -> every estimate is 0 and every finite entry is +-100 (ties everywhere); the sign of the truth
    # alternates in runs of 3 days, so the two middle values differ in sign for even n
    N[1] = 0.0
    truth[:, 1] = np.where((np.arange(LL) // 3) % 2 == 0, 1.0, -1.0) * (np.arange(LL) + 5.0)
    # region 2: negative population and truth = the PLUS estimate on two rows of three of column j = 1: those entries are
    # -0 (0 / negative), tied with each other; the rest are large positive values
    N[2] = -N[2]
    for s in rows[(rows % 3) != 0]:
        truth[LL - s, 2] = _est(SP, N[2], LL - s, 2 * F + s - 1)
    # region 3: truth = the PLUS estimate on the even rows of column j = 1: +0 entries, tied; the odd rows stay positive
    for s in rows[rows % 2 == 0]:
        truth[LL - s, 3] = _est(SP, N[3], LL - s, 3 * F + s - 1)
    # region 4: zero truth days on two rows of three of column j = 1: +Inf is the majority, so both middle order statistics
    # are +Inf and the even-n midpoint must take its (a + b) / 2 arm (a + (b - a) / 2 would give Inf + NaN = NaN)
    truth[LL - rows[(rows % 3) != 0], 4] = 0.0
    truth = np.ascontiguousarray(truth)
    tp, ts = LR.tables(SP, ch["S_SMOOTH"], truth, N, F, M)
    exp = {"est_plus": tp, "est_smooth": ts, "S_PLUS": SP, "S_SMOOTH": ch["S_SMOOTH"]}
    exp.update(LR.stats_of(tp, ts, M))
    return w, truth, N, exp


LIMITS = [(80, 70, 8), (80, 70, 7), (80, 72, 8), (140, 130, 3), (1030, 1024, 2), (1030, 1024, 1)]   # n = 63 64 65 128 1023 1024


def _bits(a, b):
    """bit for bit, -0 / +0 included; only a NaN's payload and sign are free"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64))


@pytest.mark.parametrize("LL,F,M", LIMITS, ids=[f"n{F - M + 1}" for _, F, M in LIMITS])
def test_lookahead_stats_at_the_row_limits(gpu_device, LL, F, M):
    """lookahead_stats stages and ranks n = F - M + 1 rows per column in strides of the wavefront: every lane makes a second
    pass from n = 65 on, and F = 1024 is the validated maximum.  Tables, statistics and chains bit for bit."""
    from epidemicmodeling_amd import batch
    w, truth, N, exp = _limit_case(LL, F, M)
    got = batch.lookahead(w, truth, N, F, M, device=gpu_device, chains=True)
    for k in ARRAYS + ("S_PLUS", "S_SMOOTH"):
        assert got[k].shape == exp[k].shape and _bits(got[k], exp[k]), k
    n = F - M + 1
    # the columns hold what _limit_case built them to hold
    assert np.isnan(got["median_plus"][0, 0]) and np.isnan(got["mean_plus"][0, 0])
    assert np.isinf(got["est_plus"][M - 1:, M - 1, 0]).any()
    assert set(np.abs(got["est_plus"][M - 1:, 0, 1]).tolist()) == {100.0}
    col2 = got["est_plus"][M - 1:, 0, 2]
    assert ((col2 == 0) & np.signbit(col2)).sum() >= n // 2
    col3 = got["est_plus"][M - 1:, 0, 3]
    assert ((col3 == 0) & ~np.signbit(col3)).sum() >= n // 2 - 1
    col4 = np.sort(got["est_plus"][M - 1:, 0, 4])
    assert np.isposinf(col4[(n - 1) // 2]) and np.isposinf(col4[n // 2]) and got["median_plus"][0, 4] == np.inf
    _check_stats_exactly(got, M)


def _check_stats_exactly(got, M):
    """The statistics against an exact reading of the GPU's own tables (fractions.Fraction), column by column.
    mean: recursive summation of n terms and one division: |fl(mean) - mean| <= (n + 1) u sum|x| / n (u = 2^-53; Higham,
    Accuracy and Stability, (4.4)).  std: with the computed mean off by delta, sum (x - mean~)^2 = S + n delta^2 exactly (S the
    exact sum of squares about the exact mean); each term (x - mean~)^2 carries 3 roundings and the sum n - 1 more, the
    division one and the square root one, so |fl(std) - std| <= std ((n + 4) u + n delta^2 / S) / 2 + u std + u std, taken
    with delta at its bound.  median: sorted(column)'s middle element (odd n), MATLAB's midpoint as documented (even n)."""
    from fractions import Fraction
    u = 2.0 ** -53
    for side in ("plus", "smooth"):
        tbl = got["est_" + side]
        F, _, R = tbl.shape
        n = F - M + 1
        for j in range(M):
            for r in range(R):
                col = tbl[M - 1:, j, r]
                mean, std, med = got["mean_" + side][j, r], got["std_" + side][j, r], got["median_" + side][j, r]
                if np.isnan(col).any():
                    assert np.isnan(med)
                    continue
                srt = sorted(col.tolist())
                a, b = srt[(n - 1) // 2], srt[n // 2]
                if n % 2:
                    want = a
                elif np.sign(a) != np.sign(b) or np.isinf(a) or np.isinf(b):
                    want = (a + b) / 2.0
                else:
                    want = a + (b - a) / 2.0
                assert _bits(med, want), (side, j, r)
                if not np.isfinite(col).all():
                    continue
                fx = [Fraction(float(v)) for v in col]
                m = sum(fx) / n
                sabs = sum(abs(v) for v in fx) / n
                mbound = (n + 1) * u * sabs
                assert abs(Fraction(float(mean)) - m) <= mbound + Fraction(5e-324), (side, j, r)
                if n == 1:
                    assert std == 0.0
                    continue
                S = sum((v - m) ** 2 for v in fx)
                if S == 0:
                    assert std == 0.0, (side, j, r)
                    continue
                ex = float(S / (n - 1)) ** 0.5
                rel = ((n + 4) * u + n * float(mbound) ** 2 / float(S)) / 2.0 + 2.0 * u
                assert abs(std - ex) <= rel * ex * (1 + 4 * u), (side, j, r, std, ex)


@pytest.mark.parametrize("entry", ["device", "host"])
def test_lookahead_optional_chain_outputs_alone(gpu_device, entry):
    """S_PLUS, S_SMOOTH and status are optional (NULL = not returned): off, each one alone and all three, in one poisoned
    arena with guards.  What is requested equals the all-outputs run bit for bit; no byte outside it changes."""
    import ctypes as C
    from epidemicmodeling_amd import _lib, batch
    w, truth, N = _case(3, 60)
    F, M = 14, 6
    R, LL = w.B, w.T
    ref = batch.lookahead(w, truth, N, F, M, device=gpu_device, chains=True)
    specs = [(n, (F, M, R), np.float64) for n in ("est_plus", "est_smooth")]
    specs += [(n, (M, R), np.float64) for n in ARRAYS[2:]]
    specs += [("S_PLUS", (LL, 3, R * F), np.float64), ("S_SMOOTH", (LL, 3, R * F), np.float64), ("status", (R * F,), np.int32)]
    r = batch.LookaheadRunner(w, truth, N, F, M, gpu_device)
    host_in = {k: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
               for k, v in batch._lookahead_arrays(w, truth, N).items()}
    for opt in ((), ("S_PLUS",), ("S_SMOOTH",), ("status",), ("S_PLUS", "S_SMOOTH", "status")):
        req = ARRAYS + opt
        ar = H.GuardArena(specs, device=gpu_device if entry == "device" else None)
        outs = _lib.LookaheadOutputs()
        for n in _lib.LA_OUT_NAMES:
            setattr(outs, n, C.c_void_p(ar.ptr(n)) if n in req else None)
        err = C.create_string_buffer(256)
        if entry == "device":
            import torch
            st = torch.cuda.current_stream(torch.device(gpu_device))
            rc = _lib.lib().epi_lookahead_run_device(C.byref(r.desc), C.byref(r.ins), C.byref(outs), C.c_void_p(r.ws.data_ptr()),
                                                     r.ws_bytes, C.c_void_p(st.cuda_stream), err)
        else:
            ins = _lib.LookaheadInputs()
            for n in _lib.LA_IN_NAMES:
                setattr(ins, n, None if host_in.get(n) is None else host_in[n].ctypes.data_as(C.c_void_p))
            rc = _lib.lib().epi_lookahead_run_host(C.byref(r.desc), C.byref(ins), C.byref(outs), 0, err)
        _lib.check(rc, err)
        for n in req:
            assert _bits(ar.get(n), ref[n]) if n != "status" else np.array_equal(ar.get(n), ref[n]), (opt, n)
        assert ar.untouched(req), opt

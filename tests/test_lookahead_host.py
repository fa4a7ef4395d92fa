"""CPU suite of the forecast look-ahead error study (Tools/ForecastQualityAssessment.m:359-393, 428-449): descriptor
validation of epi_lookahead_* (no GPU needed), and the restatement the GPU tests compare against (tests/lookahead_ref.py)
checked against a literal loop transcription of the .m code."""
import ctypes as C

import numpy as np
import pytest

from epidemicmodeling_amd import _lib
from tests import lookahead_ref as LR


def _desc(**kw):
    a = dict(R=4, LL=120, F=20, M=10, n_npi=12, L_=21)
    a.update(kw)
    return _lib.make_lookahead_desc(**a)


def _validate(hip_lib, d):
    err = C.create_string_buffer(256)
    rc = hip_lib.epi_lookahead_validate(C.byref(d), err)
    return rc, err.value.decode()


def test_lookahead_validate_rejects_bad_descriptors(hip_lib):
    assert _validate(hip_lib, _desc()) == (0, "")
    bad = [(dict(F=0), "F (num_forecast_days) must be >= 1"),
           (dict(F=121), "must not exceed LL"),
           (dict(M=0), "M (MaxLookAheadDays) must be >= 1"),
           (dict(LL=2000, F=1025), "limited to 1024"),
           (dict(R=0), "R and LL must be >= 1"),
           (dict(n_npi=13), "n_npi out of range"),
           (dict(shape=2), "shape must be")]
    for kw, msg in bad:
        rc, m = _validate(hip_lib, _desc(**kw))
        assert rc == -5 and msg in m, (kw, rc, m)
    rc, m = _validate(hip_lib, _desc(model="SIAlphaModelEKFOptControlled"))
    assert rc == -8 and "SIAlphaModelEKF" in m
    rc, m = _validate(hip_lib, _desc(order=3))
    assert rc == -1 and m == "Undefined order"
    d = _desc()
    d.abi_version = 5
    assert _validate(hip_lib, d)[0] == -5
    assert hip_lib.epi_lookahead_workspace_bytes(C.byref(_desc(F=0))) == 0
    # F == LL (every day masked) and F < M are valid
    assert _validate(hip_lib, _desc(F=120, M=200))[0] == 0


def test_lookahead_workspace_grows_with_regions_and_starts(hip_lib):
    ws = lambda **kw: int(hip_lib.epi_lookahead_workspace_bytes(C.byref(_desc(**kw))))
    base = ws()
    assert base > 0
    assert ws(R=8) > base and ws(F=40) > base
    # the masked per-chain observations alone: LL * R * F doubles
    assert base >= 120 * 4 * 20 * 8


def test_lookahead_host_entry_reports_validation_errors(hip_lib):
    """The host entry checks the descriptor before it touches a device."""
    d = _desc(F=0)
    ins, outs = _lib.LookaheadInputs(), _lib.LookaheadOutputs()
    err = C.create_string_buffer(256)
    rc = hip_lib.epi_lookahead_run_host(C.byref(d), C.byref(ins), C.byref(outs), 0, err)
    assert rc == -5 and "num_forecast_days" in err.value.decode()
    d = _desc()
    rc = hip_lib.epi_lookahead_run_host(C.byref(d), C.byref(ins), C.byref(outs), 0, err)
    assert rc == -5 and "NULL input array" in err.value.decode()


def _random_case(rng, R, LL, F, zero_truth=True):
    B = R * F
    SP = rng.uniform(0.1, 1.0, (LL, 3, B))
    SS = rng.uniform(0.1, 1.0, (LL, 3, B))
    truth = rng.uniform(10.0, 1000.0, (LL, R))
    pop = rng.uniform(1e3, 1e4, R)
    if zero_truth:
        truth[LL - 1, 0] = 0.0                                  # est != 0: Inf
        truth[LL - 2, 1 % R] = 0.0
        SP[LL - 2, 2, (1 % R) * F:(1 % R + 1) * F] = 0.0        # est == 0 too: 0 / 0 = NaN in the PLUS table
        SS[LL - 3, 0, :F] = -SP[LL - 3, 0, :F]                  # sign changes in the SMOOTH estimate
    return SP, SS, truth, pop


@pytest.mark.parametrize("R,LL,F,M", [(3, 40, 12, 5),      # n = 8 (even)
                                      (3, 40, 13, 5),      # n = 9 (odd)
                                      (2, 30, 6, 6),       # n = 1
                                      (2, 30, 4, 7),       # F < M: n <= 0
                                      (2, 20, 20, 3)])     # F = LL
def test_restatement_matches_loop_transcription(R, LL, F, M):
    rng = np.random.default_rng(R * 1000 + F * 10 + M)
    SP, SS, truth, pop = _random_case(rng, R, LL, F)
    tp, ts = LR.tables(SP, SS, truth, pop, F, M)
    EP, ES, st = LR.matlab_loop(SP, SS, truth, pop, F, M)
    assert np.array_equal(tp, EP, equal_nan=True) and np.array_equal(ts, ES, equal_nan=True)
    if F >= M:
        assert np.isinf(tp[:, :, 0]).any() or F < 1
    got = LR.stats_of(tp, ts, M)
    for k, v in got.items():
        ref = st[k]
        assert np.array_equal(np.isnan(v), np.isnan(ref)), k
        assert np.array_equal(np.isinf(v), np.isinf(ref)), k
        fin = np.isfinite(ref)
        assert np.array_equal(v[~fin], ref[~fin], equal_nan=True), k
        tol = 1e-15 if k.startswith("median") else 1e-12
        assert np.all(np.abs(v[fin] - ref[fin]) <= tol * np.abs(ref[fin])), (k, np.max(np.abs(v[fin] - ref[fin])))
    if F < M:
        assert all(np.isnan(v).all() for v in got.values())
    if F - M + 1 == 1:
        assert (got["std_plus"][np.isfinite(got["mean_plus"])] == 0).all()


def test_median_midpoint_rule():
    """Even n: a + (b - a) / 2, or (a + b) / 2 across a sign change or with an infinite value; NaN anywhere: NaN."""
    def med(vals):
        F = len(vals)
        tbl = np.zeros((F, 1, 1))
        tbl[:, 0, 0] = vals
        return LR.column_stats(tbl, 1)[1][0, 0]
    assert med([3.0, 1.0, 2.0]) == 2.0
    assert med([1.0, 4.0]) == 1.0 + (4.0 - 1.0) / 2.0
    assert med([-1.0, 4.0]) == 1.5
    assert med([1.0, np.inf]) == np.inf
    assert med([-np.inf, np.inf, 1.0, 2.0]) == 1.5
    assert np.isnan(med([1.0, np.nan, 2.0]))
    big = np.finfo(np.float64).max
    assert med([big, big]) == big                     # (a + b) / 2 would overflow
    rng = np.random.default_rng(5)
    for n in (2, 7, 32, 33, 1024):
        v = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4)
        assert abs(med(v) - np.median(v)) <= 1e-15 * abs(np.median(v))

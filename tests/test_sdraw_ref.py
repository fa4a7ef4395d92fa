"""The definition of the smoother draws without a GPU: the C yardstick tests/sdraw_ref.c and the NumPy reading
tests/sdraw_ref.np_sdraw agree bit for bit on the oracle's outputs of the 3-state workloads, and the two known answers hold:
(b) with z = None and the clamp the path IS the oracle's S_SMOOTH, (a) the moments of the law are the smoother's :218 / :223 --
deterministically against a 60-digit evaluation, and statistically over 4 096 draws -- and the planted days do what the
definition says."""
import numpy as np
import pytest

from tests import helpers as H
from tests import sdraw_ref as SR

NAMES = ("X", "rank", "status", "J", "L")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return SR.SdrawRef(tmp_path_factory.mktemp("sdraw_ref"))


def m33(v):
    return np.asarray(v).reshape(3, 3, order="F")


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("name", SR.WORKLOADS)
def test_c_and_numpy_agree(ref, name, storage):
    """NEWCASES and TOTALCASES, an R_v series and the adaptive scalar, a 30-day NaN tail; clamp 0 / 1, k0 = 0 / 7"""
    w, case = SR.oracle_case(name)
    assert {"cfg3": w.R_series is not None, "adaptive": w.R_scalar is not None, "total": w.obs_type == "TOTALCASES",
            "tail": bool(np.isnan(w.x[-30:]).all())}[name]
    for D, k0, clamp, zt in ((3, 0, True, np.float64), (2, 7, False, np.float64), (3, 7, True, np.float32)):
        z = SR.draws(w.T, k0, w.B, D, seed=k0 + D, dtype=zt)
        a = ref.run(case, D, z, k0=k0, clamp=clamp, storage=storage, out_f32=zt == np.float32)
        b = SR.np_sdraw(ref, case, D, z, k0=k0, clamp=clamp, storage=storage, out_f32=zt == np.float32)
        for k in NAMES:
            assert SR.same_bits(a[k], b[k]), (name, storage, D, k0, clamp, k)


@pytest.mark.parametrize("name", SR.WORKLOADS)
def test_zero_draws_are_s_smooth(ref, name):
    """property (b): every day of every chain, np.array_equal"""
    w, case = SR.oracle_case(name)
    for fn in (lambda: ref.run(case, 2), lambda: SR.np_sdraw(ref, case, 2)):
        X = fn()["X"]
        assert np.array_equal(X[:, :, 0::2], case["S_SMOOTH"]) and np.array_equal(X[:, :, 1::2], case["S_SMOOTH"]), name
    assert np.array_equal(ref.run(case, 1, k0=9)["X"], case["S_SMOOTH"][9:])


def test_zero_draws_with_s_final(ref):
    """(b) with s_final / Ps_final set: the terminal law is the last day of S_SMOOTH / P_SMOOTH"""
    import copy
    w = copy.copy(SR.oracle_case("cfg3")[0])
    w.s_final, w.Ps_final = w.s_final.copy(), w.Ps_final.copy()
    w.s_final[2] = 0.11
    w.Ps_final[8] = 1e-2
    case = SR.case_of(w, H.oracle_batch(w))
    assert not np.array_equal(case["S_SMOOTH"][-1], case["S_PLUS"][-1])
    got = ref.run(case, 1, s_term=case["S_SMOOTH"][-1], P_term=case["P_SMOOTH"][-1])
    assert np.array_equal(got["X"], case["S_SMOOTH"])
    assert not np.array_equal(ref.run(case, 1)["X"], case["S_SMOOTH"])
    # and the terminal factor is that of P_SMOOTH(T-1)
    for c in range(w.B):
        F = m33(got["L"][-1, :, c])
        P = m33(case["P_SMOOTH"][-1, :, c])
        assert np.abs(F @ F.T - P).max() <= 8 * SR.EPS * np.abs(P).max()


@pytest.mark.parametrize("name", SR.WORKLOADS)
def test_moments_deterministic(ref, name):
    """property (a): L L' + J P_s(k+1) J' from the call's own J, L and the oracle's P_SMOOTH against P_SMOOTH(k); the gate is 100 x
    the distance of that fp64 value from the same expression in 60-digit arithmetic, both relative to max |P+| of the workload.
    Measured (distance, mismatch): cfg3 2.9e-16, 6.0e-16; adaptive 3.5e-16, 3.5e-16; total 4.3e-18, 3.9e-17; tail 3.8e-16, 1.8e-16"""
    import mpmath as mp
    w, case = SR.oracle_case(name)
    o = ref.run(case, 1, want_x=False)
    scale = np.abs(case["P_PLUS"]).max()
    dist = gap = 0.0
    with mp.workdps(60):
        for c in range(w.B):
            for k in range(w.T - 1):
                J, F, Ps = m33(o["J"][k, :, c]), m33(o["L"][k, :, c]), m33(case["P_SMOOTH"][k + 1, :, c])
                v = F @ F.T + J @ Ps @ J.T
                Jm, Fm, Pm = (mp.matrix(a.tolist()) for a in (J, F, Ps))
                vm = Fm * Fm.T + Jm * Pm * Jm.T
                dist = max(dist, max(float(abs(mp.mpf(float(v[i, j])) - vm[i, j])) for i in range(3) for j in range(3)) / scale)
                gap = max(gap, float(np.abs(v - m33(case["P_SMOOTH"][k, :, c])).max()) / scale)
    print(f"{name}: distance of the fp64 expression from 60 digits {dist:.3e}, mismatch to P_SMOOTH {gap:.3e} (relative to max |P+|)")
    assert dist > 0.0 and gap <= 100.0 * dist, (name, dist, gap)


def test_moments_statistical(ref):
    """property (a) over D = 4 096 draws of the NumPy reading, clamp = 0, B = 4 x T = 60 (the workload with the NaN tail): every
    (day, row) sample mean within 6 standard errors of the unclamped mean recursion; entries of zero variance to 1e-12 max |m|"""
    w, case = SR.oracle_case("tail")
    D = 4096
    assert (w.B, w.T) == (4, 60)
    z = np.random.default_rng(20211104).standard_normal((w.T, 3, w.B * D))
    o = SR.np_sdraw(ref, case, D, z, clamp=False)
    checked = 0
    for c in range(w.B):
        m = case["S_PLUS"][-1, :, c].copy()
        F = m33(o["L"][-1, :, c])
        Cv = F @ F.T
        for k in range(w.T - 1, -1, -1):
            if k < w.T - 1:
                J, F = m33(o["J"][k, :, c]), m33(o["L"][k, :, c])
                m = case["S_PLUS"][k, :, c] + J @ (m - case["S_MINUS"][k + 1, :, c])
                Cv = J @ Cv @ J.T + F @ F.T
            mean = o["X"][k, :, c * D:(c + 1) * D].mean(axis=1)
            for i in range(3):
                if Cv[i, i] > 0.0:
                    assert abs(mean[i] - m[i]) <= 6.0 * np.sqrt(Cv[i, i] / D), (c, k, i, mean[i], m[i], Cv[i, i])
                else:
                    assert abs(mean[i] - m[i]) <= 1e-12 * np.abs(m).max(), (c, k, i)
                checked += 1
    assert checked == w.B * w.T * 3


def test_planted_days(ref):
    case = SR.planted_case()
    B, T = case["B"], case["T"]
    z = SR.draws(T, 0, B, 3, seed=6)
    for fn in (ref.run, lambda *a, **k: SR.np_sdraw(ref, *a, **k)):
        for clamp in (True, False):
            o = fn(case, 3, z, clamp=clamp)
            assert list(o["status"]) == [0, SR.NONFINITE, SR.RANK_DEFICIENT, SR.RANK_DEFICIENT, SR.NONFINITE]
            # an Inf in P_MINUS(3): J_2 = 0 by the guard and L_2 the factor of P_PLUS(2)
            P = m33(case["P_PLUS"][2, :, 1])
            F, rk = ref.pchol((P + P.T) / 2.0)
            assert not o["J"][2, :, 1].any() and SR.same_bits(m33(o["L"][2, :, 1]), np.array(F)) and o["rank"][2, 1] == rk == 3
            assert np.abs(F @ F.T - P).max() <= 8 * SR.EPS * np.abs(P).max()
            # a rank-1 P_PLUS on the last day, a zero one on day 1: the rank, zero columns
            L5 = m33(o["L"][5, :, 2])
            assert o["rank"][5, 2] == 1 and not L5[:, 1:].any() and L5[:, 0].all()
            assert o["rank"][1, 3] == 0 and not o["L"][1, :, 3].any()
            assert (np.delete(o["rank"][:, 2], 5) == 3).all()
            # a NaN in P_PLUS(3): a NaN record, and NaN paths from that day down, clamped or not
            assert o["rank"][3, 4] == -1 and np.isnan(o["J"][3, :, 4]).all() and np.isnan(o["L"][3, :, 4]).all()
            X4 = o["X"][:, :, 4 * 3:5 * 3]
            assert np.isnan(X4[:4]).all() and np.isfinite(X4[4:]).all()
            assert np.isfinite(o["X"][:, :, :4 * 3]).all()

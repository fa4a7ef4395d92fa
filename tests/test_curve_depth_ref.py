"""The two restatements of the curve statistics without a device: tests/curve_depth_ref.py equals
tests/curve_depth_ref.c bit for bit, equals literal pair enumeration on tied data and the rank formula on tie-free data, and has
the invariances and degenerate cases the definition promises."""
import numpy as np
import pytest

from tests import curve_depth_ref as S
from tests import ens_summary_ref as E


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return S.CurveDepthC(tmp_path_factory.mktemp("curve_depth_ref"))


def _same(got, want, names=S.NAMES):
    for k in names:
        assert S.same_bits(got[k], want[k]), k


CASES = [dict(), dict(storage="f32"), dict(D=64, derive=False), dict(rows=1, derive=False, D=5, R=3, first_day=None),
         dict(D=12, T=70, k0=1, k1=69, first_day=(40, 0)), dict(D=1), dict(D=2), dict(D=130, R=1, T=9, k0=0, k1=9, first_day=(9,))]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_python_equals_c_bit_for_bit(cref, case):
    kw = S.base_case(**CASES[case])
    for opt in (dict(), dict(alpha=(0.25, 0.5, 1.0), fence_factor=0.5, fence_frac=0.3), dict(alpha=(), fence_factor=0.0),
                dict(alpha=tuple(np.linspace(0.1, 1.0, 8)), fence_factor=3.0, fence_frac=1.0)):
        _same(S.statistics(**kw, **opt), cref.statistics(**kw, **opt))


def test_equals_pair_enumeration_with_ties():
    rng = np.random.default_rng(7)
    for D, T in ((2, 1), (3, 4), (5, 7), (9, 3), (8, 7)):
        v = rng.integers(0, 3, size=(T, 1, D)).astype(np.float64)          # values from {0, 1, 2}: every day has ties
        v[rng.random(v.shape) < 0.1] = np.nan
        got = S.statistics(v, 1, D, alpha=(), fence_factor=0.0)
        band, pairs = S.pair_enumeration(v[:, 0, :])
        assert (got["band_count"][0] == band).all() and (got["pair_total"][0] == pairs).all(), (D, T)


def test_equals_the_rank_formula_without_ties():
    rng = np.random.default_rng(8)
    T, D = 11, 37
    v = rng.standard_normal((T, 1, D))
    got = S.statistics(v, 1, D, alpha=(), fence_factor=0.0)
    rank = v[:, 0].argsort(axis=1).argsort(axis=1) + 1                      # 1 .. D
    band = ((rank - 1) * (D - rank) + D - 1).sum(axis=0)
    assert (got["band_count"][0] == band).all() and (got["pair_total"][0] == T * D * (D - 1) // 2).all()
    assert (got["mhi"][0] == rank.sum(axis=0) / (T * D)).all()
    assert S.same_bits(got["depth"][0], band / (T * D * (D - 1) // 2))


def test_invariance_under_monotone_maps_and_the_mirror():
    rng = np.random.default_rng(9)
    T, D, R = 9, 21, 2
    v = rng.standard_normal((T, 2, R * D))
    v[3, 0, 4] = np.nan
    a = S.statistics(v, R, D)
    b = S.statistics(np.exp(v) * 3.0 + 1.0, R, D)                           # strictly increasing
    c = S.statistics(-v, R, D)
    for k in ("depth", "depth_rank", "band_count", "pair_total", "n_valid", "n_ranked", "median_path"):
        assert S.same_bits(a[k], b[k]) and S.same_bits(a[k], c[k]), k
    assert S.same_bits(a["mhi"], b["mhi"])
    # the mirror of the hypograph index counts the members at or ABOVE the path; without ties le + ge = n_t + 1 on every valid day,
    # so (mhi + its mirror) * member_total = member_total + n_valid
    members = np.zeros_like(a["mhi"])
    for q in range(2):
        for r in range(R):
            ok = ~np.isnan(v[:, q, r * D:(r + 1) * D])
            members[q, r * D:(r + 1) * D] = (ok * ok.sum(axis=1, keepdims=True)).sum(axis=0)
    assert np.allclose((a["mhi"] + c["mhi"]) * members, members + a["n_valid"], rtol=0, atol=1e-9)


def test_permuting_the_draws_permutes_the_paths():
    T, D = 13, 33
    for seed in range(10, 30):                                              # depths are ratios of small integers: take a tie-free draw
        rng = np.random.default_rng(seed)
        v = rng.standard_normal((T, 1, D))
        a = S.statistics(v, 1, D)
        if len(np.unique(a["depth"])) == D:
            break
    assert len(np.unique(a["depth"])) == D
    perm = rng.permutation(D)
    b = S.statistics(v[:, :, perm], 1, D)
    for k in S.PATH_F64 + S.PATH_I32:
        assert S.same_bits(a[k][:, perm], b[k]), k
    assert perm[b["median_path"][0, 0]] == a["median_path"][0, 0]
    for k in S.ENV + S.DAY:
        assert S.same_bits(a[k], b[k]), k


def test_full_envelope_is_the_ensemble_min_and_max():
    rng = np.random.default_rng(11)
    T, D, R = 6, 19, 2
    v = rng.standard_normal((T, 2, R * D))
    pop = rng.uniform(1e3, 1e4, R)
    v = np.concatenate([v, rng.standard_normal((T, 1, R * D))], axis=1)
    got = S.statistics(v, R, D, alpha=(1.0,), population=pop)
    want = E.summary(v, R, D, (0.5,), population=pop)
    assert (got["n_ranked"] == D).all()
    assert S.same_bits(got["env_lo"][:, 0], np.asarray(want["min"])) and S.same_bits(got["env_hi"][:, 0], np.asarray(want["max"]))


def test_envelopes_are_nested_and_hold_the_median_curve():
    kw = S.base_case(seed=3)
    al = (0.1, 0.3, 0.5, 0.9, 1.0)
    got = S.statistics(**kw, alpha=al)
    lo, hi, mc = got["env_lo"], got["env_hi"], got["median_curve"]
    for k in range(len(al)):
        ok = ~np.isnan(mc) & ~np.isnan(lo[:, k])
        assert (lo[:, k][ok] <= mc[ok]).all() and (mc[ok] <= hi[:, k][ok]).all()
        if k:
            ok = ~np.isnan(lo[:, k - 1])
            assert not np.isnan(lo[:, k][ok]).any()
            assert (lo[:, k][ok] <= lo[:, k - 1][ok]).all() and (hi[:, k][ok] >= hi[:, k - 1][ok]).all()
    assert np.isnan(lo[:kw["k0"]]).all() and np.isnan(mc[kw["k1"]:]).all()


def test_degenerate_cases(cref):
    one = S.statistics(np.arange(5.0).reshape(5, 1, 1), 1, 1)              # D = 1: no pair anywhere
    assert one["pair_total"][0, 0] == 0 and np.isnan(one["depth"][0, 0]) and one["n_ranked"][0, 0] == 0
    assert one["depth_rank"][0, 0] == -1 and one["median_path"][0, 0] == -1 and one["n_valid"][0, 0] == 5 and one["mhi"][0, 0] == 1.0
    assert np.isnan(one["env_lo"]).all() and np.isnan(one["median_curve"]).all() and one["n_outliers"][0, 0] == 0
    two = S.statistics(np.array([[[1.0, 2.0]], [[4.0, 3.0]]]), 1, 2)       # D = 2: the one band holds both
    assert (two["depth"] == 1.0).all() and list(two["depth_rank"][0]) == [0, 1] and two["median_path"][0, 0] == 0
    v = np.random.default_rng(12).standard_normal((6, 1, 7))
    v[0, 0, 1:] = np.nan                                                   # n_t = 1
    v[1, 0, :] = np.nan                                                    # n_t = 0
    v[:, 0, 3] = np.nan                                                    # a path that is NaN throughout
    v[2, 0, 0], v[2, 0, 1], v[3, 0, 2] = np.inf, np.inf, -np.inf
    v[:, 0, 5] = v[:, 0, 4]                                                # identical paths
    got = S.statistics(v, 1, 7, alpha=(0.5, 1.0))
    _same(got, cref.statistics(v, 1, 7, alpha=(0.5, 1.0)))
    assert got["n_valid"][0, 3] == 0 and np.isnan(got["depth"][0, 3]) and np.isnan(got["mhi"][0, 3]) and got["depth_rank"][0, 3] == -1
    assert got["n_ranked"][0, 0] == 6 and got["n_valid"][0, 0] == 5
    assert got["depth"][0, 4] == got["depth"][0, 5] and got["depth_rank"][0, 5] == got["depth_rank"][0, 4] + 1
    assert np.isnan(got["env_lo"][1]).all() and got["env_hi"][2, 1, 0, 0] == np.inf and got["env_lo"][3, 1, 0, 0] == -np.inf
    band, pairs = S.pair_enumeration(v[:, 0, :])
    assert (got["band_count"][0] == band).all() and (got["pair_total"][0] == pairs).all()


def test_the_curve_envelope_keeps_the_peak_a_daily_quantile_flattens():
    """201 identical bumps of height 1 whose centres are spread over days 30 .. 90 of 120"""
    T, D = 120, 201
    t = np.arange(T, dtype=np.float64)[:, None]
    v = np.exp(-0.5 * ((t - np.linspace(30.0, 90.0, D)[None, :]) / 5.0) ** 2)[:, None, :]
    got = S.statistics(v, 1, D, alpha=(0.5,))
    q75 = np.asarray(E.summary(v, 1, D, (0.75,))["quantiles"])[:, 0, 0, 0]
    peak = got["env_hi"][:, 0, 0, 0].max()
    assert peak == 1.0 and q75.max() < 0.6 and peak > q75.max()
    assert got["median_path"][0, 0] == D // 2

"""The two restatements of the probabilistic forecast scores (tests/escore_ref.py in NumPy with the wavefront's tree restated,
tests/escore_ref.c sequential C) against each other bit for bit, and against what the scores are by definition."""
import numpy as np
import pytest

from tests import ens_summary_ref as E
from tests import escore_ref as S


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return S.EscoreC(tmp_path_factory.mktemp("escore_ref"))


def _case(D, seed, R=3, T=4, rows=3, f32=False):
    rng = np.random.default_rng(seed)
    src = rng.standard_normal((T, rows, R * D)) * 10.0 ** rng.uniform(-2, 2, size=(T, rows, 1))
    truth = rng.standard_normal((T, rows, R)) * np.abs(src).mean(axis=2, keepdims=True)
    return (src.astype(np.float32) if f32 else src), truth


def _same(a, b, names=S.NAMES):
    for k in names:
        assert S.same_bits(a[k], b[k]), k


@pytest.mark.parametrize("D", [1, 2, 7, 64, 65, 300])
def test_restatements_agree(cref, D):
    for f32 in (False, True):
        src, truth = _case(D, seed=D, f32=f32)
        src[0, 1, :D] = np.nan                                          # an item without members
        src[1, 0, D:2 * D:2] = np.nan                                   # half the members absent
        truth[2, 2, 1] = np.nan
        truth[3, 0, 0] = src[3, 0, D // 2]                              # the truth equal to a member
        kw = dict(alpha=(0.8, 0.5, 0.05), n_bins=10, first_day=[0, 2, 5], k0=1, k1=4)
        _same(S.score(src, truth, 3, D, **kw), cref.score(src, truth, 3, D, **kw))
    src, truth = _case(D, seed=50 + D, rows=3)
    src = np.abs(src)
    pop = np.array([1e6, 2e6, 3e7])
    truth = np.concatenate([truth, truth[:, :1] * 1e6], axis=1)
    kw = dict(alpha=(), n_bins=32, population=pop, truth_series=None)
    _same(S.score(src, truth, 3, D, **kw), cref.score(src, truth, 3, D, **kw))


@pytest.mark.parametrize("n", [1, 2, 7, 64, 65, 300])
def test_crps_equals_the_double_sum(n):
    rng = np.random.default_rng(n)
    for trial in range(6):
        v = rng.standard_normal(n) * 3.0
        if trial == 1:
            v = np.round(v)                                             # tied members
        y = [rng.standard_normal() * 3.0, v[n // 2], v.min() - 1.0, v.max() + 1.0, np.round(v)[0], 0.25][trial]
        got, want = S.item(v, y, ())["crps"], S.crps_double_sum(v, y)
        assert abs(got - want) <= 1e-12, (n, trial, got, want)
    v = rng.standard_normal(n + 5)
    v[:5] = np.nan                                                      # absent members do not count
    assert abs(S.item(v, 0.1, ())["crps"] - S.crps_double_sum(v, 0.1)) <= 1e-12


def test_one_member():
    for x, y in ((1.5, -2.25), (3.0, 3.0), (-1e300, 1e300)):
        it = S.item([x], y, (0.5,))
        assert it["crps"] == abs(x - y) and it["ae"] == abs(x - y) and it["count"] == 1
        assert it["width"][0] == 0.0 and it["cover"] == int(x == y)


def test_permuting_the_members_changes_only_the_tree_inputs_order():
    """the scores are functions of the sorted members: a permutation of the draws changes nothing at all (the tree runs over
    sorted positions, not over draws), unlike ensemble_summary's mean"""
    rng = np.random.default_rng(3)
    v = rng.standard_normal(300)
    v[7] = np.nan
    a = S.item(v, 0.3, (0.5, 0.05))
    b = S.item(v[rng.permutation(300)], 0.3, (0.5, 0.05))
    for k in a:
        assert S.same_bits(np.asarray(a[k]), np.asarray(b[k])), k
    x = np.sort(v[~np.isnan(v)])
    terms = S.crps_terms(x, 299, np.float64(0.3), 300)
    assert len(terms) == 512 and (terms[299:] == 0.0).all() and not np.signbit(terms[299:]).any()
    assert a["crps"] == (2.0 / (299.0 * 299.0)) * E.tree(terms)


def test_wis_without_intervals_is_the_absolute_error():
    rng = np.random.default_rng(4)
    for D in (1, 2, 65):
        v = rng.standard_normal(D)
        it = S.item(v, 0.7, ())
        assert it["wis"] == it["ae"] == abs(0.7 - E.quantile(np.sort(v), D, 0.5)) and it["cover"] == 0 and len(it["width"]) == 0


def test_wis_by_hand():
    v = np.arange(1.0, 101.0)                                            # quantile at p: 100 p + 0.5
    it = S.item(v, 120.0, (0.5, 0.1))
    l50, u50, l90, u90 = 25.5, 75.5, 5.5, 95.5
    is50 = (u50 - l50) + (2 / 0.5) * (120.0 - u50)
    is90 = (u90 - l90) + (2 / 0.1) * (120.0 - u90)
    assert it["ae"] == 69.5 and it["cover"] == 0 and list(it["width"]) == [50.0, 90.0]
    assert abs(it["wis"] - (0.5 * 69.5 + 0.25 * is50 + 0.05 * is90) / 2.5) < 1e-12
    it = S.item(v, 30.0, (0.5, 0.1))
    assert it["cover"] == 0b11 and it["rank"] == 29 and it["ties"] == 1
    it = S.item(v, 10.0, (0.5, 0.1))
    assert it["cover"] == 0b10


def test_cover_and_histogram_are_consistent_with_rank():
    D, R, T = 65, 3, 40
    src, truth = _case(D, seed=9, T=T, rows=1)
    truth[5, 0, 1] = np.nan
    out = S.score(src, truth, R, D, alpha=(0.5, 0.05), n_bins=10, first_day=[0, 3, 39])
    assert (out["n_scored"][0] == [40, 36, 1]).all()
    assert (out["pit_hist"].sum(axis=0) == out["n_scored"]).all()
    rk, ti, n = out["rank"], out["ties"], out["count"]
    ok = rk >= 0
    assert (rk[ok] + ti[ok] <= n[ok]).all() and (n == D).all()
    # a truth outside the ensemble is outside every central interval; a truth strictly inside the inner half is in both
    outside = ok & ((rk == 0) | (rk == n)) & (ti == 0)
    assert outside.any() and (out["cover"][outside] == 0).all()
    inner = ok & (rk > 0.3 * n) & (rk + ti < 0.7 * n)
    assert inner.any() and (out["cover"][inner] == 3).all()
    assert (((out["cover"] >> 1) & 1) >= (out["cover"] & 1)).all()      # the 95 % interval holds the 50 % one
    for r, fd in enumerate((0, 3, 39)):
        sel = ok[fd:, 0, r]
        assert out["cover_frac"][1, 0, r] == ((out["cover"][fd:, 0, r][sel] >> 1) & 1).sum() / sel.sum()
        bins = [S.pit_bin(a, b, c, 10) for a, b, c in zip(rk[fd:, 0, r][sel], ti[fd:, 0, r][sel], n[fd:, 0, r][sel])]
        assert (np.bincount(bins, minlength=10) == out["pit_hist"][:, 0, r]).all()
    assert S.pit_bin(0, 0, 65, 10) == 0 and S.pit_bin(65, 0, 65, 10) == 9 and S.pit_bin(0, 65, 65, 10) == 5
    assert S.pit_bin(4096, 0, 4096, 32) == 31 and S.pit_bin(1, 0, 1, 1) == 0


def test_no_scored_day():
    src, truth = _case(7, seed=2)
    out = S.score(src, truth, 3, 7, n_bins=4, k0=2, k1=2)
    assert (out["n_scored"] == 0).all() and np.isnan(out["crps_mean"]).all() and np.isnan(out["cover_frac"]).all()
    assert (out["pit_hist"] == 0).all()


def test_non_finite_members():
    v = np.array([1.0, np.inf, -np.inf, 2.0, 3.0, np.nan])
    it = S.item(v, 2.5, (0.5,))
    assert it["count"] == 5 and it["rank"] == 3 and it["ae"] == 0.5 and it["crps"] == np.inf       # both infinite terms are +Inf
    it = S.item([np.inf, np.inf, np.inf, np.inf], 0.0, (0.5,))
    assert np.isnan(it["width"][0]) and np.isnan(it["wis"]) and it["cover"] == 0                  # Inf - Inf between two members
    it = S.item([1.0, 2.0, np.inf], 1.5, (0.5,))
    assert it["crps"] == np.inf and np.isnan(it["ae"])                                            # the median: 2 + 0 * (Inf - 2)

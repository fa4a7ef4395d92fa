"""tests/ens_summary_ref.py (the reference of the ensemble statistics) against NumPy's own quantile / mean / std and
against known answers.  No GPU.

Gates.  Quantiles: the reference and np.quantile(method="hazen") make the same few roundings (n p + 0.5, the difference of
two neighbours, one product, one sum) in a different order, each at most eps/2 relative to max|x| of the item: 4 eps max|x|.
Mean and std: a pairwise tree over P terms has log2(P) levels, each adding at most eps/2 relative to the partial sums'
magnitude, and NumPy's own pairwise sum is inside the same bound: log2(P) eps max|x| (the division by n and the square root
add one rounding each and are covered by the factor 2 between eps/2 per level and eps)."""
import numpy as np
import pytest

from tests import ens_summary_ref as E

EPS = np.finfo(np.float64).eps
NS = (1, 2, 3, 63, 64, 65, 1000, 1024, 4096)
PS = (0.0, 0.025, 0.25, 0.5, 0.75, 0.975, 1.0, 1.0 / 3.0)


def _data(n):
    rng = np.random.default_rng(1000 + n)
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3)


@pytest.mark.parametrize("n", NS)
def test_quantiles_match_numpy_hazen(n):
    v = _data(n)
    got = E.item(v, PS)["quantiles"]
    want = np.quantile(v, PS, method="hazen")
    gate = 4 * EPS * np.abs(v).max()
    worst = np.abs(got - want).max()
    print(f"n={n}: worst |diff| / max|x| = {worst / np.abs(v).max():.3e}")
    assert worst <= gate


@pytest.mark.parametrize("n", NS)
def test_mean_and_std_match_numpy(n):
    v = _data(n)
    it = E.item(v, PS)
    P = 1
    while P < n:
        P *= 2
    gate = max(1.0, np.log2(P)) * EPS * np.abs(v).max()
    assert abs(it["mean"] - np.mean(v)) <= gate
    if n > 1:
        assert abs(it["std"] - np.std(v, ddof=1)) <= gate
    else:
        assert it["std"] == 0.0
    assert it["min"] == v.min() and it["max"] == v.max() and it["count"] == n


def test_nan_members_are_excluded():
    v = _data(65)
    w = v.copy()
    w[[0, 17, 64]] = np.nan
    a, b = E.item(w, PS), E.item(np.delete(v, [0, 17, 64]), PS)
    assert a["count"] == 62 and np.array_equal(a["quantiles"], b["quantiles"]) and a["min"] == b["min"] and a["max"] == b["max"]
    assert abs(a["mean"] - b["mean"]) <= 7 * EPS * np.abs(v).max()


def test_known_answers():
    it = E.item(np.full(100, 3.25), PS)                       # all members equal
    assert it["mean"] == 3.25 and it["std"] == 0.0 and it["min"] == 3.25 and it["max"] == 3.25 and (it["quantiles"] == 3.25).all()
    it = E.item([7.0], PS)                                    # D = 1
    assert it["mean"] == 7.0 and it["std"] == 0.0 and (it["quantiles"] == 7.0).all() and it["count"] == 1
    it = E.item([np.nan] * 5, PS)                             # all members NaN
    assert it["count"] == 0 and all(np.isnan(it[k]) for k in ("mean", "std", "min", "max")) and np.isnan(it["quantiles"]).all()
    it = E.item([np.nan, np.nan, -2.5, np.nan], PS)           # exactly one member
    assert it["count"] == 1 and it["mean"] == -2.5 and it["std"] == 0.0 and it["min"] == -2.5 and (it["quantiles"] == -2.5).all()
    it = E.item([1.0, np.inf, -np.inf, 2.0], PS)              # both infinities
    assert np.isnan(it["mean"]) and it["min"] == -np.inf and it["max"] == np.inf and it["count"] == 4
    it = E.item([0.0, -0.0, 0.0, -0.0], PS)                   # zeros of both signs: values, not signs
    assert it["mean"] == 0.0 and it["std"] == 0.0 and it["min"] == 0.0 and it["max"] == 0.0 and (it["quantiles"] == 0.0).all()
    it = E.item([1.0, 2.0, 3.0, 4.0], [0.0, 0.5, 1.0, 0.25])  # MATLAB: quantile([1 2 3 4], .25) = 1.5
    assert list(it["quantiles"]) == [1.0, 2.5, 4.0, 1.5] and it["mean"] == 2.5


def test_tree_order():
    a = np.array([1.0, 2.0 ** -53, 2.0 ** -53, 0.0, 0.0])     # P = 8: (1 + 0) + (2^-53 + 0) ... differs from a sequential sum
    assert E.tree(a) == ((a[0] + a[4]) + a[2]) + (a[1] + a[3])
    assert E.tree([5.0]) == 5.0 and E.tree([1.0, 2.0, 3.0]) == (1.0 + 3.0) + 2.0


def test_derived_row_association():
    s = np.array([[[0.1, 0.7], [0.3, 0.2], [1e-3, 3.0]]])
    got = E.derived_row(s, [3.0, 7.0], 2, 1)
    assert got[0, 0] == ((3.0 * 0.1) * 0.3) * 1e-3 and got[0, 1] == ((7.0 * 0.7) * 0.2) * 3.0

"""The two restatements of the path functionals (tests/pathfn_ref.py in NumPy over all paths at once, tests/pathfn_ref.c sequential
C) against each other bit for bit, and against what the functionals are by definition: np.nanmax, the first argmax, a Python loop
for the runs (exactly equal), math.fsum for the total (within the bound of a recursive sum)."""
import math

import numpy as np
import pytest

from tests import pathfn_ref as S


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return S.PathfnC(tmp_path_factory.mktemp("pathfn_ref"))


CASES = [dict(), dict(storage="f32"), dict(D=64, n_thr=0), dict(rows=1, n_thr=8, derive=False, D=5), dict(rows=5, T=55, k0=0, k1=55, D=4),
         dict(T=65, k0=1, k1=65, first_day=None, n_thr=2, D=4), dict(T=200, k0=3, k1=199, first_day=(0, 100, 198), D=4)]


@pytest.fixture(scope="module", params=range(len(CASES)))
def case(request, cref):
    kw = S.base_case(**CASES[request.param])
    return kw, S.functionals(**kw), cref.functionals(**kw)


def test_restatements_agree(case):
    _, a, b = case
    for k in S.NAMES:
        assert S.same_bits(a[k], b[k]), k


def test_against_the_definition(case):
    kw, got, _ = case
    src, R, D, k0, k1 = kw["src"], kw["R"], kw["D"], kw["k0"], kw["k1"]
    x = S.rows_with_derived(src, kw["population"], R, D)
    T, ro, N = x.shape
    W = k1 - k0
    nt = 0 if kw["thr"] is None else len(kw["thr"])
    fd = np.zeros(R, dtype=int) if kw["first_day"] is None else kw["first_day"]
    eps = 2.0 ** -52
    seen_none = seen_all = False
    for q in range(ro):
        for p in range(N):
            r = p // D
            th = [float(kw["thr"][j, q, r]) for j in range(nt)]
            b = S.brute(x[:, q, p], max(k0, int(fd[r])), k1, th)
            if b is None:
                seen_none = True
                assert got["n_valid"][q, p] == 0
                for k in S.PATH_F64:
                    assert math.isnan(got[k][q, p]), (k, q, p)
                for k in S.THR_F64:
                    assert np.isnan(got[k][:, q, p]).all(), (k, q, p)
                continue
            pv, pd, mv, md, fs, sabs, nv, per = b
            assert got["n_valid"][q, p] == nv
            assert got["peak_value"][q, p] == pv and got["peak_day"][q, p] == pd, (q, p)
            assert got["min_value"][q, p] == mv and got["min_day"][q, p] == md, (q, p)
            if fs is not None:
                assert abs(got["total"][q, p] - fs) <= W * eps * sabs, (q, p, got["total"][q, p], fs)
            for j, t in enumerate(per):
                g = [got[k][j, q, p] for k in S.THR_F64]
                if t is None:
                    assert all(math.isnan(v) for v in g)
                    continue
                seen_all |= t[1] == nv and t[2] == nv and nv > 32
                assert (math.isnan(g[0]) if t[0] is None else g[0] == t[0]) and g[1] == t[1] and g[2] == t[2], (j, q, p, g, t)
    assert seen_none
    if nt > 1 and W > 32:
        assert seen_all
    # the per-region counts from the per-path outputs
    reg = S.regions(got["peak_day"], got["first_cross"], R, D, k0, W)
    for k in S.REGION:
        assert np.array_equal(reg[k], got[k]), k
    assert (got["peak_day_hist"].sum(axis=0) == got["n_paths"]).all() and (got["cross_day_hist"].sum(axis=0) == got["n_cross"]).all()
    assert (got["n_paths"] == (got["n_valid"] > 0).reshape(ro, R, D).sum(axis=2)).all()


def test_total_is_the_plain_sum_within_one_block(cref):
    rng = np.random.default_rng(5)
    for W in (1, 31, 32):
        src = rng.standard_normal((W + 2, 2, 6)) * 1e3
        src[3 % W + 1, 0, 1] = np.nan
        for f in (S.functionals, cref.functionals):
            got = f(src, 2, 3, k0=1, k1=W + 1)["total"]
            for q in range(2):
                for p in range(6):
                    s, n = 0.0, 0
                    for t in range(1, W + 1):
                        if not math.isnan(src[t, q, p]):
                            s, n = s + float(src[t, q, p]), n + 1
                    assert got[q, p] == s if n else math.isnan(got[q, p]), (W, q, p)


def test_planted_cases_by_hand():
    kw = S.base_case()
    out = S.functionals(**kw)
    k0, k1 = kw["k0"], kw["k1"]
    assert np.isnan(out["peak_value"][1, 2]) and np.isnan(out["total"][3, 2]) and out["n_valid"][1, 2] == 0 and out["n_valid"][0, 2] == k1 - k0
    assert out["peak_value"][0, 4] == np.inf and out["peak_day"][0, 4] == 20 and out["total"][0, 4] == np.inf
    assert out["min_value"][0, 5] == -np.inf and out["min_day"][0, 5] == 21
    assert out["peak_value"][0, 6] == 1e3 and out["peak_day"][0, 6] == 12
    assert out["first_cross"][0, 0, 7] == 30 and out["days_above"][0, 0, 7] == 1 and out["longest_run"][0, 0, 7] == 1
    assert out["longest_run"][0, 0, 3] == 14 and out["days_above"][0, 0, 3] >= 19                    # days 17 .. 30 after the NaN days
    assert out["longest_run"][0, 0, 8] == k1 - k0 and out["first_cross"][0, 0, 8] == k0
    assert (out["days_above"][1, 2, :70] == out["n_valid"][2, :70]).all()                             # the threshold -Inf
    assert np.isnan(out["first_cross"][2, 1]).all() and (out["n_cross"][2, 1] == 0).all()            # the NaN threshold
    assert out["total"][0, 9] == 0.0 and not np.signbit(out["total"][0, 9])
    assert (out["n_valid"][:, 140:] == 0).all() and (out["n_paths"][:, 2] == 0).all() and (out["n_paths"][0, :2] == 70).all()
    assert (out["n_valid"][0, 70:140] == 32).all() and (out["peak_day"][0, 70:140] >= 40).all()

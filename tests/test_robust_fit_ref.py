"""The two restatements of DESIGN.md §4.10 (tests/robust_fit_ref.py in NumPy, tests/robust_fit_ref.c in C) against each other
bit for bit, against analytic known answers, and -- independently of the tree, the bitonic sort and the closed-form solve --
against scipy's bounded least squares at the fixed point the iteration stops at.  No GPU."""
import numpy as np
import pytest

from tests import robust_fit_ref as RF

INF = np.inf
# (seed, D, n, R, robust, lower, upper, max_iter, planted)
CASES = [
    (1, 60, 1, 210, 1, 0.0, INF, 50, False),        # the generator as the issue states it: one NPI per item
    (2, 60, 12, 9, 1, 0.0, INF, 50, True),
    (3, 3, 2, 9, 1, 0.0, INF, 50, True),
    (4, 4, 2, 9, 1, 0.0, INF, 50, True),
    (5, 5, 1, 9, 1, 0.0, INF, 50, True),
    (6, 63, 2, 10, 1, 0.0, INF, 50, True),
    (7, 64, 1, 10, 1, -INF, INF, 50, True),
    (8, 65, 3, 8, 1, 0.0, 0.05, 50, True),
    (9, 129, 2, 8, 1, 0.0, INF, 3, True),
    (10, 236, 12, 7, 1, 0.0, INF, 50, True),
    (11, 1024, 1, 8, 1, 0.0, INF, 50, True),
    (12, 60, 3, 20, 0, -INF, INF, 50, True),
    (13, 60, 2, 20, 1, 0.0, INF, 1, True),
    (14, 40, 2, 12, 1, 0.02, 0.02, 50, False),
]
# worst max_d |fit - bvls fit| / max |y| of the restatement over CASES, in units of sqrt(eps), as measured when this file was
# written (test_fixed_point_against_bvls prints it); the gate is 4 x that (the margin covers the contraction factor of the
# iteration, which the stop rule does not bound)
WORST_FIXED_POINT = 0.485
GATE = 4.0 * WORST_FIXED_POINT * RF.SQRT_EPS


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return RF.RobfitRef(tmp_path_factory.mktemp("robfit"))


def _case(c):
    seed, D, n, R, robust, lower, upper, max_iter, planted = c
    X, y = RF.make_case(seed, D, n, R)
    kinds = RF.plant(X, y) if planted else []
    return X, y, dict(robust=robust, lower=lower, upper=upper, max_iter=max_iter), kinds


@pytest.fixture(scope="module")
def results(cref):
    """every case once: (X, y, args, the C restatement's outputs)"""
    out = []
    for c in CASES:
        X, y, kw, _ = _case(c)
        out.append((X, y, kw, cref.run(X, y, **kw)))
    return out


def test_c_and_numpy_agree_bit_for_bit(results):
    bits = 0
    for X, y, kw, got in results:
        want = RF.np_robust_fit(X, y, **kw)
        for k in RF.OUT_NAMES:
            assert RF.same_bits(got[k], want[k]), (X.shape, kw, k)
        bits |= int(np.bitwise_or.reduce(got["status"].ravel()))
    assert bits == 31                                            # the cases reach every status bit


def _one(x, y, **kw):
    r = RF.np_robust_fit(np.asarray(x, dtype=np.float64)[:, None, None], np.asarray(y, dtype=np.float64)[:, None], **kw)
    return {k: (v[:, 0, 0] if k == "weights" else v.ravel()[0]) for k, v in r.items()}


def test_kat_exact_line():
    x = np.arange(16.0) % 8
    y = 0.25 + 0.5 * x
    r = _one(x, y)
    assert r["a"] == 0.5 and r["b_item"] == 0.25 and r["b"] == 0.25 and r["status"] == 0 and r["iters"] == 1
    assert (r["weights"] == 1.0).all()
    assert r["sigma"] == 1e-6 * np.sqrt(np.sum((y - 2.0) ** 2) / 15.0)          # tiny: every term of the sum is exact


def test_kat_negative_slope_is_clamped():
    d = np.arange(40.0)
    x = d % 4
    y = 1.0 - 0.25 * x + 0.01 * np.cos(3.0 * d)
    r = _one(x, y)
    assert r["a"] == 0.0 and r["status"] == RF.BOUND
    w = r["weights"]
    assert r["b_item"] == RF.tree(w * y) / RF.tree(w)                            # the weighted location under the final weights
    assert abs(r["b_item"] - np.median(y)) < 0.2 and 0 < r["iters"] < 50
    free = _one(x, y, lower=-INF)
    assert abs(free["a"] + 0.25) < 0.01 and free["status"] == 0


def test_kat_equal_bounds_pin_the_slope():
    X, y = RF.make_case(21, 30, 2, 6)
    r = RF.np_robust_fit(X, y, lower=0.07, upper=0.07)
    live = (r["status"] & (RF.CONST | RF.SLOPE_LOST)) == 0
    assert live.any() and (r["a"][live] == 0.07).all() and ((r["status"][live] & RF.BOUND) != 0).all()
    assert (r["a"][~live] == 0.0).all()


def test_kat_unbounded_non_robust_is_ols():
    g = np.random.default_rng(5)
    x = g.integers(0, 5, 50).astype(np.float64)
    y = 0.3 - 0.07 * x + 0.05 * g.standard_normal(50)
    r = _one(x, y, robust=0, lower=-INF)
    a, b = np.polyfit(x, y, 1)
    assert abs(r["a"] - a) <= 1e-12 * abs(a) and abs(r["b_item"] - b) <= 1e-12 * abs(b)
    assert r["iters"] == 0 and np.isnan(r["sigma"]) and (r["weights"] == 1.0).all() and r["status"] == 0


def test_kat_constant_column():
    g = np.random.default_rng(6)
    y = 0.2 + 0.01 * g.standard_normal(30)
    y[7] += 3.0
    r = _one(np.full(30, 2.0), y)
    assert r["a"] == 0.0 and r["status"] == RF.CONST and r["weights"][7] == 0.0
    assert abs(r["b_item"] - np.delete(y, 7).mean()) < 0.005 and r["b"] == RF.tree(y[:, None])[0] * (1.0 / 30)


def test_kat_leverage_clip():
    x, y = np.array([0.0, 0.0, 1.0]), np.array([0.0, 1.0, 5.0])
    xb = x.mean()
    h = 1.0 / 3 + (x - xb) ** 2 / np.sum((x - xb) ** 2)
    assert h[2] > 0.9999                                                         # the third day's leverage is 1: clipped
    r = _one(x, y)
    assert np.isfinite([r["a"], r["b_item"], r["sigma"]]).all() and np.isfinite(r["weights"]).all() and r["status"] == 0
    assert abs(r["a"] - 4.5) < 1e-9 and abs(r["b_item"] - 0.5) < 1e-9
    # with the slope pinned at 0 the third day has a residual, and its weight after one reweighting shows the clipped factor
    r = _one(x, y, lower=0.0, upper=0.0, max_iter=1)
    res = y - 2.0
    adj = 1.0 / np.sqrt(1.0 - np.array([0.5, 0.5, 0.9999]))
    rs = np.sort(np.abs(res * adj))
    s = np.median(rs[1:]) / 0.6745
    u = res * adj / (s * 4.685)
    w = np.where(np.abs(u) < 1, (1 - u * u) ** 2, 0.0)
    assert np.allclose(r["weights"], w, rtol=1e-12, atol=0) and abs(adj[2] - 100.0) < 1e-9


def test_kat_gross_outlier():
    x = np.arange(30.0) % 5
    y = 0.125 + 0.375 * x
    yo = y.copy()
    yo[11] += 100.0
    r = _one(x, yo)
    assert r["weights"][11] == 0.0 and r["status"] == 0 and 0 < r["iters"] < 50
    ref = _one(np.delete(x, 11), np.delete(y, 11))
    assert abs(r["a"] - ref["a"]) <= RF.SQRT_EPS * max(abs(r["a"]), abs(ref["a"]))
    assert abs(r["b_item"] - ref["b_item"]) <= RF.SQRT_EPS * max(abs(r["b_item"]), abs(ref["b_item"]))


def test_kat_iteration_cap():
    X, y = RF.make_case(30, 60, 1, 4)
    r = RF.np_robust_fit(X, y, max_iter=1)
    assert (r["iters"] == 1).all() and ((r["status"] & RF.MAXITER) != 0).any()
    r50 = RF.np_robust_fit(X, y)
    assert ((r50["status"] & RF.MAXITER) == 0).all() and (r50["iters"] > 1).any()


def test_fixed_point_against_bvls(results):
    """For every item that stopped by the stop rule with an identified slope: weights recomputed from the returned (a, b) with
    plain np.sort / np.median code, the weighted bounded problem solved by scipy's BVLS, fitted values compared."""
    from scipy.optimize import lsq_linear
    worst, used, skipped = 0.0, 0, 0
    for X, y, kw, got in results:
        if not kw["robust"] or kw["max_iter"] != 50:                # the cases that cut the iteration short say nothing here
            continue
        D, n, R = X.shape
        for k in range(n):
            for r in range(R):
                st = got["status"][k, r]
                if st & (RF.CONST | RF.NONFINITE):
                    continue
                if st & (RF.MAXITER | RF.SLOPE_LOST):
                    skipped += 1
                    continue
                x, yy, a, b = X[:, k, r], y[:, r], got["a"][k, r], got["b_item"][k, r]
                h = np.minimum(0.9999, 1.0 / D + (x - x.mean()) ** 2 / np.sum((x - x.mean()) ** 2))
                radj = (yy - (a * x + b)) / np.sqrt(1.0 - h)
                s = np.median(np.sort(np.abs(radj))[1:]) / 0.6745
                tiny = 1e-6 * np.std(yy, ddof=1) or 1.0
                u = radj / (max(s, tiny) * 4.685)
                sw = np.sqrt(np.where(np.abs(u) < 1, (1 - u * u) ** 2, 0.0))
                A = np.stack([x, np.ones(D)], axis=1) * sw[:, None]
                lo, hi = kw["lower"], kw["upper"]
                if lo == hi:                                                      # lsq_linear wants lb < ub
                    sol_b = np.sum(sw * sw * (yy - lo * x)) / np.sum(sw * sw)
                    fit = lo * x + sol_b
                else:
                    sol = lsq_linear(A, yy * sw, bounds=([lo, -INF], [hi, INF]), method="bvls", tol=1e-15)
                    fit = sol.x[0] * x + sol.x[1]
                worst = max(worst, np.max(np.abs(fit - (a * x + b))) / np.max(np.abs(yy)))
                used += 1
    print(f"fixed point: worst {worst / RF.SQRT_EPS:.3f} sqrt(eps) over {used} items, {skipped} skipped")
    assert skipped <= 0.05 * (used + skipped), (used, skipped)
    assert worst <= GATE, worst / RF.SQRT_EPS

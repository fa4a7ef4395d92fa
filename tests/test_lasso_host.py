"""The cross-validated LASSO without a GPU: the C restatement (tests/lasso_ref.c, the GPU suite's yardstick) against a
plain-Python reading of DESIGN.md §4.5, the lasso optimality (KKT) conditions, scikit-learn's coordinate descent, and the
fold generator batch.lasso_folds."""
import numpy as np
import pytest

from tests.lasso_ref import LassoRef, np_lasso, ST_BAD_FOLDS, ST_MAXITER, ST_NONFINITE, ST_NULL_MODEL, ST_OK


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return LassoRef(tmp_path_factory.mktemp("lasso_ref"))


def make_problem(R, D, n, K, seed, specials=True):
    """X [D, n, R] shaped like NPI_MAXES - InterventionPlans (step functions on a few integer levels, some constant) mixed
    with continuous columns, y [D, R] an affine function of them plus noise (coefficients of both signs), fold [D, R].
    With specials (R >= 5, K >= 2): region 1 has a column that is constant except on fold 0's days, region 2 a constant y
    (null model), region 3 a NaN in X, region 4 only constant columns (null model)."""
    from epidemicmodeling_amd import batch
    rng = np.random.default_rng(seed)
    X = np.empty((D, n, R))
    for r in range(R):
        for j in range(n):
            kind = rng.integers(5)
            if kind == 0:
                X[:, j, r] = rng.standard_normal(D) * rng.uniform(0.1, 3.0)
            elif kind == 1:
                X[:, j, r] = float(rng.integers(0, 4))
            else:
                lv = rng.integers(0, 5, size=4).astype(float)
                cuts = np.sort(rng.integers(0, D, size=3))
                X[:, j, r] = np.select([np.arange(D) < c for c in cuts], lv[:3], lv[3])
    beta = rng.standard_normal((n, R)) * (rng.random((n, R)) < 0.6) * 0.02
    y = 0.2 + np.einsum("djr,jr->dr", X, beta) + 0.005 * rng.standard_normal((D, R))
    fold = batch.lasso_folds(D, K, R, seed) if K >= 2 else None
    if specials and R >= 5 and K >= 2:
        X[:, 0, 1] = 2.0
        hold = fold[:, 1] == 0
        X[hold, 0, 1] = 2.0 + rng.standard_normal(hold.sum())
        y[:, 2] = 0.25
        X[D // 2, 0, 3] = np.nan
        X[:, :, 4] = 1.0
    return X, y, fold


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64))


@pytest.mark.parametrize("D, n, K, NL, max_iter, seed", [
    (2, 1, 0, 3, 100000, 1), (2, 12, 2, 5, 100000, 2), (12, 1, 3, 10, 100000, 3), (20, 12, 4, 8, 100000, 4),
    (30, 5, 5, 20, 100000, 5), (15, 4, 0, 1, 100000, 6), (25, 6, 5, 12, 2, 7), (40, 12, 10, 6, 100000, 8),
])
def test_c_restatement_matches_python_reading(ref, D, n, K, NL, max_iter, seed):
    R = 6 if K >= 2 else 3
    X, y, fold = make_problem(R, D, n, K, seed)
    got = ref.run(X, y, fold, K, NL, 1e-4, 1e-4, max_iter)
    statuses = set()
    for r in range(R):
        w = np_lasso(X[:, :, r], y[:, r], None if fold is None else fold[:, r], K, NL, 1e-4, 1e-4, max_iter, ref.exp, ref.log)
        statuses.add(w["status"])
        assert got["status"][r] == w["status"], r
        assert _same_bits(got["lambda"][:, r], w["lambda_"]), r
        assert _same_bits(got["B"][:, :, r], np.array(w["B"])), r
        assert _same_bits(got["intercept"][:, r], w["intercept"]), r
        assert np.array_equal(got["df"][:, r], w["df"]) and np.array_equal(got["iters"][:, r], w["iters"]), r
        if K >= 2:
            assert _same_bits(got["mse"][:, r], w["mse"]) and _same_bits(got["se"][:, r], w["se"]), r
            assert _same_bits(got["a"][:, r], w["a"]) and _same_bits(got["b"][r], w["b"]), r
            assert got["idx_min_mse"][r] == w["idx_min_mse"] and got["idx_1se"][r] == w["idx_1se"], r
    if K >= 2 and R >= 5:
        assert {ST_NULL_MODEL, ST_NONFINITE} <= statuses
        train = fold[:, 1] != 0                                 # region 1: column 0 is constant on fold 0's training set only
        assert X[train, 0, 1].max() == X[train, 0, 1].min() and X[:, 0, 1].max() != X[:, 0, 1].min()
    if max_iter == 2:
        assert ST_MAXITER in statuses


def test_bad_folds_and_nonfinite_status(ref):
    X, y, fold = make_problem(3, 20, 3, 4, 12, specials=False)
    f = fold[:, 0].copy()
    f[f == 3] = 1                                               # fold 3 empty
    o = ref.region(X[:, :, 0], y[:, 0], f, 4, 5)
    assert o["status"] == ST_BAD_FOLDS and np.isnan(o["a"]).all() and o["idx_min_mse"] == -1
    f = fold[:, 0].copy(); f[0] = 4
    assert ref.region(X[:, :, 0], y[:, 0], f, 4, 5)["status"] == ST_BAD_FOLDS
    yy = y[:, 0].copy(); yy[3] = np.inf
    o = ref.region(X[:, :, 0], yy, fold[:, 0], 4, 5)
    assert o["status"] == ST_NONFINITE and np.isnan(o["lambda"]).all() and (o["df"] == 0).all()


def _standardized(X, y):
    """the full fit's Xs, Y0, constant mask, in NumPy (tiny rounding differences do not matter here)"""
    D = len(y)
    mu = X.sum(0) / D
    cst = X.max(0) == X.min(0)
    sig = np.sqrt(((X - mu) ** 2).sum(0) / D)
    sig[cst] = 1.0
    Xs = (X - mu) / sig
    Xs[:, cst] = 0.0
    return Xs, y - y.sum() / D, sig, cst


def _kkt_cases():
    for seed in range(6):
        rng = np.random.default_rng(100 + seed)
        D, n = int(rng.integers(8, 80)), int(rng.integers(1, 13))
        yield D, n, seed


@pytest.mark.parametrize("D, n, seed", list(_kkt_cases()))
def test_path_meets_the_kkt_conditions(ref, D, n, seed):
    """At every lambda g = Xs' (Y0 - Xs b) / N must equal lambda sign(b_j) where b_j != 0 and lie in [-lambda, lambda] where
    b_j = 0.  The path stops when the last cycle moved every coefficient by less than RelTol (1 + |b_old|), and the pass over
    the inactive columns after it moved nothing; the columns updated after j in that cycle moved g_j by at most
    sum_k |G_jk| |db_k| with G = Xs' Xs / N, so |KKT residual_j| <= RelTol sum_k |G_jk| (1 + |b_k| + RelTol (1 + |b_k|))
    plus rounding (1e-12 relative to the scale of g)."""
    X, y, _ = make_problem(1, D, n, 0, seed, specials=False)
    rel_tol = 1e-4
    o = ref.region(X[:, :, 0], y[:, 0], None, 0, 100, 1e-4, rel_tol)
    assert o["status"] == ST_OK
    Xs, Y0, sig, cst = _standardized(X[:, :, 0], y[:, 0])
    G = Xs.T @ Xs / D
    for k in range(100):
        lam = o["lambda"][k]
        b = o["B"][k] * sig                                     # back to the standardized scale
        g = Xs.T @ (Y0 - Xs @ b) / D
        bound = rel_tol * np.abs(G) @ ((1 + np.abs(b)) * (1 + rel_tol)) + 1e-12 * (np.abs(Xs).T @ np.abs(Y0) / D + lam)
        act = (b != 0) & ~cst
        assert np.all(np.abs(g[act] - lam * np.sign(b[act])) <= bound[act]), k
        zero = (b == 0) & ~cst
        assert np.all(np.abs(g[zero]) <= lam + bound[zero]), k


@pytest.mark.parametrize("D, n, seed", list(_kkt_cases())[:4])
def test_path_agrees_with_sklearn(ref, D, n, seed):
    """sklearn.linear_model.Lasso (alpha = lambda, no intercept, tol 1e-13) on the same standardized data minimises the
    same objective 1/(2N) ||Y0 - Xs b||^2 + lambda ||b||_1.  Two near-optimal points of a lasso objective differ by at most
    ||KKT residual|| / mu_min in the directions where the Gram matrix is definite (mu_min = its smallest eigenvalue on the
    union of the supports); we compare there, with the KKT bound of the test above, and the objective values everywhere."""
    sk = pytest.importorskip("sklearn.linear_model")
    X, y, _ = make_problem(1, D, n, 0, seed, specials=False)
    rel_tol = 1e-4
    o = ref.region(X[:, :, 0], y[:, 0], None, 0, 100, 1e-4, rel_tol)
    Xs, Y0, sig, cst = _standardized(X[:, :, 0], y[:, 0])
    G = Xs.T @ Xs / D
    obj = lambda b, lam: 0.5 * np.sum((Y0 - Xs @ b) ** 2) / D + lam * np.abs(b).sum()
    checked = 0
    for k in range(0, 100, 3):
        lam = o["lambda"][k]
        b = o["B"][k] * sig
        m = sk.Lasso(alpha=lam, fit_intercept=False, tol=1e-13, max_iter=1_000_000).fit(Xs, Y0)
        bs = m.coef_
        scale = obj(np.zeros(n), lam)
        bound_k = rel_tol * np.abs(G) @ ((1 + np.abs(b)) * (1 + rel_tol)) + 1e-12
        # objective gap of a point whose subgradient residual is e: <= |e| . |b - b*| (convexity)
        assert obj(b, lam) - obj(bs, lam) <= np.abs(bound_k) @ np.abs(b - bs) + 1e-13 * scale, k
        sup = ((b != 0) | (bs != 0)) & ~cst
        if sup.any():
            mu = np.linalg.eigvalsh(G[np.ix_(sup, sup)]).min()
            if mu > 1e-3:
                assert np.linalg.norm(b[sup] - bs[sup]) <= np.linalg.norm(bound_k[sup]) / mu + 1e-10, k
                checked += 1
    assert checked > 0


def test_lasso_folds():
    from epidemicmodeling_amd import batch
    for D, K in [(60, 50), (60, 10), (7, 7), (2, 2), (256, 63), (61, 5)]:
        f = batch.lasso_folds(D, K, 9, seed=4)
        assert f.shape == (D, 9) and f.dtype == np.int32
        want = np.array([-(-D // K)] * (D % K) + [D // K] * (K - D % K))
        for r in range(9):
            assert np.array_equal(np.bincount(f[:, r], minlength=K), want)    # every day once, cvpartition's sizes
        assert np.array_equal(f, batch.lasso_folds(D, K, 9, seed=4))
        assert not np.array_equal(f, batch.lasso_folds(D, K, 9, seed=5)) or D == K == 2
        if D > K:
            assert len({f[:, r].tobytes() for r in range(9)}) > 1                # each region its own permutation
    with pytest.raises(ValueError):
        batch.lasso_folds(5, 6, 1)
    with pytest.raises(ValueError):
        batch.check_lasso_folds(np.zeros((5, 1), dtype=np.int32), 2)


def test_status_codes_match_the_header():
    from epidemicmodeling_amd import _lib
    assert _lib.LASSO_STATUS == {"ok": ST_OK, "null_model": ST_NULL_MODEL, "maxiter": ST_MAXITER,
                                 "nonfinite": ST_NONFINITE, "bad_folds": ST_BAD_FOLDS}

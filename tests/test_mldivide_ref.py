"""MATLAB's rectangular backslash without a GPU: the two restatements (tests/mldivide_ref.c and the NumPy reading in
tests/mldivide_ref.py) agree bit for bit on every shape of the GPU suite; known answers; rank, residual and solution against
LAPACK (scipy's dgeqp3, numpy's lstsq) on synthetic plans; the C reading as a stand-alone program under the address and
undefined-behaviour sanitizers."""
import shutil
import subprocess

import numpy as np
import pytest

from tests import mldivide_ref as ML

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return ML.MldivRef(tmp_path_factory.mktemp("mldiv_ref"))


def _np(ref, X, y, n_rows=None, tol_scale=1.0):
    return ML.np_mldivide(X, y, n_rows, tol_scale, ref.fma)


@pytest.mark.parametrize("i", range(len(ML.CASES)))
def test_c_and_numpy_readings_agree_bit_for_bit(ref, i):
    X, y, nr = ML.problem(i)
    a, b = ref.run(X, y, nr), _np(ref, X, y, nr)
    for k in ML.OUT_NAMES:
        assert ML.same_bits(a[k], b[k]), k


def test_the_shared_cases_reach_every_status_and_branch(ref):
    seen, ranks, rel, ties, recomputed = 0, set(), set(), 0, 0
    for i, ((D, F, K, R), nr) in enumerate(ML.CASES):
        X, y, _ = ML.problem(i)
        ref.counters(reset=True)
        o = ref.run(X, y, nr)
        c = ref.counters()
        b = _np(ref, X, y, nr) if D <= 40 else None
        assert b is None or (b["recomputed"], b["ties"]) == c            # the two readings take the same branches
        recomputed, ties = recomputed + c[0], ties + c[1]
        st = o["status"]
        seen |= int(np.bitwise_or.reduce(st.ravel()))
        assert ((st == ML.NONFINITE_INPUT) | ((st & ML.NONFINITE_INPUT) == 0)).all()   # that bit stands alone
        assert ((o["rank"] == -1) == (st == ML.NONFINITE_INPUT)).all()
        for k, n in enumerate(nr):
            rel.add("<" if n < F else "==" if n == F else ">")
            mn = min(n, F)
            for r in range(R):
                rk = int(o["rank"][k, r])
                if rk < 0:
                    continue
                ranks.add("0" if rk == 0 else "1" if rk == 1 and mn > 1 else "full" if rk == mn else "deficient")
                assert bool(st[k, r] & ML.RANK_DEFICIENT) == (rk < mn)
                assert sorted(o["perm"][k, :, r]) == list(range(F))
                assert (o["rdiag"][k, mn:, r] == 0).all() and not np.signbit(o["rdiag"][k, mn:, r]).any()
    assert seen == 7 and ranks == {"0", "1", "full", "deficient"} and rel == {"<", "==", ">"}, (seen, ranks, rel)
    assert ties > 0 and recomputed > 0, (ties, recomputed)


def test_the_planted_column_is_recomputed_under_the_safeguard(ref):
    """column 1 = column 0 + 1e-9 of a direction of its own: the first reflector cancels all but 1e-9 of it, so the downdated norm falls
    below sqrt(eps) of the last computed one and is computed again from the rows"""
    g = np.random.default_rng(3)
    X = g.normal(size=(30, 3, 1))
    X[:, 0, 0] *= 10.0
    X[:, 1, 0] = X[:, 0, 0] + 1e-9 * g.normal(size=30)
    y = g.normal(size=(30, 1))
    ref.counters(reset=True)
    o = ref.run(X, y)
    assert ref.counters()[0] >= 1 and _np(ref, X, y)["recomputed"] == ref.counters()[0]
    assert o["rank"][0, 0] == 3 and list(o["perm"][0, :, 0]) == [0, 2, 1]   # the nearly cancelled column comes last
    assert abs(o["rdiag"][0, 2, 0]) < 1e-7


def test_one_column_is_the_scalar_quotient(ref):
    g = np.random.default_rng(4)
    X, y = g.normal(size=(11, 1, 2)), g.normal(size=(11, 2))
    o = ref.run(X, y)
    for r in range(2):
        x, yy = X[:, 0, r], y[:, r]
        want = (x @ yy) / (x @ x)
        assert abs(o["m"][0, 0, r] - want) <= 8 * EPS * abs(want)       # one reflector and one division: a few eps
        # exactly the stated order: 8 chains of fma, added ascending; beta, tau, the y column's row 0, the division
        def rs(a, b, lo):
            s = [0.0] * ML.P
            for i in range(lo, 11):
                s[i % ML.P] = ref.fma(a[i], b[i], s[i % ML.P])
            t = s[0]
            for p in range(1, ML.P):
                t = t + s[p]
            return t
        alpha, ss = x[0], rs(x, x, 1)
        beta = -np.copysign(np.sqrt(ref.fma(alpha, alpha, ss)), alpha)                # far above the 2^-900 below which a reflector is skipped
        tau, scale = (beta - alpha) / beta, 1.0 / (alpha - beta)
        z0 = yy[0] - tau * (yy[0] + rs(x * scale, yy, 1))
        assert ML.same_bits(o["m"][0, 0, r], np.float64(z0 / beta))
        assert ML.same_bits(o["rdiag"][0, 0, r], np.float64(beta)) and o["rank"][0, r] == 1 and o["status"][0, r] == 0


def test_scaled_identity_columns_return_y_over_the_scale(ref):
    X = np.zeros((6, 4, 1))
    for f, row in enumerate((2, 0, 5, 3)):
        X[row, f, 0] = 4.0
    y = np.array([[3.0], [1.0], [-2.0], [7.0], [0.5], [-9.0]])
    o = ref.run(X, y)
    assert np.array_equal(o["m"][0, :, 0], np.array([-2.0, 3.0, -9.0, 7.0]) / 4.0)
    assert o["rank"][0, 0] == 4 and o["status"][0, 0] == 0
    assert o["resid"][0, 0] == np.sqrt(1.0 + 0.25)                       # the rows no column touches
    assert list(o["perm"][0, :, 0]) == [0, 1, 2, 3]                      # four equal norms: ties go to the lowest index


def test_duplicate_zero_and_all_zero_columns(ref):
    g = np.random.default_rng(6)
    X = g.integers(1, 5, size=(9, 4, 2)).astype(np.float64)
    X[:, 3, 0] = X[:, 1, 0]                                             # a duplicate of column 1
    X[:, 2, 0] = 0.0                                                    # a zero column
    X[:, :, 1] = 0.0                                                    # an all-zero matrix
    y = g.normal(size=(9, 2))
    o = ref.run(X, y)
    m = o["m"][0, :, 0]
    assert m[1] != 0 and m[3] == 0 and m[2] == 0 and not np.signbit(m[[2, 3]]).any()
    assert o["rank"][0, 0] == 2 and o["status"][0, 0] == ML.RANK_DEFICIENT
    one = ref.run(np.ascontiguousarray(X[:, :2, :1]), np.ascontiguousarray(y[:, :1]))
    assert np.allclose(m[:2], one["m"][0, :, 0], rtol=64 * EPS, atol=0)  # the whole coefficient on the lower index
    assert o["rank"][0, 1] == 0 and (o["m"][0, :, 1] == 0).all() and o["status"][0, 1] == ML.RANK_DEFICIENT
    assert (o["fitted"][0, :, 1] == 0).all() and o["resid"][0, 1] > 0


def test_consistent_system_has_no_residual(ref):
    g = np.random.default_rng(7)
    X = g.integers(-3, 4, size=(20, 5, 3)).astype(np.float64)
    m0 = g.integers(-4, 5, size=(5, 3)).astype(np.float64)
    y = np.einsum("tfr,fr->tr", X, m0)
    o = ref.run(X, y, n_rows=(20, 8))
    assert (o["rank"] == 5).all() and (o["status"] == 0).all()
    # every reflector perturbs y by a few eps ||y||; five of them and the sum of 15 squares: 32 eps ||y|| is ample
    for k, n in enumerate((20, 8)):
        assert (o["resid"][k] <= 32 * EPS * np.linalg.norm(y[:n], axis=0)).all()
    assert np.allclose(o["m"], m0[None], rtol=0, atol=1e-12) and np.allclose(o["fitted"], y[None], rtol=0, atol=1e-11)


def test_nonfinite_inputs_and_rows_beyond_n_rows(ref):
    g = np.random.default_rng(8)
    X, y = g.normal(size=(10, 3, 3)), g.normal(size=(10, 3))
    X[8, 1, 0] = np.nan                                                 # beyond the 6 used rows: only fitted sees it
    y[2, 1] = -np.inf
    o = ref.run(X, y, n_rows=(6,))
    assert o["status"][0, 0] == ML.NONFINITE and np.isnan(o["fitted"][0, 8, 0]) and np.isfinite(o["fitted"][0, :8, 0]).all()
    assert o["status"][0, 1] == ML.NONFINITE_INPUT and o["rank"][0, 1] == -1 and list(o["perm"][0, :, 1]) == [0, 1, 2]
    assert all(np.isnan(o[k][0, ..., 1]).all() for k in ("m", "rdiag", "resid", "fitted"))
    assert o["status"][0, 2] == 0


def test_tol_scale_moves_the_rank(ref):
    g = np.random.default_rng(9)
    X, y = g.normal(size=(12, 3, 1)), g.normal(size=(12, 1))
    X[:, 2, 0] = X[:, 0, 0] + 1e-6 * g.normal(size=12)
    assert ref.run(X, y)["rank"][0, 0] == 3
    o = ref.run(X, y, tol_scale=1e11)                                    # tol = 1e11 * 12 eps |R11| ~ 3e-4 |R11|
    assert o["rank"][0, 0] == 2 and o["status"][0, 0] == ML.RANK_DEFICIENT
    X2 = X.copy()
    X2[:, 2, 0] = X2[:, 0, 0]
    o0 = ref.run(X2, y, tol_scale=0.0)                                   # tol = 0: only an exact zero on the diagonal is dropped
    assert o0["rank"][0, 0] == (3 if o0["rdiag"][0, 2, 0] != 0 else 2)
    assert ML.same_bits(o0["rdiag"], ref.run(X2, y)["rdiag"])


# ---- against LAPACK -----------------------------------------------------------------------------------------------------
# Measured with the reading itself (96 regions x the row counts 20 / 60 / 120 / 275 / 366 = 480 items, seed 2024):
#                                normalised     raw
#   residual excess / ||y||      2.44e-15       5.30e-15        (over numpy.linalg.lstsq's)
#   solution distance            1.51           1.42            (max|m - m_lapack| / max|m_lapack| in units of eps cond(R11))
#   pivot sets differ            10.2 %         14.6 %  (of 480; the order of the first `rank` pivots differs on 102 / 91)
# Each gate is 8 x the worst value; the values are DESIGN.md §4.12's.
LAPACK_WORST = {True: (2.44e-15, 1.51), False: (5.30e-15, 1.42)}
ROWS = (20, 60, 120, 275, 366)


def lapack_stats(ref, normalised, regions=96, seed=2024):
    import scipy.linalg as sl
    X, y = ML.plans_problem(seed, regions, normalised=normalised)
    o = ref.run(X, y, n_rows=ROWS)
    D, F, R = X.shape
    worst_res = worst_sol = 0.0
    left = deficient = order = 0
    margin_keep, margin_drop = np.inf, 0.0
    for k, n in enumerate(ROWS):
        for r in range(R):
            A, b = X[:n, :, r], y[:n, r]
            Q, Rl, P = sl.qr(A, mode="economic", pivoting=True)
            d = np.abs(np.diag(Rl))
            tol = max(n, F) * EPS * d[0]
            rank_l = int((d > tol).sum())
            rk = int(o["rank"][k, r])
            assert rk == rank_l, (k, r, rk, rank_l)
            rd = np.abs(o["rdiag"][k, :min(n, F), r])
            margin_keep = min(margin_keep, rd[rk - 1] / rd[0])
            margin_drop = max(margin_drop, rd[rk] / rd[0]) if rk < len(rd) else margin_drop
            deficient += rk < min(n, F)
            order += list(o["perm"][k, :rk, r]) != list(P[:rk])
            res_l = np.linalg.norm(A @ np.linalg.lstsq(A, b, rcond=None)[0] - b)
            worst_res = max(worst_res, (o["resid"][k, r] - res_l) / np.linalg.norm(b))
            assert abs(np.linalg.norm(A @ o["m"][k, :, r] - b) - o["resid"][k, r]) <= 64 * EPS * np.linalg.norm(b)
            if set(o["perm"][k, :rk, r]) != set(P[:rk]):
                left += 1
                continue
            R11 = Rl[:rk, :rk]
            ml = np.zeros(F)
            ml[P[:rk]] = sl.solve_triangular(R11, (Q.T @ b)[:rk])
            worst_sol = max(worst_sol, np.abs(o["m"][k, :, r] - ml).max() / np.abs(ml).max() / (EPS * np.linalg.cond(R11)))
    return dict(resid=worst_res, sol=worst_sol, left=left / (len(ROWS) * R), deficient=deficient, order=order,
                keep=margin_keep, drop=margin_drop, items=len(ROWS) * R)


@pytest.mark.parametrize("normalised", (True, False), ids=("normalised", "raw"))
def test_rank_residual_and_solution_against_lapack(ref, normalised):
    s = lapack_stats(ref, normalised)
    print(s)
    gate_res, gate_sol = (8 * v for v in LAPACK_WORST[normalised])
    assert s["deficient"] > 0                                           # the inputs are rank-deficient by construction
    assert s["left"] <= 0.20, s
    assert s["resid"] <= gate_res and s["sol"] <= gate_sol, s


def test_c_reading_under_sanitizers(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.fail("no C compiler for tests/mldivide_ref.c")
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run([cc, *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler cannot link the sanitizer runtimes")
    exe = str(tmp_path / "ref_main")
    subprocess.run([cc, "-O1", "-g", "-ffp-contract=off", *san, "-DMLDIVIDE_MAIN", ML.SRC, "-o", exe, "-lm"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode == 0 and "status bits seen 7" in r.stdout and "ERROR" not in r.stderr, (r.stdout[-500:], r.stderr[-2000:])

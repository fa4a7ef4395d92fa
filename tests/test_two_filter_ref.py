"""The restatement tests/two_filter_ref.py of the forward-backward filter fusion against closed forms and
against an independent NumPy / LAPACK reading.  No GPU: this is what the device tests then hold the kernel to bit for bit."""
import numpy as np
import pytest

from tests import two_filter_ref as TF

FORMS = [(0, 0), (0, 1), (1, 0)]


def _diag_case(m, seed, base=4.0):
    """(pf, sf, sb): a power-of-two diagonal and integer-valued estimates.  base 4: the ratios of the entries are powers of
    FOUR.  orc_sym_pinv factorises S scaled by the power of two of its largest entry and takes the square root of each pivot,
    which is exact only for an even power of two; with base 2 the pseudo-inverse of a diagonal S is therefore good to a few
    ulp, not to the bit (measured: 1 ulp)."""
    rng = np.random.default_rng(seed)
    pf = base ** rng.integers(-6, 7, m)
    sf, sb = rng.integers(-8, 9, m).astype(float), rng.integers(-8, 9, m).astype(float)
    return pf, sf, sb


@pytest.mark.parametrize("m", [3, 6])
@pytest.mark.parametrize("form, p_solver", FORMS)
def test_diagonal_power_of_two_is_exact(m, form, p_solver):
    """Diagonal Pf, Pb with power-of-two entries (ratios powers of four, see _diag_case), Pf = Pb: S = 2 Pf and 1 / S are
    powers of two, every product is exact, so P = diag(pf pb / (pf + pb)) and s = the precision-weighted mean hold to the bit
    in both forms."""
    pf, sf, sb = _diag_case(m, 10 * m + form + p_solver)
    pb = pf.copy()
    r = TF.fuse_item(m, list(sf), np.diag(pf).tolist(), list(sb), np.diag(pb).tolist(), form, p_solver)
    assert r["rank"] == m and not r["bad"]
    P = np.array(r["P"])
    assert np.array_equal(P, np.diag(pf * pb / (pf + pb)))
    assert np.array_equal(np.array(r["s"]), (pb * sf + pf * sb) / (pf + pb))
    e = sf - sb
    assert r["d2"] == float(np.sum(e * e / (pf + pb)))


@pytest.mark.parametrize("m", [3, 6])
@pytest.mark.parametrize("form, p_solver", FORMS)
def test_diagonal_unequal_powers_of_two(m, form, p_solver):
    """Pb = 3 Pf, powers of two: S = 4 Pf, still exact.  P = (3/4) Pf, s = (3 sf + sb) / 4."""
    pf, sf, sb = _diag_case(m, 20 * m + form + p_solver)
    pb = 3.0 * pf
    r = TF.fuse_item(m, list(sf), np.diag(pf).tolist(), list(sb), np.diag(pb).tolist(), form, p_solver)
    assert np.array_equal(np.array(r["P"]), np.diag(0.75 * pf))
    assert np.array_equal(np.array(r["s"]), (3.0 * sf + sb) / 4.0)


@pytest.mark.parametrize("m", [3, 6])
@pytest.mark.parametrize("form, p_solver", FORMS)
def test_diagonal_any_power_of_two_within_4_ulp(m, form, p_solver):
    """Ratios that are odd powers of two: the only inexact steps are l = sqrt(pivot), 1 / l and (1 / l)^2 inside the
    pseudo-inverse (half an ulp each; every other operation multiplies by a power of two or adds two terms of which one is
    zero) -- and none at all in P = S \\ C, which divides powers of two.  So 4 eps relative holds with room: measured 1 ulp."""
    pf, sf, sb = _diag_case(m, 30 * m + form + p_solver, base=2.0)
    pb = pf.copy()
    r = TF.fuse_item(m, list(sf), np.diag(pf).tolist(), list(sb), np.diag(pb).tolist(), form, p_solver)
    eps = np.finfo(float).eps
    P, Pw = np.array(r["P"]), np.diag(pf / 2.0)
    s, sw = np.array(r["s"]), (sf + sb) / 2.0
    assert np.all(np.abs(P - Pw) <= 4 * eps * np.abs(Pw)) and np.all(np.abs(s - sw) <= 4 * eps * np.abs(sw))


@pytest.mark.parametrize("m", [3, 6])
@pytest.mark.parametrize("form, p_solver", FORMS)
def test_diagonal_independent_powers_of_two(m, form, p_solver):
    """Pf and Pb drawn independently (power-of-two diagonals, Pf != Pb), so that a restatement that mixed up Pf and Pb --
    the weights of sf and sb swapped -- could not pass: P = diag(pf pb / (pf + pb)), s = (pb sf + pf sb) / (pf + pb).  Not
    exact: 1 / (pf + pb) is not a power of two.  Per diagonal item the pseudo-inverse rounds sqrt, 1 / l and its square (half an
    ulp each, 2 ulp on 1 / S after squaring), the weighted sum pb sf + pf sb rounds once (exact products of a power of two
    and a small integer) and the final product once more; S \\ C is one division.  8 eps relative to the larger of the two terms
    of s (they may cancel) and to P covers it with room; a swap of Pf and Pb moves s by O(1)."""
    rng = np.random.default_rng(40 * m + form + p_solver)
    pf, pb = 2.0 ** rng.integers(-6, 7, m), 2.0 ** rng.integers(-6, 7, m)
    pb[0] = pf[0] * 8.0                                      # at least one axis on which the two differ for certain
    sf, sb = rng.integers(1, 9, m).astype(float), -rng.integers(1, 9, m).astype(float)
    r = TF.fuse_item(m, list(sf), np.diag(pf).tolist(), list(sb), np.diag(pb).tolist(), form, p_solver)
    eps = np.finfo(float).eps
    P, Pw = np.array(r["P"]), np.diag(pf * pb / (pf + pb))
    s, sw = np.array(r["s"]), (pb * sf + pf * sb) / (pf + pb)
    scale = np.maximum(np.abs(pb * sf), np.abs(pf * sb)) / (pf + pb)
    assert np.all(np.abs(P - Pw) <= 8 * eps * np.abs(Pw)) and np.all(np.abs(s - sw) <= 8 * eps * scale)
    swapped = (pf * sf + pb * sb) / (pf + pb)
    assert np.abs(s[0] - swapped[0]) > 1e-3 * scale[0]       # the check can tell the two apart


@pytest.mark.parametrize("m", [3, 6])
@pytest.mark.parametrize("form, p_solver", [(0, 1), (1, 0)])
def test_rank_one_keeps_its_subspace(m, form, p_solver):
    """Pf = Pb = diag(1, 0, ..., 0): rank 1, and nothing outside the kept axis.  (p_solver 0 of form 0 solves with the
    singular S itself, as MATLAB's backslash would: no finite answer is asked of it.)"""
    D = np.zeros((m, m))
    D[0, 0] = 1.0
    sf, sb = [float(k + 1) for k in range(m)], [float(2 * k - 1) for k in range(m)]
    r = TF.fuse_item(m, sf, D.tolist(), sb, D.tolist(), form, p_solver)
    assert r["rank"] == 1
    P, s = np.array(r["P"]), np.array(r["s"])
    assert P[0, 0] == 0.5 and np.count_nonzero(P) == 1
    assert s[0] == (sf[0] + sb[0]) / 2.0 and np.count_nonzero(s[1:]) == 0
    assert r["d2"] == (sf[0] - sb[0]) ** 2 / 2.0


def test_zero_matrices_give_rank_zero():
    Z = np.zeros((3, 3)).tolist()
    r = TF.fuse_item(3, [1.0, 2.0, 3.0], Z, [0.0, 1.0, 0.0], Z, 1, 0)
    assert r["rank"] == 0 and r["d2"] == 0.0 and not np.any(r["P"]) and not np.any(r["s"])


@pytest.mark.parametrize("where", ["Pf_upper", "Pb_diag", "sf", "sb"])
def test_nonfinite_entry_poisons_its_day_only(where):
    m, T, B = 3, 4, 2
    sf, Pf, sb, Pb = TF.planted(m, T, B, seed=3, indefinite=False, nonfinite=False)
    t0, c0 = 2, 1
    if where == "Pf_upper":
        Pf[t0, 0 + m * 2, c0] = np.nan                       # entry (0, 2)
    elif where == "Pb_diag":
        Pb[t0, 1 + m * 1, c0] = -np.inf
    elif where == "sf":
        sf[t0, 2, c0] = np.inf
    else:
        sb[t0, 0, c0] = np.nan
    for form, ps in FORMS:
        r = TF.fuse(sf, Pf, sb, Pb, form, ps)
        assert np.isnan(r["s"][t0, :, c0]).all() and np.isnan(r["P"][t0, :, c0]).all() and np.isnan(r["d2"][t0, c0])
        assert r["rank"][t0, c0] == -1 and r["status"].tolist() == [0, 1]
        keep = np.ones((T, B), dtype=bool)
        keep[t0, c0] = False
        assert (r["rank"][keep] >= 0).all() and np.isfinite(r["d2"][keep]).all()
        assert np.isfinite(r["s"].transpose(0, 2, 1)[keep]).all()


def test_lower_triangle_does_not_enter_S():
    """only the upper triangles of Pf and Pb enter S: a NaN below the diagonal leaves rank, d2 and the guard alone"""
    m = 3
    sf, Pf, sb, Pb = TF.planted(m, 1, 4, seed=5, indefinite=False, nonfinite=False)
    base = TF.fuse(sf, Pf, sb, Pb, 1)
    Pf[0, 2 + m * 0, 3] = np.nan                             # entry (2, 0)
    r = TF.fuse(sf, Pf, sb, Pb, 1)
    assert np.array_equal(r["rank"], base["rank"]) and TF.same_bits(r["d2"], base["d2"]) and not r["status"].any()


@pytest.mark.parametrize("m", [3, 6])
def test_d2_is_zero_for_equal_estimates(m):
    sf, Pf, sb, Pb = TF.planted(m, 2, m + 1, seed=7, indefinite=False, nonfinite=False)
    r = TF.fuse(sf, Pf, sf, Pb, 1)
    assert np.array_equal(r["d2"], np.zeros_like(r["d2"]))


def _spd(rng, m, cond):
    U, _ = np.linalg.qr(rng.standard_normal((m, m)))
    d = np.exp(rng.uniform(0.0, np.log(cond), m))
    d[0], d[-1] = 1.0, cond
    A = (U * d) @ U.T
    return (A + A.T) / 2.0


def _lapack_reading(m, sf, Pf, sb, Pb, form, p_solver):
    """the same formulas through np.linalg: pinv with MATLAB's tolerance (max(size) * eps(max singular value)), solve"""
    S = Pf + Pb
    sv = np.linalg.svd(S, compute_uv=False)
    X = np.linalg.pinv(S, rcond=m * np.spacing(sv.max()) / sv.max(), hermitian=True)
    e = sf - sb
    d2 = e @ (X @ e)
    if form == 0:
        s = X @ (Pb @ sf + Pf @ sb)
        P = np.linalg.solve(S, Pf @ Pb) if p_solver == 0 else X @ (Pf @ Pb)
    else:
        s = Pb @ (X @ sf) + Pf @ (X @ sb)
        P = Pf @ (X @ Pb)
        P = (P + P.T) / 2.0
    return s, P, d2


# measured distances (relative, max over 200 items per m, cond(Pf), cond(Pb) <= 1e6), see the test below
MEASURED = {3: 6.4e-8, 6: 2.3e-10}


@pytest.mark.parametrize("m", [3, 6])
def test_restatement_close_to_lapack_reading(m):
    """Well-conditioned random SPD Pf, Pb (cond <= 1e6 each, so S = Pf + Pb is SPD with cond <= 1e6 and the rank cut never
    bites: the restatement must report rank m everywhere).  The restatement is held within 100 x its measured distance to
    the NumPy / LAPACK reading -- the convention of the AR forecaster's tests.  Measured (this file, 200 items per m, all
    three form / p_solver pairs, max over s, P, d2 of |a - b| / max|b| per item): m = 3: 6.380e-08, m = 6: 2.256e-10.  s, d2
    and form 0's P stay at cond * eps (at most 7.3e-11 at m = 3); the 6.4e-8 is form 1's P = Pf (X Pb) on one item with
    cond(Pf) and cond(Pb) near 1e6: the product's terms are cond times larger than the parallel sum they add up to, so
    two correct evaluation orders differ by cond^2 * eps there.  That is a property of the formula, not of either reading."""
    rng = np.random.default_rng(1000 + m)
    worst = 0.0
    for _ in range(200):
        Pf, Pb = _spd(rng, m, 10.0 ** rng.uniform(0, 6)), _spd(rng, m, 10.0 ** rng.uniform(0, 6))
        sf, sb = rng.standard_normal(m), rng.standard_normal(m)
        for form, ps in FORMS:
            r = TF.fuse_item(m, sf.tolist(), Pf.tolist(), sb.tolist(), Pb.tolist(), form, ps)
            assert r["rank"] == m
            s, P, d2 = _lapack_reading(m, sf, Pf, sb, Pb, form, ps)
            for got, ref in ((np.array(r["s"]), s), (np.array(r["P"]), P), (np.array(r["d2"]), np.array(d2))):
                worst = max(worst, float(np.max(np.abs(got - ref)) / np.max(np.abs(ref))))
    print(f"m = {m}: distance to the LAPACK reading {worst:.3e}")
    assert worst <= 100.0 * MEASURED[m], worst


def test_blocked_layout_round_trip():
    a = np.arange(2 * 3 * 7, dtype=np.float64).reshape(2, 3, 7)
    b = TF.to_blocked(a, 4)
    assert b.shape == (2, 2, 3, 4) and np.array_equal(TF.from_blocked(b, 7), a)
    # element (t, row, c) at ((t * nblk + c / blk) * rows + row) * blk + c % blk
    t, row, c = 1, 2, 5
    assert b.ravel()[((t * 2 + c // 4) * 3 + row) * 4 + c % 4] == a[t, row, c]


def test_a_sweep_cap_sets_bit_1_of_its_chain_only():
    """TF.CAPPED: the one-sided Jacobi iteration of item (12, 5) ends at its 30th sweep still rotating; bit 1 of chain 5 and of no
    other chain, in every form, and the item's values are finite all the same.  Rounded to float the item converges: no bit."""
    sf, Pf, sb, Pb = TF.planted(*TF.CAPPED)
    for form, p_solver in FORMS:
        r = TF.fuse(sf, Pf, sb, Pb, form, p_solver)
        assert list(np.flatnonzero(r["status"] & 2)) == [5] and list(np.flatnonzero(r["status"] & 1)) == [3]
        assert r["rank"][12, 5] == 5 and r["route"][12, 5] == 0 and np.isfinite(r["s"][12, :, 5]).all() and np.isfinite(r["P"][12, :, 5]).all()
        assert not (TF.fuse(sf, Pf, sb, Pb, form, p_solver, storage="f32")["status"] & 2).any()
    m = TF.CAPPED[0]
    S = [[float(Pf[12, min(i, j) + m * max(i, j), 5] + Pb[12, min(i, j) + m * max(i, j), 5]) for j in range(m)] for i in range(m)]
    assert TF.sym_pinv(m, S)[3] and not TF.sym_pinv(m, [[float(i == j) for j in range(m)] for i in range(m)])[3]

"""The support-vector regression without a GPU: the two restatements (tests/svr_ref.c and the NumPy reading in
tests/svr_ref.py) agree bit for bit on every shape of the GPU suite; known answers; what the suite's cases reach; the duality
gap of every converged item recomputed in longdouble; scikit-learn's LIBSVM through a recorded fixture; svr_defaults; the C
reading as a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import svr_ref as SV

GOLDEN = os.path.join(SV.HERE, "golden", "svr_sklearn.npz")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return SV.SvrRef(tmp_path_factory.mktemp("svr_ref"))


_WANT = {}


def want(ref, i, kernel):
    """the C reading of case i, computed once and shared (read-only), with the counters of that run"""
    if (i, kernel) not in _WANT:
        p = SV.problem(i)
        ref.counters(reset=True)
        w = ref.run(p["X"], p["y"], **SV.run_kw(p, kernel))
        for v in w.values():
            v.setflags(write=False)
        _WANT[(i, kernel)] = (w, ref.counters())
    return _WANT[(i, kernel)]


PAIRS = [(i, k) for i, (_, ks) in enumerate(SV.CASES) for k in ks]
IDS = ["D%d-F%d-R%d-%s" % (SV.CASES[i][0][0], SV.CASES[i][0][1], SV.CASES[i][0][3], k) for i, k in PAIRS]


@pytest.mark.parametrize("i, kernel", PAIRS, ids=IDS)
def test_c_and_numpy_readings_agree_bit_for_bit(ref, i, kernel):
    p = SV.problem(i)
    w, _ = want(ref, i, kernel)
    o = SV.np_svr(p["X"], p["y"], p["n_rows"], kernel, p["box"], p["epsilon"], p["kernel_scale"], SV.TOL, SV.MAX_ITER, ref)
    assert set(o) == set(w)
    for k in w:
        assert SV.same_bits(w[k], o[k]), k


def test_one_row_is_its_own_bias(ref):
    """n_rows = 1: up = {alpha_1}, low = {alpha*_1}, m - M = (y - e) - (y + e) < 0: no step; no free variable, the midpoint
    ((y - e) + (y + e)) / 2 is y exactly where y -+ e are exact (dyadic values here)"""
    X = np.array([[[0.5]], [[0.25]]])
    y = np.array([[0.375], [0.75]])
    for kernel in SV.KERNELS:
        o = ref.run(X, y, (1,), kernel, box=1.0, epsilon=0.125, kernel_scale=1.0)
        assert (o["beta"] == 0.0).all() and not np.signbit(o["beta"]).any()
        assert o["bias"][0, 0] == 0.375 and o["n_iter"][0, 0] == 0 and o["n_sv"][0, 0] == 0 and o["status"][0, 0] == 0
        assert (o["fitted"] == 0.375).all()
        if kernel == "linear":
            assert (o["w"] == 0.0).all()


def test_constant_target_has_no_support_vector(ref):
    p = SV.problem(5)
    for kernel in SV.KERNELS:
        o = want(ref, 5, kernel)[0]
        assert (p["y"][:, 5] == 0.03125).all()
        assert (o["beta"][:, :, 5] == 0.0).all() and (o["n_iter"][:, 5] == 0).all() and (o["status"][:, 5] == 0).all()
        assert (np.abs(o["bias"][:, 5] - 0.03125) <= 2.0 ** -56).all()       # the midpoint of y - e and y + e, each rounded once


def test_two_rows_by_hand(ref):
    """x = (0, 1), y = (0, 1), linear, F = 1, e = 0.25, C = 10: K = [[0, 0], [0, 1]].  The flat tube 2e = 0.5 < 1 does not
    hold both, so beta_2 = -beta_1 = b with the dual b (y_2 - y_1) - 2 e b - b^2 K_22 / 2 maximal: b = 1 - 0.5 = 0.5.
    w = b x_2 = 0.5; the bias puts both rows on the tube's edge: f_1 = bias = y_1 + e = 0.25, f_2 = 0.75 = y_2 - e.
    With C = 0.25 the step is clipped: b = 0.25, w = 0.25, both variables on the bound: the midpoint of the bounds
    [y_1 + e, y_2 - e - w] = [0.25, 0.5] is 0.375.  Every number is dyadic: exact"""
    X = np.array([[[0.0]], [[1.0]]])
    y = np.array([[0.0], [1.0]])
    o = ref.run(X, y, (2,), "linear", box=10.0, epsilon=0.25)
    assert o["n_iter"][0, 0] == 1 and o["status"][0, 0] == 0 and o["n_sv"][0, 0] == 2
    assert o["beta"][0, :, 0].tolist() == [-0.5, 0.5] and o["w"][0, 0, 0] == 0.5 and o["bias"][0, 0] == 0.25
    assert o["fitted"][0, :, 0].tolist() == [0.25, 0.75]
    o = ref.run(X, y, (2,), "linear", box=0.25, epsilon=0.25)
    assert o["beta"][0, :, 0].tolist() == [-0.25, 0.25] and o["w"][0, 0, 0] == 0.25 and o["bias"][0, 0] == 0.375
    # Gaussian, scale 1: K_12 = exp(-1); the same pair step with curvature 2 - 2 exp(-1): b = 0.5 / (2 - 2 exp(-1))
    o = ref.run(X, y, (2,), "gaussian", box=10.0, epsilon=0.25, kernel_scale=1.0)
    b = 0.5 / (2.0 - 2.0 * np.exp(-1.0))
    assert abs(o["beta"][0, 1, 0] - b) < 4e-16 and o["beta"][0, 0, 0] == -o["beta"][0, 1, 0] and abs(o["bias"][0, 0] - 0.5) < 4e-16


def test_wide_tube_has_no_support_vector(ref):
    """region 3 of the planted cases: epsilon above max|y - median|: every row lies inside the tube of a constant"""
    for i in (1, 5):
        p = SV.problem(i)
        assert p["epsilon"][3] > np.abs(p["y"][:, 3] - np.median(p["y"][:, 3])).max()
        for kernel in SV.KERNELS:
            o = want(ref, i, kernel)[0]
            assert (o["n_sv"][:, 3] == 0).all() and (o["beta"][:, :, 3] == 0.0).all() and (o["status"][:, 3] == 0).all()


def test_max_iter_three_gives_the_three_step_iterate(ref):
    p = SV.problem(5)
    for kernel in SV.KERNELS:
        kw = SV.run_kw(p, kernel, max_iter=3)
        o = ref.run(p["X"], p["y"], **kw)
        full = want(ref, 5, kernel)[0]
        more = full["n_iter"] > 3
        assert more.sum() > 50
        assert ((o["status"] & SV.NOT_CONVERGED) != 0)[more].all() and (o["n_iter"][more] == 3).all() and (o["gap"][more] >= SV.TOL).all()
        assert not (o["status"][~more] & SV.NOT_CONVERGED).any()
        n = SV.np_svr(p["X"], p["y"], p["n_rows"], kernel, p["box"], p["epsilon"], p["kernel_scale"], SV.TOL, 3, ref, regions=range(12))
        for k in o:
            assert SV.same_bits(o[k][..., :12], n[k][..., :12]), k


def test_bad_items_leave_their_neighbours_untouched(ref):
    """(120, 49, (90, 120), 65): the regions 1, 2 and 7 are BAD_INPUT, region 6 is BAD_INPUT where the last row is used and has
    a non-finite prediction where it is not; every other region gives what it gives without them"""
    i = 5
    p = SV.problem(i)
    (D, F, nr, R), _ = SV.CASES[i]
    for kernel in SV.KERNELS:
        o = want(ref, i, kernel)[0]
        st = o["status"]
        # an Inf in a prediction row: inf . w is not finite; the Gaussian kernel turns the infinite distance into K = 0
        assert (st[:, [1, 2, 7]] == SV.BAD_INPUT).all() and st[1, 6] == SV.BAD_INPUT and st[0, 6] == (SV.NONFINITE if kernel == "linear" else 0)
        for r in (1, 2, 7):
            assert np.isnan(o["beta"][:, :, r]).all() and np.isnan(o["fitted"][:, :, r]).all() and np.isnan(o["bias"][:, r]).all()
            assert np.isnan(o["gap"][:, r]).all() and (o["n_iter"][:, r] == 0).all() and (o["n_sv"][:, r] == 0).all()
        assert np.isfinite(o["fitted"][0, :D - 1, 6]).all() and np.isfinite(o["fitted"][0, D - 1, 6]) == (kernel == "gaussian")
        keep = [r for r in range(R) if r not in (1, 2, 6, 7)]
        X, y, box, sc = (np.array(p[k]) for k in ("X", "y", "box", "kernel_scale"))
        X[0, 0, 1], X[D - 1, 0, 6], box[2], sc[7] = 0.0, 0.0, 1.0, 1.0
        clean = ref.run(X, y, **SV.run_kw(p, kernel, box=box, kernel_scale=sc))
        for k in o:
            assert SV.same_bits(o[k][..., keep], clean[k][..., keep]), k


def test_the_suite_reaches_every_path(ref):
    """Every status bit; both clips (at 0 and at C) of the opposite-sign and of the equal-sign step; a curvature replaced by
    tau (the duplicated rows); the bias as the midpoint (no free variable); every rows-per-lane instantiation (1, 2, 4 by the
    largest row count of a call).

    The pair on ONE data row (j = i +- n) cannot be reached from alpha = 0, so the counter must stay zero: alpha*_k enters the
    low set's choice only against alpha_k, which is in the low set whenever it is positive, has the same curvature and the
    larger b = gmax + G by 2 epsilon (the lower index on the tie at epsilon = 0), so alpha*_k never leaves zero while
    alpha_k > 0, and i = alpha_k with j = alpha*_k has b = -2 epsilon <= 0.  With the roles swapped the same holds.  The
    kernel's and the readings' pair step do not single the case out."""
    tot = dict.fromkeys(SV.COUNTERS, 0)
    bits, per_lane = 0, set()
    for i, kernel in PAIRS:
        w, cnt = want(ref, i, kernel)
        for k in tot:
            tot[k] += cnt[k]
        bits |= int(np.bitwise_or.reduce(w["status"].ravel()))
        per_lane.add(1 if max(SV.CASES[i][0][2]) <= 256 else 2 if max(SV.CASES[i][0][2]) <= 512 else 4)
        assert not (w["status"] & SV.NOT_CONVERGED).any(), (i, kernel)    # every case of the suite converges
    p = SV.problem(5)
    bits |= int(np.bitwise_or.reduce(ref.run(p["X"], p["y"], **SV.run_kw(p, "linear", max_iter=3))["status"].ravel()))
    print(tot, bits, per_lane)
    assert bits == 7 and per_lane == {1, 2, 4}
    for k in ("opp_clip_0", "opp_clip_C", "eq_clip_C", "eq_clip_0", "tau", "midpoint_bias"):
        assert tot[k] > 0, k
    assert tot["same_row"] == 0


# the bound of the independent check: at the returned alpha every variable's violation is below tol, so
# primal - dual <= sum_v alpha_v max(0, G_v + s_v b) + (C - alpha_v) max(0, -(G_v + s_v b)) <= 2 n C tol
@pytest.mark.parametrize("i, kernel", PAIRS, ids=IDS)
def test_duality_gap_of_every_converged_item(ref, i, kernel):
    p = SV.problem(i)
    w, _ = want(ref, i, kernel)
    worst, checked = 0.0, 0
    for k, n in enumerate(p["n_rows"]):
        for r in range(p["X"].shape[2]):
            if w["status"][k, r] != 0:
                assert w["status"][k, r] in (SV.BAD_INPUT, SV.NONFINITE), (k, r)    # nothing of the suite fails to converge
                if w["status"][k, r] == SV.BAD_INPUT:
                    continue
            C_, e = p["box"][r], p["epsilon"][r]
            gap, primal = SV.dual_gap(p["X"][:n, :, r], p["y"][:n, r], w["beta"][k, :n, r], w["bias"][k, r], kernel, p["kernel_scale"][r], C_, e)
            bound = 2 * n * C_ * SV.TOL
            assert -1e-12 * max(1.0, abs(primal)) <= gap <= bound, (k, r, gap, bound)
            worst, checked = max(worst, gap / bound), checked + 1
    print("items checked", checked, "worst gap / bound", worst)
    assert checked > 0


def test_against_libsvm_through_scikit_learn(ref):
    """tests/golden/svr_sklearn.npz (written by tests/golden/make_golden_svr.py where scikit-learn is installed): SVR.predict
    of LIBSVM at tol 1e-6 on small cases of both kernels.  The gate is 8 x the worst |fitted - sklearn| / max|y| the NumPy
    reading showed when the fixture was written (recorded in the fixture as `measured`)."""
    g = np.load(GOLDEN)
    worst = 0.0
    for c in range(int(g["n_cases"])):
        X, y, n = g[f"X{c}"], g[f"y{c}"], int(g[f"n{c}"])
        kernel = SV.KERNELS[int(g[f"kernel{c}"])]
        o = SV.np_svr(X[:, :, None], y[:, None], (n,), kernel, float(g[f"box{c}"]), float(g[f"eps{c}"]), float(g[f"scale{c}"]),
                      float(g["tol"]), SV.MAX_ITER, ref)
        assert o["status"][0, 0] == 0
        worst = max(worst, np.abs(o["fitted"][0, :, 0] - g[f"pred{c}"]).max() / np.abs(y).max())
    print("worst |fitted - sklearn| / max|y|", worst, "recorded", float(g["measured"]))
    assert worst <= 8 * float(g["measured"])


def test_svr_defaults_are_fitrsvm_s():
    from epidemicmodeling_amd import _lib
    y = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0])
    q = SV.iqr(y[:, None])[0]                                            # quantile at 0.25: pos 1.5 -> 3; at 0.75: pos 5.5 -> 48
    assert q == 45.0
    d = _lib.svr_defaults(y, "linear")
    assert d == {"box": 1.0, "epsilon": 45.0 / 13.49, "kernel_scale": 1.0}
    d = _lib.svr_defaults(np.stack([y, np.ones(8)], axis=1), "gaussian")
    assert d["box"].tolist() == [45.0 / 1.349, 0.0] and d["epsilon"].tolist() == [45.0 / 13.49, 0.1] and d["kernel_scale"].tolist() == [1.0, 1.0]
    with pytest.raises(ValueError, match="kernel must be"):
        _lib.svr_defaults(y, "rbf")


def test_c_reading_under_sanitizers(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.fail("no C compiler for tests/svr_ref.c")
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run([cc, *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler cannot link the sanitizer runtimes")
    exe = str(tmp_path / "ref_main")
    subprocess.run([cc, "-O1", "-g", "-ffp-contract=off", *san, "-DSVR_MAIN", SV.SRC, "-o", exe, "-lm"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode == 0 and "status bits seen 7" in r.stdout and "ERROR" not in r.stderr, (r.stdout[-500:], r.stderr[-2000:])

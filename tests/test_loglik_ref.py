"""The two restatements of the innovation log-likelihood against each other and against the C oracle:
tests/loglik_ref.c and np_loglik agree bit for bit on the oracle's outputs of the seven workloads, and the S they form is the
very denominator the filter divided by: K_GAIN(i, t) == (P- C')(i) / S(t) bit for bit on every observed day."""
import numpy as np
import pytest

from tests import helpers as H
from tests import loglik_ref as LR


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return LR.LoglikRef(tmp_path_factory.mktemp("loglik_ref"))


def _agree(ref, case, **kw):
    a, b = ref.run(case, **kw), LR.np_loglik(ref, case, **kw)
    for k in b:
        assert LR.same_bits(a[k], b[k]), (k, kw)
    return a


def test_fixed_order_log_is_the_librarys(ref):
    """llr_log restates epi_log: the same bits as tests/rt_window_ref.c's restatement of it, and within 1 ulp of libm"""
    from tests import rt_window_ref as RW
    import tempfile
    rw = RW.RtWindowRef(tempfile.mkdtemp())
    rng = np.random.default_rng(5)
    for v in np.concatenate([10.0 ** rng.uniform(-300, 300, 500), [2.9e-17, 1.0, 2.2250738585072014e-308]]):
        assert ref.log(v) == rw.log(v)
        assert abs(ref.log(v) - np.log(v)) <= 2.0 * np.spacing(abs(np.log(v)))


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("name", LR.WORKLOADS)
def test_c_and_numpy_agree(ref, name, storage):
    w, case = LR.oracle_case(name)
    for k0, k1 in LR.WINDOWS:
        if (k1 or w.T) > w.T or k0 >= w.T:
            continue
        got = _agree(ref, case, k0=k0, k1=k1, storage=storage)
        assert np.isfinite(got["loglik"]).all()
    full = ref.run(case, storage=storage)
    assert (full["status"] & 1 == 0).all()
    assert (full["n_valid"] == (~np.isnan(w.x[:, w.x_series if w.x_series is not None else np.arange(w.B)])).sum(axis=0)).all()
    adaptive = w.R_series is None and (w.prm[H.L.PRM_BETA_EKF] != 1.0)
    assert ((full["status"] & 4 != 0) == (adaptive if storage == "f32" else False)).all()


@pytest.mark.parametrize("name", LR.WORKLOADS)
def test_S_is_the_denominator_the_filter_divided_by(ref, name):
    """K_GAIN(i, t) == (P- C')(i) / S(t), i = 0..2, bit for bit on every valid day: no tolerance"""
    w, case = LR.oracle_case(name)
    got = ref.run(case)
    valid = ~np.isnan(got["S"])
    assert valid.sum() == got["n_valid"].sum() > 0
    assert (got["S"][valid] > 0).all()
    with np.errstate(invalid="ignore"):
        gain = got["PCt"] / got["S"][:, None, :]
    v3 = np.broadcast_to(valid[:, None, :], gain.shape)
    assert np.array_equal(gain[v3], case["K_GAIN"][:, :3, :][v3])


def test_replay_is_exercised_and_series_are_passed_through(ref):
    for name in ("row3", "row4"):
        w, case = LR.oracle_case(name)
        Ru = ref.run(case)["R_used"]
        assert w.R_series is None and (np.ptp(Ru, axis=0) > 0).all(), name          # R(k) differs between days
    for name in ("cfg3", "cfg4", "cfg3_bwd", "cfg4_bwd"):
        w, case = LR.oracle_case(name)
        Ru = ref.run(case)["R_used"]
        sx = w.x_series if w.x_series is not None else np.arange(w.B)
        by_step = Ru[::-1] if "Backward" in w.model else Ru                           # R_v is indexed by filter step
        assert np.array_equal(by_step, w.R_series[:, sx]), name


@pytest.mark.parametrize("name", ["cfg3", "cfg4", "row3", "cfg3_bwd"])
def test_missing_days_straddle_a_block_edge(ref, name):
    """x NaN at steps 7, 31, 32 of every third series, one series dark; the oracle is run again for them"""
    w = LR.with_missing_days(LR.oracle_case(name)[0])
    case = LR.case_of(w, H.oracle_batch(w))
    got = _agree(ref, case)
    sx = w.x_series if w.x_series is not None else np.arange(w.B)
    dark = np.flatnonzero(sx == 1)
    assert dark.size and (got["n_valid"][dark] == 0).all() and np.isnan(got["nis_mean"][dark]).all()
    assert (got["loglik"][dark] == 0.0).all() and (got["status"][dark] & 1 == 0).all()
    hit = np.flatnonzero((sx % 3 == 0) & (sx != 1))
    full = (~np.isnan(LR.oracle_case(name)[0].x[:, sx])).sum(axis=0)
    assert (got["n_valid"][hit] == full[hit] - 3).all()
    for k0, k1 in LR.WINDOWS[1:]:
        _agree(ref, case, k0=k0, k1=k1)


@pytest.mark.parametrize("name", ["cfg3", "cfg4", "row4"])
def test_bad_days_are_left_out(ref, name):
    w, case0 = LR.oracle_case(name)
    case = LR.with_bad_days(case0)
    got, clean = _agree(ref, case), ref.run(case0)
    assert (got["status"][[2, 3]] & 1 == 1).all() and (np.delete(got["status"], [2, 3]) & 1 == 0).all()
    assert (got["n_valid"][[2, 3]] == clean["n_valid"][[2, 3]] - 1).all()
    assert np.isnan(got["S"][9, 2]) and got["S"][11, 3] < 0 and np.isnan(got["nis"][[9, 11], [2, 3]]).all()
    assert np.isfinite(got["loglik"]).all()


def test_selection_first_maximum_tie_and_no_candidate(ref):
    """5 regions x 14 candidates of the 70-chain batch; candidate 9 of every region is candidate 3 listed again (equal bits:
    the lower index wins wherever it is the best); region 1's candidates are all unusable"""
    w, case0 = LR.oracle_case("cfg3")
    src = np.arange(70)
    src[np.arange(5) * 14 + 9] = np.arange(5) * 14 + 3
    w2 = w.select(src)
    case = LR.case_of(w2, H.oracle_batch(w2))
    case["P_MINUS"] = case["P_MINUS"].copy()
    case["P_MINUS"][10, 0, 14:28] = np.nan                   # a bad day in every candidate of region 1
    got = _agree(ref, case, G=14)
    assert got["best"][1] == -1 and np.isnan(got["best_loglik"][1])
    ll = got["loglik"].reshape(5, 14)
    assert (ll[:, 9] == ll[:, 3]).all()
    for r in (0, 2, 3, 4):
        assert got["best"][r] == np.argmax(ll[r]) and got["best_loglik"][r] == ll[r].max()
    # make the duplicated candidate the best of region 0: the tie goes to index 3
    case["innovations"] = case["innovations"].copy()
    for g in range(14):
        if g not in (3, 9):
            case["innovations"][:, g] = 1.0              # a whole population: far outside every S
    tie = _agree(ref, case, G=14)
    assert tie["best"][0] == 3 and tie["loglik"][3] == tie["loglik"][9] == tie["best_loglik"][0]

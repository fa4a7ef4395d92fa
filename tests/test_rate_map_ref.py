"""The NPI-to-growth-rate predictor without a GPU: the two restatements (tests/rate_map_ref.c and the NumPy loop reading in
tests/rate_map_ref.py) agree bit for bit on every shape of the GPU suite; known answers; the solve against an independent
solver; the C reading as a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import rate_map_ref as RM

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return RM.RatemapRef(tmp_path_factory.mktemp("ratemap_ref"))


def _base(T=12, n=2, R=3, lags=(), n_train=(8,), seed=5, **kw):
    p = RM.make_case(seed, T, n, lags, 0, len(n_train), R, n_train)
    p.update(kw)
    return p


@pytest.mark.parametrize("fit", (1, 0))
@pytest.mark.parametrize("i", range(len(RM.CASES)))
def test_c_and_numpy_readings_agree_bit_for_bit(ref, i, fit):
    p = RM.problem(i, fit)
    a = ref.run(p, [k for k in RM.OUT_NAMES if fit or k != "map"])
    b = RM.np_rate_map(p, ref.fma, ref.exp)
    assert set(a) == set(b)
    for k in a:
        assert RM.same_bits(a[k], b[k]), k


def test_the_shared_cases_reach_every_status_and_branch(ref):
    seen, per_lane, hi, lo, filled, inf_first, zero_train, const_col, zero_col = 0, set(), 0, 0, 0, 0, 0, 0, 0
    for i, ((T, n, lags, E, K, R), nt) in enumerate(RM.CASES):
        p = RM.problem(i)
        o = ref.run(p)
        F = n * (1 + len(lags)) + E
        per_lane.add(-(-((F + 1) * (F + 2) // 2 - 1) // 256))
        st = o["status"]
        seen |= int(np.bitwise_or.reduce(st.ravel()))
        assert set(np.unique(st)) <= {0, 1, 2, 4}                       # a failure status stands alone
        ok = st == 0
        for k in range(K):
            test = o["lambda_hat"][k, nt[k]:][:, ok[k]]
            hi, lo = hi + int((test == p["thr"]).sum()), lo + int((test == -p["thr"]).sum())
            assert not (np.abs(test) > p["thr"]).any()
        bad = ~np.isfinite(p["y"])
        filled += int((bad[1:] & np.isfinite(o["y_filled"][1:])).sum())
        inf_first += int(np.isinf(p["y"][0]).sum())
        zero_train += sum(int(lag >= t) for lag in lags for t in nt)
        const_col += int((p["ip"][:, :, 0] == p["ip"][0, :, 0]).all(axis=0).any())
        zero_col += int((o["x_mx"][:n] == 1.0).any() and (p["ip"] == 0).all(axis=0).any())
        assert (st[:, 1] == RM.LEADING_NAN).all() if R >= 2 else True
        assert (st[:, R - 1] == RM.NOT_PD).all() if R >= 3 else True
    assert seen == 7 and per_lane == {1, 2, 5, 9, 19}                   # every instantiation of the kernel (9 runs as 10)
    assert min(hi, lo, filled, inf_first, zero_train, const_col, zero_col) > 0, (hi, lo, filled, inf_first, zero_train, const_col, zero_col)
    for i in (1, 6):                                                    # without a fit: NaN and Inf rates reach NONFINITE
        assert set(np.unique(ref.run(RM.problem(i, 0), ("status",))["status"])) == {0, 4}


def test_one_feature_without_ridge_is_the_scalar_quotient(ref):
    p = _base(T=8, n=1, R=2, n_train=(6,), ridge=0.0)
    o = ref.run(p)
    for r in range(2):
        x = p["ip"][:, 0, r] / o["x_mx"][0, r]
        sxx, sxy = x[0] * x[0], x[0] * p["y"][0, r]
        for t in range(1, 6):
            sxx, sxy = ref.fma(x[t], x[t], sxx), ref.fma(x[t], p["y"][t, r], sxy)
        l = np.sqrt(sxx)
        assert RM.same_bits(o["map"][0, 0, r], np.float64((sxy / l) / l))
        assert abs(o["map"][0, 0, r] - sxy / sxx) <= 2 * EPS * abs(sxy / sxx)


def test_train_end_at_the_last_day(ref):
    p = _base(T=15, n=3, R=4, lags=(3,), n_train=(15,))
    o = ref.run(p)
    assert RM.same_bits(o["lambda_hat"][0], o["y_filled"]) and RM.same_bits(o["new_cases_est"][0], p["new_smoothed"])
    assert np.isfinite(o["map"]).all() and (o["status"] == 0).all()


def test_all_zero_training_columns(ref):
    p = _base(T=14, n=3, R=3, lags=(3, 9), n_train=(5, 12))
    p["ip"][:, 1, :] = 0.0                                              # a plan that is 0 throughout
    p["ip"][:3] = np.maximum(p["ip"][:3], 0.0)
    o = ref.run(p)
    assert (o["status"] == 0).all()
    assert (o["x_mx"][1] == 1.0).all() and (o["map"][:, 1] == 0.0).all()
    assert (o["x_mx"][4] == 1.0).all() and (o["x_mx"][7] == 1.0).all() and (o["map"][:, 4] == 0.0).all()
    assert (o["map"][0, 6:9] == 0.0).all()                              # lag 9 >= train end 5
    assert (o["map"][1, 6] != 0.0).any()                                # ... but not train end 12


def test_constant_rate_without_a_fit(ref):
    T, nt, c = 60, 10, 0.01
    p = _base(T=T, n=1, R=2, n_train=(nt,))
    p["lambda_in"], p["fit"] = np.full((1, T, 2), c), 0
    o = ref.run(p, ("lambda_hat", "new_cases_est", "status"))
    assert (o["status"] == 0).all() and (o["lambda_hat"] == c).all()
    for j in range(1, T - nt + 1):
        want = p["new_smoothed"][nt - 1] * np.exp(np.longdouble(j) * np.longdouble(c))
        rel = np.abs((o["new_cases_est"][0, nt + j - 1] - want) / want).astype(np.float64)
        # j - 1 roundings in the running sum (each at most u relative to |j c| < 1), exp within 1 ulp, one product
        assert (rel <= (j + 3) * EPS).all(), (j, rel / EPS)


def test_clip_touches_the_test_days_only(ref):
    T, nt = 10, 5
    p = _base(T=T, n=1, R=1, n_train=(nt,))
    lam = np.array([0.5, -0.5, 0.05, np.nan, 0.2, 0.5, -0.5, 0.05, np.nan, 0.1])
    p["lambda_in"], p["fit"] = lam.reshape(1, T, 1), 0
    o = ref.run(p, ("lambda_hat", "status"))
    assert RM.same_bits(o["lambda_hat"][0, :, 0], np.array([0.5, -0.5, 0.05, np.nan, 0.2, 0.1, -0.1, 0.05, np.nan, 0.1]))
    assert o["status"][0, 0] == RM.NONFINITE


def test_target_fill(ref):
    p = _base(T=9, n=1, R=3, n_train=(6,))
    p["y"][:, 0] = [0.1, np.nan, np.inf, 0.2, -np.inf, np.nan, 0.3, np.nan, np.nan]
    p["y"][0, 1] = np.nan
    p["y"][:3, 2] = [np.inf, np.nan, 0.1]
    o = ref.run(p)
    assert RM.same_bits(o["y_filled"][:, 0], np.array([0.1, 0.1, 0.1, 0.2, 0.2, 0.2, 0.3, 0.3, 0.3]))
    assert o["status"][0, 0] == 0 and RM.same_bits(o["lambda_hat"][0, :6, 0], o["y_filled"][:6, 0])
    assert o["status"][0, 1] == RM.LEADING_NAN
    assert np.isnan(o["map"][0, :, 1]).all() and np.isnan(o["lambda_hat"][0, :, 1]).all() and np.isnan(o["new_cases_est"][0, :, 1]).all()
    assert np.isnan(o["y_filled"][0, 1]) and np.isfinite(o["y_filled"][1:, 1]).all()      # the fill itself is as written
    assert RM.same_bits(o["y_filled"][:3, 2], np.array([np.inf, np.inf, 0.1])) and o["status"][0, 2] == RM.NONFINITE


def test_tracker_by_hand(ref):
    # the mean plan over 10 days: a rise on day 3, a fall on day 5, a rise on day 8 and a fall on day 10 (effect_lag 3: the last
    # two start on day 10, the last day)
    avg = np.array([1, 1, 2, 2, 1, 1, 1, 3, 3, 2], dtype=np.float64)
    p = _base(T=10, n=2, R=1, n_train=(5,))
    p["ip"][:, 0, 0], p["ip"][:, 1, 0] = avg + 1, avg - 1
    o = ref.run(p, ("tracker",))
    d = 0.01
    want = np.array([0, 0, 0, 0, 0, 0 - d, 0 - d, (0 - d) + d, (0 - d) + d, (((0 - d) + d) - d) + d])
    assert RM.same_bits(o["tracker"][:, 0], want)
    p["effect_lag"] = 0
    want0 = np.array([0, 0, 0 - d, 0 - d, (0 - d) + d, (0 - d) + d, (0 - d) + d, ((0 - d) + d) - d, ((0 - d) + d) - d, (((0 - d) + d) - d) + d])
    assert RM.same_bits(ref.run(p, ("tracker",))["tracker"][:, 0], want0)


def test_not_pd_stays_with_its_item(ref):
    p = _base(T=20, n=3, R=3, n_train=(12, 18), ridge=0.0)
    q = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    q["ip"][:, 1, 1] = 0.0                                              # region 1: a zero column and no ridge
    a, b = ref.run(p), ref.run(q)
    assert (a["status"] == 0).all()
    assert (b["status"][:, 1] == RM.NOT_PD).all() and (b["status"][:, [0, 2]] == 0).all()
    for k in ("map", "lambda_hat", "new_cases_est"):
        assert np.isnan(b[k][:, :, 1]).all() and RM.same_bits(a[k][:, :, [0, 2]], b[k][:, :, [0, 2]]), k


# ---- the solve against independent solvers ---------------------------------------------------------------------------
# measured on these inputs (300 items): no NOT_PD; cond(G) up to 1.5e10, the smallest pivot is the ridge; the worst normwise
# residual of the restatement's map is 1.04 eps; its distance to lstsq on the stacked system is at most 1.2 eps cond(G)
WORST_RESIDUAL_EPS, WORST_LSTSQ_EPS_COND = 1.04, 1.2


def probe_inputs(draws=50, T=366, n=12, seed=2024):
    """synthetic piecewise-constant plans with switch probabilities 0 .. 0.1 over the draws"""
    g = np.random.default_rng(seed)
    ip = np.empty((T, n, draws))
    prob = np.linspace(0.0, 0.1, draws)
    lvl = g.integers(0, 5, size=(n, draws)).astype(np.float64)
    for t in range(T):
        sw = g.random((n, draws)) < prob[None, :]
        lvl = np.where(sw, g.integers(0, 5, size=(n, draws)), lvl)
        ip[t] = lvl
    w = np.abs(g.normal(0, 0.03, size=(n, draws)))
    y = 0.15 - np.einsum("tnr,nr->tr", ip, w) + g.normal(0, 0.05, size=(T, draws))
    ns = 50.0 + 500.0 * g.random((T, draws))
    return dict(ip=ip, y=y, new_smoothed=ns, extra=None, lambda_in=None, n_train=(1, 5, 30, 120, 275, 366), lags=(3, 5, 7), fit=1,
                effect_lag=3, ridge=1e-6, thr=0.1, red=0.01)


def test_solve_against_independent_solvers(ref):
    p = probe_inputs()
    o = ref.run(p, ("map", "x_mx", "status"))
    assert (o["status"] == 0).all()                                     # no item skipped, NOT_PD does not occur
    worst, worst_ls = 0.0, 0.0
    for r in range(p["ip"].shape[2]):
        X = RM.features(p["ip"][:, :, r], p["lags"], None) / o["x_mx"][:, r][None, :]
        F = X.shape[1]
        for k, nt in enumerate(p["n_train"]):
            Xt, yt, m = X[:nt], p["y"][:nt, r], o["map"][k, :, r]
            G, c = Xt.T @ Xt + p["ridge"] * np.eye(F), Xt.T @ yt
            worst = max(worst, np.abs(G @ m - c).max() / (np.abs(G).sum(axis=1).max() * np.abs(m).max() + np.abs(c).max()) / EPS)
            mls = np.linalg.lstsq(np.vstack([Xt, np.sqrt(p["ridge"]) * np.eye(F)]), np.concatenate([yt, np.zeros(F)]), rcond=None)[0]
            worst_ls = max(worst_ls, np.abs(m - mls).max() / np.abs(mls).max() / (EPS * np.linalg.cond(G)))
    print(f"worst residual {worst:.3f} eps, worst distance to lstsq {worst_ls:.3f} eps cond(G)")
    assert worst <= 8 * WORST_RESIDUAL_EPS
    assert worst_ls <= 8 * WORST_LSTSQ_EPS_COND                         # condition-limited, not a bit gate


def test_c_reading_under_sanitizers(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.fail("no C compiler for tests/rate_map_ref.c")
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run([cc, *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler cannot link the sanitizer runtimes")
    exe = str(tmp_path / "ref_main")
    subprocess.run([cc, "-O1", "-g", "-ffp-contract=off", *san, "-DRATE_MAP_MAIN", RM.SRC, "-o", exe, "-lm"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode == 0 and "status bits seen 3" in r.stdout and "ERROR" not in r.stderr, (r.stdout[-500:], r.stderr[-2000:])

"""Generates tests/golden/aux_*.npz: seeded inputs + expected outputs of the stages around the filter
(SURVEY.md 8(f)): Rt_ExpFitEKF, per-region preprocessing, the NNLS regression, random-NPI plans and the Pareto filter;
and of the forecast look-ahead study, the sliding-window growth-rate estimators and the cross-validated LASSO.

As for make_golden.py the reference cannot run here, so outputs come from oracle/ekf_oracle.c and generation FAILS
unless the independent reading agrees: oracle/ekf_numpy.py for Rt_ExpFitEKF and the preprocessing (SciPy's lfilter /
filtfilt), SciPy's Lawson-Hanson for the NNLS, a vectorised NumPy restatement for the Pareto filter, the Random123
known-answer vectors for the generator behind the plans.  The three newer calls come from their C / Python restatements
(tests/lookahead_ref.py, tests/rt_window_ref.c, tests/lasso_ref.c), gated by the loop transcription of the .m code (look-
ahead), NumPy's readings and SciPy's Levenberg-Marquardt (rt_window), the KKT conditions and scikit-learn (LASSO).  Only
data is stored.  A file whose arrays are unchanged is not rewritten (a zip archive carries its write time).

    python tests/golden/make_golden_aux.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from epidemicmodeling_amd import synth  # noqa: E402
from oracle import ekf_numpy as enp  # noqa: E402
from oracle import oracle_lib as olib  # noqa: E402
from tests import helpers as H  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def rt_case(order):
    w = synth.make_rt(5, 140, order=order, horizon=14, w_bar=(0.5, 1e-4), seed=order)
    w.x[40:44, 1] = np.nan
    ob = olib.rt_expfit_batch(w.x, w.rp, w.L, order)
    names = ["S_MINUS", "S_PLUS", "P_MINUS", "P_PLUS", "K_GAIN", "S_SMOOTH", "P_SMOOTH", "innovations", "rho"]
    for c in range(w.B):
        rp = w.rp[:, c]
        nd = dict(zip(names, enp.rt_expfit_ekf(w.x[:, c], rp[9:11], rp[0:3], rp[3:5], rp[5], rp[11:15].reshape(2, 2, order="F"),
                                               rp[15:19].reshape(2, 2, order="F"), rp[6], rp[7], rp[8], w.L, order)))
        assert H.rel_err(ob["S_SMOOTH"][:, :, c].T, nd["S_SMOOTH"]) <= 1e-11 and H.rel_err(ob["rho"][:, c], nd["rho"]) <= 1e-11
    d = {"in_x": w.x, "in_rp": w.rp, "in_L": w.L, "in_order": order}
    d.update({"out_" + k: v for k, v in ob.items()})
    return d


def pre_case():
    raw = synth.make_raw_counts(6, 120, seed=8)
    keys = ["new_refined", "new_smoothed", "zero_lag", "x_new", "x_total", "R_v", "fatality"]
    out = {k: np.zeros((120, 6)) for k in keys}
    I0 = np.zeros(6)
    for r in range(6):
        a = olib.preprocess_region(raw["cases"][:, r], raw["deaths"][:, r], raw["population"][r])
        b = enp.preprocess_region(raw["cases"][:, r], raw["deaths"][:, r], raw["population"][r])
        for k in keys:
            assert H.rel_err(a[k], b[k]) <= 1e-13, (r, k)
            out[k][:, r] = a[k]
        I0[r] = a["I0"]
    ipf = np.stack([olib.npi_fill(np.ascontiguousarray(raw["ip"][:, :, r])) for r in range(6)], axis=2)
    assert np.array_equal(ipf[:, :, 2], enp.npi_fill(raw["ip"][:, :, 2]))
    d = {"in_" + k: raw[k] for k in ("cases", "deaths", "population", "ip")}
    d.update({"out_" + k: v for k, v in out.items()})
    d["out_I0"] = I0; d["out_ip_filled"] = ipf
    return d


def nnls_case():
    from scipy.optimize import nnls as sp_nnls
    X, y = H.make_regression_problem(9, 80, 12, seed=4)
    a = np.zeros((12, 9)); b = np.zeros(9); e = np.zeros(9); it = np.zeros(9, dtype=np.int32)
    for s in range(9):
        f = olib.nnls_affine_fit(np.ascontiguousarray(X[:, :, s]), np.ascontiguousarray(y[:, s]))
        ref, rn = sp_nnls(X[:, :, s], y[:, s])
        assert abs(np.linalg.norm(X[:, :, s] @ olib.nnls(X[:, :, s], y[:, s]) - y[:, s]) - rn) <= 1e-12
        a[:, s], b[s], e[s], it[s] = f["a"], f["b"], f["min_err"], f["iters"]
    return {"in_X": X, "in_y": y, "out_a": a, "out_b": b, "out_min_err": e, "out_iters": it}


def scenario_case():
    assert olib.philox4x32_10([0] * 4, [0] * 2) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    R, n_scen, K = 3, 10, 12
    plans = np.zeros((n_scen, R, 12, K))
    for j in range(n_scen):
        for r in range(R):
            plans[j, r] = olib.random_npi_plan(0xABCDEF0123, r, j, n_scen, K, np.zeros(12), synth.IP_MAXES)
    rng = np.random.default_rng(6)
    J0, J1 = rng.random((4, 40)), rng.random((4, 40))
    J0[:, 3] = J0[:, 1]; J0[0, 5] = np.nan
    on = np.zeros((4, 40), dtype=bool); io = np.zeros(4, dtype=np.int32)
    for r in range(4):
        on[r], io[r] = olib.pareto_front(J0[r], J1[r])
        dom = (J0[r][None, :] < J0[r][:, None]) & (J1[r][None, :] < J1[r][:, None])
        assert np.array_equal(on[r], dom.sum(axis=1) == 0)
    return {"in_seed": 0xABCDEF0123, "in_n_scen": n_scen, "in_K": K, "out_plans": plans, "in_J0": J0, "in_J1": J1,
            "out_on_front": on, "out_i_opt": io}


def lookahead_case():
    """3 regions x 80 days, F = 72, M = 8: n = 65 rows per statistics column (a second pass of the wavefront's lanes), zero
    truth days (Inf entries) on row indices 0 and 64"""
    from tests import lookahead_ref as LR
    R, LL, F, M = 3, 80, 72, 8
    w = synth.make_cfg3(R, LL)
    N = synth.make_regions(R)["N"].astype(np.float64)
    truth = w.x * N[None, :] + 50.0
    truth[LL - 1, 0] = 0.0
    truth[LL - (M + 64), 1] = 0.0
    truth = np.ascontiguousarray(truth)
    exp = LR.expected(w, truth, N, F, M)
    EP, ES, st = LR.matlab_loop(exp["S_PLUS"], exp["S_SMOOTH"], truth, N, F, M)
    assert np.array_equal(EP, exp["est_plus"], equal_nan=True) and np.array_equal(ES, exp["est_smooth"], equal_nan=True)
    for k, v in st.items():                       # NumPy's mean / std sum pairwise, its median averages: a few ulp apart
        assert np.allclose(v, exp[k], rtol=1e-12, atol=0.0, equal_nan=True), k
    assert np.isinf(exp["est_plus"][M - 1:]).any()
    d = {"in_" + k: getattr(w, k) for k in ("x", "u", "R_series", "prm", "s_init", "Ps_init", "s_final", "Ps_final", "Q")}
    d.update(in_L=w.L, in_order=w.order, in_truth=truth, in_population=N, in_F=F, in_M=M)
    d.update({"out_" + k: exp[k] for k in ("est_plus", "est_smooth", "mean_plus", "median_plus", "std_plus", "mean_smooth",
                                           "median_smooth", "std_smooth")})
    return d


RTW_CONFIGS = ((31, 1, 7.0, 1), (6, 0, 0.25, 60))       # wlen, causal, time_unit, generation_period


def rt_window_case():
    """6 noisy exponentials of 60 days through all three estimators: a causal 31-sample window with generation_period 1, and
    a centred 7-sample one with generation_period = L"""
    import tempfile
    from scipy.optimize import least_squares
    from tests.rt_window_ref import RtWindowRef, np_genratios, np_loglinreg, ST_TOLFUN, ST_TOLX
    ref = RtWindowRef(tempfile.mkdtemp())
    rng = np.random.default_rng(12)
    L, R = 60, 6
    t = np.arange(L)[:, None]
    x = rng.uniform(20, 800, R) * np.exp(rng.uniform(-0.06, 0.08, R) * t + 0.3 * np.sin(t / 9.0))
    x = np.ascontiguousarray(x * (1.0 + 0.03 * rng.standard_normal((L, R))))
    d = {"in_x": x}
    for c, (wlen, causal, tu, gp) in enumerate(RTW_CONFIGS):
        out = ref.all(x, wlen, tu, causal, gp)
        lo = wlen - 1 if causal else wlen // 2
        hi = L if causal else L - wlen // 2
        fit_windows = 0
        for r in range(R):
            for k, v in np_loglinreg(x[:, r], wlen, tu, causal).items():
                assert np.allclose(out["llr_" + k][:, r], v, rtol=1e-12, atol=1e-13), (c, r, k)
            for k, v in np_genratios(x[:, r], wlen, gp, tu).items():
                assert np.allclose(out["gr_" + k][:, r], v, rtol=1e-12, atol=1e-13), (c, r, k)
            n = np.arange(-wlen + 1, 1) if causal else np.arange(-(wlen // 2), wlen // 2 + 1)
            for mm in range(lo, hi, 4):
                seg = x[mm + n, r]
                tt = n / tu
                b = least_squares(lambda p: p[0] * np.exp(p[1] * tt) - seg, [x[mm, r], 0.0], method="lm", xtol=1e-15,
                                  ftol=1e-15, gtol=1e-15).x
                assert out["nls_status"][mm, r] in (ST_TOLX, ST_TOLFUN), (c, r, mm)
                sse = ((seg - out["nls_A"][mm, r] * np.exp(out["nls_Lambda"][mm, r] * tu * tt)) ** 2).sum()
                assert sse <= ((seg - b[0] * np.exp(b[1] * tt)) ** 2).sum() * (1 + 2e-6) + 1e-15 * (seg ** 2).sum(), (c, r, mm)
                fit_windows += 1
        assert fit_windows > 0
        d.update({f"in_c{c}_wlen": wlen, f"in_c{c}_causal": causal, f"in_c{c}_time_unit": tu, f"in_c{c}_gp": gp})
        d.update({f"out_c{c}_{k}": v for k, v in out.items()})
    return d


def lasso_case():
    """6 regions, D = 40 days, n = 12 columns, K = 5 folds, 100 lambdas; make_problem's specials (a column constant on one
    fold's training set, a constant y, a NaN in X, only constant columns)"""
    import tempfile
    from sklearn.linear_model import Lasso
    from tests.lasso_ref import LassoRef, ST_OK, sklearn_cv
    from tests.test_lasso_host import _standardized, make_problem
    ref = LassoRef(tempfile.mkdtemp())
    R, D, n, K, NL, rel_tol = 6, 40, 12, 5, 100, 1e-4
    X, y, fold = make_problem(R, D, n, K, seed=21)
    o = ref.run(X, y, fold, K, NL)
    ok = [r for r in range(R) if o["status"][r] == ST_OK]
    assert len(ok) >= 2
    gated = 0
    for r in ok:                                  # the bounds of test_lasso_host.py and of tests/lasso_ref.py::sklearn_cv
        Xs, Y0, sig, cst = _standardized(X[:, :, r], y[:, r])
        G = Xs.T @ Xs / D
        obj = lambda b, lam: 0.5 * np.sum((Y0 - Xs @ b) ** 2) / D + lam * np.abs(b).sum()
        for k in range(NL):
            lam, b = o["lambda"][k, r], o["B"][k, :, r] * sig
            g = Xs.T @ (Y0 - Xs @ b) / D
            bound = rel_tol * np.abs(G) @ ((1 + np.abs(b)) * (1 + rel_tol)) + 1e-12 * (np.abs(Xs).T @ np.abs(Y0) / D + lam)
            act, zero = (b != 0) & ~cst, (b == 0) & ~cst
            assert np.all(np.abs(g[act] - lam * np.sign(b[act])) <= bound[act]), (r, k)
            assert np.all(np.abs(g[zero]) <= lam + bound[zero]), (r, k)
            if k % 10 == 0:
                bs = Lasso(alpha=lam, fit_intercept=False, tol=1e-13, max_iter=1_000_000).fit(Xs, Y0).coef_
                assert obj(b, lam) - obj(bs, lam) <= np.abs(bound) @ np.abs(b - bs) + 1e-13 * obj(np.zeros(n), lam), (r, k)
        mse, se, g_mse, g_se = sklearn_cv(X[:, :, r], y[:, r], fold[:, r], K, o["lambda"][:, r], rel_tol)
        v = ~np.isnan(g_mse)
        assert np.all(np.abs(o["mse"][v, r] - mse[v]) <= g_mse[v]) and np.all(np.abs(o["se"][v, r] - se[v]) <= g_se[v]), r
        gated += v.sum()
    assert gated > 0
    d = {"in_X": X, "in_y": y, "in_fold": fold, "in_K": K, "in_NL": NL}
    d.update({"out_" + k: v for k, v in o.items()})
    return d


def _unchanged(path, d):
    """the file at `path` holds exactly the arrays of d (bit for bit)"""
    if not os.path.exists(path):
        return False
    with np.load(path) as g:
        if set(g.files) != set(d):
            return False
        for k, v in d.items():
            a, b = np.asarray(v), g[k]
            if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
                return False
    return True


def main():
    for name, make in (("aux_rt_order1", lambda: rt_case(1)), ("aux_rt_order2", lambda: rt_case(2)),
                       ("aux_preprocess", pre_case), ("aux_nnls", nnls_case), ("aux_scenarios", scenario_case),
                       ("aux_lookahead", lookahead_case), ("aux_rt_window", rt_window_case), ("aux_lasso", lasso_case)):
        path = os.path.join(HERE, name + ".npz")
        d = make()
        if _unchanged(path, d):
            print(f"{name}: unchanged")
            continue
        np.savez_compressed(path, **d)
        print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()

"""The two restatements of the innovation whiteness diagnostics without a device: tests/innov_diag_ref.c and the
NumPy reading np_idiag agree bit for bit on the device list's cases; on series without missing days they agree with direct
NumPy / scipy formulas; the Ljung-Box test tells white series from AR(1) ones; the p-values agree with scipy.stats.chi2."""
import numpy as np
import pytest
import scipy.stats

from tests import innov_diag_ref as DR
from tests import noise_ref as NR


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return DR.InnovDiagRef(tmp_path_factory.mktemp("innov_diag_ref"))


@pytest.mark.parametrize("name", [r[0] for r in DR.CASES])
def test_c_and_numpy_agree(ref, name):
    e, S, kw, _ = DR.make_case(name)
    got, want = ref.run(e, S, **kw), DR.np_idiag(e, S, **kw)
    assert list(got) == list(DR.ALL)
    for k in DR.ALL:
        assert DR.same_bits(got[k], want[k]), (name, k)


def test_the_cases_reach_every_status_bit_and_edge(ref):
    e, S, kw, _ = DR.make_case("plain")
    out = ref.run(e, S, **kw)
    st = out["status"]
    assert (st[[3, 4, 5, 6, 7, 8]] & DR.BAD_DAY).all() and not (st[[0, 11, 12]] & DR.BAD_DAY).any()
    assert st[1] == DR.EMPTY and out["n"][1] == 0 and np.isnan(out["mean"][1]) and out["cusumsq_step"][1] == -1
    assert st[9] & DR.DEGENERATE and np.isnan(out["acf"][:, 9]).all() and out["var"][9] == 0.0
    assert out["n"][10] == 1 and st[10] == DR.DEGENERATE | DR.FEW_LAGS and out["lb_lags"][10] == 0 and np.isnan(out["lb_q"][10])
    assert out["n"][2] == 45 - 13 and out["n"][0] == 45 - 3                 # a dark block (13 of its days exist); steps 7, 31, 32
    # H = 64 > n - 1 sets bit 3 and leaves the rows beyond Hu NaN
    e, S, kw, _ = DR.make_case("lags_64")
    out = ref.run(e, S, **kw)
    assert (out["status"][11:] & DR.FEW_LAGS).all() and out["lb_lags"][11] == 44
    assert np.isfinite(out["acf"][:44, 11]).all() and np.isnan(out["acf"][44:, 11]).all() and np.isfinite(out["lb_q"][11])
    # k0 = k1: nothing counts
    e, S, kw, _ = DR.make_case("window_empty")
    out = ref.run(e, S, **kw)
    assert (out["status"] == DR.EMPTY).all() and (out["n"] == 0).all() and np.isnan(out["het"]).all()


def test_cusum_of_the_last_counted_step_is_exactly_zero(ref):
    """cs of the last counted step is prefix / q - n / n = 0 by construction"""
    for name in ("plain", "two_blocks_ahead", "float_blocked_flip"):      # chain 10 has a single counted day: its only cs
        e, S, kw, _ = DR.make_case(name)
        out = ref.run(e, S, **kw)
        assert out["n"][10] == 1 and out["cusumsq_max"][10] == 0.0 and out["cusumsq_step"][10] == kw["k0"] + 3
    # directly: the running prefix of the last counted step equals q bit for bit, on chains with missing days and blocks
    e, S, kw, _ = DR.make_case("two_blocks_ahead")
    x = DR.np_idiag(e, S, **kw)
    for c in (0, 2, 11):
        ok = np.isfinite(S[:, c]) & (S[:, c] >= DR.DBL_MIN) & np.isfinite(e[:, c])
        nu = np.where(ok, e[:, c] / np.sqrt(np.where(ok, S[:, c], 1.0)), 0.0)
        done = 0.0
        for b in range(4):
            run = 0.0
            for k in range(32 * b, min(32 * b + 32, 100)):
                if ok[k]:
                    run = run + nu[k] * nu[k]
                    last = done + run
            done = done + run
        assert last == x["nis_sum"][c] and last / x["nis_sum"][c] - float(ok.sum()) / float(x["n"][c]) == 0.0


def _direct(nu, H, k0, k1):
    """plain formulas on one complete series"""
    v = nu[k0:k1]
    n = len(v)
    d = v - v.mean()
    m2 = (d * d).sum()
    acf = np.array([(d[:-h] * d[h:]).sum() / m2 for h in range(1, H + 1)])
    lb = n * (n + 2) * sum(acf[h - 1] ** 2 / (n - h) for h in range(1, H + 1))
    h3 = (2 * n + 3) // 6
    het = (v[n - h3:] ** 2).mean() / (v[:h3] ** 2).mean()
    return dict(acf=acf, skew=scipy.stats.skew(v), kurt=scipy.stats.kurtosis(v, fisher=False), jb=scipy.stats.jarque_bera(v).statistic,
                lb_q=lb, het=het, mean=v.mean(), var=v.var(), nis_sum=(v * v).sum())


@pytest.mark.parametrize("k0, k1", [(0, 400), (21, 390)])
def test_independent_formulas_agree(ref, k0, k1):
    rng = np.random.default_rng(20261021)
    T, B, H = 400, 8, 10
    S = np.exp(rng.uniform(-1.0, 3.0, size=(T, B)))
    e = rng.standard_normal((T, B)) * np.sqrt(S)
    out = ref.run(e, S, H=H, k0=k0, k1=k1)
    assert (out["status"] == 0).all() and (out["n"] == k1 - k0).all()
    for c in range(B):
        want = _direct(e[:, c] / np.sqrt(S[:, c]), H, k0, k1)
        for k in ("skew", "kurt"):
            assert abs(out[k][c] - want[k]) <= 1e-11, (k, c)
        assert np.abs(out["acf"][:, c] - want["acf"]).max() <= 1e-11
        for k in ("lb_q", "jb", "het"):
            assert abs(out[k][c] - want[k]) <= 1e-9 * abs(want[k]), (k, c)
        for k in ("mean", "var", "nis_sum"):
            assert abs(out[k][c] - want[k]) <= 1e-11 * max(1.0, abs(want[k])), (k, c)
        assert out["max_abs_step"][c] == k0 + int(np.argmax(np.abs(e[k0:k1, c] / np.sqrt(S[k0:k1, c]))))


LB_SEED = 7          # recorded: the first seed tried; 64 white series of batch.normal_draws' restatement, T = 400, H = 10


def test_ljung_box_discriminates(ref):
    from epidemicmodeling_amd import pipeline
    import torch
    z = NR.fill(LB_SEED, 0, 0, 400, 1, 0, 64)[:, 0, :]
    ar = np.empty_like(z)
    ar[0] = z[0]
    for k in range(1, 400):
        ar[k] = 0.5 * ar[k - 1] + z[k]
    p = {}
    for name, series in (("white", z), ("ar", ar)):
        out = ref.run(series, None, H=10)
        assert (out["lb_lags"] == 10).all() and (out["status"] == 0).all()
        p[name] = scipy.stats.chi2.sf(out["lb_q"], 10)
        mine = pipeline.diagnostic_pvalues({k: torch.as_tensor(out[k]) for k in ("lb_q", "lb_lags")})["lb_p"].numpy()
        assert np.allclose(mine, p[name], rtol=1e-7, atol=0.0)
    print("white series with lb_p < 0.01:", int((p["white"] < 0.01).sum()), " largest AR lb_p:", p["ar"].max())
    assert (p["white"] < 0.01).sum() <= 3
    assert (p["ar"] < 1e-4).all()


DOFS = list(range(1, 65)) + [100, 200, 400, 520]


def pvalue_grid():
    """(dof, x, sf, cdf) of the issue's grid: 400 points of x up to 4 dof + 50 per dof, restricted to p >= 1e-12"""
    dof = np.repeat(np.array(DOFS, dtype=np.float64), 400)
    x = np.concatenate([np.linspace(0.0, 4.0 * d + 50.0, 401)[1:] for d in DOFS])
    sf, cdf = scipy.stats.chi2.sf(x, dof), scipy.stats.chi2.cdf(x, dof)
    return dof, x, sf, cdf


def pvalue_errors(device):
    """worst relative errors of pipeline.diagnostic_pvalues' lb_p and nis_p on `device` against scipy over the grid"""
    import torch
    from epidemicmodeling_amd import pipeline
    dof, x, sf, cdf = pvalue_grid()
    t = lambda a, dt=torch.float64: torch.as_tensor(a).to(dt).to(device)
    got = pipeline.diagnostic_pvalues({"lb_q": t(x), "lb_lags": t(dof, torch.int32), "nis_sum": t(x), "n": t(dof, torch.int32),
                                       "jb": t(x)})
    lb, nis, jb = (got[k].cpu().numpy() for k in ("lb_p", "nis_p", "jb_p"))
    keep = sf >= 1e-12
    two = 2.0 * np.minimum(sf, cdf)
    keep2 = two >= 1e-12
    return {"lb_p": float(np.max(np.abs(lb[keep] - sf[keep]) / sf[keep])),
            "nis_p": float(np.max(np.abs(nis[keep2] - two[keep2]) / two[keep2])),
            "jb_p": float(np.max(np.abs(jb[x <= 55.0] - np.exp(-0.5 * x[x <= 55.0])) / np.exp(-0.5 * x[x <= 55.0])))}


def test_pvalues_against_scipy_chi2():
    err = pvalue_errors("cpu")
    print("worst relative errors on the CPU:", err)
    assert err["lb_p"] <= 1e-7 and err["nis_p"] <= 1e-7
    assert err["jb_p"] <= 1e-14                              # one exp on either side, each good to an ulp or two (p >= 1e-12)

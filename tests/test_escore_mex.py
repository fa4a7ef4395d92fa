"""The MATLAB boundary of the probabilistic forecast scores, executed: matlab/epiekf_pipeline_mex.cpp compiled against
tests/mex_shim and driven by tests/mex_shim/lasso_driver.cpp (the gateway's generic driver).  The gateway's own argument checks
and the library's limits need no device (the host entry validates before it touches one); the test that
epiekf_pipeline_mex('escore', ...) with MATLAB-shaped arrays (chain first, ONE-based indices) returns what the restatement
tests/escore_ref.py computes, bit for bit and in the documented output order, runs on the GPU."""
import numpy as np
import pytest

from tests import escore_ref as S
from tests.test_lasso_mex import _gateway, lasso_driver  # noqa: F401  (the fixture builds the gateway and its driver)

E = np.zeros((0, 0))
ORDER = ("crps", "wis", "ae", "width", "rank", "ties", "cover", "count", "crps_mean", "wis_mean", "ae_mean", "n_scored", "cover_frac",
         "pit_hist")


def _args(**kw):
    d = dict(src=np.ones((10, 3, 2)), truth=np.ones((2, 3, 2)), D=5.0, alpha=np.array([[0.5, 0.05]]), n_bins=10.0, pop=E, ts=E, fd=E,
             kf=E, kl=E)
    d.update(kw)
    return ["escore"] + [d[k] for k in ("src", "truth", "D", "alpha", "n_bins", "pop", "ts", "fd", "kf", "kl")]


def test_escore_command_errors(lasso_driver):
    g = lambda a, msg: _gateway(lasso_driver, a, 1, expect_error=msg, tag="escore_e")
    g(_args()[:10], "11 inputs expected")
    g(_args(src=E), "src must be a double array")
    g(_args(D=3.0), "D must be an integer in 1 .. 4096")
    g(_args(alpha=np.full((1, 9), 0.5)), "at most 8 levels")
    g(_args(n_bins=33.0), "n_bins must be an integer in 0 .. 32")
    g(_args(n_bins=E), "n_bins must be a double scalar")
    g(_args(pop=np.ones((3, 1))), "population must have one entry per region")
    g(_args(truth=np.ones((2, 2, 2))), "truth must be Rt x rows' x T")
    g(_args(pop=np.ones((2, 1))), "truth must be Rt x rows' x T")                     # rows' = 4 with a population
    g(_args(truth=np.ones((3, 3, 2))), "one column per region")
    g(_args(ts=np.ones((3, 1))), "truth_series must have one entry per region")
    g(_args(ts=np.array([[1.0], [3.0]])), "ONE-based columns of truth")
    g(_args(ts=np.array([[0.0], [1.0]])), "ONE-based columns of truth")
    g(_args(fd=np.ones((1, 1))), "first_day must have one entry per region")
    g(_args(fd=np.array([[0.0], [1.0]])), "ONE-based days")
    g(_args(kf=0.0), "k_first, k_last must be integers")
    g(_args(kf=2.0, kl=0.0), "k_first, k_last must be integers")
    g(_args(kl=3.0), "k_first, k_last must be integers")
    # the library's limits, with its messages
    g(_args(alpha=np.array([[0.05, 0.5]])), "alpha must be strictly descending")
    g(_args(alpha=np.array([[1.0]])), "every alpha must lie in (0, 1)")


@pytest.mark.gpu
@pytest.mark.parametrize("with_pop", [True, False])
def test_escore_command_equals_restatement(gpu_device, lasso_driver, with_pop):
    R, D, T = 3, 129, 4
    rng = np.random.default_rng(129)
    src = np.abs(rng.standard_normal((T, 3, R * D)))
    src[0, 2, 5] = np.nan
    src[1, 0, D:2 * D] = np.nan
    pop = np.array([1e6, 2e6, 3e7]) if with_pop else None
    ro = 3 + int(with_pop)
    truth = np.abs(rng.standard_normal((T, ro, 2)))
    truth[:, 3:] *= 1e6
    truth[2, 1, 0] = np.nan
    ts, fd, alpha = [1, 0, 1], [0, 2, 1], (0.8, 0.5, 0.05)
    want = S.score(src, truth, R, D, alpha, 10, population=pop, truth_series=ts, first_day=fd, k0=1, k1=4)
    got = _gateway(lasso_driver, ["escore", np.transpose(src, (2, 1, 0)), np.transpose(truth, (2, 1, 0)), float(D),
                                  np.array(alpha).reshape(1, -1), 10.0, pop.reshape(-1, 1) if with_pop else E,
                                  np.array(ts, dtype=np.float64).reshape(-1, 1) + 1.0, np.array(fd, dtype=np.float64).reshape(-1, 1) + 1.0,
                                  2.0, 4.0], nlhs=14, tag=f"escore{int(with_pop)}")
    assert len(got) == 14
    for g, k in zip(got, ORDER):
        w = want[k].astype(np.float64)
        w = np.transpose(w, tuple(range(w.ndim))[::-1])
        assert S.same_bits(np.ascontiguousarray(np.asarray(g, dtype=np.float64)), np.ascontiguousarray(w)), k

"""The MATLAB boundary of the curve statistics, executed: matlab/epiekf_pipeline_mex.cpp compiled against tests/mex_shim and driven
by tests/mex_shim/lasso_driver.cpp (the gateway's generic driver).  The gateway's own argument checks and the library's limits
need no device (the host entry validates before it touches one); the test that epiekf_pipeline_mex('cdepth', ...) with
MATLAB-shaped arrays (path first, ONE-based days, ranks and draws) returns what the restatement tests/curve_depth_ref.py computes,
bit for bit and in the documented output order, runs on the GPU."""
import numpy as np
import pytest

from tests import curve_depth_ref as S
from tests.test_lasso_mex import _gateway, lasso_driver  # noqa: F401  (the fixture builds the gateway and its driver)

E = np.zeros((0, 0))
ORDER = ("depth", "mhi", "depth_rank", "median_path", "median_curve", "env_lo", "env_hi", "whisk_lo", "whisk_hi", "out_days", "n_outliers",
         "n_ranked", "band_count", "pair_total", "n_valid")
ONE_BASED = ("depth_rank", "median_path")


def _args(**kw):
    d = dict(src=np.ones((10, 3, 40)), D=5.0, alpha=E, ff=E, frac=E, pop=E, fd=E, kf=E, kl=E)
    d.update(kw)
    return ["cdepth"] + [d[k] for k in ("src", "D", "alpha", "ff", "frac", "pop", "fd", "kf", "kl")]


def test_cdepth_command_errors(lasso_driver):
    g = lambda a, msg: _gateway(lasso_driver, a, 1, expect_error=msg, tag="cdepth_e")
    g(_args()[:9], "10 inputs expected")
    g(_args(src=E), "src must be a double array")
    g(_args(D=3.0), "D must be a positive integer that divides")
    g(_args(pop=np.ones((3, 1))), "population must have one entry per region")
    g(_args(alpha=np.linspace(0.1, 0.9, 9).reshape(1, -1)), "at most 8 fractions")
    g(_args(fd=np.ones((1, 1))), "first_day must have one entry per region")
    g(_args(fd=np.array([[0.0], [1.0]])), "ONE-based days")
    g(_args(kf=0.0), "k_first, k_last must be integers")
    g(_args(kf=3.0, kl=2.0), "k_first, k_last must be integers")
    g(_args(kl=41.0), "k_first, k_last must be integers")
    # the library's limits, with its messages
    g(_args(src=np.ones((10, 2, 40)), pop=np.ones((2, 1))), "derive_newcases needs at least 3 rows")
    g(_args(alpha=np.array([[0.9, 0.5]])), "alpha must be strictly ascending")
    g(_args(alpha=np.array([[0.5, 1.5]])), "every alpha must lie in (0, 1]")
    g(_args(ff=-1.0), "fence_factor must be >= 0")
    g(_args(frac=0.0), "fence_frac must lie in (0, 1]")
    g(_args(src=np.ones((4097, 2)), D=4097.0), "D must lie in 1 .. 4096")


@pytest.mark.gpu
@pytest.mark.parametrize("with_pop", [True, False])
def test_cdepth_command_equals_restatement(gpu_device, lasso_driver, with_pop):
    kw = S.base_case(D=33, T=70, k0=2, k1=69, first_day=(0, 40), derive=with_pop, seed=6)
    opt = dict(alpha=(0.25, 0.5, 1.0), fence_factor=1.0, fence_frac=0.4) if with_pop else dict(alpha=(0.5, 0.9), fence_factor=1.5, fence_frac=0.5)
    want = S.statistics(**kw, **opt)
    fd = np.asarray(kw["first_day"], dtype=np.float64).reshape(-1, 1) + 1.0
    extra = [np.asarray(opt["alpha"]).reshape(1, -1), opt["fence_factor"], opt["fence_frac"]] if with_pop else [E, E, E]
    got = _gateway(lasso_driver, ["cdepth", np.transpose(kw["src"], (2, 1, 0)), 33.0] + extra +
                   [kw["population"].reshape(-1, 1) if with_pop else E, fd, 3.0, 69.0], nlhs=15, tag=f"cdepth{int(with_pop)}")
    assert len(got) == 15
    for g, k in zip(got, ORDER):
        w = want[k].astype(np.float64)
        w = w + 1.0 if k in ONE_BASED else w                             # (adding 0.0 would turn a -0.0 into +0.0)
        w = np.transpose(w, tuple(range(w.ndim))[::-1])
        assert S.same_bits(np.ascontiguousarray(np.asarray(g, dtype=np.float64)).reshape(w.shape), np.ascontiguousarray(w)), k

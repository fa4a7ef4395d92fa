"""The MATLAB boundary of the path functionals, executed: matlab/epiekf_pipeline_mex.cpp compiled against tests/mex_shim and driven by
tests/mex_shim/lasso_driver.cpp (the gateway's generic driver).  The gateway's own argument checks and the library's limits need
no device (the host entry validates before it touches one); the test that epiekf_pipeline_mex('pathfn', ...) with MATLAB-shaped
arrays (path first, ONE-based days) returns what the restatement tests/pathfn_ref.py computes, bit for bit and in the documented
output order, runs on the GPU."""
import numpy as np
import pytest

from tests import pathfn_ref as S
from tests.test_lasso_mex import _gateway, lasso_driver  # noqa: F401  (the fixture builds the gateway and its driver)

E = np.zeros((0, 0))
ONE_BASED = ("peak_day", "min_day", "first_cross")


def _args(**kw):
    d = dict(src=np.ones((10, 3, 40)), D=5.0, thr=np.ones((2, 3, 2)), pop=E, fd=E, kf=E, kl=E)
    d.update(kw)
    return ["pathfn"] + [d[k] for k in ("src", "D", "thr", "pop", "fd", "kf", "kl")]


def test_pathfn_command_errors(lasso_driver):
    g = lambda a, msg: _gateway(lasso_driver, a, 1, expect_error=msg, tag="pathfn_e")
    g(_args()[:7], "8 inputs expected")
    g(_args(src=E), "src must be a double array")
    g(_args(D=3.0), "D must be a positive integer that divides")
    g(_args(pop=np.ones((3, 1))), "population must have one entry per region")
    g(_args(thr=np.ones((3, 3, 2))), "thr must be R x rows' x n_thr")
    g(_args(thr=np.ones((2, 4, 2))), "thr must be R x rows' x n_thr")
    g(_args(pop=np.ones((2, 1))), "thr must be R x rows' x n_thr")                      # rows' = 4 with a population
    g(_args(thr=np.ones((2, 3, 9))), "at most 8 thresholds")
    g(_args(fd=np.ones((1, 1))), "first_day must have one entry per region")
    g(_args(fd=np.array([[0.0], [1.0]])), "ONE-based days")
    g(_args(kf=0.0), "k_first, k_last must be integers")
    g(_args(kf=3.0, kl=2.0), "k_first, k_last must be integers")
    g(_args(kl=41.0), "k_first, k_last must be integers")
    g(_args(src=np.ones((2, 1, 4100)), D=2.0, thr=E), "at most 4096 days")
    # the library's limits, with its messages
    g(_args(src=np.ones((10, 2, 40)), thr=E, pop=np.ones((2, 1))), "derive_newcases needs at least 3 rows")


@pytest.mark.gpu
@pytest.mark.parametrize("with_pop", [True, False])
def test_pathfn_command_equals_restatement(gpu_device, lasso_driver, with_pop):
    kw = S.base_case(D=33, T=70, k0=2, k1=69, first_day=(0, 40, 69), derive=with_pop, seed=6)
    want = S.functionals(**kw)
    fd = np.asarray(kw["first_day"], dtype=np.float64).reshape(-1, 1) + 1.0
    got = _gateway(lasso_driver, ["pathfn", np.transpose(kw["src"], (2, 1, 0)), 33.0, np.transpose(kw["thr"], (2, 1, 0)),
                                  kw["population"].reshape(-1, 1) if with_pop else E, fd, 3.0, 69.0], nlhs=13, tag=f"pathfn{int(with_pop)}")
    assert len(got) == 13
    for g, k in zip(got, S.NAMES):
        w = want[k].astype(np.float64)
        w = w + 1.0 if k in ONE_BASED else w                             # (adding 0.0 would turn a -0.0 into +0.0)
        w = np.transpose(w, tuple(range(w.ndim))[::-1])
        assert S.same_bits(np.ascontiguousarray(np.asarray(g, dtype=np.float64)).reshape(w.shape), np.ascontiguousarray(w)), k

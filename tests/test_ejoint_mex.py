"""The MATLAB boundary of the joint scores, executed: matlab/epiekf_pipeline_mex.cpp compiled against tests/mex_shim and driven by
tests/mex_shim/lasso_driver.cpp (the gateway's generic driver).  The gateway's own argument checks and the library's limits need
no device (the host entry validates before it touches one); the test that epiekf_pipeline_mex('jscore', ...) with MATLAB-shaped
arrays (chain first, ONE-based indices) returns what the restatement tests/ejoint_ref.py computes, bit for bit and in the
documented output order, runs on the GPU."""
import numpy as np
import pytest

from tests import ejoint_ref as J
from tests.test_lasso_mex import _gateway, lasso_driver  # noqa: F401  (the fixture builds the gateway and its driver)

E = np.zeros((0, 0))
ORDER = ("es", "vs", "truth_term", "spread_term", "n_members", "n_days", "member_dist")


def _args(**kw):
    d = dict(src=np.ones((10, 3, 2)), truth=np.ones((2, 3, 2)), D=5.0, vs_p=0.5, max_lag=E, pop=E, ts=E, fd=E, kf=E, kl=E)
    d.update(kw)
    return ["jscore"] + [d[k] for k in ("src", "truth", "D", "vs_p", "max_lag", "pop", "ts", "fd", "kf", "kl")]


def test_jscore_command_errors(lasso_driver):
    g = lambda a, msg: _gateway(lasso_driver, a, 1, expect_error=msg, tag="jscore_e")
    g(_args()[:10], "11 inputs expected")
    g(_args(src=E), "src must be a double array")
    g(_args(D=3.0), "D must be an integer in 1 .. 4096")
    g(_args(vs_p=2.0), "vs_p must be [] or 0 (no variogram score), 0.5 or 1")
    g(_args(max_lag=-1.0), "max_lag must be an integer >= 0")
    g(_args(max_lag=1.5), "max_lag must be an integer >= 0")
    g(_args(pop=np.ones((3, 1))), "population must have one entry per region")
    g(_args(truth=np.ones((2, 2, 2))), "truth must be Rt x rows' x T")
    g(_args(pop=np.ones((2, 1))), "truth must be Rt x rows' x T")                     # rows' = 4 with a population
    g(_args(truth=np.ones((3, 3, 2))), "one column per region")
    g(_args(ts=np.ones((3, 1))), "truth_series must have one entry per region")
    g(_args(ts=np.array([[1.0], [3.0]])), "ONE-based columns of truth")
    g(_args(fd=np.ones((1, 1))), "first_day must have one entry per region")
    g(_args(fd=np.array([[0.0], [1.0]])), "ONE-based days")
    g(_args(kf=0.0), "k_first, k_last must be integers")
    g(_args(kl=3.0), "k_first, k_last must be integers")


@pytest.mark.gpu
@pytest.mark.parametrize("vs_p", [0.5, 1.0, None])
def test_jscore_command_equals_restatement(gpu_device, lasso_driver, vs_p):
    c = J.case(130, 33, np.float64, 1)
    order = {0.5: 1, 1.0: 2, None: 0}[vs_p]
    want = J.joint(vs_order=order, max_lag=4, **c)
    got = _gateway(lasso_driver, ["jscore", np.transpose(c["src"], (2, 1, 0)), np.transpose(c["truth"], (2, 1, 0)), 130.0,
                                  E if vs_p is None else vs_p, 4.0, c["population"].reshape(-1, 1),
                                  c["truth_series"].astype(np.float64).reshape(-1, 1) + 1.0,
                                  c["first_day"].astype(np.float64).reshape(-1, 1) + 1.0, float(c["k0"] + 1), float(c["k1"])],
                   nlhs=7, tag=f"jscore{order}")
    assert len(got) == 7
    for g, k in zip(got, ORDER):
        w = want[k].astype(np.float64)
        assert J.same_bits(np.ascontiguousarray(np.asarray(g, dtype=np.float64)), np.ascontiguousarray(w.T)), k

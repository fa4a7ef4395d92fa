"""The MATLAB boundary of the support-vector regression, executed: matlab/epiekf_pipeline_mex.cpp compiled against
tests/mex_shim and driven by tests/mex_shim/lasso_driver.cpp (the gateway's generic driver).  The gateway's own argument
checks and the library's limits need no device (the host entry validates before it touches one); the test that
epiekf_pipeline_mex('svr', ...) with MATLAB-shaped arrays (region first) returns what hostapi.svr returns, bit for bit, in the
documented output order, runs on the GPU."""
import numpy as np
import pytest

from tests import svr_ref as SV
from tests.test_lasso_mex import _gateway, lasso_driver  # noqa: F401  (the fixture builds the gateway and its driver)

EMPTY = np.zeros((0, 0))


def _args(X, y, n_rows, kernel=0, box=1.0, eps=0.1, scale=1.0, tol=1e-3, max_iter=50000):
    reg = lambda v: np.asarray(v, dtype=np.float64).reshape(1, -1)
    return ["svr", np.ascontiguousarray(np.transpose(X, (2, 1, 0))), np.ascontiguousarray(y.T),
            EMPTY if n_rows is None else np.asarray(n_rows, dtype=np.float64).reshape(1, -1), float(kernel), reg(box), reg(eps), reg(scale),
            float(tol), float(max_iter)]


def test_svr_command_errors(lasso_driver):
    X, y = SV.plans(3, 12, 4, 3)
    g = lambda a, msg: _gateway(lasso_driver, a, 1, expect_error=msg, tag="svr_e")
    g(_args(X, y, (6, 12))[:9], "10 inputs expected")
    g(_args(X, y[:, :2], (6, 12)), "y must be")
    g(_args(X, y, (6, 12), box=(1.0, 2.0)), "box must be a scalar or R values")
    g(_args(X, y, (6, 12), scale=(1.0, 2.0)), "kernel_scale must be a scalar or R values")
    # the library's limits, with its messages
    g(_args(X, y, (0, 6)), "every n_rows must lie in")
    g(_args(X, y, (6,), kernel=2), "kernel must be")
    g(_args(X, y, (6,), tol=0.0), "tol must be finite")
    g(_args(X, y, (6,), max_iter=0), "max_iter must lie in")
    g(_args(np.ones((3, 97, 2)), np.ones((3, 2)), None), "F is limited to 96")
    g(_args(np.ones((401, 49, 1)), np.ones((401, 1)), None), "is limited to 20000")


@pytest.mark.gpu
@pytest.mark.parametrize("i, kernel, nlhs", [(1, "linear", 8), (1, "gaussian", 8), (2, "linear", 4), (0, "gaussian", 1)])
def test_svr_command_equals_hostapi(gpu_device, lasso_driver, i, kernel, nlhs):
    from epidemicmodeling_amd import hostapi
    p = SV.problem(i)
    want = hostapi.svr(p["X"], p["y"], **SV.run_kw(p, kernel))
    got = _gateway(lasso_driver, _args(p["X"], p["y"], p["n_rows"], SV.KERNELS.index(kernel), p["box"], p["epsilon"], p["kernel_scale"], SV.TOL,
                                       SV.MAX_ITER), nlhs=nlhs, tag=f"svr{i}{kernel[0]}")
    assert len(got) == nlhs
    for k, g in zip(SV.OUT_NAMES[:nlhs], got):
        if k == "w" and kernel == "gaussian":
            assert g.size == 0
            continue
        w = want[k].astype(np.float64)
        w = np.transpose(w, (2, 1, 0)) if w.ndim == 3 else w.T
        assert SV.same_bits(g, np.ascontiguousarray(w)), k

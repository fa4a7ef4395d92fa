"""The MATLAB boundary of the element-wise robust regression, executed: matlab/epiekf_pipeline_mex.cpp compiled against
tests/mex_shim and driven by tests/mex_shim/lasso_driver.cpp (the gateway's generic driver).  The gateway's own argument
checks and the library's limits need no device (the host entry validates before it touches one); the test that
epiekf_pipeline_mex('robustfit', ...) with MATLAB-shaped arrays (region first) returns what the restatement
tests/robust_fit_ref.py computes, bit for bit and in the documented output order, runs on the GPU."""
import numpy as np
import pytest

from tests import robust_fit_ref as RF
from tests.test_lasso_mex import _gateway, lasso_driver  # noqa: F401  (the fixture builds the gateway and its driver)


def _args(X, y, robust=1.0, lower=0.0, upper=np.inf, max_iter=50.0):
    return ["robustfit", np.ascontiguousarray(np.transpose(X, (2, 1, 0))), np.ascontiguousarray(y.T), robust, lower, upper, max_iter]


def test_robustfit_command_errors(lasso_driver):
    X, y = RF.make_case(3, 20, 2, 4)
    g = lambda a, msg: _gateway(lasso_driver, a, 1, expect_error=msg, tag="robfit_e")
    g(_args(X, y)[:6], "7 inputs expected")
    g(["robustfit", X[:, :, 0].T.copy(), y.T.copy(), 1.0, 0.0, np.inf, 50.0], "X must be R x n x D")
    g(["robustfit", np.ascontiguousarray(np.transpose(X, (2, 1, 0))), y.copy(), 1.0, 0.0, np.inf, 50.0], "y must be")
    # the library's limits, with its messages
    g(_args(X, y, robust=2.0), "robust must be 0 or 1")
    g(_args(X, y, lower=1.0, upper=0.5), "lower_a must not exceed upper_a")
    g(_args(X, y, max_iter=0.0), "max_iter must lie in")
    g(_args(X[:2], y[:2]), "D must be >= 3")


@pytest.mark.gpu
@pytest.mark.parametrize("D, n, R, robust, lower, max_iter, nlhs", [(60, 12, 7, 1, 0.0, 50, 7), (5, 2, 9, 1, 0.0, 3, 6), (130, 1, 3, 0, -np.inf, 50, 2)])
def test_robustfit_command_equals_restatement(gpu_device, lasso_driver, D, n, R, robust, lower, max_iter, nlhs):
    X, y = RF.make_case(D + n + R, D, n, R)
    RF.plant(X, y)
    want = RF.np_robust_fit(X, y, robust=robust, lower=lower, max_iter=max_iter)
    got = _gateway(lasso_driver, _args(X, y, float(robust), lower, np.inf, float(max_iter)), nlhs=nlhs, tag=f"robfit{D}_{n}")
    assert len(got) == nlhs
    order = ["a", "b", "b_item", "sigma", "iters", "status", "weights"][:nlhs]
    for k, g in zip(order, got):
        w = want[k]
        w = w.reshape(-1, 1) if k == "b" else np.transpose(w, (2, 1, 0)) if k == "weights" else w.T
        assert RF.same_bits(g, np.ascontiguousarray(w, dtype=np.float64)), k

"""The MATLAB boundary of the rectangular backslash, executed: matlab/epiekf_pipeline_mex.cpp compiled against tests/mex_shim
and driven by tests/mex_shim/lasso_driver.cpp (the gateway's generic driver).  The gateway's own argument checks and the
library's limits need no device (the host entry validates before it touches one); the test that
epiekf_pipeline_mex('mldivide', ...) with MATLAB-shaped arrays (region first) returns what hostapi.mldivide returns, bit for
bit, in the documented output order and with MATLAB's 1-based column numbers, runs on the GPU."""
import numpy as np
import pytest

from tests import mldivide_ref as ML
from tests.test_lasso_mex import _gateway, lasso_driver  # noqa: F401  (the fixture builds the gateway and its driver)

EMPTY = np.zeros((0, 0))


def _args(X, y, n_rows, tol_scale=1.0):
    return ["mldivide", np.ascontiguousarray(np.transpose(X, (2, 1, 0))), np.ascontiguousarray(y.T),
            EMPTY if n_rows is None else np.asarray(n_rows, dtype=np.float64).reshape(1, -1), float(tol_scale)]


def test_mldivide_command_errors(lasso_driver):
    X, y = ML.make_case(3, 12, 4, 2, 3)
    g = lambda a, msg: _gateway(lasso_driver, a, 1, expect_error=msg, tag="mldiv_e")
    g(_args(X, y, (6, 12))[:4], "5 inputs expected")
    g(_args(X, y[:, :2], (6, 12)), "y must be")
    g(_args(X, y[:5], (6, 12)), "y must be")
    # the library's limits, with its messages
    g(_args(X, y, (0, 6)), "every n_rows must lie in")
    g(_args(X, y, (13,)), "every n_rows must lie in")
    g(_args(X, y, (6,), tol_scale=-1.0), "tol_scale must be finite")
    g(_args(np.ones((3, 97, 2)), np.ones((3, 2)), None), "F is limited to 96")
    g(_args(np.ones((401, 49, 1)), np.ones((401, 1)), None), "is limited to 20000")


@pytest.mark.gpu
@pytest.mark.parametrize("i, nlhs", [(1, 7), (3, 7), (2, 3), (0, 1)])
def test_mldivide_command_equals_hostapi(gpu_device, lasso_driver, i, nlhs):
    from epidemicmodeling_amd import hostapi
    X, y, nr = ML.problem(i)
    want = hostapi.mldivide(X, y, n_rows=nr)
    got = _gateway(lasso_driver, _args(X, y, nr), nlhs=nlhs, tag=f"mldiv{i}")
    assert len(got) == nlhs
    for k, g in zip(ML.OUT_NAMES[:nlhs], got):
        w = want[k].astype(np.float64) + (1.0 if k == "perm" else 0.0)
        w = np.transpose(w, (2, 1, 0)) if w.ndim == 3 else w.T
        assert ML.same_bits(g, np.ascontiguousarray(w)), k
    if i == 0:                                               # [] for n_rows is all D rows
        assert ML.same_bits(_gateway(lasso_driver, _args(X, y, None), nlhs=1, tag="mldiv_d")[0], got[0])

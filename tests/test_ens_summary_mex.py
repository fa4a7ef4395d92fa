"""The MATLAB boundary of the ensemble statistics, executed: matlab/epiekf_pipeline_mex.cpp compiled against tests/mex_shim
and driven by tests/mex_shim/lasso_driver.cpp (the gateway's generic driver).  epiekf_pipeline_mex('ens_summary', src, D, q,
population) with MATLAB-shaped arrays (chain first) must return what hostapi.ensemble_summary returns, value for value, in
the documented output order."""
import os

import numpy as np
import pytest

from tests import ens_summary_ref as E
from tests.test_lasso_mex import _gateway, lasso_driver  # noqa: F401  (the fixture builds the gateway and its driver)

pytestmark = pytest.mark.gpu

Q = (0.0, 1.0, 0.5, 1.0 / 3.0, 0.975)


def _eq(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("with_pop", [True, False])
def test_ens_summary_command_equals_hostapi(gpu_device, lasso_driver, with_pop):
    from epidemicmodeling_amd import hostapi
    R, D, T = 3, 129, 2
    rng = np.random.default_rng(129)
    src = np.abs(rng.standard_normal((T, 3, R * D)))
    src[0, 2, 5] = np.nan
    src[1, 0, D:2 * D] = np.nan
    pop = np.array([1e6, 2e6, 3e7]) if with_pop else None
    want = hostapi.ensemble_summary(src, R, D, q=Q, population=pop)
    ref = E.summary(src, R, D, Q, population=pop)
    mx_pop = pop.reshape(-1, 1) if with_pop else np.zeros((0, 0))
    got = _gateway(lasso_driver, ["ens_summary", np.transpose(src, (2, 1, 0)), float(D), np.array(Q).reshape(1, -1), mx_pop],
                   nlhs=6, tag=f"ens{int(with_pop)}")
    assert len(got) == 6
    for g, k in zip(got, ("mean", "std", "min", "max", "quantiles", "count")):
        w = np.transpose(want[k], (3, 2, 1, 0) if k == "quantiles" else (2, 1, 0))
        assert _eq(g, w), k
        assert _eq(w, np.transpose(ref[k], (3, 2, 1, 0) if k == "quantiles" else (2, 1, 0))), k


def test_ens_summary_command_errors(gpu_device, lasso_driver):
    src = np.ones((10, 3, 2))
    _gateway(lasso_driver, ["ens_summary", src, 5.0, np.array([[0.5]])], 1, expect_error="5 inputs expected", tag="ens_e")
    _gateway(lasso_driver, ["ens_summary", src, 3.0, np.array([[0.5]]), np.zeros((0, 0))], 1, expect_error="D must be an integer", tag="ens_e")
    _gateway(lasso_driver, ["ens_summary", src, 5.0, np.array([[1.5]]), np.zeros((0, 0))], 1, expect_error="every q must be finite", tag="ens_e")
    _gateway(lasso_driver, ["ens_summary", src, 5.0, np.zeros((1, 17)), np.zeros((0, 0))], 1, expect_error="1 .. 16", tag="ens_e")
    _gateway(lasso_driver, ["ens_summary", src, 5.0, np.array([[0.5]]), np.ones((3, 1))], 1, expect_error="population must have", tag="ens_e")

"""The MATLAB boundary of the NPI-to-growth-rate predictor, executed: matlab/epiekf_pipeline_mex.cpp compiled against
tests/mex_shim and driven by tests/mex_shim/lasso_driver.cpp (the gateway's generic driver).  The gateway's own argument
checks and the library's limits need no device (the host entry validates before it touches one); the test that
epiekf_pipeline_mex('ratemap', ...) with MATLAB-shaped arrays (region first) returns what the restatement
tests/rate_map_ref.c computes, bit for bit and in the documented output order, runs on the GPU."""
import numpy as np
import pytest

from tests import rate_map_ref as RM
from tests.test_lasso_mex import _gateway, lasso_driver  # noqa: F401  (the fixture builds the gateway and its driver)

EMPTY = np.zeros((0, 0))


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return RM.RatemapRef(tmp_path_factory.mktemp("ratemap_ref_mex"))


def _m(a, axes):
    return EMPTY if a is None else np.ascontiguousarray(np.transpose(a, axes))


def _args(p, **kw):
    q = dict(p, **kw)
    return ["ratemap", _m(q["ip"], (2, 1, 0)), _m(q["y"], (1, 0)), _m(q["new_smoothed"], (1, 0)), _m(q["extra"], (2, 1, 0)),
            _m(q["lambda_in"], (2, 1, 0)), np.asarray(q["n_train"], dtype=np.float64).reshape(1, -1),
            np.asarray(q["lags"], dtype=np.float64).reshape(1, -1) if len(q["lags"]) else EMPTY,
            float(q["ridge"]), float(q["thr"]), float(q["red"]), float(q["effect_lag"])]


def test_ratemap_command_errors(lasso_driver):
    p = RM.make_case(3, 12, 2, (3,), 1, 2, 3, (6, 12))
    g = lambda a, msg: _gateway(lasso_driver, a, 1, expect_error=msg, tag="ratemap_e")
    g(_args(p)[:11], "12 inputs expected")
    g(_args(p, y=p["y"][:, :2]), "y must be")
    g(_args(p, new_smoothed=p["new_smoothed"][:5]), "new_smoothed must be")
    g(_args(p, extra=p["extra"][:5]), "extra must be R x E x T")
    g(_args(p, lambda_in=np.ones((3, 12, 3))), "lambda_in must be R x T x K")
    g(_args(p, lags=(1, 2, 3, 4)), "at most 3 lags")
    # the library's limits, with its messages
    g(_args(p, n_train=(0, 6)), "every n_train must lie in")
    g(_args(p, lags=(12,)), "every lag must lie in")
    g(_args(p, ridge=-1.0), "ridge must be finite")
    g(_args(p, y=None), "fit = 1 needs y")


@pytest.mark.gpu
@pytest.mark.parametrize("i, fit, nlhs", [(1, 1, 7), (4, 1, 4), (3, 0, 7), (0, 1, 2)])
def test_ratemap_command_equals_restatement(gpu_device, lasso_driver, ref, i, fit, nlhs):
    p = RM.problem(i, fit)
    want = ref.run(p, [k for k in RM.OUT_NAMES if fit or k != "map"])
    got = _gateway(lasso_driver, _args(p), nlhs=nlhs, tag=f"ratemap{i}_{fit}")
    assert len(got) == nlhs
    order = ["lambda_hat", "new_cases_est", "map", "status", "x_mx", "y_filled", "tracker"][:nlhs]
    for k, g in zip(order, got):
        if k == "map" and not fit:
            assert g.size == 0
            continue
        w = want[k]
        w = np.transpose(w, (2, 1, 0)) if w.ndim == 3 else w.T
        assert RM.same_bits(g, np.ascontiguousarray(w, dtype=np.float64)), k

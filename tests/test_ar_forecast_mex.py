"""The MATLAB boundary of the autoregressive alpha forecaster, executed: matlab/epiekf_pipeline_mex.cpp compiled against
tests/mex_shim and driven by tests/mex_shim/lasso_driver.cpp (the gateway's generic driver).  The gateway's own argument
checks and the library's limits need no device (the host entry validates before it touches one); the test that
epiekf_pipeline_mex('ar_forecast', ...) with MATLAB-shaped arrays (chain first, one-based series) returns what
hostapi.ar_forecast returns, bit for bit, runs on the GPU."""
import numpy as np
import pytest

from tests import ar_forecast_ref as AR
from tests.test_lasso_mex import _gateway, lasso_driver  # noqa: F401  (the fixture builds the gateway and its driver)

E = np.zeros((0, 0))


def _args(seg, prm, p, H, D, z=E, drive=E, series=E, A=E, nv=E, dt=1.0, nv_mode=0.0):
    return ["ar_forecast", seg, prm, float(dt), float(p), float(H), float(D), z, drive, series, A, nv, float(nv_mode)]


def test_ar_forecast_command_errors(lasso_driver):
    seg, prm = np.full((3, 20), 0.3), np.ones((3, 3))
    g = lambda a, msg: _gateway(lasso_driver, a, 1, expect_error=msg, tag="arfc_e")
    g(_args(seg, prm, 2, 5, 4)[:12], "13 inputs expected")
    g(_args(seg, np.ones((3, 2)), 2, 5, 4), "prm must be")
    g(_args(seg, prm, 2.5, 5, 4), "must be integers")
    a = _args(seg, prm, 2, 5, 4)
    g(a[:12] + [E], "nv_mode must be a double scalar")                   # a trailing [] for nv_mode
    g(a[:12] + [np.zeros((1, 2))], "nv_mode must be a double scalar")
    g(a[:3] + [E] + a[4:], "dt, p, H and D must be double scalars")
    g(_args(seg, prm, 2, 5, 4, z=np.zeros((11, 5))), "z must be")
    g(_args(seg, prm, 2, 5, 4, drive=np.zeros((2, 4))), "drive must be Sd x H")
    g(_args(seg, prm, 2, 5, 4, series=np.ones((12, 1))), "drive_series without drive")
    g(_args(seg, prm, 2, 5, 4, drive=np.zeros((2, 5)), series=np.full((12, 1), 3.0)), "drive_series value outside")
    g(_args(seg, prm, 2, 5, 4, A=np.zeros((3, 2))), "given together")
    # the library's limits, with its messages
    g(_args(seg, prm, 0, 5, 4), "p must lie in 1 .. 32")
    g(_args(np.full((3, 100), 0.3), prm, 33, 5, 4), "p must lie in 1 .. 32")
    g(_args(seg, prm, 20, 5, 4), "L must be at least p + 1")
    g(_args(np.full((3, 259), 0.3), prm, 2, 5, 4), "L - p is limited to 256")
    g(_args(seg, prm, 2, 0, 4), "H must be >= 1")
    g(_args(seg, prm, 2, 5, 4, nv_mode=3), "nv_mode must be 0 or 1")
    g(_args(seg, prm, 2, 5, 4, drive=np.zeros((2, 5))), "Sd == R * D")


@pytest.mark.gpu
@pytest.mark.parametrize("given", [False, True])
def test_ar_forecast_command_equals_hostapi(gpu_device, lasso_driver, given):
    from epidemicmodeling_amd import hostapi
    R, D, L, p, H = 3, 70, 40, 4, 6
    rng = np.random.default_rng(40)
    seg = np.stack([AR.ar_series([-1.2, 0.5], L, 40 + r, noise=0.05, offset=0.3) for r in range(R)], axis=1)
    seg[:, 1] = 0.25                                      # a rank-deficient region when the model is fitted
    prm = np.stack([rng.uniform(0.1, 0.3, R), np.full(R, 0.99), np.full(R, 0.01)], axis=1)          # R x 3
    z, drive = rng.standard_normal((H, R * D)), rng.uniform(-0.1, 0.1, (H, 2))
    ser = rng.integers(0, 2, R * D)
    A = nv = None
    if given:
        A, nv = np.stack([[-1.1, 0.4, 0.05, 0.0]] * R, axis=1), np.full(R, 1e-3)
    want = hostapi.ar_forecast(seg, prm[:, 0], prm[:, 1], prm[:, 2], 0.5, p, H, D, z=z, drive=drive, drive_series=ser, A=A,
                               noise_var=nv, nv_mode=1)
    got = _gateway(lasso_driver, _args(seg.T, prm, p, H, D, z=z.T, drive=drive.T, series=(ser + 1.0).reshape(-1, 1),
                                       A=E if A is None else A.T, nv=E if nv is None else nv.reshape(-1, 1), dt=0.5, nv_mode=1),
                   nlhs=4, tag=f"arfc{int(given)}")
    assert len(got) == 4
    assert AR.same(got[0], np.transpose(want["S"], (2, 1, 0))) and AR.same(got[1], want["A"].T)
    assert AR.same(got[2].ravel(), want["noise_var"]) and np.array_equal(got[3].ravel(), want["status"])
    assert want["status"].tolist() == ([0, 0, 0] if given else [0, 1, 0])

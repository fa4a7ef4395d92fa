"""The MATLAB boundary of the cross-validated LASSO, executed: matlab/epiekf_pipeline_mex.cpp is compiled against
tests/mex_shim/mex.h (the implemented stand-in for the MEX / C Matrix API), linked with libepiekf.so and driven by
tests/mex_shim/lasso_driver.cpp.  epiekf_pipeline_mex('lasso', X, y, K, fold) with MATLAB-shaped arrays (region first,
1-based folds) must return what hostapi.lasso_cv returns, bit for bit, in the documented output order."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests.test_lasso_host import make_problem
from tests.test_mex_boundary import _read, _write

pytestmark = pytest.mark.gpu

SHIM = os.path.join(H.ROOT, "tests", "mex_shim")
BUILD = os.path.join(SHIM, "build", "lasso")


@pytest.fixture(scope="module")
def lasso_driver(hip_lib):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.fail("no g++: the gateway cannot be compiled")
    os.makedirs(BUILD, exist_ok=True)
    libdir = os.path.join(H.ROOT, "epidemicmodeling_amd")
    common = [cxx, "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + SHIM, "-I" + os.path.join(H.ROOT, "include")]
    obj = os.path.join(BUILD, "pipeline.o")
    subprocess.run(common + ["-DmexFunction=mex_pipeline", "-c", os.path.join(H.ROOT, "matlab", "epiekf_pipeline_mex.cpp"),
                             "-o", obj], check=True)
    exe = os.path.join(BUILD, "lasso_driver")
    subprocess.run(common + [os.path.join(SHIM, "lasso_driver.cpp"), os.path.join(SHIM, "mex_shim.cpp"), obj, "-L" + libdir,
                             "-lepiekf", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64",
                             "-o", exe], check=True)
    return exe


def _gateway(exe, args, nlhs, expect_error=None, tag="lasso"):
    fin, fout = os.path.join(BUILD, tag + "_in.bin"), os.path.join(BUILD, tag + "_out.bin")
    _write(fin, args)
    r = subprocess.run([exe, fin, fout, str(nlhs)], capture_output=True, text=True, timeout=300, stdin=subprocess.DEVNULL)
    if expect_error is not None:
        assert r.returncode == 3 and expect_error in r.stderr, (r.returncode, r.stderr[-400:])
        return None
    assert r.returncode == 0, r.stderr[-2000:]
    return _read(fout)


def _bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64))


@pytest.mark.parametrize("R, D, n, K", [(7, 60, 12, 50), (3, 30, 5, 10), (2, 20, 1, 0)])
def test_lasso_command_equals_hostapi(gpu_device, lasso_driver, R, D, n, K):
    from epidemicmodeling_amd import hostapi
    X, y, fold = make_problem(R, D, n, K, seed=R + D + K)
    want = hostapi.lasso_cv(X, y, K=K, folds=fold)
    mx_fold = (fold.T + 1).astype(np.float64) if K >= 2 else np.zeros((0, 0))
    got = _gateway(lasso_driver, ["lasso", np.transpose(X, (2, 1, 0)), y.T, float(K), mx_fold], nlhs=10, tag=f"l{R}_{K}")
    a, b, lam, mse, se, idx, idx1, B, icpt, df = got
    assert _bits(lam, want["lambda"].T) and _bits(B, np.transpose(want["B"], (2, 1, 0))) and _bits(icpt, want["intercept"].T)
    assert np.array_equal(df, want["df"].T.astype(np.float64))
    if K >= 2:
        assert _bits(a, want["a"].T) and _bits(b, want["b"].reshape(-1, 1))
        assert _bits(mse, want["mse"].T) and _bits(se, want["se"].T)
        assert np.array_equal(idx.ravel(), np.where(want["idx_min_mse"] >= 0, want["idx_min_mse"] + 1, 0))
        assert np.array_equal(idx1.ravel(), np.where(want["idx_1se"] >= 0, want["idx_1se"] + 1, 0))
    else:
        assert np.isnan(a).all() and np.isnan(mse).all() and (idx == 0).all()


def test_lasso_command_errors(gpu_device, lasso_driver):
    X, y, fold = make_problem(2, 20, 3, 4, seed=1, specials=False)
    args = lambda **kw: ["lasso", kw.get("X", np.transpose(X, (2, 1, 0))), kw.get("y", y.T), kw.get("K", 4.0),
                         kw.get("fold", (fold.T + 1).astype(np.float64))]
    _gateway(lasso_driver, args()[:4], 1, expect_error="5 inputs expected")
    _gateway(lasso_driver, args(y=y), 1, expect_error="y must be")
    _gateway(lasso_driver, args(fold=fold.astype(np.float64)), 1, expect_error="fold must be")
    _gateway(lasso_driver, args(fold=np.zeros_like(fold.T, dtype=np.float64)), 1, expect_error="fold value outside")
    _gateway(lasso_driver, args(K=1.0), 1, expect_error="K must be 0")

"""epi_robfit_validate and the argument checks of epi_robfit_run_host, through the C ABI (no GPU needed: every case is
rejected before a device is touched), and the new symbols in the header, in _lib.ABI_SYMBOLS and in the library."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import helpers as H

D_, N_, R_ = 20, 3, 4


def _call(fn="validate", **kw):
    from epidemicmodeling_amd import _lib
    args = dict(R=R_, D=D_, n=N_, robust=1, max_iter=50, lower_a=0.0, upper_a=float("inf"))
    args.update({k: v for k, v in kw.items() if k in args})
    d = _lib.make_robfit_desc(**args)
    if "abi_version" in kw:
        d.abi_version = kw["abi_version"]
    X, y = np.ones((D_, N_, R_)), np.ones((D_, R_))
    outs = _lib.RobfitOutputs()
    bufs = {k: np.empty(sh, dtype=np.int32 if k in _lib.ROBFIT_OUT_I32 else np.float64) for k, sh in _lib.robfit_shapes(R_, D_, N_).items()}
    for k, v in bufs.items():
        setattr(outs, k, v.ctypes.data)
    for k in kw.get("null_outs", ()):
        setattr(outs, k, None)
    err = C.create_string_buffer(256)
    xp = None if kw.get("null_x") else X.ctypes.data
    yp = None if kw.get("null_y") else y.ctypes.data
    op = None if kw.get("null_out") else C.byref(outs)
    dp = None if kw.get("null_desc") else C.byref(d)
    lib = _lib.lib()
    if fn == "validate":
        rc = lib.epi_robfit_validate(dp, xp, yp, op, err)
    else:
        rc = lib.epi_robfit_run_host(dp, xp, yp, op, 0, err)
    return rc, err.value.decode()


ALL = ("a", "b_item", "sigma", "iters", "status", "weights", "b")
BAD = [
    (dict(null_desc=True), -5, "NULL descriptor"),
    (dict(abi_version=5), -5, "ABI"),
    (dict(R=0), -5, "R must be"),
    (dict(D=2), -5, "D must be >= 3"),
    (dict(n=0), -5, "n must be"),
    (dict(robust=2), -5, "robust must be 0 or 1"),
    (dict(robust=-1), -5, "robust must be 0 or 1"),
    (dict(max_iter=0), -5, "max_iter must lie in"),
    (dict(max_iter=100001), -5, "max_iter must lie in"),
    (dict(lower_a=float("nan")), -5, "must not be NaN"),
    (dict(upper_a=float("nan")), -5, "must not be NaN"),
    (dict(lower_a=1.0, upper_a=0.5), -5, "lower_a must not exceed upper_a"),
    (dict(R=2 ** 20, D=1024, n=2), -5, "R * D * n is limited"),
    (dict(null_x=True), -5, "NULL X"),
    (dict(null_y=True), -5, "NULL X"),
    (dict(null_out=True), -5, "NULL X"),
    (dict(null_outs=ALL), -5, "every output is NULL"),
    (dict(n=13), -8, "n is limited to 12"),
    (dict(D=1025), -8, "D is limited to 1024"),
    (dict(R=(2 ** 31 - 1) // 3 + 1, D=3, n=1), -5, "R * D * n is limited to 2^31 - 1"),        # 2^31 + 1
]


@pytest.mark.parametrize("kw, rc, msg", BAD)
def test_validate_rejects(hip_lib, kw, rc, msg):
    got, text = _call("validate", **kw)
    assert got == rc and msg in text, (got, text)
    got, text = _call("run_host", **kw)                     # the host entry validates first, before any device work
    assert got == rc and msg in text, (got, text)


def test_validate_accepts(hip_lib):
    assert _call("validate") == (0, "")
    assert _call("validate", D=3, n=12, max_iter=100000, lower_a=-float("inf"))[0] == 0
    assert _call("validate", D=1024, n=1, max_iter=1, robust=0, lower_a=0.25, upper_a=0.25)[0] == 0
    # the largest product D >= 3 allows (2^31 - 1 is prime): 2^31 - 2, through the descriptor alone (X would be 16 GiB)
    assert _call("validate", R=(2 ** 31 - 1) // 3, D=3, n=1)[0] == 0
    assert _call("validate", R=(2 ** 31 - 2) // (6 * 331), D=331, n=6)[0] == 0 and (2 ** 31 - 2) % (6 * 331) == 0
    for k in ALL:                                            # every output alone is enough
        assert _call("validate", null_outs=tuple(o for o in ALL if o != k))[0] == 0


def test_symbols_header_and_structs(hip_lib):
    from epidemicmodeling_amd import _lib
    header = open(os.path.join(H.ROOT, "include", "epiekf.h")).read()
    for sym in ("epi_robfit_validate", "epi_robfit_run_device", "epi_robfit_run_host"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(hip_lib, sym) and f"int {sym}(" in header, sym
    for name in ("epi_robfit_desc", "epi_robfit_outputs"):
        assert f"}} {name};" in header
    assert "#define EPIEKF_ABI_VERSION 6" in header and hip_lib.epi_abi_version() == 6
    assert C.sizeof(_lib.RobfitDesc) == 6 * 4 + 2 * 8
    assert [n for n, _ in _lib.RobfitDesc._fields_] == ["abi_version", "R", "D", "n", "robust", "max_iter", "lower_a", "upper_a"]
    assert C.sizeof(_lib.RobfitOutputs) == 7 * C.sizeof(C.c_void_p)
    for name, bit in _lib.ROBFIT_STATUS_BITS.items():
        assert f"EPI_ROBFIT_{name.upper()} = {bit}" in header


def test_python_entry_points_check_their_arguments(hip_lib):
    from epidemicmodeling_amd import batch, hostapi, pipeline
    X, y = np.ones((D_, N_, R_)), np.ones((D_, R_))
    with pytest.raises(ValueError, match="unknown outputs"):
        hostapi.robust_affine_fit(X, y, outputs=("a", "slope"))
    with pytest.raises(ValueError, match="no output"):
        hostapi.robust_affine_fit(X, y, outputs=())
    with pytest.raises(ValueError, match="X must be"):
        hostapi.robust_affine_fit(X, y[:-1])
    with pytest.raises(ValueError, match="X must be"):
        batch.robust_affine_fit(X, y[:, :-1], device="cpu")
    from epidemicmodeling_amd._lib import EpiError
    with pytest.raises(EpiError, match="lower_a must not exceed"):
        hostapi.robust_affine_fit(X, y, lower=1.0, upper=0.0)
    assert pipeline.REGRESSIONS == ("nonnegls", "lasso", "elementwise")

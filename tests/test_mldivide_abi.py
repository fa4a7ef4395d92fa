"""epi_mldiv_validate and the argument checks of epi_mldiv_run_host, through the C ABI (no GPU needed: every case is rejected
before a device is touched), and the new symbols in the header, in _lib.ABI_SYMBOLS and in the library."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import helpers as H

D_, F_, R_, K_ = 20, 5, 4, 2
ALL = ("m", "rank", "perm", "rdiag", "resid", "fitted", "status")


def _call(fn="validate", **kw):
    from epidemicmodeling_amd import _lib
    args = dict(D=D_, F=F_, R=R_, K=K_, tol_scale=1.0)
    args.update({k: v for k, v in kw.items() if k in args})
    d = _lib.make_mldiv_desc(**args)
    if "abi_version" in kw:
        d.abi_version = kw["abi_version"]
    one = np.ones(8)                                        # validate reads n_rows alone; the other arrays only have to exist
    nr = np.ascontiguousarray(kw.get("n_rows", (5, 20)), dtype=np.int32)
    ins = _lib.MldivInputs()
    for k in _lib.MLDIV_IN_NAMES:
        setattr(ins, k, nr.ctypes.data if k == "n_rows" else one.ctypes.data)
    for k in kw.get("null_ins", ()):
        setattr(ins, k, None)
    outs = _lib.MldivOutputs()
    for k in ALL:
        setattr(outs, k, one.ctypes.data)
    for k in kw.get("null_outs", ()):
        setattr(outs, k, None)
    err = C.create_string_buffer(256)
    ip = None if kw.get("null_in") else C.byref(ins)
    op = None if kw.get("null_out") else C.byref(outs)
    dp = None if kw.get("null_desc") else C.byref(d)
    lib = _lib.lib()
    rc = lib.epi_mldiv_validate(dp, ip, op, err) if fn == "validate" else lib.epi_mldiv_run_host(dp, ip, op, 0, err)
    return rc, err.value.decode()


BAD = [
    (dict(null_desc=True), -5, "NULL descriptor"),
    (dict(abi_version=5), -5, "ABI"),
    (dict(D=0), -5, "D must be"),
    (dict(F=0), -5, "F must be"),
    (dict(R=0), -5, "R must be"),
    (dict(K=0), -5, "K must be"),
    (dict(tol_scale=-1.0), -5, "tol_scale must be finite"),
    (dict(tol_scale=float("nan")), -5, "tol_scale must be finite"),
    (dict(tol_scale=float("inf")), -5, "tol_scale must be finite"),
    (dict(F=97), -8, "F is limited to 96"),
    (dict(D=207, F=96, K=1, n_rows=(207,)), -8, "is limited to 20000"),           # 207 x 97 = 20 079
    (dict(D=401, F=49, n_rows=(5, 401)), -8, "is limited to 20000"),              # 401 x 50 = 20 050
    (dict(D=10001, F=1, K=1, n_rows=(10001,)), -8, "is limited to 20000"),
    (dict(K=2 ** 16, R=2 ** 15, n_rows=(1,) * 2 ** 16), -5, "K * R must stay below"),
    (dict(D=2 ** 20, F=2, R=2 ** 10), -5, "element count"),
    (dict(D=2 ** 11, K=2 ** 10, R=2 ** 10, n_rows=(1,) * 2 ** 10), -5, "element count"),
    (dict(F=64, K=2 ** 15, R=2 ** 10, n_rows=(1,) * 2 ** 15), -5, "element count"),
    (dict(null_in=True), -5, "NULL inputs"),
    (dict(null_out=True), -5, "NULL inputs"),
    (dict(null_ins=("X",)), -5, "NULL X"),
    (dict(null_ins=("y",)), -5, "NULL X"),
    (dict(null_ins=("n_rows",)), -5, "NULL X"),
    (dict(null_outs=ALL), -5, "every output is NULL"),
    (dict(n_rows=(0, 5)), -5, "every n_rows must lie in"),
    (dict(n_rows=(5, 21)), -5, "every n_rows must lie in"),
]


@pytest.mark.parametrize("kw, rc, msg", BAD)
def test_validate_rejects(hip_lib, kw, rc, msg):
    got, text = _call("validate", **kw)
    assert got == rc and msg in text, (got, text)
    got, text = _call("run_host", **kw)                     # the host entry validates first, before any device work
    assert got == rc and msg in text, (got, text)


def test_validate_accepts(hip_lib):
    assert _call("validate") == (0, "")
    assert _call("validate", F=96, D=206, K=1, n_rows=(206,))[0] == 0           # both limits at their exact values
    assert _call("validate", F=49, D=400, n_rows=(1, 400))[0] == 0
    assert _call("validate", F=1, D=10000, K=1, n_rows=(10000,))[0] == 0
    assert _call("validate", F=96, D=500, n_rows=(206, 1))[0] == 0              # the limit is on the rows used, not on D
    assert _call("validate", D=1, F=1, R=1, K=1, n_rows=(1,), tol_scale=0.0)[0] == 0
    for k in ALL:                                            # every output alone is enough
        assert _call("validate", null_outs=tuple(o for o in ALL if o != k))[0] == 0


def test_symbols_header_and_structs(hip_lib):
    from epidemicmodeling_amd import _build, _lib
    header = open(os.path.join(H.ROOT, "include", "epiekf.h")).read()
    for sym in ("epi_mldiv_validate", "epi_mldiv_run_device", "epi_mldiv_run_host"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(hip_lib, sym) and f"int {sym}(" in header, sym
    for name in ("epi_mldiv_desc", "epi_mldiv_inputs", "epi_mldiv_outputs"):
        assert f"}} {name};" in header
    assert "#define EPIEKF_ABI_VERSION 6" in header and hip_lib.epi_abi_version() == 6
    assert C.sizeof(_lib.MldivDesc) == 5 * 4 + 4 + 8                     # five int32, padding, one double
    assert _lib.MldivDesc.tol_scale.offset == 24
    assert [n for n, _ in _lib.MldivDesc._fields_] == ["abi_version", "D", "F", "R", "K", "tol_scale"]
    assert [n for n, _ in _lib.MldivInputs._fields_] == ["X", "y", "n_rows"]
    assert [n for n, _ in _lib.MldivOutputs._fields_] == list(ALL)
    body = header[header.index("typedef struct epi_mldiv_desc"):header.index("int epi_mldiv_validate(")]
    order = [body.index(f) for f in ("abi_version;", " D;", " F;", " R;", " K;", " tol_scale;", "*X;", "*y;", "*n_rows;", "*m;", "*rank;",
                                     "*perm;", "*rdiag;", "*resid;", "*fitted;", "*status;")]
    assert order == sorted(order)
    for name, bit in _lib.MLDIV_STATUS_BITS.items():
        assert f"EPI_MLDIV_{name.upper()} = {bit}" in header
    assert any(d.endswith("mldivide.hpp") for d in _build.DEPS)
    assert C.sizeof(_lib.RatemapDesc) == 12 * 4 + 3 * 8                  # the rate map's descriptor is as it was


def test_python_entry_points_check_their_arguments(hip_lib):
    from epidemicmodeling_amd import batch, hostapi, pipeline
    from epidemicmodeling_amd._lib import EpiError
    X, y = np.ones((D_, F_, R_)), np.ones((D_, R_))
    with pytest.raises(ValueError, match="unknown outputs"):
        hostapi.mldivide(X, y, outputs=("m", "slope"))
    with pytest.raises(ValueError, match="no output"):
        hostapi.mldivide(X, y, outputs=())
    with pytest.raises(ValueError, match="X must be"):
        hostapi.mldivide(X, y[:-1])
    with pytest.raises(ValueError, match="X must be"):
        hostapi.mldivide(X[:, :, 0], y)
    with pytest.raises(ValueError, match="X must be"):
        batch.mldivide(X, y[:, :-1], device="cpu")
    with pytest.raises(ValueError, match="unknown outputs"):
        batch.mldivide(X, y, outputs=("map",), device="cpu")
    with pytest.raises(EpiError, match="every n_rows must lie in"):
        hostapi.mldivide(X, y, n_rows=[0])
    with pytest.raises(EpiError, match="every n_rows must lie in"):
        hostapi.mldivide(X, y, n_rows=[D_ + 1])
    with pytest.raises(EpiError, match="tol_scale must be finite"):
        hostapi.mldivide(X, y, tol_scale=-1.0)
    with pytest.raises(EpiError, match="F is limited to 96"):
        hostapi.mldivide(np.ones((2, 97, 1)), np.ones((2, 1)))
    with pytest.raises(ValueError, match="solver must be"):
        pipeline.growth_forecast(np.ones((D_, R_)), np.ones(R_), np.ones((D_, 3, R_)), predict_ahead=5, solver="nope")

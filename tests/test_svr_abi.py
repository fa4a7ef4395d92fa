"""epi_svr_validate and the argument checks of epi_svr_run_host, through the C ABI (no GPU needed: every case is rejected
before a device is touched), and the new symbols in the header, in _lib.ABI_SYMBOLS and in the library."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import helpers as H

D_, F_, R_, K_ = 20, 5, 4, 2
ALL = ("beta", "bias", "w", "fitted", "n_iter", "gap", "n_sv", "status")


def _call(fn="validate", **kw):
    from epidemicmodeling_amd import _lib
    args = dict(D=D_, F=F_, R=R_, K=K_, kernel="linear", tol=1e-3, max_iter=1000)
    args.update({k: v for k, v in kw.items() if k in args})
    d = _lib.make_svr_desc(**args)
    for k in ("abi_version", "kernel_code"):
        if k in kw:
            setattr(d, k.replace("_code", ""), kw[k])
    one = np.ones(8)                                        # validate reads n_rows alone; the other arrays only have to exist
    nr = np.ascontiguousarray(kw.get("n_rows", (5, 20)), dtype=np.int32)
    ins = _lib.SvrInputs()
    for k in _lib.SVR_IN_NAMES:
        setattr(ins, k, nr.ctypes.data if k == "n_rows" else one.ctypes.data)
    for k in kw.get("null_ins", ()):
        setattr(ins, k, None)
    outs = _lib.SvrOutputs()
    for k in ALL:
        setattr(outs, k, one.ctypes.data if k != "w" or args["kernel"] == "linear" else None)
    for k in kw.get("set_outs", ()):
        setattr(outs, k, one.ctypes.data)
    for k in kw.get("null_outs", ()):
        setattr(outs, k, None)
    err = C.create_string_buffer(256)
    ip = None if kw.get("null_in") else C.byref(ins)
    op = None if kw.get("null_out") else C.byref(outs)
    dp = None if kw.get("null_desc") else C.byref(d)
    lib = _lib.lib()
    rc = lib.epi_svr_validate(dp, ip, op, err) if fn == "validate" else lib.epi_svr_run_host(dp, ip, op, 0, err)
    return rc, err.value.decode()


BAD = [
    (dict(null_desc=True), -5, "NULL descriptor"),
    (dict(abi_version=5), -5, "ABI"),
    (dict(D=0), -5, "D must be"),
    (dict(F=0), -5, "F must be"),
    (dict(R=0), -5, "R must be"),
    (dict(K=0), -5, "K must be"),
    (dict(kernel_code=2), -5, "kernel must be"),
    (dict(kernel_code=-1), -5, "kernel must be"),
    (dict(max_iter=0), -5, "max_iter must lie in"),
    (dict(max_iter=10000001), -5, "max_iter must lie in"),
    (dict(tol=0.0), -5, "tol must be finite"),
    (dict(tol=-1.0), -5, "tol must be finite"),
    (dict(tol=float("nan")), -5, "tol must be finite"),
    (dict(tol=float("inf")), -5, "tol must be finite"),
    (dict(F=97), -8, "F is limited to 96"),
    (dict(D=207, F=96, K=1, n_rows=(207,)), -8, "is limited to 20000"),           # 207 x 98 = 20 286
    (dict(D=401, F=49, n_rows=(5, 401)), -8, "is limited to 20000"),              # 401 x 50 = 20 050
    (dict(D=385, F=50, K=1, n_rows=(385,)), -8, "is limited to 20000"),           # an even F is padded: 385 x 52 = 20 020
    (dict(D=1025, F=3, K=1, n_rows=(1025,)), -8, "n_rows is limited to 1024"),
    (dict(K=2 ** 16, R=2 ** 15, n_rows=(1,) * 2 ** 16), -5, "K * R must stay below"),
    (dict(D=2 ** 20, F=2, R=2 ** 10), -5, "element count"),
    (dict(D=2 ** 11, K=2 ** 10, R=2 ** 10, n_rows=(1,) * 2 ** 10), -5, "element count"),
    (dict(F=64, K=2 ** 15, R=2 ** 10, n_rows=(1,) * 2 ** 15), -5, "element count"),
    (dict(null_in=True), -5, "NULL inputs"),
    (dict(null_out=True), -5, "NULL inputs"),
    (dict(null_ins=("X",)), -5, "NULL X"),
    (dict(null_ins=("y",)), -5, "NULL X"),
    (dict(null_ins=("n_rows",)), -5, "NULL X"),
    (dict(null_ins=("box",)), -5, "NULL box"),
    (dict(null_ins=("epsilon",)), -5, "NULL box"),
    (dict(null_ins=("kernel_scale",)), -5, "NULL box"),
    (dict(null_outs=ALL), -5, "every output is NULL"),
    (dict(kernel="gaussian", set_outs=("w",)), -5, "w exists for the linear kernel only"),
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
    assert _call("validate", kernel="gaussian") == (0, "")
    assert _call("validate", F=96, D=204, K=1, n_rows=(204,))[0] == 0           # 204 x 98 = 19 992
    assert _call("validate", F=49, D=400, n_rows=(1, 400))[0] == 0              # 400 x 50 = 20 000
    assert _call("validate", F=50, D=384, K=1, n_rows=(384,))[0] == 0           # 384 x 52 = 19 968
    assert _call("validate", F=3, D=1024, K=1, n_rows=(1024,))[0] == 0
    assert _call("validate", F=96, D=5000, n_rows=(204, 1))[0] == 0             # the limits are on the rows used, not on D
    assert _call("validate", D=1, F=1, R=1, K=1, n_rows=(1,), max_iter=1, tol=1e-300)[0] == 0
    assert _call("validate", max_iter=10000000)[0] == 0
    for k in ALL:                                            # every output alone is enough
        assert _call("validate", null_outs=tuple(o for o in ALL if o != k))[0] == 0


def test_symbols_header_and_structs(hip_lib):
    from epidemicmodeling_amd import _build, _lib
    header = open(os.path.join(H.ROOT, "include", "epiekf.h")).read()
    for sym in ("epi_svr_validate", "epi_svr_run_device", "epi_svr_run_host"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(hip_lib, sym) and f"int {sym}(" in header, sym
    for name in ("epi_svr_desc", "epi_svr_inputs", "epi_svr_outputs"):
        assert f"}} {name};" in header
    assert "#define EPIEKF_ABI_VERSION 6" in header and hip_lib.epi_abi_version() == 6
    assert C.sizeof(_lib.SvrDesc) == 7 * 4 + 4 + 8                      # seven int32, padding, one double
    assert _lib.SvrDesc.tol.offset == 32
    assert [n for n, _ in _lib.SvrDesc._fields_] == ["abi_version", "D", "F", "R", "K", "kernel", "max_iter", "tol"]
    assert [n for n, _ in _lib.SvrInputs._fields_] == ["X", "y", "n_rows", "box", "epsilon", "kernel_scale"]
    assert [n for n, _ in _lib.SvrOutputs._fields_] == list(ALL)
    body = header[header.index("typedef struct epi_svr_desc"):header.index("int epi_svr_validate(")]
    order = [body.index(f) for f in ("abi_version;", " D;", " F;", " R;", " K;", " kernel;", " max_iter;", " tol;", "*X;", "*y;", "*n_rows;",
                                     "*box;", "*epsilon;", "*kernel_scale;", "*beta;", "*bias;", "*w;", "*fitted;", "*n_iter;", "*gap;",
                                     "*n_sv;", "*status;")]
    assert order == sorted(order)
    for name, bit in _lib.SVR_STATUS_BITS.items():
        assert f"EPI_SVR_{name.upper()} = {bit}" in header
    assert "EPI_SVR_LINEAR = 0, EPI_SVR_GAUSSIAN = 1" in header and _lib.SVR_KERNELS == {"linear": 0, "gaussian": 1}
    assert any(d.endswith("svr.hpp") for d in _build.DEPS)
    assert C.sizeof(_lib.MldivDesc) == 5 * 4 + 4 + 8                    # the backslash's descriptor is as it was


def test_python_entry_points_check_their_arguments(hip_lib):
    from epidemicmodeling_amd import batch, hostapi, pipeline
    from epidemicmodeling_amd._lib import EpiError
    X, y = np.ones((D_, F_, R_)), np.ones((D_, R_))
    kw = dict(box=1.0, epsilon=0.1, kernel_scale=1.0)
    with pytest.raises(ValueError, match="unknown outputs"):
        hostapi.svr(X, y, outputs=("beta", "slope"), **kw)
    with pytest.raises(ValueError, match="no output"):
        hostapi.svr(X, y, outputs=(), **kw)
    with pytest.raises(ValueError, match="X must be"):
        hostapi.svr(X, y[:-1], **kw)
    with pytest.raises(ValueError, match="X must be"):
        batch.svr(X, y[:, :-1], device="cpu", **kw)
    with pytest.raises(ValueError, match="kernel must be"):
        hostapi.svr(X, y, kernel="rbf", **kw)
    with pytest.raises(ValueError, match="box must be a scalar or an array"):
        hostapi.svr(X, y, box=np.ones(R_ + 1), epsilon=0.1, kernel_scale=1.0)
    with pytest.raises(EpiError, match="every n_rows must lie in"):
        hostapi.svr(X, y, n_rows=[0], **kw)
    with pytest.raises(EpiError, match="tol must be finite"):
        hostapi.svr(X, y, tol=0.0, **kw)
    with pytest.raises(EpiError, match="max_iter must lie in"):
        hostapi.svr(X, y, max_iter=0, **kw)
    with pytest.raises(EpiError, match="w exists for the linear kernel only"):
        hostapi.svr(X, y, kernel="gaussian", outputs=("w",), **kw)
    with pytest.raises(EpiError, match="F is limited to 96"):
        hostapi.svr(np.ones((2, 97, 1)), np.ones((2, 1)), **kw)
    with pytest.raises(ValueError, match="no result"):
        pipeline.growth_forecast_mean([])
    assert "svr" in pipeline.GROWTH_SOLVERS and "svr_gaussian" in pipeline.GROWTH_SOLVERS

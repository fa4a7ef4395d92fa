"""epi_fuse_validate and the argument checks of epi_fuse_run_host, through the C ABI (no GPU needed: every case is rejected
before a device is touched), the exported symbols, and the argument checks of the Python entry points."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import helpers as H


def _call(fn="validate", **kw):
    from epidemicmodeling_amd import _lib
    args = dict(m=6, B=70, T=5, form=1, p_solver=0, lane_block=0, storage=0)
    args.update({k: v for k, v in kw.items() if k in args})
    d = _lib.make_fuse_desc(**args)
    for k in ("abi_version", "reserved"):
        if k in kw:
            setattr(d, k, kw[k])
    buf = np.ones(4096)                                 # never read: every case here is decided on the descriptor and pointers
    ins = _lib.FuseInputs()
    for k in _lib.FUSE_IN_NAMES:
        setattr(ins, k, buf.ctypes.data)
    for k in kw.get("null_in", ()):
        setattr(ins, k, None)
    outs = _lib.FuseOutputs()
    for k in _lib.FUSE_OUT_NAMES:
        setattr(outs, k, buf.ctypes.data)
    for k in kw.get("null_outs", ()):
        setattr(outs, k, None)
    err = C.create_string_buffer(256)
    dp = None if kw.get("null_desc") else C.byref(d)
    ip = None if kw.get("null_inputs") else C.byref(ins)
    op = None if kw.get("null_outputs") else C.byref(outs)
    lib = _lib.lib()
    rc = lib.epi_fuse_validate(dp, ip, op, err) if fn == "validate" else lib.epi_fuse_run_host(dp, ip, op, 0, err)
    return rc, err.value.decode()


BAD = [
    (dict(null_desc=True), "NULL descriptor"),
    (dict(abi_version=5), "ABI version mismatch"),
    (dict(m=2), "m must be 3 or 6"),
    (dict(m=4), "m must be 3 or 6"),
    (dict(m=7), "m must be 3 or 6"),
    (dict(B=0), "B must be >= 1"),
    (dict(T=0), "T must be >= 1"),
    (dict(lane_block=-1), "lane_block must lie in 0 .. B"),
    (dict(lane_block=71), "lane_block must lie in 0 .. B"),
    (dict(storage=2), "storage must be 0 (double) or 1 (float)"),
    (dict(storage=-1), "storage must be 0 (double) or 1 (float)"),
    (dict(form=2), "form must be 0"),
    (dict(form=-1), "form must be 0"),
    (dict(form=0, p_solver=2), "p_solver must be 0 (S \\ C) or 1"),
    (dict(form=0, p_solver=-1), "p_solver must be 0 (S \\ C) or 1"),
    (dict(form=1, p_solver=1), "p_solver must be 0 with form = 1"),
    (dict(reserved=1), "reserved must be 0"),
    (dict(null_inputs=True), "NULL inputs / outputs"),
    (dict(null_outputs=True), "NULL inputs / outputs"),
    (dict(null_in=("sf",)), "NULL sf / Pf / sb / Pb"),
    (dict(null_in=("Pf",)), "NULL sf / Pf / sb / Pb"),
    (dict(null_in=("sb",)), "NULL sf / Pf / sb / Pb"),
    (dict(null_in=("Pb",)), "NULL sf / Pf / sb / Pb"),
    (dict(null_outs=("s_out", "P_out", "d2")), "no output requested"),
]


@pytest.mark.parametrize("kw, msg", BAD)
def test_validate_rejects(hip_lib, kw, msg):
    got, text = _call("validate", **kw)
    assert got == -5 and msg in text, (got, text)
    got, text = _call("run_host", **kw)                     # the host entry validates first, before any device work
    assert got == -5 and msg in text, (got, text)


def test_validate_accepts(hip_lib):
    assert _call("validate") == (0, "")
    for m in (3, 6):
        for form, ps in ((0, 0), (0, 1), (1, 0)):
            for st in (0, 1):
                assert _call("validate", m=m, form=form, p_solver=ps, storage=st)[0] == 0
    assert _call("validate", B=1, T=1)[0] == 0
    assert _call("validate", lane_block=70)[0] == 0 and _call("validate", lane_block=40)[0] == 0
    assert _call("validate", B=2 ** 31 - 1, T=2 ** 31 - 1)[0] == 0
    # every output is optional as long as one of s_out / P_out / d2 is left
    assert _call("validate", null_outs=("P_out", "d2", "rank", "status"))[0] == 0
    assert _call("validate", null_outs=("s_out", "d2", "rank", "status"))[0] == 0
    assert _call("validate", null_outs=("s_out", "P_out", "rank", "status"))[0] == 0


def test_symbols_header_and_structs(hip_lib):
    from epidemicmodeling_amd import _lib
    header = open(os.path.join(H.ROOT, "include", "epiekf.h")).read()
    for sym in ("epi_fuse_validate", "epi_fuse_run_device", "epi_fuse_run_host"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(hip_lib, sym) and f"int {sym}(" in header, sym
    for name in ("epi_fuse_desc", "epi_fuse_inputs", "epi_fuse_outputs"):
        assert f"}} {name};" in header
    assert "#define EPIEKF_ABI_VERSION 6" in header and hip_lib.epi_abi_version() == 6
    assert C.sizeof(_lib.FuseDesc) == 9 * 4
    assert [n for n, _ in _lib.FuseDesc._fields_] == ["abi_version", "m", "B", "T", "lane_block", "storage", "form", "p_solver", "reserved"]
    assert C.sizeof(_lib.FuseInputs) == 4 * C.sizeof(C.c_void_p) and C.sizeof(_lib.FuseOutputs) == 5 * C.sizeof(C.c_void_p)
    assert "PARITY UNPINNED" in header                      # backslash's Cholesky-first path for a symmetric S


def test_python_entry_points_check_their_arguments(hip_lib):
    from epidemicmodeling_amd import hostapi
    from epidemicmodeling_amd._lib import EpiError
    sf, Pf = np.zeros((4, 3, 2)), np.zeros((4, 9, 2))
    with pytest.raises(ValueError, match="m must be 3 or 6"):
        hostapi.two_filter(np.zeros((4, 4, 2)), np.zeros((4, 16, 2)), np.zeros((4, 4, 2)), np.zeros((4, 16, 2)))
    with pytest.raises(ValueError, match="m must be 3 or 6"):
        hostapi.two_filter(sf, np.zeros((4, 8, 2)), sf, Pf)
    with pytest.raises(ValueError, match="unknown output"):
        hostapi.two_filter(sf, Pf, sf, Pf, outputs=("s", "cov"))
    with pytest.raises(EpiError, match="form must be"):
        hostapi.two_filter(sf, Pf, sf, Pf, form=2)
    with pytest.raises(EpiError, match="p_solver must be 0 with form = 1"):
        hostapi.two_filter(sf, Pf, sf, Pf, form=1, p_solver=1)
    with pytest.raises(EpiError, match="no output requested"):
        hostapi.two_filter(sf, Pf, sf, Pf, outputs=("rank", "status"))

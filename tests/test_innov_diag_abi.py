"""epi_idiag_validate, epi_idiag_workspace_bytes and the argument checks of epi_idiag_run_device / _run_host through the C ABI (no
GPU needed: every case is rejected before a device is touched), the exported symbols, and the argument checks of the Python
entry points."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import helpers as H


def _desc(**kw):
    from epidemicmodeling_amd import _lib
    args = dict(B=70, T=45, n_lags=10, k0=0, k1=None, flip=0, lane_block=0, storage=0)
    args.update({k: v for k, v in kw.items() if k in args})
    d = _lib.make_idiag_desc(**args)
    for k in ("abi_version", "reserved"):
        if k in kw:
            setattr(d, k, kw[k])
    return d


def _call(fn="validate", **kw):
    from epidemicmodeling_amd import _lib
    d = _desc(**kw)
    lib, err = _lib.lib(), C.create_string_buffer(256)
    dp = None if kw.get("null_desc") else C.byref(d)
    if fn == "validate":
        return lib.epi_idiag_validate(dp, err), err.value.decode()
    if fn == "workspace":
        n = C.c_size_t(12345)
        rc = lib.epi_idiag_workspace_bytes(dp, C.byref(n), err)
        return rc, err.value.decode(), n.value
    buf = np.ones(4096)                                 # never read: every case here is decided on the descriptor and pointers
    ins = _lib.IdiagInputs()
    ins.e = ins.S = buf.ctypes.data
    for k in kw.get("null_in", ()):
        setattr(ins, k, None)
    outs = _lib.IdiagOutputs()
    for k in kw.get("outs", _lib.IDIAG_OUT_NAMES):
        setattr(outs, k, buf.ctypes.data)
    ip = None if kw.get("null_inputs") else C.byref(ins)
    op = None if kw.get("null_outputs") else C.byref(outs)
    if fn == "run_device":
        rc = lib.epi_idiag_run_device(dp, ip, op, buf.ctypes.data, kw.get("ws_bytes", 0), None, err)
    else:
        rc = lib.epi_idiag_run_host(dp, ip, op, 0, err)
    return rc, err.value.decode()


BAD = [
    (dict(null_desc=True), -5, "NULL descriptor"),
    (dict(abi_version=5), -5, "ABI version mismatch"),
    (dict(B=0), -5, "B must be >= 1"),
    (dict(T=0), -5, "T must be >= 1"),
    (dict(lane_block=-1), -5, "lane_block must lie in 0 .. B"),
    (dict(lane_block=71), -5, "lane_block must lie in 0 .. B"),
    (dict(storage=2), -5, "storage must be 0 (double) or 1 (float)"),
    (dict(flip=2), -5, "flip must be 0 or 1"),
    (dict(k0=-1), -5, "the window must satisfy"),
    (dict(k0=10, k1=5), -5, "the window must satisfy"),
    (dict(k0=46, k1=46), -5, "the window must satisfy"),
    (dict(k1=46), -5, "the window must satisfy"),
    (dict(n_lags=-1), -5, "n_lags must be >= 0"),
    (dict(reserved=1), -5, "reserved must be 0"),
    (dict(n_lags=65), -8, "n_lags is limited to 64"),
    (dict(B=1, T=2 ** 21), -8, "T is limited to 2^21 - 1"),
    (dict(B=2 ** 31 - 1, T=45), -8, "B * ceil(T / 32) is limited"),
    (dict(B=2 ** 26, T=32 * 32), -8, "B * ceil(T / 32) is limited"),
]
BAD_ARRAYS = [
    (dict(null_inputs=True), -5, "NULL inputs / outputs"),
    (dict(null_outputs=True), -5, "NULL inputs / outputs"),
    (dict(null_in=("e",)), -5, "NULL e"),
    (dict(outs=()), -5, "no output requested"),
]


@pytest.mark.parametrize("kw, code, msg", BAD)
def test_validate_rejects(hip_lib, kw, code, msg):
    for fn in ("validate", "workspace", "run_device", "run_host"):       # every entry validates first, before any device work
        got = _call(fn, **kw)
        assert got[0] == code and msg in got[1], (fn, got)
        if fn == "workspace":
            assert got[2] == 12345                                      # not written


@pytest.mark.parametrize("kw, code, msg", BAD_ARRAYS)
def test_entries_reject_arrays(hip_lib, kw, code, msg):
    for fn in ("run_device", "run_host"):
        got = _call(fn, ws_bytes=1 << 30, **kw)
        assert got[0] == code and msg in got[1], (fn, got)


def test_workspace_too_small_is_refused(hip_lib):
    rc, _, need = _call("workspace")
    assert rc == 0 and need > 0
    got = _call("run_device", ws_bytes=need - 1)
    assert got[0] == -6 and "workspace too small" in got[1]


def test_validate_accepts_and_workspace_sizes(hip_lib):
    assert _call("validate") == (0, "")
    for kw in (dict(storage=1), dict(flip=1), dict(n_lags=0), dict(n_lags=64), dict(k0=12, k1=12), dict(k0=45, k1=45), dict(k0=0, k1=0),
               dict(lane_block=40), dict(lane_block=70), dict(B=1, T=1), dict(B=1, T=2 ** 21 - 1), dict(B=2 ** 26 + 70, T=33)):
        assert _call("validate", **kw)[0] == 0, kw
    # the records of ceil(45 / 32) = 2 blocks: 10 doubles and 7 int32 per (block, chain), 2 + 2 per chain, H doubles per (block, chain)
    up = lambda v: (v + 255) // 256 * 256
    want = 10 * up(2 * 70 * 8) + 7 * up(2 * 70 * 4) + 2 * up(70 * 8) + 2 * up(70 * 4)
    assert _call("workspace", n_lags=0)[2] == want
    assert _call("workspace")[2] == want + up(2 * 10 * 70 * 8)


def test_symbols_header_and_structs(hip_lib):
    from epidemicmodeling_amd import _lib
    header = open(os.path.join(H.ROOT, "include", "epiekf.h")).read()
    types = open(os.path.join(H.ROOT, "include", "epiekf_idiag.h")).read()      # included by epiekf.h: the call's three structures
    assert '#include "epiekf_idiag.h"' in header
    for sym in ("epi_idiag_validate", "epi_idiag_workspace_bytes", "epi_idiag_run_device", "epi_idiag_run_host"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(hip_lib, sym) and f"int {sym}(" in header, sym
        assert getattr(hip_lib, sym).restype is C.c_int
    for name in ("epi_idiag_desc", "epi_idiag_inputs", "epi_idiag_outputs"):
        assert f"}} {name};" in types
    assert "#define EPIEKF_ABI_VERSION 6" in header and hip_lib.epi_abi_version() == 6
    assert "idiag" not in _lib.FAMILIES and len(_lib.FAMILIES) == 9
    assert [n for n, _ in _lib.IdiagDesc._fields_] == ["abi_version", "B", "T", "lane_block", "storage", "flip", "k0", "k1", "n_lags",
                                                       "reserved"]
    assert C.sizeof(_lib.IdiagDesc) == 10 * 4
    assert [n for n, _ in _lib.IdiagInputs._fields_] == ["e", "S"]
    assert [n for n, _ in _lib.IdiagOutputs._fields_] == list(_lib.IDIAG_OUT_NAMES) and len(_lib.IDIAG_OUT_NAMES) == 19
    assert C.sizeof(_lib.IdiagOutputs) == 19 * C.sizeof(C.c_void_p)
    assert (_lib.IDIAG_BAD_DAY, _lib.IDIAG_EMPTY, _lib.IDIAG_DEGENERATE, _lib.IDIAG_FEW_LAGS) == (1, 2, 4, 8)


def test_python_entry_points_check_their_arguments(hip_lib):
    from epidemicmodeling_amd import hostapi
    from epidemicmodeling_amd._lib import EpiError
    T, B = 6, 4
    e, S = np.zeros((T, B)), np.ones((T, B))
    f = hostapi.innovation_diagnostics
    with pytest.raises(ValueError, match="innovations must be"):
        f(np.zeros((T, 3, B)), S)
    with pytest.raises(ValueError, match="innovations must be"):
        f(np.zeros((T, B + 1)), S, B=B)
    with pytest.raises(ValueError, match="innovations must be"):
        f(np.zeros((T, 7)), None, lane_block=3, B=5)           # two blocks of 3 are 6 columns
    with pytest.raises(ValueError, match="S must be"):
        f(e, np.ones((T + 1, B)))
    with pytest.raises(ValueError, match="need B"):
        f(np.zeros((T, 6)), None, lane_block=3)
    with pytest.raises(ValueError, match="unknown output"):
        f(e, S, outputs=("mean", "pacf"))
    with pytest.raises(EpiError, match="the window must satisfy"):
        f(e, S, k0=3, k1=2)
    with pytest.raises(EpiError, match="n_lags is limited to 64"):
        f(e, S, n_lags=65)
    with pytest.raises(EpiError, match="n_lags must be >= 0"):
        f(e, S, n_lags=-1)

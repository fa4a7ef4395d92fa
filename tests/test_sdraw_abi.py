"""epi_sdraw_validate, epi_sdraw_workspace_bytes and the argument checks of epi_sdraw_run_device / _run_host through the C ABI (no
GPU needed: every case is rejected before a device is touched), the struct layouts against the header, the exported symbols,
and the argument checks of the Python entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import helpers as H


def _desc(**kw):
    from epidemicmodeling_amd import _lib
    args = dict(B=5, T=33, D=3, k0=0, clamp=1, lane_block=0, storage=0, z_f32=0, out_f32=0, model="SIAlphaModelEKF", test_launch_groups=0)
    args.update({k: v for k, v in kw.items() if k in args})
    d = _lib.make_sdraw_desc(**args)
    if "abi_version" in kw:
        d.abi_version = kw["abi_version"]
    return d


def _call(fn="validate", **kw):
    from epidemicmodeling_amd import _lib
    d = _desc(**kw)
    lib, err = _lib.lib(), C.create_string_buffer(256)
    dp = None if kw.get("null_desc") else C.byref(d)
    if fn == "validate":
        return lib.epi_sdraw_validate(dp, err), err.value.decode()
    if fn == "workspace":
        n = C.c_size_t(12345)
        rc = lib.epi_sdraw_workspace_bytes(dp, C.byref(n), err)
        return rc, err.value.decode(), n.value
    buf = np.ones(4096)                                 # never read: every case here is decided on the descriptor and pointers
    ins = _lib.SdrawInputs()
    for k in _lib.SDRAW_IN_NAMES:
        setattr(ins, k, None if k in kw.get("null_in", ()) else buf.ctypes.data)
    outs = _lib.SdrawOutputs()
    for k in _lib.SDRAW_OUT_NAMES:
        setattr(outs, k, None if k in kw.get("null_out", ()) else buf.ctypes.data)
    ip = None if kw.get("null_inputs") else C.byref(ins)
    op = None if kw.get("null_outputs") else C.byref(outs)
    if fn == "run_device":
        rc = lib.epi_sdraw_run_device(dp, ip, op, buf.ctypes.data, kw.get("ws_bytes", 0), None, err)
    else:
        rc = lib.epi_sdraw_run_host(dp, ip, op, 0, err)
    return rc, err.value.decode()


BAD = [
    (dict(null_desc=True), -5, "NULL descriptor"),
    (dict(abi_version=5), -5, "ABI version mismatch"),
    (dict(model=9), -5, "unknown model"),
    (dict(model="SIAlphaModelEKFOptControlled"), -8, "the 6-state costate block has no meaningful factor in fp64"),
    (dict(model="SIAlphaModelBackwardEKFOptControlled"), -8, "the 6-state costate block has no meaningful factor in fp64"),
    (dict(model="NewCaseEKFEstimatorWithOptimalNPI"), -8, "smoother draws need the 3-state SIAlphaModelEKF"),
    (dict(model="SIAlphaModelBackwardEKF"), -8, "smoother draws do not take the time-flipped models"),
    (dict(B=0), -5, "B must be >= 1"),
    (dict(T=0), -5, "T must be >= 1"),
    (dict(D=0), -5, "D must be >= 1"),
    (dict(D=-4), -5, "D must be >= 1"),
    (dict(k0=-1), -5, "k0 must lie in 0 .. T-1"),
    (dict(k0=33), -5, "k0 must lie in 0 .. T-1"),
    (dict(clamp=2), -5, "clamp must be 0 or 1"),
    (dict(lane_block=-1), -5, "lane_block must lie in 0 .. B"),
    (dict(lane_block=6), -5, "lane_block must lie in 0 .. B"),
    (dict(storage=2), -5, "storage must be 0 (double) or 1 (float)"),
    (dict(z_f32=2), -5, "z_f32 must be 0 (double) or 1 (float)"),
    (dict(out_f32=-1), -5, "out_f32 must be 0 (double) or 1 (float)"),
    (dict(test_launch_groups=-1), -5, "test_launch_groups must be >= 0"),
]


@pytest.mark.parametrize("kw, code, msg", BAD)
def test_refusals(hip_lib, kw, code, msg):
    for fn in ("validate", "workspace", "run_device", "run_host"):
        got = _call(fn, **kw)
        assert got[0] == code and msg in got[1], (fn, kw, got)


def test_accepts_and_workspace(hip_lib):
    assert _call("validate") == (0, "")
    assert _call("validate", k0=32, lane_block=5, storage=1, z_f32=1, out_f32=1, clamp=0)[0] == 0
    assert _call("workspace") == (0, "", 33 * 5 * 24 * 8)
    assert _call("workspace", B=300, T=520, D=1024)[2] == 300 * 520 * 192


def test_pointer_checks(hip_lib):
    for fn in ("run_device", "run_host"):
        assert _call(fn, null_inputs=True) == (-5, "NULL inputs / outputs")
        assert _call(fn, null_outputs=True) == (-5, "NULL inputs / outputs")
        for k in ("S_PLUS", "P_PLUS", "S_MINUS", "P_MINUS", "prm"):
            assert _call(fn, null_in=(k,)) == (-5, "NULL S_PLUS / P_PLUS / S_MINUS / P_MINUS / prm")
        assert _call(fn, null_out=("X", "rank", "status", "J", "L"))[1].startswith("no output requested")
    assert _call("run_device", ws_bytes=33 * 5 * 24 * 8 - 1) == (-6, "workspace too small (epi_sdraw_workspace_bytes)")


def test_struct_layouts_symbols_and_constants(hip_lib):
    from epidemicmodeling_amd import _lib
    header = open(os.path.join(H.ROOT, "include", "epiekf.h")).read()
    body = lambda name: re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    fields = lambda txt: [n for decl in re.findall(r"(?:const )?\w+ \*?[^;]*;", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
                          for n in re.findall(r"\*?(\w+)\s*[,;]", decl)]
    assert fields(body("epi_sdraw_desc")) == [n for n, _ in _lib.SdrawDesc._fields_]
    assert fields(body("epi_sdraw_inputs")) == list(_lib.SDRAW_IN_NAMES) == [n for n, _ in _lib.SdrawInputs._fields_]
    assert fields(body("epi_sdraw_outputs")) == list(_lib.SDRAW_OUT_NAMES) == [n for n, _ in _lib.SdrawOutputs._fields_]
    assert C.sizeof(_lib.SdrawDesc) == 12 * 4 and C.sizeof(_lib.SdrawInputs) == 8 * 8 and C.sizeof(_lib.SdrawOutputs) == 5 * 8
    for sym in ("epi_sdraw_validate", "epi_sdraw_workspace_bytes", "epi_sdraw_run_device", "epi_sdraw_run_host"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(hip_lib, sym) and f"int {sym}(" in header, sym
    assert "EPI_SDRAW_NONFINITE = 1, EPI_SDRAW_RANK_DEFICIENT = 2" in header
    assert (_lib.SDRAW_NONFINITE, _lib.SDRAW_RANK_DEFICIENT) == (1, 2)
    assert re.search(r"#define\s+EPIEKF_ABI_VERSION\s+6\b", header)
    assert _lib.sdraw_shapes(5, 33, 3, 11) == dict(X=(22, 3, 15), rank=(33, 5), status=(5,), J=(33, 9, 5), L=(33, 9, 5))


def test_python_argument_checks(hip_lib):
    """hostapi.smoother_draws refuses what it can before the library is asked (no device is touched)"""
    from epidemicmodeling_amd import hostapi
    T, B = 6, 4
    S, P, prm = np.zeros((T, 3, B)), np.zeros((T, 9, B)), np.zeros((61, B))
    f = lambda *a, **k: hostapi.smoother_draws(*a, **k)
    with pytest.raises(ValueError, match="3-state model"):
        f(np.zeros((T, 6, B)), np.zeros((T, 36, B)), np.zeros((T, 6, B)), np.zeros((T, 36, B)), prm, 2)
    with pytest.raises(ValueError, match="lane_block given with classic"):
        f(S, P, S, P, prm, 2, lane_block=2)
    with pytest.raises(ValueError, match="need lane_block = blk"):
        f(*(np.zeros((T, 2, r, 2)) for r in (3, 9, 3, 9)), prm, 2, lane_block=3)
    with pytest.raises(ValueError, match="prm must be"):
        f(S, P, S, P, np.zeros((60, B)), 2)
    with pytest.raises(ValueError, match=r"z must be \[T - k0, 3, B \* D\]"):
        f(S, P, S, P, prm, 2, z=np.zeros((T, 3, B * 2)), k0=1)
    with pytest.raises(ValueError, match="s_term must be"):
        f(S, P, S, P, prm, 2, s_term=np.zeros((3, B + 1)))
    with pytest.raises(ValueError, match="P_term must be"):
        f(S, P, S, P, prm, 2, P_term=np.zeros((3, B)))
    with pytest.raises(ValueError, match="out_dtype must be"):
        f(S, P, S, P, prm, 2, out_dtype=np.int32)
    with pytest.raises(ValueError, match=r"unknown outputs \['nope'\]"):
        f(S, P, S, P, prm, 2, outputs=("X", "nope"))
    with pytest.raises(RuntimeError, match="D must be >= 1"):
        f(S, P, S, P, prm, 0)
    with pytest.raises(RuntimeError, match="k0 must lie in"):
        f(S, P, S, P, prm, 2, k0=T)

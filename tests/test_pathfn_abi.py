"""epi_pathfn_validate, epi_pathfn_workspace_bytes and the argument checks of epi_pathfn_run_device / _run_host through the C ABI
(no GPU needed: every case is rejected before a device is touched), the struct layouts against the header, the exported symbols,
and the argument checks of the Python entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import helpers as H


def _desc(**kw):
    from epidemicmodeling_amd import _lib
    args = dict(T=80, rows=3, R=4, D=65, n_thr=2, storage=0, derive_newcases=0, k0=0, k1=None, test_segments=0, test_launch_groups=0)
    args.update({k: v for k, v in kw.items() if k in args})
    d = _lib.make_pathfn_desc(**args)
    if "abi_version" in kw:
        d.abi_version = kw["abi_version"]
    return d


def _call(fn="validate", **kw):
    from epidemicmodeling_amd import _lib
    d = _desc(**kw)
    lib, err = _lib.lib(), C.create_string_buffer(256)
    dp = None if kw.get("null_desc") else C.byref(d)
    if fn == "workspace":
        n = C.c_size_t(12345)
        rc = lib.epi_pathfn_workspace_bytes(dp, C.byref(n), err)
        return rc, err.value.decode(), n.value
    buf = np.ones(4096)                                 # never read: every case here is decided on the descriptor and pointers
    ins = _lib.PathfnInputs()
    for k in _lib.PATHFN_IN_NAMES:
        setattr(ins, k, None if k in kw.get("null_in", ("population", "first_day")) else buf.ctypes.data)
    outs = _lib.PathfnOutputs()
    for k in _lib.PATHFN_OUT_NAMES:
        setattr(outs, k, None if k in kw.get("null_out", ()) else buf.ctypes.data)
    ip = None if kw.get("null_inputs") else C.byref(ins)
    op = None if kw.get("null_outputs") else C.byref(outs)
    if fn == "validate":
        rc = lib.epi_pathfn_validate(dp, ip, op, err)
    elif fn == "run_device":
        rc = lib.epi_pathfn_run_device(dp, ip, op, buf.ctypes.data, kw.get("ws_bytes", 0), None, err)
    else:
        rc = lib.epi_pathfn_run_host(dp, ip, op, 0, err)
    return rc, err.value.decode()


BAD_DESC = [
    (dict(null_desc=True), "NULL descriptor"),
    (dict(abi_version=5), "ABI version mismatch"),
    (dict(T=0), "T must be >= 1"),
    (dict(rows=0), "rows must lie in 1 .. 4096"),
    (dict(rows=4097), "rows must lie in 1 .. 4096"),
    (dict(R=0), "R must be >= 1"),
    (dict(D=0), "D must be >= 1"),
    (dict(R=1 << 20, D=4096), "R * D is limited to 2^31 - 1"),
    (dict(n_thr=-1), "n_thr must lie in 0 .. 8"),
    (dict(n_thr=9), "n_thr must lie in 0 .. 8"),
    (dict(k0=-1), "k0, k1 must satisfy 0 <= k0 < k1 <= T"),
    (dict(k0=4, k1=4), "k0, k1 must satisfy 0 <= k0 < k1 <= T"),
    (dict(k0=4, k1=3), "k0, k1 must satisfy 0 <= k0 < k1 <= T"),
    (dict(k1=81), "k0, k1 must satisfy 0 <= k0 < k1 <= T"),
    (dict(storage=2), "storage must be 0 (double) or 1 (float)"),
    (dict(derive_newcases=2), "derive_newcases must be 0 or 1"),
    (dict(derive_newcases=1, rows=2), "derive_newcases needs at least 3 rows"),
    (dict(test_segments=-1), "test_segments must lie in 0 .. min(ceil((k1 - k0) / 32), 1024)"),
    (dict(test_segments=4), "test_segments must lie in 0 .. min(ceil((k1 - k0) / 32), 1024)"),          # 80 days are three blocks
    (dict(k0=10, k1=42, test_segments=2), "a segment is whole 32-day blocks"),
    (dict(T=40000, test_segments=1025), "test_segments must lie in"),
    (dict(test_launch_groups=-1), "test_launch_groups must be >= 0"),
]
THR_OUT = ("first_cross", "days_above", "longest_run", "n_cross", "cross_day_hist")
BAD_ARGS = [
    (dict(null_inputs=True), "NULL inputs / outputs"),
    (dict(null_outputs=True), "NULL inputs / outputs"),
    (dict(null_in=("src",)), "NULL src"),
    (dict(derive_newcases=1), "NULL population (derive_newcases)"),
    (dict(null_in=("thr", "population", "first_day")), "NULL thr (n_thr > 0)"),
    (dict(n_thr=0), "need n_thr >= 1"),
    (dict(T=4097), "a histogram holds at most 4096 days (k1 - k0)"),
    (dict(T=5000, k0=3, k1=4100, null_out=("peak_day_hist",)), "a histogram holds at most 4096 days (k1 - k0)"),
    (dict(null_out=("peak_value", "peak_day", "min_value", "min_day", "total", "n_valid", "n_paths", "peak_day_hist") + THR_OUT), "no output requested"),
]


@pytest.mark.parametrize("kw, msg", BAD_DESC)
def test_descriptor_refusals(hip_lib, kw, msg):
    for fn in ("validate", "workspace", "run_device", "run_host"):
        got = _call(fn, **kw)
        assert got[0] == -5 and msg in got[1], (fn, kw, got)


@pytest.mark.parametrize("kw, msg", BAD_ARGS)
def test_argument_refusals(hip_lib, kw, msg):
    for fn in ("validate", "run_device", "run_host"):
        got = _call(fn, **kw)
        assert got[0] == -5 and msg in got[1], (fn, kw, got)


def test_accepts_and_workspace(hip_lib):
    assert _call("validate") == (0, "")
    assert _call("validate", n_thr=0, null_out=THR_OUT) == (0, "")
    assert _call("validate", T=5000, k1=4096, n_thr=8, storage=1, test_segments=128)[0] == 0
    assert _call("validate", T=5000, null_out=("peak_day_hist", "cross_day_hist"))[0] == 0      # only the histograms bound the window
    assert _call("validate", derive_newcases=1, null_in=("first_day",))[0] == 0
    assert _call("validate", k0=79, k1=80, test_segments=1)[0] == 0
    M = 3 * 4 * 65
    assert _call("workspace", test_segments=1) == (0, "", (1 + 2) * M * 8)
    # three segments of one block each: two doubles and three int32 a segment, a block sum a block, five int32 a segment and threshold
    assert _call("workspace", test_segments=3)[2] == (1 + 2) * M * 8 + (2 * 3 + 3) * M * 8 + 3 * (3 + 5 * 2) * M * 4
    assert _call("workspace", test_segments=2)[2] == (1 + 2) * M * 8 + (2 * 2 + 3) * M * 8 + 2 * (3 + 5 * 2) * M * 4
    assert _call("workspace", T=520, rows=3, derive_newcases=1, R=300, D=1024, n_thr=0)[2] == 4 * 300 * 1024 * 8     # many waves: one segment
    assert _call("run_device", ws_bytes=(1 + 2) * M * 8 - 1, test_segments=1) == (-6, "workspace too small (epi_pathfn_workspace_bytes)")


def test_struct_layouts_symbols_and_constants(hip_lib):
    from epidemicmodeling_amd import _lib
    header = open(os.path.join(H.ROOT, "include", "epiekf.h")).read()
    body = lambda name: re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    fields = lambda txt: [n for decl in re.findall(r"(?:const )?\w+ \*?[^;]*;", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
                          for n in re.findall(r"\*?(\w+)(?:\[\d+\])?\s*[,;]", decl)]
    assert fields(body("epi_pathfn_desc")) == [n for n, _ in _lib.PathfnDesc._fields_]
    assert fields(body("epi_pathfn_inputs")) == list(_lib.PATHFN_IN_NAMES) == [n for n, _ in _lib.PathfnInputs._fields_]
    assert fields(body("epi_pathfn_outputs")) == list(_lib.PATHFN_OUT_NAMES) == [n for n, _ in _lib.PathfnOutputs._fields_]
    assert C.sizeof(_lib.PathfnDesc) == 12 * 4 and C.sizeof(_lib.PathfnInputs) == 4 * 8 and C.sizeof(_lib.PathfnOutputs) == 13 * 8
    for sym in ("epi_pathfn_validate", "epi_pathfn_workspace_bytes", "epi_pathfn_run_device", "epi_pathfn_run_host"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(hip_lib, sym) and f"int {sym}(" in header, sym
        assert getattr(hip_lib, sym).restype is C.c_int
    assert "pathfn" not in _lib.FAMILIES and len(_lib.FAMILIES) == 9
    assert re.search(r"#define\s+EPIEKF_ABI_VERSION\s+6\b", header) and _lib.ABI_VERSION == 6 and hip_lib.epi_abi_version() == 6
    sh = _lib.pathfn_shapes(3, 4, 65, 2, 67, 1)
    assert sh["peak_value"] == sh["total"] == sh["n_valid"] == (4, 260) and sh["first_cross"] == sh["longest_run"] == (2, 4, 260)
    assert sh["n_paths"] == (4, 4) and sh["peak_day_hist"] == (67, 4, 4) and sh["n_cross"] == (2, 4, 4) and sh["cross_day_hist"] == (67, 2, 4, 4)
    assert list(sh) == list(_lib.PATHFN_OUT_NAMES) and set(_lib.PATHFN_OUT_I32) == {"n_valid", "n_paths", "peak_day_hist", "n_cross", "cross_day_hist"}
    assert _lib.pathfn_out_names(None, 0) == [k for k in _lib.PATHFN_OUT_NAMES if k not in THR_OUT]
    assert _lib.pathfn_out_names(None, 1) == list(_lib.PATHFN_OUT_NAMES)
    assert _lib.pathfn_out_names(("n_paths", "total"), 0) == ["total", "n_paths"]


def test_python_argument_checks(hip_lib):
    """hostapi.path_functionals refuses what it can before a device is touched"""
    from epidemicmodeling_amd import hostapi
    T, R, D = 40, 3, 7
    src = np.zeros((T, 2, R * D))
    f = hostapi.path_functionals
    with pytest.raises(ValueError, match="chain-blocked"):
        f(np.zeros((T, 2, 2, 8)), R, D)
    with pytest.raises(ValueError, match=r"src must be \[T, rows, B\] or \[T, B\]"):
        f(np.zeros(R * D), R, D)
    with pytest.raises(ValueError, match="src holds 21 chains, R \\* D = 24"):
        f(src, R, 8)
    with pytest.raises(ValueError, match=r"population must be \[R\]"):
        f(src, R, D, population=np.ones(R + 1))
    with pytest.raises(ValueError, match=r"thresholds must be \[n_thr, rows', R\] = \[n_thr, 2, 3\]"):
        f(src, R, D, thresholds=np.zeros((2, 3, R)))
    with pytest.raises(ValueError, match=r"thresholds must be \[n_thr, rows', R\] = \[n_thr, 4, 3\]"):
        f(np.zeros((T, 3, R * D)), R, D, thresholds=np.zeros((2, 3, R)), population=np.ones(R))    # the derived row has thresholds too
    with pytest.raises(ValueError, match=r"first_day must be \[R\]"):
        f(src, R, D, first_day=[0])
    with pytest.raises(ValueError, match=r"unknown outputs \['nope'\]"):
        f(src, R, D, outputs=("total", "nope"))
    with pytest.raises(RuntimeError, match="n_thr must lie in 0 .. 8"):
        f(src, R, D, thresholds=np.zeros((9, 2, R)))
    with pytest.raises(RuntimeError, match="k0, k1 must satisfy"):
        f(src, R, D, k0=3, k1=3)
    with pytest.raises(RuntimeError, match="need n_thr >= 1"):
        f(src, R, D, outputs=("days_above",))
    with pytest.raises(RuntimeError, match="derive_newcases needs at least 3 rows"):
        f(src, R, D, population=np.ones(R))
    with pytest.raises(RuntimeError, match="test_segments must lie in"):
        f(src, R, D, test_segments=3)
    with pytest.raises(RuntimeError, match="a histogram holds at most 4096 days"):
        f(np.zeros((4097, R * D)), R, D)

"""epi_cdepth_validate, epi_cdepth_workspace_bytes and the argument checks of epi_cdepth_run_device / _run_host through the C ABI
(no GPU needed: every case is rejected before a device is touched), the struct layouts against the header, the exported symbols,
and the argument checks of the Python entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import helpers as H

FENCE_OUT = ("out_days", "n_outliers", "whisk_lo", "whisk_hi")
ENV_OUT = ("env_lo", "env_hi")


def _desc(**kw):
    from epidemicmodeling_amd import _lib
    args = dict(T=80, rows=3, R=4, D=65, alpha=(0.5, 0.9), fence_factor=1.5, fence_frac=0.5, storage=0, derive_newcases=0, k0=0, k1=None,
                test_segments=0, test_launch_groups=0)
    args.update({k: v for k, v in kw.items() if k in args})
    d = _lib.make_cdepth_desc(**args)
    for k in ("abi_version", "n_alpha"):
        if k in kw:
            setattr(d, k, kw[k])
    return d


def _call(fn="validate", **kw):
    from epidemicmodeling_amd import _lib
    d = _desc(**kw)
    lib, err = _lib.lib(), C.create_string_buffer(256)
    dp = None if kw.get("null_desc") else C.byref(d)
    if fn == "workspace":
        n = C.c_size_t(12345)
        rc = lib.epi_cdepth_workspace_bytes(dp, C.byref(n), err)
        return rc, err.value.decode(), n.value
    buf = np.ones(4096)                                 # never read: every case here is decided on the descriptor and pointers
    ins = _lib.CdepthInputs()
    for k in _lib.CDEPTH_IN_NAMES:
        setattr(ins, k, None if k in kw.get("null_in", ("population", "first_day")) else buf.ctypes.data)
    outs = _lib.CdepthOutputs()
    for k in _lib.CDEPTH_OUT_NAMES:
        setattr(outs, k, None if k in kw.get("null_out", ()) else buf.ctypes.data)
    ip = None if kw.get("null_inputs") else C.byref(ins)
    op = None if kw.get("null_outputs") else C.byref(outs)
    if fn == "validate":
        rc = lib.epi_cdepth_validate(dp, ip, op, err)
    elif fn == "run_device":
        rc = lib.epi_cdepth_run_device(dp, ip, op, buf.ctypes.data, kw.get("ws_bytes", 0), None, err)
    else:
        rc = lib.epi_cdepth_run_host(dp, ip, op, 0, err)
    return rc, err.value.decode()


BAD_DESC = [
    (dict(null_desc=True), "NULL descriptor"),
    (dict(abi_version=5), "ABI version mismatch"),
    (dict(T=0), "T must be >= 1"),
    (dict(rows=0), "rows must lie in 1 .. 4096"),
    (dict(rows=4097), "rows must lie in 1 .. 4096"),
    (dict(R=0), "R must be >= 1"),
    (dict(D=0), "D must lie in 1 .. 4096"),
    (dict(D=4097), "D must lie in 1 .. 4096"),
    (dict(R=1 << 20, D=4096), "R * D is limited to 2^31 - 1"),
    (dict(k0=-1), "k0, k1 must satisfy 0 <= k0 < k1 <= T"),
    (dict(k0=4, k1=4), "k0, k1 must satisfy 0 <= k0 < k1 <= T"),
    (dict(k0=4, k1=3), "k0, k1 must satisfy 0 <= k0 < k1 <= T"),
    (dict(k1=81), "k0, k1 must satisfy 0 <= k0 < k1 <= T"),
    (dict(storage=2), "storage must be 0 (double) or 1 (float)"),
    (dict(derive_newcases=2), "derive_newcases must be 0 or 1"),
    (dict(derive_newcases=1, rows=2), "derive_newcases needs at least 3 rows"),
    (dict(n_alpha=-1), "n_alpha must lie in 0 .. 8"),
    (dict(n_alpha=9), "n_alpha must lie in 0 .. 8"),
    (dict(alpha=(0.0, 0.5)), "every alpha must lie in (0, 1]"),
    (dict(alpha=(0.5, 1.0000001)), "every alpha must lie in (0, 1]"),
    (dict(alpha=(0.5, float("nan"))), "every alpha must lie in (0, 1]"),
    (dict(alpha=(-0.5,)), "every alpha must lie in (0, 1]"),
    (dict(alpha=(0.5, 0.5)), "alpha must be strictly ascending"),
    (dict(alpha=(0.9, 0.5)), "alpha must be strictly ascending"),
    (dict(fence_factor=-1.5), "fence_factor must be >= 0"),
    (dict(fence_factor=float("nan")), "fence_factor must be >= 0"),
    (dict(fence_frac=0.0), "fence_frac must lie in (0, 1]"),
    (dict(fence_frac=1.5), "fence_frac must lie in (0, 1]"),
    (dict(fence_frac=float("nan")), "fence_frac must lie in (0, 1]"),
    (dict(test_segments=-1), "test_segments must lie in 0 .. min(ceil((k1 - k0) / 32), 1024)"),
    (dict(test_segments=4), "test_segments must lie in 0 .. min(ceil((k1 - k0) / 32), 1024)"),          # 80 days are three blocks
    (dict(k0=10, k1=42, test_segments=2), "a segment is whole 32-day blocks"),
    (dict(T=40000, test_segments=1025), "test_segments must lie in"),
    (dict(test_launch_groups=-1), "test_launch_groups must be >= 0"),
]
BAD_ARGS = [
    (dict(null_inputs=True), "NULL inputs / outputs"),
    (dict(null_outputs=True), "NULL inputs / outputs"),
    (dict(null_in=("src",)), "NULL src"),
    (dict(derive_newcases=1), "NULL population (derive_newcases)"),
    (dict(alpha=()), "env_lo and env_hi need n_alpha >= 1"),
    (dict(alpha=(), null_out=("env_lo",)), "env_lo and env_hi need n_alpha >= 1"),
    (dict(fence_factor=0.0), "out_days, n_outliers, whisk_lo and whisk_hi need fence_factor > 0"),
    (dict(fence_factor=0.0, null_out=FENCE_OUT[:3]), "out_days, n_outliers, whisk_lo and whisk_hi need fence_factor > 0"),
    (dict(null_out=("depth", "mhi", "band_count", "pair_total", "n_valid", "depth_rank", "n_ranked", "median_path", "median_curve")
          + ENV_OUT + FENCE_OUT), "no output requested"),
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
    assert _call("validate", alpha=(), null_out=ENV_OUT) == (0, "")
    assert _call("validate", fence_factor=0.0, fence_frac=0.0, null_out=FENCE_OUT) == (0, "")          # no boxplot: fence_frac is not looked at
    assert _call("validate", alpha=tuple(np.linspace(0.125, 1.0, 8)), fence_frac=1.0, D=4096, storage=1)[0] == 0
    assert _call("validate", T=5000, k1=4096, test_segments=128)[0] == 0
    assert _call("validate", derive_newcases=1, null_in=("first_day",))[0] == 0
    assert _call("validate", k0=79, k1=80, test_segments=1)[0] == 0
    M, plane, T = 3 * 4 * 65, 3 * 4, 80
    # depth and the fence envelope in doubles; three 32-day blocks of four 32-bit sums a path, ranks, out_days, n_ranked, median_path
    want = (M + 2 * T * plane) * 8 + (3 * 4 * M + 2 * M + 2 * plane) * 4
    for seg in (0, 1, 2, 3):                            # the records are per block, however the blocks are shared out
        assert _call("workspace", test_segments=seg) == (0, "", want)
    assert _call("workspace", k0=10, k1=42)[2] == (M + 2 * T * plane) * 8 + (1 * 4 * M + 2 * M + 2 * plane) * 4
    M, plane = 4 * 300 * 1024, 4 * 300
    assert _call("workspace", T=520, derive_newcases=1, R=300, D=1024)[2] == (M + 2 * 520 * plane) * 8 + (17 * 4 * M + 2 * M + 2 * plane) * 4
    assert _call("run_device", ws_bytes=want - 1) == (-6, "workspace too small (epi_cdepth_workspace_bytes)")


def test_struct_layouts_symbols_and_constants(hip_lib):
    from epidemicmodeling_amd import _lib
    top = open(os.path.join(H.ROOT, "include", "epiekf.h")).read()
    header = open(os.path.join(H.ROOT, "include", "epiekf_cdepth.h")).read()
    assert '#include "epiekf_cdepth.h"' in top and "epi_cdepth_desc {" not in top
    body = lambda name: re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    fields = lambda txt: [n for decl in re.findall(r"(?:const )?\w+ \*?[^;]*;", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
                          for n in re.findall(r"\*?(\w+)(?:\[\d+\])?\s*[,;]", decl)]
    assert fields(body("epi_cdepth_desc")) == [n for n, _ in _lib.CdepthDesc._fields_]
    assert fields(body("epi_cdepth_inputs")) == list(_lib.CDEPTH_IN_NAMES) == [n for n, _ in _lib.CdepthInputs._fields_]
    assert fields(body("epi_cdepth_outputs")) == list(_lib.CDEPTH_OUT_NAMES) == [n for n, _ in _lib.CdepthOutputs._fields_]
    assert C.sizeof(_lib.CdepthDesc) == 12 * 4 + 10 * 8 and _lib.CdepthDesc.alpha.offset == 48 and _lib.CdepthDesc.fence_frac.offset == 120
    assert C.sizeof(_lib.CdepthInputs) == 3 * 8 and C.sizeof(_lib.CdepthOutputs) == 15 * 8
    for sym in ("epi_cdepth_validate", "epi_cdepth_workspace_bytes", "epi_cdepth_run_device", "epi_cdepth_run_host"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(hip_lib, sym) and f"int {sym}(" in top, sym
        assert getattr(hip_lib, sym).restype is C.c_int
    assert "cdepth" not in _lib.FAMILIES
    assert re.search(r"#define\s+EPIEKF_ABI_VERSION\s+6\b", top) and _lib.ABI_VERSION == 6 and hip_lib.epi_abi_version() == 6
    sh = _lib.cdepth_shapes(67, 3, 4, 65, 2, 1)
    assert sh["depth"] == sh["pair_total"] == sh["n_valid"] == sh["depth_rank"] == sh["out_days"] == (4, 260)
    assert sh["n_ranked"] == sh["median_path"] == sh["n_outliers"] == (4, 4)
    assert sh["env_lo"] == sh["env_hi"] == (67, 2, 4, 4) and sh["median_curve"] == sh["whisk_lo"] == sh["whisk_hi"] == (67, 4, 4)
    assert list(sh) == list(_lib.CDEPTH_OUT_NAMES)
    assert set(_lib.CDEPTH_OUT_I32) == {"n_valid", "depth_rank", "out_days", "n_ranked", "median_path", "n_outliers"}
    assert _lib.cdepth_out_names(None, 2, 1.5) == list(_lib.CDEPTH_OUT_NAMES)
    assert _lib.cdepth_out_names(None, 0, 1.5) == [k for k in _lib.CDEPTH_OUT_NAMES if k not in ENV_OUT]
    assert _lib.cdepth_out_names(None, 2, 0.0) == [k for k in _lib.CDEPTH_OUT_NAMES if k not in FENCE_OUT]
    assert _lib.cdepth_out_names(("whisk_hi", "depth"), 0, 0.0) == ["depth", "whisk_hi"]
    assert (_lib.CDEPTH_DEFAULT_ALPHA, _lib.CDEPTH_DEFAULT_FENCE_FACTOR, _lib.CDEPTH_DEFAULT_FENCE_FRAC) == ((0.5, 0.9), 1.5, 0.5)


def test_python_argument_checks(hip_lib):
    """hostapi.curve_statistics refuses what it can before a device is touched"""
    from epidemicmodeling_amd import hostapi
    T, R, D = 40, 3, 7
    src = np.zeros((T, 2, R * D))
    f = hostapi.curve_statistics
    with pytest.raises(ValueError, match="chain-blocked.*ensemble_summary takes the classic layout"):
        f(np.zeros((T, 2, 2, 8)), R, D)
    with pytest.raises(ValueError, match=r"src must be \[T, rows, B\] or \[T, B\]"):
        f(np.zeros(R * D), R, D)
    with pytest.raises(ValueError, match="src holds 21 chains, R \\* D = 24"):
        f(src, R, 8)
    with pytest.raises(ValueError, match=r"population must be \[R\]"):
        f(src, R, D, population=np.ones(R + 1))
    with pytest.raises(ValueError, match=r"first_day must be \[R\]"):
        f(src, R, D, first_day=[0])
    with pytest.raises(ValueError, match=r"unknown outputs \['nope'\]"):
        f(src, R, D, outputs=("depth", "nope"))
    with pytest.raises(ValueError, match="at most 8 central regions"):
        f(src, R, D, alpha=np.linspace(0.1, 0.9, 9))
    with pytest.raises(RuntimeError, match="alpha must be strictly ascending"):
        f(src, R, D, alpha=(0.9, 0.5))
    with pytest.raises(RuntimeError, match="k0, k1 must satisfy"):
        f(src, R, D, k0=3, k1=3)
    with pytest.raises(RuntimeError, match="need fence_factor > 0"):
        f(src, R, D, fence_factor=0, outputs=("out_days",))
    with pytest.raises(RuntimeError, match="need n_alpha >= 1"):
        f(src, R, D, alpha=(), outputs=("env_hi",))
    with pytest.raises(RuntimeError, match="fence_frac must lie in"):
        f(src, R, D, fence_frac=0.0)
    with pytest.raises(RuntimeError, match="derive_newcases needs at least 3 rows"):
        f(src, R, D, population=np.ones(R))
    with pytest.raises(RuntimeError, match="test_segments must lie in"):
        f(src, R, D, test_segments=3)
    with pytest.raises(RuntimeError, match="D must lie in 1 .. 4096"):
        f(np.zeros((2, 4097)), 1, 4097)

"""epi_ejoint_validate, epi_ejoint_workspace_bytes and the argument checks of epi_ejoint_run_device / _run_host through the C ABI
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
    args = dict(T=6, rows=3, R=4, D=65, Rt=4, vs_order=1, max_lag=0, storage=0, derive_newcases=0, k0=0, k1=None, test_launch_tiles=0)
    args.update({k: v for k, v in kw.items() if k in args})
    d = _lib.make_ejoint_desc(**args)
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
        rc = lib.epi_ejoint_workspace_bytes(dp, C.byref(n), err)
        return rc, err.value.decode(), n.value
    buf = np.ones(4096)                                 # never read: every case here is decided on the descriptor and pointers
    ins = _lib.EjointInputs()
    for k in _lib.EJOINT_IN_NAMES:
        setattr(ins, k, None if k in kw.get("null_in", ("population", "truth_series", "first_day")) else buf.ctypes.data)
    outs = _lib.EjointOutputs()
    for k in _lib.EJOINT_OUT_NAMES:
        setattr(outs, k, None if k in kw.get("null_out", ()) else buf.ctypes.data)
    ip = None if kw.get("null_inputs") else C.byref(ins)
    op = None if kw.get("null_outputs") else C.byref(outs)
    if fn == "validate":
        rc = lib.epi_ejoint_validate(dp, ip, op, err)
    elif fn == "run_device":
        rc = lib.epi_ejoint_run_device(dp, ip, op, buf.ctypes.data, kw.get("ws_bytes", 0), None, err)
    else:
        rc = lib.epi_ejoint_run_host(dp, ip, op, 0, err)
    return rc, err.value.decode()


BAD_DESC = [
    (dict(null_desc=True), "NULL descriptor"),
    (dict(abi_version=5), "ABI version mismatch"),
    (dict(T=0), "T must be >= 1"),
    (dict(rows=0), "rows must be >= 1"),
    (dict(R=0), "R must be >= 1"),
    (dict(Rt=0), "Rt must be >= 1"),
    (dict(D=0), "D must lie in 1 .. 4096"),
    (dict(D=4097), "D must lie in 1 .. 4096"),
    (dict(R=1 << 20, Rt=1 << 20, D=4096), "R * D is limited to 2^31 - 1"),
    (dict(R=(1 << 30) + 1, Rt=(1 << 30) + 1, D=1, rows=2), "(rows + derive_newcases) * R is limited to 2^31 - 1"),
    (dict(rows=1 << 12, R=1 << 18, Rt=1 << 18, D=4096), "is limited to 2^40"),         # 2^30 items * 2 080 tiles: refused, not cut
    (dict(R=1 << 21, Rt=1 << 21, D=1, T=1 << 20), "is limited to 2^40"),               # items * days
    (dict(k0=-1), "k0, k1 must satisfy 0 <= k0 <= k1 <= T"),
    (dict(k0=4, k1=3), "k0, k1 must satisfy 0 <= k0 <= k1 <= T"),
    (dict(k1=7), "k0, k1 must satisfy 0 <= k0 <= k1 <= T"),
    (dict(storage=2), "storage must be 0 (double) or 1 (float)"),
    (dict(derive_newcases=2), "derive_newcases must be 0 or 1"),
    (dict(derive_newcases=1, rows=2), "derive_newcases needs at least 3 rows"),
    (dict(vs_order=-1), "vs_order must be 0 (no variogram score), 1 (p = 0.5) or 2 (p = 1)"),
    (dict(vs_order=3), "vs_order must be 0 (no variogram score), 1 (p = 0.5) or 2 (p = 1)"),
    (dict(max_lag=-1), "max_lag must be >= 0"),
    (dict(test_launch_tiles=-1), "test_launch_tiles must be >= 0"),
]
BAD_ARGS = [
    (dict(null_inputs=True), "NULL inputs / outputs"),
    (dict(null_outputs=True), "NULL inputs / outputs"),
    (dict(null_in=("src",)), "NULL src"),
    (dict(null_in=("truth",)), "NULL truth"),
    (dict(derive_newcases=1), "NULL population (derive_newcases)"),
    (dict(Rt=3), "without truth_series, truth must hold R columns"),
    (dict(vs_order=0), "vs needs vs_order 1 (p = 0.5) or 2 (p = 1)"),
    (dict(null_out=("es", "truth_term", "spread_term", "vs", "n_members", "n_days", "member_dist")), "no output requested"),
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


def _ws(items, D, wcap):
    nb = (D + 63) // 64
    return items * ((1 + nb * (nb + 1) // 2 + wcap + nb) * 8 + (2 + wcap) * 4)


def test_accepts_and_workspace(hip_lib):
    assert _call("validate") == (0, "")
    assert _call("validate", vs_order=0, null_out=("vs",)) == (0, "")
    assert _call("validate", vs_order=2, max_lag=1 << 30, k0=6, k1=6, storage=1, D=4096)[0] == 0
    assert _call("validate", derive_newcases=1, null_in=("truth_series", "first_day"))[0] == 0
    assert _call("validate", Rt=2, null_in=("population", "first_day"))[0] == 0
    assert _call("validate", null_out=("es", "truth_term", "spread_term", "vs", "n_members", "n_days"))[0] == 0
    assert _call("workspace") == (0, "", _ws(12, 65, 6))
    assert _call("workspace", k0=2, k1=5)[2] == _ws(12, 65, 3)
    assert _call("workspace", T=520, k0=400, k1=520, rows=3, derive_newcases=1, R=300, Rt=300, D=1024)[2] == _ws(1200, 1024, 120) == 1200 * 2672
    assert _call("run_device", ws_bytes=_ws(12, 65, 6) - 1) == (-6, "workspace too small (epi_ejoint_workspace_bytes)")


def test_struct_layouts_symbols_and_constants(hip_lib):
    from epidemicmodeling_amd import _lib
    header = open(os.path.join(H.ROOT, "include", "epiekf.h")).read()
    body = lambda name: re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    fields = lambda txt: [n for decl in re.findall(r"(?:const )?\w+ \*?[^;]*;", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
                          for n in re.findall(r"\*?(\w+)(?:\[\d+\])?\s*[,;]", decl)]
    assert fields(body("epi_ejoint_desc")) == [n for n, _ in _lib.EjointDesc._fields_]
    assert fields(body("epi_ejoint_inputs")) == list(_lib.EJOINT_IN_NAMES) == [n for n, _ in _lib.EjointInputs._fields_]
    assert fields(body("epi_ejoint_outputs")) == list(_lib.EJOINT_OUT_NAMES) == [n for n, _ in _lib.EjointOutputs._fields_]
    assert C.sizeof(_lib.EjointDesc) == 14 * 4
    assert C.sizeof(_lib.EjointInputs) == 5 * 8 and C.sizeof(_lib.EjointOutputs) == 7 * 8
    for sym in ("epi_ejoint_validate", "epi_ejoint_workspace_bytes", "epi_ejoint_run_device", "epi_ejoint_run_host"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(hip_lib, sym) and f"int {sym}(" in header, sym
        assert getattr(hip_lib, sym).restype is C.c_int
    assert "ejoint" not in _lib.FAMILIES
    assert re.search(r"#define\s+EPIEKF_ABI_VERSION\s+6\b", header) and _lib.ABI_VERSION == 6 and hip_lib.epi_abi_version() == 6
    sh = _lib.ejoint_shapes(3, 4, 65, 1)
    assert sh["es"] == sh["vs"] == sh["n_days"] == (4, 4) and sh["member_dist"] == (4, 260) and list(sh) == list(_lib.EJOINT_OUT_NAMES)
    assert _lib.ejoint_out_names(None, 0) == [k for k in _lib.EJOINT_OUT_NAMES if k != "vs"]
    assert _lib.ejoint_out_names(None, 2) == list(_lib.EJOINT_OUT_NAMES)
    assert _lib.ejoint_out_names(("n_days", "es"), 0) == ["es", "n_days"]


def test_python_argument_checks(hip_lib):
    """hostapi.ensemble_joint_score refuses what it can before a device is touched"""
    from epidemicmodeling_amd import hostapi
    T, R, D = 5, 3, 7
    src, truth = np.zeros((T, 2, R * D)), np.zeros((T, 2, R))
    f = hostapi.ensemble_joint_score
    with pytest.raises(ValueError, match="chain-blocked"):
        f(np.zeros((T, 2, 2, 8)), truth, R, D)
    with pytest.raises(ValueError, match=r"src must be \[T, rows, B\] or \[T, B\]"):
        f(np.zeros(R * D), truth, R, D)
    with pytest.raises(ValueError, match="src holds 21 chains, R \\* D = 24"):
        f(src, truth, R, 8)
    with pytest.raises(ValueError, match=r"population must be \[R\]"):
        f(src, truth, R, D, population=np.ones(R + 1))
    with pytest.raises(ValueError, match="truth must be"):
        f(src, np.zeros((T, 3, R)), R, D)
    with pytest.raises(ValueError, match="pass truth_series"):
        f(src, np.zeros((T, 2, 2)), R, D)
    with pytest.raises(ValueError, match="entries in 0 .. Rt-1"):
        f(src, np.zeros((T, 2, 2)), R, D, truth_series=[0, 1, 2])
    with pytest.raises(ValueError, match=r"first_day must be \[R\]"):
        f(src, truth, R, D, first_day=[0])
    with pytest.raises(ValueError, match=r"unknown outputs \['nope'\]"):
        f(src, truth, R, D, outputs=("es", "nope"))
    with pytest.raises(ValueError, match="vs_p must be None, 0.5 or 1"):
        f(src, truth, R, D, vs_p=2)
    with pytest.raises(RuntimeError, match="max_lag must be >= 0"):
        f(src, truth, R, D, vs_p=0.5, max_lag=-1)
    with pytest.raises(RuntimeError, match="vs needs vs_order"):
        f(src, truth, R, D, outputs=("vs",))
    with pytest.raises(RuntimeError, match="k0, k1 must satisfy"):
        f(src, truth, R, D, k0=3, k1=2)
    with pytest.raises(RuntimeError, match="derive_newcases needs at least 3 rows"):
        f(src, np.zeros((T, 3, R)), R, D, population=np.ones(R))


def test_the_device_call_refuses_a_chain_blocked_tensor_with_ensemble_scores_message():
    import inspect

    from epidemicmodeling_amd import batch
    a, b = inspect.getsource(batch.ensemble_score), inspect.getsource(batch.ensemble_joint_score)
    msg = re.search(r'raise ValueError\("src is a chain-blocked tensor.*?"\)', a, re.S).group(0)
    assert msg in b

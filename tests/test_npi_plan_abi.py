"""epi_plan_validate, epi_plan_workspace_bytes and the argument checks of epi_plan_run_device / _run_host through the C ABI (no
GPU needed: every case is rejected before a device is touched), the exported symbols, and the argument checks of the Python
entry points."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import helpers as H


def _desc(**kw):
    from epidemicmodeling_amd import _lib
    args = dict(R=5, P=13, H=30, n_npi=12, prefix_days=0, max_iter=64, max_halvings=30, tol=1e-9)
    args.update({k: v for k, v in kw.items() if k in args})
    d = _lib.make_plan_desc(**args)
    if "abi_version" in kw:
        d.abi_version = kw["abi_version"]
    return d


def _call(fn="validate", **kw):
    from epidemicmodeling_amd import _lib
    d = _desc(**kw)
    lib, err = _lib.lib(), C.create_string_buffer(256)
    dp = None if kw.get("null_desc") else C.byref(d)
    if fn == "validate":
        return lib.epi_plan_validate(dp, err), err.value.decode()
    if fn == "workspace":
        n = C.c_size_t(12345)
        rc = lib.epi_plan_workspace_bytes(dp, C.byref(n), err)
        return rc, err.value.decode(), n.value
    buf = np.ones(4096)                                 # never read: every case here is decided on the descriptor and pointers
    ins = _lib.PlanInputs()
    for k in _lib.PLAN_IN_NAMES:
        setattr(ins, k, buf.ctypes.data)
    for k in kw.get("null_in", ()):
        setattr(ins, k, None)
    outs = _lib.PlanOutputs()
    for k in _lib.PLAN_OUT_NAMES:
        setattr(outs, k, None if k in kw.get("null_out", ()) else buf.ctypes.data)
    ip = None if kw.get("null_inputs") else C.byref(ins)
    op = None if kw.get("null_outputs") else C.byref(outs)
    if fn == "run_device":
        rc = lib.epi_plan_run_device(dp, ip, op, buf.ctypes.data, kw.get("ws_bytes", 0), None, err)
    else:
        rc = lib.epi_plan_run_host(dp, ip, op, 0, err)
    return rc, err.value.decode()


BAD = [
    (dict(null_desc=True), -5, "NULL descriptor"),
    (dict(abi_version=5), -5, "ABI version mismatch"),
    (dict(R=0), -5, "R and P must be >= 1"),
    (dict(P=0), -5, "R and P must be >= 1"),
    (dict(P=-3), -5, "R and P must be >= 1"),
    (dict(H=0), -5, "H must be >= 1"),
    (dict(n_npi=0), -5, "n_npi must lie in 1 .. 12"),
    (dict(n_npi=13), -5, "n_npi must lie in 1 .. 12"),
    (dict(prefix_days=-1), -5, "prefix_days must be >= 0"),
    (dict(max_iter=0), -5, "max_iter must lie in 1 .. 255"),
    (dict(max_iter=256), -5, "max_iter must lie in 1 .. 255"),
    (dict(max_halvings=-1), -5, "max_halvings must lie in 0 .. 30"),
    (dict(max_halvings=31), -5, "max_halvings must lie in 0 .. 30"),
    (dict(tol=-1e-9), -5, "tol must be finite and >= 0"),
    (dict(tol=float("nan")), -5, "tol must be finite and >= 0"),
    (dict(tol=float("inf")), -5, "tol must be finite and >= 0"),
    # index products of 2^31 or more are refused, not cut into launches
    (dict(R=1 << 16, P=1 << 15), -8, "are limited to 2^31 - 1"),
    (dict(R=1 << 12, P=1 << 12, H=128, n_npi=1), -8, "are limited to 2^31 - 1"),            # H * 3 * B = 3 * 2^31
    (dict(R=1 << 12, P=1 << 12, H=11, n_npi=12), -8, "are limited to 2^31 - 1"),            # H * n * B > 2^31
    (dict(R=1 << 12, P=1 << 12, H=1, n_npi=1, max_iter=128), -8, "are limited to 2^31 - 1"),  # max_iter * B = 2^31
    (dict(R=1, P=1, H=(1 << 31) // 3 + 1, n_npi=1), -8, "are limited to 2^31 - 1"),
]
BAD_ARRAYS = [
    (dict(null_inputs=True), -5, "NULL inputs / outputs"),
    (dict(null_outputs=True), -5, "NULL inputs / outputs"),
    (dict(null_in=("sp",)), -5, "NULL sp / u_min / eps"),
    (dict(null_in=("u_min",)), -5, "NULL sp / u_min / eps"),
    (dict(null_in=("eps",)), -5, "NULL sp / u_min / eps"),
    (dict(prefix_days=10, null_in=("J0_prefix",)), -5, "prefix_days > 0 needs J0_prefix and J1_prefix"),
    (dict(prefix_days=10, null_in=("J1_prefix",)), -5, "prefix_days > 0 needs J0_prefix and J1_prefix"),
] + [(dict(null_out=(k,)), -5, "NULL plan / J0 / J1 / F / gap / iters / halvings / status")
     for k in ("plan", "J0", "J1", "F", "gap", "iters", "halvings", "status")]


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
    got = _call("run_device", ws_bytes=need - 1, null_out=("states",))
    assert got[0] == -6 and "workspace too small" in got[1]


def test_validate_accepts_and_workspace_sizes(hip_lib):
    assert _call("validate") == (0, "")
    assert _call("validate", R=1, P=1, H=1, n_npi=1, max_iter=1, max_halvings=0, tol=0.0)[0] == 0
    assert _call("validate", max_iter=255, max_halvings=30, prefix_days=400)[0] == 0
    assert _call("validate", R=300, P=250, H=120)[0] == 0
    assert _call("validate", R=1 << 12, P=1 << 12, H=10, n_npi=12, max_iter=127)[0] == 0   # 10 * 12 * 2^24 < 2^31
    # the second plan, the states of both sides, one mask word a day
    up = lambda v: (v + 255) // 256 * 256
    B = 65
    assert _call("workspace")[2] == up(30 * 12 * B * 8) + 2 * up(30 * 3 * B * 8) + up(30 * B * 4)


def test_symbols_header_and_structs(hip_lib):
    from epidemicmodeling_amd import _lib
    header = open(os.path.join(H.ROOT, "include", "epiekf.h")).read()
    for sym in ("epi_plan_validate", "epi_plan_workspace_bytes", "epi_plan_run_device", "epi_plan_run_host"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(hip_lib, sym) and f"int {sym}(" in header, sym
        assert getattr(hip_lib, sym).restype is C.c_int
    for name in ("epi_plan_desc", "epi_plan_inputs", "epi_plan_outputs"):
        assert f"}} {name};" in header
    assert "#define EPIEKF_ABI_VERSION 6" in header and hip_lib.epi_abi_version() == 6
    assert [n for n, _ in _lib.PlanDesc._fields_] == ["abi_version", "R", "P", "H", "n_npi", "prefix_days", "max_iter", "max_halvings", "tol"]
    assert C.sizeof(_lib.PlanDesc) == 8 * 4 + 8 and _lib.PlanDesc.tol.offset == 32
    assert [n for n, _ in _lib.PlanInputs._fields_] == ["sp", "u_min", "eps", "u_fixed", "u_init", "J0_prefix", "J1_prefix"]
    assert [n for n, _ in _lib.PlanOutputs._fields_] == ["plan", "J0", "J1", "F", "gap", "iters", "halvings", "status", "states", "mu",
                                                         "F_trace"]
    assert C.sizeof(_lib.PlanInputs) == 7 * C.sizeof(C.c_void_p) and C.sizeof(_lib.PlanOutputs) == 11 * C.sizeof(C.c_void_p)
    assert _lib.PLAN_SIM_PRM_COUNT == 48 and "EPI_SIM_PRM_COUNT = 48" in header


def test_python_entry_points_check_their_arguments(hip_lib):
    from epidemicmodeling_amd import hostapi
    from epidemicmodeling_amd._lib import EpiError
    R, P, Hh, n = 3, 4, 5, 12
    sp, um, eps = np.zeros((48, R)), np.zeros((n, R)), np.linspace(0.1, 0.9, P)
    f = hostapi.npi_plan
    with pytest.raises(ValueError, match="sp must be"):
        f(np.zeros((47, R)), um, eps, Hh)
    with pytest.raises(ValueError, match="u_min must be"):
        f(sp, np.zeros((n, R + 1)), eps, Hh)
    with pytest.raises(ValueError, match="eps must be"):
        f(sp, um, eps.reshape(2, 2), Hh)
    with pytest.raises(ValueError, match="u_fixed must be"):
        f(sp, um, eps, Hh, u_fixed=np.zeros((Hh, n, R * P)))
    with pytest.raises(ValueError, match="u_init must be"):
        f(sp, um, eps, Hh, u_init=np.zeros((Hh, n, R)))
    with pytest.raises(ValueError, match="prefix_days > 0 needs"):
        f(sp, um, eps, Hh, prefix_days=3, J0_prefix=np.zeros(R))
    with pytest.raises(ValueError, match="J0_prefix / J1_prefix must be"):
        f(sp, um, eps, Hh, prefix_days=3, J0_prefix=np.zeros(R), J1_prefix=np.zeros(R + 1))
    with pytest.raises(ValueError, match="unknown output"):
        f(sp, um, eps, Hh, outputs=("states", "lambda"))
    with pytest.raises(EpiError, match="max_iter must lie in"):
        f(sp, um, eps, Hh, max_iter=0)
    with pytest.raises(EpiError, match="max_halvings must lie in"):
        f(sp, um, eps, Hh, max_halvings=31)
    with pytest.raises(EpiError, match="tol must be finite"):
        f(sp, um, eps, Hh, tol=-1.0)
    with pytest.raises(EpiError, match="H must be >= 1"):
        f(sp, um, eps, 0)
    with pytest.raises(EpiError, match="n_npi must lie in"):
        f(sp, np.zeros((13, R)), eps, Hh)

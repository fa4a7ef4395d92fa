"""epi_loglik_validate, epi_loglik_workspace_bytes and the argument checks of epi_loglik_run_device / _run_host through the C ABI
(no GPU needed: every case is rejected before a device is touched), the exported symbols, and the argument checks of the Python
entry points."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import helpers as H


def _desc(**kw):
    from epidemicmodeling_amd import _lib
    args = dict(model="SIAlphaModelEKFOptControlled", B=70, T=45, L_=21, obs_type="NEWCASES", r_mode=1, Sx=70, lane_block=0, storage=0,
                k0=0, k1=None, G=0)
    args.update({k: v for k, v in kw.items() if k in args})
    d = _lib.make_loglik_desc(**args)
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
        return lib.epi_loglik_validate(dp, err), err.value.decode()
    if fn == "workspace":
        n = C.c_size_t(12345)
        rc = lib.epi_loglik_workspace_bytes(dp, C.byref(n), err)
        return rc, err.value.decode(), n.value
    buf = np.ones(4096)                                 # never read: every case here is decided on the descriptor and pointers
    ins = _lib.LoglikInputs()
    for k in _lib.LOGLIK_IN_NAMES:
        setattr(ins, k, buf.ctypes.data)
    for k in kw.get("null_in", ()):
        setattr(ins, k, None)
    outs = _lib.LoglikOutputs()
    for k in kw.get("outs", _lib.LOGLIK_OUT_NAMES[:7]):
        setattr(outs, k, buf.ctypes.data)
    ip = None if kw.get("null_inputs") else C.byref(ins)
    op = None if kw.get("null_outputs") else C.byref(outs)
    if fn == "run_device":
        rc = lib.epi_loglik_run_device(dp, ip, op, buf.ctypes.data, kw.get("ws_bytes", 0), None, err)
    else:
        rc = lib.epi_loglik_run_host(dp, ip, op, 0, err)
    return rc, err.value.decode()


BAD = [
    (dict(null_desc=True), -5, "NULL descriptor"),
    (dict(abi_version=5), -5, "ABI version mismatch"),
    (dict(model=6), -5, "unknown model"),
    (dict(model=-1), -5, "unknown model"),
    (dict(obs_type=2), -4, "unknown observation type"),
    (dict(obs_type="DEATHS"), -4, "unknown observation type"),
    (dict(B=0), -5, "B must be >= 1"),
    (dict(T=0), -5, "T must be >= 1"),
    (dict(L_=0), -5, "L must be >= 1"),
    (dict(Sx=0), -5, "Sx must be >= 1"),
    (dict(r_mode=2), -5, "r_mode must be 0"),
    (dict(k0=-1), -5, "the window must satisfy"),
    (dict(k0=45), -5, "the window must satisfy"),
    (dict(k0=10, k1=10), -5, "the window must satisfy"),
    (dict(k0=10, k1=5), -5, "the window must satisfy"),
    (dict(k1=46), -5, "the window must satisfy"),
    (dict(k1=-1), -5, "the window must satisfy"),
    (dict(G=-1), -5, "G must be 0 or divide B"),
    (dict(G=13), -5, "G must be 0 or divide B"),
    (dict(lane_block=-1), -5, "lane_block must lie in 0 .. B"),
    (dict(lane_block=71), -5, "lane_block must lie in 0 .. B"),
    (dict(storage=2), -5, "storage must be 0 (double) or 1 (float)"),
    (dict(reserved=1), -5, "reserved must be 0"),
    (dict(r_mode=0, L_=65), -8, "L too large"),
    (dict(B=2 ** 31 - 1, Sx=1, T=45), -8, "B * ceil(T / 32) is limited"),
]
BAD_ARRAYS = [
    (dict(null_inputs=True), -5, "NULL inputs / outputs"),
    (dict(null_outputs=True), -5, "NULL inputs / outputs"),
    (dict(null_in=("S_MINUS",)), -5, "NULL S_MINUS / P_MINUS / innovations / x / prm"),
    (dict(null_in=("P_MINUS",)), -5, "NULL S_MINUS / P_MINUS / innovations / x / prm"),
    (dict(null_in=("innovations",)), -5, "NULL S_MINUS / P_MINUS / innovations / x / prm"),
    (dict(null_in=("x",)), -5, "NULL S_MINUS / P_MINUS / innovations / x / prm"),
    (dict(null_in=("prm",)), -5, "NULL S_MINUS / P_MINUS / innovations / x / prm"),
    (dict(null_in=("R_series",)), -5, "r_mode 1 needs R_series"),
    (dict(r_mode=0, null_in=("R_scalar",)), -5, "r_mode 0 needs R_scalar"),
    (dict(Sx=5, null_in=("x_series",)), -5, "x_series is NULL: Sx must equal B"),
    (dict(outs=("n_valid", "status")), -5, "no output requested"),
    (dict(outs=("loglik", "best")), -5, "best / best_loglik need G > 0"),
    (dict(outs=("loglik", "best_loglik")), -5, "best / best_loglik need G > 0"),
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
    for model in range(6):
        for st in (0, 1):
            for r_mode in (0, 1):
                assert _call("validate", model=model, storage=st, r_mode=r_mode)[0] == 0
    assert _call("validate", model=5, obs_type=7)[0] == 0               # the codegen model ignores it, as the filter does
    assert _call("validate", B=1, T=1, Sx=1)[0] == 0
    assert _call("validate", lane_block=70)[0] == 0 and _call("validate", lane_block=40)[0] == 0
    assert _call("validate", k0=44, k1=45)[0] == 0 and _call("validate", k0=44, k1=0)[0] == 0
    assert _call("validate", G=14)[0] == 0 and _call("validate", G=70)[0] == 0 and _call("validate", r_mode=0, L_=64)[0] == 0
    # the block sums of ceil(45 / 32) = 2 blocks and the per-chain words; r_mode 0 adds R(k) [T][B]
    up = lambda v: (v + 255) // 256 * 256
    want = 2 * up(2 * 70 * 8) + 2 * up(2 * 70 * 4) + up(70 * 8) + 2 * up(70 * 4)
    assert _call("workspace")[2] == want
    assert _call("workspace", r_mode=0)[2] == want + up(45 * 70 * 8)


def test_symbols_header_and_structs(hip_lib):
    from epidemicmodeling_amd import _lib
    header = open(os.path.join(H.ROOT, "include", "epiekf.h")).read()
    for sym in ("epi_loglik_validate", "epi_loglik_workspace_bytes", "epi_loglik_run_device", "epi_loglik_run_host"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(hip_lib, sym) and f"int {sym}(" in header, sym
        assert getattr(hip_lib, sym).restype is C.c_int
    for name in ("epi_loglik_desc", "epi_loglik_inputs", "epi_loglik_outputs"):
        assert f"}} {name};" in header
    assert "#define EPIEKF_ABI_VERSION 6" in header and hip_lib.epi_abi_version() == 6
    assert "loglik" not in _lib.FAMILIES and len(_lib.FAMILIES) == 9
    assert [n for n, _ in _lib.LoglikDesc._fields_] == ["abi_version", "model", "B", "T", "L", "obs_type", "r_mode", "Sx", "lane_block",
                                                        "storage", "k0", "k1", "G", "reserved"]
    assert C.sizeof(_lib.LoglikDesc) == 14 * 4
    assert [n for n, _ in _lib.LoglikInputs._fields_] == ["S_MINUS", "P_MINUS", "innovations", "x", "R_series", "R_scalar", "x_series", "prm"]
    assert [n for n, _ in _lib.LoglikOutputs._fields_] == ["loglik", "nis_mean", "n_valid", "status", "S", "nis", "R_used", "best",
                                                           "best_loglik"]
    assert C.sizeof(_lib.LoglikInputs) == 8 * C.sizeof(C.c_void_p) and C.sizeof(_lib.LoglikOutputs) == 9 * C.sizeof(C.c_void_p)


def test_python_entry_points_check_their_arguments(hip_lib):
    from epidemicmodeling_amd import hostapi
    from epidemicmodeling_amd._lib import EpiError
    T, B = 6, 4
    sm, pm, e, x, prm = np.zeros((T, 3, B)), np.zeros((T, 9, B)), np.zeros((T, B)), np.zeros((T, B)), np.zeros((61, B))
    f = lambda *a, **k: hostapi.innovation_likelihood(*a, **{"R_series": x, **k})
    with pytest.raises(ValueError, match="unknown model"):
        f(sm, pm, e, x, prm, "SIR")
    with pytest.raises(ValueError, match="has m = 6"):
        f(sm, pm, e, x, prm, "SIAlphaModelEKFOptControlled")
    with pytest.raises(ValueError, match="has m = 3"):
        f(sm, np.zeros((T, 8, B)), e, x, prm, "SIAlphaModelEKF")
    with pytest.raises(ValueError, match="innovations must be"):
        f(sm, pm, np.zeros((T, B + 1)), x, prm, "SIAlphaModelEKF")
    with pytest.raises(ValueError, match="x must be"):
        f(sm, pm, e, np.zeros((T + 1, B)), prm, "SIAlphaModelEKF")
    with pytest.raises(ValueError, match="prm must be"):
        f(sm, pm, e, x, np.zeros((60, B)), "SIAlphaModelEKF")
    with pytest.raises(ValueError, match="exactly one of R_series / R_scalar"):
        f(sm, pm, e, x, prm, "SIAlphaModelEKF", R_scalar=np.ones(B))
    with pytest.raises(ValueError, match="exactly one of R_series / R_scalar"):
        f(sm, pm, e, x, prm, "SIAlphaModelEKF", R_series=None)
    with pytest.raises(ValueError, match="without x_series"):
        f(sm, pm, e, x[:, :2], prm, "SIAlphaModelEKF", R_series=x[:, :2])
    with pytest.raises(ValueError, match="x_series must be"):
        f(sm, pm, e, x, prm, "SIAlphaModelEKF", x_series=np.zeros(B + 1, dtype=np.int32))
    with pytest.raises(ValueError, match="lane_block given with classic"):
        f(sm, pm, e, x, prm, "SIAlphaModelEKF", lane_block=2)
    with pytest.raises(ValueError, match="unknown output"):
        f(sm, pm, e, x, prm, "SIAlphaModelEKF", outputs=("loglik", "aic"))
    with pytest.raises(EpiError, match="the window must satisfy"):
        f(sm, pm, e, x, prm, "SIAlphaModelEKF", k0=3, k1=2)
    with pytest.raises(EpiError, match="G must be 0 or divide B"):
        f(sm, pm, e, x, prm, "SIAlphaModelEKF", G=3)
    with pytest.raises(EpiError, match="best / best_loglik need G > 0"):
        f(sm, pm, e, x, prm, "SIAlphaModelEKF", outputs=("loglik", "best"))
    with pytest.raises(EpiError, match="no output requested"):
        f(sm, pm, e, x, prm, "SIAlphaModelEKF", outputs=("status",))
    with pytest.raises(EpiError, match="unknown observation type"):
        f(sm, pm, e, x, prm, "SIAlphaModelEKF", obs_type="DEATHS")

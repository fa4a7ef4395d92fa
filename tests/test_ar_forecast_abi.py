"""epi_arfc_validate and the argument checks of epi_arfc_run_host, through the C ABI (no GPU needed: every case is rejected
before a device is touched), the exported symbols, and the argument checks of the Python entry points."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import helpers as H

R_, D_, L_, P_, H_ = 3, 4, 20, 2, 5


def _call(fn="validate", **kw):
    from epidemicmodeling_amd import _lib
    args = dict(R=R_, D=D_, L=L_, p=P_, H=H_, dt=1.0, fit=1, nv_mode=0, Sd=0)
    args.update({k: v for k, v in kw.items() if k in args})
    d = _lib.make_arfc_desc(**args)
    if "abi_version" in kw:
        d.abi_version = kw["abi_version"]
    buf = np.ones(4096)                                 # never read: every case here is decided on the descriptor and pointers
    ibuf = np.zeros(4096, dtype=np.int32)
    ins = _lib.ArfcInputs()
    for k in ("seg", "beta", "s0", "i0"):
        setattr(ins, k, buf.ctypes.data)
    for k in kw.get("with_in", ()):
        setattr(ins, k, ibuf.ctypes.data if k == "drive_series" else buf.ctypes.data)
    for k in kw.get("null_in", ()):
        setattr(ins, k, None)
    outs = _lib.ArfcOutputs()
    for k in _lib.ARFC_OUT_NAMES:
        setattr(outs, k, ibuf.ctypes.data if k == "status" else buf.ctypes.data)
    for k in kw.get("null_outs", ()):
        setattr(outs, k, None)
    err = C.create_string_buffer(256)
    dp = None if kw.get("null_desc") else C.byref(d)
    ip = None if kw.get("null_inputs") else C.byref(ins)
    op = None if kw.get("null_outputs") else C.byref(outs)
    lib = _lib.lib()
    rc = lib.epi_arfc_validate(dp, ip, op, err) if fn == "validate" else lib.epi_arfc_run_host(dp, ip, op, 0, err)
    return rc, err.value.decode()


BAD = [
    (dict(null_desc=True), "NULL descriptor"),
    (dict(abi_version=5), "ABI"),
    (dict(R=0), "R must be"),
    (dict(D=0), "D must be"),
    (dict(p=0), "p must lie in 1 .. 32"),
    (dict(p=33, L=100), "p must lie in 1 .. 32"),
    (dict(L=P_), "L must be at least p + 1"),
    (dict(L=P_ + 257), "L - p is limited to 256"),
    (dict(p=32, L=48), "2 (L - p) must be at least p + 1"),
    (dict(H=0), "H must be >= 1"),
    (dict(R=2 ** 16, D=2 ** 15), "R * D is limited"),
    (dict(fit=2), "fit must be"),
    (dict(nv_mode=2), "nv_mode must be"),
    (dict(dt=float("inf")), "dt must be finite"),
    (dict(null_inputs=True), "NULL inputs"),
    (dict(null_outputs=True), "NULL inputs"),
    (dict(null_in=("seg",)), "NULL seg"),
    (dict(null_in=("i0",)), "NULL seg"),
    (dict(fit=0), "fit = 0 needs A and noise_var"),
    (dict(fit=0, with_in=("A",)), "fit = 0 needs A and noise_var"),
    (dict(null_outs=("A_out",)), "fit = 1 needs A_out and noise_var_out"),
    (dict(with_in=("drive",), Sd=0), "Sd must be >= 1"),
    (dict(with_in=("drive",), Sd=5), "drive without drive_series needs Sd == R * D"),
    (dict(null_outs=("S",)), "NULL S output"),
    (dict(R=2, D=2 ** 30), "R * D is limited to 2^31 - 1"),
]


@pytest.mark.parametrize("kw, msg", BAD)
def test_validate_rejects(hip_lib, kw, msg):
    got, text = _call("validate", **kw)
    assert got == -5 and msg in text, (got, text)
    got, text = _call("run_host", **kw)                     # the host entry validates first, before any device work
    assert got == -5 and msg in text, (got, text)


def test_validate_accepts(hip_lib):
    assert _call("validate") == (0, "")
    assert _call("validate", p=1, L=2, H=1, R=1, D=1)[0] == 0
    assert _call("validate", p=32, L=288)[0] == 0
    assert _call("validate", p=32, L=49)[0] == 0
    assert _call("validate", R=2 ** 16, D=2 ** 15 - 1)[0] == 0
    # R * D = 2^31 - 1 itself (a prime: one region of 2^31 - 1 draws, or the transpose) -- the descriptor alone, S would be 144 GiB
    assert _call("validate", R=1, D=2 ** 31 - 1)[0] == 0
    assert _call("validate", R=2 ** 31 - 1, D=1)[0] == 0
    assert _call("validate", fit=0, with_in=("A", "noise_var"), null_outs=("A_out", "noise_var_out", "status"))[0] == 0
    assert _call("validate", null_outs=("status",))[0] == 0
    assert _call("validate", with_in=("drive",), Sd=R_ * D_)[0] == 0
    assert _call("validate", with_in=("drive", "drive_series"), Sd=2)[0] == 0


def test_symbols_header_and_structs(hip_lib):
    from epidemicmodeling_amd import _lib
    header = open(os.path.join(H.ROOT, "include", "epiekf.h")).read()
    for sym in ("epi_arfc_validate", "epi_arfc_run_device", "epi_arfc_run_host"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(hip_lib, sym) and f"int {sym}(" in header, sym
    for name in ("epi_arfc_desc", "epi_arfc_inputs", "epi_arfc_outputs"):
        assert f"}} {name};" in header
    assert "#define EPIEKF_ABI_VERSION 6" in header and hip_lib.epi_abi_version() == 6
    assert C.sizeof(_lib.ArfcDesc) == 10 * 4 + 8 and _lib.ArfcDesc.dt.offset == 40
    assert C.sizeof(_lib.ArfcInputs) == 9 * C.sizeof(C.c_void_p) and C.sizeof(_lib.ArfcOutputs) == 4 * C.sizeof(C.c_void_p)
    assert "NOT PINNED" in header                           # the noise variance's normalisation


def test_python_entry_points_check_their_arguments(hip_lib):
    from epidemicmodeling_amd import batch, hostapi
    from epidemicmodeling_amd._lib import EpiError
    seg, one = np.full((20, 3), 0.3), np.ones(3)
    with pytest.raises(ValueError, match="given together"):
        hostapi.ar_forecast(seg, one, one, one, 1.0, 2, 5, 4, A=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="given together"):
        batch.ar_forecast(seg, one, one, one, 1.0, 2, 5, 4, noise_var=one)
    with pytest.raises(ValueError, match="z must have shape"):
        hostapi.ar_forecast(seg, one, one, one, 1.0, 2, 5, 4, z=np.zeros((5, 11)))
    with pytest.raises(ValueError, match="drive_series without drive"):
        hostapi.ar_forecast(seg, one, one, one, 1.0, 2, 5, 4, drive_series=np.zeros(12))
    with pytest.raises(ValueError, match="0 .. Sd-1"):
        hostapi.ar_forecast(seg, one, one, one, 1.0, 2, 5, 4, drive=np.zeros((5, 2)), drive_series=np.full(12, 2))
    with pytest.raises(EpiError, match="p must lie in 1 .. 32"):
        hostapi.ar_forecast(np.full((100, 3), 0.3), one, one, one, 1.0, 33, 5, 4)
    with pytest.raises(EpiError, match="L - p is limited"):
        hostapi.ar_forecast(np.full((300, 3), 0.3), one, one, one, 1.0, 2, 5, 4)
    with pytest.raises(EpiError, match="H must be"):
        hostapi.ar_forecast(seg, one, one, one, 1.0, 2, 0, 4)

"""epi_escore_validate, epi_escore_workspace_bytes and the argument checks of epi_escore_run_device / _run_host through the C ABI
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
    args = dict(T=6, rows=3, R=4, D=65, Rt=4, alpha=(0.5, 0.05), n_bins=10, storage=0, derive_newcases=0, k0=0, k1=None, test_launch_items=0)
    args.update({k: v for k, v in kw.items() if k in args})
    d = _lib.make_escore_desc(**args)
    for k in ("abi_version", "n_a"):
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
        rc = lib.epi_escore_workspace_bytes(dp, C.byref(n), err)
        return rc, err.value.decode(), n.value
    buf = np.ones(4096)                                 # never read: every case here is decided on the descriptor and pointers
    ins = _lib.EscoreInputs()
    for k in _lib.ESCORE_IN_NAMES:
        setattr(ins, k, None if k in kw.get("null_in", ("population", "truth_series", "first_day")) else buf.ctypes.data)
    outs = _lib.EscoreOutputs()
    for k in _lib.ESCORE_OUT_NAMES:
        setattr(outs, k, None if k in kw.get("null_out", ()) else buf.ctypes.data)
    ip = None if kw.get("null_inputs") else C.byref(ins)
    op = None if kw.get("null_outputs") else C.byref(outs)
    if fn == "validate":
        rc = lib.epi_escore_validate(dp, ip, op, err)
    elif fn == "run_device":
        rc = lib.epi_escore_run_device(dp, ip, op, buf.ctypes.data, kw.get("ws_bytes", 0), None, err)
    else:
        rc = lib.epi_escore_run_host(dp, ip, op, 0, err)
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
    (dict(n_a=-1), "n_a must lie in 0 .. 8"),
    (dict(alpha=(0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1)), "n_a must lie in 0 .. 8"),
    (dict(n_bins=-1), "n_bins must lie in 0 .. 32"),
    (dict(n_bins=33), "n_bins must lie in 0 .. 32"),
    (dict(alpha=(0.0,)), "every alpha must lie in (0, 1)"),
    (dict(alpha=(1.0,)), "every alpha must lie in (0, 1)"),
    (dict(alpha=(0.5, -0.1)), "every alpha must lie in (0, 1)"),
    (dict(alpha=(float("nan"),)), "every alpha must lie in (0, 1)"),
    (dict(alpha=(0.05, 0.5)), "alpha must be strictly descending"),
    (dict(alpha=(0.5, 0.5)), "alpha must be strictly descending"),
    (dict(k0=-1), "k0, k1 must satisfy 0 <= k0 <= k1 <= T"),
    (dict(k0=4, k1=3), "k0, k1 must satisfy 0 <= k0 <= k1 <= T"),
    (dict(k1=7), "k0, k1 must satisfy 0 <= k0 <= k1 <= T"),
    (dict(storage=2), "storage must be 0 (double) or 1 (float)"),
    (dict(derive_newcases=2), "derive_newcases must be 0 or 1"),
    (dict(derive_newcases=1, rows=2), "derive_newcases needs at least 3 rows"),
    (dict(test_launch_items=-1), "test_launch_items must be >= 0"),
]
BAD_ARGS = [
    (dict(null_inputs=True), "NULL inputs / outputs"),
    (dict(null_outputs=True), "NULL inputs / outputs"),
    (dict(null_in=("src",)), "NULL src"),
    (dict(null_in=("truth",)), "NULL truth"),
    (dict(derive_newcases=1), "NULL population (derive_newcases)"),
    (dict(Rt=3), "without truth_series, truth must hold R columns"),
    (dict(n_bins=0), "pit_hist needs n_bins >= 1"),
    (dict(null_out=("crps", "wis", "ae", "width", "rank", "ties", "cover", "count", "crps_mean", "wis_mean", "ae_mean", "n_scored",
                    "cover_frac", "pit_hist")), "no output requested"),
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
    assert _call("validate", alpha=(), n_bins=0, null_out=("pit_hist",)) == (0, "")
    assert _call("validate", k0=6, k1=6, storage=1, D=4096, n_bins=32, alpha=(0.9, 0.8, 0.6, 0.5, 0.3, 0.2, 0.1, 0.05))[0] == 0
    assert _call("validate", derive_newcases=1, null_in=("truth_series", "first_day"))[0] == 0
    assert _call("validate", Rt=2, null_in=("population", "first_day"))[0] == 0
    assert _call("workspace") == (0, "", 6 * 3 * 4 * 40)
    assert _call("workspace", T=400, rows=3, derive_newcases=1, R=300, Rt=300, D=1024)[2] == 400 * 4 * 300 * 40
    assert _call("run_device", ws_bytes=6 * 3 * 4 * 40 - 1) == (-6, "workspace too small (epi_escore_workspace_bytes)")


def test_struct_layouts_symbols_and_constants(hip_lib):
    from epidemicmodeling_amd import _lib
    header = open(os.path.join(H.ROOT, "include", "epiekf.h")).read()
    body = lambda name: re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    fields = lambda txt: [n for decl in re.findall(r"(?:const )?\w+ \*?[^;]*;", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
                          for n in re.findall(r"\*?(\w+)(?:\[\d+\])?\s*[,;]", decl)]
    assert fields(body("epi_escore_desc")) == [n for n, _ in _lib.EscoreDesc._fields_]
    assert fields(body("epi_escore_inputs")) == list(_lib.ESCORE_IN_NAMES) == [n for n, _ in _lib.EscoreInputs._fields_]
    assert fields(body("epi_escore_outputs")) == list(_lib.ESCORE_OUT_NAMES) == [n for n, _ in _lib.EscoreOutputs._fields_]
    assert C.sizeof(_lib.EscoreDesc) == 14 * 4 + 8 * 8 and _lib.EscoreDesc.alpha.offset == 56
    assert C.sizeof(_lib.EscoreInputs) == 5 * 8 and C.sizeof(_lib.EscoreOutputs) == 14 * 8
    for sym in ("epi_escore_validate", "epi_escore_workspace_bytes", "epi_escore_run_device", "epi_escore_run_host"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(hip_lib, sym) and f"int {sym}(" in header, sym
        assert getattr(hip_lib, sym).restype is C.c_int
    assert "escore" not in _lib.FAMILIES
    assert re.search(r"#define\s+EPIEKF_ABI_VERSION\s+6\b", header) and _lib.ABI_VERSION == 6 and hip_lib.epi_abi_version() == 6
    sh = _lib.escore_shapes(6, 3, 4, 2, 10, 1)
    assert sh["crps"] == sh["rank"] == (6, 4, 4) and sh["width"] == (6, 2, 4, 4) and sh["crps_mean"] == sh["n_scored"] == (4, 4)
    assert sh["cover_frac"] == (2, 4, 4) and sh["pit_hist"] == (10, 4, 4) and list(sh) == list(_lib.ESCORE_OUT_NAMES)
    assert _lib.escore_out_names(None, 0) == [k for k in _lib.ESCORE_OUT_NAMES if k != "pit_hist"]
    assert _lib.escore_out_names(("wis_mean", "crps"), 0) == ["crps", "wis_mean"]


def test_python_argument_checks(hip_lib):
    """hostapi.ensemble_score refuses what it can before a device is touched"""
    from epidemicmodeling_amd import hostapi
    T, R, D = 5, 3, 7
    src, truth = np.zeros((T, 2, R * D)), np.zeros((T, 2, R))
    f = hostapi.ensemble_score
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
    with pytest.raises(ValueError, match="truth must be"):
        f(np.zeros((T, 3, R * D)), np.zeros((T, 3, R)), R, D, population=np.ones(R))        # the derived row has a truth row too
    with pytest.raises(ValueError, match="pass truth_series"):
        f(src, np.zeros((T, 2, 2)), R, D)
    with pytest.raises(ValueError, match=r"truth_series must be \[R\]"):
        f(src, np.zeros((T, 2, 2)), R, D, truth_series=[0, 1])
    with pytest.raises(ValueError, match="entries in 0 .. Rt-1"):
        f(src, np.zeros((T, 2, 2)), R, D, truth_series=[0, 1, 2])
    with pytest.raises(ValueError, match=r"first_day must be \[R\]"):
        f(src, truth, R, D, first_day=[0])
    with pytest.raises(ValueError, match=r"unknown outputs \['nope'\]"):
        f(src, truth, R, D, outputs=("crps", "nope"))
    with pytest.raises(RuntimeError, match="alpha must be strictly descending"):
        f(src, truth, R, D, alpha=(0.05, 0.5))
    with pytest.raises(RuntimeError, match="n_bins must lie in"):
        f(src, truth, R, D, n_bins=33)
    with pytest.raises(RuntimeError, match="k0, k1 must satisfy"):
        f(src, truth, R, D, k0=3, k1=2)
    with pytest.raises(RuntimeError, match="pit_hist needs n_bins"):
        f(src, truth, R, D, outputs=("pit_hist",))
    with pytest.raises(RuntimeError, match="derive_newcases needs at least 3 rows"):
        f(src, np.zeros((T, 3, R)), R, D, population=np.ones(R))


def test_pipeline_refusals_need_no_device():
    from epidemicmodeling_amd import pipeline, synth
    raw = synth.make_raw_counts(n_regions=3, T=40, seed=3)
    args = (raw["cases"], raw["deaths"], raw["population"], raw["ip"])
    with pytest.raises(ValueError, match="num_forecast_days must be >= 1"):
        pipeline.fan_quality(*args, 0, (1,))
    with pytest.raises(ValueError, match="starts must hold forecast starts in 1 .. num_forecast_days"):
        pipeline.fan_quality(*args, 10, (11,))
    with pytest.raises(ValueError, match="starts must hold"):
        pipeline.fan_quality(*args, 10, ())

"""epi_ratemap_validate and the argument checks of epi_ratemap_run_host, through the C ABI (no GPU needed: every case is
rejected before a device is touched), and the new symbols in the header, in _lib.ABI_SYMBOLS and in the library."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import helpers as H

T_, N_, R_, E_, K_ = 20, 3, 4, 2, 2
ALL = ("map", "x_mx", "y_filled", "lambda_hat", "new_cases_est", "tracker", "status")


def _call(fn="validate", **kw):
    from epidemicmodeling_amd import _lib
    args = dict(T=T_, n=N_, R=R_, E=E_, K=K_, lags=(3, 5, 7), fit=1, effect_lag=3, ridge=1e-6, lambda_threshold=0.1, reduction_effect=0.01)
    args.update({k: v for k, v in kw.items() if k in args})
    d = _lib.make_ratemap_desc(**args)
    for k in ("abi_version", "n_lags"):
        if k in kw:
            setattr(d, k, kw[k])
    one = np.ones(8)                                        # validate reads n_train alone; the other arrays only have to exist
    nt = np.ascontiguousarray(kw.get("n_train", (5, 20)), dtype=np.int32)
    ins = _lib.RatemapInputs()
    for k in _lib.RATEMAP_IN_NAMES:
        setattr(ins, k, nt.ctypes.data if k == "n_train" else one.ctypes.data)
    for k in kw.get("null_ins", ()):
        setattr(ins, k, None)
    outs = _lib.RatemapOutputs()
    for k in ALL:
        setattr(outs, k, one.ctypes.data)
    for k in kw.get("null_outs", ()):
        setattr(outs, k, None)
    err = C.create_string_buffer(256)
    ip = None if kw.get("null_in") else C.byref(ins)
    op = None if kw.get("null_out") else C.byref(outs)
    dp = None if kw.get("null_desc") else C.byref(d)
    lib = _lib.lib()
    rc = lib.epi_ratemap_validate(dp, ip, op, err) if fn == "validate" else lib.epi_ratemap_run_host(dp, ip, op, 0, err)
    return rc, err.value.decode()


BAD = [
    (dict(null_desc=True), -5, "NULL descriptor"),
    (dict(abi_version=5), -5, "ABI"),
    (dict(T=0), -5, "T must be"),
    (dict(n=0), -5, "n must be"),
    (dict(R=0), -5, "R must be"),
    (dict(E=-1), -5, "E must be"),
    (dict(K=0), -5, "K must be"),
    (dict(n_lags=-1), -5, "n_lags must be"),
    (dict(fit=2), -5, "fit must be 0 or 1"),
    (dict(effect_lag=-1), -5, "effect_lag must be"),
    (dict(ridge=-1.0), -5, "ridge must be finite"),
    (dict(ridge=float("nan")), -5, "ridge must be finite"),
    (dict(ridge=float("inf")), -5, "ridge must be finite"),
    (dict(lambda_threshold=-0.1), -5, "lambda_threshold must be"),
    (dict(lambda_threshold=float("nan")), -5, "lambda_threshold must be"),
    (dict(reduction_effect=float("inf")), -5, "reduction_effect must be finite"),
    (dict(n=25, lags=()), -8, "n is limited to 24"),
    (dict(n_lags=4), -8, "n_lags is limited to 3"),
    (dict(E=9), -8, "E is limited to 8"),
    (dict(n=24, E=1), -8, "is limited to 96"),
    (dict(lags=(3, 0, 7)), -5, "every lag must lie in"),
    (dict(lags=(3, 5, 20)), -5, "every lag must lie in"),
    (dict(K=2 ** 16, R=2 ** 15, n_train=(1,) * 2 ** 16), -5, "K * R must stay below"),
    (dict(T=2 ** 20, R=2 ** 10), -5, "element count"),
    (dict(T=2 ** 11, K=2 ** 10, R=2 ** 10, n_train=(1,) * 2 ** 10), -5, "element count"),
    (dict(null_in=True), -5, "NULL inputs"),
    (dict(null_out=True), -5, "NULL inputs"),
    (dict(null_ins=("ip",)), -5, "NULL ip"),
    (dict(null_ins=("new_smoothed",)), -5, "NULL ip"),
    (dict(null_ins=("n_train",)), -5, "NULL ip"),
    (dict(null_ins=("extra",)), -5, "E > 0 needs extra"),
    (dict(null_ins=("y",)), -5, "fit = 1 needs y"),
    (dict(fit=0, null_ins=("lambda_in",), null_outs=("map",)), -5, "fit = 0 needs lambda_in"),
    (dict(null_outs=ALL), -5, "every output is NULL"),
    (dict(fit=0), -5, "map needs fit = 1"),
    (dict(fit=0, null_ins=("y",), null_outs=("map",)), -5, "y_filled needs y"),
    (dict(n_train=(0, 5)), -5, "every n_train must lie in"),
    (dict(n_train=(5, 21)), -5, "every n_train must lie in"),
]


@pytest.mark.parametrize("kw, rc, msg", BAD)
def test_validate_rejects(hip_lib, kw, rc, msg):
    got, text = _call("validate", **kw)
    assert got == rc and msg in text, (got, text)
    got, text = _call("run_host", **kw)                     # the host entry validates first, before any device work
    assert got == rc and msg in text, (got, text)


def test_validate_accepts(hip_lib):
    assert _call("validate") == (0, "")
    assert _call("validate", n=24, E=0, lags=(1, 2, 19))[0] == 0         # F = 96, the lags at both ends
    assert _call("validate", n=22, E=8)[0] == 0
    assert _call("validate", T=1, lags=(), n_train=(1, 1), ridge=0.0, lambda_threshold=0.0, effect_lag=0)[0] == 0
    assert _call("validate", fit=0, null_ins=("y",), null_outs=("map", "y_filled"))[0] == 0
    assert _call("validate", E=0, null_ins=("extra", "lambda_in"))[0] == 0
    for k in ALL:                                            # every output alone is enough
        assert _call("validate", null_outs=tuple(o for o in ALL if o != k))[0] == 0


def test_symbols_header_and_structs(hip_lib):
    from epidemicmodeling_amd import _build, _lib
    header = open(os.path.join(H.ROOT, "include", "epiekf.h")).read()
    for sym in ("epi_ratemap_validate", "epi_ratemap_run_device", "epi_ratemap_run_host"):
        assert sym in _lib.ABI_SYMBOLS and hasattr(hip_lib, sym) and f"int {sym}(" in header, sym
    for name in ("epi_ratemap_desc", "epi_ratemap_inputs", "epi_ratemap_outputs"):
        assert f"}} {name};" in header
    assert "#define EPIEKF_ABI_VERSION 6" in header and hip_lib.epi_abi_version() == 6
    assert C.sizeof(_lib.RatemapDesc) == 12 * 4 + 3 * 8
    assert [n for n, _ in _lib.RatemapDesc._fields_] == ["abi_version", "T", "n", "R", "E", "K", "n_lags", "lags", "fit", "effect_lag",
                                                         "ridge", "lambda_threshold", "reduction_effect"]
    assert [n for n, _ in _lib.RatemapInputs._fields_] == ["ip", "y", "new_smoothed", "extra", "lambda_in", "n_train"]
    assert [n for n, _ in _lib.RatemapOutputs._fields_] == list(ALL)
    body = header[header.index("typedef struct epi_ratemap_desc"):header.index("int epi_ratemap_validate(")]
    order = [body.index(f) for f in ("abi_version;", " T;", " n;", " R;", " E;", " K;", " n_lags;", " lags[3];", " fit;", " effect_lag;",
                                     " ridge;", " lambda_threshold;", " reduction_effect;", "*ip;", "*y;", "*new_smoothed;", "*extra;",
                                     "*lambda_in;", "*n_train;", "*map;", "*x_mx;", "*y_filled;", "*lambda_hat, *new_cases_est;",
                                     "*tracker;", "*status;")]
    assert order == sorted(order)
    for name, bit in _lib.RATEMAP_STATUS_BITS.items():
        assert f"EPI_RATEMAP_{name.upper()} = {bit}" in header
    assert any(d.endswith("rate_map.hpp") for d in _build.DEPS)


def test_python_entry_points_check_their_arguments(hip_lib):
    from epidemicmodeling_amd import batch, hostapi, pipeline
    from epidemicmodeling_amd._lib import EpiError
    ip, ns, y = np.ones((T_, N_, R_)), np.ones((T_, R_)), np.ones((T_, R_))
    with pytest.raises(ValueError, match="unknown outputs"):
        hostapi.rate_map(ip, ns, [10], y=y, outputs=("map", "slope"))
    with pytest.raises(ValueError, match="no output"):
        hostapi.rate_map(ip, ns, [10], y=y, outputs=())
    with pytest.raises(ValueError, match="ip must be"):
        hostapi.rate_map(ip, ns[:-1], [10], y=y)
    with pytest.raises(ValueError, match="y must be"):
        hostapi.rate_map(ip, ns, [10], y=y[:, :-1])
    with pytest.raises(ValueError, match="y must be"):
        hostapi.rate_map(ip, ns, [10, 12], lambda_in=np.ones((1, T_, R_)))
    with pytest.raises(ValueError, match="is needed"):
        hostapi.rate_map(ip, ns, [10])
    with pytest.raises(ValueError, match="at most 3 lags"):
        hostapi.rate_map(ip, ns, [10], y=y, lags=(1, 2, 3, 4))
    with pytest.raises(ValueError, match="ip must be"):
        batch.rate_map(ip, ns[:, :-1], [10], y=y, device="cpu")
    with pytest.raises(EpiError, match="every n_train must lie in"):
        hostapi.rate_map(ip, ns, [0], y=y)
    with pytest.raises(EpiError, match="every lag must lie in"):
        hostapi.rate_map(ip, ns, [10], y=y, lags=(T_,))
    with pytest.raises(ValueError, match="target must be"):
        pipeline.growth_forecast(np.ones((T_, R_)), np.ones(R_), ip, predict_ahead=5, target="Rt")
    with pytest.raises(ValueError, match="predict_ahead or n_train"):
        pipeline.growth_forecast(np.ones((T_, R_)), np.ones(R_), ip)

"""The one call path of the batched family calls (_lib.FAMILIES, _call.run_family, the two backends).  Without a GPU: what
lib() registers for the 27 family symbols equals the lists written out here, out_names raises its two errors, and hostapi
imports without torch.  On the GPU: for the six families whose device and host entry points share one body, batch.X and
hostapi.X give the same keys in the same order, the same dtypes and shapes and the same bits on the same inputs, with all
outputs and with a single one -- at shapes whose dimensions all differ, so that a swapped field, pointer or shape shows."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from epidemicmodeling_amd import _lib
from tests import helpers as H

P = C.POINTER
# the argument types between the descriptor and the tail, as the C header has them (include/epiekf.h)
FAMILY_ARGS = {
    "rtwin": [P(_lib.RtwinDesc), C.c_void_p, P(_lib.RtwinOutputs)],
    "lasso": [P(_lib.LassoDesc), C.c_void_p, C.c_void_p, C.c_void_p, P(_lib.LassoOutputs)],
    "robfit": [P(_lib.RobfitDesc), C.c_void_p, C.c_void_p, P(_lib.RobfitOutputs)],
    "ratemap": [P(_lib.RatemapDesc), P(_lib.RatemapInputs), P(_lib.RatemapOutputs)],
    "mldiv": [P(_lib.MldivDesc), P(_lib.MldivInputs), P(_lib.MldivOutputs)],
    "svr": [P(_lib.SvrDesc), P(_lib.SvrInputs), P(_lib.SvrOutputs)],
    "ens": [P(_lib.EnsDesc), C.c_void_p, C.c_void_p, P(_lib.EnsOutputs)],
    "arfc": [P(_lib.ArfcDesc), P(_lib.ArfcInputs), P(_lib.ArfcOutputs)],
    "fuse": [P(_lib.FuseDesc), P(_lib.FuseInputs), P(_lib.FuseOutputs)],
}


@pytest.mark.parametrize("fam", sorted(FAMILY_ARGS))
def test_registered_signatures(hip_lib, fam):
    want = {"validate": FAMILY_ARGS[fam] + [C.c_char_p],
            "run_device": FAMILY_ARGS[fam] + [C.c_void_p, C.c_char_p],
            "run_host": FAMILY_ARGS[fam] + [C.c_int, C.c_char_p]}
    for kind, argtypes in want.items():
        fn = getattr(hip_lib, f"epi_{fam}_{kind}")
        assert list(fn.argtypes) == argtypes, (fam, kind)
        assert fn.restype is C.c_int, (fam, kind)


def test_families_are_the_nine_and_name_their_outputs():
    assert sorted(_lib.FAMILIES) == sorted(FAMILY_ARGS)
    for prefix, f in _lib.FAMILIES.items():
        assert f.prefix == prefix
        outs = f.args[-1]._type_
        assert tuple(n for n, _ in outs._fields_) == tuple(f.out_names), prefix
        assert set(f.out_i32) <= set(f.out_names), prefix
        assert all(s in _lib.ABI_SYMBOLS for s in (f"epi_{prefix}_validate", f"epi_{prefix}_run_device", f"epi_{prefix}_run_host"))


def test_older_symbols_keep_their_return_types(hip_lib):
    own = {"epi_ekf_workspace_bytes": C.c_size_t, "epi_preprocess_workspace_bytes": C.c_size_t,
           "epi_lookahead_workspace_bytes": C.c_size_t, "epi_status_string": C.c_char_p, "epi_host_pool_release": None}
    for name in _lib.ABI_SYMBOLS:
        assert getattr(hip_lib, name).restype is own.get(name, C.c_int), name


def test_out_names():
    names = ("a", "b", "c")
    assert _lib.out_names(names, None, ["a", "c"]) == ["a", "c"]
    assert _lib.out_names(names, ("c", "a"), names) == ["c", "a"]
    with pytest.raises(ValueError, match=r"^unknown outputs \['x', 'y'\]$"):
        _lib.out_names(names, ["a", "x", "y"], names)
    with pytest.raises(ValueError, match=r"^no output requested$"):
        _lib.out_names(names, [], names)
    # the four callers: their defaults, and the shared errors
    assert _lib.robfit_out_names(None) == [k for k in _lib.ROBFIT_OUT_NAMES if k != "weights"]
    assert _lib.ratemap_out_names(None, False, False) == [k for k in _lib.RATEMAP_OUT_NAMES if k not in ("map", "y_filled")]
    assert _lib.mldiv_out_names(None) == list(_lib.MLDIV_OUT_NAMES)
    assert _lib.svr_out_names(None, "gaussian") == [k for k in _lib.SVR_OUT_NAMES if k != "w"]
    for call in (lambda o: _lib.robfit_out_names(o), lambda o: _lib.ratemap_out_names(o, True, True), lambda o: _lib.mldiv_out_names(o),
                 lambda o: _lib.svr_out_names(o, "linear")):
        with pytest.raises(ValueError, match=r"unknown outputs \['nope'\]"):
            call(["nope"])
        with pytest.raises(ValueError, match="no output requested"):
            call([])


def test_hostapi_imports_without_torch():
    code = "import sys; import epidemicmodeling_amd.hostapi, epidemicmodeling_amd._call; sys.exit(int('torch' in sys.modules))"
    r = subprocess.run([sys.executable, "-c", code], cwd=H.ROOT, capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])


def _family_inputs():
    """name -> (positional arguments, keyword arguments, (family, one output to ask for alone) or None): every dimension
    another number"""
    rng = np.random.default_rng(11)
    X73, y7 = rng.standard_normal((7, 3, 2)), rng.standard_normal((7, 2))          # D = 7, F = 3, R = 2
    ip = rng.integers(0, 4, (9, 2, 3)).astype(np.float64)                           # T = 9, n = 2, R = 3
    ns = rng.random((9, 3)) * 50.0 + 5.0
    lam = 0.05 * rng.standard_normal((9, 3))
    lam[4, 1] = np.nan                                                              # filled forward: NaN handling on both paths
    extra = rng.standard_normal((9, 1, 3))                                          # E = 1
    X82, y8 = rng.random((8, 2, 3)), rng.random((8, 3))                             # D = 8, n = 2, R = 3
    cases = rng.random((12, 2)) * 100.0 + 10.0                                      # L = 12, R = 2
    cases[3, 1] = np.nan
    return {
        "mldivide": ((X73, y7), dict(n_rows=[4, 7]), ("mldiv", "rank")),
        "svr": ((X73, y7), dict(n_rows=[4, 7]), ("svr", "n_sv")),
        "rate_map": ((ip, ns, [5, 8]), dict(y=lam, extra=extra, lags=(1, 2)), ("ratemap", "tracker")),
        "robust_affine_fit": ((X82, y8), {}, ("robfit", "iters")),
        "lasso_cv": ((X82, y8), dict(K=2, seed=3, num_lambda=5), None),             # lasso_cv has no outputs argument
        "rt_window": ((cases, 5), dict(generation_period=4), None),                 # rt_window selects by method
    }


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mldivide", "svr", "rate_map", "robust_affine_fit", "lasso_cv", "rt_window"])
def test_device_and_host_entry_agree(gpu_device, name):
    import torch
    from epidemicmodeling_amd import batch, hostapi
    args, kw, one = _family_inputs()[name]
    # the second run asks for one output; the two calls without an `outputs` argument narrow their set the way they can:
    # rt_window by method (the four arrays of GenRatios), lasso_cv by K = 0 (the path without the cross-validation)
    if one is not None:
        kw = dict(kw, outputs=list(_lib.FAMILIES[one[0]].out_names))       # all of them, not the default selection
        second, keys = dict(kw, outputs=[one[1]]), [one[1]]
    elif name == "rt_window":
        second, keys = dict(kw, methods=("GenRatios",)), ["gr_Rt", "gr_Lambda", "gr_RtSmoothed", "gr_LambdaSmoothed"]
    else:
        second, keys = dict(kw, K=0), ["lambda", "B", "intercept", "df", "iters", "status"]
    for k, want_keys in ((kw, kw.get("outputs")), (second, keys)):
        dev = getattr(batch, name)(*args, device=gpu_device, **k)
        torch.cuda.synchronize()
        host = getattr(hostapi, name)(*args, device=0, **k)
        assert list(dev) == list(host), (name, list(dev), list(host))
        assert want_keys is None or list(dev) == want_keys, (name, list(dev))
        for key, h in host.items():
            d = dev[key].cpu().numpy()
            assert d.dtype == h.dtype and d.shape == h.shape and d.size > 0, (name, key, d.dtype, h.dtype, d.shape, h.shape)
            assert d.tobytes() == h.tobytes(), (name, key)          # bit for bit, NaNs included

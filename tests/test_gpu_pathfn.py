"""The path functionals on the device (epi_pathfn_run_device / _host, batch.path_functionals, hostapi.path_functionals,
pipeline.path_outlook): every output equal bit for bit (every NaN one value) to the sequential C restatement tests/pathfn_ref.c of
DESIGN.md §4.18.  Outputs start as a finite sentinel and carry guard elements behind them; no sentinel survives a call."""
import ctypes as C

import numpy as np
import pytest

from tests import pathfn_ref as S

pytestmark = pytest.mark.gpu

FILL, I32_FILL, GUARD = -98765.4321, -12345, 8


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return S.PathfnC(tmp_path_factory.mktemp("pathfn_ref"))


@pytest.fixture(scope="module")
def base(cref):
    """the base shape in both storages with its reference, computed once and left unchanged"""
    res = {}
    for storage in ("f64", "f32"):
        kw = S.base_case(storage=storage)
        res[storage] = (kw, cref.functionals(**kw))
    return res


def _run_device(src, R, D, thr=None, population=None, first_day=None, k0=0, k1=None, names=None, device="cuda:0", calls=1,
                test_segments=0, test_launch_groups=0):
    """epi_pathfn_run_device `calls` times back to back on sentinel-filled outputs with GUARD elements behind each; returns one
    dict per call (NumPy), the outputs not named (never handed to the library) included"""
    import torch
    from epidemicmodeling_amd import _lib
    dev = torch.device(device)
    put = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)
    sd = torch.as_tensor(np.ascontiguousarray(src), device=dev)
    n_thr = 0 if thr is None else len(thr)
    ins_t = (sd, put(population, np.float64), put(thr, np.float64), put(first_day, np.int32))
    T, rows, _ = src.shape
    d = _lib.make_pathfn_desc(T, rows, R, D, n_thr, storage=1 if src.dtype == np.float32 else 0, derive_newcases=int(population is not None),
                              k0=k0, k1=k1, test_segments=test_segments, test_launch_groups=test_launch_groups)
    shapes = _lib.pathfn_shapes(rows, R, D, n_thr, d.k1 - d.k0, d.derive_newcases)
    names = _lib.pathfn_out_names(None, n_thr) if names is None else names
    ins = _lib.PathfnInputs()
    for k, v in zip(_lib.PATHFN_IN_NAMES, ins_t):
        setattr(ins, k, None if v is None else C.c_void_p(v.data_ptr()))
    st = torch.cuda.current_stream(dev)
    err = C.create_string_buffer(256)
    n = C.c_size_t(0)
    _lib.check(_lib.lib().epi_pathfn_workspace_bytes(C.byref(d), C.byref(n), err), err)
    runs = []
    for _ in range(calls):
        ws = torch.full(((n.value + 7) // 8 + GUARD,), FILL, dtype=torch.float64, device=dev)   # n is a multiple of 4, not always of 8
        flat = {k: torch.full((int(np.prod(sh)) + GUARD,), I32_FILL if k in _lib.PATHFN_OUT_I32 else FILL,
                              dtype=torch.int32 if k in _lib.PATHFN_OUT_I32 else torch.float64, device=dev) for k, sh in shapes.items()}
        outs = _lib.PathfnOutputs()
        for k in _lib.PATHFN_OUT_NAMES:
            setattr(outs, k, C.c_void_p(flat[k].data_ptr()) if k in names else None)
        rc = _lib.lib().epi_pathfn_run_device(C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(ws.data_ptr()), n.value,
                                              C.c_void_p(st.cuda_stream), err)
        _lib.check(rc, err)
        runs.append((flat, ws))
    torch.cuda.synchronize(dev)
    res = []
    for flat, ws in runs:
        assert (ws[-GUARD:].cpu().numpy() == FILL).all(), "workspace guard elements overwritten"
        out = {}
        for k, sh in shapes.items():
            a = flat[k].cpu().numpy()
            fill = I32_FILL if k in _lib.PATHFN_OUT_I32 else FILL
            assert (a[len(a) - GUARD:] == fill).all(), f"{k}: guard elements overwritten"
            out[k] = a[:len(a) - GUARD].reshape(sh)
            if k in names:
                assert not (out[k] == fill).any(), f"{k}: a poisoned word survived"
        res.append(out)
    return res if calls > 1 else res[0]


def _same(got, want, names=S.NAMES):
    for k in names:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        if not S.same_bits(g, w):
            bad = ~((g == w) | (np.isnan(g) & np.isnan(w))) if g.dtype == np.float64 else g != w
            raise AssertionError((k, np.argwhere(bad)[:4].tolist(), g[bad][:4], w[bad][:4]))


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("segments", [1, 2, 3])
def test_base_shape_equals_reference_for_every_segment_count(gpu_device, base, storage, segments):
    kw, want = base[storage]
    got = _run_device(device=gpu_device, test_segments=segments, **kw)
    _same(got, want)
    # the planted cases, by hand (tests/test_pathfn_ref.py holds the reference to the same)
    W = kw["k1"] - kw["k0"]
    assert np.isnan(got["peak_value"][1, 2]) and got["n_valid"][1, 2] == 0 and np.isnan(got["total"][3, 2])
    assert got["peak_value"][0, 4] == np.inf and got["min_value"][0, 5] == -np.inf
    assert got["peak_day"][0, 6] == 12 and got["first_cross"][0, 0, 7] == 30 and got["days_above"][0, 0, 7] == 1
    assert got["longest_run"][0, 0, 3] == 14 and got["longest_run"][0, 0, 8] == W
    assert (got["days_above"][1, 2, :70] == got["n_valid"][2, :70]).all() and np.isnan(got["first_cross"][2, 1]).all()
    assert (got["n_paths"][:, 2] == 0).all() and (got["n_valid"][:, 140:] == 0).all()


def test_the_library_rule_equals_reference(gpu_device, base):
    kw, want = base["f64"]
    _same(_run_device(device=gpu_device, **kw), want)


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_whole_wavefronts_without_thresholds(gpu_device, cref, storage):
    kw = S.base_case(storage=storage, D=64, n_thr=0, seed=2)
    want = cref.functionals(**kw)
    for segments in (1, 3):
        got = _run_device(device=gpu_device, test_segments=segments, **kw)
        _same(got, want)
    assert got["first_cross"].shape == (0, 4, 192) and got["cross_day_hist"].shape == (67, 0, 4, 3)


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_two_dimensional_source_with_eight_thresholds(gpu_device, cref, storage):
    import torch
    from epidemicmodeling_amd import batch
    kw = S.base_case(storage=storage, rows=1, n_thr=8, derive=False, seed=3)
    want = cref.functionals(**kw)
    for segments in (1, 2):
        _same(_run_device(device=gpu_device, test_segments=segments, **kw), want)
    res = batch.path_functionals(torch.as_tensor(kw["src"][:, 0], device=gpu_device), 3, 70, thresholds=kw["thr"][:, 0], first_day=kw["first_day"],
                                 k0=kw["k0"], k1=kw["k1"])
    assert tuple(res["peak_day"].shape) == (210,) and tuple(res["first_cross"].shape) == (8, 210) and tuple(res["cross_day_hist"].shape) == (67, 8, 3)
    _same({k: v.cpu().numpy() for k, v in res.items()}, {k: v.reshape(v.shape[:-2] + v.shape[-1:]) for k, v in want.items()})


def test_more_rows_than_the_derived_group(gpu_device, cref):
    kw = S.base_case(rows=5, T=70, k0=0, k1=70, D=33, n_thr=2, seed=4)
    want = cref.functionals(**kw)
    for segments in (1, 3):
        _same(_run_device(device=gpu_device, test_segments=segments, **kw), want)


def test_launch_cut_equals_the_uncut_call(gpu_device, base):
    kw, want = base["f32"]
    for segments in (1, 2):
        _same(_run_device(device=gpu_device, test_launch_groups=1, test_segments=segments, **kw), want)


def test_each_output_alone(gpu_device, base):
    """each output asked for alone equals its slice of the full call: the histograms then read the workspace"""
    from epidemicmodeling_amd import _lib
    kw, want = base["f64"]
    for segments in (1, 3):
        for name in _lib.PATHFN_OUT_NAMES:
            got = _run_device(device=gpu_device, names=(name,), test_segments=segments, **kw)
            _same(got, want, names=(name,))
            for k in S.NAMES:
                if k != name:
                    assert (got[k] == (I32_FILL if k in S.I32 else FILL)).all(), (name, k)


def test_repeat_call_on_one_stream(gpu_device, base):
    kw, want = base["f64"]
    a, b = _run_device(device=gpu_device, calls=2, test_segments=2, **kw)
    _same(a, b)
    _same(a, want)


def test_batch_equals_hostapi(gpu_device, base):
    import torch
    from epidemicmodeling_amd import batch, hostapi
    for storage in ("f64", "f32"):
        kw, want = base[storage]
        args = dict(thresholds=kw["thr"], population=kw["population"], first_day=kw["first_day"], k0=kw["k0"], k1=kw["k1"])
        got = hostapi.path_functionals(kw["src"], 3, 70, **args)
        dev = batch.path_functionals(torch.as_tensor(kw["src"], device=gpu_device), 3, 70, test_segments=2, **args)
        assert list(got) == list(dev) == list(S.NAMES)
        _same(got, {k: v.cpu().numpy() for k, v in dev.items()})
        _same(got, want)
    res = batch.path_functionals(torch.as_tensor(kw["src"], device=gpu_device), 3, 70, outputs=("total", "peak_day_hist"), **args)
    assert list(res) == ["total", "peak_day_hist"]
    _same({k: v.cpu().numpy() for k, v in res.items()}, want, names=("total", "peak_day_hist"))
    blocked = torch.zeros((5, 25, 3, 8), device=gpu_device)
    with pytest.raises(ValueError, match="EkfRunner.unblocked"):
        batch.path_functionals(blocked, 3, 70)


def test_path_outlook_end_to_end(gpu_device):
    import torch
    from epidemicmodeling_amd import pipeline, synth
    B, T, D, k0 = 4, 40, 65, 8
    w = synth.make_cfg3(B, T)
    N = np.linspace(1e6, 5e6, B)
    q = (0.1, 0.5, 0.9)
    r, X, summ, z = pipeline.smoothed_fan(w, D, q=q, population=N, seed=5, k0=k0, device=gpu_device)
    Xh = X.cpu().numpy()
    new = S.rows_with_derived(Xh, N, B, D)[:, 3]
    thr = np.full((2, 4, B), np.nan)
    thr[0, 3], thr[1, 3] = np.nanquantile(new.reshape(-1, B, D), 0.5, axis=(0, 2)), np.nanquantile(new.reshape(-1, B, D), 0.95, axis=(0, 2))
    out = pipeline.path_outlook(X, B, D, thr, population=N, q=q, k0=2, k1=T - k0)
    fn = {k: v.cpu().numpy() for k, v in out["functionals"].items()}
    _same(fn, S.functionals(Xh, B, D, thr, population=N, k0=2, k1=T - k0))
    # the quantiles of the peak day over the draws: MATLAB's quantile of the copied-back paths in NumPy
    pd = fn["peak_day"].reshape(4, B, D)
    got = out["peak_day"]["quantiles"].cpu().numpy()                     # [rows', n_q, B]
    for k, p in enumerate(q):
        x = np.sort(pd, axis=2)
        h = D * p + 0.5
        kf = int(np.floor(h))
        want = x[..., kf - 1] + (h - kf) * (x[..., kf] - x[..., kf - 1])
        assert np.array_equal(got[:, k], want), p
    pc = out["p_cross_by_day"].cpu().numpy()                             # [W, n_thr, rows', B]
    assert pc.shape == (T - k0 - 2, 2, 4, B) and (np.diff(pc[:, :, 3], axis=0) >= 0).all()
    assert np.array_equal(pc[-1, :, 3], fn["n_cross"][:, 3] / fn["n_paths"][3])
    pp = out["p_peak_by_day"].cpu().numpy()
    assert (np.diff(pp, axis=0) >= 0).all() and np.allclose(pp[-1], 1.0)
    assert np.isnan(out["days_above"]["mean"].cpu().numpy()[:, :3]).all() and np.isfinite(out["days_above"]["mean"].cpu().numpy()[:, 3]).all()


def test_forecast_outlook_end_to_end(gpu_device):
    from epidemicmodeling_amd import pipeline, synth
    Sg, T, Hh, D = 4, 120, 21, 32
    raw = synth.make_raw_counts(n_regions=Sg, T=T, seed=3)
    raw["cases"][:, -1] = np.cumsum(np.full(T, 40.0))                # the all-NaN region of the generator: give it data
    N = np.asarray(raw["population"], dtype=np.float64)
    thr = np.full((1, 4, Sg), np.nan)
    thr[0, 3] = 10.0 * N / 1e5                                       # ten daily new cases per 100 000 inhabitants
    out = pipeline.forecast_outlook(raw["cases"], raw["deaths"], N, raw["ip"], Hh, thr, n_draws=D, seed=4, device=gpu_device)
    X = out["X"].cpu().numpy()
    assert X.shape == (Hh, 3, Sg * D)
    ol = out["outlook"]
    _same({k: v.cpu().numpy() for k, v in ol["functionals"].items()}, S.functionals(X, Sg, D, thr, population=N))
    assert tuple(ol["p_cross_by_day"].shape) == (Hh, 1, 4, Sg) and tuple(ol["total"]["mean"].shape) == (4, Sg)
    cnt = ol["days_above"]["count"].cpu().numpy()
    assert (cnt[0, 3] == ol["functionals"]["n_paths"][3].cpu().numpy()).all() and (cnt[0, :3] == 0).all()


def test_counts_alone_over_a_window_longer_than_the_bins(gpu_device, cref):
    """only the histograms bound the window: the per-path outputs and the two counts run over 4 200 days"""
    from epidemicmodeling_amd import _lib
    rng = np.random.default_rng(8)
    src = rng.standard_normal((4200, 1, 6))
    src[:, 0, 4] = np.nan
    thr = np.array([[[1.5, 9.0]]])
    want = cref.functionals(src, 2, 3, thr)
    names = [k for k in _lib.PATHFN_OUT_NAMES if not k.endswith("_hist")]
    for segments in (1, 5):
        _same(_run_device(src, 2, 3, thr, names=names, device=gpu_device, test_segments=segments), want, names=names)
    assert list(want["n_paths"][0]) == [3, 2] and list(want["n_cross"][0, 0]) == [3, 0]
    with pytest.raises(_lib.EpiError, match="at most 4096 days"):
        _run_device(src, 2, 3, thr, device=gpu_device)


def test_a_workspace_that_ends_on_half_a_double(gpu_device, cref):
    """The shape a random hunt met (tests/test_gpu_fuzz_calls.py, seed 18 of its first run): 68 days in the library's own
    three segments, 5 rows' x 63 paths, two thresholds.  The workspace's int32 tail then holds an odd number of words, so its
    size is a multiple of 4 and not of 8, and a helper that sized the guarded workspace with bytes // 8 took the call's last
    word for a write behind its end.  Every output against the C restatement; the guards hold."""
    import ctypes as C
    from epidemicmodeling_amd import _lib
    rng = np.random.default_rng(18)
    T, rows, R, D = 68, 4, 1, 63
    src = rng.standard_normal((T, rows, R * D)) * 10.0 ** rng.uniform(-2, 2, size=(T, rows, 1))
    pop = np.array([2.0e4])
    thr = rng.standard_normal((2, rows + 1, R))
    kw = dict(src=src, R=R, D=D, thr=thr, population=pop, first_day=np.array([18], dtype=np.int32), k0=0, k1=T)
    d = _lib.make_pathfn_desc(T, rows, R, D, 2, storage=0, derive_newcases=1, k0=0, k1=T)
    n, err = C.c_size_t(0), C.create_string_buffer(256)
    _lib.check(_lib.lib().epi_pathfn_workspace_bytes(C.byref(d), C.byref(n), err), err)
    assert n.value % 8 == 4
    _same(_run_device(device=gpu_device, **kw), cref.functionals(**kw))

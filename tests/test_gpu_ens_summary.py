"""The Monte-Carlo ensemble statistics on the device (epi_ens_run_device / _host, batch.ensemble_summary, hostapi.
ensemble_summary, pipeline.monte_carlo_eks): every output equal, as values and with NaN matching NaN, to the NumPy
restatement tests/ens_summary_ref.py.  Outputs start as a finite sentinel and carry guard elements behind them."""
import ctypes as C

import numpy as np
import pytest

from tests import ens_summary_ref as E

pytestmark = pytest.mark.gpu

FILL, I32_FILL, GUARD = -98765.4321, -12345, 8
Q16 = (0.0, 1.0, 0.5, 1.0 / 3.0, 0.025, 0.25, 0.75, 0.975, 0.01, 0.99, 0.1, 0.9, 0.2, 0.8, 2.0 / 3.0, 0.6)
R_, T_, ROWS_ = 3, 2, 3
# the draws per item of the shape grid: every register count NV = P / 64 of the dispatch in epi_ens_run_device (P the power of
# two >= D) and both sides of each of its `<=` (test_the_grid_reaches_every_instantiation)
GRID_D = [1, 2, 3, 63, 64, 65, 127, 128, 129, 256, 257, 300, 512, 513, 1000, 1024, 1025, 2000, 2048, 2049, 4095, 4096]


def _run_device(src, R, D, q, population=None, names=None, device="cuda:0", calls=1):
    """epi_ens_run_device `calls` times back to back on sentinel-filled outputs with GUARD elements behind each; returns
    one dict per call (NumPy), the outputs not named (never handed to the library) included"""
    import torch
    from epidemicmodeling_amd import _lib
    dev = torch.device(device)
    sd = torch.as_tensor(np.ascontiguousarray(src), device=dev)
    pd = None if population is None else torch.as_tensor(np.ascontiguousarray(population, dtype=np.float64), device=dev)
    T, rows, _ = src.shape
    d = _lib.make_ens_desc(T, rows, R, D, q, storage=1 if src.dtype == np.float32 else 0, derive_newcases=int(pd is not None))
    shapes = _lib.ens_shapes(T, rows, R, d.n_q, d.derive_newcases)
    names = _lib.ENS_OUT_NAMES if names is None else names
    st = torch.cuda.current_stream(dev)
    err = C.create_string_buffer(256)
    runs = []
    for _ in range(calls):
        flat = {k: (torch.full((int(np.prod(sh)) + GUARD,), I32_FILL, dtype=torch.int32, device=dev) if k == "count" else
                    torch.full((int(np.prod(sh)) + GUARD,), FILL, dtype=torch.float64, device=dev)) for k, sh in shapes.items()}
        outs = _lib.EnsOutputs()
        for k in _lib.ENS_OUT_NAMES:
            setattr(outs, k, C.c_void_p(flat[k].data_ptr()) if k in names else None)
        rc = _lib.lib().epi_ens_run_device(C.byref(d), C.c_void_p(sd.data_ptr()), None if pd is None else C.c_void_p(pd.data_ptr()),
                                           C.byref(outs), C.c_void_p(st.cuda_stream), err)
        _lib.check(rc, err)
        runs.append(flat)
    torch.cuda.synchronize(dev)
    res = []
    for flat in runs:
        out = {}
        for k, sh in shapes.items():
            a = flat[k].cpu().numpy()
            assert (a[-GUARD:] == (I32_FILL if k == "count" else FILL)).all(), f"{k}: guard elements overwritten"
            out[k] = a[:-GUARD].reshape(sh)
        res.append(out)
    return res if calls > 1 else res[0]


def _same(got, want, names=("mean", "std", "min", "max", "quantiles", "count")):
    for k in names:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (k, g.shape, w.shape)
        if k == "count":
            assert np.array_equal(g, w), k
        else:
            bad = ~((g == w) | (np.isnan(g) & np.isnan(w)))
            assert not bad.any(), (k, np.argwhere(bad)[:4].tolist(), g[bad][:4], w[bad][:4])


def _source(D, storage, seed, R=R_, T=T_, rows=ROWS_):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((T, rows, R * D)) * 10.0 ** rng.uniform(-2, 2, size=(T, rows, 1))
    return s.astype(np.float32) if storage == "f32" else s


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("D", GRID_D)
def test_shape_grid_equals_reference(gpu_device, D, storage):
    src = _source(D, storage, seed=D)
    for q in ((1.0 / 3.0,), Q16):
        got = _run_device(src, R_, D, q, device=gpu_device)
        _same(got, E.summary(src, R_, D, q))
        assert (got["count"] == D).all()


def test_the_grid_reaches_every_instantiation():
    """what the shape grid above covers of epi_ens_run_device's dispatch (D <= 64: ens_summary<1>, <= 128: <2>, ... <= 2048:
    <32>, else <64>): every instantiation is launched, by more than one D where the range allows, and every threshold has a D
    on it and a D one beyond it; the planted members run NV = 8 and NV = 32 too"""
    nv = lambda D: max(64, 1 << (D - 1).bit_length()) // 64
    assert {nv(D) for D in GRID_D} == {1, 2, 4, 8, 16, 32, 64}
    for edge in (64, 128, 256, 512, 1024, 2048):
        assert edge in GRID_D and edge + 1 in GRID_D and nv(edge + 1) == 2 * nv(edge), edge
    assert 1 in GRID_D and 4096 in GRID_D and 4095 in GRID_D                # validate's ends: 1 .. kEnsMaxD
    for n in (8, 32):
        assert any(nv(D) == n and D % 64 for D in GRID_D), n                # with a partly filled last register
    assert {nv(D) for D in (64, 65, 300, 1000, 2000)} == {1, 2, 8, 16, 32}  # test_planted_members


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("D", [64, 65, 300, 1000, 2000])
def test_planted_members(gpu_device, D, storage):
    src = _source(D, storage, seed=100 + D)
    big = 300 if storage == "f64" else 30
    item = lambda t, row, r: src[t, row, r * D:(r + 1) * D]          # a view: assignments plant into src
    item(0, 0, 0)[D // 3] = np.nan                                   # one NaN
    item(0, 0, 1)[np.arange(D) != D - 2] = np.nan                    # D - 1 NaNs
    item(0, 1, 0)[:] = np.nan                                        # all NaN, this item only
    item(0, 1, 1)[[1, D - 1]] = [np.inf, -np.inf]                    # both infinities
    item(0, 2, 0)[3:3 + min(D - 3, 70)] = 1.25                       # a run of equal values (longer than a wavefront where D allows)
    item(0, 2, 1)[:] = (10.0 ** np.linspace(-big, big, D) * np.where(np.arange(D) % 2, -1.0, 1.0))[np.random.default_rng(D).permutation(D)]
    item(1, 0, 0)[[0, 5, 6, 7]] = [-0.0, 0.0, -0.0, 0.0]             # zeros of both signs
    item(1, 0, 1)[:] = 0.0
    item(1, 0, 1)[::2] = -0.0
    item(1, 1, 2)[[0, 2]] = np.inf                                   # +Inf twice: a quantile between them is Inf - Inf
    got = _run_device(src, R_, D, Q16, device=gpu_device)
    want = E.summary(src, R_, D, Q16)
    _same(got, want)
    assert got["count"][0, 0, 0] == D - 1 and got["count"][0, 0, 1] == 1 and got["count"][0, 1, 0] == 0
    assert got["std"][0, 0, 1] == 0.0 and np.isnan(got["mean"][0, 1, 0]) and np.isnan(got["quantiles"][0, :, 1, 0]).all()
    assert np.isnan(got["mean"][0, 1, 1]) and got["min"][0, 1, 1] == -np.inf and got["max"][0, 1, 1] == np.inf
    assert got["count"][0, 1, 1] == D and not np.isnan(got["mean"][0, 1, 2])             # the neighbours of the planted items


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("D", [65, 1000])
def test_derived_row(gpu_device, D, storage):
    rng = np.random.default_rng(D)
    src = np.abs(_source(D, storage, seed=200 + D))
    pop = rng.uniform(1e5, 1e8, R_)
    src[1, 1, D + 3] = np.nan                                        # NaN in one factor of one chain of region 1
    got = _run_device(src, R_, D, Q16, population=pop, device=gpu_device)
    _same(got, E.summary(src, R_, D, Q16, population=pop))
    s = src.astype(np.float64)
    new = ((np.repeat(pop, D)[None, :] * s[:, 0]) * s[:, 1]) * s[:, 2]                    # the look-ahead study's association
    assert got["count"][1, 3, 1] == D - 1 and got["count"][1, 1, 1] == D - 1 and got["count"][1, 0, 1] == D
    for r in range(R_):
        x = new[0, r * D:(r + 1) * D]
        assert got["min"][0, 3, r] == x.min() and got["max"][0, 3, r] == x.max()
        assert got["quantiles"][0, 2, 3, r] == E.item(x, (0.5,))["quantiles"][0]


def test_optional_outputs(gpu_device):
    import torch
    from epidemicmodeling_amd import batch
    D = 129
    src = _source(D, "f64", seed=7)
    got = _run_device(src, R_, D, Q16, names=("count", "quantiles"), device=gpu_device)
    _same(got, E.summary(src, R_, D, Q16), names=("count", "quantiles"))
    for k in ("mean", "std", "min", "max"):
        assert (got[k] == FILL).all(), k
    got = _run_device(src, R_, D, Q16, names=("count", "mean"), device=gpu_device)       # no order statistic wanted
    _same(got, E.summary(src, R_, D, Q16), names=("count", "mean"))
    assert (got["quantiles"] == FILL).all() and (got["min"] == FILL).all()
    res = batch.ensemble_summary(torch.as_tensor(src, device=gpu_device), R_, D, q=Q16, outputs=("quantiles",))
    assert set(res) == {"quantiles", "count"}
    _same({k: v.cpu().numpy() for k, v in res.items()}, E.summary(src, R_, D, Q16), names=("count", "quantiles"))


def test_repeat_call_on_one_stream(gpu_device):
    D = 1000
    src = _source(D, "f32", seed=11)
    a, b = _run_device(src, R_, D, Q16, device=gpu_device, calls=2)
    _same(a, b)
    _same(a, E.summary(src, R_, D, Q16))


def test_batch_entry_point_and_two_dimensional_source(gpu_device):
    import torch
    from epidemicmodeling_amd import batch
    D = 65
    src = _source(D, "f64", seed=13)
    want = E.summary(src, R_, D, (0.025, 0.25, 0.5, 0.75, 0.975))
    res = batch.ensemble_summary(torch.as_tensor(src, device=gpu_device), R_, D)
    _same({k: v.cpu().numpy() for k, v in res.items()}, want)
    res = batch.ensemble_summary(torch.as_tensor(src[:, 1], device=gpu_device), R_, D)      # [T, B]: one row, no row axis
    assert tuple(res["mean"].shape) == (T_, R_) and tuple(res["quantiles"].shape) == (T_, 5, R_)
    _same({k: v.cpu().numpy() for k, v in res.items()},
          {k: (v[:, :, 1] if k == "quantiles" else v[:, 1]) for k, v in want.items()})
    blocked = torch.zeros((T_, 25, ROWS_, 8), device=gpu_device)
    with pytest.raises(ValueError, match="EkfRunner.unblocked"):
        batch.ensemble_summary(blocked, R_, D)


def test_hostapi_equals_device_call(gpu_device):
    from epidemicmodeling_amd import hostapi
    D = 129
    for storage in ("f64", "f32"):
        src = _source(D, storage, seed=17)
        src[0, 2, 5] = np.nan
        pop = np.array([1e6, 2e6, 3e7])
        got = hostapi.ensemble_summary(src, R_, D, q=Q16, population=pop)
        _same(got, _run_device(src, R_, D, Q16, population=pop, device=gpu_device))
        _same(got, E.summary(src, R_, D, Q16, population=pop))


@pytest.fixture(scope="module")
def cfg5():
    from epidemicmodeling_amd import synth
    from tests import helpers as H
    w = synth.make_cfg5(3, 65, 40)
    return w, H.oracle_batch(w, outputs=["S_SMOOTH"])["S_SMOOTH"]


@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_monte_carlo_eks_end_to_end(gpu_device, cfg5, storage):
    from epidemicmodeling_amd import pipeline, synth
    w, oracle_S = cfg5
    q = (0.025, 0.25, 0.5, 0.75, 0.975)
    pop = synth.make_regions(3)["N"]
    res = pipeline.monte_carlo_eks(w, 3, q=q, population=pop, storage=storage, device=gpu_device)
    got = {k: v.cpu().numpy() for k, v in res["S_SMOOTH"].items()}
    S = res["runner"].out["S_SMOOTH"].cpu().numpy()
    assert S.dtype == (np.float32 if storage == "f32" else np.float64) and S.shape == (40, 3, 3 * 65)
    assert got["mean"].shape == (40, 4, 3) and got["quantiles"].shape == (40, 5, 4, 3)
    _same(got, E.summary(S, 3, 65, q, population=pop))
    if storage == "f64":
        _same(got, E.summary(oracle_S, 3, 65, q, population=pop))          # the GPU's S_SMOOTH is the oracle's, bit for bit
    assert np.isfinite(got["mean"]).all() and (got["count"] == 65).all() and (got["std"][:, :3] > 0).any()

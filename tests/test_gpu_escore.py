"""The probabilistic forecast scores on the device (epi_escore_run_device / _host, batch.ensemble_score, hostapi.ensemble_score,
pipeline.fan_quality): every output equal bit for bit (every NaN one value) to the NumPy restatement tests/escore_ref.py of
DESIGN.md §4.17.  Outputs start as a finite sentinel and carry guard elements behind them."""
import ctypes as C

import numpy as np
import pytest

from tests import ens_summary_ref as E
from tests import escore_ref as S
from tests.test_gpu_ens_summary import GRID_D

pytestmark = pytest.mark.gpu

FILL, I32_FILL, GUARD = -98765.4321, -12345, 8
A8 = (0.9, 0.8, 0.6, 0.5, 0.3, 0.2, 0.1, 0.05)
R_, T_, ROWS_ = 3, 2, 2


def _run_device(src, truth, R, D, alpha=(0.5, 0.05), n_bins=0, population=None, truth_series=None, first_day=None, k0=0, k1=None,
                names=None, device="cuda:0", calls=1, test_launch_items=0):
    """epi_escore_run_device `calls` times back to back on sentinel-filled outputs with GUARD elements behind each; returns one
    dict per call (NumPy), the outputs not named (never handed to the library) included"""
    import torch
    from epidemicmodeling_amd import _lib
    dev = torch.device(device)
    put = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)
    sd = torch.as_tensor(np.ascontiguousarray(src), device=dev)
    ins_t = (sd, put(population, np.float64), put(truth, np.float64), put(truth_series, np.int32), put(first_day, np.int32))
    T, rows, _ = src.shape
    d = _lib.make_escore_desc(T, rows, R, D, np.shape(truth)[2], alpha, n_bins, storage=1 if src.dtype == np.float32 else 0,
                              derive_newcases=int(population is not None), k0=k0, k1=k1, test_launch_items=test_launch_items)
    shapes = _lib.escore_shapes(T, rows, R, d.n_a, d.n_bins, d.derive_newcases)
    names = _lib.ESCORE_OUT_NAMES if names is None else names
    ins = _lib.EscoreInputs()
    for k, v in zip(_lib.ESCORE_IN_NAMES, ins_t):
        setattr(ins, k, None if v is None else C.c_void_p(v.data_ptr()))
    st = torch.cuda.current_stream(dev)
    err = C.create_string_buffer(256)
    n = C.c_size_t(0)
    _lib.check(_lib.lib().epi_escore_workspace_bytes(C.byref(d), C.byref(n), err), err)
    assert n.value == T * (rows + d.derive_newcases) * R * 40
    runs = []
    for _ in range(calls):
        ws = torch.full((n.value // 8 + GUARD,), FILL, dtype=torch.float64, device=dev)
        flat = {k: torch.full((int(np.prod(sh)) + GUARD,), I32_FILL if k in _lib.ESCORE_OUT_I32 else FILL,
                              dtype=torch.int32 if k in _lib.ESCORE_OUT_I32 else torch.float64, device=dev) for k, sh in shapes.items()}
        outs = _lib.EscoreOutputs()
        for k in _lib.ESCORE_OUT_NAMES:
            setattr(outs, k, C.c_void_p(flat[k].data_ptr()) if k in names else None)
        rc = _lib.lib().epi_escore_run_device(C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(ws.data_ptr()), n.value,
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
            assert (a[len(a) - GUARD:] == (I32_FILL if k in _lib.ESCORE_OUT_I32 else FILL)).all(), f"{k}: guard elements overwritten"
            out[k] = a[:len(a) - GUARD].reshape(sh)
        res.append(out)
    return res if calls > 1 else res[0]


def _same(got, want, names=S.NAMES):
    for k in names:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        if not S.same_bits(g, w):
            bad = ~((g == w) | (np.isnan(g) & np.isnan(w))) if g.dtype == np.float64 else g != w
            raise AssertionError((k, np.argwhere(bad)[:4].tolist(), g[bad][:4], w[bad][:4]))


def _source(D, storage, seed, R=R_, T=T_, rows=ROWS_):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((T, rows, R * D)) * 10.0 ** rng.uniform(-2, 2, size=(T, rows, 1))
    s = s.astype(np.float32) if storage == "f32" else s
    truth = rng.standard_normal((T, rows, R)) * np.abs(s).astype(np.float64).mean(axis=2, keepdims=True)
    return s, truth


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("D", GRID_D)
def test_shape_grid_equals_reference(gpu_device, D, storage):
    src, truth = _source(D, storage, seed=D)
    for alpha, nb in (((0.5, 0.05), 10), (A8, 32)):
        got = _run_device(src, truth, R_, D, alpha, nb, device=gpu_device)
        _same(got, S.score(src, truth, R_, D, alpha, nb))
        assert (got["count"] == D).all() and (got["n_scored"] == T_).all()


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("D", [64, 65, 300, 1000, 2000])
def test_planted_items(gpu_device, D, storage):
    src, truth = _source(D, storage, seed=100 + D, rows=3)
    item = lambda t, row, r: src[t, row, r * D:(r + 1) * D]          # a view: assignments plant into src
    truth[0, 0, 0] = np.nan                                          # y NaN
    truth[0, 0, 1] = item(0, 0, 1).min() - 1.0                       # below all
    truth[0, 0, 2] = item(0, 0, 2).max() + 1.0                       # above all
    truth[0, 1, 0] = item(0, 1, 0)[D // 3]                           # equal to one member
    item(0, 1, 1)[3:3 + min(D - 3, 70)] = 1.25                       # tied members (longer than a wavefront where D allows) ...
    truth[0, 1, 1] = 1.25                                            # ... and the truth equal to all of them
    item(0, 1, 2)[:] = np.nan                                        # all members NaN, this item only
    item(0, 2, 0)[np.arange(D) != D - 2] = np.nan                    # one member left
    item(0, 2, 1)[[1, D - 1]] = [np.inf, -np.inf]                    # both infinities
    item(0, 2, 2)[5:9] = 2.5                                         # tied members, the truth elsewhere
    item(1, 0, 0)[D // 2] = np.nan                                   # one NaN member
    item(1, 0, 1)[[0, 2]] = np.inf                                   # +Inf twice
    truth[1, 0, 1] = np.inf                                          # an infinite truth
    got = _run_device(src, truth, 3, D, (0.5, 0.05), 10, device=gpu_device)
    want = S.score(src, truth, 3, D, (0.5, 0.05), 10)
    _same(got, want)
    rk, ti, n = got["rank"], got["ties"], got["count"]
    assert rk[0, 0, 0] == -1 and ti[0, 0, 0] == -1 and n[0, 0, 0] == D and np.isnan(got["crps"][0, 0, 0]) and got["cover"][0, 0, 0] == 0
    assert rk[0, 0, 1] == 0 and ti[0, 0, 1] == 0 and got["cover"][0, 0, 1] == 0
    assert rk[0, 0, 2] == D and got["cover"][0, 0, 2] == 0
    assert ti[0, 1, 0] == 1 and ti[0, 1, 1] == min(D - 3, 70)
    assert rk[0, 1, 2] == -1 and n[0, 1, 2] == 0 and np.isnan(got["width"][0, :, 1, 2]).all()
    assert n[0, 2, 0] == 1 and got["crps"][0, 2, 0] == got["ae"][0, 2, 0] == abs(np.float64(item(0, 2, 0)[D - 2]) - truth[0, 2, 0])
    assert n[0, 2, 1] == D and got["crps"][0, 2, 1] == np.inf and np.isfinite(got["ae"][0, 2, 1])
    assert n[1, 0, 0] == D - 1 and ti[1, 0, 1] == 2 and rk[1, 0, 1] == D - 2
    assert (n[1, 1:] == D).all() and np.isfinite(got["crps"][1, 1:]).all() and (rk[1, 1:] >= 0).all()      # the neighbours: untouched
    assert got["n_scored"][0, 0] == 1 and got["n_scored"][1, 2] == 1 and got["n_scored"][2, 0] == 2


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("D", [65, 1000])
def test_derived_row(gpu_device, D, storage):
    rng = np.random.default_rng(D)
    src, truth = _source(D, storage, seed=200 + D, rows=3)
    src = np.abs(src)
    pop = rng.uniform(1e5, 1e8, 3)
    src[1, 1, D + 3] = np.nan                                        # NaN in one factor of one chain of region 1
    new = E.derived_row(src, pop, 3, D)
    truth = np.concatenate([truth, np.nanmedian(new.reshape(T_, 3, D), axis=2)[:, None, :] * rng.uniform(0.5, 1.5, (T_, 1, 3))], axis=1)
    got = _run_device(src, truth, 3, D, (0.5, 0.05), 10, population=pop, device=gpu_device)
    _same(got, S.score(src, truth, 3, D, (0.5, 0.05), 10, population=pop))
    assert got["count"][1, 3, 1] == D - 1 and got["count"][1, 1, 1] == D - 1 and got["count"][1, 0, 1] == D
    assert got["crps"].shape == (T_, 4, 3) and np.isfinite(got["crps"][:, 3]).all()


def test_truth_series_first_day_and_window(gpu_device):
    D, R, T = 129, 6, 7
    src, _ = _source(D, "f64", seed=31, R=R, T=T)
    truth = np.random.default_rng(32).standard_normal((T, ROWS_, 2))
    ts, fd = [0, 0, 1, 1, 1, 0], [0, 2, 6, 7, 3, 1]                  # shared columns; an origin at T: no scored day
    for k0, k1 in ((0, None), (1, 5), (3, 3)):
        kw = dict(alpha=(0.5, 0.05), n_bins=7, truth_series=ts, first_day=fd, k0=k0, k1=k1)
        got = _run_device(src, truth, R, D, device=gpu_device, **kw)
        _same(got, S.score(src, truth, R, D, **kw))
    assert (got["n_scored"] == 0).all() and np.isnan(got["crps_mean"]).all() and (got["pit_hist"] == 0).all()
    got = _run_device(src, truth, R, D, n_bins=7, truth_series=ts, first_day=fd, device=gpu_device)
    assert (got["n_scored"][0] == [7, 5, 1, 0, 4, 6]).all() and np.isnan(got["wis_mean"][:, 3]).all()
    assert (got["pit_hist"].sum(axis=0) == got["n_scored"]).all()


def test_optional_outputs(gpu_device):
    import torch
    from epidemicmodeling_amd import _lib, batch
    D = 129
    src, truth = _source(D, "f64", seed=7)
    want = S.score(src, truth, R_, D, (0.5, 0.05), 10)
    for names in (("crps",), ("rank", "ties"), ("crps_mean",), ("pit_hist", "cover_frac"), ("wis", "ae_mean", "n_scored"), ("width", "cover")):
        got = _run_device(src, truth, R_, D, (0.5, 0.05), 10, names=names, device=gpu_device)
        _same(got, want, names=names)
        for k in S.NAMES:
            if k not in names:
                assert (got[k] == (I32_FILL if k in S.I32 else FILL)).all(), (names, k)
    res = batch.ensemble_score(torch.as_tensor(src, device=gpu_device), truth, R_, D, n_bins=10, outputs=("wis_mean", "crps"))
    assert list(res) == ["crps", "wis_mean"]
    _same({k: v.cpu().numpy() for k, v in res.items()}, want, names=("crps", "wis_mean"))
    with pytest.raises(_lib.EpiError, match="n_bins"):
        batch.ensemble_score(torch.as_tensor(src, device=gpu_device), truth, R_, D, n_bins=0, outputs=("pit_hist",))


def test_launch_cut_equals_the_uncut_call(gpu_device):
    D = 300
    src, truth = _source(D, "f32", seed=9, T=3)
    whole = _run_device(src, truth, R_, D, A8, 32, device=gpu_device)
    assert 3 * ROWS_ * R_ > 3 * 5                                     # several launches of five items and a shorter last one
    _same(_run_device(src, truth, R_, D, A8, 32, device=gpu_device, test_launch_items=5), whole)
    _same(whole, S.score(src, truth, R_, D, A8, 32))


def test_repeat_call_on_one_stream(gpu_device):
    D = 1000
    src, truth = _source(D, "f32", seed=11)
    a, b = _run_device(src, truth, R_, D, n_bins=10, device=gpu_device, calls=2)
    _same(a, b)
    _same(a, S.score(src, truth, R_, D, n_bins=10))


def test_batch_entry_point(gpu_device):
    import torch
    from epidemicmodeling_amd import batch
    D = 65
    src, truth = _source(D, "f64", seed=13)
    want = S.score(src, truth, R_, D, (0.5, 0.05), 10)
    res = batch.ensemble_score(torch.as_tensor(src, device=gpu_device), torch.as_tensor(truth, device=gpu_device), R_, D, n_bins=10)
    assert list(res) == list(S.NAMES)
    _same({k: v.cpu().numpy() for k, v in res.items()}, want)
    res = batch.ensemble_score(torch.as_tensor(src[:, 1], device=gpu_device), truth[:, 1], R_, D, n_bins=10, test_launch_items=5)
    assert tuple(res["crps"].shape) == (T_, R_) and tuple(res["width"].shape) == (T_, 2, R_) and tuple(res["pit_hist"].shape) == (10, R_)
    one = S.score(src[:, 1:2], truth[:, 1:2], R_, D, (0.5, 0.05), 10)
    _same({k: v.cpu().numpy() for k, v in res.items()}, {k: v.reshape(v.shape[:-2] + v.shape[-1:]) for k, v in one.items()})
    blocked = torch.zeros((T_, 25, ROWS_, 8), device=gpu_device)
    with pytest.raises(ValueError, match="EkfRunner.unblocked"):
        batch.ensemble_score(blocked, truth, R_, D)
    with pytest.raises(ValueError, match="truth_series"):
        batch.ensemble_score(torch.as_tensor(src, device=gpu_device), truth[:, :, :2], R_, D)


def test_hostapi_equals_batch(gpu_device):
    import torch
    from epidemicmodeling_amd import batch, hostapi
    D = 129
    for storage in ("f64", "f32"):
        src, truth = _source(D, storage, seed=17, rows=3)
        src = np.abs(src)
        src[0, 2, 5] = np.nan
        pop = np.array([1e6, 2e6, 3e7])
        truth = np.concatenate([truth, truth[:, :1] * 1e5], axis=1)
        kw = dict(alpha=(0.8, 0.5, 0.05), n_bins=10, population=pop, truth_series=[2, 0, 0], first_day=[0, 1, 0])
        got = hostapi.ensemble_score(src, truth, 3, D, **kw)
        dev = batch.ensemble_score(torch.as_tensor(src, device=gpu_device), truth, 3, D, **kw)
        assert list(got) == list(dev)
        _same(got, {k: v.cpu().numpy() for k, v in dev.items()})
        _same(got, S.score(src, truth, 3, D, **kw))


def test_fan_quality_end_to_end(gpu_device):
    import torch
    from epidemicmodeling_amd import batch, pipeline, synth
    Sg, LL, F, D, starts = 3, 40, 10, 65, (10, 4)
    raw = synth.make_raw_counts(n_regions=Sg, T=LL, seed=3)
    raw["cases"][:, -1] = np.cumsum(np.full(LL, 40.0))               # the all-NaN region of the generator: give it data
    out = pipeline.fan_quality(raw["cases"], raw["deaths"], raw["population"], raw["ip"], F, starts, n_draws=D, seed=5, device=gpu_device)
    B, k0, N = Sg * 2, LL - 10, np.asarray(raw["population"], dtype=np.float64)
    assert out["k0"] == k0 and list(out["origin"]) == [30, 36] * Sg and out["workload"].B == B
    assert np.isnan(out["workload"].x[36:, 1]).all() and not np.isnan(out["workload"].x[30:36, 1]).any()
    X = out["X"]
    assert tuple(X.shape) == (10, 3, B * D)
    # the same steps by hand: the fan's bands by ensemble_summary, the scores by the restatement
    rr = np.repeat(np.arange(Sg), 2)
    tw = np.full((10, 4, Sg), np.nan)
    tw[:, 3] = out["truth"][k0:]
    want = S.score(X.cpu().numpy(), tw, B, D, (0.5, 0.05), 10, population=N[rr], truth_series=rr, first_day=out["origin"] - k0)
    got = {k: v.cpu().numpy() for k, v in out["scores"].items()}
    _same(got, want)
    q_lo, q_hi = S.probabilities((0.5, 0.05))                       # the probabilities as the call forms them
    q = (q_lo[1], q_lo[0], 0.5, q_hi[0], q_hi[1])
    summ = {k: v.cpu().numpy() for k, v in batch.ensemble_summary(X, B, D, q=q, population=torch.as_tensor(N[rr])).items()}
    assert np.array_equal(got["width"][:, 0, 3], summ["quantiles"][:, 3, 3] - summ["quantiles"][:, 1, 3])
    assert np.array_equal(got["width"][:, 1, 3], summ["quantiles"][:, 4, 3] - summ["quantiles"][:, 0, 3])
    y = out["truth"][k0:][:, rr]
    assert np.array_equal(got["ae"][:, 3], np.abs(y - summ["quantiles"][:, 2, 3]))
    inside = (summ["quantiles"][:, 0, 3] <= y) & (y <= summ["quantiles"][:, 4, 3])
    assert np.array_equal((got["cover"][:, 3] >> 1) & 1, inside.astype(np.int32))
    assert (got["rank"][:, :3] == -1).all() and (got["n_scored"][3] == [10, 4] * Sg).all() and (got["n_scored"][:3] == 0).all()
    # by lead: lead l of chain c is day origin_c - k0 + l
    crps = got["crps"][:, 3]
    lead = out["crps_by_lead"].cpu().numpy()
    assert lead.shape == (10, Sg) and tuple(out["cover_by_lead"].shape) == (2, 10, Sg)
    for r in range(Sg):
        for l in range(10):
            vals = [crps[0 + l, 2 * r]] + ([crps[6 + l, 2 * r + 1]] if l < 4 else [])
            assert abs(lead[l, r] - np.mean(vals)) <= 1e-12 * abs(np.mean(vals))
    assert np.isfinite(lead).all() and np.isfinite(out["wis_by_lead"].cpu().numpy()).all()
    assert abs(got["crps_mean"][3, 1] - crps[6:, 1].mean()) <= 1e-12 * crps[6:, 1].mean()

"""The autoregressive alpha forecaster on the device (epi_arfc_run_device / _host, batch.ar_forecast, hostapi.ar_forecast,
pipeline.ar_forecast): S, A, the noise variance and the status equal bit for bit -- NaN positions included -- to the C
restatement tests/ar_forecast_ref.c of DESIGN.md §4.8.  Outputs start as a finite sentinel and carry guard elements."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import ar_forecast_ref as AR

pytestmark = pytest.mark.gpu

FILL, I32_FILL, GUARD = -98765.4321, -12345, 8


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return AR.ArRef(tmp_path_factory.mktemp("arfc"))


def _problem(R, D, L, H, seed, z=True, drive=None, noise=0.05, offset=0.3):
    """alpha-like segments (a stable AR(2) around `offset`), SI parameters and draws"""
    rng = np.random.default_rng(seed)
    seg = np.stack([AR.ar_series([-1.2, 0.5], L, 1000 * seed + r, noise=noise, offset=offset) for r in range(R)], axis=1)
    pr = dict(seg=seg, beta=rng.uniform(0.1, 0.3, R), s0=rng.uniform(0.9, 0.999, R), dt=1.0, H=H, D=D)
    pr["i0"] = 1.0 - pr["s0"]
    B = R * D
    pr["z"] = rng.standard_normal((H, B)) if z else None
    pr["drive"] = pr["drive_series"] = None
    if drive == "series":
        pr["drive"] = rng.uniform(-0.2, 0.2, (H, R + 2))
        pr["drive_series"] = rng.integers(0, R + 2, B).astype(np.int32)
    elif drive == "chain":
        pr["drive"] = rng.uniform(-0.2, 0.2, (H, B))
    return pr


def _run_device(pr, p, A=None, noise_var=None, nv_mode=0, device="cuda:0", calls=1):
    """epi_arfc_run_device `calls` times back to back on one stream, on sentinel-filled outputs with GUARD elements behind
    each; returns one dict per call (NumPy) under the names of batch.ar_forecast"""
    import torch
    from epidemicmodeling_amd import _lib
    dev = torch.device(device)
    up = lambda v, dt=np.float64: None if v is None else torch.as_tensor(np.ascontiguousarray(v, dtype=dt), device=dev)
    L, R = pr["seg"].shape
    vals = [up(pr["seg"]), up(pr["beta"]), up(pr["s0"]), up(pr["i0"]), up(pr["z"]), up(pr["drive"]),
            up(pr["drive_series"], np.int32), up(A), up(noise_var)]
    d = _lib.make_arfc_desc(R, pr["D"], L, p, pr["H"], pr["dt"], fit=int(A is None), nv_mode=nv_mode,
                            Sd=0 if pr["drive"] is None else pr["drive"].shape[1])
    ins = _lib.ArfcInputs()
    for k, v in zip(_lib.ARFC_IN_NAMES, vals):
        setattr(ins, k, None if v is None else C.c_void_p(v.data_ptr()))
    shapes = _lib.arfc_shapes(R, pr["D"], L, p, pr["H"])
    st = torch.cuda.current_stream(dev)
    err = C.create_string_buffer(256)
    runs = []
    for _ in range(calls):
        flat = {k: (torch.full((int(np.prod(sh)) + GUARD,), I32_FILL, dtype=torch.int32, device=dev) if k == "status" else
                    torch.full((int(np.prod(sh)) + GUARD,), FILL, dtype=torch.float64, device=dev)) for k, sh in shapes.items()}
        outs = _lib.ArfcOutputs()
        for k in _lib.ARFC_OUT_NAMES:
            setattr(outs, k, C.c_void_p(flat[k].data_ptr()))
        rc = _lib.lib().epi_arfc_run_device(C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(st.cuda_stream), err)
        _lib.check(rc, err)
        runs.append(flat)
    torch.cuda.synchronize(dev)
    res = []
    for flat in runs:
        out = {}
        for k, sh in shapes.items():
            a = flat[k].cpu().numpy()
            fill = I32_FILL if k == "status" else FILL
            assert (a[-GUARD:] == fill).all(), f"{k}: guard elements overwritten"
            assert not (a[:-GUARD] == fill).any(), f"{k}: elements left unwritten"
            out[k] = a[:-GUARD].reshape(sh)
        res.append({"S": out["S"], "A": out["A_out"], "noise_var": out["noise_var_out"], "status": out["status"]})
    return res if calls > 1 else res[0]


def _want(ref, pr, p, A=None, noise_var=None, nv_mode=0):
    return ref.run(pr["seg"], pr["beta"], pr["s0"], pr["i0"], pr["dt"], p, pr["H"], pr["D"], z=pr["z"], drive=pr["drive"],
                   drive_series=pr["drive_series"], A=A, noise_var=noise_var, nv_mode=nv_mode)


def _same(got, want):
    for k in ("status", "A", "noise_var", "S"):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (k, g.shape, w.shape)
        if k == "status":
            assert np.array_equal(g, w), (k, g, w)
        else:
            bad = ~((g == w) | (np.isnan(g) & np.isnan(w)))
            assert not bad.any(), (k, int(bad.sum()), np.argwhere(bad)[:4].tolist(), g[bad][:4], w[bad][:4])


def _check(ref, pr, p, gpu_device, **kw):
    got, want = _run_device(pr, p, device=gpu_device, **kw), _want(ref, pr, p, **kw)
    _same(got, want)
    return got, want


@pytest.mark.parametrize("nv_mode", [0, 1])
def test_reference_shape(gpu_device, ref, nv_mode):
    """the reference's order and history: p = 24, L = 120"""
    got, _ = _check(ref, _problem(5, 3, 120, 7, seed=1), 24, gpu_device, nv_mode=nv_mode)
    assert (got["status"] == 0).all() and np.isfinite(got["S"]).all()


def test_smallest_problem(gpu_device, ref):
    got, _ = _check(ref, _problem(1, 1, 2, 1, seed=2), 1, gpu_device)
    assert got["status"][0] == 0 and got["S"].shape == (3, 3, 1)


def test_largest_problem(gpu_device, ref):
    """p = 32, L = 288: both limits, M = 512 rows in 132 KiB of LDS"""
    got, _ = _check(ref, _problem(2, 5, 288, 3, seed=3, noise=1.0), 32, gpu_device)
    assert (got["status"] == 0).all()


@pytest.mark.parametrize("M, p", [(62, 7), (64, 8), (66, 5), (128, 24), (130, 3)])
def test_row_counts_around_the_wave_width(gpu_device, ref, M, p):
    got, _ = _check(ref, _problem(3, 2, M // 2 + p, 4, seed=M), p, gpu_device)
    assert (got["status"] == 0).all()


@pytest.mark.parametrize("R, D", [(1, 1), (3, 21), (1, 64), (64, 1), (5, 13), (257, 1), (1, 257), (5, 205), (41, 25)])
def test_chain_counts(gpu_device, ref, R, D):
    """B = 1, 63, 64, 65, 257, 1 025: draws that end inside a workgroup, regions that are no divisor of its 64 lanes"""
    _check(ref, _problem(R, D, 20, 5, seed=R + D, drive="series"), 3, gpu_device)


def test_given_model(gpu_device, ref):
    pr = _problem(4, 70, 30, 6, seed=5)
    rng = np.random.default_rng(5)
    A = np.stack([[-1.1, 0.4, 0.05]] * 4, axis=1) + 0.01 * rng.standard_normal((3, 4))
    nv = rng.uniform(1e-4, 1e-2, 4)
    A[1, 2] = np.nan                                   # a model that cannot be used: NaN from day L on, region 2 only
    got, want = _check(ref, pr, 3, gpu_device, A=A, noise_var=nv)
    assert (got["status"] == 0).all() and AR.same(got["A"], A) and np.array_equal(got["noise_var"], nv)
    c = slice(2 * 70, 3 * 70)
    assert np.isnan(got["S"][30:, :, c]).all() and np.isfinite(got["S"][:30, :, c]).all()
    assert np.isfinite(np.delete(got["S"], np.r_[c], axis=2)).all()


@pytest.mark.parametrize("drive", ["series", "chain"])
def test_drive(gpu_device, ref, drive):
    pr = _problem(3, 50, 40, 9, seed=6, drive=drive)
    got, _ = _check(ref, pr, 4, gpu_device)
    pr0 = dict(pr, drive=None, drive_series=None)
    assert not np.array_equal(got["S"][40:, 2], _want(ref, pr0, 4)["S"][40:, 2])       # the drive reaches alpha_hat


def test_no_draws_is_the_deterministic_continuation(gpu_device, ref):
    pr = _problem(3, 5, 40, 9, seed=7, z=False)
    got, _ = _check(ref, pr, 4, gpu_device)
    assert (got["S"][:, :, ::5] == got["S"][:, :, 1::5]).all()                         # every draw of a region is the same chain


def test_clamp_acts(gpu_device, ref):
    """zero-mean segments: the continuation is negative about half the time"""
    pr = _problem(4, 40, 60, 30, seed=8, noise=1.0, offset=0.0)
    got, want = _check(ref, pr, 6, gpu_device)
    share = (want["S"][60:, 2] == 0.0).mean()
    print(f"clamped share of the forecast days (C reading): {share:.3f}")
    assert share >= 1.0 / 3.0 and (want["S"][:, 2] >= 0.0).all()


def test_sick_regions_among_healthy_ones(gpu_device, ref):
    pr = _problem(5, 9, 50, 6, seed=9)
    pr["seg"][:, 1] = 0.25                              # constant: rank-deficient for p >= 2
    pr["seg"][17, 3] = np.inf                           # BAD_INPUT
    got, want = _check(ref, pr, 4, gpu_device)
    assert got["status"].tolist() == [0, AR.ST_RANK_DEFICIENT, 0, AR.ST_BAD_INPUT, 0]
    S = got["S"]
    assert np.isnan(S[50:, :, 9:18]).all() and np.isfinite(S[:50, :, 9:18]).all() and np.isnan(S[:, :, 27:36]).all()
    assert np.isnan(got["A"][:, [1, 3]]).all() and np.isnan(got["noise_var"][[1, 3]]).all()
    healthy = dict(pr, seg=_problem(5, 9, 50, 6, seed=9)["seg"])
    alone = _want(ref, healthy, 4)
    for r in (0, 2, 4):                                 # untouched by their neighbours
        assert np.array_equal(S[:, :, 9 * r:9 * r + 9], alone["S"][:, :, 9 * r:9 * r + 9])
        assert np.array_equal(got["A"][:, r], alone["A"][:, r])


def test_two_calls_back_to_back(gpu_device, ref):
    pr = _problem(6, 100, 120, 10, seed=10)
    a, b = _run_device(pr, 24, device=gpu_device, calls=2)
    for k in a:
        assert AR.same(a[k], b[k]) and a[k].tobytes() == b[k].tobytes(), k
    _same(a, _want(ref, pr, 24))


def test_python_entry_points(gpu_device, ref):
    import torch
    from epidemicmodeling_amd import batch, hostapi
    pr = _problem(3, 33, 40, 5, seed=11, drive="series")
    want = _want(ref, pr, 4)
    kw = dict(z=pr["z"], drive=pr["drive"], drive_series=pr["drive_series"])
    res = batch.ar_forecast(torch.as_tensor(pr["seg"], device=gpu_device), pr["beta"], pr["s0"], pr["i0"], 1.0, 4, 5, 33,
                            device=gpu_device, **kw)
    assert res["S"].is_cuda and res["status"].dtype == torch.int32
    _same({k: v.cpu().numpy() for k, v in res.items()}, want)
    _same(hostapi.ar_forecast(pr["seg"], pr["beta"], pr["s0"], pr["i0"], 1.0, 4, 5, 33, **kw), want)
    got = hostapi.ar_forecast(pr["seg"], pr["beta"], pr["s0"], pr["i0"], 1.0, 4, 5, 33, A=want["A"], noise_var=want["noise_var"], **kw)
    assert np.array_equal(got["S"], want["S"])          # the fitted model handed back in gives the same chains


def test_pipeline_fan_chart(gpu_device, ref):
    """pipeline.ar_forecast end to end.  tests/golden/xprize/ holds no case table, so the counts are synth.make_raw_counts'
    and the excerpt supplies the plan (future_ip_head.csv: 29 days x 12 NPIs, the same plan for every region)."""
    from epidemicmodeling_amd import dataio, hostapi, pipeline, synth
    from tests import helpers as H
    plan1 = dataio.read_ip_file(os.path.join(H.ROOT, "tests", "golden", "xprize", "future_ip_head.csv"))["ip"]     # [29, 12, 1]
    raw = synth.make_raw_counts(n_regions=4, T=150, seed=3)
    Hh, D, L, p = plan1.shape[0], 65, 60, 6
    plan = np.repeat(plan1, 4, axis=2)
    q = (0.025, 0.25, 0.5, 0.75, 0.975)
    out = pipeline.ar_forecast(raw["cases"], raw["deaths"], raw["population"], raw["ip"], horizon=Hh, ar_order=p, history=L,
                               n_draws=D, plan=plan, q=q, seed=5, device=gpu_device)
    fc = {k: v.cpu().numpy() for k, v in out["forecast"].items()}
    sm = {k: v.cpu().numpy() for k, v in out["summary"].items()}
    print("status", fc["status"].tolist())
    assert fc["S"].shape == (L + Hh, 3, 4 * D) and fc["A"].shape == (p, 4) and out["drive"].shape == (Hh, 4)
    assert sm["mean"].shape == (L + Hh, 4, 4) and sm["quantiles"].shape == (L + Hh, 5, 4, 4)
    assert np.array_equal(out["seg"], out["alpha_round2"][150 - L:])
    ok = fc["status"] == 0
    # the expected status vector is the C reading's on the same segments (a smoothed alpha can sit at a bound for 60 days: a
    # constant segment is rank-deficient), and a fit that lost most regions would not pass as "some region is fine"
    assert fc["status"].tolist() == [ref.fit(out["seg"][:, r], p)[2] for r in range(4)] and ok.sum() >= 3, fc["status"].tolist()
    assert (sm["count"][:, :, ok] == D).all() and (sm["count"][:L][:, :, fc["status"] != AR.ST_BAD_INPUT] == D).all()
    qs = sm["quantiles"][:, :, :, ok]
    assert (np.diff(qs, axis=1) >= 0).all() and (sm["min"][:, :, ok] <= qs[:, 0]).all() and (qs[:, -1] <= sm["max"][:, :, ok]).all()
    assert (sm["std"][L:, 2][:, ok] > 0).any() and (sm["min"][:L, :, ok] == sm["max"][:L, :, ok]).all()     # the draws differ over the forecast only
    # the same two stages chained by hand through the host entry points
    N, I0 = np.asarray(raw["population"], dtype=np.float64), out["pre"]["I0"]
    hand = hostapi.ar_forecast(out["seg"], np.full(4, synth.MODEL_BETA), (N - I0) / N, I0 / N, 1.0, p, Hh, D,
                               z=out["z"].cpu().numpy(), drive=out["drive"], drive_series=np.repeat(np.arange(4), D))
    _same(fc, hand)
    hs = hostapi.ensemble_summary(hand["S"], 4, D, q=q, population=N)
    for k in sm:
        assert AR.same(sm[k], hs[k]), k

"""The seeded standard-normal draws on the device.  The fill kernel equals the restatement tests/noise_ref.c bit
for bit, as double and as float, on windows that reach the high counter words and in launches cut small, in sentinel-filled
outputs with guard words.  Each of the four consumers, called with a seed, equals on every output word the existing call given
z = normal_draws(...) of the same seed and stream -- at the smallest shapes at which the kernels can go wrong.  The same seed
twice gives the same bits, another stream or seed other bits; pipeline.smoothed_fan(rng="device") returns the summary of
smoothed_fan(z=normal_draws(...)); the hostapi twins agree with batch."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import loglik_ref as LR
from tests import noise_ref as NR
from tests import sdraw_ref as SR

pytestmark = pytest.mark.gpu

SEED = 0x452821E638D01377
FILL, I32_FILL, GUARD = -98765.4321, -12345, 8


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return NR.NoiseRef(tmp_path_factory.mktemp("noise_ref"))


def _fill_raw(seed, stream, t0, nt, rows, lane0, n, f32=False, groups=0, device="cuda:0"):
    """epi_noise_fill_device into a sentinel-filled buffer with GUARD words on either side"""
    import torch
    from epidemicmodeling_amd import _lib
    dt = torch.float32 if f32 else torch.float64
    cnt = nt * rows * n
    buf = torch.full((cnt + 2 * GUARD,), FILL, dtype=dt, device=device)
    d, err = _lib.make_noise_desc(seed, stream), C.create_string_buffer(256)
    st = torch.cuda.current_stream(torch.device(device))
    rc = _lib.lib().epi_noise_fill_device(C.byref(d), t0, nt, rows, lane0, n, int(f32), C.c_void_p(buf.data_ptr() + GUARD * buf.element_size()),
                                          groups, C.c_void_p(st.cuda_stream), err)
    _lib.check(rc, err)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    fill = np.asarray(FILL, dtype=h.dtype)
    assert (h[:GUARD] == fill).all() and (h[GUARD + cnt:] == fill).all(), "guard words overwritten"
    out = h[GUARD:GUARD + cnt].reshape(nt, rows, n)
    assert not (out == fill).any(), "sentinel left"
    return out


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("stream", [0, 2 ** 30 - 1])
def test_fill_equals_restatement(gpu_device, ref, rows, stream):
    for t0 in (0, 2 ** 32 - 3):                       # t is one counter word: 2^32 - 3 is the last start of a 3-day window
        for lane0 in (0, 2 ** 32 - 2, 2 ** 40 + 1):
            want = ref.fill(SEED, stream, t0, 3, rows, lane0, 130)
            assert NR.same_bits(_fill_raw(SEED, stream, t0, 3, rows, lane0, 130), want), (t0, lane0)
            assert NR.same_bits(_fill_raw(SEED, stream, t0, 3, rows, lane0, 130, f32=True), want.astype(np.float32)), (t0, lane0)
    # 3 * pairs * 300 items: several 256-lane workgroups, the last ragged, one workgroup per launch
    want = ref.fill(SEED, stream, 1, 3, rows, 9, 300)
    assert NR.same_bits(_fill_raw(SEED, stream, 1, 3, rows, 9, 300, groups=1), want)
    assert NR.same_bits(_fill_raw(SEED, stream, 1, 3, rows, 9, 300, f32=True, groups=2), want.astype(np.float32))


def test_normal_draws_repeat_and_differ(gpu_device, ref):
    import torch
    from epidemicmodeling_amd import batch, hostapi
    a = batch.normal_draws(4, 3, 200, SEED, stream=3, t0=2, lane0=11, device=gpu_device)
    b = batch.normal_draws(4, 3, 200, SEED, stream=3, t0=2, lane0=11, device=gpu_device)
    torch.cuda.synchronize()
    assert a.dtype == torch.float64 and tuple(a.shape) == (4, 3, 200)
    assert NR.same_bits(a.cpu().numpy(), b.cpu().numpy()) and NR.same_bits(a.cpu().numpy(), ref.fill(SEED, 3, 2, 4, 3, 11, 200))
    for other in (batch.normal_draws(4, 3, 200, SEED, stream=4, t0=2, lane0=11, device=gpu_device),
                  batch.normal_draws(4, 3, 200, SEED ^ 1, stream=3, t0=2, lane0=11, device=gpu_device)):
        assert not (other == a).any()
    f = batch.normal_draws(4, 3, 200, SEED, stream=3, t0=2, lane0=11, dtype=torch.float32, device=gpu_device)
    assert NR.same_bits(f.cpu().numpy(), a.cpu().numpy().astype(np.float32))
    h = hostapi.normal_draws(4, 3, 200, SEED, stream=3, t0=2, lane0=11)
    assert NR.same_bits(h, a.cpu().numpy())
    assert NR.same_bits(hostapi.normal_draws(2, 1, 70, SEED, dtype=np.float32), ref.fill(SEED, 0, 0, 2, 1, 0, 70).astype(np.float32))


# ---- smoother draws ----
@functools.lru_cache(maxsize=None)
def _case(B, T):
    from epidemicmodeling_amd import synth
    w = synth.make_cfg3(B, T)
    return w, SR.case_of(w, H.oracle_batch(w))


SD_NAMES = ("X", "rank", "status", "J", "L")
SD_I32 = ("rank", "status")


def _sdraw_raw(case, D, z=None, noise=None, k0=0, clamp=True, storage="f64", out_f32=False, blk=0, groups=0, device="cuda:0"):
    """epi_sdraw_run_device (z) or epi_sdraw_run_device_seeded (noise) on sentinel-filled outputs with GUARD words behind each
    and a sentinel-filled workspace; returns the dict of NumPy arrays after checking the guards"""
    import torch
    from epidemicmodeling_amd import _lib
    dev = torch.device(device)
    B, T = case["B"], case["T"]
    ndt = np.float32 if storage == "f32" else np.float64
    up = lambda a, dt=np.float64: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)
    with np.errstate(over="ignore", invalid="ignore"):
        big = [case[k].astype(ndt) for k in SR.BIG]
    if blk:
        big = [LR.to_blocked(a, blk, np.nan) for a in big]
    tens = [up(a, ndt) for a in big] + [up(case["prm"]), z, None, None]
    shapes = _lib.sdraw_shapes(B, T, D, k0)
    d = _lib.make_sdraw_desc(B, T, D, k0, clamp, blk, int(storage == "f32"), 0, int(out_f32), test_launch_groups=groups)
    ins = _lib.SdrawInputs()
    for k, v in zip(_lib.SDRAW_IN_NAMES, tens):
        setattr(ins, k, None if v is None else C.c_void_p(v.data_ptr()))
    tdt = {k: torch.int32 if k in SD_I32 else (torch.float32 if k == "X" and out_f32 else torch.float64) for k in SD_NAMES}
    fill = {k: I32_FILL if k in SD_I32 else FILL for k in SD_NAMES}
    flat = {k: torch.full((int(np.prod(shapes[k])) + GUARD,), fill[k], dtype=tdt[k], device=dev) for k in SD_NAMES}
    outs = _lib.SdrawOutputs()
    for k in SD_NAMES:
        setattr(outs, k, C.c_void_p(flat[k].data_ptr()))
    err, n = C.create_string_buffer(256), C.c_size_t(0)
    _lib.check(_lib.lib().epi_sdraw_workspace_bytes(C.byref(d), C.byref(n), err), err)
    ws = torch.full((n.value // 8 + GUARD,), FILL, dtype=torch.float64, device=dev)
    tail = (C.byref(ins), C.byref(outs), C.c_void_p(ws.data_ptr()), n.value, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), err)
    if noise is None:
        rc = _lib.lib().epi_sdraw_run_device(C.byref(d), *tail)
    else:
        rc = _lib.lib().epi_sdraw_run_device_seeded(C.byref(d), C.byref(noise), *tail)
    _lib.check(rc, err)
    torch.cuda.synchronize(dev)
    assert bool((ws[n.value // 8:] == FILL).all()), "wrote behind the workspace"
    res = {}
    for k in SD_NAMES:
        h = flat[k].cpu().numpy()
        cnt = int(np.prod(shapes[k]))
        assert (h[cnt:] == np.asarray(fill[k], dtype=h.dtype)).all(), f"{k}: guard words overwritten"
        res[k] = h[:cnt].reshape(shapes[k])
        assert not (res[k] == np.asarray(fill[k], dtype=h.dtype)).any(), f"{k}: sentinel left"
    return res


@pytest.mark.parametrize("T", [6, 3])                 # above and below the 4-day prefetch of the z loads
@pytest.mark.parametrize("blk", [0, 2])
def test_sdraw_seeded_equals_given_draws(gpu_device, T, blk):
    from epidemicmodeling_amd import _lib, batch
    B, D = 3, 70                                      # 210 paths: one 256-lane workgroup, partly empty; a wavefront straddles chains
    w, case = _case(B, T)
    for k0 in (0, 2):
        noise = _lib.make_noise_desc(SEED, 5)
        z = batch.normal_draws(T - k0, 3, B * D, SEED, stream=5, device=gpu_device)
        for clamp in (False, True):
            for storage, of in (("f64", False), ("f32", False), ("f64", True)):
                kw = dict(k0=k0, clamp=clamp, storage=storage, out_f32=of, blk=blk)
                want = _sdraw_raw(case, D, z=z, **kw)
                got = _sdraw_raw(case, D, noise=noise, **kw)
                for k in SD_NAMES:
                    assert NR.same_bits(got[k], want[k]), (k, kw)
                assert float(np.std(got["X"][0, 2].astype(np.float64).reshape(B, D), axis=1).min()) > 0.0
        # 7 chains x 70 draws = 490 paths: two workgroups, one per launch
    w7, case7 = _case(7, T)
    z = batch.normal_draws(T, 3, 7 * D, SEED, device=gpu_device)
    want = _sdraw_raw(case7, D, z=z, blk=blk, groups=1)
    got = _sdraw_raw(case7, D, noise=_lib.make_noise_desc(SEED), blk=blk, groups=1)
    for k in SD_NAMES:
        assert NR.same_bits(got[k], want[k]), (k, "cut")


def test_sdraw_python_twins(gpu_device):
    """batch.smoother_draws(seed=) = batch.smoother_draws(z=normal_draws) = hostapi.smoother_draws(seed=); another seed or stream:
    other draws"""
    import torch
    from epidemicmodeling_amd import batch, hostapi
    w, case = _case(3, 6)
    big = [np.ascontiguousarray(case[k]) for k in SR.BIG]
    dev = [torch.as_tensor(a).cuda() for a in big]
    z = batch.normal_draws(4, 3, 3 * 70, SEED, stream=2, device=gpu_device)
    a = batch.smoother_draws(*dev, case["prm"], 70, z=z, k0=2, outputs=SD_NAMES)
    b = batch.smoother_draws(*dev, case["prm"], 70, seed=SEED, noise_stream=2, k0=2, outputs=SD_NAMES)
    b2 = batch.smoother_draws(*dev, case["prm"], 70, seed=SEED, noise_stream=2, k0=2, outputs=SD_NAMES)
    h = hostapi.smoother_draws(*big, case["prm"], 70, seed=SEED, noise_stream=2, k0=2, outputs=SD_NAMES)
    torch.cuda.synchronize()
    assert list(a) == list(b) == list(h) == list(SD_NAMES)
    for k in SD_NAMES:
        assert NR.same_bits(a[k].cpu().numpy(), b[k].cpu().numpy()) and NR.same_bits(b[k].cpu().numpy(), b2[k].cpu().numpy()), k
        assert NR.same_bits(h[k], b[k].cpu().numpy()), k
    for kw in (dict(seed=SEED, noise_stream=3), dict(seed=SEED ^ (1 << 63), noise_stream=2)):
        c = batch.smoother_draws(*dev, case["prm"], 70, k0=2, **kw)
        assert not (c["X"] == b["X"]).all()
    with pytest.raises(ValueError, match="seed and z together"):
        batch.smoother_draws(*dev, case["prm"], 70, z=z, seed=SEED, k0=2)


# ---- the AR forecaster ----
@pytest.mark.parametrize("R,D", [(1, 70), (2, 35)])
@pytest.mark.parametrize("drive", [False, True])
def test_ar_forecast_seeded_equals_given_draws(gpu_device, R, D, drive):
    import torch
    from epidemicmodeling_amd import batch, hostapi
    rng = np.random.default_rng(5)
    L, p, Hh, B = 20, 3, 5, R * D
    seg = 0.3 + 0.05 * np.cumsum(rng.standard_normal((L, R)), axis=0) * 0.2
    beta, s0 = np.full(R, 0.2), np.full(R, 0.95)
    kw = dict(nv_mode=0)
    if drive:
        kw.update(drive=0.05 * rng.standard_normal((Hh, R + 1)), drive_series=rng.integers(0, R + 1, B).astype(np.int32))
    z = batch.normal_draws(Hh, 1, B, SEED, stream=1, device=gpu_device)[:, 0].contiguous()
    a = batch.ar_forecast(seg, beta, s0, 1 - s0, 0.5, p, Hh, D, z=z, device=gpu_device, **kw)
    b = batch.ar_forecast(seg, beta, s0, 1 - s0, 0.5, p, Hh, D, seed=SEED, noise_stream=1, device=gpu_device, **kw)
    h = hostapi.ar_forecast(seg, beta, s0, 1 - s0, 0.5, p, Hh, D, seed=SEED, noise_stream=1, **kw)
    c = batch.ar_forecast(seg, beta, s0, 1 - s0, 0.5, p, Hh, D, seed=SEED, noise_stream=2, device=gpu_device, **kw)
    torch.cuda.synchronize()
    for k in a:
        assert NR.same_bits(a[k].cpu().numpy(), b[k].cpu().numpy()) and NR.same_bits(h[k], b[k].cpu().numpy()), k
    S = b["S"].cpu().numpy()
    assert (b["status"].cpu().numpy() == 0).all() and np.isfinite(S).all()
    assert float(np.std(S[L + 1, 2].reshape(R, D), axis=1).min()) > 0.0 and not (c["S"] == b["S"]).all()


# ---- the simulator and its scoring tail ----
def _sim_inputs(B, n, rng):
    from epidemicmodeling_amd import batch, synth
    N = 10.0 ** rng.uniform(4, 9, B)
    sp = np.zeros((batch.SIM_PRM_COUNT, B))
    sp[0] = 1 - 100 / N; sp[1] = 100 / N; sp[2] = synth.ALPHA0; sp[3] = 1e-8; sp[4] = 100.0; sp[5] = 1 / 7
    sp[6] = 0.01; sp[7] = synth.MODEL_BETA; sp[8] = 10 / N; sp[9] = 30 / N; sp[10] = 1e-2; sp[11] = 1.0
    sp[batch.SIM_A:batch.SIM_A + n] = rng.random((n, B)) * 0.03
    sp[batch.SIM_U_MAX:batch.SIM_U_MAX + n] = synth.IP_MAXES[:n, None]
    sp[batch.SIM_W:batch.SIM_W + n] = rng.random((n, B)) + 0.5
    return sp


def test_sialpha_sim_and_score_seeded_equal_given_draws(gpu_device):
    import torch
    from epidemicmodeling_amd import _lib, batch
    rng = np.random.default_rng(8)
    B, K, n, Su = 70, 5, 12, 4
    sp = _sim_inputs(B, n, rng)
    u = np.floor(rng.random((K, n, Su)) * 3)
    us = rng.integers(0, Su, B).astype(np.int32)                    # a shared u_series
    z = batch.normal_draws(K, 3, B, SEED, stream=7, device=gpu_device)
    a = batch.sialpha_sim(u, sp, z=z, u_series=us, with_cost=True, device=gpu_device)
    b = batch.sialpha_sim(u, sp, seed=SEED, noise_stream=7, u_series=us, with_cost=True, device=gpu_device)
    c = batch.sialpha_sim(u, sp, seed=SEED, noise_stream=8, u_series=us, with_cost=True, device=gpu_device)
    torch.cuda.synchronize()
    assert list(a) == list(b) == ["s", "i", "alpha", "J0", "J1"]
    for k in a:
        assert NR.same_bits(a[k].cpu().numpy(), b[k].cpu().numpy()), k
    assert not (c["alpha"] == b["alpha"]).all() and bool(torch.isfinite(b["alpha"]).all())
    # the scoring tail: a historic prefix of the two sums, sentinel-filled outputs with guard words
    dev = torch.device(gpu_device)
    t = lambda v, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(v), dtype=dt, device=dev)
    tu, tsp, tus, j0p, j1p = t(u), t(sp), t(us, torch.int32), t(rng.random(B)), t(rng.random(B))
    d = _lib.SimDesc()
    d.abi_version, d.B, d.K, d.Su, d.n_npi, d.noise, d.with_cost, d.prefix_days = _lib.ABI_VERSION, B, K, Su, n, 1, 1, 33
    noise, res = _lib.make_noise_desc(SEED, 7), {}
    p = lambda v: None if v is None else C.c_void_p(v.data_ptr())
    for mode in ("z", "seeded"):
        o = {k: torch.full((cnt + GUARD,), FILL, dtype=torch.float64, device=dev) for k, cnt in (("s", K * B), ("i", K * B), ("alpha", K * B), ("J0", B), ("J1", B))}
        err = C.create_string_buffer(256)
        tail = (p(tus), p(tu), p(tsp), p(z) if mode == "z" else None, p(j0p), p(j1p), p(o["s"]), p(o["i"]), p(o["alpha"]), p(o["J0"]), p(o["J1"]),
                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), err)
        rc = _lib.lib().epi_sialpha_score_device(C.byref(d), *tail) if mode == "z" else \
            _lib.lib().epi_sialpha_score_device_seeded(C.byref(d), C.byref(noise), *tail)
        _lib.check(rc, err)
        torch.cuda.synchronize()
        res[mode] = {k: v.cpu().numpy() for k, v in o.items()}
        for k, v in res[mode].items():
            assert (v[-GUARD:] == FILL).all() and not (v[:-GUARD] == FILL).any(), (mode, k)
    for k in res["z"]:
        assert NR.same_bits(res["z"][k], res["seeded"][k]), k
    assert not NR.same_bits(res["seeded"]["J0"][:B], b["J0"].cpu().numpy())           # the prefix entered


# ---- the random-NPI Monte-Carlo ----
def test_random_npi_mc_seeded_equals_given_draws_and_the_oracle(gpu_device, ref):
    import torch
    from epidemicmodeling_amd import batch, hostapi, synth
    from oracle import oracle_lib as olib
    rng = np.random.default_rng(13)
    R, n_scen, K, n = 3, 30, 5, 12
    sp = _sim_inputs(R, n, rng)
    u_min = np.zeros((n, R)); u_min[3] = 1.0
    seed = 0x1234567890                                             # the same seed for the plans and the noise
    z = batch.normal_draws(K, 3, n_scen * R, seed, device=gpu_device)
    a = batch.random_npi_mc(sp, u_min, n_scen, K, seed=seed, z=z, store_u=True, device=gpu_device)
    b = batch.random_npi_mc(sp, u_min, n_scen, K, seed=seed, noise_seed=seed, store_u=True, device=gpu_device)
    h = hostapi.random_npi_mc(sp, u_min, n_scen, K, seed=seed, noise_seed=seed, store_u=True)
    c = batch.random_npi_mc(sp, u_min, n_scen, K, seed=seed, noise_seed=seed, noise_stream=1, store_u=True, device=gpu_device)
    torch.cuda.synchronize()
    for k in ("u", "J0", "J1"):
        assert NR.same_bits(a[k].cpu().numpy(), b[k].cpu().numpy()) and NR.same_bits(h[k], b[k].cpu().numpy()), k
    assert NR.same_bits(c["u"].cpu().numpy(), b["u"].cpu().numpy()) and not (c["J0"] == b["J0"]).all()   # the plans do not see the noise
    # against the restatements: the oracle's plan, SIalpha_Controlled on the noise restatement's columns, NPICost
    U, gJ0, gJ1 = b["u"].cpu().numpy(), b["J0"].cpu().numpy(), b["J1"].cpu().numpy()
    zr = ref.fill(seed, 0, 0, K, 3, 0, n_scen * R)
    assert NR.same_bits(z.cpu().numpy(), zr)
    lib = olib.lib()
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    for (j, r) in ((0, 0), (13, 2), (14, 1), (29, 2)):
        cc = j * R + r
        plan = olib.random_npi_plan(seed, r, j, n_scen, K, u_min[:, r], synth.IP_MAXES)
        assert np.array_equal(U[:, :, cc].T, plan), (j, r)
        s, i, al = np.zeros(K), np.zeros(K), np.zeros(K)
        aa = np.ascontiguousarray(sp[batch.SIM_A:batch.SIM_A + n, r]); um = np.ascontiguousarray(sp[batch.SIM_U_MAX:batch.SIM_U_MAX + n, r])
        zc = np.ascontiguousarray(zr[:, :, cc])
        lib.orc_sialpha_controlled(dp(plan), C.c_int(n), *[C.c_double(sp[k, r]) for k in (0, 1, 2)], dp(um),
                                   C.c_double(sp[3, r]), C.c_double(sp[4, r]), C.c_double(sp[5, r]), dp(aa),
                                   C.c_double(sp[6, r]), C.c_double(sp[7, r]), C.c_double(sp[8, r]),
                                   C.c_double(sp[9, r]), C.c_double(sp[10, r]), C.c_int(K), C.c_double(1.0), dp(zc), dp(s), dp(i), dp(al))
        nc = np.ascontiguousarray(s * i * al)
        w_all = np.asfortranarray(np.repeat(sp[batch.SIM_W:batch.SIM_W + n, r][:, None], K, axis=1))
        J0, J1 = C.c_double(), C.c_double()
        lib.orc_npi_cost(dp(nc), dp(plan), dp(w_all), C.c_int(n), C.c_int(K), C.byref(J0), C.byref(J1))
        assert gJ0[j, r] == J0.value and gJ1[j, r] == J1.value, (j, r)


# ---- the pipeline ----
def test_smoothed_fan_device_rng(gpu_device):
    import torch
    from epidemicmodeling_amd import batch, pipeline, synth
    w = synth.make_cfg3(6, 40)
    N = np.linspace(1e6, 5e6, 6)
    r, X, summ, z = pipeline.smoothed_fan(w, 70, population=N, seed=7, k0=5, rng="device")
    assert z is None
    zz = batch.normal_draws(35, 3, 6 * 70, 7, device=gpu_device)
    _, X2, summ2, z2 = pipeline.smoothed_fan(w, 70, population=N, seed=7, k0=5, z=zz)
    _, X3, _, _ = pipeline.smoothed_fan(w, 70, population=N, seed=8, k0=5, rng="device")
    torch.cuda.synchronize()
    assert z2 is zz and bool(H.words_equal(X, X2).all()) and not bool(H.words_equal(X, X3).all())
    assert list(summ) == list(summ2)
    for k in summ:
        assert bool(H.words_equal(summ[k], summ2[k]).all()), k
    with pytest.raises(ValueError, match='rng="device" and z together'):
        pipeline.smoothed_fan(w, 70, z=zz, rng="device")
    with pytest.raises(ValueError, match="rng must be"):
        pipeline.smoothed_fan(w, 70, rng="numpy")

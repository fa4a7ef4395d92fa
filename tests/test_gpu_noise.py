"""The seeded standard-normal draws on the device.  The fill kernel equals the restatement tests/noise_ref.c bit
for bit, as double and as float, on windows that reach the high counter words and in launches cut small, in sentinel-filled
outputs with guard words.  Each of the four consumers, called with a seed, equals on every output word the existing call given
z = normal_draws(...) of the same seed and stream -- at the smallest shapes at which the kernels can go wrong.  The same seed
twice gives the same bits, another stream or seed other bits; pipeline.smoothed_fan(rng="device") returns the summary of
smoothed_fan(z=normal_draws(...)); the hostapi twins agree with batch.

Where chance never goes (tests/noise_place.py): the fill kernel at uniforms CHOSEN by inverting Philox -- the far tail, both
branch boundaries, the extremes -- and each of the five seeded consumer kernels at a recorded seed whose first draws hold a
far-tail uniform, against z made by the C restatement (not by the library's fill)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import loglik_ref as LR
from tests import noise_place as NP
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


def _sdraw_raw(case, D, z=None, noise=None, k0=0, clamp=True, storage="f64", out_f32=False, blk=0, groups=0, device="cuda:0", s_term=None,
               P_term=None):
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
    tens = [up(a, ndt) for a in big] + [up(case["prm"]), z, up(s_term), up(P_term)]
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


# ---- where chance never goes: chosen uniforms under the fill kernel, recorded far-tail seeds under the consumers ----
def _placed_windows():
    """(n, stream, row, t0, lane0, t - t0, lane - lane0) of every target of tests/noise_place.py in either slot and as a row-0
    placement, with its 3-day, 5-lane window"""
    rng = np.random.default_rng([SEED & 0xFFFFFFFF, SEED >> 32])
    for n in NP.targets():
        for slot, row0 in ((0, False), (1, False), (0, True)):
            stream, t, row, lane = NP.place(SEED, n, slot, rng, row0_only=row0)
            t0, lane0 = NP.window(t, lane)
            yield n, stream, row, t0, lane0, t - t0, lane - lane0


def test_fill_at_placed_uniforms(gpu_device, ref):
    """The far-tail branch (min(u, 1 - u) < e^-25), both branch boundaries with their neighbours, the two u next to 1/2, every
    power of two and the extremes u = 2^-53, 1 - 2^-53, each put under the fill kernel by inverting Philox (tests/noise_place.py):
    a 3 x 3 x 5 window around the placed counter -- and a 3 x 1 x 5 one where the placement is row 0 -- equals the C restatement
    bit for bit, as double and as float, and the placed element itself is icdf(u) of the target.

    That it bites (scratch builds, never committed; epi_normal_icdf of csrc/noise.hpp): `far = rt > 6.0` fails here at n = 1
    (-8.076571004127453 for -8.076571004130123; n = 0 has rt = 6.06); NE[2] and NE[5] swapped (-8.4256 for -8.2095) and the far
    branch's `rt - 5.0` made `rt - 1.6` (-13.12) fail at the first target, n = 0; every older test of this file passes.  `<= 0.425`
    made `< 0.425` passes, as it must: no lattice point lies on |u - 1/2| = 0.425 (tests/test_noise_place.py asserts it), so the
    two spellings are one function of the 2^52 uniforms; the neighbours either side are what pins the boundary."""
    far = 0
    z_ext = {}
    for n, stream, row, t0, lane0, dt, dl in _placed_windows():
        u = NP.u_of(n)
        zt = ref.icdf([u])[0]
        far += NP.classify(u) == "far"
        for rows in ((3, 1) if row == 0 else (3,)):
            want = ref.fill(SEED, stream, t0, 3, rows, lane0, 5)
            assert want[dt, row, dl] == zt, (n, row, "the window misses the target")
            got = _fill_raw(SEED, stream, t0, 3, rows, lane0, 5)
            assert NR.same_bits(got, want), (n, row, rows, got[dt, row, dl], zt)
            assert NR.same_bits(_fill_raw(SEED, stream, t0, 3, rows, lane0, 5, f32=True), want.astype(np.float32)), (n, row, rows)
            assert got[dt, row, dl] == zt and np.abs(got).max() < 8.2096
            if n in (0, NP.TOP):
                z_ext.setdefault(n, set()).add(float(got[dt, row, dl]))
    assert far >= 3 * 40
    assert len(z_ext[0]) == len(z_ext[NP.TOP]) == 1 and z_ext[0].pop() == -z_ext[NP.TOP].pop()      # equal and opposite


def _far_entries(box):
    """every recorded seed of a box: both tails, and in 'rows3' each of the rows 0 .. 2.  All of them, because a mutation that
    moves a far-tail draw by a few ulp (`far = rt > 6.0`: the near-tail polynomial is still good to 1 .. 8 ulp at these rt = 5.01
    .. 5.18, and at three of the entries to the bit) reaches an output word only where the draw's scale lets it"""
    entries = NP.recorded_seeds()[box]
    assert {e["tail"] for e in entries} == {"lower", "upper"} and {e["row"] for e in entries} == ({0, 1, 2} if box == "rows3" else {0})
    return entries


def _z_with_far_draw(ref, e, nt, rows, lanes):
    """the window [0, nt) x rows x [0, lanes) of the entry's seed by the C restatement, after checking that it holds the recorded
    far-tail draw; and the same array with that one element set to 0"""
    z = ref.fill(e["seed"], 0, 0, nt, rows, 0, lanes)
    assert e["t"] < nt and e["row"] < rows and e["lane"] < lanes
    zt = z[e["t"], e["row"], e["lane"]]
    assert zt == ref.icdf([NP.u_of(e["n"])])[0] and NP.classify(NP.u_of(e["n"])) == "far" and abs(zt) > 6.5, e
    z0 = z.copy()
    z0[e["t"], e["row"], e["lane"]] = 0.0
    return z, z0


@pytest.mark.parametrize("out_f32", [False, True])                 # sdraw_paths_seeded<0> and <1>
def test_sdraw_seeded_far_tail_draw(gpu_device, ref, out_f32):
    """A recorded far-tail draw inside sdraw_paths_seeded: the seeded call equals the z call given the C restatement's array on
    every output word, that array holds the draw, and the draw enters X at its path.

    That it bites (scratch builds, never committed): NE[2] / NE[5] swapped and `rt - 1.6` in the far branch
    (test_fill_at_placed_uniforms) fail here in both instantiations (X, at the first entry), with every older test of this file
    passing; `far = rt > 6.0` fails <0> (X, the row-2 entry n = 13 597) and passes <1>: it moves these draws by at most 8 ulp, which
    the float rounding of X absorbs; sd_ldz taking row 0's draw for row 2 fails both."""
    import torch
    from epidemicmodeling_amd import _lib
    B, D, T = 3, 70, 6
    w, case = _case(B, T)
    for e in _far_entries("rows3"):
        z, z0 = _z_with_far_draw(ref, e, T, 3, B * D)
        for clamp in (False, True):
            kw = dict(clamp=clamp, out_f32=out_f32)
            want = _sdraw_raw(case, D, z=torch.as_tensor(z, device=gpu_device), **kw)
            got = _sdraw_raw(case, D, noise=_lib.make_noise_desc(e["seed"], 0), **kw)
            for k in SD_NAMES:
                assert NR.same_bits(got[k], want[k]), (k, kw, e)
            if not clamp:                                                             # unclamped: a draw cannot be cut away
                without = _sdraw_raw(case, D, z=torch.as_tensor(z0, device=gpu_device), **kw)
                differs = without["X"] != got["X"]
        assert differs[:, :, e["lane"]].any(), e                                  # the draw enters its own path
        assert not np.delete(differs, e["lane"], axis=2).any(), e                 # and no other


def test_ar_forecast_seeded_far_tail_draw(gpu_device, ref):
    """A recorded far-tail draw of row 0 inside ar_simulate_seeded (the single row of epi_arfc_*), as in
    test_sdraw_seeded_far_tail_draw.  That it bites: the three far-branch mutations each fail here (S, at n = 10 855)."""
    import torch
    from epidemicmodeling_amd import batch, hostapi
    rng = np.random.default_rng(5)
    R, D, L, p, Hh = 2, 35, 20, 3, 5
    B = R * D                                                      # 70 chains: the box's 64 lanes, and a second 64-lane workgroup
    seg = 0.3 + 0.05 * np.cumsum(rng.standard_normal((L, R)), axis=0) * 0.2
    beta, s0 = np.full(R, 0.2), np.full(R, 0.95)
    args = (seg, beta, s0, 1 - s0, 0.5, p, Hh, D)
    for e in _far_entries("row0"):
        z, z0 = _z_with_far_draw(ref, e, Hh, 1, B)
        a = batch.ar_forecast(*args, z=torch.as_tensor(z[:, 0].copy(), device=gpu_device), device=gpu_device)
        a0 = batch.ar_forecast(*args, z=torch.as_tensor(z0[:, 0].copy(), device=gpu_device), device=gpu_device)
        b = batch.ar_forecast(*args, seed=e["seed"], device=gpu_device)
        h = hostapi.ar_forecast(*args, seed=e["seed"])
        torch.cuda.synchronize()
        for k in a:
            assert NR.same_bits(a[k].cpu().numpy(), b[k].cpu().numpy()) and NR.same_bits(h[k], b[k].cpu().numpy()), (k, e)
        assert (b["status"].cpu().numpy() == 0).all()
        differs = (a0["S"] != b["S"]).cpu().numpy()
        assert differs[:, :, e["lane"]].any() and not np.delete(differs, e["lane"], axis=2).any(), e


def _score_raw(d, u, sp, us, j0p, j1p, z=None, noise=None, device="cuda:0"):
    """epi_sialpha_score_device (z) or epi_sialpha_score_device_seeded (noise) on sentinel-filled outputs with guard words"""
    import torch
    from epidemicmodeling_amd import _lib
    dev = torch.device(device)
    K, B = d.K, d.B
    t = lambda v, dt=torch.float64: None if v is None else torch.as_tensor(np.ascontiguousarray(v), dtype=dt, device=dev)
    p = lambda v: None if v is None else C.c_void_p(v.data_ptr())
    tens = [t(us, torch.int32), t(u), t(sp), t(z), t(j0p), t(j1p)]
    o = {k: torch.full((cnt + GUARD,), FILL, dtype=torch.float64, device=dev) for k, cnt in (("s", K * B), ("i", K * B), ("alpha", K * B), ("J0", B), ("J1", B))}
    err = C.create_string_buffer(256)
    tail = (*[p(v) for v in tens], p(o["s"]), p(o["i"]), p(o["alpha"]), p(o["J0"]), p(o["J1"]), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), err)
    rc = _lib.lib().epi_sialpha_score_device(C.byref(d), *tail) if noise is None else \
        _lib.lib().epi_sialpha_score_device_seeded(C.byref(d), C.byref(noise), *tail)
    _lib.check(rc, err)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in o.items()}
    for k, v in res.items():
        assert (v[-GUARD:] == FILL).all() and not (v[:-GUARD] == FILL).any(), k
    return {k: v[:-GUARD] for k, v in res.items()}


def test_sialpha_sim_and_score_seeded_far_tail_draw(gpu_device, ref):
    """A recorded far-tail draw inside sialpha_sim_seeded, through epi_sialpha_sim_device_seeded (batch.sialpha_sim) and through
    the scoring tail, as in test_sdraw_seeded_far_tail_draw.  That it bites: the three far-branch mutations each fail here
    (`far = rt > 6.0` at the row-1 entry n = 31 146, i; the other two at the first entry, s)."""
    import torch
    from epidemicmodeling_amd import _lib, batch
    rng = np.random.default_rng(8)
    B, K, n, Su = 70, 5, 12, 4
    sp = _sim_inputs(B, n, rng)
    u = np.floor(rng.random((K, n, Su)) * 3)
    us = rng.integers(0, Su, B).astype(np.int32)
    j0p, j1p = rng.random(B), rng.random(B)
    d = _lib.SimDesc()
    d.abi_version, d.B, d.K, d.Su, d.n_npi, d.noise, d.with_cost, d.prefix_days = _lib.ABI_VERSION, B, K, Su, n, 1, 1, 33
    for e in _far_entries("rows3"):
        z, z0 = _z_with_far_draw(ref, e, K, 3, B)
        tz, tz0 = (torch.as_tensor(v, device=gpu_device) for v in (z, z0))
        a = batch.sialpha_sim(u, sp, z=tz, u_series=us, with_cost=True, device=gpu_device)
        a0 = batch.sialpha_sim(u, sp, z=tz0, u_series=us, with_cost=True, device=gpu_device)
        b = batch.sialpha_sim(u, sp, seed=e["seed"], u_series=us, with_cost=True, device=gpu_device)
        torch.cuda.synchronize()
        a, a0, b = ({k: v.cpu().numpy() for k, v in r.items()} for r in (a, a0, b))
        sa = _score_raw(d, u, sp, us, j0p, j1p, z=z)
        sa0 = _score_raw(d, u, sp, us, j0p, j1p, z=z0)
        sb = _score_raw(d, u, sp, us, j0p, j1p, noise=_lib.make_noise_desc(e["seed"], 0))
        for x, x0, y in ((a, a0, b), (sa, sa0, sb)):
            assert list(x) == ["s", "i", "alpha", "J0", "J1"]
            for k in x:
                assert NR.same_bits(x[k], y[k]), (k, e)
            name = ("s", "i", "alpha")[e["row"]]
            differs = (x0[name] != y[name]).reshape(K, B)
            assert differs[:, e["lane"]].any() and not np.delete(differs, e["lane"], axis=1).any(), e
            for k in ("s", "i", "alpha", "J0", "J1"):                              # nothing of another chain moves
                dk = (x0[k] != y[k]).reshape(-1, B)
                assert not np.delete(dk, e["lane"], axis=1).any(), (k, e)
            assert np.isfinite(y["alpha"]).all()


def test_random_npi_mc_seeded_far_tail_draw(gpu_device, ref):
    """A recorded far-tail draw inside random_npi_mc_seeded, as in test_sdraw_seeded_far_tail_draw.  That it bites: the three
    far-branch mutations each fail here (J0; `far = rt > 6.0` at the row-2 entry of the upper tail)."""
    import torch
    from epidemicmodeling_amd import batch, hostapi
    rng = np.random.default_rng(13)
    R, n_scen, K, n = 3, 30, 5, 12                                  # 90 chains, chain = scenario * R + region
    sp = _sim_inputs(R, n, rng)
    u_min = np.zeros((n, R)); u_min[3] = 1.0
    for e in _far_entries("rows3"):
        z, z0 = _z_with_far_draw(ref, e, K, 3, n_scen * R)
        kw = dict(seed=0x1234567890, store_u=True)
        a = batch.random_npi_mc(sp, u_min, n_scen, K, z=torch.as_tensor(z, device=gpu_device), device=gpu_device, **kw)
        a0 = batch.random_npi_mc(sp, u_min, n_scen, K, z=torch.as_tensor(z0, device=gpu_device), device=gpu_device, **kw)
        b = batch.random_npi_mc(sp, u_min, n_scen, K, noise_seed=e["seed"], device=gpu_device, **kw)
        h = hostapi.random_npi_mc(sp, u_min, n_scen, K, noise_seed=e["seed"], **kw)
        torch.cuda.synchronize()
        for k in ("u", "J0", "J1"):
            assert NR.same_bits(a[k].cpu().numpy(), b[k].cpu().numpy()) and NR.same_bits(h[k], b[k].cpu().numpy()), (k, e)
        j, r = divmod(e["lane"], R)
        differs = (a0["J0"] != b["J0"]).cpu().numpy() | (a0["J1"] != b["J1"]).cpu().numpy()
        assert differs[j, r] and differs.sum() == 1, e

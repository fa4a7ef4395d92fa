"""The smoother draws on the device (epi_sdraw_run_device / _host, batch.smoother_draws, hostapi.smoother_draws,
pipeline.smoothed_fan): X, J, L, rank and status equal the restatement tests/sdraw_ref.py of DESIGN.md §4.16 bit for bit -- any
NaN equal to any NaN.  Every output starts as a poison value and carries guard elements behind it; the workspace is poisoned
too.  The shapes are the smallest that reach every edge: B = 5 x D = 3, 64, 70 (a wavefront straddles chain borders, the last
one is partly empty), B = 21 in 8-chain blocks (a partial block), B = 70 from a live runner (more than one wavefront of chains),
and launches cut through a small bound."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import loglik_ref as LR
from tests import sdraw_ref as SR

pytestmark = pytest.mark.gpu

FILL, I32_FILL, GUARD = -98765.4321, -12345, 8
NAMES = ("X", "rank", "status", "J", "L")
I32 = ("rank", "status")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return SR.SdrawRef(tmp_path_factory.mktemp("sdraw_ref"))


@functools.lru_cache(maxsize=None)
def _case(B, T):
    from epidemicmodeling_amd import synth
    w = synth.make_cfg3(B, T)
    return w, SR.case_of(w, H.oracle_batch(w))


def _run_device(case, D, z=None, s_term=None, P_term=None, k0=0, clamp=True, storage="f64", out_f32=False, blk=0, groups=0,
                device="cuda:0"):
    """epi_sdraw_run_device on poison-filled outputs with GUARD elements behind each and a poisoned workspace.  The case's
    classic arrays are uploaded chain-blocked with blk (padding lanes = NaN: never read).  Returns (dict of NumPy arrays, dict
    name -> True if the guards still hold the poison)."""
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
    tens = [up(a, ndt) for a in big] + [up(case["prm"]), up(z, None if z is None else z.dtype), up(s_term), up(P_term)]
    shapes = _lib.sdraw_shapes(B, T, D, k0)
    d = _lib.make_sdraw_desc(B, T, D, k0, clamp, blk, int(storage == "f32"), int(z is not None and z.dtype == np.float32), int(out_f32),
                             test_launch_groups=groups)
    ins = _lib.SdrawInputs()
    for k, v in zip(_lib.SDRAW_IN_NAMES, tens):
        setattr(ins, k, None if v is None else C.c_void_p(v.data_ptr()))
    tdt = {k: torch.int32 if k in I32 else (torch.float32 if k == "X" and out_f32 else torch.float64) for k in NAMES}
    fill = {k: I32_FILL if k in I32 else FILL for k in NAMES}
    flat = {k: torch.full((int(np.prod(shapes[k])) + GUARD,), fill[k], dtype=tdt[k], device=dev) for k in NAMES}
    outs = _lib.SdrawOutputs()
    for k in NAMES:
        setattr(outs, k, C.c_void_p(flat[k].data_ptr()))
    err = C.create_string_buffer(256)
    n = C.c_size_t(0)
    _lib.check(_lib.lib().epi_sdraw_workspace_bytes(C.byref(d), C.byref(n), err), err)
    ws = torch.full((n.value // 8 + GUARD,), FILL, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev)
    rc = _lib.lib().epi_sdraw_run_device(C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(ws.data_ptr()), n.value,
                                         C.c_void_p(st.cuda_stream), err)
    _lib.check(rc, err)
    torch.cuda.synchronize(dev)
    res, clean = {}, {"workspace": bool((ws[n.value // 8:] == FILL).all())}
    for k in NAMES:
        h = flat[k].cpu().numpy()
        cnt = int(np.prod(shapes[k]))
        clean[k] = bool((h[cnt:] == np.asarray(fill[k], dtype=h.dtype)).all())
        res[k] = h[:cnt].reshape(shapes[k])
    return res, clean


def _assert_equal(got, clean, want, what):
    assert clean["workspace"], f"{what}: wrote behind the workspace"
    for k, v in got.items():
        assert clean[k], f"{what}: {k} wrote outside its elements"
        assert SR.same_bits(v, want[k]), f"{what}: {k} differs from the restatement"
        assert not (v == np.asarray(I32_FILL if k in I32 else FILL, dtype=v.dtype)).any(), f"{what}: {k} keeps poison"


@pytest.mark.parametrize("D", [3, 64, 70])
def test_b5_t33(gpu_device, ref, D):
    """k0 = 0 and 11, clamp 0 and 1, z = None and random z; D = 70 also in launches of one workgroup"""
    w, case = _case(5, 33)
    for k0 in (0, 11):
        for clamp in (True, False):
            for noise in (False, True):
                z = SR.draws(w.T, k0, w.B, D, seed=D + k0) if noise else None
                want = ref.run(case, D, z, k0=k0, clamp=clamp)
                got, clean = _run_device(case, D, z, k0=k0, clamp=clamp, groups=1 if D == 70 and noise else 0)
                _assert_equal(got, clean, want, f"D={D} k0={k0} clamp={clamp} noise={noise}")


@pytest.mark.parametrize("blk", [0, 8])
def test_b21_t9_layouts_and_types(gpu_device, ref, blk):
    w, case = _case(21, 9)
    for storage, zt, of in (("f64", np.float64, False), ("f32", np.float64, False), ("f64", np.float32, True), ("f32", np.float32, True)):
        z = SR.draws(w.T, 0, w.B, 7, seed=3, dtype=zt)
        want = ref.run(case, 7, z, storage=storage, out_f32=of)
        got, clean = _run_device(case, 7, z, storage=storage, out_f32=of, blk=blk)
        _assert_equal(got, clean, want, f"blk={blk} {storage} z={zt.__name__} X f32={of}")


@pytest.mark.parametrize("storage", ["f64"])
def test_zero_draws_are_the_runners_s_smooth(gpu_device, storage):
    """property (b) on the device: from a live runner's arrays as they lie, z = None gives the runner's own S_SMOOTH, word for word"""
    import torch
    from epidemicmodeling_amd import batch, synth
    w = synth.make_cfg3(70, 40)
    dw = batch.DeviceWorkload(w)
    for lane_block in (0, "auto"):
        r = batch.EkfRunner(dw, ["S_PLUS", "P_PLUS", "S_MINUS", "P_MINUS", "S_SMOOTH"], lane_block=lane_block, storage=storage)
        r.run()
        blk = 0 if r.blk == w.B else r.blk
        res = batch.smoother_draws(r.out["S_PLUS"], r.out["P_PLUS"], r.out["S_MINUS"], r.out["P_MINUS"], dw.prm, 1, lane_block=blk, B=w.B)
        torch.cuda.synchronize()
        ss = r.out["S_SMOOTH"]
        if blk:
            ss = ss.permute(0, 2, 1, 3).reshape(w.T, 3, -1)[:, :, :w.B]
        assert list(res) == ["X", "rank", "status"]
        assert bool(H.words_equal(res["X"], ss.contiguous()).all()), lane_block
        assert not (res["status"] & 1).any()


def test_planted_days(gpu_device, ref):
    case = SR.planted_case()
    for clamp in (True, False):
        z = SR.draws(case["T"], 0, case["B"], 3, seed=6)
        want = ref.run(case, 3, z, clamp=clamp)
        got, clean = _run_device(case, 3, z, clamp=clamp, blk=2)
        _assert_equal(got, clean, want, f"planted clamp={clamp}")


def test_smoothed_fan(gpu_device, ref):
    """its summary equals ensemble_summary of the restatement's X; the same seed gives the same bits; the draws captured in a
    graph and replayed once into poisoned outputs"""
    import torch
    from epidemicmodeling_amd import batch, pipeline, synth
    w = synth.make_cfg3(6, 40)
    N = np.linspace(1e6, 5e6, 6)
    r, X, summ, z = pipeline.smoothed_fan(w, 128, population=N, seed=7)
    torch.cuda.synchronize()
    case = SR.case_of(w, H.oracle_batch(w))
    want = ref.run(case, 128, z.cpu().numpy(), s_term=case["S_SMOOTH"][-1], P_term=case["P_SMOOTH"][-1])
    assert SR.same_bits(X.cpu().numpy(), want["X"])
    ws = batch.ensemble_summary(torch.as_tensor(want["X"]).cuda(), 6, 128, population=N)
    for k in ws:
        assert bool(H.words_equal(summ[k], ws[k]).all()), k
    _, X2, summ2, z2 = pipeline.smoothed_fan(w, 128, population=N, seed=7)
    assert bool(H.words_equal(z, z2).all()) and bool(H.words_equal(X, X2).all()) and all(bool(H.words_equal(summ[k], summ2[k]).all()) for k in ws)
    # the draws alone in a graph, on a side stream
    dw = batch.DeviceWorkload(w)
    args = (r.out["S_PLUS"], r.out["P_PLUS"], r.out["S_MINUS"], r.out["P_MINUS"], dw.prm, 128)
    blk = 0 if r.blk == w.B else r.blk
    kw = dict(z=z, s_term=torch.as_tensor(case["S_SMOOTH"][-1]).cuda(), P_term=torch.as_tensor(case["P_SMOOTH"][-1]).cuda(),
              lane_block=blk, B=w.B)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        res = batch.smoother_draws(*args, **kw)
    res["X"].fill_(FILL)
    res["rank"].fill_(I32_FILL)
    res["status"].fill_(I32_FILL)
    g.replay()
    torch.cuda.synchronize()
    for k in ("X", "rank", "status"):
        assert SR.same_bits(res[k].cpu().numpy(), want[k]), k


def test_hostapi_equals_batch(gpu_device, ref):
    import torch
    from epidemicmodeling_amd import batch, hostapi
    w, case = _case(21, 9)
    z = SR.draws(w.T, 2, w.B, 5, seed=9, dtype=np.float32)
    big = [np.ascontiguousarray(LR.to_blocked(case[k], 8, np.nan)) for k in SR.BIG]
    kw = dict(z=z, s_term=case["S_SMOOTH"][-1], P_term=case["P_SMOOTH"][-1], k0=2, lane_block=8, B=21, outputs=NAMES)
    host = hostapi.smoother_draws(*big, case["prm"], 5, out_dtype=np.float32, **kw)
    dev = batch.smoother_draws(*(torch.as_tensor(a).cuda() for a in big), case["prm"], 5, out_dtype=torch.float32, **kw)
    torch.cuda.synchronize()
    want = ref.run(case, 5, z, s_term=kw["s_term"], P_term=kw["P_term"], k0=2, out_f32=True)
    assert list(host) == list(dev) == list(NAMES)
    for k in host:
        d = dev[k].cpu().numpy()
        assert host[k].dtype == d.dtype and SR.same_bits(host[k], d) and SR.same_bits(host[k], want[k]), k

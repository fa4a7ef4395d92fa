"""The forward-backward filter fusion on the device (epi_fuse_run_device / _host, batch.two_filter, hostapi.two_filter,
pipeline.two_filter_smooth): s, P, d2, rank and status equal bit for bit -- any NaN equal to any NaN -- to the restatement
tests/two_filter_ref.py of DESIGN.md §4.9.  Every output starts as a poison value and carries guard elements; the
restatement's results are computed once per case and shared.  Bit 1 of status (a Jacobi sweep cap) is the restatement's too:
the oracle's iteration has the kernel's caps and reports them (test_an_item_at_the_sweep_cap)."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import two_filter_ref as TF

pytestmark = pytest.mark.gpu

FILL, I32_FILL, GUARD = -98765.4321, -12345, 8
FORMS = [(0, 0), (0, 1), (1, 0)]


@functools.lru_cache(maxsize=None)
def _planted(m, T, B):
    return TF.planted(m, T, B, seed=100 * m + B, indefinite=True, nonfinite=True)


@functools.lru_cache(maxsize=None)
def _planted_ref(m, T, B, form, p_solver, storage):
    return TF.fuse(*_planted(m, T, B), form, p_solver, storage=storage)


def _run_device(arrs, m, B, T, form, p_solver, storage="f64", blk=0, outputs=None, stream=None, device="cuda:0"):
    """epi_fuse_run_device on poison-filled outputs with GUARD elements behind each.  arrs: classic NumPy [T, rows, B]; with
    blk they are uploaded chain-blocked (padding lanes = NaN: never read) and the outputs are unblocked for the comparison.
    Returns (dict of NumPy arrays under batch.two_filter's names, dict name -> True if the guards and -- blocked -- the
    padding lanes still hold the poison)."""
    import torch
    from epidemicmodeling_amd import _lib
    dev = torch.device(device)
    ndt, tdt = (np.float32, torch.float32) if storage == "f32" else (np.float64, torch.float64)
    ups = []
    for a in arrs:
        a = np.asarray(a).astype(ndt)
        if blk:
            a = TF.to_blocked(a, blk, fill=np.nan)
        ups.append(torch.as_tensor(np.ascontiguousarray(a), device=dev))
    names = _lib.FUSE_OUT_NAMES if outputs is None else outputs
    shapes = _lib.fuse_shapes(m, B, T, blk)
    d = _lib.make_fuse_desc(m, B, T, form, p_solver=p_solver, lane_block=blk, storage=int(storage == "f32"))
    ins = _lib.FuseInputs()
    for k, v in zip(_lib.FUSE_IN_NAMES, ups):
        setattr(ins, k, C.c_void_p(v.data_ptr()))
    odt = {"s_out": tdt, "P_out": tdt, "d2": torch.float64, "rank": torch.int32, "status": torch.int32}
    flat = {k: torch.full((int(np.prod(shapes[k])) + GUARD,), I32_FILL if odt[k] == torch.int32 else FILL, dtype=odt[k], device=dev)
            for k in names}
    outs = _lib.FuseOutputs()
    for k in names:
        setattr(outs, k, C.c_void_p(flat[k].data_ptr()))
    st = torch.cuda.current_stream(dev) if stream is None else stream
    err = C.create_string_buffer(256)
    rc = _lib.lib().epi_fuse_run_device(C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(st.cuda_stream), err)
    _lib.check(rc, err)
    torch.cuda.synchronize(dev)
    res, clean = {}, {}
    key = {"s_out": "s", "P_out": "P", "d2": "d2", "rank": "rank", "status": "status"}
    for k in names:
        h = flat[k].cpu().numpy()
        n = int(np.prod(shapes[k]))
        poison = I32_FILL if h.dtype == np.int32 else h.dtype.type(FILL)
        ok = bool((h[n:] == poison).all())
        a = h[:n].reshape(shapes[k])
        if blk and k in ("s_out", "P_out") and a.ndim == 4:   # lane_block = B is the classic layout: one block, no padding
            Tn, nblk, rows, bl = a.shape
            pad = a.transpose(0, 2, 1, 3).reshape(Tn, rows, nblk * bl)[:, :, B:]
            ok = ok and bool((pad == poison).all())
            a = TF.from_blocked(a, B)
        res[key[k]], clean[key[k]] = a, ok
    return res, clean


def _assert_equal(got, clean, want, what):
    for k, v in got.items():
        assert clean[k], f"{what}: {k} wrote outside its elements"
        assert TF.same_bits(v, want[k]), f"{what}: {k} differs from the restatement"
        if v.dtype.kind == "f":
            assert not (v == v.dtype.type(FILL)).any(), f"{what}: {k} keeps poison"
        else:
            assert not (v == I32_FILL).any(), f"{what}: {k} keeps poison"


def test_planted_set_reaches_ranks_and_routes():
    """the condition the planted cases stand on, asserted on the restatement: at least three distinct ranks, both pseudo-
    inverse routes (0 / 2: factorisation, 1: two-sided Jacobi), one non-finite item"""
    for m in (3, 6):
        r = _planted_ref(m, 5, 70, 1, 0, "f64")
        ranks = set(r["rank"].ravel().tolist())
        assert ranks >= set(range(m + 1)) | {-1}, ranks
        routes = set(r["route"].ravel().tolist())
        assert 1 in routes and (0 in routes or 2 in routes), routes
        assert (r["rank"] == -1).sum() == 1 and r["status"].sum() == 1


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("form, p_solver", FORMS)
@pytest.mark.parametrize("m", [3, 6])
def test_planted_ranks_bit_for_bit(gpu_device, m, form, p_solver, storage):
    """B = 70 = 64 + 6 (a partial last wavefront: the tail lanes run the ballots on a clamped item), T = 5, ranks 0 .. m, one
    indefinite S, one non-finite day; classic layout and 40-chain blocks (70 is no multiple of 40)."""
    T, B = 5, 70
    want = _planted_ref(m, T, B, form, p_solver, storage)
    if storage == "f64":
        assert len(set(want["rank"].ravel().tolist())) >= 3 and 1 in want["route"]
    for blk in (0, 40):
        got, clean = _run_device(_planted(m, T, B), m, B, T, form, p_solver, storage=storage, blk=blk)
        _assert_equal(got, clean, want, f"m={m} form={form} p_solver={p_solver} {storage} blk={blk}")


@pytest.mark.parametrize("m", [3, 6])
def test_single_item(gpu_device, m):
    """B = 1, T = 1: one live lane, every other lane of the wavefront clamped onto it"""
    arrs = TF.planted(m, 1, 1, seed=9 + m, indefinite=False, nonfinite=False)
    arrs[1][0, :, 0] = np.eye(m).ravel() * 2.0               # rank m
    arrs[3][0, :, 0] = np.diag(np.arange(1.0, m + 1.0)).ravel()
    for form, ps in FORMS:
        want = TF.fuse(*arrs, form, ps)
        assert want["rank"][0, 0] == m
        got, clean = _run_device(arrs, m, 1, 1, form, ps)
        _assert_equal(got, clean, want, f"single item m={m} form={form} p_solver={ps}")


def test_optional_outputs(gpu_device):
    """each of s_out / P_out / d2 alone, without rank and status"""
    m, T, B = 6, 5, 70
    for only in ("s_out", "P_out", "d2"):
        for form, ps in ((0, 0), (1, 0)):
            want = _planted_ref(m, T, B, form, ps, "f64")
            got, clean = _run_device(_planted(m, T, B), m, B, T, form, ps, outputs=(only,))
            assert list(got) == [{"s_out": "s", "P_out": "P", "d2": "d2"}[only]]
            _assert_equal(got, clean, want, f"only {only} form={form}")


@functools.lru_cache(maxsize=None)
def _real_case(which):
    """(w, forward oracle outputs, backward oracle outputs) of the 3-state batch (7 chains x 40 days) or the 6-state sweep
    (10 chains x (30 + 30 NaN-horizon) days)"""
    from epidemicmodeling_amd import synth
    w = synth.make_cfg3(7, 40) if which == 3 else synth.make_cfg4(2, 5, 30, 30)
    return w, H.oracle_batch(w), H.oracle_batch(synth.as_backward(w))


@pytest.mark.parametrize("which, blk", [(3, 4), (6, 4), (6, 0)])
def test_real_filter_outputs_from_blocked_runners(gpu_device, which, blk):
    """Forward and reverse-time filters run on the device with chain-blocked outputs (4-chain blocks: 7 and 10 chains are no
    multiples of 4) and fused from the runners' arrays as they lie; the restatement is fed with the ORACLE's forward and
    backward outputs.  On the 6-state case the restatement reports rank < 6 on at least a tenth of the items (146 of 600
    when this was written)."""
    import torch
    from epidemicmodeling_amd import batch, synth
    w, of, ob = _real_case(which)
    m = which
    want = TF.fuse(of["S_PLUS"], of["P_PLUS"], ob["S_MINUS"], ob["P_MINUS"], 1)
    if which == 6:
        assert (want["rank"] < 6).mean() >= 0.1, (want["rank"] < 6).mean()
    rf = batch.EkfRunner(batch.DeviceWorkload(w), ["S_PLUS", "P_PLUS"], lane_block=blk)
    rb = batch.EkfRunner(batch.DeviceWorkload(synth.as_backward(w)), ["S_MINUS", "P_MINUS"], lane_block=blk)
    assert rf.blk == (blk or w.B) and rb.blk == rf.blk
    rf.run()
    rb.run()
    for form, ps in FORMS:
        want = TF.fuse(of["S_PLUS"], of["P_PLUS"], ob["S_MINUS"], ob["P_MINUS"], form, ps)
        got = batch.two_filter(rf.out["S_PLUS"], rf.out["P_PLUS"], rb.out["S_MINUS"], rb.out["P_MINUS"], form=form, p_solver=ps,
                               lane_block=blk, B=w.B)
        torch.cuda.synchronize()
        for k in ("s", "P"):
            a = got[k].cpu().numpy()
            assert a.shape == ((w.T, rf.nblk, m * (m if k == "P" else 1), blk) if blk else (w.T, m * (m if k == "P" else 1), w.B))
            a = TF.from_blocked(a, w.B) if blk else a
            assert TF.same_bits(a, want[k]), f"{which}-state form={form} p_solver={ps}: {k}"
        for k in ("d2", "rank", "status"):
            assert TF.same_bits(got[k].cpu().numpy(), want[k]), f"{which}-state form={form} p_solver={ps}: {k}"


def test_pipeline_two_filter_smooth(gpu_device):
    """pipeline.two_filter_smooth on the 3-state case equals the pieces run by hand (the restatement on the oracle's forward
    and backward outputs); with backward="plus", form=0 it is the reference's formula on PLUS with PLUS"""
    import torch
    from epidemicmodeling_amd import pipeline
    w, of, ob = _real_case(3)
    for kw, want in ((dict(), TF.fuse(of["S_PLUS"], of["P_PLUS"], ob["S_MINUS"], ob["P_MINUS"], 1)),
                     (dict(backward="plus", form=0), TF.fuse(of["S_PLUS"], of["P_PLUS"], ob["S_PLUS"], ob["P_PLUS"], 0, 0))):
        res = pipeline.two_filter_smooth(w, **kw)
        torch.cuda.synchronize()
        assert res["B"] == w.B and res["forward"].dw.model == "SIAlphaModelEKF" and res["backward"].dw.model == "SIAlphaModelBackwardEKF"
        blk = res["lane_block"]
        for k in ("s", "P"):
            a = res["fused"][k].cpu().numpy()
            a = TF.from_blocked(a, w.B) if a.ndim == 4 else a
            assert TF.same_bits(a, want[k]), (kw, k, blk)
        for k in ("d2", "rank", "status"):
            assert TF.same_bits(res["fused"][k].cpu().numpy(), want[k]), (kw, k)
    with pytest.raises(ValueError, match="backward must be"):
        pipeline.two_filter_smooth(w, backward="both")


def test_on_a_side_stream_between_two_kernels(gpu_device):
    """enqueued on a non-default stream after a kernel that produces its inputs and before one that consumes its outputs;
    one synchronise at the end"""
    import torch
    from epidemicmodeling_amd import batch
    m, T, B = 6, 5, 70
    want = _planted_ref(m, T, B, 1, 0, "f64")
    host = [torch.as_tensor(np.ascontiguousarray(a)) for a in _planted(m, T, B)]
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        half = [h.cuda(non_blocking=False) * 0.5 for h in host]
        ins = [x + x for x in half]                           # produced on `st`: x * 0.5 * 2 is exact
        got = batch.two_filter(*ins, form=1, stream=st)
        total = got["rank"].sum()                            # consumes an output on `st`
    st.synchronize()
    for k in ("s", "P", "d2", "rank", "status"):
        assert TF.same_bits(got[k].cpu().numpy(), want[k]), k
    assert int(total.item()) == int(want["rank"].sum())


def test_host_entry_point(gpu_device):
    """epi_fuse_run_host through hostapi.two_filter, float64 and float32"""
    from epidemicmodeling_amd import hostapi
    m, T, B = 3, 5, 70
    arrs = _planted(m, T, B)
    for storage, dt in (("f64", np.float64), ("f32", np.float32)):
        want = _planted_ref(m, T, B, 0, 0, storage)
        got = hostapi.two_filter(*(a.astype(dt) for a in arrs), form=0, p_solver=0)
        for k in ("s", "P", "d2", "rank", "status"):
            assert TF.same_bits(got[k], want[k]), (storage, k)


@pytest.mark.parametrize("form, p_solver", FORMS)
def test_an_item_at_the_sweep_cap(gpu_device, form, p_solver):
    """TF.CAPPED, the example a random hunt met: item (day 12, chain 5) runs the one-sided Jacobi iteration to its 30th sweep.
    Every output bit for bit, status exactly [0 0 0 1 0 2 0 ...] in double storage (bit 0: the planted non-finite item of
    chain 3) and without bit 1 in float storage, classic and chain-blocked."""
    m, T, B, seed = TF.CAPPED
    arrs = TF.planted(m, T, B, seed)
    for storage, st5 in (("f64", 2), ("f32", 0)):
        want = TF.fuse(*arrs, form, p_solver, storage=storage)
        assert list(want["status"]) == [0, 0, 0, 1, 0, st5] + [0] * 8
        for blk in (0, 8):
            got, clean = _run_device(arrs, m, B, T, form, p_solver, storage=storage, blk=blk, device=gpu_device)
            _assert_equal(got, clean, want, f"form={form} p_solver={p_solver} {storage} blk={blk}")

"""The innovation whiteness diagnostics on the device (epi_idiag_run_device / _host, batch.innovation_diagnostics,
hostapi.innovation_diagnostics, pipeline.filter_diagnostics / tune_filter(min_lb_p=...)): every output equals the restatement
tests/innov_diag_ref.py of DESIGN.md §4.22 bit for bit -- any NaN equal to any NaN.  Every output starts as a poison value and
carries guard elements behind it; the workspace is poisoned and guarded too; no output word keeps poison.  The shapes
(innov_diag_ref.CASES) are the smallest that reach every edge: B = 70 (a partial last wavefront), B = 1, T = 45 (one full and
one partial 32-step block), T = 100 with 40 lags (two blocks ahead), every lag count, the windows, both layouts and storages,
flip, no S, the planted missing days, bad values and degenerate chains."""
import ctypes as C

import numpy as np
import pytest

from tests import innov_diag_ref as DR
from tests.test_innov_diag_emu import blocked_input

pytestmark = pytest.mark.gpu

FILL, I32_FILL, GUARD = -98765.4321, -12345, 8


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return DR.InnovDiagRef(tmp_path_factory.mktemp("innov_diag_ref"))


def run_device(e, S, H=10, k0=0, k1=None, flip=False, storage="f64", blk=0, outputs=None, device="cuda:0", e_dev=None, B=None):
    """epi_idiag_run_device on poison-filled outputs with GUARD elements behind each and a poisoned, guarded workspace.  e
    [T, B] is uploaded as the runner leaves it (blocked_input: padding lanes NaN), or e_dev is taken as it lies.  Returns (dict
    of NumPy arrays, dict name -> True if the guards still hold the poison)."""
    import torch
    from epidemicmodeling_amd import _lib
    dev = torch.device(device)
    if e_dev is None:
        T, B = e.shape
        e_dev = torch.as_tensor(blocked_input(e, blk, storage), device=dev)
    T = int(e_dev.shape[0])
    S_dev = None if S is None else torch.as_tensor(np.ascontiguousarray(S, dtype=np.float64), device=dev)
    names = _lib.idiag_out_names(outputs)
    shapes = _lib.idiag_shapes(B, H)
    d = _lib.make_idiag_desc(B, T, H, k0, k1, int(bool(flip)), blk, int(storage == "f32"))
    ins = _lib.IdiagInputs()
    ins.e, ins.S = C.c_void_p(e_dev.data_ptr()), None if S_dev is None else C.c_void_p(S_dev.data_ptr())
    flat = {k: torch.full((int(np.prod(shapes[k])) + GUARD,), I32_FILL if k in DR.I32 else FILL,
                          dtype=torch.int32 if k in DR.I32 else torch.float64, device=dev) for k in names}
    outs = _lib.IdiagOutputs()
    for k in names:
        setattr(outs, k, C.c_void_p(flat[k].data_ptr()))
    err = C.create_string_buffer(256)
    n = C.c_size_t(0)
    _lib.check(_lib.lib().epi_idiag_workspace_bytes(C.byref(d), C.byref(n), err), err)
    ws = torch.full((n.value // 8 + GUARD,), FILL, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev)
    rc = _lib.lib().epi_idiag_run_device(C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(ws.data_ptr()), n.value,
                                         C.c_void_p(st.cuda_stream), err)
    _lib.check(rc, err)
    torch.cuda.synchronize(dev)
    res, clean = {}, {"workspace": bool((ws[n.value // 8:] == FILL).all())}
    for k in names:
        fill = I32_FILL if k in DR.I32 else FILL
        cnt = int(np.prod(shapes[k]))
        clean[k] = bool((flat[k][cnt:] == fill).all())
        clean[k + " poison"] = not bool((flat[k][:cnt] == fill).any())
        res[k] = flat[k][:cnt].cpu().numpy().reshape(shapes[k])
    return res, clean


def assert_equal(got, clean, want, what):
    assert clean["workspace"], f"{what}: wrote behind the workspace"
    for k, v in got.items():
        assert clean[k], f"{what}: {k} wrote outside its elements"
        assert clean[k + " poison"], f"{what}: {k} keeps poison"
        assert DR.same_bits(v, want[k]), f"{what}: {k} differs from the restatement"


@pytest.mark.parametrize("name", [r[0] for r in DR.CASES])
def test_cases_bit_for_bit(gpu_device, ref, name):
    e, S, kw, blk = DR.make_case(name)
    want = ref.run(e, S, **kw)
    got, clean = run_device(e, S, blk=blk, **kw)
    assert list(got) == list(DR.ALL)
    assert_equal(got, clean, want, name)


def test_the_planted_cases_reach_their_status_bits(gpu_device, ref):
    e, S, kw, blk = DR.make_case("plain")
    got, _ = run_device(e, S, blk=blk, **kw)
    st = got["status"]
    assert (st[[3, 4, 5, 6, 7, 8]] & DR.BAD_DAY).all() and st[1] == DR.EMPTY and st[9] & DR.DEGENERATE
    assert st[10] == DR.DEGENERATE | DR.FEW_LAGS and got["n"][10] == 1 and got["cusumsq_max"][10] == 0.0      # cs of the last day
    e, S, kw, blk = DR.make_case("lags_64")
    got, _ = run_device(e, S, blk=blk, **kw)
    assert (got["status"][11:] & DR.FEW_LAGS).all() and np.isnan(got["acf"][44:, 11]).all()
    e, S, kw, blk = DR.make_case("window_empty")
    got, _ = run_device(e, S, blk=blk, **kw)
    assert (got["status"] == DR.EMPTY).all() and (got["n"] == 0).all()


def test_single_outputs_and_subsets(gpu_device, ref):
    e, S, kw, _ = DR.make_case("two_blocks_ahead")
    want = ref.run(e, S, **kw)
    for k in DR.ALL:
        got, clean = run_device(e, S, blk=40, outputs=(k,), **kw)
        assert list(got) == [k]
        assert_equal(got, clean, want, f"only {k}")
    got, clean = run_device(e, S, outputs=("mean", "status", "het"), **kw)
    assert_equal(got, clean, want, "no lagged products")


def _by_hand(w, storage, shape, n_lags, burn_in, k1):
    """the runner, the likelihood with S and the new call, one after the other"""
    from epidemicmodeling_amd import batch
    dw = batch.DeviceWorkload(w)
    r = batch.EkfRunner(dw, ["S_MINUS", "P_MINUS", "innovations"], lane_block="auto", shape=shape, storage=storage)
    r.run()
    lb = 0 if r.blk == w.B else r.blk
    lik = batch.innovation_likelihood(r.out["S_MINUS"], r.out["P_MINUS"], r.out["innovations"], dw.x, dw.prm, w.model,
                                      R_series=dw.R_series, R_scalar=dw.R_scalar, x_series=dw.x_series, L=w.L, obs_type=w.obs_type,
                                      k0=burn_in, k1=k1, lane_block=lb, B=w.B, outputs=("loglik", "S"))
    res = batch.innovation_diagnostics(r.out["innovations"], lik["S"], n_lags=n_lags, k0=burn_in, k1=k1, flip="Backward" in w.model,
                                       lane_block=lb, B=w.B)
    return r, lik, res, lb


@pytest.mark.parametrize("which", ["three_state", "six_state", "six_state_backward_f32"])
def test_filter_diagnostics_end_to_end(gpu_device, ref, which):
    """pipeline.filter_diagnostics equals the three calls by hand, the restatement on the same arrays brought to the host, and
    hostapi.innovation_diagnostics"""
    import torch
    from epidemicmodeling_amd import hostapi, pipeline, synth
    from tests import loglik_ref as LR
    if which == "three_state":
        w, storage, k1 = synth.make_cfg3(8, 120), "f64", None
    elif which == "six_state":
        w, storage, k1 = synth.make_cfg4(2, 4, 90, 30), "f64", 100
    else:
        w, storage, k1 = LR.oracle_case("cfg4_bwd")[0], "f32", None
    r, res = pipeline.filter_diagnostics(w, n_lags=12, burn_in=7, k1=k1, storage=storage)
    r2, lik, hand, lb = _by_hand(w, storage, 0, 12, 7, k1)
    torch.cuda.synchronize()
    assert list(res) == list(DR.ALL) + ["lb_p", "jb_p", "nis_p", "loglik"]
    for k in DR.ALL:
        assert DR.same_bits(res[k].cpu().numpy(), hand[k].cpu().numpy()), (which, k)
    assert DR.same_bits(res["loglik"].cpu().numpy(), lik["loglik"].cpu().numpy())
    e_host, S_host = r2.out["innovations"].cpu().numpy(), lik["S"].cpu().numpy()
    e_classic = e_host[:, :w.B]                                # one row per day: chain c of day t lies at t * nblk * blk + c
    want = ref.run(e_classic.astype(np.float64), S_host, H=12, k0=7, k1=k1, flip="Backward" in w.model)
    assert (want["n"] > 12).any() and np.isfinite(want["lb_q"]).any()
    for k in DR.ALL:
        assert DR.same_bits(res[k].cpu().numpy(), want[k]), (which, k)
    host = hostapi.innovation_diagnostics(e_host, S_host, n_lags=12, k0=7, k1=k1, flip="Backward" in w.model, lane_block=lb, B=w.B)
    assert list(host) == list(DR.ALL)
    for k in DR.ALL:
        assert host[k].dtype == want[k].dtype and DR.same_bits(host[k], want[k]), (which, k)
    import scipy.stats
    ok = want["lb_lags"] > 0
    assert np.allclose(res["lb_p"].cpu().numpy()[ok], scipy.stats.chi2.sf(want["lb_q"][ok], want["lb_lags"][ok]), rtol=1e-6, atol=1e-300,
                       equal_nan=True)
    assert np.allclose(res["jb_p"].cpu().numpy(), np.exp(-0.5 * want["jb"]), rtol=1e-12, atol=0.0, equal_nan=True)


def test_tune_filter_chooses_among_the_white_candidates(gpu_device):
    """a 2 x 2 grid: with min_lb_p the choice is the largest likelihood among the candidates with lb_p >= min_lb_p, -1 where
    none qualifies; best_any keeps the choice by likelihood alone; min_lb_p = None returns the parent's keys"""
    import torch
    from epidemicmodeling_amd import pipeline, synth
    w = synth.make_cfg3(6, 120)
    kw = dict(q_scale=(0.1, 10.0), r_scale=(0.25, 4.0), burn_in=21)
    plain = pipeline.tune_filter(w, **kw)
    assert list(plain) == ["loglik", "n_valid", "status", "best", "best_loglik", "chosen", "table", "runner", "workload"]
    loose = pipeline.tune_filter(w, min_lb_p=0.0, n_lags=8, **kw)
    torch.cuda.synchronize()
    assert list(loose) == list(plain) + ["best_any", "lb_p"]
    lb_p = loose["lb_p"].cpu().numpy()
    assert lb_p.shape == (6, 4) and np.isfinite(lb_p).all()
    for k in ("loglik", "n_valid", "status"):
        assert DR.same_bits(loose[k].cpu().numpy(), plain[k].cpu().numpy()), k
    assert DR.same_bits(loose["best_any"].cpu().numpy(), plain["best"].cpu().numpy())
    assert DR.same_bits(loose["best"].cpu().numpy(), plain["best"].cpu().numpy())          # every candidate passes p >= 0
    ll = plain["loglik"].cpu().numpy()
    cut = float(np.sort(lb_p, axis=1)[:, 2].mean())            # a threshold some candidates of some regions pass
    for thr in (cut, float(np.median(lb_p)), 2.0):             # 2.0: no p-value qualifies
        out = pipeline.tune_filter(w, min_lb_p=thr, n_lags=8, **kw)
        best, bl, chosen = (out[k].cpu().numpy() for k in ("best", "best_loglik", "chosen"))
        table = out["table"].cpu().numpy()
        for r in range(6):
            cand = [g for g in range(4) if lb_p[r, g] >= thr]
            if not cand:
                assert best[r] == -1 and np.isnan(bl[r]) and np.isnan(chosen[r]).all()
            else:
                g = max(cand, key=lambda g: (ll[r, g], -g))
                assert best[r] == g and bl[r] == ll[r, g] and lb_p[r, best[r]] >= thr
                assert np.array_equal(chosen[r, :2], table[g, :2])
        if thr == 2.0:
            assert (best == -1).all()
        assert DR.same_bits(out["best_any"].cpu().numpy(), plain["best"].cpu().numpy())

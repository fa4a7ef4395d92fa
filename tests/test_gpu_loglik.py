"""The innovation log-likelihood on the device (epi_loglik_run_device / _host, batch.innovation_likelihood,
hostapi.innovation_likelihood, pipeline.filter_likelihood / tune_filter): every output equals the restatement
tests/loglik_ref.py of DESIGN.md §4.14 bit for bit -- any NaN equal to any NaN.  Every output starts as a poison value and
carries guard elements behind it; the workspace is poisoned too.  The shapes are the smallest that reach every edge: B = 70 (a
partial last wavefront), T = 45 (one full and one partial 32-step block, more than 2 L steps), T = 150 / 200 for the adaptive
replay (five / seven blocks), B = 4."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import loglik_ref as LR

pytestmark = pytest.mark.gpu

FILL, I32_FILL, GUARD = -98765.4321, -12345, 8
I32 = ("n_valid", "status", "best")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return LR.LoglikRef(tmp_path_factory.mktemp("loglik_ref"))


@functools.lru_cache(maxsize=None)
def _planted_case(name):
    """missing days (steps 7, 31, 32 of every third series, one series dark: the oracle is run again) and two bad days"""
    w = LR.with_missing_days(LR.oracle_case(name)[0])
    return w, LR.with_bad_days(LR.case_of(w, H.oracle_batch(w)))


def _run_device(case, k0=0, k1=None, storage="f64", G=0, blk=0, outputs=None, device="cuda:0"):
    """epi_loglik_run_device on poison-filled outputs with GUARD elements behind each and a poisoned workspace.  The case's
    classic arrays are uploaded chain-blocked with blk (padding lanes = NaN: never read).  Returns (dict of NumPy arrays, dict
    name -> True if the guards still hold the poison)."""
    import torch
    from epidemicmodeling_amd import _lib
    dev = torch.device(device)
    B, T = case["B"], case["T"]
    ndt = np.float32 if storage == "f32" else np.float64
    up = lambda a, dt=np.float64: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)
    with np.errstate(over="ignore"):
        big = [case[k].astype(ndt) for k in ("S_MINUS", "P_MINUS", "innovations")]
    if blk:
        big = [LR.to_blocked(a, blk, np.nan) for a in big]
    tens = [up(a, ndt) for a in big] + [up(case["x"]), up(case["R_series"]), up(case["R_scalar"]), up(case["x_series"], np.int32),
                                        up(case["prm"])]
    names = _lib.loglik_out_names(outputs, G)
    shapes = _lib.loglik_shapes(B, T, G)
    d = _lib.make_loglik_desc(case["model"], B, T, case["L"], case["obs_type"], int(case["R_series"] is not None), case["x"].shape[1],
                              blk, int(storage == "f32"), k0, k1, G)
    ins = _lib.LoglikInputs()
    for k, v in zip(_lib.LOGLIK_IN_NAMES, tens):
        setattr(ins, k, None if v is None else C.c_void_p(v.data_ptr()))
    flat = {k: torch.full((int(np.prod(shapes[k])) + GUARD,), I32_FILL if k in I32 else FILL,
                          dtype=torch.int32 if k in I32 else torch.float64, device=dev) for k in names}
    outs = _lib.LoglikOutputs()
    for k in names:
        setattr(outs, k, C.c_void_p(flat[k].data_ptr()))
    err = C.create_string_buffer(256)
    n = C.c_size_t(0)
    _lib.check(_lib.lib().epi_loglik_workspace_bytes(C.byref(d), C.byref(n), err), err)
    ws = torch.full((n.value // 8 + GUARD,), FILL, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev)
    rc = _lib.lib().epi_loglik_run_device(C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(ws.data_ptr()), n.value,
                                          C.c_void_p(st.cuda_stream), err)
    _lib.check(rc, err)
    torch.cuda.synchronize(dev)
    res, clean = {}, {"workspace": bool((ws[n.value // 8:] == FILL).all())}
    for k in names:
        h = flat[k].cpu().numpy()
        cnt = int(np.prod(shapes[k]))
        clean[k] = bool((h[cnt:] == (I32_FILL if k in I32 else FILL)).all())
        res[k] = h[:cnt].reshape(shapes[k])
    return res, clean


def _assert_equal(got, clean, want, what):
    assert clean["workspace"], f"{what}: wrote behind the workspace"
    for k, v in got.items():
        assert clean[k], f"{what}: {k} wrote outside its elements"
        assert LR.same_bits(v, want[k]), f"{what}: {k} differs from the restatement"
        assert not (v == (I32_FILL if k in I32 else FILL)).any(), f"{what}: {k} keeps poison"


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("name", LR.WORKLOADS)
def test_seven_workloads_bit_for_bit(gpu_device, ref, name, storage):
    """all nine outputs (G = a divisor of B), every window, classic layout and chain blocks that do not divide B"""
    w, case = LR.oracle_case(name)
    G = {70: 14, 24: 6, 4: 2, 6: 3, 12: 4}[w.B]
    for k0, k1 in LR.WINDOWS:
        if (k1 or w.T) > w.T:
            continue
        want = ref.run(case, k0=k0, k1=k1, storage=storage, G=G)
        for blk in ((0, 40) if w.B > 40 else (0, 3)) if (k0, k1) == (0, None) else (0,):
            got, clean = _run_device(case, k0, k1, storage, G, blk, outputs=LR.ALL)
            assert list(got) == list(LR.ALL)
            _assert_equal(got, clean, want, f"{name} {storage} window=({k0}, {k1}) blk={blk}")


@pytest.mark.parametrize("name", ["cfg3", "cfg4", "row3", "cfg3_bwd"])
def test_planted_days(gpu_device, ref, name):
    w, case = _planted_case(name)
    for storage in ("f64", "f32"):
        want = ref.run(case, storage=storage)
        assert (want["status"] & 1).sum() >= 1 and (want["n_valid"] == 0).any() and np.isnan(want["nis_mean"]).any()
        got, clean = _run_device(case, storage=storage, blk=40 if w.B > 40 else 0, outputs=LR.ALL[:7])
        _assert_equal(got, clean, want, f"{name} planted {storage}")


@pytest.mark.parametrize("name", ["cfg3", "row3"])
def test_single_outputs(gpu_device, ref, name):
    """each output alone (r_mode 1 and the adaptive replay), and the selection without the per-chain outputs"""
    w, case = LR.oracle_case(name)
    G = 14 if name == "cfg3" else 6
    want = ref.run(case, G=G)
    for k in LR.ALL[:7]:
        if k in ("n_valid", "status"):
            continue                                          # not enough on their own (validate refuses them: CPU suite)
        got, clean = _run_device(case, outputs=(k,))
        assert list(got) == [k]
        _assert_equal(got, clean, want, f"{name} only {k}")
    got, clean = _run_device(case, G=G, outputs=("R_used", "best", "best_loglik"))
    _assert_equal(got, clean, want, f"{name} selection without loglik")


def test_selection_tie_and_no_candidate(gpu_device, ref):
    """R = 5 regions x G = 14 candidates; candidate 9 is candidate 3 again (equal bits: the lower index wins), region 1 has no
    usable candidate (-1, NaN)"""
    w, _ = LR.oracle_case("cfg3")
    src = np.arange(70)
    src[np.arange(5) * 14 + 9] = np.arange(5) * 14 + 3
    w2 = w.select(src)
    case = LR.case_of(w2, H.oracle_batch(w2))
    case["P_MINUS"], case["innovations"] = case["P_MINUS"].copy(), case["innovations"].copy()
    case["P_MINUS"][10, 0, 14:28] = np.nan
    for g in range(14):
        if g not in (3, 9):
            case["innovations"][:, g] = 1.0
    want = ref.run(case, G=14)
    assert want["best"][0] == 3 and want["best"][1] == -1 and np.isnan(want["best_loglik"][1]) and want["loglik"][3] == want["loglik"][9]
    got, clean = _run_device(case, G=14)
    _assert_equal(got, clean, want, "tie")


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("which, shape", [(3, 0), (6, "lane"), (6, "hex")])
def test_from_a_runners_arrays_as_they_lie(gpu_device, ref, which, shape, storage):
    """EkfRunner(..., lane_block="auto") leaves S_MINUS, P_MINUS, innovations chain-blocked; the likelihood reads them in place.
    The restatement is fed with the ORACLE's outputs (rounded once for f32)."""
    import torch
    from epidemicmodeling_amd import batch
    name = "cfg3" if which == 3 else "cfg4"
    w, case = LR.oracle_case(name)
    dw = batch.DeviceWorkload(w)
    r = batch.EkfRunner(dw, ["S_MINUS", "P_MINUS", "innovations"], lane_block="auto", shape=shape, storage=storage)
    r.run()
    got = batch.innovation_likelihood(r.out["S_MINUS"], r.out["P_MINUS"], r.out["innovations"], dw.x, dw.prm, w.model,
                                      R_series=dw.R_series, x_series=dw.x_series, L=w.L, obs_type=w.obs_type,
                                      lane_block=0 if r.blk == w.B else r.blk, B=w.B, k0=5, outputs=LR.ALL[:7])
    torch.cuda.synchronize()
    want = ref.run(case, k0=5, storage=storage)
    assert list(got) == list(LR.ALL[:7])
    for k, v in got.items():
        assert LR.same_bits(v.cpu().numpy(), want[k]), (which, shape, storage, r.blk, k)


def test_pipeline_filter_likelihood_and_tune_filter(gpu_device, ref):
    """pipeline.filter_likelihood on the adaptive 6-state batch, and pipeline.tune_filter with R = 5 regions x G = 14
    candidates of which candidate 9 repeats candidate 3 (q_scale lists 1.0 twice ... the planted tie), against the
    restatement on the oracle's run of the grid workload"""
    import torch
    from epidemicmodeling_amd import pipeline, synth
    w, case = LR.oracle_case("row3")
    r, res = pipeline.filter_likelihood(w, k0=3, k1=140)
    torch.cuda.synchronize()
    want = ref.run(case, k0=3, k1=140)
    assert list(res) == list(LR.PER_CHAIN)
    for k, v in res.items():
        assert LR.same_bits(v.cpu().numpy(), want[k]), k
    w5 = synth.make_cfg3(5, 45)
    kw = dict(q_scale=(0.5, 1.0, 2.0, 4.0, 1.0, 8.0, 16.0), r_scale=(1.0, 2.0))      # candidates 2, 3 and 8, 9 are the same settings
    out = pipeline.tune_filter(w5, burn_in=5, **kw)
    torch.cuda.synchronize()
    gw, table = pipeline.likelihood_grid(w5, **kw)
    assert table.shape == (14, 4) and (table[8:10, :2] == table[2:4, :2]).all() and np.isnan(table[:, 2:]).all()
    want = ref.run(LR.case_of(gw, H.oracle_batch(gw)), k0=5, G=14)
    assert LR.same_bits(out["loglik"].cpu().numpy(), want["loglik"].reshape(5, 14))
    assert LR.same_bits(out["best"].cpu().numpy(), want["best"]) and LR.same_bits(out["best_loglik"].cpu().numpy(), want["best_loglik"])
    ll = want["loglik"].reshape(5, 14)
    assert (ll[:, 8:10] == ll[:, 2:4]).all() and not (want["best"] == 8).any() and not (want["best"] == 9).any()
    assert np.array_equal(want["best"], np.argmax(ll, axis=1))
    chosen = out["chosen"].cpu().numpy()
    assert np.array_equal(chosen[:, :2], table[want["best"], :2]) and np.isnan(chosen[:, 2:]).all()


@pytest.mark.parametrize("name, storage", [("cfg3", "f64"), ("cfg4", "f32"), ("row4", "f64")])
def test_hostapi_equals_batch(gpu_device, ref, name, storage):
    """the host entry against the device entry: same keys, order, dtypes and bits"""
    import torch
    from epidemicmodeling_amd import batch, hostapi
    w, case = LR.oracle_case(name)
    dt = np.float32 if storage == "f32" else np.float64
    with np.errstate(over="ignore"):
        big = [np.ascontiguousarray(case[k].astype(dt)) for k in ("S_MINUS", "P_MINUS", "innovations")]
    G = 14 if w.B == 70 else 2
    kw = dict(R_series=case["R_series"], R_scalar=case["R_scalar"], x_series=case["x_series"], L=case["L"], obs_type=case["obs_type"],
              k0=2, k1=40, G=G, outputs=LR.ALL)
    host = hostapi.innovation_likelihood(*big, case["x"], case["prm"], case["model"], **kw)
    dev = batch.innovation_likelihood(*(torch.as_tensor(a).cuda() for a in big), case["x"], case["prm"], case["model"], **kw)
    torch.cuda.synchronize()
    want = ref.run(case, k0=2, k1=40, storage=storage, G=G)
    assert list(host) == list(dev) == list(LR.ALL)
    for k in host:
        d = dev[k].cpu().numpy()
        assert host[k].dtype == d.dtype and LR.same_bits(host[k], d) and LR.same_bits(host[k], want[k]), (name, k)
    dflt = hostapi.innovation_likelihood(*big, case["x"], case["prm"], case["model"], **{**kw, "outputs": None})
    assert list(dflt) == list(LR.PER_CHAIN + LR.SELECT)

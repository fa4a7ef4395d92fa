"""The support-vector regression on the device (epi_svr_run_device / _host, batch.svr, hostapi.svr and
pipeline.growth_forecast(solver="svr" | "svr_gaussian"), growth_forecast_mean): every output and status bit-identical to the C
restatement tests/svr_ref.c, any NaN equal to any NaN.  Outputs are pre-filled with NaN poison (the integer ones with an
integer one), so an element the kernel did not write shows as a NaN the restatement does not have; GUARD poisoned elements lie
behind every output."""
import ctypes as C

import numpy as np
import pytest

from tests import rate_map_ref as RM
from tests import svr_ref as SV

pytestmark = pytest.mark.gpu

I32_POISON, GUARD = -12345, 64
# every NaN the restatement produces is the default quiet NaN; the poison carries a payload, so the two can be told apart
POISON_BITS = np.int64(0x7FF8DEADBEEF0001)


@pytest.fixture(scope="session")
def ref(tmp_path_factory):
    return SV.SvrRef(tmp_path_factory.mktemp("svr_ref_gpu"))


_WANT = {}


def _want(ref, i, kernel, max_iter=SV.MAX_ITER):
    """the C restatement's outputs, computed once per case and shared (read-only)"""
    if (i, kernel, max_iter) not in _WANT:
        p = SV.problem(i)
        w = ref.run(p["X"], p["y"], **SV.run_kw(p, kernel, max_iter=max_iter))
        for v in w.values():
            v.setflags(write=False)
        _WANT[(i, kernel, max_iter)] = w
    return _WANT[(i, kernel, max_iter)]


def _run_device(p, kernel, names, max_iter=SV.MAX_ITER, device="cuda:0", calls=1):
    """epi_svr_run_device `calls` times back to back on one stream, no synchronisation in between, each into its own
    poison-filled outputs with GUARD poisoned elements behind each; the guards are checked here"""
    import torch
    from epidemicmodeling_amd import _lib
    dev = torch.device(device)
    D, F, R = p["X"].shape
    nr = np.ascontiguousarray(p["n_rows"], dtype=np.int32)
    d, shapes = _lib.make_svr_desc(D, F, R, len(nr), kernel, SV.TOL, max_iter), _lib.svr_shapes(D, F, R, len(nr))
    t = {k: torch.as_tensor(np.array(p[k], dtype=np.float64), device=dev) for k in ("X", "y", "box", "epsilon", "kernel_scale")}   # copies
    ins = _lib.SvrInputs()
    for k, v in t.items():
        setattr(ins, k, C.c_void_p(v.data_ptr()))
    ins.n_rows = nr.ctypes.data
    st = torch.cuda.current_stream(dev)
    bufs = []
    for _ in range(calls):
        buf = {}
        for k in names:
            m = int(np.prod(shapes[k]))
            if k in _lib.SVR_OUT_I32:
                buf[k] = torch.full((m + GUARD,), I32_POISON, dtype=torch.int32, device=dev)
            else:
                buf[k] = torch.full((m + GUARD,), int(POISON_BITS), dtype=torch.int64, device=dev)
        outs = _lib.SvrOutputs()
        for k in _lib.SVR_OUT_NAMES:
            setattr(outs, k, C.c_void_p(buf[k].data_ptr()) if k in buf else None)
        err = C.create_string_buffer(256)
        rc = _lib.lib().epi_svr_run_device(C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(st.cuda_stream), err)
        _lib.check(rc, err)
        bufs.append(buf)
    torch.cuda.synchronize(dev)
    res = []
    for buf in bufs:
        o = {}
        for k, v in buf.items():
            h = v.cpu().numpy()
            m = h.size - GUARD
            assert (h[m:] == (I32_POISON if k in _lib.SVR_OUT_I32 else POISON_BITS)).all(), f"{k}: written behind its end"
            assert not (h[:m] == (I32_POISON if k in _lib.SVR_OUT_I32 else POISON_BITS)).any(), f"{k}: an element was not written"
            o[k] = h[:m].reshape(shapes[k]) if k in _lib.SVR_OUT_I32 else h[:m].view(np.float64).reshape(shapes[k])
        res.append(o)
    return res if calls > 1 else res[0]


def _same(got, want, names=None):
    names = list(want) if names is None else list(names)
    assert set(got) == set(names), (set(got), names)
    for k in names:
        assert SV.same_bits(np.asarray(got[k]), np.asarray(want[k])), k


PAIRS = [(i, k) for i, (_, ks) in enumerate(SV.CASES) for k in ks]
IDS = ["D%d-F%d-R%d-%s" % (SV.CASES[i][0][0], SV.CASES[i][0][1], SV.CASES[i][0][3], k) for i, k in PAIRS]


@pytest.mark.parametrize("i, kernel", PAIRS, ids=IDS)
def test_bit_identical_to_restatement(gpu_device, ref, i, kernel):
    """every shape of the table, with its planted regions (tests/svr_ref.plant): BAD_INPUT, the wide tube whose variables all
    stay on a bound, the duplicated rows, the constant target, the per-region box / epsilon / kernel_scale arrays"""
    want = _want(ref, i, kernel)
    _same(_run_device(SV.problem(i), kernel, SV.out_names(kernel), device=gpu_device), want)
    assert not (want["status"] & SV.NOT_CONVERGED).any()


@pytest.mark.parametrize("kernel", SV.KERNELS)
def test_max_iter_three_is_not_converged(gpu_device, ref, kernel):
    want = _want(ref, 1, kernel, 3)
    assert (want["status"] & SV.NOT_CONVERGED).any() and (want["n_iter"].max() == 3)
    _same(_run_device(SV.problem(1), kernel, SV.out_names(kernel), max_iter=3, device=gpu_device), want)


def test_bad_items_leave_their_neighbours_untouched(gpu_device, ref):
    p = SV.problem(1)
    got = _run_device(p, "linear", SV.out_names("linear"), device=gpu_device)
    assert (got["status"][:, [1, 2, 7]] == SV.BAD_INPUT).all() and np.isnan(got["fitted"][:, :, [1, 2, 7]]).all()
    X, y, box, sc = (np.array(p[k]) for k in ("X", "y", "box", "kernel_scale"))
    X[0, 0, 1], X[-1, 0, 6], box[2], sc[7] = 0.0, 0.0, 1.0, 1.0
    clean = ref.run(X, y, **SV.run_kw(p, "linear", box=box, kernel_scale=sc))
    keep = [r for r in range(X.shape[2]) if r not in (1, 2, 6, 7)]
    for k in clean:
        assert SV.same_bits(got[k][..., keep], clean[k][..., keep]), k


def test_each_output_alone(gpu_device, ref):
    for kernel in SV.KERNELS:
        want = _want(ref, 1, kernel)
        for k in SV.out_names(kernel):
            _same(_run_device(SV.problem(1), kernel, [k], device=gpu_device), want, [k])


def test_two_calls_back_to_back_on_one_stream(gpu_device, ref):
    a, b = _run_device(SV.problem(2), "gaussian", SV.out_names("gaussian"), device=gpu_device, calls=2)
    _same(a, _want(ref, 2, "gaussian"))
    _same(b, _want(ref, 2, "gaussian"))


@pytest.mark.parametrize("i, kernel", [(1, "linear"), (2, "gaussian"), (4, "linear")])
def test_device_batch_and_host_entries_are_equal(gpu_device, ref, i, kernel):
    from epidemicmodeling_amd import batch, hostapi
    p = SV.problem(i)
    want = _want(ref, i, kernel)
    kw = SV.run_kw(p, kernel)
    _same({k: v.cpu().numpy() for k, v in batch.svr(p["X"], p["y"], device=gpu_device, **kw).items()}, want)
    _same(hostapi.svr(p["X"], p["y"], **kw), want)
    _same(hostapi.svr(p["X"], p["y"], outputs=("fitted", "n_iter"), **kw), want, ("fitted", "n_iter"))
    if i == 4:                                               # scalars are broadcast; n_rows defaults to all D rows; the defaults
        from epidemicmodeling_amd import _lib
        _same(hostapi.svr(p["X"], p["y"], box=0.5, epsilon=0.01, kernel_scale=1.0, outputs=("beta",)),
              ref.run(p["X"], p["y"], None, "linear", 0.5, 0.01, 1.0, outputs=("beta",)))
        dflt = _lib.svr_defaults(p["y"], "linear")
        _same(hostapi.svr(p["X"], p["y"], outputs=("fitted",)), ref.run(p["X"], p["y"], None, "linear", outputs=("fitted",), **{
            "box": dflt["box"], "epsilon": dflt["epsilon"], "kernel_scale": dflt["kernel_scale"], "tol": 1e-3, "max_iter": 100000}))


def test_growth_forecast_svr_equals_its_stages_and_the_mean(gpu_device, ref, tmp_path_factory):
    from epidemicmodeling_amd import _lib, batch, pipeline, synth
    rm_ref = RM.RatemapRef(tmp_path_factory.mktemp("ratemap_ref_svr"))
    rng = np.random.default_rng(12)
    T, S, n = 40, 3, 4
    daily = rng.uniform(10, 200, (T, S)) * np.exp(0.02 * np.arange(T))[:, None]
    cases = np.cumsum(daily, axis=0)
    N = rng.uniform(1e6, 1e7, S)
    ip = np.repeat(rng.integers(0, 4, size=(T // 5, n, S)), 5, axis=0).astype(np.float64)
    ip[22:24, 1, 2] = np.nan                                                 # N/A days: preprocess fills them
    nts = (30, 36)
    kw = dict(n_train=list(nts), lags=(3, 5, 7), target="llr_Lambda", device=gpu_device)
    pre = batch.preprocess(cases, N, ip=ip, W=7, min_cases=synth.MIN_CASES, first_num_days=7, device=gpu_device)
    ns, ipf = pre["new_smoothed"].cpu().numpy(), pre["ip_filled"].cpu().numpy()
    y = batch.rt_window(ns, 7, 1.0, 1, 3, ("LogLinReg", "GenRatios", "NonlinLS"), device=gpu_device)["llr_Lambda"].cpu().numpy()
    p = dict(ip=ipf, y=y, new_smoothed=ns, extra=None, lambda_in=None, n_train=nts, lags=(3, 5, 7), fit=1, effect_lag=3,
             ridge=1e-6, thr=0.1, red=0.01)
    rm_want = rm_ref.run(p)
    results = [pipeline.growth_forecast(cases, N, ip, **kw)]
    for solver, kernel, hyper in (("svr", "linear", None), ("svr_gaussian", "gaussian", dict(box=0.5, epsilon=0.01, kernel_scale=2.0))):
        out = pipeline.growth_forecast(cases, N, ip, solver=solver, normalise=True, **(hyper or {}), **kw)
        results.append(out)
        Xr = np.stack([RM.features(ipf[:, :, s], (3, 5, 7), None) for s in range(S)], axis=2) / rm_want["x_mx"][None]
        h = hyper or _lib.svr_defaults(rm_want["y_filled"][:max(nts)], kernel)     # None: fitrsvm's defaults of the training target
        sv = ref.run(Xr, rm_want["y_filled"], nts, kernel, h["box"], h["epsilon"], h["kernel_scale"], 1e-3, 100000)
        for a, b in (("beta", "beta"), ("bias", "bias"), ("n_iter", "n_iter"), ("gap", "gap"), ("n_sv", "n_sv"), ("svr_status", "status")):
            assert SV.same_bits(out[a], sv[b]), a
        assert (sv["status"] == 0).all() and (sv["n_iter"] > 0).all()
        assert ("map" in out) == (kernel == "linear") and (kernel != "linear" or SV.same_bits(out["map"], sv["w"]))
        lam = np.stack([np.concatenate([rm_want["y_filled"][:nt], sv["fitted"][k, nt:]]) for k, nt in enumerate(nts)])
        want = rm_ref.run(dict(p, fit=0, lambda_in=lam), ("lambda_hat", "new_cases_est", "status"))
        for k in ("lambda_hat", "new_cases_est", "status"):
            assert SV.same_bits(out[k], want[k]), k
        for k in ("x_mx", "y_filled", "tracker"):
            assert SV.same_bits(out[k], rm_want[k]), k
        for k, nt in enumerate(nts):
            e = want["new_cases_est"][k, nt:] - ns[nt:]
            assert np.array_equal(out["err"][k, nt:], e, equal_nan=True) and np.isnan(out["err"][k, :nt]).all()
    # the script's mean([...], 1): the three rows added in the order given, divided by 3, through the same clip and rebuild
    mean = pipeline.growth_forecast_mean(results, device=gpu_device)
    lam = ((results[0]["lambda_hat"] + results[1]["lambda_hat"]) + results[2]["lambda_hat"]) / 3.0
    assert SV.same_bits(mean["lambda_mean"], lam)
    want = rm_ref.run(dict(p, fit=0, lambda_in=lam), ("lambda_hat", "new_cases_est", "status"))
    for k in ("lambda_hat", "new_cases_est", "status"):
        assert SV.same_bits(mean[k], want[k]), k
    assert np.allclose(mean["mae"], np.nanmean(np.abs(mean["err"]), axis=1), rtol=1e-13, equal_nan=True)

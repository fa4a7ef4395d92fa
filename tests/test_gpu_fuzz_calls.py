"""Property-based parity of the batched calls added since the LASSO: for every call the examples of its generator in
tests/fuzz_calls.py -- sizes, options, layouts, output subsets, launch cuts and data drawn together from one seed -- go through
the call's own device helper (sentinel-filled outputs with guard elements) and must equal the restatement bit for bit, every NaN
one value; an output not asked for stays untouched; about one example in four also goes through the hostapi entry, and the
one-row ensembles through the batch entry as a 2-D src, with the same bits.  An example of ar_forecast or smoother_draws may be
followed by its seeded twin (FZ.seeded_twin): the call under test gets a noise seed in place of z, the restatement the z of that
seed by tests/noise_ref.c.

The default run takes the seeds 0 .. N - 1 of the call (tests/test_fuzz_calls.py asserts without a device what they cover).
EPI_FUZZ_EXAMPLES=n runs n seeds from EPI_FUZZ_SEED on (default: a fresh start, printed), a longer hunt."""
import os
import time

import numpy as np
import pytest

from tests import fuzz_calls as FZ

pytestmark = pytest.mark.gpu

_N = int(os.environ.get("EPI_FUZZ_EXAMPLES", "0"))
_START = int(os.environ.get("EPI_FUZZ_SEED", str(time.time_ns() % 10 ** 9))) if _N else 0


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    return FZ.Refs(tmp_path_factory)


def _seeds(call):
    if _N:
        print(f"{call}: EPI_FUZZ_SEED={_START} EPI_FUZZ_EXAMPLES={_N}")
        return range(_START, _START + _N)
    return range(FZ.CALLS[call].n)


def _untouched(got, names, fill, i32_fill):
    """the outputs the helper filled and never handed to the library still hold the sentinel"""
    for k, a in got.items():
        if k not in names:
            assert (np.asarray(a) == (i32_fill if np.asarray(a).dtype.kind == "i" else fill)).all(), f"{k}: written without being asked for"


def _equal(got, want, names, what, flat=False):
    for k in names:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if flat and g.shape != w.shape:                          # a 2-D src: the result may come without its row axis of length 1
            assert g.size == w.size and [n for n in g.shape if n != 1] == [n for n in w.shape if n != 1], (what, k, g.shape, w.shape)
            g = g.reshape(w.shape)
        assert FZ.same_bits(g, w), (what, k)


def _hunt(call, refs, device_run, host_run=None, flat_run=None):
    for case in (c for seed in _seeds(call) for c in FZ.cases_of(refs, call, seed)):         # an example, then its seeded twin if any
        want = FZ.reference(refs, case)
        try:
            device_run(case, want)
            if case.host and host_run is not None:
                _equal(host_run(case), want, case.names, "hostapi", flat=case.flat)
            if case.flat and flat_run is not None:
                _equal({k: v.cpu().numpy() for k, v in flat_run(case).items()}, want, case.names, "batch, 2-D src", flat=True)
        except AssertionError as e:
            raise AssertionError(f"{case.summary}: {e}") from e


def _flat_kw(case, torch, device):
    kw = dict(case.kw)
    kw["src"] = torch.as_tensor(np.ascontiguousarray(kw["src"][:, 0]), device=device)
    if "truth" in kw:
        kw["truth"] = np.ascontiguousarray(kw["truth"][:, 0])
    return kw


def _host_kw(case):
    kw = dict(case.kw)
    if case.flat:
        kw["src"] = np.ascontiguousarray(kw["src"][:, 0])
        if "truth" in kw:
            kw["truth"] = np.ascontiguousarray(kw["truth"][:, 0])
    return kw


def test_random_ensemble_summary_matches_the_restatement(gpu_device, refs):
    """That it bites (a scratch build, never committed): ens_summary.hpp, the quantile's interpolation: `xk + g * (xk1 -
    xk)` written as `xk + (g * xk1 - g * xk)` (a rounding moved); the default seeds fail at seed 2 (quantiles)."""
    import torch
    from epidemicmodeling_amd import batch, hostapi
    from tests import test_gpu_ens_summary as G

    def dev(case, want):
        got = G._run_device(names=case.names, device=gpu_device, **case.kw)
        G._same(got, want, case.names)
        _untouched(got, case.names, G.FILL, G.I32_FILL)

    outs = lambda case: tuple(n for n in case.names if n != "count")
    _hunt("ensemble_summary", refs, dev,
          lambda case: hostapi.ensemble_summary(outputs=outs(case), **_host_kw(case)),
          lambda case: batch.ensemble_summary(outputs=outs(case), **_flat_kw(case, torch, gpu_device)))


def test_random_ensemble_score_matches_the_restatement(gpu_device, refs):
    """That it bites (a scratch build, never committed): ens_score.hpp, the rank's ballot: `w[j] < y` made `w[j] <= y` (a
    member equal to the truth counted below it); the default seeds fail at seed 2."""
    import torch
    from epidemicmodeling_amd import batch, hostapi
    from tests import test_gpu_escore as G

    def dev(case, want):
        got = G._run_device(names=case.names, device=gpu_device, **case.cut, **case.kw)
        G._same(got, want, case.names)
        _untouched(got, case.names, G.FILL, G.I32_FILL)

    _hunt("ensemble_score", refs, dev,
          lambda case: hostapi.ensemble_score(outputs=case.names, **case.cut, **_host_kw(case)),
          lambda case: batch.ensemble_score(outputs=case.names, **case.cut, **_flat_kw(case, torch, gpu_device)))


def _pathfn_kw(kw):
    kw = dict(kw)
    kw["thresholds"] = kw.pop("thr")
    return kw


def test_random_path_functionals_matches_the_restatement(gpu_device, refs):
    """That it bites (a scratch build, never committed): path_functionals.hpp, the running peak: `x > mx` made `x >= mx`
    (the tie-break flipped: the last of equal days wins); the default seeds fail at seed 3 (peak_day)."""
    import torch
    from epidemicmodeling_amd import batch, hostapi
    from tests import test_gpu_pathfn as G

    def dev(case, want):
        got = G._run_device(names=case.names, device=gpu_device, **case.cut, **case.kw)
        G._same(got, want, case.names)
        _untouched(got, case.names, G.FILL, G.I32_FILL)

    _hunt("path_functionals", refs, dev,
          lambda case: hostapi.path_functionals(outputs=case.names, **case.cut, **_pathfn_kw(_host_kw(case))),
          lambda case: batch.path_functionals(outputs=case.names, **case.cut, **_pathfn_kw(_flat_kw(case, torch, gpu_device))))


def _ejoint_kw(kw):
    kw = dict(kw)
    kw["vs_p"] = {0: None, 1: 0.5, 2: 1}[kw.pop("vs_order")]
    return kw


def test_random_ensemble_joint_score_matches_the_restatement(gpu_device, refs):
    """That it bites (a scratch build, never committed): ens_joint.hpp, the pair distance: `acc + d * d` made `fma(d, d,
    acc)` (a rounding moved); the default seeds fail at seed 17."""
    import torch
    from epidemicmodeling_amd import batch, hostapi
    from tests import test_gpu_ejoint as G

    def dev(case, want):
        G._same(G._run_device(names=case.names, device=gpu_device, **case.cut, **case.kw), want, case.names)   # checks the untouched ones itself

    _hunt("ensemble_joint_score", refs, dev,
          lambda case: hostapi.ensemble_joint_score(outputs=case.names, **case.cut, **_ejoint_kw(_host_kw(case))),
          lambda case: batch.ensemble_joint_score(outputs=case.names, **case.cut, **_ejoint_kw(_flat_kw(case, torch, gpu_device))))


def test_random_mldivide_matches_the_restatement(gpu_device, refs):
    """That it bites (a scratch build, never committed): mldivide.hpp, the pivot choice on equal norms: `col[q] < col[best]`
    made `col[q] > col[best]` (the tie-break flipped); the default seeds fail at seed 2 (perm)."""
    from epidemicmodeling_amd import hostapi
    from tests import test_gpu_mldivide as G

    def dev(case, want):
        kw = case.kw
        G._same(G._run_device(kw["X"], kw["y"], kw["n_rows"], case.names, tol_scale=kw["tol_scale"], device=gpu_device), want, case.names)

    _hunt("mldivide", refs, dev, lambda case: hostapi.mldivide(outputs=case.names, **case.kw))


def test_random_svr_matches_the_restatement(gpu_device, refs):
    """That it bites (a scratch build, never committed): svr.hpp, sv_wave_best on equal values: `i2 < i` made `i2 > i` (the
    tie-break flipped); the default seeds fail at seed 0."""
    from epidemicmodeling_amd import hostapi
    from tests import test_gpu_svr as G

    def dev(case, want):
        kw = case.kw
        R = kw["X"].shape[2]
        p = dict(X=kw["X"], y=kw["y"], n_rows=kw["n_rows"],
                 **{k: np.ascontiguousarray(np.broadcast_to(np.asarray(kw[k], dtype=np.float64), (R,))) for k in ("box", "epsilon", "kernel_scale")})
        assert kw["tol"] == G.SV.TOL
        G._same(G._run_device(p, kw["kernel"], case.names, max_iter=kw["max_iter"], device=gpu_device), want, case.names)

    _hunt("svr", refs, dev, lambda case: hostapi.svr(outputs=case.names, **case.kw))


def test_random_rate_map_matches_the_restatement(gpu_device, refs):
    """That it bites (a scratch build, never committed): rate_map.hpp, the test days' prediction: `fma(x / mx, m, v)` made
    `v + (x / mx) * m` (a rounding moved); the default seeds fail at seed 3."""
    from epidemicmodeling_amd import hostapi
    from tests import test_gpu_rate_map as G

    def dev(case, want):
        G._same(G._run_device(case.kw["p"], case.names, device=gpu_device), want, case.names)

    def host(case):
        p = case.kw["p"]
        return hostapi.rate_map(p["ip"], p["new_smoothed"], p["n_train"], y=p["y"], extra=p["extra"], lambda_in=p["lambda_in"], lags=p["lags"],
                                ridge=p["ridge"], lambda_threshold=p["thr"], reduction_effect=p["red"], effect_lag=p["effect_lag"],
                                outputs=case.names)

    _hunt("rate_map", refs, dev, host)


def test_random_robust_affine_fit_matches_the_restatement(gpu_device, refs):
    """That it bites (a scratch build, never committed): robust_fit.hpp, the scale: `med / 0.6745` made `med * (1.0 /
    0.6745)` (a rounding moved); the default seeds fail at seed 1 (a)."""
    from epidemicmodeling_amd import hostapi
    from tests import test_gpu_robust_fit as G

    def dev(case, want):
        kw = case.kw
        setting = (kw["robust"], kw["max_iter"], kw["lower"], kw["upper"])
        G._same(G._run_device(kw["X"], kw["y"], setting, names=case.names, device=gpu_device), want, list(case.names))

    _hunt("robust_affine_fit", refs, dev, lambda case: hostapi.robust_affine_fit(outputs=case.names, **case.kw))


def test_random_npi_plan_matches_the_restatement(gpu_device, refs):
    """That it bites (a scratch build, never committed): npi_plan.hpp, the objective: `ome * acc0 + eps * acc1` made
    `fma(ome, acc0, eps * acc1)` (a rounding moved); the default seeds fail at seed 0."""
    from epidemicmodeling_amd import hostapi
    from tests import test_gpu_npi_plan as G

    def dev(case, want):
        got, clean = G._run_device(case.kw["case"], names=case.names, device=gpu_device)
        G._assert_equal(got, clean, want, "device entry")

    def host(case):
        c = case.kw["case"]
        opt = [k for k in case.names if k in FZ.PLAN_OPTIONAL]
        return hostapi.npi_plan(c["sp"], c["u_min"], c["eps"], c["H"], u_fixed=c.get("u_fixed"), u_init=c.get("u_init"),
                                J0_prefix=c.get("J0_prefix"), J1_prefix=c.get("J1_prefix"), prefix_days=c["prefix_days"],
                                max_iter=c["max_iter"], max_halvings=c["max_halvings"], tol=c["tol"], outputs=list(FZ.PLAN_CORE) + opt)

    _hunt("npi_plan", refs, dev, host)


def test_random_ar_forecast_matches_the_restatement(gpu_device, refs):
    """That it bites (a scratch build, never committed): ar_forecast.hpp, the recursion: `fma(-coef[k], ring, acc)` made
    `acc - coef[k] * ring` (a rounding moved); the default seeds fail at seed 0 (S).  The seeded twins (FZ.seeded_twin) go
    through batch.ar_forecast(seed=, noise_stream=) and, where the example says so, hostapi's."""
    from epidemicmodeling_amd import batch, hostapi
    from tests import test_gpu_ar_forecast as G

    def seeded_kw(case):
        """a twin's arguments for the call under test: the noise seed and stream in place of z"""
        return dict({k: v for k, v in case.kw.items() if k != "z"}, seed=case.noise[0], noise_stream=case.noise[1])

    def dev(case, want):
        kw = case.kw
        if case.noise is not None:                                # a seeded twin: `want` is ArRef on the noise restatement's z
            G._same({k: v.cpu().numpy() for k, v in batch.ar_forecast(device=gpu_device, **seeded_kw(case)).items()}, want)
            return
        G._same(G._run_device(kw, kw["p"], A=kw["A"], noise_var=kw["noise_var"], nv_mode=kw["nv_mode"], device=gpu_device), want)

    _hunt("ar_forecast", refs, dev, lambda case: hostapi.ar_forecast(**(case.kw if case.noise is None else seeded_kw(case))))


def test_random_smoother_draws_matches_the_restatement(gpu_device, refs):
    """That it bites (a scratch build, never committed): smoother_draws.hpp, J (x - s-): `fma(w, dv, acc)` made `acc + w *
    dv` (a rounding moved); the default seeds fail at seed 1 (X).  The seeded twins (FZ.seeded_twin) go through
    epi_sdraw_run_device_seeded, batch.smoother_draws(seed=, noise_stream=) and, where the example says so, hostapi's."""
    import torch
    from epidemicmodeling_amd import _lib, batch, hostapi
    from tests import loglik_ref as LR
    from tests import sdraw_ref as SR
    from tests import test_gpu_noise as N
    from tests import test_gpu_sdraw as G

    def dev(case, want):
        if case.noise is not None:
            # a seeded twin: `want` is the C restatement on the noise restatement's z.  The device entry with the example's layout
            # and launch cut (sentinel-filled outputs, guard words checked), then batch.smoother_draws on the same arrays
            kw = {k: v for k, v in case.kw.items() if k != "z"}
            got = N._sdraw_raw(kw.pop("case"), kw.pop("D"), noise=_lib.make_noise_desc(*case.noise), device=gpu_device, **case.cut, **kw)
            for k in got:
                assert SR.same_bits(got[k], want[k]), f"seeded device entry: {k} differs from the restatement"
            c = SR.stored(case.kw["case"], kw["storage"])
            ndt = np.float32 if kw["storage"] == "f32" else np.float64
            with np.errstate(over="ignore", invalid="ignore"):
                big = [c[k].astype(ndt) for k in SR.BIG]
            blk = case.cut["blk"] if case.cut["blk"] < c["B"] else 0      # batch takes one block of all chains as classic arrays
            if blk:
                big = [LR.to_blocked(a, blk, np.nan) for a in big]
            dev_t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=gpu_device)
            res = batch.smoother_draws(*[dev_t(a) for a in big], dev_t(c["prm"]), case.kw["D"], s_term=dev_t(kw["s_term"]), P_term=dev_t(kw["P_term"]),
                                       k0=kw["k0"], clamp=kw["clamp"], lane_block=blk, B=c["B"],
                                       out_dtype=torch.float32 if kw["out_f32"] else torch.float64, outputs=case.names, seed=case.noise[0],
                                       noise_stream=case.noise[1])
            _equal({k: v.cpu().numpy() for k, v in res.items()}, want, case.names, "batch, seeded")
            return
        got, clean = G._run_device(device=gpu_device, **case.cut, **case.kw)
        G._assert_equal(got, clean, want, "device entry")

    def host(case):
        kw = dict(case.kw)
        if case.noise is not None:
            kw.update(z=None, seed=case.noise[0], noise_stream=case.noise[1])
        c, storage, out_f32 = SR.stored(kw.pop("case"), kw["storage"]), kw.pop("storage"), kw.pop("out_f32")
        ndt = np.float32 if storage == "f32" else np.float64
        with np.errstate(over="ignore", invalid="ignore"):
            big = [c[k].astype(ndt) for k in SR.BIG]
        return hostapi.smoother_draws(*big, c["prm"], out_dtype=np.float32 if out_f32 else np.float64, outputs=case.names, **kw)

    _hunt("smoother_draws", refs, dev, host)


def test_random_innovation_likelihood_matches_the_restatement(gpu_device, refs):
    """That it bites (a scratch build, never committed): loglik.hpp, `q = e * e / S` made `q = e * (e / S)` (a rounding
    moved), in a second build: the first build's `-0.5 * (sum + n log 2 pi)` distributed over its two addends changes no bit
    (a product with 0.5 is exact) and left the test green; the default seeds fail at seed 2 (nis)."""
    from epidemicmodeling_amd import hostapi
    from tests import test_gpu_loglik as G

    def dev(case, want):
        got, clean = G._run_device(outputs=case.names, device=gpu_device, **case.cut, **case.kw)
        assert set(got) == set(case.names)
        G._assert_equal(got, clean, want, "device entry")

    def host(case):
        kw = dict(case.kw)
        c, storage = kw.pop("case"), kw.pop("storage")
        ndt = np.float32 if storage == "f32" else np.float64
        with np.errstate(over="ignore"):
            big = [c[k].astype(ndt) for k in ("S_MINUS", "P_MINUS", "innovations")]
        return hostapi.innovation_likelihood(*big, c["x"], c["prm"], c["model"], R_series=c["R_series"], R_scalar=c["R_scalar"],
                                             x_series=c["x_series"], L=c["L"], obs_type=c["obs_type"], outputs=case.names, **kw)

    _hunt("innovation_likelihood", refs, dev, host)


def test_random_two_filter_matches_the_restatement(gpu_device, refs):
    """That it bites (a scratch build, never committed): two_filter.hpp, d2's outer sum: `d2 + e[i] * acc` made `fma(e[i],
    acc, d2)` (a rounding moved); the default seeds fail at seed 0 (d2).

    Found by the first 500-seed hunt (seed 734000005): an item at the one-sided Jacobi sweep cap, where the device set bit 1 of
    status and the restatement, which then had no view of a cap, did not; every value was equal.  The oracle now reports the
    cap, the restatement carries the bit, and the example is tests/test_gpu_two_filter.py::test_an_item_at_the_sweep_cap."""
    from epidemicmodeling_amd import hostapi
    from tests import test_gpu_two_filter as G

    abi = {"s": "s_out", "P": "P_out", "d2": "d2", "rank": "rank", "status": "status"}

    def dev(case, want):
        kw = case.kw
        T, m, B = kw["sf"].shape
        got, clean = G._run_device([kw[k] for k in ("sf", "Pf", "sb", "Pb")], m, B, T, kw["form"], kw["p_solver"], storage=kw["storage"],
                                   outputs=[abi[k] for k in case.names], device=gpu_device, **case.cut)
        assert set(got) == set(case.names)
        G._assert_equal(got, clean, want, "device entry")

    def host(case):
        kw = case.kw
        ndt = np.float32 if kw["storage"] == "f32" else np.float64
        with np.errstate(over="ignore"):
            arrs = [np.asarray(kw[k]).astype(ndt) for k in ("sf", "Pf", "sb", "Pb")]
        return hostapi.two_filter(*arrs, form=kw["form"], p_solver=kw["p_solver"], outputs=case.names)

    _hunt("two_filter", refs, dev, host)

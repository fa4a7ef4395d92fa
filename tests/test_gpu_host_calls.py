"""What the shared frame of the host-pointer entry points owns (csrc/host_stage.hpp: with_ctx, run_call): the calling
thread keeps its current device, a failed context acquisition is an ordinary error that leaves nothing behind, and a context
one entry point returns to the pool serves the next one.  Every call is made at a tiny shape (the frame does not depend on
size) and compared bit for bit with the same call made before; that the calls compute the right thing is the business of
the per-call suites."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

R, D, T = 3, 16, 24
MOVED = ("sialpha_sim", "sialpha_sim_seeded", "random_npi_mc", "random_npi_mc_seeded", "seirp_sim", "si_controlled", "npi_cost", "sir_sim",
         "preprocess", "nnls_affine_fit", "rt_expfit_run")


def _same(got, want, tag):
    assert set(got) == set(want), tag
    for k in want:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=True), (tag, k)


@pytest.fixture(scope="module")
def calls(gpu_device):
    """name -> f(device): every kind of host entry point on fixed inputs, returning a dict of NumPy arrays."""
    from epidemicmodeling_amd import batch, hostapi, synth
    rng = np.random.default_rng(5)
    w4 = synth.make_cfg4(n_regions=R, n_eps=2, T_hist=16, horizon=8)            # one block of 6 chains x 24 days
    w3 = synth.make_cfg3(R, T)
    N = synth.make_regions(R)["N"].astype(np.float64)
    truth = np.ascontiguousarray(w3.x * N[None, :] + 50.0)
    cases = rng.random((T, R)) * 100.0 + 10.0
    X, y = rng.random((D, 3, R)), rng.random((D, R))
    folds = batch.lasso_folds(D, 4, R, 0)
    src = rng.standard_normal((4, 3, R * D))
    seg = 0.2 + 0.05 * rng.standard_normal((12, R))
    z = rng.standard_normal((5, R * 4))
    sf, sb = rng.standard_normal((5, 3, R)), rng.standard_normal((5, 3, R))
    G = rng.standard_normal((2, 5, 3, 3, R))
    Pf, Pb = (np.ascontiguousarray((np.einsum("tikb,tjkb->tijb", g, g) + np.eye(3)[None, :, :, None]).reshape(5, 9, R)) for g in G)
    flat = H.flat_call_cases()        # the simulators and small fits, straight on the library: the Tools/ wrappers take one chain
    moved = {k: flat[k + "/full"] for k in MOVED if not k.endswith("_seeded")}
    moved.update({k: flat[k[:-len("_seeded")] + "/seeded"] for k in MOVED if k.endswith("_seeded")})
    return {
        **{k: (lambda dev, c=c: H.flat_call(c[0], c[1], device=dev)) for k, c in moved.items()},
        "ekf_run_host": lambda dev: H.host_call(w4, device=dev),
        "lookahead": lambda dev: batch.lookahead_host(w3, truth, N, 6, 4, device=dev, chains=True),
        "rtwin": lambda dev: hostapi.rt_window(cases, 7, 1.0, 1, 3, device=dev),
        "lasso": lambda dev: hostapi.lasso_cv(X, y, K=4, folds=folds, num_lambda=10, device=dev),
        "robfit": lambda dev: hostapi.robust_affine_fit(X, y, device=dev),
        "ens": lambda dev: hostapi.ensemble_summary(src, R, D, device=dev),
        "arfc": lambda dev: hostapi.ar_forecast(seg, np.full(R, 0.1), np.full(R, 0.99), np.full(R, 0.01), 1.0, 2, 5, 4, z=z, device=dev),
        "fuse": lambda dev: hostapi.two_filter(sf, Pf, sb, Pb, device=dev),
    }


@pytest.fixture(scope="module")
def first(calls):
    """the result of every call on device 0 with device 0 current: computed once, compared against, never written"""
    import torch
    torch.cuda.set_device(0)
    return {k: f(0) for k, f in calls.items()}


def test_calling_thread_keeps_its_device(calls, first):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    torch.cuda.set_device(1)
    try:
        for k, f in calls.items():
            got = f(0)
            assert torch.cuda.current_device() == 1, k
            _same(got, first[k], k)
    finally:
        torch.cuda.set_device(0)


def test_missing_device_is_an_error_and_leaves_nothing_behind(calls, first):
    import torch
    from epidemicmodeling_amd import _lib
    bad = torch.cuda.device_count()               # below the library's limit of 64 devices, and not there
    assert bad < 64
    cur = torch.cuda.current_device()
    for k, f in calls.items():
        with pytest.raises(_lib.EpiError, match="hipSetDevice / context") as ei:
            f(bad)
        assert ei.value.status != 0 and str(ei.value), k
        assert torch.cuda.current_device() == cur, k
        _same(f(0), first[k], k)


def test_a_context_left_by_one_entry_point_serves_another(calls, first, hip_lib):
    import torch
    torch.cuda.set_device(0)
    hip_lib.epi_host_pool_release()
    order = ("ekf_run_host", "lasso", "sir_sim", "ekf_run_host", "fuse", "preprocess", "arfc", "sialpha_sim", "lookahead",
             "random_npi_mc_seeded", "ens", "rt_expfit_run", "rtwin", "nnls_affine_fit", "robfit", "seirp_sim", "sialpha_sim_seeded",
             "si_controlled", "random_npi_mc", "npi_cost", "ekf_run_host")
    for k in order:                               # the first call creates the device's one context, the others reuse it
        _same(calls[k](0), first[k], k)

"""pipeline.prescribe(planner="direct") on the synthetic tracker file of examples/prescribe_from_csv.py: the documented keys, the
call's outputs against the C reading tests/npi_plan_ref.c from the inputs the pipeline reports, the Pareto selection against
the oracle's; the default planner="sweep" returns what it returned before the planner existed (a call recorded in
tests/golden/prescribe_sweep_default.npz by tests/golden/make_golden_prescribe_sweep.py); the example's --planner switch."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as H
from tests import npi_plan_ref as PR

GOLDEN = os.path.join(H.ROOT, "tests", "golden", "prescribe_sweep_default.npz")
RECORDED = ("J0", "J1", "front", "i_opt", "prescription", "eps_grid", "J0_prefix_region", "J1_prefix_region", "sp_region")
SWEEP_KEYS = ["pre", "alpha_round1", "fit1", "alpha_round2", "fit2", "X_reg", "R_mean", "historic", "sp_region", "J0_prefix_region",
              "J1_prefix_region", "x_sweep", "R_sweep", "u_sweep", "sweep_region", "I0", "u_fixed", "eps_grid", "sp", "J0_prefix", "J1_prefix",
              "J0", "J1", "front", "i_opt", "sweep", "prescription"]
HORIZON, N_EPS = 30, 20


def synthetic_inputs(tmp):
    """(cases, deaths, population, ip) of the example's synthetic tracker file, read back through dataio as the example does"""
    from epidemicmodeling_amd import dataio
    spec = importlib.util.spec_from_file_location("prescribe_from_csv", os.path.join(H.ROOT, "examples", "prescribe_from_csv.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    data, pops, start, end = ex.synthetic_files(str(tmp))
    d = dataio.read_oxcgrt(data, start, end)
    return d["cases"], d["deaths"], dataio.read_populations(pops, d["geo_ids"]), d["ip"]


def test_unknown_planner_is_refused():
    from epidemicmodeling_amd import pipeline
    with pytest.raises(ValueError, match='planner must be "sweep" or "direct"'):
        pipeline.prescribe(np.zeros((10, 2)), np.zeros((10, 2)), np.ones(2), np.zeros((10, 12, 2)), planner="shooting")


@pytest.mark.gpu
def test_direct_planner_keys_and_values(gpu_device, tmp_path, tmp_path_factory):
    from epidemicmodeling_amd import pipeline, synth
    from oracle import oracle_lib as olib
    cases, deaths, N, ip = synthetic_inputs(tmp_path)
    out = pipeline.prescribe(cases, deaths, N, ip, horizon=HORIZON, n_eps=N_EPS, planner="direct", device=gpu_device)
    S, n = cases.shape[1], ip.shape[1]
    for k in ("sweep", "x_sweep", "R_sweep", "u_sweep", "sweep_region"):
        assert k not in out
    want_keys = [k for k in SWEEP_KEYS if k not in ("sweep", "x_sweep", "R_sweep", "u_sweep", "sweep_region")] + \
        ["plan", "plan_F", "plan_gap", "plan_iters", "plan_halvings", "plan_status"]
    assert sorted(out) == sorted(want_keys)
    assert out["prescription"].shape == (HORIZON, n, S) and out["front"].shape == (S, N_EPS) and out["i_opt"].shape == (S,)
    for k in ("J0", "J1", "plan_F", "plan_gap", "plan_iters", "plan_halvings", "plan_status"):
        assert out[k].shape == (S, N_EPS), k
    assert out["plan_iters"].dtype == np.int32 and out["plan_status"].dtype == np.int32 and tuple(out["plan"].shape) == (HORIZON, n, S * N_EPS)
    # the call, from the inputs the pipeline reports
    ref = PR.PlanRef(tmp_path_factory.mktemp("npi_plan_ref"))
    case = dict(R=S, P=N_EPS, H=HORIZON, n=n, sp=out["sp_region"], u_min=np.repeat(synth.IP_MINS[:n, None], S, axis=1), eps=out["eps_grid"],
                J0_prefix=out["J0_prefix_region"], J1_prefix=out["J1_prefix_region"], prefix_days=cases.shape[0], max_iter=64,
                max_halvings=30, tol=1e-9)
    want = ref.run(case)
    assert PR.same_bits(out["plan"].cpu().numpy(), want["plan"])
    for k, w in (("J0", "J0"), ("J1", "J1"), ("plan_F", "F"), ("plan_gap", "gap"), ("plan_iters", "iters"), ("plan_halvings", "halvings"),
                 ("plan_status", "status")):
        assert PR.same_bits(out[k], want[w].reshape(S, N_EPS)), k
    # the sweep's own selection over these points
    for r in range(S):
        front, i_opt = olib.pareto_front(out["J0"][r], out["J1"][r])
        assert np.array_equal(out["front"][r], np.asarray(front, dtype=bool)) and out["i_opt"][r] == i_opt
        assert np.array_equal(out["prescription"][:, :, r], want["plan"][:, :, r * N_EPS + out["i_opt"][r]])


@pytest.mark.gpu
def test_sweep_default_returns_what_it_did(gpu_device, tmp_path):
    from epidemicmodeling_amd import pipeline
    cases, deaths, N, ip = synthetic_inputs(tmp_path)
    out = pipeline.prescribe(cases, deaths, N, ip, horizon=HORIZON, n_eps=N_EPS, device=gpu_device)
    rec = np.load(GOLDEN)
    assert list(out) == SWEEP_KEYS == [str(k) for k in rec["keys"]]
    for k in RECORDED:
        assert PR.same_bits(np.asarray(out[k]), rec[k]), k
    same = pipeline.prescribe(cases, deaths, N, ip, horizon=HORIZON, n_eps=N_EPS, device=gpu_device, planner="sweep")
    assert list(same) == SWEEP_KEYS and all(PR.same_bits(np.asarray(same[k]), rec[k]) for k in RECORDED)


@pytest.mark.gpu
def test_example_runs_with_the_direct_planner(gpu_device):
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "examples", "prescribe_from_csv.py"), "--planner", "direct"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "planner: direct" in r.stdout and "chains met the tolerance" in r.stdout

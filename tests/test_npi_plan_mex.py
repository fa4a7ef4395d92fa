"""The MATLAB boundary of the direct optimal-NPI planner, executed: matlab/epiekf_pipeline_mex.cpp compiled against
tests/mex_shim and driven by tests/mex_shim/lasso_driver.cpp (the gateway's generic driver).  The gateway's own argument checks
and the library's limits need no device (the gateway validates before it touches one); the test that
epiekf_pipeline_mex('plan', ...) with MATLAB-shaped arrays returns what the C reading tests/npi_plan_ref.c computes, bit for
bit, runs on the GPU."""
import numpy as np
import pytest

from tests import npi_plan_ref as PR
from tests.test_lasso_mex import _gateway, lasso_driver  # noqa: F401  (the fixture builds the gateway and its driver)

E = np.zeros((0, 0))


def _args(R=3, n=12, P=4, Hh=5.0, **kw):
    d = dict(sp=np.zeros((R, 48)), um=np.zeros((R, n)), eps=np.linspace(0.1, 0.9, P).reshape(1, P), H=Hh, uf=E, ui=E, j0=E, j1=E, pd=0.0,
             mi=8.0, mh=4.0, tol=1e-9)
    d.update(kw)
    return ["plan", d["sp"], d["um"], d["eps"], d["H"], d["uf"], d["ui"], d["j0"], d["j1"], d["pd"], d["mi"], d["mh"], d["tol"]]


def test_plan_command_errors(lasso_driver):
    g = lambda a, msg: _gateway(lasso_driver, a, 1, expect_error=msg, tag="plan_e")
    g(_args()[:12], "13 inputs expected")
    g(_args(eps=E), "must be non-empty double arrays")
    g(_args(tol=E), "must be scalars")
    g(_args(sp=np.zeros((3, 47))), "sp must be 3 x 48")
    g(_args(um=np.zeros((4, 12))), "u_min must be R x n_npi")
    g(_args(uf=np.zeros((3, 12, 4))), "u_fixed must be R x n_npi x H")
    g(_args(ui=np.zeros((3, 12, 5))), "u_init must be (P*R) x n_npi x H")
    g(_args(pd=3.0), "J0_prefix, J1_prefix must have one entry per region")
    # the library's limits, with its messages
    g(_args(Hh=0.0), "H must be >= 1")
    g(_args(um=np.zeros((3, 13))), "n_npi must lie in 1 .. 12")
    g(_args(mi=256.0), "max_iter must lie in 1 .. 255")
    g(_args(mh=31.0), "max_halvings must lie in 0 .. 30")
    g(_args(tol=-1.0), "tol must be finite and >= 0")


@pytest.mark.gpu
def test_plan_command_equals_the_c_reading(gpu_device, lasso_driver, tmp_path_factory):
    ref = PR.PlanRef(tmp_path_factory.mktemp("npi_plan_ref"))
    rng = np.random.default_rng(2)
    R, P, Hh, n = 3, 5, 9, 11
    case = dict(PR.region_case((5, 150, 100), (1e-12, 1e-3, 0.1, 0.5, 1.0 - 1e-12), Hh, n=n), max_iter=12, max_halvings=6)
    uf = np.full((Hh, n, R), np.nan)
    uf[rng.random(uf.shape) < 0.3] = 1.0
    case.update(u_fixed=uf, u_init=rng.integers(0, 3, (Hh, n, R * P)).astype(np.float64), J0_prefix=rng.random(R), J1_prefix=rng.random(R) * 50,
                prefix_days=40)
    want = ref.run(case)
    ml = lambda a: np.ascontiguousarray(np.transpose(a, tuple(range(a.ndim))[::-1]))     # the ABI's [..][B] as MATLAB's B x ..
    got = _gateway(lasso_driver, ["plan", ml(case["sp"]), ml(case["u_min"]), case["eps"].reshape(1, P), float(Hh), ml(uf), ml(case["u_init"]),
                                  case["J0_prefix"].reshape(R, 1), case["J1_prefix"].reshape(R, 1), 40.0, 12.0, 6.0, 1e-9], nlhs=11, tag="plan_run")
    assert len(got) == 11
    for k, v in zip(PR.ALL, got):
        w = want[k].astype(np.float64)
        assert PR.same_bits(np.asarray(v, dtype=np.float64).ravel(order="F"), w.ravel()), k
    few = _gateway(lasso_driver, ["plan", ml(case["sp"]), ml(case["u_min"]), case["eps"].reshape(1, P), float(Hh), ml(uf), ml(case["u_init"]),
                                  case["J0_prefix"].reshape(R, 1), case["J1_prefix"].reshape(R, 1), 40.0, 12.0, 6.0, 1e-9], nlhs=2, tag="plan_two")
    assert len(few) == 2 and PR.same_bits(np.asarray(few[1]).ravel(order="F"), want["J0"])

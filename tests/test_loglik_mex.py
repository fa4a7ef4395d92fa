"""The MATLAB boundary of the innovation log-likelihood, executed: matlab/epiekf_pipeline_mex.cpp compiled against
tests/mex_shim and driven by tests/mex_shim/lasso_driver.cpp (the gateway's generic driver).  The gateway's own argument checks
and the library's limits need no device (the host entry validates before it touches one); the test that
epiekf_pipeline_mex('loglik', ...) with MATLAB-shaped arrays of one chain returns what the restatement tests/loglik_ref.py
computes, bit for bit, runs on the GPU."""
import numpy as np
import pytest

from epidemicmodeling_amd import layout as L
from tests import loglik_ref as LR
from tests.test_lasso_mex import _gateway, lasso_driver  # noqa: F401  (the fixture builds the gateway and its driver)

E = np.zeros((0, 0))


def _args(model=0.0, m=3, T=6, **kw):
    d = dict(S=np.zeros((m, T)), P=np.zeros((m, m, T)), e=np.zeros((1, T)), x=np.zeros((1, T)), R=np.ones((1, T)),
             prm=np.zeros((L.PRM_COUNT, 1)), Lw=21.0, obs=0.0, kf=E, kl=E)
    d.update(kw)
    return ["loglik", model, d["S"], d["P"], d["e"], d["x"], d["R"], d["prm"], d["Lw"], d["obs"], d["kf"], d["kl"]]


def test_loglik_command_errors(lasso_driver):
    g = lambda a, msg: _gateway(lasso_driver, a, 1, expect_error=msg, tag="loglik_e")
    g(_args()[:11], "12 inputs expected")
    g(_args(S=E), "must be non-empty double arrays")
    g(_args(model=9.0), "unknown model id")
    g(_args(model=1.0), "S_MINUS must be m x T")
    g(_args(P=np.zeros((3, 3, 7))), "P_MINUS must be m x m x T")
    g(_args(e=np.zeros((1, 5))), "innovations and x must be 1 x T")
    g(_args(R=np.ones((1, 4))), "R_v must be 1 x T or a scalar")
    g(_args(prm=np.zeros((60, 1))), "prm must hold EPI_PRM_COUNT entries")
    g(_args(kf=0.0), "k_first, k_last must be integers")
    g(_args(kf=4.0, kl=3.0), "k_first, k_last must be integers")
    g(_args(kl=7.0), "k_first, k_last must be integers")
    g(_args(kf=1.5), "k_first, k_last must be integers")
    # the library's limits, with its messages
    g(_args(obs=3.0), "unknown observation type")
    g(_args(Lw=0.0), "L must be >= 1")


@pytest.mark.gpu
@pytest.mark.parametrize("name, chain", [("cfg3", 5), ("row3", 7), ("row4", 1), ("cfg4_bwd", 6)])
def test_loglik_command_equals_restatement(gpu_device, lasso_driver, tmp_path_factory, name, chain):
    ref = LR.LoglikRef(tmp_path_factory.mktemp("loglik_ref"))
    w, case = LR.oracle_case(name)
    w1 = w.select([chain])
    one = LR.case_of(w1, {k: case[k][..., chain:chain + 1] for k in ("S_MINUS", "P_MINUS", "innovations", "K_GAIN")})
    want = ref.run(one, k0=2, k1=w.T - 3)
    m, T = w.m, w.T
    R = w1.R_series[:, 0].reshape(1, T) if w1.R_series is not None else float(w1.R_scalar[0])
    got = _gateway(lasso_driver, ["loglik", float(L.MODEL_IDS[w.model]), np.ascontiguousarray(one["S_MINUS"][:, :, 0].T),
                                  np.ascontiguousarray(one["P_MINUS"][:, :, 0].reshape(T, m, m).transpose(2, 1, 0)),
                                  one["innovations"].reshape(1, T), w1.x.reshape(1, T), R, w1.prm.reshape(-1, 1), float(w.L),
                                  float(L.OBS_IDS[w.obs_type]), 3.0, float(T - 3)], nlhs=7, tag="loglik_" + name)
    assert len(got) == 7
    for k, v in zip(LR.ALL[:7], got):
        assert LR.same_bits(v.ravel(), want[k].ravel().astype(np.float64)), (name, k)

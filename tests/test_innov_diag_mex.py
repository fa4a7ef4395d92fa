"""The MATLAB boundary of the innovation whiteness diagnostics, executed: matlab/epiekf_pipeline_mex.cpp compiled against
tests/mex_shim and driven by tests/mex_shim/lasso_driver.cpp (the gateway's generic driver).  The gateway's own argument checks
and the library's limits need no device (the host entry validates before it touches one); the test that
epiekf_pipeline_mex('idiag', ...) with MATLAB-shaped arrays of one chain returns what the restatement tests/innov_diag_ref.py
computes, bit for bit, runs on the GPU."""
import numpy as np
import pytest

from tests import innov_diag_ref as DR
from tests.test_lasso_mex import _gateway, lasso_driver  # noqa: F401  (the fixture builds the gateway and its driver)

E = np.zeros((0, 0))


def _args(T=6, **kw):
    d = dict(e=np.zeros((1, T)), S=np.ones((1, T)), H=2.0, kf=E, kl=E, flip=0.0)
    d.update(kw)
    return ["idiag", d["e"], d["S"], d["H"], d["kf"], d["kl"], d["flip"]]


def test_idiag_command_errors(lasso_driver):
    g = lambda a, msg: _gateway(lasso_driver, a, 1, expect_error=msg, tag="idiag_e")
    g(_args()[:6], "7 inputs expected")
    g(_args(e=E), "must be non-empty double arrays")
    g(_args(H=E), "must be non-empty double arrays")
    g(_args(S=np.ones((1, 5))), "S must be 1 x T or []")
    g(_args(H=1.5), "n_lags must be an integer")
    g(_args(flip=2.0), "flip must be 0 or 1")
    g(_args(kf=0.0), "k_first, k_last must be integers")
    g(_args(kf=4.0, kl=2.0), "k_first, k_last must be integers")
    g(_args(kl=7.0), "k_first, k_last must be integers")
    g(_args(kf=1.5), "k_first, k_last must be integers")
    # the library's limits, with its messages
    g(_args(H=65.0), "n_lags is limited to 64")
    g(_args(H=-1.0), "n_lags must be >= 0")


@pytest.mark.gpu
@pytest.mark.parametrize("name, chain, with_S", [("two_blocks_ahead", 0, True), ("plain", 4, True), ("flip", 11, True), ("no_S", 12, False),
                                                 ("plain", 1, True)])
def test_idiag_command_equals_restatement(gpu_device, lasso_driver, tmp_path_factory, name, chain, with_S):
    ref = DR.InnovDiagRef(tmp_path_factory.mktemp("innov_diag_ref"))
    e, S, kw, _ = DR.make_case(name)
    T = e.shape[0]
    e1, S1 = e[:, chain:chain + 1], (S[:, chain:chain + 1] if with_S else None)
    k0, k1 = 2, T - 3
    want = ref.run(e1, S1, H=kw["H"], k0=k0, k1=k1, flip=kw["flip"])
    got = _gateway(lasso_driver, ["idiag", e1.reshape(1, T).copy(), S1.reshape(1, T).copy() if with_S else E, float(kw["H"]),
                                  float(k0 + 1), float(k1), float(kw["flip"])], nlhs=2, tag="idiag_" + name)
    assert len(got) == 2
    stats = np.concatenate([np.array([want[k][0] for k in DR.F64]),
                            np.array([float(want[k][0]) + (1.0 if k in ("cusumsq_step", "max_abs_step") else 0.0) for k in DR.I32])])
    assert DR.same_bits(got[0].ravel(), stats), name
    assert DR.same_bits(got[1].ravel(), want["acf"][:, 0]), name

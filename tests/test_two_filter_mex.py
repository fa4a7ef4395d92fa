"""The MATLAB boundary of the forward-backward filter fusion, executed: matlab/epiekf_pipeline_mex.cpp compiled against
tests/mex_shim and driven by tests/mex_shim/lasso_driver.cpp (the gateway's generic driver).  The gateway's own argument
checks and the library's limits need no device (the host entry validates before it touches one); the test that
epiekf_pipeline_mex('fuse', ...) with MATLAB-shaped arrays (m x T, m x m x T) returns what the restatement
tests/two_filter_ref.py computes, bit for bit, runs on the GPU."""
import numpy as np
import pytest

from tests import two_filter_ref as TF
from tests.test_lasso_mex import _gateway, lasso_driver  # noqa: F401  (the fixture builds the gateway and its driver)

E = np.zeros((0, 0))


def _args(sf, Pf, sb, Pb, form=1.0, p_solver=0.0):
    return ["fuse", sf, Pf, sb, Pb, form, p_solver]


def test_fuse_command_errors(lasso_driver):
    m, T = 3, 4
    s, P = np.zeros((m, T)), np.zeros((m, m, T))
    g = lambda a, msg: _gateway(lasso_driver, a, 1, expect_error=msg, tag="fuse_e")
    g(_args(s, P, s, P)[:6], "7 inputs expected")
    g(_args(E, P, s, P), "must be non-empty double arrays")
    g(_args(np.zeros((4, T)), np.zeros((4, 4, T)), np.zeros((4, T)), np.zeros((4, 4, T))), "m must be 3 or 6")
    g(_args(s, P, np.zeros((m, T + 1)), P), "S_b must be")
    g(_args(s, np.zeros((m, m, T + 1)), s, P), "P_f must be m x m x T")
    g(_args(s, P, s, np.zeros((m, m + 1, T))), "P_b must be m x m x T")
    g(_args(s, np.zeros((m, m)), s, P), "P_f must be m x m x T")
    g(_args(s, P, s, P, form=E), "form and p_solver must be double scalars")
    g(_args(s, P, s, P, p_solver=np.zeros((1, 2))), "form and p_solver must be double scalars")
    g(_args(s, P, s, P, form=2.0), "form and p_solver must be 0 or 1")
    g(_args(s, P, s, P, form=0.5), "form and p_solver must be 0 or 1")
    # the library's limit, with its message
    g(_args(s, P, s, P, form=1.0, p_solver=1.0), "p_solver must be 0 with form = 1")


@pytest.mark.gpu
@pytest.mark.parametrize("m, form, p_solver", [(3, 0, 0), (6, 1, 0), (6, 0, 1)])
def test_fuse_command_equals_restatement(gpu_device, lasso_driver, m, form, p_solver):
    T = 2 * (m + 1) + 1
    sf, Pf, sb, Pb = TF.planted(m, T, 1, seed=70 + m, indefinite=True, nonfinite=True)
    want = TF.fuse(sf, Pf, sb, Pb, form, p_solver)
    assert len(set(want["rank"].ravel().tolist())) >= 4 and (want["rank"] == -1).sum() == 1
    mx_vec = lambda v: np.ascontiguousarray(v[:, :, 0].T)                        # m x T
    mx_mat = lambda A: np.ascontiguousarray(A[:, :, 0].reshape(T, m, m).transpose(2, 1, 0))   # [t, j, i] -> (i, j, t)
    got = _gateway(lasso_driver, _args(mx_vec(sf), mx_mat(Pf), mx_vec(sb), mx_mat(Pb), float(form), float(p_solver)), nlhs=4,
                   tag=f"fuse{m}{form}{p_solver}")
    assert len(got) == 4
    assert got[0].shape == (m, T) and got[1].shape == (m, m, T) and got[2].shape == (1, T) and got[3].shape == (1, T)
    assert TF.same_bits(got[0], mx_vec(want["s"])) and TF.same_bits(got[1], mx_mat(want["P"]))
    assert TF.same_bits(got[2].ravel(), want["d2"][:, 0]) and np.array_equal(got[3].ravel(), want["rank"][:, 0].astype(np.float64))

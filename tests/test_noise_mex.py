"""The MATLAB boundary of the seeded draws, executed: matlab/epiekf_pipeline_mex.cpp and matlab/epiekf_sim_mex.cpp compiled
against tests/mex_shim.  The gateways' own checks of the seed argument need no device.  On the GPU: epiekf_pipeline_mex('noise',
...) returns the restatement tests/noise_ref.c bit for bit in MATLAB's shape, and 'sdraw', 'ar_forecast', 'mc' and
epiekf_sim_mex('sialpha', ...) given a seed return, on every output word, what they return given z = that array."""
import numpy as np
import pytest

from epidemicmodeling_amd import layout as L
from tests import noise_ref as NR
from tests.test_lasso_mex import _gateway, lasso_driver  # noqa: F401  (the fixture builds the pipeline gateway and its driver)
from tests.test_mex_boundary import _call, driver  # noqa: F401  (all gateways, the simulators' among them)

E = np.zeros((0, 0))
SEED = 7.0


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return NR.NoiseRef(tmp_path_factory.mktemp("noise_ref"))


def _sdraw_args(T=6, **kw):
    d = dict(Sp=np.zeros((3, T)), Pp=np.zeros((3, 3, T)), Sm=np.zeros((3, T)), Pm=np.zeros((3, 3, T)), prm=np.zeros((L.PRM_COUNT, 1)),
             D=2.0, z=E, st=E, Pt=E, kf=E, clamp=E)
    d.update(kw)
    return ["sdraw", d["Sp"], d["Pp"], d["Sm"], d["Pm"], d["prm"], d["D"], d["z"], d["st"], d["Pt"], d["kf"], d["clamp"]]


def test_seed_argument_errors(lasso_driver, driver):
    g = lambda a, msg: _gateway(lasso_driver, a, 1, expect_error=msg, tag="noise_e")
    g(["noise", 3.0, 3.0, 5.0], "5 to 7 inputs expected")
    g(["noise", 3.0, 2.0, 5.0, SEED], "rows must be 1 or 3")
    g(["noise", 0.0, 3.0, 5.0, SEED], "nt and lanes must be >= 1")
    g(["noise", 3.0, 3.0, 2.0 ** 30, SEED], "ask for a window")
    g(["noise", 3.0, 3.0, 5.5, SEED], "must be non-negative integers")
    g(["noise", 3.0, 3.0, 5.0, E], "seed must be a double scalar or [seed, stream]")
    g(["noise", 3.0, 3.0, 5.0, np.array([[1.0, 2.0, 3.0]])], "seed must be a double scalar or [seed, stream]")
    g(["noise", 3.0, 3.0, 5.0, -1.0], "seed must be an integer in 0 .. 2^53")
    g(["noise", 3.0, 3.0, 5.0, 1.5], "seed must be an integer in 0 .. 2^53")
    g(["noise", 3.0, 3.0, 5.0, np.array([[1.0, -2.0]])], "stream must be a non-negative integer")
    # the library's limits, with its messages
    g(["noise", 3.0, 3.0, 5.0, np.array([[1.0, 2.0 ** 30]])], "stream must be below 2^30")
    g(["noise", 3.0, 3.0, 5.0, SEED, 2.0 ** 32 - 2], "t is one counter word")
    g(_sdraw_args() + [SEED, 1.0], "12 inputs expected")
    g(_sdraw_args(z=np.zeros((2, 3, 6))) + [SEED], "seed and z together")
    g(_sdraw_args() + [np.array([[1.0, 2.0 ** 30]])], "stream must be below 2^30")
    arf = ["ar_forecast", np.zeros((2, 20)), np.zeros((2, 3)), 1.0, 3.0, 5.0, 3.0, np.zeros((6, 5)), E, E, E, E, 0.0]
    g(arf + [SEED], "seed and z together")
    mc = ["mc", np.zeros((2, 48)), np.zeros((2, 3)), 4.0, 5.0, 1.0, np.zeros((8, 3, 5)), E, E, 0.0]
    g(mc + [SEED], "noise_seed and z together")
    s = lambda a, msg: _call(driver, "sim", a, 1, expect_error=msg)
    s(["sialpha", np.zeros((2, 5)), np.zeros((48, 1)), np.zeros((3, 5)), SEED], "seed and z together")
    s(["sialpha", np.zeros((2, 5)), np.zeros((48, 1)), E, 0.5], "seed must be an integer in 0 .. 2^53")
    s(["sialpha", np.zeros((2, 5)), np.zeros((48, 1)), E, SEED, 1.0], "4 inputs expected")


@pytest.mark.gpu
def test_noise_command_equals_restatement(gpu_device, lasso_driver, ref):
    for rows, seed, stream, t0, lane0 in ((3, 7, 0, 0, 0), (1, 2 ** 53, 2 ** 30 - 1, 2 ** 32 - 3, 2 ** 40 + 1)):
        args = ["noise", 3.0, float(rows), 130.0, np.array([[float(seed), float(stream)]]), float(t0), float(lane0)]
        z, = _gateway(lasso_driver, args, nlhs=1, tag="noise")
        assert z.shape[:2] == (130, rows) and z.size == 3 * rows * 130
        assert NR.same_bits(np.ascontiguousarray(np.asarray(z).reshape(130, rows, 3).transpose(2, 1, 0)), ref.fill(seed, stream, t0, 3, rows, lane0, 130))
    z, = _gateway(lasso_driver, ["noise", 2.0, 3.0, 4.0, SEED], nlhs=1, tag="noise")          # t0, lane0 absent
    assert NR.same_bits(np.ascontiguousarray(np.asarray(z).reshape(4, 3, 2).transpose(2, 1, 0)), ref.fill(7, 0, 0, 2, 3, 0, 4))


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert NR.same_bits(np.ascontiguousarray(a), np.ascontiguousarray(b))


@pytest.mark.gpu
def test_sdraw_command_with_a_seed(gpu_device, lasso_driver, ref):
    from tests import sdraw_ref as SR
    w, case = SR.oracle_case("cfg3")
    T, D, k0, chain = w.T, 70, 3, 5
    one = {k: np.ascontiguousarray(case[k][..., chain:chain + 1]) for k in SR.BIG}
    mat3 = lambda a: np.ascontiguousarray(a[:, :, 0].reshape(T, 3, 3).transpose(2, 1, 0))
    head = ["sdraw", np.ascontiguousarray(one["S_PLUS"][:, :, 0].T), mat3(one["P_PLUS"]), np.ascontiguousarray(one["S_MINUS"][:, :, 0].T),
            mat3(one["P_MINUS"]), np.ascontiguousarray(w.prm[:, chain:chain + 1]), float(D)]
    z = ref.fill(7, 4, 0, T - k0, 3, 0, D)                                         # "70 draws, seed 7" (stream 4)
    want = _gateway(lasso_driver, head + [np.ascontiguousarray(z.transpose(2, 1, 0)), E, E, float(k0 + 1), 1.0], nlhs=5, tag="sdraw_z")
    got = _gateway(lasso_driver, head + [E, E, E, float(k0 + 1), 1.0, np.array([[7.0, 4.0]])], nlhs=5, tag="sdraw_s")
    _same(got, want)
    assert float(np.std(np.asarray(got[0])[:, 2, 0])) > 0.0


@pytest.mark.gpu
def test_ar_forecast_mc_and_sialpha_commands_with_a_seed(gpu_device, lasso_driver, driver, ref):
    from tests.test_gpu_noise import _sim_inputs
    rng = np.random.default_rng(3)
    # ar_forecast: R = 2 regions x D = 35 draws, H = 5
    R, D, Ls, p, Hh = 2, 35, 20, 3, 5
    seg = 0.3 + 0.01 * np.cumsum(rng.standard_normal((R, Ls)), axis=1)
    prm = np.stack([np.full(R, 0.2), np.full(R, 0.95), np.full(R, 0.05)], axis=1)
    z = ref.fill(7, 0, 0, Hh, 1, 0, R * D)[:, 0]                                   # [H, B] -> MATLAB's B x H
    head = ["ar_forecast", seg, prm, 0.5, float(p), float(Hh), float(D)]
    want = _gateway(lasso_driver, head + [np.ascontiguousarray(z.T), E, E, E, E, 0.0], nlhs=4, tag="arf_z")
    got = _gateway(lasso_driver, head + [E, E, E, E, E, 0.0, SEED], nlhs=4, tag="arf_s")
    _same(got, want)
    assert (np.asarray(got[3]) == 0).all() and float(np.std(np.asarray(got[0])[:D, 2, Ls + 1])) > 0.0
    # mc: the same number keys the plans and the noise
    R, n_scen, K, n = 3, 30, 5, 12
    sp = _sim_inputs(R, n, rng)
    u_min = np.zeros((R, n))
    z = ref.fill(5, 0, 0, K, 3, 0, n_scen * R)
    head = ["mc", np.ascontiguousarray(sp.T), u_min, float(n_scen), float(K), 5.0]
    want = _gateway(lasso_driver, head + [np.ascontiguousarray(z.transpose(2, 1, 0)), E, E, 0.0], nlhs=3, tag="mc_z")
    got = _gateway(lasso_driver, head + [E, E, E, 0.0, 5.0], nlhs=3, tag="mc_s")
    _same(got, want)
    plain = _gateway(lasso_driver, head + [E, E, E, 0.0], nlhs=3, tag="mc_p")
    assert NR.same_bits(np.ascontiguousarray(plain[2]), np.ascontiguousarray(got[2])) and not (np.asarray(plain[0]) == np.asarray(got[0])).all()
    # the simulator, one chain: epi_sialpha_sim_host_seeded
    K = 9
    sp1 = _sim_inputs(1, n, rng)
    u = np.floor(rng.random((n, K)) * 3)
    z = ref.fill(7, 2, 0, K, 3, 0, 1)[:, :, 0]                                     # [K, 3] -> MATLAB's 3 x K
    want = _call(driver, "sim", ["sialpha", u, sp1, np.ascontiguousarray(z.T)], nlhs=3)
    got = _call(driver, "sim", ["sialpha", u, sp1, E, np.array([[7.0, 2.0]])], nlhs=3)
    _same(got, want)
    quiet = _call(driver, "sim", ["sialpha", u, sp1, E], nlhs=3)
    assert not (np.asarray(quiet[2]) == np.asarray(got[2])).all()

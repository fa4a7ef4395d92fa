"""GPU parity: HIP kernels (through the C ABI) vs the CPU oracle on identical seeded inputs.

Tolerances (written here, per BASELINE.json north_star): 1e-6 relative on filtered states and
predicted new cases is the acceptance bar; because the kernels and the oracle are both built
without FMA contraction and evaluate in the same order, we additionally require <= 1e-9 (and
report bit-exactness) on every output, including the ill-conditioned 6-state smoother, where the
pinv truncation ranks must be identical."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

NORTH_STAR_TOL = 1e-6
TIGHT_TOL = 1e-9


def _compare(w, got, ref, tight=TIGHT_TOL):
    names = [n for n in H.OUT_NAMES if n in got]
    report = {}
    for n in names:
        e = H.rel_err(got[n], ref[n])
        report[n] = (e, bool(np.array_equal(got[n], ref[n], equal_nan=True)))
    bad = {n: v for n, v in report.items() if not v[0] <= tight}
    assert not bad, f"{w.model}: outputs beyond {tight:g}: {bad}"
    # predicted new cases N*s*i*alpha from the filtered state (north-star quantity)
    nc_g = got["S_PLUS"][:, 0] * got["S_PLUS"][:, 1] * got["S_PLUS"][:, 2]
    nc_r = ref["S_PLUS"][:, 0] * ref["S_PLUS"][:, 1] * ref["S_PLUS"][:, 2]
    assert H.rel_err(nc_g, nc_r) <= NORTH_STAR_TOL
    return report


def _run(w, device, **kw):
    from epidemicmodeling_amd import batch
    return batch.run_workload(w, device=device, **kw)


def _room_for_clones(r, device):
    """Before a second copy of a runner's outputs is taken on the device: assert that it fits (a failure, not a skip)."""
    import torch
    torch.cuda.empty_cache()
    need = r.output_bytes() + (r.pinv_rank.numel() + r.status.numel()) * 4
    free, total = torch.cuda.mem_get_info(device)
    assert free >= need + (2 << 30), ("clones of the outputs (%.1f GB) do not fit beside them: %.1f GB of %.1f GB free"
                                      % (need / 1e9, free / 1e9, total / 1e9))


def _peak_memory(tag):
    import torch
    print("peak device memory [%s]: %.1f GB" % (tag, torch.cuda.max_memory_allocated() / 1e9))


def _back_to_back_and_graph_replay(r, saved, enqueue, what):
    """The conditions bench.py times under, which one cold pass behind a synchronise does not meet ("Every chain of the
    full-size runs"): every output and the workspace poisoned by stream-ordered fills, then FIVE passes (bench.py's documented
    --steps 5; a fixed count, not a loop until something differs) enqueued back to back without a synchronisation between them,
    one synchronise, and the whole batch against `saved` (clones of outputs that equalled the oracle chain by chain).  Then the
    same call captured into a HIP graph behind a warm-up pass, the outputs poisoned again, ONE replay, and the whole batch again.
    enqueue(): one pass on the current stream."""
    import torch
    H.poison_runner(r)
    for _ in range(5):
        enqueue()
    torch.cuda.synchronize()
    H.device_outputs_equal(r, saved, what=what + ", last of 5 passes back to back")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        r.run()                                         # warm-up outside the capture (helper streams get created)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        r.run(stream=s)
    H.poison_runner(r)
    g.replay(); torch.cuda.synchronize()
    H.device_outputs_equal(r, saved, what=what + ", graph replay")
    del g


SHAPES = ["lane", "quad", "wave", "hex"]     # epi_batch_desc.shape: one lane / four lanes / one wavefront / six lanes per chain (6-state generic models)


def test_cfg3_sia3_parity(gpu_device):
    from epidemicmodeling_amd import synth
    w = synth.make_cfg3(300, 400)            # BASELINE config 3 at full size (120k steps)
    got, ref = _run(w, gpu_device), H.oracle_batch(w)
    rep = _compare(w, got, ref)
    assert np.array_equal(got["pinv_rank"], ref["pinv_rank"])
    print("cfg3 bit-exact:", {k: v[1] for k, v in rep.items()})


@pytest.mark.parametrize("shape", SHAPES)
def test_cfg4_sia6_sweep_parity(gpu_device, shape):
    from epidemicmodeling_amd import synth
    w = synth.make_cfg4(n_regions=12, n_eps=50, T_hist=200, horizon=60)   # 600 chains x 260 days
    got, ref = _run(w, gpu_device, shape=shape), H.oracle_batch(w)
    rep = _compare(w, got, ref)
    assert np.array_equal(got["pinv_rank"], ref["pinv_rank"]), "pinv truncation pattern differs"
    print("cfg4 bit-exact:", {k: v[1] for k, v in rep.items()})


@pytest.mark.parametrize("shape", SHAPES)
def test_row3_adaptive_R_parity(gpu_device, shape):
    from epidemicmodeling_amd import synth
    w = synth.make_row3(n_regions=6, n_eps=20)
    got, ref = _run(w, gpu_device, shape=shape), H.oracle_batch(w)
    _compare(w, got, ref)
    assert np.array_equal(got["pinv_rank"], ref["pinv_rank"])


@pytest.mark.parametrize("codegen", [False, True])
def test_newcase6_parity(gpu_device, codegen):
    from epidemicmodeling_amd import synth
    w = synth.make_row4(n_regions=70, T=200, predict_ahead=90, codegen=codegen)
    got, ref = _run(w, gpu_device), H.oracle_batch(w)
    assert "u_opt_smooth" not in got
    _compare(w, got, ref)


def test_backward_models_parity(gpu_device):
    from epidemicmodeling_amd import synth
    w3 = synth.as_backward(synth.make_cfg3(70, 150))
    _compare(w3, _run(w3, gpu_device), H.oracle_batch(w3))
    w6 = synth.as_backward(synth.make_cfg4(8, 10, 40, 0))
    _compare(w6, _run(w6, gpu_device), H.oracle_batch(w6))


def test_totalcases_observation(gpu_device):
    from epidemicmodeling_amd import synth
    w = synth.make_cfg3(64, 120)
    w.obs_type = "TOTALCASES"
    w.x = np.cumsum(w.x, axis=0)
    _compare(w, _run(w, gpu_device), H.oracle_batch(w))


@pytest.mark.parametrize("name", H.GOLDEN_CASES)
def test_gpu_reproduces_golden_vectors(gpu_device, name):
    """Committed fixtures (tests/golden, generated by the two CPU restatements): bit-for-bit."""
    w, exp = H.load_golden(name)
    got = _run(w, gpu_device)
    for n, e in exp.items():
        if n.startswith("meta"):
            continue
        assert np.array_equal(got[n], e, equal_nan=True), f"{name}: {n}"


def test_tools_single_call_matches_oracle(gpu_device):
    """The drop-in Tools/-named functions (host pointers -> epi_ekf_run_host), B = 1, MATLAB shapes."""
    from epidemicmodeling_amd import synth, tools
    from oracle import oracle_lib as olib
    w = synth.make_cfg4(2, 3, 50, 20)
    c = 4
    args = H.chain_args(w, c)
    u, x, p = args[0], args[1], args[2]
    params = dict(dt=p.dt, a=p.a, b=p.b, u_min=p.u_min, u_max=p.u_max, alpha_min=p.alpha_min, alpha_max=p.alpha_max,
                  gamma=p.gamma, beta=p.beta, sigma=p.sigma, epsilon=p.epsilon, w=np.ones((1, 12)),
                  obs_type="NEWCASES")
    got = tools.SIAlphaModelEKFOptControlled(u, x.reshape(1, -1), params, *args[3:])
    names = ["u_opt", "u_opt_smooth", "S_MINUS", "S_PLUS", "S_SMOOTH", "P_MINUS", "P_PLUS", "P_SMOOTH", "K_GAIN",
             "innovations", "rho"]
    ref = olib.run("SIAlphaModelEKFOptControlled", u, x, params, np.ones(12), *args[3:7], args[8], *args[9:])
    assert got[0].shape == (12, 70) and got[5].shape == (6, 6, 70) and got[8].shape == (6, 1, 70)
    assert got[9].shape == (1, 70) and got[10].shape == (70, 1)
    for n, g in zip(names, got):
        assert np.array_equal(np.asarray(g).reshape(-1), np.asarray(ref[n]).reshape(-1), equal_nan=True), n
    # 10-output NewCase variant, Tools/ order
    w4 = synth.make_row4(1, 80, 30)
    a4 = H.chain_args(w4, 0)
    p4 = a4[2]
    prm4 = dict(dt=p4.dt, a=p4.a, b=p4.b, u_min=p4.u_min, u_max=p4.u_max, alpha_min=p4.alpha_min,
                alpha_max=p4.alpha_max, gamma=p4.gamma, beta=p4.beta, sigma=p4.sigma, epsilon=p4.epsilon,
                w=np.ones(12), obs_type="NEWCASES")
    out4 = tools.NewCaseEKFEstimatorWithOptimalNPI(a4[0], a4[1].reshape(1, -1), prm4, *a4[3:])
    assert len(out4) == 10
    ref4 = olib.run("NewCaseEKFEstimatorWithOptimalNPI", a4[0], a4[1], prm4, np.ones(12), *a4[3:7], a4[8], *a4[9:])
    for n, g in zip(["u_opt", "S_MINUS", "S_PLUS", "S_SMOOTH", "P_MINUS", "P_PLUS", "P_SMOOTH", "K_GAIN"], out4):
        assert np.array_equal(np.asarray(g).reshape(-1), np.asarray(ref4[n]).reshape(-1), equal_nan=True), n


def test_reduced_output_mode_uses_workspace(gpu_device):
    """out_mask = u_opt_smooth + S_SMOOTH only: forward quantities go to the workspace, results unchanged."""
    from epidemicmodeling_amd import batch, synth
    w = synth.make_cfg4(6, 20, 80, 30)
    full = batch.run_workload(w, device=gpu_device)
    red = batch.run_workload(w, outputs=["u_opt_smooth", "S_SMOOTH"], device=gpu_device)
    assert set(red) == {"u_opt_smooth", "S_SMOOTH", "pinv_rank", "status"}
    assert np.array_equal(red["S_SMOOTH"], full["S_SMOOTH"]) and np.array_equal(red["u_opt_smooth"], full["u_opt_smooth"])


def test_sialpha_sim_and_cost_parity(gpu_device):
    import ctypes as C
    from epidemicmodeling_amd import batch, synth
    from oracle import oracle_lib as olib
    rng = np.random.default_rng(3)
    B, K, n = 130, 120, 12
    u = rng.integers(0, 4, size=(K, n, B)).astype(np.float64)
    sp = np.zeros((batch.SIM_PRM_COUNT, B))
    N = 10.0 ** rng.uniform(4, 9, B)
    sp[0] = 1 - 100 / N; sp[1] = 100 / N; sp[2] = synth.ALPHA0; sp[3] = 1e-8; sp[4] = 100.0; sp[5] = 1 / 7
    sp[6] = 0.01; sp[7] = synth.MODEL_BETA; sp[8] = 10 / N; sp[9] = 30 / N; sp[10] = 1e-2; sp[11] = 1.0
    sp[batch.SIM_A:batch.SIM_A + n] = rng.random((n, B)) * 0.03
    sp[batch.SIM_U_MAX:batch.SIM_U_MAX + n] = synth.IP_MAXES[:, None]
    sp[batch.SIM_W:batch.SIM_W + n] = rng.random((n, B))
    z = rng.standard_normal((K, 3, B))
    for zz in (None, z):
        got = batch.sialpha_sim(u, sp, z=zz, with_cost=True, device=gpu_device)
        gs, gi, ga = (got[k].cpu().numpy() for k in ("s", "i", "alpha"))
        lib = olib.lib()
        dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
        for c in (0, 17, B - 1):
            uc = np.asfortranarray(u[:, :, c].T)
            zc = None if zz is None else np.ascontiguousarray(z[:, :, c])
            s, i, a = np.zeros(K), np.zeros(K), np.zeros(K)
            aa = np.ascontiguousarray(sp[batch.SIM_A:batch.SIM_A + n, c]); um = np.ascontiguousarray(sp[batch.SIM_U_MAX:batch.SIM_U_MAX + n, c])
            lib.orc_sialpha_controlled(dp(uc), C.c_int(n), *[C.c_double(sp[k, c]) for k in (0, 1, 2)], dp(um),
                                       C.c_double(sp[3, c]), C.c_double(sp[4, c]), C.c_double(sp[5, c]), dp(aa),
                                       C.c_double(sp[6, c]), C.c_double(sp[7, c]), C.c_double(sp[8, c]),
                                       C.c_double(sp[9, c]), C.c_double(sp[10, c]), C.c_int(K), C.c_double(1.0),
                                       None if zc is None else dp(zc), dp(s), dp(i), dp(a))
            assert np.array_equal(gs[:, c], s) and np.array_equal(gi[:, c], i) and np.array_equal(ga[:, c], a)
            wts = np.asfortranarray(np.repeat(sp[batch.SIM_W:batch.SIM_W + n, c][:, None], K, axis=1))
            J0, J1 = C.c_double(), C.c_double()
            nc = np.ascontiguousarray(s * i * a)
            lib.orc_npi_cost(dp(nc), dp(uc), dp(wts), C.c_int(n), C.c_int(K), C.byref(J0), C.byref(J1))
            assert got["J0"][c].item() == J0.value and got["J1"][c].item() == J1.value


def test_seirp_sim_parity_and_rk4_order(gpu_device):
    """BASELINE config 2 shape (reduced): Euler is bit-exact vs the oracle (SEIRP.m:26-32), mass is conserved,
    and the RK4 extension converges with order 4 against a fine-step reference."""
    import ctypes as C
    from epidemicmodeling_amd import batch
    from oracle import oracle_lib as olib
    rng = np.random.default_rng(8)
    B, Tdays, dt = 200, 100, 0.1
    K = int(round(Tdays / dt))
    base = np.array([0.6, 0.005, 0.05, 0.08, 0.1, 0.02, 0.001])       # testSEIRP02.m:22-29
    par = (base[:, None] * np.exp(rng.uniform(np.log(0.5), np.log(2.0), (7, B))))[None]
    init = np.zeros((5, B)); init[1] = 1e-6; init[0] = 1 - init[1]
    out = batch.seirp_sim(par, init, dt, K, device=gpu_device).cpu().numpy()
    assert np.max(np.abs(out.sum(axis=1) - 1.0)) < 1e-12
    lib = olib.lib()
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    for c in (0, 77, B - 1):
        cols = [np.full(K, par[0, j, c]) for j in range(7)]
        res = [np.zeros(K) for _ in range(5)]
        lib.orc_seirp(*[dp(v) for v in cols], *[C.c_double(init[q, c]) for q in range(5)], C.c_int(K), C.c_double(dt),
                      *[dp(v) for v in res])
        for q in range(5):
            assert np.array_equal(out[:, q, c], res[q])
    # saturated-resource variant (tanh in the fixed operation order both sides share: bit for bit)
    sat = np.stack([np.full(B, 0.1), np.full(B, 0.02), np.full(B, 0.02), np.full(B, 0.08), np.full(B, 0.01), np.full(B, 0.05)])
    outs = batch.seirp_sim(par, init, dt, K, sat=sat, device=gpu_device).cpu().numpy()
    c = 5
    cols = [np.full(K, par[0, j, c]) for j in (0, 1, 2, 3, 6)]
    res = [np.zeros(K) for _ in range(5)]
    lib.orc_seirp_saturated(*[dp(v) for v in cols], *[C.c_double(init[q, c]) for q in range(5)], C.c_int(K),
                            C.c_double(dt), *[C.c_double(sat[j, c]) for j in range(6)], *[dp(v) for v in res])
    for q in range(5):
        assert np.array_equal(outs[:, q, c], res[q])
    # RK4 convergence order: error(dt) / error(dt/2) ~ 16
    def rk4_end(step):
        Kk = int(round(20.0 / step)) + 1
        return batch.seirp_sim(par, init, step, Kk, integrator="rk4", device=gpu_device)[-1].cpu().numpy()
    ref = rk4_end(0.0125)
    e1, e2 = np.abs(rk4_end(0.4) - ref).max(), np.abs(rk4_end(0.2) - ref).max()
    assert 10.0 < e1 / e2 < 24.0, e1 / e2


def test_dense_fallback_path(gpu_device):
    """A non-diagonal Q_w / non-symmetric Ps_init must route the batch to the dense kernels (ekf_precheck),
    which mirror the oracle term for term."""
    from epidemicmodeling_amd import synth
    w = synth.make_cfg4(4, 8, 60, 20)
    w.Q[1 + 6 * 0] = 1e-12; w.Q[0 + 6 * 1] = 2e-12          # off-diagonal, not even symmetric
    w.Ps_init[2 + 6 * 1, 3] = 1e-9                           # one chain with a non-symmetric Ps_init
    _compare(w, _run(w, gpu_device), H.oracle_batch(w))
    w3 = synth.make_cfg3(40, 80)
    w3.Q[1 + 3 * 2] = 1e-13
    _compare(w3, _run(w3, gpu_device), H.oracle_batch(w3))


@pytest.mark.parametrize("shape", SHAPES)
def test_time_pipelined_forward_segments(gpu_device, shape):
    """time_pipe = 1 (and what time_pipe = 0 picks for a batch that leaves SIMDs idle): the forward kernel in five launches
    (40, 30, 20, 8, 2 % of the days), each resuming from the S_MINUS / P_MINUS the previous one stored, and on a helper
    stream the eks_pinv grid of the days each launch has finished.  Same bits as the oracle for both lane mappings and as
    the plain launch (time_pipe = -1); the time-flipped wrappers too (array positions reversed)."""
    from epidemicmodeling_amd import synth
    cases = [synth.make_cfg4(5, 9, 150, 30)]
    if shape == "lane":
        cases += [synth.make_cfg3(40, 200), synth.as_backward(synth.make_cfg3(20, 160))]
    for w in cases:
        ref = H.oracle_batch(w)
        for tp in (1, 0, -1):
            got = _run(w, gpu_device, time_pipe=tp, shape=shape)
            for n in H.OUT_NAMES:
                if n in ref:
                    assert np.array_equal(got[n], ref[n], equal_nan=True), (w.model, shape, tp, n)
            assert np.array_equal(got["pinv_rank"], ref["pinv_rank"])
    # the time-flipped 6-state wrapper: over >= 128 days its costates overflow (in the reference's arithmetic too, and
    # DESIGN.md 2 says where the packed kernels may then place non-finite values differently from the dense oracle), so
    # the pipelined call is held against the same kernels launched the plain way: same bits, NaNs included
    w = synth.as_backward(synth.make_cfg4(3, 4, 100, 30))
    got = _run(w, gpu_device, time_pipe=1, shape=shape)
    plain = _run(w, gpu_device, time_pipe=-1, shape=shape)
    assert np.isfinite(plain["S_SMOOTH"]).mean() > 0.5
    for n in list(H.OUT_NAMES) + ["pinv_rank"]:
        if n in plain:
            assert np.array_equal(got[n], plain[n], equal_nan=(got[n].dtype.kind == "f")), (w.model, shape, n)


@pytest.mark.parametrize("precheck", [True, False])
def test_path_hint_and_device_side_selection_agree(gpu_device, precheck):
    """precheck=True: host asks once, only the selected variant is enqueued; False: both are enqueued and the
    device-side flag decides.  Covers a batch that qualifies for the packed kernels and one that does not."""
    from epidemicmodeling_amd import batch, synth
    for dense in (False, True):
        w = synth.make_cfg4(4, 20, 50, 15)
        if dense:
            w.Q[4 + 6 * 3] = 1e-10
        got = batch.run_workload(w, device=gpu_device, precheck=precheck)
        _compare(w, got, H.oracle_batch(w))


def _tiny(model_maker, **over):
    w = model_maker()
    for k, v in over.items():
        setattr(w, k, v)
    return w


@pytest.mark.parametrize("T,B,L", [(1, 1, 21), (2, 3, 1), (3, 65, 2), (7, 64, 50), (40, 130, 5)])
def test_edge_sizes_all_models(gpu_device, T, B, L):
    """Ragged and minimal shapes: T = 1 (no smoother step), T = 2, B not a multiple of 64, window longer or
    shorter than the series, for every model variant."""
    from epidemicmodeling_amd import synth
    nreg = max(1, (B + 4) // 5)
    makers = [
        lambda: synth.make_cfg3(B, T),
        lambda: synth.make_cfg4(nreg, 5, max(1, T - T // 3), T // 3).select(np.arange(B)),
        lambda: synth.make_row4(B, T, T // 2),
        lambda: synth.as_backward(synth.make_cfg3(B, T)),
        lambda: synth.as_backward(synth.make_cfg4(nreg, 5, T, 0)).select(np.arange(B)),
    ]
    for mk in makers:
        w = mk()
        w.L = L
        got, ref = _run(w, gpu_device), H.oracle_batch(w)
        _compare(w, got, ref)
        if "pinv_rank" in ref and not w.model.startswith("NewCase"):
            assert np.array_equal(got["pinv_rank"], ref["pinv_rank"])


def test_fewer_than_twelve_npis(gpu_device):
    """n_npi < 12: the u arrays are n_npi x T, the parameter vectors are zero-padded."""
    from epidemicmodeling_amd import synth
    n = 5
    w = H.with_npis(synth.make_cfg4(5, 6, 40, 12), n)
    got, ref = _run(w, gpu_device), H.oracle_batch(w)
    assert got["u_opt"].shape == (52, n, 30)
    _compare(w, got, ref)


def test_missing_observations_inside_series(gpu_device):
    """NaN gaps in x (GenericEKF.m:130-135) and the adaptive-R reset after a missing sample."""
    from epidemicmodeling_amd import synth
    w = synth.make_row3(3, 4, 30, 30)
    w.x[[5, 6, 17, 40], :] = np.nan
    _compare(w, _run(w, gpu_device), H.oracle_batch(w))
    w3 = synth.make_cfg3(70, 60)
    w3.x[10:20, ::3] = np.nan
    _compare(w3, _run(w3, gpu_device), H.oracle_batch(w3))


def test_status_and_guard_on_nonfinite_covariance(gpu_device):
    """Q = Inf drives P_MINUS non-finite: the :211 guard gives J = 0, S_SMOOTH(k) = clamp(S_PLUS(k)), the rank
    word is -1 and status bit 0 is set; healthy chains in the same batch are unaffected (bit-exact)."""
    from epidemicmodeling_amd import synth
    w = synth.make_cfg3(8, 30)
    w.Q[0, 2] = np.inf
    got, ref = _run(w, gpu_device), H.oracle_batch(w)
    assert np.all(got["pinv_rank"][:, 2] == -1) and (got["status"][2] & 1) == 1
    assert np.array_equal(got["S_SMOOTH"][:-1, :, 2], got["S_PLUS"][:-1, :, 2])
    keep = [c for c in range(8) if c != 2]
    for n in ("S_PLUS", "S_SMOOTH", "P_SMOOTH", "rho"):
        assert np.array_equal(got[n][..., keep], ref[n][..., keep])
    assert not (got["status"][keep] & 1).any()


def test_scenario_scoring_tail_of_the_sweep(gpu_device):
    """after the 6-state sweep, simulate the horizon under u_opt_smooth from the end-of-history
    state and score NPICost over [historic, horizon] (TrainPredictPrescribeNPI.m:481-493) -- (J0, J1) per chain
    bit-identical to SIalpha_Controlled + NPICost of the oracle on the concatenated series."""
    import ctypes as C
    import torch
    from epidemicmodeling_amd import batch, layout as L_, synth
    from oracle import oracle_lib as olib
    w = synth.make_cfg4(6, 12, 70, 40)
    t_hist, H, B, n = 70, 40, w.B, 12
    dw = batch.DeviceWorkload(w, gpu_device)
    r = batch.EkfRunner(dw, outputs=["u_opt_smooth", "S_SMOOTH"])
    out = r.run()
    torch.cuda.synchronize()
    S = out["S_SMOOTH"].cpu().numpy(); U = out["u_opt_smooth"].cpu().numpy()
    rng = np.random.default_rng(9)
    wts = rng.random((n, B)) + 0.5
    nc_hist = S[:t_hist, 0] * S[:t_hist, 1] * S[:t_hist, 2]                    # [t_hist, B]
    J0p = np.cumsum(nc_hist, axis=0)[-1]                                       # sequential sums
    terms = (wts[None] * U[:t_hist]).reshape(t_hist * n, B)                    # column-major order: NPI fastest
    J1p = np.cumsum(terms, axis=0)[-1]
    sp = np.zeros((batch.SIM_PRM_COUNT, B))
    sp[0], sp[1], sp[2] = S[t_hist - 1, 0], S[t_hist - 1, 1], S[t_hist - 1, 2]
    sp[3] = w.prm[L_.PRM_ALPHA_MIN]; sp[4] = w.prm[L_.PRM_ALPHA_MAX]; sp[5] = w.prm[L_.PRM_GAMMA]
    sp[6] = w.prm[L_.PRM_B]; sp[7] = w.prm[L_.PRM_BETA]; sp[11] = 1.0
    sp[batch.SIM_A:batch.SIM_A + n] = w.prm[L_.PRM_A:L_.PRM_A + n]
    sp[batch.SIM_U_MAX:batch.SIM_U_MAX + n] = w.prm[L_.PRM_U_MAX:L_.PRM_U_MAX + n]
    sp[batch.SIM_W:batch.SIM_W + n] = wts
    got = batch.score_sweep(out["u_opt_smooth"], t_hist, sp, J0p, J1p, store=True)
    gJ0, gJ1 = got["J0"].cpu().numpy(), got["J1"].cpu().numpy()
    lib = olib.lib()
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    for c in (0, 7, 31, B - 1):
        uc = np.asfortranarray(U[t_hist:, :, c].T)                              # n x H
        s, i, a = np.zeros(H), np.zeros(H), np.zeros(H)
        aa = np.ascontiguousarray(sp[batch.SIM_A:batch.SIM_A + n, c]); um = np.ascontiguousarray(sp[batch.SIM_U_MAX:batch.SIM_U_MAX + n, c])
        lib.orc_sialpha_controlled(dp(uc), C.c_int(n), C.c_double(sp[0, c]), C.c_double(sp[1, c]), C.c_double(sp[2, c]),
                                   dp(um), C.c_double(sp[3, c]), C.c_double(sp[4, c]), C.c_double(sp[5, c]), dp(aa),
                                   C.c_double(sp[6, c]), C.c_double(sp[7, c]), C.c_double(0), C.c_double(0), C.c_double(0),
                                   C.c_int(H), C.c_double(1.0), None, dp(s), dp(i), dp(a))
        assert np.array_equal(got["s"][:, c].cpu().numpy(), s) and np.array_equal(got["alpha"][:, c].cpu().numpy(), a)
        nc_all = np.ascontiguousarray(np.concatenate([nc_hist[:, c], s * i * a]))
        u_all = np.asfortranarray(U[:, :, c].T)                                 # n x T
        w_all = np.asfortranarray(np.repeat(wts[:, c][:, None], t_hist + H, axis=1))
        J0, J1 = C.c_double(), C.c_double()
        lib.orc_npi_cost(dp(nc_all), dp(u_all), dp(w_all), C.c_int(n), C.c_int(t_hist + H), C.byref(J0), C.byref(J1))
        assert gJ0[c] == J0.value and gJ1[c] == J1.value


@pytest.mark.parametrize("time_pipe", [0, 1])
def test_hip_graph_capture_and_replay(gpu_device, time_pipe):
    """The launch path contains no allocation / synchronisation (cdna_hip_programming.md G9): a full call -- also
    the fork/join over the helper stream (monitor beside the smoother; the pinv grids of the forward pass's time
    segments) -- can be captured into a HIP graph and replayed."""
    import torch
    from epidemicmodeling_amd import batch, synth
    w = synth.make_cfg3(300, 160)                    # BASELINE config 3 shape: launch-bound, 5 waves
    ref = H.oracle_batch(w)
    dw = batch.DeviceWorkload(w, gpu_device)
    r = batch.EkfRunner(dw, extras=True, time_pipe=time_pipe)
    r.run()                                          # warm-up outside capture (creates the helper streams)
    torch.cuda.synchronize()
    for t in r.out.values():
        t.zero_()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            r.run(stream=s)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    for n in ("S_PLUS", "S_SMOOTH", "P_SMOOTH", "rho", "u_opt_smooth"):
        assert np.array_equal(r.out[n].cpu().numpy(), ref[n], equal_nan=True), n


def test_c_abi_from_plain_c_program(gpu_device, tmp_path):
    """The boundary is a C ABI: examples/c_abi_demo.c (gcc, no Python/torch in the process, system HIP runtime)
    calls epi_ekf_run_host with MATLAB-layout B = 1 arrays; outputs equal the oracle's bit for bit."""
    import os
    import struct
    import subprocess
    from epidemicmodeling_amd import layout as L_, synth
    from oracle import oracle_lib as olib
    root = H.ROOT
    exe = str(tmp_path / "c_abi_demo")
    libdir = os.path.join(root, "epidemicmodeling_amd")
    subprocess.check_call(["gcc", "-O2", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "c_abi_demo.c"),
                           "-o", exe, "-L" + libdir, "-lepiekf", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    w = synth.make_cfg4(2, 3, 50, 20)
    c = 4
    a = H.chain_args(w, c)
    T, n = w.T, 12
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("4i", T, n, w.L, 1))
        for arr in (np.asfortranarray(a[0]).ravel(order="F"), a[1], a[10], w.prm[:, c], a[3], a[4].ravel(order="F"), a[5],
                    a[6].ravel(order="F"), a[9].ravel(order="F")):
            f.write(np.ascontiguousarray(arr, dtype=np.float64).tobytes())
    outp = tmp_path / "out.bin"
    env = dict(os.environ)
    env.pop("LD_PRELOAD", None)
    res = subprocess.run([exe, str(inp), str(outp)], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "order=3 -> rc -1, message 'Undefined order'" in res.stdout
    assert "placement: 3 arenas tried" in res.stdout, res.stdout           # epi_batch_desc.placement_tries from plain C
    got = np.fromfile(outp, dtype=np.float64)
    ref = H.oracle_batch(w.select([c]))
    exp = np.concatenate([ref["S_PLUS"][:, :, 0].ravel(), ref["S_SMOOTH"][:, :, 0].ravel(), ref["P_SMOOTH"][:, :, 0].ravel(),
                          ref["u_opt_smooth"][:, :, 0].ravel(), ref["rho"][:, 0]])
    assert np.array_equal(got, exp, equal_nan=True)


def test_lookahead_mask_ensemble(gpu_device):
    """SURVEY.md batch axis 4 (ForecastQualityAssessment.m:383-386): one chain per (region, masked tail length)."""
    from epidemicmodeling_amd import synth
    w = synth.make_mask_ensemble(6, 150, 25)
    got, ref = _run(w, gpu_device), H.oracle_batch(w)
    _compare(w, got, ref)
    # a longer mask only changes the filter from the first masked day on
    c0, c1 = 0, 24                                    # region 0: 1 and 25 masked days
    assert np.array_equal(got["S_PLUS"][:125, :, c0], got["S_PLUS"][:125, :, c1])
    assert not np.array_equal(got["S_PLUS"][140:, :, c0], got["S_PLUS"][140:, :, c1])


def test_nonsymmetric_ps_final_takes_dense_path(gpu_device):
    """Ps_final overrides P_SMOOTH(:,:,T) entry by entry (GenericEKF.m:198-202): a non-symmetric Ps_final makes the
    terminal covariance non-symmetric, which only the dense kernels represent; ekf_precheck must route there."""
    from epidemicmodeling_amd import synth
    w = synth.make_cfg4(3, 6, 50, 15)
    w.Ps_final[4 + 6 * 5, :] = 3e-9          # entry (5,6) set, (6,5) left at 0: not symmetric
    _compare(w, _run(w, gpu_device), H.oracle_batch(w))


def test_time_varying_process_noise(gpu_device):
    """Q_w as m x m x T / length-T vector / m x m x D pages used cyclically (GenericExtendedKalmanFilter.m:63-73)."""
    from epidemicmodeling_amd import synth, tools
    from oracle import oracle_lib as olib
    for mk in (lambda: synth.make_cfg4(3, 5, 60, 20), lambda: synth.make_cfg3(30, 70),
               lambda: synth.as_backward(synth.make_cfg4(2, 3, 50, 0))):
        w = H.with_time_varying_q(mk())
        got, ref = _run(w, gpu_device), H.oracle_batch(w)
        _compare(w, got, ref)
        for n in H.OUT_NAMES:
            assert np.array_equal(got[n], ref[n], equal_nan=True), (w.model, n)
        assert np.array_equal(got["pinv_rank"], ref["pinv_rank"])
    # Tools/ call shapes: vector (q(k)*eye), and 3 pages on a 20-day series (repmat => cyclic)
    T = 20
    params = dict(dt=1.0, a=np.full(12, 1e-3), b=0.05, u_max=synth.IP_MAXES, alpha_min=1e-8, alpha_max=100.0,
                  gamma=1 / 7, beta=synth.MODEL_BETA, obs_type="NEWCASES", s_min=1e-6, i_min=1e-6)
    rng = np.random.default_rng(3)
    u = np.floor(rng.random((12, T)) * 3); x = 1e-5 * (1 + rng.random(T))
    base = dict(s_init=np.array([0.99, 0.01, 1.1]), Ps_init=np.eye(3) * 1e-4, s_final=np.full(3, np.nan),
                Ps_final=np.full((3, 3), np.nan))
    qv = 1e-6 * (1 + rng.random(T))
    pages = 1e-6 * (1 + rng.random((3, 3, 3)))
    for Q_w, Q_full in ((qv, qv[None, None, :] * np.eye(3)[:, :, None]), (pages, pages[:, :, np.arange(T) % 3])):
        got = tools.SIAlphaModelEKF(u, x.reshape(1, -1), params, base["s_init"], base["Ps_init"], base["s_final"],
                                    base["Ps_final"], np.zeros(3), 0.0, Q_w, 1e-10, 0.9, 0.995, 21, 1)
        ref = olib.run("SIAlphaModelEKF", u, x, params, np.zeros(12), base["s_init"], base["Ps_init"],
                       base["s_final"], base["Ps_final"], 0.0, Q_full, 1e-10, 0.9, 0.995, 21, 1)
        for n, g in zip(H.OUT_NAMES, got):
            assert np.array_equal(np.asarray(g).reshape(-1), np.asarray(ref[n]).reshape(-1), equal_nan=True), n


def test_random_npi_monte_carlo_scenarios(gpu_device):
    """SURVEY.md 8(f1), TrainPredictPrescribeNPI.m:496-521: plans, trajectories and (J0, J1) of the random-NPI
    scenarios are bit-identical to the oracle's plan generator + SIalpha_Controlled + NPICost on [IP, u]."""
    import ctypes as C
    from epidemicmodeling_amd import batch, synth
    from oracle import oracle_lib as olib
    rng = np.random.default_rng(21)
    R, n_scen, K, n, t_hist = 37, 60, 45, 12, 80
    N = 10.0 ** rng.uniform(4, 9, R)
    sp = np.zeros((batch.SIM_PRM_COUNT, R))
    sp[0] = 1 - 100 / N; sp[1] = 100 / N; sp[2] = synth.ALPHA0; sp[3] = 1e-8; sp[4] = 100.0; sp[5] = 1 / 7
    sp[6] = 0.01; sp[7] = synth.MODEL_BETA; sp[8] = 10 / N; sp[9] = 30 / N; sp[10] = 1e-2; sp[11] = 1.0
    sp[batch.SIM_A:batch.SIM_A + n] = rng.random((n, R)) * 0.03
    sp[batch.SIM_U_MAX:batch.SIM_U_MAX + n] = synth.IP_MAXES[:, None]
    sp[batch.SIM_W:batch.SIM_W + n] = rng.random((n, R)) + 0.5
    u_min = np.zeros((n, R)); u_min[3] = 1.0
    # historic part of NPICost: new cases and weighted inputs of t_hist observed days per region
    nc_hist = rng.random((t_hist, R)) * 1e-4
    ip_hist = np.floor(rng.random((t_hist, n, R)) * (synth.IP_MAXES[None, :, None] + 1))
    J0p = np.cumsum(nc_hist, axis=0)[-1]
    J1p = np.cumsum((sp[batch.SIM_W:batch.SIM_W + n][None] * ip_hist).reshape(t_hist * n, R), axis=0)[-1]
    z = rng.standard_normal((K, 3, n_scen * R))
    lib = olib.lib()
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    for zz, pre in ((None, 0), (z, t_hist)):
        got = batch.random_npi_mc(sp, u_min, n_scen, K, seed=0x1234567890, z=zz, J0_prefix=J0p if pre else None,
                                  J1_prefix=J1p if pre else None, prefix_days=pre, store_u=True, device=gpu_device)
        U = got["u"].cpu().numpy(); gJ0 = got["J0"].cpu().numpy(); gJ1 = got["J1"].cpu().numpy()
        assert gJ0.shape == (n_scen, R)
        for (j, r) in ((0, 0), (28, 5), (29, 36), (30, 1), (59, 36), (44, 17)):
            c = j * R + r
            plan = olib.random_npi_plan(0x1234567890, r, j, n_scen, K, u_min[:, r], synth.IP_MAXES)
            assert np.array_equal(U[:, :, c].T, plan), (j, r)
            assert (plan == plan[:, :1]).all() == (2 * (j + 1) < n_scen)
            s, i, a = np.zeros(K), np.zeros(K), np.zeros(K)
            aa = np.ascontiguousarray(sp[batch.SIM_A:batch.SIM_A + n, r]); um = np.ascontiguousarray(sp[batch.SIM_U_MAX:batch.SIM_U_MAX + n, r])
            zc = None if zz is None else np.ascontiguousarray(z[:, :, c])
            lib.orc_sialpha_controlled(dp(plan), C.c_int(n), *[C.c_double(sp[k, r]) for k in (0, 1, 2)], dp(um),
                                       C.c_double(sp[3, r]), C.c_double(sp[4, r]), C.c_double(sp[5, r]), dp(aa),
                                       C.c_double(sp[6, r]), C.c_double(sp[7, r]), C.c_double(sp[8, r]),
                                       C.c_double(sp[9, r]), C.c_double(sp[10, r]), C.c_int(K), C.c_double(1.0),
                                       None if zc is None else dp(zc), dp(s), dp(i), dp(a))
            if pre:
                nc_all = np.ascontiguousarray(np.concatenate([nc_hist[:, r], s * i * a]))
                u_all = np.asfortranarray(np.concatenate([ip_hist[:, :, r].T, plan], axis=1))
            else:
                nc_all, u_all = np.ascontiguousarray(s * i * a), plan
            D = nc_all.shape[0]
            w_all = np.asfortranarray(np.repeat(sp[batch.SIM_W:batch.SIM_W + n, r][:, None], D, axis=1))
            J0, J1 = C.c_double(), C.c_double()
            lib.orc_npi_cost(dp(nc_all), dp(u_all), dp(w_all), C.c_int(n), C.c_int(D), C.byref(J0), C.byref(J1))
            assert gJ0[j, r] == J0.value and gJ1[j, r] == J1.value, (j, r, pre)
        # without u_out the scores are the same
        again = batch.random_npi_mc(sp, u_min, n_scen, K, seed=0x1234567890, z=zz, J0_prefix=J0p if pre else None,
                                    J1_prefix=J1p if pre else None, prefix_days=pre, device=gpu_device)
        assert np.array_equal(again["J0"].cpu().numpy(), gJ0) and np.array_equal(again["J1"].cpu().numpy(), gJ1)


@pytest.mark.parametrize("R,P", [(1, 1), (3, 2), (300, 250), (5, 1000), (2, 8192)])
def test_pareto_front_filter(gpu_device, R, P):
    """TrainPredictPrescribeNPI.m:624-633 per region: non-dominated mask and I_opt identical to the oracle."""
    import torch
    from epidemicmodeling_amd import batch
    from oracle import oracle_lib as olib
    rng = np.random.default_rng(R * 10007 + P)
    x = rng.random((R, P))
    J0 = x + 0.05 * rng.random((R, P)); J1 = 0.2 / (x + 0.1) + 0.05 * rng.random((R, P))
    if P > 8:
        J0[:, 3] = J0[:, 1]; J1[:, 4] = J1[:, 2]; J0[0, 5] = np.nan; J1[-1, 7] = np.nan
        J0[:, 6] = J0[:, 0]; J1[:, 6] = J1[:, 0]          # exact duplicate point: same score, first index wins
    on, io = batch.pareto_front(torch.as_tensor(J0.reshape(-1)).to(gpu_device), torch.as_tensor(J1.reshape(-1)).to(gpu_device), R)
    on, io = on.cpu().numpy(), io.cpu().numpy()
    for r in range(R):
        ron, rio = olib.pareto_front(J0[r], J1[r])
        assert np.array_equal(on[r], ron), r
        assert io[r] == rio, r
    if R == 1:
        bad = batch.pareto_front(torch.full((4,), float("nan"), dtype=torch.float64, device=gpu_device),
                                 torch.arange(4, dtype=torch.float64, device=gpu_device), 1)
        assert bad[0].all().item() and bad[1].item() == 0


# Rt_ExpFitEKF calls exp/tanh: oracle and kernels evaluate them in the same fixed operation order (epi_exp/epi_tanh), so
# this stage is bit for bit like the rest


@pytest.mark.parametrize("order", [1, 2])
def test_rt_expfit_parity(gpu_device, order):
    """Tools/Rt_ExpFitEKF.m, both orders, forecast tail + gaps + shared series, vs the C oracle.
    Bit for bit (exp/tanh are evaluated in one fixed operation order on both sides)."""
    from epidemicmodeling_amd import batch, synth
    from oracle import oracle_lib as olib
    w = synth.make_rt(40, 300, n_draws=5, order=order, horizon=21, w_bar=(0.5, 1e-4), seed=7 + order)
    w.x[100:104, 3] = np.nan
    got = batch.rt_expfit(w, gpu_device)
    ref = olib.rt_expfit_batch(w.x, w.rp, w.L, order, x_series=w.x_series)
    for n in ref:
        assert np.array_equal(got[n], ref[n], equal_nan=True), (order, n)
    # forward-only call leaves the same forward quantities
    fwd = batch.rt_expfit(w, gpu_device, outputs=["S_PLUS", "rho"])
    assert np.array_equal(fwd["S_PLUS"], got["S_PLUS"]) and np.array_equal(fwd["rho"], got["rho"]) and "S_SMOOTH" not in fwd


@pytest.mark.parametrize("T,B,L", [(1, 1, 21), (2, 3, 1), (5, 65, 2), (30, 130, 50)])
def test_rt_expfit_edge_sizes(gpu_device, T, B, L):
    from epidemicmodeling_amd import batch, synth
    from oracle import oracle_lib as olib
    w = synth.make_rt(B, max(T, 16), order=2, L=L, seed=T)
    w.x = np.ascontiguousarray(w.x[:T])
    got = batch.rt_expfit(w, gpu_device)
    ref = olib.rt_expfit_batch(w.x, w.rp, w.L, 2)
    for n in ref:
        assert np.array_equal(got[n], ref[n], equal_nan=True), n


def test_rt_expfit_tools_single_call(gpu_device):
    """Tools/Rt_ExpFitEKF.m signature and shapes through epi_rt_expfit_run_host (B = 1)."""
    from epidemicmodeling_amd import synth, tools
    from oracle import oracle_lib as olib
    w = synth.make_rt(2, 120, order=2, horizon=14)
    rp = w.rp[:, 1]
    args = (w.x[:, 1].reshape(1, -1), rp[9:11], rp[0:3], rp[3:5], rp[5], rp[11:15].reshape(2, 2, order="F"),
            rp[15:19].reshape(2, 2, order="F"), rp[6], rp[7], rp[8], w.L, 2)
    got = tools.Rt_ExpFitEKF(*args)
    ref = olib.rt_expfit(*args)
    names = ["S_MINUS", "S_PLUS", "P_MINUS", "P_PLUS", "K_GAIN", "S_SMOOTH", "P_SMOOTH", "innovations", "rho"]
    assert got[0].shape == (2, 120) and got[2].shape == (2, 2, 120) and got[4].shape == (2, 1, 120)
    assert got[7].shape == (1, 120) and got[8].shape == (120, 1)
    for n, g in zip(names, got):
        assert np.array_equal(np.asarray(g).reshape(-1), np.asarray(ref[n]).reshape(-1), equal_nan=True), n


@pytest.mark.parametrize("W", [7, 1, 2, 10, 32])
def test_preprocessing_parity(gpu_device, W):
    """data-set columns -> x, R_v, u on the device, bit-identical to the oracle per region."""
    from epidemicmodeling_amd import batch, synth
    from oracle import oracle_lib as olib
    raw = synth.make_raw_counts(70, 130, seed=W)
    got = batch.preprocess(raw["cases"], raw["population"], raw["deaths"], raw["ip"], W=W, min_cases=1.0,
                           first_num_days=7, device=gpu_device)
    g = {k: v.cpu().numpy() for k, v in got.items()}
    for r in range(70):
        ref = olib.preprocess_region(raw["cases"][:, r], raw["deaths"][:, r], raw["population"][r], W=W, min_cases=1.0)
        for k in ("new_refined", "new_smoothed", "zero_lag", "x_new", "x_total", "R_v", "fatality"):
            assert np.array_equal(g[k][:, r], ref[k], equal_nan=True), (W, r, k)
        assert g["I0"][r] == ref["I0"]
    for r in (0, 2, 69):
        assert np.array_equal(g["ip_filled"][:, :, r], olib.npi_fill(np.ascontiguousarray(raw["ip"][:, :, r])))
    # reduced selection, no deaths / NPIs
    few = batch.preprocess(raw["cases"], raw["population"], W=W, outputs=["x_new", "R_v", "I0"], device=gpu_device)
    assert set(few) == {"x_new", "R_v", "I0"} and np.array_equal(few["R_v"].cpu().numpy(), g["R_v"])


def test_preprocessing_feeds_the_filter(gpu_device):
    """End to end on the device: raw columns -> preprocess -> SIAlphaModelEKF inputs -> filter, equal to the oracle
    run on the oracle's preprocessing of the same columns."""
    import torch
    from epidemicmodeling_amd import batch, synth, layout as L_
    from oracle import oracle_lib as olib
    S, T = 24, 160
    raw = synth.make_raw_counts(S, T, seed=11)
    pre = batch.preprocess(raw["cases"], raw["population"], raw["deaths"], raw["ip"], device=gpu_device)
    w = synth.make_cfg3(S, T)                       # parameters / initial conditions; series replaced below
    w.x = pre["x_new"].cpu().numpy(); w.R_series = pre["R_v"].cpu().numpy() + 1e-16; w.u = pre["ip_filled"].cpu().numpy()
    got = batch.run_workload(w, device=gpu_device)
    x_o = np.stack([olib.preprocess_region(raw["cases"][:, r], None, raw["population"][r])["x_new"] for r in range(S)], axis=1)
    assert np.array_equal(w.x, x_o)
    ref = H.oracle_batch(w)
    for n in H.OUT_NAMES:
        assert np.array_equal(got[n], ref[n], equal_nan=True), n


def test_preprocessing_errors(gpu_device):
    import torch
    from epidemicmodeling_amd import batch
    from epidemicmodeling_amd._lib import EpiError
    c = np.cumsum(np.ones((9, 3)), axis=0)
    with pytest.raises(EpiError, match="Data length must be larger than 9 samples"):
        batch.preprocess(c, np.ones(3), device=gpu_device)
    with pytest.raises(EpiError, match="Insufficient data"):
        batch.preprocess(c[:1], np.ones(3), device=gpu_device)
    with pytest.raises(EpiError, match="SmoothingWinLen"):
        batch.preprocess(np.cumsum(np.ones((200, 3)), axis=0), np.ones(3), W=33, device=gpu_device)


@pytest.mark.parametrize("S,D,n", [(70, 120, 12), (1, 30, 12), (33, 60, 5), (40, 8, 12), (5, 200, 1)])
def test_nnls_affine_fit_parity(gpu_device, S, D, n):
    """the batched NNLS + intercept loop on the device, bit-identical to the oracle per region
    (including rank-deficient windows: constant, collinear and zero columns, fewer days than NPIs)."""
    from epidemicmodeling_amd import batch
    from oracle import oracle_lib as olib
    X, y = H.make_regression_problem(S, D, n, seed=S + D)
    got = batch.nnls_affine_fit(X, y, device=gpu_device)
    g = {k: v.cpu().numpy() for k, v in got.items()}
    for s in range(S):
        ref = olib.nnls_affine_fit(np.ascontiguousarray(X[:, :, s]), np.ascontiguousarray(y[:, s]))
        assert np.array_equal(g["a"][:, s], ref["a"]), s
        assert g["b"][s] == ref["b"] and g["min_err"][s] == ref["min_err"] and g["iters"][s] == ref["iters"], s
        assert (g["a"][:, s] >= 0).all() and g["flag"][s] == 1


def test_prescription_pipeline_stage_by_stage(gpu_device):
    """The device stages of TrainPredictPrescribeNPI.m chained for all regions (epidemicmodeling_amd/pipeline.py): every
    stage is re-derived from the previous stage's output with the CPU oracle and must agree bit for bit."""
    from epidemicmodeling_amd import pipeline, synth
    from oracle import oracle_lib as olib
    S, T, H_, n_eps, D = 7, 150, 25, 12, 50
    raw = synth.make_raw_counts(S, T, seed=31)
    raw["cases"][:, -1] = np.cumsum(np.full(T, 40.0))            # the all-NaN region of the generator: give it data
    out = pipeline.prescribe(raw["cases"], raw["deaths"], raw["population"], raw["ip"], horizon=H_, n_eps=n_eps,
                             num_regression_days=D, device=gpu_device)
    N = raw["population"]; pre = out["pre"]
    for r in range(S):
        ref = olib.preprocess_region(raw["cases"][:, r], raw["deaths"][:, r], N[r])
        assert np.array_equal(pre["x_new"][:, r], ref["x_new"]) and np.array_equal(pre["R_v"][:, r], ref["R_v"]) and pre["I0"][r] == ref["I0"]
    x, R, u, I0 = pre["x_new"], pre["R_v"], pre["ip_filled"], pre["I0"]
    n = u.shape[1]
    o1 = H.oracle_batch(pipeline.workload3(x, R, np.zeros_like(u), N, I0, np.zeros((n, S)), np.zeros(S)), outputs=["S_SMOOTH"])
    assert np.array_equal(out["alpha_round1"], o1["S_SMOOTH"][:, 2])
    X = synth.IP_MAXES[None, :n, None] - u[T - D:]
    for r in range(S):
        f = olib.nnls_affine_fit(np.ascontiguousarray(X[:, :, r]), np.ascontiguousarray(out["alpha_round1"][T - D:, r]))
        assert np.array_equal(out["fit1"]["a"][:, r], f["a"]) and out["fit1"]["b"][r] == f["b"]
    o2 = H.oracle_batch(pipeline.workload3(x, R, u, N, I0, out["fit1"]["a"], out["fit1"]["b"]), outputs=["S_SMOOTH"])
    assert np.array_equal(out["alpha_round2"], o2["S_SMOOTH"][:, 2])
    for r in range(S):
        f = olib.nnls_affine_fit(np.ascontiguousarray(X[:, :, r]), np.ascontiguousarray(out["alpha_round2"][T - D:, r]))
        assert np.array_equal(out["fit2"]["a"][:, r], f["a"]) and out["fit2"]["b"][r] == f["b"]
    assert (out["fit2"]["a"] >= 0).all()
    os_ = H.oracle_batch(out["sweep"], outputs=["u_opt_smooth"])
    chains = np.arange(S) * n_eps + out["i_opt"]
    assert np.array_equal(out["prescription"], os_["u_opt_smooth"][T:][:, :, chains])
    assert out["prescription"].shape == (H_, n, S)
    lv = out["prescription"][:-1]                                 # bang-bang plans: every level is u_min or u_max
    assert np.isin(lv, np.concatenate([[0.0], synth.IP_MAXES])).all()
    for r in range(S):
        on, io = olib.pareto_front(out["J0"][r], out["J1"][r])
        assert np.array_equal(out["front"][r], on) and out["i_opt"][r] == io
    assert np.isfinite(out["J0"]).all() and np.isfinite(out["J1"]).all()


def test_batch_beyond_the_resident_wave_slots(gpu_device):
    """More chains than the device has wave slots for the one-wave-per-SIMD kernels (the launch then narrows its waves so
    that the rounds are equally full): 66 300 chains x 6 days; same bits as the oracle, also when the call is captured
    into a HIP graph and replayed."""
    import torch
    from epidemicmodeling_amd import batch, synth
    w = synth.make_cfg4(68, 975, 4, 2)
    assert w.B > 4 * torch.cuda.get_device_properties(0).multi_processor_count * 64
    ref = H.oracle_batch(w)
    got = batch.run_workload(w, device=gpu_device)
    for n in H.OUT_NAMES:
        assert np.array_equal(got[n], ref[n], equal_nan=True), n
    assert np.array_equal(got["pinv_rank"], ref["pinv_rank"])
    dw = batch.DeviceWorkload(w, gpu_device)
    # reduced outputs: the forward kernel's two-waves-per-SIMD variant, one launch; all outputs: forward kernel and pinv grid in two
    # chain ranges, the first range's grid on the helper stream beside the second forward launch (round 6) -- both captured
    for outs in (["S_SMOOTH", "u_opt_smooth"], None):
        r = batch.EkfRunner(dw, outputs=outs)
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            r.run()                                     # warm-up outside the capture (helper streams get created)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            r.run(stream=s)
        for t in r.out.values():
            t.zero_()
        g.replay(); torch.cuda.synchronize()
        for n in r.out:
            assert np.array_equal(r.out[n].cpu().numpy(), ref[n], equal_nan=True), (outs, n)
        del g, r


def test_gpu_reproduces_aux_golden_vectors(gpu_device):
    """The committed fixtures of the stages around the filter (tests/golden/aux_*.npz) through the HIP path: bit for bit."""
    import os
    import torch
    from epidemicmodeling_amd import batch, synth
    ld = lambda n: np.load(os.path.join(H.ROOT, "tests", "golden", n + ".npz"))
    for order in (1, 2):
        g = ld(f"aux_rt_order{order}")
        w = synth.RtWorkload(x=g["in_x"], rp=g["in_rp"], x_series=None, L=int(g["in_L"]), order=order)
        got = batch.rt_expfit(w, gpu_device)
        for k, v in got.items():
            assert np.array_equal(v, g["out_" + k], equal_nan=True), (order, k)
    g = ld("aux_preprocess")
    got = {k: v.cpu().numpy() for k, v in batch.preprocess(g["in_cases"], g["in_population"], g["in_deaths"], g["in_ip"],
                                                           device=gpu_device).items()}
    for k in ("new_refined", "new_smoothed", "zero_lag", "x_new", "x_total", "R_v", "fatality", "I0", "ip_filled"):
        assert np.array_equal(got[k], g["out_" + k]), k
    g = ld("aux_nnls")
    got = {k: v.cpu().numpy() for k, v in batch.nnls_affine_fit(g["in_X"], g["in_y"], device=gpu_device).items()}
    assert np.array_equal(got["a"], g["out_a"]) and np.array_equal(got["b"], g["out_b"])
    assert np.array_equal(got["min_err"], g["out_min_err"]) and np.array_equal(got["iters"], g["out_iters"])
    g = ld("aux_scenarios")
    P = g["out_plans"]; n_scen, R, n, K = P.shape
    sp = np.zeros((batch.SIM_PRM_COUNT, R)); sp[0] = 0.99; sp[1] = 0.01; sp[2] = 1.0; sp[4] = 100.0; sp[5] = 1 / 7; sp[11] = 1.0
    sp[batch.SIM_U_MAX:batch.SIM_U_MAX + n] = synth.IP_MAXES[:, None]
    mc = batch.random_npi_mc(sp, np.zeros((n, R)), n_scen, K, seed=int(g["in_seed"]), store_u=True, device=gpu_device)
    U = mc["u"].cpu().numpy()                                       # [K, n, n_scen*R], chain = scenario * R + region
    assert np.array_equal(U.reshape(K, n, n_scen, R).transpose(2, 3, 1, 0), P)
    on, io = batch.pareto_front(torch.as_tensor(g["in_J0"].reshape(-1)).to(gpu_device),
                                torch.as_tensor(g["in_J1"].reshape(-1)).to(gpu_device), g["in_J0"].shape[0])
    assert np.array_equal(on.cpu().numpy(), g["out_on_front"]) and np.array_equal(io.cpu().numpy(), g["out_i_opt"])
    # the look-ahead study, the sliding-window estimators and the LASSO (NaN payloads free, everything else bit for bit)
    from tests import lookahead_ref as LR
    from tests.test_gpu_lasso import _run_device, _same as same_lasso
    from tests.test_gpu_rt_window import _same as same_rtw
    g = ld("aux_lookahead")
    got = batch.lookahead(LR.golden_workload(g), g["in_truth"], g["in_population"], int(g["in_F"]), int(g["in_M"]),
                          device=gpu_device)
    want = {k[4:]: g[k] for k in g.files if k.startswith("out_")}
    same_lasso({k: got[k] for k in want}, want)
    g = ld("aux_rt_window")
    for c in range(2):
        got = batch.rt_window(g["in_x"], int(g[f"in_c{c}_wlen"]), float(g[f"in_c{c}_time_unit"]), int(g[f"in_c{c}_causal"]),
                              int(g[f"in_c{c}_gp"]), ("LogLinReg", "GenRatios", "NonlinLS"), device=gpu_device)
        torch.cuda.synchronize()
        same_rtw(got, {k[len(f"out_c{c}_"):]: g[k] for k in g.files if k.startswith(f"out_c{c}_")})
    g = ld("aux_lasso")
    got = _run_device(g["in_X"], g["in_y"], g["in_fold"], int(g["in_K"]), int(g["in_NL"]), device=gpu_device)
    same_lasso(got, {k[4:]: g[k] for k in g.files if k.startswith("out_")})


@pytest.mark.parametrize("blk", [8, 40, 3])
def test_chain_blocked_output_layout(gpu_device, blk):
    """epi_batch_desc.lane_block: the outputs (and the workspace) in the chain-blocked layout
    ((t*nblk + c/blk)*rows + row)*blk + c%blk hold exactly the values of the classic [T][rows][B] run -- all model
    variants, chain counts that are not a multiple of the block, reduced output sets, chunked launches."""
    from epidemicmodeling_amd import batch, synth
    cases = [synth.make_cfg4(5, 13, 40, 15),                       # 65 chains, 6-state packed kernels
             synth.make_cfg3(37, 50),                               # 3-state
             synth.make_row4(11, 60, 20),                           # NewCase (dense kernels)
             synth.as_backward(synth.make_cfg4(3, 7, 30, 0))]       # time-flipped
    for w in cases:
        ref = H.oracle_batch(w)
        got = batch.run_workload(w, device=gpu_device, lane_block=blk)
        for n in H.OUT_NAMES:
            if n in got:
                assert got[n].shape == ref[n].shape and np.array_equal(got[n], ref[n], equal_nan=True), (w.model, blk, n)
        assert np.array_equal(got["pinv_rank"], ref["pinv_rank"]), (w.model, blk)
    w = cases[0]
    ref = H.oracle_batch(w)
    few = batch.run_workload(w, outputs=["u_opt_smooth", "S_SMOOTH"], device=gpu_device, lane_block=blk, time_pipe=1)
    assert np.array_equal(few["u_opt_smooth"], ref["u_opt_smooth"], equal_nan=True) and np.array_equal(few["S_SMOOTH"], ref["S_SMOOTH"], equal_nan=True)
    wd = synth.make_cfg4(4, 8, 60, 20); wd.Q[1 + 6 * 0] = 1e-12                      # dense fallback path
    assert np.array_equal(batch.run_workload(wd, device=gpu_device, lane_block=blk)["P_SMOOTH"], H.oracle_batch(wd)["P_SMOOTH"], equal_nan=True)


def test_scoring_reads_blocked_u_opt_smooth(gpu_device):
    import torch
    from epidemicmodeling_amd import batch, synth
    w = synth.make_cfg4(6, 12, 70, 40)
    dw = batch.DeviceWorkload(w, gpu_device)
    sp = np.zeros((batch.SIM_PRM_COUNT, w.B)); sp[0] = 0.99; sp[1] = 0.01; sp[2] = 1.0; sp[4] = 100.0; sp[5] = 1 / 7; sp[11] = 1.0
    sp[batch.SIM_A:batch.SIM_A + 12] = 0.01; sp[batch.SIM_U_MAX:batch.SIM_U_MAX + 12] = synth.IP_MAXES[:, None]; sp[batch.SIM_W:batch.SIM_W + 12] = 1.0
    z = np.zeros(w.B)
    res = []
    for blk in (0, 8):
        r = batch.EkfRunner(dw, outputs=["u_opt_smooth", "S_SMOOTH"], lane_block=blk)
        r.run(); torch.cuda.synchronize()
        sc = batch.score_sweep(r.out["u_opt_smooth"], 70, sp, z, z, B=w.B)
        res.append((sc["J0"].cpu().numpy(), sc["J1"].cpu().numpy()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def _sweep_scoring_inputs(w, rng):
    """sp [48, B], J0_prefix, J1_prefix [B] of a scoring tail for workload `w` (random weights and prefixes: the tail's
    arithmetic does not care where they come from)."""
    from epidemicmodeling_amd import batch, layout as L_, synth
    n, B = w.n_npi, w.B
    sp = np.zeros((batch.SIM_PRM_COUNT, B))
    sp[0] = 1.0 - 1e-3 * rng.random(B); sp[1] = 1e-3 * rng.random(B); sp[2] = synth.ALPHA0 * (0.5 + rng.random(B))
    sp[3] = w.prm[L_.PRM_ALPHA_MIN]; sp[4] = w.prm[L_.PRM_ALPHA_MAX]; sp[5] = w.prm[L_.PRM_GAMMA]
    sp[6] = w.prm[L_.PRM_B]; sp[7] = w.prm[L_.PRM_BETA]; sp[11] = 1.0
    sp[batch.SIM_A:batch.SIM_A + n] = w.prm[L_.PRM_A:L_.PRM_A + n]
    sp[batch.SIM_U_MAX:batch.SIM_U_MAX + n] = w.prm[L_.PRM_U_MAX:L_.PRM_U_MAX + n]
    sp[batch.SIM_W:batch.SIM_W + n] = rng.random((n, B)) + 0.5
    return sp, rng.random(B) * 1e-2, rng.random(B) * 50.0


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("lane_block", [0, "auto"])
def test_sweep_entry_equals_filter_then_scoring_then_front(gpu_device, shape, lane_block):
    """epi_sweep_run_device = epi_ekf_run_device + epi_sialpha_score_device + epi_pareto_front_device, bit for bit: the
    smoother cut in two launches where the horizon ends (hand-over through the workspace), scoring and Pareto filter on the
    helper stream beside the second one.  Filter outputs against the oracle; (J0, J1), front and I_opt against the three
    separate calls.  Cases: long and short (time-pipelined or not), a horizon of one day (no cut: t_hist = T - 1), all
    outputs and the reduced set, both layouts, both lane mappings, the dense fall-back (non-diagonal Q_w)."""
    import torch
    from epidemicmodeling_amd import batch, synth
    rng = np.random.default_rng(77)
    cases = [(synth.make_cfg4(5, 9, 150, 30), 150, None), (synth.make_cfg4(7, 11, 40, 25), 40, ["u_opt_smooth", "S_SMOOTH"]),
             (synth.make_cfg4(3, 6, 30, 1), 30, ["u_opt_smooth"]), (synth.make_cfg4(4, 5, 1, 9), 1, None)]
    dense = synth.make_cfg4(3, 5, 50, 12); dense.Q = dense.Q.copy(); dense.Q[1] = 1e-13
    cases.append((dense, 50, None))
    for w, t_hist, outputs in cases:
        ref = H.oracle_batch(w)
        sp, j0p, j1p = _sweep_scoring_inputs(w, rng)
        dw = batch.DeviceWorkload(w, gpu_device)
        to = lambda a: torch.as_tensor(a, dtype=torch.float64).to(gpu_device)
        sp_d, j0_d, j1_d = to(sp), to(j0p), to(j1p)
        # the three separate calls
        r0 = batch.EkfRunner(dw, outputs=outputs, extras=True, lane_block=lane_block, shape=shape)
        r0.run()
        sc0 = batch.score_sweep(r0.out["u_opt_smooth"], t_hist, sp_d, j0_d, j1_d, B=w.B)
        on0, io0 = batch.pareto_front(sc0["J0"], sc0["J1"], w.Sx)
        torch.cuda.synchronize()
        # one call; the outputs and the workspace poisoned first
        r1 = batch.EkfRunner(dw, outputs=outputs, extras=True, lane_block=lane_block, shape=shape)
        for t in list(r1.out.values()) + [r1.ws]:
            t.fill_(float("nan"))
        sc1 = r1.run_sweep(t_hist, sp_d, j0_d, j1_d, n_regions=w.Sx)
        torch.cuda.synchronize()
        for n in r1.out:
            assert np.array_equal(r1.unblocked(n).cpu().numpy(), ref[n], equal_nan=True), (w.T, t_hist, shape, lane_block, n)
        assert np.array_equal(r1.unblocked("pinv_rank").cpu().numpy(), ref["pinv_rank"])
        assert np.array_equal(r1.status.cpu().numpy(), r0.status.cpu().numpy())      # accumulated across the two launches
        for k in ("J0", "J1"):
            assert np.array_equal(sc1[k].cpu().numpy(), sc0[k].cpu().numpy()), (w.T, t_hist, shape, lane_block, k)
        assert np.array_equal(sc1["on_front"].bool().cpu().numpy(), on0.cpu().numpy())
        assert np.array_equal(sc1["i_opt"].cpu().numpy(), io0.cpu().numpy())
        # a shard that does not hold whole regions: scoring only
        r2 = batch.EkfRunner(dw, outputs=outputs, lane_block=lane_block, shape=shape)
        sc2 = r2.run_sweep(t_hist, sp_d, j0_d, j1_d)
        torch.cuda.synchronize()
        assert "on_front" not in sc2 and np.array_equal(sc2["J0"].cpu().numpy(), sc0["J0"].cpu().numpy())


def test_sweep_entry_rejects_what_it_cannot_score(gpu_device):
    import torch
    from epidemicmodeling_amd import _lib, batch, synth
    w = synth.make_cfg4(3, 4, 20, 5)
    dw = batch.DeviceWorkload(w, gpu_device)
    z = torch.zeros(w.B, dtype=torch.float64, device=gpu_device)
    sp = torch.zeros((batch.SIM_PRM_COUNT, w.B), dtype=torch.float64, device=gpu_device)
    r = batch.EkfRunner(dw, outputs=["S_SMOOTH"])
    with pytest.raises(_lib.EpiError, match="u_opt_smooth"):
        r.run_sweep(20, sp, z, z)
    r = batch.EkfRunner(dw)
    for bad in (0, w.T, w.T + 3):
        with pytest.raises(_lib.EpiError, match="t_hist"):
            r.run_sweep(bad, sp, z, z)
    with pytest.raises(ValueError):
        r.run_sweep(20, sp, z, z, n_regions=5)                 # 12 chains are not 5 whole regions
    w3 = synth.make_cfg3(6, 30)
    r3 = batch.EkfRunner(batch.DeviceWorkload(w3, gpu_device))
    with pytest.raises(_lib.EpiError, match="SIAlphaModelEKFOptControlled"):
        r3.run_sweep(20, sp, z, z)


def _region_sweep_problem(S, P, T_hist, hor, seed=0, n=12):
    """A cost-weight sweep of `n` NPIs given by PER-REGION inputs (what epi_sweep_prescribe_host takes) and the per-chain
    workload the library expands it to (what the oracle runs)."""
    from epidemicmodeling_amd import pipeline, synth
    w0 = synth.make_cfg4(S, 1, T_hist, hor)                      # one chain per region: the regions' series and constants
    rng = np.random.default_rng(seed)
    N = np.asarray(synth.make_regions(S)["N"], dtype=np.float64)
    I0 = np.maximum(1.0, rng.random(S) * 50.0)
    a, b = rng.random((n, S)) * 0.02, rng.random(S) * 0.05
    eps = synth.epsilon_grid(P)
    x, R, u = w0.x, w0.R_series, np.ascontiguousarray(w0.u[:, :n, :])
    reg = pipeline.sweep_region_inputs(N, I0, a, b, n)
    w6 = pipeline.workload6(x, R, u, N, I0, a, b, eps)
    sp = pipeline.scoring_region_inputs(np.stack([1.0 - 1e-3 * rng.random(S), 1e-3 * rng.random(S), synth.ALPHA0 * (0.5 + rng.random(S))]),
                                        a, b, synth.IP_MAXES[:n], rng.random((n, S)) + 0.5)
    return dict(x=x, R=R, u=u, reg=reg, eps=eps, sp=sp, J0p=rng.random(S) * 1e-2, J1p=rng.random(S) * 40.0, w6=w6, t_hist=T_hist)


def test_sweep_prescribe_host_all_regions_in_one_call(gpu_device):
    """epi_sweep_prescribe_host: per-region host arrays in; (J0, J1), front, I_opt and the optimum's plan / smoothed states
    out.  Against the chain of device calls on the expanded per-chain workload (filter outputs also against the oracle):
    one device, the regions cut into three ragged blocks (the one GPU named three times: whole regions per block, no
    exchange), per-chain extras (classic layout) and none (blocked layout), a batch on the dense kernels."""
    import torch
    from epidemicmodeling_amd import batch, hostapi
    for S, P, T_hist, hor, dense in ((7, 11, 60, 15, False), (4, 25, 140, 30, False), (3, 6, 30, 8, True)):
        pr = _region_sweep_problem(S, P, T_hist, hor, seed=S)
        if dense:
            pr["reg"]["Q"][1] = 1e-13                                  # non-diagonal Q_w: the host precheck picks the dense kernels
            pr["w6"].Q = pr["reg"]["Q"][:, np.repeat(np.arange(S), P)]
        w6, T = pr["w6"], T_hist + hor
        ref = H.oracle_batch(w6)
        rr = np.repeat(np.arange(S), P)
        dw = batch.DeviceWorkload(w6, gpu_device)
        r0 = batch.EkfRunner(dw, outputs=["u_opt_smooth", "S_SMOOTH"])
        to = lambda v: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64).to(gpu_device)
        sc = r0.run_sweep(T_hist, to(pr["sp"][:, rr]), to(pr["J0p"][rr]), to(pr["J1p"][rr]), n_regions=S)
        torch.cuda.synchronize()
        J0 = sc["J0"].cpu().numpy().reshape(S, P); J1 = sc["J1"].cpu().numpy().reshape(S, P)
        io = sc["i_opt"].cpu().numpy(); on = sc["on_front"].bool().cpu().numpy()
        chains = np.arange(S) * P + io
        for devices, extras in (((0,), ()), ((0, 0, 0), ()), ((0,), ("u_opt_smooth", "S_SMOOTH", "P_SMOOTH", "rho")), ((0, 0), ("S_PLUS",))):
            got = hostapi.sweep_prescribe(pr["x"], pr["u"], pr["R"], pr["reg"], pr["eps"], pr["sp"], pr["J0p"], pr["J1p"], T_hist,
                                          devices=devices, extras=extras)
            tag = (S, P, devices, extras)
            assert np.array_equal(got["J0"], J0) and np.array_equal(got["J1"], J1), tag
            assert np.array_equal(got["on_front"], on) and np.array_equal(got["i_opt"], io), tag
            assert np.array_equal(got["u_opt"], ref["u_opt_smooth"][:, :, chains]), tag
            assert np.array_equal(got["S_opt"], ref["S_SMOOTH"][:, :, chains], equal_nan=True), tag
            for n in extras:
                assert np.array_equal(got[n], ref[n], equal_nan=True), (tag, n)
        # epi_prescribe_desc.placement_tries: the arena kept is the fastest of two candidates, results unchanged
        from epidemicmodeling_amd import _lib
        _lib.lib().epi_host_pool_release()
        got = hostapi.sweep_prescribe(pr["x"], pr["u"], pr["R"], pr["reg"], pr["eps"], pr["sp"], pr["J0p"], pr["J1p"], T_hist, placement_tries=2)
        assert got["placement"]["tries"] == 2 and len(got["placement"]["ms"]) == 2, got["placement"]
        assert np.array_equal(got["J0"], J0) and np.array_equal(got["J1"], J1) and np.array_equal(got["i_opt"], io)
        assert np.array_equal(got["u_opt"], ref["u_opt_smooth"][:, :, chains])
    with pytest.raises(Exception, match="t_hist"):
        hostapi.sweep_prescribe(pr["x"], pr["u"], pr["R"], pr["reg"], pr["eps"], pr["sp"], pr["J0p"], pr["J1p"], T)


def test_host_forms_of_the_stages_around_the_filter(gpu_device):
    """epi_preprocess_host / epi_nnls_affine_fit_host / epi_random_npi_mc_host = their device forms on the same arrays."""
    from epidemicmodeling_amd import batch, hostapi, synth
    raw = synth.make_raw_counts(9, 120, seed=4)
    a = hostapi.preprocess(raw["cases"], raw["population"], raw["deaths"], raw["ip"])
    b = batch.preprocess(raw["cases"], raw["population"], raw["deaths"], raw["ip"], device=gpu_device)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k].cpu().numpy(), equal_nan=True), k
    rng = np.random.default_rng(2)
    X = rng.integers(0, 4, size=(40, 12, 9)).astype(np.float64); y = rng.random((40, 9))
    fa, fb = hostapi.nnls_affine_fit(X, y), batch.nnls_affine_fit(X, y, device=gpu_device)
    for k in fa:
        assert np.array_equal(fa[k], fb[k].cpu().numpy()), k
    sp = np.zeros((batch.SIM_PRM_COUNT, 9)); sp[0] = 0.99; sp[1] = 0.01; sp[2] = 1.0; sp[4] = 100.0; sp[5] = 1 / 7; sp[7] = synth.MODEL_BETA; sp[11] = 1.0
    sp[batch.SIM_A:batch.SIM_A + 12] = 0.01; sp[batch.SIM_U_MAX:batch.SIM_U_MAX + 12] = synth.IP_MAXES[:, None]; sp[batch.SIM_W:batch.SIM_W + 12] = 1.0
    ma = hostapi.random_npi_mc(sp, np.zeros((12, 9)), 30, 25, seed=77, store_u=True)
    mb = batch.random_npi_mc(sp, np.zeros((12, 9)), 30, 25, seed=77, store_u=True, device=gpu_device)
    for k in ("J0", "J1", "u"):
        assert np.array_equal(ma[k], mb[k].cpu().numpy()), k


def test_host_forms_of_the_simulators_and_small_fits_equal_their_device_forms(gpu_device):
    """Each of the nine host functions of the simulators and small fits = its *_device sibling on the same inputs, word for
    word, once with every optional array present and once with every optional array absent (H.flat_call_cases: u_series /
    alpha_series NULL against a shared series, no z, no J0 / J1, no u_out, prefix_days 0 and 7, no sat, no deaths / ip with
    n_npi = 0, single outputs of the fits, Rt_ExpFitEKF asked for S_SMOOTH alone -- its four forward arrays then live on the
    device only -- and for everything).  The seeded forms = the unseeded ones fed normal_draws of the same seed and stream."""
    from epidemicmodeling_amd import _lib, hostapi
    cases = H.flat_call_cases()
    host = {}
    for name, (sym, args, dev_args) in cases.items():
        host[name] = H.flat_call(sym, args)
        dev = H.flat_call(sym, dev_args, gpu=gpu_device)
        assert host[name] and set(host[name]) <= set(dev), name
        for k, v in host[name].items():
            assert v.dtype == dev[k].dtype and np.array_equal(v, dev[k], equal_nan=True), (name, k)
            assert not (np.isnan(v).all() if v.dtype == np.float64 else (v == -1).all()), (name, k)     # (written at all)
    for fn in ("sialpha_sim", "random_npi_mc"):
        sym, args, _ = cases[fn + "/seeded"]
        args = [a for a in args if not isinstance(a, _lib.NoiseDesc)]
        zi = next(i for i, a in enumerate(args) if a is None)               # the first NULL of a seeded call is its z
        K, lanes = (args[0].K, args[0].B) if fn == "sialpha_sim" else (args[0].K, args[0].R * args[0].n_scen)
        args[zi] = hostapi.normal_draws(K, 3, lanes, H.FLAT_SEED, stream=H.FLAT_STREAM)
        args[0].noise = 1
        fed = H.flat_call(sym, args)
        args[0].noise = 0
        for k, v in host[fn + "/seeded"].items():
            assert np.array_equal(v, fed[k], equal_nan=True), (fn, k)


@pytest.mark.parametrize("adaptive", [False, True])
def test_quad_shape_with_the_longest_monitor_window(gpu_device, adaptive):
    """inv_monitor_len = 106 (the largest the library accepts) with four lanes per chain: with an adaptive scalar R_v the
    monitor stays inside ekf_fwd_quad and its six windows of 106 samples for 16 chains need 83 KB of dynamic LDS -- above the
    default limit, so the launch raises the kernel's limit first; with a per-day R_v the monitor kernel takes the general
    (L != 21) path.  Same bits as the oracle either way."""
    from epidemicmodeling_amd import synth
    w = synth.make_row3(3, 7, 40, 90) if adaptive else synth.make_cfg4(3, 7, 110, 30)
    w.L = 106
    ref = H.oracle_batch(w)
    for blk in (0, "auto"):
        got = _run(w, gpu_device, shape="quad", lane_block=blk)
        for n in H.OUT_NAMES:
            assert np.array_equal(got[n], ref[n], equal_nan=True), (adaptive, blk, n)
        assert np.array_equal(got["pinv_rank"], ref["pinv_rank"])


def test_preferred_lane_block_matches_launch(gpu_device):
    """epi_ekf_preferred_lane_block = chains per wavefront of the launch; "auto" uses it and gives the same results."""
    import ctypes as C
    from epidemicmodeling_amd import _lib, batch, synth
    w = synth.make_cfg4(5, 13, 40, 15)
    dw = batch.DeviceWorkload(w, gpu_device)
    r = batch.EkfRunner(dw, lane_block="auto", extras=True)
    assert r.blk == 1                                          # 65 chains: one WAVEFRONT per chain, a chain's rows together
    r_quad = batch.EkfRunner(dw, lane_block="auto", shape="quad")
    assert r_quad.blk == 16                                    # ... four lanes per chain: 16 chains per wavefront
    r_lane = batch.EkfRunner(dw, lane_block="auto", shape="lane")
    assert r_lane.blk == 64                                    # ... or, one lane per chain, in one round of 64-lane waves
    r.run()
    import torch
    torch.cuda.synchronize()
    ref = H.oracle_batch(w)
    for n in H.OUT_NAMES:
        assert np.array_equal(r.unblocked(n).cpu().numpy(), ref[n], equal_nan=True), n
    d = _lib.make_desc("SIAlphaModelEKFOptControlled", 75000, 520, 300, 300, 12, 21, 1, "NEWCASES", 1, 0xFFFF)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    blk = _lib.lib().epi_ekf_preferred_lane_block(C.byref(d))
    assert blk % 8 == 0 and (75000 + blk - 1) // blk <= 2 * cus * 4 and blk == 40 or cus != 256


@pytest.mark.parametrize("blk", [8, "auto", 40])
def test_time_pipelined_launch_with_blocked_layout(gpu_device, blk):
    """The time-pipelined launch writes the chain-blocked layouts correctly too (T >= 128 so that it engages; reduced
    outputs as well: S+-, P+- then live in the workspace, upper triangles only)."""
    from epidemicmodeling_amd import batch, synth
    w = synth.make_cfg4(16, 50, 110, 20)                   # 800 chains x 130 days
    ref = H.oracle_batch(w)
    got = batch.run_workload(w, device=gpu_device, time_pipe=1, lane_block=blk)
    for n in H.OUT_NAMES:
        assert np.array_equal(got[n], ref[n], equal_nan=True), (blk, n)
    assert np.array_equal(got["pinv_rank"], ref["pinv_rank"])
    few = batch.run_workload(w, outputs=["u_opt_smooth", "S_SMOOTH"], device=gpu_device, time_pipe=1, lane_block=blk)
    for n in ("u_opt_smooth", "S_SMOOTH", "pinv_rank"):
        assert np.array_equal(few[n], ref[n], equal_nan=True), (blk, n)


@pytest.mark.parametrize("lane_block,live", [(0, False), ("auto", False), ("auto", True)])
def test_headline_sweep_at_full_size_sampled_chains(gpu_device, lane_block, live):
    """BASELINE's headline configuration at full size -- 300 regions x 250 cost weights x (400 + 120) days = 75 000 chains,
    all 11 outputs (49 GB) -- checked through a size-independent property: chains are independent, so every chain of the
    big batch must equal, bit for bit, the oracle's run of that chain alone.  First 257 chains spread over the batch (first,
    last, wave and block boundaries included: where an error that depends on a chain's PLACE would sit), then ALL 75 000, in chain
    ranges (H.all_chains_equal_oracle: an error that depends on WHEN something happens -- a stale LDS-DMA image, a missing event
    edge between the chain ranges' launches -- hits a few waves somewhere, and the sample would see one bad wave of 1 875 with
    13 %).  The second pass, through the one-call sweep entry into poisoned outputs, is compared over the whole batch with device
    clones of the first; on the library's own layout and the dead workload also the last of five sweep passes enqueued back to
    back and the replay of a captured graph (_back_to_back_and_graph_replay).  live: the same sweep on the living multi-wave epidemic
    (synth.make_cfg4(live=True), `bench.py --workload cfg4-live`), whose covariances keep full rank for ~150 days and then
    drop to rank 1 -- another mix of the pinv routes than the survey's series."""
    _headline_sweep_sampled(gpu_device, lane_block, live)


def test_headline_sweep_at_full_size_one_npi(gpu_device):
    """The headline sweep at full size with n_npi = 1, on the library's own 40-chain layout: the one-lane smoother that takes X
    by LDS-DMA (eks_bwd_lane6 with XD = 1) then issues the fewest vector-memory operations between that DMA and the image's
    reads (64 + n_npi), and this is the one test that runs it under the memory pressure of 75 000 chains -- all of which are
    compared with the oracle, not a sample of them (a stale image would be whole 40-chain blocks from one day down)."""
    _headline_sweep_sampled(gpu_device, "auto", False, n=1)


def _headline_sweep_sampled(gpu_device, lane_block, live, n=12):
    import torch
    from epidemicmodeling_amd import batch, synth
    torch.cuda.reset_peak_memory_stats()
    w = synth.make_cfg4(live=live)
    assert (w.B, w.T) == (75000, 520)
    if n < 12:
        w = H.with_npis(w, n)
    idx = np.unique(np.concatenate([np.linspace(0, w.B - 1, 241).astype(np.int64),
                                    [39, 40, 41, 63, 64, 65, 74959, 74960, 74998, 65535, 65536, 249, 250, 251,
                                     40919, 40959, 40960, 40961, 41000]]))   # 40 960: where the two chain ranges of the launches meet
    ref = H.oracle_batch(w.select(idx))
    dw = batch.DeviceWorkload(w, gpu_device)
    r = batch.EkfRunner(dw, extras=True, lane_block=lane_block)
    if n < 12:
        assert r.blk == 40 and w.B % 40 == 0 and r.out["u_opt_smooth"].shape[2] == n
    r.run()
    torch.cuda.synchronize()
    sel = torch.as_tensor(idx, device=gpu_device)
    for k in H.OUT_NAMES:
        got = r.unblocked(k).index_select(-1, sel).cpu().numpy()
        assert np.array_equal(got, ref[k], equal_nan=True), (lane_block, live, n, k)
    assert np.array_equal(r.unblocked("pinv_rank").index_select(-1, sel).cpu().numpy(), ref["pinv_rank"])
    st = r.status.cpu().numpy()
    assert (st & 1).sum() == 0                      # no chain hit the non-finite guard
    if live:
        # what makes this workload "live" (verdict r03 item 1): smoothed i at the end of the history in [1e-6, 1e-1] for
        # EVERY region, cases and R_v positive on >= 90 % of the observed days, two or more waves
        i400 = r.unblocked_at("S_SMOOTH", 399)[1].cpu().numpy().reshape(300, 250)
        assert i400.min() >= 1e-6 and i400.max() <= 1e-1, (i400.min(), i400.max())
        assert (w.x[:400] > 0).mean(axis=0).min() >= 0.9 and (w.R_series[:400] > 0).mean(axis=0).min() >= 0.9
        ti = w.meta["truth"][:, 1]
        mid = np.sqrt(ti[30:].min(axis=0) * ti[30:].max(axis=0))
        waves = ((ti[31:] > mid) & (ti[30:-1] <= mid)).sum(axis=0)
        assert waves.min() >= 2, waves.min()
    # every chain, not the sample: 75 000 of 75 000 (the count is asserted inside)
    tag = "headline lane_block=%s live=%s n_npi=%d" % (lane_block, live, n)
    assert H.all_chains_equal_oracle(r, w, what=tag)["chains"] == 75000
    # the same batch through the one-call sweep entry (what bench.py times): the smoother cut in two, scoring and Pareto
    # filter beside its second launch.  Outputs poisoned first; the sampled chains again, the WHOLE batch against device clones
    # of the outputs verified above, and (J0, J1), front, I_opt against the separate scoring / filter calls on the first run's
    # u_opt_smooth
    _room_for_clones(r, gpu_device)
    saved = H.snapshot_outputs(r)
    rng = np.random.default_rng(4)
    sp, j0p, j1p = _sweep_scoring_inputs(w, rng)
    to = lambda a: torch.as_tensor(a, dtype=torch.float64).to(gpu_device)
    sp_d, j0_d, j1_d = to(sp), to(j0p), to(j1p)
    sc0 = batch.score_sweep(r.out["u_opt_smooth"], 400, sp_d, j0_d, j1_d, B=w.B)
    on0, io0 = batch.pareto_front(sc0["J0"], sc0["J1"], w.Sx)
    J0_0, J1_0 = sc0["J0"].clone(), sc0["J1"].clone()
    for t in r.out.values():
        t.fill_(float("nan"))
    sc1 = r.run_sweep(400, sp_d, j0_d, j1_d, n_regions=w.Sx)
    torch.cuda.synchronize()
    for k in H.OUT_NAMES:
        got = r.unblocked(k).index_select(-1, sel).cpu().numpy()
        assert np.array_equal(got, ref[k], equal_nan=True), (lane_block, n, k, "sweep entry")
    assert torch.equal(sc1["J0"], J0_0) and torch.equal(sc1["J1"], J1_0)
    assert torch.equal(sc1["on_front"].bool(), on0) and torch.equal(sc1["i_opt"], io0)
    assert np.array_equal(r.status.cpu().numpy(), st)
    assert H.device_outputs_equal(r, saved, what=tag + ", sweep entry")["chains"] == 75000
    if lane_block == "auto" and not live and n == 12:
        for k, v in (("J0", float("nan")), ("J1", float("nan")), ("on_front", -1), ("i_opt", -1)):
            sc1[k].fill_(v)
        _back_to_back_and_graph_replay(r, saved, lambda: r.run_sweep(400, sp_d, j0_d, j1_d, n_regions=w.Sx), tag)
        assert torch.equal(sc1["J0"], J0_0) and torch.equal(sc1["J1"], J1_0)        # sc1 holds the views the sweep passes wrote
        assert torch.equal(sc1["on_front"].bool(), on0) and torch.equal(sc1["i_opt"], io0)
    _peak_memory(tag)
    del r, dw, saved
    torch.cuda.empty_cache()


def test_monte_carlo_eks_at_full_size_sampled_chains(gpu_device):
    """BASELINE config 5 at full size (300 regions x 1024 draws x 400 days = 307 200 three-state chains, fp64): sampled
    chains, and then all 307 200 in chain ranges, equal the oracle's run of the same chains alone, bit for bit."""
    import torch
    from epidemicmodeling_amd import batch, synth
    torch.cuda.reset_peak_memory_stats()
    w = synth.make_cfg5(300, 1024, 400)
    assert w.B == 307200
    idx = np.unique(np.concatenate([np.linspace(0, w.B - 1, 200).astype(np.int64), [55, 56, 57, 63, 64, 1023, 1024, 307199]]))
    ref = H.oracle_batch(w.select(idx))
    dw = batch.DeviceWorkload(w, gpu_device)
    r = batch.EkfRunner(dw, extras=True, lane_block="auto")
    r.run()
    torch.cuda.synchronize()
    sel = torch.as_tensor(idx, device=gpu_device)
    for n in H.OUT_NAMES:
        assert np.array_equal(r.unblocked(n).index_select(-1, sel).cpu().numpy(), ref[n], equal_nan=True), n
    assert H.all_chains_equal_oracle(r, w, what="Monte-Carlo EKS fp64")["chains"] == 307200
    _peak_memory("Monte-Carlo EKS fp64")
    del r, dw
    torch.cuda.empty_cache()


def test_batched_host_call_with_matlab_shaped_arrays(gpu_device):
    """What matlab/epiekf_batch_mex.cpp does: B > 1 chains through epi_ekf_run_host with MATLAB (column-major) arrays whose
    FIRST dimension is the chain -- u Su x n_npi x T, x Sx x T, prm B x 61, outputs B x m x T -- no transposition."""
    import ctypes as C
    from epidemicmodeling_amd import _lib, layout as L_, synth
    w = synth.make_cfg4(3, 4, 30, 10)                       # 12 chains sharing 3 series
    B, T, m, n = w.B, w.T, 6, 12
    F = lambda a: np.asfortranarray(a)
    # MATLAB-side arrays (Fortran order), chain index first
    u_m = F(np.transpose(w.u, (2, 1, 0)))                   # Su x n_npi x T
    x_m = F(w.x.T); R_m = F(w.R_series.T)                   # Sx x T
    prm_m = F(w.prm.T)                                      # B x 61
    si, Pi, sf, Pf, Q = (F(a.T) for a in (w.s_init, w.Ps_init, w.s_final, w.Ps_final, w.Q))
    names = ["u_opt", "u_opt_smooth", "S_MINUS", "S_PLUS", "S_SMOOTH", "P_MINUS", "P_PLUS", "P_SMOOTH", "K_GAIN", "innovations", "rho"]
    rows = {"u_opt": n, "u_opt_smooth": n, "S_MINUS": m, "S_PLUS": m, "S_SMOOTH": m, "P_MINUS": m * m, "P_PLUS": m * m,
            "P_SMOOTH": m * m, "K_GAIN": m}
    out = {k: np.zeros((B, rows[k], T), order="F") if k in rows else np.zeros((B, T), order="F") for k in names}
    d = _lib.make_desc(w.model, B, T, w.Sx, w.Su, n, w.L, w.order, w.obs_type, 1, L_.OUT_ALL)
    ins, outs = _lib.Inputs(), _lib.Outputs()
    xs, us = np.ascontiguousarray(w.x_series), np.ascontiguousarray(w.u_series)
    ins.x_series, ins.u_series = xs.ctypes.data, us.ctypes.data
    ins.x, ins.u, ins.R_series, ins.prm = x_m.ctypes.data, u_m.ctypes.data, R_m.ctypes.data, prm_m.ctypes.data
    ins.s_init, ins.Ps_init, ins.s_final, ins.Ps_final, ins.Q = (a.ctypes.data for a in (si, Pi, sf, Pf, Q))
    for k in names:
        setattr(outs, k, out[k].ctypes.data)
    err = C.create_string_buffer(256)
    _lib.check(_lib.lib().epi_ekf_run_host(C.byref(d), C.byref(ins), C.byref(outs), 0, err), err)
    ref = H.oracle_batch(w)
    for k in names:
        got = np.transpose(out[k], (2, 1, 0)) if k in rows else out[k].T          # back to the ABI's [T][rows][B] view
        assert np.array_equal(got, ref[k], equal_nan=True), k
    # chain c of the batched result is what one reference call returns: S_SMOOTH(c, :, :) is m x T
    assert np.array_equal(out["S_SMOOTH"][5], ref["S_SMOOTH"][:, :, 5].T)


def test_nonfinite_initial_covariance_takes_dense_path(gpu_device):
    """Found by tests/test_gpu_fuzz.py: a time-flipped wrapper started from NaN "free end point" markers (its s_final /
    Ps_final ARE the flipped filter's initial condition).  The packed kernels skip structural zeros, which is exact only
    for finite operands, so ekf_precheck sends such a batch to the dense kernels, which mirror the oracle's NaN placement."""
    from epidemicmodeling_amd import batch, synth
    for mk in (lambda: synth.as_backward(synth.make_cfg3(3, 12)), lambda: synth.as_backward(synth.make_cfg4(2, 2, 10, 0))):
        w = mk()
        w.Ps_final = w.Ps_final.copy(); w.s_final = w.s_final.copy()
        w.Ps_final[0, 0] = np.nan; w.Ps_final[1 + w.m * 2, :] = np.nan; w.Ps_final[2 + w.m * 1, :] = np.nan
        w.s_final[1, -1] = np.nan
        got, ref = batch.run_workload(w, device=gpu_device), H.oracle_batch(w)
        for n in H.OUT_NAMES:
            assert np.array_equal(got[n], ref[n], equal_nan=True), (w.model, n)
    w = synth.make_cfg4(2, 3, 20, 5)
    w.Ps_init = w.Ps_init.copy(); w.Ps_init[0, 1] = np.inf
    got, ref = batch.run_workload(w, device=gpu_device), H.oracle_batch(w)
    for n in H.OUT_NAMES:
        assert np.array_equal(got[n], ref[n], equal_nan=True), n


def test_tools_named_simulators_and_npicost(gpu_device):
    """SURVEY.md 8 rows a7-a9 behind the reference's own signatures (tools.SIalpha_Controlled, SEIRP,
    SEIRPSaturatedResource, NPICost) and the batched epi_npi_cost_device: bit for bit against the C oracle; MATLAB's
    index errors for too-short per-step arrays."""
    import ctypes as C
    from epidemicmodeling_amd import batch, synth, tools
    from oracle import oracle_lib as olib
    lib = olib.lib()
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    rng = np.random.default_rng(5)
    n, K = 12, 90
    u = np.asfortranarray(rng.integers(0, 4, size=(n, K)).astype(np.float64))
    a = rng.random(n) * 0.03; um = synth.IP_MAXES.astype(np.float64).copy()
    args = dict(s0=0.999, i0=1e-3, alpha0=1.1, alpha_min=1e-8, alpha_max=100.0, gamma=1 / 7, b=0.01, beta=synth.MODEL_BETA,
                s_std=1e-5, i_std=3e-5, a_std=1e-2, dt=1.0)
    z = rng.standard_normal((3, K))
    for noise in (None, z):
        stds = (0.0, 0.0, 0.0) if noise is None else (args["s_std"], args["i_std"], args["a_std"])
        s, i, al = tools.SIalpha_Controlled(u, args["s0"], args["i0"], args["alpha0"], um, args["alpha_min"], args["alpha_max"],
                                            args["gamma"], a, args["b"], args["beta"], *stds, K, args["dt"], noise=noise,
                                            device=gpu_device)
        assert s.shape == (1, K) and i.shape == (1, K) and al.shape == (1, K)
        rs, ri, ra = np.zeros(K), np.zeros(K), np.zeros(K)
        zc = None if noise is None else np.ascontiguousarray(noise.T)
        lib.orc_sialpha_controlled(dp(u), C.c_int(n), C.c_double(args["s0"]), C.c_double(args["i0"]), C.c_double(args["alpha0"]),
                                   dp(um), C.c_double(args["alpha_min"]), C.c_double(args["alpha_max"]), C.c_double(args["gamma"]),
                                   dp(a), C.c_double(args["b"]), C.c_double(args["beta"]), *[C.c_double(v) for v in stds],
                                   C.c_int(K), C.c_double(args["dt"]), None if zc is None else dp(zc), dp(rs), dp(ri), dp(ra))
        assert np.array_equal(s[0], rs) and np.array_equal(i[0], ri) and np.array_equal(al[0], ra)
    with pytest.raises(IndexError):
        tools.SIalpha_Controlled(u[:, :10], 0.9, 0.1, 1.0, um, 0, 10, 0.1, a, 0, 0.1, 0, 0, 0, K, 1.0, device=gpu_device)
    # NPICost: per-day weights, one weight column, and the batched entry point with shared input series
    wts = np.asfortranarray(rng.random((n, K)))
    nc = np.ascontiguousarray(s[0] * i[0] * al[0])
    J0, J1 = C.c_double(), C.c_double()
    lib.orc_npi_cost(dp(nc), dp(u), dp(wts), C.c_int(n), C.c_int(K), C.byref(J0), C.byref(J1))
    assert tools.NPICost(nc, u, wts, device=gpu_device) == (J0.value, J1.value)
    w1 = np.asfortranarray(np.repeat(wts[:, :1], K, axis=1))
    lib.orc_npi_cost(dp(nc), dp(u), dp(w1), C.c_int(n), C.c_int(K), C.byref(J0), C.byref(J1))
    assert tools.NPICost(nc.reshape(1, K), u, wts[:, :1], device=gpu_device) == (J0.value, J1.value)
    with pytest.raises(ValueError):
        tools.NPICost(nc, u, wts[:, :5], device=gpu_device)
    B, Su = 300, 7
    ub = rng.integers(0, 4, size=(K, n, Su)).astype(np.float64); ser = rng.integers(0, Su, B).astype(np.int32)
    ncb = rng.random((K, B)); wb = rng.random((K, n, B))
    g0, g1 = (t.cpu().numpy() for t in batch.npi_cost(ncb, ub, wb, u_series=ser, device=gpu_device))
    h0, h1 = (t.cpu().numpy() for t in batch.npi_cost(ncb, ub, wb[0], u_series=ser, device=gpu_device))
    for c in (0, 129, B - 1):
        uc = np.asfortranarray(ub[:, :, ser[c]].T); wc = np.asfortranarray(wb[:, :, c].T)
        lib.orc_npi_cost(dp(np.ascontiguousarray(ncb[:, c])), dp(uc), dp(wc), C.c_int(n), C.c_int(K), C.byref(J0), C.byref(J1))
        assert (g0[c], g1[c]) == (J0.value, J1.value)
        wc = np.asfortranarray(np.repeat(wb[0, :, c][:, None], K, axis=1))
        lib.orc_npi_cost(dp(np.ascontiguousarray(ncb[:, c])), dp(uc), dp(wc), C.c_int(n), C.c_int(K), C.byref(J0), C.byref(J1))
        assert (h0[c], h1[c]) == (J0.value, J1.value)
    # SEIRP / SEIRPSaturatedResource (testSEIRP02.m's parameter set), K = round(T/dt)
    T, dt = 36.5, 0.1
    Ks = 365
    par = {k: np.full(Ks, v) * (1 + 0.1 * rng.random(Ks)) for k, v in
           dict(alpha_e=0.6, alpha_i=0.005, kappa=0.05, rho=0.08, beta=0.1, mu=0.02, gamma=0.001).items()}
    init = (1 - 1e-6, 1e-6, 0.0, 0.0, 0.0)
    got = tools.SEIRP(*[par[k] for k in ("alpha_e", "alpha_i", "kappa", "rho", "beta", "mu", "gamma")], *init, T, dt,
                      device=gpu_device)
    ref = [np.zeros(Ks) for _ in range(5)]
    lib.orc_seirp(*[dp(par[k]) for k in ("alpha_e", "alpha_i", "kappa", "rho", "beta", "mu", "gamma")],
                  *[C.c_double(v) for v in init], C.c_int(Ks), C.c_double(dt), *[dp(v) for v in ref])
    for q in range(5):
        assert got[q].shape == (1, Ks) and np.array_equal(got[q][0], ref[q]), q
    assert got[0][0, 0] == init[0] and abs(sum(g[0, -1] for g in got) - 1.0) < 1e-12     # mass conservation (KAT vi)
    sat = (0.1, 0.02, 0.02, 0.08, 0.01, 0.05)
    got = tools.SEIRPSaturatedResource(*[par[k] for k in ("alpha_e", "alpha_i", "kappa", "rho", "gamma")], *init, T, dt, *sat,
                                       device=gpu_device)
    ref = [np.zeros(Ks) for _ in range(5)]
    lib.orc_seirp_saturated(*[dp(par[k]) for k in ("alpha_e", "alpha_i", "kappa", "rho", "gamma")],
                            *[C.c_double(v) for v in init], C.c_int(Ks), C.c_double(dt), *[C.c_double(v) for v in sat],
                            *[dp(v) for v in ref])
    for q in range(5):
        assert np.array_equal(got[q][0], ref[q]), q
    with pytest.raises(IndexError):
        tools.SEIRP(0.6, 0.005, 0.05, 0.08, 0.1, 0.02, 0.001, *init, T, dt, device=gpu_device)   # scalars: alpha_e(2) fails


def test_si_controlled_parity(gpu_device):
    """Tools/SI_Controlled.m (the 2-state clamped SI model; here with testSIR01.m's alpha, beta, N, dt and K, but it is NOT
    that script's model -- BASELINE config 1 is the 3-compartment SIR, test_sir_config1_parity below) behind its own
    signature and batched with shared infection-rate series: bit for bit against the C oracle."""
    import ctypes as C
    from epidemicmodeling_amd import batch, tools
    from oracle import oracle_lib as olib
    lib = olib.lib()
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    K, dt, N = 1500, 0.1, 84e6
    alpha = np.full(K, 0.5)
    s, i = tools.SI_Controlled(alpha, 0.05, (N - 1) / N, 1 / N, K, dt, device=gpu_device)
    rs, ri = np.zeros(K), np.zeros(K)
    lib.orc_si_controlled(dp(alpha), C.c_double(0.05), C.c_double((N - 1) / N), C.c_double(1 / N), C.c_int(K), C.c_double(dt),
                          dp(rs), dp(ri))
    assert s.shape == (1, K) and np.array_equal(s[0], rs) and np.array_equal(i[0], ri)
    assert s[0, 0] == (N - 1) / N and 0.0 < i[0].max() <= 1.0 and s[0, -1] < 0.01        # the epidemic runs its course
    with pytest.raises(IndexError):
        tools.SI_Controlled(alpha[:100], 0.05, 0.9, 0.1, K, dt, device=gpu_device)
    rng = np.random.default_rng(9)
    B, Sa, Kb = 257, 5, 300
    al = rng.uniform(0.0, 2.0, (Kb - 1, Sa)); ser = rng.integers(0, Sa, B).astype(np.int32)
    beta = rng.uniform(0.01, 0.3, B); s0 = rng.uniform(0.5, 1.0, B); i0 = 1 - s0
    gs, gi = (t.cpu().numpy() for t in batch.si_controlled(al, beta, s0, i0, Kb, 0.5, alpha_series=ser, device=gpu_device))
    for c in (0, 100, B - 1):
        rs, ri = np.zeros(Kb), np.zeros(Kb)
        lib.orc_si_controlled(dp(np.ascontiguousarray(al[:, ser[c]])), C.c_double(beta[c]), C.c_double(s0[c]), C.c_double(i0[c]),
                              C.c_int(Kb), C.c_double(0.5), dp(rs), dp(ri))
        assert np.array_equal(gs[:, c], rs) and np.array_equal(gi[:, c], ri)


def test_sir_config1_parity(gpu_device):
    """BASELINE config 1 (testScripts/testSIR01.m:15-36: 3-compartment SIR with return flow, 1500 Euler samples; "CPU
    plumbing" in BASELINE's own words, so one chain is all the reference runs): the kernel reproduces the oracle bit for
    bit for the script's parameter set and for a batch of 1 000 random ones."""
    from epidemicmodeling_amd import hostapi
    from oracle import oracle_lib as olib
    N, K, dt = 84.0e6, 1500, 0.1
    s, i, r = hostapi.sir(0.5, 0.05, 0.04, (N - 1) / N, 1 / N, 0.0, K, dt)
    rs, ri, rr = olib.sir(0.5, 0.05, 0.04, (N - 1) / N, 1 / N, 0.0, K, dt)
    assert s.shape == (K, 1) and np.array_equal(s[:, 0], rs) and np.array_equal(i[:, 0], ri) and np.array_equal(r[:, 0], rr)
    rng = np.random.default_rng(1)
    B = 1000
    al, be, ga = rng.uniform(0.1, 1.0, B), rng.uniform(0.01, 0.2, B), rng.uniform(0.0, 0.1, B)
    i0 = rng.uniform(1e-8, 1e-3, B)
    gs, gi, gr = hostapi.sir(al, be, ga, 1.0 - i0, i0, 0.0, 400, 0.25)
    for c in (0, 1, 499, B - 1):
        rs, ri, rr = olib.sir(al[c], be[c], ga[c], 1.0 - i0[c], i0[c], 0.0, 400, 0.25)
        assert np.array_equal(gs[:, c], rs) and np.array_equal(gi[:, c], ri) and np.array_equal(gr[:, c], rr)
    assert np.abs(gs + gi + gr - 1.0).max() < 1e-12


def test_bench_contract_single_and_two_ranks(gpu_device, tmp_path):
    """bench.py end to end on a small sweep: the one JSON line of a plain run carries the headline fields and nothing that
    takes work of its own; with --full it carries every field of the driver's contract (metric, value, roofline,
    cpu_baseline ...); --dump-outputs writes the last timed pass's outputs, the same from run to run; and the N = 2 path
    (barriers, max-over-ranks timing, end-of-sweep gather to rank 0) runs as two processes sharing the one GPU with the
    gloo rehearsal backend."""
    import json
    import os
    import subprocess
    import sys
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    small = ["--regions", "6", "--eps", "40", "--t-hist", "60", "--horizon", "20", "--steps", "2", "--warmup", "1"]
    r0 = subprocess.run([sys.executable, os.path.join(H.ROOT, "bench.py"), *small, "--dump-outputs", str(tmp_path / "plain")],
                        capture_output=True, text=True, timeout=600, env=env, cwd=H.ROOT)
    assert r0.returncode == 0, r0.stderr[-2000:]
    line = [l for l in r0.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1
    d0 = json.loads(line[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "dtype", "config"):
        assert k in d0, k
    for k in ("roofline", "kernels", "cpu_baseline", "box_normalised"):
        assert k not in d0, k
    assert d0["steps"] == 2 and d0["higher_is_better"] is True and d0["dtype"] == "f64" and d0["unit"] == "region-day EKF steps/s"
    assert abs(d0["value"] - 6 * 40 * 80 * 2 / (d0["ms_per_step"] * 2e-3)) <= 1e-6 * d0["value"]
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "bench.py"), *small, "--full", "--cpu-sample-chains", "32",
                        "--dump-outputs", str(tmp_path / "full")],
                       capture_output=True, text=True, timeout=600, env=env, cwd=H.ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1
    d = json.loads(line[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "strong" and d["dtype"] == "f64"
    assert d["vs_baseline"] is None and d["higher_is_better"] is True and "workload" in d["config"]
    assert d["value"] > 0 and abs(d["value"] - 6 * 40 * 80 * 2 / (d["ms_per_step"] * 2e-3)) <= 1e-6 * d["value"]
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb
    # --dump-outputs: all 11 outputs of the 240 chains, [T, rows, B] in float64, the per-chain scores and the per-region front,
    # identical in two runs of the same arguments; what the oracle computes for the same chains
    from epidemicmodeling_amd import batch, synth
    names = sorted(p.name for p in (tmp_path / "plain").iterdir())
    assert names == sorted(n + ".npy" for n in list(batch.OUT_NAMES) + ["J0", "J1", "on_front", "i_opt"]), names
    assert sorted(p.name for p in (tmp_path / "full").iterdir()) == names
    w = synth.make_cfg4(6, 40, 60, 20)
    ref = H.oracle_batch(w)
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)
        assert a.dtype == np.float64 and np.array_equal(a, b, equal_nan=True), n
        total += a.nbytes
        if n[:-4] in ("S_MINUS", "S_PLUS", "P_PLUS", "K_GAIN", "innovations", "rho", "u_opt", "S_SMOOTH", "u_opt_smooth"):
            assert H.rel_err(a, ref[n[:-4]]) <= 1e-9, n
    assert np.load(tmp_path / "plain" / "J0.npy").shape == (240,) and np.load(tmp_path / "plain" / "on_front.npy").shape == (6, 40)
    assert total <= 64 << 20
    env2 = dict(env, EPI_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    r2 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                         "127.0.0.1", "--master-port", "29731", os.path.join(H.ROOT, "bench.py"), "--gpus", "2", *small],
                        capture_output=True, text=True, timeout=600, env=env2, cwd=H.ROOT)
    assert r2.returncode == 0, r2.stderr[-2000:]
    line = [l for l in r2.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1                                   # rank 0 alone prints
    d2 = json.loads(line[0])
    # default = strong scaling: the SAME 240-chain sweep, 120 chains per rank; value is the whole job's rate
    assert d2["n_gpus"] == 2 and "cpu_baseline" not in d2 and d2["scaling"] == "strong"
    assert d2["config"]["chains_per_gpu"] == 120 and d2["config"]["sweep_chains_total"] == 240
    # round 4: the N > 1 line can be decomposed -- every rank's own ms per pass, the end-of-sweep gather alone, the ranks
    rk = d2["ranks"]
    assert rk["rccl_ranks"] == 2 and len(rk["ms_per_step_by_rank"]) == 2 and len(rk["gather_ms_hip_events_by_rank"]) == 2
    assert 0 < rk["ms_per_step_min"] <= rk["ms_per_step_max"] <= d2["ms_per_step"] * 1.0001 + 1e-9
    assert all(g >= 0 for g in rk["gather_ms_host_clock_by_rank"]) and rk["backend"] in ("gloo", "nccl")
    assert "ranks" not in d
    assert abs(d2["value"] - 6 * 40 * 80 * 2 / (d2["ms_per_step"] * 2e-3)) <= 1e-6 * d2["value"]
    r3 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                         "127.0.0.1", "--master-port", "29732", os.path.join(H.ROOT, "bench.py"), "--gpus", "2", "--scaling", "weak", *small],
                        capture_output=True, text=True, timeout=600, env=env2, cwd=H.ROOT)
    assert r3.returncode == 0, r3.stderr[-2000:]
    d3 = json.loads([l for l in r3.stdout.splitlines() if l.startswith("{")][0])
    assert d3["scaling"] == "weak" and d3["config"]["chains_per_gpu"] == 240
    assert abs(d3["value"] - 2 * 6 * 40 * 80 * 2 / (d3["ms_per_step"] * 2e-3)) <= 1e-6 * d3["value"]   # whole-job aggregate
    # started BARE, the way the driver starts it (`python bench.py --gpus N`, no WORLD_SIZE): bench.py launches its own
    # ranks as child processes before it touches a GPU, relays rank 0's line and returns their exit code
    env4 = {k: v for k, v in env2.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r4 = subprocess.run([sys.executable, os.path.join(H.ROOT, "bench.py"), "--gpus", "2", *small],
                        capture_output=True, text=True, timeout=600, env=env4, cwd=H.ROOT)
    assert r4.returncode == 0, r4.stderr[-2000:]
    line = [l for l in r4.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1
    d4 = json.loads(line[0])
    assert d4["n_gpus"] == 2 and d4["scaling"] == "strong" and d4["config"]["chains_per_gpu"] == 120
    # ... and a failing rank makes the bare call fail (cfg3 does not shard: every rank exits non-zero)
    r5 = subprocess.run([sys.executable, os.path.join(H.ROOT, "bench.py"), "--gpus", "2", "--workload", "cfg3", *small],
                        capture_output=True, text=True, timeout=600, env=env4, cwd=H.ROOT)
    assert r5.returncode != 0 and not [l for l in r5.stdout.splitlines() if l.startswith("{")]


def test_newcase_sweep_at_full_size_sampled_chains(gpu_device):
    """BASELINE's "NewCaseEKFEstimatorWithOptimalNPI: 300 regions x 250 NPI-cost weights x 120-day horizon" at full size
    (75 000 dense-kernel chains x 520 days, mrdivide smoother): every sampled chain of the big batch equals the oracle's run
    of that chain alone, bit for bit (first, last, wave and layout-block boundaries included), and then every chain of all 75 000
    does (the outputs the reference has; its mrdivide smoother has no pinv ranks)."""
    import torch
    from epidemicmodeling_amd import batch, synth
    torch.cuda.reset_peak_memory_stats()
    w = synth.make_newcase_sweep()
    assert (w.B, w.T) == (75000, 520)
    idx = np.unique(np.concatenate([np.linspace(0, w.B - 1, 121).astype(np.int64),
                                    [39, 40, 41, 63, 64, 65, 74959, 74960, 74998, 65535, 65536, 249, 250, 251]]))
    ref = H.oracle_batch(w.select(idx))
    dw = batch.DeviceWorkload(w, gpu_device)
    r = batch.EkfRunner(dw, extras=True, lane_block="auto")
    r.run()
    torch.cuda.synchronize()
    sel = torch.as_tensor(idx, device=gpu_device)
    names = [n for n in H.OUT_NAMES if n in r.out and n in ref]
    assert "S_SMOOTH" in names and "P_SMOOTH" in names and "u_opt" in names
    for n in names:
        got = r.unblocked(n).index_select(-1, sel).cpu().numpy()
        assert np.array_equal(got, ref[n], equal_nan=True), n
    assert H.all_chains_equal_oracle(r, w, names=names, what="NewCase sweep")["chains"] == 75000
    _peak_memory("NewCase sweep")
    del r, dw
    torch.cuda.empty_cache()


def _hip_vs_lapack_sweep_report(gpu_device, t_hist, horizon, pool, live=False):
    """HIP output and LAPACK reading of 10 regions x 250 cost weights of the sweep with `t_hist` observed and `horizon`
    free days; returns (per-decade parity report, front report, worst gated errors, worst J0 difference of the chains in
    which no control flipped)."""
    import json
    import torch
    from epidemicmodeling_amd import batch, layout as L_, synth
    regions = (0, 11, 29, 57, 88, 120, 157, 199, 230, 281)
    full = synth.make_cfg4(300, 250, t_hist, horizon, live=live)
    E, T = 250, full.T
    idx = np.concatenate([np.arange(r * E, (r + 1) * E) for r in regions])
    w = full.select(idx)
    eps = w.prm[H.L.PRM_EPSILON]
    got = _run(w, gpu_device)
    jobs = [(w, np.arange(c0, min(c0 + 25, w.B))) for c0 in range(0, w.B, 25)]
    res = [r for chunk in pool.map(lapack_worker_entry, jobs) for r in chunk]
    hist = int(np.sum(~np.isnan(w.x[:, 0])))
    dec = np.floor(np.log10(eps)).astype(int)
    rows = {}
    worst = {"S_PLUS": 0.0, "new_cases_filtered": 0.0, "new_cases_predicted": 0.0}
    worst_smooth = 0.0
    flips_of_chain = np.zeros(w.B, dtype=np.int64)
    for c, nd in enumerate(res):
        g = {n: H.batch_chain(got, n, c, 6) for n in ("S_MINUS", "S_PLUS", "S_SMOOTH", "u_opt_smooth")}
        e_sp = H.rowwise_abs_rel_err(g["S_PLUS"][:3], nd["S_PLUS"][:3])
        nc = lambda S: S[0] * S[1] * S[2]
        e_ncf = H.rel_err(nc(g["S_PLUS"]), nc(nd["S_PLUS"]))
        e_ncp = H.rel_err(nc(g["S_MINUS"]), nc(nd["S_MINUS"]))
        worst["S_PLUS"] = max(worst["S_PLUS"], e_sp)
        worst["new_cases_filtered"] = max(worst["new_cases_filtered"], e_ncf)
        worst["new_cases_predicted"] = max(worst["new_cases_predicted"], e_ncp)
        r = rows.setdefault(int(dec[c]), {"chains": 0, "S_SMOOTH_1to3": 0.0, "S_SMOOTH_costates": 0.0, "rank_mismatch_steps": 0,
                                          "u_opt_smooth_entries": 0, "u_opt_smooth_flips": 0, "worst_chain_flip_rate": 0.0})
        r["chains"] += 1
        r["S_SMOOTH_1to3"] = max(r["S_SMOOTH_1to3"], H.rowwise_abs_rel_err(g["S_SMOOTH"][:3], nd["S_SMOOTH"][:3]))
        worst_smooth = max(worst_smooth, H.rowwise_abs_rel_err(g["S_SMOOTH"][:3], nd["S_SMOOTH"][:3]))
        r["S_SMOOTH_costates"] = max(r["S_SMOOTH_costates"], H.rowwise_abs_rel_err(g["S_SMOOTH"][3:], nd["S_SMOOTH"][3:]))
        r["rank_mismatch_steps"] += int(np.sum(got["pinv_rank"][:, c] != nd["pinv_rank"]))
        ug, un = g["u_opt_smooth"][:, hist:T - 1], nd["u_opt_smooth"][:, hist:T - 1]      # the free (NaN) controls
        flips = int(np.sum(ug != un))
        flips_of_chain[c] = flips
        r["u_opt_smooth_entries"] += ug.size
        r["u_opt_smooth_flips"] += flips
        r["worst_chain_flip_rate"] = max(r["worst_chain_flip_rate"], flips / ug.size)
    for r in rows.values():
        r["flip_rate"] = r["u_opt_smooth_flips"] / max(1, r["u_opt_smooth_entries"])
    report = {"what": "HIP kernels (libepiekf.so) vs oracle/ekf_numpy.py (NumPy, LAPACK SVD pinv)",
              "workload": f"{'cfg4-live' if live else 'cfg4'} regions {list(regions)} x 250 epsilon x {T} days ({w.B} chains)",
              "gated_at_1e-6": worst, "reported_S_SMOOTH_1to3_max": worst_smooth, "reported_per_epsilon_decade": {str(k): rows[k] for k in sorted(rows)},
              "total_flip_rate": sum(r["u_opt_smooth_flips"] for r in rows.values()) / sum(r["u_opt_smooth_entries"] for r in rows.values()),
              "total_rank_mismatch_steps": sum(r["rank_mismatch_steps"] for r in rows.values())}
    # ---- both plans through the scoring tail and the front filter ----
    n, B = 12, w.B
    S = got["S_SMOOTH"]
    sp = np.zeros((batch.SIM_PRM_COUNT, B))
    sp[0:3] = S[hist - 1, 0:3]                                    # end-of-history state (the same for both plans)
    sp[3], sp[4], sp[5] = w.prm[L_.PRM_ALPHA_MIN], w.prm[L_.PRM_ALPHA_MAX], w.prm[L_.PRM_GAMMA]
    sp[6], sp[7], sp[11] = w.prm[L_.PRM_B], w.prm[L_.PRM_BETA], 1.0
    sp[batch.SIM_A:batch.SIM_A + n] = w.prm[L_.PRM_A:L_.PRM_A + n]
    sp[batch.SIM_U_MAX:batch.SIM_U_MAX + n] = w.prm[L_.PRM_U_MAX:L_.PRM_U_MAX + n]
    sp[batch.SIM_W:batch.SIM_W + n] = 1.0                         # npi_weights = ones (testPrescribeXPRIZE02.m:56)
    J0p = np.cumsum(S[:hist, 0] * S[:hist, 1] * S[:hist, 2], axis=0)[-1]
    J1p = np.cumsum(got["u_opt_smooth"][:hist].reshape(hist * n, B), axis=0)[-1]
    u_lap = np.stack([nd["u_opt_smooth"] for nd in res], axis=-1)               # [n, T, B]
    u_lap = np.ascontiguousarray(np.transpose(u_lap, (1, 0, 2)))                # [T, n, B]
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(gpu_device)
    out = {}
    for tag, U in (("hip", got["u_opt_smooth"]), ("lapack", u_lap)):
        sc = batch.score_sweep(to(U), hist, to(sp), to(J0p), to(J1p))
        on, io = batch.pareto_front(sc["J0"], sc["J1"], len(regions))
        out[tag] = {"J0": sc["J0"].cpu().numpy().reshape(len(regions), E), "J1": sc["J1"].cpu().numpy().reshape(len(regions), E),
                    "on": on.cpu().numpy(), "io": io.cpu().numpy()}
    fl = flips_of_chain.reshape(len(regions), E)
    rel = lambda a, b: np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    per_region, worst_unflipped = {}, 0.0
    for k, r in enumerate(regions):
        d0, d1 = rel(out["hip"]["J0"][k], out["lapack"]["J0"][k]), rel(out["hip"]["J1"][k], out["lapack"]["J1"][k])
        clean = fl[k] == 0
        wu = float(d0[clean].max()) if clean.any() else 0.0
        worst_unflipped = max(worst_unflipped, wu)
        j0 = out["hip"]["J0"][k]
        per_region[str(r)] = {"chains_with_a_flipped_control": int((~clean).sum()), "flipped_entries": int(fl[k].sum()),
                              # how much of the objective the plan can move at all: the infected share the horizon starts from
                              # and the horizon's share of J0 (a region whose epidemic has died out by the end of the history
                              # has a degenerate objective: every plan gives the same J0 and the control is decided by rounding)
                              "i_at_end_of_history_min_max": [float(sp[1, k * E:(k + 1) * E].min()), float(sp[1, k * E:(k + 1) * E].max())],
                              "horizon_share_of_J0_max": float(np.max((j0 * T - J0p[k * E:(k + 1) * E]) / np.maximum(j0 * T, 1e-300))),
                              "J0_max_rel_diff": float(d0.max()), "J1_max_rel_diff": float(d1.max()),
                              "J0_max_rel_diff_where_no_control_flipped": wu,
                              "on_front_hip": int(out["hip"]["on"][k].sum()), "on_front_lapack": int(out["lapack"]["on"][k].sum()),
                              "on_front_flag_differs": int((out["hip"]["on"][k] != out["lapack"]["on"][k]).sum()),
                              "I_opt_hip": int(out["hip"]["io"][k]), "I_opt_lapack": int(out["lapack"]["io"][k]),
                              "I_opt_same": bool(out["hip"]["io"][k] == out["lapack"]["io"][k]),
                              "prescribed_plan_identical": bool(np.array_equal(got["u_opt_smooth"][hist:, :, k * E + out["hip"]["io"][k]],
                                                                               u_lap[hist:, :, k * E + out["lapack"]["io"][k]]))}
    front = {"what": "u_opt_smooth of the HIP kernels and of the LAPACK-SVD reading pushed through the same scoring tail "
                     "(SIalpha_Controlled + NPICost over [historic, horizon]) and Pareto filter, TrainPredictPrescribeNPI.m:481-493, 624-633",
             "workload": report["workload"], "gate": "J0 within 1e-6 relative for every chain in which no control flipped",
             "J0_max_rel_diff_where_no_control_flipped": worst_unflipped,
             "regions_with_the_same_I_opt": int(sum(v["I_opt_same"] for v in per_region.values())),
             "regions_with_the_identical_prescribed_plan": int(sum(v["prescribed_plan_identical"] for v in per_region.values())),
             "on_front_flags_differing": int(sum(v["on_front_flag_differs"] for v in per_region.values())),
             "points": int(len(regions) * E), "per_region": per_region}
    return report, front, worst, worst_unflipped


def test_hip_vs_lapack_reading_on_the_headline_epsilon_grid(gpu_device):
    """HIP output against oracle/ekf_numpy.py (LAPACK SVD pinv -- the stand-in for MATLAB's own pinv) on the headline
    workload's full epsilon grid at full T: 10 regions x all 250 cost weights x 520 days.  GATED at the north-star
    tolerance (1e-6 relative) on the filtered states and the predicted new cases; REPORTED, per epsilon decade, for what
    no two SVD implementations can promise on covariances with cond 1e30-1e60: smoothed epidemic states, smoothed
    costates, pinv truncation ranks and the flip rate of the bang-bang u_opt_smooth (gpurun_out/parity_vs_lapack.json).

    And where the user feels it (TrainPredictPrescribeNPI.m:481-493, 624-633): BOTH u_opt_smooth -- the kernels' and the
    LAPACK reading's -- go through the same scoring tail and Pareto filter.  Per region: the largest relative difference of
    (J0, J1), the number of points whose on-front flag differs, whether I_opt (the prescribed cost weight) is the same.
    GATED: J0 (the mean predicted new cases) within 1e-6 for every chain in which no control flipped.  The headline
    workload's synthetic epidemic has died out by day 400 (smoothed i = 0 at the end of the history), so there no plan can
    move J0 and the bang-bang control of the regions concerned is decided by rounding; the same report is therefore also made
    for the sweep cut after 60 observed days, when every region's epidemic is alive.  gpurun_out/front_vs_lapack.json
    (committed copies of both reports under profiles/r03/)."""
    import json
    import multiprocessing as mp
    import os
    with mp.get_context("spawn").Pool(min(16, os.cpu_count() or 1)) as pool:
        report, front, worst, wu = _hip_vs_lapack_sweep_report(gpu_device, 400, 120, pool)
        report2, front2, worst2, wu2 = _hip_vs_lapack_sweep_report(gpu_device, 60, 120, pool)
    os.makedirs(os.path.join(H.ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(H.ROOT, "gpurun_out", "parity_vs_lapack.json"), "w") as f:
        json.dump({"headline_400_plus_120_days": report, "live_epidemic_60_plus_120_days": report2}, f, indent=1)
    with open(os.path.join(H.ROOT, "gpurun_out", "front_vs_lapack.json"), "w") as f:
        json.dump({"headline_400_plus_120_days": front, "live_epidemic_60_plus_120_days": front2}, f, indent=1)
    for fr in (front, front2):
        print(json.dumps({k: fr[k] for k in fr if k != "per_region"}))
    for w_ in (worst, worst2):
        assert w_["S_PLUS"] <= NORTH_STAR_TOL and w_["new_cases_filtered"] <= NORTH_STAR_TOL and w_["new_cases_predicted"] <= NORTH_STAR_TOL, w_
    assert wu <= NORTH_STAR_TOL and wu2 <= NORTH_STAR_TOL, (wu, wu2)


def lapack_worker_entry(job):
    return H.lapack_reading_worker(job)


def test_hip_vs_lapack_reading_on_the_live_sweep(gpu_device):
    """The same HIP-vs-LAPACK report on the LIVING epidemic (synth.make_cfg4(live=True): every region's smoothed i(400) in
    [1e-6, 1e-1], cases on >= 90 % of the days, 5-8 waves), 10 regions x 250 cost weights, at 400 + 120 and at 60 + 120
    days.  Reports: gpurun_out/parity_vs_lapack_live.json, gpurun_out/front_vs_lapack_live.json.

    GATED at 1e-6 on both: filtered states, filtered / predicted new cases, and J0 of every chain in which no control
    flipped.  The SMOOTHED epidemic states are reported here and gated against the exact evaluation instead
    (test_hip_against_frozen_referee_and_lapack_vectors): there the kernels stand at 1e-13 ... 1e-11 and the LAPACK
    reading at 3e-9 (400 + 120) and 3e-5 (60 + 120, up to 3e-2 over all 2 500 chains at the few steps where its SVD keeps
    another rank) -- profiles/r04/referee_report.json -- so a gate against the LAPACK reading would measure ITS error.
    GATED on the 60 + 120-day sweep, where the smoother is well conditioned: no control differs, and front, I_opt and the
    prescribed plan are identical in every region.
    REPORTED on the 400 + 120-day sweep: control flips, front flags, I_opt.  There the verdict of round 3 asked for
    identity wherever the horizon's share of J0 exceeds 1 %; the referee shows why that cannot be had from ANY fp64
    implementation, MATLAB's included: the forward-propagated costates reach 1e12 and the smoother must cancel them to
    recover values of order 1e-3, so in fp64 the smoothed costates are rounding noise 1e13 times larger than the exact
    values and the sign of phi = eps w - gamma lambda3 a follows that noise.  Measured against the exact plan on 20
    chains: the kernels differ in 717 of 28 560 free controls, the LAPACK reading in 1 287 (tests/golden/ref_cfg4_live_400_120.npz,
    gated in test_hip_against_frozen_referee_and_lapack_vectors).  Two fp64 readings that are both wrong cannot be
    required to be wrong in the same way."""
    import json
    import multiprocessing as mp
    import os
    with mp.get_context("spawn").Pool(min(16, os.cpu_count() or 1)) as pool:
        report, front, worst, wu = _hip_vs_lapack_sweep_report(gpu_device, 400, 120, pool, live=True)
        report2, front2, worst2, wu2 = _hip_vs_lapack_sweep_report(gpu_device, 60, 120, pool, live=True)
    os.makedirs(os.path.join(H.ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(H.ROOT, "gpurun_out", "parity_vs_lapack_live.json"), "w") as f:
        json.dump({"live_400_plus_120_days": report, "live_60_plus_120_days": report2}, f, indent=1)
    with open(os.path.join(H.ROOT, "gpurun_out", "front_vs_lapack_live.json"), "w") as f:
        json.dump({"live_400_plus_120_days": front, "live_60_plus_120_days": front2}, f, indent=1)
    for fr in (front, front2):
        print(json.dumps({k: fr[k] for k in fr if k != "per_region"}))
    for w_ in (worst, worst2):
        assert max(w_.values()) <= NORTH_STAR_TOL, w_
    assert wu <= NORTH_STAR_TOL and wu2 <= NORTH_STAR_TOL, (wu, wu2)
    # every region of the live workload has something to steer: the horizon carries more than 1 % of J0
    for fr in (front, front2):
        assert min(v["horizon_share_of_J0_max"] for v in fr["per_region"].values()) > 0.01, fr["per_region"]
    assert report2["total_flip_rate"] == 0.0 and front2["on_front_flags_differing"] == 0, (report2["total_flip_rate"], front2)
    assert front2["regions_with_the_same_I_opt"] == 10 and front2["regions_with_the_identical_prescribed_plan"] == 10, front2


def test_hip_against_frozen_referee_and_lapack_vectors(gpu_device):
    """HIP output against tests/golden/ref_*.npz: the reference's formulas in 160-digit arithmetic (oracle/referee_mp.py)
    and the LAPACK reading, both frozen -- vectors that do not move when the kernels' or the C oracle's algorithm does.
    Same gates as tests/test_referee.py applies to the C oracle (tests.helpers.referee_compare); both lane mappings where
    the model has them.  Report: gpurun_out/hip_vs_referee.json."""
    import json
    import os
    rep, fails = {}, []
    for name in H.REFEREE_CASES:
        w, fx = H.load_referee(name)
        shapes = (1, 2, 3) if w.model == "SIAlphaModelEKFOptControlled" or w.model == "SIAlphaModelBackwardEKFOptControlled" else (0,)
        for shape in shapes:
            got = _run(w, gpu_device, shape=shape)
            f, r = H.referee_compare(w, got, fx, f"{name}/shape{shape}")
            fails += f
            rep[f"{name}/shape{shape}"] = r
    os.makedirs(os.path.join(H.ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(H.ROOT, "gpurun_out", "hip_vs_referee.json"), "w") as f:
        json.dump(rep, f, indent=1)
    assert not fails, fails


def test_hip_vs_lapack_reading_on_the_other_baseline_configs(gpu_device):
    """The same independent reading (NumPy, LAPACK SVD `pinv` / LU `mrdivide`) against the HIP output for every other
    configuration BASELINE.json names and every model of the path: config 3 at full size (SIAlphaModelEKF, 300 regions x 400
    days), config 5 (Monte-Carlo EKS, sampled chains), the NewCaseEKFEstimatorWithOptimalNPI sweep (sampled), both
    time-flipped wrappers and the adaptive-R case.  GATED at 1e-6 relative on the filtered states and the filtered /
    predicted new cases (north star); smoothed quantities and ranks are reported.  The time-flipped wrappers run the
    epidemic map backwards, which is unstable: there the reading is also run with every observation moved by ONE ulp, and
    the gate is 1e-6 or ten times what that one ulp does to the reading's own output, whichever is larger (both numbers
    are in the report).  Report: gpurun_out/parity_vs_lapack_other_configs.json (committed copy under profiles/r02/)."""
    import json
    import multiprocessing as mp
    import os
    from epidemicmodeling_amd import synth
    nc_full = synth.make_newcase_sweep()
    cfg5 = synth.make_cfg5(300, 4, 400)
    cases = [("cfg3: SIAlphaModelEKF, 300 regions x 400 days (all chains)", synth.make_cfg3(300, 400)),
             ("cfg5: 3-state MC-EKS, 120 chains sampled from 300 regions x 4 draws x 400 days",
              cfg5.select(np.linspace(0, cfg5.B - 1, 120).astype(np.int64))),
             ("NewCaseEKFEstimatorWithOptimalNPI sweep, regions 0 / 11 / 157 x 10 cost weights x 520 days",
              nc_full.select(np.concatenate([r * 250 + np.linspace(0, 249, 10).astype(np.int64) for r in (0, 11, 157)]))),
             ("SIAlphaModelBackwardEKF, 60 regions x 200 days", synth.as_backward(synth.make_cfg3(60, 200))),
             ("SIAlphaModelBackwardEKF, 60 regions x 120 days (plain 1e-6 gate)", synth.as_backward(synth.make_cfg3(60, 120))),
             ("SIAlphaModelBackwardEKFOptControlled, 6 regions x 10 cost weights x 40 days", synth.as_backward(synth.make_cfg4(6, 10, 30, 10))),
             ("SIAlphaModelEKFOptControlled, adaptive scalar R (beta = 0.9), 4 regions x 6 cost weights x 150 days", synth.make_row3(4, 6, 30, 120))]
    report, failed = {}, []
    with mp.get_context("spawn").Pool(min(8, os.cpu_count() or 1)) as pool:
        for name, w in cases:
            got = _run(w, gpu_device)
            flipped = "Backward" in w.model
            jobs = [(w, np.arange(c0, min(c0 + 8, w.B)), flipped) for c0 in range(0, w.B, 8)]
            res = [r for chunk in pool.map(lapack_worker_entry, jobs) for r in chunk]
            m = w.m
            nc = lambda S: S[0] * S[1] * S[2]
            row = {"chains": w.B, "days": w.T, "S_PLUS_1to3": 0.0, "new_cases_filtered": 0.0, "new_cases_predicted": 0.0,
                   "S_SMOOTH_1to3": 0.0, "rank_mismatch_steps": 0, "u_opt_smooth_flips": 0, "u_opt_smooth_entries": 0}
            for c, nd in enumerate(res):
                g = {n: H.batch_chain(got, n, c, m) for n in ("S_MINUS", "S_PLUS", "S_SMOOTH")}
                row["S_PLUS_1to3"] = max(row["S_PLUS_1to3"], H.rowwise_abs_rel_err(g["S_PLUS"][:3], nd["S_PLUS"][:3]))
                row["new_cases_filtered"] = max(row["new_cases_filtered"], H.rel_err(nc(g["S_PLUS"]), nc(nd["S_PLUS"])))
                row["new_cases_predicted"] = max(row["new_cases_predicted"], H.rel_err(nc(g["S_MINUS"]), nc(nd["S_MINUS"])))
                row["S_SMOOTH_1to3"] = max(row["S_SMOOTH_1to3"], H.rowwise_abs_rel_err(g["S_SMOOTH"][:3], nd["S_SMOOTH"][:3]))
                if flipped:
                    sens = max(H.rowwise_abs_rel_err(nd["S_PLUS_1ulp"][:3], nd["S_PLUS"][:3]),
                               H.rel_err(nc(nd["S_PLUS_1ulp"]), nc(nd["S_PLUS"])), H.rel_err(nc(nd["S_MINUS_1ulp"]), nc(nd["S_MINUS"])))
                    row["reading_moved_by_one_ulp_of_x"] = max(row.get("reading_moved_by_one_ulp_of_x", 0.0), sens)
                if "pinv_rank" in nd:
                    row["rank_mismatch_steps"] += int(np.sum(got["pinv_rank"][:, c] != nd["pinv_rank"]))
                if "u_opt_smooth" in nd and m == 6:
                    ug, un = H.batch_chain(got, "u_opt_smooth", c, m), nd["u_opt_smooth"]
                    free = np.isnan(w.u[:, :, int(w.u_series[c]) if w.u_series is not None else c].T)
                    row["u_opt_smooth_flips"] += int(np.sum(ug[free] != un[free]))
                    row["u_opt_smooth_entries"] += int(free.sum())
            report[name] = row
            # the 120-day case of the three-state flipped wrapper is held to the plain north-star tolerance: over that span
            # the backward map's instability has not yet amplified one ulp beyond it.  The longer flipped cases are gated at
            # TEN TIMES what one ulp on the observations does to the LAPACK reading's own output (stated in the report as
            # `gate` beside `reading_moved_by_one_ulp_of_x`) -- and, round 4, against the exact evaluation: on the first
            # three chains the HIP output may be no further from the 160-digit referee than ten times the LAPACK reading is
            row["gate"] = NORTH_STAR_TOL if "plain 1e-6 gate" in name else max(NORTH_STAR_TOL, 10.0 * row.get("reading_moved_by_one_ulp_of_x", 0.0))
            row["gate_is"] = "1e-6" if row["gate"] == NORTH_STAR_TOL else "10 x the one-ulp sensitivity of the reading"
            if max(row["S_PLUS_1to3"], row["new_cases_filtered"], row["new_cases_predicted"]) > row["gate"]:
                failed.append(name)
            if flipped:
                from oracle import referee_mp as rf
                dh = dl = 0.0
                for c in range(min(3, w.B)):
                    ex = rf.run_model(w.model, *H.chain_args(w, c))
                    dh = max(dh, H.rowwise_abs_rel_err(H.batch_chain(got, "S_PLUS", c, m)[:3], ex["S_PLUS"][:3]))
                    dl = max(dl, H.rowwise_abs_rel_err(res[c]["S_PLUS"][:3], ex["S_PLUS"][:3]))
                row["S_PLUS_1to3_distance_from_exact"] = {"hip": dh, "lapack_reading": dl}
                if dh > 10.0 * dl + 1e-12:
                    failed.append(name + " (vs the exact evaluation)")
    os.makedirs(os.path.join(H.ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(H.ROOT, "gpurun_out", "parity_vs_lapack_other_configs.json"), "w") as f:
        json.dump({"what": "HIP kernels (libepiekf.so) vs oracle/ekf_numpy.py (NumPy, LAPACK SVD pinv / LU mrdivide)",
                   "gate": "1e-6 relative on S_PLUS(1:3), filtered and predicted new cases; time-flipped wrappers: or 10 x "
                           "what one ulp on the observations does to the reading itself, if larger", "cases": report}, f, indent=1)
    print(json.dumps(report))
    assert not failed, (failed, report)


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_sia6_both_shapes(gpu_device, shape):
    """SIAlphaModelBackwardEKFOptControlled through both lane mappings, blocked and classic layouts; rho in filter-step
    order (un-reversed, as MATLAB returns it -- tests/test_oracle.py::test_kat_backward_wrapper_returns_rho_unreversed)."""
    from epidemicmodeling_amd import synth
    w = synth.as_backward(synth.make_cfg4(8, 10, 40, 0))
    ref = H.oracle_batch(w)
    for blk in (0, 16, 5):
        got = _run(w, gpu_device, shape=shape, lane_block=blk)
        for n in H.OUT_NAMES:
            assert np.array_equal(got[n], ref[n], equal_nan=True), (shape, blk, n)
        assert np.array_equal(got["pinv_rank"], ref["pinv_rank"])
    assert np.all(ref["rho"][0] == 0.0) and np.any(ref["rho"][-1] != 0.0)


@pytest.mark.parametrize("shape", ["auto", "quad"])
@pytest.mark.parametrize("rank", [0, 7])
def test_strong_scaling_shard_at_full_size(gpu_device, rank, shape):
    """What one of 8 GPUs runs when the FIXED headline sweep (75 000 chains x 520 days) is sharded by chain blocks
    (bench.py --gpus 8): 9 375 chains, which the library maps six lanes per chain, ten chains per wavefront (shape auto,
    round 5; four lanes per chain until round 4 -- still run here when asked for).  Sampled chains of the shard -- lane-group,
    wavefront and layout-block boundaries of both shapes included -- equal the oracle's run of those chains alone, and then all
    9 375 do (938 hex wavefronts: the stale image of DESIGN.md 4.1 sat in about 3 of them, which the sample saw with 35 %).  Rank
    0 on the library's own shape also runs five passes back to back and one replay of a captured graph -- the fork/join of the
    reverse-time pipeline inside it -- into poisoned outputs, each compared over the whole shard (_back_to_back_and_graph_replay)."""
    import torch
    from epidemicmodeling_amd import batch, synth
    w = synth.make_cfg4()
    lo, hi = batch.shard_chains(w.B, rank, 8)
    assert hi - lo == 9375
    torch.cuda.reset_peak_memory_stats()
    ws = w.select(np.arange(lo, hi))
    idx = np.unique(np.concatenate([np.linspace(0, ws.B - 1, 120).astype(np.int64),
                                    [9, 10, 11, 15, 16, 17, 59, 60, 63, 64, 9359, 9360, 9369, 9370, 9374]]))
    ref = H.oracle_batch(ws.select(idx))
    dw = batch.DeviceWorkload(ws, gpu_device)
    r = batch.EkfRunner(dw, extras=True, lane_block="auto", shape=shape)
    assert r.blk == {"auto": 10, "quad": 16}[shape]   # the lane mapping the library chose: its wavefront's chains are one layout block
    r.run()
    torch.cuda.synchronize()
    sel = torch.as_tensor(idx, device=gpu_device)
    for n in H.OUT_NAMES:
        assert np.array_equal(r.unblocked(n).index_select(-1, sel).cpu().numpy(), ref[n], equal_nan=True), n
    assert np.array_equal(r.unblocked("pinv_rank").index_select(-1, sel).cpu().numpy(), ref["pinv_rank"])
    tag = "shard rank %d shape %s" % (rank, shape)
    assert H.all_chains_equal_oracle(r, ws, what=tag)["chains"] == 9375
    if rank == 0 and shape == "auto":
        _room_for_clones(r, gpu_device)
        saved = H.snapshot_outputs(r)
        _back_to_back_and_graph_replay(r, saved, r.run, tag)
    _peak_memory(tag)


def _sweep_params(w, device, seed=5):
    """scoring parameters / prefixes of a sweep, as tests/test_gpu_fuzz.py draws them"""
    import torch
    from epidemicmodeling_amd import batch, layout as L_, synth
    rng = np.random.default_rng(seed)
    n, B = w.n_npi, w.B
    sp = np.zeros((batch.SIM_PRM_COUNT, B))
    sp[0] = 1.0 - 1e-3 * rng.random(B); sp[1] = 1e-3 * rng.random(B); sp[2] = synth.ALPHA0 * (0.5 + rng.random(B))
    sp[3] = w.prm[L_.PRM_ALPHA_MIN]; sp[4] = w.prm[L_.PRM_ALPHA_MAX]; sp[5] = w.prm[L_.PRM_GAMMA]
    sp[6] = w.prm[L_.PRM_B]; sp[7] = w.prm[L_.PRM_BETA]; sp[11] = 1.0
    sp[batch.SIM_A:batch.SIM_A + n] = w.prm[L_.PRM_A:L_.PRM_A + n]
    sp[batch.SIM_U_MAX:batch.SIM_U_MAX + n] = w.prm[L_.PRM_U_MAX:L_.PRM_U_MAX + n]
    sp[batch.SIM_W:batch.SIM_W + n] = rng.random((n, B)) + 0.5
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(device)
    return to(sp), to(rng.random(B) * 1e-2), to(rng.random(B) * 40.0)


def _check_sweep_entry(r, w, t_hist, n_regions, ref, device, sel=None):
    """run_sweep against the oracle (filter outputs) and against the separate scoring / Pareto calls on the u_opt_smooth it wrote.
    sel given (a batch too large to bring down whole; `ref` holds chains sel only): a plain run() first, EVERY chain of it against
    the oracle in chain ranges, device clones of that; then run_sweep into poisoned outputs, its sampled chains against `ref` and
    its whole batch against the clones."""
    import torch
    from epidemicmodeling_amd import batch
    sp, j0, j1 = _sweep_params(w, device)
    saved = None
    if sel is not None:
        r.run()
        torch.cuda.synchronize()
        assert H.all_chains_equal_oracle(r, w, what="reverse-time pipeline, %d chains x %d days" % (w.B, w.T))["chains"] == w.B
        _room_for_clones(r, device)
        saved = H.snapshot_outputs(r)
    for t in list(r.out.values()) + [r.ws]:
        t.fill_(float("nan"))
    sc = r.run_sweep(t_hist, sp, j0, j1, n_regions=n_regions)
    torch.cuda.synchronize()
    pick = (lambda t: t) if sel is None else (lambda t: t.index_select(-1, sel))
    for n in r.out:
        assert np.array_equal(pick(r.unblocked(n)).cpu().numpy(), ref[n], equal_nan=True), n
    assert np.array_equal(pick(r.unblocked("pinv_rank")).cpu().numpy(), ref["pinv_rank"])
    if saved is not None:
        assert H.device_outputs_equal(r, saved, what="sweep entry, %d chains x %d days" % (w.B, w.T))["chains"] == w.B
    sc2 = batch.score_sweep(r.out["u_opt_smooth"], t_hist, sp, j0, j1, B=w.B)
    assert torch.equal(sc["J0"], sc2["J0"]) and torch.equal(sc["J1"], sc2["J1"])
    if n_regions:
        on2, io2 = batch.pareto_front(sc2["J0"], sc2["J1"], n_regions)
        assert torch.equal(sc["on_front"].bool(), on2) and torch.equal(sc["i_opt"], io2)


def test_both_monitor_kernels_replay_the_same_rho(gpu_device):
    """With a per-day R_v the innovation monitor (GenericEKF.m:172-179) is replayed from the stored innovations by one of two
    kernels: the scan-free grid ekf_monitor_par (one lane per chain and 8 days; up to 65 536 chains) or the scan kernel ekf_monitor
    (time segments with a 2L - 2 step warm-up; beyond).  epi_batch_desc.test_flags bit 1 forces the scan kernel at any size: both
    must give the oracle's rho bit for bit -- forward and time-flipped models, day counts that are not a multiple of 8, fewer days
    than the window, 3 and 6 states, the classic and a blocked layout."""
    from epidemicmodeling_amd import synth
    cases = [synth.make_cfg4(5, 9, 37, 6), synth.as_backward(synth.make_cfg4(4, 8, 29, 4)), synth.make_cfg4(3, 5, 11, 2),
             synth.make_cfg3(12, 75), synth.as_backward(synth.make_cfg3(7, 19)), synth.make_cfg4(2, 6, 150, 9)]
    for w in cases:
        ref = H.oracle_batch(w)
        assert np.any(ref["rho"] != 0.0)
        for blk in (0, 16):
            par = _run(w, gpu_device, shape="lane", lane_block=blk)
            scan = _run(w, gpu_device, shape="lane", lane_block=blk, test_flags=2)
            assert np.array_equal(par["rho"], ref["rho"], equal_nan=True), (w.model, w.T, blk, "par")
            assert np.array_equal(scan["rho"], ref["rho"], equal_nan=True), (w.model, w.T, blk, "scan")


@pytest.mark.parametrize("window", [0, 4])
def test_hex_reverse_time_pipeline_forced_at_small_batches(gpu_device, window):
    """The reverse-time pipeline of the hex shape (launch_chain: the pinv grids of the earlier days on the helper stream beside the
    smoother's first launches, the smoother cut into segments that hand their state over through the hand-over rows, the scoring
    tail forked onto the helper stream) engages beyond 768 hex wavefronts and 128 days; epi_batch_desc.test_flags bit 0 forces it
    at any size, so that it meets what the small tests vary: forward and time-flipped model, a call without a scoring tail, the
    horizon / history cut at both ends of the day range, few days (segments of one or two steps), short addressing windows --
    against the oracle and against the same call with the pipeline off (time_pipe = -1)."""
    import torch
    from epidemicmodeling_amd import batch, synth
    cases = [(synth.make_cfg4(8, 10, 40, 7), 40), (synth.make_cfg4(5, 12, 30, 12), 1), (synth.make_cfg4(5, 12, 30, 12), 40),
             (synth.make_cfg4(3, 7, 9, 3), 9), (synth.make_cfg4(6, 9, 140, 10), 140), (synth.make_cfg4(2, 5, 3, 1), 2)]
    for w, t_hist in cases:
        ref = H.oracle_batch(w)
        for blk in (10, 0):
            got = _run(w, gpu_device, shape="hex", lane_block=blk, test_flags=1, test_window=window)
            off = _run(w, gpu_device, shape="hex", lane_block=blk, time_pipe=-1)
            for n in H.OUT_NAMES:
                assert np.array_equal(got[n], ref[n], equal_nan=True), (w.T, t_hist, blk, n)
                assert np.array_equal(got[n], off[n], equal_nan=True), (w.T, t_hist, blk, n)
            dw = batch.DeviceWorkload(w, gpu_device)
            r = batch.EkfRunner(dw, extras=True, lane_block=blk, shape="hex", test_flags=1, test_window=window)
            _check_sweep_entry(r, w, t_hist, len(np.unique(w.x_series)), ref, gpu_device)
    wb = synth.as_backward(synth.make_cfg4(7, 10, 33, 6))          # the time-flipped model: run() only (the sweep is the forward model's)
    ref = H.oracle_batch(wb)
    got = _run(wb, gpu_device, shape="hex", lane_block=10, test_flags=1, test_window=window)
    for n in H.OUT_NAMES:
        assert np.array_equal(got[n], ref[n], equal_nan=True), ("backward", n)
    assert np.array_equal(got["pinv_rank"], ref["pinv_rank"])


@pytest.mark.parametrize("regions,eps,T_hist,hor", [(75, 125, 400, 120), (83, 125, 120, 12)])
def test_sweep_entry_through_the_reverse_time_pipeline_at_size(gpu_device, regions, eps, T_hist, hor):
    """The call bench.py times for the 8-GPU shard -- epi_sweep_run_device on 9 375 chains x 520 days -- and a batch beyond one hex
    wavefront per SIMD with T >= 128 (10 375 chains x 132 days: the smoother's no-prefetch variant resuming from hand-over rows)
    both take the reverse-time pipeline by themselves: sampled chains and then all 9 375 / 10 375 against the oracle (a plain call),
    the sweep entry's whole batch against device clones of that, (J0, J1) / front / I_opt against the separate calls."""
    import torch
    from epidemicmodeling_amd import batch, synth
    w = synth.make_cfg4(n_regions=regions, n_eps=eps, T_hist=T_hist, horizon=hor)
    idx = np.unique(np.concatenate([np.linspace(0, w.B - 1, 70).astype(np.int64), [9, 10, 11, 59, 60, 63, 64, w.B - 6, w.B - 5, w.B - 1]]))
    ref = H.oracle_batch(w.select(idx))
    dw = batch.DeviceWorkload(w, gpu_device)
    r = batch.EkfRunner(dw, extras=True, lane_block="auto", shape="auto")
    assert r.blk == 10
    _check_sweep_entry(r, w, T_hist, regions, ref, gpu_device, sel=torch.as_tensor(idx, device=gpu_device))


@pytest.mark.parametrize("window", [2, 6])
def test_hex_addressing_windows(gpu_device, window):
    """The hex kernels address every array relative to the first day of a WINDOW of days (the day offset travels in the buffer
    instructions' 32-bit scalar offset; ekf_hex.hpp, hx_window) and move the bases when a window ends -- with the default size
    (2 GiB worth of days) no test would ever cross a boundary, so epi_batch_desc.test_window shortens it to a few days: forward and
    time-flipped model, chain-blocked and classic layouts, a day count that is not a multiple of the window, the sweep's
    horizon / observed-days cut of the smoother, T == 1 .. 3."""
    from epidemicmodeling_amd import synth
    cases = [synth.make_cfg4(8, 10, 40, 7), synth.as_backward(synth.make_cfg4(8, 10, 33, 0)), synth.make_cfg4(3, 7, 2, 1),
             synth.make_cfg4(2, 5, 1, 0), synth.make_cfg4(2, 5, 2, 0)]
    for w in cases:
        ref = H.oracle_batch(w)
        for blk in (0, 10, 5):
            got = _run(w, gpu_device, shape="hex", lane_block=blk, test_window=window)
            for n in H.OUT_NAMES:
                assert np.array_equal(got[n], ref[n], equal_nan=True), (w.model, w.T, window, blk, n)
            assert np.array_equal(got["pinv_rank"], ref["pinv_rank"])


@pytest.mark.parametrize("window", [0, 2, 5])
def test_lane6_fixed_descriptor_kernels(gpu_device, window):
    """The one-lane kernels with fixed descriptors per addressing window (ekf_lane6.hpp) run whenever the layout block is the 40
    chains they are instantiated for -- at full size that is the headline sweep's own layout; here small batches are put on that
    layout on purpose: forward and time-flipped model, free controls over the horizon (the wave-level fast path of the bang-bang
    substitution is taken on the historic days only), a chain count that is not a multiple of 40, all outputs and reduced ones,
    the sweep's cut of the smoother at the horizon, T == 1 .. 3, and addressing windows of a few days."""
    from epidemicmodeling_amd import synth
    cases = [synth.make_cfg4(9, 10, 40, 7), synth.as_backward(synth.make_cfg4(8, 11, 33, 4)), synth.make_cfg4(3, 7, 2, 1),
             synth.make_cfg4(2, 5, 1, 0), synth.make_cfg4(2, 5, 2, 0), synth.make_cfg4(7, 30, 25, 12, live=True),
             # chain counts that are multiples of 40: the variant that takes X of the next step by LDS-DMA (every lane alive)
             synth.make_cfg4(8, 10, 37, 9), synth.as_backward(synth.make_cfg4(6, 20, 29, 5)), synth.make_cfg4(4, 10, 3, 1),
             synth.make_cfg4(2, 20, 1, 0), synth.make_cfg4(5, 40, 30, 11, live=True)]
    for w in cases:
        ref = H.oracle_batch(w)
        for blk, tp in ((40, 0), (40, -1), (48, 0), (56, 0)):
            if blk >= w.B:
                continue
            got = _run(w, gpu_device, shape="lane", lane_block=blk, time_pipe=tp, test_window=window)
            for n in H.OUT_NAMES:
                assert np.array_equal(got[n], ref[n], equal_nan=True), (w.model, w.T, w.B, window, blk, tp, n)
            assert np.array_equal(got["pinv_rank"], ref["pinv_rank"])


def test_one_lane_batch_cut_into_two_chain_ranges(gpu_device):
    """A one-lane batch of more waves than SIMDs (the headline sweep: 1 875 waves on 1 024 SIMDs) is launched as two chain ranges --
    forward kernel, pinv grid (the first range's on the helper stream beside the second forward launch), and on the 40 / 48 / 56
    chain layouts the smoother with the monitor between its two launches.  epi_batch_desc.test_flags bit 2 cuts a batch of two
    waves or more in the middle the same way, so that these few hundred chains reach every launch of it: forward and time-flipped
    model, free controls, chain counts that are and are not multiples of the layout block, the layouts whose smoother takes chain
    ranges and those whose smoother runs whole, both monitor kernels -- all outputs against the oracle, bit for bit -- and the
    sweep's entry (scoring tail and Pareto filter behind the second smoother launch)."""
    from epidemicmodeling_amd import synth
    cases = [synth.make_cfg4(9, 30, 40, 7), synth.as_backward(synth.make_cfg4(8, 21, 33, 4)), synth.make_cfg4(7, 30, 25, 12, live=True),
             synth.make_cfg4(8, 25, 37, 9), synth.make_cfg4(13, 10, 3, 1), synth.make_cfg4(4, 33, 1, 0)]
    for w in cases:
        ref = H.oracle_batch(w)
        for blk, flags in ((40, 4), (40, 6), (48, 4), (56, 4), (0, 4), (64, 4), (16, 6)):
            got = _run(w, gpu_device, shape="lane", lane_block=blk, time_pipe=-1, test_flags=flags)
            for n in H.OUT_NAMES:
                assert np.array_equal(got[n], ref[n], equal_nan=True), (w.model, w.T, w.B, blk, flags, n)
            assert np.array_equal(got["pinv_rank"], ref["pinv_rank"])
    from epidemicmodeling_amd import batch
    w = synth.make_cfg4(n_regions=6, n_eps=40, T_hist=30, horizon=9)
    ref = H.oracle_batch(w)
    for blk in (40, 64):
        r = batch.EkfRunner(batch.DeviceWorkload(w, gpu_device), extras=True, lane_block=blk, shape="lane", time_pipe=-1, test_flags=4)
        _check_sweep_entry(r, w, 30, 6, ref, gpu_device)


@pytest.mark.parametrize("window", [0, 4])
def test_hex_two_waves_per_simd_kernels(gpu_device, window):
    """Beyond one hex wavefront per SIMD (10 240 chains on MI355X) the library launches the hex kernels' other variants -- no
    prefetch set in the smoother, no register clobber in the forward kernel, two waves per SIMD -- which no smaller test reaches:
    10 375 chains x 26 days, sampled chains and then all 10 375 against the oracle's run of those chains alone; once more with
    short addressing windows (see test_hex_addressing_windows)."""
    import torch
    from epidemicmodeling_amd import batch, synth
    w = synth.make_cfg4(n_regions=83, n_eps=125, T_hist=20, horizon=6)
    assert w.B == 10375
    idx = np.unique(np.concatenate([np.linspace(0, w.B - 1, 90).astype(np.int64), [9, 10, 11, 59, 60, 63, 64, 10239, 10240, 10241, 10369, 10370, 10374]]))
    ref = H.oracle_batch(w.select(idx))
    dw = batch.DeviceWorkload(w, gpu_device)
    r = batch.EkfRunner(dw, extras=True, lane_block="auto", shape="auto", test_window=window)
    assert r.blk == 10
    r.run()
    torch.cuda.synchronize()
    sel = torch.as_tensor(idx, device=gpu_device)
    for n in H.OUT_NAMES:
        assert np.array_equal(r.unblocked(n).index_select(-1, sel).cpu().numpy(), ref[n], equal_nan=True), n
    assert np.array_equal(r.unblocked("pinv_rank").index_select(-1, sel).cpu().numpy(), ref["pinv_rank"])
    assert H.all_chains_equal_oracle(r, w, what="hex, two waves per SIMD, window %d" % window)["chains"] == 10375


def test_whole_batch_comparisons_see_one_word_on_the_device(gpu_device):
    """The whole-batch helpers (tests/test_whole_batch_helpers.py tests them on CPU tensors) where the full-size tests use them: on
    device tensors the library wrote, hex shape on its 10-chain layout with a padded last block.  One word of the device's output
    moved by 1 ulp, in a chain the full-size tests' kind of sample does not hold, fails both comparisons with its (chain, day, row)
    and block; put back, both pass again."""
    import torch
    from epidemicmodeling_amd import batch, synth
    w = synth.make_cfg4(n_regions=9, n_eps=37, T_hist=20, horizon=6)            # 333 chains: 34 blocks of 10, the last one of 3
    r = batch.EkfRunner(batch.DeviceWorkload(w, gpu_device), extras=True, lane_block=10, shape="hex")
    r.run()
    torch.cuda.synchronize()
    assert H.all_chains_equal_oracle(r, w, chunk=100)["chains"] == 333
    saved = H.snapshot_outputs(r)
    idx = np.unique(np.concatenate([np.linspace(0, w.B - 1, 3).astype(np.int64), [9, 10, 11, 59, 60, 63, 64, w.B - 1]]))
    chain, day, row = 217, 13, 7
    assert chain not in idx
    word = r.out["P_SMOOTH"][day, chain // 10, row]
    old = float(word[chain % 10])
    assert np.isfinite(old) and old != 0.0
    word[chain % 10] = float(np.nextafter(old, np.inf))
    where = "(chain %d, day %d, row %d)" % (chain, day, row)
    for check in (lambda: H.all_chains_equal_oracle(r, w, chunk=100), lambda: H.device_outputs_equal(r, saved)):
        with pytest.raises(AssertionError) as e:
            check()
        assert "P_SMOOTH differs in 1 chain(s)" in str(e.value) and where in str(e.value) and "(chain // 10): [21]" in str(e.value), str(e.value)
    word[chain % 10] = old
    H.all_chains_equal_oracle(r, w, chunk=100)
    H.device_outputs_equal(r, saved)
    H.poison_runner(r)
    with pytest.raises(AssertionError):
        H.device_outputs_equal(r, saved)


def test_host_entry_keeps_the_fastest_of_several_arenas(gpu_device):
    """epi_batch_desc.placement_tries (ABI 6): a host-pointer call that has to allocate a new device arena times its own kernels on
    up to N candidate arenas and keeps the fastest, with that arena's complete results -- the outputs equal the oracle's whichever
    arena was kept, the report names every candidate, and the next call of the same size finds the arena in its pooled context
    (no new tries).  epi_ekf_time_stages_device, the device-pointer caller's way to compare allocations, times the same stages."""
    import ctypes as C
    from epidemicmodeling_amd import _lib, batch, synth
    _lib.lib().epi_host_pool_release()                        # no pooled arena from earlier tests
    w = synth.make_cfg4(6, 40, 50, 12)                        # 240 chains x 62 days
    ref = H.oracle_batch(w)
    rep = []
    got = H.host_call(w, placement_tries=3, report=rep)
    for n in H.OUT_NAMES:
        assert np.array_equal(got[n], ref[n], equal_nan=True), n
    assert np.array_equal(got["pinv_rank"], ref["pinv_rank"])
    assert rep[0]["tries"] == 3 and 0 <= rep[0]["chosen"] < 3 and all(ms > 0 for ms in rep[0]["ms"]), rep
    assert rep[0]["ms"][rep[0]["chosen"]] == min(rep[0]["ms"])
    again = H.host_call(w, placement_tries=3, report=rep)     # the pooled context still holds the arena that was kept
    assert rep[1]["tries"] == 0
    for n in H.OUT_NAMES:
        assert np.array_equal(again[n], ref[n], equal_nan=True), n
    off = H.host_call(w, report=rep)                          # placement_tries = 0: no report either
    assert rep[2]["tries"] == 0 and np.array_equal(off["S_SMOOTH"], ref["S_SMOOTH"], equal_nan=True)
    _lib.lib().epi_host_pool_release()
    dw = batch.DeviceWorkload(w, gpu_device)
    r = batch.EkfRunner(dw, extras=True)
    f, p, b = r.stage_ms(min_ms=5.0)
    assert f > 0 and p > 0 and b > 0
    for n in H.OUT_NAMES:                                     # the timed rounds are ordinary passes: they leave the results
        assert np.array_equal(r.unblocked(n).cpu().numpy(), ref[n], equal_nan=True), n


def test_host_multi_device_entry_shards_chains(gpu_device):
    """epi_ekf_run_host_multi: the chains of ONE host call cut into contiguous blocks, one host thread per block, outputs
    written straight into the caller's arrays.  The box has one GPU, so the blocks name device 0 several times (they then
    run concurrently on pooled contexts of that device): ragged last block, an empty block (more blocks than chains),
    series shared between chains of different blocks, per-chain series (identity x_series / u_series) and adaptive scalar R."""
    from epidemicmodeling_amd import synth
    cases = [(synth.make_cfg4(3, 5, 30, 10), [0, 0]),             # 15 chains -> 8 + 7; region 1's chains straddle the cut
             (synth.make_cfg4(2, 7, 25, 6), [0, 0, 0, 0]),        # 14 chains -> 4 + 4 + 4 + 2
             (synth.make_cfg5(3, 3, 40), [0, 0]),                 # per-chain series (Sx == B, no index arrays), 3-state
             (synth.make_row3(2, 3, 20, 8), [0, 0, 0]),           # adaptive scalar R_v
             (synth.make_cfg4(1, 3, 20, 5), [0, 0, 0, 0, 0])]     # 3 chains over 5 blocks: two blocks are empty
    for w, devs in cases:
        ref = H.oracle_batch(w)
        one = H.host_call(w)
        many = H.host_call(w, devices=devs)
        for n in H.OUT_NAMES:
            if n in ref:
                assert np.array_equal(one[n], ref[n], equal_nan=True), (w.model, n)
                assert np.array_equal(many[n], ref[n], equal_nan=True), (w.model, len(devs), n)
        assert np.array_equal(many["pinv_rank"], one["pinv_rank"]) and np.array_equal(many["status"], one["status"])
        assert np.array_equal(one["pinv_rank"], ref["pinv_rank"])


def test_host_call_copy_routes(gpu_device):
    """The host entry points move the caller's arrays by one of four routes (HostIO in epiekf.hip): packed through the pinned
    buffer (small calls: every other host test), ONE copy per array straight to / from pageable memory (a call over all chains
    above 8 MiB), packed strided pieces (chain blocks of a multi-device call that fit the pinned buffer) and 2-D copies (blocks
    beyond it).  Each route must deliver the oracle's bits into the right rows and columns, and leave the NaN fill of the
    caller's arrays nowhere."""
    from epidemicmodeling_amd import synth
    cases = [(synth.make_cfg4(1, 60, 100, 20), "9 MB of outputs: dense direct / strided packed"),
             (synth.make_cfg4(1, 250, 400, 120), "164 MB: dense direct / 82 MB blocks as 2-D copies")]
    for w, what in cases:
        ref = H.oracle_batch(w)
        for devs in (None, [0, 0]):
            got = H.host_call(w, devices=devs)
            for n in H.OUT_NAMES:
                if n in ref:
                    assert np.array_equal(got[n], ref[n], equal_nan=True), (what, devs, n)
            assert np.array_equal(got["pinv_rank"], ref["pinv_rank"]), (what, devs)
            assert not (got["status"] == -7).any()


def test_simulator_host_call_takes_both_copy_routes(gpu_device):
    """epi_sir_sim_host at B = 4096, K = 128 writes one dense 12.6 MB array, above the 8 MiB below which a call is packed
    through the pinned buffer: it goes straight into the caller's array and equals the device call; a small call on the same
    context then goes through the pinned buffer again."""
    rng = np.random.default_rng(3)
    for B, K in ((4096, 128), (5, 6)):
        prm = np.stack([0.3 + 0.1 * rng.random(B), np.full(B, 0.1), np.full(B, 0.01), np.full(B, 0.99), np.full(B, 0.01), np.zeros(B)])
        args = [B, K, 0.5, prm, ("out", (K, 3, B))]
        got, want = H.flat_call("sir_sim", args)["out"], H.flat_call("sir_sim", args, gpu=gpu_device)["out"]
        assert np.isfinite(got).all() and np.array_equal(got, want), (B, K)


def test_host_entry_points_from_concurrent_threads_and_pool_release(gpu_device):
    """The host entry points are thread-safe and keep their state in pools that epi_host_pool_release frees: six threads
    call epi_ekf_run_host / epi_ekf_run_host_multi (three blocks on the one device: the per-device worker) / the sweep entry /
    SIalpha_Controlled / nnls_affine_fit at the same time, several rounds (contexts and helper streams are leased concurrently, workers are shared); every result
    equals the oracle's.  Then the pools are released and everything runs again (pools, helper streams and worker threads are
    created anew)."""
    import threading
    from epidemicmodeling_amd import _lib, hostapi, synth
    ws = [synth.make_cfg4(3, 9, 150, 20), synth.make_cfg3(40, 130), synth.make_cfg4(5, 4, 30, 6), synth.make_row3(2, 5, 25, 10),
          synth.as_backward(synth.make_cfg3(10, 60)), synth.make_row4(3, 60, 20)]
    refs = [H.oracle_batch(w) for w in ws]
    pr = _region_sweep_problem(4, 7, 50, 12, seed=3)
    sweep_ref = hostapi.sweep_prescribe(pr["x"], pr["u"], pr["R"], pr["reg"], pr["eps"], pr["sp"], pr["J0p"], pr["J1p"], 50)
    # two workers also make one call of a simulator / a small fit per round (the same pooled contexts)
    from epidemicmodeling_amd import tools
    rng = np.random.default_rng(8)
    sim_args = (rng.random((2, 30)), 0.99, 0.01, 0.3, [3.0, 2.0], 0.0, 100.0, 1 / 7, [0.01, 0.02], 0.0, synth.MODEL_BETA, 1e-3, 1e-3, 1e-3, 30, 1.0)
    sim_noise = rng.standard_normal((3, 30))
    sim_ref = tools.SIalpha_Controlled(*sim_args, noise=sim_noise)
    X, y = rng.integers(0, 4, size=(16, 3, 3)).astype(np.float64), rng.random((16, 3))
    fit_ref = hostapi.nnls_affine_fit(X, y)
    errors = []

    def worker(i):
        try:
            for rnd in range(4):
                w, ref = ws[i], refs[i]
                got = H.host_call(w, devices=[0, 0, 0] if (i + rnd) % 2 else None)
                for n in H.OUT_NAMES:
                    if n in ref and n in got and not np.array_equal(got[n], ref[n], equal_nan=True):
                        errors.append((i, rnd, n))
                if i == 0:
                    g = hostapi.sweep_prescribe(pr["x"], pr["u"], pr["R"], pr["reg"], pr["eps"], pr["sp"], pr["J0p"], pr["J1p"], 50,
                                                devices=(0, 0))
                    if not (np.array_equal(g["J0"], sweep_ref["J0"]) and np.array_equal(g["u_opt"], sweep_ref["u_opt"])):
                        errors.append((i, rnd, "sweep"))
                if i == 1 and not all(np.array_equal(a, b) for a, b in zip(tools.SIalpha_Controlled(*sim_args, noise=sim_noise), sim_ref)):
                    errors.append((i, rnd, "SIalpha_Controlled"))
                if i == 2:
                    fit = hostapi.nnls_affine_fit(X, y)
                    if not all(np.array_equal(fit[k], fit_ref[k]) for k in fit_ref):
                        errors.append((i, rnd, "nnls_affine_fit"))
        except Exception as e:                       # noqa: BLE001 -- reported below
            errors.append((i, repr(e)))

    for phase in range(2):
        threads = [threading.Thread(target=worker, args=(i,)) for i in range(len(ws))]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
        assert not errors, (phase, errors)
        _lib.lib().epi_host_pool_release()


def test_host_call_latency_report(gpu_device):
    """Wall time of ONE reference-shaped call (B = 1, T = 520, 6 states, all outputs) through epi_ekf_run_host -- pooled
    context: no allocation after the first call, one copy each way -- next to the CPU oracle's single-thread time for the
    same chain, and of the 250-cost-weight batch of one region (what SIAlphaModelEKFOptControlledSweep.m sends).  Reported
    in gpurun_out/single_call_latency.json (committed copy: profiles/r03/).  Report only: a wall-clock bound does not belong
    in a correctness suite that may run on a shared box; the assertion is on the results."""
    import json, os, time
    from epidemicmodeling_amd import synth
    full = synth.make_cfg4(2, 250, 400, 120)
    w1 = full.select(np.array([137]))
    w250 = full.select(np.arange(250))
    rep = {}
    for tag, w in (("B1", w1), ("B250", w250)):
        H.host_call(w, extras=False)                         # first call: creates the context, sizes the arena
        ts = []
        for _ in range(7):
            t0 = time.perf_counter(); got = H.host_call(w, extras=False); ts.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); ref = H.oracle_batch(w, n_threads=1); t_cpu = time.perf_counter() - t0
        assert np.array_equal(got["S_SMOOTH"], ref["S_SMOOTH"], equal_nan=True)
        rep[tag] = {"chains": w.B, "days": w.T, "gpu_call_ms_median": 1e3 * float(np.median(ts)), "gpu_call_ms_min": 1e3 * min(ts),
                    "cpu_oracle_one_thread_ms": 1e3 * t_cpu,
                    "note": "python packing of the ctypes call included in the GPU figure (~0.1 ms)"}
    os.makedirs(os.path.join(H.ROOT, "gpurun_out"), exist_ok=True)
    json.dump(rep, open(os.path.join(H.ROOT, "gpurun_out", "single_call_latency.json"), "w"), indent=1)
    print(json.dumps(rep))


def test_fp32_storage_outputs_are_the_fp64_results_rounded_once(gpu_device):
    """epi_batch_desc.storage = 1 (BASELINE config 5's "fp32" as SURVEY.md 0 resolves it: fp32 STORAGE, fp64 register
    arithmetic, the smoother's inputs kept in an fp64 workspace): every output equals float32(oracle fp64 output) bit for bit
    -- 3- and 6-state packed kernels, forward and time-flipped, classic and blocked layouts, a subset of the outputs."""
    from epidemicmodeling_amd import synth
    for w in (synth.make_cfg5(4, 9, 60), synth.make_cfg4(3, 7, 40, 12), synth.as_backward(synth.make_cfg3(5, 30)),
              synth.make_row3(2, 5, 20, 8)):
        ref = H.oracle_batch(w)
        for blk in (0, 8, "auto"):
            got = _run(w, gpu_device, storage="f32", lane_block=blk, shape="lane")
            for n in H.OUT_NAMES:
                assert got[n].dtype == np.float32
                assert np.array_equal(got[n], ref[n].astype(np.float32), equal_nan=True), (w.model, blk, n)
            assert np.array_equal(got["pinv_rank"], ref["pinv_rank"])
        sub = _run(w, gpu_device, storage="f32", outputs=["S_SMOOTH", "u_opt_smooth", "rho"])
        for n in ("S_SMOOTH", "u_opt_smooth", "rho"):
            assert np.array_equal(sub[n], ref[n].astype(np.float32), equal_nan=True), (w.model, n)


def test_monte_carlo_eks_fp32_storage_at_full_size_sampled_chains(gpu_device):
    """BASELINE config 5 as written -- 300 regions x 1024 draws x 400 days, fp32 storage -- at full size (307 200 chains):
    sampled chains of the big batch equal float32(the oracle's fp64 run of those chains alone), bit for bit.  The rule "fp32
    storage is the fp64 result rounded once" is then checked on the device over ALL 307 200 chains against an fp64 run of the same
    batch -- the run that test_monte_carlo_eks_at_full_size_sampled_chains holds against the oracle chain by chain (the oracle is
    not run a second time over 123 M chain-days; here the fp64 run's sampled chains are held against it)."""
    import torch
    from epidemicmodeling_amd import batch, synth
    torch.cuda.reset_peak_memory_stats()
    w = synth.make_cfg5(300, 1024, 400)
    idx = np.unique(np.concatenate([np.linspace(0, w.B - 1, 200).astype(np.int64), [55, 56, 57, 63, 64, 1023, 1024, 307199]]))
    ref = H.oracle_batch(w.select(idx))
    dw = batch.DeviceWorkload(w, gpu_device)
    r = batch.EkfRunner(dw, extras=True, lane_block="auto", storage="f32")
    r.run()
    torch.cuda.synchronize()
    sel = torch.as_tensor(idx, device=gpu_device)
    for n in H.OUT_NAMES:
        got = r.unblocked(n).index_select(-1, sel).cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got, ref[n].astype(np.float32), equal_nan=True), n
    torch.cuda.empty_cache()
    r64 = batch.EkfRunner(dw, extras=True, lane_block="auto")
    assert r64.blk == r.blk
    r64.run()
    torch.cuda.synchronize()
    for n in H.OUT_NAMES:
        assert np.array_equal(r64.unblocked(n).index_select(-1, sel).cpu().numpy(), ref[n], equal_nan=True), n
    st = H.device_outputs_equal(r, H.snapshot_views(r64), rounded=True, what="fp32 storage against the fp64 run rounded once")
    assert st["chains"] == 307200
    _peak_memory("Monte-Carlo EKS fp32 storage + fp64 run")
    del r64
    del r, dw
    torch.cuda.empty_cache()


def test_seirp_ensemble_at_full_size_sampled_members(gpu_device):
    """BASELINE config 2 at full size: a 10 000-member parameter ensemble x 365 days at dt = 0.1 (K = 3 650 Euler steps,
    SEIRP.m:26-32; the reference has no RK4 -- SURVEY.md 0).  Sampled members, and then all 10 000 (the oracle's simulator takes a
    member in well under a millisecond), equal the oracle bit for bit; the mass
    s + e + i + r + p stays 1 for EVERY member and step (a size-independent property: the right-hand sides sum to zero)."""
    import ctypes as C
    import torch
    from epidemicmodeling_amd import batch
    from oracle import oracle_lib as olib
    rng = np.random.default_rng(3)
    B, Tdays, dt = 10000, 365, 0.1
    K = int(round(Tdays / dt))
    assert K == 3650
    base = np.array([0.6, 0.005, 0.05, 0.08, 0.1, 0.02, 0.001])       # testSEIRP02.m:22-29
    par = (base[:, None] * np.exp(rng.uniform(np.log(0.5), np.log(2.0), (7, B))))[None]
    init = np.zeros((5, B)); init[1] = 1.0 / 84e6; init[0] = 1 - init[1]
    out = batch.seirp_sim(par, init, dt, K, device=gpu_device)
    assert float((out.sum(dim=1) - 1.0).abs().max()) < 1e-12
    lib = olib.lib()
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    for c in (0, 63, 64, 255, 256, 4999, 9999):
        cols = [np.full(K, par[0, j, c]) for j in range(7)]
        res = [np.zeros(K) for _ in range(5)]
        lib.orc_seirp(*[dp(v) for v in cols], *[C.c_double(init[q, c]) for q in range(5)], C.c_int(K), C.c_double(dt),
                      *[dp(v) for v in res])
        got = out[:, :, c].cpu().numpy()
        for q in range(5):
            assert np.array_equal(got[:, q], res[q]), (c, q)
    compared, step = 0, 500
    cols = [np.empty(K) for _ in range(7)]
    for lo in range(0, B, step):
        hi = min(B, lo + step)
        exp = np.zeros((hi - lo, 5, K))
        for c in range(lo, hi):
            for j in range(7):
                cols[j].fill(par[0, j, c])
            lib.orc_seirp(*[dp(v) for v in cols], *[C.c_double(init[q, c]) for q in range(5)], C.c_int(K), C.c_double(dt),
                          *[dp(exp[c - lo, q]) for q in range(5)])
        got = out[:, :, lo:hi].permute(2, 1, 0).contiguous().cpu().numpy()
        if not np.array_equal(got, exp, equal_nan=True):
            bad = np.argwhere(got != exp)
            raise AssertionError("members [%d, %d): %d words differ, first (member, state, step) %s" % (lo, hi, len(bad), (bad[0] + [lo, 0, 0]).tolist()))
        compared += hi - lo
    assert compared == B == 10000
    del out
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shape", SHAPES)
def test_mid_run_covariance_overflow_on_the_packed_path(gpu_device, shape):
    """One chain of a batch is driven into covariance overflow in mid-run (a costate variance of 1e305 that the costate
    map multiplies by (1 + gamma dt)^2 every day: A P A' exceeds 1.8e308 after about 25 days).  The packed kernels skip products with structural zeros, which is exact only for
    finite operands, so AFTER the overflow that chain's non-finite values need not sit where a dense evaluation puts them
     -- what must hold, and is checked against the oracle: every other chain of the batch stays bit-exact; the
    overflowing chain is bit-exact up to the day of the overflow; from then on P_MINUS is non-finite on both sides, the
    guard of GenericEKF.m:211 fires at exactly the same smoother steps (pinv_rank = -1), status bit 0 is set for that chain
    and for no other."""
    from epidemicmodeling_amd import synth
    w = synth.make_cfg4(3, 6, 40, 10)
    bad = 7
    w.Ps_init = w.Ps_init.copy()
    w.Ps_init[5 * 6 + 5, bad] = 1e305                  # var(lambda_3) grows by (1 + gamma dt)^2 per day: Inf after ~25 days
    ref = H.oracle_batch(w)
    got = _run(w, gpu_device, shape=shape, exact_nonfinite=False)          # opted out: what the fast kernels leave
    fin = np.isfinite(ref["P_MINUS"][:, :, bad]).all(axis=1)
    t_over = int(np.argmin(fin))                       # first day with a non-finite P(k|k-1)
    assert 0 < t_over < w.T - 5 and not fin[t_over:].any(), "the test input no longer overflows in mid-run"
    others = np.array([c for c in range(w.B) if c != bad])
    for n in H.OUT_NAMES:
        assert np.array_equal(got[n][..., others], ref[n][..., others], equal_nan=True), (shape, n)
    for n in ("S_MINUS", "P_MINUS", "S_PLUS", "P_PLUS", "K_GAIN", "innovations", "u_opt"):
        assert np.array_equal(got[n][:t_over - 1, ..., bad], ref[n][:t_over - 1, ..., bad], equal_nan=True), (shape, n)
    assert not np.isfinite(got["P_MINUS"][t_over:, :, bad]).all(axis=1).any()
    assert np.array_equal(got["pinv_rank"][:, bad] == -1, ref["pinv_rank"][:, bad] == -1)
    assert np.array_equal(got["pinv_rank"][:, others], ref["pinv_rank"][:, others])
    st = got["status"]
    assert (st[bad] & 1) == 1 and not (st[others] & 1).any()
    # epi_batch_desc.exact_nonfinite (round 4; the DEFAULT since round 5 / ABI 5): the marked chain is run again by the dense
    # kernels, in place -- now EVERY output of EVERY chain equals the oracle's, Inf / NaN pattern of the overflowed chain
    # included; a default-constructed descriptor, the explicit flag, classic and blocked layouts, all outputs and the reduced
    # set (whose forward quantities live in the workspace, upper triangles only)
    dflt = _run(w, gpu_device, shape=shape)
    for n in H.OUT_NAMES:
        assert np.array_equal(dflt[n], ref[n], equal_nan=True), (shape, n, "default descriptor")
    assert np.array_equal(dflt["pinv_rank"], ref["pinv_rank"])
    for blk in (0, "auto"):
        ex = _run(w, gpu_device, shape=shape, exact_nonfinite=True, lane_block=blk)
        for n in H.OUT_NAMES:
            assert np.array_equal(ex[n], ref[n], equal_nan=True), (shape, blk, n, "exact_nonfinite")
        assert np.array_equal(ex["pinv_rank"], ref["pinv_rank"])
        assert np.array_equal((ex["status"] & 1).astype(bool), H.oracle_guard_fired(ref, w.model))
    few = _run(w, gpu_device, shape=shape, exact_nonfinite=True, outputs=["u_opt_smooth", "S_SMOOTH"], lane_block="auto")
    for n in ("u_opt_smooth", "S_SMOOTH"):
        assert np.array_equal(few[n], ref[n], equal_nan=True), (shape, n, "exact_nonfinite, reduced outputs")
    # a host call always returns the dense evaluation's values
    hc = H.host_call(w, shape={"lane": 1, "quad": 2, "wave": 3, "hex": 4}[shape])
    for n in H.OUT_NAMES:
        assert np.array_equal(hc[n], ref[n], equal_nan=True), (shape, n, "host call")


def test_rccl_leg_of_the_end_of_sweep_gather_single_rank(gpu_device):
    """The only collective of the path over RCCL (backend "nccl"), as far as a one-GPU box allows: a world of ONE rank on
    the real backend.  batch.gather_shards_to_root / gather_to_root issue their collective for every world size, so here
    ncclAllGather (all_gather_into_tensor) and the gather really execute on the device -- the test counts the calls that
    reach torch.distributed and checks the gathered values, padding of a short shard included.  (Two ranks cannot share a
    GPU under RCCL; the ragged two-rank partition is covered over gloo in tests/test_distributed_cpu.py, the eight-rank
    run is the driver's.)"""
    import os
    import subprocess
    import sys
    code = (
        "import os, torch, torch.distributed as dist\n"
        "from epidemicmodeling_amd import batch\n"
        "os.environ.setdefault('MASTER_ADDR', '127.0.0.1'); os.environ.setdefault('MASTER_PORT', '29741')\n"
        "torch.cuda.set_device(0)\n"
        "dist.init_process_group('nccl', rank=0, world_size=1, device_id=torch.device('cuda', 0))\n"
        "calls = {'all_gather_into_tensor': 0, 'gather': 0}\n"
        "def counted(name):\n"
        "    orig = getattr(dist, name)\n"
        "    def f(*a, **k):\n"
        "        calls[name] += 1\n"
        "        return orig(*a, **k)\n"
        "    setattr(dist, name, f)\n"
        "counted('all_gather_into_tensor'); counted('gather')\n"
        "t = torch.arange(2 * 37, dtype=torch.float64, device='cuda:0').reshape(2, 37)\n"
        "full = batch.gather_shards_to_root(t, 37)\n"
        "assert calls['all_gather_into_tensor'] == 1, calls\n"
        "assert full is not None and full.data_ptr() != t.data_ptr() and torch.equal(full, t)\n"
        "parts = batch.gather_to_root(t)\n"
        "assert calls['gather'] == 1, calls\n"
        "assert len(parts) == 1 and parts[0].data_ptr() != t.data_ptr() and torch.equal(parts[0], t)\n"
        "torch.cuda.synchronize()\n"
        "dist.barrier(); dist.destroy_process_group(); print('rccl ok', calls)\n")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=H.ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=H.ROOT)
    assert r.returncode == 0 and "rccl ok" in r.stdout, r.stderr[-2000:]


@pytest.mark.gpu
def test_tune_placement_reallocates_and_keeps_the_results(gpu_device):
    """EkfRunner.tune_placement (round 5): outputs and workspace are allocated `tries` times, a staged pass is timed on each and
    the fastest allocation is kept -- the arrays the runner ends up with are live, bound to the library's descriptor, and a run
    into them gives the oracle's bits; run_sweep works afterwards (the staged timing leaves the descriptor's phase behind)."""
    import torch
    from epidemicmodeling_amd import batch, synth
    w = synth.make_cfg4(4, 25, 60, 20)
    dw = batch.DeviceWorkload(w, gpu_device)
    r = batch.EkfRunner(dw, extras=True, lane_block="auto")
    first = {n: t.data_ptr() for n, t in r.out.items()}
    rep = r.tune_placement(3)
    assert len(rep["tries"]) == 3 and 0 <= rep["chosen"] < 3 and all(t["sum_ms"] > 0 for t in rep["tries"])
    if rep["chosen"] != 0:
        assert any(r.out[n].data_ptr() != first[n] for n in first)
    for n, t in r.out.items():
        t.fill_(float("nan"))
    r.run()
    torch.cuda.synchronize()
    ref = H.oracle_batch(w)
    for n in H.OUT_NAMES:
        assert np.array_equal(r.unblocked(n).cpu().numpy(), ref[n], equal_nan=True), n
    B = w.B
    sp = torch.zeros((batch.SIM_PRM_COUNT, B), dtype=torch.float64, device=gpu_device)
    sp[0], sp[1], sp[2], sp[4], sp[5], sp[11] = 0.999, 1e-3, 1.0, 100.0, 1.0 / 7.0, 1.0
    z = torch.zeros(B, dtype=torch.float64, device=gpu_device)
    r.stage_ms(1)
    sc = r.run_sweep(60, sp, z, z, n_regions=4)
    torch.cuda.synchronize()
    assert np.array_equal(r.unblocked("u_opt_smooth").cpu().numpy(), ref["u_opt_smooth"], equal_nan=True)
    assert sc["J0"].shape == (B,)

"""Every NPI count 1..12 on every filter / smoother variant and entry point.

epi_batch_desc.n_npi accepts 1..12, and every kernel has its own code for the rows of u_opt / u_opt_smooth beyond n_npi:
a fast branch for 12 and per-row stores for the rest (store_u in epiekf.hip, st_u in ekf_lane6.hpp), store_rows_f32<kNpi>
for fp32 storage, and lane mappings whose boundaries sit at 4/5 and 8/9 (quad: lane q owns rows q, q+4, q+8), 6/7 (hex:
rows j, j+6), 9/10 (wave3: rows e, 9+e).  Each launch below is run for every n against the C oracle, bit for bit, NaN
patterns included, with every output poisoned (NaN) first: a row the kernel never writes shows up as a mismatch, a row it
writes too many lands in the next chain's or the next block's rows and does too."""
import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

NPIS = list(range(1, 13))
ENTRY_NPIS = [1, 5, 7, 11]


def _perturb(w, seed):
    """Missing observations on some historic days and free (NaN) controls inside the history as well as over the horizon
    (the bang-bang substitution then writes the n rows of u_opt / u_opt_smooth on days where only some lanes of a wave have
    free controls, and on days where all have)."""
    rng = np.random.default_rng(seed)
    w.x = w.x.copy()
    w.x[rng.random(w.x.shape) < 0.1] = np.nan
    if w.m == 6:
        w.u = w.u.copy()
        w.u[rng.random(w.u.shape) < 0.15] = np.nan
    return w


def _run(w, device, outputs=None, storage="f64", **kw):
    """One EkfRunner call on a poisoned output set: outputs and workspace NaN, pinv_rank -7, status -1 (guard bit set)."""
    import torch
    from epidemicmodeling_amd import batch
    r = batch.EkfRunner(batch.DeviceWorkload(w, device), outputs=outputs, extras=True, storage=storage, **kw)
    for t in list(r.out.values()) + [r.ws]:
        t.fill_(float("nan"))
    r.pinv_rank.fill_(-7)
    r.status.fill_(-1)
    r.run()
    torch.cuda.synchronize()
    got = {n: r.unblocked(n).cpu().numpy() for n in r.out}
    got["pinv_rank"] = r.unblocked("pinv_rank").cpu().numpy()
    got["status"] = r.status.cpu().numpy()
    return got, r


def _check(w, got, ref, tag, f32=False):
    n, B, T = w.n_npi, w.B, w.T
    for k in ("u_opt", "u_opt_smooth"):
        if k in got:
            assert got[k].shape == (T, n, B), (tag, k, got[k].shape)
    for k in H.OUT_NAMES:
        if k not in got:
            continue
        exp = ref[k].astype(np.float32) if f32 else ref[k]
        assert got[k].dtype == exp.dtype and got[k].shape == exp.shape, (tag, k)
        assert np.array_equal(got[k], exp, equal_nan=True), (tag, k)
    assert np.array_equal(got["pinv_rank"], ref["pinv_rank"]), (tag, "pinv_rank")
    if not w.model.startswith("NewCase"):
        assert np.array_equal((got["status"] & 1).astype(bool), H.oracle_guard_fired(ref, w.model)), (tag, "status")


# The 6-state generic model (SIAlphaModelEKFOptControlled and its time-flipped wrapper): (id, workload, EkfRunner arguments)
# with the launches each reaches, following plan_launch in csrc/launch_plan.hpp (tests/launch_plan_test.cpp asserts them).  Workloads: "b80" = 4
# regions x 20 cost weights (80 chains, two 40-chain blocks) x 40 days, "b70" = its first 70 chains, "dense" = b80 with a
# non-diagonal Q_w, "long" = 40 chains x 130 days (forward model only).
SIA6_LAUNCHES = [
    # ekf_fwd_sym (one lane per chain) + eks_bwd_sym<6>: store_u's per-row branch, classic layout
    ("lane-classic", "b80", dict(shape="lane")),
    # the same kernels on 8-chain blocks (blk is not a lane6 block)
    ("lane-blk8", "b80", dict(shape="lane", lane_block=8)),
    # eks_bwd_lane6<FLIP, 48, 0>: st_u's per-row branch, one 48-chain block and a ragged one
    ("lane-blk48", "b80", dict(shape="lane", lane_block=48)),
    # eks_bwd_lane6<FLIP, 56, 0>
    ("lane-blk56", "b80", dict(shape="lane", lane_block=56)),
    # eks_bwd_lane6<FLIP, 40, 1> (XD = 1, X of the next step by LDS-DMA): 80 chains = two workgroups, every lane alive
    ("lane-blk40-xd", "b80", dict(shape="lane", lane_block=40)),
    # eks_bwd_lane6<FLIP, 40, 0> (XD = 0): 70 chains are not a multiple of 40
    ("lane-blk40-ragged", "b70", dict(shape="lane", lane_block=40)),
    # test_flags bit 2: forward kernel and pinv grid in two chain ranges, the XD smoother in two launches with the monitor between
    ("lane-blk40-split", "b80", dict(shape="lane", lane_block=40, time_pipe=-1, test_flags=4)),
    # the XD smoother with 2-day addressing windows: a flush and a rebase at every window end
    ("lane-blk40-window2", "b80", dict(shape="lane", lane_block=40, test_window=2)),
    # ekf_fwd_quad<FLIP, 0, 0, ...> + eks_bwd_quad<FLIP, 0>: lane q stores rows q, q+4, q+8
    ("quad-classic", "b80", dict(shape="quad")),
    # ekf_fwd_quad<FLIP, kQC, 21, ...> + eks_bwd_quad<FLIP, kQC> on 16-chain blocks
    ("quad-blk16", "b80", dict(shape="quad", lane_block=16)),
    # ekf_fwd_wave + eks_bwd_wave: one wavefront per chain
    ("wave", "b80", dict(shape="wave")),
    # ekf_fwd_hex<FLIP, kHG, 1> + eks_bwd_hex<FLIP, kHG, 2> on 10-chain blocks: lane j stores rows j, j+6
    ("hex-blk10", "b80", dict(shape="hex", lane_block=10)),
    # ekf_fwd_hex<FLIP, 0, 1> + eks_bwd_hex<FLIP, 0, 1>, classic layout, 4-day addressing windows
    ("hex-classic-window4", "b80", dict(shape="hex", test_window=4)),
    # test_flags bit 0: the hex reverse-time pipeline (smoother in segments handing over through the hand-over rows), 4-day windows
    ("hex-reverse-pipe", "b80", dict(shape="hex", lane_block=10, test_window=4, test_flags=1)),
    # non-diagonal Q_w: the precheck sends the batch to the dense kernels ekf_fwd<6, FLIP, 1> + eks_bwd<6, FLIP, 1>
    ("dense", "dense", dict(shape="lane")),
    # T >= 128 with time_pipe = 1: the forward kernel in time segments, the pinv grid of each beside the next (40 chains in the
    # classic layout are one 40-chain block: the XD smoother)
    ("time-pipe", "long", dict(shape="lane", time_pipe=1)),
    # reduced outputs: u_opt_smooth alone (forward quantities in the workspace, upper triangles only; 80 chains run 64-lane waves, so
    # ekf_fwd_sym<6, FLIP, 0, 0, 0> -- the two-waves-per-SIMD variant needs waves of <= 40 lanes, tests/launch_plan_test.cpp), XD smoother
    ("reduced-u-blk40", "b80", dict(shape="lane", lane_block=40, outputs=["u_opt_smooth"])),
    # reduced outputs S_SMOOTH, u_opt_smooth, rho, classic layout
    ("reduced-3-classic", "b80", dict(shape="lane", outputs=["S_SMOOTH", "u_opt_smooth", "rho"])),
]


def _sia6_workloads(n, backward):
    from epidemicmodeling_amd import synth
    mk = lambda: synth.make_cfg4(4, 20, 30, 10)
    b80 = _perturb(H.with_npis(synth.as_backward(mk()) if backward else mk(), n), seed=n)
    dense = b80.select(np.arange(b80.B))
    dense.Q = dense.Q.copy()
    dense.Q[1] = 1e-13
    dense.Q[6] = 1e-13
    wl = {"b80": b80, "dense": dense}
    if not backward:
        wl["long"] = _perturb(H.with_npis(synth.make_cfg4(2, 20, 120, 10), n), seed=100 + n)
    return wl


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "flipped"])
@pytest.mark.parametrize("n", NPIS)
def test_sia6_every_launch(gpu_device, n, backward):
    wl = _sia6_workloads(n, backward)
    refs = {k: H.oracle_batch(w) for k, w in wl.items()}
    wl["b70"] = wl["b80"].select(np.arange(70))
    refs["b70"] = {k: v[..., :70] for k, v in refs["b80"].items()}
    for name, key, kw in SIA6_LAUNCHES:
        if key not in wl:
            continue
        w, ref = wl[key], refs[key]
        got, r = _run(w, gpu_device, **kw)
        if name.startswith("lane-blk40") and key == "b80":
            assert r.blk == 40 and w.B % 40 == 0 and w.B // 40 >= 2
        _check(w, got, ref, (n, w.model, name))


@pytest.mark.parametrize("n", NPIS)
def test_fp32_storage_every_npi_count(gpu_device, n):
    """storage = 1 (ekf_fwd_sym<M, FLIP, 0, 1> + eks_bwd_sym<M, FLIP, 1>, store_rows_f32<kNpi>): every output equals
    float32(oracle), 6- and 3-state, forward and flipped, classic and 8-chain blocked layouts."""
    from epidemicmodeling_amd import synth
    cases = [synth.make_cfg4(3, 10, 30, 8), synth.as_backward(synth.make_cfg4(3, 10, 30, 8)),
             synth.make_cfg3(30, 36), synth.as_backward(synth.make_cfg3(30, 36))]
    for i, w in enumerate(cases):
        w = _perturb(H.with_npis(w, n), seed=10 * n + i)
        ref = H.oracle_batch(w)
        for blk in (0, 8):
            got, _ = _run(w, gpu_device, storage="f32", shape="lane", lane_block=blk)
            _check(w, got, ref, (n, w.model, "f32", blk), f32=True)


@pytest.mark.parametrize("n", NPIS)
def test_sia3_lane_and_wave3(gpu_device, n):
    """The 3-state SIAlphaModelEKF (cfg3's one chain per region, cfg5's Monte-Carlo draws, the time-flipped wrapper): one lane
    per chain (ekf_fwd_sym<3> + eks_bwd_sym<3>, classic and 8-chain blocks) and seven chains per wavefront (ekf_fwd_wave3 +
    eks_bwd_wave3: lane e stores rows e and 9+e, so n = 9 / 10 is its boundary)."""
    from epidemicmodeling_amd import synth
    cases = [synth.make_cfg3(23, 40), synth.make_cfg5(2, 20, 36), synth.as_backward(synth.make_cfg3(15, 30))]
    for i, w in enumerate(cases):
        w = _perturb(H.with_npis(w, n), seed=20 * n + i)
        ref = H.oracle_batch(w)
        for kw in (dict(shape="lane"), dict(shape="lane", lane_block=8), dict(shape="wave"), dict(shape="wave", lane_block=7)):
            got, _ = _run(w, gpu_device, **kw)
            _check(w, got, ref, (n, w.model, kw))


@pytest.mark.parametrize("n", NPIS)
def test_newcase_dense_and_wave(gpu_device, n):
    """NewCaseEKFEstimatorWithOptimalNPI, plain and codegen: the dense kernels (ekf_fwd<6, 0, 0> + eks_bwd<6, 0, 0>) and one
    wavefront per chain (ekf_fwd_wave<0, 1, 21, 0> + eks_bwd_wave_nc: lane k < n_npi stores row k)."""
    from epidemicmodeling_amd import synth
    for codegen in (False, True):
        w = _perturb(H.with_npis(synth.make_row4(7, 40, 12, codegen=codegen), n), seed=30 * n + codegen)
        ref = H.oracle_batch(w)
        for kw in (dict(shape="lane"), dict(shape="wave"), dict(shape="wave", lane_block=8)):
            got, _ = _run(w, gpu_device, **kw)
            assert "u_opt" in got and "u_opt_smooth" not in got
            _check(w, got, ref, (n, w.model, codegen, kw))


def _scoring_inputs(w, rng):
    """sp [48, B] with SIM_A, SIM_U_MAX and SIM_W filled for the workload's n rows only, and the two prefix sums."""
    from epidemicmodeling_amd import batch, layout as L_, synth
    n, B = w.n_npi, w.B
    sp = np.zeros((batch.SIM_PRM_COUNT, B))
    sp[0] = 1.0 - 1e-3 * rng.random(B); sp[1] = 1e-3 * rng.random(B); sp[2] = synth.ALPHA0 * (0.5 + rng.random(B))
    sp[3] = w.prm[L_.PRM_ALPHA_MIN]; sp[4] = w.prm[L_.PRM_ALPHA_MAX]; sp[5] = w.prm[L_.PRM_GAMMA]
    sp[6] = w.prm[L_.PRM_B]; sp[7] = w.prm[L_.PRM_BETA]; sp[11] = 1.0
    sp[batch.SIM_A:batch.SIM_A + n] = w.prm[L_.PRM_A:L_.PRM_A + n]
    sp[batch.SIM_U_MAX:batch.SIM_U_MAX + n] = w.prm[L_.PRM_U_MAX:L_.PRM_U_MAX + n]
    sp[batch.SIM_W:batch.SIM_W + n] = rng.random((n, B)) + 0.5
    return sp, rng.random(B) * 1e-2, rng.random(B) * 40.0


@pytest.mark.parametrize("n", ENTRY_NPIS)
def test_sweep_entry_every_npi_count(gpu_device, n):
    """epi_sweep_run_device with n NPIs, with and without the Pareto filter, on 40-chain blocks (80 chains: the XD smoother,
    and the scoring tail reading the blocked u_opt_smooth with n rows per block) and on the library's own layout: filter
    outputs equal the oracle's; (J0, J1), front and I_opt equal the separate scoring / filter calls on the same u_opt_smooth
    and the scoring of the oracle's u_opt_smooth in the classic layout."""
    import torch
    from epidemicmodeling_amd import batch, synth
    R, T_hist = 2, 30
    w = _perturb(H.with_npis(synth.make_cfg4(R, 40, T_hist, 11), n), seed=40 + n)
    B = w.B
    rng = np.random.default_rng(n)
    sp, j0p, j1p = _scoring_inputs(w, rng)
    to = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(gpu_device)
    sp_d, j0_d, j1_d = to(sp), to(j0p), to(j1p)
    ref = H.oracle_batch(w)
    sc_ref = batch.score_sweep(to(ref["u_opt_smooth"]), T_hist, sp_d, j0_d, j1_d)
    on_ref, io_ref = batch.pareto_front(sc_ref["J0"], sc_ref["J1"], R)
    dw = batch.DeviceWorkload(w, gpu_device)
    for lane_block in (40, "auto"):
        for with_front in (False, True):
            tag = (n, lane_block, with_front)
            r = batch.EkfRunner(dw, extras=True, lane_block=lane_block, shape="lane" if lane_block == 40 else 0)
            if lane_block == 40:
                assert r.blk == 40 and B % 40 == 0
            for t in list(r.out.values()) + [r.ws]:
                t.fill_(float("nan"))
            sc = r.run_sweep(T_hist, sp_d, j0_d, j1_d, n_regions=R if with_front else None)
            torch.cuda.synchronize()
            for k in r.out:
                assert np.array_equal(r.unblocked(k).cpu().numpy(), ref[k], equal_nan=True), (tag, k)
            assert np.array_equal(r.unblocked("pinv_rank").cpu().numpy(), ref["pinv_rank"]), tag
            J0, J1 = sc["J0"].clone(), sc["J1"].clone()
            sc2 = batch.score_sweep(r.out["u_opt_smooth"], T_hist, sp_d, j0_d, j1_d, B=B)
            assert torch.equal(J0, sc2["J0"]) and torch.equal(J1, sc2["J1"]), tag
            assert torch.equal(J0, sc_ref["J0"]) and torch.equal(J1, sc_ref["J1"]), tag
            if with_front:
                on2, io2 = batch.pareto_front(sc2["J0"], sc2["J1"], R)
                assert torch.equal(sc["on_front"].bool(), on2) and torch.equal(sc["i_opt"], io2), tag
                assert torch.equal(on2, on_ref) and torch.equal(io2, io_ref), tag


@pytest.mark.parametrize("n", ENTRY_NPIS)
def test_host_sweep_entry_every_npi_count(gpu_device, n):
    """epi_sweep_prescribe_host with n NPIs (per-region host arrays): against the chain of device calls on the expanded
    per-chain workload, filter outputs also against the oracle -- one device and the regions cut into three blocks."""
    import torch
    from epidemicmodeling_amd import batch, hostapi
    from tests.test_gpu_parity import _region_sweep_problem
    S, P, T_hist, hor = 5, 9, 40, 12
    pr = _region_sweep_problem(S, P, T_hist, hor, seed=n, n=n)
    w6 = pr["w6"]
    assert w6.n_npi == n and pr["u"].shape == (T_hist + hor, n, S)
    ref = H.oracle_batch(w6)
    rr = np.repeat(np.arange(S), P)
    r0 = batch.EkfRunner(batch.DeviceWorkload(w6, gpu_device), outputs=["u_opt_smooth", "S_SMOOTH"])
    to = lambda v: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64).to(gpu_device)
    sc = r0.run_sweep(T_hist, to(pr["sp"][:, rr]), to(pr["J0p"][rr]), to(pr["J1p"][rr]), n_regions=S)
    torch.cuda.synchronize()
    assert np.array_equal(r0.out["u_opt_smooth"].cpu().numpy(), ref["u_opt_smooth"], equal_nan=True)
    J0 = sc["J0"].cpu().numpy().reshape(S, P); J1 = sc["J1"].cpu().numpy().reshape(S, P)
    io = sc["i_opt"].cpu().numpy(); on = sc["on_front"].bool().cpu().numpy()
    chains = np.arange(S) * P + io
    for devices, extras in (((0,), ()), ((0, 0, 0), ("u_opt_smooth", "S_SMOOTH", "rho"))):
        got = hostapi.sweep_prescribe(pr["x"], pr["u"], pr["R"], pr["reg"], pr["eps"], pr["sp"], pr["J0p"], pr["J1p"], T_hist,
                                      devices=devices, extras=extras)
        tag = (n, devices, extras)
        assert np.array_equal(got["J0"], J0) and np.array_equal(got["J1"], J1), tag
        assert np.array_equal(got["on_front"], on) and np.array_equal(got["i_opt"], io), tag
        assert got["u_opt"].shape == (T_hist + hor, n, S), tag
        assert np.array_equal(got["u_opt"], ref["u_opt_smooth"][:, :, chains]), tag
        assert np.array_equal(got["S_opt"], ref["S_SMOOTH"][:, :, chains], equal_nan=True), tag
        for k in extras:
            assert np.array_equal(got[k], ref[k], equal_nan=True), (tag, k)


@pytest.mark.parametrize("n", ENTRY_NPIS)
def test_tools_calls_every_npi_count(gpu_device, n):
    """The Tools/-named functions with an n x T u: SIAlphaModelEKFOptControlled and NewCaseEKFEstimatorWithOptimalNPI equal
    the oracle called with the same MATLAB-shaped arguments, bit for bit."""
    from epidemicmodeling_amd import synth, tools
    from oracle import oracle_lib as olib
    w_eff = np.zeros(12); w_eff[:n] = 1.0
    for fn, w, names in ((tools.SIAlphaModelEKFOptControlled, synth.make_cfg4(2, 3, 40, 15), H.OUT_NAMES),
                         (tools.NewCaseEKFEstimatorWithOptimalNPI, synth.make_row4(1, 50, 20),
                          [k for k in H.OUT_NAMES if k != "u_opt_smooth"])):
        w = _perturb(H.with_npis(w, n), seed=50 + n)
        args = H.chain_args(w, w.B - 1)
        u, x, p = args[0], args[1], args[2]
        assert u.shape == (n, w.T)
        params = dict(dt=p.dt, a=p.a, b=p.b, u_min=p.u_min, u_max=p.u_max, alpha_min=p.alpha_min, alpha_max=p.alpha_max,
                      gamma=p.gamma, beta=p.beta, sigma=p.sigma, epsilon=p.epsilon, w=np.ones((1, n)), obs_type="NEWCASES")
        got = fn(u, x.reshape(1, -1), params, *args[3:])
        ref = olib.run(w.model, u, x, params, w_eff, *args[3:7], args[8], *args[9:])
        assert len(got) == len(names) and np.shape(got[0]) == (n, w.T)
        for k, g in zip(names, got):
            assert np.array_equal(np.asarray(g).reshape(-1), np.asarray(ref[k]).reshape(-1), equal_nan=True), (n, w.model, k)

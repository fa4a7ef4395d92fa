"""The straight-line path of eks_bwd_lane6 (ekf_lane6.hpp) for a day on which EVERY control of every live lane of a wave is free --
the horizon days of the sweep -- against the oracle, bit for bit, beside the general path (some control of some lane free) and the
skip (none free), which must keep giving the oracle's bits.  Lane shape and lane block are forced through the descriptor as
test_lane6_fixed_descriptor_kernels does; a batch of B chains on lane block BLK runs eks_bwd_lane6<., BLK, XD> with XD = 1 (X of
the next step by LDS-DMA) exactly when B is a multiple of BLK.  Batches are a few dozen chains x 12 days (7 observed, 5 free).

Two things the launch plan decides and a test cannot force:
  * the phi >= 0 flag belongs to the NewCase models, which are not `generic` and never take the fixed-descriptor smoother
    (launch_plan.hpp: lane6_ok) -- that case runs here on the layout of 40 and checks whichever smoother the plan picks;
  * time_pipe = 1 cuts the FORWARD kernel in time and engages from 128 days; the fixed-descriptor smoother resumes from hand-over
    rows where the sweep entry cuts it for the scoring tail, at the t_hist the call is given -- so the hand-over is put inside the
    free days by giving the entry a later t_hist than the day the controls become free.  A 130-day time_pipe = 1 run is kept too."""
import copy

import numpy as np
import pytest

from tests import helpers as H

T_HIST, HORIZON = 7, 5
_refs = {}


def _per_chain_controls(w):
    """The same workload with a control series per chain (u [T][n_npi][B], identity u_series), so that one chain's can be edited."""
    w2 = copy.copy(w)
    w2.u = np.ascontiguousarray(w.u[:, :, w.u_series])
    w2.u_series = None
    return w2


def _sweep(B):
    from epidemicmodeling_amd import synth
    n_eps = 10 if B % 10 == 0 else B
    return synth.make_cfg4(B // n_eps, n_eps, T_HIST, HORIZON)


def _crossing(B=40):
    """Costates on both sides of every control's switching point and slope intervals of both widths in ONE wave: epsilon = 1/2,
    lambda_3 (state 6) spread over +-3 x the switching value epsilon / (gamma mean|a|) along the chains at the start and, reversed,
    at the terminal condition; sigma alternates between 1/4 (|phi| < 4: most controls inside the slope interval) and 64."""
    from epidemicmodeling_amd import layout as L_, synth
    w = _sweep(B)
    w.prm = w.prm.copy(); w.s_init = w.s_init.copy(); w.s_final = w.s_final.copy()
    c = np.arange(B)
    w.prm[L_.PRM_EPSILON] = 0.5
    w.prm[L_.PRM_SIGMA] = np.where(c % 2 == 0, 0.25, 64.0)
    a_mean = np.abs(w.prm[L_.PRM_A:L_.PRM_A + 12]).mean(axis=0)
    spread = np.linspace(-3.0, 3.0, B) * 0.5 / (synth.MODEL_GAMMA * a_mean)
    w.s_init[5] = spread
    w.s_final[5] = spread[::-1]
    return w


def _phi(w, S, day, c):
    """phi(k) of OptControlled.m:50 from a state the oracle wrote, the operations of resolve_control()"""
    from epidemicmodeling_amd import layout as L_
    gs6 = w.prm[L_.PRM_GAMMA, c] * S[day, 5, c]
    return w.prm[L_.PRM_EPSILON, c] * w.prm[L_.PRM_W_EFF:L_.PRM_W_EFF + 12, c] - gs6 * w.prm[L_.PRM_A:L_.PRM_A + 12, c]


def _cases():
    from epidemicmodeling_amd import synth
    out = {}
    # the new path on full waves (DMA image) at 40 / 48 / 56, and at 41 chains: a partial last workgroup, no DMA
    for B, blk in ((40, 40), (48, 48), (56, 56), (41, 40)):
        out["full-%d-blk%d" % (B, blk)] = (lambda B=B: _sweep(B), dict(lane_block=blk))
    # the mixed case: one chain with ONE finite control on one free day / one chain whose controls are all finite
    def one_finite():
        w = _per_chain_controls(_sweep(40))
        w.u[T_HIST + 2, 4, 17] = 1.0
        return w
    def one_chain_finite():
        w = _per_chain_controls(_sweep(40))
        w.u[T_HIST:, :, 23] = w.u[T_HIST - 1, :, 23]
        return w
    out["mixed-one-control"] = (one_finite, dict(lane_block=40))
    out["mixed-one-chain"] = (one_chain_finite, dict(lane_block=40))
    for n in (1, 11, 12):
        out["npi-%d" % n] = (lambda n=n: H.with_npis(_sweep(40), n), dict(lane_block=40))
    out["time-flipped"] = (lambda: synth.as_backward(_sweep(40)), dict(lane_block=40))
    out["time-flipped-41"] = (lambda: synth.as_backward(_sweep(41)), dict(lane_block=40))
    out["phi-ge"] = (lambda: synth.make_newcase_sweep(4, 10, T_HIST, HORIZON), dict(lane_block=40))
    out["window-2"] = (lambda: _sweep(40), dict(lane_block=40, test_window=2))
    out["two-ranges"] = (lambda: _sweep(80), dict(lane_block=40, test_flags=4, time_pipe=-1))
    out["two-ranges-ragged"] = (lambda: _sweep(90), dict(lane_block=40, test_flags=4, time_pipe=-1))
    out["time-pipe-1"] = (lambda: synth.make_cfg4(4, 10, 123, 7), dict(lane_block=40, time_pipe=1))
    out["crossing"] = (lambda: _crossing(40), dict(lane_block=40))
    out["crossing-48"] = (lambda: _crossing(48), dict(lane_block=48))
    return out


CASES = _cases()


def _ref(name):
    if name not in _refs:
        w = CASES[name][0]()
        _refs[name] = (w, H.oracle_batch(w))
    return _refs[name]


def _free_days(w):
    """per (day, series): is every / is some control free?"""
    nan = np.isnan(w.u)
    return nan.all(axis=1), nan.any(axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_lane6_horizon_path_matches_the_oracle(gpu_device, name):
    from epidemicmodeling_amd import batch
    w, ref = _ref(name)
    every, some = _free_days(w)
    assert every[-HORIZON:].all(axis=0).any() and not some[:3].any()          # days of both kinds
    if name.startswith("npi-") and w.n_npi < 12:
        assert w.n_npi in (1, 11)        # (rows beyond n_npi are padded with 0.0, not NaN: such a batch keeps the general path)
    if name == "mixed-one-control":
        assert some[T_HIST + 2, 17] and not every[T_HIST + 2, 17] and every[T_HIST + 2].sum() == w.B - 1
    if name == "mixed-one-chain":
        assert not some[:, 23].any() and every[T_HIST:, :23].all() and every[T_HIST:, 24:].all()
    got = batch.run_workload(w, device=gpu_device, shape="lane", **CASES[name][1])
    for n in H.OUT_NAMES:
        if n in ref and n in got:        # (the NewCase models have no u_opt_smooth)
            assert np.array_equal(got[n], ref[n], equal_nan=True), (name, n)
    assert np.array_equal(got["pinv_rank"], ref["pinv_rank"]), name


def test_crossing_case_reaches_both_sides_of_every_test():
    """What the `crossing` batches are for, asserted on the oracle's own outputs (no GPU): over the free days of ONE wave the first
    substitution and the slope term (phi from s(k|k)) and the second substitution (phi from the smoothed state) each see controls at
    u_min and at u_max, and the slope interval holds some controls and not others -- in every one of those days' columns, so a
    lane-uniform shortcut would show."""
    for name in ("crossing", "crossing-48"):
        w, ref = _ref(name)
        from epidemicmodeling_amd import layout as L_
        inv_sigma = 1.0 / w.prm[L_.PRM_SIGMA]
        for day in range(T_HIST, w.T - 1):              # the smoother's steps over free days
            for S in (ref["S_PLUS"], ref["S_SMOOTH"]):
                phi = np.stack([_phi(w, S, day, c) for c in range(w.B)], axis=1)        # [12][B]
                lo = phi > 0.0
                assert lo.any() and (~lo).any(), (name, day)
            phi = np.stack([_phi(w, ref["S_PLUS"], day, c) for c in range(w.B)], axis=1)
            inside = (phi > -inv_sigma) & (phi < inv_sigma)
            assert inside.any() and (~inside).any(), (name, day)
        uos = ref["u_opt_smooth"][T_HIST:w.T - 1]
        u_min = w.prm[L_.PRM_U_MIN:L_.PRM_U_MIN + 12][None]
        u_max = w.prm[L_.PRM_U_MAX:L_.PRM_U_MAX + 12][None]
        assert (uos == u_min).any() and (uos == u_max).any() and ((uos == u_min) | (uos == u_max)).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("t_cut", [T_HIST + 2, T_HIST])
def test_lane6_smoother_resumed_inside_the_free_days(gpu_device, t_cut):
    """The sweep entry cuts the smoother at the t_hist it is given and resumes it from the hand-over rows: with t_hist two days
    INSIDE the free days the first launch ends and the second begins on an all-free day (and with the cut on the boundary the second
    begins on the last observed day).  Filter outputs against the oracle, the scores against the separate scoring call."""
    import torch
    from epidemicmodeling_amd import batch
    from tests.test_gpu_parity import _sweep_params
    w, ref = _ref("full-40-blk40")
    r = batch.EkfRunner(batch.DeviceWorkload(w, gpu_device), extras=True, lane_block=40, shape="lane")
    sp, j0, j1 = _sweep_params(w, gpu_device)
    for t in list(r.out.values()) + [r.ws]:
        t.fill_(float("nan"))
    sc = r.run_sweep(t_cut, sp, j0, j1, n_regions=4)
    torch.cuda.synchronize()
    for n in r.out:
        assert np.array_equal(r.unblocked(n).cpu().numpy(), ref[n], equal_nan=True), (t_cut, n)
    assert np.array_equal(r.unblocked("pinv_rank").cpu().numpy(), ref["pinv_rank"])
    sc2 = batch.score_sweep(r.out["u_opt_smooth"], t_cut, sp, j0, j1, B=w.B)
    assert torch.equal(sc["J0"], sc2["J0"]) and torch.equal(sc["J1"], sc2["J1"])

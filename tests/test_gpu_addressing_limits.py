"""Every kernel family at the edges of its 32-bit addressing, the calls around the filter at their batch-count limits, and the
rejections beyond them.

The filter / smoother kernels address memory through buffer descriptors and 32-bit byte offsets.  The limits that keep
this safe are written into epi_ekf_validate (epiekf.hip), shape_of and plan_launch (launch_plan.hpp) and into lw_window / hx_window
(ekf_lane6.hpp, ekf_hex.hpp); here each is run AT its value.  An offset that wraps, or a store the descriptor's bounds
check drops, gives plausible numbers for the wrong chain or leaves the output untouched, so every case follows three rules:

 1. inputs distinct per chain, by formula (helpers.FormulaBatch: evaluated by torch on the device for the whole batch and by
    NumPy for the sampled chains, the two compared bit for bit before the run);
 2. outputs, workspace, pinv_rank and status poisoned (a NaN with a payload no arithmetic produces), and after the run no
    word of any selected output of the WHOLE batch may still hold the poison;
 3. the chains compared with the C oracle, bit for bit and on every day, sit where the offsets are extreme
    (helpers.extreme_sample), and the test asserts that its sample holds each class it relies on.

Device memory of a case is estimated before it allocates; too little free memory fails the case with the numbers.

Measured on one MI355X (torch.cuda.max_memory_allocated, wall time of the case): 2^20 chains x 14 days, all 11 outputs
21.8 GiB, the reduced three 15.7 GiB; 2^23 chains x 3 days, all outputs with n_npi = 1 46.3 - 46.5 GiB, the reduced three
38.6 - 41.2 GiB; the 3-state model at 2^23 x 8 days 43.7 GiB; fp32 storage at 2^23 (fp64 workspace included) 49.5 - 51.6
GiB, the largest of the module; rt_window 39 / 26 GiB, LASSO 25 GiB.  Every filter call is below 0.1 s, a case 0.1 - 1.5 s
(1 - 6 s more where a fresh 40 GiB allocation is slow: another case every run); the module 23 - 37 s."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

REDUCED = ["S_SMOOTH", "u_opt_smooth", "rho"]
LW_RECORDS = 0x7FFFFFF8          # kLwRecords / kHexRecords: the record count of a fixed descriptor, just below 2 GiB


def lane_window(bp):
    """lw_window (ekf_lane6.hpp) with test_window = 0: days per addressing window of the fixed-descriptor one-lane smoother."""
    return max(2, LW_RECORDS // (bp * 288) - 3)


def hex_window(bp, n_npi, Su):
    """hx_window (ekf_hex.hpp) with test_window = 0."""
    w = LW_RECORDS // max(bp * 288, n_npi * Su * 8) - 3
    return 2 if w < 2 else w & ~1


def _base(n_npi, T_hist, horizon, S=16, kind="sia6"):
    """S regions, one chain each, identity series: the headline sweep's parameterisation (sia6; sia6b: its time-flipped
    wrapper), BASELINE config 3 (sia3: the 3-state model, no horizon) or testSIModelOptimalControl04EKS's
    NewCaseEKFEstimatorWithOptimalNPI (newcase: scalar adaptive R_v, dense kernels)."""
    from epidemicmodeling_amd import synth
    if kind == "sia3":
        w = synth.make_cfg3(S, T_hist + horizon)
    elif kind == "newcase":
        w = synth.make_row4(S, T_hist + horizon, horizon)
    else:
        w = synth.make_cfg4(S, 1, T_hist, horizon)
        if kind == "sia6b":
            w = synth.as_backward(w)
    w = H.with_npis(w, n_npi) if n_npi < 12 else w
    w.x_series = w.u_series = None
    return w


def _need_bytes(B, T, m, n, outputs, blocked_pad=1.0):
    names = H.OUT_NAMES if outputs is None else outputs
    rows = {"u_opt": n, "u_opt_smooth": n, "S_MINUS": m, "S_PLUS": m, "S_SMOOTH": m, "P_MINUS": m * m, "P_PLUS": m * m,
            "P_SMOOTH": m * m, "K_GAIN": m, "innovations": 1, "rho": 1}
    per_day = sum(rows[k] for k in names)
    per_day += sum(rows[k] for k in ("S_MINUS", "S_PLUS", "P_MINUS", "P_PLUS", "innovations") if k not in names)   # workspace
    per_day += m * (m + 1) // 2 + 1                     # packed X, rank word and pinv_rank
    per_chain = (L_PRM + 2 * m + 3 * m * m + 3 * m + m * m + 4) * 8       # inputs, hand-over rows, second-pass lists
    return int(B * blocked_pad * (T * per_day * 8 + per_chain) * 1.15) + (1 << 30)      # + the survivors check's masks


L_PRM = 61


def run_case(device, fb, idx, classes, outputs=None, oracle_threads=16, dense=False, extra_bytes=0, **kw):
    """One poisoned EkfRunner call on FormulaBatch `fb` with the three rules above.  dense: path_hint = 2 (the dense kernels
    for a batch that would qualify for the packed ones).  Chains planted with fb.plant must be the only ones whose status
    carries the guard bit.  Returns (runner facts, seconds, peak bytes)."""
    import torch
    from epidemicmodeling_amd import _lib, batch
    b = fb.base
    f32 = kw.get("storage") == "f32"
    need = _need_bytes(fb.B, b.T, b.m, b.n_npi, outputs) + int(extra_bytes)
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info(device)
    if free < need:
        pytest.fail(f"needs ~{need / 2**30:.1f} GiB of device memory, {free / 2**30:.1f} of {total / 2**30:.1f} GiB are free")
    torch.cuda.reset_peak_memory_stats(device)
    t0 = time.perf_counter()
    # rule 1: the sample and its neighbours at +-1, +-blk, +-2^k have pairwise different inputs, and the device's evaluation
    # of the closed forms equals the host's on the sample
    blk = kw.get("lane_block", 0) or 0
    steps = [1] + ([blk] if isinstance(blk, int) and blk > 1 else []) + [1 << k for k in range(1, 23)]
    nb = np.unique(np.concatenate([idx] + [idx + s for s in steps] + [idx - s for s in steps]))
    nb = nb[(nb >= 0) & (nb < fb.B)]
    wn = fb.host_workload(nb)
    key = np.concatenate([wn.prm, wn.s_init, wn.Ps_init], axis=0)
    assert np.unique(key, axis=1).shape[1] == nb.size, "two chains of the sample's neighbourhood share their inputs"
    ws = fb.host_workload(idx)
    dw = fb.device_workload(device)
    for k, v in fb.inputs_of(dw, idx).items():
        exp = ws.u[:, :, ws.u_series] if k == "u_of_chain" else getattr(ws, k)
        assert np.array_equal(v, exp, equal_nan=True), ("device and host evaluate the input formula differently", k)
    ref = H.oracle_batch(ws, n_threads=oracle_threads)
    r = batch.EkfRunner(dw, outputs=outputs, extras=True, precheck=not dense, **kw)
    if dense:
        r.desc.path_hint = 2
    H.poison_runner(r)
    r.run()
    torch.cuda.synchronize()
    # rule 2, over the whole batch
    left = H.surviving_poison(r)
    assert not left, ("outputs that still hold the poison pattern (words)", left, kw)
    # rule 3
    for k in list(r.out) + ["pinv_rank"]:
        got = H.sampled_output(r, k, idx)
        exp = ref[k].astype(np.float32) if f32 and k != "pinv_rank" else ref[k]
        assert got.dtype == exp.dtype, (k, got.dtype)
        if not np.array_equal(got, exp, equal_nan=True):
            same = (got == exp) | (np.isnan(got) & np.isnan(exp))
            bad = np.flatnonzero(~np.all(same.reshape(got.shape[0], -1, idx.size), axis=(0, 1)))
            days = np.flatnonzero(~np.all(same.reshape(got.shape[0], -1), axis=1))
            raise AssertionError((k, kw, "chains", idx[bad][:12].tolist(), "days", days[:12].tolist(),
                                  {c: v for c, v in classes.items() if c != "spread" and set(v) & set(idx[bad].tolist())}))
    st = r.status.index_select(0, torch.as_tensor(idx, device=device)).cpu().numpy()
    if not b.model.startswith("NewCase"):
        assert np.array_equal((st & 1).astype(bool), H.oracle_guard_fired(ref, b.model)), "status bit 0"
        flagged = torch.nonzero(r.status & 1).reshape(-1).cpu().numpy()
        assert np.array_equal(flagged, np.unique([p[0] for p in fb.planted])), ("chains with the guard bit", flagged[:12])
    probe = _lib.BatchDesc.from_buffer_copy(r.desc)
    facts = {"blk": r.blk, "nblk": r.nblk, "padded": r.blk * r.nblk, "ref": ref,
             "chains_per_wave": int(_lib.lib().epi_ekf_preferred_lane_block(C.byref(probe)))}
    peak = torch.cuda.max_memory_allocated(device)
    del r, dw
    torch.cuda.empty_cache()
    dt = time.perf_counter() - t0
    print(f"[addressing] B={fb.B} T={b.T} n_npi={b.n_npi} {kw} outputs={'all' if outputs is None else len(outputs)}: "
          f"{dt:.1f} s, peak {peak / 2**30:.1f} GiB, sample {idx.size}")
    return facts, dt, peak


# ------------------------------------------------------------------------------------------------------------------ A1
# eks_bwd_lane6 runs while blk * nblk <= 2^20 (enqueue_bwd); one block more and eks_bwd_sym<6> takes the batch.  The library
# reports no kernel names, so which smoother ran is asserted through the guard's own operands (blk * nblk of the runner).
A1 = [  # id, lane_block, B, outputs
    # 26 214 blocks of 40, every lane alive: eks_bwd_lane6<FLIP, 40, 1> (XD = 1: X by LDS-DMA); all 11 outputs, ~19 GB
    ("blk40-at-guard-xd-all", 40, 1048560, None),
    # the same padded batch, the last block ragged: XD = 0
    ("blk40-at-guard-ragged-all", 40, 1048560 - 13, None),
    # the reduced selection: the unselected outputs have empty descriptors, the forward quantities live in the workspace
    ("blk40-at-guard-xd-reduced", 40, 1048560, REDUCED),
    # one block beyond the guard: eks_bwd_sym<6>, per-day descriptors
    ("blk40-beyond-guard-all", 40, 1048560 + 40, None),
    ("blk48-at-guard-all", 48, 1048560, None),
    ("blk56-at-guard-all", 56, 1048544, None),
]


@pytest.mark.parametrize("blk,B,outputs", [c[1:] for c in A1], ids=[c[0] for c in A1])
def test_one_lane_fixed_descriptor_smoother_at_its_guard(gpu_device, blk, B, outputs):
    """shape = lane on 40 / 48 / 56-chain blocks with the padded batch at the largest multiple of the block <= 2^20 (and one
    block beyond), 14 days, test_window = 0: the natural addressing window is 4 days (asserted from lw_window's formula), so
    the run has windows of 4, 4, 4 and 2 days.  21.8 GiB and 0.1 - 0.8 s per all-outputs case on an MI355X.  With `- 3`
    replaced by `- 1` in lw_window (a scratch build) the all-outputs cases fail here: 33.5 M words of P_SMOOTH keep the
    poison, no fault -- the descriptor's bounds check drops the stores beyond the record count."""
    T_hist, hor = 10, 4
    padded = (B + blk - 1) // blk * blk
    at_guard = padded <= (1 << 20)
    assert padded + blk > (1 << 20) >= padded - blk, "the batch is neither at the guard nor one block beyond it"
    w = lane_window(padded)
    assert w == 4 and (T_hist + hor) // w >= 3 and (T_hist + hor) % w != 0, w
    # the widest offset a window reaches (its last day, the prefetched day beyond it, the last chain's last row) stays below the
    # record count, and one window more would not
    assert (w + 2) * padded * 288 <= LW_RECORDS < (w + 4) * padded * 288
    fb = H.FormulaBatch(_base(12, T_hist, hor), B)
    idx, cls = H.extreme_sample(B, blk, units=(blk, 64, 4 * blk, 4096, 65536))
    assert {0, 1, B - 2, B - 1} <= set(idx.tolist()) and cls["unit%d" % blk]
    facts, _, _ = run_case(gpu_device, fb, idx, cls, outputs=outputs, shape="lane", lane_block=blk, test_window=0)
    assert facts["blk"] == blk and facts["padded"] == padded
    assert (facts["padded"] <= (1 << 20)) == at_guard       # lane6 at the guard, eks_bwd_sym<6> beyond it


# ------------------------------------------------------------------------------------------------------------------ A2
A2 = [  # id, B, lane_block, T_hist, horizon, outputs
    # 2^20 chains on 10-chain blocks: the last wavefront holds 6 live chains and 4 dead groups (bit-31 offsets beside live
    # offsets near 2^31); eks_bwd_hex<FLIP, kHG, 0> (two waves per SIMD)
    ("2^20-blk10-all", 1 << 20, 10, 10, 4, None),
    # classic layout, every wavefront full
    ("2^20-6-classic-all", (1 << 20) - 6, 0, 10, 4, None),
    # a production-sized hex batch whose natural window ends: 20 480 chains x 760 days (windows of 360, 360 and 40 days)
    ("20480-natural-windows", 20480, 10, 600, 160, REDUCED),
]


@pytest.mark.parametrize("B,blk,T_hist,hor,outputs", [c[1:] for c in A2], ids=[c[0] for c in A2])
def test_hex_shape_forced_to_its_limit(gpu_device, B, blk, T_hist, hor, outputs):
    """shape = hex at shape_of's limit B = 2^20 and at the natural second window of a 20 480-chain batch, test_window = 0."""
    T = T_hist + hor
    bp = (B + blk - 1) // blk * blk if blk else B
    w = hex_window(bp, 12, 16)
    assert w == (4 if B > 20480 else 360), w
    assert T // w >= (3 if B > 20480 else 2) and T % w != 0
    assert bp * T * 288 > (1 << 31)
    fb = H.FormulaBatch(_base(12, T_hist, hor), B)
    idx, cls = H.extreme_sample(B, blk or B, units=(10, 64, 640, 4096, 65536), n_spread=200 if B > 20480 else 120)
    assert B - 1 in idx and B - 7 in idx or B <= 20480 or blk == 0
    facts, _, _ = run_case(gpu_device, fb, idx, cls, outputs=outputs, shape="hex", lane_block=blk, test_window=0)
    assert facts["chains_per_wave"] == 10          # shape_of kept the hex shape (kHG chains per wavefront)


# ------------------------------------------------------------------------------------------------------------------ A3
A3 = [  # id, shape, lane_block, n_npi, x_mode, u_mode, outputs, time_pipe
    # a 36-row day slice is 2.25 GiB: offsets with bit 31 set, in every kernel that takes per-day descriptors
    ("quad-classic-n1-shared-all", "quad", 0, 1, "one", "one", None, 0),
    ("quad-blk16-n12-own", "quad", 16, 12, "own", "own", REDUCED, 0),
    ("lane-classic-n12-own-x-shared-u", "lane", 0, 12, "own", "one", REDUCED, -1),
    ("lane-blk64-n1-own-all", "lane", 64, 1, "one", "own", None, 0),
]


@pytest.mark.parametrize("shape,blk,n,x_mode,u_mode,outputs,time_pipe", [c[1:] for c in A3], ids=[c[0] for c in A3])
def test_per_day_descriptor_kernels_at_validates_limit(gpu_device, shape, blk, n, x_mode, u_mode, outputs, time_pipe):
    """B = 2^23 = padded B (epi_ekf_validate's limit), 3 days, forward + smoother: shape = quad and shape = lane (eks_bwd_sym<6>:
    64 is no lane6 block and 2^23 is beyond its guard), classic and blocked, one shared series (Sx = Su = 1) and one per chain
    (Sx = Su = B), n_npi 1 and 12.  All 11 outputs with n_npi = 1 are ~45 GB with the workspace."""
    B = 1 << 23
    fb = H.FormulaBatch(_base(n, 2, 1), B, x_mode=x_mode, u_mode=u_mode)
    idx, cls = H.extreme_sample(B, blk or B, units=(blk or 16, 16, 64, 256, 4096, 65536))
    # the sample holds a chain whose offset in a day of the 36-row array has bit 31 set
    off = H.chain_offsets(idx, 36, B, blk or B)
    assert "rows36_bit31" in cls and (off >= (1 << 31)).any() and (off < (1 << 31)).any()
    assert off.max() < (1 << 32)
    facts, _, _ = run_case(gpu_device, fb, idx, cls, outputs=outputs, shape=shape, lane_block=blk, time_pipe=time_pipe)
    assert facts["padded"] == B
    if shape == "quad":
        assert facts["chains_per_wave"] == 16      # shape_of kept the quad shape (kQC chains per wavefront)


def test_time_flipped_wrapper_at_the_one_lane_guard(gpu_device):
    """SIAlphaModelBackwardEKFOptControlled (FLIP = 1 instantiations: the smoother walks the arrays in the other direction, the
    windows are entered from their other end) on 40-chain blocks at the lane6 guard, all outputs."""
    B, blk = 1048560, 40
    assert lane_window(B) == 4
    fb = H.FormulaBatch(_base(12, 10, 4, kind="sia6b"), B)
    idx, cls = H.extreme_sample(B, blk, units=(blk, 64, 4 * blk, 4096, 65536))
    facts, _, _ = run_case(gpu_device, fb, idx, cls, shape="lane", lane_block=blk, test_window=0)
    assert facts["padded"] == B


@pytest.mark.parametrize("over", [0, 1], ids=["n_npi*Su=2^25", "one-series-more"])
def test_hex_window_set_by_the_control_table(gpu_device, over):
    """The `su` branch of hx_window: a SMALL batch (4 000 chains) reading from a table of 2^22 control series of 8 NPIs -- a day
    of the table (n_npi Su 8 = 2^28 bytes) is wider than a day of any output, so the table sets the window: 4 days, 14 days
    run.  n_npi * Su = 2^25 is shape_of's limit for the hex shape; with one series more the call must leave it (the quad shape:
    16 chains per wavefront) and give the same bits.  Chains read series 0, Su - 1, the two in the middle and hashed ones."""
    B, n, Su = 4000, 8, (1 << 22) + over
    assert (n * Su <= (1 << 25)) == (not over)
    assert hex_window(B, n, Su) == 4 and n * Su * 8 > B * 288
    fb = H.FormulaBatch(_base(n, 10, 4), B, u_mode="table", Su=Su)
    idx, cls = H.extreme_sample(B, 10, units=(10, 64, 640), n_spread=150)
    ser = fb.table_series(idx)
    assert {0, Su - 1, Su // 2, Su // 2 - 1} <= set(ser.tolist()) and np.unique(ser).size > idx.size // 4      # half the chains read hashed series
    # the widest control offset of a window (its last day, the prefetched one beyond, the last row's last series) is in range
    assert 6 * n * Su * 8 <= LW_RECORDS or over
    facts, _, _ = run_case(gpu_device, fb, idx, cls, shape="hex", lane_block=10, test_window=0, extra_bytes=14 * n * Su * 8 * 2)
    assert facts["chains_per_wave"] == (16 if over else 10)


# ------------------------------------------------------------------------------------------------------------------ A4
A4 = [  # id, base kind, n_npi, T_hist, horizon, lane_block, outputs, run_case arguments
    # ekf_fwd_sym<3> + eks_bwd_sym<3>: 9 rows x 2^23 chains x 8 days = 4.5 GiB per covariance array
    ("sia3-lane-classic", "sia3", 12, 8, 0, 0, None, dict(shape="lane")),
    ("sia3-lane-blk8", "sia3", 12, 8, 0, 8, None, dict(shape="lane")),
    # fp32 storage: ekf_fwd_sym<6, FLIP, 0, 1> + eks_bwd_sym<6, FLIP, 1>, every store a 4-byte twin
    ("sia6-f32-classic", "sia6", 12, 2, 1, 0, None, dict(shape="lane", storage="f32")),
    ("sia6-f32-blk8", "sia6", 1, 2, 1, 8, None, dict(shape="lane", storage="f32")),
    # the dense kernels: the NewCase model's own, and a generic batch sent there by path_hint = 2
    ("newcase-dense", "newcase", 12, 2, 1, 0, None, dict(shape="lane")),
    ("sia6-dense-by-hint", "sia6", 1, 2, 1, 0, None, dict(shape="lane", dense=True)),
]


@pytest.mark.parametrize("kind,n,T_hist,hor,blk,outputs,kw", [c[1:] for c in A4], ids=[c[0] for c in A4])
def test_other_one_lane_families_at_two_to_the_23(gpu_device, kind, n, T_hist, hor, blk, outputs, kw):
    """The 3-state model, fp32 storage and the dense kernels at B = 2^23.  With 4-byte stores (and 9-row arrays) no offset
    within a day reaches 2^31: the sample is recomputed for the item size and the class is asserted only where it exists."""
    B = 1 << 23
    f32 = kw.get("storage") == "f32"
    fb = H.FormulaBatch(_base(n, T_hist, hor, kind=kind), B)
    idx, cls = H.extreme_sample(B, blk or B, units=(blk or 64, 64, 256, 4096, 65536), rows=(fb.m * fb.m, 21),
                                itemsize=4 if f32 else 8)
    assert ("rows36_bit31" in cls) == (fb.m == 6 and not f32)
    run_case(gpu_device, fb, idx, cls, outputs=outputs, lane_block=blk, **kw)


A4_PLANTED = [  # id, B, T_hist, horizon, Ps_init(6,6) of the planted chains, lane_block, outputs
    # mid-run overflow (day 8 of 14) under the fixed-descriptor smoother, all outputs
    ("2^20-blk40-mid-run", 1048560, 10, 4, 1e307, 40, None),
    # overflow on the first day at validate's limit
    ("2^23-classic-day-1", 1 << 23, 2, 1, 1.7e308, 0, REDUCED),
]


@pytest.mark.parametrize("B,T_hist,hor,val,blk,outputs", [c[1:] for c in A4_PLANTED], ids=[c[0] for c in A4_PLANTED])
def test_dense_second_pass_at_the_extreme_indices(gpu_device, B, T_hist, hor, val, blk, outputs):
    """exact_nonfinite (the default): chains whose covariance overflows are listed (only[]) and run again by the dense kernels,
    in place.  A handful planted at the extreme indices as test_mid_run_covariance_overflow_on_the_packed_path plants one:
    their status carries the guard bit and no other chain's does, and every output of every sampled chain -- planted ones and
    their neighbours -- equals the oracle's, Inf / NaN pattern included."""
    fb = H.FormulaBatch(_base(12, T_hist, hor), B)
    idx, cls = H.extreme_sample(B, blk or B, units=(blk or 64, 64, 4096, 65536))
    planted = [0, B - 1, B // 2, (blk or 64) * ((B // 2) // (blk or 64)) - 1] + [int(c) for c in cls.get("rows36_bit31", [])[:2]]
    for c in planted:
        fb.plant(c, 35, val)
    idx = np.unique(np.concatenate([idx, planted, np.asarray(planted) + 1, np.asarray(planted) - 1]))
    idx = idx[(idx >= 0) & (idx < B)]
    facts, _, _ = run_case(gpu_device, fb, idx, cls, outputs=outputs, shape="lane", lane_block=blk)
    sel = np.searchsorted(idx, np.unique(planted))
    rk = facts["ref"]["pinv_rank"][:, sel]
    assert (rk[:-1] == -1).any(axis=0).all(), "a planted chain no longer overflows"
    if val < 1e308:
        assert (rk[0] != -1).all(), "the overflow is no longer in mid-run"


# ------------------------------------------------------------------------------------------------------------ alignment
@pytest.mark.parametrize("shape,blk,B", [("lane", 40, 80), ("hex", 10, 80)], ids=["lane6-xd", "hex-dma"])
def test_device_pointers_eight_bytes_off_their_allocation(gpu_device, shape, blk, B):
    """eks_bwd_lane6 (blk 40, cn % 40 == 0) and the hex smoother (one wave per SIMD) copy P_PLUS and X with 16-byte-per-lane
    LDS-DMA, and include/epiekf.h asks for no alignment beyond the element's.  Every device pointer of the call -- inputs,
    outputs, workspace -- 8 bytes off its allocation (a tensor slice): the call must give the oracle's bits or refuse cleanly
    with EPI_ERR_BAD_ARG.  It gives the bits (include/epiekf.h, "Alignment")."""
    import torch
    from epidemicmodeling_amd import _lib, batch, synth
    w = synth.make_cfg4(B // 20, 20, 30, 10)
    ref = H.oracle_batch(w)
    dw = batch.DeviceWorkload(w, gpu_device)

    def off8(t):
        if t is None:
            return None
        raw = torch.empty(t.numel() + 3, dtype=t.dtype, device=t.device)
        k = 8 // t.element_size()
        v = raw[k:k + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 8 and v.is_contiguous()
        return v
    for k in ("x", "u", "R_series", "x_series", "u_series", "prm", "s_init", "Ps_init", "s_final", "Ps_final", "Q"):
        setattr(dw, k, off8(getattr(dw, k)))
    r = batch.EkfRunner(dw, extras=True, shape=shape, lane_block=blk, test_window=0)
    assert r.blk == blk and B % blk == 0
    r.out = {k: off8(t) for k, t in r.out.items()}
    r.ws, r.pinv_rank, r.status = off8(r.ws), off8(r.pinv_rank), off8(r.status)
    r._bind()
    H.poison_runner(r)
    try:
        r.run()
    except _lib.EpiError as e:
        assert e.status == -5, e
        torch.cuda.synchronize()
        assert all(bool((t.view(torch.int64) == H.POISON64).all()) for t in r.out.values()), "a refused call wrote outputs"
        return
    torch.cuda.synchronize()
    assert not H.surviving_poison(r)
    for k in H.OUT_NAMES:
        assert np.array_equal(r.unblocked(k).cpu().numpy(), ref[k], equal_nan=True), k
    assert np.array_equal(r.unblocked("pinv_rank").cpu().numpy(), ref["pinv_rank"])


# ------------------------------------------------------------------------------------------------------------------ A5
REJECTED = [  # id, B, Sx, Su, lane_block, text
    ("B", (1 << 23) + 1, 16, 16, 0, "B, Sx, Su are limited to 2^23"),
    ("Sx", 1 << 20, (1 << 23) + 1, 16, 0, "B, Sx, Su are limited to 2^23"),
    ("Su", 1 << 20, 16, (1 << 23) + 1, 0, "B, Sx, Su are limited to 2^23"),
    ("padded-B", (1 << 23) - 7, 16, 16, 40, "B rounded up to lane_block exceeds 2^23"),
]


@pytest.mark.parametrize("B,Sx,Su,blk,text", [c[1:] for c in REJECTED], ids=[c[0] for c in REJECTED])
def test_batches_beyond_the_limits_are_rejected_untouched(gpu_device, B, Sx, Su, blk, text):
    """B, Sx, Su = 2^23 + 1 and a padded B above 2^23 (B below it): EPI_ERR_BAD_ARG with the documented text from
    epi_ekf_validate, epi_ekf_workspace_bytes = 0, and epi_ekf_run_device / epi_ekf_precheck_device return the same before
    they read a pointer or launch anything: every pointer of the call is a small poisoned buffer (inputs, outputs, workspace)
    that must come back unchanged."""
    import torch
    from epidemicmodeling_amd import _lib, layout as L_
    h = _lib.lib()
    d = _lib.make_desc("SIAlphaModelEKFOptControlled", B, 4, Sx, Su, 12, 21, 1, "NEWCASES", 1, L_.OUT_ALL)
    d.lane_block = blk
    err = C.create_string_buffer(256)
    assert h.epi_ekf_validate(C.byref(d), err) == -5 and text in err.value.decode()        # EPI_ERR_BAD_ARG
    h.epi_ekf_workspace_bytes.restype = C.c_size_t
    assert h.epi_ekf_workspace_bytes(C.byref(d)) == 0
    d_ok = _lib.make_desc("SIAlphaModelEKFOptControlled", 1 << 23, 4, 1 << 23, 1 << 23, 12, 21, 1, "NEWCASES", 1, L_.OUT_ALL)
    assert h.epi_ekf_validate(C.byref(d_ok), err) == 0                                       # the limit itself is legal
    buf = torch.full((64, 4096), 0xA7, dtype=torch.uint8, device=gpu_device)
    ins, outs = _lib.Inputs(), _lib.Outputs()
    k = 0
    for s, names in ((ins, ("x_series", "u_series", "x", "u", "R_series", "prm", "s_init", "Ps_init", "s_final", "Ps_final", "Q")),
                     (outs, tuple(H.OUT_NAMES) + ("pinv_rank", "status"))):
        for nme in names:
            setattr(s, nme, C.c_void_p(buf[k].data_ptr()))
            k += 1
    st = torch.cuda.current_stream(gpu_device)
    err2 = C.create_string_buffer(256)
    rc = h.epi_ekf_run_device(C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(buf[40].data_ptr()), 4096 * 20,
                              C.c_void_p(st.cuda_stream), err2)
    assert rc == -5 and text in err2.value.decode()
    ok = C.c_int(7)
    rc = h.epi_ekf_precheck_device(C.byref(d), C.byref(ins), C.c_void_p(st.cuda_stream), C.byref(ok), err2)
    assert rc == -5 and text in err2.value.decode()
    torch.cuda.synchronize()
    assert bool((buf == 0xA7).all())


# ------------------------------------------------------------------------------------------------------------------ B
def _pareto_points(c, xp_float):
    """(J0, J1) of point c = r * P + p: 24-bit hashes x 2^-24, exact on device and host."""
    return xp_float((H.chain_hash(c, 3) >> 8) + 1) * 2.0 ** -24, xp_float((H.chain_hash(c, 4) >> 8) + 1) * 2.0 ** -24


@pytest.mark.parametrize("R,P", [(1024, 8192), (1 << 23, 1), ((1 << 24) + 1000, 1)])
def test_pareto_filter_at_its_batch_limit(gpu_device, R, P):
    """epi_pareto_front_device with R * P = 2^23 (the limit epi_sweep_prescribe_host states for the sweep it feeds): points by
    formula, the NaN / tie / duplicate columns of test_pareto_front_filter planted in the first, middle and last regions,
    outputs poisoned; sampled regions against the oracle and no poison left in the whole front / I_opt.  The device entry itself
    states no limit on R: 2^24 + 1000 regions are one 256-lane workgroup each, more than 2^32 lanes -- in ONE launch the thread
    count wrapped and 1 000 regions were written; the launch is sliced now."""
    import torch
    from epidemicmodeling_amd import _lib
    from oracle import oracle_lib as olib
    dev = torch.device(gpu_device)
    c = torch.arange(R * P, dtype=torch.int64, device=dev)
    J0, J1 = _pareto_points(c, lambda t: t.to(torch.float64))
    J0, J1 = J0.reshape(R, P), J1.reshape(R, P)
    planted = [0, R // 2, R - 1]

    def plant(a0, a1, first, last):
        if P > 8:
            a0[:, 3] = a0[:, 1]; a1[:, 4] = a1[:, 2]
            a0[:, 6] = a0[:, 0]; a1[:, 6] = a1[:, 0]
            if first:
                a0[0, 5] = float("nan")
            if last:
                a1[-1, 7] = float("nan")
    for i, r in enumerate(planted):
        plant(J0[r:r + 1], J1[r:r + 1], i == 0, i == 2)
    # (8 192 points cost the oracle's O(P^2) loop 0.2 s per region: a dozen regions there; a region is a workgroup of its own,
    # so only the ends and a spread matter)
    reg, _ = H.extreme_sample(R, R, units=(64, 256) if P == 1 else (), n_spread=200 if P == 1 else 8, rows=())
    reg = np.unique(np.concatenate([reg, planted]))
    cc = (reg[:, None] * P + np.arange(P)[None]).astype(np.int64)
    h0, h1 = _pareto_points(cc, lambda a: a.astype(np.float64))
    for i, r in enumerate(planted):
        j = int(np.searchsorted(reg, r))
        plant(h0[j:j + 1], h1[j:j + 1], i == 0, i == 2)
    sel = torch.as_tensor(reg, device=dev)
    assert np.array_equal(J0.index_select(0, sel).cpu().numpy(), h0, equal_nan=True)
    assert np.array_equal(J1.index_select(0, sel).cpu().numpy(), h1, equal_nan=True)
    on = torch.full((R, P), -7, dtype=torch.int32, device=dev)
    io = torch.full((R,), -7, dtype=torch.int32, device=dev)
    err = C.create_string_buffer(256)
    st = torch.cuda.current_stream(dev)
    rc = _lib.lib().epi_pareto_front_device(R, P, C.c_void_p(J0.data_ptr()), C.c_void_p(J1.data_ptr()), C.c_void_p(on.data_ptr()),
                                            C.c_void_p(io.data_ptr()), C.c_void_p(st.cuda_stream), err)
    _lib.check(rc, err)
    torch.cuda.synchronize()
    assert not bool((on == -7).any()) and not bool((io == -7).any())
    assert bool(((on == 0) | (on == 1)).all()) and bool(((io >= 0) & (io < P)).all())
    g_on, g_io = on.index_select(0, sel).cpu().numpy(), io.index_select(0, sel).cpu().numpy()
    for j, r in enumerate(reg):
        ron, rio = olib.pareto_front(h0[j], h1[j])
        assert np.array_equal(g_on[j].astype(bool), ron) and g_io[j] == rio, int(r)


def test_pareto_and_prescribe_rejections(gpu_device):
    """P = 8193 is refused by the filter (outputs untouched); epi_sweep_prescribe_host refuses R * P = 2^23 + 1 and P = 8193
    through its descriptor, before it reads an input pointer (all NULL here)."""
    import torch
    from epidemicmodeling_amd import _lib
    dev = torch.device(gpu_device)
    h = _lib.lib()
    err = C.create_string_buffer(256)
    J = torch.zeros(8193, dtype=torch.float64, device=dev)
    on = torch.full((8193,), -7, dtype=torch.int32, device=dev)
    io = torch.full((1,), -7, dtype=torch.int32, device=dev)
    rc = h.epi_pareto_front_device(1, 8193, C.c_void_p(J.data_ptr()), C.c_void_p(J.data_ptr()), C.c_void_p(on.data_ptr()),
                                   C.c_void_p(io.data_ptr()), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), err)
    torch.cuda.synchronize()
    assert rc == -8 and b"8192" in err.value and bool((on == -7).all()) and int(io[0]) == -7      # EPI_ERR_UNSUPPORTED
    for R, P, code, text in (((1 << 23) + 1, 1, -5, b"R * P <= 2^23"), (2796203, 3, -5, b"R * P <= 2^23"),
                             (1, 8193, -8, b"8192")):
        d = _lib.PrescribeDesc()
        d.abi_version, d.R, d.P, d.T, d.t_hist = _lib.ABI_VERSION, R, P, 20, 10
        ins, outs = _lib.PrescribeInputs(), _lib.PrescribeOutputs()
        ids = (C.c_int * 1)(0)
        rc = h.epi_sweep_prescribe_host(C.byref(d), C.byref(ins), C.byref(outs), 1, ids, err)
        assert rc == code and text in err.value, (R, P, rc, err.value)


def test_lookahead_batch_count_rejections():
    """epi_lookahead_validate: R * F = 2^23 is accepted, 2^23 + 1 is not; R * M beyond 2^31 - 1 is not (descriptor alone)."""
    from epidemicmodeling_amd import _lib
    h = _lib.lib()
    err = C.create_string_buffer(256)
    mk = lambda R, F, M: _lib.make_lookahead_desc(R, 1024, F, M, 12, 21)
    assert h.epi_lookahead_validate(C.byref(mk(1 << 13, 1024, 1)), err) == 0, err.value
    assert h.epi_lookahead_validate(C.byref(mk(1 << 23, 1, 1)), err) == 0, err.value
    assert h.epi_lookahead_validate(C.byref(mk(2796203, 3, 1)), err) == -5 and b"R * F chains are limited to 2^23" in err.value
    assert h.epi_lookahead_validate(C.byref(mk(1 << 23, 1, 255)), err) == 0, err.value          # 2^31 - 2^23 columns
    assert h.epi_lookahead_validate(C.byref(mk(1 << 23, 1, 256)), err) == -5 and b"M * R table columns exceed the grid" in err.value


def test_rt_window_and_lasso_element_count_rejections():
    """epi_rtwin_validate and epi_lasso_validate just below R * L and R * D * n = 2^31 (accepted) and at 2^31 (rejected),
    through the descriptors alone: validation reads no array, every pointer is one 8-byte dummy."""
    from epidemicmodeling_amd import _lib
    h = _lib.lib()
    err = C.create_string_buffer(256)
    dummy = np.zeros(1)
    p = dummy.ctypes.data
    ro = _lib.RtwinOutputs()
    ok = _lib.make_rtwin_desc(((1 << 31) - 1) // 7, 7, 7, generation_period=5)
    assert ok.R * ok.L > (1 << 31) - 8
    assert h.epi_rtwin_validate(C.byref(ok), p, C.byref(ro), err) == 0, err.value
    bad = _lib.make_rtwin_desc(1 << 24, 128, 7, generation_period=5)
    assert h.epi_rtwin_validate(C.byref(bad), p, C.byref(ro), err) == -5 and b"R * L is limited to 2^31 - 1" in err.value
    lo = _lib.LassoOutputs()
    for k in _lib.LASSO_OUT_NAMES:
        setattr(lo, k, p)
    ok = _lib.make_lasso_desc(((1 << 31) - 1) // (16 * 12), 16, 12, 2)
    assert ok.R * ok.D * ok.n > (1 << 31) - 1 - 16 * 12
    assert h.epi_lasso_validate(C.byref(ok), p, p, p, C.byref(lo), err) == 0, err.value
    bad = _lib.make_lasso_desc(1 << 23, 16, 16, 2)
    assert h.epi_lasso_validate(C.byref(bad), p, p, p, C.byref(lo), err) == -5 and b"R * D * n is limited to 2^31 - 1" in err.value


# ---------------------------------------------------------------------------------- B: runs at the batch-count limits
_poisoned, _holds_poison, _need_free = H.poisoned, H.holds_poison, H.need_free        # shared with tests/test_gpu_call_limits.py
_formula_rows, _crossing_regions = H.formula_rows, H.crossing_regions


@pytest.mark.parametrize("R,F,LL,M", [(1 << 21, 4, 12, 2), (1 << 23, 1, 4, 9)], ids=["4-starts", "2^26-table-columns"])
def test_lookahead_at_two_to_the_23_chains(gpu_device, R, F, LL, M):
    """epi_lookahead_run_device with R * F = 2^23 masked chains.  2^21 regions x 4 starts, LL = 12 days, M = 2: the smallest
    study that still has statistics over more than one row (rows M .. F).  2^23 regions x 1 start, M = 9: M * R = 9 x 2^23 table
    columns, one 64-lane workgroup each -- more than 2^32 lanes, which one launch cannot hold (the thread count wraps silently:
    the statistics of all but 2^23 columns were left unwritten before the launches were sliced); F < M, so every statistic is
    NaN and must be WRITTEN as NaN.  Regions by formula (FormulaBatch, one series per region), truth and population gathered
    from the 16 base regions; outputs, chain arrays and workspace poisoned.  Sampled regions -- every start of each -- against
    tests/lookahead_ref.py on those regions alone: tables, statistics and chains."""
    import torch
    from epidemicmodeling_amd import batch, synth
    from tests import lookahead_ref as LR
    S = 16
    assert R * F == 1 << 23 and (M * R * 64 >= 1 << 32) == (F == 1)
    _need_free(gpu_device, 45 << 30)
    base = _base(12, LL, 0, S=S, kind="sia3")
    N = synth.make_regions(S)["N"].astype(np.float64)
    truth16 = np.ascontiguousarray(base.x * N[None, :] + 50.0)
    fb = H.FormulaBatch(base, R, x_mode="own", u_mode="own")
    reg, cls = H.extreme_sample(R, R, units=(16, 64, 256, 4096, 65536), rows=(9,))
    ws_host = fb.host_workload(reg)
    rr = fb.region(reg)
    truth_s, pop_s = np.ascontiguousarray(truth16[:, rr]), np.ascontiguousarray(N[rr])
    dw = fb.device_workload(gpu_device)
    for k, v in fb.inputs_of(dw, reg).items():
        assert np.array_equal(v, getattr(ws_host, k), equal_nan=True), k
    r_dev = fb.region(torch.arange(R, dtype=torch.int64, device=gpu_device))
    truth = torch.as_tensor(truth16).to(gpu_device).index_select(1, r_dev)
    pop = torch.as_tensor(N).to(gpu_device).index_select(0, r_dev)
    run = batch.LookaheadRunner(dw, truth, pop, F, M, device=gpu_device, chains=True)
    for k, t in run.out.items():
        if k == "status":
            t.fill_(H.POISON_STATUS)
        else:
            t.view(torch.int64).fill_(H.POISON64)
    run.ws.view(torch.int64).fill_(H.POISON64)
    run.run()
    torch.cuda.synchronize()
    for k, t in run.out.items():
        assert not (bool((t == H.POISON_STATUS).any()) if k == "status" else _holds_poison(t)), k
    exp = LR.expected(ws_host, truth_s, pop_s, F, M, n_threads=16)
    sel = torch.as_tensor(reg, device=gpu_device)
    for k in batch.LA_TABLES + batch.LA_STATS:
        assert np.array_equal(run.out[k].index_select(-1, sel).cpu().numpy(), exp[k], equal_nan=True), k
    chains = torch.as_tensor((reg[:, None] * F + np.arange(F)[None]).reshape(-1), device=gpu_device)
    assert int(chains.max()) == R * F - 1
    for k in ("S_PLUS", "S_SMOOTH"):
        assert np.array_equal(run.out[k].index_select(-1, chains).cpu().numpy(), exp[k], equal_nan=True), k
    print(f"[addressing] lookahead R={R} F={F}: peak {torch.cuda.max_memory_allocated(gpu_device) / 2**30:.1f} GiB")
    del run, dw, truth, pop
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def rtref(tmp_path_factory):
    from tests.rt_window_ref import RtWindowRef
    return RtWindowRef(tmp_path_factory.mktemp("rtwin_ref_limits"))


@pytest.mark.parametrize("methods", [("LogLinReg", "GenRatios"), ("NonlinLS",)], ids=["llr+gr", "nls"])
def test_rt_window_across_the_2_and_4_gib_offsets(gpu_device, rtref, methods):
    """epi_rtwin_run_device on new_cases [40, R] with 40 R just above 2^29 doubles: every array's byte offset passes 2^31 (day
    19) and 2^32 (day 39) -- the limit itself, 2^31 - 1 elements, would be 16 GiB per array and is asserted through the
    descriptor only.  Cases by formula (positive, exact), outputs poisoned; regions on both sides of each crossing and spread
    ones against tests/rt_window_ref.c, every day.  LogLinReg + GenRatios hold ~39 GB, NonlinLS ~26 GB."""
    import torch
    from epidemicmodeling_amd import _lib
    L_, wlen, gp = 40, 7, 4
    R = (1 << 29) // L_ + 7
    assert L_ * R > (1 << 29) and L_ * R * 8 > (1 << 32)
    from epidemicmodeling_amd.batch import _rtwin_names
    bits, names = _rtwin_names(methods)
    _need_free(gpu_device, (len(names) + 1) * L_ * R * 8 + (2 << 30))
    cases = lambda c: ((H.chain_hash(c, 9) >> 12) + 1)            # x 2^-10: (0, 1024]
    x = _formula_rows(L_, R, gpu_device, lambda c: cases(c).to(torch.float64) * 2.0 ** -10, torch.float64)
    cross = _crossing_regions(L_, R)
    assert len(cross) == 8
    reg, _ = H.extreme_sample(R, R, units=(64, 256, 65536), rows=())
    reg = np.unique(np.concatenate([reg, cross]))
    xs = (cases(np.arange(L_, dtype=np.int64)[:, None] * R + reg[None]).astype(np.float64) * 2.0 ** -10)
    sel = torch.as_tensor(reg, device=gpu_device)
    assert np.array_equal(x.index_select(1, sel).cpu().numpy(), xs)
    d = _lib.make_rtwin_desc(R, L_, wlen, 1.0, 1, gp, bits)
    out = {n: _poisoned((L_, R), torch.int32 if n in _lib.RTWIN_OUT_I32 else torch.float64, gpu_device) for n in names}
    outs = _lib.RtwinOutputs()
    for n in _lib.RTWIN_OUT_NAMES:
        setattr(outs, n, None if n not in out else C.c_void_p(out[n].data_ptr()))
    err = C.create_string_buffer(256)
    t0 = time.perf_counter()
    rc = _lib.lib().epi_rtwin_run_device(C.byref(d), C.c_void_p(x.data_ptr()), C.byref(outs),
                                         C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream), err)
    _lib.check(rc, err)
    torch.cuda.synchronize()
    print(f"[addressing] rt_window {methods} L*R={L_ * R}: {time.perf_counter() - t0:.2f} s, "
          f"peak {torch.cuda.max_memory_allocated(gpu_device) / 2**30:.1f} GiB")
    for n, t in out.items():
        assert not _holds_poison(t), n
    want = {}
    if "LogLinReg" in methods:
        want.update({"llr_" + k: v for k, v in rtref.loglinreg(xs, wlen, 1.0, 1).items()})
    if "GenRatios" in methods:
        want.update({"gr_" + k: v for k, v in rtref.genratios(xs, wlen, gp, 1.0).items()})
    if "NonlinLS" in methods:
        want.update({"nls_" + k: v for k, v in rtref.nonlinls(xs, wlen, 1.0, 1).items()})
    assert set(want) == set(names)
    for n in names:
        assert np.array_equal(out[n].index_select(1, sel).cpu().numpy(), want[n], equal_nan=True), n
    del out, x
    torch.cuda.empty_cache()


def test_lasso_across_the_2_and_4_gib_offsets(gpu_device, tmp_path_factory):
    """epi_lasso_run_device with the size coming from R: D = 4 days, n = 1, K = 2 folds, 2 lambdas, R = 2^27 + 1000 regions,
    so X [4, 1, R] and y [4, R] pass 2^31 bytes (day 1 -> 2) and 2^32 (day 3) -- R * D * n = 2^31 - 1 itself would be 16 GiB
    of X and is asserted through the descriptor only.  Expected time, from profiles/lasso/bench.json: 236 regions x 51 fits x
    100 lambdas of 60 x 12 take 15 - 117 ms, i.e. <= 10 us per fit and lambda for one wavefront; a region here is 3 fits x 2
    lambdas of 4 x 1, a few us of one wavefront, with ~4 000 wavefronts in flight: 0.1 - 1 s for 1.3e8 regions.  It took 1.7 s
    (five launches of 2^25 regions: before the launch was sliced, 1 000 regions ran and the rest kept the poison).  Regions on both sides of each crossing and spread ones against tests/lasso_ref.c."""
    import torch
    from epidemicmodeling_amd import _lib
    from tests.lasso_ref import LassoRef
    ref = LassoRef(tmp_path_factory.mktemp("lasso_ref_limits"))
    D, n, K, NL = 4, 1, 2, 2
    R = (1 << 27) + 1000
    assert R * D * n * 8 > (1 << 32) and R * D * n <= 0x7FFFFFFF
    _need_free(gpu_device, 30 << 30)
    lev = lambda c: H.chain_hash(c, 7) % 5                        # NPI_MAXES - plan: integer levels 0 .. 4
    yv = lambda c: (H.chain_hash(c, 8) >> 12) + 1                 # x 2^-20
    X = _formula_rows(D, R, gpu_device, lambda c: lev(c).to(torch.float64), torch.float64).reshape(D, n, R)
    y = _formula_rows(D, R, gpu_device, lambda c: yv(c).to(torch.float64) * 2.0 ** -20, torch.float64)
    fold = (torch.arange(D, dtype=torch.int32, device=gpu_device) % K)[:, None].expand(D, R).contiguous()
    cross = _crossing_regions(D, R)
    assert len(cross) == 8
    reg, _ = H.extreme_sample(R, R, units=(64, 256, 65536), rows=())
    reg = np.unique(np.concatenate([reg, cross]))
    cc = np.arange(D, dtype=np.int64)[:, None] * R + reg[None]
    Xs, ys = lev(cc).astype(np.float64)[:, None, :], yv(cc).astype(np.float64) * 2.0 ** -20
    fs = np.ascontiguousarray(np.broadcast_to((np.arange(D, dtype=np.int32) % K)[:, None], (D, reg.size)))
    sel = torch.as_tensor(reg, device=gpu_device)
    assert np.array_equal(X.index_select(2, sel).cpu().numpy(), Xs) and np.array_equal(y.index_select(1, sel).cpu().numpy(), ys)
    d = _lib.make_lasso_desc(R, D, n, K, NL)
    out = {k: _poisoned(sh, torch.int32 if k in _lib.LASSO_OUT_I32 else torch.float64, gpu_device)
           for k, sh in _lib.lasso_shapes(R, D, n, K, NL).items()}
    outs = _lib.LassoOutputs()
    for k in _lib.LASSO_OUT_NAMES:
        setattr(outs, k, None if k not in out else C.c_void_p(out[k].data_ptr()))
    err = C.create_string_buffer(256)
    t0 = time.perf_counter()
    rc = _lib.lib().epi_lasso_run_device(C.byref(d), C.c_void_p(X.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(fold.data_ptr()),
                                         C.byref(outs), C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream), err)
    _lib.check(rc, err)
    torch.cuda.synchronize()
    print(f"[addressing] lasso R={R}: {time.perf_counter() - t0:.2f} s, peak {torch.cuda.max_memory_allocated(gpu_device) / 2**30:.1f} GiB")
    for k, t in out.items():
        assert not _holds_poison(t), k
    want = ref.run(np.ascontiguousarray(Xs), np.ascontiguousarray(ys), fs, K, NL)
    for k in out:
        assert np.array_equal(out[k].index_select(-1, sel).cpu().numpy(), want[k], equal_nan=True), k
    del out, X, y, fold
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- the seeded normal draws' fill kernel at its production bounds
NOISE_GUARD = 64                                                     # poisoned words before and behind the output
NOISE_CHUNK = 1 << 24                                                # lanes of one separate call of the every-word check


def _noise_fill(out, guard, seed, stream, t0, rows, lane0, n, groups=0):
    """epi_noise_fill_device of one day into the flat tensor `out` behind `guard` leading words; returns the call's seconds"""
    import torch
    from epidemicmodeling_amd import _lib
    d, err = _lib.make_noise_desc(seed, stream), C.create_string_buffer(256)
    torch.cuda.synchronize()
    t = time.perf_counter()
    rc = _lib.lib().epi_noise_fill_device(C.byref(d), t0, 1, rows, lane0, n, int(out.dtype == torch.float32),
                                          C.c_void_p(out.data_ptr() + guard * out.element_size()), groups,
                                          C.c_void_p(torch.cuda.current_stream(out.device).cuda_stream), err)
    _lib.check(rc, err)
    torch.cuda.synchronize()
    return time.perf_counter() - t


@pytest.mark.parametrize("case", ["N1", "N2"])
def test_noise_fill_at_its_production_bounds(gpu_device, tmp_path_factory, case):
    """epi_noise_fill_device with test_launch_groups = 0: the real cut kNoiseLaunchGroups = 2^22 workgroups.
    N1: float, rows = 3, one day, 2^30 + 2^29 + 300 lanes: 2 n = 3.2e9 items go out in FOUR launches (wg0 = k 2^22), the 3 n =
    4.8e9 output words pass element 2^32 (row 2) and byte 2^32 (row 0, lane 2^30: the first launch boundary as well), 18 GiB.
    N2: double, rows = 1, 2^29 + 300 lanes: one launch whose double stores pass byte 2^32.
    The output is poisoned with guard words either side: no poison left, the guards intact; 130-lane windows of all rows at the
    first and the last lanes, either side of every launch boundary (items k 2^30) and of word and byte 2^32 equal
    tests/noise_ref.c, rounded to float for N1; and EVERY word equals the same array made by separate calls of 2^24 lanes at
    lane0 + j 2^24 -- a window is a window, so that is an identity.  Measured on one MI355X: N1 the call 0.05 s, the case 0.6 s, peak 18.3 GiB; N2 0.01 s, 0.1 s, 4.3 GiB.

    That it bites (scratch builds, never committed; noise_fill / noise_fill_lane of csrc/noise.hpp): `wg0` dropped from the item
    index -- N1 fails (poison left: launches 2 .. 4 rewrite the first 2^30 items); `o` taken through uint32_t -- N1 fails (poison
    left behind word 2^32, and the window behind it)."""
    import torch
    from tests import noise_ref as NR
    ref = NR.NoiseRef(tmp_path_factory.mktemp("noise_ref_limits"))
    t_case = time.perf_counter()
    seed, stream, t0, lane0 = 0x9E3779B97F4A7C15, 3, 7, (1 << 33) + 5            # the high lane word is in use
    if case == "N1":
        dt, rows, n = torch.float32, 3, (1 << 30) + (1 << 29) + 300
    else:
        dt, rows, n = torch.float64, 1, (1 << 29) + 300
    pairs, esz = (rows + 1) // 2, 4 if dt == torch.float32 else 8
    items, words = pairs * n, rows * n
    bounds = [k << 30 for k in range(1, 4) if (k << 30) < items]                # first items of the launches 2 ..
    assert len(bounds) == (3 if case == "N1" else 0) and words * esz > (1 << 32) and (words > (1 << 32)) == (case == "N1")
    # the lanes at which something wraps if it wraps: item -> lane (item % n), word and byte 2^32 -> lane (word % n)
    marks = [0, n] + [b % n for b in bounds] + [w % n for w in ((1 << 32), (1 << 32) // esz) if w < words]
    starts = sorted({min(max(m - 65, 0), n - 130) for m in marks})
    assert len(starts) == (6 if case == "N1" else 3), starts                     # N1: byte 2^32 IS the first launch boundary
    _need_free(gpu_device, words * esz + 3 * rows * NOISE_CHUNK * esz + (2 << 30))
    flat = _poisoned((words + 2 * NOISE_GUARD,), dt, gpu_device)
    t_call = _noise_fill(flat, NOISE_GUARD, seed, stream, t0, rows, lane0, n)
    head, body, tail = flat[:NOISE_GUARD], flat[NOISE_GUARD:NOISE_GUARD + words].view(rows, n), flat[NOISE_GUARD + words:]
    poison = _poisoned((NOISE_GUARD,), dt, gpu_device)
    as_int = lambda t: t.view(torch.int32 if dt == torch.float32 else torch.int64)
    assert torch.equal(as_int(head), as_int(poison)) and torch.equal(as_int(tail), as_int(poison)), "guard words overwritten"
    for r in range(rows):
        for lo in range(0, n, 1 << 28):
            assert not _holds_poison(body[r, lo:lo + (1 << 28)]), ("poison left", r, lo)
    for s in starts:
        want = ref.fill(seed, stream, t0, 1, rows, lane0 + s, 130)[0]
        got = body[:, s:s + 130].cpu().numpy()
        assert NR.same_bits(got, want.astype(got.dtype)), ("window at lane", s)
    # every word: the same array in pieces
    piece = _poisoned((rows * NOISE_CHUNK,), dt, gpu_device)
    for j in range(0, n, NOISE_CHUNK):
        m = min(NOISE_CHUNK, n - j)
        _noise_fill(piece, 0, seed, stream, t0, rows, lane0 + j, m)
        assert torch.equal(as_int(piece[:rows * m].view(rows, m)), as_int(body[:, j:j + m])), ("lanes from", j)
    H.report_limits(f"noise_fill {case}: {rows} x {n} {'float' if esz == 4 else 'double'}, {len(bounds) + 1} launches", t_call, t_case,
                    gpu_device)
    del flat, head, body, tail, piece
    torch.cuda.empty_cache()

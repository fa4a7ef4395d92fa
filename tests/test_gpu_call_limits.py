"""The four newest device calls -- ensemble statistics, AR forecaster, forward-backward fusion, robust regression -- past one
launch and across the 2 / 4 / 8 GiB byte offsets of their arrays.

Each entry point cuts its grid into launches of at most 2^25 (fusion: 2^23) workgroups, because a launch's thread count is a
32-bit number, and hands the kernel the first item of the launch (item0 / r0 / blk0 / wg0), which the kernel decodes into
(day, row, region), (NPI, region), region or (day, tile).  The small-shape modules never reach a second launch, so a loop
that stopped after one, or a kernel that forgot its offset, left them green.  The cases here are the smallest that take a
second launch, and they follow the three rules of tests/test_gpu_addressing_limits.py:

 1. inputs by formula per element (helpers.chain_hash), evaluated by torch on the device for the whole array and by NumPy for
    the sample, the two compared bit for bit before the run;
 2. every output poisoned (helpers.POISON64 / POISON32 / POISON_RANK / POISON_STATUS); after the run no word of any output of
    the WHOLE call may still hold the poison -- this is what catches a slice that never ran.  (The fusion's status words are
    zeroed by the call itself and OR-ed into; a blocked output's padding lanes must KEEP the poison.);
 3. the sampled regions / days -- both sides of every launch boundary (items k 2^n - 2 .. k 2^n + 1), both sides of the element
    where an array's byte offset first reaches 2^31, 2^32 (2^33), the first and last items, a spread -- equal, bit for bit and
    NaN to NaN, the family's restatement run on the sample alone; each test asserts that its sample holds these classes.

Device memory is estimated before a case allocates; too little free memory fails the case with the numbers.

What stays with the small shapes (tests/test_gpu_ar_forecast.py::test_chain_counts, tests/test_gpu_two_filter.py): the decode
with more than one workgroup per region (bpr >= 2) or per day (tiles >= 2) ACROSS a launch boundary -- it needs ~78 GB of S
or of each P array.  The product limits themselves (R D = 2^31 - 1, ...) cost 16 GiB or more per array: they are asserted
through the descriptors in tests/test_*_abi.py, and the launch geometry at D, B near 2^31 in tests/test_ar_forecast_emu.py and
tests/test_two_filter_emu.py (CPU).

Measured on one MI355X (the library call alone / the whole case with input generation, sampling and the restatement /
torch.cuda.max_memory_allocated):
  ens_summary, double   0.16 s / 0.9 s / 18.9 GiB       ens_summary, float    0.15 s / 0.2 s / 16.1 GiB
  robust_fit            0.37 s / 0.4 s / 18.6 GiB       ar_forecast           0.07 s / 1.6 s / 26.2 GiB
  two_filter (a)        0.08 s / 0.3 s / 21.5 GiB       two_filter (b)        0.25 s / 0.3 s /  6.6 GiB
The module takes 6 s.  No time is asserted; every case prints its figures in a line that starts with [limits].
"""
import ctypes as C
import time

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

LAUNCH = 1 << 25            # kEnsLaunchItems, kRfLaunchItems, kArLaunchBlocks
FUSE_LAUNCH = 1 << 23       # kFuseLaunchGroups


# the small helpers this module shares with tests/test_gpu_regression_limits.py
_fl, _pos, _sgn = H.as_f64, H.hash_pos, H.hash_sgn
_bits_equal, _both_sides, _poison_words, _report = H.bits_equal, H.both_sides, H.poison_words, H.report_limits


# ------------------------------------------------------------------------------------------------------------------ ens
def _ens_value(c):
    return _fl(_pos(c, 11)) * 2.0 ** -10           # (0, 1024], 20 significant bits: exact in float too


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_ens_summary_past_one_launch(gpu_device, storage):
    """epi_ens_run_device with T = 3, rows = 3 + the derived row, D = 5 draws, R = 2^24 + 1000 regions, two quantiles, all six
    outputs: 12 R = 6 x 2^25 + 12 000 items, seven launches of ens_summary<1>.  The decode item -> (t, r, row) = ((item / 4)
    / R, (item / 4) % R, item % 4) meets a launch boundary twice in each of the three days, in mid-day (and once 1 000 regions
    before a day ends).  src holds 45 R = 7.5e8 elements: 6.0 GB as double (byte offsets pass 2^31 in row 3, 2^32 in row 6), 3.0 GB
    as float (2^31 in row 6); quantiles [3, 2, 4, R] passes 2^31.  Planted: one NaN member in an item before and in one behind
    the first boundary, one all-NaN item at the third.  Sampled regions -- every day and row of each -- against
    tests/ens_summary_ref.summary on their own columns.  With item0 ignored by the kernel (a scratch build) this test fails on
    rule 2: every launch rewrites the first 2^25 items and the other 1.7e8 keep the poison."""
    import torch
    from epidemicmodeling_amd import _lib, synth
    from tests import ens_summary_ref as E
    T, rows, D, R, q = 3, 3, 5, (1 << 24) + 1000, (0.25, 0.9)
    ro, B = rows + 1, R * D
    f32 = storage == "f32"
    es, tdt, ndt = (4, torch.float32, np.float32) if f32 else (8, torch.float64, np.float64)
    items = T * ro * R
    assert 6 * LAUNCH < items < 7 * LAUNCH and (1 << 23) < R
    H.need_free(gpu_device, T * rows * B * es + (4 * T * ro + T * len(q) * ro) * R * 8 + T * ro * R * 4 + (3 << 30))
    t_case = time.perf_counter()
    dev = torch.device(gpu_device)
    src = H.formula_rows(T * rows, B, dev, _ens_value, tdt).reshape(T, rows, B)
    N16 = synth.make_regions(16)["N"].astype(np.float64)
    pop = torch.as_tensor(N16, device=dev).index_select(0, torch.arange(R, dtype=torch.int64, device=dev) % 16)
    # the sample
    bnd_items = H.boundary_items(LAUNCH, items)
    region_of = lambda i: (i // ro) % R
    bnd = sorted({region_of(i) for i in bnd_items})
    days_met = sorted({(i // ro) // R for i in bnd_items})
    cross_cols = H.crossing_regions(T * rows, B, itemsize=es)        # columns of src [9, B]; the regions that hold them, +- 1
    cross_src = sorted({c // D + dd for c in cross_cols for dd in (-1, 0, 1)})
    cross_q = H.crossing_regions(T * len(q) * ro, R)
    k1 = LAUNCH // ro                                    # the first boundary: day 0, region k1, row 0
    t3, r3 = divmod(3 * LAUNCH // ro, R)                 # the third: in day 1
    one_nan = [(0, 1, k1 - 1, 2), (0, 2, k1, 0)]         # (t, row, r, draw): items 2^25 - 3 and 2^25 + 2
    assert [((t * R + r) * ro + row) - LAUNCH for t, row, r, _ in one_nan] == [-3, 2] and t3 == 1
    reg, cls = H.extreme_sample(R, R, n_spread=64, rows=())
    reg = np.unique(np.concatenate([reg, bnd, cross_src, cross_q, [r3 - 1, r3, r3 + 1]]).astype(np.int64))
    S = set(reg.tolist())
    assert {0, 1, R - 2, R - 1} <= S and set(cls["spread"]) <= S
    assert len(bnd_items) == 24 and _both_sides(S, bnd_items, region_of) and days_met == [0, 1, 2]
    assert len(cross_cols) == (4 if f32 else 8) and set(cross_src) <= S and len(cross_q) == 4 and set(cross_q) <= S
    assert T * rows * B * es > (1 << (31 if f32 else 32)) and T * len(q) * ro * R * 8 > (1 << 31)
    # rule 1
    cols = (reg[:, None] * D + np.arange(D, dtype=np.int64)[None]).reshape(-1)
    flat = np.arange(T * rows, dtype=np.int64)[:, None] * B + cols[None]
    src_s = _ens_value(flat).astype(ndt).reshape(T, rows, cols.size)
    j_of = lambda r: int(np.searchsorted(reg, r))
    for t, row, r, e in one_nan:
        src[t, row, r * D + e] = float("nan")
        src_s[t, row, j_of(r) * D + e] = np.nan
    src[t3, 0, r3 * D:(r3 + 1) * D] = float("nan")
    src_s[t3, 0, j_of(r3) * D:(j_of(r3) + 1) * D] = np.nan
    sel = torch.as_tensor(reg, device=dev)
    held = src.index_select(2, torch.as_tensor(cols, device=dev)).cpu().numpy()
    assert held.dtype == src_s.dtype and np.array_equal(held, src_s, equal_nan=True), "device and host evaluate the formula differently"
    pop_s = N16[reg % 16]
    assert np.array_equal(pop.index_select(0, sel).cpu().numpy(), pop_s)
    # rule 2
    d = _lib.make_ens_desc(T, rows, R, D, q, storage=storage, derive_newcases=1)
    out = {k: H.poisoned(sh, torch.int32 if k == "count" else torch.float64, dev) for k, sh in _lib.ens_shapes(T, rows, R, len(q), 1).items()}
    outs = _lib.EnsOutputs()
    for k in _lib.ENS_OUT_NAMES:
        setattr(outs, k, C.c_void_p(out[k].data_ptr()))
    err = C.create_string_buffer(256)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    rc = _lib.lib().epi_ens_run_device(C.byref(d), C.c_void_p(src.data_ptr()), C.c_void_p(pop.data_ptr()), C.byref(outs),
                                       C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), err)
    _lib.check(rc, err)
    torch.cuda.synchronize(dev)
    t_call = time.perf_counter() - t0
    left = {k: _poison_words(t, H.POISON_RANK) for k, t in out.items()}
    assert not any(left.values()), ("outputs that still hold the poison pattern (words)", left)
    # rule 3
    want = E.summary(src_s, reg.size, D, q, population=pop_s)
    for k in _lib.ENS_OUT_NAMES:
        got = out[k].index_select(-1, sel).cpu().numpy()
        assert _bits_equal(got, want[k]), (k, "regions", reg[np.flatnonzero(~np.all(
            (got == want[k]) | (np.isnan(got) & np.isnan(want[k])), axis=tuple(range(got.ndim - 1))))][:12].tolist())
    cnt = want["count"]
    assert cnt[0, 1, j_of(k1 - 1)] == D - 1 and cnt[0, 3, j_of(k1 - 1)] == D - 1 and cnt[0, 2, j_of(k1)] == D - 1
    assert cnt[t3, 0, j_of(r3)] == 0 and cnt[t3, 3, j_of(r3)] == 0 and np.isnan(want["mean"][t3, 0, j_of(r3)])
    assert (np.delete(cnt, [j_of(k1 - 1), j_of(k1), j_of(r3)], axis=2) == D).all()
    _report(f"ens_summary {storage} T={T} rows={rows}+1 D={D} R={R} ({items} items, {-(-items // LAUNCH)} launches), sample {reg.size} regions",
            t_call, t_case, dev)
    del out, src, pop, held
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ robust fit
def _rf_level(c):
    return H.chain_hash(c, 7) % 5                  # NPI_MAXES - plan: integer levels 0 .. 4


def _rf_y(c):
    return _fl(_pos(c, 8)) * 2.0 ** -20            # (0, 1]


@pytest.fixture(scope="module")
def robfit_ref(tmp_path_factory):
    from tests.robust_fit_ref import RobfitRef
    return RobfitRef(tmp_path_factory.mktemp("robfit_ref_limits"))


def test_robust_fit_past_one_launch(gpu_device, robfit_ref):
    """epi_robfit_run_device with D = 9 days, n = 2 NPIs, R = 2^25 + 1000 regions, robust, max_iter = 3 (short, and most items
    stop at the cap: the MAXITER bit), bounds (0, Inf), all seven outputs.  n R = 2^26 + 2000 items: three launches of
    robfit_items<1>, the decode item -> (k, r) = (item / R, item % R) changes k inside the second; robfit_intercept<1> takes
    two launches over R.  X and weights hold 18 R > 2^29 doubles (byte offsets pass 2^31 and 2^32), y passes 2^31.  X is
    integer levels 0 .. 4, y dyadic; every eighth region's y is the exact line 1/4 + x_0 / 2 (converges at once: status 0);
    one non-finite y in the region at the first boundary.  Sampled regions, both NPIs of each, against tests/robust_fit_ref.c."""
    import torch
    from epidemicmodeling_amd import _lib
    from tests import robust_fit_ref as RF
    D, n, R, max_iter = 9, 2, (1 << 25) + 1000, 3
    items = n * R
    assert 2 * LAUNCH < items < 3 * LAUNCH and LAUNCH < R < 2 * LAUNCH and R * D * n <= 0x7FFFFFFF
    H.need_free(gpu_device, (2 * D * n + D + 3 * n + 1) * R * 8 + 2 * n * R * 4 + (3 << 30))
    t_case = time.perf_counter()
    dev = torch.device(gpu_device)
    X = H.formula_rows(D * n, R, dev, lambda c: _fl(_rf_level(c)), torch.float64).reshape(D, n, R)
    y = H.formula_rows(D, R, dev, _rf_y, torch.float64)
    y[:, ::8] = 0.25 + 0.5 * X[:, 0, ::8]
    bad_r = LAUNCH                                       # the first region of the second launch (items and intercepts)
    y[3, bad_r] = float("inf")
    bnd_items = H.boundary_items(LAUNCH, items)          # item = k R + r
    bnd_regions = H.boundary_items(LAUNCH, R)            # robfit_intercept
    cross_X, cross_y = H.crossing_regions(D * n, R), H.crossing_regions(D, R)
    reg, cls = H.extreme_sample(R, R, n_spread=150, rows=())
    exact = [0, 8, LAUNCH - 8, LAUNCH + 8, (R - 1) // 8 * 8]
    reg = np.unique(np.concatenate([reg, [i % R for i in bnd_items], bnd_regions, cross_X, cross_y, exact]).astype(np.int64))
    S = set(reg.tolist())
    assert {0, 1, R - 2, R - 1} <= S and set(cls["spread"]) <= S
    assert len(bnd_items) == 8 and _both_sides(S, bnd_items, lambda i: i % R) and {i // R for i in bnd_items} == {0, 1}
    assert len(bnd_regions) == 4 and set(bnd_regions) <= S
    assert len(cross_X) == 8 and set(cross_X) <= S and len(cross_y) == 4 and set(cross_y) <= S
    # rule 1
    cx = np.arange(D * n, dtype=np.int64)[:, None] * R + reg[None]
    Xs = _rf_level(cx).astype(np.float64).reshape(D, n, reg.size)
    ys = _rf_y(np.arange(D, dtype=np.int64)[:, None] * R + reg[None])
    ev = reg % 8 == 0
    ys[:, ev] = 0.25 + 0.5 * Xs[:, 0, ev]
    ys[3, int(np.searchsorted(reg, bad_r))] = np.inf
    sel = torch.as_tensor(reg, device=dev)
    assert np.array_equal(X.index_select(2, sel).cpu().numpy(), Xs) and np.array_equal(y.index_select(1, sel).cpu().numpy(), ys)
    # rule 2
    d = _lib.make_robfit_desc(R, D, n, 1, max_iter, 0.0, float("inf"))
    out = {k: H.poisoned(sh, torch.int32 if k in _lib.ROBFIT_OUT_I32 else torch.float64, dev) for k, sh in _lib.robfit_shapes(R, D, n).items()}
    outs = _lib.RobfitOutputs()
    for k in _lib.ROBFIT_OUT_NAMES:
        setattr(outs, k, C.c_void_p(out[k].data_ptr()))
    err = C.create_string_buffer(256)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    rc = _lib.lib().epi_robfit_run_device(C.byref(d), C.c_void_p(X.data_ptr()), C.c_void_p(y.data_ptr()), C.byref(outs),
                                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), err)
    _lib.check(rc, err)
    torch.cuda.synchronize(dev)
    t_call = time.perf_counter() - t0
    left = {k: _poison_words(t, H.POISON_RANK) for k, t in out.items()}
    assert not any(left.values()), ("outputs that still hold the poison pattern (words)", left)
    # rule 3
    want = robfit_ref.run(Xs, ys, robust=1, lower=0.0, upper=np.inf, max_iter=max_iter)
    for k in _lib.ROBFIT_OUT_NAMES:
        got = out[k].index_select(-1, sel).cpu().numpy()
        assert RF.same_bits(got, want[k]), (k, "regions", reg[np.flatnonzero(~np.all(
            (got == want[k]) | ((got != got) & (want[k] != want[k])), axis=tuple(range(got.ndim - 1))))][:12].tolist())
    st = want["status"]
    jb = int(np.searchsorted(reg, bad_r))
    assert (st[:, jb] == RF.NONFINITE).all() and np.isnan(want["b"][jb]) and (st[:, [jb - 1, jb + 1]] != RF.NONFINITE).all()
    assert (st == 0).any() and (st & RF.BOUND).any() and (st & RF.MAXITER).any() and (st == RF.NONFINITE).sum() == n, np.unique(st)
    assert (st[0, ev & (reg != bad_r)] == 0).all()
    _report(f"robust_fit D={D} n={n} R={R} max_iter={max_iter} ({items} items, 3 + 2 launches), sample {reg.size} regions", t_call, t_case, dev)
    del out, X, y
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------- AR forecaster
@pytest.fixture(scope="module")
def ar_ref(tmp_path_factory):
    from tests.ar_forecast_ref import ArRef
    return ArRef(tmp_path_factory.mktemp("arfc_limits"))


def test_ar_forecast_past_one_launch(gpu_device, ar_ref):
    """epi_arfc_run_device with fit = 1, p = 2, L = 5, H = 2, D = 2 draws, R = 2^25 + 1000 regions, z given, no drive: ar_fit
    takes two launches over R; ar_simulate two over R * bpr = R workgroups (bpr = 1: 62 of a workgroup's 64 lanes are
    inactive), the decode blk -> (r, d) = (blk / bpr, 64 (blk % bpr) + lane).  S is [7, 3, 2 R], 1.4e9 doubles or 11.3 GB: its
    byte offsets pass 2^31, 2^32 and 2^33; no other array of the call reaches 2^31.  seg is positive and dyadic, beta, s0, i0
    dyadic in (0, 1), z dyadic in [-2, 2).  A NaN planted in seg for region 2^25 - 1 (the last workgroup of the first launch)
    and for region 2^25 (the first of the second): both BAD_INPUT with NaN columns, their neighbours healthy.  Sampled regions,
    both chains of each, against tests/ar_forecast_ref.c.  The decode with bpr >= 2 past 2^25 workgroups would need
    R * 65 * 9 * 8 B = 78 GB of S: it stays with test_gpu_ar_forecast.py::test_chain_counts."""
    import torch
    from epidemicmodeling_amd import _lib
    from tests import ar_forecast_ref as AR
    p, L, Hh, D, R, dt = 2, 5, 2, 2, (1 << 25) + 1000, 0.5
    B, K = R * D, L + Hh
    assert LAUNCH < R < 2 * LAUNCH and -(-D // 64) == 1
    H.need_free(gpu_device, (K * 3 * B + L * R + Hh * B + 3 * R + (p + 1) * R) * 8 + R * 4 + (3 << 30))
    t_case = time.perf_counter()
    dev = torch.device(gpu_device)
    f_seg = lambda c: _fl(_pos(c, 12)) * 2.0 ** -20                 # (0, 1]
    f_beta = lambda c: _fl(_pos(c, 13)) * 2.0 ** -21                # (0, 1/2]
    f_s0 = lambda c: _fl((1 << 21) - _pos(c, 14)) * 2.0 ** -21      # [1/2, 1)
    f_i0 = lambda c: _fl(_pos(c, 15)) * 2.0 ** -24                  # (0, 1/16]
    f_z = lambda c: _fl(_sgn(c, 16)) * 2.0 ** -18                   # [-2, 2)
    seg = H.formula_rows(L, R, dev, f_seg, torch.float64)
    beta, s0, i0 = (H.formula_rows(1, R, dev, f, torch.float64).reshape(R) for f in (f_beta, f_s0, f_i0))
    z = H.formula_rows(Hh, B, dev, f_z, torch.float64)
    sick = [LAUNCH - 1, LAUNCH]
    for r in sick:
        seg[2, r] = float("nan")
    bnd = H.boundary_items(LAUNCH, R)                    # regions = workgroups of both kernels
    cross_S = sorted({c // D for c in H.crossing_regions(K * 3, B, bits=(31, 32, 33))})
    reg, cls = H.extreme_sample(R, R, n_spread=100, rows=())
    reg = np.unique(np.concatenate([reg, bnd, cross_S]).astype(np.int64))
    S_ = set(reg.tolist())
    assert {0, 1, R - 2, R - 1} <= S_ and set(cls["spread"]) <= S_
    assert bnd == [LAUNCH - 2, LAUNCH - 1, LAUNCH, LAUNCH + 1] and set(bnd) <= S_
    assert K * 3 * B * 8 > (1 << 33) and len(cross_S) >= 6 and set(cross_S) <= S_
    assert max(L * R, Hh * B) * 8 < (1 << 31)
    # rule 1
    rr = reg[None]
    seg_s = f_seg(np.arange(L, dtype=np.int64)[:, None] * R + rr)
    for r in sick:
        seg_s[2, int(np.searchsorted(reg, r))] = np.nan
    cols = (reg[:, None] * D + np.arange(D, dtype=np.int64)[None]).reshape(-1)
    z_s = f_z(np.arange(Hh, dtype=np.int64)[:, None] * B + cols[None])
    beta_s, s0_s, i0_s = f_beta(reg), f_s0(reg), f_i0(reg)
    sel, csel = torch.as_tensor(reg, device=dev), torch.as_tensor(cols, device=dev)
    assert np.array_equal(seg.index_select(1, sel).cpu().numpy(), seg_s, equal_nan=True)
    assert np.array_equal(z.index_select(1, csel).cpu().numpy(), z_s)
    for t, h in ((beta, beta_s), (s0, s0_s), (i0, i0_s)):
        assert np.array_equal(t.index_select(0, sel).cpu().numpy(), h) and (h > 0).all() and (h < 1).all()
    # rule 2
    d = _lib.make_arfc_desc(R, D, L, p, Hh, dt, fit=1)
    ins = _lib.ArfcInputs()
    for k, v in zip(_lib.ARFC_IN_NAMES, (seg, beta, s0, i0, z, None, None, None, None)):
        setattr(ins, k, None if v is None else C.c_void_p(v.data_ptr()))
    out = {k: H.poisoned(sh, torch.int32 if k == "status" else torch.float64, dev) for k, sh in _lib.arfc_shapes(R, D, L, p, Hh).items()}
    out["status"].fill_(H.POISON_STATUS)
    outs = _lib.ArfcOutputs()
    for k in _lib.ARFC_OUT_NAMES:
        setattr(outs, k, C.c_void_p(out[k].data_ptr()))
    err = C.create_string_buffer(256)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    rc = _lib.lib().epi_arfc_run_device(C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), err)
    _lib.check(rc, err)
    torch.cuda.synchronize(dev)
    t_call = time.perf_counter() - t0
    left = {k: _poison_words(t, H.POISON_STATUS) for k, t in out.items()}
    assert not any(left.values()), ("outputs that still hold the poison pattern (words)", left)
    # rule 3
    want = ar_ref.run(seg_s, beta_s, s0_s, i0_s, dt, p, Hh, D, z=z_s)
    got = {"S": out["S"].index_select(2, csel), "A": out["A_out"].index_select(1, sel), "noise_var": out["noise_var_out"].index_select(0, sel),
           "status": out["status"].index_select(0, sel)}
    for k, t in got.items():
        g = t.cpu().numpy()
        assert _bits_equal(g, want[k]), (k, "regions / chains", np.flatnonzero(~np.all(
            (g == want[k]) | ((g != g) & (want[k] != want[k])), axis=tuple(range(g.ndim - 1))))[:12].tolist())
    j0 = int(np.searchsorted(reg, sick[0]))
    st = want["status"]
    assert st[j0 - 1:j0 + 3].tolist() == [0, AR.ST_BAD_INPUT, AR.ST_BAD_INPUT, 0], st[j0 - 1:j0 + 3]
    Sw = want["S"].reshape(K, 3, reg.size, D)
    assert np.isnan(Sw[:, :, j0:j0 + 2]).all() and np.isfinite(Sw[:, :, [j0 - 1, j0 + 2]]).all()
    assert (st == AR.ST_BAD_INPUT).sum() == 2 and (st == 0).sum() == reg.size - 2, np.bincount(st)
    _report(f"ar_forecast p={p} L={L} H={Hh} D={D} R={R} (2 + 2 launches), sample {reg.size} regions", t_call, t_case, dev)
    del out, seg, z, got
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------ fusion
def _fuse_P(t, c, B, m, side):
    """the m * m rows (e = i + m j) of P = L L' of item (t, c): L lower-triangular from the hash, off-diagonal -2 .. 2, diagonal
    0 .. 3; a column whose diagonal is 0 is zero altogether, so rank L = the number of non-zero diagonals.  int64, exact."""
    idx = t * B + c
    Lm = {}
    for j in range(m):
        dj = H.chain_hash(idx, 100 + 50 * side + j * m + j) % 4
        Lm[j, j] = dj
        for i in range(j + 1, m):
            Lm[i, j] = (H.chain_hash(idx, 100 + 50 * side + i * m + j) % 5 - 2) * (dj != 0)
    rows = []
    for j in range(m):
        for i in range(m):
            acc = Lm[i, 0] * Lm[j, 0]
            for k in range(1, min(i, j) + 1):
                acc = acc + Lm[i, k] * Lm[j, k]
            rows.append(acc)
    return rows


def _fuse_s(t, c, B, m, side):
    return [_fl(_sgn(t * B + c, 200 + 10 * side + i)) * 2.0 ** -16 for i in range(m)]       # [-8, 8), 20 bits: exact in float


def _fuse_zero_diagonals(t, c, B, m):
    """number of axes k on which BOTH factors have a zero diagonal (S = Pf + Pb then has rank <= m - that)"""
    idx = t * B + c
    return sum(((H.chain_hash(idx, 100 + k * m + k) % 4 == 0) & (H.chain_hash(idx, 150 + k * m + k) % 4 == 0)).astype(np.int64)
               for k in range(m))


FUSE_CASES = [  # id, m, B, lane_block, storage, form, p_solver
    ("m3-blk4-f64-reference-pinv", 3, 7, 4, "f64", 0, 1),
    ("m6-classic-f32-information", 6, 1, 0, "f32", 1, 0),
]


@pytest.mark.parametrize("m,B,lane_block,storage,form,p_solver", [c[1:] for c in FUSE_CASES], ids=[c[0] for c in FUSE_CASES])
def test_two_filter_past_one_launch(gpu_device, m, B, lane_block, storage, form, p_solver):
    """epi_fuse_run_device over T = 2^23 + 1000 days, all five outputs.  B <= one workgroup of chains, so tiles = 1, day t is
    workgroup t and the second launch starts at day 2^23 (wg0 -> (t, tile) = (wg / tiles, wg % tiles)).
    (a) m = 3, B = 7 on 4-chain blocks (nblk = 2, one padding lane), double, the reference's form with pinv(S) * C: each P array
        is T * 72 doubles = 4.8 GB and passes 2^31 and 2^32 bytes (days 3 728 270 and 7 456 540); ~20 GB in all.  The padding
        lanes of s_out and P_out must still hold the poison afterwards.
    (b) m = 6, B = 1, classic layout, float storage, the information form; ~4 GB, no array reaches 2^31 bytes.
    P = L L' from small integer triangular factors (diagonal 0 .. 3, computed in int64 and converted: exact on both sides, ranks
    vary), state vectors dyadic.  Sampled days (the boundary's, the crossings', the ends, a spread, and the days of a 65 536-day
    scan whose factors share the most zero diagonals: the lowest ranks) against tests/two_filter_ref.fuse on those days alone --
    items are independent per (chain, day).  Crossing 2^23 workgroups with tiles >= 2 needs B > 256 (m = 3) or > 64 (m = 6)
    chains over 2^22 days, 78 GB or more: it stays with tests/test_gpu_two_filter.py."""
    import torch
    from epidemicmodeling_amd import _lib
    from tests import two_filter_ref as TF
    T = FUSE_LAUNCH + 1000
    f32 = storage == "f32"
    es, tdt, ndt = (4, torch.float32, np.float32) if f32 else (8, torch.float64, np.float64)
    blk = lane_block or B
    nblk = -(-B // blk)
    Bp = blk * nblk
    assert B <= (64 if m == 6 else 256) and FUSE_LAUNCH < T < 2 * FUSE_LAUNCH
    H.need_free(gpu_device, 3 * T * Bp * (m + m * m) * es + T * B * (12 + 8 * (m * (m + 1) // 2 + m * m)) + (4 << 30))
    t_case = time.perf_counter()
    dev = torch.device(gpu_device)

    def put(arr, row, val):                              # val [T, B] -> row `row` of the blocked [T, nblk, rows, blk]
        for cb in range(nblk):
            w = min(blk, B - cb * blk)
            arr[:, cb, row, :w] = val[:, cb * blk:cb * blk + w].to(arr.dtype)
    tt = torch.arange(T, dtype=torch.int64, device=dev)[:, None]
    cc = torch.arange(B, dtype=torch.int64, device=dev)[None, :]
    arrs = {}
    for side, (sn, Pn) in enumerate((("sf", "Pf"), ("sb", "Pb"))):
        arrs[sn] = torch.full((T, nblk, m, blk), float("nan"), dtype=tdt, device=dev)      # padding lanes: NaN, never read
        arrs[Pn] = torch.full((T, nblk, m * m, blk), float("nan"), dtype=tdt, device=dev)
        for i, v in enumerate(_fuse_s(tt, cc, B, m, side)):
            put(arrs[sn], i, v)
        for e, v in enumerate(_fuse_P(tt, cc, B, m, side)):
            put(arrs[Pn], e, v)
        del v
    # the sample
    bnd = H.boundary_items(FUSE_LAUNCH, T)
    day_elems = nblk * m * m * blk
    cross = [((1 << b) // es) // day_elems + dd for b in (31, 32) if (1 << b) // es < T * day_elems for dd in (-1, 0, 1)]
    scan = np.linspace(0, T - 1, 65536).astype(np.int64)
    zd = _fuse_zero_diagonals(scan[:, None], np.arange(B, dtype=np.int64)[None], B, m).max(axis=1)
    low = scan[np.argsort(-zd, kind="stable")[:8]].tolist()
    days, cls = H.extreme_sample(T, T, n_spread=40 if m == 3 else 120, rows=())
    days = np.unique(np.concatenate([days, bnd, cross, low]).astype(np.int64))
    S = set(days.tolist())
    assert {0, 1, T - 2, T - 1} <= S and set(cls["spread"]) <= S
    assert bnd == [FUSE_LAUNCH - 2, FUSE_LAUNCH - 1, FUSE_LAUNCH, FUSE_LAUNCH + 1] and set(bnd) <= S
    assert (len(cross) == 6 and set(cross) <= S and T * day_elems * es > (1 << 32)) if m == 3 else (not cross and T * day_elems * es < (1 << 31))
    # rule 1
    th, ch = days[:, None], np.arange(B, dtype=np.int64)[None, :]
    host = {}
    for side, (sn, Pn) in enumerate((("sf", "Pf"), ("sb", "Pb"))):
        host[sn] = np.stack([np.broadcast_to(v, (days.size, B)) for v in _fuse_s(th, ch, B, m, side)], axis=1).astype(ndt)
        host[Pn] = np.stack([np.broadcast_to(v, (days.size, B)) for v in _fuse_P(th, ch, B, m, side)], axis=1).astype(ndt)
    dsel = torch.as_tensor(days, device=dev)
    for k in ("sf", "Pf", "sb", "Pb"):
        held = arrs[k].index_select(0, dsel).cpu().numpy()
        assert held.dtype == host[k].dtype and np.array_equal(TF.from_blocked(held, B), host[k]), ("device and host evaluate the formula differently", k)
        assert np.isnan(held.transpose(0, 2, 1, 3).reshape(days.size, -1, Bp)[:, :, B:]).all()
    # rule 2
    d = _lib.make_fuse_desc(m, B, T, form, p_solver=p_solver, lane_block=lane_block, storage=int(f32))
    shapes = _lib.fuse_shapes(m, B, T, lane_block)
    odt = {"s_out": tdt, "P_out": tdt, "d2": torch.float64, "rank": torch.int32, "status": torch.int32}
    out = {k: H.poisoned(shapes[k], odt[k], dev) for k in _lib.FUSE_OUT_NAMES}
    ins, outs = _lib.FuseInputs(), _lib.FuseOutputs()
    for k in _lib.FUSE_IN_NAMES:
        setattr(ins, k, C.c_void_p(arrs[k].data_ptr()))
    for k in _lib.FUSE_OUT_NAMES:
        setattr(outs, k, C.c_void_p(out[k].data_ptr()))
    err = C.create_string_buffer(256)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    rc = _lib.lib().epi_fuse_run_device(C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), err)
    _lib.check(rc, err)
    torch.cuda.synchronize(dev)
    t_call = time.perf_counter() - t0
    left, pad_written = {}, {}
    for k, t in out.items():
        if k in ("s_out", "P_out"):
            hit = (t.view(torch.int32) == H.POISON32) if f32 else (t.view(torch.int64) == H.POISON64)
            hit = hit.reshape(T, nblk, -1, blk)
            left[k] = int(torch.count_nonzero(hit[:, :nblk - 1])) + int(torch.count_nonzero(hit[:, nblk - 1, :, :B - (nblk - 1) * blk]))
            pad_written[k] = int(torch.count_nonzero(~hit[:, nblk - 1, :, B - (nblk - 1) * blk:]))
        else:
            left[k] = _poison_words(t, H.POISON_RANK)
    assert not any(left.values()), ("outputs that still hold the poison pattern (words)", left)
    assert not any(pad_written.values()), ("padding lanes of a blocked output were written (words)", pad_written)
    # rule 3
    want = TF.fuse(host["sf"], host["Pf"], host["sb"], host["Pb"], form, p_solver, storage=storage)
    ranks = set(want["rank"].ravel().tolist())
    assert len(ranks) >= 3 and not want["status"].any(), ranks
    for k, name in (("s_out", "s"), ("P_out", "P")):
        g = TF.from_blocked(out[k].reshape(T, nblk, -1, blk).index_select(0, dsel).cpu().numpy(), B)
        assert TF.same_bits(g, want[name]), (k, "days", days[np.flatnonzero(~np.all(
            (g == want[name]) | ((g != g) & (want[name] != want[name])), axis=(1, 2)))][:12].tolist())
    for k in ("d2", "rank"):
        g = out[k].index_select(0, dsel).cpu().numpy()
        assert TF.same_bits(g, want[k]), (k, "days", days[np.flatnonzero(~np.all(
            (g == want[k]) | ((g != g) & (want[k] != want[k])), axis=1))][:12].tolist())
    # status is OR-ed over all T days of a chain, so the sample cannot predict it: no item is non-finite (bit 0 stays clear in
    # every chain), but the one-sided Jacobi iteration of the pseudo-inverse runs into its 30-sweep cap on ~1.3e-4 of these
    # integer matrices (diag(0, [13 6; 6 8]) is one: the oracle's orc_sym_pinv_ex reports 30 sweeps for it too, with the same
    # bits), which the call reports in bit 1; the restatement reports it too, but only for the sampled days it is run on
    st = out["status"].cpu().numpy()
    assert st.shape == (B,) and not (st & ~_lib.FUSE_SWEEP_CAP).any(), st
    _report(f"two_filter m={m} B={B} lane_block={lane_block} {storage} form={form} p_solver={p_solver} T={T} (2 launches), "
            f"sample {days.size} days, ranks {sorted(ranks)}", t_call, t_case, dev)
    del out, arrs
    torch.cuda.empty_cache()

"""The five newest device calls -- innovation log-likelihood (epi_loglik_run_device), the direct optimal-NPI planner
(epi_plan_run_device), smoother draws (epi_sdraw_run_device), forecast scores (epi_escore_run_device), path functionals
(epi_pathfn_run_device) -- at their production launch bounds and across the 2 / 4 / 8 GiB byte offsets of their arrays.

sdraw, escore and pathfn cut their grids at kSdLaunchGroups = 2^22, kEnsLaunchItems = 2^25 and kPfLaunchGroups = 2^22 and hand the
kernel the first workgroup / item of a launch (wg0, item0, group0); the small modules reach a second launch only through the
descriptor hooks test_launch_groups / test_launch_items / test_segments, with grids of a handful of workgroups, so neither the
constants nor the cap / (nseg * nz) arithmetic of launch_paths ran at their real values.  loglik runs ll_blocks as one 2-D grid
(ceil(B / 256), ceil(T / 32)) whose grid.y never exceeded 3; npi_plan is one launch of ceil(R P / 64) wavefronts whose largest
batch was 257 chains.  No offset of the five -- slot M blk + cr and t bp + c against t B + c, ((t n + k) B + c), (k - k0) 3 N + p,
(s 5 n_thr + j) M + m, (t n_a + k) plane + .. -- was ever evaluated past a few thousand elements.

The cases follow the three rules of tests/test_gpu_call_limits.py and tests/test_gpu_regression_limits.py:

 1. inputs by formula per element (helpers.chain_hash, hash_pos, hash_sgn; small integers and dyadic values of 20 significant
    bits, exact in float; sdraw's S- = S+ plus units of 2^-30 is rounded once to the storage type on both sides), evaluated by
    torch on the device for the whole array and by NumPy for the sample, the two compared bit for bit before the call;
 2. every output poisoned (helpers.poisoned), and the workspace where the call must fill it (sdraw's records, pathfn's partial
    records) or must leave it alone (escore with every item output given); after the call no word of any output of the WHOLE call
    may still hold the poison.  Exceptions: the padding lanes of the blocked INPUTS hold NaN and are never read (the outputs
    of these calls are unpadded); sdraw's status is zeroed by the call and OR-ed into, so no poison survives there either;
 3. the sample -- both sides of every launch boundary, both sides of the element where each array's byte offset first reaches
    2^31, 2^32, 2^33, items 0, 1, last - 1, last, a spread (helpers.extreme_sample) -- equals, bit for bit and NaN to NaN, the
    family's C restatement (tests/loglik_ref.c, npi_plan_ref.c, sdraw_ref.c, escore_ref.c, pathfn_ref.c through their Python
    loaders) run on the sample alone.  The sample is a self-contained sub-problem: whole regions (all D members / draws, all P
    weights) for escore, pathfn and npi_plan, whole chains for sdraw, whole groups of G chains for loglik.  Each test asserts that
    its sample holds these classes and that the arrays pass exactly the offsets listed here (_assert_passes, over EVERY array).

The cases and which of 2^31 / 2^32 / 2^33 bytes each array passes (an array not named stays below 2^31):
  L1  loglik, 3-state, classic, double, r_mode 0 (ll_replay), B = 2^22 + 40, T = 65, L = 4, G = 8, nine outputs.
      P_MINUS [65, 9, B] all three; S_MINUS 2^31, 2^32; innovations, x, S, nis, R_used [65, B] 2^31.
  L2  loglik, 6-state, time-flipped, lane_block 64 (Bp = B + 24), float, r_mode 1, B = 2^21 + 40, T = 33, Sx = 2^16 + 3.
      P_MINUS [33, nblk, 36, 64] float all three.
  L3  loglik, B = 5, T = 32 x 65 535 (grid.y at its limit), r_mode 1, every chain and day compared; T + 1: EPI_ERR_UNSUPPORTED.
  N1  npi_plan, R = 2^20 + 25, P = 4, H = 22, n = 12, max_iter = 3, prefix, u_fixed, u_init, eleven outputs.
      plan, u_init (and the workspace's second plan) all three; states, mu, u_fixed 2^31.
  S1  sdraw, B = 2^20 + 36, classic, double, T = 43, D = 2, k0 = 41.  workspace [43, B, 24] all three; P_PLUS, P_MINUS, J, L 2^31.
  S2  sdraw, B = 1 073 800 in 256-chain blocks, D = 1000, T = 2, float storage / z / X: 2^22 + 228 path workgroups, two
      launches, the boundary path 2^30 inside chain 1 073 741.  X, z [2, 3, N] float all three.
  E1  escore, double and float, T = 3, rows 3 + 1, D = 9, R = 2^24 + 1000: seven launches.  src all three (float: 2^31, 2^32);
      width 2^31.
  P1  pathfn, R = 2^17 + 10, D = 2, eight thresholds, T = 40, window 3 .. 36: pathfn_regions in two launches.  None.
  P2  pathfn, rows 35 + 1, R = 2^22 + 125, D = 8, T = 2, float: the second launch_paths call (nz = 32, per = 2^17) in two
      launches, pathfn_regions in 37.  src, total, peak_day, first_cross all three; n_valid 2^31, 2^32.
  P3  pathfn, R = 2^18 + 3, D = 8, T = 256, test_segments = 8, eight thresholds, float.  p_thr [8, 5, 8, M] int32 all three;
      src 2^31, 2^32.
N1's start state is (0.9, 0.05, 0.25), not the trained tables' (0.97, 2e-3, 0.25): from the latter every chain of this horizon
stops at its second iteration whatever tol is; tol = 1e-3 then gives two iteration counts, and the chains of three carry the cap bit.
S2: with T = 2 a sample of sixty chains holds a rank-deficient day only by luck, so 20 000 chains are scanned with the
restatement's gains and the first two rank-deficient ones join the sample.

Showing that the tests bite (scratch builds of the library with one line of index arithmetic changed, never committed; every
access stays inside its array):
  (i)    escore_items with item = blockIdx.x (item0 dropped): E1 fails in both storages on rule 2 -- every later launch rewrites
         the items of the first, and the 167 784 160 = 12 R - 2^25 items behind it keep the poison in each of the seven item
         outputs (width: twice as many words).
  (ii)   pathfn_regions with g = blockIdx.x (group0 dropped): P1, P2 and P3 all fail on rule 2 (P1: 17 313 384 words of
         cross_day_hist and the counts behind workgroup 2^22; P2: 146 805 140 = 36 R - 2^22 words of n_paths; P3's region pass
         has 9.4 M workgroups and loses its tail in the same way).
  (iii)  pathfn_paths with the element offset of its p_thr stores taken through 32 bits of bytes ((uint32_t)(.. * 4) / 4): P3
         alone fails, on rule 2 over the workspace -- 1 342 204 928 words of p_int / p_thr, everything past 4 GiB, are never
         written; P1 and P2 (one segment, no partial records) pass.
  (iv)   sdraw_paths with p = blockIdx.x * 256 + lane (wg0 dropped): S2 fails on rule 2 -- 349 056 words of X, the six words of
         each of the 58 176 paths behind path 2^30, keep the poison; S1 (one launch) passes.
  (v)    sdraw_gain with the record's offset taken through 32 bits of bytes: S1 fails on rule 2 -- the records past 4 GiB are
         never written, sdraw_paths reads poison there and copies it into X (12 583 344 words, X's whole size: every chain
         has a day whose record lies past 4 GiB); S2 (a workspace of 0.4 GB) passes.
  (vi)   plan_solve reading u_init through 32 bits of bytes: N1 fails on rule 3, at J0 of one sampled region (423 902), in one
         word: the wrapped offset reads another element of the same 0 / 1 / 2 formula, and a chain that reaches its vertex
         forgets its start -- only the chains that stop at the cap keep a trace of it.  The case sees a wrong READ of the start
         plan weakly; a wrong write of plan, states or mu is caught by rule 2 or by every sampled word.
  (vii)  ll_blocks with P_MINUS's offset masked to 2^29 elements: L1 fails on rule 3 in all 400 sampled chains (loglik), L2 in
         all 448; L3 (P_MINUS of 0.75 GB) passes.
  (viii) ll_blocks with blockIdx.y & 0x7FFF: L3 fails on rule 2 -- 5 242 720 = 5 x 32 x 32 767 words each of S, nis and R_used,
         the days of blocks 32 768 .. 65 534, keep the poison; L1 and L2 (three and two blocks) pass.

What stays unreachable on one device: sdraw's gain grid past 2^22 workgroups (it needs T B > 2^30: the workspace alone would be
206 GB); pathfn's combine loop past one launch (rows N > 2^30 over at least 64 days); the product limits themselves.  They stay
with the descriptor hooks and the *_abi.py / *_emu.py tests.

Measured on one MI355X (the library call alone / the whole case with input generation, sampling and the restatement /
torch.cuda.max_memory_allocated):
  L1  0.01 s / 0.3 - 5.0 s / 41.3 GiB  L2  0.00 s / 0.2 s / 14.4 GiB        L3  0.01 s / 2.4 s /   1.9 GiB
  N1  0.05 s / 0.2 - 3.4 s / 45.4 GiB  S1  0.02 s / 0.1 - 1.3 s / 32.1 GiB  S2  0.02 s / 3.8 - 4.7 s / 103.4 GiB
  E1, double  0.16 s / 1.1 - 2.1 s / 42.0 GiB                               E1, float  0.15 s / 1.8 s / 36.9 GiB
  P1  0.01 s / 0.1 s /  2.3 GiB        P2  0.14 s / 2.5 - 2.8 s / 70.1 GiB  P3  0.04 s / 2.5 s / 44.9 GiB
The ranges are four runs: a fresh allocation of 40 GiB takes up to some seconds on one case or another, a different one every run
(DESIGN.md 2 has the same of the addressing module).  The peaks of the float cases S2 and P3 are about twice the arrays of the call
(S2: 51.6 GB of X and z): temporaries of the formulas and of the poison counts come on top, and need_free asks for that much.
The module takes 24 - 25 s (the three older limits modules: 5 s, 6 s, 23 - 37 s); S2, the largest case, takes 4 - 5 s in the whole
suite; no case came near 10 s, so H, max_iter and D stand as the cases above give them.
No time is asserted; every case prints its figures in a line that starts with [limits].
"""
import ctypes as C
import time

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

BITS = (31, 32, 33)
ES_LAUNCH = 1 << 25         # kEnsLaunchItems (ens_score.hpp cuts its grid with it)
PF_LAUNCH = 1 << 22         # kPfLaunchGroups
SD_LAUNCH = 1 << 22         # kSdLaunchGroups
NAN, INF = float("nan"), float("inf")


# the pieces the cases share live in tests/helpers.py
_dyadic10 = H.dyadic10
_with_nan = H.with_nan
_assert_passes = H.assert_passes
_crossing = H.crossing_sample
_sample = H.region_sample
_no_poison = H.assert_no_poison
_compare = H.compare_sample
_call = H.timed_device_call
_population = H.cycled_population
_scaled_rows = H.scaled_rows


# ------------------------------------------------------------------------------------------------------------------ escore
@pytest.fixture(scope="module")
def escore_c(tmp_path_factory):
    from tests.escore_ref import EscoreC
    return EscoreC(tmp_path_factory.mktemp("escore_ref_limits"))


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_escore_past_one_launch(gpu_device, escore_c, storage):
    """E1.  epi_escore_run_device with T = 3, rows = 3 + the derived row, D = 9 members, R = 2^24 + 1000 regions, two levels, four
    PIT bins, k0 = 0, k1 = 3, first_day 0 .. 2 by formula, all fourteen outputs: 12 R = 6 x 2^25 + 12 000 items in seven launches
    of escore_items<1>; the decode item -> (t, r, row) = ((item / 4) / R, (item / 4) % R, item % 4) meets a launch boundary twice
    in every day.  src [3, 3, 9 R] passes 2^31, 2^32 and (double) 2^33 bytes; width [3, 2, 4, R] passes 2^31; every other array
    stays below 2^31.  Planted: a NaN member in the item three before and in the item two behind the first boundary, an all-NaN
    item at the third boundary, a NaN truth in region 1.  The sampled regions -- every day and row of each -- against
    tests/escore_ref.c on their own columns."""
    import torch
    from epidemicmodeling_amd import _lib
    T, rows, D, R, alpha, n_bins = 3, 3, 9, (1 << 24) + 1000, (0.5, 0.05), 4
    ro, B, n_a = rows + 1, R * D, len(alpha)
    f32 = storage == "f32"
    es, tdt, ndt = (4, torch.float32, np.float32) if f32 else (8, torch.float64, np.float64)
    items = T * ro * R
    assert 6 * ES_LAUNCH < items < 7 * ES_LAUNCH and B <= 0x7FFFFFFF
    shapes = _lib.escore_shapes(T, rows, R, n_a, n_bins, 1)
    nbytes = {k: int(np.prod(sh, dtype=np.int64)) * (4 if k in _lib.ESCORE_OUT_I32 else 8) for k, sh in shapes.items()}
    nbytes.update(src=T * rows * B * es, truth=T * ro * R * 8, population=R * 8, first_day=R * 4)
    _assert_passes(nbytes, {"src": (31, 32) if f32 else BITS, "width": (31,)})
    ws_bytes = items * 40
    H.need_free(gpu_device, sum(nbytes.values()) + ws_bytes + (12 << 30))
    t_case = time.perf_counter()
    dev = torch.device(gpu_device)
    value, first_day = _dyadic10(61), lambda c: H.chain_hash(c, 63) % 3
    truth_dev, truth_host = _scaled_rows(_dyadic10(62), ro, 3, 2.0 ** 37)
    src = H.formula_rows(T * rows, B, dev, value, tdt).reshape(T, rows, B)
    truth = truth_dev(T, R, dev)
    fd = first_day(torch.arange(R, dtype=torch.int64, device=dev)).to(torch.int32)
    pop, N16 = _population(R, dev)
    # the sample
    bnd_items = H.boundary_items(ES_LAUNCH, items)
    region_of = lambda i: (i // ro) % R
    k1 = ES_LAUNCH // ro                                 # the first boundary: day 0, region k1, row 0
    t3, r3 = divmod(3 * ES_LAUNCH // ro, R)              # the third: in day 1
    one_nan = [(0, 1, k1 - 1, 2), (0, 2, k1, 0)]         # (t, row, r, member): items 2^25 - 3 and 2^25 + 2
    assert [((t * R + r) * ro + row) - ES_LAUNCH for t, row, r, _ in one_nan] == [-3, 2] and t3 == 1
    cross_src = _crossing(T * rows, B, es, H.passed_bits(nbytes["src"]), of=lambda c: c // D)
    cross_w = _crossing(T * n_a * ro, R, 8, (31,))
    reg, S = _sample(R, 48, [region_of(i) for i in bnd_items], cross_src, cross_w, [r3 - 1, r3, r3 + 1])
    assert len(bnd_items) == 24 and H.both_sides(S, bnd_items, region_of) and sorted({(i // ro) // R for i in bnd_items}) == [0, 1, 2]
    assert set(cross_src) <= S and set(cross_w) <= S
    # rule 1
    cols = H.region_columns(reg, D)
    j_of = lambda r: int(np.searchsorted(reg, r))
    src_s = H.formula_sample(T * rows, B, cols, value, ndt).reshape(T, rows, cols.size)
    truth_s = truth_host(T, R, reg)
    for t, row, r, e in one_nan:
        src[t, row, r * D + e] = NAN
        src_s[t, row, j_of(r) * D + e] = np.nan
    src[t3, 0, r3 * D:(r3 + 1) * D] = NAN
    src_s[t3, 0, j_of(r3) * D:(j_of(r3) + 1) * D] = np.nan
    truth[2, 1, 1] = NAN
    truth_s[2, 1, j_of(1)] = np.nan
    fd_s, pop_s = first_day(reg).astype(np.int32), N16[reg % 16]
    sel, csel = torch.as_tensor(reg, device=dev), torch.as_tensor(cols, device=dev)
    held = H.selected(src, csel)
    assert held.dtype == src_s.dtype and np.array_equal(held, src_s, equal_nan=True), "device and host evaluate the formula differently"
    assert np.array_equal(H.selected(truth, sel), truth_s, equal_nan=True) and np.array_equal(H.selected(fd, sel), fd_s)
    assert np.array_equal(H.selected(pop, sel), pop_s) and set(fd_s.tolist()) == {0, 1, 2}
    # rule 2
    d = _lib.make_escore_desc(T, rows, R, D, R, alpha, n_bins, storage=storage, derive_newcases=1, k0=0, k1=T)
    out = {k: H.poisoned(sh, torch.int32 if k in _lib.ESCORE_OUT_I32 else torch.float64, dev) for k, sh in shapes.items()}
    ins, outs = _lib.EscoreInputs(), _lib.EscoreOutputs()
    for k, v in zip(_lib.ESCORE_IN_NAMES, (src, pop, truth, None, fd)):
        setattr(ins, k, None if v is None else C.c_void_p(v.data_ptr()))
    for k in _lib.ESCORE_OUT_NAMES:
        setattr(outs, k, C.c_void_p(out[k].data_ptr()))
    ws = H.poisoned_words(ws_bytes // 8, dev)            # every item output is handed over: the call must leave the workspace alone
    t_call = _call("epi_escore_run_device", dev, C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(ws.data_ptr()), C.c_size_t(ws_bytes))
    _no_poison(out)
    assert H.poison_words(ws, 0) == ws.numel(), "the workspace was written although every item output was given"
    # rule 3
    want = escore_c.score(src_s, truth_s, reg.size, D, alpha, n_bins, population=pop_s, first_day=fd_s, k0=0, k1=T)
    _compare(out, want, sel, reg)
    cnt, rk = want["count"], want["rank"]
    assert cnt[0, 1, j_of(k1 - 1)] == D - 1 and cnt[0, 3, j_of(k1 - 1)] == D - 1 and cnt[0, 2, j_of(k1)] == D - 1
    assert cnt[t3, 0, j_of(r3)] == 0 and cnt[t3, 3, j_of(r3)] == 0 and rk[t3, 0, j_of(r3)] == -1 and rk[2, 1, j_of(1)] == -1
    assert (np.delete(cnt, [j_of(k1 - 1), j_of(k1), j_of(r3)], axis=2) == D).all() and (rk < 0).sum() == 3
    assert len(np.unique(rk[:, :3])) >= D and np.array_equal(want["n_scored"][2], T - fd_s) and (want["pit_hist"].sum(axis=0) == want["n_scored"]).all()
    H.report_limits(f"escore {storage} T={T} rows={rows}+1 D={D} R={R} ({items} items, {-(-items // ES_LAUNCH)} launches), sample {reg.size} regions",
                    t_call, t_case, dev)
    del out, src, truth, ws, held
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------ pathfn
@pytest.fixture(scope="module")
def pathfn_c(tmp_path_factory):
    from tests.pathfn_ref import PathfnC
    return PathfnC(tmp_path_factory.mktemp("pathfn_ref_limits"))


def _pf_thr(c):
    """a threshold: dyadic in (0, 1024]; NaN (not asked) for one hash value in eight, -Inf (every valid day is above) for another"""
    h = H.chain_hash(c, 74) % 8
    return H.replaced(h == 1, -INF, H.replaced(h == 0, NAN, _dyadic10(73)(c)))


_pf_value = _with_nan(_dyadic10(71), 72, 16)             # a path's day: dyadic in (0, 1024], one in sixteen NaN


def _pathfn_case(gpu_device, cref, what, *, T, rows, R, D, n_thr, storage, k0, k1, names, segments, passes, ws_passes, boundaries, n_spread=40):
    """One pathfn case.  names: the outputs asked for; passes: {array: bits} over the inputs and those outputs; ws_passes: the
    same for the arrays of the workspace that the call must fill (the segments' partial records; empty without segments);
    boundaries(geom) -> [(label, [regions on both sides of a launch boundary])].  Returns (want, reg, geom)."""
    import torch
    from epidemicmodeling_amd import _lib
    ro, N = rows + 1, R * D
    M, W = ro * N, k1 - k0
    f32 = storage == "f32"
    es, tdt, ndt = (4, torch.float32, np.float32) if f32 else (8, torch.float64, np.float64)
    d = _lib.make_pathfn_desc(T, rows, R, D, n_thr, storage=storage, derive_newcases=1, k0=k0, k1=k1, test_segments=segments)
    nblk = -(-W // 32)
    nseg = max(1, segments)
    assert segments == 0 and (-(-N // 64)) * (rows - 2) >= 1024 or segments > 1 and nblk % segments == 0      # the library's rule: one segment
    shapes = {k: sh for k, sh in _lib.pathfn_shapes(rows, R, D, n_thr, W, 1).items() if k in names}
    assert set(shapes) == set(names)
    nbytes = {k: int(np.prod(sh, dtype=np.int64)) * (4 if k in _lib.PATHFN_OUT_I32 else 8) for k, sh in shapes.items()}
    nbytes.update(src=T * rows * N * es, thr=n_thr * ro * R * 8, population=R * 8, first_day=R * 4)
    _assert_passes(nbytes, passes)
    # the workspace: peak_day [M], first_cross [n_thr][M] (doubles), then p_mx, p_mn [nseg][M], p_bsum [nblk][M], p_int [nseg][3][M],
    # p_thr [nseg][5][n_thr][M] (int32)
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    _lib.check(_lib.lib().epi_pathfn_workspace_bytes(C.byref(d), C.byref(n), err), err)
    head = (1 + n_thr) * M
    parts = {} if nseg == 1 else {"p_mx": (nseg * M, 8), "p_mn": (nseg * M, 8), "p_bsum": (nblk * M, 8), "p_int": (nseg * 3 * M, 4),
                                  "p_thr": (nseg * 5 * n_thr * M, 4)}
    assert n.value == head * 8 + sum(c * sz for c, sz in parts.values())
    _assert_passes({k: c * sz for k, (c, sz) in parts.items()}, ws_passes)
    H.need_free(gpu_device, 2 * (sum(nbytes.values()) + n.value) + (3 << 30))      # the measured peak: up to twice the arrays
    t_case = time.perf_counter()
    dev = torch.device(gpu_device)
    # first_day: 0 .. k0 + 2, on both sides of the window's first day; one region in eight starts at T and has no valid day
    first_day = lambda c: H.chain_hash(c, 75) % (k0 + 3) + (T - H.chain_hash(c, 75) % (k0 + 3)) * ((H.chain_hash(c, 76) % 8 == 0) * 1)
    thr_dev, thr_host = _scaled_rows(_pf_thr, ro, 3, 2.0 ** 37)
    src = H.formula_rows(T * rows, N, dev, _pf_value, tdt).reshape(T, rows, N)
    thr = thr_dev(n_thr, R, dev)
    fd = first_day(torch.arange(R, dtype=torch.int64, device=dev)).to(torch.int32)
    pop, N16 = _population(R, dev)
    # the sample
    geom = dict(N=N, M=M, pg=-(-N // 256), nseg=nseg, ro=ro)
    more, S_need = [], []
    for label, regs in boundaries(geom):
        assert regs and all(0 <= r < R for r in regs), (label, regs)
        more.append(regs)
        S_need.append((label, regs))
    path_of = lambda c: (c % N) // D                                     # a column of an array [.., M] or [.., N] -> its region
    cross = {"src": _crossing(T * rows, N, es, passes.get("src", ()), of=path_of)}
    for k, sh in shapes.items():
        last = sh[-1]
        cross[k] = _crossing(int(np.prod(sh[:-1], dtype=np.int64)), last, 4 if k in _lib.PATHFN_OUT_I32 else 8, passes.get(k, ()),
                             of=path_of if last == N else (lambda c: c))
    for k, (c, sz) in parts.items():
        cross[k] = _crossing(c // M, M, sz, ws_passes.get(k, ()), of=path_of)
    reg, S = _sample(R, n_spread, *more, *cross.values())
    assert all(set(regs) <= S for _, regs in S_need) and all(set(v) <= S for v in cross.values())
    # rule 1
    cols = H.region_columns(reg, D)
    src_s = H.formula_sample(T * rows, N, cols, _pf_value, ndt).reshape(T, rows, cols.size)
    thr_s = thr_host(n_thr, R, reg)
    fd_s, pop_s = first_day(reg).astype(np.int32), N16[reg % 16]
    sel, csel = torch.as_tensor(reg, device=dev), torch.as_tensor(cols, device=dev)
    held = H.selected(src, csel)
    assert held.dtype == src_s.dtype and np.array_equal(held, src_s, equal_nan=True), "device and host evaluate the formula differently"
    assert np.array_equal(H.selected(thr, sel), thr_s, equal_nan=True) and np.array_equal(H.selected(fd, sel), fd_s)
    assert np.array_equal(H.selected(pop, sel), pop_s) and fd_s.min() <= k0 < np.sort(np.unique(fd_s))[-2] and fd_s.max() == T
    # rule 2
    out = {k: H.poisoned(sh, torch.int32 if k in _lib.PATHFN_OUT_I32 else torch.float64, dev) for k, sh in shapes.items()}
    ins, outs = _lib.PathfnInputs(), _lib.PathfnOutputs()
    for k, v in zip(_lib.PATHFN_IN_NAMES, (src, pop, thr, fd)):
        setattr(ins, k, C.c_void_p(v.data_ptr()))
    for k in _lib.PATHFN_OUT_NAMES:
        setattr(outs, k, C.c_void_p(out[k].data_ptr()) if k in out else None)
    ws = H.poisoned_words(-(-n.value // 8), dev)
    wi = ws[head + (2 * nseg + nblk) * M * (nseg > 1):].view(torch.int32)
    wi.fill_(H.POISON_RANK)                                              # the int32 records: a day or a count is never -7
    t_call = _call("epi_pathfn_run_device", dev, C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(ws.data_ptr()), C.c_size_t(n.value))
    _no_poison(out)
    if nseg > 1:
        left = {"p_mx, p_mn, p_bsum": H.poison_words(ws[head:head + (2 * nseg + nblk) * M], 0),
                "p_int, p_thr": H.poison_words(wi[:nseg * (3 + 5 * n_thr) * M], H.POISON_RANK)}
        assert not any(left.values()), ("partial records that still hold the poison pattern (words)", left)
    # rule 3
    want = cref.functionals(src_s, reg.size, D, thr_s, population=pop_s, first_day=fd_s, k0=k0, k1=k1)
    _compare(out, want, {k: csel if shapes[k][-1] == N else sel for k in out}, reg)
    assert (want["n_valid"] == 0).any() and len(np.unique(want["n_valid"])) >= 3 and np.isnan(want["peak_day"]).any()
    if "first_cross" in want and n_thr:
        fc = want["first_cross"]
        assert np.isnan(fc).any() and (fc >= k0).any()
    H.report_limits(f"pathfn {what} {storage} T={T} rows={rows}+1 D={D} R={R} n_thr={n_thr} window {k0}..{k1} segments={nseg}, "
                    f"sample {reg.size} regions", t_call, t_case, dev)
    del out, src, thr, ws, wi, held
    torch.cuda.empty_cache()
    return want, reg, geom


def _around(p_first, D, R):
    """the regions of the last path before and the first path of a launch, and their neighbours"""
    return sorted({r for r in ((p_first - 1) // D - 1, (p_first - 1) // D, p_first // D, p_first // D + 1) if 0 <= r < R})


def test_pathfn_region_pass_past_one_launch(gpu_device, pathfn_c):
    """P1.  epi_pathfn_run_device with T = 40, window 3 .. 36, rows = 3 + the derived row, D = 2, R = 2^17 + 10, eight thresholds,
    every output: pathfn_regions runs 9 x 4 x R = 4 718 952 workgroups (h, q, r), more than 2^22: two launches, whose boundary
    decodes to h = 7 (the crossings of threshold 6), q = 3, inside a plane.  No array reaches 2^31 bytes."""
    from epidemicmodeling_amd import _lib
    T, rows, R, D, n_thr = 40, 3, (1 << 17) + 10, 2, 8
    rg = (1 + n_thr) * (rows + 1) * R
    assert PF_LAUNCH < rg < 2 * PF_LAUNCH and PF_LAUNCH // ((rows + 1) * R) == 7 and 0 < PF_LAUNCH % R < R - 2
    bnd = [g % R for g in H.boundary_items(PF_LAUNCH, rg)]
    assert len(bnd) == 4 and bnd == list(range(bnd[0], bnd[0] + 4))
    _pathfn_case(gpu_device, pathfn_c, "P1", T=T, rows=rows, R=R, D=D, n_thr=n_thr, storage="f64", k0=3, k1=36,
                 names=_lib.PATHFN_OUT_NAMES, segments=0, passes={}, ws_passes={}, boundaries=lambda g: [("pathfn_regions", bnd)])


def test_pathfn_path_grid_past_one_launch(gpu_device, pathfn_c):
    """P2.  rows = 35 + the derived row, R = 2^22 + 125, D = 8 (N = 2^25 + 1000 paths in 131 076 workgroups), T = 2, float source,
    one threshold; outputs total, peak_day, n_valid, first_cross, n_paths.  The derived group (rows 0, 1, 2 and the derived row in
    one lane, grid.z = 1) takes one launch; the 32 other rows go into grid.z, so a launch holds 2^22 / 32 = 2^17 workgroups and
    the second starts at path 2^25, the first of region 2^22.  pathfn_regions takes 36 R workgroups in 37 launches.  src (9.4 GB)
    and each double output [36, N] (9.66 GB) pass 2^31, 2^32 and 2^33 bytes; n_valid passes 2^31 and 2^32."""
    T, rows, R, D, n_thr = 2, 35, (1 << 22) + 125, 8, 1
    ro, N = rows + 1, R * D
    pg = -(-N // 256)
    per = PF_LAUNCH // (rows - 3)
    assert pg <= PF_LAUNCH and per == 1 << 17 and per < pg <= 2 * per and N == (1 << 25) + 1000
    rg = ro * R
    bnd_r = sorted({g % R for g in H.boundary_items(PF_LAUNCH, rg)})
    assert -(-rg // PF_LAUNCH) == 37
    _pathfn_case(gpu_device, pathfn_c, "P2", T=T, rows=rows, R=R, D=D, n_thr=n_thr, storage="f32", k0=0, k1=2,
                 names=("total", "peak_day", "n_valid", "first_cross", "n_paths"), segments=0,
                 passes={"src": BITS, "total": BITS, "peak_day": BITS, "first_cross": BITS, "n_valid": (31, 32)}, ws_passes={},
                 boundaries=lambda g: [("pathfn_paths, rows 3 .. 34", _around(per * 256, D, R)), ("pathfn_regions", bnd_r)], n_spread=24)


def test_pathfn_segment_records_across_byte_offsets(gpu_device, pathfn_c):
    """P3.  rows = 3 + the derived row, R = 2^18 + 3, D = 8, T = 256, the whole window in eight segments of one 32-day block
    (test_segments = 8), eight thresholds, float source; every per-path output, n_paths and n_cross.  The workspace is poisoned:
    pathfn_paths must fill every partial record, pathfn_combine folds them.  p_thr [8, 5, 8, M] int32 (10.7 GB) passes 2^31, 2^32
    and 2^33 bytes, src 2^31 and 2^32; the paths on both sides of each of those elements are sampled."""
    from epidemicmodeling_amd import _lib
    T, rows, R, D, n_thr = 256, 3, (1 << 18) + 3, 8, 8
    names = [k for k in _lib.PATHFN_OUT_NAMES if not k.endswith("_hist")]
    want, reg, geom = _pathfn_case(gpu_device, pathfn_c, "P3", T=T, rows=rows, R=R, D=D, n_thr=n_thr, storage="f32", k0=0, k1=T, names=names,
                                   segments=8, passes={"src": (31, 32)}, ws_passes={"p_thr": BITS},
                                   boundaries=lambda g: [("ends", [0, R - 1])])
    run = want["longest_run"]
    assert (run[np.isfinite(run)] > 32).any()                          # runs longer than a segment: the prefix / suffix join


# ------------------------------------------------------------------------------------------------------------------- sdraw
@pytest.fixture(scope="module")
def sdraw_ref(tmp_path_factory):
    from tests.sdraw_ref import SdrawRef
    return SdrawRef(tmp_path_factory.mktemp("sdraw_ref_limits"))


def _sd_factor(idx, side):
    """the nine rows (entry i + 3 j) of L L', L an integer lower-triangular factor of item idx: diagonal 1 .. 3, below it -2 .. 2"""
    Lm = {}
    for j in range(3):
        for i in range(j, 3):
            h = H.chain_hash(idx, 300 + 20 * side + 3 * i + j)
            Lm[i, j] = h % 3 + 1 if i == j else h % 5 - 2
    rows = []
    for j in range(3):
        for i in range(3):
            acc = Lm[i, 0] * Lm[j, 0]
            for k in range(1, min(i, j) + 1):
                acc = acc + Lm[i, k] * Lm[j, k]
            rows.append(acc)
    return rows


def _sd_values(idx):
    """{array: its rows} of the items idx = t B + c (int64, NumPy or torch), in double.  P+ = L L' 2^-24, P- = L L' 2^-16 from two
    independent factors; S+ holds s, alpha in (0, 1] and i in (0, 2^-6]; S- = S+ plus 0 .. 3 units of 2^-30"""
    sp = [H.as_f64(H.hash_pos(idx, 340 + i)) * 2.0 ** e for i, e in enumerate((-20, -26, -20))]
    sm = [sp[i] + H.as_f64(H.chain_hash(idx, 343 + i) % 4) * 2.0 ** -30 for i in range(3)]
    return {"S_PLUS": sp, "P_PLUS": [H.as_f64(v) * 2.0 ** -24 for v in _sd_factor(idx, 0)], "S_MINUS": sm,
            "P_MINUS": [H.as_f64(v) * 2.0 ** -16 for v in _sd_factor(idx, 1)]}


_sd_z = lambda c: H.as_f64(H.hash_sgn(c, 350)) * 2.0 ** -18                 # [-2, 2), 20 significant bits: exact in float


def _sd_host_case(T, B, chains, ndt, prm16):
    """the sdraw_ref case of the sampled chains alone: the four arrays as the storage type holds them (rounded once), widened"""
    case = dict(B=chains.size, T=T, prm=np.ascontiguousarray(prm16[:, chains % 16]), S_SMOOTH=None, P_SMOOTH=None)
    per_day = [_sd_values(t * B + chains) for t in range(T)]
    for k in ("S_PLUS", "P_PLUS", "S_MINUS", "P_MINUS"):
        case[k] = np.stack([np.stack(d[k]) for d in per_day]).astype(ndt).astype(np.float64)
    return case


def _sd_case(gpu_device, ref, what, *, B, T, D, k0, blk, f32, n_spread, planted_z, passes, scan=0):
    """One sdraw case, every output, workspace poisoned.  f32: float storage, float z and float X.  planted_z: paths whose z of the
    last day is NaN.  scan: so many chains are run through the restatement's gains, and the first two that are rank-deficient
    join the sample.  Returns (want, chains, case)."""
    import torch
    from epidemicmodeling_amd import _lib, synth
    from epidemicmodeling_amd import layout as L
    from tests import sdraw_ref as SR
    N, Tk = B * D, T - k0
    bk = blk or B
    nblk = -(-B // bk)
    Bp = nblk * bk
    es, tdt, ndt = (4, torch.float32, np.float32) if f32 else (8, torch.float64, np.float64)
    shapes = _lib.sdraw_shapes(B, T, D, k0)
    nbytes = {k: int(np.prod(sh, dtype=np.int64)) * (4 if k in _lib.SDRAW_OUT_I32 else 8) for k, sh in shapes.items()}
    nbytes.update(X=Tk * 3 * N * es, z=Tk * 3 * N * es, prm=L.PRM_COUNT * B * 8, workspace=T * B * 24 * 8)
    nbytes.update({k: T * r * Bp * es for k, r in (("S_PLUS", 3), ("P_PLUS", 9), ("S_MINUS", 3), ("P_MINUS", 9))})
    _assert_passes(nbytes, passes)
    H.need_free(gpu_device, 2 * sum(nbytes.values()) + (4 << 30))      # the measured peak: twice the arrays (temporaries of the formulas and checks)
    t_case = time.perf_counter()
    dev = torch.device(gpu_device)
    prm16 = synth.make_cfg3(16, T).prm
    prm = torch.as_tensor(prm16, device=dev).index_select(1, torch.arange(B, dtype=torch.int64, device=dev) % 16).contiguous()
    arrs = {k: torch.full((T, nblk, r, bk), NAN, dtype=tdt, device=dev) for k, r in (("S_PLUS", 3), ("P_PLUS", 9), ("S_MINUS", 3), ("P_MINUS", 9))}
    c_all = torch.arange(B, dtype=torch.int64, device=dev)
    pad = torch.full((Bp,), NAN, dtype=tdt, device=dev)              # padding lanes: NaN, never read
    for t in range(T):
        for k, rows in _sd_values(c_all + t * B).items():
            for e, v in enumerate(rows):
                pad[:B] = v.to(tdt)
                arrs[k][t, :, e, :] = pad.reshape(nblk, bk)
    z = torch.empty((Tk * 3, N), dtype=tdt, device=dev)
    step = 1 << 27                                                   # the hash's temporaries stay small
    for row in range(Tk * 3):
        for lo in range(0, N, step):
            hi = min(N, lo + step)
            z[row, lo:hi] = _sd_z(torch.arange(lo, hi, dtype=torch.int64, device=dev) + row * N).to(tdt)
    z = z.reshape(Tk, 3, N)
    for p in planted_z:
        z[Tk - 1, 1, p] = NAN
    # the sample
    pg, cap = -(-N // 256), SD_LAUNCH
    bnd_paths = [w0 * 256 + d for w0 in range(cap, pg, cap) for d in (-1, 0)]
    bnd = sorted({p // D + d for p in bnd_paths for d in (-1, 0, 1)})
    cross = {"X, z": _crossing(Tk * 3, N, es, passes.get("X", ()), of=lambda c: c // D)}
    for k in ("P_PLUS", "P_MINUS", "J", "L"):
        sz = es if k.startswith("P_") else 8
        cross[k] = _crossing(T * 9, B, sz, passes.get(k, ())) if bk == B else []
    cross["workspace"] = _crossing(T, B * 24, 8, passes.get("workspace", ()), of=lambda c: c // 24)
    low = []
    if scan:
        cand = np.linspace(0, B - 1, scan).astype(np.int64)
        g = ref.run(_sd_host_case(T, B, cand, ndt, prm16), D, want_x=False, storage="f32" if f32 else "f64")
        low = cand[np.flatnonzero(g["status"] & SR.RANK_DEFICIENT)[:2]].tolist()
        assert low, "no rank-deficient chain among the scanned ones"
    chains, cls = H.extreme_sample(B, bk, units=(bk, 256), n_spread=n_spread, rows=())
    chains = np.unique(np.concatenate([chains, bnd, low, [p // D for p in planted_z]] + list(cross.values())).astype(np.int64))
    chains = chains[(chains >= 0) & (chains < B)]
    S = set(chains.tolist())
    assert {0, 1, B - 2, B - 1} <= S and set(cls["spread"]) <= S and all(set(v) <= S for v in cross.values())
    assert len(bnd_paths) == 2 * ((pg - 1) // cap) and {p // D for p in bnd_paths} <= S
    # rule 1
    case = _sd_host_case(T, B, chains, ndt, prm16)
    sel = torch.as_tensor(chains, device=dev)
    for k, a in arrs.items():
        rows = a.shape[2]
        pos = torch.as_tensor((H.chain_offsets(chains, rows, B, bk) // 8).reshape(-1), device=dev)
        held = a.reshape(T, -1).index_select(1, pos).cpu().numpy().reshape(T, rows, chains.size)
        assert held.dtype == ndt and np.array_equal(held.astype(np.float64), case[k]), ("device and host evaluate the formula differently", k)
        assert Bp == B or bool(torch.isnan(a[:, -1, :, B - (nblk - 1) * bk:]).all())
    assert np.array_equal(H.selected(prm, sel), case["prm"], equal_nan=True)
    cols = H.region_columns(chains, D)
    csel = torch.as_tensor(cols, device=dev)
    z_s = H.formula_sample(Tk * 3, N, cols, _sd_z, ndt).reshape(Tk, 3, cols.size)
    for p in planted_z:
        z_s[Tk - 1, 1, int(np.searchsorted(cols, p))] = np.nan
    assert np.array_equal(H.selected(z, csel), z_s, equal_nan=True)
    # rule 2
    odt = {"X": tdt, "rank": torch.int32, "status": torch.int32, "J": torch.float64, "L": torch.float64}
    out = {k: H.poisoned(shapes[k], odt[k], dev) for k in _lib.SDRAW_OUT_NAMES}
    d = _lib.make_sdraw_desc(B, T, D, k0, True, blk, int(f32), int(f32), int(f32))
    ins, outs = _lib.SdrawInputs(), _lib.SdrawOutputs()
    for k, v in zip(_lib.SDRAW_IN_NAMES, (arrs["S_PLUS"], arrs["P_PLUS"], arrs["S_MINUS"], arrs["P_MINUS"], prm, z, None, None)):
        setattr(ins, k, None if v is None else C.c_void_p(v.data_ptr()))
    for k in _lib.SDRAW_OUT_NAMES:
        setattr(outs, k, C.c_void_p(out[k].data_ptr()))
    ws = H.poisoned_words(T * B * 24, dev)
    t_call = _call("epi_sdraw_run_device", dev, C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(ws.data_ptr()), C.c_size_t(ws.numel() * 8))
    _no_poison(dict(out, workspace=ws))                                # status: zeroed by the call and OR-ed into
    # rule 3
    want = ref.run(case, D, z_s, k0=k0, storage="f32" if f32 else "f64", out_f32=f32)
    _compare(out, want, {k: csel if k == "X" else sel for k in out}, chains)
    rk, st = want["rank"], want["status"]
    assert (rk == 3).mean() >= 0.95 and (st & SR.RANK_DEFICIENT).any() and not (st & SR.NONFINITE).any(), ((rk == 3).mean(), np.bincount(st))
    Xw = want["X"].reshape(Tk, 3, chains.size, D)
    for p in planted_z:
        j = int(np.searchsorted(chains, p // D))
        assert np.isnan(Xw[:, :, j, p % D]).all()
    assert np.isnan(want["X"]).sum() == sum(np.isnan(Xw[:, :, int(np.searchsorted(chains, p // D)), p % D]).sum() for p in planted_z)
    H.report_limits(f"sdraw {what} B={B} T={T} D={D} k0={k0} lane_block={blk} {'float' if f32 else 'double'} ({pg} path workgroups, "
                    f"{-(-pg // cap)} launches), sample {chains.size} chains", t_call, t_case, dev)
    del out, arrs, z, ws, prm, pad
    torch.cuda.empty_cache()
    return want, chains, case


def test_sdraw_gain_across_byte_offsets(gpu_device, sdraw_ref):
    """S1.  epi_sdraw_run_device with B = 2^20 + 36 chains, classic layout, double, T = 43, D = 2, k0 = 41, every output.  The
    workspace [43, B, 24] (8.66 GB) passes 2^31, 2^32 and 2^33 bytes; P_PLUS, P_MINUS, J and L [43, 9, B] (3.25 GB) pass 2^31.
    The chains whose records and entries lie on both sides of those offsets are sampled."""
    B = (1 << 20) + 36
    _sd_case(gpu_device, sdraw_ref, "S1", B=B, T=43, D=2, k0=41, blk=0, f32=False, n_spread=48, planted_z=(),
             passes={"workspace": BITS, "P_PLUS": (31,), "P_MINUS": (31,), "J": (31,), "L": (31,)})


def test_sdraw_paths_past_one_launch(gpu_device, sdraw_ref):
    """S2.  B = 1 073 800 chains in 256-chain blocks (the last block holds 136), D = 1000 draws, T = 2, k0 = 0, float storage, float
    z, float X: N = 1 073 800 000 paths in 2^22 + 228 workgroups of sdraw_paths<2, 1>, two launches at the production bound.  The
    second launch starts at path 2^30, draw 824 of chain 1 073 741.  X and z [2, 3, N] float (25.8 GB each) pass 2^31, 2^32 and
    2^33 bytes.  Planted: a NaN z on the last day in path 2^30 - 1 and in path 2^30 + 1.  With T = 2 few sampled chains are
    rank-deficient by chance, so 20 000 chains are scanned with the restatement's gains and two such chains join the sample."""
    B, D = 1073800, 1000
    N = B * D
    assert -(-N // 256) == SD_LAUNCH + 228 and divmod(SD_LAUNCH * 256, D) == (1073741, 824) and B % 256 == 136
    _sd_case(gpu_device, sdraw_ref, "S2", B=B, T=2, D=D, k0=0, blk=256, f32=True, n_spread=32, planted_z=((1 << 30) - 1, (1 << 30) + 1),
             passes={"X": BITS, "z": BITS}, scan=20000)


# ---------------------------------------------------------------------------------------------------------------- npi_plan
@pytest.fixture(scope="module")
def plan_ref(tmp_path_factory):
    from tests.npi_plan_ref import PlanRef
    return PlanRef(tmp_path_factory.mktemp("npi_plan_ref_limits"))


# the start state: with the trained tables' (0.97, 2e-3, 0.25) every chain of this short horizon stops at its second iteration
# whatever tol is; from 5 % infected the chains of the second cost weight take two or three iterations, those of three stop at the cap
PLAN_START = (0.9, 0.05, 0.25)
PLAN = dict(R=(1 << 20) + 25, P=4, H=22, n=12, prefix_days=40, max_iter=3, max_halvings=4, tol=1e-3)
_plan_start = lambda c: H.as_f64(H.chain_hash(c, 82) % 3)               # u_init: 0, 1, 2
_plan_j0 = lambda c: H.as_f64(H.hash_pos(c, 83)) * 2.0 ** -20           # J0_prefix: (0, 1]
_plan_j1 = lambda c: H.as_f64(H.hash_pos(c, 84)) * 2.0 ** -13           # J1_prefix: (0, 128]


def _plan_held(c):
    """u_fixed: 1.0 (held) for three hash values in ten, NaN (free) for the others"""
    h = H.chain_hash(c, 81) % 10
    return H.replaced(h >= 3, NAN, H.as_f64(h * 0 + 1))


def _plan_regions16():
    """sp [48, 16] of synth.make_regions(16) from PLAN_START and the four cost weights of tests/test_gpu_npi_plan.py's spread"""
    from epidemicmodeling_amd import synth
    from tests import npi_plan_ref as PR
    from tests.test_gpu_npi_plan import _spread
    g = synth.make_regions(16)
    return PR.scoring_block(np.ascontiguousarray(g["a"][:, :PLAN["n"]].T), g["b"], start=PLAN_START), _spread(PLAN["P"])


def _plan_host_case(reg):
    """the call's problem on the regions reg alone (all P chains of each)"""
    R, P, Hh, n = PLAN["R"], PLAN["P"], PLAN["H"], PLAN["n"]
    sp16, eps = _plan_regions16()
    chains = H.region_columns(reg, P)
    return dict(PLAN, R=reg.size, sp=np.ascontiguousarray(sp16[:, reg % 16]), u_min=np.zeros((n, reg.size)), eps=eps,
                u_fixed=H.formula_sample(Hh * n, R, reg, _plan_held).reshape(Hh, n, reg.size),
                u_init=H.formula_sample(Hh * n, R * P, chains, _plan_start).reshape(Hh, n, chains.size),
                J0_prefix=_plan_j0(reg), J1_prefix=_plan_j1(reg))


def test_npi_plan_across_byte_offsets(gpu_device, plan_ref):
    """N1.  epi_plan_run_device with R = 2^20 + 25 regions x P = 4 cost weights (B = 4 194 404 chains, one launch of 65 538
    wavefronts), H = 22, n_npi = 12, max_iter = 3, max_halvings = 4, tol = 1e-3, a 40-day prefix, u_fixed (1.0 or NaN) and u_init
    (0, 1, 2) by formula, every output with states, mu and F_trace.  H n B = 1.107e9 lies between 2^30 and 2^31: plan, u_init (and
    the workspace's second plan) hold 8.86 GB and pass 2^31, 2^32 and 2^33 bytes; states, mu [22, 3, B] and u_fixed [22, 12, R]
    hold 2.21 GB and pass 2^31.  The sampled regions -- all four chains of each -- against tests/npi_plan_ref.c."""
    import torch
    from epidemicmodeling_amd import _lib
    R, P, Hh, n, max_iter = (PLAN[k] for k in ("R", "P", "H", "n", "max_iter"))
    B = R * P
    assert (1 << 30) < Hh * n * B < (1 << 31)
    shapes = _lib.plan_shapes(R, P, Hh, n, max_iter)
    nbytes = {k: int(np.prod(sh, dtype=np.int64)) * (4 if k in _lib.PLAN_OUT_I32 else 8) for k, sh in shapes.items()}
    nbytes.update(sp=48 * R * 8, u_min=n * R * 8, u_fixed=Hh * n * R * 8, u_init=Hh * n * B * 8, J0_prefix=R * 8, J1_prefix=R * 8)
    _assert_passes(nbytes, {"plan": BITS, "u_init": BITS, "states": (31,), "mu": (31,), "u_fixed": (31,)})
    d = _lib.make_plan_desc(R, P, Hh, n, PLAN["prefix_days"], max_iter, PLAN["max_halvings"], PLAN["tol"])
    nws = C.c_size_t(0)
    err = C.create_string_buffer(256)
    _lib.check(_lib.lib().epi_plan_workspace_bytes(C.byref(d), C.byref(nws), err), err)
    assert nws.value > Hh * n * B * 8 > (1 << 33)
    H.need_free(gpu_device, sum(nbytes.values()) + nws.value + (12 << 30))
    t_case = time.perf_counter()
    dev = torch.device(gpu_device)
    sp16, eps = _plan_regions16()
    r_all = torch.arange(R, dtype=torch.int64, device=dev)
    t = dict(sp=torch.as_tensor(sp16, device=dev).index_select(1, r_all % 16).contiguous(), u_min=torch.zeros((n, R), dtype=torch.float64, device=dev),
             eps=torch.as_tensor(eps, device=dev), u_fixed=H.formula_rows(Hh * n, R, dev, _plan_held, torch.float64),
             u_init=H.formula_rows(Hh * n, B, dev, _plan_start, torch.float64), J0_prefix=_plan_j0(r_all), J1_prefix=_plan_j1(r_all))
    # the sample
    cross = {k: _crossing(Hh * n, B, 8, BITS, of=lambda c: c // P) for k in ("plan", "u_init")}
    cross.update({k: _crossing(Hh * 3, B, 8, (31,), of=lambda c: c // P) for k in ("states", "mu")})
    cross["u_fixed"] = _crossing(Hh * n, R, 8, (31,))
    reg, S = _sample(R, 48, *cross.values())
    assert all(set(v) <= S for v in cross.values())
    # rule 1
    case = _plan_host_case(reg)
    chains = H.region_columns(reg, P)
    sel, csel = torch.as_tensor(reg, device=dev), torch.as_tensor(chains, device=dev)
    for k in ("sp", "u_min", "u_fixed", "J0_prefix", "J1_prefix"):
        assert np.array_equal(H.selected(t[k], sel).reshape(case[k].shape), case[k], equal_nan=True), ("device and host evaluate the formula differently", k)
    assert np.array_equal(H.selected(t["u_init"], csel).reshape(case["u_init"].shape), case["u_init"])
    held = ~np.isnan(case["u_fixed"])
    assert 0.2 < held.mean() < 0.4 and set(np.unique(case["u_init"]).tolist()) == {0.0, 1.0, 2.0}
    # rule 2
    out = {k: H.poisoned(sh, torch.int32 if k in _lib.PLAN_OUT_I32 else torch.float64, dev) for k, sh in shapes.items()}
    ins, outs = _lib.PlanInputs(), _lib.PlanOutputs()
    for k in _lib.PLAN_IN_NAMES:
        setattr(ins, k, C.c_void_p(t[k].data_ptr()))
    for k in _lib.PLAN_OUT_NAMES:
        setattr(outs, k, C.c_void_p(out[k].data_ptr()))
    ws = H.poisoned_words(-(-nws.value // 8), dev)
    t_call = _call("epi_plan_run_device", dev, C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(ws.data_ptr()), C.c_size_t(nws.value))
    _no_poison(out)                                                    # F_trace too: the iterations a chain never ran hold NaN
    # rule 3
    want = plan_ref.run(case)
    _compare(out, want, {k: csel for k in out}, reg)
    it, st = want["iters"], want["status"]
    assert len(np.unique(it)) >= 2 and not (st & _lib.PLAN_STOP_CAP).all() and (st & _lib.PLAN_STOP_CAP).any(), (np.bincount(it), np.bincount(st))
    assert not (st & _lib.PLAN_STOP_NONFINITE).any() and len(np.unique(want["halvings"])) >= 2 and np.isnan(want["F_trace"][max_iter - 1]).any()
    assert (want["plan"][np.repeat(held, P, axis=2)] == 1.0).all()
    H.report_limits(f"npi_plan R={R} P={P} H={Hh} n={n} max_iter={max_iter} (B={B}, one launch), sample {reg.size} regions", t_call, t_case, dev)
    del out, t, ws
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------ loglik
EPI_ERR_UNSUPPORTED = -8                                             # include/epiekf.h


@pytest.fixture(scope="module")
def loglik_ref(tmp_path_factory):
    from tests.loglik_ref import LoglikRef
    return LoglikRef(tmp_path_factory.mktemp("loglik_ref_limits"))


def _ll_rows(m):
    """{array: one formula per row} over the items idx = t B + c: s and every entry of P- positive (so S = C P C' + gamma R is a sum
    of positive terms), the innovation dyadic in [-8, 8); 20 significant bits each: exact in float"""
    pos = lambda k, e: (lambda idx: H.as_f64(H.hash_pos(idx, k)) * 2.0 ** e)
    return {"S_MINUS": [pos(400 + i, -20) for i in range(m)], "P_MINUS": [pos(410 + e, -24) for e in range(m * m)],
            "innovations": [lambda idx: H.as_f64(H.hash_sgn(idx, 450)) * 2.0 ** -16]}


_ll_x = _with_nan(_dyadic10(451), 452, 11)                           # an observation: only its being NaN or not is read
_ll_R = lambda c: H.as_f64(H.hash_pos(c, 453)) * 2.0 ** -20          # R_scalar [B] / R_series [T, Sx]: (0, 1]


def _ll_prm(prm16, c, adaptive):
    """prm [61, n] of chains c: the 16 columns of synth.make_cfg3 in turn; with the adaptive replay beta_ekf = 0.9 except for every
    third chain, which keeps 1.0 (no replay)"""
    from epidemicmodeling_amd import layout as L
    prm = np.ascontiguousarray(prm16[:, c % 16])
    if adaptive:
        prm[L.PRM_BETA_EKF] = np.where(c % 3 == 0, 1.0, 0.9)
    return prm


def _ll_fill(arr, fns, T, B, bk, dev):
    """arr [T, nblk, rows, bk] (a one-row array: [T, nblk * bk]) from the row formulas, some days at a time; padding lanes NaN"""
    import torch
    one = arr.dim() == 2
    nblk = arr.shape[1] // bk if one else arr.shape[1]
    Bp = nblk * bk
    c = torch.arange(Bp, dtype=torch.int64, device=dev)
    live = (c < B)[None]
    nan = torch.full((1, 1), NAN, dtype=arr.dtype, device=dev)
    days = max(1, (1 << 25) // Bp)
    for t0 in range(0, T, days):
        t1 = min(T, t0 + days)
        idx = torch.arange(t0, t1, dtype=torch.int64, device=dev)[:, None] * B + c[None]
        for e, fn in enumerate(fns):
            v = torch.where(live, fn(idx).to(arr.dtype), nan)
            if one:
                arr[t0:t1] = v
            else:
                arr[t0:t1, :, e, :] = v.reshape(t1 - t0, nblk, bk)


def _ll_blocked_crossing(T, rows, B, bk, itemsize, bits):
    """the chains on both sides of the elements of a blocked array [T][nblk][rows][bk] whose byte offsets first reach 2^bit"""
    nblk = -(-B // bk)
    out = []
    for b in bits:
        for e in ((1 << b) // itemsize - 1, (1 << b) // itemsize):
            assert e < T * nblk * rows * bk
            out.append(((e // (rows * bk)) % nblk) * bk + e % bk)
    return out


def _ll_case(gpu_device, ref, what, *, model, B, T, Lw, G, blk, f32, r_mode, Sx, passes, plants=(), groups=None, n_spread=32):
    """One loglik case, all nine outputs, workspace poisoned.  plants: [(array, index, value)] with index (t, row, chain) -- (t, chain)
    for innovations, (t, series) for x.  groups: the sampled groups of G chains (None: the ends, the unit boundaries, the byte-offset
    crossings, a spread).  Returns (want, chains, case)."""
    import torch
    from epidemicmodeling_amd import _lib, synth
    from epidemicmodeling_amd import layout as L
    from tests import loglik_ref as LR
    m = LR.model_info(model)[0]
    bk = blk or B
    nblk = -(-B // bk)
    Bp = nblk * bk
    es, tdt, ndt = (4, torch.float32, np.float32) if f32 else (8, torch.float64, np.float64)
    own_x = Sx == B
    shapes = _lib.loglik_shapes(B, T, G)
    nbytes = {k: int(np.prod(sh, dtype=np.int64)) * (4 if k in _lib.LOGLIK_OUT_I32 else 8) for k, sh in shapes.items()}
    nbytes.update(S_MINUS=T * m * Bp * es, P_MINUS=T * m * m * Bp * es, innovations=T * Bp * es, x=T * Sx * 8, prm=L.PRM_COUNT * B * 8,
                  x_series=0 if own_x else B * 4, **({"R_series": T * Sx * 8} if r_mode else {"R_scalar": B * 8}))
    _assert_passes(nbytes, passes)
    d = _lib.make_loglik_desc(model, B, T, Lw, "NEWCASES", r_mode, Sx, blk, int(f32), 0, None, G)
    nws = C.c_size_t(0)
    err = C.create_string_buffer(256)
    _lib.check(_lib.lib().epi_loglik_workspace_bytes(C.byref(d), C.byref(nws), err), err)
    H.need_free(gpu_device, sum(nbytes.values()) + nws.value + (4 << 30))
    t_case = time.perf_counter()
    dev = torch.device(gpu_device)
    fns = _ll_rows(m)
    arrs = {"S_MINUS": torch.empty((T, nblk, m, bk), dtype=tdt, device=dev), "P_MINUS": torch.empty((T, nblk, m * m, bk), dtype=tdt, device=dev),
            "innovations": torch.empty((T, Bp), dtype=tdt, device=dev)}
    for k, a in arrs.items():
        _ll_fill(a, fns[k], T, B, bk, dev)
    x = H.formula_rows(T, Sx, dev, _ll_x, torch.float64) if Sx > (1 << 12) else \
        _ll_x(torch.arange(T * Sx, dtype=torch.int64, device=dev)).reshape(T, Sx)
    c_all = torch.arange(B, dtype=torch.int64, device=dev)
    xs = None if own_x else (H.chain_hash(c_all, 454) % Sx).to(torch.int32)
    Rt = H.formula_rows(T, Sx, dev, _ll_R, torch.float64) if r_mode and Sx > (1 << 12) else \
        _ll_R(torch.arange(T * Sx if r_mode else B, dtype=torch.int64, device=dev)).reshape((T, Sx) if r_mode else (B,))
    prm16 = synth.make_cfg3(16, 8).prm
    prm = torch.as_tensor(prm16, device=dev).index_select(1, c_all % 16).contiguous()
    if not r_mode:
        prm[L.PRM_BETA_EKF] = torch.as_tensor([1.0, 0.9, 0.9], dtype=torch.float64, device=dev).index_select(0, c_all % 3)
    for name, idx, val in plants:
        if name == "x":
            x[idx] = val
        elif name == "innovations":
            arrs[name][idx] = val
        else:
            t, row, c = idx
            arrs[name][t, c // bk, row, c % bk] = val
    # the sample: whole groups of G chains
    if groups is None:
        chains0, cls = H.extreme_sample(B, bk, units=(64, 256, bk), n_spread=n_spread, rows=())
        cross = {}
        for k, rows, sz in (("S_MINUS", m, es), ("P_MINUS", m * m, es), ("innovations", 1, es)):
            cross[k] = _ll_blocked_crossing(T, rows, B, bk, sz, passes.get(k, ())) if bk < B else \
                [c for c in H.crossing_regions(T * rows, B, bits=passes.get(k, ()), itemsize=sz)]
        for k in ("S", "nis", "R_used") + (("x",) if own_x else ()):
            cross[k] = H.crossing_regions(T, B, bits=passes.get(k, ()), itemsize=8)
        assert all(len(cross[k]) >= 2 * len(passes.get(k, ())) for k in cross) and all(len(cross[k]) > 0 for k in passes if k in cross), cross
        planted = [idx[-1] for name, idx, _ in plants if name != "x" or own_x]
        groups, S = _sample(B // G, 0, chains0 // G, *[[c // G + dd for c in v for dd in (-1, 0, 1)] for v in cross.values()], [c // G for c in planted])
        assert all({c // G for c in v} <= S for v in cross.values()) and {c // G for c in cls["spread"]} <= S
    chains = H.region_columns(groups, G)
    n = chains.size
    # rule 1
    tt = np.arange(T, dtype=np.int64)[:, None]
    case = dict(model=model, B=n, T=T, L=Lw, obs_type="NEWCASES", K_GAIN=None, x_series=None, prm=_ll_prm(prm16, chains, not r_mode))
    whole = n == B and T > (1 << 16)                 # every chain over very many days: the formulas on a sample of days only,
    ds = np.unique(np.concatenate([np.linspace(0, T - 1, 64).astype(np.int64), [1, 31, 32, T - 33, T - 32, T - 2]])) if whole else tt[:, 0]
    for k, f in fns.items():
        case[k] = np.stack([fn(ds[:, None] * B + chains[None]) for fn in f], axis=1)
        if whole:                                    # and the restatement reads what the device holds
            assert bk == B and np.array_equal(arrs[k].reshape(T, -1, B)[ds].cpu().numpy().astype(np.float64), case[k].astype(ndt).astype(np.float64)), k
            case[k] = arrs[k].reshape(T, -1, B).cpu().numpy().astype(np.float64)
    case["innovations"] = case["innovations"][:, 0]
    sx = chains if own_x else (H.chain_hash(chains, 454) % Sx)
    case["x"] = _ll_x(tt * Sx + sx[None])
    case["R_series"], case["R_scalar"] = (_ll_R(tt * Sx + sx[None]), None) if r_mode else (None, _ll_R(chains))
    for name, idx, val in plants:
        if name == "x":
            case["x"][idx[0], sx == idx[1]] = val
        else:
            case[name][idx[:-1] + (int(np.searchsorted(chains, idx[-1])),)] = val
    for k in fns:
        case[k] = case[k].astype(ndt).astype(np.float64)
    sel = torch.as_tensor(chains, device=dev)
    for k in ("S_MINUS", "P_MINUS"):
        rows = arrs[k].shape[2]
        pos = torch.as_tensor((H.chain_offsets(chains, rows, B, bk) // 8).reshape(-1), device=dev)
        held = arrs[k].reshape(T, -1).index_select(1, pos).cpu().numpy().reshape(T, rows, n)
        assert held.dtype == ndt and np.array_equal(held.astype(np.float64), case[k], equal_nan=True), ("device and host evaluate the formula differently", k)
        assert Bp == B or bool(torch.isnan(arrs[k][:, -1, :, B - (nblk - 1) * bk:]).all())
    assert np.array_equal(H.selected(arrs["innovations"], sel).astype(np.float64), case["innovations"], equal_nan=True)
    assert Bp == B or bool(torch.isnan(arrs["innovations"][:, B:]).all())
    ssel = torch.as_tensor(sx, device=dev)
    assert np.array_equal(H.selected(x, ssel), case["x"], equal_nan=True) and np.array_equal(H.selected(prm, sel), case["prm"], equal_nan=True)
    assert np.array_equal(H.selected(Rt, ssel if r_mode else sel), case["R_series"] if r_mode else case["R_scalar"])
    assert own_x or np.array_equal(H.selected(xs, sel), sx)
    # rule 2
    out = {k: H.poisoned(sh, torch.int32 if k in _lib.LOGLIK_OUT_I32 else torch.float64, dev) for k, sh in shapes.items()}
    ins, outs = _lib.LoglikInputs(), _lib.LoglikOutputs()
    for k, v in zip(_lib.LOGLIK_IN_NAMES, (arrs["S_MINUS"], arrs["P_MINUS"], arrs["innovations"], x, Rt if r_mode else None, None if r_mode else Rt, xs, prm)):
        setattr(ins, k, None if v is None else C.c_void_p(v.data_ptr()))
    for k in _lib.LOGLIK_OUT_NAMES:
        setattr(outs, k, C.c_void_p(out[k].data_ptr()))
    ws = H.poisoned_words(-(-nws.value // 8), dev)
    t_call = _call("epi_loglik_run_device", dev, C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(ws.data_ptr()), C.c_size_t(nws.value))
    _no_poison(out)
    # rule 3
    want = ref.run(case, storage="f32" if f32 else "f64", G=G)
    want.pop("PCt")
    gsel = torch.as_tensor(groups, device=dev)
    _compare(out, want, {k: gsel if k in ("best", "best_loglik") else sel for k in out}, groups)
    H.report_limits(f"loglik {what} {model} B={B} T={T} L={Lw} G={G} lane_block={blk} {'float' if f32 else 'double'} r_mode={r_mode} Sx={Sx} "
                    f"(ll_blocks grid {-(-B // 256)} x {-(-T // 32)}), sample {n} chains", t_call, t_case, dev)
    del out, arrs, x, Rt, prm, ws
    torch.cuda.empty_cache()
    return want, chains, case


def test_loglik_across_byte_offsets(gpu_device, loglik_ref):
    """L1.  epi_loglik_run_device, the 3-state model, classic layout, double, r_mode 0 (ll_replay runs; every third chain has
    beta_ekf = 1 and no replay), B = 2^22 + 40 chains (a multiple of 8, not of 256), T = 65 (three 32-step blocks, the last of one
    day), L = 4, G = 8, all nine outputs.  P_MINUS [65, 9, B] (19.6 GB) passes 2^31, 2^32 and 2^33 bytes, S_MINUS 2^31 and 2^32;
    innovations, x, S, nis and R_used [65, B] pass 2^31.  Every unplanted observed day is good (S is a sum of positive terms).
    Planted in the three chains around the 2^32 edge of P_MINUS, on its day: a NaN x, an infinite innovation, and a P- whose
    diagonal is -1e300 (S < 0)."""
    B, T, G = (1 << 22) + 40, 65, 8
    assert B % G == 0 and B % 256 and -(-T // 32) == 3 and T % 32 == 1 and T * B > (1 << 28)
    e32 = (1 << 32) // 8
    t32, q = (e32 // B) // 9, e32 % B
    plants = [("x", (t32, q - 1), NAN), ("innovations", (t32, q), INF)] + [("P_MINUS", (t32, e, q + 1), -1e300) for e in (0, 4, 8)]
    want, chains, case = _ll_case(gpu_device, loglik_ref, "L1", model="SIAlphaModelEKF", B=B, T=T, Lw=4, G=G, blk=0, f32=False, r_mode=0, Sx=B,
                                  passes={"P_MINUS": BITS, "S_MINUS": (31, 32), "innovations": (31,), "x": (31,), "S": (31,), "nis": (31,), "R_used": (31,)},
                                  plants=plants)
    j = int(np.searchsorted(chains, q))
    st = want["status"]
    assert st[j - 1] == 0 and st[j] == 1 and st[j + 1] == 1 and (np.delete(st, [j, j + 1]) == 0).all()
    assert np.isnan(want["S"][t32, j - 1]) and want["S"][t32, j + 1] < 0 and (want["n_valid"] == (~np.isnan(case["x"])).sum(axis=0) - (st & 1)).all()
    ru = want["R_used"]
    assert (ru[:, chains % 3 == 0] == ru[:1, chains % 3 == 0]).all() and (ru[1:, chains % 3 == 1] != ru[:-1, chains % 3 == 1]).any(axis=0).all()
    assert (want["best"] >= 0).all() and len(np.unique(want["best"])) == G


def test_loglik_blocked_float_flipped(gpu_device, loglik_ref):
    """L2.  The 6-state time-flipped model, chain-blocked with lane_block = 64, float storage, r_mode 1, B = 2^21 + 40 (not a multiple
    of 64: Bp = 2^21 + 64, 24 padding lanes that hold NaN), T = 33, x_series by formula onto Sx = 2^16 + 3 series, R_series [33, Sx].
    P_MINUS as float [33, nblk, 36, 64] (9.97 GB) passes 2^31, 2^32 and 2^33 bytes with the M = 6 strides of the blocked offsets
    slot M blk + cr; the outputs are [T, B], unpadded."""
    B, T = (1 << 21) + 40, 33
    assert B % 64 == 40 and B % 8 == 0
    want, chains, case = _ll_case(gpu_device, loglik_ref, "L2", model="SIAlphaModelBackwardEKFOptControlled", B=B, T=T, Lw=4, G=8, blk=64, f32=True,
                                  r_mode=1, Sx=(1 << 16) + 3, passes={"P_MINUS": BITS})
    assert not want["status"].any() and (want["n_valid"] == (~np.isnan(case["x"])).sum(axis=0)).all() and len(np.unique(want["n_valid"])) >= 3


def test_loglik_grid_y_at_its_limit(gpu_device, loglik_ref):
    """L3.  B = 5 chains over T = 32 x 65 535 days, 3-state, r_mode 1 (with r_mode 0 one lane would walk 2.1 M steps serially), G = 5,
    all nine outputs, every chain and day compared: ll_blocks runs as a grid of 1 x 65 535, the largest grid.y the call admits.
    T + 1 is one block more and must be rejected with EPI_ERR_UNSUPPORTED."""
    from epidemicmodeling_amd import _lib
    B, T = 5, 32 * 65535
    want, chains, case = _ll_case(gpu_device, loglik_ref, "L3", model="SIAlphaModelEKF", B=B, T=T, Lw=4, G=5, blk=0, f32=False, r_mode=1, Sx=B,
                                  passes={}, groups=np.arange(1, dtype=np.int64))
    assert chains.size == B and not want["status"].any() and want["n_valid"].min() > 0.8 * T and want["S"].shape == (T, B)
    d = _lib.make_loglik_desc("SIAlphaModelEKF", B, T + 1, 4, "NEWCASES", 1, B, 0, 0, 0, None, 5)
    err = C.create_string_buffer(256)
    assert _lib.lib().epi_loglik_validate(C.byref(d), err) == EPI_ERR_UNSUPPORTED, err.value
    d.T = T
    assert _lib.lib().epi_loglik_validate(C.byref(d), err) == 0, err.value

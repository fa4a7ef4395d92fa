"""The three regression calls -- MATLAB's backslash (epi_mldiv_run_device), support-vector regression (epi_svr_run_device), the
NPI-to-growth-rate predictor (epi_ratemap_run_device) -- past 64 row counts / train ends, past one launch, and across the
2 / 4 / 8 GiB byte offsets of their arrays.

The three entry points share one host pattern.  A launch carries at most 64 counts by value, so the K counts are cut into
chunks (k0, kc); the dynamic LDS size (and svr's g.lds) is taken from the chunk's own largest / smallest count; the kc * R items
of a chunk are cut into launches of at most 2^22 workgroups, each of which gets its first item (item0); the kernel decodes
item = item0 + blockIdx.x into (kk, r) = (item / R, item % R), reads n = nr[kk] and writes to k = k0 + kk.  ratemap_region is cut
over R in the same way.  The shared case tables stop at K = 4, R = 65, so every other GPU test runs with k0 = 0 and item0 = 0 in
one launch; the *_emu.py modules re-state the loop on the host.  A kernel that dropped k0 or item0, indexed nr[k] instead of
nr[kk], took its LDS size from the first chunk, or formed (k D + t) R + r in 32 bits left the suite green.

The cases follow the three rules of tests/test_gpu_call_limits.py:

 1. inputs by formula per element (helpers.chain_hash; small integers and dyadic values), evaluated by torch on the device for
    the whole array and by NumPy for the sample, the two compared bit for bit before the call;
 2. every output poisoned; after the call no word of any output of the WHOLE call may still hold the poison;
 3. the sampled regions -- both sides of every launch boundary (items j 2^22 - 2 .. j 2^22 + 1 of every chunk), both sides of the
    element where an array's byte offset first reaches 2^31, 2^32, 2^33, regions 0, 1, R - 2, R - 1, a spread -- equal, for EVERY
    k of the call, bit for bit and NaN to NaN, the family's C restatement (tests/mldivide_ref.c, svr_ref.c, rate_map_ref.c) run on
    the sampled columns alone; each test asserts that its sample holds these classes.

Case A, every family (svr: both kernels): K = 130 counts, R = 2^16 + 40.  Chunks (0, 64), (64, 64), (128, 2); each of the first
two has 2^22 + 2 560 items and takes two launches, whose boundary decodes to kk = 63, r = 63 016 (inside a k); the third takes one
launch with k0 = 128.  The counts differ from those 64 earlier (a chunk that read the first chunk's counts gives other bits);
the chunk maxima are 5, 6, 4 and the minima 1, 2, 3, so the LDS sizes differ between chunks in both directions.  A non-finite
input sits in the region of the last item of a first launch (63 015), of the first item of a second launch (63 016) and in
region 40 003.  The same 130-count problem, cut down to three sampled regions, goes through batch.* and hostapi.* as well.

Case B, every family (svr: the linear kernel): R = 2^22 + 1000 and K = 4 (rate_map: 3) distinct counts: K + 1 launches, kk
changes inside a launch.  X [16, 16, R] (rate_map: ip [22, 12, R]) passes 2^31, 2^32 and 2^33 bytes; the [K, F, R] and [K, D, R]
outputs pass 2^31; ratemap_region takes two launches over R.

Showing that the tests bite (scratch builds of the library with one line of a kernel's index arithmetic changed; every access
stays inside the arrays):
  (i)  mldivide_items with item = blockIdx.x (item0 dropped): both mldivide cases fail on rule 2, the other nine tests pass --
       every later launch rewrites the items of the first, and the items behind 2^22 keep the poison (A: 5 120 words of rank,
       the 2 x 2 560 items behind the boundary of chunks 1 and 2; B: 12 586 912 = 4 R - 2^22 words of rank).
  (ii) svr_items with k = kk (k0 dropped): the case-A tests of svr (both kernels) and its batch / host tests fail, the other
       seven pass.  On the device path rule 2 catches it first (66 R = 4 328 016 words of bias, k = 64 .. 129, are never
       written); the batch / host tests, whose outputs the wrappers allocate unpoisoned, fail on rule 3 at beta (k = 0 .. 63 hold
       the results of later chunks).  Case B has one chunk, k0 = 0, and cannot see it.

What stays uncovered: the product limits themselves (K R, D F R near 2^31: 16 GiB or more per array; asserted through the
descriptors in tests/test_*_abi.py).  The launch bounds and byte-offset edges of the five newer calls (loglik, npi_plan,
smoother_draws, ens_score, path_functionals) run in tests/test_gpu_newer_call_limits.py.

Measured on one MI355X (the library call alone / the whole case with input generation, sampling and the restatement /
torch.cuda.max_memory_allocated):
  mldivide A            0.03 s / 0.7 s /  1.3 GiB       mldivide B            0.35 s / 0.4 s / 18.0 GiB
  svr A, linear         0.13 s / 0.1 s /  1.6 GiB       svr A, gaussian       0.18 s / 0.2 s /  1.4 GiB
  svr B, linear         0.36 s / 0.4 s / 17.3 GiB       rate_map B            0.71 s / 0.8 s / 20.7 GiB
  rate_map A, fit = 1   0.06 s / 0.1 s /  1.8 GiB       rate_map A, fit = 0   0.02 s / 0.1 s /  2.1 GiB
The module takes 5 s; no case came near 10 s, so D, F and max_iter stand as the cases above give them.
No time is asserted; every case prints its figures in a line that starts with [limits].
"""
import ctypes as C
import time

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

LAUNCH = 1 << 22            # kMlLaunchItems, kSvLaunchItems, kRmLaunchItems
COUNTS = 64                 # kMlRowCounts, kSvRowCounts, kRmTrainEnds
BITS = (31, 32, 33)

# case A: chunk maxima 5, 6, 4, minima 1, 2, 3; counts[k] = counts[k - 64] + 1 in the second chunk
R_A = (1 << 16) + 40
COUNTS_A = tuple([1 + k % 5 for k in range(64)] + [2 + k % 5 for k in range(64)] + [3, 4])
PLANTED_A = (63015, 63016, 40003)           # the last item of a first launch, the first item of a second launch, a third
CONSTANT_A = (0, 8, 63008, 63024, R_A - 8)  # svr: sampled regions r % 8 == 0, whose y is constant
ENTRY_REGIONS = (63014, 63015, 8)           # the three regions of the batch / host tests: healthy, planted, constant y
# case B
R_B = (1 << 22) + 1000

FAMILY = {  # inputs, outputs, output names, the int32 ones, the entry point, the field of the host array of counts
    "mldiv": ("MldivInputs", "MldivOutputs", "MLDIV_OUT_NAMES", "MLDIV_OUT_I32", "epi_mldiv_run_device", "n_rows"),
    "svr": ("SvrInputs", "SvrOutputs", "SVR_OUT_NAMES", "SVR_OUT_I32", "epi_svr_run_device", "n_rows"),
    "ratemap": ("RatemapInputs", "RatemapOutputs", "RATEMAP_OUT_NAMES", "RATEMAP_OUT_I32", "epi_ratemap_run_device", "n_train"),
}


# ---------------------------------------------------------------------------------------------------------- the formulas
def _levels(k):
    return lambda c: H.as_f64(H.chain_hash(c, k) % 5)                       # integer levels 0 .. 4


def _dyadic(k, e):
    return lambda c: H.as_f64(H.hash_sgn(c, k)) * 2.0 ** e                  # [-2^(19 + e), 2^(19 + e))


def _positive(k, e):
    return lambda c: H.as_f64(H.hash_pos(c, k)) * 2.0 ** e                  # (0, 2^(20 + e)]


def _quarter_steps(k, lo):
    return lambda c: H.as_f64(H.chain_hash(c, k) % 4 + lo) * 0.5            # lo / 2 .. (lo + 3) / 2


def _host_arrays(spec, R, reg):
    """{name: [*shape, len(reg)]}: the formulas of `spec` -- [(name, shape, fn)], an array [*shape, R] -- on the regions reg"""
    out = {}
    for name, shape, fn in spec:
        rows = int(np.prod(shape, dtype=np.int64))
        out[name] = fn(np.arange(rows, dtype=np.int64)[:, None] * R + reg[None]).reshape(tuple(shape) + (reg.size,))
    return out


def _device_arrays(spec, R, dev):
    import torch
    return {name: H.formula_rows(int(np.prod(shape, dtype=np.int64)), R, dev, fn, torch.float64).reshape(tuple(shape) + (R,))
            for name, shape, fn in spec}


def _plant(arrs, plants, reg=None):
    """plants: [(name, index without the region, region, value)]; reg: the sample of host arrays, None for device arrays"""
    for name, idx, r, v in plants:
        arrs[name][tuple(idx) + (r if reg is None else _j(reg, r),)] = v


def _j(reg, r):
    """positions of the regions r in the sample"""
    j = np.searchsorted(reg, r)
    assert np.array_equal(reg[j], np.asarray(r)), r
    return j if np.ndim(r) else int(j)


# ---------------------------------------------------------------------------------------------------------- the samples
def _chunks(K):
    return [(k0, min(COUNTS, K - k0)) for k0 in range(0, K, COUNTS)]


def _sample_a():
    """the sampled regions of case A; asserts the structural conditions of the case"""
    n, R, K = COUNTS_A, R_A, len(COUNTS_A)
    ch = _chunks(K)
    assert ch == [(0, 64), (64, 64), (128, 2)] and [-(-kc * R // LAUNCH) for _, kc in ch] == [2, 2, 1]
    assert all(n[k] != n[k - COUNTS] for k in range(COUNTS, K))
    mx, mn = ([f(n[k0:k0 + kc]) for k0, kc in ch] for f in (max, min))
    assert mx[1] > mx[0] > mx[2] and len(set(mn)) == 3, (mx, mn)
    bnd = [H.boundary_items(LAUNCH, kc * R) for _, kc in ch]
    assert [[divmod(i, R) for i in b] for b in bnd] == [[(63, 63014 + d) for d in range(4)]] * 2 + [[]]
    assert (LAUNCH - 1) % R == PLANTED_A[0] and LAUNCH % R == PLANTED_A[1]
    reg, cls = H.extreme_sample(R, R, n_spread=40, rows=())
    near = [p + d for p in PLANTED_A for d in (-1, 0, 1)]
    reg = np.unique(np.concatenate([reg, [i % R for b in bnd for i in b], near, CONSTANT_A]).astype(np.int64))
    S = set(reg.tolist())
    assert {0, 1, R - 2, R - 1} <= S and set(cls["spread"]) <= S
    assert all(H.both_sides(S, b, lambda i: i % R) for b in bnd[:2]) and set(ENTRY_REGIONS) <= S
    assert all(r % 8 == 0 for r in CONSTANT_A) and not any(r % 8 == 0 for r in _neighbours())
    return reg


def _neighbours():
    """the healthy regions next to the planted ones"""
    return sorted({p + d for p in PLANTED_A for d in (-1, 1)} - set(PLANTED_A))


def _sample_b(K, arrays, passes, region_kernel=False):
    """the sampled regions of case B.  arrays: {name: (rows, itemsize)} of EVERY array of the call, seen as [rows, R];
    passes: {name: bits} the arrays that pass 2^bit bytes -- every other array must stay below 2^31"""
    R, items = R_B, K * R_B
    assert -(-items // LAUNCH) == K + 1
    assert all(j * LAUNCH < j * R < (j + 1) * LAUNCH for j in range(1, K))                  # kk changes inside launch j
    bnd = H.boundary_items(LAUNCH, items)
    assert len(bnd) == 4 * K and {i // R for i in bnd} == set(range(K))
    assert {name: [b for b in BITS if rows * R * sz > (1 << b)] for name, (rows, sz) in arrays.items()} == \
        {name: list(passes.get(name, ())) for name in arrays}
    cross = {name: H.crossing_regions(rows, R, bits=BITS, itemsize=sz) for name, (rows, sz) in arrays.items()}
    assert all(len(cross[name]) == 4 * len(passes.get(name, ())) for name in arrays)
    bnd_r = H.boundary_items(LAUNCH, R) if region_kernel else []
    assert not region_kernel or bnd_r == [LAUNCH - 2, LAUNCH - 1, LAUNCH, LAUNCH + 1]
    reg, cls = H.extreme_sample(R, R, n_spread=24, rows=())
    reg = np.unique(np.concatenate([reg, [i % R for i in bnd], bnd_r] + list(cross.values())).astype(np.int64))
    S = set(reg.tolist())
    assert {0, 1, R - 2, R - 1} <= S and set(cls["spread"]) <= S and H.both_sides(S, bnd, lambda i: i % R)
    assert all(set(c) <= S for c in cross.values()) and set(bnd_r) <= S
    return reg


# ---------------------------------------------------------------------------------------------------------- the call
def _nbytes(shapes, i32):
    return sum(int(np.prod(s, dtype=np.int64)) * (4 if k in i32 else 8) for k, s in shapes.items())


def _device_call(family, d, tensors, counts, shapes, names, dev):
    """the family's device entry on the current stream, every output of `names` poisoned before (rule 2: no word of any of them
    may hold the poison afterwards).  tensors: {input name: device tensor or None}.  Returns (outputs, seconds of the call)"""
    import torch
    from epidemicmodeling_amd import _lib
    Ins, Outs, all_names, i32, entry, count_field = FAMILY[family]
    ins = getattr(_lib, Ins)()
    for k, t in tensors.items():
        setattr(ins, k, None if t is None else C.c_void_p(t.data_ptr()))
    nr = np.ascontiguousarray(counts, dtype=np.int32)
    setattr(ins, count_field, nr.ctypes.data)
    out = {k: H.poisoned(shapes[k], torch.int32 if k in getattr(_lib, i32) else torch.float64, dev) for k in names}
    outs = getattr(_lib, Outs)()
    for k in getattr(_lib, all_names):
        setattr(outs, k, C.c_void_p(out[k].data_ptr()) if k in out else None)
    err = C.create_string_buffer(256)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    rc = getattr(_lib.lib(), entry)(C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), err)
    _lib.check(rc, err)
    torch.cuda.synchronize(dev)
    t_call = time.perf_counter() - t0
    left = {k: H.poison_words(t, H.POISON_RANK) for k, t in out.items()}
    assert not any(left.values()), ("outputs that still hold the poison pattern (words)", left)
    return out, t_call


def _rule_1(dev_arrays, host, sel):
    for k, h in host.items():
        held = dev_arrays[k].index_select(-1, sel).cpu().numpy()
        assert held.dtype == h.dtype and np.array_equal(held, h, equal_nan=True), ("device and host evaluate the formula differently", k)


def _rule_3(out, want, reg, sel):
    assert set(out) == set(want), (sorted(out), sorted(want))
    for k, w in want.items():
        got = out[k].index_select(-1, sel).cpu().numpy()
        assert H.bits_equal(got, w), (k, "regions", reg[np.flatnonzero(~np.all(
            (got == w) | ((got != got) & (w != w)), axis=tuple(range(got.ndim - 1))))][:12].tolist())


def _same(got, want):
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k, w in want.items():
        assert H.bits_equal(np.asarray(got[k]), w), k


def _three(reg, host, want):
    """the problem and the restatement's result cut down to the columns ENTRY_REGIONS (items are independent per region)"""
    j = _j(reg, np.asarray(ENTRY_REGIONS))
    return {k: np.ascontiguousarray(v[..., j]) for k, v in host.items()}, {k: np.ascontiguousarray(v[..., j]) for k, v in want.items()}


def _frozen(*dicts):
    for d in dicts:
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return dicts


_A = {}                       # the case-A problems on their sample and the restatement's results: computed once, read-only


# ------------------------------------------------------------------------------------------------------------ mldivide
@pytest.fixture(scope="module")
def ml_ref(tmp_path_factory):
    from tests.mldivide_ref import MldivRef
    return MldivRef(tmp_path_factory.mktemp("mldiv_ref_limits"))


def _ml_spec(D, F):
    return [("X", (D, F), _levels(31)), ("y", (D,), _dyadic(32, -16))]


ML_PLANTS_A = [("X", (0, 0), PLANTED_A[0], float("nan")), ("y", (0,), PLANTED_A[1], float("inf")), ("X", (0, 1), PLANTED_A[2], float("-inf"))]


def _ml_a(ref):
    if "ml" not in _A:
        reg = _sample_a()
        host = _host_arrays(_ml_spec(6, 2), R_A, reg)
        _plant(host, ML_PLANTS_A, reg)
        _A["ml"] = (reg,) + _frozen(host, ref.run(host["X"], host["y"], COUNTS_A))
    return _A["ml"]


def test_mldivide_past_64_row_counts(gpu_device, ml_ref):
    """epi_mldiv_run_device, case A: D = 6, F = 2, K = 130 row counts 1 .. 6 (the counts below F take the under-determined
    branch), R = 2^16 + 40, all seven outputs.  X integer levels 0 .. 4, y dyadic.  Planted in row 0, which every count uses: a
    NaN in X (region 63 015), an Inf in y (63 016), a -Inf in X (40 003): NONFINITE_INPUT for every k of exactly these regions."""
    import torch
    from epidemicmodeling_amd import _lib
    from tests import mldivide_ref as ML
    D, F, R, K = 6, 2, R_A, len(COUNTS_A)
    reg, host, want = _ml_a(ml_ref)
    assert min(COUNTS_A) < F < max(COUNTS_A) <= D
    shapes = _lib.mldiv_shapes(D, F, R, K)
    assert max(_nbytes({k: s}, ML.OUT_I32) for k, s in shapes.items()) < (1 << 31)
    H.need_free(gpu_device, _nbytes(shapes, ML.OUT_I32) + (D * F + D) * R * 8 + (3 << 30))
    t_case = time.perf_counter()
    dev = torch.device(gpu_device)
    t = _device_arrays(_ml_spec(D, F), R, dev)
    _plant(t, ML_PLANTS_A)
    sel = torch.as_tensor(reg, device=dev)
    _rule_1(t, host, sel)
    out, t_call = _device_call("mldiv", _lib.make_mldiv_desc(D, F, R, K), t, COUNTS_A, shapes, ML.OUT_NAMES, dev)
    _rule_3(out, want, reg, sel)
    st, jp, jn = want["status"], _j(reg, np.asarray(PLANTED_A)), _j(reg, np.asarray(_neighbours()))
    assert (st[:, jp] == ML.NONFINITE_INPUT).all() and (st == ML.NONFINITE_INPUT).sum() == K * len(PLANTED_A)
    assert not (st[:, jn] & (ML.NONFINITE_INPUT | ML.NONFINITE)).any() and np.isfinite(want["m"][:, :, jn]).all()
    assert (want["rank"][:, jp] == -1).all() and (want["rank"][:, jn] >= 0).all() and (st == 0).any() and (st == ML.RANK_DEFICIENT).any()
    H.report_limits(f"mldivide A D={D} F={F} K={K} R={R} (chunks of 64 + 64 + 2 counts, 2 + 2 + 1 launches), sample {reg.size} regions",
                    t_call, t_case, dev)
    del out, t
    torch.cuda.empty_cache()


def test_mldivide_130_row_counts_batch_and_host(gpu_device, ml_ref):
    """the K = 130 problem of case A on three of its sampled regions through batch.mldivide and hostapi.mldivide: the Python call
    path carries 130 row counts (three chunks) into both entry points"""
    from epidemicmodeling_amd import batch, hostapi
    h3, w3 = _three(*_ml_a(ml_ref))
    _same({k: v.cpu().numpy() for k, v in batch.mldivide(h3["X"], h3["y"], n_rows=COUNTS_A, device=gpu_device).items()}, w3)
    _same(hostapi.mldivide(h3["X"], h3["y"], n_rows=COUNTS_A), w3)


def test_mldivide_across_byte_offsets(gpu_device, ml_ref):
    """epi_mldiv_run_device, case B: D = 16, F = 16, row counts (5, 16, 11, 13), R = 2^22 + 1000, all seven outputs: 4 R items in
    five launches.  X holds 256 R doubles (2^33 + 2 MB bytes: passes 2^31, 2^32, 2^33); m, rdiag [4, 16, R] and fitted [4, 16, R]
    hold 64 R doubles and pass 2^31; perm (int32), y and the [4, R] outputs stay below 2^31."""
    import torch
    from epidemicmodeling_amd import _lib
    from tests import mldivide_ref as ML
    D, F, R, counts = 16, 16, R_B, (5, 16, 11, 13)
    K = len(counts)
    assert len(set(counts)) == K
    shapes = _lib.mldiv_shapes(D, F, R, K)
    arrays = {"X": (D * F, 8), "y": (D, 8)}
    arrays.update({k: (int(np.prod(s[:-1])), 4 if k in ML.OUT_I32 else 8) for k, s in shapes.items()})
    reg = _sample_b(K, arrays, {"X": BITS, "m": (31,), "rdiag": (31,), "fitted": (31,)})
    H.need_free(gpu_device, _nbytes(shapes, ML.OUT_I32) + (D * F + D) * R * 8 + (3 << 30))
    t_case = time.perf_counter()
    dev = torch.device(gpu_device)
    t = _device_arrays(_ml_spec(D, F), R, dev)
    host = _host_arrays(_ml_spec(D, F), R, reg)
    sel = torch.as_tensor(reg, device=dev)
    _rule_1(t, host, sel)
    out, t_call = _device_call("mldiv", _lib.make_mldiv_desc(D, F, R, K), t, counts, shapes, ML.OUT_NAMES, dev)
    want = ml_ref.run(host["X"], host["y"], counts)
    _rule_3(out, want, reg, sel)
    assert not (want["status"] & ML.NONFINITE_INPUT).any() and len(np.unique(want["rank"])) >= 3, np.unique(want["rank"])
    H.report_limits(f"mldivide B D={D} F={F} K={K} R={R} ({K * R} items, {K + 1} launches), sample {reg.size} regions", t_call, t_case, dev)
    del out, t
    torch.cuda.empty_cache()


# ----------------------------------------------------------------------------------------------------------------- svr
SVR_TOL, SVR_MAX_ITER = 1e-3, 3


@pytest.fixture(scope="module")
def sv_ref(tmp_path_factory):
    from tests.svr_ref import SvrRef
    return SvrRef(tmp_path_factory.mktemp("svr_ref_limits"))


def _sv_spec(D, F):
    """X integer levels, y dyadic in [-1/2, 1/2); per region: box 1/2 .. 2, epsilon 0 .. 3/64, kernel_scale 1/2 .. 2"""
    return [("X", (D, F), _levels(41)), ("y", (D,), _dyadic(42, -20)), ("box", (), _quarter_steps(43, 1)),
            ("epsilon", (), lambda c: H.as_f64(H.chain_hash(c, 44) % 4) * 2.0 ** -6), ("kernel_scale", (), _quarter_steps(45, 1))]


SV_PLANTS_A = [("X", (0, 0), PLANTED_A[0], float("nan")), ("y", (0,), PLANTED_A[1], float("inf")), ("X", (0, 1), PLANTED_A[2], float("inf"))]


def _sv_kw(h, counts, kernel):
    return dict(n_rows=counts, kernel=kernel, box=h["box"], epsilon=h["epsilon"], kernel_scale=h["kernel_scale"], tol=SVR_TOL,
                max_iter=SVR_MAX_ITER)


def _sv_a(ref, kernel):
    if "sv_host" not in _A:
        reg = _sample_a()
        host = _host_arrays(_sv_spec(6, 2), R_A, reg)
        host["y"][:, reg % 8 == 0] = 0.25                    # every eighth region: a constant target, which converges at once
        _plant(host, SV_PLANTS_A, reg)
        _A["sv_host"] = (reg,) + _frozen(host)
    if ("sv", kernel) not in _A:
        reg, host = _A["sv_host"]
        _A["sv", kernel] = _frozen(ref.run(host["X"], host["y"], **_sv_kw(host, COUNTS_A, kernel)))[0]
    return _A["sv_host"] + (_A["sv", kernel],)


@pytest.mark.parametrize("kernel", ["linear", "gaussian"])
def test_svr_past_64_row_counts(gpu_device, sv_ref, kernel):
    """epi_svr_run_device, case A with both kernels: D = 6, F = 2, K = 130 row counts 1 .. 6, R = 2^16 + 40, max_iter = 3 (most
    items stop at the cap: NOT_CONVERGED), every output.  The chunks' largest AND smallest counts differ, so g.lds and the
    Gaussian kernel's room for the prediction rows differ between the chunks.  Every eighth region's y is constant (status 0
    without a step).  Planted in row 0: a NaN in X (63 015), an Inf in y (63 016), an Inf in X (40 003): BAD_INPUT for every k
    of exactly these regions."""
    import torch
    from epidemicmodeling_amd import _lib
    from tests import svr_ref as SV
    D, F, R, K = 6, 2, R_A, len(COUNTS_A)
    reg, host, want = _sv_a(sv_ref, kernel)
    names = SV.out_names(kernel)
    shapes = _lib.svr_shapes(D, F, R, K)
    assert max(_nbytes({k: s}, SV.OUT_I32) for k, s in shapes.items()) < (1 << 31)
    H.need_free(gpu_device, _nbytes(shapes, SV.OUT_I32) + (D * F + D + 3) * R * 8 + (3 << 30))
    t_case = time.perf_counter()
    dev = torch.device(gpu_device)
    t = _device_arrays(_sv_spec(D, F), R, dev)
    t["y"][:, ::8] = 0.25
    _plant(t, SV_PLANTS_A)
    sel = torch.as_tensor(reg, device=dev)
    _rule_1(t, host, sel)
    out, t_call = _device_call("svr", _lib.make_svr_desc(D, F, R, K, kernel, SVR_TOL, SVR_MAX_ITER), t, COUNTS_A, shapes, names, dev)
    _rule_3(out, want, reg, sel)
    st, jp, jn = want["status"], _j(reg, np.asarray(PLANTED_A)), _j(reg, np.asarray(_neighbours()))
    assert (st[:, jp] == SV.BAD_INPUT).all() and (st == SV.BAD_INPUT).sum() == K * len(PLANTED_A)
    assert not (st[:, jn] & (SV.BAD_INPUT | SV.NONFINITE)).any() and np.isfinite(want["fitted"][:, :, jn]).all()
    const = (reg % 8 == 0) & ~np.isin(reg, PLANTED_A)
    assert const.sum() >= len(CONSTANT_A) - 1 and (st[:, const] == 0).all() and (want["n_iter"][:, const] == 0).all()
    assert (st == SV.NOT_CONVERGED).any() and want["n_iter"].max() == SVR_MAX_ITER and len(np.unique(st)) >= 3, np.unique(st)
    H.report_limits(f"svr A {kernel} D={D} F={F} K={K} R={R} max_iter={SVR_MAX_ITER} (chunks of 64 + 64 + 2 counts, 2 + 2 + 1 launches), "
                    f"sample {reg.size} regions", t_call, t_case, dev)
    del out, t
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kernel", ["linear", "gaussian"])
def test_svr_130_row_counts_batch_and_host(gpu_device, sv_ref, kernel):
    """the K = 130 problem of case A on three of its sampled regions through batch.svr and hostapi.svr"""
    from epidemicmodeling_amd import batch, hostapi
    h3, w3 = _three(*_sv_a(sv_ref, kernel))
    kw = _sv_kw(h3, COUNTS_A, kernel)
    _same({k: v.cpu().numpy() for k, v in batch.svr(h3["X"], h3["y"], device=gpu_device, **kw).items()}, w3)
    _same(hostapi.svr(h3["X"], h3["y"], **kw), w3)


def test_svr_across_byte_offsets(gpu_device, sv_ref):
    """epi_svr_run_device, case B, the linear kernel: D = 16, F = 16, row counts (5, 16, 11, 13), R = 2^22 + 1000, max_iter = 3,
    all eight outputs: 4 R items in five launches.  X passes 2^31, 2^32 and 2^33 bytes; beta, fitted [4, 16, R] and w [4, 16, R]
    pass 2^31; y, the per-region arrays and the [4, R] outputs stay below 2^31."""
    import torch
    from epidemicmodeling_amd import _lib
    from tests import svr_ref as SV
    D, F, R, counts, kernel = 16, 16, R_B, (5, 16, 11, 13), "linear"
    K = len(counts)
    assert len(set(counts)) == K
    shapes = _lib.svr_shapes(D, F, R, K)
    arrays = {"X": (D * F, 8), "y": (D, 8), "box": (1, 8), "epsilon": (1, 8), "kernel_scale": (1, 8)}
    arrays.update({k: (int(np.prod(s[:-1])), 4 if k in SV.OUT_I32 else 8) for k, s in shapes.items()})
    reg = _sample_b(K, arrays, {"X": BITS, "beta": (31,), "w": (31,), "fitted": (31,)})
    H.need_free(gpu_device, _nbytes(shapes, SV.OUT_I32) + (D * F + D + 3) * R * 8 + (3 << 30))
    t_case = time.perf_counter()
    dev = torch.device(gpu_device)
    t = _device_arrays(_sv_spec(D, F), R, dev)
    host = _host_arrays(_sv_spec(D, F), R, reg)
    sel = torch.as_tensor(reg, device=dev)
    _rule_1(t, host, sel)
    out, t_call = _device_call("svr", _lib.make_svr_desc(D, F, R, K, kernel, SVR_TOL, SVR_MAX_ITER), t, counts, shapes, SV.out_names(kernel), dev)
    want = sv_ref.run(host["X"], host["y"], **_sv_kw(host, counts, kernel))
    _rule_3(out, want, reg, sel)
    assert not (want["status"] & SV.BAD_INPUT).any() and want["n_iter"].max() == SVR_MAX_ITER
    H.report_limits(f"svr B {kernel} D={D} F={F} K={K} R={R} max_iter={SVR_MAX_ITER} ({K * R} items, {K + 1} launches), sample {reg.size} regions",
                    t_call, t_case, dev)
    del out, t
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ rate_map
RM_KW = dict(effect_lag=3, ridge=1e-6, thr=0.1, red=0.01)
RM_NO_FIT = ("lambda_hat", "new_cases_est", "status")


@pytest.fixture(scope="module")
def rm_ref(tmp_path_factory):
    from tests.rate_map_ref import RatemapRef
    return RatemapRef(tmp_path_factory.mktemp("ratemap_ref_limits"))


def _rm_spec(T, n, K=None):
    """ip integer levels, y dyadic in [-1/4, 1/4), new_smoothed dyadic in (0, 1024]; K: lambda_in [K, T, R] dyadic in [-1/4, 1/4)"""
    spec = [("ip", (T, n), _levels(51)), ("y", (T,), _dyadic(52, -21)), ("new_smoothed", (T,), _positive(53, -10))]
    return spec + ([("lambda_in", (K, T), _dyadic(54, -21))] if K else [])


RM_PLANTS_A = [("y", (0,), r, float("nan")) for r in PLANTED_A]                                  # fit = 1: a leading NaN target
RM_PLANTS_A0 = [("lambda_in", (slice(None), 7), r, float("nan")) for r in PLANTED_A]             # fit = 0: a NaN rate on the last day


def _rm_problem(h, counts, lags, fit):
    return dict(ip=h["ip"], y=h["y"] if fit else None, new_smoothed=h["new_smoothed"], extra=None, lambda_in=None if fit else h["lambda_in"],
                n_train=tuple(counts), lags=tuple(lags), fit=fit, **RM_KW)


def _rm_a(ref):
    if "rm" not in _A:
        reg = _sample_a()
        host = _host_arrays(_rm_spec(8, 1, len(COUNTS_A)), R_A, reg)
        _plant(host, RM_PLANTS_A + RM_PLANTS_A0, reg)
        want1 = ref.run(_rm_problem(host, COUNTS_A, (1,), 1))
        want0 = ref.run(_rm_problem(host, COUNTS_A, (1,), 0), RM_NO_FIT)
        _A["rm"] = (reg,) + _frozen(host, want1, want0)
    return _A["rm"]


def _rm_tensors(t, fit):
    return {"ip": t["ip"], "y": t["y"] if fit else None, "new_smoothed": t["new_smoothed"], "extra": None,
            "lambda_in": None if fit else t["lambda_in"]}


def test_rate_map_past_64_train_ends(gpu_device, rm_ref):
    """epi_ratemap_run_device, case A: T = 8, n = 1, one lag (F = 2), E = 0, K = 130 train ends 1 .. 6, R = 2^16 + 40.  First
    fit = 1 with all seven outputs, then fit = 0 with lambda_in [130, 8, R] and lambda_hat, new_cases_est, status.  Planted: a NaN
    in y's first day of regions 63 015, 63 016 and 40 003 (LEADING_NAN for every k of exactly these regions); for fit = 0 a NaN
    in lambda_in's last day of the same regions (NONFINITE; an Inf there would be clipped to the threshold).  Every other sampled item has status 0."""
    import torch
    from epidemicmodeling_amd import _lib
    from tests import rate_map_ref as RM
    T, n, lags, R, K = 8, 1, (1,), R_A, len(COUNTS_A)
    reg, host, want1, want0 = _rm_a(rm_ref)
    assert max(COUNTS_A) <= T
    shapes = _lib.ratemap_shapes(T, n, R, 0, K, len(lags))
    assert max(_nbytes({k: s}, ("status",)) for k, s in shapes.items()) < (1 << 31)
    H.need_free(gpu_device, _nbytes(shapes, ("status",)) + (T * n + 2 * T + K * T) * R * 8 + (3 << 30))
    dev = torch.device(gpu_device)
    jp, jn = _j(reg, np.asarray(PLANTED_A)), _j(reg, np.asarray(_neighbours()))
    for fit, want, names, bad in ((1, want1, RM.OUT_NAMES, RM.LEADING_NAN), (0, want0, RM_NO_FIT, RM.NONFINITE)):
        t_case = time.perf_counter()
        t = _device_arrays(_rm_spec(T, n, None if fit else K), R, dev)
        _plant(t, RM_PLANTS_A if fit else RM_PLANTS_A + RM_PLANTS_A0)
        sel = torch.as_tensor(reg, device=dev)
        _rule_1(t, {k: host[k] for k in t}, sel)
        d = _lib.make_ratemap_desc(T, n, R, 0, K, lags, fit, RM_KW["effect_lag"], RM_KW["ridge"], RM_KW["thr"], RM_KW["red"])
        out, t_call = _device_call("ratemap", d, _rm_tensors(t, fit), COUNTS_A, shapes, names, dev)
        _rule_3(out, want, reg, sel)
        st = want["status"]
        assert (st[:, jp] == bad).all() and (st != 0).sum() == K * len(PLANTED_A) and (st[:, jn] == 0).all()
        assert np.isfinite(want["new_cases_est"][:, :, jn]).all() and not np.isfinite(want["new_cases_est"][:, :, jp]).all()
        H.report_limits(f"rate_map A fit={fit} T={T} n={n} lags={lags} K={K} R={R} (chunks of 64 + 64 + 2 train ends, 2 + 2 + 1 launches), "
                        f"sample {reg.size} regions", t_call, t_case, dev)
        del out, t
        torch.cuda.empty_cache()


def test_rate_map_130_train_ends_batch_and_host(gpu_device, rm_ref):
    """the K = 130 problem of case A on three of its sampled regions through batch.rate_map and hostapi.rate_map, with and
    without a fit"""
    from epidemicmodeling_amd import batch, hostapi
    reg, host, want1, want0 = _rm_a(rm_ref)
    h3, w1 = _three(reg, host, want1)
    _, w0 = _three(reg, host, want0)
    kw = dict(lags=(1,), ridge=RM_KW["ridge"], lambda_threshold=RM_KW["thr"], reduction_effect=RM_KW["red"], effect_lag=RM_KW["effect_lag"])
    for api, extra in ((batch, dict(device=gpu_device)), (hostapi, {})):
        cpu = lambda o: {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in o.items()}
        _same(cpu(api.rate_map(h3["ip"], h3["new_smoothed"], COUNTS_A, y=h3["y"], **kw, **extra)), w1)
        _same(cpu(api.rate_map(h3["ip"], h3["new_smoothed"], COUNTS_A, lambda_in=h3["lambda_in"], outputs=RM_NO_FIT, **kw, **extra)), w0)


def test_rate_map_across_byte_offsets(gpu_device, rm_ref):
    """epi_ratemap_run_device, case B: T = 22, n = 12, one lag (F = 24), E = 0, train ends (9, 22, 15), R = 2^22 + 1000, fit = 1,
    all seven outputs: 3 R items in four launches of ratemap_items, two launches of ratemap_region over R (regions 2^22 - 2 ..
    2^22 + 1 are sampled, and x_mx, y_filled and tracker are compared there).  ip holds 264 R doubles and passes 2^31, 2^32 and
    2^33 bytes; map [3, 24, R] (72 R) and lambda_hat, new_cases_est [3, 22, R] (66 R) pass 2^31; x_mx, y, y_filled, tracker,
    new_smoothed and status stay below 2^31."""
    import torch
    from epidemicmodeling_amd import _lib
    from tests import rate_map_ref as RM
    T, n, lags, R, counts = 22, 12, (1,), R_B, (9, 22, 15)
    K = len(counts)
    assert len(set(counts)) == K
    shapes = _lib.ratemap_shapes(T, n, R, 0, K, len(lags))
    arrays = {"ip": (T * n, 8), "y": (T, 8), "new_smoothed": (T, 8)}
    arrays.update({k: (int(np.prod(s[:-1])), 4 if k == "status" else 8) for k, s in shapes.items()})
    reg = _sample_b(K, arrays, {"ip": BITS, "map": (31,), "lambda_hat": (31,), "new_cases_est": (31,)}, region_kernel=True)
    assert {LAUNCH - 2, LAUNCH - 1, LAUNCH, LAUNCH + 1} <= set(reg.tolist())
    H.need_free(gpu_device, _nbytes(shapes, ("status",)) + (T * n + 2 * T) * R * 8 + (3 << 30))
    t_case = time.perf_counter()
    dev = torch.device(gpu_device)
    t = _device_arrays(_rm_spec(T, n), R, dev)
    host = _host_arrays(_rm_spec(T, n), R, reg)
    sel = torch.as_tensor(reg, device=dev)
    _rule_1(t, host, sel)
    d = _lib.make_ratemap_desc(T, n, R, 0, K, lags, 1, RM_KW["effect_lag"], RM_KW["ridge"], RM_KW["thr"], RM_KW["red"])
    out, t_call = _device_call("ratemap", d, _rm_tensors(t, 1), counts, shapes, RM.OUT_NAMES, dev)
    want = rm_ref.run(_rm_problem(host, counts, lags, 1))
    assert {"x_mx", "y_filled", "tracker"} <= set(want)
    _rule_3(out, want, reg, sel)
    assert (want["status"] == 0).any() and not (want["status"] & RM.LEADING_NAN).any()
    H.report_limits(f"rate_map B T={T} n={n} lags={lags} K={K} R={R} ({K * R} items, {K + 1} + 2 launches), sample {reg.size} regions",
                    t_call, t_case, dev)
    del out, t
    torch.cuda.empty_cache()

"""The joint scores (epi_ejoint_run_device, csrc/ens_joint.hpp) at their production launch bound and across the
2 / 4 / 8 GiB byte offsets of their arrays and of their workspace.

ejoint_members, ejoint_pairs and ejoint_vario cut their unit grids (items; items x tiles; items x wcap) at kEnsLaunchItems = 2^25
and hand the kernel the first unit of a launch (unit0).  tests/test_gpu_ejoint.py reaches a second launch only through the
descriptor hook test_launch_tiles with a few hundred units, so neither the constant nor u / tiles, u % tiles, u / wcap and
ejoint_swizzle over a launch of 2^25 blocks and over a ragged last one ran on a device, and no offset -- item tiles + tile,
item wcap + s, item nb + I, item wcap into the day list, (t rows + row) R D + r D + e, item D + e of member_dist -- was evaluated
past a few kilobytes.

The cases follow the three rules of tests/test_gpu_newer_call_limits.py, through the pieces of tests/helpers.py:

 1. inputs by formula per element (helpers.chain_hash; dyadic values of 20 significant bits, exact in float; one element in
    sixteen of src and of the truth NaN, so that members are absent and days are missing), evaluated by torch on the
    device for the whole array and by NumPy for the sample, the two compared bit for bit before the call;
 2. every output poisoned (helpers.poisoned); after the call no word of any output of the WHOLE call may hold the poison.  The
    workspace is poisoned too, but the poison rule is NOT applied to it as it stands: ejoint_pairs and ejoint_vario return early,
    by design, for an undefined item (no member left or no day), and ejoint_vario for s >= W, so those slots stay unwritten and
    ejoint_final never reads them.  Instead the unwritten words are counted per array, from the layout of ejoint_ws_size /
    ejoint_carve, and must be exactly those: none in tsum, mask, n_mem, n_day; tiles a word for every undefined item in tile;
    wcap - W (wcap for an undefined item) in vrow; wcap - W in days (int32 words) -- counted from the call's own n_members and
    n_days, which rule 3 holds to the restatement;
 3. a sample of WHOLE regions -- all D members, all four rows, the region's own truth_series column and first_day -- equals, bit
    for bit and NaN to NaN, tests/ejoint_ref.c run on the sample alone.  The sample holds both sides of every launch boundary of
    each of the three kernels (units translated to items and to regions), both sides of the element where each array's byte
    offset first reaches 2^31, 2^32, 2^33 -- src, member_dist, and the workspace arrays tile, vrow, mask, days both by their
    position in the workspace and by their offset from their own base --, regions 0, 1, last - 1, last, and a spread.  Each test
    asserts that its sample holds these classes and that the arrays pass exactly the offsets listed here (helpers.assert_passes,
    over EVERY array).

Undefined items are part of every case: first_day = k1 for one region in sixteen, a window without a truth, and a planted region
whose row 0 (and with it the derived row) has every member absent.  Their share is capped: the formula gives first_day >= k1 to
at most one region in eight, and the call reports at most one undefined item in eight (asserted), so no case passes by leaving
its items out.

The cases and which of 2^31 / 2^32 / 2^33 bytes each array passes (an array not named stays below 2^31):
  J1  double and float, T = 3, rows 3 + 1, D = 9, R = 2^24 + 1000, window 0 .. 3, vs_order 1, max_lag 1, every output.
      2^26 + 4000 items: ejoint_members<1> and ejoint_pairs (one tile an item) in three launches, ejoint_vario<1> (3 units an item)
      in seven.  src all three (float: 2^31, 2^32); member_dist 2^31, 2^32; the workspace (68 B an item, 4.56 GB) 2^31 (inside
      vrow) and 2^32 (inside days).
  J2  float, T = 3, rows 3 + 1, D = 130 (3 blocks, 6 tiles, two members in the last block), R = 2^21 + 100, vs_order 0.
      6 x (2^23 + 400) = 50 334 048 tile units in two launches; unit 2^25 is tile 2 of item 5 592 405: the boundary lies inside an
      item.  src (T = 3 rather than 2: 9.8 GB, so that it does pass 2^33) and member_dist (8.7 GB) all three; the workspace
      (0.99 GB) none.
  J3  float, T = 2, rows 3 + 1, D = 4 096 (64 blocks, 2 080 tiles; NV = 64), R = 2^16 + 50, window 0 .. 2 (one or two days by
      first_day), vs_order 0.  545 675 520 tile units in 17 launches.  tile [items][2080] (4.37 GB) 2^31 and 2^32 from its own
      base; src 2^31, 2^32; member_dist all three; the workspace (4.51 GB) 2^31 and 2^32, both inside tile.

Showing that the tests bite (scratch builds of the library with one line of ens_joint.hpp changed, never committed; every access
stays inside its array):
  (i)    ejoint_pairs with u = ejoint_swizzle(blockIdx.x, a.units) (unit0 dropped): J1 (both storages), J2 and J3 all fail on rule
         2 -- every later launch rewrites the slots of the first, ejoint_final adds the poison the later slots still hold and
         the payload survives the sum: 30 859 126 words of spread_term in J1, 2 575 711 in J2, 221 783 in J3 (es = tt - sp gets
         the NaN of the subtraction, not the payload).  Both launch-cut tests of tests/test_gpu_ejoint.py fail on their bits.
  (ii)   the tile slot's offset taken through 32 bits of bytes ((uint32_t)(.. * 8) / 8): J3 alone fails, on rule 2 -- 3 839
         words of spread_term, the defined items whose slots lie past 4 GiB; J1, J2 and tests/test_gpu_ejoint.py pass.
  (iii)  ejoint_vario's vrow offset with the item masked to 25 bits and narrowed to int: J1 fails in both storages on rule 2 --
         30 859 126 words of vs, the defined items behind item 2^25; J2 and J3 (no variogram score) and the small module pass.
  (iv)   D <= 2048 dispatched to NV = 16: the member-count grid fails at 1 025, 2 000 and 2 048 in both storages ("member_dist: a
         word left unwritten": the members from 1 024 on), as does the launch cut at D = 1 025; every D <= 1 024 and the D
         >= 2 049 pass, and so do J1 - J3 (NV = 1, 4, 64).
  (v)    ej = I * 64 + lane in ejoint_pairs: the grid fails at every D from 65 on (34 cases) and passes at 1 .. 64; the seven other
         tests of tests/test_gpu_ejoint.py with D > 64 fail; J2 and J3 fail on rule 3 (J3: 242 words of es over every sampled
         region); J1 (D = 9: one block) passes.
No mutation went uncaught.

What stays unrun on one device: the refusal of items x max(tiles, wcap) > 2^40 at its value (the workspace would hold 8.8 TB),
rows' R near 2^31, vrow and days past 2^33 bytes (items x wcap > 2^30 with src [wcap, rows, R D] beside them), tile past 2^33.
They stay with tests/test_ejoint_abi.py and tests/test_ejoint_emu.py.

Measured on one MI355X (the library call alone / the whole case with input generation, sampling and the restatement /
torch.cuda.max_memory_allocated):
  J1, double  0.34 s / 1.5 s / 26.8 GiB      J1, float  0.34 s / 0.5 s / 21.8 GiB
  J2          0.19 s / 2.2 s / 27.7 GiB      J3         1.91 s / 4.2 - 5.4 s / 27.2 GiB
J3's 545.7 M one- and two-day tiles take 3.5 ns each; its restatement of 33 regions takes 2.6 s of the case.  The case stays
below 10 s, so tile keeps its 2^32 crossing.  The module takes 12 s (J3: 4.2 s inside the whole suite, 5.4 s run alone).
No time is asserted; every case prints its figures in a line that starts with [limits].
"""
import ctypes as C
import time

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

BITS = H.LIMIT_BITS
LAUNCH = 1 << 25            # kEnsLaunchItems: ejoint_for_units cuts every unit grid with it
NAN = float("nan")

_value = H.with_nan(H.dyadic10(91), 92, 16)              # a member's day: dyadic in (0, 1024], one in sixteen NaN
_truth = H.with_nan(H.dyadic10(93), 94, 16)              # the truth: one day in sixteen missing
RT = 61                                                  # truth columns; region r reads column chain_hash(r, 95) % RT
_series = lambda c: H.chain_hash(c, 95) % RT


def _first_day(T, k1):
    """0 .. T - 1 by hash; k1 (no day: an undefined item) for one region in sixteen"""
    return lambda c: H.chain_hash(c, 96) % T + (k1 - H.chain_hash(c, 96) % T) * ((H.chain_hash(c, 97) % 16 == 0) * 1)


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    from tests.ejoint_ref import EjointC
    return EjointC(tmp_path_factory.mktemp("ejoint_ref_limits"))


def _ws_layout(items, nb, tiles, wcap):
    """the workspace as ejoint_carve lays it out: [(array, first byte, elements an item, element size)] and its size, which is
    ejoint_ws_size's items ((1 + tiles + wcap + nb) 8 + (2 + wcap) 4)"""
    parts, pos = [], 0
    for name, per, sz in (("tsum", 1, 8), ("tile", tiles, 8), ("vrow", wcap, 8), ("mask", nb, 8), ("n_mem", 1, 4), ("n_day", 1, 4),
                          ("days", wcap, 4)):
        parts.append((name, pos, per, sz))
        pos += items * per * sz
    assert pos == items * ((1 + tiles + wcap + nb) * 8 + (2 + wcap) * 4)
    return parts, pos


def _ws_crossings(parts, items, R):
    """{label: regions}: the items (as regions) on both sides of the element of a workspace array that holds byte 2^bit of the
    workspace, and of the element whose offset from the array's own base first reaches 2^bit"""
    out = {}
    for bit in BITS:
        for name, pos, per, sz in parts:
            size = items * per * sz
            for label, byte in ((f"workspace 2^{bit} in {name}", (1 << bit) - pos), (f"{name} 2^{bit}", 1 << bit)):
                if 0 < byte < size:
                    e = byte // sz
                    out[label] = sorted({((e + d) // per) % R for d in (-2, -1, 0, 1) if 0 <= e + d < items * per})
    return out


def _words32(t, value):
    import torch
    return int(torch.count_nonzero(t == value))


def _case(gpu_device, cref, what, *, T, rows, R, D, storage, k0, k1, vs_order, max_lag, passes, ws_in, n_spread, wide=True):
    """One case.  passes: {array: bits} over every input, output and workspace array (an array's own size) and "workspace" (its
    whole size); ws_in: {bit: the workspace array that holds byte 2^bit of the workspace}; wide: the regions next to a crossing's
    join the sample (off where a region costs the restatement 8.4 M pairs a row).  Returns (want, reg, info)."""
    import torch
    from epidemicmodeling_amd import _lib
    ro, B = rows + 1, R * D
    items, nb, wcap = ro * R, (D + 63) // 64, k1 - k0
    tiles = nb * (nb + 1) // 2
    f32 = storage == "f32"
    es, tdt, ndt = (4, torch.float32, np.float32) if f32 else (8, torch.float64, np.float64)
    names = [k for k in _lib.EJOINT_OUT_NAMES if k != "vs" or vs_order]
    shapes = {k: sh for k, sh in _lib.ejoint_shapes(rows, R, D, 1).items() if k in names}
    d = _lib.make_ejoint_desc(T, rows, R, D, RT, vs_order, max_lag, storage=storage, derive_newcases=1, k0=k0, k1=k1)
    n = C.c_size_t(0)
    err = C.create_string_buffer(256)
    _lib.check(_lib.lib().epi_ejoint_workspace_bytes(C.byref(d), C.byref(n), err), err)
    parts, total = _ws_layout(items, nb, tiles, wcap)
    assert n.value == total and total % 8 == 0
    nbytes = {k: int(np.prod(sh, dtype=np.int64)) * (4 if k in _lib.EJOINT_OUT_I32 else 8) for k, sh in shapes.items()}
    nbytes.update(src=T * rows * B * es, truth=T * ro * RT * 8, population=R * 8, truth_series=R * 4, first_day=R * 4, workspace=total)
    nbytes.update({"ws." + name: items * per * sz for name, _, per, sz in parts})
    H.assert_passes(nbytes, passes)
    for bit, name in ws_in.items():
        pos, per, sz = next((p, pe, s) for nm, p, pe, s in parts if nm == name)
        assert pos <= (1 << bit) < pos + items * per * sz, (bit, name)
    assert sorted(ws_in) == list(passes.get("workspace", ()))
    H.need_free(gpu_device, 2 * sum(v for k, v in nbytes.items() if not k.startswith("ws.")) + (4 << 30))
    t_case = time.perf_counter()
    dev = torch.device(gpu_device)
    first_day = _first_day(T, k1)
    truth_dev, truth_host = H.scaled_rows(_truth, ro, 3, 2.0 ** 37)
    src = H.formula_rows(T * rows, B, dev, _value, tdt).reshape(T, rows, B)
    truth = truth_dev(T, RT, dev)
    r_all = torch.arange(R, dtype=torch.int64, device=dev)
    fd, ts = first_day(r_all).to(torch.int32), _series(r_all).to(torch.int32)
    pop, N16 = H.cycled_population(R, dev)
    assert float((fd >= k1).double().mean()) <= 1.0 / 8.0 and bool((fd >= k1).any()) and bool((fd == 0).any())
    # the sample: launch boundaries in units of each kernel, translated to the unit's item and the item's region
    grids = {"ejoint_members": (items, 1), "ejoint_pairs": (items * tiles, tiles)}
    if vs_order:
        grids["ejoint_vario"] = (items * wcap, wcap)
    bnd = {k: sorted({(u // per) % R for u in H.boundary_items(LAUNCH, units)}) for k, (units, per) in grids.items()}
    launches = {k: -(-units // LAUNCH) for k, (units, _) in grids.items()}
    side = (-1, 0, 1) if wide else (0,)
    cross = {}
    for k, rws, N, sz in (("src", T * rows, B, es), ("member_dist", ro, B, 8)):
        cols = H.crossing_regions(rws, N, bits=BITS, itemsize=sz)
        assert len(cols) == 4 * len(passes.get(k, ())), (k, cols)
        cross[k] = sorted({c // D + s for c in cols for s in side})
    for k, regs in _ws_crossings(parts, items, R).items():
        cross[k] = sorted({r + s for r in regs for s in side})
    assert sum(k.startswith("workspace 2^") for k in cross) == len(ws_in)
    assert sorted(k for k in cross if not k.startswith("workspace") and k not in ("src", "member_dist")) == \
        sorted(f"{k[3:]} 2^{b}" for k, bits in passes.items() if k.startswith("ws.") for b in bits)
    r_bad = bnd["ejoint_pairs"][0]                                       # every member of row 0 absent there
    r_none = int(torch.nonzero(fd >= k1)[0])                             # the first region without a day
    reg, S = H.region_sample(R, n_spread, *bnd.values(), *cross.values(), [r_none])
    for k, regs in list(bnd.items()) + list(cross.items()):
        assert set(r for r in regs if 0 <= r < R) <= S and (regs or launches.get(k) == 1), k
    assert all(launches[k] == 1 or len(H.boundary_items(LAUNCH, grids[k][0])) == 4 * (launches[k] - 1) for k in grids)
    # rule 1
    cols = H.region_columns(reg, D)
    j_of = lambda r: int(np.searchsorted(reg, r))
    src_s = H.formula_sample(T * rows, B, cols, _value, ndt).reshape(T, rows, cols.size)
    truth_s = truth_host(T, RT, np.arange(RT))
    src[:, 0, r_bad * D:(r_bad + 1) * D] = NAN
    src_s[:, 0, j_of(r_bad) * D:(j_of(r_bad) + 1) * D] = np.nan
    fd_s, ts_s, pop_s = first_day(reg).astype(np.int32), _series(reg).astype(np.int32), N16[reg % 16]
    sel, csel = torch.as_tensor(reg, device=dev), torch.as_tensor(cols, device=dev)
    held = H.selected(src, csel)
    assert held.dtype == src_s.dtype and np.array_equal(held, src_s, equal_nan=True), "device and host evaluate the formula differently"
    assert np.array_equal(truth.cpu().numpy(), truth_s, equal_nan=True) and np.array_equal(H.selected(fd, sel), fd_s)
    assert np.array_equal(H.selected(ts, sel), ts_s) and np.array_equal(H.selected(pop, sel), pop_s)
    del held
    # rule 2
    out = {k: H.poisoned(sh, torch.int32 if k in _lib.EJOINT_OUT_I32 else torch.float64, dev) for k, sh in shapes.items()}
    ins, outs = _lib.EjointInputs(), _lib.EjointOutputs()
    for k, v in zip(_lib.EJOINT_IN_NAMES, (src, pop, truth, ts, fd)):
        setattr(ins, k, C.c_void_p(v.data_ptr()))
    for k in _lib.EJOINT_OUT_NAMES:
        setattr(outs, k, C.c_void_p(out[k].data_ptr()) if k in out else None)
    ws = H.poisoned_words(total // 8, dev)
    t_call = H.timed_device_call("epi_ejoint_run_device", dev, C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(ws.data_ptr()), C.c_size_t(total))
    H.assert_no_poison(out)
    # the workspace: exactly the slots the kernels leave out by design are unwritten
    nm, nd = out["n_members"].reshape(-1).long(), out["n_days"].reshape(-1).long()
    und = (nm == 0) | (nd == 0)
    n_und, days_all, days_def = int(und.sum()), int(nd.sum()), int(nd[~und].sum())
    assert 0 < n_und <= items // 8, ("undefined items", n_und, items)
    part = {name: ws[pos // 8:(pos + items * per * sz) // 8] for name, pos, per, sz in parts}
    lo, hi = H.POISON64 & 0xFFFFFFFF, H.POISON64 >> 32
    i32 = lambda t: t.view(torch.int32)
    left = {k: H.poison_words(part[k], 0) for k in ("tsum", "tile", "vrow", "mask")}
    left.update({k: _words32(i32(part[k]), lo - (1 << 32)) + _words32(i32(part[k]), hi) for k in ("n_mem", "n_day", "days")})
    expect = dict(tsum=0, mask=0, n_mem=0, n_day=0, tile=tiles * n_und, days=items * wcap - days_all,
                  vrow=items * wcap - days_def if vs_order else items * wcap)
    assert left == expect, ("unwritten workspace words (found, expected)", left, expect)
    # rule 3
    want = cref.joint(src_s, truth_s, reg.size, D, vs_order=vs_order, max_lag=max_lag, population=pop_s, truth_series=ts_s, first_day=fd_s,
                      k0=k0, k1=k1)
    H.compare_sample(out, want, {k: csel if k == "member_dist" else sel for k in out}, reg)
    wm, wd = want["n_members"], want["n_days"]
    assert ((wm[0, j_of(r_bad)] == 0) or (wd[0, j_of(r_bad)] == 0)) and (wm[3, j_of(r_bad)] == 0 or wd[3, j_of(r_bad)] == 0)
    assert (wd[:, j_of(r_none)] == 0).all() and (wm[:, j_of(r_none)] == D).all()
    assert ((wm > 0) & (wm < D) & (wd > 0)).any() and len(np.unique(wd)) >= min(3, wcap + 1)
    assert np.isfinite(want["es"]).sum() >= want["es"].size // 2 and np.isnan(want["es"]).any()
    H.report_limits(f"ejoint {what} {storage} T={T} rows={rows}+1 D={D} R={R} window {k0}..{k1} vs_order={vs_order} ({items} items, launches "
                    f"{launches}), {n_und} undefined items, sample {reg.size} regions", t_call, t_case, dev)
    info = dict(bnd=bnd, cross=cross, launches=launches, items=items, tiles=tiles)
    del out, src, truth, ws, part, nm, nd, und
    torch.cuda.empty_cache()
    return want, reg, info


@pytest.mark.parametrize("storage", ["f64", "f32"])
def test_many_small_items_past_one_launch(gpu_device, cref, storage):
    """J1.  2^26 + 4000 items of D = 9 members and three days: ejoint_members<1> and ejoint_pairs in three launches each,
    ejoint_vario<1> in seven; item = unit0 + blockIdx.x, u / wcap and u % wcap past 2^27 units.  src passes 2^31, 2^32 and (double)
    2^33 bytes, member_dist 2^31 and 2^32; byte 2^31 of the workspace lies in vrow, byte 2^32 in days."""
    R = (1 << 24) + 1000
    _, _, info = _case(gpu_device, cref, "J1", T=3, rows=3, R=R, D=9, storage=storage, k0=0, k1=3, vs_order=1, max_lag=1,
                       passes={"src": (31, 32) if storage == "f32" else BITS, "member_dist": (31, 32), "workspace": (31, 32)},
                       ws_in={31: "vrow", 32: "days"}, n_spread=48)
    assert info["items"] == (1 << 26) + 4000 and info["launches"] == {"ejoint_members": 3, "ejoint_pairs": 3, "ejoint_vario": 7}


def test_tiles_past_one_launch(gpu_device, cref):
    """J2.  D = 130: 6 tiles an item, 6 x (2^23 + 400) tile units in a full launch of 2^25 blocks and a ragged second one; the
    boundary is tile 2 of item 5 592 405 (row 2), inside an item, so u / tiles, u % tiles and ejoint_swizzle decide which slots of
    that item either launch fills.  src and member_dist pass 2^31, 2^32 and 2^33 bytes."""
    R = (1 << 21) + 100
    assert divmod(LAUNCH, 6) == (5592405, 2) and 5592405 // R == 2 and LAUNCH < 6 * 4 * R < 2 * LAUNCH
    _, reg, info = _case(gpu_device, cref, "J2", T=3, rows=3, R=R, D=130, storage="f32", k0=0, k1=3, vs_order=0, max_lag=0,
                         passes={"src": BITS, "member_dist": BITS}, ws_in={}, n_spread=48)
    assert info["launches"] == {"ejoint_members": 1, "ejoint_pairs": 2} and info["bnd"]["ejoint_pairs"] == [5592405 % R]


def test_tile_slots_past_four_gib_at_64_registers(gpu_device, cref):
    """J3.  D = 4 096: ejoint_members<64, float>, 2 080 tiles an item, 4 (2^16 + 50) items: 545 675 520 tile units in 17 launches,
    the tile slots [items][2080] passing 2^31 and 2^32 bytes from their own base (and the workspace's bytes 2^31 and 2^32 lying
    inside them); src passes 2^31 and 2^32, member_dist 2^31, 2^32 and 2^33.  A sampled region costs the restatement 8.4 M pairs
    a row and day, so only the regions that hold a boundary or a crossing and a spread of six are sampled (about thirty)."""
    R = (1 << 16) + 50
    assert 4 * R * 2080 * 8 > (1 << 32) + (1 << 25) and R * 4096 < (1 << 31) and 4 * (R - 1100) * 2080 * 8 < (1 << 32)
    _, reg, info = _case(gpu_device, cref, "J3", T=2, rows=3, R=R, D=4096, storage="f32", k0=0, k1=2, vs_order=0, max_lag=0,
                         passes={"src": (31, 32), "member_dist": BITS, "ws.tile": (31, 32), "workspace": (31, 32)},
                         ws_in={31: "tile", 32: "tile"}, n_spread=6, wide=False)
    assert info["launches"] == {"ejoint_members": 1, "ejoint_pairs": 17} and len(info["bnd"]["ejoint_pairs"]) >= 16 and reg.size <= 40

"""Generators of the random hunts of the batched calls added since the LASSO (tests/test_fuzz_calls.py without a device,
tests/test_gpu_fuzz_calls.py on one).  Plain NumPy: no torch, no device.

`make_<call>(seed)` is a pure function of the integer: it builds np.random.default_rng(seed), draws every size, option and
datum from it ("sizes from a drawn seed: hypothesis alone keeps them near their minima", tests/test_gpu_fuzz.py) and returns a
Case: `kw`, the keyword arguments the call's restatement takes (the GPU test maps them onto the call's `_run_device` helper);
`names`, the outputs asked for; `cut`, the launch-cut hook of the descriptor; `host`, whether the example also goes through
the hostapi entry; `summary`, one line for assertion messages; `features`, the strings naming what the example exercises.

CALLS maps a call's name to its Spec: the generator, the number of default seeds N (seeds 0 .. N - 1), the declared feature
list FEATURES (tests/test_fuzz_calls.py asserts that the default seeds reach every entry and nothing else) and
`result_features`, which names what only the restatement's result can tell (status values).  The size caps (*_FUZZ_CAP) say
what they keep under which time; profiles/fuzz_calls/README.md holds the measured seconds behind every N."""
from __future__ import annotations

import dataclasses
import warnings
from typing import Callable

import numpy as np


@dataclasses.dataclass
class Case:
    call: str
    seed: int
    kw: dict
    names: tuple
    cut: dict
    host: bool
    summary: str
    features: set
    flat: bool = False               # the ensemble calls: the example also goes through the batch entry with a 2-D src [T, B]
    noise: tuple = None              # a seeded twin (seeded_twin): (seed, stream) the call under test draws from; kw["z"] is their array


@dataclasses.dataclass
class Spec:
    make: Callable
    n: int
    features: tuple
    result_features: Callable = lambda want: set()


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _subset(rng, names, p_all=0.3):
    """a random non-empty subset of names, in their order; all of them with probability p_all"""
    names = tuple(names)
    if len(names) <= 1 or rng.random() < p_all:
        return names
    k = int(rng.integers(1, len(names)))
    keep = set(rng.permutation(len(names))[:k].tolist())
    return tuple(n for i, n in enumerate(names) if i in keep)


def _out_features(f, all_names, names):
    for n in all_names:
        f.add(f"out:{n}:{'yes' if n in names else 'no'}")


def _out_list(all_names):
    return tuple(f"out:{n}:{s}" for n in all_names for s in ("yes", "no"))


# ======================================================================================================================
# the four calls on a region-major ensemble: ensemble_summary, ensemble_score, path_functionals, ensemble_joint_score
# ======================================================================================================================
BIG_D = (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096)
EDGE_D = (1, 2, 3, 63, 64, 65, 127, 128, 129, 130)
NV = (1, 2, 4, 8, 16, 32, 64)                       # registers per lane of the dispatch by D: P / 64, P the power of two >= D
# items (day, row, region) of one example: keeps the NumPy restatements of the summary and the scores (a Python loop per item)
# under about 0.15 s an example on one CPU core
ENS_FUZZ_CAP = 400
# (rows, regions, days, draws) of a joint-score example, as rows' * R * W * D and, for the pair sums, rows' * R * W * D^2 / 64:
# keeps the NumPy restatement of one example under about 0.3 s
EJOINT_FUZZ_CAP = 200_000

_ENS_COMMON = (("storage:f64", "storage:f32", "population:yes", "population:no", "nonfinite:0", "nonfinite:0.02", "nonfinite:0.3",
                "item:all-nan:yes", "item:all-nan:no", "D:big", "D:small", "src:2-D", "src:3-D", "host:yes", "host:no")
               + tuple(f"D:nv={v}" for v in NV))


def nv_of(D):
    return max(64, 1 << (D - 1).bit_length()) // 64


def _ens_source(rng, f, cap, max_T=70):
    """src [T, rows, R * D], population or None; D mostly 1 .. 130 (two in five from EDGE_D), one in five from BIG_D with R <= 2,
    T <= 3, rows <= 2; R 1 .. 5, T 1 .. max_T cut down to `cap` items, rows 1 .. 4; both storages; NaN, +-Inf and tied members
    at 0 %, 2 % or 30 %; one whole item of NaN in half of the examples; population (the derived row) in half of those with
    rows >= 3; half of the examples with one row are also handed over as a 2-D src [T, R * D]"""
    if rng.random() < 0.2:
        D, R, T, rows = int(_pick(rng, BIG_D)), int(rng.integers(1, 3)), int(rng.integers(1, 4)), int(rng.integers(1, 3))
        f.add("D:big")
    else:
        D = int(_pick(rng, EDGE_D)) if rng.random() < 0.4 else int(rng.integers(1, 131))
        R, T, rows = int(rng.integers(1, 6)), int(rng.integers(1, max_T + 1)), int(rng.integers(1, 5))
        T = max(1, min(T, cap // ((rows + 1) * R)))
        f.add("D:small")
    f.add(f"D:nv={nv_of(D)}")
    src = rng.standard_normal((T, rows, R * D)) * 10.0 ** rng.uniform(-2, 2, size=(T, rows, 1))
    p = float(_pick(rng, (0.0, 0.02, 0.3)))
    f.add(f"nonfinite:{p:g}")
    m = rng.random(src.shape)
    src[m < p / 3] = np.nan
    src[(m >= p / 3) & (m < p / 2)] = np.inf
    src[(m >= p / 2) & (m < 2 * p / 3)] = -np.inf
    src[(m >= 2 * p / 3) & (m < p)] = 1.25
    all_nan = rng.random() < 0.5
    if all_nan:
        t, j, r = int(rng.integers(T)), int(rng.integers(rows)), int(rng.integers(R))
        src[t, j, r * D:(r + 1) * D] = np.nan
    f.add(f"item:all-nan:{'yes' if all_nan else 'no'}")
    f32 = rng.random() < 0.5
    f.add("storage:f32" if f32 else "storage:f64")
    if f32:
        src = src.astype(np.float32)
    pop = 10.0 ** rng.uniform(3, 7, R) if rows >= 3 and rng.random() < 0.5 else None
    f.add("population:yes" if pop is not None else "population:no")
    f.add("src:2-D" if rows == 1 and rng.random() < 0.5 else "src:3-D")
    return src, R, D, pop


def _truth(rng, f, src, R, D, pop):
    """truth [T, rows', Rt] and truth_series: Rt = R without a series, else Rt 1 .. R + 1 and any columns; a truth near the
    members, equal to one of them (one in ten), NaN (one in twenty) or +Inf (one in fifty)"""
    T, rows, _ = src.shape
    ro = rows + int(pop is not None)
    if rng.random() < 0.5:
        Rt = int(rng.integers(1, R + 2))
        ts = rng.integers(0, Rt, R).astype(np.int32)
        f.add("truth_series:yes")
        f.add("Rt!=R" if Rt != R else "Rt==R")
    else:
        Rt, ts = R, None
        f.add("truth_series:no")
    s = src.astype(np.float64)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # an item without a finite member has no mean: scale 1
        scale = np.nanmean(np.where(np.isfinite(s), np.abs(s), np.nan), axis=2, keepdims=True)
    scale = np.where(np.isfinite(scale), scale, 1.0)
    if pop is not None:
        scale = np.concatenate([scale, np.full((T, 1, 1), 1e3)], axis=1)
    truth = rng.standard_normal((T, ro, Rt)) * scale
    for c in range(Rt):                                      # equal to a member of a region that reads this column
        rs = [r for r in range(R) if (r if ts is None else int(ts[r])) == c]
        if not rs:
            continue
        r = int(_pick(rng, rs))
        hit = rng.random((T, rows)) < 0.1
        mem = s[:, :, r * D + int(rng.integers(D))]
        truth[:, :rows, c] = np.where(hit & ~np.isnan(mem), mem, truth[:, :rows, c])
    m = rng.random(truth.shape)
    truth[m < 0.05] = np.nan
    truth[(m >= 0.05) & (m < 0.07)] = np.inf
    return np.ascontiguousarray(truth), ts


def _window(rng, f, T, empty_ok):
    """k0, k1 anywhere in 0 <= k0 <= k1 <= T (k0 < k1 where the call has no empty window); one in four is the whole series"""
    if rng.random() < 0.25:
        k0, k1 = 0, T
    else:
        k0 = int(rng.integers(0, T + (1 if empty_ok else 0)))
        k1 = int(rng.integers(k0 + (0 if empty_ok else 1), T + 1))
    f.add("window:whole" if (k0, k1) == (0, T) else ("window:empty" if k0 == k1 else "window:part"))
    return k0, k1


def _first_day(rng, f, R, T):
    fd = rng.integers(0, T + 2, R).astype(np.int32) if rng.random() < 0.5 else None
    f.add("first_day:yes" if fd is not None else "first_day:no")
    return fd


def _host(rng, f):
    h = bool(rng.random() < 0.25)
    f.add("host:yes" if h else "host:no")
    return h


# ---- ensemble_summary ---------------------------------------------------------------------------------------------------
ENS_OUT = ("mean", "std", "min", "max", "quantiles")         # count is always handed over: validate refuses a call without it
ENS_FEATURES = _ENS_COMMON + _out_list(ENS_OUT) + ("n_q:1", "n_q:16", "q:0", "q:1")


def make_ensemble_summary(seed):
    """epi_ens_validate: T, rows, R >= 1, D 1 .. 4096, n_q 1 .. 16 with every q in [0, 1], population only with rows >= 3.
    The source is _ens_source's; q holds 0 and 1 now and then (the ends of the order statistics) and repeats."""
    rng, f = np.random.default_rng(seed), set()
    src, R, D, pop = _ens_source(rng, f, ENS_FUZZ_CAP)
    n_q = int(_pick(rng, (1, 16))) if rng.random() < 0.3 else int(rng.integers(1, 17))
    q = rng.random(n_q)
    ends = rng.random(n_q)
    q[ends < 0.1] = 0.0
    q[ends > 0.9] = 1.0
    if n_q in (1, 16):
        f.add(f"n_q:{n_q}")
    f.update({"q:0"} if (q == 0).any() else set())
    f.update({"q:1"} if (q == 1).any() else set())
    names = _subset(rng, ENS_OUT) + ("count",)
    _out_features(f, ENS_OUT, names)
    host = _host(rng, f)
    T, rows, _ = src.shape
    return Case("ensemble_summary", seed, dict(src=src, R=R, D=D, q=tuple(float(v) for v in q), population=pop), names, {}, host,
                f"ensemble_summary seed={seed} T={T} rows={rows} R={R} D={D} {src.dtype} n_q={n_q} pop={pop is not None} names={names}", f, flat="src:2-D" in f)


# ---- ensemble_score -----------------------------------------------------------------------------------------------------
ESCORE_OUT = ("crps", "wis", "ae", "width", "rank", "ties", "cover", "count", "crps_mean", "wis_mean", "ae_mean", "n_scored",
              "cover_frac", "pit_hist")
ESCORE_FEATURES = (_ENS_COMMON + _out_list(ESCORE_OUT) + ("truth_series:yes", "truth_series:no", "Rt!=R", "Rt==R", "window:whole",
                   "window:empty", "window:part", "first_day:yes", "first_day:no", "n_a:0", "n_a:8", "n_bins:0", "n_bins:32",
                   "launches:1", "launches:>1"))


def make_ensemble_score(seed):
    """escore_check_desc / epi_escore_validate: T, rows, R, Rt >= 1, D 1 .. 4096, n_a 0 .. 8 with alpha in (0, 1) strictly
    descending, n_bins 0 .. 32, 0 <= k0 <= k1 <= T (the empty window included), Rt = R without truth_series, pit_hist only
    with n_bins >= 1 (width and cover_frac only with n_a >= 1: they are empty without a level), test_launch_items >= 0 (here: below the item count, no multiple of R where that can be had, so a cut
    falls inside an item row)."""
    rng, f = np.random.default_rng(seed), set()
    src, R, D, pop = _ens_source(rng, f, ENS_FUZZ_CAP)
    truth, ts = _truth(rng, f, src, R, D, pop)
    T, rows, _ = src.shape
    n_a = int(_pick(rng, (0, 8))) if rng.random() < 0.3 else int(rng.integers(0, 9))
    alpha = tuple(float(v) for v in np.sort(rng.uniform(0.01, 0.99, n_a))[::-1])
    while len(set(alpha)) < n_a:                             # strictly descending (a repeat has probability ~ 0)
        alpha = tuple(float(v) for v in np.sort(rng.uniform(0.01, 0.99, n_a))[::-1])
    n_bins = int(_pick(rng, (0, 32))) if rng.random() < 0.3 else int(rng.integers(0, 33))
    for k, v, ends in (("n_a", n_a, (0, 8)), ("n_bins", n_bins, (0, 32))):
        if v in ends:
            f.add(f"{k}:{v}")
    k0, k1 = _window(rng, f, T, True)
    fd = _first_day(rng, f, R, T)
    # width and cover_frac hold n_a planes: with n_a = 0 they are empty, and an entry asked for nothing else answers "no output requested"
    names = _subset(rng, [n for n in ESCORE_OUT if (n != "pit_hist" or n_bins >= 1) and (n_a or n not in ("width", "cover_frac"))])
    _out_features(f, ESCORE_OUT, names)
    items = T * (rows + int(pop is not None)) * R
    cut = 0
    if items > 1 and rng.random() < 0.5:
        cut = int(rng.integers(1, items))
        if R > 1 and cut % R == 0:
            cut = cut - 1 if cut > 1 else cut + 1
    f.add("launches:>1" if cut else "launches:1")
    host = _host(rng, f)
    kw = dict(src=src, truth=truth, R=R, D=D, alpha=alpha, n_bins=n_bins, population=pop, truth_series=ts, first_day=fd, k0=k0, k1=k1)
    return Case("ensemble_score", seed, kw, names, dict(test_launch_items=cut), host,
                f"ensemble_score seed={seed} T={T} rows={rows} R={R} D={D} {src.dtype} Rt={truth.shape[2]} n_a={n_a} n_bins={n_bins} "
                f"k0={k0} k1={k1} fd={None if fd is None else fd.tolist()} pop={pop is not None} cut={cut} names={names}", f, flat="src:2-D" in f)


# ---- path_functionals ---------------------------------------------------------------------------------------------------
PATHFN_PATH = ("peak_value", "peak_day", "min_value", "min_day", "total")
PATHFN_THR = ("first_cross", "days_above", "longest_run")
PATHFN_REGION = ("n_paths", "peak_day_hist", "n_cross", "cross_day_hist")
PATHFN_NEED_THR = PATHFN_THR + ("n_cross", "cross_day_hist")
PATHFN_OUT = PATHFN_PATH + PATHFN_THR + ("n_valid",) + PATHFN_REGION
PATHFN_FEATURES = (_ENS_COMMON + _out_list(PATHFN_OUT) + ("window:whole", "window:part", "window:k0-inside-a-block",
                   "window:over-a-block-edge", "first_day:yes", "first_day:no", "n_thr:0", "n_thr:1-2", "n_thr:3-8", "thr:nan",
                   "segments:library", "segments:1", "segments:>1", "launches:1", "launches:>1"))
PF_BLOCK, PF_WG = 32, 256                                   # days of a block of the total; paths of a workgroup


def make_path_functionals(seed):
    """pathfn_check_desc / epi_pathfn_validate: T, R, D >= 1, rows 1 .. 4096, n_thr 0 .. 8 (the threshold outputs only with
    n_thr >= 1), 0 <= k0 < k1 <= T (no empty window), test_segments 0 .. min(ceil(W / 32), 1024), test_launch_groups >= 0.
    One example in three has T 33 .. 140 so that the window crosses 32-day block edges and can be cut into segments; its k0
    is mostly no multiple of 32."""
    rng, f = np.random.default_rng(seed), set()
    long_ = rng.random() < 0.34
    src, R, D, pop = _ens_source(rng, f, ENS_FUZZ_CAP, max_T=70)
    T, rows, _ = src.shape
    if long_ and "D:small" in f:                             # more days of the same kind: the restatement is vectorised over paths
        T2 = int(rng.integers(33, 141))
        reps = -(-T2 // T)
        src = np.ascontiguousarray(np.concatenate([src] * reps, axis=0)[:T2] * (1.0 + 0.01 * np.arange(T2))[:, None, None].astype(src.dtype))
        T = T2
    ro = rows + int(pop is not None)
    k0, k1 = _window(rng, f, T, False)
    W = k1 - k0
    if k0 % PF_BLOCK:
        f.add("window:k0-inside-a-block")
    if W > PF_BLOCK:
        f.add("window:over-a-block-edge")
    fd = _first_day(rng, f, R, T)
    n_thr = int(_pick(rng, (0, 0, 1, 2, 3, 8))) if rng.random() < 0.5 else int(rng.integers(0, 9))
    f.add("n_thr:0" if n_thr == 0 else ("n_thr:1-2" if n_thr <= 2 else "n_thr:3-8"))
    thr = None
    if n_thr:
        s = src.astype(np.float64)
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)      # a region without a finite value has no median: threshold 0
            base = np.nanmedian(np.where(np.isfinite(s), s, np.nan).reshape(T, rows, R, D), axis=(0, 3))      # [rows, R]
        base = np.where(np.isfinite(base), base, 0.0)
        if pop is not None:
            base = np.concatenate([base, np.zeros((1, R))], axis=0)
        thr = base[None] + rng.standard_normal((n_thr, ro, R)) * (np.abs(base[None]) + 1.0)
        if rng.random() < 0.3:
            thr[rng.random(thr.shape) < 0.2] = np.nan
            if np.isnan(thr).any():
                f.add("thr:nan")
    nb = -(-W // PF_BLOCK)
    seg = int(rng.integers(0, min(nb, 4) + 1))
    f.add("segments:library" if seg == 0 else ("segments:1" if seg == 1 else "segments:>1"))
    pg = -(-(R * D) // PF_WG)
    groups = int(rng.integers(1, 4)) if rng.random() < 0.5 else 0
    # a launch holds max(groups / (segments * row groups), 1) workgroups of the pg a row group has: more than one launch when that is < pg
    nseg = seg if seg else 1
    f.add("launches:>1" if groups and max(groups // nseg, 1) < pg else "launches:1")
    names = _subset(rng, [n for n in PATHFN_OUT if n_thr or n not in PATHFN_NEED_THR])
    _out_features(f, PATHFN_OUT, names)
    host = _host(rng, f)
    kw = dict(src=src, R=R, D=D, thr=thr, population=pop, first_day=fd, k0=k0, k1=k1)
    return Case("path_functionals", seed, kw, names, dict(test_segments=seg, test_launch_groups=groups), host,
                f"path_functionals seed={seed} T={T} rows={rows} R={R} D={D} {src.dtype} n_thr={n_thr} k0={k0} k1={k1} "
                f"fd={None if fd is None else fd.tolist()} pop={pop is not None} seg={seg} groups={groups} names={names}", f, flat="src:2-D" in f)


# ---- ensemble_joint_score -----------------------------------------------------------------------------------------------
EJOINT_OUT = ("es", "truth_term", "spread_term", "vs", "n_members", "n_days", "member_dist")
EJOINT_FEATURES = (_ENS_COMMON + _out_list(EJOINT_OUT) + ("truth_series:yes", "truth_series:no", "Rt!=R", "Rt==R", "window:whole",
                   "window:empty", "window:part", "first_day:yes", "first_day:no", "vs_p:None", "vs_p:0.5", "vs_p:1",
                   "max_lag:0", "max_lag:>0", "launches:1", "launches:>1", "tiles:1", "tiles:>1"))


def make_ensemble_joint_score(seed):
    """ejoint_check_desc / epi_ejoint_validate: T, rows, R, Rt >= 1, D 1 .. 4096, 0 <= k0 <= k1 <= T (the empty window
    included), vs_order 0 .. 2 (vs only with vs_order > 0), max_lag >= 0, test_launch_tiles >= 0 (here: below the number of
    tiles of all items, so a cut falls inside an item's tile row).  T is cut down so that rows' R W D max(1, D / 64) stays
    within EJOINT_FUZZ_CAP; at the 30 % setting the single NaN members lie on the middle day only (a NaN on any day removes its
    member from the item)."""
    rng, f = np.random.default_rng(seed), set()
    src, R, D, pop = _ens_source(rng, f, ENS_FUZZ_CAP, max_T=40)
    T, rows, _ = src.shape
    ro = rows + int(pop is not None)
    T2 = max(1, min(T, EJOINT_FUZZ_CAP // (ro * R * D * max(1, D // 64))))
    src = np.ascontiguousarray(src[:T2])
    T = T2
    # a NaN on any day of the window removes the member, so the 10 % of NaN per value of the 30 % setting would leave next to
    # none over many days: the NaN of every other day than the middle one become the tied value (the share of NaN per value stays
    # what it is on that day; the +-Inf and the whole item of NaN stay everywhere)
    if "nonfinite:0.3" in f and T > 1:
        other = np.arange(T) != T // 2
        whole = np.isnan(src).reshape(T, rows, R, D).all(axis=3, keepdims=True)
        part = (np.isnan(src).reshape(T, rows, R, D) & ~whole & other[:, None, None, None]).reshape(src.shape)
        src[part] = 1.25
    truth, ts = _truth(rng, f, src, R, D, pop)
    k0, k1 = _window(rng, f, T, True)
    fd = _first_day(rng, f, R, T)
    vs_p = _pick(rng, (None, 0.5, 1))
    f.add(f"vs_p:{vs_p}")
    max_lag = int(rng.integers(0, max(k1 - k0, 0) + 1))
    f.add("max_lag:0" if max_lag == 0 else "max_lag:>0")
    names = _subset(rng, [n for n in EJOINT_OUT if n != "vs" or vs_p is not None])
    _out_features(f, EJOINT_OUT, names)
    nb = -(-D // 64)
    tiles = nb * (nb + 1) // 2
    f.add("tiles:1" if tiles == 1 else "tiles:>1")
    units = ro * R * tiles
    cut = 0
    if units > 1 and rng.random() < 0.5:
        cut = int(rng.integers(1, units))
        if tiles > 1 and cut % tiles == 0:
            cut += 1
    f.add("launches:>1" if cut else "launches:1")
    host = _host(rng, f)
    kw = dict(src=src, truth=truth, R=R, D=D, vs_order={None: 0, 0.5: 1, 1: 2}[vs_p], max_lag=max_lag, population=pop, truth_series=ts,
              first_day=fd, k0=k0, k1=k1)
    return Case("ensemble_joint_score", seed, kw, names, dict(test_launch_tiles=cut), host,
                f"ensemble_joint_score seed={seed} T={T} rows={rows} R={R} D={D} {src.dtype} Rt={truth.shape[2]} vs_p={vs_p} "
                f"max_lag={max_lag} k0={k0} k1={k1} fd={None if fd is None else fd.tolist()} pop={pop is not None} cut={cut} names={names}", f, flat="src:2-D" in f)


# ======================================================================================================================
# the three regression calls on X [D, F, R] with a list of row counts: mldivide, svr, rate_map
# ======================================================================================================================
LDS_ELEMS = 20000                                           # max(n_rows) (F + 1) of mldivide, max(n_rows) ((F | 1) + 1) of svr
# K R min(D, F) (D + F), the reflector steps of one example times their length: keeps the NumPy reading of the backslash (a
# Python loop per column and row) under about 1.5 s an example; the C restatement then needs milliseconds
MLDIV_FUZZ_CAP = 150_000
# K R min(max_iter, 40 n): the pair steps an example can take; keeps the NumPy reading of the SMO loop under about 2 s
SVR_FUZZ_CAP = 40_000
# K R T F^2: the normal equations of an example; keeps the NumPy reading of the Cholesky loop under about a second
RATEMAP_FUZZ_CAP = 1_500_000


def _row_counts(rng, f, D, max_n=None):
    """1 .. 70 row counts, unsorted with repeats, 1 and D (or the largest count the call allows) among them where there are at
    least two; one list in five is longer than 64 (a second chunk of 64 counts)"""
    top = D if max_n is None else min(D, max_n)
    K = int(rng.integers(65, 71)) if rng.random() < 0.2 else int(rng.integers(1, 9))
    nr = rng.integers(1, top + 1, K)
    if K >= 2:
        i, j = rng.permutation(K)[:2]
        nr[i], nr[j] = 1, top
    if K >= 3:
        nr[int(rng.integers(K))] = nr[int(rng.integers(K))]
    f.add("row-counts:>64" if K > 64 else "row-counts:<=64")
    return tuple(int(v) for v in nr)


def _plans(rng, D, F, R):
    """piecewise-constant integer plans as columns, a target that follows them plus noise (tests/mldivide_ref.make_case)"""
    X = np.empty((D, F, R))
    lvl = rng.integers(0, 5, size=(F, R)).astype(np.float64)
    for t in range(D):
        sw = rng.random((F, R)) < 0.1
        lvl = np.where(sw, rng.integers(0, 5, size=(F, R)), lvl)
        X[t] = lvl
    w = rng.normal(0, 0.03, size=(F, R))
    y = 0.15 - np.einsum("tfr,fr->tr", X, np.abs(w)) + rng.normal(0, 0.05, size=(D, R))
    return X, y


def _plant_columns(rng, f, X, y):
    """a duplicated, a zero and a lagged-copy column and a non-finite row, each in a region of its own choice, each with
    probability 1 / 2; a column that is constant over the first rows only makes a matrix rank-deficient for some of its row
    counts and not for others"""
    D, F, R = X.shape
    if F >= 2 and rng.random() < 0.5:
        a, b = rng.permutation(F)[:2]
        r = int(rng.integers(R))
        X[:, b, r] = X[:, a, r]
        f.add("column:duplicate")
    if rng.random() < 0.5:
        X[:, int(rng.integers(F)), int(rng.integers(R))] = 0.0
        f.add("column:zero")
    if F >= 2 and D >= 3 and rng.random() < 0.5:
        a, b = rng.permutation(F)[:2]
        lag, r = int(rng.integers(1, min(D, 8))), int(rng.integers(R))
        X[lag:, b, r] = X[:D - lag, a, r]
        X[:lag, b, r] = 0.0
        f.add("column:lagged-copy")
    if D >= 4 and F >= 2 and rng.random() < 0.5:
        a, b = rng.permutation(F)[:2]
        h, r = int(rng.integers(2, D)), int(rng.integers(R))
        X[:h, b, r] = X[:h, a, r]                            # equal over the first h rows: deficient for n_rows <= h only
        f.add("column:equal-over-the-first-rows")
    if rng.random() < 0.4:
        t, r = int(rng.integers(D)), int(rng.integers(R))
        if rng.random() < 0.5:
            X[t, int(rng.integers(F)), r] = _pick(rng, (np.nan, np.inf))
        else:
            y[t, r] = _pick(rng, (np.nan, -np.inf))
        f.add("row:nonfinite")


_REG_COMMON = ("row-counts:>64", "row-counts:<=64", "column:duplicate", "column:zero", "column:lagged-copy",
               "column:equal-over-the-first-rows", "row:nonfinite", "host:yes", "host:no")

# ---- mldivide ------------------------------------------------------------------------------------------------------------
MLDIV_OUT = ("m", "rank", "perm", "rdiag", "resid", "fitted", "status")
MLDIV_FEATURES = (_REG_COMMON + _out_list(MLDIV_OUT) + ("tol_scale:0", "tol_scale:1", "tol_scale:1e+06", "F:1", "F:>64", "rows<cols",
                  "rows>=cols", "status:0", "status:RANK_DEFICIENT", "status:NONFINITE_INPUT", "status:NONFINITE"))


def _mldiv_status(want):
    st = np.asarray(want["status"])
    out = set()
    if (st == 0).any():
        out.add("status:0")
    for bit, name in ((1, "RANK_DEFICIENT"), (2, "NONFINITE_INPUT"), (4, "NONFINITE")):
        if (st & bit).any():
            out.add(f"status:{name}")
    return out


def _reg_sizes(rng, max_D=120):
    """F 1 .. 96 (one in four from 1, 2, 63 .. 65, 95, 96), D 1 .. max_D with D (F + 2) within the LDS limit, R 1 .. 6"""
    F = int(_pick(rng, (1, 2, 63, 64, 65, 95, 96))) if rng.random() < 0.25 else int(rng.integers(1, 97))
    D = int(rng.integers(1, min(max_D, LDS_ELEMS // (F + 2)) + 1))
    R = int(rng.integers(1, 7))
    return D, F, R


def make_mldivide(seed):
    """epi_mldiv_validate: D, R, K >= 1, F 1 .. 96, every n_rows in 1 .. D with max(n_rows) (F + 1) <= 20000, tol_scale finite
    and >= 0 (here 0, 1 or 1e6).  D 1 .. 120; the sizes are cut down (first R to 1, then the larger of D
    and F by a third at a time; the row counts follow D) until K R min(D, F) (D + F) <= MLDIV_FUZZ_CAP.  One example in eight holds a column of 1e200 t, whose sum
    of squares overflows (status NONFINITE)."""
    rng, f = np.random.default_rng(seed), set()
    D, F, R = _reg_sizes(rng)
    nr = _row_counts(rng, f, D)
    K = len(nr)
    while K * R * min(D, F) * (D + F) > MLDIV_FUZZ_CAP:
        if R > 1:
            R -= 1
        elif D >= F and D > 1:
            D = max(1, D * 2 // 3)
        else:
            F = max(1, F * 2 // 3)
    nr = tuple(min(n, D) for n in nr[:-1]) + (D,) if K >= 2 else (min(nr[0], D),)
    X, y = _plans(rng, D, F, R)
    _plant_columns(rng, f, X, y)
    if rng.random() < 0.125:
        X[:, int(rng.integers(F)), int(rng.integers(R))] = 1e200 * np.arange(1, D + 1)
    tol_scale = float(_pick(rng, (0.0, 1.0, 1e6)))
    f.add(f"tol_scale:{tol_scale:g}")
    if F == 1:
        f.add("F:1")
    if F > 64:
        f.add("F:>64")
    f.add("rows<cols" if min(nr) < F else "rows>=cols")
    if max(nr) >= F:
        f.add("rows>=cols")
    names = _subset(rng, MLDIV_OUT)
    _out_features(f, MLDIV_OUT, names)
    host = _host(rng, f)
    return Case("mldivide", seed, dict(X=X, y=y, n_rows=nr, tol_scale=tol_scale), names, {}, host,
                f"mldivide seed={seed} D={D} F={F} R={R} K={K} n_rows={nr[:8]}{'...' if K > 8 else ''} tol_scale={tol_scale:g} names={names}", f)


# ---- svr -----------------------------------------------------------------------------------------------------------------
SVR_OUT = ("beta", "bias", "w", "fitted", "n_iter", "gap", "n_sv", "status")
SVR_FEATURES = (_REG_COMMON + _out_list(SVR_OUT) + ("kernel:linear", "kernel:gaussian", "max_iter:3", "max_iter:200", "max_iter:20000",
                "box:scalar", "box:array", "epsilon:scalar", "epsilon:array", "kernel_scale:scalar", "kernel_scale:array",
                "region:bad-parameter", "status:0", "status:NOT_CONVERGED", "status:BAD_INPUT", "status:NONFINITE"))


def _svr_status(want):
    st = np.asarray(want["status"])
    out = set()
    if (st == 0).any():
        out.add("status:0")
    for bit, name in ((1, "NOT_CONVERGED"), (2, "BAD_INPUT"), (4, "NONFINITE")):
        if (st & bit).any():
            out.add(f"status:{name}")
    return out


def make_svr(seed):
    """epi_svr_validate: D, R, K >= 1, F 1 .. 96, both kernels (w with the linear one only), max_iter 1 .. 1e7 (here 3, 200 or
    20000), tol > 0 (1e-3), every n_rows in 1 .. min(D, 1024) with max(n_rows) ((F | 1) + 1) <= 20000.  box, epsilon and
    kernel_scale are scalars or [R] arrays; one region in ten of an array gets a value the call answers with BAD_INPUT (a
    box <= 0, a negative epsilon, a kernel_scale of 0).  D 1 .. 80; K and R are cut down until K R min(max_iter, 40 D) <=
    SVR_FUZZ_CAP."""
    rng, f = np.random.default_rng(seed), set()
    D, F, R = _reg_sizes(rng, max_D=80)
    nr = _row_counts(rng, f, D)
    max_iter = int(_pick(rng, (3, 200, 20000)))
    f.add(f"max_iter:{max_iter}")
    steps = min(max_iter, 40 * D)
    while len(nr) * R * steps > SVR_FUZZ_CAP and R > 1:
        R -= 1
    if len(nr) * steps > SVR_FUZZ_CAP:
        keep = max(1, SVR_FUZZ_CAP // steps)
        nr = nr[:keep - 1] + (D,) if keep >= 2 else (D,)
        f.discard("row-counts:>64")
        f.add("row-counts:<=64")
    kernel = _pick(rng, ("linear", "gaussian"))
    f.add(f"kernel:{kernel}")
    X, y = _plans(rng, D, F, R)
    X = X / 4.0
    _plant_columns(rng, f, X, y)
    sd = float(np.nanstd(np.where(np.isfinite(y), y, np.nan))) if np.isfinite(y).any() else 0.1
    sd = sd if np.isfinite(sd) and sd > 0 else 0.1
    par = {}
    for k, base in (("box", sd * 4.0 ** float(rng.integers(0, 3))), ("epsilon", sd / 10.0 * float(rng.integers(0, 3))),
                    ("kernel_scale", 1.0 + 0.5 * float(rng.integers(0, 4)))):
        if rng.random() < 0.5:
            par[k] = float(base)
            f.add(f"{k}:scalar")
        else:
            v = base * (1.0 + rng.integers(0, 3, R))
            bad = rng.random(R) < 0.1
            if bad.any():
                v[bad] = {"box": -1.0, "epsilon": -0.5, "kernel_scale": 0.0}[k]
                f.add("region:bad-parameter")
            par[k] = np.ascontiguousarray(v, dtype=np.float64)
            f.add(f"{k}:array")
    names = _subset(rng, [n for n in SVR_OUT if n != "w" or kernel == "linear"])
    _out_features(f, SVR_OUT, names)
    host = _host(rng, f)
    kw = dict(X=X, y=y, n_rows=nr, kernel=kernel, tol=1e-3, max_iter=max_iter, **par)
    return Case("svr", seed, kw, names, {}, host,
                f"svr seed={seed} D={D} F={F} R={R} K={len(nr)} n_rows={nr[:8]}{'...' if len(nr) > 8 else ''} {kernel} max_iter={max_iter} "
                f"box={par['box']} epsilon={par['epsilon']} kernel_scale={par['kernel_scale']} names={names}", f)


# ---- rate_map ------------------------------------------------------------------------------------------------------------
RATEMAP_OUT = ("map", "x_mx", "y_filled", "lambda_hat", "new_cases_est", "tracker", "status")
RATEMAP_FEATURES = (("row-counts:>64", "row-counts:<=64", "host:yes", "host:no") + _out_list(RATEMAP_OUT)
                    + ("n_lags:0", "n_lags:1", "n_lags:2", "n_lags:3", "E:0", "E:>0", "E:8", "fit:1", "fit:0", "ridge:0", "ridge:>0",
                       "effect_lag:0", "effect_lag:>0", "lag>=train-end", "plan:constant", "plan:zero", "plan:nan", "y:leading-nan",
                       "y:nonfinite-inside", "F:>64", "status:0", "status:LEADING_NAN", "status:NOT_PD", "status:NONFINITE"))


def _ratemap_status(want):
    st = np.asarray(want["status"])
    out = set()
    if (st == 0).any():
        out.add("status:0")
    for bit, name in ((1, "LEADING_NAN"), (2, "NOT_PD"), (4, "NONFINITE")):
        if (st & bit).any():
            out.add(f"status:{name}")
    return out


def make_rate_map(seed):
    """epi_ratemap_validate: T, n, R, K >= 1, n <= 24, n_lags 0 .. 3 with every lag in 1 .. T - 1, E 0 .. 8, F = n (1 + n_lags) +
    E <= 96, fit 0 (lambda_in given; no map) or 1 (y given), ridge finite and >= 0, effect_lag >= 0, every n_train in 1 .. T;
    y_filled needs y.  T 2 .. 60, R 1 .. 6; K and R are cut down until K R T F^2 <= RATEMAP_FUZZ_CAP."""
    rng, f = np.random.default_rng(seed), set()
    T = int(rng.integers(2, 61))
    n_lags = int(rng.integers(0, min(3, T - 1) + 1))
    lags = tuple(sorted(int(v) for v in rng.permutation(np.arange(1, T))[:n_lags]))
    if n_lags and rng.random() < 0.5:
        lags = tuple(sorted(int(v) for v in rng.permutation(np.arange(1, min(T, 9)))[:n_lags]))
        n_lags = len(lags)
    f.add(f"n_lags:{n_lags}")
    E = 0 if rng.random() < 0.4 else int(rng.integers(1, 9))
    f.add("E:0" if E == 0 else "E:>0")
    if E == 8:
        f.add("E:8")
    n = int(rng.integers(1, min(24, (96 - E) // (1 + n_lags)) + 1))
    F = n * (1 + n_lags) + E
    if F > 64:
        f.add("F:>64")
    R = int(rng.integers(1, 7))
    nt = _row_counts(rng, f, T)
    while len(nt) * R * T * F * F > RATEMAP_FUZZ_CAP and R > 1:
        R -= 1
    if len(nt) * T * F * F > RATEMAP_FUZZ_CAP:
        keep = max(1, RATEMAP_FUZZ_CAP // (T * F * F))
        nt = nt[:keep - 1] + (T,) if keep >= 2 else (T,)
        f.discard("row-counts:>64")
        f.add("row-counts:<=64")
    K = len(nt)
    if lags and max(lags) >= min(nt):
        f.add("lag>=train-end")
    fit = int(rng.random() < 0.7)
    f.add(f"fit:{fit}")
    ip, y = _plans(rng, T, n, R)
    ns = 50.0 + 500.0 * rng.random((T, R))
    extra = None
    if E:
        extra = rng.normal(0, 1, size=(T, E, R))
        extra[:, 0, :] = 1.0
    if rng.random() < 0.4:
        ip[:, int(rng.integers(n)), int(rng.integers(R))] = 2.0
        f.add("plan:constant")
    if rng.random() < 0.4:
        ip[:, int(rng.integers(n)), int(rng.integers(R))] = 0.0
        f.add("plan:zero")
    if rng.random() < 0.2:
        ip[int(rng.integers(T)), int(rng.integers(n)), int(rng.integers(R))] = np.nan
        f.add("plan:nan")
    if rng.random() < 0.3:
        y[0, int(rng.integers(R))] = np.nan
        f.add("y:leading-nan")
    if T > 3 and rng.random() < 0.4:
        r = int(rng.integers(R))
        y[int(rng.integers(1, T)), r] = np.nan
        y[int(rng.integers(1, T)), r] = np.inf
        f.add("y:nonfinite-inside")
    lam = None
    if not fit:
        lam = 0.12 * rng.normal(0, 1, size=(K, T, R))
        if rng.random() < 0.3:
            lam[:, int(rng.integers(T)), int(rng.integers(R))] = np.nan
    ridge = 0.0 if rng.random() < 0.3 else float(_pick(rng, (1e-6, 1e-3, 1.0)))
    f.add("ridge:0" if ridge == 0 else "ridge:>0")
    effect_lag = int(rng.integers(0, 6))
    f.add("effect_lag:0" if effect_lag == 0 else "effect_lag:>0")
    have_y = fit or rng.random() < 0.5
    p = dict(ip=ip, y=y if have_y else None, new_smoothed=ns, extra=extra, lambda_in=lam, n_train=nt, lags=lags, fit=fit,
             effect_lag=effect_lag, ridge=ridge, thr=0.1, red=0.01)
    names = _subset(rng, [k for k in RATEMAP_OUT if (fit or k != "map") and (have_y or k != "y_filled")])
    _out_features(f, RATEMAP_OUT, names)
    host = _host(rng, f)
    return Case("rate_map", seed, dict(p=p), names, {}, host,
                f"rate_map seed={seed} T={T} n={n} lags={lags} E={E} R={R} K={K} n_train={nt[:8]}{'...' if K > 8 else ''} fit={fit} "
                f"ridge={ridge:g} effect_lag={effect_lag} y={have_y} names={names}", f)


# ======================================================================================================================
# robust_affine_fit, npi_plan, ar_forecast
# ======================================================================================================================
# R D n, the elements of X: keeps the NumPy reading of one example (a Python loop per item, up to max_iter passes of whole-array
# operations) under about 0.5 s
ROBFIT_FUZZ_CAP = 40_000
ROBFIT_EDGE_D = (3, 4, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)
ROBFIT_OUT = ("a", "b_item", "sigma", "iters", "status", "weights", "b")
ROBFIT_FEATURES = (_out_list(ROBFIT_OUT) + tuple(f"D:nv={v}" for v in (1, 2, 4, 8, 16)) + ("robust:0", "robust:1", "max_iter:1", "max_iter:3",
                   "max_iter:50", "bounds:none", "bounds:lower-0", "bounds:equal", "bounds:box", "column:constant", "outliers:gross",
                   "item:nonfinite", "line:exact", "host:yes", "host:no", "status:0", "status:NONFINITE", "status:CONST", "status:SLOPE_LOST",
                   "status:MAXITER", "status:BOUND"))


def _robfit_status(want):
    st = np.asarray(want["status"])
    out = {"status:0"} if (st == 0).any() else set()
    for bit, name in ((1, "NONFINITE"), (2, "CONST"), (4, "SLOPE_LOST"), (8, "MAXITER"), (16, "BOUND")):
        if (st & bit).any():
            out.add(f"status:{name}")
    return out


def make_robust_affine_fit(seed):
    """epi_robfit_validate: D 3 .. 1024 (half of the examples from ROBFIT_EDGE_D, both sides of every edge of the dispatch by D),
    n 1 .. 12, R 1 .. 70 cut down to R D n <= ROBFIT_FUZZ_CAP, robust 0 / 1, max_iter 1 .. 100000 (here 1, 3 or 50), lower_a <=
    upper_a and neither NaN (none, [0, Inf), an interval, equal bounds).  Levels 0 .. 4 that switch now and then, y on one of
    the columns; constant columns, gross outliers, exact lines, a non-finite item and, for D <= 6, a single day that carries
    the whole slope (its weight can vanish: SLOPE_LOST)."""
    rng, f = np.random.default_rng(seed), set()
    D = int(_pick(rng, ROBFIT_EDGE_D)) if rng.random() < 0.5 else (int(rng.integers(3, 8)) if rng.random() < 0.3 else int(rng.integers(3, 1025)))
    n = int(rng.integers(1, 13))
    n = max(1, min(n, ROBFIT_FUZZ_CAP // D))
    R = max(1, min(int(rng.integers(1, 71)), ROBFIT_FUZZ_CAP // (D * n)))
    f.add(f"D:nv={max(64, 1 << (D - 1).bit_length()) // 64}")
    X = np.empty((D, n, R))
    lvl = rng.integers(0, 5, size=(n, R))
    for d in range(D):
        sw = rng.random((n, R)) < 0.08
        lvl = np.where(sw, rng.integers(0, 5, size=(n, R)), lvl)
        X[d] = lvl
    days = np.arange(D, dtype=np.float64)
    slope = rng.choice((-0.02, 0.0, 0.03, 0.1), R)
    own = rng.integers(0, n, R)
    y = 0.2 + slope[None] * X[:, own, np.arange(R)] + 0.01 * rng.standard_normal((D, R)) + 0.001 * days[:, None]
    for r in range(R):
        u = rng.random()
        if u < 0.15:
            X[:, int(rng.integers(n)), r] = float(rng.integers(0, 4))
            f.add("column:constant")
        elif u < 0.3:
            at = rng.choice(D, size=max(1, D // 10), replace=False)
            y[at, r] += _pick(rng, (0.5, 100.0)) * rng.choice((-1.0, 1.0), size=at.size)
            f.add("outliers:gross")
        elif u < 0.4:
            y[:, r] = 0.25 + 0.5 * X[:, int(own[r]), r]
            f.add("line:exact")
        elif u < 0.45:
            if rng.random() < 0.5:
                X[int(rng.integers(D)), int(rng.integers(n)), r] = _pick(rng, (np.nan, np.inf))
            else:
                y[int(rng.integers(D)), r] = np.nan
            f.add("item:nonfinite")
        elif u < 0.6 and D <= 6:
            k = int(rng.integers(n))
            X[:, k, r] = 0.0
            X[D - 1, k, r] = 1.0
            y[:, r] = 0.001 * np.cos(2.0 * days)
            y[D - 1, r] = -10.0
    robust = int(rng.random() < 0.7)
    f.add(f"robust:{robust}")
    max_iter = int(_pick(rng, (1, 3, 50)))
    f.add(f"max_iter:{max_iter}")
    kind = _pick(rng, ("none", "lower-0", "lower-0", "equal", "box"))
    lower, upper = {"none": (-np.inf, np.inf), "lower-0": (0.0, np.inf), "equal": (0.02, 0.02), "box": (-0.01, 0.05)}[kind]
    f.add(f"bounds:{kind}")
    names = _subset(rng, ROBFIT_OUT)
    _out_features(f, ROBFIT_OUT, names)
    host = _host(rng, f)
    kw = dict(X=X, y=y, robust=robust, lower=lower, upper=upper, max_iter=max_iter)
    return Case("robust_affine_fit", seed, kw, names, {}, host,
                f"robust_affine_fit seed={seed} D={D} n={n} R={R} robust={robust} max_iter={max_iter} bounds=({lower}, {upper}) names={names}", f)


# ---- npi_plan ------------------------------------------------------------------------------------------------------------
# R P H n max_iter (max_halvings + 2) / 8, the forward passes of an example times their length: keeps the NumPy reading (a Python
# loop per day of every pass) under about 2 s an example; the examples that stop early cost far less
PLAN_FUZZ_CAP = 60_000
PLAN_P = (1, 2, 3, 63, 64, 65, 255, 256, 257)
PLAN_OUT = ("plan", "J0", "J1", "F", "gap", "iters", "halvings", "status", "states", "mu", "F_trace")
PLAN_CORE, PLAN_OPTIONAL = PLAN_OUT[:8], PLAN_OUT[8:]           # the entries refuse a call without every core output
PLAN_FEATURES = (_out_list(PLAN_OPTIONAL) + ("P:1-3", "P:63-65", "P:255-257", "u_fixed:yes", "u_fixed:no", "u_init:yes", "u_init:no", "prefix:yes",
                 "prefix:no", "max_iter:1", "max_iter:8", "max_iter:64", "max_halvings:0", "max_halvings:3", "max_halvings:30", "tol:0",
                 "tol:1e-09", "tol:0.001", "host:yes", "host:no", "status:0", "status:MAXITER", "status:NO_DESCENT", "status:NONFINITE"))
PLAN_IP_MAXES = (3.0, 3.0, 2.0, 4.0, 2.0, 3.0, 2.0, 4.0, 2.0, 3.0, 2.0, 4.0)


def _plan_status(want):
    st = np.asarray(want["status"])
    out = {"status:0"} if (st == 0).any() else set()
    for bit, name in ((1, "MAXITER"), (2, "NO_DESCENT"), (4, "NONFINITE")):
        if (st & bit).any():
            out.add(f"status:{name}")
    return out


def make_npi_plan(seed):
    """epi_plan_validate: R, P, H >= 1, n_npi 1 .. 12, prefix_days >= 0, max_iter 1 .. 255 (here 1, 8 or 64), max_halvings 0 .. 30
    (0, 3 or 30), tol finite and >= 0 (0, 1e-9 or 1e-3).  R 1 .. 5, P from PLAN_P (both sides of the wavefront and of four
    wavefronts), H 1 .. 40, cut down (first R, then H, then P to its group's smallest) until R P H n max_iter (max_halvings +
    2) / 8 <= PLAN_FUZZ_CAP.  Cost weights eps over (0, 1) dense near 0; held entries u_fixed, a starting plan u_init and a
    prefix, each in half of the examples; one region in twelve has a cost weight of NaN or Inf (status NONFINITE)."""
    from tests import npi_plan_ref as PR
    rng, f = np.random.default_rng(seed), set()
    R, P, H, n = int(rng.integers(1, 6)), int(_pick(rng, PLAN_P)), int(rng.integers(1, 41)), int(rng.integers(1, 13))
    max_iter, max_halvings, tol = int(_pick(rng, (1, 8, 64))), int(_pick(rng, (0, 3, 30))), float(_pick(rng, (0.0, 1e-9, 1e-3)))
    cost = lambda: R * P * H * n * max_iter * (max_halvings + 2) // 8
    while cost() > PLAN_FUZZ_CAP:
        if R > 1:
            R -= 1
        elif H > 2:
            H = H // 2
        elif P > 3:
            P = {0: 1, 1: 63, 2: 255}[PLAN_P.index(P) // 3] if P not in (1, 63, 255) else (1 if P == 63 else 63)
        else:
            n = max(1, n // 2)
            if n == 1:
                break
    f.add("P:1-3" if P <= 3 else ("P:63-65" if P <= 65 else "P:255-257"))
    f.update({f"max_iter:{max_iter}", f"max_halvings:{max_halvings}", f"tol:{tol:g}"})
    a = np.abs(rng.normal(0.0, 0.02, (n, R)))
    b = rng.uniform(0.0, 0.05, R)
    w = rng.uniform(0.5, 2.0, (n, R)) if rng.random() < 0.5 else None
    sp = PR.scoring_block(a, b, weights=w, u_max=PLAN_IP_MAXES[:n])
    sp[0] = 1.0 - 10.0 ** rng.uniform(-4, -1.5, R)
    sp[1] = 1.0 - sp[0]
    sp[2] = rng.uniform(0.05, 0.6, R)
    if rng.random() < 1.0 / 12.0 * R:                          # a cost weight that is no number: F is not finite from the first pass on
        sp[PR.ROW_W + int(rng.integers(n)), int(rng.integers(R))] = _pick(rng, (np.nan, np.inf))
    u_min = np.minimum(np.floor(rng.random((n, R)) * 2), np.asarray(PLAN_IP_MAXES[:n])[:, None]) if rng.random() < 0.5 else np.zeros((n, R))
    eps = np.clip(np.sort(rng.random(P)) ** 4, 1e-12, 1.0 - 1e-12)
    case = dict(R=R, P=P, H=H, n=n, sp=sp, u_min=u_min, eps=eps, prefix_days=0, max_iter=max_iter, max_halvings=max_halvings, tol=tol)
    if rng.random() < 0.5:
        uf = np.full((H, n, R), np.nan)
        hold = rng.random(uf.shape) < 0.3
        uf[hold] = np.floor(rng.random(int(hold.sum())) * 3)
        case["u_fixed"] = uf
    f.add("u_fixed:yes" if "u_fixed" in case else "u_fixed:no")
    if rng.random() < 0.5:
        case["u_init"] = rng.integers(0, 3, (H, n, R * P)).astype(np.float64)
    f.add("u_init:yes" if "u_init" in case else "u_init:no")
    if rng.random() < 0.5:
        case.update(J0_prefix=rng.random(R) * 1e-3, J1_prefix=rng.random(R) * 100.0, prefix_days=int(rng.integers(1, 60)))
    f.add("prefix:yes" if case["prefix_days"] else "prefix:no")
    names = PLAN_CORE + tuple(k for k in PLAN_OPTIONAL if rng.random() < 0.5)
    _out_features(f, PLAN_OPTIONAL, names)
    host = _host(rng, f)
    return Case("npi_plan", seed, dict(case=case), names, {}, host,
                f"npi_plan seed={seed} R={R} P={P} H={H} n={n} max_iter={max_iter} max_halvings={max_halvings} tol={tol:g} "
                f"u_fixed={'u_fixed' in case} u_init={'u_init' in case} prefix={case['prefix_days']} names={names}", f)


# ---- ar_forecast ---------------------------------------------------------------------------------------------------------
# R D (L + H): the simulated chain-days of an example; the C restatement needs microseconds for each, the cap keeps the arrays small
ARFC_FUZZ_CAP = 200_000
ARFC_FEATURES = ("B:<=64", "B:65-256", "B:>256", "rows:<=64", "rows:65-128", "rows:>128", "model:fit", "model:given", "nv_mode:0", "nv_mode:1",
                 "drive:none", "drive:series", "drive:chain", "z:yes", "z:no", "z:seeded", "region:constant", "region:nan", "p:1", "p:24", "host:yes",
                 "host:no", "status:OK", "status:RANK_DEFICIENT", "status:BAD_INPUT")


def _arfc_status(want):
    st = np.asarray(want["status"])
    return {f"status:{n}" for v, n in ((0, "OK"), (1, "RANK_DEFICIENT"), (2, "BAD_INPUT")) if (st == v).any()}


def _ar_series(rng, coefs, L, noise, offset, burn=200):
    """a stable autoregression around `offset` (tests/ar_forecast_ref.ar_series, on the example's own generator)"""
    p = len(coefs)
    x = np.zeros(burn + L + p)
    e = rng.standard_normal(burn + L + p) * noise
    for t in range(p, len(x)):
        x[t] = e[t] - sum(coefs[k] * x[t - 1 - k] for k in range(p))
    return x[-L:] + offset


def make_ar_forecast(seed):
    """epi_arfc_validate: R, D, H >= 1, p 1 .. 32 (here 1 .. 24), p + 1 <= L, L - p <= 256, 2 (L - p) >= p + 1, fit 0 (A and
    noise_var given) or 1, nv_mode 0 / 1, a drive [H, Sd] per chain (Sd = R D) or through drive_series.  The stacked rows M = 2
    (L - p) lie around 64 and 128 in half of the examples (62 .. 66, 126 .. 130), else anywhere up to 200; R D lies around 64
    and 256 in half of them (R 1 .. 6, D from the quotient), else R 1 .. 6 and D 1 .. 70; horizon 1 .. 40.  One region in six is
    constant (RANK_DEFICIENT) or holds a NaN (BAD_INPUT) among healthy ones."""
    rng, f = np.random.default_rng(seed), set()
    p = int(_pick(rng, (1, 24))) if rng.random() < 0.2 else int(rng.integers(1, 25))
    if p in (1, 24):
        f.add(f"p:{p}")
    if rng.random() < 0.5:
        M = int(_pick(rng, (62, 64, 66, 126, 128, 130)))
    else:
        M = 2 * int(rng.integers((p + 2) // 2, 101))
    M = max(M, p + 1 + ((p + 1) % 2))
    L = M // 2 + p
    f.add("rows:<=64" if M <= 64 else ("rows:65-128" if M <= 128 else "rows:>128"))
    R = int(rng.integers(1, 7))
    if rng.random() < 0.5:
        D = max(1, int(_pick(rng, (63, 64, 65, 255, 256, 257))) // R + int(rng.integers(0, 2)))
    else:
        D = int(rng.integers(1, 71))
    H = int(rng.integers(1, 41))
    D = max(1, min(D, ARFC_FUZZ_CAP // (R * (L + H))))
    B = R * D
    f.add("B:<=64" if B <= 64 else ("B:65-256" if B <= 256 else "B:>256"))
    seg = np.stack([_ar_series(rng, [-1.2, 0.5], L, float(_pick(rng, (0.05, 1.0))), 0.3) for _ in range(R)], axis=1)
    for r in range(R):
        u = rng.random()
        if u < 1.0 / 12.0:
            seg[:, r] = 0.25
            f.add("region:constant")
        elif u < 1.0 / 6.0:
            seg[int(rng.integers(L)), r] = np.nan
            f.add("region:nan")
    s0 = rng.uniform(0.9, 0.999, R)
    kw = dict(seg=seg, beta=rng.uniform(0.1, 0.3, R), s0=s0, i0=1.0 - s0, dt=float(_pick(rng, (1.0, 0.5))), p=p, H=H, D=D)
    kw["z"] = rng.standard_normal((H, B)) if rng.random() < 0.7 else None
    f.add("z:yes" if kw["z"] is not None else "z:no")
    drive = _pick(rng, ("none", "series", "chain"))
    f.add(f"drive:{drive}")
    kw["drive"] = kw["drive_series"] = None
    if drive == "series":
        Sd = int(rng.integers(1, R + 3))
        kw["drive"] = rng.uniform(-0.2, 0.2, (H, Sd))
        kw["drive_series"] = rng.integers(0, Sd, B).astype(np.int32)
    elif drive == "chain":
        kw["drive"] = rng.uniform(-0.2, 0.2, (H, B))
    kw["A"] = kw["noise_var"] = None
    if rng.random() < 0.3:
        A = np.zeros((p, R))
        A[0] = -rng.uniform(0.2, 0.9, R)
        if p > 1:
            A[1:] = rng.normal(0, 0.02, (p - 1, R))
        kw["A"], kw["noise_var"] = A, rng.uniform(0.0, 0.01, R)
        f.add("model:given")
    else:
        f.add("model:fit")
    kw["nv_mode"] = int(rng.integers(0, 2))
    f.add(f"nv_mode:{kw['nv_mode']}")
    host = _host(rng, f)
    return Case("ar_forecast", seed, kw, ("S", "A", "noise_var", "status"), {}, host,
                f"ar_forecast seed={seed} R={R} D={D} L={L} p={p} M={M} H={H} dt={kw['dt']} z={kw['z'] is not None} drive={drive} "
                f"given={kw['A'] is not None} nv_mode={kw['nv_mode']}", f)


# ======================================================================================================================
# the three calls on a runner's arrays: smoother_draws, innovation_likelihood, two_filter
# ======================================================================================================================
BLOCKS = (3, 8, 40)


def _layout(rng, f, B):
    """classic, or chain-blocked with lane_block 3, 8 or 40 where B holds a block (lane_block <= B); a B that is no multiple of
    the block leaves a ragged last block"""
    blk = int(_pick(rng, (0, 0) + tuple(b for b in BLOCKS if b <= B)))       # classic twice as often as each block that fits
    f.add("layout:classic" if blk == 0 else f"layout:blocked-{blk}")
    if blk and B % blk:
        f.add("layout:ragged-last-block")
    return blk


def _storage(rng, f):
    st = _pick(rng, ("f64", "f32"))
    f.add(f"storage:{st}")
    return st


# ---- smoother_draws ------------------------------------------------------------------------------------------------------
# B T D, the path-days of an example: keeps the NumPy reading (a Python loop per chain and day, whole-array over the draws) under
# about half a second an example
SDRAW_FUZZ_CAP = 120_000
SDRAW_D = (1, 2, 3, 63, 64, 65, 66, 70)
SDRAW_WG = 256                                              # lanes of a workgroup of either grid
SDRAW_KINDS = ("cfg3", "adaptive", "total", "tail")
SDRAW_FEATURES = (tuple(f"workload:{k}" for k in SDRAW_KINDS) + ("layout:classic", "layout:blocked-3", "layout:blocked-8", "layout:blocked-40",
                  "layout:ragged-last-block", "storage:f64", "storage:f32", "planted:yes", "planted:no", "D:<64", "D:64", "D:>64", "k0:0",
                  "k0:>0", "k0:T-1", "clamp:0", "clamp:1", "z:none", "z:f64", "z:f32", "z:seeded", "out_f32:0", "out_f32:1", "s_term:yes", "s_term:no",
                  "P_term:yes", "P_term:no", "launch-groups:library", "launch-groups:1-3", "launches:1", "launches:gain>1", "launches:paths>1", "host:yes", "host:no", "status:0",
                  "status:NONFINITE", "status:RANK_DEFICIENT"))


def _sdraw_status(want):
    st = np.asarray(want["status"])
    out = {"status:0"} if (st == 0).any() else set()
    for bit, name in ((1, "NONFINITE"), (2, "RANK_DEFICIENT")):
        if (st & bit).any():
            out.add(f"status:{name}")
    return out


def make_smoother_draws(seed):
    """epi_sdraw_validate: the 3-state forward model, B, T, D >= 1, k0 0 .. T - 1, clamp / storage / z_f32 / out_f32 0 or 1,
    lane_block 0 .. B, test_launch_groups >= 0.  The arrays are the oracle's run of a synth.make_cfg3(B, T) workload (B, T 1 ..
    70, cut down to B T D <= SDRAW_FUZZ_CAP) with an R_v series, an adapted scalar R_v, TOTALCASES or a forecast tail without
    observations; half of the examples carry planted days (an Inf in P-, a NaN, a zero and a rank-1 P+)."""
    import copy
    from epidemicmodeling_amd import layout as L, synth
    from tests import helpers as H
    from tests import sdraw_ref as SR
    rng, f = np.random.default_rng(seed), set()
    D = int(_pick(rng, SDRAW_D))
    f.add("D:<64" if D < 64 else ("D:64" if D == 64 else "D:>64"))
    B, T = int(rng.integers(1, 71)), int(rng.integers(1, 71))
    while B * T * D > SDRAW_FUZZ_CAP:
        if B >= T:
            B = max(1, B * 2 // 3)
        else:
            T = max(1, T * 2 // 3)
    kind = _pick(rng, SDRAW_KINDS)
    f.add(f"workload:{kind}")
    w = copy.copy(synth.make_cfg3(B, T))
    if kind == "adaptive":
        w.prm = w.prm.copy()
        w.prm[L.PRM_BETA_EKF] = 0.9
        w.R_scalar = np.ascontiguousarray(np.nanmean(w.R_series, axis=0))
        w.R_series = None
    elif kind == "total":
        w.obs_type = "TOTALCASES"
        w.x = np.cumsum(w.x, axis=0)
    elif kind == "tail":
        w.x = w.x.copy()
        w.x[T - T // 3:] = np.nan
    case = SR.case_of(w, H.oracle_batch(w))
    planted = rng.random() < 0.5
    f.add("planted:yes" if planted else "planted:no")
    if planted:
        for k in SR.BIG:
            case[k] = case[k].copy()
        at = lambda: (int(rng.integers(T)), int(rng.integers(B)))
        t, c = at()
        case["P_MINUS"][t, 5, c] = np.inf
        t, c = at()
        case["P_PLUS"][t, 0, c] = np.nan
        t, c = at()
        case["P_PLUS"][t, :, c] = 0.0
        t, c = at()
        v = np.array([1e-3, -2e-3, 5e-4])
        case["P_PLUS"][t, :, c] = np.outer(v, v).ravel(order="F")
    u = rng.random()
    k0 = 0 if u < 0.3 else (T - 1 if u < 0.4 else int(rng.integers(0, T)))
    f.add("k0:0" if k0 == 0 else "k0:>0")
    if k0 == T - 1:
        f.add("k0:T-1")
    clamp = bool(rng.random() < 0.5)
    f.add(f"clamp:{int(clamp)}")
    zk = _pick(rng, ("none", "f64", "f32"))
    f.add(f"z:{zk}")
    z = None if zk == "none" else rng.standard_normal((T - k0, 3, B * D)).astype(np.float32 if zk == "f32" else np.float64)
    out_f32 = bool(rng.random() < 0.5)
    f.add(f"out_f32:{int(out_f32)}")
    s_term = case["S_PLUS"][T - 1] * (1.0 + 0.01 * rng.standard_normal((3, B))) if rng.random() < 0.5 else None
    P_term = case["P_PLUS"][T - 1] * 0.5 if rng.random() < 0.5 else None
    f.add("s_term:yes" if s_term is not None else "s_term:no")
    f.add("P_term:yes" if P_term is not None else "P_term:no")
    blk, storage = _layout(rng, f, B), _storage(rng, f)
    groups = int(rng.integers(1, 4)) if rng.random() < 0.5 else 0
    f.add("launch-groups:1-3" if groups else "launch-groups:library")
    # the gain grid has ceil(B / 256) T workgroups, the path grid ceil(B D / 256); each goes out in launches of `groups` of them
    gain, paths = -(-B // SDRAW_WG) * T, -(-(B * D) // SDRAW_WG)
    if groups and gain > groups:
        f.add("launches:gain>1")
    if groups and paths > groups:
        f.add("launches:paths>1")
    if not groups or (gain <= groups and paths <= groups):
        f.add("launches:1")
    host = _host(rng, f)
    kw = dict(case=case, D=D, z=z, s_term=s_term, P_term=P_term, k0=k0, clamp=clamp, storage=storage, out_f32=out_f32)
    return Case("smoother_draws", seed, kw, ("X", "rank", "status", "J", "L"), dict(blk=blk, groups=groups), host,
                f"smoother_draws seed={seed} {kind} B={B} T={T} D={D} k0={k0} clamp={clamp} z={zk} out_f32={out_f32} s_term={s_term is not None} "
                f"P_term={P_term is not None} blk={blk} {storage} groups={groups} planted={planted}", f)


# ---- innovation_likelihood -------------------------------------------------------------------------------------------------
# B T: the chain-days of an example; keeps the oracle's run and the NumPy reading (a Python loop per chain and day) under about
# 0.1 s an example
LOGLIK_FUZZ_CAP = 4_000
LOGLIK_KINDS = ("cfg3", "cfg4", "row3", "row4", "row4_codegen", "cfg3_bwd", "cfg4_bwd")
LOGLIK_OUT = ("loglik", "nis_mean", "n_valid", "status", "S", "nis", "R_used", "best", "best_loglik")
LOGLIK_FEATURES = (tuple(f"model:{k}" for k in LOGLIK_KINDS) + _out_list(LOGLIK_OUT) + ("layout:classic", "layout:blocked-3", "layout:blocked-8",
                   "layout:blocked-40", "layout:ragged-last-block", "storage:f64", "storage:f32", "R:series", "R:scalar-adapted", "obs:NEWCASES",
                   "obs:TOTALCASES", "x_series:yes", "x_series:no", "missing:0", "missing:0.05", "missing:0.3", "bad-days:yes", "bad-days:no",
                   "window:whole", "window:part", "window:k0-inside-a-block", "window:k1-inside-a-block", "G:0", "G:>0", "G:ties", "host:yes",
                   "host:no", "status:0", "status:BAD_DAY", "status:F32_REPLAY"))


def _loglik_status(want):
    st = np.asarray(want["status"])
    out = {"status:0"} if (st == 0).any() else set()
    for bit, name in ((1, "BAD_DAY"), (4, "F32_REPLAY")):
        if (st & bit).any():
            out.add(f"status:{name}")
    return out


def make_innovation_likelihood(seed):
    """epi_loglik_validate: any model, B, T, L, Sx >= 1, r_mode 0 (R_scalar, adapted over L <= 64 days) or 1 (R_series), 0 <= k0
    < k1 <= T, G 0 or a divisor of B, lane_block 0 .. B, storage 0 / 1, Sx = B without x_series.  Every model of
    tests/loglik_ref.WORKLOADS at B, T <= 70 (B T <= LOGLIK_FUZZ_CAP), through the oracle; the generic models with an R_v series
    or its mean as an adapted scalar (L 1 .. 30), both observation types, observations missing at 0 %, 5 % or 30 %; a window
    whose ends are mostly no multiples of 32; with G > 0 a chain copied onto another of its group in half of the examples (a
    tie of the selection); a NaN and a negative-definite P- planted in half of them."""
    from epidemicmodeling_amd import layout as L, synth
    from tests import helpers as H
    from tests import loglik_ref as LR
    rng, f = np.random.default_rng(seed), set()
    kind = _pick(rng, LOGLIK_KINDS)
    f.add(f"model:{kind}")
    R, E = int(rng.integers(1, 6)), int(rng.integers(1, 15))
    T = int(rng.integers(3, 71))
    while R * E * T > LOGLIK_FUZZ_CAP:
        if E > 1:
            E -= 1
        else:
            R -= 1
    hor = int(rng.integers(0, max(T // 3, 1)))
    if kind in ("cfg3", "cfg3_bwd"):
        w = synth.make_cfg3(R * E, T)
    elif kind in ("cfg4", "cfg4_bwd"):
        w = synth.make_cfg4(R, E, max(T - hor, 2), 0 if kind == "cfg4_bwd" else hor)
    elif kind == "row3":
        w = synth.make_row3(R, E, max(T - hor, 2), hor)
    else:
        w = synth.make_row4(R, T, min(hor, T - 1), codegen=(kind == "row4_codegen"))
    if kind.endswith("_bwd"):
        w = synth.as_backward(w)
    generic = not w.model.startswith("NewCase")
    w.L = int(rng.integers(1, 31))
    w.prm = w.prm.copy()
    w.prm[L.PRM_BETA_EKF] = float(_pick(rng, (1.0, 0.9, 0.5)))
    w.prm[L.PRM_GAMMA_EKF] = float(_pick(rng, (1.0, 0.995, 0.9)))
    if generic and w.R_series is not None and rng.random() < 0.5:
        col = np.nanmean(w.R_series, axis=0) + 1e-14
        w.R_scalar = np.ascontiguousarray(col if w.x_series is None else col[w.x_series])
        w.R_series = None
    f.add("R:series" if w.R_series is not None else "R:scalar-adapted")
    if generic and rng.random() < 0.5:
        w.obs_type = "TOTALCASES"
    f.add(f"obs:{w.obs_type}")
    f.add("x_series:yes" if w.x_series is not None else "x_series:no")
    miss = float(_pick(rng, (0.0, 0.05, 0.3)))
    f.add(f"missing:{miss:g}")
    if miss:
        w.x = w.x.copy()
        w.x[rng.random(w.x.shape) < miss] = np.nan
    B, T = w.B, w.T
    case = LR.case_of(w, H.oracle_batch(w))
    divs = [g for g in range(2, B + 1) if B % g == 0]
    G = int(_pick(rng, divs)) if divs and rng.random() < 0.5 else 0
    f.add("G:>0" if G else "G:0")
    if G and rng.random() < 0.5:                             # a tie: chain b becomes a copy of chain a of its group
        g0 = int(rng.integers(B // G)) * G
        a, b = (int(v) + g0 for v in rng.permutation(G)[:2])
        for k, v in list(case.items()):
            if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[-1] == B and k != "x_series" and not (k in ("x", "R_series") and case["x_series"] is not None):
                v = v.copy()
                v[..., b] = v[..., a]
                case[k] = v
        if case["x_series"] is not None:
            xs = case["x_series"].copy()
            xs[b] = xs[a]
            case["x_series"] = xs
        f.add("G:ties")
    bad = rng.random() < 0.5
    f.add("bad-days:yes" if bad else "bad-days:no")
    if bad:
        case = LR.with_bad_days(case, chain_nan=int(rng.integers(B)), day_nan=int(rng.integers(T)), chain_neg=int(rng.integers(B)),
                                day_neg=int(rng.integers(T)))
    if rng.random() < 0.25:
        k0, k1 = 0, T
    else:
        k0 = int(rng.integers(0, T))
        k1 = int(rng.integers(k0 + 1, T + 1))
    f.add("window:whole" if (k0, k1) == (0, T) else "window:part")
    if k0 % 32:
        f.add("window:k0-inside-a-block")
    if k1 % 32 and k1 != T:
        f.add("window:k1-inside-a-block")
    blk, storage = _layout(rng, f, B), _storage(rng, f)
    names = ()
    while not set(names) & {"loglik", "nis_mean", "S", "nis", "R_used"}:     # the call wants one of these
        names = _subset(rng, [k for k in LOGLIK_OUT if G or k not in ("best", "best_loglik")])
    _out_features(f, LOGLIK_OUT, names)
    host = _host(rng, f)
    kw = dict(case=case, k0=k0, k1=k1, storage=storage, G=G)
    return Case("innovation_likelihood", seed, kw, names, dict(blk=blk), host,
                f"innovation_likelihood seed={seed} {kind} B={B} T={T} L={w.L} {w.obs_type} R_series={w.R_series is not None} miss={miss:g} "
                f"k0={k0} k1={k1} G={G} ties={'G:ties' in f} bad={bad} blk={blk} {storage} names={names}", f)


# ---- two_filter ------------------------------------------------------------------------------------------------------------
# T B m^3: the items of an example times the size of their pseudo-inverse; keeps the restatement (nested Python lists, one item at
# a time) under about 0.3 s an example
FUSE_FUZZ_CAP = 60_000
FUSE_PAIRS = ((0, 0), (0, 1), (1, 0))                       # (form, p_solver): the information form has one solver
FUSE_OUT = ("s", "P", "d2", "rank", "status")               # batch.two_filter's names (the ABI's: s_out, P_out)
FUSE_FEATURES = (_out_list(FUSE_OUT) + ("m:3", "m:6", "pair:(0, 0)", "pair:(0, 1)", "pair:(1, 0)", "layout:classic", "layout:blocked-3",
                 "layout:blocked-8", "layout:blocked-40", "layout:ragged-last-block", "storage:f64", "storage:f32", "source:oracle",
                 "source:planted-ranks", "item:indefinite", "item:nonfinite", "host:yes", "host:no", "status:0", "status:NONFINITE",
                 "rank:deficient", "rank:full", "route:jacobi", "route:factorisation"))


def _fuse_status(want):
    st, rk, rt = (np.asarray(want[k]) for k in ("status", "rank", "route"))
    out = {"status:0"} if (st == 0).any() else set()
    if (st & 1).any():
        out.add("status:NONFINITE")
    m = int(round(np.sqrt(np.asarray(want["P"]).shape[1])))
    if ((rk >= 0) & (rk < m)).any():
        out.add("rank:deficient")
    if (rk == m).any():
        out.add("rank:full")
    if (rt == 1).any():
        out.add("route:jacobi")
    if ((rt == 0) | (rt == 2)).any():
        out.add("route:factorisation")
    return out


def make_two_filter(seed):
    """epi_fuse_validate: m 3 or 6, B, T >= 1, the three (form, p_solver) pairs the call takes, one of s / P / d2 asked for, lane_block 0 .. B, storage 0 / 1.
    Half of the examples fuse a forward and a time-flipped run of the oracle (cfg3: m = 3, cfg4: m = 6; the backward run's arrays
    reversed in time), half tests/two_filter_ref.planted's inputs with a planted rank of Pf + Pb per item, an indefinite and a
    non-finite item.  B, T 1 .. 70 cut down to T B m^3 <= FUSE_FUZZ_CAP."""
    from epidemicmodeling_amd import synth
    from tests import helpers as H
    from tests import two_filter_ref as TF
    rng, f = np.random.default_rng(seed), set()
    m = int(_pick(rng, (3, 6)))
    f.add(f"m:{m}")
    B, T = int(rng.integers(1, 71)), int(rng.integers(2, 71))
    wide = rng.random() < 0.25                               # room for a block of 40 chains: few days instead of few chains
    if wide:
        B = int(rng.integers(40, 71))
    while T * B * m ** 3 > FUSE_FUZZ_CAP:
        if B >= T and not (wide and T > 2):
            B = max(1, B * 2 // 3)
        else:
            T = max(2, T * 2 // 3)
    form, p_solver = FUSE_PAIRS[int(rng.integers(3))]
    f.add(f"pair:{(form, p_solver)}")
    if rng.random() < 0.5:
        f.add("source:oracle")
        if m == 3:
            w = synth.make_cfg3(B, T)
        else:
            E = int(_pick(rng, [e for e in range(1, B + 1) if B % e == 0]))
            w = synth.make_cfg4(B // E, E, T, 0)
        fw, bw = H.oracle_batch(w), H.oracle_batch(synth.as_backward(w))
        arrs = [fw["S_PLUS"], fw["P_PLUS"], bw["S_MINUS"][::-1], bw["P_MINUS"][::-1]]
        arrs = [np.ascontiguousarray(a, dtype=np.float64) for a in arrs]
    else:
        f.add("source:planted-ranks")
        arrs = list(TF.planted(m, T, B, int(rng.integers(1 << 30)), indefinite=True, nonfinite=True))
        if T * B >= 3:
            f.add("item:indefinite")
        if T * B >= 2:
            f.add("item:nonfinite")
    blk, storage = _layout(rng, f, B), _storage(rng, f)
    names = ()
    while not set(names) & {"s", "P", "d2"}:                   # the call wants one of these
        names = _subset(rng, FUSE_OUT)
    _out_features(f, FUSE_OUT, names)
    host = _host(rng, f)
    kw = dict(sf=arrs[0], Pf=arrs[1], sb=arrs[2], Pb=arrs[3], form=form, p_solver=p_solver, storage=storage)
    return Case("two_filter", seed, kw, names, dict(blk=blk), host,
                f"two_filter seed={seed} m={m} B={B} T={T} form={form} p_solver={p_solver} blk={blk} {storage} "
                f"source={'oracle' if 'source:oracle' in f else 'planted'} names={names}", f)


# ======================================================================================================================
CALLS = {
    "ensemble_summary": Spec(make_ensemble_summary, 200, ENS_FEATURES),
    "ensemble_score": Spec(make_ensemble_score, 120, ESCORE_FEATURES),
    "path_functionals": Spec(make_path_functionals, 120, PATHFN_FEATURES),
    "ensemble_joint_score": Spec(make_ensemble_joint_score, 100, EJOINT_FEATURES),
    "mldivide": Spec(make_mldivide, 40, MLDIV_FEATURES, _mldiv_status),
    "svr": Spec(make_svr, 40, SVR_FEATURES, _svr_status),
    "rate_map": Spec(make_rate_map, 60, RATEMAP_FEATURES, _ratemap_status),
    "robust_affine_fit": Spec(make_robust_affine_fit, 60, ROBFIT_FEATURES, _robfit_status),
    "npi_plan": Spec(make_npi_plan, 40, PLAN_FEATURES, _plan_status),
    "ar_forecast": Spec(make_ar_forecast, 100, ARFC_FEATURES, _arfc_status),
    "smoother_draws": Spec(make_smoother_draws, 40, SDRAW_FEATURES, _sdraw_status),
    "innovation_likelihood": Spec(make_innovation_likelihood, 80, LOGLIK_FEATURES, _loglik_status),
    "two_filter": Spec(make_two_filter, 60, FUSE_FEATURES, _fuse_status),
}


# what the loaders of the C restatements pre-fill their outputs with (int32, float64); the other restatements allocate theirs
# unfilled or build them item by item
SENTINELS = {"mldivide": (-7, -7777.25), "svr": (-7, -7777.25), "rate_map": (-7, -7777.25), "robust_affine_fit": (-7, -7.0),
             "npi_plan": (-7, -7.0)}
ONE_READING = ("ensemble_summary", "ar_forecast", "two_filter")      # calls with a single complete restatement


# ---- seeded twins --------------------------------------------------------------------------------------
# ar_forecast and smoother_draws also take seed= / noise_stream= in place of z: the draws are then made inside the kernel.  A twin
# is DERIVED from a generated example that has a z -- the example itself, and every draw of its generator, stay what they were --
# for the seeds that are a multiple of TWIN_EVERY: one example in three keeps the restatements' time of the two hunts within 1.5
# times what it was without twins (profiles/fuzz_calls/README.md).
SEEDED_CALLS = ("ar_forecast", "smoother_draws")
TWIN_EVERY = 3


def seeded_twin(refs, case):
    """The seeded twin of an example of SEEDED_CALLS, or None (no z, or a seed that gets none).  The noise seed and stream come
    from a generator of their own, keyed on the example's seed; the twin's kw["z"] is the array of that seed by the C restatement
    tests/noise_ref.c, as double ([T - k0, 3, B D] for smoother_draws, t = 0 at day k0; [H, B] for ar_forecast: the single row,
    squeezed), so `reference` and `second_reading` take the twin as they take any example; `noise` = (seed, stream) is what the
    call under test receives in place of z."""
    if case.call not in SEEDED_CALLS or case.noise is not None or case.kw["z"] is None or case.seed % TWIN_EVERY:
        return None
    rng = np.random.default_rng([case.seed, 0x5EED])
    nseed, stream = int(rng.integers(0, 2 ** 64, dtype=np.uint64)), int(_pick(rng, (0, 1, 2 ** 30 - 1, int(rng.integers(0, 2 ** 30)))))
    kw = dict(case.kw)
    nt, lanes = case.kw["z"].shape[0], case.kw["z"].shape[-1]
    if case.call == "ar_forecast":
        kw["z"] = np.ascontiguousarray(refs.get("noise").fill(nseed, stream, 0, nt, 1, 0, lanes)[:, 0])
    else:
        kw["z"] = refs.get("noise").fill(nseed, stream, 0, nt, 3, 0, lanes)
    f = {v for v in case.features if not v.startswith("z:")} | {"z:seeded"}
    return dataclasses.replace(case, kw=kw, features=f, noise=(nseed, stream),
                               summary=f"{case.summary} [seeded twin: seed={nseed:#x} stream={stream}]")


def cases_of(refs, call, seed):
    """the example of a seed, followed by its seeded twin where it has one"""
    case = CALLS[call].make(seed)
    twin = seeded_twin(refs, case) if refs is not None else None
    return [case] if twin is None else [case, twin]


def default_cases(call, refs=None):
    """the examples of the call's default seeds; with refs (the noise restatement has to be built) also their seeded twins"""
    spec = CALLS[call]
    return [c for s in range(spec.n) for c in cases_of(refs, call, s)]


# ======================================================================================================================
# the restatements: `reference` is what the GPU test compares with (the C one where a call has it), `second_reading` the
# other one (None where a call has a single restatement)
# ======================================================================================================================
class Refs:
    """the C restatements, each built on first use into its own directory under `root` (a pytest tmp_path_factory)"""

    def __init__(self, factory):
        self.factory, self.built = factory, {}

    def get(self, call):
        if call not in self.built:
            d = self.factory.mktemp("fuzz_" + call)
            if call == "ensemble_score":
                from tests.escore_ref import EscoreC as Cls
            elif call == "path_functionals":
                from tests.pathfn_ref import PathfnC as Cls
            elif call == "ensemble_joint_score":
                from tests.ejoint_ref import EjointC as Cls
            elif call == "mldivide":
                from tests.mldivide_ref import MldivRef as Cls
            elif call == "svr":
                from tests.svr_ref import SvrRef as Cls
            elif call == "rate_map":
                from tests.rate_map_ref import RatemapRef as Cls
            elif call == "robust_affine_fit":
                from tests.robust_fit_ref import RobfitRef as Cls
            elif call == "npi_plan":
                from tests.npi_plan_ref import PlanRef as Cls
            elif call == "ar_forecast":
                from tests.ar_forecast_ref import ArRef as Cls
            elif call == "smoother_draws":
                from tests.sdraw_ref import SdrawRef as Cls
            elif call == "noise":
                from tests.noise_ref import NoiseRef as Cls
            elif call == "innovation_likelihood":
                from tests.loglik_ref import LoglikRef as Cls
            else:
                raise KeyError(call)
            self.built[call] = Cls(d)
        return self.built[call]


def reference(refs, case):
    """the dict of every output of `case` by the restatement the GPU test compares with"""
    kw = case.kw
    if case.call == "ensemble_summary":
        from tests import ens_summary_ref as E
        return E.summary(**kw)
    if case.call == "ensemble_score":
        return refs.get(case.call).score(**kw)
    if case.call == "path_functionals":
        return refs.get(case.call).functionals(**kw)
    if case.call == "ensemble_joint_score":
        return refs.get(case.call).joint(**kw)
    if case.call == "mldivide":
        return refs.get(case.call).run(kw["X"], kw["y"], kw["n_rows"], kw["tol_scale"])
    if case.call == "svr":
        return refs.get(case.call).run(**kw)
    if case.call == "rate_map":
        p = kw["p"]
        return refs.get(case.call).run(p, [k for k in RATEMAP_OUT if (p["fit"] or k != "map") and (p["y"] is not None or k != "y_filled")])
    if case.call == "robust_affine_fit":
        return refs.get(case.call).run(**kw)
    if case.call == "npi_plan":
        return refs.get(case.call).run(kw["case"])
    if case.call == "ar_forecast":
        return refs.get(case.call).run(**kw)
    if case.call in ("smoother_draws", "innovation_likelihood"):
        return refs.get(case.call).run(**kw)
    if case.call == "two_filter":
        from tests import two_filter_ref as TF
        return TF.fuse(kw["sf"], kw["Pf"], kw["sb"], kw["Pb"], kw["form"], kw["p_solver"], storage=kw["storage"])
    raise KeyError(case.call)


def second_reading(refs, case):
    """the other restatement's outputs, or None"""
    kw = case.kw
    if case.call == "ensemble_score":
        from tests import escore_ref as S
        return S.score(**kw)
    if case.call == "path_functionals":
        from tests import pathfn_ref as S
        return S.functionals(**kw)
    if case.call == "ensemble_joint_score":
        from tests import ejoint_ref as J
        return J.joint(**kw)
    if case.call == "mldivide":
        from tests import mldivide_ref as ML
        o = ML.np_mldivide(kw["X"], kw["y"], kw["n_rows"], kw["tol_scale"], refs.get(case.call).fma)
        return {k: o[k] for k in MLDIV_OUT}
    if case.call == "svr":
        from tests import svr_ref as SV
        return SV.np_svr(kw["X"], kw["y"], kw["n_rows"], kw["kernel"], kw["box"], kw["epsilon"], kw["kernel_scale"], kw["tol"],
                         kw["max_iter"], refs.get(case.call))
    if case.call == "rate_map":
        from tests import rate_map_ref as RM
        r = refs.get(case.call)
        return RM.np_rate_map(kw["p"], r.fma, r.exp)
    if case.call == "robust_affine_fit":
        from tests import robust_fit_ref as RF
        return RF.np_robust_fit(**kw)
    if case.call == "npi_plan":
        from tests import npi_plan_ref as PR
        o = PR.np_plan(refs.get(case.call).fma, kw["case"])
        return {k: o[k] for k in PLAN_OUT if k != "F_trace"}   # the NumPy reading leaves the trace's unused tail NaN
    if case.call == "smoother_draws":
        from tests import sdraw_ref as SR
        return SR.np_sdraw(refs.get(case.call), **kw)
    if case.call == "innovation_likelihood":
        from tests import loglik_ref as LR
        return LR.np_loglik(refs.get(case.call), **kw)
    return None


def expected_shapes(case):
    """name -> shape of every output of the example, from the library's own shape rules (epidemicmodeling_amd._lib, no device)"""
    from epidemicmodeling_amd import _lib
    kw = case.kw
    if case.call in ("ensemble_summary", "ensemble_score", "path_functionals", "ensemble_joint_score"):
        T, rows, _ = kw["src"].shape
        R, D, der = kw["R"], kw["D"], int(kw["population"] is not None)
        if case.call == "ensemble_summary":
            return _lib.ens_shapes(T, rows, R, len(kw["q"]), der)
        if case.call == "ensemble_score":
            return _lib.escore_shapes(T, rows, R, len(kw["alpha"]), kw["n_bins"], der)
        if case.call == "path_functionals":
            return _lib.pathfn_shapes(rows, R, D, 0 if kw["thr"] is None else len(kw["thr"]), kw["k1"] - kw["k0"], der)
        return _lib.ejoint_shapes(rows, R, D, der)
    if case.call in ("mldivide", "svr"):
        D, F, R = kw["X"].shape
        return (_lib.mldiv_shapes if case.call == "mldivide" else _lib.svr_shapes)(D, F, R, len(kw["n_rows"]))
    if case.call == "rate_map":
        p = kw["p"]
        T, n, R = p["ip"].shape
        return _lib.ratemap_shapes(T, n, R, 0 if p["extra"] is None else p["extra"].shape[1], len(p["n_train"]), len(p["lags"]))
    if case.call == "robust_affine_fit":
        D, n, R = kw["X"].shape
        return _lib.robfit_shapes(R, D, n)
    if case.call == "npi_plan":
        c = kw["case"]
        return _lib.plan_shapes(c["R"], c["P"], c["H"], c["n"], c["max_iter"])
    if case.call == "ar_forecast":
        L, R = kw["seg"].shape
        sh = _lib.arfc_shapes(R, kw["D"], L, kw["p"], kw["H"])
        return {"S": sh["S"], "A": sh["A_out"], "noise_var": sh["noise_var_out"], "status": sh["status"]}
    if case.call == "smoother_draws":
        return _lib.sdraw_shapes(kw["case"]["B"], kw["case"]["T"], kw["D"], kw["k0"])
    if case.call == "innovation_likelihood":
        return _lib.loglik_shapes(kw["case"]["B"], kw["case"]["T"], kw["G"])
    if case.call == "two_filter":
        T, m, B = kw["sf"].shape
        sh = _lib.fuse_shapes(m, B, T, 0)
        return {"s": sh["s_out"], "P": sh["P_out"], "d2": sh["d2"], "rank": sh["rank"], "status": sh["status"]}
    raise KeyError(case.call)


def same_bits(a, b):
    """bit for bit, every NaN one value; dtype and shape included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        na, nb = np.isnan(a), np.isnan(b)
        u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        return bool((na == nb).all() and np.array_equal(a[~na].view(u), b[~nb].view(u)))
    return bool(np.array_equal(a, b))

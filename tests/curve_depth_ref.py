"""NumPy restatement of the curve statistics of the ensembles (include/epiekf_cdepth.h) and the driver of its
sequential C twin tests/curve_depth_ref.c.  The counts come from the sorted valid members of a day (searchsorted on both
sides), which is the rank form; tests/test_curve_depth_ref.py holds it to literal pair enumeration."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np

PATH_F64 = ("depth", "mhi", "band_count", "pair_total")
PATH_I32 = ("n_valid", "depth_rank", "out_days")
REGION_I32 = ("n_ranked", "median_path", "n_outliers")
ENV = ("env_lo", "env_hi")
DAY = ("median_curve", "whisk_lo", "whisk_hi")
NAMES = PATH_F64 + PATH_I32 + REGION_I32 + ENV + DAY
I32 = PATH_I32 + REGION_I32
NEED_FENCE = ("out_days", "n_outliers", "whisk_lo", "whisk_hi")


def rows_with_derived(src, population, R, D):
    """[T, rows', N] float64: src widened, and the derived row ((N_r v0) v1) v2 behind it"""
    x = np.asarray(src).astype(np.float64)
    if population is None:
        return x
    pop = np.repeat(np.asarray(population, dtype=np.float64), D)
    with np.errstate(all="ignore"):
        return np.concatenate([x, (((pop * x[:, 0]) * x[:, 1]) * x[:, 2])[:, None]], axis=1)


def deepest(f, n):
    return min(n, max(1, int(math.ceil(float(f) * float(n)))))


def _min(v):
    lo = v.min()
    return -0.0 if lo == 0 and np.signbit(v[v == 0]).any() else lo


def _max(v):
    hi = v.max()
    return 0.0 if hi == 0 and (~np.signbit(v[v == 0])).any() else hi


def _envelope(x, keep):
    """(lo, hi) [W] over the members keep [D] of x [W, D] that are not NaN, NaN without one"""
    lo, hi = np.full(len(x), np.nan), np.full(len(x), np.nan)
    for i, row in enumerate(x):
        v = row[keep & ~np.isnan(row)]
        if len(v):
            lo[i], hi[i] = _min(v), _max(v)
    return lo, hi


def empty_outputs(T, ro, R, D, na, fill=None, ifill=None):
    N = R * D
    sh = {k: (ro, N) for k in PATH_F64 + PATH_I32}
    sh.update({k: (ro, R) for k in REGION_I32})
    sh.update({k: (T, na, ro, R) for k in ENV})
    sh.update({k: (T, ro, R) for k in DAY})
    mk = lambda k: (np.empty(sh[k], dtype=np.int32) if ifill is None else np.full(sh[k], ifill, dtype=np.int32)) if k in I32 else \
        (np.empty(sh[k]) if fill is None else np.full(sh[k], fill))
    return {k: mk(k) for k in NAMES}


def statistics(src, R, D, alpha=(0.5, 0.9), fence_factor=1.5, fence_frac=0.5, population=None, first_day=None, k0=0, k1=None):
    """every output of epi_cdepth_run_* as a dict of NumPy arrays (the boxplot's are 0 / NaN with fence_factor = 0)"""
    x = rows_with_derived(src, population, R, D)
    T, ro, N = x.shape
    k1 = T if k1 is None else int(k1)
    alpha = [float(a) for a in (() if alpha is None else alpha)]
    na = len(alpha)
    out = empty_outputs(T, ro, R, D, na, np.nan, 0)
    for q in range(ro):
        for r in range(R):
            lo = max(k0, 0 if first_day is None else int(first_day[r]))
            sl = slice(r * D, (r + 1) * D)
            v = x[lo:k1, q, sl] if lo < k1 else np.zeros((0, D))                # [W', D]
            acc = np.zeros((5, D), dtype=np.int64)                              # band, pairs, le, members, days
            for row in v:
                ok = ~np.isnan(row)
                s = np.sort(row[ok])
                n = len(s)
                below = np.searchsorted(s, row[ok], side="left").astype(np.int64)
                le = np.searchsorted(s, row[ok], side="right").astype(np.int64)
                above = n - le
                c2 = n * (n - 1) // 2
                acc[0, ok] += c2 - below * (below - 1) // 2 - above * (above - 1) // 2
                acc[1, ok] += c2
                acc[2, ok] += le
                acc[3, ok] += n
                acc[4, ok] += 1
            with np.errstate(all="ignore"):
                depth = np.where(acc[1] > 0, acc[0].astype(np.float64) / acc[1].astype(np.float64), np.nan)
                mhi = np.where(acc[4] > 0, acc[2].astype(np.float64) / acc[3].astype(np.float64), np.nan)
            out["depth"][q, sl], out["mhi"][q, sl] = depth, mhi
            out["band_count"][q, sl], out["pair_total"][q, sl], out["n_valid"][q, sl] = acc[0], acc[1], acc[4]
            ranked = np.flatnonzero(~np.isnan(depth))
            order = ranked[np.argsort(-depth[ranked], kind="stable")]          # deepest first, the lower draw first among equals
            rank = np.full(D, -1, dtype=np.int64)
            rank[order] = np.arange(len(order))
            nr = len(order)
            mp = int(order[0]) if nr else -1
            out["depth_rank"][q, sl], out["n_ranked"][q, r], out["median_path"][q, r] = rank, nr, mp
            for k, a in enumerate(alpha):
                out["env_lo"][lo:k1, k, q, r], out["env_hi"][lo:k1, k, q, r] = _envelope(v, (rank >= 0) & (rank < deepest(a, nr)))
            if mp >= 0:
                out["median_curve"][lo:k1, q, r] = v[:, mp]
            if not fence_factor > 0.0:
                continue
            flo, fhi = _envelope(v, (rank >= 0) & (rank < deepest(fence_frac, nr)))
            with np.errstate(all="ignore"):
                w = fhi - flo
                fw = fence_factor * w
                lo_f, hi_f = (flo - fw)[:, None], (fhi + fw)[:, None]
                od = (~np.isnan(v) & ((v < lo_f) | (v > hi_f))).sum(axis=0)
            out["out_days"][q, sl] = od
            out["n_outliers"][q, r] = int(((rank >= 0) & (od > 0)).sum())
            out["whisk_lo"][lo:k1, q, r], out["whisk_hi"][lo:k1, q, r] = _envelope(v, (rank >= 0) & (od == 0))
    return out


def pair_enumeration(v):
    """one (row, region) v [W, D] by the literal definition: (band_count, pair_total) [D], counting for every day on which the path
    is valid the unordered pairs {e, f} of valid members, e = f excluded but the path itself allowed, whose closed band
    [min, max] holds the path's value"""
    W, D = v.shape
    band, pairs = np.zeros(D, dtype=np.int64), np.zeros(D, dtype=np.int64)
    for t in range(W):
        ok = [e for e in range(D) if not math.isnan(v[t, e])]
        for d in ok:
            for i, e in enumerate(ok):
                for f in ok[i + 1:]:
                    pairs[d] += 1
                    band[d] += min(v[t, e], v[t, f]) <= v[t, d] <= max(v[t, e], v[t, f])
    return band, pairs


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:                           # every NaN is one value; the zeros keep their sign
        na, nb = np.isnan(a), np.isnan(b)
        return bool((na == nb).all() and (a[~na].view(np.uint64) == b[~nb].view(np.uint64)).all())
    return bool((a == b).all())


class CurveDepthC:
    """tests/curve_depth_ref.c built with the host C compiler into `tmp` and called through ctypes"""

    def __init__(self, tmp):
        cc = shutil.which("cc") or shutil.which("gcc")
        if not cc:
            raise RuntimeError("no C compiler for tests/curve_depth_ref.c")
        here = os.path.dirname(os.path.abspath(__file__))
        so = os.path.join(str(tmp), "curve_depth_ref.so")
        subprocess.run([cc, "-O2", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
                        os.path.join(here, "curve_depth_ref.c"), "-o", so, "-lm"], check=True)
        self.lib = C.CDLL(so)
        self.lib.cdepth_ref.restype = C.c_int

    def statistics(self, src, R, D, alpha=(0.5, 0.9), fence_factor=1.5, fence_frac=0.5, population=None, first_day=None, k0=0, k1=None):
        src = np.ascontiguousarray(src, dtype=np.float32 if np.asarray(src).dtype == np.float32 else np.float64)
        T, rows, N = src.shape
        k1 = T if k1 is None else int(k1)
        ro = rows + int(population is not None)
        al = np.ascontiguousarray(() if alpha is None else alpha, dtype=np.float64)
        pop = None if population is None else np.ascontiguousarray(population, dtype=np.float64)
        fd = None if first_day is None else np.ascontiguousarray(first_day, dtype=np.int32)
        out = empty_outputs(T, ro, R, D, len(al))
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        rc = self.lib.cdepth_ref(C.c_int(T), C.c_int(rows), C.c_int(R), C.c_int(D), C.c_int(len(al)), C.c_int(int(src.dtype == np.float32)),
                                 C.c_int(int(pop is not None)), C.c_int(k0), C.c_int(k1), p(src), p(pop), p(fd), p(al),
                                 C.c_double(float(fence_factor or 0.0)), C.c_double(float(fence_frac)), *[p(out[k]) for k in NAMES])
        assert rc == 0
        return out


def base_case(storage="f64", R=2, D=70, rows=3, T=40, k0=3, k1=38, first_day=(0, 20), derive=True, seed=1, planted=True):
    """A small ensemble with the planted cases in region 0 of row 0: an all-NaN path, NaN days, both infinities, two identical
    paths, a day of ties, signed zeros.  Returns the keyword arguments of statistics() with src first"""
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None, None]
    src = np.abs(rng.standard_normal((T, rows, R * D))) * 10.0 ** rng.uniform(-1, 1, size=(1, rows, 1)) + \
        np.exp(-0.5 * ((t - rng.uniform(0, T, size=(1, rows, R * D))) / 4.0) ** 2)
    src = src.astype(np.float32) if storage == "f32" else src
    pop = rng.uniform(1e5, 1e7, R) if derive else None
    if planted and D >= 12 and T >= 23:
        src[:, min(1, rows - 1), 2] = np.nan                             # an all-NaN path (and its derived row)
        src[10:14, 0, 3] = np.nan                                       # NaN days
        src[20, 0, 4], src[21, 0, 5] = np.inf, -np.inf
        src[22, 0, 4], src[22, 0, 6] = np.inf, np.inf                   # two members at +Inf on one day
        src[:, 0, 8] = src[:, 0, 7]                                     # two identical paths: the index breaks the tie
        src[15, 0, :D] = np.round(src[15, 0, :D])                       # a day of ties
        src[16, 0, 9], src[16, 0, 10] = 0.0, -0.0
        src[17, 0, 1:D] = np.nan                                        # a day with one member
        src[18, 0, :D] = np.nan                                         # and one with none
    fd = None if first_day is None else np.asarray(first_day[:R] + (0,) * max(0, R - len(first_day)), dtype=np.int32)
    return dict(src=src, R=R, D=D, population=pop, first_day=fd, k0=k0, k1=k1)

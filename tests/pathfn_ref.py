"""NumPy restatement of the path functionals (include/epiekf.h): every path at once, the days one after the other
in ascending order, one IEEE double operation per written operation.  PathfnC drives the sequential C restatement
tests/pathfn_ref.c.  brute() is an independent formulation (np.nanmax, first argmax, a Python loop for the runs, math.fsum) that
the two are held against."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np

PATH_F64 = ("peak_value", "peak_day", "min_value", "min_day", "total")
THR_F64 = ("first_cross", "days_above", "longest_run")
REGION = ("n_paths", "peak_day_hist", "n_cross", "cross_day_hist")
NAMES = PATH_F64 + THR_F64 + ("n_valid",) + REGION
I32 = ("n_valid",) + REGION
BLOCK = 32


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:                       # every NaN is one value: the payload of a produced NaN is not pinned
        a, b = np.where(np.isnan(a), np.nan, a), np.where(np.isnan(b), np.nan, b)
        return bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
    return bool(np.array_equal(a, b))


def rows_with_derived(src, population, R, D):
    """[T, rows', N] in double: a float32 value widened once, the derived row ((N_r v0) v1) v2 appended"""
    x = np.asarray(src).astype(np.float64)
    if population is None:
        return x
    Np = np.repeat(np.asarray(population, dtype=np.float64), D)[None, :]
    with np.errstate(all="ignore"):
        new = ((Np * x[:, 0]) * x[:, 1]) * x[:, 2]
    return np.concatenate([x, new[:, None]], axis=1)


def functionals(src, R, D, thr=None, population=None, first_day=None, k0=0, k1=None):
    src = np.asarray(src)
    T, rows, N = src.shape
    assert N == R * D
    k1 = T if k1 is None else int(k1)
    W = k1 - k0
    x = rows_with_derived(src, population, R, D)
    ro = x.shape[1]
    thr = np.zeros((0, ro, R)) if thr is None else np.asarray(thr, dtype=np.float64).reshape(-1, ro, R)
    nt = thr.shape[0]
    thp = np.repeat(thr, D, axis=2)                                     # [nt, ro, N]
    fd = np.zeros(R, dtype=np.int64) if first_day is None else np.asarray(first_day, dtype=np.int64)
    lo = np.maximum(k0, np.repeat(fd, D))[None, :]                       # [1, N]
    mx, mn = np.zeros((ro, N)), np.zeros((ro, N))
    mxd, mnd, nv = (np.zeros((ro, N), dtype=np.int64) for _ in range(3))
    tot, bs = np.zeros((ro, N)), np.zeros((ro, N))
    first = np.full((nt, ro, N), -1, dtype=np.int64)
    cnt, cur, best = (np.zeros((nt, ro, N), dtype=np.int64) for _ in range(3))
    with np.errstate(all="ignore"):
        for t in range(k0, k1):
            if (t - k0) % BLOCK == 0 and t > k0:
                tot = tot + bs
                bs = np.zeros((ro, N))
            v = x[t]
            ok = (t >= lo) & ~np.isnan(v)
            gt, lt = ok & ((nv == 0) | (v > mx)), ok & ((nv == 0) | (v < mn))
            mx, mxd = np.where(gt, v, mx), np.where(gt, t, mxd)
            mn, mnd = np.where(lt, v, mn), np.where(lt, t, mnd)
            nv = nv + ok
            bs = np.where(ok, bs + v, bs)
            ab = ok[None] & (v[None] >= thp)
            first = np.where(ab & (first < 0), t, first)
            cnt = cnt + ab
            cur = np.where(ab, cur + 1, 0)
            best = np.maximum(best, cur)
        tot = tot + bs
    any_ = nv > 0
    nanif = lambda a, keep: np.where(keep, a.astype(np.float64), np.nan)
    out = dict(peak_value=nanif(mx, any_), peak_day=nanif(mxd, any_), min_value=nanif(mn, any_), min_day=nanif(mnd, any_),
               total=nanif(tot, any_))
    asked = any_[None] & ~np.isnan(thp)
    out.update(first_cross=nanif(first, asked & (first >= 0)), days_above=nanif(cnt, asked), longest_run=nanif(best, asked))
    out["n_valid"] = nv.astype(np.int32)
    out.update(regions(out["peak_day"], out["first_cross"], R, D, k0, W))
    return {k: out[k] for k in NAMES}


def regions(peak_day, first_cross, R, D, k0, W):
    ro, nt = peak_day.shape[0], first_cross.shape[0]
    n_paths, n_cross = np.zeros((ro, R), dtype=np.int32), np.zeros((nt, ro, R), dtype=np.int32)
    ph, ch = np.zeros((W, ro, R), dtype=np.int32), np.zeros((W, nt, ro, R), dtype=np.int32)
    for q in range(ro):
        for r in range(R):
            d = peak_day[q, r * D:(r + 1) * D]
            d = d[~np.isnan(d)].astype(np.int64)
            n_paths[q, r] = len(d)
            ph[:, q, r] = np.bincount(d - k0, minlength=W)
            for j in range(nt):
                c = first_cross[j, q, r * D:(r + 1) * D]
                c = c[~np.isnan(c)].astype(np.int64)
                n_cross[j, q, r] = len(c)
                ch[:, j, q, r] = np.bincount(c - k0, minlength=W)
    return dict(n_paths=n_paths, peak_day_hist=ph, n_cross=n_cross, cross_day_hist=ch)


def brute(v, lo, k1, thr):
    """one path's row v [T] by definition: (peak_value, peak_day, min_value, min_day, fsum, sum|v|, n_valid, [(first, days, run)])"""
    idx = [t for t in range(max(lo, 0), k1) if not math.isnan(v[t])]
    if not idx:
        return None
    w = np.array([v[t] for t in idx], dtype=np.float64)
    pv, nv_ = np.nanmax(w), np.nanmin(w)
    pd, md = idx[int(np.argmax(w))], idx[int(np.argmin(w))]
    fin = [float(a) for a in w if math.isfinite(a)]
    per = []
    for th in thr:
        if math.isnan(th):
            per.append(None)
            continue
        above = [t for t in idx if v[t] >= th]
        run = best = 0
        prev = None
        for t in above:
            run = run + 1 if prev is not None and t == prev + 1 else 1
            best, prev = max(best, run), t
        per.append((above[0] if above else None, len(above), best))
    return pv, pd, nv_, md, (math.fsum(fin) if len(fin) == len(w) else None), float(np.sum(np.abs(fin))), len(idx), per


class PathfnC:
    """tests/pathfn_ref.c built with the host C compiler into `tmp` and called through ctypes"""

    def __init__(self, tmp):
        cc = shutil.which("cc") or shutil.which("gcc")
        if not cc:
            raise RuntimeError("no C compiler for tests/pathfn_ref.c")
        here = os.path.dirname(os.path.abspath(__file__))
        so = os.path.join(str(tmp), "pathfn_ref.so")
        subprocess.run([cc, "-O1", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", os.path.join(here, "pathfn_ref.c"),
                        "-o", so, "-lm"], check=True)
        self.lib = C.CDLL(so)

    def functionals(self, src, R, D, thr=None, population=None, first_day=None, k0=0, k1=None):
        src = np.ascontiguousarray(src, dtype=np.float32 if np.asarray(src).dtype == np.float32 else np.float64)
        T, rows, N = src.shape
        k1 = T if k1 is None else int(k1)
        ro, W = rows + int(population is not None), k1 - k0
        thr = np.zeros((0, ro, R)) if thr is None else np.ascontiguousarray(np.asarray(thr, dtype=np.float64).reshape(-1, ro, R))
        nt = thr.shape[0]
        pop = None if population is None else np.ascontiguousarray(population, dtype=np.float64)
        fd = None if first_day is None else np.ascontiguousarray(first_day, dtype=np.int32)
        out = empty_outputs(ro, R, D, nt, W)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self.lib.pathfn_ref(C.c_int(T), C.c_int(rows), C.c_int(R), C.c_int(D), C.c_int(nt), C.c_int(int(src.dtype == np.float32)),
                            C.c_int(int(pop is not None)), C.c_int(k0), C.c_int(k1), p(src), p(pop), p(thr), p(fd),
                            *[p(out[k]) for k in NAMES])
        return out


def empty_outputs(ro, R, D, nt, W, fill=None, ifill=None):
    N = R * D
    sh = {k: (ro, N) for k in PATH_F64}
    sh.update({k: (nt, ro, N) for k in THR_F64})
    sh.update(n_valid=(ro, N), n_paths=(ro, R), peak_day_hist=(W, ro, R), n_cross=(nt, ro, R), cross_day_hist=(W, nt, ro, R))
    mk = lambda k: (np.empty(sh[k], dtype=np.int32) if ifill is None else np.full(sh[k], ifill, dtype=np.int32)) if k in I32 else \
        (np.empty(sh[k]) if fill is None else np.full(sh[k], fill))
    return {k: mk(k) for k in NAMES}


def base_case(storage="f64", R=3, D=70, rows=3, T=75, n_thr=3, k0=5, k1=72, first_day=(0, 40, 72), derive=True, seed=1):
    """The smallest shape that reaches every branch (a wavefront spans two regions, the last one is partial; the window is two whole
    blocks and three days; the third region has no valid day), with the planted cases in region 0: returns the keyword arguments
    of functionals() with src first"""
    rng = np.random.default_rng(seed)
    src = np.abs(rng.standard_normal((T, rows, R * D))) * 10.0 ** rng.uniform(-1, 1, size=(1, rows, 1))
    src = src.astype(np.float32) if storage == "f32" else src
    pop = rng.uniform(1e5, 1e7, R) if derive else None
    src[:, min(1, rows - 1), 2] = np.nan                                # an all-NaN path (and its derived row)
    src[10:31, 0, 3] = 50.0
    src[15:17, 0, 3] = np.nan                                           # NaN days inside a run
    src[20, 0, 4], src[21, 0, 5] = np.inf, -np.inf
    src[12, 0, 6] = src[50, 0, 6] = 1e3                                 # the maximum on two days: the first wins
    src[:, 0, 7] = 0.001
    src[30, 0, 7] = 7.5                                                 # exactly its threshold (below)
    src[:, 0, 8] = 60.0                                                 # above on every day: the run spans every border
    src[:, 0, 9] = -0.0                                                 # a total of signed zeros
    if n_thr == 0:
        thr = None
    else:
        x = rows_with_derived(src, pop, R, D)
        ro = x.shape[1]
        lev = np.linspace(0.5, 0.99, n_thr)
        with np.errstate(all="ignore"):
            fin = np.where(np.isfinite(x), x, np.nan)
            thr = np.stack([np.nanquantile(fin.reshape(T, ro, R, D), l, axis=(0, 3)) for l in lev])      # [n_thr, ro, R]
        thr[0, 0, 0] = 7.5
        if n_thr > 1:
            thr[1, min(2, ro - 1), 0] = -np.inf                         # every valid day is above
        if n_thr > 2:
            thr[2, min(1, ro - 1), :] = np.nan                          # not asked for this row
    fd = None if first_day is None else np.asarray(first_day, dtype=np.int32)
    return dict(src=src, R=R, D=D, thr=thr, population=pop, first_day=fd, k0=k0, k1=k1)

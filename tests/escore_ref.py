"""The probabilistic forecast scores of epi_escore_run_* (include/epiekf.h) in NumPy, statement for statement:
every operation below is one IEEE double operation, in the order the definition gives.  The CRPS terms are summed by sorted
position through the pairwise tree of tests/ens_summary_ref.py over P positions, P the power of two >= max(D, 64) -- the tree the
wavefront runs.  tests/escore_ref.c says the same sequentially in C; EscoreC builds and calls it."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from tests import ens_summary_ref as E

ITEM_F64 = ("crps", "wis", "ae")
ITEM_I32 = ("rank", "ties", "cover", "count")
REGION_F64 = ("crps_mean", "wis_mean", "ae_mean")
NAMES = ITEM_F64 + ("width",) + ITEM_I32 + REGION_F64 + ("n_scored", "cover_frac", "pit_hist")
I32 = ITEM_I32 + ("n_scored", "pit_hist")


def probabilities(alpha):
    """q_lo, q_hi of the levels: formed once, in double (the library does the same on the host)"""
    a = np.asarray(alpha, dtype=np.float64).reshape(-1)
    return a / np.float64(2.0), np.float64(1.0) - a / np.float64(2.0)


def positions(D):
    """P: the sorted positions the tree runs over"""
    P = 64
    while P < D:
        P *= 2
    return P


def pos(d):
    return d if d > 0.0 else np.float64(0.0)


def crps_terms(x, n, y, D):
    """the tree's inputs: the term of every sorted position 1 .. n, +0.0 at n+1 .. P"""
    nd = np.float64(n)
    i = np.arange(1, n + 1, dtype=np.float64)
    with np.errstate(all="ignore"):
        coef = (np.where(y < x[:n], nd, np.float64(0.0)) - i) + np.float64(0.5)
        term = (x[:n] - y) * coef
    return np.concatenate([term, np.zeros(positions(D) - n)])


def item(v, y, alpha):
    """v [D] (any NaN = absent member), the truth y, the levels -> dict crps, wis, ae, width [n_a], rank, ties, cover, count"""
    with np.errstate(all="ignore"):
        v = np.asarray(v, dtype=np.float64)
        y = np.float64(y)
        alpha = np.asarray(alpha, dtype=np.float64).reshape(-1)
        ok = ~np.isnan(v)
        n = int(ok.sum())
        nan = np.float64(np.nan)
        if n == 0 or np.isnan(y):
            return dict(crps=nan, wis=nan, ae=nan, width=np.full(len(alpha), nan), rank=-1, ties=-1, cover=0, count=n)
        rank, ties = int((v < y).sum()), int((v == y).sum())
        x = np.sort(v[ok])
        med = E.quantile(x, n, np.float64(0.5))
        ae = np.abs(y - med)
        acc = np.float64(0.5) * ae
        q_lo, q_hi = probabilities(alpha)
        width, cover = np.empty(len(alpha)), 0
        for k in range(len(alpha)):
            l, u = E.quantile(x, n, q_lo[k]), E.quantile(x, n, q_hi[k])
            wd, c = u - l, np.float64(2.0) / alpha[k]
            IS = (wd + c * pos(l - y)) + c * pos(y - u)
            acc = acc + (alpha[k] / np.float64(2.0)) * IS
            if l <= y and y <= u:
                cover |= 1 << k
            width[k] = wd
        wis = acc / (np.float64(len(alpha)) + np.float64(0.5))
        nd = np.float64(n)
        crps = (np.float64(2.0) / (nd * nd)) * E.tree(crps_terms(x, n, y, len(v)))
        return dict(crps=crps, wis=wis, ae=ae, width=width, rank=rank, ties=ties, cover=cover, count=n)


def crps_double_sum(v, y):
    """the definition: (1/n) sum |x_i - y| - (1/(2 n^2)) sum sum |x_i - x_j| over the members that are not NaN"""
    x = np.asarray(v, dtype=np.float64)
    x = x[~np.isnan(x)]
    n = len(x)
    return np.abs(x - y).sum() / n - np.abs(x[:, None] - x[None, :]).sum() / (2.0 * n * n)


def pit_bin(rank, ties, count, n_bins):
    return min(n_bins - 1, ((2 * int(rank) + int(ties) + 1) * int(n_bins)) // (2 * (int(count) + 1)))


def regions(it, n_a, n_bins, first_day=None, k0=0, k1=None):
    """the per-item arrays [T, rows', R] -> the per-(row, region) outputs: the days ascending from 0.0"""
    T, ro, R = it["rank"].shape
    k1 = T if k1 is None else k1
    out = {k: np.empty((ro, R)) for k in REGION_F64}
    out["n_scored"] = np.zeros((ro, R), dtype=np.int32)
    out["cover_frac"] = np.empty((n_a, ro, R))
    out["pit_hist"] = np.zeros((n_bins, ro, R), dtype=np.int32)
    nan = np.float64(np.nan)
    for row in range(ro):
        for r in range(R):
            fd = 0 if first_day is None else int(first_day[r])
            s = {k: np.float64(0.0) for k in ITEM_F64}
            ns, cov = 0, [0] * n_a
            for t in range(k0, k1):
                if t < fd or it["rank"][t, row, r] < 0:
                    continue
                ns += 1
                for k in ITEM_F64:
                    s[k] = s[k] + it[k][t, row, r]
                for k in range(n_a):
                    cov[k] += (int(it["cover"][t, row, r]) >> k) & 1
                if n_bins:
                    out["pit_hist"][pit_bin(it["rank"][t, row, r], it["ties"][t, row, r], it["count"][t, row, r], n_bins), row, r] += 1
            out["n_scored"][row, r] = ns
            with np.errstate(all="ignore"):
                for k in ITEM_F64:
                    out[k + "_mean"][row, r] = s[k] / np.float64(ns) if ns else nan
                for k in range(n_a):
                    out["cover_frac"][k, row, r] = np.float64(cov[k]) / np.float64(ns) if ns else nan
    return out


def score(src, truth, R, D, alpha=(0.5, 0.05), n_bins=0, population=None, truth_series=None, first_day=None, k0=0, k1=None):
    """src [T, rows, R * D] float32 / float64, truth [T, rows', Rt] -> the dict of batch.ensemble_score as NumPy arrays"""
    s = np.asarray(src).astype(np.float64)
    if population is not None:
        s = np.concatenate([s, E.derived_row(s, population, R, D)[:, None, :]], axis=1)
    truth = np.asarray(truth, dtype=np.float64)
    alpha = np.asarray(alpha, dtype=np.float64).reshape(-1)
    T, ro, _ = s.shape
    n_a = len(alpha)
    out = {k: np.empty((T, ro, R)) for k in ITEM_F64}
    out["width"] = np.empty((T, n_a, ro, R))
    out.update({k: np.empty((T, ro, R), dtype=np.int32) for k in ITEM_I32})
    for t in range(T):
        for j in range(ro):
            for r in range(R):
                ts = r if truth_series is None else int(truth_series[r])
                it = item(s[t, j, r * D:(r + 1) * D], truth[t, j, ts], alpha)
                for k in ITEM_F64 + ITEM_I32:
                    out[k][t, j, r] = it[k]
                out["width"][t, :, j, r] = it["width"]
    out.update(regions(out, n_a, n_bins, first_day, k0, k1))
    return {k: out[k] for k in NAMES}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:                       # every NaN is one value: the payload of a produced NaN is not pinned
        a, b = np.where(np.isnan(a), np.nan, a), np.where(np.isnan(b), np.nan, b)
        return bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))
    return bool(np.array_equal(a, b))


class EscoreC:
    """tests/escore_ref.c built with the host C compiler into `tmp` and called through ctypes"""

    def __init__(self, tmp):
        cc = shutil.which("cc") or shutil.which("gcc")
        if not cc:
            raise RuntimeError("no C compiler for tests/escore_ref.c")
        here = os.path.dirname(os.path.abspath(__file__))
        so = os.path.join(str(tmp), "escore_ref.so")
        subprocess.run([cc, "-O1", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", os.path.join(here, "escore_ref.c"),
                        "-o", so, "-lm"], check=True)
        self.lib = C.CDLL(so)

    def score(self, src, truth, R, D, alpha=(0.5, 0.05), n_bins=0, population=None, truth_series=None, first_day=None, k0=0, k1=None):
        src = np.ascontiguousarray(src, dtype=np.float32 if np.asarray(src).dtype == np.float32 else np.float64)
        T, rows, _ = src.shape
        truth = np.ascontiguousarray(truth, dtype=np.float64)
        alpha = np.ascontiguousarray(np.asarray(alpha, dtype=np.float64).reshape(-1))
        q_lo, q_hi = (np.ascontiguousarray(v) for v in probabilities(alpha))
        n_a, ro = len(alpha), rows + int(population is not None)
        pop = None if population is None else np.ascontiguousarray(population, dtype=np.float64)
        ts = None if truth_series is None else np.ascontiguousarray(truth_series, dtype=np.int32)
        fd = None if first_day is None else np.ascontiguousarray(first_day, dtype=np.int32)
        out = {k: np.empty((T, ro, R)) for k in ITEM_F64}
        out["width"] = np.empty((T, n_a, ro, R))
        out.update({k: np.empty((T, ro, R), dtype=np.int32) for k in ITEM_I32})
        out.update({k: np.empty((ro, R)) for k in REGION_F64})
        out["n_scored"] = np.empty((ro, R), dtype=np.int32)
        out["cover_frac"] = np.empty((n_a, ro, R))
        out["pit_hist"] = np.empty((n_bins, ro, R), dtype=np.int32)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self.lib.escore_ref(C.c_int(T), C.c_int(rows), C.c_int(R), C.c_int(D), C.c_int(truth.shape[2]), C.c_int(n_a), C.c_int(n_bins),
                            C.c_int(int(src.dtype == np.float32)), C.c_int(int(pop is not None)), C.c_int(k0), C.c_int(T if k1 is None else k1),
                            p(src), p(pop), p(truth), p(ts), p(fd), p(alpha), p(q_lo), p(q_hi), *[p(out[k]) for k in NAMES])
        return out

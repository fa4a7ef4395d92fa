"""The joint scores of epi_ejoint_run_* (include/epiekf.h) in NumPy, statement for statement: every operation
below is one IEEE double operation, in the order the definition gives; the pairwise tree is tests/ens_summary_ref.tree.  Also
the driver of the sequential C restatement tests/ejoint_ref.c (EjointC) and the cases the CPU and the GPU tests share."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from tests import ens_summary_ref as E
from tests.escore_ref import same_bits  # noqa: F401  (the tests compare through it)

F64 = ("es", "truth_term", "spread_term", "vs")
I32 = ("n_members", "n_days")
NAMES = F64 + I32 + ("member_dist",)


def g(a, vs_order):
    a = np.abs(a)
    return np.sqrt(a) if vs_order == 1 else a


def padded(v, P):
    return np.concatenate([v, np.zeros(P - len(v))])


def item(x, y, days, vs_order=0, max_lag=0, parts=("es", "vs")):
    """x [W, D] the members on the item's days, y [W] the truth, days [W] their calendar days -> dict of the item's outputs"""
    W, D = x.shape
    nan = np.float64(np.nan)
    ok = ~np.isnan(x).any(axis=0)
    n = int(ok.sum())
    out = dict(n_members=n, n_days=W, es=nan, truth_term=nan, spread_term=nan, vs=nan, member_dist=np.full(D, nan))
    if n == 0 or W == 0:
        return out
    P = 64
    while P < D:
        P *= 2
    nd = np.float64(n)
    with np.errstate(all="ignore"):
        d2 = np.zeros(D)
        for w in range(W):
            d = x[w] - y[w]
            d2 = d2 + d * d
        e = np.sqrt(d2)
        out["member_dist"] = np.where(ok, e, nan)
        out["truth_term"] = E.tree(padded(np.where(ok, e, 0.0), P)) / nd
        if "es" in parts:
            nb = (D + 63) // 64
            xp = np.zeros((W, nb * 64))
            xp[:, :D] = x
            okp = np.zeros(nb * 64, dtype=bool)
            okp[:D] = ok
            ii, jj = np.arange(64)[:, None], np.arange(64)[None, :]
            ps = np.float64(0.0)
            for I in range(nb):
                for J in range(I, nb):
                    a, b = xp[:, I * 64:(I + 1) * 64], xp[:, J * 64:(J + 1) * 64]
                    acc = np.zeros((64, 64))
                    for w in range(W):
                        d = a[w][:, None] - b[w][None, :]
                        acc = acc + d * d
                    on = okp[I * 64:(I + 1) * 64][:, None] & okp[J * 64:(J + 1) * 64][None, :]
                    if I == J:
                        on = on & (jj > ii)
                    c = np.where(on, np.sqrt(acc), 0.0)
                    s = np.zeros(64)
                    for j in range(64):
                        s = s + c[:, j]
                    ps = ps + E.tree(s)
            out["spread_term"] = ps / (nd * nd)
            out["es"] = out["truth_term"] - out["spread_term"]
        if vs_order and "vs" in parts:
            vs = np.float64(0.0)
            for s in range(W):
                v = np.float64(0.0)
                for t in range(s + 1, W):
                    if max_lag > 0 and days[t] - days[s] > max_lag:
                        break
                    m = E.tree(padded(np.where(ok, g(x[s] - x[t], vs_order), 0.0), P)) / nd
                    term = g(y[s] - y[t], vs_order) - m
                    v = v + term * term
                vs = vs + v
            out["vs"] = vs
    return out


def joint(src, truth, R, D, vs_order=0, max_lag=0, population=None, truth_series=None, first_day=None, k0=0, k1=None, parts=("es", "vs")):
    """src [T, rows, R * D] float32 / float64, truth [T, rows', Rt] -> the dict of batch.ensemble_joint_score as NumPy arrays
    (every name of NAMES; what `parts` leaves out, or vs with vs_order = 0, is NaN)"""
    s = np.asarray(src).astype(np.float64)
    if population is not None:
        s = np.concatenate([s, E.derived_row(s, population, R, D)[:, None, :]], axis=1)
    truth = np.asarray(truth, dtype=np.float64)
    T, ro, _ = s.shape
    k1 = T if k1 is None else int(k1)
    out = {k: np.empty((ro, R)) for k in F64}
    out.update({k: np.empty((ro, R), dtype=np.int32) for k in I32})
    out["member_dist"] = np.empty((ro, R * D))
    for row in range(ro):
        for r in range(R):
            ts = r if truth_series is None else int(truth_series[r])
            fd = 0 if first_day is None else int(first_day[r])
            days = np.array([t for t in range(max(int(k0), fd), k1) if not np.isnan(truth[t, row, ts])], dtype=np.int64)
            it = item(s[days, row, r * D:(r + 1) * D], truth[days, row, ts], days, vs_order, max_lag, parts)
            for k in F64 + I32:
                out[k][row, r] = it[k]
            out["member_dist"][row, r * D:(r + 1) * D] = it["member_dist"]
    return out


class EjointC:
    """tests/ejoint_ref.c built with the host C compiler into `tmp` and called through ctypes"""

    def __init__(self, tmp):
        cc = shutil.which("cc") or shutil.which("gcc")
        if not cc:
            raise RuntimeError("no C compiler for tests/ejoint_ref.c")
        here = os.path.dirname(os.path.abspath(__file__))
        so = os.path.join(str(tmp), "ejoint_ref.so")
        subprocess.run([cc, "-O1", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", os.path.join(here, "ejoint_ref.c"),
                        "-o", so, "-lm"], check=True)
        self.lib = C.CDLL(so)

    def joint(self, src, truth, R, D, vs_order=0, max_lag=0, population=None, truth_series=None, first_day=None, k0=0, k1=None):
        src = np.ascontiguousarray(src, dtype=np.float32 if np.asarray(src).dtype == np.float32 else np.float64)
        T, rows, _ = src.shape
        truth = np.ascontiguousarray(truth, dtype=np.float64)
        ro = rows + int(population is not None)
        pop = None if population is None else np.ascontiguousarray(population, dtype=np.float64)
        ts = None if truth_series is None else np.ascontiguousarray(truth_series, dtype=np.int32)
        fd = None if first_day is None else np.ascontiguousarray(first_day, dtype=np.int32)
        out = {k: np.empty((ro, R)) for k in F64}
        out.update({k: np.empty((ro, R), dtype=np.int32) for k in I32})
        out["member_dist"] = np.empty((ro, R * D))
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self.lib.ejoint_ref(C.c_int(T), C.c_int(rows), C.c_int(R), C.c_int(D), C.c_int(truth.shape[2]), C.c_int(int(src.dtype == np.float32)),
                            C.c_int(int(pop is not None)), C.c_int(k0), C.c_int(T if k1 is None else k1), C.c_int(vs_order), C.c_int(max_lag),
                            p(src), p(pop), p(truth), p(ts), p(fd), *[p(out[k]) for k in NAMES])
        return out


# ---- the cases the restatement tests and the GPU tests share ----
CASE_D = (1, 2, 63, 64, 65, 130, 300)
CASE_W = (1, 2, 33)
R_CASE, ROWS_CASE = 3, 3


def case(D, W, dtype, variant, seed=None):
    """One call's arguments: R = 3 regions of D draws, 3 rows plus the derived row, a window 1 <= t < T - 1 of W + 1 days of which
    column 0 of the truth has one NaN day (W days left), regions 0 and 2 sharing column 0.  It carries a member absent on one
    day only (row 1, so the derived row too), a NaN member on the day without a truth (which leaves the member present), a region
    with every member absent and, by variant, a first_day at k1 (0) or past k1 (1)."""
    rng = np.random.default_rng(1000 * D + 10 * W + variant if seed is None else seed)
    R, rows, T = R_CASE, ROWS_CASE, W + 3
    k0, k1 = 1, T - 1
    src = (0.5 + rng.random((T, rows, R * D))).astype(dtype)
    truth = 0.5 + rng.random((T, rows + 1, 2))
    truth[:, rows] *= 3.0e3                                             # the derived row's scale: N * v0 * v1 * v2
    t_gap = k0 + (W + 1) // 2
    truth[t_gap, :, 0] = np.nan
    src[t_gap, 0, 0] = np.nan                                           # not a day of the item: the member stays
    t_abs = k1 - 1 if t_gap != k1 - 1 else k0
    src[t_abs, 1, (0 if D > 1 else 2 * D) + D // 2] = np.nan            # a member absent on one day only
    src[k0 + W // 2, :, D:2 * D] = np.nan                               # region 1: nobody left
    pop = np.array([3.0e3, 5.0e3, 4.0e3])
    first_day = np.array([0, 0, k1] if variant == 0 else [k0 + 1, k1 + 2, 0], dtype=np.int32)
    return dict(src=src, truth=truth, R=R, D=D, population=pop, truth_series=np.array([0, 1, 0], dtype=np.int32), first_day=first_day,
                k0=k0, k1=k1)


# ---- the member-count grid: every register count NV of ejoint_launch's dispatch, every block count of ejoint_pairs ----
nv_of = lambda D: max(64, 1 << (D - 1).bit_length()) // 64            # D <= 64: 1, <= 128: 2, .. <= 2048: 32, else 64
nb_of = lambda D: (D + 63) // 64
# the member counts of the CPU comparison of the two restatements beyond CASE_D: one of each of NV = 16, 32, 64
BIG_D = (1000, 2000, 4096)


def grid_absent(D):
    """the members grid_case makes absent on one day beyond case()'s (region, row, member): for D > 64 the last member (the
    last block) and, for D > 128, one of block 1 and one of the middle block -- blocks I, J > 0 whose mask words decide a bit"""
    if D <= 64:
        return []
    nb = nb_of(D)
    out = [(0, 1, D - 1), (2, 0, D - 1)]
    if nb > 2:
        out += [(0, 1, 64 + 5), (2, 0, (nb // 2) * 64 + 7)]
    return out


def grid_case(D, W, dtype, variant):
    """case(D, W, dtype, variant) with the members of grid_absent(D) absent on one day of their items (W >= 2)"""
    c = case(D, W, dtype, variant)
    assert W >= 2
    k0, k1 = c["k0"], c["k1"]
    t_gap = k0 + (W + 1) // 2
    t_abs = k1 - 1                                                      # a day of every defined item: W >= 2 keeps it off t_gap
    assert t_abs != t_gap and t_abs >= k0 + 1
    for r, row, e in grid_absent(D):
        c["src"][t_abs, row, r * D + e] = np.nan
    return c

"""MATLAB's rectangular backslash (csrc/mldivide.hpp) restated twice: the loader of tests/mldivide_ref.c, the
bit-exact C yardstick, and `np_mldivide`, a NumPy reading that keeps LAPACK's own shape -- the columns are swapped in place as
dgeqp3's unblocked dlaqp2 swaps them, the reflector is stored below the diagonal, the update is a matrix-vector product over
whole column blocks, R is cut out as a triangle and solved -- in the operation order §4.12 pins.  Both must agree bit for bit.
Also here: the shapes and planted inputs the CPU and GPU suites share and the generator of the plans of the LAPACK comparison.

The test modules build the C twin in a session fixture: `MldivRef(tmp_path_factory.mktemp("mldiv"))`."""
from __future__ import annotations

import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "mldivide_ref.c")

RANK_DEFICIENT, NONFINITE_INPUT, NONFINITE = 1, 2, 4
OUT_NAMES = ("m", "rank", "perm", "rdiag", "resid", "fitted", "status")
OUT_I32 = ("rank", "perm", "status")
P = 8                                   # the interleaved chains of every sum over rows
EPS = 2.0 ** -52
TOL3Z = 2.0 ** -26
TINY = 2.0 ** -900                      # a column whose squares sum to less has no reflector

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


def shapes(D, F, R, K):
    return {"m": (K, F, R), "rank": (K, R), "perm": (K, F, R), "rdiag": (K, F, R), "resid": (K, R), "fitted": (K, D, R),
            "status": (K, R)}


class MldivRef:
    """tests/mldivide_ref.c behind ctypes"""

    def __init__(self, build_dir):
        cc = shutil.which("gcc") or shutil.which("cc")
        if cc is None:
            raise RuntimeError("no C compiler for tests/mldivide_ref.c")
        so = os.path.join(str(build_dir), "libmldivide_ref.so")
        subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", so, "-lm"])
        h = C.CDLL(so)
        h.mldivide_run.restype = None
        h.mldivide_run.argtypes = [_dp, _dp, _ip] + [C.c_int] * 4 + [C.c_double, _dp, _ip, _ip, _dp, _dp, _dp, _ip]
        h.ml_fma_pub.restype = C.c_double
        h.ml_fma_pub.argtypes = [C.c_double] * 3
        h.ml_fma_vec.restype = None
        h.ml_fma_vec.argtypes = [_dp, _dp, _dp, _dp, C.c_int]
        h.ml_recomputed_pub.restype = C.c_long
        h.ml_ties_pub.restype = C.c_long
        self.h = h

    def fma(self, a, b, c):
        """element-wise fma(a, b, c), one rounding"""
        if np.ndim(a) == 0 and np.ndim(b) == 0 and np.ndim(c) == 0:
            return self.h.ml_fma_pub(a, b, c)
        a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
        a, b, c = (np.ascontiguousarray(v) for v in (a, b, c))
        o = np.empty(a.shape)
        self.h.ml_fma_vec(a.ctypes.data_as(_dp), b.ctypes.data_as(_dp), c.ctypes.data_as(_dp), o.ctypes.data_as(_dp), a.size)
        return o

    def counters(self, reset=False):
        """(norms recomputed under the safeguard, pivot choices that met a tie) since the last reset"""
        v = (int(self.h.ml_recomputed_pub()), int(self.h.ml_ties_pub()))
        if reset:
            self.h.ml_counters_reset()
        return v

    def run(self, X, y, n_rows=None, tol_scale=1.0, outputs=OUT_NAMES):
        """X [D, F, R], y [D, R] -> the outputs asked for as NumPy arrays (poisoned where the call must write)"""
        X, y = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
        D, F, R = X.shape
        nr = np.ascontiguousarray([D] if n_rows is None else n_rows, dtype=np.int32)
        sh = shapes(D, F, R, len(nr))
        o = {k: np.full(sh[k], -7 if k in OUT_I32 else -7777.25, dtype=np.int32 if k in OUT_I32 else np.float64) for k in outputs}
        op = lambda k: None if k not in o else o[k].ctypes.data_as(_ip if k in OUT_I32 else _dp)
        self.h.mldivide_run(X.ctypes.data_as(_dp), y.ctypes.data_as(_dp), nr.ctypes.data_as(_ip), D, F, R, len(nr), float(tol_scale),
                            op("m"), op("rank"), op("perm"), op("rdiag"), op("resid"), op("fitted"), op("status"))
        return o


def same_bits(u, v):
    """bit for bit, any NaN equal to any NaN"""
    u, v = np.asarray(u), np.asarray(v)
    if u.shape != v.shape or u.dtype != v.dtype:
        return False
    if u.dtype.kind != "f":
        return bool((u == v).all())
    nu, nv = np.isnan(u), np.isnan(v)
    return bool((nu == nv).all() and (u.view(np.int64)[~nu] == v.view(np.int64)[~nv]).all())


# ---- the NumPy reading, one item at a time -----------------------------------------------------------------------------
def rowsum(a, b, lo, fma):
    """sum over the rows lo .. of a_i b_i for every column of a, b [n, c]: P interleaved fma chains from +0 (row i in chain
    i mod P), added in ascending order"""
    n = a.shape[0]
    s = np.zeros((P,) + a.shape[1:])
    for i in range(lo, n):
        s[i % P] = fma(a[i], b[i], s[i % P])
    t = s[0].copy()
    for p in range(1, P):
        t = t + s[p]
    return t


def np_item(Xn, yn, tol_scale, fma, Xall):
    """one item: Xn [n, F], yn [n] the used rows, Xall [D, F] -> dict; also 'recomputed' and 'ties'"""
    n, F = Xn.shape
    mn = min(n, F)
    if not (np.isfinite(Xn).all() and np.isfinite(yn).all()):
        return dict(m=np.full(F, np.nan), rank=-1, perm=np.arange(F), rdiag=np.full(F, np.nan), resid=np.nan,
                    fitted=np.full(Xall.shape[0], np.nan), status=NONFINITE_INPUT, recomputed=0, ties=0)
    A = np.hstack([Xn, yn[:, None]]).copy()                               # [n, F + 1], swapped in place like dlaqp2
    jpvt = np.arange(F)
    vn1 = np.sqrt(rowsum(A[:, :F], A[:, :F], 0, fma))
    vn2 = vn1.copy()
    rdiag = np.zeros(F)
    recomputed = ties = 0
    with np.errstate(all="ignore"):
        for j in range(mn):
            # the largest partial norm; ties to the lowest ORIGINAL index (LAPACK: the lowest current position)
            best = j
            for q in range(j + 1, F):
                if vn1[q] > vn1[best] or (vn1[q] == vn1[best] and jpvt[q] < jpvt[best]):
                    best = q
            ties += int((vn1[j:] == vn1[best]).sum() > 1)
            if best != j:
                A[:, [j, best]] = A[:, [best, j]]
                jpvt[[j, best]], vn1[[j, best]], vn2[[j, best]] = jpvt[[best, j]], vn1[[best, j]], vn2[[best, j]]
            # dlarfg
            alpha = A[j, j]
            ss = float(rowsum(A[:, j:j + 1], A[:, j:j + 1], j + 1, fma)[0])
            beta, tau = alpha, 0.0
            t2 = fma(alpha, alpha, ss)
            if ss != 0.0 and t2 >= TINY:
                beta = -np.copysign(np.sqrt(t2), alpha)
                tau = (beta - alpha) / beta
                A[j + 1:, j] = A[j + 1:, j] * (1.0 / (alpha - beta))
            rdiag[j] = beta
            # dlarf on the trailing block and y
            if tau != 0.0:
                v = np.repeat(A[:, j:j + 1], F - j, axis=1)
                w = A[j, j + 1:] + rowsum(v, A[:, j + 1:], j + 1, fma)
                tw = tau * w
                A[j, j + 1:] = A[j, j + 1:] - tw
                A[j + 1:, j + 1:] = fma(-tw[None, :], A[j + 1:, j:j + 1], A[j + 1:, j + 1:])
            A[j, j] = beta
            for q in range(j + 1, F):
                if vn1[q] == 0.0:
                    continue
                t = abs(A[j, q]) / vn1[q]
                temp = 1.0 - t * t
                if temp < 0.0:
                    temp = 0.0
                u = vn1[q] / vn2[q]
                if temp * (u * u) <= TOL3Z:
                    vn1[q] = vn2[q] = np.sqrt(float(rowsum(A[:, q:q + 1], A[:, q:q + 1], j + 1, fma)[0]))
                    recomputed += 1
                else:
                    vn1[q] = vn1[q] * np.sqrt(temp)
        tol = tol_scale * float(max(n, F)) * EPS * abs(rdiag[0])
        rank = 0
        while rank < mn and abs(rdiag[rank]) > tol:
            rank += 1
        Rm, z = np.triu(A[:mn, :F]), A[:, F]
        s, mp = z[:rank].copy(), np.zeros(rank)
        for q in range(rank - 1, -1, -1):
            mp[q] = s[q] / Rm[q, q]
            if q:
                s[:q] = fma(-Rm[:q, q], mp[q], s[:q])
        m = np.zeros(F)
        m[jpvt[:rank]] = mp
        resid = float(np.sqrt(rowsum(z[:, None], z[:, None], rank, fma)[0]))
        fitted = Xall[:, 0] * m[0]
        for f in range(1, F):
            fitted = fma(Xall[:, f], m[f], fitted)
    bad = not (np.isfinite(m).all() and np.isfinite(rdiag).all() and np.isfinite(resid) and np.isfinite(fitted).all())
    return dict(m=m, rank=rank, perm=jpvt.copy(), rdiag=rdiag, resid=resid, fitted=fitted,
                status=(RANK_DEFICIENT if rank < mn else 0) | (NONFINITE if bad else 0), recomputed=recomputed, ties=ties, R=Rm)


def np_mldivide(X, y, n_rows, tol_scale, fma):
    """every output of the call; also 'recomputed' and 'ties' summed over the items"""
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    D, F, R = X.shape
    nr = [D] if n_rows is None else list(n_rows)
    o = {k: np.zeros(s, dtype=np.int32 if k in OUT_I32 else np.float64) for k, s in shapes(D, F, R, len(nr)).items()}
    o["recomputed"] = o["ties"] = 0
    for k, n in enumerate(nr):
        for r in range(R):
            it = np_item(X[:n, :, r], y[:n, r], tol_scale, fma, X[:, :, r])
            for name in ("m", "perm", "rdiag", "fitted"):
                o[name][k, :, r] = it[name]
            for name in ("rank", "resid", "status"):
                o[name][k, r] = it[name]
            o["recomputed"] += it["recomputed"]
            o["ties"] += it["ties"]
    return o


# ---- the shapes and inputs the suites share: (D, F, K, R) and the row counts --------------------------------------------
CASES = [
    ((1, 1, 1, 1), (1,)),
    ((5, 5, 2, 63), (3, 5)),
    ((12, 7, 3, 64), (1, 7, 12)),
    ((40, 17, 2, 65), (25, 40)),
    ((257, 3, 3, 2), (255, 256, 257)),
    ((206, 96, 1, 2), (206,)),                                          # on the LDS limit: 206 x 97 = 19 982
    ((400, 49, 1, 3), (400,)),                                          # on the LDS limit: 400 x 50 = 20 000
]


def make_case(seed, D, F, K, R):
    """piecewise-constant integer plans as columns, a target that follows them plus noise; nothing planted"""
    g = np.random.default_rng(seed)
    X = np.empty((D, F, R))
    lvl = g.integers(0, 5, size=(F, R)).astype(np.float64)
    for t in range(D):
        sw = g.random((F, R)) < 0.1
        lvl = np.where(sw, g.integers(0, 5, size=(F, R)), lvl)
        X[t] = lvl
    w = g.normal(0, 0.03, size=(F, R))
    y = 0.15 - np.einsum("tfr,fr->tr", X, np.abs(w)) + g.normal(0, 0.05, size=(D, R))
    return X, y


def plant(X, y):
    """the sick items.  Region 0: column 2 duplicates column 0 (a tie and a rank deficiency), column 1 is zero, column 4 is
    column 0 plus 1e-9 of column 3 (the first reflector nearly cancels it: its norm is recomputed under the safeguard).
    Region 1: a NaN in the first row of X.  Region 2: an Inf in y's first row.  Region 3: a column of 1e200 t, which overflows
    the sum of squares.  The last region (R >= 6): all zero"""
    D, F, R = X.shape
    if F >= 3:
        X[:, 2, 0] = X[:, 0, 0]
        X[:, 1, 0] = 0.0
    if F >= 5:
        X[:, 4, 0] = X[:, 0, 0] + 1e-9 * X[:, 3, 0]
    if R >= 2:
        X[0, 0, 1] = np.nan
    if R >= 3:
        y[0, 2] = np.inf
    if R >= 4:
        X[:, 0, 3] = 1e200 * np.arange(1, D + 1)
    if R >= 6:
        X[:, :, R - 1] = 0.0
    return X, y


@functools.lru_cache(maxsize=None)
def problem(i):
    """case i of CASES with its planted inputs: (X, y, n_rows); shared and read-only"""
    (D, F, K, R), nr = CASES[i]
    X, y = plant(*make_case(200 + i, D, F, K, R))
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y, nr


def plans_problem(seed, regions, T=366, lags=(3, 5, 7), normalised=True):
    """the inputs of the LAPACK comparison: synthetic piecewise-constant integer plans, n = 12 with maxima
    [3 3 2 4 2 3 2 4 2 3 2 4], the switch probability of a region drawn from U(0, 0.1), the plans' copies lagged by 3 / 5 / 7
    and a ones column (F = 49), the columns divided by their max(abs) (0 -> 1) when `normalised`, y ~ N(0, 0.05).
    Returns X [T, 49, regions], y [T, regions]"""
    g = np.random.default_rng(seed)
    mx = np.array([3, 3, 2, 4, 2, 3, 2, 4, 2, 3, 2, 4])
    n = len(mx)
    X = np.zeros((T, n * (1 + len(lags)) + 1, regions))
    for r in range(regions):
        ps = g.uniform(0, 0.1)
        ip = np.empty((T, n))
        lvl = g.integers(0, mx + 1)
        for t in range(T):
            sw = g.random(n) < ps
            lvl = np.where(sw, g.integers(0, mx + 1), lvl)
            ip[t] = lvl
        blocks = [ip] + [np.vstack([np.zeros((lag, n)), ip[:T - lag]]) for lag in lags] + [np.ones((T, 1))]
        Xr = np.hstack(blocks)
        if normalised:
            m = np.abs(Xr).max(axis=0)
            m[m == 0] = 1.0
            Xr = Xr / m
        X[:, :, r] = Xr
    return X, g.normal(0, 0.05, size=(T, regions))

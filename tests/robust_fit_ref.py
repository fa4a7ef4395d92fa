"""NumPy restatement of DESIGN.md §4.10 (the element-wise robust regression), the loader of its C twin
tests/robust_fit_ref.c, and the seeded case generator the robust-fit tests share.

`np_robust_fit` runs every item at once: all operations are element-wise over the items, so the bits are those of one item
after the other.  The test modules build the C twin in a session fixture: `RobfitRef(tmp_path_factory.mktemp("robfit"))`."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "robust_fit_ref.c")

NONFINITE, CONST, SLOPE_LOST, MAXITER, BOUND = 1, 2, 4, 8, 16
OUT_NAMES = ("a", "b_item", "sigma", "iters", "status", "weights", "b")
EPS = 2.220446049250313e-16
SQRT_EPS = 1.4901161193847656e-08

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


def shapes(R, D, n):
    return {"a": (n, R), "b_item": (n, R), "sigma": (n, R), "iters": (n, R), "status": (n, R), "weights": (D, n, R), "b": (R,)}


def tree(v):
    """the pairwise tree over axis 0: a[i] += a[i + h], h = P/2 .. 1, +0.0 in the places D .. P-1"""
    D = v.shape[0]
    P = max(64, 1 << (D - 1).bit_length())
    a = np.zeros((P,) + v.shape[1:])
    a[:D] = v
    h = P // 2
    while h >= 1:
        a[:h] = a[:h] + a[h:2 * h]
        h //= 2
    return a[0]


def _wls(x, y, w, cst, lower, upper):
    sw = tree(w)
    mx = tree(w * x) / sw
    my = tree(w * y) / sw
    sxx = tree((w * (x - mx)) * (x - mx))
    sxy = tree((w * (x - mx)) * (y - my))
    swxx = tree((w * x) * x)
    ident = ~cst & (sxx > EPS * swxx)
    raw = sxy / sxx
    v = np.where(raw < lower, lower, raw)
    v = np.where(v > upper, upper, v)
    a = np.where(ident, v, 0.0)
    flags = np.where(ident, np.where(v != raw, BOUND, 0), np.where(cst, 0, SLOPE_LOST))
    return a, my - a * mx, flags.astype(np.int32)


def np_robust_fit(X, y, robust=1, lower=0.0, upper=np.inf, max_iter=50):
    """X [D, n, R], y [D, R] -> dict of every output of §4.10"""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    D, n, R = X.shape
    M = n * R
    with np.errstate(all="ignore"):
        x = X.reshape(D, M).copy()                       # item = k * R + r
        yy = np.tile(y, (1, n))
        bad = ~(np.isfinite(x).all(axis=0) & np.isfinite(yy).all(axis=0))
        x[:, bad] = 0.0
        yy[:, bad] = 0.0
        cst = x.max(axis=0) == x.min(axis=0)
        Dd = float(D)
        xbar = tree(x) / Dd
        sxx0 = tree((x - xbar) * (x - xbar))
        h = 1.0 / Dd + ((x - xbar) * (x - xbar)) / sxx0
        h = np.where(h < 0.9999, h, 0.9999)
        h = np.where(cst, 1.0 / Dd, h)
        adj = 1.0 / np.sqrt(1.0 - h)
        ybar = tree(yy) / Dd
        tiny = 1e-6 * np.sqrt(tree((yy - ybar) * (yy - ybar)) / (Dd - 1.0))
        tiny = np.where(tiny == 0.0, 1.0, tiny)
        w = np.ones((D, M))
        a, b, flags = _wls(x, yy, w, cst, lower, upper)
        sigma = np.full(M, np.nan)
        iters = np.zeros(M, dtype=np.int32)
        cap = np.zeros(M, dtype=np.int32)
        act = ~bad if robust else np.zeros(M, dtype=bool)
        m = D - 1
        while act.any():
            i = np.nonzero(act)[0]
            xi, yi = x[:, i], yy[:, i]
            radj = (yi - (a[i] * xi + b[i])) * adj[:, i]
            rs = np.sort(np.abs(radj), axis=0)
            med = rs[1 + (m - 1) // 2] if m & 1 else (rs[m // 2] + rs[m // 2 + 1]) / 2.0
            sg = med / 0.6745
            sg = np.where(sg > tiny[i], sg, tiny[i])
            u = radj / (sg * 4.685)
            t = 1.0 - u * u
            wi = np.where(np.abs(u) < 1.0, t * t, 0.0)
            a1, b1, f1 = _wls(xi, yi, wi, cst[i], lower, upper)
            a0, b0 = a[i], b[i]
            w[:, i], a[i], b[i], flags[i], sigma[i] = wi, a1, b1, f1, sg
            iters[i] += 1
            conv = (np.abs(a1 - a0) <= SQRT_EPS * np.maximum(np.abs(a1), np.abs(a0))) & \
                   (np.abs(b1 - b0) <= SQRT_EPS * np.maximum(np.abs(b1), np.abs(b0)))
            capped = ~conv & (iters[i] == max_iter)
            cap[i[capped]] = MAXITER
            act[i[conv | capped]] = False
        status = (np.where(cst, CONST, 0) | flags | cap).astype(np.int32)
        a[bad] = b[bad] = sigma[bad] = np.nan
        w[:, bad] = np.nan
        iters[bad] = 0
        status[bad] = NONFINITE
        a2 = a.reshape(n, R)
        t = np.zeros((D, R))
        for k in range(n):
            t = t + X[:, k, :] * a2[k]
        breg = (1.0 / Dd) * tree(y - t)
    return {"a": a2, "b_item": b.reshape(n, R), "sigma": sigma.reshape(n, R), "iters": iters.reshape(n, R),
            "status": status.reshape(n, R), "weights": w.reshape(D, n, R), "b": breg}


class RobfitRef:
    """tests/robust_fit_ref.c behind ctypes"""

    def __init__(self, build_dir):
        cc = shutil.which("gcc") or shutil.which("cc")
        if cc is None:
            raise RuntimeError("no C compiler for tests/robust_fit_ref.c")
        so = os.path.join(str(build_dir), "librobust_fit_ref.so")
        subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", so, "-lm"])
        h = C.CDLL(so)
        h.robfit_run.restype = None
        h.robfit_run.argtypes = [_dp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double,
                                 _dp, _dp, _dp, _ip, _ip, _dp, _dp]
        self.h = h

    def run(self, X, y, robust=1, lower=0.0, upper=np.inf, max_iter=50):
        X = np.ascontiguousarray(X, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        D, n, R = X.shape
        o = {k: (np.full(s, -7, dtype=np.int32) if k in ("iters", "status") else np.full(s, -7.0)) for k, s in shapes(R, D, n).items()}
        p = lambda k: o[k].ctypes.data_as(_ip if o[k].dtype == np.int32 else _dp)
        self.h.robfit_run(X.ctypes.data_as(_dp), y.ctypes.data_as(_dp), R, D, n, int(robust), int(max_iter), float(lower), float(upper),
                          p("a"), p("b_item"), p("sigma"), p("iters"), p("status"), p("weights"), p("b"))
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


SLOPES = (-0.02, 0.0, 0.03, 0.1)


def make_case(seed, D, n, R):
    """The seeded generator: per item (k, r) a piecewise-constant integer level in 0 .. 4 that switches with probability 0.08
    per day; region r's y follows its NPI k = r mod n: y = 0.2 + slope x + 0.01 N(0, 1) + 0.001 d, slope cycling through
    SLOPES; every fifth region gets max(1, D // 10) outliers of +-0.5, every seventh is an exact line (no noise, no trend)."""
    g = np.random.default_rng(seed)
    X = np.empty((D, n, R))
    lvl = g.integers(0, 5, size=(n, R))
    for d in range(D):
        sw = g.random((n, R)) < 0.08
        lvl = np.where(sw, g.integers(0, 5, size=(n, R)), lvl)
        X[d] = lvl
    y = np.empty((D, R))
    days = np.arange(D, dtype=np.float64)
    for r in range(R):
        slope = SLOPES[r % 4]
        xr = X[:, r % n, r]
        if r % 7 == 6:
            y[:, r] = 0.2 + slope * xr
            continue
        y[:, r] = 0.2 + slope * xr + 0.01 * g.standard_normal(D) + 0.001 * days
        if r % 5 == 4:
            at = g.choice(D, size=max(1, D // 10), replace=False)
            y[at, r] += 0.5 * g.choice((-1.0, 1.0), size=at.size)
    return X, y


def plant(X, y):
    """overwrite the first regions of a generated case with the planted item kinds (every region that the shape has room for):
    0 exact line, 1 negative slope (BOUND), 2 constant column, 3 one gross outlier, 4 the slope lost under the final weights
    (with lower_a = 0), 5 a non-finite item, 6 the 0.9999 leverage clip.  Returns the kinds that were planted."""
    D, n, R = X.shape
    d = np.arange(D, dtype=np.float64)
    done = []
    if R > 0:
        X[:, 0, 0] = d % 8
        y[:, 0] = 0.25 + 0.5 * X[:, 0, 0]
        done.append("exact")
    if R > 1:
        X[:, 0, 1] = d % 4
        y[:, 1] = 0.5 - 0.125 * X[:, 0, 1] + 0.001 * np.cos(3.0 * d)
        done.append("negative")
    if R > 2:
        X[:, n - 1, 2] = 3.0
        done.append("const")
    if R > 3:
        X[:, 0, 3] = d % 3
        y[:, 3] = 0.1 + 0.25 * X[:, 0, 3] + 0.001 * np.sin(5.0 * d)
        y[D // 2, 3] += 100.0
        done.append("outlier")
    if R > 4 and D <= 5:
        X[:, 0, 4] = 0.0
        X[D - 1, 0, 4] = 1.0
        y[:, 4] = 0.001 * np.cos(2.0 * d)
        y[D - 1, 4] = -10.0
        done.append("slope_lost")
    if R > 5:
        X[D - 1, n - 1, 5] = np.inf
        done.append("nonfinite")
    if R > 6:
        X[:, 0, 6] = 0.0
        X[D - 1, 0, 6] = 1.0
        y[:, 6] = 0.3 + 0.01 * np.sin(d)
        done.append("clip")
    return done

"""The support-vector regression (csrc/svr.hpp) restated twice: the loader of tests/svr_ref.c, the bit-exact C
yardstick, and `np_svr`, a NumPy reading of another shape -- the whole kernel matrix of a region is formed once, the 2n
variables are NumPy vectors, the selections are masked argmax calls -- in the operation order §4.13 pins.  Both must agree bit
for bit.  Also here: the shapes and planted inputs the CPU and GPU suites share, the generator of the synthetic plans, and
`dual_gap`, the independent check of the optimum in longdouble.

The test modules build the C twin in a session fixture: `SvrRef(tmp_path_factory.mktemp("svr"))`."""
from __future__ import annotations

import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "svr_ref.c")

NOT_CONVERGED, BAD_INPUT, NONFINITE = 1, 2, 4
OUT_NAMES = ("beta", "bias", "w", "fitted", "n_iter", "gap", "n_sv", "status")
OUT_I32 = ("n_iter", "n_sv", "status")
KERNELS = ("linear", "gaussian")
TAU = 1e-12
COUNTERS = ("opp_clip_0", "opp_clip_C", "eq_clip_C", "eq_clip_0", "same_row", "tau", "midpoint_bias")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


def shapes(D, F, R, K):
    return {"beta": (K, D, R), "bias": (K, R), "w": (K, F, R), "fitted": (K, D, R), "n_iter": (K, R), "gap": (K, R),
            "n_sv": (K, R), "status": (K, R)}


def out_names(kernel, outputs=None):
    return tuple(k for k in (OUT_NAMES if outputs is None else outputs) if k != "w" or kernel == "linear")


class SvrRef:
    """tests/svr_ref.c behind ctypes"""

    def __init__(self, build_dir):
        cc = shutil.which("gcc") or shutil.which("cc")
        if cc is None:
            raise RuntimeError("no C compiler for tests/svr_ref.c")
        so = os.path.join(str(build_dir), "libsvr_ref.so")
        subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", so, "-lm"])
        h = C.CDLL(so)
        h.svr_run.restype = None
        h.svr_run.argtypes = [_dp, _dp, _ip, _dp, _dp, _dp] + [C.c_int] * 5 + [C.c_double, C.c_int, _dp, _dp, _dp, _dp, _ip, _dp, _ip, _ip]
        h.sv_fma_pub.restype = C.c_double
        h.sv_fma_pub.argtypes = [C.c_double] * 3
        h.sv_fma_vec.restype = None
        h.sv_fma_vec.argtypes = [_dp, _dp, _dp, _dp, C.c_int]
        h.sv_exp_vec.restype = None
        h.sv_exp_vec.argtypes = [_dp, _dp, C.c_int]
        h.sv_counters.restype = None
        h.sv_counters.argtypes = [C.POINTER(C.c_long)]
        h.sv_counters_reset.restype = None
        self.h = h

    def fma(self, a, b, c):
        """element-wise fma(a, b, c), one rounding"""
        if np.ndim(a) == 0 and np.ndim(b) == 0 and np.ndim(c) == 0:
            return self.h.sv_fma_pub(a, b, c)
        a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
        a, b, c = (np.ascontiguousarray(v) for v in (a, b, c))
        o = np.empty(a.shape)
        self.h.sv_fma_vec(a.ctypes.data_as(_dp), b.ctypes.data_as(_dp), c.ctypes.data_as(_dp), o.ctypes.data_as(_dp), a.size)
        return o

    def exp(self, x):
        """element-wise epi_exp"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        o = np.empty(x.shape)
        self.h.sv_exp_vec(x.ctypes.data_as(_dp), o.ctypes.data_as(_dp), x.size)
        return o

    def counters(self, reset=False):
        """what the items since the last reset went through, by COUNTERS"""
        buf = (C.c_long * len(COUNTERS))()
        self.h.sv_counters(buf)
        if reset:
            self.h.sv_counters_reset()
        return dict(zip(COUNTERS, (int(v) for v in buf)))

    def run(self, X, y, n_rows=None, kernel="linear", box=1.0, epsilon=0.1, kernel_scale=1.0, tol=1e-3, max_iter=50000, outputs=None):
        """X [D, F, R], y [D, R] -> the outputs asked for as NumPy arrays (poisoned where the call must write)"""
        X, y = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
        D, F, R = X.shape
        nr = np.ascontiguousarray([D] if n_rows is None else n_rows, dtype=np.int32)
        reg = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (R,))) for v in (box, epsilon, kernel_scale)]
        sh = shapes(D, F, R, len(nr))
        names = out_names(kernel, outputs)
        o = {k: np.full(sh[k], -7 if k in OUT_I32 else -7777.25, dtype=np.int32 if k in OUT_I32 else np.float64) for k in names}
        op = lambda k: None if k not in o else o[k].ctypes.data_as(_ip if k in OUT_I32 else _dp)
        self.h.svr_run(X.ctypes.data_as(_dp), y.ctypes.data_as(_dp), nr.ctypes.data_as(_ip), *(v.ctypes.data_as(_dp) for v in reg),
                       D, F, R, len(nr), KERNELS.index(kernel), float(tol), int(max_iter),
                       op("beta"), op("bias"), op("w"), op("fitted"), op("n_iter"), op("gap"), op("n_sv"), op("status"))
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


# ---- the NumPy reading -------------------------------------------------------------------------------------------------
def kernel_matrix(Xa, Xb, kernel, scale, ref):
    """K(a_t, b_i) [len(Xa), len(Xb)] over f ascending: the first product (square), then fma"""
    a, b = Xa[:, None, :], Xb[None, :, :]
    with np.errstate(all="ignore"):
        if kernel == "gaussian":
            t = a[..., 0] - b[..., 0]
            d = t * t
            for f in range(1, Xa.shape[1]):
                t = a[..., f] - b[..., f]
                d = ref.fma(t, t, d)
            return ref.exp(-(d / (scale * scale)))
        acc = a[..., 0] * b[..., 0]
        for f in range(1, Xa.shape[1]):
            acc = ref.fma(a[..., f], b[..., f], acc)
        return acc


def np_item(Km, Xall, yn, kernel, C_, e, tol, max_iter, ref):
    """one item: Km [D, n] the kernel matrix of all rows against the used ones, Xall [D, F], yn [n] -> dict"""
    n = yn.size
    D = Km.shape[0]
    sgn = np.concatenate([np.ones(n), -np.ones(n)])
    row = np.concatenate([np.arange(n), np.arange(n)])
    a = np.zeros(2 * n)
    G = np.concatenate([e - yn, e + yn])
    QD = np.diagonal(Km[:n]).copy()[row]
    it = 0
    with np.errstate(all="ignore"):
        while True:
            val = -(sgn * G)
            up = np.where(sgn > 0, a < C_, a > 0.0)
            low = np.where(sgn > 0, a > 0.0, a < C_)
            m = np.where(up & ~np.isnan(val), val, -np.inf)
            i = int(np.argmax(m))
            gmax = m[i]
            gmin = np.where(low & ~np.isnan(val), val, np.inf).min()
            gap = gmax - gmin
            if not (gap >= tol) or it == max_iter:
                break
            ci = Km[:n, row[i]][row]
            cur = (QD[i] + QD) - 2.0 * ci
            cur = np.where(cur > 0.0, cur, TAU)
            b = gmax - val
            o = (b * b) / cur
            o = np.where(low & (b > 0.0) & ~np.isnan(o), o, -np.inf)
            j = int(np.argmax(o))
            if o[j] == -np.inf:
                break
            cj = Km[:n, row[j]][row]
            quad = (QD[i] + QD[j]) - 2.0 * ci[j]
            if not quad > 0.0:
                quad = TAU
            ai = ai0 = a[i]
            aj = aj0 = a[j]
            if sgn[i] != sgn[j]:
                delta, diff = (-G[i] - G[j]) / quad, ai - aj
                ai, aj = ai + delta, aj + delta
                if diff > 0.0:
                    if aj < 0.0:
                        aj, ai = 0.0, diff
                elif ai < 0.0:
                    ai, aj = 0.0, -diff
                if diff > 0.0:
                    if ai > C_:
                        ai, aj = C_, C_ - diff
                elif aj > C_:
                    aj, ai = C_, C_ + diff
            else:
                delta, sm = (G[i] - G[j]) / quad, ai + aj
                ai, aj = ai - delta, aj + delta
                if sm > C_:
                    if ai > C_:
                        ai, aj = C_, sm - C_
                elif aj < 0.0:
                    aj, ai = 0.0, sm
                if sm > C_:
                    if aj > C_:
                        aj, ai = C_, sm - C_
                elif ai < 0.0:
                    ai, aj = 0.0, sm
            a[i], a[j] = ai, aj
            G = ref.fma(ci * (sgn * sgn[i]), ai - ai0, G)
            G = ref.fma(cj * (sgn * sgn[j]), aj - aj0, G)
            it += 1
        free = (a > 0.0) & (a < C_)
        if free.any():
            s = 0.0
            for v in np.flatnonzero(free):
                s = s + sgn[v] * G[v]
            bias = -(s / float(free.sum()))
        else:
            bias = (gmax + gmin) * 0.5
        beta = a[:n] - a[n:]
        out = dict(beta=np.concatenate([beta, np.zeros(D - n)]), bias=bias, n_iter=it, gap=gap, n_sv=int((beta != 0.0).sum()))
        if kernel == "linear":
            w = beta[0] * Xall[0]
            for q in range(1, n):
                w = ref.fma(beta[q], Xall[q], w)
            fit = Xall[:, 0] * w[0]
            for f in range(1, Xall.shape[1]):
                fit = ref.fma(Xall[:, f], w[f], fit)
            out["w"] = w
        else:
            fit = beta[0] * Km[:, 0]
            for q in range(1, n):
                fit = ref.fma(beta[q], Km[:, q], fit)
        out["fitted"] = fit + bias
    vals = [out["beta"], out["fitted"], np.asarray([bias, gap])] + ([out["w"]] if kernel == "linear" else [])
    bad = not all(np.isfinite(v).all() for v in vals)
    out["status"] = (0 if gap < tol else NOT_CONVERGED) | (NONFINITE if bad else 0)
    return out


def np_svr(X, y, n_rows, kernel, box, epsilon, kernel_scale, tol, max_iter, ref, regions=None):
    """every output of the call for the regions asked for (default: all); the others stay zero"""
    X, y = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    D, F, R = X.shape
    nr = [D] if n_rows is None else list(n_rows)
    box, epsilon, kernel_scale = (np.broadcast_to(np.asarray(v, dtype=np.float64), (R,)) for v in (box, epsilon, kernel_scale))
    o = {k: np.zeros(s, dtype=np.int32 if k in OUT_I32 else np.float64) for k, s in shapes(D, F, R, len(nr)).items() if k != "w" or kernel == "linear"}
    for r in (range(R) if regions is None else regions):
        C_, e, s = float(box[r]), float(epsilon[r]), float(kernel_scale[r])
        ok = C_ > 0 and np.isfinite(C_) and e >= 0 and np.isfinite(e) and s > 0 and np.isfinite(s)
        Km = kernel_matrix(X[:, :, r], X[:max(nr), :, r], kernel, s, ref) if ok else None
        for k, n in enumerate(nr):
            if not (ok and np.isfinite(X[:n, :, r]).all() and np.isfinite(y[:n, r]).all()):
                for name in o:
                    o[name][k, ..., r] = {"n_iter": 0, "n_sv": 0, "status": BAD_INPUT}.get(name, np.nan)
                continue
            it = np_item(Km[:, :n], X[:, :, r], y[:n, r], kernel, C_, e, tol, max_iter, ref)
            for name in o:
                o[name][k, ..., r] = it[name]
    return o


# ---- the independent check of the optimum ------------------------------------------------------------------------------
def dual_gap(Xn, yn, beta, bias, kernel, scale, C_, e):
    """(primal - dual objective, the primal objective) of (beta, bias) on the rows used, in longdouble with a dense kernel
    matrix of its own (np.exp / matrix products: not the readings' order, not the solver's gradient).
    primal = beta'K beta / 2 + C sum max(0, |y - f| - e), f = K beta + bias;
    dual   = -beta'K beta / 2 - e sum|beta| + y'beta (alpha_i alpha*_i = 0, so alpha + alpha* = |beta|)."""
    L = np.longdouble
    Xl, yl, bl = Xn.astype(L), yn.astype(L), beta.astype(L)
    if kernel == "gaussian":
        d = ((Xl[:, None, :] - Xl[None, :, :]) ** 2).sum(axis=2)
        Kl = np.exp(-d / (L(scale) * L(scale)))
    else:
        Kl = Xl @ Xl.T
    f = Kl @ bl + L(bias)
    quad = bl @ Kl @ bl / 2
    primal = quad + L(C_) * np.maximum(0, np.abs(yl - f) - L(e)).sum()
    dual = -quad - L(e) * np.abs(bl).sum() + yl @ bl
    return float(primal - dual), float(primal)


# ---- the shapes and inputs the suites share: (D, F, n_rows, R) and the kernels ------------------------------------------
CASES = [
    ((2, 1, (1, 2), 1), KERNELS),                                       # the smallest item
    ((9, 3, (5, 9), 63), KERNELS),
    ((66, 7, (63, 64, 65), 2), KERNELS),                                # the wave edge
    ((258, 5, (255, 256, 257), 3), KERNELS),                            # the lane-stride edge: one and two rows a lane
    ((40, 96, (40,), 2), KERNELS),                                      # the F limit
    ((120, 49, (90, 120), 65), KERNELS),
    ((366, 49, (276,), 2), ("linear",)),                                # the workload's item, once
    ((516, 3, (513,), 2), KERNELS),                                     # four rows a lane
]
TOL, MAX_ITER = 1e-3, 50000


def iqr(y):
    """MATLAB's iqr of every column of y [n, R] (quantile at (i - 0.5) / n, linear in between)"""
    s = np.sort(y, axis=0)
    n = s.shape[0]

    def q(p):
        pos = min(max(p * n - 0.5, 0.0), n - 1.0)
        lo = min(int(np.floor(pos)), n - 2) if n > 1 else 0
        return s[lo] + (pos - lo) * (s[min(lo + 1, n - 1)] - s[lo])
    return q(0.75) - q(0.25)


def plans(seed, D, F, R):
    """§4.11's synthetic plans: piecewise-constant integer levels 0 .. mx_f (mx cycling through 3 3 2 4 2 3 2 4 2 3 2 4), the
    switch probability of a region drawn from U(0.02, 0.1), every column divided by its max(abs) (0 -> 1); for F > 1 the last
    column is ones.  y follows a slow wave, the plans' mean and noise.  Returns X [D, F, R], y [D, R]"""
    g = np.random.default_rng(seed)
    mx = np.resize(np.array([3, 3, 2, 4, 2, 3, 2, 4, 2, 3, 2, 4]), F)
    X = np.empty((D, F, R))
    for r in range(R):
        ps = g.uniform(0.02, 0.1)
        lvl = g.integers(0, mx + 1)
        for t in range(D):
            sw = g.random(F) < ps
            lvl = np.where(sw, g.integers(0, mx + 1), lvl)
            X[t, :, r] = lvl
    if F > 1:
        X[:, F - 1, :] = 1.0
    m = np.abs(X).max(axis=0)
    m[m == 0] = 1.0
    X = X / m[None]
    y = 0.05 * np.sin(np.arange(D) / 40.0)[:, None] - 0.02 * X[:, :max(F - 1, 1), :].mean(axis=1) + g.normal(0, 0.01, size=(D, R))
    return X, y


def plant(X, y, box, eps, scale, nmax):
    """the sick and the special regions, for R >= 8.  1: a NaN in the first row of X.  2: box = -1.  3: epsilon above
    max|y - median| (no support vector: n_iter 0, the midpoint bias).  4: the odd rows copy their even neighbours with another
    y (zero curvature: tau; both alpha_k and alpha*_k can leave zero: the same-row pair).  5: a constant y.  6: an Inf in the
    LAST row of X (a BAD_INPUT where that row is used, a NONFINITE prediction where it is not).  7: kernel_scale = 0.
    8 (R >= 9): a small box and epsilon = 0: every variable ends on a bound or free with clips on the way"""
    D, F, R = X.shape
    if R < 8:
        if R >= 2:                                                       # small cases: region 1 gets the duplicated rows
            X[1:nmax:2, :, 1] = X[0:nmax - 1:2, :, 1][:len(X[1:nmax:2, :, 1])]
        return
    X[0, 0, 1] = np.nan
    box[2] = -1.0
    eps[3] = 2.0 * np.abs(y[:, 3] - np.median(y[:, 3])).max() + 1.0
    X[1:nmax:2, :, 4] = X[0:nmax - 1:2, :, 4][:len(X[1:nmax:2, :, 4])]
    y[1:nmax:2, 4] = -y[1:nmax:2, 4]
    y[:, 5] = 0.03125
    X[D - 1, 0, 6] = np.inf
    scale[7] = 0.0
    if R >= 9:
        box[8] = box[8] * 0.05
        eps[8] = 0.0


@functools.lru_cache(maxsize=None)
def problem(i):
    """case i of CASES with its planted inputs: dict X, y, n_rows, box, epsilon, kernel_scale (per region); shared, read-only.
    box = iqr / 1.349 times 1, 4 or 16 by region, epsilon = iqr / 13.49, kernel_scale = 1, 1.5, 2 or 2.5 by region"""
    (D, F, nr, R), _ = CASES[i]
    X, y = plans(300 + i, D, F, R)
    q = iqr(y[:max(nr)])
    q = np.where(q > 0, q, 0.1)
    box, eps = q / 1.349 * 4.0 ** (np.arange(R) % 3), q / 13.49
    scale = 1.0 + 0.5 * (np.arange(R) % 4)
    if (D, F) == (366, 49):
        box = q / 1.349                                                  # the workload's item: C = iqr / 1.349
    plant(X, y, box, eps, scale, max(nr))
    p = dict(X=X, y=y, n_rows=nr, box=box, epsilon=eps, kernel_scale=scale)
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p


def run_kw(p, kernel, **kw):
    """the keyword arguments of SvrRef.run / batch.svr / hostapi.svr for problem p"""
    d = dict(n_rows=p["n_rows"], kernel=kernel, box=p["box"], epsilon=p["epsilon"], kernel_scale=p["kernel_scale"], tol=TOL, max_iter=MAX_ITER)
    d.update(kw)
    return d

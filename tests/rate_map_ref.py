"""The NPI-to-growth-rate predictor (csrc/rate_map.hpp) restated twice: the loader of tests/rate_map_ref.c,
the bit-exact C yardstick, and `np_rate_map`, a NumPy loop reading of testScripts/test04FullFeatureExtMLpipeline.m
(:292-404, :418-431, :576-642) that keeps the script's own shape -- the feature matrix is built whole, the tracker is the
script's O(T^2) loop over index ranges, the forward substitution is a pass of its own -- in the operation order §4.11 pins.
Both must agree bit for bit.  Also here: the shapes and planted inputs the CPU and GPU suites share.

The test modules build the C twin in a session fixture: `RatemapRef(tmp_path_factory.mktemp("ratemap"))`."""
from __future__ import annotations

import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "rate_map_ref.c")

LEADING_NAN, NOT_PD, NONFINITE = 1, 2, 4
OUT_NAMES = ("map", "x_mx", "y_filled", "lambda_hat", "new_cases_est", "tracker", "status")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


def shapes(T, n, R, E, K, n_lags):
    F = n * (1 + n_lags) + E
    return {"map": (K, F, R), "x_mx": (F, R), "y_filled": (T, R), "lambda_hat": (K, T, R), "new_cases_est": (K, T, R),
            "tracker": (T, R), "status": (K, R)}


class RatemapRef:
    """tests/rate_map_ref.c behind ctypes"""

    def __init__(self, build_dir):
        cc = shutil.which("gcc") or shutil.which("cc")
        if cc is None:
            raise RuntimeError("no C compiler for tests/rate_map_ref.c")
        so = os.path.join(str(build_dir), "libratemap_ref.so")
        subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", so, "-lm"])
        h = C.CDLL(so)
        h.ratemap_run.restype = None
        h.ratemap_run.argtypes = [_dp] * 5 + [_ip, _ip] + [C.c_int] * 8 + [C.c_double] * 3 + [_dp] * 6 + [_ip]
        h.rm_exp_pub.restype = C.c_double
        h.rm_exp_pub.argtypes = [C.c_double]
        h.rm_fma_pub.restype = C.c_double
        h.rm_fma_pub.argtypes = [C.c_double] * 3
        h.rm_fma_vec.restype = None
        h.rm_fma_vec.argtypes = [_dp, _dp, _dp, _dp, C.c_int]
        self.h = h

    def exp(self, v):
        return self.h.rm_exp_pub(float(v))

    def fma(self, a, b, c):
        """element-wise fma(a, b, c), one rounding"""
        if np.ndim(a) == 0 and np.ndim(b) == 0 and np.ndim(c) == 0:
            return self.h.rm_fma_pub(a, b, c)
        a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
        a, b, c = (np.ascontiguousarray(v) for v in (a, b, c))
        o = np.empty(a.shape)
        self.h.rm_fma_vec(a.ctypes.data_as(_dp), b.ctypes.data_as(_dp), c.ctypes.data_as(_dp), o.ctypes.data_as(_dp), a.size)
        return o

    def run(self, p, outputs=OUT_NAMES):
        """p: a problem dict (see `problem`) -> the outputs asked for as NumPy arrays"""
        ip = np.ascontiguousarray(p["ip"], dtype=np.float64)
        T, n, R = ip.shape
        lags = np.ascontiguousarray(list(p["lags"]) + [0] * (3 - len(p["lags"])), dtype=np.int32)
        nt = np.ascontiguousarray(p["n_train"], dtype=np.int32)
        K, E = len(nt), 0 if p.get("extra") is None else p["extra"].shape[1]
        sh = shapes(T, n, R, E, K, len(p["lags"]))
        o = {k: np.full(sh[k], -7 if k == "status" else -7777.25, dtype=np.int32 if k == "status" else np.float64)
             for k in outputs}
        keep = [np.ascontiguousarray(p[k], dtype=np.float64) if p.get(k) is not None else None for k in ("y", "new_smoothed", "extra", "lambda_in")]
        ptr = lambda a: None if a is None else a.ctypes.data_as(_dp)
        op = lambda k: None if k not in o else o[k].ctypes.data_as(_ip if k == "status" else _dp)
        self.h.ratemap_run(ip.ctypes.data_as(_dp), ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), nt.ctypes.data_as(_ip),
                           lags.ctypes.data_as(_ip), T, n, R, E, K, len(p["lags"]), int(p["fit"]), int(p["effect_lag"]),
                           float(p["ridge"]), float(p["thr"]), float(p["red"]),
                           op("map"), op("x_mx"), op("y_filled"), op("lambda_hat"), op("new_cases_est"), op("tracker"), op("status"))
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


# ---- NumPy loop reading of the .m lines (one region at a time) -------------------------------------------------------
def features(ip_r, lags, extra_r):
    """:355 AllFeatures = [IP, lagged(lag1), .., extra] for one region: ip_r [T, n], extra_r [T, E] or None"""
    T = ip_r.shape[0]
    blocks = [ip_r]
    for lag in lags:
        blocks.append(np.vstack([np.zeros((lag, ip_r.shape[1])), ip_r[:T - lag]]))
    if extra_r is not None:
        blocks.append(extra_r)
    return np.hstack(blocks)


def chol_solve(G, c, fma):
    """G m = c by unblocked lower Cholesky, forward and back substitution in the order of DESIGN.md §4.11: every dot
    acc = a0 b0; acc = fma(a_k, b_k, acc) with k ascending, one subtraction, one division per L(i,j), sqrt per pivot; the
    back substitution by columns, k descending.  Returns (m, ok)."""
    F = len(c)
    L = np.zeros((F, F))

    def dot(u, v):
        u, v = u.tolist(), v.tolist()
        d = u[0] * v[0]
        for k in range(1, len(u)):
            d = fma(u[k], v[k], d)
        return d

    for j in range(F):
        piv = G[j, j] - dot(L[j, :j], L[j, :j]) if j else G[j, j]
        if not (piv > 0.0) or piv == np.inf:
            return None, False
        L[j, j] = np.sqrt(piv)
        if j + 1 < F:
            v = G[j + 1:, j].copy()
            if j:
                d = L[j + 1:, 0] * L[j, 0]
                for k in range(1, j):
                    d = fma(L[j + 1:, k], L[j, k], d)
                v = v - d
            L[j + 1:, j] = v / L[j, j]
    z = np.zeros(F)
    for i in range(F):
        z[i] = (c[i] - dot(L[i, :i], z[:i]) if i else c[i]) / L[i, i]
    m, s = np.zeros(F), z.copy()
    for k in range(F - 1, -1, -1):
        m[k] = s[k] / L[k, k]
        if k:
            s[:k] = fma(-L[k, :k], m[k], s[:k])
    return m, True


def np_rate_map(p, fma, exp):
    """every output of the call for the problem dict p; fma / exp: RatemapRef.fma / .exp"""
    ip, ns, lags = np.asarray(p["ip"], dtype=np.float64), np.asarray(p["new_smoothed"], dtype=np.float64), list(p["lags"])
    T, n, R = ip.shape
    extra = p.get("extra")
    E, K, fit = 0 if extra is None else extra.shape[1], len(p["n_train"]), int(p["fit"])
    o = {k: np.full(s, np.nan) for k, s in shapes(T, n, R, E, K, len(lags)).items()}
    o["status"] = np.zeros((K, R), dtype=np.int32)
    with np.errstate(all="ignore"):
        for r in range(R):
            X = features(ip[:, :, r], lags, None if extra is None else np.asarray(extra, dtype=np.float64)[:, :, r])
            F = X.shape[1]
            # :375-377
            x_mx = np.array([np.nan if np.isnan(X[:, f]).all() else np.nanmax(np.abs(X[:, f])) for f in range(F)])
            x_mx[x_mx == 0] = 1.0
            o["x_mx"][:, r] = x_mx
            Xn = X / x_mx[None, :]
            # :305-311
            yf = None
            if p.get("y") is not None:
                yf = np.asarray(p["y"], dtype=np.float64)[:, r].copy()
                for jj in range(1, T):
                    if np.isnan(yf[jj]) or np.isinf(yf[jj]):
                        yf[jj] = yf[jj - 1]
                o["y_filled"][:, r] = yf
            # :418-431, the script's loop over index ranges
            avg = ip[:, 0, r].copy()
            for q in range(1, n):
                avg = avg + ip[:, q, r]
            avg = avg / float(n)
            inc = np.zeros(T)
            for ii in range(2, T + 1):                                  # MATLAB's 1-based day
                first = min(ii + int(p["effect_lag"]), T)
                if avg[ii - 1] > avg[ii - 2]:
                    inc[first - 1:] = inc[first - 1:] - p["red"]
                elif avg[ii - 1] < avg[ii - 2]:
                    inc[first - 1:] = inc[first - 1:] + p["red"]
            o["tracker"][:, r] = inc
            for k, nt in enumerate(p["n_train"]):
                if fit:
                    if np.isnan(yf[0]):
                        o["status"][k, r] = LEADING_NAN
                        continue
                    # :396-402: every entry of X'X and X'y one chain over the days ascending
                    aug = np.hstack([Xn[:nt], yf[:nt, None]])           # [nt, F + 1]
                    acc = aug[0][:, None] * aug[0][None, :F]
                    for t in range(1, nt):
                        acc = fma(aug[t][:, None], aug[t][None, :F], acc)
                    G, c = acc[:F].copy(), acc[F].copy()
                    G[np.arange(F), np.arange(F)] = G[np.arange(F), np.arange(F)] + p["ridge"]
                    m, ok = chol_solve(G, c, fma)
                    if not ok:
                        o["status"][k, r] = NOT_PD
                        continue
                    o["map"][k, :, r] = m
                    pred = Xn[nt:, 0] * m[0]
                    for f in range(1, F):
                        pred = fma(Xn[nt:, f], m[f], pred)
                    lam = np.concatenate([yf[:nt], pred])
                else:
                    lam = np.asarray(p["lambda_in"], dtype=np.float64)[k, :, r].copy()
                # :578-584
                counter = np.arange(1, T + 1)
                i_pos, i_neg = (lam > p["thr"]) & (counter > nt), (lam < -p["thr"]) & (counter > nt)
                lam[i_pos], lam[i_neg] = p["thr"], -p["thr"]
                # :627-632
                est, cum = ns[:, r].copy(), 0.0
                for t in range(nt, T):
                    cum = cum + lam[t]
                    est[t] = ns[nt - 1, r] * exp(cum)
                o["lambda_hat"][k, :, r], o["new_cases_est"][k, :, r] = lam, est
                bad = not (np.isfinite(lam).all() and np.isfinite(est).all() and (not fit or np.isfinite(o["map"][k, :, r]).all()))
                o["status"][k, r] = NONFINITE if bad else 0
    if not fit:
        del o["map"]
    if p.get("y") is None:
        del o["y_filled"]
    return o


# ---- the shapes and inputs the suites share: (T, n, lags, E, K, R) and the train ends -------------------------------
CASES = [
    ((8, 1, (), 0, 1, 1), (6,)),
    ((9, 3, (1,), 0, 2, 63), (4, 8)),
    ((12, 12, (3, 5, 7), 0, 3, 64), (1, 7, 12)),                        # a lag >= the train end: all-zero training columns
    ((40, 16, (3, 5, 7), 1, 2, 65), (25, 39)),                          # F = 65
    ((30, 22, (3, 5, 7), 8, 1, 2), (20,)),                              # F = 96
    ((20, 24, (), 0, 1, 3), (15,)),
    ((366, 12, (3, 5, 7), 0, 4, 5), (30, 120, 275, 366)),
]


def make_case(seed, T, n, lags, E, K, R, n_train, fit=1, ridge=1e-6):
    """piecewise-constant plans, a rate that follows them plus noise, smoothed cases; nothing planted"""
    g = np.random.default_rng(seed)
    ip = np.empty((T, n, R))
    lvl = g.integers(0, 5, size=(n, R)).astype(np.float64)
    for t in range(T):
        sw = g.random((n, R)) < 0.1
        lvl = np.where(sw, g.integers(0, 5, size=(n, R)), lvl)
        ip[t] = lvl
    w = g.normal(0, 0.03, size=(n, R))
    y = 0.15 - np.einsum("tnr,nr->tr", ip, np.abs(w)) + g.normal(0, 0.05, size=(T, R))
    ns = 50.0 + 500.0 * g.random((T, R))
    extra = None
    if E:
        extra = g.normal(0, 1, size=(T, E, R))
        extra[:, 0, :] = 1.0                                            # test05's ones column
    p = dict(ip=ip, y=y, new_smoothed=ns, extra=extra, lambda_in=None, n_train=tuple(n_train), lags=tuple(lags), fit=fit,
             effect_lag=3, ridge=ridge, thr=0.1, red=0.01)
    if not fit:
        p["lambda_in"] = 0.12 * g.normal(0, 1, size=(K, T, R))
    return p


def plant(p):
    """the sick inputs: region 0 a constant plan, a zero plan and NaN / Inf targets in the middle and at the end; region 1 a
    leading-NaN target; the last region (R >= 3) a NaN plan on day 1, so a pivot is NaN (NOT_PD); region 2 (R >= 4) an Inf
    first target, which stays and propagates"""
    T, n, R = p["ip"].shape
    p["ip"][:, 0, 0] = 2.0
    if n >= 2:
        p["ip"][:, n - 1, 0] = 0.0
    if T > 5:
        p["y"][2, 0], p["y"][3, 0], p["y"][T - 1, 0] = np.nan, np.inf, np.nan
    if R >= 2:
        p["y"][0, 1] = np.nan
    if R >= 3:
        p["ip"][0, 0, R - 1] = np.nan
    if R >= 4:
        p["y"][0, 2] = np.inf
    if p["lambda_in"] is not None:
        p["lambda_in"][:, T // 2, 0] = np.nan
        p["lambda_in"][:, T - 1, R - 1] = np.inf
    return p


@functools.lru_cache(maxsize=None)
def problem(i, fit=1):
    """case i of CASES with its planted inputs; shared and read-only"""
    (T, n, lags, E, K, R), nt = CASES[i]
    p = plant(make_case(100 + i, T, n, lags, E, K, R, nt, fit=fit))
    for v in p.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p

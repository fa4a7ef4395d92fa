"""Loader of tests/ar_forecast_ref.c, the independent C restatement of the autoregressive alpha forecaster (the bit-exact
yardstick of csrc/ar_forecast.hpp), plus a plain NumPy reading of the same definition that checks it:
np.linalg.lstsq on the same stacked forward-backward matrix, scipy.signal.lfiltic / lfilter where scipy imports (else the
direct loop), the clamp and SI_Controlled.

The test modules build the C reading in a session fixture: `ArRef(tmp_path_factory.mktemp("arfc"))`."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "ar_forecast_ref.c")

ST_OK, ST_RANK_DEFICIENT, ST_BAD_INPUT = range(3)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


def _p(a, t=_dp):
    return None if a is None else a.ctypes.data_as(t)


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


class ArRef:
    def __init__(self, build_dir):
        cc = shutil.which("gcc") or shutil.which("cc")
        if cc is None:
            raise RuntimeError("no C compiler for tests/ar_forecast_ref.c")
        so = os.path.join(str(build_dir), "libar_forecast_ref.so")
        subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", so, "-lm"])
        h = C.CDLL(so)
        h.arf_fit.restype = C.c_int
        h.arf_fit.argtypes = [_dp, C.c_int, C.c_int, C.c_int, _dp, _dp]
        h.arf_run.restype = None
        h.arf_run.argtypes = [_dp] * 6 + [_ip, _dp, _dp] + [C.c_int] * 8 + [C.c_double, _dp, _dp, _dp, _ip]
        self.h = h

    def fit(self, y, p, nv_mode=0):
        """one region: y [L] -> (a [p], noise variance, status)"""
        y = _f64(y)
        a, nv = np.empty(int(p)), np.empty(1)
        st = self.h.arf_fit(_p(y), len(y), int(p), int(nv_mode), _p(a), _p(nv))
        return a, float(nv[0]), st

    def run(self, seg, beta, s0, i0, dt, p, H, D, z=None, drive=None, drive_series=None, A=None, noise_var=None, nv_mode=0):
        """the arguments of batch.ar_forecast as NumPy arrays -> dict S [K, 3, B], A [p, R], noise_var [R], status [R]"""
        seg = _f64(seg)
        L, R = seg.shape
        B, K = R * int(D), L + int(H)
        beta, s0, i0, z, drive, A, noise_var = (_f64(v) for v in (beta, s0, i0, z, drive, A, noise_var))
        ser = None if drive_series is None else np.ascontiguousarray(drive_series, dtype=np.int32)
        Sd = 0 if drive is None else drive.shape[1]
        out = dict(S=np.empty((K, 3, B)), A=np.empty((int(p), R)), noise_var=np.empty(R), status=np.empty(R, dtype=np.int32))
        self.h.arf_run(_p(seg), _p(beta), _p(s0), _p(i0), _p(z), _p(drive), _p(ser, _ip), _p(A), _p(noise_var), R, int(D), L,
                       int(p), int(H), Sd, int(A is None), int(nv_mode), float(dt), _p(out["S"]), _p(out["A"]),
                       _p(out["noise_var"]), _p(out["status"], _ip))
        return out


# ---- the plain NumPy reading (one region) ---------------------------------------------------------------------------
def stacked(y, p):
    """the forward-backward system of DESIGN.md §4.8: X [2 (L - p), p], b [2 (L - p)]; the model minimises |b + X a|"""
    y = np.asarray(y, dtype=np.float64)
    L = len(y)
    t = np.arange(p, L)
    Xf = np.stack([y[t - k] for k in range(1, p + 1)], axis=1)
    Xb = np.stack([y[t - p + k] for k in range(1, p + 1)], axis=1)
    return np.concatenate([Xf, Xb]), np.concatenate([y[t], y[t - p]])


def np_fit(y, p, nv_mode=0):
    """-> a [p], noise variance, rank of the stacked matrix as NumPy reports it"""
    X, b = stacked(y, p)
    a, _, rank, _ = np.linalg.lstsq(X, -b, rcond=None)
    n = len(y) - p
    e = b + X @ a
    frss, brss = float(e[:n] @ e[:n]), float(e[n:] @ e[n:])
    return a, ((frss + brss) / (2 * n) if nv_mode == 0 else frss / n), int(rank)


def np_continue(y, a, nv, H, z=None):
    """filter(sqrt(nv), [1, a], z, filtic(sqrt(nv), [1, a], y(end:-1:1))) -> [H]"""
    y, a = np.asarray(y, dtype=np.float64), np.asarray(a, dtype=np.float64)
    z = np.zeros(H) if z is None else np.asarray(z, dtype=np.float64)
    b0 = np.sqrt(nv)
    try:
        from scipy.signal import lfilter, lfiltic
        den = np.concatenate([[1.0], a])
        zi = lfiltic([b0], den, y[::-1][:len(a)])
        return lfilter([b0], den, z, zi=zi)[0]
    except ImportError:
        w = list(y)
        for t in range(H):
            w.append(b0 * z[t] - sum(a[k - 1] * w[-k] for k in range(1, len(a) + 1)))
        return np.array(w[len(y):])


def np_si_controlled(alpha, beta, s0, i0, K, dt):
    """Tools/SI_Controlled.m:12-22"""
    s, i = np.zeros(K), np.zeros(K)
    s[0], i[0] = s0, i0
    for t in range(K - 1):
        s[t + 1] = max(0.0, min(1.0, s[t] - dt * alpha[t] * s[t] * i[t]))
        i[t + 1] = max(0.0, min(1.0, i[t] + dt * (alpha[t] * s[t] * i[t] - beta * i[t])))
    return s, i


def np_chain(y, a, nv, H, beta, s0, i0, dt, z=None, drive=None):
    """one chain -> S [K, 3]"""
    yp = np_continue(y, a, nv, H, z)
    if drive is not None:
        yp = yp + np.asarray(drive, dtype=np.float64)
    al = np.concatenate([np.asarray(y, dtype=np.float64), yp])
    al[al < 0] = 0.0
    s, i = np_si_controlled(al, beta, s0, i0, len(al), dt)
    return np.stack([s, i, al], axis=1)


# ---- test series ----------------------------------------------------------------------------------------------------
def ar_series(coefs, L, seed, noise=1.0, burn=200, offset=0.0):
    """a realisation of y(t) = -sum a_k y(t-k) + noise * e(t) (a = coefs, MATLAB's sign), after a burn-in"""
    rng = np.random.default_rng(seed)
    p = len(coefs)
    w = list(rng.standard_normal(p))
    for _ in range(burn + L):
        w.append(noise * rng.standard_normal() - sum(coefs[k] * w[-1 - k] for k in range(p)))
    return np.array(w[-L:]) + offset


def same(a, b):
    """equal as values, NaN matching NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())

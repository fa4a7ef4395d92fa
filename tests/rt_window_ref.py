"""Loader of tests/rt_window_ref.c, the independent C restatement of the sliding-window growth-rate estimators (the bit-exact
yardstick of csrc/rt_window.hpp), plus plain NumPy loop readings of the three .m files that check it.

The test modules build it in a session fixture: `RtWindowRef(tmp_path_factory.mktemp("rtwin"))`."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "rt_window_ref.c")

ST_OUTSIDE, ST_TOLX, ST_TOLFUN, ST_MAXITER, ST_STALL, ST_SKIPPED, ST_MODEL_ERROR = range(7)
LLR = ("Rt", "A", "Lambda", "ExpFit")
GR = ("Rt", "Lambda", "RtSmoothed", "LambdaSmoothed")
NLS = ("Rt", "A", "Lambda", "ExpFit", "status", "iters")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


class RtWindowRef:
    def __init__(self, build_dir):
        cc = shutil.which("gcc") or shutil.which("cc")
        if cc is None:
            raise RuntimeError("no C compiler for tests/rt_window_ref.c")
        so = os.path.join(str(build_dir), "librt_window_ref.so")
        subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", so, "-lm"])
        h = C.CDLL(so)
        h.rw_exp.restype = h.rw_log.restype = C.c_double
        h.rw_exp.argtypes = h.rw_log.argtypes = [C.c_double]
        h.rw_loglinreg.argtypes = [_dp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int] + [_dp] * 4
        h.rw_genratios.argtypes = [_dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double] + [_dp] * 4
        h.rw_nonlinls.argtypes = [_dp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int] + [_dp] * 4 + [_ip] * 2
        self.h = h

    def log(self, v):
        return self.h.rw_log(float(v))

    def exp(self, v):
        return self.h.rw_exp(float(v))

    @staticmethod
    def _cols(x):
        x = np.asarray(x, dtype=np.float64)
        return x.reshape(-1, 1) if x.ndim == 1 else x

    def loglinreg(self, x, wlen, time_unit=1.0, causal=1):
        """x [L] or [L, R] -> dict Rt, A, Lambda, ExpFit of the same shape"""
        X = self._cols(x)
        L, R = X.shape
        out = {k: np.empty((L, R)) for k in LLR}
        for r in range(R):
            col = np.ascontiguousarray(X[:, r])
            o = {k: np.empty(L) for k in LLR}
            self.h.rw_loglinreg(col.ctypes.data_as(_dp), 1, L, int(wlen), float(time_unit), int(causal),
                                *[o[k].ctypes.data_as(_dp) for k in LLR])
            for k in LLR:
                out[k][:, r] = o[k]
        return {k: v.reshape(np.shape(x)) for k, v in out.items()}

    def genratios(self, x, wlen, generation_period, time_unit=1.0):
        X = self._cols(x)
        L, R = X.shape
        out = {k: np.empty((L, R)) for k in GR}
        for r in range(R):
            col = np.ascontiguousarray(X[:, r])
            o = {k: np.empty(L) for k in GR}
            self.h.rw_genratios(col.ctypes.data_as(_dp), 1, L, int(wlen), int(generation_period), float(time_unit),
                                *[o[k].ctypes.data_as(_dp) for k in GR])
            for k in GR:
                out[k][:, r] = o[k]
        return {k: v.reshape(np.shape(x)) for k, v in out.items()}

    def nonlinls(self, x, wlen, time_unit=1.0, causal=1):
        X = self._cols(x)
        L, R = X.shape
        out = {k: np.empty((L, R)) for k in NLS[:4]}
        out.update(status=np.empty((L, R), dtype=np.int32), iters=np.empty((L, R), dtype=np.int32))
        for r in range(R):
            col = np.ascontiguousarray(X[:, r])
            o = {k: np.empty(L) for k in NLS[:4]}
            o.update(status=np.empty(L, dtype=np.int32), iters=np.empty(L, dtype=np.int32))
            self.h.rw_nonlinls(col.ctypes.data_as(_dp), 1, L, int(wlen), float(time_unit), int(causal),
                               *[o[k].ctypes.data_as(_dp) for k in NLS[:4]], o["status"].ctypes.data_as(_ip),
                               o["iters"].ctypes.data_as(_ip))
            for k in NLS:
                out[k][:, r] = o[k]
        return {k: v.reshape(np.shape(x)) for k, v in out.items()}

    def all(self, x, wlen, time_unit=1.0, causal=1, generation_period=3):
        """the three estimators on x [L, R], keyed like batch.rt_window's result"""
        res = {}
        for k, v in self.loglinreg(x, wlen, time_unit, causal).items():
            res["llr_" + k] = v
        for k, v in self.genratios(x, wlen, generation_period, time_unit).items():
            res["gr_" + k] = v
        for k, v in self.nonlinls(x, wlen, time_unit, causal).items():
            res["nls_" + k] = v
        return res


# ---- plain NumPy loop readings of the .m files (1-based indices kept in the comments) ----
def np_loglinreg(x, wlen, time_unit=1.0, causal=1):
    x = np.asarray(x, dtype=np.float64).ravel()
    L = len(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        lg = np.log(x)
    ALog, r = np.zeros(L), np.zeros(L)
    if causal == 1:
        n = np.arange(-wlen + 1, 1, dtype=np.float64)
        days = range(wlen, L + 1)
        seg_of = lambda mm: lg[mm - wlen:mm]
    else:
        h = wlen // 2
        n = np.arange(-h, h + 1, dtype=np.float64)
        days = range(h + 1, L - h + 1)
        seg_of = lambda mm: lg[mm - h - 1:mm + h]
    En, En2 = n.mean(), (n ** 2).mean()
    Det = En2 - En ** 2
    for mm in days:
        seg = seg_of(mm)
        with np.errstate(invalid="ignore"):
            ALog[mm - 1] = (seg.mean() * En2 - (n * seg).mean() * En) / Det
            r[mm - 1] = ((n * seg).mean() - seg.mean() * En) / Det
    A, Rt = np.exp(ALog), np.exp(r)
    return {"Rt": Rt, "A": A, "Lambda": r / time_unit, "ExpFit": A * Rt}


def np_genratios(x, wlen, gp, time_unit=1.0):
    x = np.asarray(x, dtype=np.float64).ravel()
    L = len(x)
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = np.concatenate([np.zeros(gp), np.log(x[gp:] / x[:L - gp])]) / gp
    sm = np.zeros(L)
    for t in range(L):                        # filter(ones(1,wlen), wlen, .)
        sm[t] = sum(lam[t - k] / wlen for k in range(wlen) if t - k >= 0)
    return {"Rt": np.exp(lam * time_unit), "Lambda": lam, "RtSmoothed": np.exp(sm * time_unit), "LambdaSmoothed": sm}

"""Loader of tests/loglik_ref.c, the bit-exact C yardstick of the innovation log-likelihood, and np_loglik, a
plain NumPy reading of the same definition that keeps the replay of the adaptive R as the filter's `cat`-style windows
(GenericExtendedKalmanFilter.m:172-185).  The two must agree bit for bit (tests/test_loglik_ref.py); the kernel is held to them.

A *case* is a dict of one filter run in the classic layout: model, B, T, L, obs_type, S_MINUS [T, m, B], P_MINUS [T, m*m, B],
innovations [T, B], K_GAIN [T, m, B], x [T, Sx], R_series [T, Sx] or R_scalar [B], x_series [B] or None, prm [61, B]
(case_of(workload, oracle outputs)).  The test modules build the C file in a fixture: `LoglikRef(tmp_path_factory.mktemp(..))`."""
from __future__ import annotations

import copy
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np

from epidemicmodeling_amd import layout as L

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "loglik_ref.c")
LOG2PI = 1.8378770664093453
DBL_MIN = 2.2250738585072014e-308
PER_CHAIN, PER_DAY, SELECT = ("loglik", "nis_mean", "n_valid", "status"), ("S", "nis", "R_used"), ("best", "best_loglik")
ALL = PER_CHAIN + PER_DAY + SELECT
WINDOWS = [(0, None), (5, 40), (32, 45), (44, 45)]


def same_bits(a, b):
    """equal shapes and dtypes, and every element the same number or both NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))


def model_info(model):
    """(m, flip, generic, obs is fixed to NEWCASES)"""
    return L.MODEL_DIM[model], "Backward" in model, not model.startswith("NewCase"), model.endswith("_codegen")


def case_of(w, out):
    return dict(model=w.model, B=w.B, T=w.T, L=w.L, obs_type=w.obs_type, S_MINUS=out["S_MINUS"], P_MINUS=out["P_MINUS"],
                innovations=out["innovations"], K_GAIN=out["K_GAIN"], x=w.x, R_series=w.R_series, R_scalar=w.R_scalar,
                x_series=w.x_series, prm=w.prm)


def stored(case, storage):
    """the case as a runner with float storage leaves it: S_MINUS, P_MINUS, innovations rounded once"""
    if storage == "f64":
        return case
    c = dict(case)
    with np.errstate(over="ignore"):                         # a covariance beyond float's range is stored as Inf
        for k in ("S_MINUS", "P_MINUS", "innovations"):
            c[k] = case[k].astype(np.float32).astype(np.float64)
    return c


def to_blocked(a, blk, fill=np.nan):
    """classic [T, rows, B] ([T, B]) -> chain-blocked [T, nblk, rows, blk] ([T, nblk * blk]); padding lanes hold `fill`"""
    one = a.ndim == 2
    a3 = a[:, None, :] if one else a
    T, rows, B = a3.shape
    nblk = (B + blk - 1) // blk
    p = np.full((T, rows, nblk * blk), fill, dtype=a.dtype)
    p[:, :, :B] = a3
    p = np.ascontiguousarray(p.reshape(T, rows, nblk, blk).transpose(0, 2, 1, 3))
    return np.ascontiguousarray(p.transpose(0, 2, 1, 3).reshape(T, nblk * blk)) if one else p


class LoglikRef:
    def __init__(self, build_dir):
        cc = shutil.which("gcc") or shutil.which("cc")
        if cc is None:
            raise RuntimeError("no C compiler for tests/loglik_ref.c")
        so = os.path.join(str(build_dir), "libloglik_ref.so")
        subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", SRC, "-o", so, "-lm"])
        h = C.CDLL(so)
        h.llr_fma.restype = h.llr_log.restype = C.c_double
        h.llr_fma.argtypes, h.llr_log.argtypes = [C.c_double] * 3, [C.c_double]
        h.llr_run.argtypes = [C.c_int] * 12 + [C.c_void_p] * 17
        h.llr_run.restype = h.llr_select.restype = None
        h.llr_select.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 5
        self.h = h

    def fma(self, a, b, c):
        return self.h.llr_fma(float(a), float(b), float(c))

    def log(self, v):
        return self.h.llr_log(float(v))

    def run(self, case, k0=0, k1=None, storage="f64", G=0):
        """every output of the call, and PCt [T, 3, B] (P- C' of the valid days, for the gain identity)"""
        cs = stored(case, storage)
        m, flip, generic, fixed = model_info(cs["model"])
        B, T = cs["B"], cs["T"]
        keep = []

        def p(a, dt=np.float64):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dt)
            keep.append(a)
            return a.ctypes.data
        out = {k: np.empty(B, dtype=np.int32 if k in ("n_valid", "status") else np.float64) for k in PER_CHAIN}
        out.update({k: np.empty((T, B)) for k in PER_DAY})
        out["PCt"] = np.empty((T, 3, B))
        self.h.llr_run(m, int(flip), int(generic), int(fixed or cs["obs_type"] == "NEWCASES"), B, T, cs["L"], cs["x"].shape[1],
                       int(cs["R_series"] is not None), int(k0), T if k1 is None else int(k1), int(storage == "f32"),
                       p(cs["S_MINUS"]), p(cs["P_MINUS"]), p(cs["innovations"]), p(cs["x"]), p(cs["R_series"]), p(cs["R_scalar"]),
                       p(cs["x_series"], np.int32), p(cs["prm"][L.PRM_GAMMA_EKF]), p(cs["prm"][L.PRM_BETA_EKF]),
                       *[out[k].ctypes.data for k in PER_CHAIN + PER_DAY + ("PCt",)])
        if G:
            out["best"], out["best_loglik"] = np.empty(B // G, dtype=np.int32), np.empty(B // G)
            self.h.llr_select(B // G, G, *[out[k].ctypes.data for k in ("loglik", "n_valid", "status", "best", "best_loglik")])
        return out


def np_select(loglik, n_valid, status, G):
    """NumPy's first-maximum rule over the usable candidates of every region"""
    R = loglik.size // G
    best, bl = np.full(R, -1, dtype=np.int32), np.full(R, np.nan)
    for r in range(R):
        sl = slice(r * G, (r + 1) * G)
        ok = np.flatnonzero(((status[sl] & 1) == 0) & (n_valid[sl] > 0))
        if ok.size:
            best[r] = ok[np.argmax(loglik[sl][ok])]
            bl[r] = loglik[sl][best[r]]
    return best, bl


def np_loglik(ref, case, k0=0, k1=None, storage="f64", G=0):
    """The definition read again in NumPy, a chain and a day at a time; `ref` lends fma and the fixed-order log."""
    cs = stored(case, storage)
    m, flip, generic, fixed = model_info(cs["model"])
    B, T, Lw = cs["B"], cs["T"], cs["L"]
    k1 = T if k1 is None else k1
    newcases = fixed or cs["obs_type"] == "NEWCASES"
    out = {k: np.empty(B, dtype=np.int32 if k in ("n_valid", "status") else np.float64) for k in PER_CHAIN}
    out.update({k: np.full((T, B), np.nan) for k in PER_DAY})
    fma = ref.fma
    for c in range(B):
        sx = c if cs["x_series"] is None else int(cs["x_series"][c])
        gamma, beta = float(cs["prm"][L.PRM_GAMMA_EKF, c]), float(cs["prm"][L.PRM_BETA_EKF, c])
        # ---- R(k) of every filter step
        R = np.empty(T)
        if cs["R_series"] is not None:
            R[:] = cs["R_series"][:, sx]
        else:
            Rv = float(cs["R_scalar"][c])
            R[:] = Rv if generic else np.nan
            R[0] = Rv
            mean_win, cov_win = np.zeros(Lw), np.zeros(Lw)
            for k in range(T):
                t = T - 1 - k if flip else k
                e = float(cs["innovations"][t, c])
                cnt = min(k + 1, Lw)
                mean_win = np.concatenate(([e], mean_win[:Lw - 1]))          # cat(2, innovations(:, k), InnovationsMean(1 : L-1))
                mu = functools.reduce(lambda a, b: a + b, mean_win.tolist()) / cnt
                cc = (e - mu) * (e - mu)
                cov_win = np.concatenate(([cc], cov_win[:Lw - 1]))
                observed = not np.isnan(cs["x"][t, sx])
                if generic:
                    if beta != 1.0 and observed and k < T - 1:
                        R[k + 1] = beta * R[k] + (1.0 - beta) * (functools.reduce(lambda a, b: a + b, cov_win.tolist()) / cnt)
                elif k < T - 1:
                    R[k + 1] = R[k]
                    if beta != 1.0 and observed:
                        R[k + 1] = beta * R[k] + (1.0 - beta) * functools.reduce(lambda a, b: a + b, cov_win.tolist()) / cnt
        # ---- the days
        term, q, good, bad = np.zeros(T), np.zeros(T), np.zeros(T, dtype=bool), False
        for k in range(T):
            t = T - 1 - k if flip else k
            out["R_used"][t, c] = R[k]
            if np.isnan(cs["x"][t, sx]) or not k0 <= k < k1:
                continue
            s = cs["S_MINUS"][t, :, c]
            P = cs["P_MINUS"][t, :, c].reshape(m, m, order="F")
            Cj = [s[1] * s[2], s[0] * s[2], s[0] * s[1]] if newcases else [-1.0, 0.0, 0.0]
            CP = [fma(Cj[2], P[2, j], fma(Cj[1], P[1, j], Cj[0] * P[0, j])) for j in range(3)]
            S = fma(CP[2], Cj[2], fma(CP[1], Cj[1], CP[0] * Cj[0])) + gamma * R[k]
            e = float(cs["innovations"][t, c])
            out["S"][t, c] = S
            if np.isfinite(S) and S >= DBL_MIN and np.isfinite(e):
                q[k] = e * e / S
                term[k] = ref.log(S) + q[k]
                good[k] = True
                out["nis"][t, c] = q[k]
            else:
                bad = True
        tot_t, tot_q, n = 0.0, 0.0, 0
        for b0 in range(0, T, 32):                           # blocks of 32 filter steps, each from 0.0, then in order
            bt, bq = 0.0, 0.0
            for k in range(b0, min(T, b0 + 32)):
                if good[k]:
                    bt, bq, n = bt + term[k], bq + q[k], n + 1
            tot_t, tot_q = tot_t + bt, tot_q + bq
        out["loglik"][c] = -0.5 * (tot_t + n * LOG2PI)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["nis_mean"][c] = np.float64(tot_q) / np.float64(n)
        out["n_valid"][c] = n
        out["status"][c] = int(bad) | (4 if storage == "f32" and cs["R_series"] is None and beta != 1.0 else 0)
    if G:
        out["best"], out["best_loglik"] = np_select(out["loglik"], out["n_valid"], out["status"], G)
    return out


# ---- the workloads and the planted inputs ----
def workloads():
    """name -> synth.Workload: the seven runs the definition was checked on"""
    from epidemicmodeling_amd import synth
    return {"cfg3": synth.make_cfg3(70, 45), "cfg4": synth.make_cfg4(5, 14, 33, 12), "row3": synth.make_row3(), "row4": synth.make_row4(),
            "row4_codegen": synth.make_row4(codegen=True), "cfg3_bwd": synth.as_backward(synth.make_cfg3(6, 45)),
            "cfg4_bwd": synth.as_backward(synth.make_cfg4(3, 4, 33, 12))}


WORKLOADS = ("cfg3", "cfg4", "row3", "row4", "row4_codegen", "cfg3_bwd", "cfg4_bwd")


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """(workload, case) of one of the seven, through the C oracle (computed once per process; do not modify)"""
    from tests import helpers as H
    w = workloads()[name]
    return w, case_of(w, H.oracle_batch(w))


def with_missing_days(w, steps=(7, 31, 32), every=3, dark=1):
    """copy of `w` with x NaN at filter steps `steps` of every `every`-th observation series, and series `dark` never observed"""
    w2 = copy.copy(w)
    w2.x = w.x.copy()
    T = w.T
    for k in steps:
        if k < T:
            w2.x[(T - 1 - k) if "Backward" in w.model else k, ::every] = np.nan
    if dark is not None and dark < w2.x.shape[1]:
        w2.x[:, dark] = np.nan
    return w2


def with_bad_days(case, chain_nan=2, day_nan=9, chain_neg=3, day_neg=11):
    """copy of a case with a NaN in P_MINUS (row 0) of (day_nan, chain_nan) and an S <= 0 on (day_neg, chain_neg): the
    upper-left 3 x 3 of that P_MINUS is -1e300 I, so that C P C' is hugely negative whatever C"""
    c = dict(case)
    c["P_MINUS"] = case["P_MINUS"].copy()
    m = L.MODEL_DIM[case["model"]]
    c["P_MINUS"][day_nan, 0, chain_nan] = np.nan
    for i in range(3):
        for j in range(3):
            c["P_MINUS"][day_neg, i + m * j, chain_neg] = -1e300 if i == j else 0.0
    return c

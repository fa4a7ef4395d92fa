"""Loader of tests/innov_diag_ref.c, the bit-exact C yardstick of the innovation whiteness diagnostics, and
np_idiag, a NumPy reading of the same definition (all chains at once, a Python loop over the filter steps and the lags).  The
two must agree bit for bit (tests/test_innov_diag_ref.py); the kernels are held to them.

A *case* is (e [T, B] float64, S [T, B] float64 or None) in the classic layout; `stored` rounds e once for float storage.  The
test modules build the C file in a fixture: `InnovDiagRef(tmp_path_factory.mktemp(..))`."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from tests.loglik_ref import same_bits, to_blocked  # noqa: F401  (shared by the test modules)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "innov_diag_ref.c")
DBL_MIN = 2.2250738585072014e-308
F64 = ("mean", "var", "skew", "kurt", "jb", "nis_sum", "nis_mean", "lb_q", "het", "cusumsq_max", "max_abs")
I32 = ("n", "lb_lags", "het_n1", "het_n2", "cusumsq_step", "max_abs_step", "status")
ALL = F64 + I32 + ("acf",)
BAD_DAY, EMPTY, DEGENERATE, FEW_LAGS = 1, 2, 4, 8


def shapes(B, H):
    sh = {k: (B,) for k in F64 + I32}
    sh["acf"] = (H, B)
    return sh


def stored(e, storage):
    if storage == "f64":
        return np.ascontiguousarray(e, dtype=np.float64)
    with np.errstate(over="ignore"):
        return e.astype(np.float32).astype(np.float64)


class InnovDiagRef:
    def __init__(self, build_dir):
        cc = shutil.which("gcc") or shutil.which("cc")
        if cc is None:
            raise RuntimeError("no C compiler for tests/innov_diag_ref.c")
        so = os.path.join(str(build_dir), "libinnov_diag_ref.so")
        subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", so, "-lm"])
        h = C.CDLL(so)
        h.idr_run.argtypes = [C.c_int] * 6 + [C.c_void_p] * 21
        h.idr_run.restype = None
        self.h = h

    def run(self, e, S=None, H=10, k0=0, k1=None, flip=False, storage="f64"):
        """every output of the call for e [T, B], S [T, B] or None"""
        e = stored(e, storage)
        T, B = e.shape
        S = None if S is None else np.ascontiguousarray(S, dtype=np.float64)
        out = {k: np.full(s, -7, dtype=np.int32 if k in I32 else np.float64) for k, s in shapes(B, H).items()}
        self.h.idr_run(B, T, int(H), int(bool(flip)), int(k0), T if k1 is None else int(k1), e.ctypes.data,
                       None if S is None else S.ctypes.data, *[out[k].ctypes.data for k in ALL])
        return out


def np_idiag(e, S=None, H=10, k0=0, k1=None, flip=False, storage="f64"):
    """the definition read off DESIGN.md §4.22 in NumPy: vectors over the chains, loops over the steps"""
    e = stored(e, storage)
    T, B = e.shape
    k1 = T if k1 is None else int(k1)
    if flip:
        e, S = e[::-1], (None if S is None else S[::-1])
    nb = (T + 31) // 32
    ok = np.zeros((T, B), dtype=bool)
    nu = np.zeros((T, B))
    bad = np.zeros(B, dtype=bool)
    with np.errstate(all="ignore"):
        for k in range(k0, k1):
            if S is not None:
                s = S[k]
                good = np.isfinite(s) & (s >= DBL_MIN) & np.isfinite(e[k])
                bad |= ~np.isnan(s) & ~good
                nu[k] = np.where(good, e[k] / np.sqrt(np.where(good, s, 1.0)), 0.0)
            else:
                good = np.isfinite(e[k])
                bad |= ~np.isnan(e[k]) & ~good
                nu[k] = np.where(good, e[k], 0.0)
            ok[k] = good

        def blocked(term, cond):
            """sum of term[k] over the steps with cond[k], each block from 0.0 ascending, the blocks from 0.0 ascending;
            also the per-block sums"""
            tot, per = np.zeros(B), np.zeros((nb, B))
            for b in range(nb):
                acc = np.zeros(B)
                for k in range(32 * b, min(32 * b + 32, T)):
                    acc = np.where(cond[k], acc + term[k], acc)
                per[b] = acc
                tot = tot + acc
            return tot, per

        sq = nu * nu
        sum1, _ = blocked(nu, ok)
        q, q_blocks = blocked(sq, ok)
        n = ok.sum(axis=0).astype(np.int32)
        dn = n.astype(np.float64)
        mean = sum1 / dn
        d = np.where(ok, nu - mean, 0.0)
        dd = d * d
        m2, _ = blocked(dd, ok)
        m3, _ = blocked(dd * d, ok)
        m4, _ = blocked(dd * dd, ok)
        h3 = (2 * (k1 - k0) + 3) // 6
        ks = np.arange(T)[:, None]
        first, last = ok & (ks < k0 + h3), ok & (ks >= k1 - h3)
        f, _ = blocked(sq, first)
        l, _ = blocked(sq, last)
        nf, nl = first.sum(axis=0).astype(np.int32), last.sum(axis=0).astype(np.int32)
        # the largest value and the CUSUM of squares, in ascending k; a NaN, once held, stays
        mx, mxk, cs, csk = np.zeros(B), np.full(B, -1, np.int32), np.zeros(B), np.full(B, -1, np.int32)
        done, j = np.zeros(B), np.zeros(B, dtype=np.int64)
        for b in range(nb):
            run = np.zeros(B)
            for k in range(32 * b, min(32 * b + 32, T)):
                c = ok[k]
                run = np.where(c, run + sq[k], run)
                j = j + c
                v = np.abs((done + run) / q - j.astype(np.float64) / dn)
                take = c & ((csk < 0) | (v > cs) | (np.isnan(v) & ~np.isnan(cs)))
                cs, csk = np.where(take, v, cs), np.where(take, k, csk).astype(np.int32)
                a = np.abs(nu[k])
                take = c & ((mxk < 0) | (a > mx) | (np.isnan(a) & ~np.isnan(mx)))
                mx, mxk = np.where(take, a, mx), np.where(take, k, mxk).astype(np.int32)
            done = done + run
        empty = n == 0
        deg = ~empty & ((m2 == 0.0) | ~np.isfinite(m2))
        Hu = np.minimum(H, n - 1).astype(np.int32)
        var = m2 / dn
        sd = np.sqrt(var)
        skew, kurt = (m3 / dn) / (var * sd), (m4 / dn) / (var * var)
        jb = (dn / 6.0) * (skew * skew + ((kurt - 3.0) * (kurt - 3.0)) / 4.0)
        acf = np.full((H, B), np.nan)
        lbsum = np.zeros(B)
        for h in range(1, H + 1):
            pair = np.zeros((T, B), dtype=bool)
            prod = np.zeros((T, B))
            if h < T:
                pair[:T - h] = ok[:T - h] & ok[h:]
                prod[:T - h] = d[:T - h] * d[h:]
            ch, _ = blocked(prod, pair)
            use = (h <= Hu) & ~deg & ~empty
            ac = ch / m2
            acf[h - 1] = np.where(use, ac, np.nan)
            lbsum = np.where(use, lbsum + (ac * ac) / (dn - h), lbsum)
        lb = (dn * (dn + 2.0)) * lbsum
        lb = np.where(deg | ((Hu < H) & (Hu == 0)), np.nan, lb)
        het = np.where((nf == 0) | (nl == 0), np.nan, (l / nl) / (f / nf))
        nis_mean = q / dn
    nan = np.full(B, np.nan)
    pick = lambda v, hide=empty: np.where(hide, nan, v)
    status = (bad * BAD_DAY + empty * EMPTY + deg * DEGENERATE + (~empty & (Hu < H)) * FEW_LAGS).astype(np.int32)
    return {"mean": pick(mean), "var": pick(var), "skew": pick(skew, empty | deg), "kurt": pick(kurt, empty | deg),
            "jb": pick(jb, empty | deg), "nis_sum": pick(q), "nis_mean": pick(nis_mean), "lb_q": pick(lb), "het": pick(het),
            "cusumsq_max": pick(cs), "max_abs": pick(mx), "n": n, "lb_lags": np.where(empty, 0, Hu).astype(np.int32),
            "het_n1": nf, "het_n2": nl, "cusumsq_step": csk, "max_abs_step": mxk, "status": status, "acf": acf}


# ---- the cases of the device list of the issue, shared by the restatement, emulation and device tests ----
def series(T, B, seed, with_S=True):
    """seeded innovations and variances of an ordinary run: e ~ sqrt(S) z, S log-uniform in [0.5, 50]"""
    rng = np.random.default_rng(seed)
    S = np.exp(rng.uniform(np.log(0.5), np.log(50.0), size=(T, B)))
    e = rng.standard_normal((T, B)) * np.sqrt(S)
    return (e, S) if with_S else (rng.standard_normal((T, B)), None)


def with_missing_days(e, S, steps=(7, 31, 32), every=3, dark_block=1, dark_chain=1):
    """steps 7, 31, 32 of every third chain missing, one whole block dark in chain 2, chain `dark_chain` all dark"""
    e, S = e.copy(), (None if S is None else S.copy())
    tgt = e if S is None else S
    T, B = e.shape
    for k in steps:
        if k < T:
            tgt[k, ::every] = np.nan
    if B > 2:
        tgt[32 * dark_block:32 * dark_block + 32, 2] = np.nan
    if B > dark_chain:
        tgt[:, dark_chain] = np.nan
    return e, S


def with_bad_values(e, S):
    """S in {0, -1, +Inf, a subnormal} and e = +-Inf, one per chain 3..8 (chain % B), each inside every test window"""
    e, S = e.copy(), (None if S is None else S.copy())
    T, B = e.shape
    day = min(36, T - 1)
    if S is not None:
        for c, v in zip((3, 4, 5, 6), (0.0, -1.0, np.inf, 1e-310)):
            S[day, c % B] = v
    e[day, 7 % B] = np.inf
    e[day, 8 % B] = -np.inf
    return e, S


def with_degenerate_chains(e, S, k0=0, flip=False):
    """chain 9 constant (m2 = 0), chain 10 with a single counted day: filter step k0 + 3"""
    e, S = e.copy(), (None if S is None else S.copy())
    T, B = e.shape
    if B > 10:
        e[:, 9] = 2.0
        if S is not None:
            S[:, 9] = 4.0
        tgt = e if S is None else S
        keep = min(T - 1, k0 + 3)
        keep = T - 1 - keep if flip else keep
        tgt[:keep, 10] = np.nan
        tgt[keep + 1:, 10] = np.nan
    return e, S


# (name, T, B, H, k0, k1, storage, flip, with_S, blk): the device list of the issue at its smallest shapes
CASES = [
    ("plain", 45, 70, 10, 0, None, "f64", False, True, 0),
    ("one_chain", 45, 1, 10, 0, None, "f64", False, True, 0),
    ("no_lags", 45, 70, 0, 0, None, "f64", False, True, 0),
    ("one_lag", 45, 70, 1, 0, None, "f64", False, True, 0),
    ("lags_40", 45, 70, 40, 0, None, "f64", False, True, 0),
    ("lags_64", 45, 70, 64, 0, None, "f64", False, True, 0),
    ("two_blocks_ahead", 100, 70, 40, 0, None, "f64", False, True, 0),
    ("window_5_37", 45, 70, 10, 5, 37, "f64", False, True, 0),
    ("window_33_45", 45, 70, 10, 33, 45, "f64", False, True, 0),
    ("window_empty", 45, 70, 10, 12, 12, "f64", False, True, 0),
    ("thirds_split_a_block", 100, 70, 10, 3, 99, "f64", False, True, 0),
    ("blocked", 45, 70, 10, 0, None, "f64", False, True, 40),
    ("float", 45, 70, 10, 0, None, "f32", False, True, 0),
    ("float_blocked_flip", 100, 70, 40, 5, 90, "f32", True, True, 40),
    ("flip", 45, 70, 10, 5, 37, "f64", True, True, 0),
    ("no_S", 45, 70, 10, 0, None, "f64", False, False, 0),
    ("no_S_float_blocked", 100, 70, 40, 0, None, "f32", False, False, 40),
]


def make_case(name, planted=True):
    """(e, S, kwargs of run / np_idiag, blk) of one CASES row; planted: the missing days, bad values and degenerate chains"""
    row = next(r for r in CASES if r[0] == name)
    _, T, B, H, k0, k1, storage, flip, with_S, blk = row
    e, S = series(T, B, seed=1000 + [r[0] for r in CASES].index(name), with_S=with_S)
    if planted and B > 1:
        e, S = with_missing_days(e, S)
        e, S = with_bad_values(e, S)
        e, S = with_degenerate_chains(e, S, k0, flip)
    return e, S, dict(H=H, k0=k0, k1=k1, flip=flip, storage=storage), blk

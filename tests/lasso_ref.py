"""Loader of tests/lasso_ref.c, the independent C restatement of the cross-validated LASSO (the bit-exact yardstick of
csrc/lasso.hpp), plus a plain-Python loop reading of DESIGN.md §4.5 that checks it.

The test modules build it in a session fixture: `LassoRef(tmp_path_factory.mktemp("lasso"))`."""
from __future__ import annotations

import ctypes as C
import math
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "lasso_ref.c")

ST_OK, ST_NULL_MODEL, ST_MAXITER, ST_NONFINITE, ST_BAD_FOLDS = range(5)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


def _p(a, t=_dp):
    return None if a is None else a.ctypes.data_as(t)


class LassoRef:
    def __init__(self, build_dir):
        cc = shutil.which("gcc") or shutil.which("cc")
        if cc is None:
            raise RuntimeError("no C compiler for tests/lasso_ref.c")
        so = os.path.join(str(build_dir), "liblasso_ref.so")
        subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", so, "-lm"])
        h = C.CDLL(so)
        h.ls_exp.restype = h.ls_log.restype = C.c_double
        h.ls_exp.argtypes = h.ls_log.argtypes = [C.c_double]
        h.ls_lasso.restype = C.c_int
        h.ls_lasso.argtypes = [_dp, _dp, _ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                               _dp, _dp, _dp, _ip, _ip, _dp, _dp, _ip, _ip, _dp, _dp, _ip]
        self.h = h

    def exp(self, v):
        return self.h.ls_exp(float(v))

    def log(self, v):
        return self.h.ls_log(float(v))

    def region(self, X, y, fold, K, num_lambda=100, lambda_ratio=1e-4, rel_tol=1e-4, max_iter=100000):
        """one region: X [D, n], y [D], fold [D] (None when K = 0) -> dict (lambda, intercept, df, iters, mse, se [NL],
        B [NL, n], a [n], b, idx_min_mse, idx_1se, status, lane_iters [NL, K+1] (the full fit last))"""
        X = np.ascontiguousarray(X, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        D, n = X.shape
        NL = int(num_lambda)
        f = None if K < 2 else np.ascontiguousarray(fold, dtype=np.int32)
        o = {k: np.empty(NL) for k in ("lambda", "intercept", "mse", "se")}
        o.update(B=np.empty((NL, n)), df=np.empty(NL, dtype=np.int32), iters=np.empty(NL, dtype=np.int32), a=np.empty(n),
                 b=np.empty(1), idx_min_mse=np.full(1, -7, dtype=np.int32), idx_1se=np.full(1, -7, dtype=np.int32),
                 lane_iters=np.empty((NL, (K + 1) if K >= 2 else 1), dtype=np.int32))
        st = self.h.ls_lasso(_p(X), _p(y), _p(f, _ip), D, n, int(K), NL, float(lambda_ratio), float(rel_tol), int(max_iter),
                             _p(o["lambda"]), _p(o["B"]), _p(o["intercept"]), _p(o["df"], _ip), _p(o["iters"], _ip),
                             _p(o["mse"]), _p(o["se"]), _p(o["idx_min_mse"], _ip), _p(o["idx_1se"], _ip), _p(o["a"]),
                             _p(o["b"]), _p(o["lane_iters"], _ip))
        o["status"] = st
        o["b"] = o["b"][0]
        o["idx_min_mse"], o["idx_1se"] = int(o["idx_min_mse"][0]), int(o["idx_1se"][0])
        if K < 2:
            for k in ("mse", "se", "a", "b", "idx_min_mse", "idx_1se"):
                del o[k]
        return o

    def run(self, X, y, fold, K, num_lambda=100, lambda_ratio=1e-4, rel_tol=1e-4, max_iter=100000, lane_iters=False):
        """every region of X [D, n, R], y [D, R], fold [D, R] -> the dict of batch.lasso_cv as NumPy arrays (+ lane_iters
        [NL, K+1, R] when asked)"""
        D, n, R = X.shape
        one = lambda r: self.region(X[:, :, r], y[:, r], None if K < 2 else fold[:, r], K, num_lambda, lambda_ratio, rel_tol,
                                    max_iter)
        with ThreadPoolExecutor(max_workers=min(8, R)) as ex:    # ctypes drops the GIL: regions run side by side
            res = list(ex.map(one, range(R)))
        out = {}
        for k in res[0]:
            if k == "lane_iters" and not lane_iters:
                continue
            v = np.stack([np.asarray(q[k]) for q in res], axis=-1)
            out[k] = v.astype(np.int32) if k in ("status", "idx_min_mse", "idx_1se") else v
        return out


# ---- plain-Python loop reading of DESIGN.md §4.5 (one region) -------------------------------------------------------
def np_lasso(X, y, fold, K, num_lambda, lambda_ratio, rel_tol, max_iter, exp, log):
    """X [D, n], y [D], fold [D]; exp / log: the shared fixed-order functions (LassoRef.exp / .log).  Python floats are
    IEEE doubles and every operation below is one rounding, so this must agree with tests/lasso_ref.c bit for bit."""
    X = [[float(v) for v in row] for row in np.asarray(X, dtype=np.float64)]
    y = [float(v) for v in np.asarray(y, dtype=np.float64)]
    D, n, NL = len(y), len(X[0]), int(num_lambda)
    nan = float("nan")
    fin = all(math.isfinite(v) for row in X for v in row) and all(math.isfinite(v) for v in y)
    bad = False
    if K >= 2:
        fl = [int(v) for v in fold]
        bad = any(f < 0 or f >= K for f in fl) or any(fl.count(f) == 0 for f in range(K))
    if bad or not fin:
        o = dict(lambda_=[nan] * NL, intercept=[nan] * NL, B=[[nan] * n for _ in range(NL)], df=[0] * NL, iters=[0] * NL,
                 mse=[nan] * NL, se=[nan] * NL, a=[nan] * n, b=nan, idx_min_mse=-1, idx_1se=-1,
                 status=ST_BAD_FOLDS if bad else ST_NONFINITE)
        return o

    def fit(inset):
        N = float(sum(inset))
        F = dict(inset=inset, N=N, cnt=sum(inset), cst=set(), active=set(), mu=[0.0] * n, sigma=[1.0] * n, colsq=[1.0] * n,
                 b=[0.0] * n)
        days = [i for i in range(D) if inset[i]]
        for j in range(n):
            s = 0.0
            for i in days:
                s = s + X[i][j]
            F["mu"][j] = s / N
            col = [X[i][j] for i in days]
            if max(col) == min(col):
                F["cst"].add(j)
                continue
            s = 0.0
            for i in days:
                d = X[i][j] - F["mu"][j]
                s = s + d * d
            F["sigma"][j] = math.sqrt(s / N)
            s = 0.0
            for i in days:
                xs = (X[i][j] - F["mu"][j]) / F["sigma"][j]
                s = s + xs * xs
            F["colsq"][j] = s / N
        s = 0.0
        for i in days:
            s = s + y[i]
        F["muY"] = s / N
        F["r"] = [y[i] - F["muY"] if inset[i] else 0.0 for i in range(D)]
        F["days"] = days
        return F

    def xs(F, i, j):
        return (X[i][j] - F["mu"][j]) / F["sigma"][j]

    def update(F, j, lam):
        bj, r = F["b"][j], F["r"]
        rho = 0.0
        for i in F["days"]:
            x = xs(F, i, j)
            rj = r[i] + x * bj
            r[i] = rj
            rho = rho + x * rj
        rho = rho / F["N"]
        t = abs(rho) - lam
        t = t if t > 0.0 else 0.0
        bn = (t if rho > 0.0 else (-t if rho < 0.0 else 0.0)) / F["colsq"][j]
        for i in F["days"]:
            r[i] = r[i] - xs(F, i, j) * bn
        F["b"][j] = bn

    def descend(F, lam):
        it, hit = 0, False
        while True:
            while F["active"]:
                if it >= max_iter:
                    return it, True
                dmax = 0.0
                for j in sorted(F["active"]):
                    bold = F["b"][j]
                    update(F, j, lam)
                    d = abs(F["b"][j] - bold) / (1.0 + abs(bold))
                    dmax = d if d > dmax else dmax
                it += 1
                if dmax < rel_tol:
                    break
            if it >= max_iter:
                return it, True
            grew = set()
            for j in range(n):
                if j in F["active"] or j in F["cst"]:
                    continue
                update(F, j, lam)
                if F["b"][j] != 0.0:
                    grew.add(j)
            it += 1
            if not grew:
                return it, hit
            F["active"] |= grew

    def coefs(F):
        s, B = 0.0, []
        for j in range(n):
            Bj = 0.0 if j in F["cst"] else F["b"][j] / F["sigma"][j]
            B.append(Bj)
            s = s + F["mu"][j] * Bj
        return B, F["muY"] - s, sum(1 for v in B if v != 0.0)

    cv = K >= 2
    fits = [fit([int(fold[i]) != f for i in range(D)]) for f in range(K)] if cv else []
    full = fit([True] * D)
    lmax = 0.0
    for j in range(n):
        if j in full["cst"]:
            continue
        s = 0.0
        for i in range(D):
            s = s + xs(full, i, j) * full["r"][i]
        v = abs(s) / full["N"]
        lmax = v if v > lmax else lmax
    null = len(full["cst"]) == n or max(y) == min(y) or not lmax > 0.0
    if null:
        lam = [0.0] * NL
    elif NL == 1:
        lam = [lmax]
    else:
        l0, l1 = log(lmax), log(lmax * lambda_ratio)
        st = (l1 - l0) / float(NL - 1)
        lam = [exp(l0 + float(k) * st) for k in range(NL)]
    o = dict(lambda_=[0.0] * NL, intercept=[0.0] * NL, B=[None] * NL, df=[0] * NL, iters=[0] * NL, mse=[0.0] * NL,
             se=[0.0] * NL, a=[nan] * n, b=nan)
    hit_any, best, im = False, float("inf"), -1
    for k in range(NL):
        kk = NL - 1 - k
        sse, msef = [], []
        for F in fits + [full]:
            it = 0
            if not null:
                it, hit = descend(F, lam[k])
                hit_any |= hit
            B, icpt, df = coefs(F)
            if F is full:
                o["lambda_"][kk], o["B"][kk], o["intercept"][kk], o["df"][kk], o["iters"][kk] = lam[k], B, icpt, df, it
            else:
                s = 0.0
                for i in range(D):
                    if F["inset"][i]:
                        continue
                    xb = 0.0
                    for j in range(n):
                        xb = xb + X[i][j] * B[j]
                    e = (y[i] - icpt) - xb
                    s = s + e * e
                sse.append(s)
                msef.append(s / float(D - F["cnt"]))
        if cv:
            s = m = v = 0.0
            for f in range(K):
                s = s + sse[f]
            for f in range(K):
                m = m + msef[f]
            m = m / float(K)
            for f in range(K):
                d = msef[f] - m
                v = v + d * d
            o["mse"][kk] = s / float(D)
            o["se"][kk] = math.sqrt(v / float(K - 1)) / math.sqrt(float(K))
            if o["mse"][kk] <= best:
                best, im = o["mse"][kk], kk
                B, icpt, _ = coefs(full)
                o["a"], o["b"] = list(B), icpt
    if cv:
        thr = o["mse"][im] + o["se"][im]
        o["idx_min_mse"] = im
        o["idx_1se"] = max(k for k in range(NL) if o["mse"][k] <= thr)
    o["status"] = ST_NULL_MODEL if null else ST_MAXITER if hit_any else ST_OK
    return o


# ---- the CV half against scikit-learn (one region) -------------------------------------------------------------------
def sklearn_cv(X, y, fold, K, lam, rel_tol, mu_floor=1e-3):
    """Refit every fold of one region (X [D, n], y [D], fold [D]) at the lambdas `lam` with sklearn.linear_model.Lasso on
    that fold's own standardization (training-set mean, population std, constant columns left out; alpha = lambda, no
    intercept, tol 1e-13), and recompute the held-out MSE = sum of the folds' SSEs / D and SE = std(SSE_f / |f|, ddof=1) /
    sqrt(K).  Returns mse, se and their gates (NaN where no gate can be derived) as arrays over `lam`.

    Gate.  A fold fit that stopped by the RelTol rule has a KKT residual e with |e_j| <= RelTol sum_k |G_jk| (1 + |b_k|)
    (1 + RelTol) (G = Xs' Xs / N on the training set; test_lasso_host.py::test_path_meets_the_kkt_conditions), so by strong
    convexity it lies within ||e|| / mu_min of the optimum, mu_min the smallest eigenvalue of G over the non-constant columns
    (required > mu_floor; b is taken at sklearn's point, which is the optimum to 1e-13).  A held-out prediction is
    mean(y_train) + Xs_i b, so it moves by at most d_i = ||Xs_i|| ||e|| / mu_min, the fold's SSE by sum 2 |r_i| d_i + d_i^2
    (r_i sklearn's residual), the MSE by the sum of those over D.  SE is sqrt(K - 1)^-1 sqrt(K)^-1 times a centred 2-norm,
    which is 1-Lipschitz: it moves by at most ||(dSSE_f / |f|)_f|| / sqrt((K - 1) K).  Both gates get 1e-12 of their value
    for rounding."""
    from sklearn.linear_model import Lasso
    X, y, fold = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(fold)
    D = len(y)
    NL = len(lam)
    sse, dsse, cnt = np.zeros((NL, K)), np.zeros((NL, K)), np.zeros(K)
    for f in range(K):
        tr, ho = fold != f, fold == f
        cnt[f] = ho.sum()
        Xt, yt = X[tr], y[tr]
        N = tr.sum()
        mu = Xt.sum(0) / N
        cst = Xt.max(0) == Xt.min(0)
        sig = np.sqrt(((Xt - mu) ** 2).sum(0) / N)
        sig[cst] = 1.0
        Xs = (Xt - mu) / sig
        Xs[:, cst] = 0.0
        Xh = (X[ho] - mu) / sig
        Xh[:, cst] = 0.0
        muY = yt.sum() / N
        G = Xs.T @ Xs / N
        nc = ~cst
        mu_min = np.linalg.eigvalsh(G[np.ix_(nc, nc)]).min() if nc.any() else np.inf
        for k in range(NL):
            b = Lasso(alpha=lam[k], fit_intercept=False, tol=1e-13, max_iter=1_000_000).fit(Xs, yt - muY).coef_
            r = y[ho] - (muY + Xh @ b)
            sse[k, f] = (r ** 2).sum()
            if mu_min > mu_floor:
                e = rel_tol * np.abs(G) @ ((1 + np.abs(b)) * (1 + rel_tol))
                d = np.linalg.norm(Xh, axis=1) * np.linalg.norm(e) / mu_min
                dsse[k, f] = (2 * np.abs(r) * d + d * d).sum()
            else:
                dsse[k, f] = np.nan
    mse = sse.sum(1) / D
    msef = sse / cnt
    se = msef.std(axis=1, ddof=1) / np.sqrt(K)
    g_mse = dsse.sum(1) / D + 1e-12 * mse
    g_se = np.linalg.norm(dsse / cnt, axis=1) / np.sqrt((K - 1) * K) + 1e-12 * se
    return mse, se, g_mse, g_se


def cv_indices_agree(mse, se, g_mse, g_se, idx_min, idx_1se, mse_sk, se_sk):
    """idx_min_mse / idx_1se of a fit whose mse / se lie within the gates of sklearn_cv's: wherever sklearn's MSE margin
    exceeds the gates the indices must be the ones sklearn's values give (ties to the smaller index, as lasso does).
    Returns the number of indices that were decidable (and checked)."""
    checked = 0
    s_min = int(np.flatnonzero(mse_sk == mse_sk.min())[0])
    if idx_min != s_min:           # only where the two minima are within the gates of each other
        assert mse_sk[idx_min] - mse_sk[s_min] <= g_mse[idx_min] + g_mse[s_min], (idx_min, s_min)
        return checked
    others = np.arange(len(mse_sk)) != s_min
    if (mse_sk[others] - mse_sk[s_min] > g_mse[others] + g_mse[s_min]).all():
        checked += 1
    thr, g_thr = mse_sk[s_min] + se_sk[s_min], g_mse[s_min] + g_se[s_min]
    s_1se = int(np.flatnonzero(mse_sk <= thr).max())
    if idx_1se != s_1se:
        lo, hi = sorted((idx_1se, s_1se))
        assert (np.abs(mse_sk[lo:hi + 1] - thr) <= g_mse[lo:hi + 1] + g_thr).any(), (idx_1se, s_1se)
    elif (np.abs(mse_sk - thr) > g_mse + g_thr).all():
        checked += 1
    return checked

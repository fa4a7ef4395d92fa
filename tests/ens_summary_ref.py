"""The Monte-Carlo ensemble statistics of epi_ens_run_* (include/epiekf.h) in NumPy, statement for
statement: every operation below is one IEEE double operation, in the order the definition gives."""
import numpy as np


def tree(a):
    """pairwise sum in draw order: pad with +0.0 to the power of two P >= len(a), then a[i] = a[i] + a[i + h], h = P/2 .. 1"""
    P = 1
    while P < len(a):
        P *= 2
    a = np.concatenate([np.asarray(a, dtype=np.float64), np.zeros(P - len(a))])
    h = P // 2
    while h >= 1:
        a = a[:h] + a[h:2 * h]
        h //= 2
    return a[0]


def quantile(x, n, p):
    """MATLAB's quantile / NumPy's method="hazen" on the ascending x(1 .. n) (x is 0-based here)"""
    h = np.float64(n) * np.float64(p) + np.float64(0.5)
    k = np.floor(h)
    g = h - k
    if k < 1:
        return x[0]
    if k >= n:
        return x[n - 1]
    k = int(k)
    return x[k - 1] + g * (x[k] - x[k - 1])


def item(v, q):
    """v [D] (any NaN = excluded member) -> dict mean, std, min, max, quantiles [n_q], count"""
    with np.errstate(all="ignore"):
        v = np.asarray(v, dtype=np.float64)
        ok = ~np.isnan(v)
        n = int(ok.sum())
        nan = np.float64(np.nan)
        if n == 0:
            return dict(mean=nan, std=nan, min=nan, max=nan, quantiles=np.full(len(q), nan), count=0)
        mean = tree(np.where(ok, v, 0.0)) / np.float64(n)
        dev = np.where(ok, v - mean, 0.0)
        std = np.float64(0.0) if n == 1 else np.sqrt(tree(dev * dev) / np.float64(n - 1))
        x = np.sort(v[ok])
        return dict(mean=mean, std=std, min=x[0], max=x[n - 1], quantiles=np.array([quantile(x, n, p) for p in q]), count=n)


def derived_row(src, population, R, D):
    """((N_r * v0) * v1) * v2 of rows 0, 1, 2: src [T, rows, R * D] (widened to double) -> [T, R * D]"""
    s = np.asarray(src).astype(np.float64)
    N = np.repeat(np.asarray(population, dtype=np.float64), D)
    with np.errstate(all="ignore"):
        return ((N[None, :] * s[:, 0]) * s[:, 1]) * s[:, 2]


def summary(src, R, D, q, population=None):
    """src [T, rows, R * D] float32 / float64 -> the dict of batch.ensemble_summary as NumPy arrays"""
    s = np.asarray(src).astype(np.float64)
    if population is not None:
        s = np.concatenate([s, derived_row(s, population, R, D)[:, None, :]], axis=1)
    T, rows, _ = s.shape
    out = {k: np.empty((T, rows, R)) for k in ("mean", "std", "min", "max")}
    out["quantiles"] = np.empty((T, len(q), rows, R))
    out["count"] = np.empty((T, rows, R), dtype=np.int32)
    for t in range(T):
        for j in range(rows):
            for r in range(R):
                it = item(s[t, j, r * D:(r + 1) * D], q)
                for k in ("mean", "std", "min", "max", "count"):
                    out[k][t, j, r] = it[k]
                out["quantiles"][t, :, j, r] = it["quantiles"]
    return out

"""Measurement of the cross-validated LASSO as one device call (epi_lasso_run_device; bench.py stays the headline's
yardstick).  Writes profiles/lasso/bench.json and prints it as one JSON line.

    python tools/bench_lasso.py                  # 236 regions x D 60 x n 12, K = 50, NumLambda = 100
    python tools/bench_lasso.py --profile-only   # a few calls, for rocprofv3 --kernel-trace --stats

Two inputs: X and y from the front half (pipeline._front_half on synth.make_raw_counts: NPI_MAXES - plans over the last 60
days and the round-1 alpha), and a synthetic problem (step-function and Gaussian columns, some constant, y affine in them).
Per input: the call's device time (HIP events around each of 30 calls after warm-up: median, p10, p90), the coordinate
cycles per lambda of the full fit (from the iters output) and of the wave (the slowest of its K + 1 lanes, from the C
restatement's per-fit counts), mean / p90 / max.  The CPU baseline is the C restatement tests/lasso_ref.c on ONE thread over
a sample of regions, scaled by regions and labelled as scaled.  Last, the front half (preprocessing, two EKF rounds, two
regressions) with NNLS against the front half with LASSO, wall clock per call with a synchronisation at the end."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R, T, D, N_NPI, K, NL = 236, 200, 60, 12, 50, 100


def synthetic(seed=0):
    rng = np.random.default_rng(seed)
    X = np.empty((D, N_NPI, R))
    for r in range(R):
        for j in range(N_NPI):
            kind = rng.integers(5)
            if kind == 0:
                X[:, j, r] = rng.standard_normal(D)
            elif kind == 1:
                X[:, j, r] = float(rng.integers(0, 4))
            else:
                lv = rng.integers(0, 5, size=4).astype(float)
                cuts = np.sort(rng.integers(0, D, size=3))
                X[:, j, r] = np.select([np.arange(D) < c for c in cuts], lv[:3], lv[3])
    beta = rng.standard_normal((N_NPI, R)) * (rng.random((N_NPI, R)) < 0.6) * 0.02
    y = 0.2 + np.einsum("djr,jr->dr", X, beta) + 0.005 * rng.standard_normal((D, R))
    return np.ascontiguousarray(X), np.ascontiguousarray(y)


def front_half_inputs(device):
    from epidemicmodeling_amd import pipeline, synth
    raw = synth.make_raw_counts(R, T, seed=7)
    raw["cases"][:, -1] = np.cumsum(np.full(T, 40.0))
    out = pipeline._front_half(raw["cases"], raw["deaths"], np.asarray(raw["population"], dtype=np.float64), raw["ip"], D, 7, device)
    return np.ascontiguousarray(out["X_reg"]), np.ascontiguousarray(out["alpha_round1"][T - D:]), raw


def time_calls(fn, calls, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)),
            "calls": calls}


def dist(v):
    v = np.asarray(v, dtype=np.float64).ravel()
    return {"mean": float(v.mean()), "p90": float(np.percentile(v, 90)), "max": float(v.max())}


def measure(name, X, y, folds, ref, device, calls, cpu_regions):
    import torch
    from epidemicmodeling_amd import batch
    Xd = torch.as_tensor(X, device=device)
    yd = torch.as_tensor(y, device=device)
    fd = torch.as_tensor(folds, device=device)
    res = {"input": name}
    res["device"] = time_calls(lambda: batch.lasso_cv(Xd, yd, K=K, folds=fd, num_lambda=NL, device=device), calls, 5)
    out = {k: v.cpu().numpy() for k, v in batch.lasso_cv(Xd, yd, K=K, folds=fd, num_lambda=NL, device=device).items()}
    ok = out["status"] != 3
    res["status_counts"] = {int(s): int((out["status"] == s).sum()) for s in np.unique(out["status"])}
    res["cycles_per_lambda_full_fit"] = dist(out["iters"][:, ok])
    res["df_at_idx_min_mse"] = dist((out["a"][:, ok] != 0).sum(axis=0))
    # the C restatement on ONE thread over a sample of regions: the wave's cycles per lambda and the scaled CPU baseline
    idx = np.linspace(0, R - 1, cpu_regions).astype(int)
    waves = []
    t0 = time.perf_counter()
    for r in idx:
        o = ref.region(X[:, :, r], y[:, r], folds[:, r], K, NL)
        waves.append(o["lane_iters"].max(axis=1))
    cpu_s = time.perf_counter() - t0
    res["cycles_per_lambda_wave"] = dist(np.concatenate(waves))
    res["cpu_one_thread_ms_scaled"] = {"ms": cpu_s * 1e3 * R / len(idx), "regions_run": int(len(idx)),
                                       "note": "C restatement, one thread, scaled by regions"}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--cpu-regions", type=int, default=24)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lasso", "bench.json"))
    args = ap.parse_args()
    import torch
    from epidemicmodeling_amd import _build, batch, pipeline, synth
    from tests.lasso_ref import LassoRef
    _build.build_library()
    device = "cuda:0"
    folds = batch.lasso_folds(D, K, R, 0)
    Xs, ys = synthetic()
    if args.profile_only:
        for _ in range(5):
            batch.lasso_cv(Xs, ys, K=K, folds=folds, device=device)
        torch.cuda.synchronize()
        return
    ref = LassoRef(tempfile.mkdtemp(prefix="lasso_ref_"))
    Xf, yf, raw = front_half_inputs(device)
    res = {"shape": {"R": R, "D": D, "n": N_NPI, "K": K, "num_lambda": NL}, "timing": "HIP events around each call",
           "source_hash": _build.source_hash(), "gpu": torch.cuda.get_device_name(0)}
    res["front_half_inputs"] = measure("front half (synth.make_raw_counts, round-1 alpha)", Xf, yf, folds, ref, device,
                                       args.calls, args.cpu_regions)
    res["synthetic"] = measure("synthetic", Xs, ys, folds, ref, device, args.calls, args.cpu_regions)
    N = np.asarray(raw["population"], dtype=np.float64)
    fh = {}
    for reg in ("nonnegls", "lasso"):
        run = lambda: pipeline._front_half(raw["cases"], raw["deaths"], N, raw["ip"], D, 7, device, regression=reg)
        run()
        ms = []
        for _ in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        fh[reg] = {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "calls": 7}
    res["front_half_wall_ms"] = fh
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

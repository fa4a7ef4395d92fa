"""Measurement of the sliding-window growth-rate estimators as one device call (epi_rtwin_run_device; bench.py stays the
headline's yardstick).  Prints one JSON line.

    python tools/bench_rt_window.py                     # article size (236 x 366, wlen 7) and 300 x 520
    python tools/bench_rt_window.py --profile-only      # a few calls per size, for rocprofv3 --kernel-trace --stats

Per size: the call's device time (HIP events around each call, >= 20 calls after warm-up: median, p10, p90) for NonlinLS
alone and for all three estimators together, and the distribution of the LM iteration counts.  The baseline is the C
restatement tests/rt_window_ref.c (one CPU thread) on a sample of regions, scaled by regions and labelled as scaled."""
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

ALL = ("LogLinReg", "GenRatios", "NonlinLS")


def make_case(R, L, seed=0):
    """smoothed-looking daily counts: a per-region exponential with a slow wobble and 5 % noise, a few zero days"""
    rng = np.random.default_rng(seed)
    t = np.arange(L)[:, None]
    x = rng.uniform(5, 2000, R) * np.exp(rng.uniform(-0.03, 0.05, R) * t + 0.5 * np.sin(t / rng.uniform(10, 40, R)))
    x *= 1.0 + 0.05 * rng.standard_normal((L, R))
    x[rng.random((L, R)) < 0.01] = 0.0
    return np.ascontiguousarray(np.abs(x))


def time_calls(fn, calls, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)),
            "calls": int(calls)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--wlen", type=int, default=7)
    ap.add_argument("--ref-regions", type=int, default=24, help="regions the CPU baseline runs (scaled to the full size)")
    ap.add_argument("--profile-only", action="store_true")
    args = ap.parse_args()
    import torch
    from epidemicmodeling_amd import batch
    sizes = [(236, 366), (300, 520)]
    res = {"tool": "bench_rt_window", "device": torch.cuda.get_device_name(0), "wlen": args.wlen, "sizes": []}
    for R, L in sizes:
        x = torch.as_tensor(make_case(R, L), device="cuda:0")
        if args.profile_only:
            for m in (("NonlinLS",), ALL):
                for _ in range(3):
                    batch.rt_window(x, args.wlen, 1.0, 1, 3, m)
            torch.cuda.synchronize()
            continue
        entry = {"R": R, "L": L}
        entry["nonlinls"] = time_calls(lambda: batch.rt_window(x, args.wlen, 1.0, 1, 3, ("NonlinLS",)), args.calls, args.warmup)
        entry["all_three"] = time_calls(lambda: batch.rt_window(x, args.wlen, 1.0, 1, 3, ALL), args.calls, args.warmup)
        out = batch.rt_window(x, args.wlen, 1.0, 1, 3, ALL)
        it = out["nls_iters"].cpu().numpy()
        st = out["nls_status"].cpu().numpy()
        fitted = it[st != 0]
        entry["iters"] = {"mean": float(fitted.mean()), "p50": float(np.percentile(fitted, 50)),
                          "p90": float(np.percentile(fitted, 90)), "max": int(fitted.max()),
                          "status_counts": {int(k): int(v) for k, v in zip(*np.unique(st, return_counts=True))}}
        # CPU baseline: the C restatement on a sample of regions, scaled
        from tests.rt_window_ref import RtWindowRef
        ref = RtWindowRef(tempfile.mkdtemp())
        n = min(args.ref_regions, R)
        xs = np.ascontiguousarray(x.cpu().numpy()[:, :n])
        t0 = time.perf_counter()
        ref.nonlinls(xs, args.wlen, 1.0, 1)
        t1 = time.perf_counter()
        ref.loglinreg(xs, args.wlen, 1.0, 1)
        ref.genratios(xs, args.wlen, 3, 1.0)
        t2 = time.perf_counter()
        scale = R / n
        entry["cpu_ref_scaled"] = {"regions_run": n, "scale": scale, "threads": 1,
                                   "nonlinls_ms": (t1 - t0) * 1e3 * scale, "all_three_ms": (t2 - t0) * 1e3 * scale,
                                   "label": f"C restatement on {n} of {R} regions, 1 thread, scaled by {scale:.2f}"}
        res["sizes"].append(entry)
    if args.profile_only:
        print(json.dumps({"tool": "bench_rt_window", "profile_only": True}))
        return
    print(json.dumps(res))


if __name__ == "__main__":
    main()

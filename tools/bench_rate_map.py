"""Measurement of the NPI-to-growth-rate predictor as one device call (epi_ratemap_run_device; bench.py stays the headline's
yardstick).  Writes profiles/rate_map/bench.json and prints it as one JSON line.

    python tools/bench_rate_map.py                  # 236 regions x 91 train ends x 366 days, 12 NPIs, lags 3 / 5 / 7 (F = 48)
    python tools/bench_rate_map.py --small          # 20 regions x 8 train ends x 120 days: a quick run of the same kind
    python tools/bench_rate_map.py --profile-only   # a few calls, for rocprofv3 --kernel-trace --stats

The inputs come from the seeded generator of tests/rate_map_ref.py (piecewise-constant plans, a rate that follows them plus
noise); the train ends are the last 91 days (predict_ahead = 90 .. 0).  In this process and on this device (HIP events around
each call after warm-up: median, p10, p90):
  call        batch.rate_map, every output
  call_nofit  the same clip and rebuild with lambda_in instead of the fit
and on ONE CPU thread the C restatement tests/rate_map_ref.c over a sample of regions, scaled by regions (labelled scaled).
The call's outputs are compared with the restatement on that sample, bit for bit."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu-regions", type=int, default=4)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_map", "bench.json"))
    a = ap.parse_args()
    import torch
    from epidemicmodeling_amd import _build, batch
    from tests import rate_map_ref as RM
    if not torch.cuda.is_available():
        raise SystemExit("bench_rate_map needs a GPU")
    dev = "cuda:0"
    R, K, T, n, lags = (20, 8, 120, 12, (3, 5, 7)) if a.small else (236, 91, 366, 12, (3, 5, 7))
    nt = tuple(range(T - K + 1, T + 1))
    p = RM.make_case(7, T, n, lags, 0, K, R, nt)
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v), device=dev)
    ipd, yd, nsd = t(p["ip"]), t(p["y"]), t(p["new_smoothed"])
    call = lambda: batch.rate_map(ipd, nsd, nt, y=yd, lags=lags, device=dev)
    if a.profile_only:
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        return
    F = n * (1 + len(lags))
    res = {"tool": "bench_rate_map", "device": torch.cuda.get_device_name(0), "source_hash": _build.source_hash(),
           "regions": R, "train_ends": K, "days": T, "npis": n, "lags": list(lags), "features": F, "items": R * K,
           "input_bytes": int(p["ip"].nbytes + p["y"].nbytes + p["new_smoothed"].nbytes)}
    res["call"] = time_calls(call, a.calls, a.warmup)
    got = {k: v.cpu().numpy() for k, v in call().items()}
    res["output_bytes"] = int(sum(v.nbytes for v in got.values()))
    lam = torch.as_tensor(got["lambda_hat"], device=dev)
    res["call_nofit"] = time_calls(lambda: batch.rate_map(ipd, nsd, nt, lambda_in=lam, lags=lags, device=dev), a.calls, a.warmup)
    rs = min(R, a.cpu_regions)
    q = dict(p, ip=np.ascontiguousarray(p["ip"][:, :, :rs]), y=np.ascontiguousarray(p["y"][:, :rs]),
             new_smoothed=np.ascontiguousarray(p["new_smoothed"][:, :rs]))
    ref = RM.RatemapRef(tempfile.mkdtemp(prefix="ratemap_ref_"))
    t0 = time.perf_counter()
    want = ref.run(q)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    res["c_restatement_one_thread"] = {"regions_run": rs, "ms": cpu_ms, "scaled_ms": cpu_ms * R / rs}
    res["sample_equals_restatement"] = bool(all(RM.same_bits(got[k][..., :rs], want[k]) for k in got))
    res["status_bits"] = {name: int(((got["status"] & bit) != 0).sum()) for name, bit in (("leading_nan", 1), ("not_pd", 2), ("nonfinite", 4))}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

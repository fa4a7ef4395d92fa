"""Measurement of MATLAB's rectangular backslash as one device call (epi_mldiv_run_device; bench.py stays the headline's
yardstick).  Writes profiles/mldivide/bench.json and prints it as one JSON line.

    python tools/bench_mldivide.py                  # 236 regions x 91 row counts (276 .. 366) x 49 columns
    python tools/bench_mldivide.py --small          # 20 regions x 8 row counts x 120 days: a quick run of the same kind
    python tools/bench_mldivide.py --profile-only   # a few calls, for rocprofv3 --kernel-trace --stats

The inputs come from the seeded generator of tests/mldivide_ref.py (synthetic piecewise-constant integer plans, their copies
lagged by 3 / 5 / 7 and a ones column, raw columns; y ~ N(0, 0.05)); the row counts are the last 91 days.  In this process
and on this device (HIP events around each call after warm-up: median, p10, p90):
  call            batch.mldivide, every output
  call_m_only     the same with m, rank and status alone (no X m over all rows)
  rate_map_fit    batch.rate_map's ridge fit at the same shape (F = 48 without the ones column), every output, and
  rate_map_nofit  its clip and rebuild alone: the difference is the fit the backslash stands beside
and on ONE CPU thread the C restatement tests/mldivide_ref.c over a sample of regions, scaled by regions (labelled scaled).
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
    ap.add_argument("--cpu-regions", type=int, default=2)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mldivide", "bench.json"))
    a = ap.parse_args()
    import torch
    from epidemicmodeling_amd import _build, batch
    from tests import mldivide_ref as ML
    from tests import rate_map_ref as RM
    if not torch.cuda.is_available():
        raise SystemExit("bench_mldivide needs a GPU")
    dev = "cuda:0"
    R, K, T = (20, 8, 120) if a.small else (236, 91, 366)
    nr = tuple(range(T - K + 1, T + 1))
    X, y = ML.plans_problem(7, R, T=T, normalised=False)
    F = X.shape[1]
    Xd, yd = torch.as_tensor(X, device=dev), torch.as_tensor(y, device=dev)
    call = lambda: batch.mldivide(Xd, yd, n_rows=nr, device=dev)
    if a.profile_only:
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        return
    res = {"tool": "bench_mldivide", "device": torch.cuda.get_device_name(0), "source_hash": _build.source_hash(),
           "regions": R, "row_counts": K, "rows": T, "columns": F, "items": R * K, "input_bytes": int(X.nbytes + y.nbytes)}
    res["call"] = time_calls(call, a.calls, a.warmup)
    got = {k: v.cpu().numpy() for k, v in call().items()}
    res["output_bytes"] = int(sum(v.nbytes for v in got.values()))
    res["call_m_only"] = time_calls(lambda: batch.mldivide(Xd, yd, n_rows=nr, outputs=("m", "rank", "status"), device=dev), a.calls, a.warmup)
    p = RM.make_case(7, T, 12, (3, 5, 7), 0, K, R, nr)
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v), device=dev)
    ipd, pyd, nsd = t(p["ip"]), t(p["y"]), t(p["new_smoothed"])
    res["rate_map_fit"] = time_calls(lambda: batch.rate_map(ipd, nsd, nr, y=pyd, lags=(3, 5, 7), device=dev), a.calls, a.warmup)
    lam = batch.rate_map(ipd, nsd, nr, y=pyd, lags=(3, 5, 7), outputs=("lambda_hat",), device=dev)["lambda_hat"]
    res["rate_map_nofit"] = time_calls(lambda: batch.rate_map(ipd, nsd, nr, lambda_in=lam, lags=(3, 5, 7), device=dev), a.calls, a.warmup)
    rs = min(R, a.cpu_regions)
    ref = ML.MldivRef(tempfile.mkdtemp(prefix="mldiv_ref_"))
    t0 = time.perf_counter()
    want = ref.run(np.ascontiguousarray(X[:, :, :rs]), np.ascontiguousarray(y[:, :rs]), nr)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    res["c_restatement_one_thread"] = {"regions_run": rs, "ms": cpu_ms, "scaled_ms": cpu_ms * R / rs}
    res["sample_equals_restatement"] = bool(all(ML.same_bits(got[k][..., :rs], want[k]) for k in got))
    res["status_bits"] = {name: int(((got["status"] & bit) != 0).sum()) for name, bit in (("rank_deficient", 1), ("nonfinite_input", 2), ("nonfinite", 4))}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

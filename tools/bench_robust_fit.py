"""Measurement of the element-wise robust regression as one device call (epi_robfit_run_device; bench.py stays the headline's
yardstick).  Writes profiles/robust_fit/bench.json (after every shape) and prints it as one JSON line.

    python tools/bench_robust_fit.py                  # 236 regions x 12 NPIs x 60 days and 4096 x 12 x 366
    python tools/bench_robust_fit.py --small          # 20 x 12 x 60 only: a quick run of the same kind
    python tools/bench_robust_fit.py --profile-only   # a few calls, for rocprofv3 --kernel-trace --stats

X and y come from the seeded generator of tests/robust_fit_ref.py (piecewise-constant NPI levels, alpha affine in one of them
plus noise, a trend, outliers in every fifth region).  In this process and on this device (HIP events around each call after
warm-up: median, p10, p90):
  call   batch.robust_affine_fit, all outputs but the weights
  nnls   batch.nnls_affine_fit on the same X, y (REGRESSION_TYPE 'NONNEGATIVELS', the default regression)
and on ONE CPU thread the C restatement tests/robust_fit_ref.c over a sample of regions, scaled by regions (labelled scaled).
The call's outputs are compared with the restatement on that sample, bit for bit; the iteration counts are summarised."""
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
    ap.add_argument("--cpu-regions", type=int, default=24)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust_fit", "bench.json"))
    a = ap.parse_args()
    import torch
    from epidemicmodeling_amd import _build, batch
    from tests import robust_fit_ref as RF
    if not torch.cuda.is_available():
        raise SystemExit("bench_robust_fit needs a GPU")
    dev = "cuda:0"
    shapes = [(20, 12, 60)] if a.small else [(236, 12, 60), (4096, 12, 366)]
    ref = RF.RobfitRef(tempfile.mkdtemp(prefix="robfit_ref_"))
    res = {"tool": "bench_robust_fit", "device": torch.cuda.get_device_name(0), "source_hash": _build.source_hash(), "shapes": []}
    for R, n, D in shapes:
        X, y = RF.make_case(7, D, n, R)
        Xd, yd = torch.as_tensor(X, device=dev), torch.as_tensor(y, device=dev)
        call = lambda: batch.robust_affine_fit(Xd, yd, device=dev)
        if a.profile_only:
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            continue
        one = {"regions": R, "npis": n, "days": D, "input_bytes": int(X.nbytes + y.nbytes),
               "call": time_calls(call, a.calls, a.warmup)}
        try:
            one["nnls"] = time_calls(lambda: batch.nnls_affine_fit(Xd, yd, device=dev), a.calls, a.warmup)
        except Exception as e:                                   # a shape the NNLS call does not take: recorded, not fatal
            one["nnls"] = {"error": str(e)}
        got = {k: v.cpu().numpy() for k, v in call().items()}
        rs = min(R, a.cpu_regions)
        Xs, ys = np.ascontiguousarray(X[:, :, :rs]), np.ascontiguousarray(y[:, :rs])
        t0 = time.perf_counter()
        want = ref.run(Xs, ys)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        one["c_restatement_one_thread"] = {"regions_run": rs, "ms": cpu_ms, "scaled_ms": cpu_ms * R / rs}
        one["sample_equals_restatement"] = bool(all(RF.same_bits(got[k][..., :rs], want[k]) for k in got))
        it = got["iters"].ravel()
        one["iters"] = {"mean": float(it.mean()), "p90": float(np.percentile(it, 90)), "max": int(it.max())}
        one["status_bits"] = {name: int(((got["status"] & bit) != 0).sum()) for name, bit in
                              (("nonfinite", 1), ("const", 2), ("slope_lost", 4), ("maxiter", 8), ("bound", 16))}
        res["shapes"].append(one)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    if not a.profile_only:
        print(json.dumps(res))


if __name__ == "__main__":
    main()

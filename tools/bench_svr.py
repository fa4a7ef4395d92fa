"""Measurement of the support-vector regression as one device call (epi_svr_run_device; bench.py stays the headline's
yardstick).  Writes profiles/svr/bench.json and prints it as one JSON line.

    python tools/bench_svr.py                  # 236 regions x 91 row counts (276 .. 366) x 366 days x 49 columns, both kernels
    python tools/bench_svr.py --small          # 20 regions x 8 row counts x 120 days: a quick run of the same kind
    python tools/bench_svr.py --profile-only   # one call per kernel, for rocprofv3 --kernel-trace --stats

The inputs come from the seeded generator of tests/svr_ref.py (synthetic piecewise-constant plans with a ones column, every
column divided by its maximum; a target that follows a slow wave, the plans and noise); the row counts are the last 91 days;
box, epsilon and kernel_scale are _lib.svr_defaults of the target, tol = 1e-3.  In this process and on this device (HIP events
around each call after warm-up: median, p10, p90), per kernel:
  call            batch.svr, every output
and beside them, at the same shape,
  mldivide        batch.mldivide on the same X and y
  rate_map_fit    batch.rate_map's ridge fit (F = 48 without the ones column), every output
and on ONE CPU thread the C restatement tests/svr_ref.c over a sample of regions and row counts, scaled by items (labelled
scaled).  Recorded with them: the histogram of n_iter, the share of NOT_CONVERGED items at the chosen max_iter, and whether
the call's outputs equal the restatement on that sample, bit for bit."""
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
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=0, help="calls before the timed ones, beyond the one whose outputs are checked")
    ap.add_argument("--max-iter", type=int, default=100000)
    ap.add_argument("--cpu-regions", type=int, default=2)
    ap.add_argument("--cpu-row-counts", type=int, default=2)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svr", "bench.json"))
    a = ap.parse_args()
    import torch
    from epidemicmodeling_amd import _build, _lib, batch
    from tests import rate_map_ref as RM
    from tests import svr_ref as SV
    if not torch.cuda.is_available():
        raise SystemExit("bench_svr needs a GPU")
    dev = "cuda:0"
    R, K, T = (20, 8, 120) if a.small else (236, 91, 366)
    nr = tuple(range(T - K + 1, T + 1))
    X, y = SV.plans(7, T, 49, R)
    F = X.shape[1]
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v), device=dev)
    Xd, yd = t(X), t(y)
    res = {"tool": "bench_svr", "device": torch.cuda.get_device_name(0), "source_hash": _build.source_hash(), "regions": R,
           "row_counts": K, "rows": T, "columns": F, "items": R * K, "tol": 1e-3, "max_iter": a.max_iter,
           "input_bytes": int(X.nbytes + y.nbytes)}
    ref = SV.SvrRef(tempfile.mkdtemp(prefix="svr_ref_"))
    rs, ks = min(R, a.cpu_regions), min(K, a.cpu_row_counts)
    for kernel in SV.KERNELS:
        h = {k: t(v) for k, v in _lib.svr_defaults(y, kernel).items()}
        call = lambda: batch.svr(Xd, yd, n_rows=nr, kernel=kernel, tol=1e-3, max_iter=a.max_iter, device=dev, **h)
        if a.profile_only:
            call()
            torch.cuda.synchronize()
            continue
        got = {k: v.cpu().numpy() for k, v in call().items()}       # the first call: the outputs that are checked, and the warm-up
        print(kernel, "first call done", file=sys.stderr, flush=True)
        r = {"call": time_calls(call, a.calls, a.warmup)}
        print(kernel, r["call"], file=sys.stderr, flush=True)
        it = got["n_iter"].ravel()
        edges = [0, 1, 10, 100, 300, 1000, 3000, 10000, 30000, 100000, 10000001]
        r["n_iter_histogram"] = {f"{lo}..{hi - 1}": int(((it >= lo) & (it < hi)).sum()) for lo, hi in zip(edges[:-1], edges[1:])}
        r["n_iter_median"], r["n_iter_max"], r["n_iter_sum"] = float(np.median(it)), int(it.max()), int(it.sum())
        r["not_converged_share"] = float(((got["status"] & SV.NOT_CONVERGED) != 0).mean())
        r["status_bits"] = {name: int(((got["status"] & bit) != 0).sum()) for name, bit in _lib.SVR_STATUS_BITS.items()}
        hh = {k: v.cpu().numpy()[:rs] for k, v in h.items()}
        t0 = time.perf_counter()
        want = ref.run(np.ascontiguousarray(X[:, :, :rs]), np.ascontiguousarray(y[:, :rs]), nr[:ks], kernel, hh["box"], hh["epsilon"],
                       hh["kernel_scale"], 1e-3, a.max_iter)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        r["c_restatement_one_thread"] = {"items_run": rs * ks, "ms": cpu_ms, "scaled_ms": cpu_ms * R * K / (rs * ks)}
        r["sample_equals_restatement"] = bool(all(SV.same_bits(got[k][:ks, ..., :rs], want[k]) for k in want))
        res[kernel] = r
    if a.profile_only:
        return
    res["mldivide"] = time_calls(lambda: batch.mldivide(Xd, yd, n_rows=nr, device=dev), a.calls, a.warmup)
    p = RM.make_case(7, T, 12, (3, 5, 7), 0, K, R, nr)
    ipd, pyd, nsd = t(p["ip"]), t(p["y"]), t(p["new_smoothed"])
    res["rate_map_fit"] = time_calls(lambda: batch.rate_map(ipd, nsd, nr, y=pyd, lags=(3, 5, 7), device=dev), a.calls, a.warmup)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Measurement of the autoregressive alpha forecaster as one device call (epi_arfc_run_device; bench.py stays the headline's
yardstick).  Writes profiles/ar_forecast/bench.json and prints it as one JSON line.

    python tools/bench_ar_forecast.py                   # 236 regions x 1024 draws x (120 + 90) days, order 24
    python tools/bench_ar_forecast.py --regions 20      # a smaller run of the same kind
    python tools/bench_ar_forecast.py --profile-only    # a few calls, for rocprofv3 --kernel-trace --stats

The segments are synthetic alpha-like series (a stable AR(2) around 0.3, one realisation per region); the draws are
torch.randn.  In this process and on this device (HIP events around each call after warm-up: median, p10, p90):
  call         batch.ar_forecast (fit + simulation, S [K, 3, B] written)
  composition  the obvious torch composition: torch.linalg.lstsq on the stacked matrix of every region, a Python loop over
               the H forecast days (one batched matrix-vector product per day), the clamp, batch.si_controlled
and a fixed sample of chains of the call's result is compared with the composition (the two differ by the conditioning of
the least-squares problem, not bit for bit: the worst difference is reported, nothing is asserted on it)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_segments(R, L, seed=5):
    rng = np.random.default_rng(seed)
    w = np.zeros((L + 200, R))
    e = rng.standard_normal((L + 200, R))
    for t in range(2, L + 200):
        w[t] = 1.2 * w[t - 1] - 0.5 * w[t - 2] + 0.02 * e[t]
    return np.ascontiguousarray(0.3 + w[200:])


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


def torch_composition(seg, chain_prm, z, p, H, D, device):
    """lstsq + a Python loop over the horizon + batch.si_controlled -> S [K, 3, B]; chain_prm = (beta, s0, i0) per CHAIN as
    NumPy arrays, expanded outside the timed region"""
    import torch
    from epidemicmodeling_amd import batch
    L, R = seg.shape
    y = seg.T                                                                        # [R, L]
    t = torch.arange(p, L, device=seg.device)
    Xf = torch.stack([y[:, t - k] for k in range(1, p + 1)], dim=2)                  # [R, L - p, p]
    Xb = torch.stack([y[:, t - p + k] for k in range(1, p + 1)], dim=2)
    X, b = torch.cat([Xf, Xb], dim=1), torch.cat([y[:, t], y[:, t - p]], dim=1)
    a = torch.linalg.lstsq(X, -b[:, :, None]).solution[:, :, 0]                      # [R, p]
    e = b + (X @ a[:, :, None])[:, :, 0]
    nv = (e * e).sum(dim=1) / (2 * (L - p))
    b0 = torch.sqrt(nv).repeat_interleave(D)                                         # [B]
    ac = a.repeat_interleave(D, dim=0)                                               # [B, p]
    past = y[:, L - p:].flip(1).repeat_interleave(D, dim=0).contiguous()             # [B, p]: y(t-1) .. y(t-p)
    ys = []
    for h in range(H):
        v = b0 * z[h] - (ac * past).sum(dim=1)
        ys.append(v)
        past = torch.cat([v[:, None], past[:, :-1]], dim=1)
    al = torch.cat([seg.repeat_interleave(D, dim=1), torch.stack(ys)]).clamp_min(0.0)            # [K, B]
    s, i = batch.si_controlled(al[:-1].contiguous(), *chain_prm, L + H, 1.0, device=device)
    return torch.stack([s, i, al], dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=236)
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--history", type=int, default=120)
    ap.add_argument("--horizon", type=int, default=90)
    ap.add_argument("--order", type=int, default=24)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ar_forecast", "bench.json"))
    a = ap.parse_args()
    import torch
    from epidemicmodeling_amd import _build, batch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ar_forecast needs a GPU")
    dev = "cuda:0"
    R, D, L, H, p = a.regions, a.draws, a.history, a.horizon, a.order
    seg = torch.as_tensor(make_segments(R, L), device=dev)
    rng = np.random.default_rng(6)
    beta = torch.as_tensor(rng.uniform(0.1, 0.3, R), device=dev)
    s0 = torch.as_tensor(rng.uniform(0.9, 0.999, R), device=dev)
    i0 = 1.0 - s0
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    z = torch.randn((H, R * D), dtype=torch.float64, device=dev, generator=g)
    call = lambda: batch.ar_forecast(seg, beta, s0, i0, 1.0, p, H, D, z=z)
    if a.profile_only:
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        return
    chain_prm = tuple(v.repeat_interleave(D).cpu().numpy() for v in (beta, s0, i0))
    comp = lambda: torch_composition(seg, chain_prm, z, p, H, D, dev)
    res = {"tool": "bench_ar_forecast", "device": torch.cuda.get_device_name(0), "source_hash": _build.source_hash(),
           "shape": {"regions": R, "draws": D, "history": L, "horizon": H, "order": p},
           "output_bytes": (L + H) * 3 * R * D * 8, "call": time_calls(call, a.calls, a.warmup),
           "composition": time_calls(comp, max(3, a.calls // 4), 1)}
    got, want = call(), comp()
    torch.cuda.synchronize()
    sample = torch.arange(0, R * D, max(1, (R * D) // 997), device=dev)
    res["status_counts"] = np.bincount(got["status"].cpu().numpy(), minlength=3).tolist()
    res["worst_abs_difference_on_sample"] = float((got["S"][:, :, sample] - want[:, :, sample]).abs().nan_to_num(0.0).max())
    res["speedup_over_composition"] = res["composition"]["median_ms"] / res["call"]["median_ms"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

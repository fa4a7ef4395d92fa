"""Measurement of the Monte-Carlo ensemble statistics as one device call (epi_ens_run_device; bench.py stays the headline's
yardstick).  Writes profiles/ens_summary/bench.json and prints it as one JSON line.

    python tools/bench_ens_summary.py                   # config 5's shape: 300 regions x 1024 draws x 400 days, 3 rows + new cases
    python tools/bench_ens_summary.py --regions 30      # a smaller run of the same kind
    python tools/bench_ens_summary.py --profile-only    # a few calls, for rocprofv3 --kernel-trace --stats

The source is a synthetic S_SMOOTH-like array [T, 3, R * D] (susceptible and infected fractions and a rate, every chain its
own draw; a few NaN members planted), in float32 and in float64 storage.  Per storage, in this process and on this device
(HIP events around each call after warm-up: median, p10, p90):
  call         batch.ensemble_summary with the population (mean, std, min, max, 5 quantiles, count of 4 rows)
  copy         a device-to-device copy of the source: the call's byte floor (every value read once, and written once more)
  composition  what a caller would write with torch today, in the source's own dtype: the new-case row, torch.sort along the
               draws, gathers and the interpolation for the same quantiles, torch.mean / torch.std (no NaN handling: it is
               timed on the source before the NaNs are planted)
and a fixed sample of items of the call's result is compared, value for value, with tests/ens_summary_ref.py."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q = (0.025, 0.25, 0.5, 0.75, 0.975)


def make_source(R, D, T, dtype, device):
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(5)
    B = R * D
    src = torch.empty((T, 3, B), dtype=dtype, device=device)
    day = torch.linspace(0.0, 1.0, T, device=device, dtype=torch.float64)[:, None]
    for row, (lo, hi, jit) in enumerate(((1.0, 0.9, 1e-3), (1e-4, 2e-2, 0.2), (0.6, 0.3, 0.05))):
        z = torch.randn((T, B), generator=g, device=device, dtype=torch.float64)
        src[:, row] = ((lo + (hi - lo) * day) * (1.0 + jit * z)).to(dtype)
    return src


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


def torch_composition(src, pop, R, D):
    """mean, std, min, max and the hazen quantiles of 3 rows + the new-case row with torch alone (no NaN members)"""
    import torch
    T = src.shape[0]
    s = src.view(T, 3, R, D)
    new = ((pop.to(src.dtype)[None, :, None] * s[:, 0]) * s[:, 1]) * s[:, 2]
    s = torch.cat([s, new[:, None]], dim=1)
    srt = torch.sort(s, dim=-1).values
    out = {"mean": s.mean(dim=-1), "std": s.std(dim=-1), "min": srt[..., 0], "max": srt[..., -1]}
    qs = []
    for p in Q:
        h = D * p + 0.5
        k = int(np.floor(h))
        g = h - k
        if k < 1:
            qs.append(srt[..., 0])
        elif k >= D:
            qs.append(srt[..., D - 1])
        else:
            lo, hi = srt[..., k - 1], srt[..., k]
            qs.append(lo + g * (hi - lo))
    out["quantiles"] = torch.stack(qs, dim=1)
    return out


def check_sample(src, pop, res, R, D, n_items=24):
    """a fixed sample of items (days, rows incl. the derived one, regions spread over the arrays) against the reference"""
    from tests import ens_summary_ref as E
    T = src.shape[0]
    rng = np.random.default_rng(0)
    bad, items = [], []
    for i in range(n_items):
        t, row, r = int(rng.integers(T)) if i else 0, i % 4, int(rng.integers(R)) if i > 1 else 0
        rows = src[t, :, r * D:(r + 1) * D].cpu().numpy().astype(np.float64)
        v = rows[row] if row < 3 else ((float(pop[r]) * rows[0]) * rows[1]) * rows[2]
        want = E.item(v, Q)
        for k in ("mean", "std", "min", "max", "count"):
            g = res[k][t, row, r].item()
            if not (g == want[k] or (np.isnan(g) and np.isnan(want[k]))):
                bad.append([t, row, r, k, g, float(want[k])])
        gq = res["quantiles"][t, :, row, r].cpu().numpy()
        if not ((gq == want["quantiles"]) | (np.isnan(gq) & np.isnan(want["quantiles"]))).all():
            bad.append([t, row, r, "quantiles", gq.tolist(), want["quantiles"].tolist()])
        items.append([t, row, r])
    return {"items": len(items), "mismatches": bad}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=300)
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--days", type=int, default=400)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ens_summary", "bench.json"))
    args = ap.parse_args()
    import torch
    from epidemicmodeling_amd import _build, batch
    _build.build_library()
    device = "cuda:0"
    R, D, T = args.regions, args.draws, args.days
    pop = torch.as_tensor(np.random.default_rng(1).uniform(1e5, 1e8, R), device=device)
    res = {"shape": {"R": R, "D": D, "T": T, "rows": 3, "derived_row": 1, "q": list(Q)}, "timing": "HIP events around each call",
           "source_hash": _build.source_hash(), "gpu": torch.cuda.get_device_name(0)}
    for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        src = make_source(R, D, T, dtype, device)
        call = lambda: batch.ensemble_summary(src, R, D, q=Q, population=pop)
        if args.profile_only:
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            continue
        r = {"source_bytes": src.numel() * src.element_size()}
        dst = torch.empty_like(src)
        r["copy"] = time_calls(lambda: dst.copy_(src), args.calls, 2)
        del dst
        r["call"] = time_calls(call, args.calls, 2)
        r["composition"] = time_calls(lambda: torch_composition(src, pop, R, D), max(3, args.calls // 3), 1)
        comp = torch_composition(src, pop, R, D)
        got = call()
        r["call_vs_composition_max_rel_diff"] = {k: float(((got[k] - comp[k].double()).abs() / comp[k].double().abs().clamp_min(1e-300)).max())
                                                 for k in ("mean", "std", "min", "max", "quantiles")}
        del comp
        torch.cuda.empty_cache()
        flat = src.view(-1)
        flat[torch.arange(0, flat.numel(), 1000003, device=device)] = float("nan")          # NaN members for the checked call
        got = call()
        torch.cuda.synchronize()
        r["reference_check"] = check_sample(src, pop.cpu().numpy(), got, R, D)
        r["nan_members"] = int((got["count"][:, :3] != D).sum().item())
        r["call_faster_than_composition"] = bool(r["call"]["median_ms"] < r["composition"]["median_ms"])
        r["call_over_copy"] = r["call"]["median_ms"] / r["copy"]["median_ms"]
        res[name] = r
        del src, got
        torch.cuda.empty_cache()
    if args.profile_only:
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

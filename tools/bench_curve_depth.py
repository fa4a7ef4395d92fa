"""Measurement of the curve statistics as one device call (epi_cdepth_run_device; bench.py stays the headline's yardstick).  Writes
profiles/curve_depth/bench.json and prints it as one JSON line.

    python tools/bench_curve_depth.py                   # the documented shape: 300 regions x 1024 draws x 120 and 520 days, 3 rows + new cases
    python tools/bench_curve_depth.py --regions 30      # a smaller run of the same kind
    python tools/bench_curve_depth.py --profile-only    # a few calls, for rocprofv3 --kernel-trace --stats

The source is a synthetic S_SMOOTH-like array [T, 3, R * D] without NaN, in float64 and in float32 storage.  Per storage and number
of days, in this process and on this device, after a warm-up of every member,
  cdepth   batch.curve_statistics with the population: every output, alpha = (0.5, 0.9), the functional boxplot
  torch    the same outputs formulated in torch on the device (torch_formulation: per-day argsort of argsort for the ranks, which
           is the same quantity on tie-free values, integer sums, a sort of the depths, masked amin / amax)
  copy     a device-to-device copy of the source bytes
run in alternation, one call of each per round, HIP events around each call.  The record holds each member's median, minimum and
maximum, the two ratios, whether the call's slowest run beat torch's fastest (`gate`), torch's peak temporaries, and how many of
the float64 call's band counts differ from torch's (they are exact integers: none may)."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALPHA, FENCE_FACTOR, FENCE_FRAC = (0.5, 0.9), 1.5, 0.5
DAYS = (120, 520)


def source_bytes(R, D, T, elem, rows=3):
    """bytes of the source array: what the call has to read at least once"""
    return int(T) * int(rows) * int(R) * int(D) * int(elem)


def waves(R, T, rows=3, derive=1):
    """wavefronts of the depth pass: one per (row, region, 32-day block)"""
    return (int(rows) + int(derive)) * int(R) * ((int(T) + 31) // 32)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "calls": len(ms)}


def ratios(r):
    """the figures DESIGN.md 4.23 quotes, from the timings of one storage and length; gate: the ranges do not overlap"""
    return {"torch_over_cdepth": r["torch"]["median_ms"] / r["cdepth"]["median_ms"],
            "cdepth_over_copy": r["cdepth"]["median_ms"] / r["copy"]["median_ms"],
            "gate": bool(r["cdepth"]["max_ms"] < r["torch"]["min_ms"])}


def deepest(f, n):
    return min(n, max(1, int(np.ceil(float(f) * float(n)))))


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


def torch_formulation(src, pop, R, D):
    """the outputs of the call in torch, for values without NaN and without ties"""
    import torch
    T = src.shape[0]
    x = src.double() if src.dtype != torch.float64 else src
    pr = pop.repeat_interleave(D)[None, :]
    x = torch.cat([x, (((pr * x[:, 0]) * x[:, 1]) * x[:, 2])[:, None]], dim=1).view(T, 4, R, D)
    rank = x.argsort(dim=-1).argsort(dim=-1) + 1                            # 1 .. D on every day
    band = ((rank - 1) * (D - rank) + (D - 1)).sum(dim=0)
    le = rank.sum(dim=0)
    pairs = T * (D * (D - 1) // 2)
    depth, mhi = band.double() / float(pairs), le.double() / float(T * D)
    drank = (-depth).argsort(dim=-1, stable=True).argsort(dim=-1)
    inf = float("inf")
    env = lambda keep: (torch.where(keep[None], x, inf).amin(dim=-1), torch.where(keep[None], x, -inf).amax(dim=-1))
    lo_hi = [env(drank < deepest(a, D)) for a in ALPHA]
    median_path = drank.argmin(dim=-1)
    median_curve = x.gather(-1, median_path[None, ..., None].expand(T, 4, R, 1))[..., 0]
    flo, fhi = env(drank < deepest(FENCE_FRAC, D))
    fw = FENCE_FACTOR * (fhi - flo)
    out_days = ((x < (flo - fw)[..., None]) | (x > (fhi + fw)[..., None])).sum(dim=0)
    wlo, whi = env(out_days == 0)
    return dict(depth=depth, mhi=mhi, band_count=band, depth_rank=drank, median_path=median_path,
                env_lo=torch.stack([l for l, _ in lo_hi], dim=1), env_hi=torch.stack([h for _, h in lo_hi], dim=1),
                median_curve=median_curve, out_days=out_days, n_outliers=(out_days > 0).sum(dim=-1), whisk_lo=wlo, whisk_hi=whi)


def alternate(fns, rounds):
    """one call of each of `fns` per round, events around each: {name: [ms]}"""
    import torch
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=300)
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--days", type=int, nargs="*", default=list(DAYS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from epidemicmodeling_amd import _build, batch
    _build.build_library()
    device = "cuda:0"
    R, D = args.regions, args.draws
    pop = torch.as_tensor(np.random.default_rng(1).uniform(1e5, 1e8, R), device=device)
    res = {"shape": {"R": R, "D": D, "days": list(args.days), "rows": 3, "derived_row": 1, "alpha": list(ALPHA),
                     "fence_factor": FENCE_FACTOR, "fence_frac": FENCE_FRAC},
           "timing": "HIP events around each call; cdepth, torch and copy alternate, one call of each per round",
           "source_hash": _build.source_hash(), "gpu": torch.cuda.get_device_name(0)}
    for T in args.days:
        for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            src = make_source(R, D, T, dtype, device)
            dst = torch.empty_like(src)
            call = lambda: batch.curve_statistics(src, R, D, alpha=ALPHA, fence_factor=FENCE_FACTOR, fence_frac=FENCE_FRAC, population=pop)
            if args.profile_only:
                for _ in range(3):
                    call()
                torch.cuda.synchronize()
                continue
            fns = {"cdepth": call, "torch": lambda: torch_formulation(src, pop, R, D), "copy": lambda: dst.copy_(src)}
            alternate(fns, 1)                                              # warm-up: code objects, allocator, clocks
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            torch_formulation(src, pop, R, D)
            torch.cuda.synchronize()
            peak = int(torch.cuda.max_memory_allocated() - base)
            r = {k: stats(v) for k, v in alternate(fns, max(5, args.rounds)).items()}
            r.update(source_bytes=source_bytes(R, D, T, src.element_size()), waves=waves(R, T), torch_peak_extra_bytes=peak)
            r.update(ratios(r))
            if name == "f64":                                               # exact integers on tie-free values: none may differ
                got, want = call(), torch_formulation(src, pop, R, D)
                r["band_count_mismatches"] = int((got["band_count"].view(4, R, D) != want["band_count"].double()).sum().item())
                r["depth_rank_mismatches"] = int((got["depth_rank"].view(4, R, D) != want["depth_rank"]).sum().item())
                del got, want
            res.setdefault(f"days_{T}", {})[name] = r
            del src, dst
            torch.cuda.empty_cache()
    if args.profile_only:
        return
    res["gate"] = all(r["gate"] for k, v in res.items() if k.startswith("days_") for r in v.values())
    out = args.out or os.path.join(ROOT, "profiles", "curve_depth", "bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

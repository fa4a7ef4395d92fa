"""Measurement of the probabilistic forecast scores as one device call (epi_escore_run_device; bench.py stays the headline's
yardstick).  Writes profiles/ens_score/bench.json and prints it as one JSON line.

    python tools/bench_ens_score.py                   # config 5's shape: 300 regions x 1024 draws x 400 days, 3 rows + new cases
    python tools/bench_ens_score.py --regions 30      # a smaller run of the same kind
    python tools/bench_ens_score.py --profile-only    # a few calls, for rocprofv3 --kernel-trace --stats

The source is the synthetic S_SMOOTH-like array [T, 3, R * D] of tools/bench_ens_summary.py (a few NaN members planted), in
float32 and in float64 storage; the truth of every item is the mean of the first eight draws of its region, so it lies inside
the ensemble.  Per storage, in this process and on this device, after a warm-up of every call and of the clocks, the three
  score     batch.ensemble_score with the population: every output (crps, wis, ae, width, rank, ties, cover, count of 4 rows,
            the per-region means, coverage and the 10-bin rank histogram) at the levels 0.5 and 0.05
  summary   batch.ensemble_summary with the population and five quantiles on the same array: the same loads and the same sort
  copy      a device-to-device copy of the source: the byte floor (every value read once, and written once more)
run in alternation, one call of each per round, HIP events around each call (median, p10, p90); score_over_summary and
score_over_copy are the ratios of the medians, summary_spread the (p90 - p10) / median of ensemble_summary in the same rounds.
A fixed sample of items of the call's result is compared bit for bit with tests/escore_ref.py."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q = (0.025, 0.25, 0.5, 0.75, 0.975)
ALPHA = (0.5, 0.05)
N_BINS = 10


def source_bytes(R, D, T, elem, rows=3):
    """bytes of the source array: what the call has to read once"""
    return int(T) * int(rows) * int(R) * int(D) * int(elem)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)),
            "calls": len(ms)}


def ratios(r):
    """the figures DESIGN.md 4.17 quotes, from the three timings of one storage"""
    return {"score_over_summary": r["score"]["median_ms"] / r["summary"]["median_ms"],
            "score_over_copy": r["score"]["median_ms"] / r["copy"]["median_ms"],
            "summary_spread": (r["summary"]["p90_ms"] - r["summary"]["p10_ms"]) / r["summary"]["median_ms"]}


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


def make_truth(src, pop, R, D):
    """[T, 4, R]: the mean of the first eight draws of every region, the new-case row from those means"""
    import torch
    T = src.shape[0]
    m = src.view(T, 3, R, D)[..., :min(8, D)].double().mean(dim=-1)
    new = ((pop[None, :] * m[:, 0]) * m[:, 1]) * m[:, 2]
    return torch.cat([m, new[:, None]], dim=1).contiguous()


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


def check_sample(src, truth, pop, res, R, D, n_items=24):
    """a fixed sample of items (days, rows incl. the derived one, regions spread over the arrays) against the restatement"""
    from tests import escore_ref as S
    T = src.shape[0]
    rng = np.random.default_rng(0)
    bad, n = [], 0
    for i in range(n_items):
        t, row, r = int(rng.integers(T)) if i else 0, i % 4, int(rng.integers(R)) if i > 1 else 0
        rows = src[t, :, r * D:(r + 1) * D].cpu().numpy().astype(np.float64)
        v = rows[row] if row < 3 else ((float(pop[r]) * rows[0]) * rows[1]) * rows[2]
        want = S.item(v, truth[t, row, r].item(), ALPHA)
        for k in ("crps", "wis", "ae", "rank", "ties", "cover", "count"):
            if not S.same_bits(np.asarray(res[k][t, row, r].item()), np.asarray(want[k], dtype=np.asarray(res[k][t, row, r].item()).dtype)):
                bad.append([t, row, r, k, res[k][t, row, r].item(), float(want[k])])
        if not S.same_bits(res["width"][t, :, row, r].cpu().numpy(), want["width"]):
            bad.append([t, row, r, "width"])
        n += 1
    return {"items": n, "mismatches": bad}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=300)
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--days", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ens_score", "bench.json"))
    args = ap.parse_args()
    import torch
    from epidemicmodeling_amd import _build, batch
    _build.build_library()
    device = "cuda:0"
    R, D, T = args.regions, args.draws, args.days
    pop = torch.as_tensor(np.random.default_rng(1).uniform(1e5, 1e8, R), device=device)
    res = {"shape": {"R": R, "D": D, "T": T, "rows": 3, "derived_row": 1, "alpha": list(ALPHA), "n_bins": N_BINS, "q": list(Q)},
           "timing": "HIP events around each call; score, summary and copy alternate, one call of each per round",
           "source_hash": _build.source_hash(), "gpu": torch.cuda.get_device_name(0)}
    for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        src = make_source(R, D, T, dtype, device)
        flat = src.view(-1)
        flat[torch.arange(0, flat.numel(), 1000003, device=device)] = float("nan")          # NaN members
        truth = make_truth(torch.nan_to_num(src, nan=0.5), pop, R, D)
        dst = torch.empty_like(src)
        fns = {"score": lambda: batch.ensemble_score(src, truth, R, D, alpha=ALPHA, n_bins=N_BINS, population=pop),
               "summary": lambda: batch.ensemble_summary(src, R, D, q=Q, population=pop),
               "copy": lambda: dst.copy_(src)}
        if args.profile_only:
            for _ in range(3):
                fns["score"]()
            torch.cuda.synchronize()
            continue
        alternate(fns, 6)                                                                    # warm-up: code objects, allocator, clocks
        torch.cuda.synchronize()
        r = {k: stats(v) for k, v in alternate(fns, args.rounds).items()}
        r["source_bytes"] = source_bytes(R, D, T, src.element_size())
        r.update(ratios(r))
        got = fns["score"]()
        torch.cuda.synchronize()
        r["reference_check"] = check_sample(src, truth, pop.cpu().numpy(), got, R, D)
        r["scored_items"] = int((got["rank"] >= 0).sum().item())
        r["cover_frac_mean"] = [float(v) for v in got["cover_frac"].mean(dim=(1, 2)).cpu().numpy()]
        res[name] = r
        del src, dst, got, truth
        torch.cuda.empty_cache()
    if args.profile_only:
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Measurement of the joint scores (energy score, variogram score) as one device call (epi_ejoint_run_device; bench.py stays the
headline's yardstick).  Writes profiles/ens_joint/bench.json and prints it as one JSON line.

    python tools/bench_ens_joint.py                   # 300 regions x 1024 draws x the 120-day forecast window, 3 rows + new cases
    python tools/bench_ens_joint.py --regions 30      # a smaller run of the same kind
    python tools/bench_ens_joint.py --profile-only    # a few calls, for rocprofv3 --kernel-trace --stats

The source is the synthetic array [T, 3, R * D] of tools/bench_ens_score.py (a few NaN members planted), in float32 and in
float64 storage, with that tool's truth.  Per storage, in this process and on this device, after a warm-up of every call and of
the clocks, these run in alternation, one call of each per round, HIP events around each call (median, p10, p90):
  es          batch.ensemble_joint_score, outputs es, truth_term, spread_term, n_members, n_days: the pre-pass, the pair tiles,
              the final pass
  vs_all      the same call with outputs vs only, p = 0.5, every pair of days (max_lag = 0)
  vs_lag7     the same with max_lag = 7
  torch_es    the energy score formulated in torch: the derived row and the float64 copy of the source formed once per call, then
              per chunk of regions torch.cdist in float64 over every item's members and its sum (the temporaries' bytes are
              recorded; members with a NaN are not taken out, so it does less than the call).  torch.cdist as one writes it: for
              this many members it forms the distances from a matrix product, |a|^2 + |b|^2 - 2 a.b
  torch_exact the same with compute_mode="donot_use_mm_for_euclid_dist": the differences formed member by member, as the call
              forms them
  escore      batch.ensemble_score on the same array and truth, for scale
es_over_torch is the ratio of the medians.  pair_flops counts three float64 operations per pair of members and day over the
n (n - 1) / 2 pairs the score needs; tile_flops counts what the tiles execute (64 x 64 per tile, the diagonal tiles' lower halves
included); both are divided by the es call's median, which includes the pre-pass and the final pass, and set beside the device's
vector float64 peak (78.6e12 a second counting a fused multiply-add as two; the call's operations are single adds and
multiplies, because every operation of the definition is rounded, so its ceiling is half of that).  reread_bytes is an item's
bytes times its tiles: what the pair kernel asks of L2, against the call's time.
A fixed sample of items of the call's result is compared bit for bit with tests/ejoint_ref.py."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP64_VECTOR = 78.6e12          # MI355X, vector float64, a fused multiply-add counted as two operations
ROWS_OUT = 4


def tiles(D):
    nb = (int(D) + 63) // 64
    return nb * (nb + 1) // 2


def pair_flops(R, D, W, rows_out=ROWS_OUT):
    """three float64 operations (subtract, multiply, add) per pair of members and day, over the pairs the score needs"""
    return 3 * int(rows_out) * int(R) * (int(D) * (int(D) - 1) // 2) * int(W)


def tile_flops(R, D, W, rows_out=ROWS_OUT):
    """the same three operations over what the tiles execute: 64 x 64 pairs per tile"""
    return 3 * int(rows_out) * int(R) * tiles(D) * 4096 * int(W)


def reread_bytes(R, D, W, elem, rows_out=ROWS_OUT):
    """what the pair kernel loads: every tile reads two blocks of 64 members on every day (three source rows for the derived row)"""
    per_tile_day = 2 * 64 * int(elem)
    return int(R) * tiles(D) * int(W) * per_tile_day * (int(rows_out) - 1 + 3)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)),
            "calls": len(ms)}


def rates(r, R, D, W, elem):
    """the figures DESIGN.md 4.20 quotes, from the timings of one storage"""
    s = r["es"]["median_ms"] * 1e-3
    return {"es_over_torch": r["es"]["median_ms"] / r["torch_es"]["median_ms"],
            "torch_over_es": r["torch_es"]["median_ms"] / r["es"]["median_ms"],
            "torch_exact_over_es": r["torch_exact"]["median_ms"] / r["es"]["median_ms"],
            "es_over_escore": r["es"]["median_ms"] / r["escore"]["median_ms"],
            "pair_flops": pair_flops(R, D, W), "tile_flops": tile_flops(R, D, W),
            "pair_flops_per_s": pair_flops(R, D, W) / s, "tile_flops_per_s": tile_flops(R, D, W) / s,
            "peak_fp64_vector_flops_per_s": PEAK_FP64_VECTOR,
            "tile_share_of_peak": tile_flops(R, D, W) / s / PEAK_FP64_VECTOR,
            "tile_share_of_unfused_peak": tile_flops(R, D, W) / s / (PEAK_FP64_VECTOR / 2),
            "reread_bytes": reread_bytes(R, D, W, elem), "reread_bytes_per_s": reread_bytes(R, D, W, elem) / s}


def torch_energy_score(src, truth, pop, R, D, chunk=25, compute_mode="use_mm_for_euclid_dist_if_necessary"):
    """es [4, R] in torch, and the bytes of its temporaries: the float64 rows with the derived one, then per chunk of regions the
    [chunk * 4, D, D] distance matrices of torch.cdist"""
    import torch
    T = src.shape[0]
    s = src.double()
    s = torch.cat([s, (((pop.repeat_interleave(D)[None, :] * s[:, 0]) * s[:, 1]) * s[:, 2])[:, None]], dim=1)     # [T, 4, B]
    x = s.view(T, ROWS_OUT, R, D).permute(1, 2, 3, 0)                                                              # [4, R, D, T]
    es = torch.empty((ROWS_OUT, R), dtype=torch.float64, device=src.device)
    tmp = s.numel() * 8
    for r0 in range(0, R, chunk):
        xc = x[:, r0:r0 + chunk].reshape(-1, D, T).contiguous()
        yc = truth[:, :, r0:r0 + chunk].permute(1, 2, 0).reshape(-1, 1, T)
        dist = torch.cdist(xc, xc, compute_mode=compute_mode)
        tt = torch.linalg.vector_norm(xc - yc, dim=2).mean(dim=1)
        es[:, r0:r0 + chunk] = (tt - dist.sum(dim=(1, 2)) / (2.0 * D * D)).view(ROWS_OUT, -1)
        tmp = max(tmp, s.numel() * 8 + xc.numel() * 8 * 2 + dist.numel() * 8)
    return es, tmp


def agreement(got, te, full):
    """|es - torch's| / truth_term over the items without an absent member: the largest, where it is, and how many pass 1e-9"""
    import torch
    rel = torch.where(full, (got["es"] - te).abs() / got["truth_term"], torch.zeros_like(te))
    bad = full & ~(rel <= 1e-9)                             # a NaN counts
    k = int(torch.nan_to_num(rel, nan=float("inf")).argmax().item())
    row, reg = divmod(k, rel.shape[1])
    return {"max_rel_diff": float(rel.view(-1)[k].item()), "at_row_region": [row, reg], "items_over_1e-9": int(bad.sum().item()),
            "es": float(got["es"][row, reg].item()), "torch": float(te[row, reg].item()), "truth_term": float(got["truth_term"][row, reg].item())}


def check_sample(src, truth, pop, res, R, D, vs_p, max_lag, n_items=4):
    """a fixed sample of items (every row, the derived one included; regions spread over the array) against the NumPy restatement"""
    from tests import ejoint_ref as J
    rng = np.random.default_rng(0)
    bad, n = [], 0
    for i in range(n_items):
        row, r = i % ROWS_OUT, int(rng.integers(R)) if i else 0
        rows, tr = src[:, :, r * D:(r + 1) * D].cpu().numpy(), truth[:, :, r:r + 1].cpu().numpy()
        kw = dict(vs_order={0.5: 1, 1: 2}[vs_p], max_lag=max_lag)
        if row < 3:
            want, at = J.joint(rows[:, row:row + 1], tr[:, row:row + 1], 1, D, **kw), 0
        else:
            want, at = J.joint(rows, tr, 1, D, population=pop[r:r + 1], **kw), 3
        for k in ("es", "truth_term", "spread_term", "vs", "n_members", "n_days"):
            if k not in res:
                continue
            g = np.asarray(res[k][row, r].item())
            if not J.same_bits(g, np.asarray(want[k][at, 0]).astype(g.dtype)):
                bad.append([row, r, k, g.item(), float(want[k][at, 0])])
        n += 1
    return {"items": n, "mismatches": bad}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=300)
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--days", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ens_joint", "bench.json"))
    args = ap.parse_args()
    import torch
    from epidemicmodeling_amd import _build, batch
    from tools import bench_ens_score as BS
    _build.build_library()
    device = "cuda:0"
    R, D, T = args.regions, args.draws, args.days
    pop = torch.as_tensor(np.random.default_rng(1).uniform(1e5, 1e8, R), device=device)
    res = {"shape": {"R": R, "D": D, "T": T, "rows": 3, "derived_row": 1, "tiles": tiles(D), "vs_p": 0.5},
           "timing": "HIP events around each call; es, vs_all, vs_lag7, torch_es, torch_exact and escore alternate, one call of each per round",
           "source_hash": _build.source_hash(), "gpu": torch.cuda.get_device_name(0)}
    for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        src = BS.make_source(R, D, T, dtype, device)
        flat = src.view(-1)
        flat[torch.arange(0, flat.numel(), 1000003, device=device)] = float("nan")          # NaN members
        truth = BS.make_truth(torch.nan_to_num(src, nan=0.5), pop, R, D)
        es_names = ("es", "truth_term", "spread_term", "n_members", "n_days")
        fns = {"es": lambda: batch.ensemble_joint_score(src, truth, R, D, population=pop, outputs=es_names),
               "vs_all": lambda: batch.ensemble_joint_score(src, truth, R, D, vs_p=0.5, max_lag=0, population=pop, outputs=("vs",)),
               "vs_lag7": lambda: batch.ensemble_joint_score(src, truth, R, D, vs_p=0.5, max_lag=7, population=pop, outputs=("vs",)),
               "torch_es": lambda: torch_energy_score(src, truth, pop, R, D),
               "torch_exact": lambda: torch_energy_score(src, truth, pop, R, D, compute_mode="donot_use_mm_for_euclid_dist"),
               "escore": lambda: batch.ensemble_score(src, truth, R, D, population=pop)}
        if args.profile_only:
            for _ in range(3):
                fns["es"](), fns["vs_all"]()
            torch.cuda.synchronize()
            continue
        BS.alternate(fns, 2)                                                                 # warm-up: code objects, allocator, clocks
        torch.cuda.synchronize()
        r = {k: stats(v) for k, v in BS.alternate(fns, args.rounds).items()}
        r["source_bytes"] = BS.source_bytes(R, D, T, src.element_size())
        r.update(rates(r, R, D, T, src.element_size()))
        got = fns["es"]()
        got.update(batch.ensemble_joint_score(src, truth, R, D, vs_p=0.5, max_lag=7, population=pop, outputs=("vs",)))
        full = got["n_members"] == D                       # the torch formulations keep members with a NaN: compare where there is none
        r["items_without_absent_members"] = int(full.sum().item())
        for key in ("torch_es", "torch_exact"):
            te, r["torch_temporaries_bytes"] = fns[key]()
            torch.cuda.synchronize()
            r[key]["agreement"] = agreement(got, te, full)
        r["reference_check"] = check_sample(src, truth, pop.cpu().numpy(), got, R, D, 0.5, 7)
        res[name] = r
        del src, got, truth, te
        torch.cuda.empty_cache()
    if args.profile_only:
        return
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

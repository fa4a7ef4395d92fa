"""Measurement of the path functionals as one device call (epi_pathfn_run_device; bench.py stays the headline's yardstick).  Writes
profiles/path_functionals/bench.json (and with --segments profiles/path_functionals/segments.json) and prints it as one JSON line.

    python tools/bench_path_functionals.py                   # the documented shape: 300 regions x 1024 draws x 520 days, 3 rows + new cases
    python tools/bench_path_functionals.py --regions 30      # a smaller run of the same kind
    python tools/bench_path_functionals.py --segments        # the segment rule's crossover: 300 x 64 and 300 x 256 draws, 1 / 2 / 4 / 8 segments
    python tools/bench_path_functionals.py --profile-only    # a few calls, for rocprofv3 --kernel-trace --stats

The source is the synthetic S_SMOOTH-like array [T, 3, R * D] of tools/bench_ens_score.py (a few NaN values planted), in float64
and in float32 storage; the thresholds of every row and region are quantiles of its own values.  Per storage and n_thr in 0, 2, 8,
in this process and on this device, after a warm-up of every call and of the clocks,
  pathfn   batch.path_functionals with the population: every output
  copy     epi_calib_copy_f64_device of source_bytes / 16 doubles: it moves (reads plus writes) the bytes the call reads once
run in alternation, one call of each per round, HIP events around each call (median, p10, p90).  `torch` is the same outputs
formulated in torch on the device (torch_formulation: its passes over arrays of the size of the window, and its peak memory), a
few calls.  even_waves repeats n_thr = 0 at 256 regions: 4 096 wavefronts are four to each of the 1 024 SIMDs, 4 800 are not.  A
fixed sample of paths of the call's result is compared bit for bit with tests/pathfn_ref.py."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_THR = (0, 2, 8)
SEGMENTS = (1, 2, 4, 8)
SIMDS = 1024


def source_bytes(R, D, T, elem, rows=3):
    """bytes of the source array: what the call has to read once"""
    return int(T) * int(rows) * int(R) * int(D) * int(elem)


def waves(R, D, rows=3, derive=1):
    """wavefronts of the path grid of one segment: 64 paths each, one row group for rows 0 .. 2 with the derived row"""
    return ((int(R) * int(D) + 63) // 64) * (rows - 2 if derive else rows)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)),
            "calls": len(ms)}


def ratios(r):
    """the figures DESIGN.md 4.18 quotes, from the timings of one storage and n_thr"""
    out = {"pathfn_over_copy": r["pathfn"]["median_ms"] / r["copy"]["median_ms"],
           "pathfn_gb_per_s": r["source_bytes"] / r["pathfn"]["median_ms"] / 1e6}
    if "torch" in r:
        out["torch_over_pathfn"] = r["torch"]["median_ms"] / r["pathfn"]["median_ms"]
    return out


def best_segments(by_seg):
    """{segments: stats} -> the count with the smallest median"""
    return int(min(by_seg, key=lambda s: by_seg[s]["median_ms"]))


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
    flat = src.view(-1)
    flat[torch.arange(0, flat.numel(), 1000003, device=device)] = float("nan")
    return src


def make_thresholds(src, pop, R, D, n_thr):
    """[n_thr, 4, R]: quantiles (0.5 .. 0.99) over the first eight draws and all days of every row and region"""
    import torch
    if n_thr == 0:
        return None
    T = src.shape[0]
    x = torch.nan_to_num(src.view(T, 3, R, D)[..., :min(8, D)].double(), nan=0.0)
    new = ((pop[None, :, None] * x[:, 0]) * x[:, 1]) * x[:, 2]
    x = torch.cat([x, new[:, None]], dim=1).permute(1, 2, 0, 3).reshape(4, R, -1)
    lev = torch.linspace(0.5, 0.99, n_thr, device=src.device, dtype=torch.float64)
    return torch.quantile(x, lev, dim=2).contiguous()


def torch_formulation(src, pop, thr, R, D):
    """the same outputs in torch: returns (dict, passes), passes the number of kernels that read or write an array of the size of
    the window [T, 4, N] (booleans and int64 included)"""
    import torch
    T = src.shape[0]
    passes = 0
    x = src.double() if src.dtype != torch.float64 else src
    passes += int(src.dtype != torch.float64)
    pr = pop.repeat_interleave(D)[None, :]
    new = ((pr * x[:, 0]) * x[:, 1]) * x[:, 2]
    x = torch.cat([x, new[:, None]], dim=1)
    passes += 2                                          # the three products (a third of a pass each), the concatenation
    valid = ~torch.isnan(x)
    pv, pd = torch.where(valid, x, -torch.inf).max(dim=0)
    mv, md = torch.where(valid, x, torch.inf).min(dim=0)
    total = torch.where(valid, x, 0.0).sum(dim=0)
    nv = valid.sum(dim=0)
    passes += 8
    out = dict(peak_value=pv, peak_day=pd, min_value=mv, min_day=md, total=total, n_valid=nv)
    if thr is not None:
        fc, da, lr = [], [], []
        for j in range(thr.shape[0]):
            ab = valid & (x >= thr[j].repeat_interleave(D, dim=1)[None])
            c = ab.cumsum(dim=0)
            reset = torch.where(ab, 0, c).cummax(dim=0).values
            lr.append((c - reset).max(dim=0).values)
            da.append(c[-1])
            fc.append(torch.where(c[-1] > 0, ab.to(torch.int8).argmax(dim=0), -1))
            passes += 8
        out.update(first_cross=torch.stack(fc), days_above=torch.stack(da), longest_run=torch.stack(lr))
    return out, passes


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


def check_sample(src, pop, thr, res, R, D, n_paths=16):
    """a fixed sample of paths (all rows, the derived one included) against the restatement"""
    from tests import pathfn_ref as S
    rng = np.random.default_rng(0)
    ps = sorted({0, R * D - 1} | {int(v) for v in rng.integers(R * D, size=n_paths - 2)})
    bad = []
    for p in ps:
        r = p // D
        one = src[:, :, p:p + 1].cpu().numpy()
        th = None if thr is None else thr[:, :, r:r + 1].cpu().numpy()
        want = S.functionals(one, 1, 1, th, population=pop[r:r + 1])
        for k in S.PATH_F64 + S.THR_F64 + ("n_valid",):
            if k in res and not S.same_bits(res[k][..., p].cpu().numpy(), want[k][..., 0]):
                bad.append([p, k])
    return {"paths": len(ps), "mismatches": bad}


def calib_copy(n, device):
    import torch
    from epidemicmodeling_amd import _lib
    a, b = torch.zeros(n, dtype=torch.float64, device=device), torch.empty(n, dtype=torch.float64, device=device)
    h = _lib.lib()
    err = C.create_string_buffer(256)

    def fn():
        _lib.check(h.epi_calib_copy_f64_device(a.data_ptr(), b.data_ptr(), n, C.c_void_p(torch.cuda.current_stream().cuda_stream), err), err)
    return fn, (a, b)


def measure_segments(args, device):
    import torch
    from epidemicmodeling_amd import batch
    R, T = args.regions, args.days
    res = {"what": "batch.path_functionals, every output, float64, n_thr = 2, with test_segments forced; HIP events, the segment "
                   "counts alternating per round", "shapes": []}
    pop = torch.as_tensor(np.random.default_rng(1).uniform(1e5, 1e8, R), device=device)
    for D in (64, 256, 1024):
        src = make_source(R, D, T, torch.float64, device)
        thr = make_thresholds(src, pop, R, D, 2)
        fns = {s: (lambda s=s: batch.path_functionals(src, R, D, thresholds=thr, population=pop, test_segments=s)) for s in SEGMENTS}
        alternate(fns, 3)
        torch.cuda.synchronize()
        by = {s: stats(v) for s, v in alternate(fns, args.rounds).items()}
        res["shapes"].append({"R": R, "D": D, "T": T, "waves": waves(R, D), "by_segments": {str(s): v for s, v in by.items()},
                              "best": best_segments(by)})
        del src
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=300)
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--days", type=int, default=520)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--segments", action="store_true")
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from epidemicmodeling_amd import _build, batch
    _build.build_library()
    device = "cuda:0"
    prof = os.path.join(ROOT, "profiles", "path_functionals")
    if args.segments:
        res = measure_segments(args, device)
        res.update(source_hash=_build.source_hash(), gpu=torch.cuda.get_device_name(0))
        out = args.out or os.path.join(prof, "segments.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return
    R, D, T = args.regions, args.draws, args.days
    pop = torch.as_tensor(np.random.default_rng(1).uniform(1e5, 1e8, R), device=device)
    res = {"shape": {"R": R, "D": D, "T": T, "rows": 3, "derived_row": 1, "n_thr": list(N_THR)},
           "timing": "HIP events around each call; pathfn and copy alternate, one call of each per round; torch a few calls of its own",
           "waves": waves(R, D), "waves_per_simd": waves(R, D) / SIMDS,
           "source_hash": _build.source_hash(), "gpu": torch.cuda.get_device_name(0)}
    for name, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        src = make_source(R, D, T, dtype, device)
        sb = source_bytes(R, D, T, src.element_size())
        copy, keep = calib_copy(sb // 16, device)
        res[name] = {}
        for nt in N_THR:
            thr = make_thresholds(src, pop, R, D, nt)
            fns = {"pathfn": lambda: batch.path_functionals(src, R, D, thresholds=thr, population=pop), "copy": copy}
            if args.profile_only:
                for _ in range(3):
                    fns["pathfn"]()
                torch.cuda.synchronize()
                continue
            alternate(fns, 4)                                                                # warm-up: code objects, allocator, clocks
            torch.cuda.synchronize()
            r = {k: stats(v) for k, v in alternate(fns, args.rounds).items()}
            r["source_bytes"] = sb
            got = fns["pathfn"]()
            torch.cuda.synchronize()
            r["reference_check"] = check_sample(src, pop.cpu().numpy(), thr, got, R, D)
            r["paths_with_a_peak"] = int(got["n_paths"].sum().item())
            del got
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            tf = {"torch": lambda: torch_formulation(src, pop, thr, R, D)}
            alternate(tf, 1)
            r["torch"] = stats(alternate(tf, 3)["torch"])
            r["torch"]["passes"] = torch_formulation(src[:2], pop, thr, R, D)[1]
            r["torch"]["peak_extra_bytes"] = int(torch.cuda.max_memory_allocated() - base)
            torch.cuda.empty_cache()
            r.update(ratios(r))
            res[name][f"n_thr_{nt}"] = r
        if not args.profile_only and name == "f64" and R > 256:
            Re = 256                                                                         # four wavefronts to every SIMD exactly
            sub = src[:, :, :Re * D].contiguous()
            fns = {"pathfn": lambda: batch.path_functionals(sub, Re, D, population=pop[:Re])}
            alternate(fns, 3)
            e = stats(alternate(fns, args.rounds)["pathfn"])
            e.update(R=Re, waves=waves(Re, D), waves_per_simd=waves(Re, D) / SIMDS, source_bytes=source_bytes(Re, D, T, 8))
            e["pathfn_gb_per_s"] = e["source_bytes"] / e["median_ms"] / 1e6
            res["even_waves"] = e
            del sub
        del src, keep
        torch.cuda.empty_cache()
    if args.profile_only:
        return
    out = args.out or os.path.join(prof, "bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

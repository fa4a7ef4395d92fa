"""Measurement of the forecast look-ahead error study as one device call (epi_lookahead_run_device; bench.py stays the
headline's yardstick).  Prints one JSON line.

    python tools/bench_lookahead.py                       # article size (236 x 366, F = 91, M = 60) and 300 regions
    python tools/bench_lookahead.py --profile-only        # a few calls per size and shape, for rocprofv3 --kernel-trace --stats
    python tools/bench_lookahead.py --merge TIMING_JSON --kernel-db results.db     # no GPU: fold the rocprofv3 database of a
                                                                                   # --profile-only run into the timing line

Per size: the call's device time (HIP events around each call, >= 20 calls after warm-up: median, min, max, p10, p90) in
both lane mappings of the 3-state filter (epi_lookahead_desc.shape 1 and 3) and in the one the study picks (shape 0);
"algorithmic bytes" = a model of the least HBM traffic the study needs (below) over the call's median time; and the C
oracle's time for the same study (its batched EKF + EKS over the masked chains on n_threads CPU threads, plus the NumPy
tables) -- a baseline, run in full unless --oracle-regions samples it (then scaled by regions and said so)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def algorithmic_bytes(R, LL, F, M):
    """Least traffic of one study, in bytes: the per-region inputs read once; the masked x and R_v written by the expansion
    and read by the forward pass (2 x 2 doubles per chain-day); the forward quantities the smoother needs -- S_MINUS, S_PLUS
    and the six distinct entries of P_MINUS and P_PLUS -- written once and read back once (2 x 18 doubles); S_SMOOTH written
    (3); S_PLUS and S_SMOOTH of the look-ahead days read by the error kernel (6 per table entry); the two tables written and
    read by the statistics (4 per entry) and the statistics written (6 per column)."""
    B = R * F
    n_npi = 12
    inputs = 8 * R * (LL * (3 + n_npi) + 61 + 3 + 9 + 3 + 9 + 9 + 1)
    chain_days = 8 * B * LL * (4 + 36 + 3)
    tables = 8 * F * M * R * (6 + 4) + 8 * M * R * 6
    return inputs + chain_days + tables


def make_case(R, LL):
    from epidemicmodeling_amd import synth
    w = synth.make_cfg3(R, LL)
    N = synth.make_regions(R)["N"].astype(np.float64)
    return w, np.ascontiguousarray(w.x * N[None, :] + 50.0), N


def time_calls(runner, calls, warmup):
    import torch
    for _ in range(warmup):
        runner.run()
    torch.cuda.synchronize(runner.device)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        runner.run()
        b.record()
    torch.cuda.synchronize(runner.device)
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    return {"median": float(np.median(ms)), "min": float(ms.min()), "max": float(ms.max()),
            "p10": float(np.percentile(ms, 10)), "p90": float(np.percentile(ms, 90)), "n": int(ms.size)}


def oracle_ms(w, truth, N, F, M, n_threads, sample):
    from tests import lookahead_ref as LR
    R = w.B
    idx = np.arange(R) if sample <= 0 or sample >= R else np.linspace(0, R - 1, sample).round().astype(int)
    sub = LR.regions(w, idx)
    ens = LR.mask_ensemble(sub, F)
    from tests import helpers as H
    t0 = time.perf_counter()
    ref = H.oracle_batch(ens, n_threads=n_threads, outputs=["S_PLUS", "S_SMOOTH"])
    LR.tables(ref["S_PLUS"], ref["S_SMOOTH"], truth[:, idx], N[idx], F, M)
    ms = (time.perf_counter() - t0) * 1e3
    full = idx.size == R
    return {"ms": ms * (R / idx.size), "n_threads": n_threads, "mode": "full" if full else f"sampled {idx.size} of {R} regions, scaled by {R / idx.size:.2f}",
            "measured_ms": ms, "includes": "C oracle EKF + EKS over the R * F masked chains + NumPy error tables (statistics not timed)"}


def kernel_breakdown(db, sizes, shapes=(0, 1, 3), calls=3):
    """Per-kernel device time of one study call, from the rocprofv3 (--kernel-trace) database of a --profile-only run: its
    calls are cut at every lookahead_expand dispatch, in the order that run makes them (per size, per shape, `calls` calls).
    Returns {size: {shape: {"kernels": {name: mean ns per call}, "sum_ns": ..., "span_ns": first start -> last end}}}."""
    import sqlite3
    rows = sqlite3.connect(db).execute("select name, start, end from kernels order by start").fetchall()
    groups = []
    for name, t0, t1 in rows:
        if "lookahead_expand" in name:
            groups.append([])
        if groups and not name.startswith("__amd_rocclr"):
            groups[-1].append((name, t0, t1))
    per = len(shapes) * calls
    assert len(groups) == len(sizes) * per, (len(groups), sizes)
    out = {}
    for i, sz in enumerate(sizes):
        out[sz] = {}
        for k, sh in enumerate(shapes):
            gs = groups[i * per + k * calls:i * per + (k + 1) * calls]
            acc = {}
            for g in gs:
                for name, t0, t1 in g:
                    acc[name] = acc.get(name, 0.0) + (t1 - t0) / len(gs)
            out[sz][f"shape{sh}"] = {"kernels": dict(sorted(acc.items(), key=lambda kv: -kv[1])), "sum_ns": sum(acc.values()),
                                     "span_ns": float(np.mean([g[-1][2] - g[0][1] for g in gs]))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="236x366,300x366")
    ap.add_argument("--F", type=int, default=91)
    ap.add_argument("--M", type=int, default=60)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--oracle-threads", type=int, default=16)
    ap.add_argument("--oracle-regions", type=int, default=0, help="0 = the oracle runs the whole study")
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--merge", default=None, help="timing JSON line (file) of an earlier run")
    ap.add_argument("--kernel-db", default=None)
    a = ap.parse_args()
    if a.merge:
        res = json.loads([ln for ln in open(a.merge) if ln.startswith("{")][-1])
        sizes = [f"{r['R']}x{r['LL']}" for r in res["sizes"]]
        res["kernel_breakdown"] = kernel_breakdown(a.kernel_db, sizes)
        res["kernel_breakdown_source"] = "rocprofv3 --kernel-trace --stats, separate --profile-only run, mean of 3 calls"
        print(json.dumps(res))
        return
    import torch
    from epidemicmodeling_amd import batch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lookahead needs a GPU")
    res = {"workload": "lookahead_study", "F": a.F, "M": a.M, "device": torch.cuda.get_device_name(0), "sizes": []}
    for sz in a.sizes.split(","):
        R, LL = (int(v) for v in sz.split("x"))
        w, truth, N = make_case(R, LL)
        row = {"R": R, "LL": LL, "chains": R * a.F, "algorithmic_bytes": algorithmic_bytes(R, LL, a.F, a.M), "device_ms": {}}
        for shape in (0, 1, 3):
            r = batch.LookaheadRunner(w, truth, N, a.F, a.M, device="cuda:0", shape=shape)
            if a.profile_only:
                for _ in range(3):
                    r.run()
                torch.cuda.synchronize()
                continue
            row["device_ms"][f"shape{shape}"] = time_calls(r, a.calls, a.warmup)
            del r
            torch.cuda.empty_cache()
        if not a.profile_only:
            med = row["device_ms"]["shape0"]["median"]
            row["GBps_algorithmic"] = row["algorithmic_bytes"] / (med * 1e-3) / 1e9
            row["oracle"] = oracle_ms(w, truth, N, a.F, a.M, a.oracle_threads, a.oracle_regions)
            row["speedup_vs_oracle"] = row["oracle"]["ms"] / med
        res["sizes"].append(row)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""Measurement of the seeded draws (bench.py stays the headline's yardstick).  Writes profiles/noise/bench.json and
prints it as one JSON line.

    python tools/bench_noise.py                  # 300 chains x 1 024 draws x 520 days
    python tools/bench_noise.py --scale 0.1      # a tenth of the chains

In this process and on this device, after warm-up, the members of a case alternating (median, p10, p90):
  (a) paths     the smoother draws on a live runner's arrays, z read (ZM 1) against z generated (ZM 3), and the call asked for rank
                and status only (sdraw_gain alone): sdraw_paths is the call minus that.  HIP events.
  (b) pipeline  pipeline.smoothed_fan end to end, rng="torch" against rng="device": a host clock around the call and a device
                synchronise, and torch's peak allocated bytes of each.
  (c) host      hostapi.smoother_draws with z from host memory against seeded, a host clock around the synchronous call, at
                --host-scale of the chains (the z array alone is 3.8 GB at the full size).
  (d) fill      batch.normal_draws against epi_calib_copy_f64_device over its bytes and against torch.randn of its shape.  HIP events.
Byte counts come from the shapes (fill_bytes, paths_bytes below)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fill_bytes(nt, rows, lanes, elem_bytes=8):
    """what the fill kernel has to write"""
    return nt * rows * lanes * elem_bytes


def paths_bytes(B, T, D, k0, seeded):
    """what sdraw_paths has to move per call: X out, and z in unless it is generated (doubles)"""
    return B * D * (T - k0) * 3 * 8 * (1 if seeded else 2)


def make_workload(scale=1.0, T=520):
    from epidemicmodeling_amd import synth
    return synth.make_cfg3(max(1, int(round(300 * scale))), T)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)),
            "calls": len(ms)}


def _events(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _wall(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _alternate(cases, calls, timer):
    for fn in cases.values():                                 # warm-up: every shape the timed window uses, twice
        fn()
        fn()
    ms = {k: [] for k in cases}
    for _ in range(calls):
        for k, fn in cases.items():
            ms[k].append(timer(fn))
    return {k: stats(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 300 chains")
    ap.add_argument("--host-scale", type=float, default=0.1, help="fraction of the 300 chains of case (c)")
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--days", type=int, default=520)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise", "bench.json"))
    args = ap.parse_args()
    import torch
    from epidemicmodeling_amd import _build, _lib, batch, hostapi, pipeline
    _build.build_library()
    w = make_workload(args.scale, args.days)
    B, T, D = w.B, w.T, args.draws
    dev = torch.device("cuda:0")
    res = {"timing": "per case its members alternating; (a), (d) HIP events, (b), (c) a host clock around a synchronised call",
           "source_hash": _build.source_hash(), "gpu": torch.cuda.get_device_name(0), "B": B, "T": T, "D": D, "seed": args.seed}

    # ---- (d) the fill kernel, a copy of its bytes, torch.randn ----
    nb = fill_bytes(T, 3, B * D)
    src = torch.ones(nb // 16, dtype=torch.float64, device=dev)
    dst = torch.empty_like(src)
    err, st = C.create_string_buffer(256), torch.cuda.current_stream()

    def copy():
        _lib.check(_lib.lib().epi_calib_copy_f64_device(src.data_ptr(), dst.data_ptr(), src.numel(), C.c_void_p(st.cuda_stream), err), err)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    d = _alternate({"fill": lambda: batch.normal_draws(T, 3, B * D, args.seed),
                    "copy": copy,
                    "torch_randn": lambda: torch.randn((T, 3, B * D), dtype=torch.float64, device=dev, generator=gen)}, args.calls, _events)
    d["bytes_written"] = nb
    d["copy"]["bytes_moved"] = nb                                 # half read, half written
    d["fill"]["GB_per_s_written"] = nb / d["fill"]["median_ms"] / 1e6
    d["fill_over_copy"] = d["fill"]["median_ms"] / d["copy"]["median_ms"]
    d["fill_over_torch_randn"] = d["fill"]["median_ms"] / d["torch_randn"]["median_ms"]
    res["fill"] = d
    del src, dst
    torch.cuda.empty_cache()

    # ---- (a) sdraw_paths, z read against z generated ----
    dw = batch.DeviceWorkload(w)
    r = batch.EkfRunner(dw, ["S_PLUS", "P_PLUS", "S_MINUS", "P_MINUS"], lane_block="auto")
    r.run()
    torch.cuda.synchronize()
    lb = 0 if r.blk == B else r.blk
    big = (r.out["S_PLUS"], r.out["P_PLUS"], r.out["S_MINUS"], r.out["P_MINUS"])
    z = batch.normal_draws(T, 3, B * D, args.seed)
    a = _alternate({"z_read": lambda: batch.smoother_draws(*big, dw.prm, D, z=z, lane_block=lb, B=B, outputs=("X", "status")),
                    "z_generated": lambda: batch.smoother_draws(*big, dw.prm, D, seed=args.seed, lane_block=lb, B=B, outputs=("X", "status")),
                    "gain": lambda: batch.smoother_draws(*big, dw.prm, D, lane_block=lb, B=B, outputs=("rank", "status"))}, args.calls, _events)
    for k, seeded in (("z_read", False), ("z_generated", True)):
        a[k]["paths_ms"] = a[k]["median_ms"] - a["gain"]["median_ms"]
        a[k]["paths_bytes"] = paths_bytes(B, T, D, 0, seeded)
        a[k]["paths_GB_per_s"] = a[k]["paths_bytes"] / a[k]["paths_ms"] / 1e6
    a["generated_over_read"] = a["z_generated"]["paths_ms"] / a["z_read"]["paths_ms"]
    x1 = batch.smoother_draws(*big, dw.prm, D, z=z, lane_block=lb, B=B, outputs=("X",))["X"]
    x3 = batch.smoother_draws(*big, dw.prm, D, seed=args.seed, lane_block=lb, B=B, outputs=("X",))["X"]
    a["same_bits"] = bool(torch.equal(x1.view(torch.int64), x3.view(torch.int64)))
    res["paths"] = a
    del z, x1, x3, r, big, dw
    torch.cuda.empty_cache()

    # ---- (b) the pipeline end to end, with the peak memory of each ----
    peak = {}
    fan = {"torch": lambda: pipeline.smoothed_fan(w, D, seed=args.seed), "device": lambda: pipeline.smoothed_fan(w, D, seed=args.seed, rng="device")}
    for fn in fan.values():                                   # warm-up; the caching allocator then holds the blocks of both
        fn()
        fn()
    ms = {k: [] for k in fan}
    for _ in range(args.calls):
        for k, fn in fan.items():
            ms[k].append(_wall(fn))
    for k, fn in fan.items():                                 # the peak of each, from an empty allocator
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[k] = int(torch.cuda.max_memory_allocated())
    b = {k: dict(stats(v), peak_allocated_bytes=peak[k]) for k, v in ms.items()}
    b["device_over_torch_ms"] = b["device"]["median_ms"] / b["torch"]["median_ms"]
    b["device_over_torch_peak"] = peak["device"] / peak["torch"]
    res["pipeline"] = b

    # ---- (c) the host-pointer call, z from host memory against seeded ----
    wh = make_workload(args.host_scale, args.days)
    dwh = batch.DeviceWorkload(wh)
    rh = batch.EkfRunner(dwh, ["S_PLUS", "P_PLUS", "S_MINUS", "P_MINUS"])
    rh.run()
    torch.cuda.synchronize()
    hb = [rh.out[k].cpu().numpy() for k in ("S_PLUS", "P_PLUS", "S_MINUS", "P_MINUS")]
    zh = hostapi.normal_draws(T, 3, wh.B * D, args.seed)
    c = _alternate({"z_from_host": lambda: hostapi.smoother_draws(*hb, wh.prm, D, z=zh, outputs=("X", "status")),
                    "seeded": lambda: hostapi.smoother_draws(*hb, wh.prm, D, seed=args.seed, outputs=("X", "status"))},
                   args.calls, _wall)
    c["B"], c["z_bytes"] = wh.B, int(zh.nbytes)
    c["seeded_over_z_from_host"] = c["seeded"]["median_ms"] / c["z_from_host"]["median_ms"]
    res["host"] = c

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

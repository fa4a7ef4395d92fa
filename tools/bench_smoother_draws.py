"""Measurement of the smoother draws as one device call (epi_sdraw_run_device; bench.py stays the headline's yardstick).  Writes
profiles/smoother_draws/bench.json and prints it as one JSON line.

    python tools/bench_smoother_draws.py                  # 300 chains x 1 024 draws x 520 days
    python tools/bench_smoother_draws.py --scale 0.1      # a tenth of the chains
    python tools/bench_smoother_draws.py --profile-only   # a few calls, for rocprofv3 --kernel-trace --stats

In this process and on this device: the 3-state smoother runs once (EkfRunner, chain-blocked S_PLUS, P_PLUS, S_MINUS, P_MINUS)
and the draws are timed on those arrays where they lie, HIP events around each call after warm-up (median, p10, p90):
  f64        z and X float64
  f32        z and X float32
  gain       the same call asked for rank and status only: sdraw_gain alone (sdraw_paths is not launched without X); the share of
             sdraw_paths is the call minus this
  copy       epi_calib_copy_f64_device over as many bytes as sdraw_paths' floor, timed alternating with the f64 call
Byte floors (floor_bytes below, from the shapes): sdraw_paths 3 (sizeof z + sizeof X) per path-day; sdraw_gain its inputs (24
stored elements per chain-day) and its workspace record (192 B per chain-day), once."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def floor_bytes(B, T, D, k0, z_bytes, x_bytes, elem_bytes):
    """(sdraw_paths, sdraw_gain): what each kernel has to move whatever it looks like"""
    return B * D * (T - k0) * 3 * (z_bytes + x_bytes), B * T * (24 * elem_bytes + 192)


def make_workload(scale=1.0, T=520):
    from epidemicmodeling_amd import synth
    return synth.make_cfg3(max(1, int(round(300 * scale))), T)


def _events(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms):
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)),
            "calls": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 300 chains")
    ap.add_argument("--draws", type=int, default=1024)
    ap.add_argument("--days", type=int, default=520)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smoother_draws", "bench.json"))
    args = ap.parse_args()
    import torch
    from epidemicmodeling_amd import _build, _lib, batch
    _build.build_library()
    w = make_workload(args.scale, args.days)
    B, T, D = w.B, w.T, args.draws
    dw = batch.DeviceWorkload(w)
    r = batch.EkfRunner(dw, ["S_PLUS", "P_PLUS", "S_MINUS", "P_MINUS"], lane_block="auto")
    r.run()
    torch.cuda.synchronize()
    lb = 0 if r.blk == B else r.blk
    big = (r.out["S_PLUS"], r.out["P_PLUS"], r.out["S_MINUS"], r.out["P_MINUS"])
    gen = torch.Generator(device=dw.device)
    gen.manual_seed(0)
    z64 = torch.randn((T, 3, B * D), dtype=torch.float64, device=dw.device, generator=gen)
    z32 = z64.to(torch.float32)
    call64 = lambda: batch.smoother_draws(*big, dw.prm, D, z=z64, lane_block=lb, B=B, outputs=("X", "status"))
    call32 = lambda: batch.smoother_draws(*big, dw.prm, D, z=z32, lane_block=lb, B=B, out_dtype=torch.float32, outputs=("X", "status"))
    gain = lambda: batch.smoother_draws(*big, dw.prm, D, lane_block=lb, B=B, outputs=("rank", "status"))
    if args.profile_only:
        for fn in (call64, call32, gain):
            fn()
        torch.cuda.synchronize()
        return
    pb64, gb = floor_bytes(B, T, D, 0, 8, 8, 8)
    pb32, _ = floor_bytes(B, T, D, 0, 4, 4, 8)
    n = pb64 // 16
    src = torch.ones(n, dtype=torch.float64, device=dw.device)
    dst = torch.empty_like(src)
    err = C.create_string_buffer(256)
    st = torch.cuda.current_stream()

    def copy():
        _lib.check(_lib.lib().epi_calib_copy_f64_device(src.data_ptr(), dst.data_ptr(), n, C.c_void_p(st.cuda_stream), err), err)
    for fn in (call64, copy, call32, gain):
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {"f64": [], "copy": [], "f32": [], "gain": []}
    for _ in range(args.calls):                                # alternating: every round times each once
        for key, fn in (("f64", call64), ("copy", copy), ("f32", call32), ("gain", gain)):
            ms[key].append(_events(fn))
    res = {"timing": "HIP events around each call, the four alternating", "source_hash": _build.source_hash(),
           "gpu": torch.cuda.get_device_name(0), "B": B, "T": T, "D": D, "lane_block": r.blk, "prefetch_days": 4,
           "paths_floor_bytes_f64": pb64, "paths_floor_bytes_f32": pb32, "gain_floor_bytes": gb}
    for key in ms:
        res[key] = stats(ms[key])
    res["copy"]["bytes"] = 16 * n
    res["copy"]["GB_per_s"] = 16 * n / res["copy"]["median_ms"] / 1e6
    for key, pb in (("f64", pb64), ("f32", pb32)):
        t = res[key]
        t["paths_ms"] = t["median_ms"] - res["gain"]["median_ms"]
        t["GB_per_s"] = (pb + gb) / t["median_ms"] / 1e6
        t["floor_ms"] = (pb + gb) / (16 * n / res["copy"]["median_ms"])
        t["call_over_floor"] = t["median_ms"] / t["floor_ms"]
    res["f64"]["call_over_copy"] = res["f64"]["median_ms"] / res["copy"]["median_ms"]
    res["gain"]["floor_ms"] = gb / (16 * n / res["copy"]["median_ms"])
    got = call64()
    torch.cuda.synchronize()
    res["finite_fraction"] = float(torch.isfinite(got["X"]).double().mean())
    res["status_bits"] = [int((got["status"] & 1).sum()), int(((got["status"] >> 1) & 1).sum())]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

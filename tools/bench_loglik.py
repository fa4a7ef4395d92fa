"""Measurement of the innovation log-likelihood as one device call (epi_loglik_run_device; bench.py stays the headline's
yardstick).  Writes profiles/loglik/bench.json and prints it as one JSON line.

    python tools/bench_loglik.py                    # the three sizes below
    python tools/bench_loglik.py --scale 0.1        # a tenth of the regions of each
    python tools/bench_loglik.py --profile-only     # a few calls, for rocprofv3 --kernel-trace --stats

Per size, in this process and on this device: the filter runs once (EkfRunner, chain-blocked outputs S_MINUS, P_MINUS,
innovations) and the likelihood is timed on those arrays where they lie, for r_mode 1 (the workload's R_v series) and for a
scalar R_v with beta = 0.9 (the adaptive replay; for the timing only -- the arrays are those of the series run, so the numbers
it returns are not a likelihood of that filter).  HIP events around each call after warm-up (median, p10, p90):
  headline   75 000 x 520 six-state chains (300 regions x 250 cost weights), float64
  shard      its first 9 375 chains (one of eight devices' share)
  ensemble   307 200 x 400 three-state chains (300 regions x 1024 draws), float32 storage
  copy       epi_calib_copy_f64_device over 2^29 doubles (--copy-doubles)
Reported per call: ms, the algorithmic bytes (algorithmic_bytes below: computed from the shapes), those bytes over the time, and
the time over (bytes / the copy's rate) -- the yardstick: a streaming reduction cannot beat the copy rate."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PER_CHAIN_BYTES = {"loglik": 8, "nis_mean": 8, "n_valid": 4, "status": 4}
PER_DAY = ("S", "nis", "R_used")


def algorithmic_bytes(B, T, elem_bytes, outputs):
    """What the call has to move whatever its kernels look like: per chain-day the nine elements of the upper-left 3 x 3 of
    P_MINUS, three of S_MINUS and the innovation (elem_bytes each: 8, or 4 for float storage), x and R (8 each), plus 8 per
    requested per-day output; per chain the requested per-chain outputs."""
    day = 13 * elem_bytes + 16 + 8 * sum(1 for k in outputs if k in PER_DAY)
    return B * T * day + B * sum(PER_CHAIN_BYTES.get(k, 0) for k in outputs)


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


def copy_rate(n, calls):
    """bytes per millisecond of epi_calib_copy_f64_device over n doubles (8 n read + 8 n written)"""
    import torch
    from epidemicmodeling_amd import _lib
    src = torch.ones(n, dtype=torch.float64, device="cuda:0")
    dst = torch.empty_like(src)
    err = C.create_string_buffer(256)
    st = torch.cuda.current_stream()

    def fn():
        _lib.check(_lib.lib().epi_calib_copy_f64_device(src.data_ptr(), dst.data_ptr(), n, C.c_void_p(st.cuda_stream), err), err)
    t = time_calls(fn, calls, 2)
    t["doubles"] = n
    t["bytes_per_ms"] = 16.0 * n / t["median_ms"]
    return t


def make_sizes(scale=1.0):
    """[(name, workload, storage)] of the three sizes, `scale` x the regions"""
    from epidemicmodeling_amd import synth
    nreg = max(1, int(round(300 * scale)))
    w6 = synth.make_cfg4(nreg, 250, 400, 120)
    shard = w6.select(np.arange(max(1, w6.B // 8)))
    w3 = synth.make_cfg5(nreg, 1024, 400)
    return [("headline", w6, "f64"), ("shard", shard, "f64"), ("ensemble", w3, "f32")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the regions of each size")
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--copy-doubles", type=int, default=1 << 29, help="doubles of the copy that sets the byte floor")
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loglik", "bench.json"))
    args = ap.parse_args()
    import torch
    from epidemicmodeling_amd import _build, batch, layout as L
    _build.build_library()
    res = {"timing": "HIP events around each call", "source_hash": _build.source_hash(), "gpu": torch.cuda.get_device_name(0)}
    if not args.profile_only:
        res["copy"] = copy_rate(args.copy_doubles, args.calls)

    def write():                                             # after every size: a later failure loses nothing measured
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    outputs = ("loglik", "nis_mean", "n_valid", "status")
    for name, w, storage in make_sizes(args.scale):
        dw = batch.DeviceWorkload(w)
        r = batch.EkfRunner(dw, ["S_MINUS", "P_MINUS", "innovations"], lane_block="auto", storage=storage)
        r.run()
        torch.cuda.synchronize()
        lb = 0 if r.blk == w.B else r.blk
        big = (r.out["S_MINUS"], r.out["P_MINUS"], r.out["innovations"])
        xs = dw.x_series.long() if dw.x_series is not None else torch.arange(w.B, device=dw.device)
        prm9 = dw.prm.clone()
        prm9[L.PRM_BETA_EKF] = 0.9
        modes = {"r_series": dict(prm=dw.prm, R_series=dw.R_series),
                 "r_scalar_beta0.9": dict(prm=prm9, R_scalar=dw.R_series[0].index_select(0, xs).contiguous())}
        nbytes = algorithmic_bytes(w.B, w.T, 4 if storage == "f32" else 8, outputs)
        s = {"m": w.m, "B": w.B, "T": w.T, "storage": storage, "lane_block": r.blk, "outputs": list(outputs), "bytes": nbytes}
        for key, kw in modes.items():
            call = lambda: batch.innovation_likelihood(*big, dw.x, kw["prm"], w.model, R_series=kw.get("R_series"),
                                                       R_scalar=kw.get("R_scalar"), x_series=dw.x_series, L=w.L, obs_type=w.obs_type,
                                                       lane_block=lb, B=w.B, outputs=outputs)
            if args.profile_only:
                call()
                continue
            t = time_calls(call, args.calls, 2)
            t["bytes_per_ms"] = nbytes / t["median_ms"]
            t["GB_per_s"] = nbytes / t["median_ms"] / 1e6
            t["floor_ms"] = nbytes / res["copy"]["bytes_per_ms"]
            t["call_over_floor"] = t["median_ms"] / t["floor_ms"]
            got = call()
            torch.cuda.synchronize()
            t["finite_loglik_fraction"] = float(torch.isfinite(got["loglik"]).double().mean())
            t["bad_day_chains"] = int((got["status"] & 1).sum())
            s[key] = t
        res[name] = s
        if not args.profile_only:
            write()
        del r, big, dw
        torch.cuda.empty_cache()
    if args.profile_only:
        torch.cuda.synchronize()
        return
    print(json.dumps(res))


if __name__ == "__main__":
    main()

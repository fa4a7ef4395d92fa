"""Measurement of the direct optimal-NPI planner as one device call (epi_plan_run_device; bench.py stays the headline's
yardstick).  Writes profiles/npi_plan/bench.json and prints it as one JSON line.

    python tools/bench_npi_plan.py                    # 300 regions x 250 cost weights x 120 days
    python tools/bench_npi_plan.py --scale 0.1        # a tenth of the regions
    python tools/bench_npi_plan.py --start active --out profiles/npi_plan/bench_active.json   # an epidemic under way everywhere
    python tools/bench_npi_plan.py --profile-only     # two calls, for rocprofv3 --kernel-trace --stats

The regions are those of the synthetic workload (synth.make_cfg3: the trained a, b, the simulated epidemic's state at the end of
its 400-day history, the NPICost prefix of that history), the cost weights synth.epsilon_grid(250), unit NPICost weights.  HIP
events around each call after warm-up (median, p10, p90).  Next to the time: the histograms of iterations and halvings, the
share of chains per status, and two values the tool computes itself to set the time against:
  floor      the bytes of the passes actually executed (executed_bytes below, from the returned iters and halvings) at the
             box's measured copy rate (epi_calib_copy_f64_device over --copy-doubles doubles)
  one pass   the same number of chain-days scored once by random_npi_mc (its forward pass is the planner's: sialpha_step +
             npicost_accumulate, no plan read), and the returned plans scored once by sialpha_sim (the scoring tail, plan read)."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def executed_bytes(H, n, iters, halvings):
    """HBM bytes of the passes a call executed, from its per-chain iters and halvings (arrays): per chain-day the starting pass
    writes the plan (8 n), the states (24) and the mask word (4); every adjoint pass reads the states (24) and the plan (8 n) and
    reads and writes the mask word (8); every trial pass -- iters - 1 accepted ones and `halvings` rejected ones -- reads the
    plan and the mask word (8 n + 4) and writes the trial plan and its states (8 n + 24); a chain that stops on the second side
    (an odd number of accepted steps) copies its plan over (16 n).  Per chain 52 bytes of results.  The per-region inputs are
    not counted."""
    it, hv = np.asarray(iters, dtype=np.int64), np.asarray(halvings, dtype=np.int64)
    acc = np.maximum(it - 1, 0)
    day = (8 * n + 28) + it * (8 * n + 32) + (acc + hv) * (16 * n + 28) + (acc & 1) * (16 * n)
    return int((H * day + 52).sum())


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


def make_inputs(scale=1.0, n_eps=250, horizon=120, t_hist=400, start=None):
    """the call's inputs from the synthetic workload, `scale` x the 300 regions: dict sp [48, R], u_min [12, R], eps [n_eps],
    J0_prefix, J1_prefix [R], prefix_days, H.  start = (s, i, alpha) replaces the workload's end-of-history state in every region
    (the workload's epidemics have died out by day 400, which leaves most chains nothing to plan)"""
    from epidemicmodeling_amd import layout as L, synth
    R = max(1, int(round(300 * scale)))
    w = synth.make_cfg3(R, t_hist)
    end = np.asarray(w.meta["truth_end"], dtype=np.float64)
    end = end if end.shape == (3, R) else end.T
    if start is not None:
        end = np.repeat(np.asarray(start, dtype=np.float64)[:, None], R, axis=1)
    n = w.n_npi
    sp = np.zeros((48, R))
    sp[0:3] = end[0:3]
    sp[3], sp[4], sp[5] = synth.ALPHA_MIN, synth.ALPHA_MAX, synth.MODEL_GAMMA
    sp[6], sp[7], sp[11] = w.prm[L.PRM_B], synth.MODEL_BETA, 1.0
    sp[12:12 + n] = w.prm[L.PRM_A:L.PRM_A + n]
    sp[24:24 + n] = synth.IP_MAXES[:n, None]
    sp[36:36 + n] = 1.0
    # the prefix of a history that sat at its end state: the planner only adds it to J0 / J1
    J0p = t_hist * (end[0] * end[1] * end[2])
    J1p = np.cumsum(w.u.reshape(t_hist * n, R), axis=0)[-1]
    return dict(sp=sp, u_min=np.repeat(synth.IP_MINS[:n, None], R, axis=1), eps=synth.epsilon_grid(n_eps), J0_prefix=J0p, J1_prefix=J1p,
                prefix_days=t_hist, H=horizon)


def histogram(v):
    u, c = np.unique(np.asarray(v), return_counts=True)
    return {str(int(a)): int(b) for a, b in zip(u, c)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 300 regions")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=64)
    ap.add_argument("--max-halvings", type=int, default=30)
    ap.add_argument("--tol", type=float, default=1e-9)
    ap.add_argument("--copy-doubles", type=int, default=1 << 29, help="doubles of the copy that sets the byte floor")
    ap.add_argument("--start", choices=("workload", "active"), default="workload",
                    help="the end-of-history state: the workload's own, or (0.97, 2e-3, 0.25) in every region: an epidemic under way")
    ap.add_argument("--profile-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "npi_plan", "bench.json"))
    args = ap.parse_args()
    import torch
    from epidemicmodeling_amd import _build, batch
    _build.build_library()
    inp = make_inputs(args.scale, start=(0.97, 2e-3, 0.25) if args.start == "active" else None)
    R, P, H, n = inp["sp"].shape[1], inp["eps"].shape[0], inp["H"], inp["u_min"].shape[0]
    dev = torch.device("cuda:0")
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    sp, um, eps, j0p, j1p = (up(inp[k]) for k in ("sp", "u_min", "eps", "J0_prefix", "J1_prefix"))
    call = lambda: batch.npi_plan(sp, um, eps, H, J0_prefix=j0p, J1_prefix=j1p, prefix_days=inp["prefix_days"], max_iter=args.max_iter,
                                  max_halvings=args.max_halvings, tol=args.tol, device=dev)
    if args.profile_only:
        call(); call()
        torch.cuda.synchronize()
        return
    res = {"timing": "HIP events around each call", "source_hash": _build.source_hash(), "gpu": torch.cuda.get_device_name(0),
           "start": args.start, "R": R, "P": P, "H": H, "n_npi": n, "max_iter": args.max_iter, "max_halvings": args.max_halvings, "tol": args.tol}
    res["copy"] = copy_rate(args.copy_doubles, args.calls)
    t = time_calls(call, args.calls, 1)
    got = call()
    torch.cuda.synchronize()
    it, hv, st = (got[k].cpu().numpy() for k in ("iters", "halvings", "status"))
    nbytes = executed_bytes(H, n, it, hv)
    B = R * P
    t.update(bytes=nbytes, floor_ms=nbytes / res["copy"]["bytes_per_ms"])
    t["call_over_floor"] = t["median_ms"] / t["floor_ms"]
    t["GB_per_s"] = nbytes / t["median_ms"] / 1e6
    res["plan"] = t
    res["iters_histogram"], res["halvings_histogram"] = histogram(it), histogram(hv)
    res["status_share"] = {str(k): float((st == k).mean()) for k in np.unique(st)}
    res["forward_passes"] = int((1 + np.maximum(it - 1, 0) + hv).sum())
    res["adjoint_passes"] = int(it.sum())
    # a wavefront lives as long as its slowest lane: the passes of the slowest lane of every wavefront of 64 chains, over the mean
    passes = (1 + np.maximum(it - 1, 0) + hv + it).astype(np.float64)
    pad = np.concatenate([passes, np.zeros(-B % 64)]).reshape(-1, 64)
    res["divergence"] = {"mean_passes_per_chain": float(passes.mean()), "mean_of_wavefront_maxima": float(pad.max(axis=1).mean()),
                         "slowest_wavefront": float(pad.max())}
    gap_rel = (got["gap"] / got["F"].abs()).cpu().numpy()
    res["worst_gap_over_F"] = float(np.nanmax(gap_rel))
    # one forward pass over the same chain-days: the Monte-Carlo's (no plan read) and the scoring tail's on the plans returned
    mc = time_calls(lambda: batch.random_npi_mc(sp, um, P, H, seed=1, J0_prefix=j0p, J1_prefix=j1p, prefix_days=inp["prefix_days"], device=dev),
                    args.calls, 1)
    res["random_npi_mc_one_pass"] = mc
    rr = torch.arange(R, device=dev).repeat_interleave(P)
    spB = sp.index_select(1, rr).contiguous()
    sc = time_calls(lambda: batch.sialpha_sim(got["plan"], spB, with_cost=True, store=False, device=dev), args.calls, 1)
    res["scoring_tail_one_pass"] = sc
    res["plan_over_mc_pass"] = t["median_ms"] / mc["median_ms"]
    res["plan_over_scoring_pass"] = t["median_ms"] / sc["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

"""The direct planner against the reference's sweep where the sweep is well conditioned: pipeline.prescribe with both planners on
a 60-day history and a 120-day horizon (over 60 + 120 days every reading of the sweep agrees).  Both score
their plans with the same NPICost tail, so per chain F = (1 - eps) sum s i alpha + eps sum w'u over the horizon follows from
(J0, J1) and the prefix.  Writes profiles/npi_plan/direct_vs_sweep.json: F_direct - F_sweep per chain, summarised.  A finding,
not a gate.

    python profiles/npi_plan/direct_vs_sweep.py [--regions 20] [--eps 50]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def horizon_F(out, days, n):
    """F per (region, cost weight) from NPICost's means over [historic, horizon] and the historic prefix"""
    eps = out["eps_grid"][None, :]
    s0 = out["J0"] * days - out["J0_prefix_region"][:, None]
    s1 = out["J1"] * (n * days) - out["J1_prefix_region"][:, None]
    return (1.0 - eps) * s0 + eps * s1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=20)
    ap.add_argument("--eps", type=int, default=50)
    ap.add_argument("--history", type=int, default=60)
    ap.add_argument("--horizon", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "npi_plan", "direct_vs_sweep.json"))
    a = ap.parse_args()
    from epidemicmodeling_amd import pipeline, synth
    raw = synth.make_raw_counts(a.regions, a.history, seed=1)
    n = raw["ip"].shape[1]
    run = lambda planner: pipeline.prescribe(raw["cases"], raw["deaths"], raw["population"], raw["ip"], horizon=a.horizon, n_eps=a.eps,
                                             num_regression_days=a.history, planner=planner)
    sw, di = run("sweep"), run("direct")
    assert np.array_equal(sw["sp_region"], di["sp_region"])
    days = a.history + a.horizon
    Fs, Fd = horizon_F(sw, days, n), horizon_F(di, days, n)
    d = Fd - Fs
    rel = d / np.abs(Fs)
    ok = np.isfinite(d)
    res = {"regions": a.regions, "n_eps": a.eps, "history": a.history, "horizon": a.horizon, "chains": int(d.size), "finite": int(ok.sum()),
           "end_of_history_state_range": {k: [float(sw["sp_region"][j].min()), float(sw["sp_region"][j].max())] for j, k in enumerate("sia")},
           "F_direct_minus_F_sweep": {"min": float(d[ok].min()), "median": float(np.median(d[ok])), "max": float(d[ok].max())},
           "relative_to_F_sweep": {"min": float(rel[ok].min()), "median": float(np.median(rel[ok])), "max": float(rel[ok].max())},
           "direct_lower": int((d[ok] < 0).sum()), "equal": int((d[ok] == 0).sum()), "direct_higher": int((d[ok] > 0).sum()),
           "direct_higher_beyond_1e-9_relative": int((rel[ok] > 1e-9).sum()),
           "plan_F_consistency_max_rel": float(np.nanmax(np.abs(Fd - di["plan_F"]) / np.abs(di["plan_F"]))),
           "direct_status_share": {str(k): float((di["plan_status"] == k).mean()) for k in np.unique(di["plan_status"])},
           "direct_iters_max": int(di["plan_iters"].max()), "direct_worst_gap_over_F": float(np.nanmax(di["plan_gap"] / np.abs(di["plan_F"]))),
           "i_opt_sweep": sw["i_opt"].tolist(), "i_opt_direct": di["i_opt"].tolist(),
           "per_region_max_rel": rel.max(axis=1).tolist(), "per_region_min_rel": rel.min(axis=1).tolist()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

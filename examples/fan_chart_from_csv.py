"""Tracker CSV in, a fan chart of the forecast new cases out: the credible band of ((N s) i) alpha per region and forecast day from
joint posterior draws of the smoother's paths (epidemicmodeling_amd/pipeline.py: forecast_fan), for all regions of
the file at once.

    python examples/fan_chart_from_csv.py [--rng device] [--curves] [--score-last N [--joint]] [--threshold C] OxCGRT_latest.csv populations.csv 2020-03-01 2020-12-31 fan.csv [horizon [draws]]

The front half of Tools/TrainPredictPrescribeNPI.m (preprocessing, two EKF rounds, two regressions), then its forecast filter
(:356-377: NaN observations over the horizon, the last day's NPIs held), then 256 backward-simulated paths per region and their
quantiles per day.  The output holds one row per region and forecast day: the 2.5, 25, 50, 75 and 97.5 % quantiles and the mean of
the daily new cases.  Without arguments (or with only the output path) a small synthetic tracker file is generated first (there is
no data set in this repository).

--score-last N holds the last N days of the window out, forecasts them from the days before, and prints how good the fans were
(pipeline.fan_quality): per region the mean CRPS and weighted interval score of the daily new cases, the share of
days the 50 % and the 95 % band held the truth, and the rank histogram in ten bins, with forecast starts N and N / 2 days before
the end of the window.  With --joint the same fans are also scored as paths (pipeline.fan_quality(joint=True)):
the energy score and the variogram score (p = 0.5, pairs of days up to a week apart) of every region's forecast, which tell
joint draws from draws with the same bands and no dependence between days.

--threshold C (or --outlook for the peak alone) prints the outlook over the horizon from the same joint draws (pipeline.path_outlook;
DESIGN.md 4.18): per region the median and the 95 % band of the day of the peak of the daily new cases and of its height, the median
of the cases summed over the horizon, and with a threshold the probability that the daily new cases reach C per 100 000 inhabitants
within the horizon, the median first day they do, and the median longest run of days at or above it.

--curves adds the bands made of curves (pipeline.curve_boxplot): the drawn paths of every region are ranked by
modified band depth, and the output gains the deepest path (curve_median) and the envelopes of the deepest 50 % and 90 % of the
paths (curve_lo50 .. curve_hi90).  Unlike the per-day quantiles these keep the height of a peak that the paths reach on different
days.  The number of paths outside the functional boxplot's fences is printed per region.

--rng device draws the noise inside the kernel from the seed instead of filling an array with torch.randn first:
other draws of the same law, and half the memory."""
import os
import sys
import tempfile

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epidemicmodeling_amd import dataio, pipeline  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from prescribe_from_csv import synthetic_files  # noqa: E402

Q = (0.025, 0.25, 0.5, 0.75, 0.975)


def score_table(d, N, keep, n_last, draws, joint=False, rng="torch"):
    """the forecast of the last n_last days of the window, scored against them: one row per region and start"""
    starts = sorted({n_last, max(1, n_last // 2)}, reverse=True)
    fq = pipeline.fan_quality(d["cases"][:, keep], d["deaths"][:, keep], N[keep], d["ip"][:, :, keep], n_last, starts, n_draws=draws,
                              joint=joint, vs_p=0.5, max_lag=7, rng=rng)
    sc = {k: v.cpu().numpy() for k, v in fq["scores"].items()}
    rows = []
    for j, r in enumerate(keep):
        for i, s in enumerate(starts):
            c = j * len(starts) + i                       # chain = region * len(starts) + start; row 3 is the new cases
            rows.append([d["geo_ids"][r], s, int(sc["n_scored"][3, c]), sc["crps_mean"][3, c], sc["wis_mean"][3, c], sc["ae_mean"][3, c],
                         sc["cover_frac"][0, 3, c], sc["cover_frac"][1, 3, c], " ".join(str(v) for v in sc["pit_hist"][:, 3, c])])
    table = pd.DataFrame(rows, columns=["region", "start", "days", "crps", "wis", "abs_err", "cover50", "cover95", "pit_hist"])
    if joint:                                             # per chain, in the rows' order
        table.insert(5, "energy", fq["es"].cpu().numpy())
        table.insert(6, "variogram", fq["vs"].cpu().numpy())
    return table


def outlook_table(out, d, N, keep, draws, per_100k):
    """the forecast's path functionals, summarised over the draws: one row per region (row 3 is the new cases)"""
    S = len(keep)
    thr = None
    if per_100k is not None:
        thr = np.full((1, 4, S), np.nan)
        thr[0, 3] = per_100k * N[keep] / 1e5
    o = pipeline.path_outlook(out["X"], S, draws, thr, population=N[keep], q=Q)
    g = lambda k, n: o[k][n].cpu().numpy()
    pd_q, pv_q, tot_q = g("peak_day", "quantiles")[3], g("peak_value", "quantiles")[3], g("total", "quantiles")[3]    # [n_q, S]
    cols = ["region", "peak_day_q2.5", "peak_day_q50", "peak_day_q97.5", "peak_q2.5", "peak_q50", "peak_q97.5", "cases_q50"]
    rows = [[d["geo_ids"][r], pd_q[0, j] + 1, pd_q[2, j] + 1, pd_q[4, j] + 1, pv_q[0, j], pv_q[2, j], pv_q[4, j], tot_q[2, j]]
            for j, r in enumerate(keep)]
    if thr is not None:
        p = o["p_cross_by_day"][-1, 0, 3].cpu().numpy()
        first = pipeline.batch.ensemble_summary(o["functionals"]["first_cross"], S, draws, q=(0.5,))["quantiles"][0, 0, 3].cpu().numpy()
        run = g("longest_run", "quantiles")[0, 2, 3]
        cols += ["p_reached", "first_day_q50", "longest_run_q50"]
        rows = [row + [p[j], first[j] + 1, run[j]] for j, row in enumerate(rows)]
    return pd.DataFrame(rows, columns=cols)


def main():
    horizon, draws = 30, 256
    n_last, outlook, per_100k, rng = 0, False, None, "torch"
    if "--rng" in sys.argv:
        i = sys.argv.index("--rng")
        rng = sys.argv[i + 1]
        del sys.argv[i:i + 2]
    if "--outlook" in sys.argv:
        sys.argv.remove("--outlook")
        outlook = True
    if "--threshold" in sys.argv:
        i = sys.argv.index("--threshold")
        outlook, per_100k = True, float(sys.argv[i + 1])
        del sys.argv[i:i + 2]
    curves = "--curves" in sys.argv
    if curves:
        sys.argv.remove("--curves")
    joint = "--joint" in sys.argv
    if joint:
        sys.argv.remove("--joint")
    if "--score-last" in sys.argv:
        i = sys.argv.index("--score-last")
        n_last = int(sys.argv[i + 1])
        del sys.argv[i:i + 2]
    if len(sys.argv) >= 6:
        data, pops, start, end, dst = sys.argv[1:6]
        horizon = int(sys.argv[6]) if len(sys.argv) > 6 else horizon
        draws = int(sys.argv[7]) if len(sys.argv) > 7 else draws
    else:
        tmp = tempfile.mkdtemp()
        data, pops, start, end = synthetic_files(tmp)
        dst = sys.argv[1] if len(sys.argv) == 2 else os.path.join(tmp, "fan_chart.csv")
    d = dataio.read_oxcgrt(data, start, end)
    N = dataio.read_populations(pops, d["geo_ids"])
    keep = np.flatnonzero(np.isfinite(N) & np.isfinite(d["cases"]).any(axis=0))
    out = pipeline.forecast_fan(d["cases"][:, keep], d["deaths"][:, keep], N[keep], d["ip"][:, :, keep], horizon, n_draws=draws, q=Q, rng=rng,
                                curves=True if curves else None)
    qs = out["summary"]["quantiles"].cpu().numpy()[:, :, 3]       # [horizon, n_q, S]: row 3 is the new cases
    mean = out["summary"]["mean"].cpu().numpy()[:, 3]
    status = out["summary"]["status"].cpu().numpy()
    rows = []
    for j, r in enumerate(keep):
        for t in range(horizon):
            rows.append([d["geo_ids"][r], t + 1] + [qs[t, k, j] for k in range(len(Q))] + [mean[t, j], int(status[j])])
    table = pd.DataFrame(rows, columns=["region", "day_ahead"] + [f"q{100 * v:g}" for v in Q] + ["mean", "status"])
    if curves:                                                    # [horizon, rows', S] and [horizon, n_alpha, rows', S]: row 3, alpha = (0.5, 0.9)
        cv = {k: out["summary"]["curves"][k].cpu().numpy() for k in ("median_curve", "env_lo", "env_hi", "n_outliers", "n_ranked")}
        cols = {"curve_median": cv["median_curve"][:, 3], "curve_lo50": cv["env_lo"][:, 0, 3], "curve_hi50": cv["env_hi"][:, 0, 3],
                "curve_lo90": cv["env_lo"][:, 1, 3], "curve_hi90": cv["env_hi"][:, 1, 3]}
        for name, v in cols.items():
            table[name] = v.T.reshape(-1)                         # the rows run region by region, day by day
    table.to_csv(dst, index=False)
    print(f"{len(keep)} regions x {draws} draws x {horizon} days -> {dst}")
    print(table.head(12).to_string(index=False))
    if curves:
        print("paths outside the functional boxplot's fences (of the ranked paths), per region:")
        print(" ".join(f"{d['geo_ids'][r]}: {cv['n_outliers'][3, j]}/{cv['n_ranked'][3, j]}" for j, r in enumerate(keep)))
    if outlook:
        print(f"the outlook over the {horizon} days (day 1 is the first forecast day):")
        print(outlook_table(out, d, N, keep, draws, per_100k).to_string(index=False))
    if n_last > 0:
        print(f"the last {n_last} days held out and forecast from the days before them:")
        print(score_table(d, N, keep, n_last, draws, joint, rng).to_string(index=False))


if __name__ == "__main__":
    main()

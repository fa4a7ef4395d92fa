"""Tracker CSV in, a fan chart of the forecast new cases out: the credible band of ((N s) i) alpha per region and forecast day from
joint posterior draws of the smoother's paths (epidemicmodeling_amd/pipeline.py: forecast_fan), for all regions of
the file at once.

    python examples/fan_chart_from_csv.py OxCGRT_latest.csv populations.csv 2020-03-01 2020-12-31 fan.csv [horizon [draws]]

The front half of Tools/TrainPredictPrescribeNPI.m (preprocessing, two EKF rounds, two regressions), then its forecast filter
(:356-377: NaN observations over the horizon, the last day's NPIs held), then 256 backward-simulated paths per region and their
quantiles per day.  The output holds one row per region and forecast day: the 2.5, 25, 50, 75 and 97.5 % quantiles and the mean of
the daily new cases.  Without arguments (or with only the output path) a small synthetic tracker file is generated first (there is
no data set in this repository)."""
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


def main():
    horizon, draws = 30, 256
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
    out = pipeline.forecast_fan(d["cases"][:, keep], d["deaths"][:, keep], N[keep], d["ip"][:, :, keep], horizon, n_draws=draws, q=Q)
    qs = out["summary"]["quantiles"].cpu().numpy()[:, :, 3]       # [horizon, n_q, S]: row 3 is the new cases
    mean = out["summary"]["mean"].cpu().numpy()[:, 3]
    status = out["summary"]["status"].cpu().numpy()
    rows = []
    for j, r in enumerate(keep):
        for t in range(horizon):
            rows.append([d["geo_ids"][r], t + 1] + [qs[t, k, j] for k in range(len(Q))] + [mean[t, j], int(status[j])])
    table = pd.DataFrame(rows, columns=["region", "day_ahead"] + [f"q{100 * v:g}" for v in Q] + ["mean", "status"])
    table.to_csv(dst, index=False)
    print(f"{len(keep)} regions x {draws} draws x {horizon} days -> {dst}")
    print(table.head(12).to_string(index=False))


if __name__ == "__main__":
    main()

"""Tracker CSV in, look-ahead forecast error curves out -- the forecast-quality study of Tools/ForecastQualityAssessment.m
for all regions of the file at once (epidemicmodeling_amd/pipeline.py: forecast_quality).

    python examples/forecast_quality_from_csv.py OxCGRT_latest.csv populations.csv 2020-03-04 2021-03-04 91 60 errors.csv

The first LL - num_forecast_days days (91 above) train the filter; every region is then filtered once per start
1 .. num_forecast_days with that many last days hidden, and the error of N * s * i * alpha against the smoothed new cases
is reduced to mean / median / std per look-ahead day (1 .. 60 above).  Without arguments (or with only the output path) a
small synthetic tracker file is generated first (there is no data set in this repository)."""
import os
import sys
import tempfile

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epidemicmodeling_amd import dataio, pipeline  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from prescribe_from_csv import synthetic_files  # noqa: E402

STATS = ("mean_plus", "median_plus", "std_plus", "mean_smooth", "median_smooth", "std_smooth")


def main():
    if len(sys.argv) >= 8:
        data, pops, start, end = sys.argv[1:5]
        F, M, dst = int(sys.argv[5]), int(sys.argv[6]), sys.argv[7]
    else:
        tmp = tempfile.mkdtemp()
        data, pops, start, end = synthetic_files(tmp)
        F, M = 30, 20
        dst = sys.argv[1] if len(sys.argv) == 2 else os.path.join(tmp, "lookahead_errors.csv")
    d = dataio.read_oxcgrt(data, start, end)
    N = dataio.read_populations(pops, d["geo_ids"])
    keep = np.flatnonzero(np.isfinite(N) & np.isfinite(d["cases"]).any(axis=0))
    out = pipeline.forecast_quality(d["cases"][:, keep], d["deaths"][:, keep], N[keep], d["ip"][:, :, keep], F, max_lookahead=M)
    rows = []
    for i, k in enumerate(keep):
        for j in range(M):
            rows.append([d["geo_ids"][k], j + 1] + [out[s][j, i] for s in STATS])
    pd.DataFrame(rows, columns=["region", "lookahead_day", *STATS]).to_csv(dst, index=False)
    print(f"{len(keep)} regions x {d['cases'].shape[0]} days, {F} starts, {M} look-ahead days -> {dst}")
    print(f"median over regions of the median EKS error (%) at look-ahead day 1 / {M}:",
          np.nanmedian(out["median_smooth"][0]), np.nanmedian(out["median_smooth"][M - 1]))


if __name__ == "__main__":
    main()

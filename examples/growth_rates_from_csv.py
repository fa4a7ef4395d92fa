"""Tracker CSV in, per-region growth-rate series out -- the growth-rate features of
testScripts/test04FullFeatureExtMLpipeline.m for all regions of the file at once (epidemicmodeling_amd/pipeline.py:
growth_rates).

    python examples/growth_rates_from_csv.py OxCGRT_latest.csv populations.csv 2020-03-04 2021-03-04 growth.csv

Per region and day the output holds the smoothed new cases and the growth rate lambda of the three sliding-window
estimators (log-linear regression, generation ratios, nonlinear least squares) and of the exponential-fit EKS (order 1).
Without arguments (or with only the output path) a small synthetic tracker file is generated first (there is no data set
in this repository)."""
import os
import sys
import tempfile

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epidemicmodeling_amd import dataio, pipeline  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from prescribe_from_csv import synthetic_files  # noqa: E402

COLS = ("new_smoothed", "llr_Lambda", "gr_Lambda", "gr_LambdaSmoothed", "nls_Lambda", "nls_status")


def main():
    if len(sys.argv) >= 6:
        data, pops, start, end, dst = sys.argv[1:6]
    else:
        tmp = tempfile.mkdtemp()
        data, pops, start, end = synthetic_files(tmp)
        dst = sys.argv[1] if len(sys.argv) == 2 else os.path.join(tmp, "growth_rates.csv")
    d = dataio.read_oxcgrt(data, start, end)
    N = dataio.read_populations(pops, d["geo_ids"])
    keep = np.flatnonzero(np.isfinite(N) & np.isfinite(d["cases"]).any(axis=0))
    out = pipeline.growth_rates(d["cases"][:, keep], N[keep], wlen=7, generation_period=3, causal=1)
    T = d["cases"].shape[0]
    rows = []
    for i, k in enumerate(keep):
        for t in range(T):
            rows.append([d["geo_ids"][k], t + 1] + [out[c][t, i] for c in COLS] + [out["ekf1_S_SMOOTH"][t, 1, i]])
    pd.DataFrame(rows, columns=["region", "day", *COLS, "ekf_lambda"]).to_csv(dst, index=False)
    print(f"{len(keep)} regions x {T} days -> {dst}")
    print("median over regions of the last day's lambda (LogLinReg / GenRatios / NonlinLS / EKS):",
          *(np.nanmedian(out[c][-1]) for c in ("llr_Lambda", "gr_Lambda", "nls_Lambda")), np.nanmedian(out["ekf1_S_SMOOTH"][-1, 1]))


if __name__ == "__main__":
    main()

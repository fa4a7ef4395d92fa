"""Tracker CSV in, per-region growth-rate forecast out -- the phase-I predictor of
testScripts/test04FullFeatureExtMLpipeline.m for all regions of the file and several train / test splits at once
(epidemicmodeling_amd/pipeline.py: growth_forecast).

    python examples/growth_forecast_from_csv.py OxCGRT_latest.csv populations.csv 2020-03-04 2021-03-04 forecast.csv

The growth rate (log-linear regression over a sliding window) is regressed on the intervention plans and their copies lagged
by 3, 5 and 7 days over the training days, predicted over the days ahead (14, 28 and 42 here), clipped to +-0.1 and turned
back into new cases.  Per region, split and test day the output holds the smoothed new cases, the predicted rate and the
rebuilt new cases.  Without arguments (or with only the output path) a small synthetic tracker file is generated first
(there is no data set in this repository).

    python examples/growth_forecast_from_csv.py --solver svr ...      # ridge (default), backslash, svr, svr_gaussian or mean

`--solver svr` / `svr_gaussian` take the fitrsvm rows of the reference's scripts (support-vector regression with the linear /
the Gaussian kernel on the normalised columns, fitrsvm's default hyper-parameters); `--solver mean` is the scripts' average
of the ridge map and the two support-vector rows."""
import os
import sys
import tempfile

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epidemicmodeling_amd import dataio, pipeline  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from prescribe_from_csv import synthetic_files  # noqa: E402

AHEAD = (14, 28, 42)


def main():
    argv, solver = list(sys.argv[1:]), "ridge"
    if "--solver" in argv:
        i = argv.index("--solver")
        solver = argv[i + 1]
        del argv[i:i + 2]
    if solver not in pipeline.GROWTH_SOLVERS + ("mean",):
        raise SystemExit(f"--solver must be one of {pipeline.GROWTH_SOLVERS + ('mean',)}")
    if len(argv) >= 5:
        data, pops, start, end, dst = argv[:5]
    else:
        tmp = tempfile.mkdtemp()
        data, pops, start, end = synthetic_files(tmp)
        dst = argv[0] if len(argv) == 1 else os.path.join(tmp, "growth_forecast.csv")
    d = dataio.read_oxcgrt(data, start, end)
    N = dataio.read_populations(pops, d["geo_ids"])
    keep = np.flatnonzero(np.isfinite(N) & np.isfinite(d["cases"]).any(axis=0))
    T = d["cases"].shape[0]
    ahead = [a for a in AHEAD if a < T - 8]
    run = lambda sv: pipeline.growth_forecast(d["cases"][:, keep], N[keep], d["ip"][:, :, keep], predict_ahead=ahead, solver=sv,
                                              normalise=sv != "ridge")
    out = pipeline.growth_forecast_mean([run(sv) for sv in ("ridge", "svr", "svr_gaussian")]) if solver == "mean" else run(solver)
    rows = []
    for i, k in enumerate(keep):
        for j, nt in enumerate(out["n_train"]):
            for t in range(int(nt), T):
                rows.append([d["geo_ids"][k], T - int(nt), t + 1, out["new_smoothed"][t, i], out["lambda_hat"][j, t, i],
                             out["new_cases_est"][j, t, i], int(out["status"][j, i])])
    pd.DataFrame(rows, columns=["region", "days_ahead", "day", "new_smoothed", "lambda_hat", "new_cases_est", "status"]).to_csv(dst, index=False)
    print(f"{len(keep)} regions x {len(ahead)} splits x {T} days -> {dst}")
    with np.errstate(all="ignore"):
        print("median over regions of the mean absolute error of the rebuilt new cases, by days ahead:",
              {int(a): float(np.nanmedian(m)) for a, m in zip(ahead, out["mae"])})


if __name__ == "__main__":
    main()

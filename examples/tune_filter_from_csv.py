"""Tracker CSV in, the filter's noise settings per region out -- chosen by the innovation likelihood of the first EKF round of
Tools/TrainPredictPrescribeNPI.m (SIAlphaModelEKF, zero input), where the reference hand-picks Q_w, R_v, gamma and beta
(:12-22, :229-240), for all regions of the file at once (epidemicmodeling_amd/pipeline.py: tune_filter).

    python examples/tune_filter_from_csv.py OxCGRT_latest.csv populations.csv 2020-03-01 2020-12-31 tuned.csv

Every region runs under each candidate (Q_w and R_v scaled, fading memory gamma) as one batch of regions x candidates chains;
the output holds, per region, the candidate with the largest log-likelihood after a burn-in of 21 days.  The likelihood is the
EKF's own linearised one: a score for comparing candidates of one region, not a calibrated probability.  Without arguments (or
with only the output path) a small synthetic tracker file is generated first (there is no data set in this repository).

    python examples/tune_filter_from_csv.py --diagnose [the same arguments]

also asks whether the chosen candidate's filter run is statistically consistent (pipeline.filter_diagnostics on the chosen
chains): per region the days that count n, the mean normalised innovation squared nis_mean (1 for a consistent filter), the
p-values of the Ljung-Box test for serial correlation lb_p and of the Jarque-Bera test for normality jb_p, the variance ratio
het of the last third of the window over the first, and cusumsq_step, the day where the innovation variance breaks most."""
import os
import sys
import tempfile

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from epidemicmodeling_amd import batch, dataio, pipeline, synth  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from prescribe_from_csv import synthetic_files  # noqa: E402

Q_SCALE, R_SCALE, GAMMA_EKF = (0.1, 1.0, 10.0), (0.25, 1.0, 4.0), (1.0, 0.98)


def main():
    argv = [a for a in sys.argv[1:] if a != "--diagnose"]
    diagnose = len(argv) != len(sys.argv) - 1
    if len(argv) >= 5:
        data, pops, start, end, dst = argv[:5]
    else:
        tmp = tempfile.mkdtemp()
        data, pops, start, end = synthetic_files(tmp)
        dst = argv[0] if len(argv) == 1 else os.path.join(tmp, "tuned_filter.csv")
    d = dataio.read_oxcgrt(data, start, end)
    N = dataio.read_populations(pops, d["geo_ids"])
    keep = np.flatnonzero(np.isfinite(N) & np.isfinite(d["cases"]).any(axis=0))
    N = N[keep]
    pre = {k: v.cpu().numpy() for k, v in batch.preprocess(d["cases"][:, keep], N, d["deaths"][:, keep], d["ip"][:, :, keep], W=7,
                                                            min_cases=synth.MIN_CASES, first_num_days=7).items()}
    x, R, u, I0 = pre["x_new"], pre["R_v"], pre["ip_filled"], pre["I0"]
    S, n = x.shape[1], u.shape[1]
    w = pipeline.workload3(x, R, np.zeros_like(u), N, I0, np.zeros((n, S)), np.zeros(S))      # EKF round 1 (:203-248)
    out = pipeline.tune_filter(w, q_scale=Q_SCALE, r_scale=R_SCALE, gamma_ekf=GAMMA_EKF, burn_in=21)
    best, ll, chosen = (out[k].cpu().numpy() for k in ("best", "best_loglik", "chosen"))
    table = pd.DataFrame({"region": [d["geo_ids"][k] for k in keep], "candidate": best, "loglik": ll, "q_scale": chosen[:, 0],
                          "r_scale": chosen[:, 1], "gamma_ekf": chosen[:, 2]})
    if diagnose:
        G = out["table"].shape[0]
        picked = out["workload"].select(np.arange(S) * G + np.maximum(best, 0))      # the chosen candidate of every region
        _, dg = pipeline.filter_diagnostics(picked, n_lags=10, burn_in=21,
                                            outputs=("n", "nis_mean", "lb_q", "lb_lags", "jb", "het", "cusumsq_step"))
        for k in ("n", "nis_mean", "lb_p", "jb_p", "het", "cusumsq_step"):
            table[k] = np.where(best >= 0, dg[k].cpu().numpy(), np.nan)
    table.to_csv(dst, index=False)
    print(f"{S} regions x {out['table'].shape[0]} candidates x {x.shape[0]} days -> {dst}")
    print(table.to_string(index=False))


if __name__ == "__main__":
    main()

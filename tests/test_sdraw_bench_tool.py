"""tools/bench_smoother_draws.py on the CPU: its byte floors against a hand count, the workload it builds, and that the record it
committed (profiles/smoother_draws/bench.json) parses and holds the numbers the documents quote."""
import importlib.util
import json
import os

from tests import helpers as H


def _tool():
    spec = importlib.util.spec_from_file_location("bench_smoother_draws", os.path.join(H.ROOT, "tools", "bench_smoother_draws.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_floor_bytes_against_a_hand_count():
    f = _tool().floor_bytes
    # 2 chains x 3 draws x 5 days, doubles: 30 path-days x 3 x 16 B = 1440 B; the gain: 10 chain-days x (24 x 8 + 192) B = 3840 B
    assert f(2, 5, 3, 0, 8, 8, 8) == (1440, 3840)
    # k0 = 2: 18 path-days; float z and X: 3 x 8 B; float storage: 24 x 4 + 192
    assert f(2, 5, 3, 2, 4, 4, 4) == (18 * 24, 10 * 288)
    assert f(300, 520, 1024, 0, 8, 8, 8)[0] == 7667712000       # the 7.7 GB of the full size


def test_the_workload():
    w = _tool().make_workload(scale=2.0 / 300.0, T=40)
    assert (w.model, w.m, w.B, w.T) == ("SIAlphaModelEKF", 3, 2, 40)


def test_the_committed_record_parses():
    rec = json.load(open(os.path.join(H.ROOT, "profiles", "smoother_draws", "bench.json")))
    assert (rec["B"], rec["T"], rec["D"]) == (300, 520, 1024) and rec["paths_floor_bytes_f64"] == 7667712000
    for key in ("f64", "f32", "copy", "gain"):
        t = rec[key]
        assert t["calls"] >= 5 and 0.0 < t["p10_ms"] <= t["median_ms"] <= t["p90_ms"]
    assert abs(rec["f64"]["call_over_copy"] - rec["f64"]["median_ms"] / rec["copy"]["median_ms"]) < 1e-12
    assert rec["finite_fraction"] == 1.0

"""tools/bench_ens_score.py on the CPU: its byte count and ratios against a hand count, and that the record it committed
(profiles/ens_score/bench.json) parses and holds the numbers the documents quote."""
import importlib.util
import json
import os

from tests import helpers as H


def _tool():
    spec = importlib.util.spec_from_file_location("bench_ens_score", os.path.join(H.ROOT, "tools", "bench_ens_score.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bytes_and_ratios_against_a_hand_count():
    t = _tool()
    assert t.source_bytes(2, 5, 3, 8) == 2 * 5 * 3 * 3 * 8
    assert t.source_bytes(300, 1024, 400, 4) == 1474560000 and t.source_bytes(300, 1024, 400, 8) == 2949120000
    s = t.stats([1.0, 2.0, 3.0, 4.0, 5.0])
    assert s["median_ms"] == 3.0 and s["calls"] == 5 and s["p10_ms"] < 3.0 < s["p90_ms"]
    r = t.ratios({"score": {"median_ms": 6.0}, "summary": {"median_ms": 4.0, "p10_ms": 3.9, "p90_ms": 4.3}, "copy": {"median_ms": 2.0}})
    assert r["score_over_summary"] == 1.5 and r["score_over_copy"] == 3.0 and abs(r["summary_spread"] - 0.1) < 1e-12
    assert t.ALPHA == (0.5, 0.05) and t.N_BINS == 10 and len(t.Q) == 5


def test_the_committed_record_parses():
    rec = json.load(open(os.path.join(H.ROOT, "profiles", "ens_score", "bench.json")))
    assert rec["shape"] == {"R": 300, "D": 1024, "T": 400, "rows": 3, "derived_row": 1, "alpha": [0.5, 0.05], "n_bins": 10,
                            "q": [0.025, 0.25, 0.5, 0.75, 0.975]}
    for name, elem in (("f32", 4), ("f64", 8)):
        r = rec[name]
        assert r["source_bytes"] == 300 * 1024 * 400 * 3 * elem
        for key in ("score", "summary", "copy"):
            t = r[key]
            assert t["calls"] >= 5 and 0.0 < t["p10_ms"] <= t["median_ms"] <= t["p90_ms"]
        assert abs(r["score_over_summary"] - r["score"]["median_ms"] / r["summary"]["median_ms"]) < 1e-12
        assert abs(r["score_over_copy"] - r["score"]["median_ms"] / r["copy"]["median_ms"]) < 1e-12
        assert r["reference_check"]["items"] == 24 and r["reference_check"]["mismatches"] == []
        assert r["scored_items"] == 400 * 4 * 300

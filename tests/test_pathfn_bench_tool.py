"""tools/bench_path_functionals.py on the CPU: its byte and wavefront counts and ratios against a hand count, and that the records
it committed (profiles/path_functionals/bench.json, segments.json) parse and hold the numbers the documents quote."""
import importlib.util
import json
import os

from tests import helpers as H


def _tool():
    spec = importlib.util.spec_from_file_location("bench_path_functionals", os.path.join(H.ROOT, "tools", "bench_path_functionals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bytes_waves_and_ratios_against_a_hand_count():
    t = _tool()
    assert t.source_bytes(2, 5, 3, 8) == 2 * 5 * 3 * 3 * 8
    assert t.source_bytes(300, 1024, 520, 8) == 3833856000 and t.source_bytes(300, 1024, 520, 4) == 1916928000
    assert t.waves(300, 1024) == 4800 and t.waves(300, 64) == 300 and t.waves(256, 1024) == 4096 and t.waves(3, 70, rows=5) == 4 * 3
    assert t.waves(3, 70, rows=2, derive=0) == 8
    s = t.stats([1.0, 2.0, 3.0, 4.0, 5.0])
    assert s["median_ms"] == 3.0 and s["calls"] == 5 and s["p10_ms"] < 3.0 < s["p90_ms"]
    r = t.ratios({"pathfn": {"median_ms": 2.0}, "copy": {"median_ms": 1.0}, "torch": {"median_ms": 50.0}, "source_bytes": 4000000000})
    assert r["pathfn_over_copy"] == 2.0 and r["torch_over_pathfn"] == 25.0 and r["pathfn_gb_per_s"] == 2000.0
    assert t.best_segments({1: {"median_ms": 3.0}, 2: {"median_ms": 2.5}, 8: {"median_ms": 2.6}}) == 2
    assert t.N_THR == (0, 2, 8) and t.SEGMENTS == (1, 2, 4, 8)


def test_the_committed_records_parse():
    rec = json.load(open(os.path.join(H.ROOT, "profiles", "path_functionals", "bench.json")))
    assert rec["shape"] == {"R": 300, "D": 1024, "T": 520, "rows": 3, "derived_row": 1, "n_thr": [0, 2, 8]}
    assert rec["waves"] == 4800 and rec["even_waves"]["waves"] == 4096
    for name, elem in (("f32", 4), ("f64", 8)):
        for nt in (0, 2, 8):
            r = rec[name][f"n_thr_{nt}"]
            assert r["source_bytes"] == 300 * 1024 * 520 * 3 * elem
            for key in ("pathfn", "copy", "torch"):
                t = r[key]
                assert t["calls"] >= 3 and 0.0 < t["p10_ms"] <= t["median_ms"] <= t["p90_ms"]
            assert abs(r["pathfn_over_copy"] - r["pathfn"]["median_ms"] / r["copy"]["median_ms"]) < 1e-12
            assert abs(r["torch_over_pathfn"] - r["torch"]["median_ms"] / r["pathfn"]["median_ms"]) < 1e-12
            assert r["torch"]["passes"] == 10 + int(elem == 4) + 8 * nt and r["torch"]["peak_extra_bytes"] > r["source_bytes"]
            assert r["reference_check"]["paths"] >= 10 and r["reference_check"]["mismatches"] == []
    seg = json.load(open(os.path.join(H.ROOT, "profiles", "path_functionals", "segments.json")))
    assert [s["D"] for s in seg["shapes"]] == [64, 256, 1024] and [s["waves"] for s in seg["shapes"]] == [300, 1200, 4800]
    for s in seg["shapes"]:
        assert sorted(s["by_segments"]) == ["1", "2", "4", "8"]
        assert s["best"] == int(min(s["by_segments"], key=lambda k: s["by_segments"][k]["median_ms"]))
    # the library's rule (epiekf.hip: kPfSegWaves, kPfSegMost): cut below 1 024 wavefronts, not at 4 800
    assert seg["shapes"][0]["best"] == 8 and seg["shapes"][2]["best"] == 1

"""tools/bench_ens_joint.py on the CPU: its operation and byte counts against a hand count, and that the record it committed
(profiles/ens_joint/bench.json) parses and holds the numbers the documents quote."""
import importlib.util
import json
import os

from tests import helpers as H


def _tool():
    spec = importlib.util.spec_from_file_location("bench_ens_joint", os.path.join(H.ROOT, "tools", "bench_ens_joint.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_counts_against_a_hand_count():
    t = _tool()
    assert t.tiles(1) == 1 and t.tiles(64) == 1 and t.tiles(65) == 3 and t.tiles(130) == 6 and t.tiles(1024) == 136 and t.tiles(4096) == 2080
    assert t.pair_flops(1, 2, 1, rows_out=1) == 3 and t.pair_flops(300, 1024, 120) == 3 * 1200 * 523776 * 120 == 226271232000
    assert t.tile_flops(1, 65, 2, rows_out=1) == 3 * 3 * 4096 * 2 and t.tile_flops(300, 1024, 120) == 240648192000
    assert t.reread_bytes(300, 1024, 120, 8) == 300 * 136 * 120 * 2 * 64 * 8 * 6 == 30081024000
    s = t.stats([1.0, 2.0, 3.0, 4.0, 5.0])
    assert s["median_ms"] == 3.0 and s["calls"] == 5 and s["p10_ms"] < 3.0 < s["p90_ms"]
    r = t.rates({"es": {"median_ms": 10.0}, "torch_es": {"median_ms": 25.0}, "torch_exact": {"median_ms": 40.0}, "escore": {"median_ms": 2.5}},
                300, 1024, 120, 8)
    assert r["torch_over_es"] == 2.5 and r["es_over_torch"] == 0.4 and r["torch_exact_over_es"] == 4.0 and r["es_over_escore"] == 4.0
    assert abs(r["tile_flops_per_s"] - 240648192000 / 0.01) < 1.0 and abs(r["tile_share_of_unfused_peak"] - 2 * r["tile_share_of_peak"]) < 1e-15
    assert t.PEAK_FP64_VECTOR == 78.6e12


def test_the_committed_record_parses():
    rec = json.load(open(os.path.join(H.ROOT, "profiles", "ens_joint", "bench.json")))
    assert rec["shape"] == {"R": 300, "D": 1024, "T": 120, "rows": 3, "derived_row": 1, "tiles": 136, "vs_p": 0.5}
    for name, elem in (("f32", 4), ("f64", 8)):
        r = rec[name]
        assert r["source_bytes"] == 300 * 1024 * 120 * 3 * elem
        for key in ("es", "vs_all", "vs_lag7", "torch_es", "torch_exact", "escore"):
            t = r[key]
            assert t["calls"] >= 5 and 0.0 < t["p10_ms"] <= t["median_ms"] <= t["p90_ms"]
        assert abs(r["torch_over_es"] - r["torch_es"]["median_ms"] / r["es"]["median_ms"]) < 1e-12
        assert r["torch_over_es"] > 1.0                      # the condition of the call: faster than the torch formulation
        assert r["pair_flops"] == 226271232000 and r["tile_flops"] == 240648192000
        assert abs(r["tile_flops_per_s"] - r["tile_flops"] / (r["es"]["median_ms"] * 1e-3)) < 1e-3 * r["tile_flops_per_s"]
        assert r["reference_check"]["items"] == 4 and r["reference_check"]["mismatches"] == []
        assert r["torch_es"]["agreement"]["max_rel_diff"] < 1e-6

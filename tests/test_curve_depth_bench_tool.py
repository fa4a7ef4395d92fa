"""tools/bench_curve_depth.py on the CPU: its byte and wavefront counts and ratios against a hand count, its torch formulation
against the restatement on a small tie-free ensemble, and that the record it committed (profiles/curve_depth/bench.json) parses
and holds the requirement the documents quote."""
import importlib.util
import json
import os

import numpy as np

from tests import helpers as H
from tests import curve_depth_ref as S


def _tool():
    spec = importlib.util.spec_from_file_location("bench_curve_depth", os.path.join(H.ROOT, "tools", "bench_curve_depth.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_bytes_waves_and_ratios_against_a_hand_count():
    t = _tool()
    assert t.source_bytes(2, 5, 3, 8) == 2 * 5 * 3 * 3 * 8
    assert t.source_bytes(300, 1024, 120, 8) == 884736000 and t.source_bytes(300, 1024, 520, 4) == 1916928000
    assert t.waves(300, 120) == 4 * 300 * 4 and t.waves(300, 520) == 4 * 300 * 17 and t.waves(3, 32, rows=2, derive=0) == 6
    s = t.stats([1.0, 2.0, 3.0, 4.0, 5.0])
    assert s == {"median_ms": 3.0, "min_ms": 1.0, "max_ms": 5.0, "calls": 5}
    r = t.ratios({"cdepth": {"median_ms": 2.0, "max_ms": 2.5}, "copy": {"median_ms": 1.0}, "torch": {"median_ms": 50.0, "min_ms": 40.0}})
    assert r == {"torch_over_cdepth": 25.0, "cdepth_over_copy": 2.0, "gate": True}
    assert not t.ratios({"cdepth": {"median_ms": 2.0, "max_ms": 41.0}, "copy": {"median_ms": 1.0}, "torch": {"median_ms": 50.0, "min_ms": 40.0}})["gate"]
    assert (t.ALPHA, t.FENCE_FACTOR, t.FENCE_FRAC, t.DAYS) == ((0.5, 0.9), 1.5, 0.5, (120, 520))
    assert [t.deepest(f, n) for f, n in ((0.5, 1024), (0.9, 1024), (0.5, 3), (1e-9, 7), (1.0, 7))] == [512, 922, 2, 1, 7]
    assert all(t.deepest(f, n) == S.deepest(f, n) for f in (0.1, 0.5, 0.9, 1.0) for n in (1, 2, 33, 1000))


def test_the_torch_formulation_is_the_same_quantity():
    import torch
    t = _tool()
    R, D, T = 2, 33, 10
    src = t.make_source(R, D, T, torch.float64, "cpu")
    pop = torch.tensor([1e5, 3e6], dtype=torch.float64)
    got = t.torch_formulation(src, pop, R, D)
    want = S.statistics(src.numpy(), R, D, alpha=t.ALPHA, fence_factor=t.FENCE_FACTOR, fence_frac=t.FENCE_FRAC, population=pop.numpy())
    for k in ("depth", "mhi", "band_count", "depth_rank", "out_days"):
        assert np.array_equal(got[k].reshape(4, -1).numpy().astype(np.float64), want[k].astype(np.float64)), k
    for k in ("median_path", "n_outliers", "env_lo", "env_hi", "median_curve", "whisk_lo", "whisk_hi"):
        assert np.array_equal(got[k].numpy(), want[k], equal_nan=True), k


def test_the_committed_record_parses():
    rec = json.load(open(os.path.join(H.ROOT, "profiles", "curve_depth", "bench.json")))
    assert rec["shape"] == {"R": 300, "D": 1024, "days": [120, 520], "rows": 3, "derived_row": 1, "alpha": [0.5, 0.9], "fence_factor": 1.5,
                            "fence_frac": 0.5}
    for T in (120, 520):
        for name, elem in (("f64", 8), ("f32", 4)):
            r = rec[f"days_{T}"][name]
            assert r["source_bytes"] == 300 * 1024 * T * 3 * elem and r["waves"] == 1200 * ((T + 31) // 32)
            for key in ("cdepth", "torch", "copy"):
                t = r[key]
                assert t["calls"] >= 5 and 0.0 < t["min_ms"] <= t["median_ms"] <= t["max_ms"]
            assert abs(r["torch_over_cdepth"] - r["torch"]["median_ms"] / r["cdepth"]["median_ms"]) < 1e-12
            assert abs(r["cdepth_over_copy"] - r["cdepth"]["median_ms"] / r["copy"]["median_ms"]) < 1e-12
            assert r["torch_peak_extra_bytes"] > r["source_bytes"]
            # the requirement: the call's slowest run is faster than the torch formulation's fastest
            assert r["gate"] and r["cdepth"]["max_ms"] < r["torch"]["min_ms"]
            if name == "f64":
                assert r["band_count_mismatches"] == 0 and r["depth_rank_mismatches"] == 0
    assert rec["gate"] is True

"""tools/bench_noise.py on the CPU: its byte counts against a hand count, the workload it builds, and that the records it committed
(profiles/noise/bench.json, profiles/noise/headline_ab.json) parse and hold the numbers DESIGN.md §4.21 quotes."""
import importlib.util
import json
import os

from tests import helpers as H


def _tool():
    spec = importlib.util.spec_from_file_location("bench_noise", os.path.join(H.ROOT, "tools", "bench_noise.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_byte_counts_against_a_hand_count():
    t = _tool()
    assert t.fill_bytes(5, 3, 6) == 5 * 3 * 6 * 8 and t.fill_bytes(5, 1, 6, 4) == 120
    # 2 chains x 3 draws x 5 days: 30 path-days x 3 doubles out, and as many in when z is read
    assert t.paths_bytes(2, 5, 3, 0, True) == 720 and t.paths_bytes(2, 5, 3, 0, False) == 1440
    assert t.paths_bytes(300, 520, 1024, 0, False) == 7667712000 and t.fill_bytes(520, 3, 300 * 1024) == 3833856000
    w = t.make_workload(scale=2.0 / 300.0, T=40)
    assert (w.model, w.B, w.T) == ("SIAlphaModelEKF", 2, 40)


def test_the_committed_records_parse_and_hold_what_the_design_quotes():
    rec = json.load(open(os.path.join(H.ROOT, "profiles", "noise", "bench.json")))
    assert (rec["B"], rec["T"], rec["D"]) == (300, 520, 1024)
    for case, keys in (("fill", ("fill", "copy", "torch_randn")), ("paths", ("z_read", "z_generated", "gain")), ("pipeline", ("torch", "device")),
                       ("host", ("z_from_host", "seeded"))):
        for k in keys:
            t = rec[case][k]
            assert t["calls"] >= 5 and 0.0 < t["p10_ms"] <= t["median_ms"] <= t["p90_ms"], (case, k)
    assert rec["paths"]["same_bits"] is True
    design = open(os.path.join(H.ROOT, "DESIGN.md")).read()
    p, f, b, h = rec["paths"], rec["fill"], rec["pipeline"], rec["host"]
    for text in ("`ZM = 1`: %.2f ms" % p["z_read"]["paths_ms"], "`ZM = 3`: **%.2f ms**" % p["z_generated"]["paths_ms"],
                 "%.2f x" % p["generated_over_read"], "`rng=\"torch\"`: %.2f ms, peak %.2f GB" % (b["torch"]["median_ms"], b["torch"]["peak_allocated_bytes"] / 1e9),
                 "`rng=\"device\"`: %.2f ms (%.2f x), peak **%.2f GB** (%.2f x)" % (b["device"]["median_ms"], b["device_over_torch_ms"],
                                                                              b["device"]["peak_allocated_bytes"] / 1e9, b["device_over_torch_peak"]),
                 "z from host memory: %.1f ms" % h["z_from_host"]["median_ms"], "seeded: %.1f ms (%.2f x)" % (h["seeded"]["median_ms"], h["seeded_over_z_from_host"]),
                 "%.2f ms (%.0f GB/s)" % (f["fill"]["median_ms"], f["fill"]["GB_per_s_written"]),
                 "a device copy of its bytes %.2f ms (%.1f x)" % (f["copy"]["median_ms"], f["fill_over_copy"]),
                 "`torch.randn` %.2f ms (%.1f x)" % (f["torch_randn"]["median_ms"], f["fill_over_torch_randn"])):
        assert text in design, text
    ab = json.load(open(os.path.join(H.ROOT, "profiles", "noise", "headline_ab.json")))
    assert len(ab["visits"]) == 3 and all(v["branch_runs"] == 4 and len(v["ms_per_step"]) == 8 for v in ab["visits"])
    assert "branch / parent = %.3f" % ab["branch_over_parent_of_medians"] in design

"""tools/bench_two_filter.py: its workload construction on the CPU (both shapes get a valid reverse-time twin that the oracle
can run), and, on the GPU, one run of the tool at one region per shape that must write both shapes' results."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import helpers as H


def _tool():
    spec = importlib.util.spec_from_file_location("bench_two_filter", os.path.join(H.ROOT, "tools", "bench_two_filter.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_both_shapes_have_a_valid_reverse_time_twin():
    shapes = _tool().make_shapes(scale=1.0 / 300.0)
    assert [(n, w.m, w.B, w.T) for n, w, _ in shapes] == [("m6_sweep", 6, 250, 520), ("m3_ensemble", 3, 1024, 400)]
    for name, w, wb in shapes:
        assert wb.model == {"m6_sweep": "SIAlphaModelBackwardEKFOptControlled", "m3_ensemble": "SIAlphaModelBackwardEKF"}[name]
        assert wb.B == w.B and wb.T == w.T and np.isfinite(wb.s_final).all() and np.isfinite(wb.Ps_final).all()
        assert np.array_equal(wb.x, w.x, equal_nan=True) and np.array_equal(wb.prm, w.prm, equal_nan=True)
        # the epidemic states of the twin's start are the simulated end state of the chain's own region
        assert (wb.s_final[:2] >= 0).all() and (wb.s_final[:2] <= 1).all()
        few = wb.select(np.arange(0, w.B, max(1, w.B // 4))[:4])
        ref = H.oracle_batch(few, outputs=["S_MINUS", "P_MINUS"])
        assert np.isfinite(ref["S_MINUS"]).all() and np.isfinite(ref["P_MINUS"]).all()


@pytest.mark.gpu
def test_tool_runs_both_shapes(gpu_device, tmp_path):
    out = str(tmp_path / "bench.json")
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "tools", "bench_two_filter.py"), "--scale", str(1.0 / 300.0), "--calls", "2",
                        "--copy-doubles", str(1 << 22), "--out", out], capture_output=True, text=True, timeout=280, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.load(open(out))
    for name, m in (("m6_sweep", 6), ("m3_ensemble", 3)):
        s = res[name]
        assert s["m"] == m and s["floor_ms"] > 0 and s["eks_pinv_ms"] > 0
        for key in ("form1_solver0", "form0_solver0", "form0_solver1"):
            assert s[key]["median_ms"] > 0 and s[key]["reference_check"] == {"items": 16, "mismatches": 0}, (name, key, s[key])

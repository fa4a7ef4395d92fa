"""tools/bench_npi_plan.py on the CPU: its byte count against a hand count at a toy shape, and the inputs it builds."""
import importlib.util
import os

import numpy as np

from tests import helpers as H


def _tool():
    spec = importlib.util.spec_from_file_location("bench_npi_plan", os.path.join(H.ROOT, "tools", "bench_npi_plan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_executed_bytes_against_a_hand_count():
    f = _tool().executed_bytes
    # one chain, H = 2 days, n = 12, stopped by its first adjoint pass: start 96 + 24 + 4 = 124 B a day, adjoint 24 + 96 + 8 = 128 B
    # a day -> 2 x 252 = 504 B, and 52 B of results
    assert f(2, 12, [1], [0]) == 504 + 52
    # three adjoint passes, two accepted steps, one rejected trial: 124 + 3 x 128 + 3 x (96 + 4 + 96 + 24 = 220) = 1168 B a day;
    # an even number of accepted steps: no copy
    assert f(2, 12, [3], [1]) == 2 * 1168 + 52
    # two passes, one accepted step: the plan is copied over (192 B a day): 124 + 256 + 220 + 192 = 792
    assert f(1, 12, [2], [0]) == 792 + 52
    # n = 1, and a chain that never ran an adjoint pass (F not finite): the starting pass alone
    assert f(3, 1, [0], [0]) == 3 * (8 + 28) + 52
    assert f(2, 12, [1, 3], [0, 1]) == (504 + 52) + (2 * 1168 + 52)


def test_the_inputs():
    t = _tool()
    inp = t.make_inputs(scale=2.0 / 300.0, n_eps=7, horizon=11, t_hist=50)
    assert inp["sp"].shape == (48, 2) and inp["u_min"].shape == (12, 2) and inp["eps"].shape == (7,) and inp["H"] == 11
    assert inp["J0_prefix"].shape == (2,) and inp["J1_prefix"].shape == (2,) and inp["prefix_days"] == 50
    assert np.isfinite(inp["sp"]).all() and (inp["sp"][0] > 0).all() and (inp["sp"][0] <= 1).all() and (inp["sp"][11] == 1.0).all()
    assert t.histogram([1, 1, 3]) == {"1": 2, "3": 1}

"""tools/bench_innov_diag.py on the CPU: its byte count against a hand count, the sizes it builds, and its torch formulation
against the restatement on a complete series (it is the comparison the measurement reports, so it must compute the same things)."""
import importlib.util
import os

import numpy as np

from tests import helpers as H
from tests import innov_diag_ref as DR


def _tool():
    spec = importlib.util.spec_from_file_location("bench_innov_diag", os.path.join(H.ROOT, "tools", "bench_innov_diag.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_input_bytes_against_a_hand_count():
    f = _tool().input_bytes
    assert f(4, 5, 8) == 4 * 5 * 16 == 320                  # a double innovation and a double S per chain-day
    assert f(4, 5, 4) == 4 * 5 * 12 == 240                  # float storage
    assert f(3, 7, 4, with_S=False) == 84


def test_the_sizes():
    sizes = _tool().make_sizes(scale=1.0 / 300.0)
    assert [(n, w.m, w.B, w.T, st, lags) for n, w, st, lags in sizes] == [("headline", 6, 250, 520, "f64", (10, 32)),
                                                                           ("ensemble", 3, 1024, 400, "f32", (10,))]


def test_the_torch_formulation_computes_the_same_statistics(tmp_path):
    import torch
    e, S = DR.series(200, 5, seed=3)
    want = DR.InnovDiagRef(tmp_path).run(e, S, H=6, k0=21)
    got = _tool().torch_diagnostics(torch.as_tensor(e), torch.as_tensor(S), 6, 21)
    for k, v in got.items():
        assert np.allclose(v.numpy(), want[k], rtol=1e-9, atol=1e-12), k

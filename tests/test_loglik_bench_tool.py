"""tools/bench_loglik.py on the CPU: its byte count against a hand count at a toy shape, and the three sizes it builds."""
import importlib.util
import os

from tests import helpers as H


def _tool():
    spec = importlib.util.spec_from_file_location("bench_loglik", os.path.join(H.ROOT, "tools", "bench_loglik.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_algorithmic_bytes_against_a_hand_count():
    f = _tool().algorithmic_bytes
    # B = 4 chains, T = 5 days, doubles: per chain-day 9 + 3 + 1 stored values, x and R = 15 doubles = 120 B -> 2400 B;
    # loglik, nis_mean (8 B) and n_valid, status (4 B) per chain = 24 B -> 96 B
    assert f(4, 5, 8, ("loglik", "nis_mean", "n_valid", "status")) == 2400 + 96 == 2496
    # float storage: 13 x 4 + 16 = 68 B per chain-day -> 1360 B; S and R_used add 16 B per chain-day -> 320 B; loglik 32 B
    assert f(4, 5, 4, ("loglik", "S", "R_used")) == 1360 + 320 + 32 == 1712
    assert f(1, 1, 8, ("nis",)) == 120 + 8 and f(1, 1, 8, ("best", "best_loglik")) == 120


def test_the_three_sizes():
    sizes = _tool().make_sizes(scale=1.0 / 300.0)
    assert [(n, w.m, w.B, w.T, st) for n, w, st in sizes] == [("headline", 6, 250, 520, "f64"), ("shard", 6, 31, 520, "f64"),
                                                               ("ensemble", 3, 1024, 400, "f32")]
    assert all(w.R_series is not None for _, w, _ in sizes)

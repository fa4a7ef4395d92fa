"""The random hunt of the curve statistics without a device: every example of tests/fuzz_curve_depth.py through the NumPy
restatement, and through the host build of the lane-shaped kernels (tests/curve_depth_emu.cpp) where the example has a fence
envelope to hand them, against the C restatement, bit for bit; and what the default seeds cover.  EPI_FUZZ_EXAMPLES=n runs n seeds
from EPI_FUZZ_SEED on."""
import os
import time

import pytest

from tests import curve_depth_ref as S
from tests import fuzz_curve_depth as FZ
from tests.test_curve_depth_emu import LANE, run_emu
from tests.test_curve_depth_emu import cref, emu  # noqa: F401  (fixtures)

_N = int(os.environ.get("EPI_FUZZ_EXAMPLES", "0"))
_START = int(os.environ.get("EPI_FUZZ_SEED", str(time.time_ns() % 10 ** 9))) if _N else 0


def test_the_default_seeds_cover_the_axes():
    cov = FZ.coverage()
    assert all(v >= 2 for v in cov.values()), cov
    assert cov["host"] == FZ.DEFAULT_EXAMPLES // 4


def test_restatements_and_emulation_agree(emu, cref):  # noqa: F811
    seeds = range(_START, _START + _N) if _N else range(FZ.DEFAULT_EXAMPLES)
    if _N:
        print(f"EPI_FUZZ_SEED={_START} EPI_FUZZ_EXAMPLES={_N}")
    for s in seeds:
        x = FZ.draw(s)
        want = cref.statistics(**x["kw"], **x["opt"])
        alt = S.statistics(**x["kw"], **x["opt"])
        for k in x["names"]:
            assert S.same_bits(alt[k], want[k]), (s, k, "numpy")
        ff, frac = x["opt"]["fence_factor"], x["opt"]["fence_frac"]
        fence = cref.statistics(**x["kw"], alpha=(frac,), fence_factor=ff, fence_frac=frac)
        got, _ = run_emu(emu, (fence["env_lo"][:, 0], fence["env_hi"][:, 0]), fence_factor=ff, **x["kw"])
        for k in LANE:
            if ff > 0 or k not in S.NEED_FENCE:
                assert S.same_bits(got[k], want[k]), (s, k, "emu")

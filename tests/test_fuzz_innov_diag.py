"""The random hunt of the innovation whiteness diagnostics without a device: every example of tests/fuzz_innov_diag.py through
the host build of the kernels' source (tests/innov_diag_emu.cpp) against the restatement, bit for bit; the NumPy restatement on
every fourth; and what the default seeds cover.  EPI_FUZZ_EXAMPLES=n runs n seeds from EPI_FUZZ_SEED on."""
import os
import time

import pytest

from tests import fuzz_innov_diag as FZ
from tests import innov_diag_ref as DR
from tests.test_innov_diag_emu import build_emu, run_emu

_N = int(os.environ.get("EPI_FUZZ_EXAMPLES", "0"))
_START = int(os.environ.get("EPI_FUZZ_SEED", str(time.time_ns() % 10 ** 9))) if _N else 0


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return DR.InnovDiagRef(tmp_path_factory.mktemp("innov_diag_ref"))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build_emu(tmp_path_factory.mktemp("innov_diag_emu"))


def test_the_default_seeds_cover_the_axes():
    cov = FZ.coverage()
    assert all(v >= 2 for v in cov.values()), cov
    assert cov["host"] == FZ.DEFAULT_EXAMPLES // 4


def test_emulation_equals_the_restatement(emu, ref):
    seeds = range(_START, _START + _N) if _N else range(FZ.DEFAULT_EXAMPLES)
    if _N:
        print(f"EPI_FUZZ_SEED={_START} EPI_FUZZ_EXAMPLES={_N}")
    for s in seeds:
        x = FZ.draw(s)
        want = ref.run(x["e"], x["S"], **x["kw"])
        got = run_emu(emu, x["e"], x["S"], blk=x["blk"], names=x["outputs"], poison=True, **x["kw"])
        assert list(got) == [k for k in DR.ALL if x["outputs"] is None or k in x["outputs"]]
        for k, v in got.items():
            assert DR.same_bits(v, want[k]), (s, k)
        if s % 4 == 1:
            alt = DR.np_idiag(x["e"], x["S"], **x["kw"])
            for k in DR.ALL:
                assert DR.same_bits(alt[k], want[k]), (s, k, "numpy")

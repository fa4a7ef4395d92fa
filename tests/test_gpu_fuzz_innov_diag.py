"""The random hunt of the innovation whiteness diagnostics on the device: every example of tests/fuzz_innov_diag.py through
epi_idiag_run_device on poisoned, guarded outputs and workspace against the restatement, bit for bit; one example in four also
through hostapi.innovation_diagnostics.  The default run takes the seeds 0 .. DEFAULT_EXAMPLES - 1 (a few seconds);
EPI_FUZZ_EXAMPLES=n runs n seeds from EPI_FUZZ_SEED on (default: a fresh start, printed), a longer hunt."""
import os
import time

import pytest

from tests import fuzz_innov_diag as FZ
from tests import innov_diag_ref as DR
from tests.test_gpu_innov_diag import assert_equal, run_device
from tests.test_innov_diag_emu import blocked_input

pytestmark = pytest.mark.gpu

_N = int(os.environ.get("EPI_FUZZ_EXAMPLES", "0"))
_START = int(os.environ.get("EPI_FUZZ_SEED", str(time.time_ns() % 10 ** 9))) if _N else 0


def test_device_equals_the_restatement(gpu_device, tmp_path_factory):
    from epidemicmodeling_amd import hostapi
    ref = DR.InnovDiagRef(tmp_path_factory.mktemp("innov_diag_ref"))
    seeds = range(_START, _START + _N) if _N else range(FZ.DEFAULT_EXAMPLES)
    if _N:
        print(f"EPI_FUZZ_SEED={_START} EPI_FUZZ_EXAMPLES={_N}")
    for s in seeds:
        x = FZ.draw(s)
        kw = x["kw"]
        want = ref.run(x["e"], x["S"], **kw)
        got, clean = run_device(x["e"], x["S"], blk=x["blk"], outputs=x["outputs"], **kw)
        assert_equal(got, clean, want, f"seed {s}")
        if x["host"]:
            host = hostapi.innovation_diagnostics(blocked_input(x["e"], x["blk"], kw["storage"]), x["S"], n_lags=kw["H"], k0=kw["k0"],
                                                  k1=kw["k1"], flip=kw["flip"], lane_block=x["blk"], B=x["e"].shape[1],
                                                  outputs=x["outputs"])
            assert list(host) == list(got)
            for k, v in host.items():
                assert DR.same_bits(v, want[k]), (s, k, "hostapi")

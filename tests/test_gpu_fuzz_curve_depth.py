"""The random hunt of the curve statistics on the device: every example of tests/fuzz_curve_depth.py through epi_cdepth_run_device
on poisoned, guarded outputs and workspace against the C restatement, bit for bit; one example in four also through
hostapi.curve_statistics.  The default run takes the seeds 0 .. DEFAULT_EXAMPLES - 1 (a few seconds); EPI_FUZZ_EXAMPLES=n runs n
seeds from EPI_FUZZ_SEED on (default: a fresh start, printed), a longer hunt."""
import os
import time

import pytest

from tests import curve_depth_ref as S
from tests import fuzz_curve_depth as FZ
from tests.test_gpu_curve_depth import FILL, I32_FILL, _run_device, _same

pytestmark = pytest.mark.gpu

_N = int(os.environ.get("EPI_FUZZ_EXAMPLES", "0"))
_START = int(os.environ.get("EPI_FUZZ_SEED", str(time.time_ns() % 10 ** 9))) if _N else 0


def test_device_equals_the_restatement(gpu_device, tmp_path_factory):
    from epidemicmodeling_amd import hostapi
    ref = S.CurveDepthC(tmp_path_factory.mktemp("curve_depth_ref"))
    seeds = range(_START, _START + _N) if _N else range(FZ.DEFAULT_EXAMPLES)
    if _N:
        print(f"EPI_FUZZ_SEED={_START} EPI_FUZZ_EXAMPLES={_N}")
    for s in seeds:
        x = FZ.draw(s)
        want = ref.statistics(**x["kw"], **x["opt"])
        names = x["names"] if x["outputs"] is None else [k for k in S.NAMES if k in x["outputs"]]
        try:
            got = _run_device(device=gpu_device, names=names, test_segments=x["segments"], test_launch_groups=x["launch_groups"],
                              **x["kw"], **x["opt"])
            _same(got, want, names=names)
        except AssertionError as e:
            raise AssertionError(f"seed {s}: {e}") from e
        for k in S.NAMES:
            if k not in names:
                assert (got[k] == (I32_FILL if k in S.I32 else FILL)).all(), (s, k)
        if x["host"]:
            host = hostapi.curve_statistics(outputs=x["outputs"], test_segments=x["segments"], **x["kw"], **x["opt"])
            assert list(host) == names
            _same(host, want, names=names)

"""The kernels' source without a GPU: tests/ar_forecast_emu.cpp compiles csrc/ar_forecast.hpp for the host, runs every
workgroup as 64 lock-stepped threads (shuffles, ballots and barriers through a std::barrier) and compares ar_fit,
ar_given_status and ar_simulate with tests/ar_forecast_ref.c bit for bit on fifteen shapes: p = 24 / L = 120 in both nv_modes,
the smallest problem, both limits, row counts 62 .. 130, draws that end inside a workgroup, more regions than a workgroup has
lanes, drive with and without a series, the given model, rank-deficient / non-finite regions, a clamp that acts."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from tests import helpers as H


def test_kernel_source_in_lock_step_equals_the_c_reading(tmp_path):
    cc, cxx = shutil.which("gcc") or shutil.which("cc"), shutil.which("g++")
    if not cc or not cxx:
        pytest.fail("no C / C++ compiler for tests/ar_forecast_emu.cpp")
    t = os.path.join(H.ROOT, "tests")
    obj, exe = str(tmp_path / "ref.o"), str(tmp_path / "emu")
    subprocess.run([cc, "-O2", "-ffp-contract=off", "-c", os.path.join(t, "ar_forecast_ref.c"), "-o", obj], check=True)
    subprocess.run([cxx, "-std=c++20", "-O1", "-ffp-contract=off", "-I" + os.path.join(H.ROOT, "epidemicmodeling_amd", "csrc"),
                    os.path.join(t, "ar_forecast_emu.cpp"), obj, "-o", exe, "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, stdin=subprocess.DEVNULL)
    print(r.stdout)
    assert r.returncode == 0 and "cases 15, differing values 0" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-500:])


@pytest.mark.parametrize("D", [1, 64, 65, 2**31 - 64, 2**31 - 63, 2**31 - 1])
def test_blocks_per_region_at_the_ends_of_int(emu_so, D):
    """ar_blocks_per_region (csrc/ar_forecast.hpp), the function epi_arfc_run_device takes ar_simulate's workgroups per region
    from, is ceil(D / 64) up to D = 2^31 - 1, which epi_arfc_validate accepts with R = 1.  `(D + 63) / 64` in int, the
    expression it replaces, leaves int for D > 2^31 - 64: bpr and the block count went negative, no workgroup ran and the
    call returned EPI_OK with S untouched.  A GPU run at that D needs ~144 GiB of S, so this is a CPU test."""
    assert emu_so.emu_ar_blocks_per_region(C.c_int(D)) == -(-D // 64)


@pytest.fixture(scope="module")
def emu_so(tmp_path_factory):
    cc, cxx = shutil.which("gcc") or shutil.which("cc"), shutil.which("g++")
    if not cc or not cxx:
        pytest.fail("no C / C++ compiler for tests/ar_forecast_emu.cpp")
    d = tmp_path_factory.mktemp("ar_forecast_emu")
    obj, so = str(d / "ref.o"), str(d / "emu.so")
    subprocess.run([cc, "-O2", "-ffp-contract=off", "-fPIC", "-c", os.path.join(H.ROOT, "tests", "ar_forecast_ref.c"), "-o", obj], check=True)
    subprocess.run([cxx, "-std=c++20", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I" + os.path.join(H.ROOT, "epidemicmodeling_amd", "csrc"),
                    os.path.join(H.ROOT, "tests", "ar_forecast_emu.cpp"), obj, "-o", so, "-lpthread"], check=True)
    h = C.CDLL(so)
    h.emu_ar_blocks_per_region.restype = C.c_int
    return h

"""The kernels' source without a GPU: tests/rate_map_emu.cpp compiles csrc/rate_map.hpp for the host, runs every workgroup as
256 lock-stepped threads (__syncthreads through a std::barrier, the LDS one static array) and compares ratemap_items and
ratemap_region with tests/rate_map_ref.c bit for bit on ten shapes: F = 1, 2, 6, 7, 15, 24, 48, 65 and 96 (every
instantiation: 1, 2, 5, 10 and 19 entries of the triangle a lane), T = 1 .. 600 (test days beyond one block of 256), with
and without a fit, no ridge, launches cut into slices of train ends and of items, and planted leading-NaN, filled, zero-column
and NaN-pivot items."""
import os
import shutil
import subprocess

import pytest

from tests import helpers as H


def test_kernel_source_in_lock_step_equals_the_c_reading(tmp_path):
    cc, cxx = shutil.which("gcc") or shutil.which("cc"), shutil.which("g++")
    if not cc or not cxx:
        pytest.fail("no C / C++ compiler for tests/rate_map_emu.cpp")
    t = os.path.join(H.ROOT, "tests")
    obj, exe = str(tmp_path / "ref.o"), str(tmp_path / "emu")
    subprocess.run([cc, "-O2", "-ffp-contract=off", "-c", os.path.join(t, "rate_map_ref.c"), "-o", obj], check=True)
    subprocess.run([cxx, "-std=c++20", "-O1", "-ffp-contract=off", "-I" + os.path.join(H.ROOT, "epidemicmodeling_amd", "csrc"),
                    os.path.join(t, "rate_map_emu.cpp"), obj, "-o", exe, "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, stdin=subprocess.DEVNULL)
    print(r.stdout)
    assert r.returncode == 0 and "cases 10, status bits seen 7, differing values 0" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-500:])

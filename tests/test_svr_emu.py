"""The kernel's source without a GPU: tests/svr_emu.cpp compiles csrc/svr.hpp for the host, runs every workgroup as 256
lock-stepped threads (__syncthreads through a std::barrier, the LDS one static array of 160 KiB, poisoned behind the bytes a
launch asks for) and compares svr_items with tests/svr_ref.c bit for bit, both kernels, on (D, F, n_rows) = (2, 1, [1, 2]),
(9, 3, [5, 9]), (66, 7, [63, 64, 65]), (258, 5, [255, 256, 257]), (44, 96, [40]), (120, 49, [90]), (516, 3, [513]) -- one, two
and four rows a lane, prediction rows staged through LDS -- and on a launch cut into slices of row counts and of items with
max_iter = 3, with a planted NaN, a bad box and an overflowing column."""
import os
import shutil
import subprocess

import pytest

from tests import helpers as H


def test_kernel_source_in_lock_step_equals_the_c_reading(tmp_path):
    cc, cxx = shutil.which("gcc") or shutil.which("cc"), shutil.which("g++")
    if not cc or not cxx:
        pytest.fail("no C / C++ compiler for tests/svr_emu.cpp")
    t = os.path.join(H.ROOT, "tests")
    obj, exe = str(tmp_path / "ref.o"), str(tmp_path / "emu")
    subprocess.run([cc, "-O2", "-ffp-contract=off", "-c", os.path.join(t, "svr_ref.c"), "-o", obj], check=True)
    subprocess.run([cxx, "-std=c++20", "-O1", "-ffp-contract=off", "-I" + os.path.join(H.ROOT, "epidemicmodeling_amd", "csrc"),
                    os.path.join(t, "svr_emu.cpp"), obj, "-o", exe, "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, stdin=subprocess.DEVNULL)
    print(r.stdout)
    assert r.returncode == 0 and "cases 8, status bits seen 7, differing values 0\n" == r.stdout.splitlines(True)[-1], \
        (r.returncode, r.stdout[-2000:], r.stderr[-500:])

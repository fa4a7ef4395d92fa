"""The kernel's source without a GPU: tests/mldivide_emu.cpp compiles csrc/mldivide.hpp for the host, runs every workgroup as
256 lock-stepped threads (__syncthreads through a std::barrier, the LDS one static array of 160 KiB) and compares
mldivide_items with tests/mldivide_ref.c bit for bit on (n_rows, F) = (1, 1), (3, 5), (5, 5), (7, 2), (255, 3), (256, 3),
(257, 3), (206, 96) and (400, 49) -- the last two on the LDS limit, one to four rounds of 32 columns -- and on a launch cut
into slices of row counts and of items, with planted duplicate, zero, nearly cancelled, NaN and overflowing columns."""
import os
import shutil
import subprocess

import pytest

from tests import helpers as H


def test_kernel_source_in_lock_step_equals_the_c_reading(tmp_path):
    cc, cxx = shutil.which("gcc") or shutil.which("cc"), shutil.which("g++")
    if not cc or not cxx:
        pytest.fail("no C / C++ compiler for tests/mldivide_emu.cpp")
    t = os.path.join(H.ROOT, "tests")
    obj, exe = str(tmp_path / "ref.o"), str(tmp_path / "emu")
    subprocess.run([cc, "-O2", "-ffp-contract=off", "-c", os.path.join(t, "mldivide_ref.c"), "-o", obj], check=True)
    subprocess.run([cxx, "-std=c++20", "-O1", "-ffp-contract=off", "-I" + os.path.join(H.ROOT, "epidemicmodeling_amd", "csrc"),
                    os.path.join(t, "mldivide_emu.cpp"), obj, "-o", exe, "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, stdin=subprocess.DEVNULL)
    print(r.stdout)
    assert r.returncode == 0 and "cases 7, status bits seen 7" in r.stdout and "differing values 0\n" in r.stdout.splitlines(True)[-1], \
        (r.returncode, r.stdout[-2000:], r.stderr[-500:])

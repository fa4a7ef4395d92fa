"""The kernels' source without a GPU: tests/robust_fit_emu.cpp compiles csrc/robust_fit.hpp (and the ens_tree / ens_sort /
ens_pick it includes) for the host, runs every workgroup as 64 lock-stepped threads (shuffles and ballots through a
std::barrier) and compares robfit_items and robfit_intercept with tests/robust_fit_ref.c bit for bit on fourteen shapes:
D = 3, 4, 5, 63, 64, 65, 129, 300, 513 and 1024 (every NV), n = 1, 2 and 12, both robust settings, iteration caps that act,
three bounds settings, the intercept kernel fitting the items itself, and planted constant, slope-lost and non-finite items."""
import os
import shutil
import subprocess

import pytest

from tests import helpers as H


def test_kernel_source_in_lock_step_equals_the_c_reading(tmp_path):
    cc, cxx = shutil.which("gcc") or shutil.which("cc"), shutil.which("g++")
    if not cc or not cxx:
        pytest.fail("no C / C++ compiler for tests/robust_fit_emu.cpp")
    t = os.path.join(H.ROOT, "tests")
    obj, exe = str(tmp_path / "ref.o"), str(tmp_path / "emu")
    subprocess.run([cc, "-O2", "-ffp-contract=off", "-c", os.path.join(t, "robust_fit_ref.c"), "-o", obj], check=True)
    subprocess.run([cxx, "-std=c++20", "-O1", "-ffp-contract=off", "-I" + os.path.join(H.ROOT, "epidemicmodeling_amd", "csrc"),
                    os.path.join(t, "robust_fit_emu.cpp"), obj, "-o", exe, "-lpthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, stdin=subprocess.DEVNULL)
    print(r.stdout)
    assert r.returncode == 0 and "cases 14, status bits seen 31, differing values 0" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-500:])

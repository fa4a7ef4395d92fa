"""The joint score's host-side source without a GPU: tests/ejoint_emu.cpp compiles csrc/ens_joint.hpp for the host, and is built
with tests/ejoint_ref.c into a stand-alone program with -fsanitize=address,undefined and run.  It runs the header's workspace
layout, launch loop, block -> unit map, tile numbering and final pass on the restatement cases (D in 1, 2, 63, 64, 65, 130, 300; W
in 1, 2, 33; both storages; both first_day variants), uncut and in launches of 4, 5 and 7 units, and compares every output with the
C restatement bit for bit, and one case of D = 4 096 (64 blocks, 2 080 tiles an item) in launches of 1 003 units, a size that is no
multiple of 8; a slot outside the workspace is a sanitizer report."""
import os
import shutil
import subprocess

import pytest

from tests import helpers as H


def test_final_pass_and_unit_arithmetic_equal_the_c_restatement(tmp_path):
    cxx, cc = shutil.which("g++"), shutil.which("cc") or shutil.which("gcc")
    if not cxx or not cc:
        pytest.fail("no C / C++ compiler for tests/ejoint_emu.cpp")
    os.makedirs(tmp_path / "hip")
    (tmp_path / "hip" / "hip_runtime.h").write_text("#pragma once\n#define __device__\n#define __host__\n"
                                                    "#define __forceinline__ inline __attribute__((always_inline))\n")
    san = ["-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    ref_o, exe = str(tmp_path / "ejoint_ref.o"), str(tmp_path / "ejoint_emu")
    subprocess.run([cc, "-std=c11", "-fno-fast-math", *san, "-c", os.path.join(H.ROOT, "tests", "ejoint_ref.c"), "-o", ref_o], check=True)
    subprocess.run([cxx, "-std=c++17", *san, "-I" + str(tmp_path), "-I" + os.path.join(H.ROOT, "epidemicmodeling_amd", "csrc"),
                    os.path.join(H.ROOT, "tests", "ejoint_emu.cpp"), ref_o, "-o", exe, "-lm"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, stdin=subprocess.DEVNULL)
    print(r.stdout)
    assert r.returncode == 0 and "ejoint emu ok: 337 cases" in r.stdout and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])

"""The launch plan of csrc/launch_plan.hpp without a GPU: tests/launch_plan_test.cpp includes the header directly (plain C++17,
no HIP), is built as a stand-alone program with -fsanitize=address,undefined and run.  It checks the shape thresholds of
DESIGN.md 4.1, the headline sweep's and its shards' kernels and schedules, the kernels and schedule of every row of
SIA6_LAUNCHES (tests/test_gpu_npi_counts.py), and the tiling invariants of the forward / pinv / smoother lists over sizes,
shapes and test hooks; the expected values are written out in the program, worked out from the launch logic by hand."""
import os
import re
import shutil
import subprocess

import pytest

from tests import helpers as H

CSRC = os.path.join(H.ROOT, "epidemicmodeling_amd", "csrc")


def test_plan_picks_the_documented_kernels_and_its_lists_tile(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.fail("no C++ compiler for tests/launch_plan_test.cpp")
    exe = str(tmp_path / "launch_plan")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-variable", "-Wno-unused-function",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                    os.path.join(H.ROOT, "tests", "launch_plan_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, stdin=subprocess.DEVNULL)
    print(r.stdout)
    assert r.returncode == 0 and re.search(r"launch plan ok: 5\d cases, \d{6} plans", r.stdout) and not r.stderr, \
        (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    # the program's rows are the rows of SIA6_LAUNCHES, by name
    rows = re.findall(r'^    \("([a-z0-9-]+)", "', open(os.path.join(H.ROOT, "tests", "test_gpu_npi_counts.py")).read(), re.M)
    prog = open(os.path.join(H.ROOT, "tests", "launch_plan_test.cpp")).read()
    assert len(rows) == 18 and all('{"%s", ' % n in prog for n in rows), rows
    # the header stands alone (no HIP), and epiekf.hip decides nothing the plan decides
    hdr = open(os.path.join(CSRC, "launch_plan.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", hdr).lower()
    src = open(os.path.join(CSRC, "epiekf.hip")).read()
    assert "shape_of(" not in src and "balanced_lanes(" not in src and "lane6_block(" not in src
    assert src.count("simd_count(") == 2        # its definition and plan_input, the one place that feeds the plan

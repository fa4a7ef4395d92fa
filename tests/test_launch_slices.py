"""The launch helpers of csrc/epiekf.hip without a GPU: the lines between the "[launch slices]" markers (for_slices,
copy_counts: plain host C++) are copied into a header, tests/launch_slices_test.cpp is built around them as a stand-alone
program with -fsanitize=address,undefined and run.  It checks that the slices tile [0, items) exactly for items = 1, cap - 1,
cap, cap + 1, 2 cap + 3 (cap = 4) and past 2^33, that the first failing launch ends the loop, and that the chunks of at most
64 counts copy the right ones for K = 1, 63, 64, 65, 130."""
import os
import shutil
import subprocess

import pytest

from tests import helpers as H


def test_slices_tile_the_items_and_chunks_copy_the_counts(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.fail("no C++ compiler for tests/launch_slices_test.cpp")
    src = open(os.path.join(H.ROOT, "epidemicmodeling_amd", "csrc", "epiekf.hip")).read()
    begin, end = "// [launch slices]", "// [/launch slices]"
    assert src.count(begin) == 1 and src.count(end) == 1
    section = src[src.index(begin):src.index(end) + len(end)] + "\n"
    assert "for_slices" in section and "copy_counts" in section
    (tmp_path / "launch_slices_section.hpp").write_text(section)
    exe = str(tmp_path / "launch_slices")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + str(tmp_path),
                    os.path.join(H.ROOT, "tests", "launch_slices_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, stdin=subprocess.DEVNULL)
    print(r.stdout)
    assert r.returncode == 0 and "launch slices ok: 12 cases" in r.stdout and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    # every slice loop of the five entry points goes through the helper: none is written out any more
    assert src.count("for_slices(") == 1 + 7 and src.count("copy_counts(") == 1 + 3
    assert "+= kRfLaunchItems" not in src and "+= kRmLaunchItems" not in src and "+= kMlLaunchItems" not in src \
        and "+= kSvLaunchItems" not in src and "+= kEnsLaunchItems" not in src

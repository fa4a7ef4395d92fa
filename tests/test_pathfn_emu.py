"""The path functionals' source without a GPU: tests/pathfn_emu.cpp compiles csrc/path_functionals.hpp for the host and runs the
bodies of pathfn_paths and pathfn_combine one lane at a time; the per-path outputs equal the sequential C restatement
tests/pathfn_ref.c bit for bit, and the same bytes come out for 1, 2 and 3 segments and for one segment per 32-day block."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import pathfn_ref as S

PATH = S.PATH_F64 + S.THR_F64 + ("n_valid",)
FILL, I32_FILL = -98765.4321, -12345


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.fail("no C++ compiler for tests/pathfn_emu.cpp")
    d = tmp_path_factory.mktemp("pathfn_emu")
    os.makedirs(d / "hip")
    (d / "hip" / "hip_runtime.h").write_text("#pragma once\n#define __device__\n#define __host__\n"
                                             "#define __forceinline__ inline __attribute__((always_inline))\n")
    so = str(d / "emu.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I" + str(d),
                    "-I" + os.path.join(H.ROOT, "epidemicmodeling_amd", "csrc"), os.path.join(H.ROOT, "tests", "pathfn_emu.cpp"),
                    "-o", so], check=True)
    lib = C.CDLL(so)
    lib.emu_pathfn.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return S.PathfnC(tmp_path_factory.mktemp("pathfn_ref"))


def run_emu(lib, src, R, D, thr=None, population=None, first_day=None, k0=0, k1=None, segments=1, names=PATH):
    src = np.ascontiguousarray(src)
    T, rows, _ = src.shape
    k1 = T if k1 is None else k1
    ro = rows + int(population is not None)
    thr = None if thr is None else np.ascontiguousarray(thr, dtype=np.float64)
    nt = 0 if thr is None else len(thr)
    pop = None if population is None else np.ascontiguousarray(population, dtype=np.float64)
    fd = None if first_day is None else np.ascontiguousarray(first_day, dtype=np.int32)
    out = S.empty_outputs(ro, R, D, nt, k1 - k0, FILL, I32_FILL)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    nseg = lib.emu_pathfn(T, rows, R, D, nt, int(src.dtype == np.float32), int(pop is not None), k0, k1, segments, p(src), p(pop), p(thr),
                          p(fd), *[p(out[k]) if k in names else None for k in PATH])
    return {k: out[k] for k in PATH}, nseg


CASES = [dict(), dict(storage="f32"), dict(D=64, n_thr=0), dict(rows=1, n_thr=8, derive=False, D=5), dict(rows=5, T=55, k0=0, k1=55, D=4),
         dict(T=65, k0=1, k1=65, first_day=None, n_thr=2, D=4), dict(T=200, k0=3, k1=199, first_day=(0, 100, 198), D=4)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_lanes_equal_the_restatement_for_every_segment_count(emu, cref, case):
    kw = S.base_case(**CASES[case])
    want = cref.functionals(**kw)
    nblk = (kw["k1"] - kw["k0"] + 31) // 32
    seen = set()
    for segments in (1, 2, 3, nblk):
        got, nseg = run_emu(emu, segments=segments, **kw)
        seen.add(nseg)
        assert nseg <= min(segments, nblk)
        for k in PATH:
            assert S.same_bits(got[k], want[k]), (k, segments)
    assert seen >= {1, min(2, nblk), nblk}


def test_optional_outputs_are_left_alone(emu, cref):
    kw = S.base_case()
    want = cref.functionals(**kw)
    for segments in (1, 3):
        for names in (("total",), ("peak_day", "longest_run"), ("n_valid", "first_cross", "min_value")):
            got, _ = run_emu(emu, segments=segments, names=names, **kw)
            for k in PATH:
                if k in names:
                    assert S.same_bits(got[k], want[k]), k
                else:
                    assert (got[k] == (I32_FILL if got[k].dtype == np.int32 else FILL)).all(), k


def test_a_run_across_every_border(emu):
    """one path above on all 200 days, one broken only on the first day of a block, one above only on the last day of each block"""
    T, k0 = 200, 4
    src = np.zeros((T, 1, 3))
    src[:, 0, 0] = 2.0
    src[:, 0, 1] = 2.0
    src[k0 + 64, 0, 1] = 0.0
    src[k0 + 31::32, 0, 2] = 2.0
    thr = np.ones((1, 1, 1))
    want = S.functionals(src, 1, 3, thr, k0=k0)
    assert list(want["longest_run"][0, 0]) == [196.0, 131.0, 1.0] and list(want["days_above"][0, 0]) == [196.0, 195.0, 6.0]
    for segments in (1, 2, 3, 4, 7):
        got, _ = run_emu(emu, src, 1, 3, thr, k0=k0, segments=segments)
        for k in PATH:
            assert S.same_bits(got[k], want[k]), (k, segments)

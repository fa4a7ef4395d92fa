"""The seeded draws' kernel source without a GPU: tests/noise_emu.cpp compiles csrc/noise.hpp (and csrc/smoother_draws.hpp over
it) for the host.  The fill lane, walked in cut launches, equals the restatement tests/noise_ref.c bit for bit on the windows
that reach the high counter words, as double and as float; the one-draw function equals it too; and the smoother-draw path lane
in its generated-noise mode equals the same lane given the filled array."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import noise_ref as NR

SEED = 0x13198A2E03707344


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return NR.NoiseRef(tmp_path_factory.mktemp("noise_ref"))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.fail("no C++ compiler for tests/noise_emu.cpp")
    d = tmp_path_factory.mktemp("noise_emu")
    os.makedirs(d / "hip")
    (d / "hip" / "hip_runtime.h").write_text("#pragma once\n#define __device__\n#define __host__\n"
                                             "#define __forceinline__ inline __attribute__((always_inline))\n")
    so = str(d / "emu.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-I" + str(d),
                    "-I" + os.path.join(H.ROOT, "epidemicmodeling_amd", "csrc"), os.path.join(H.ROOT, "tests", "noise_emu.cpp"),
                    "-o", so], check=True)
    h = C.CDLL(so)
    h.emu_noise_fill.argtypes = [C.c_uint32] * 4 + [C.c_int] * 2 + [C.c_uint64] * 2 + [C.c_int] * 2 + [C.c_void_p]
    h.emu_normal_draw.argtypes = [C.c_uint32] * 5 + [C.c_uint64]
    h.emu_normal_draw.restype = C.c_double
    h.emu_sdraw_paths.argtypes = [C.c_int] * 6 + [C.c_uint32] * 3 + [C.c_void_p] * 7
    h.emu_noise_fill.restype = h.emu_sdraw_paths.restype = None
    return h


def emu_fill(h, seed, stream, t0, nt, rows, lane0, n, f32=False, groups=1 << 20):
    buf = np.full(nt * rows * n + 8, -7, dtype=np.float32 if f32 else np.float64)        # four guard words on either side
    h.emu_noise_fill(seed & 0xFFFFFFFF, seed >> 32, stream, t0, nt, rows, lane0, n, int(f32), groups, buf[4:].ctypes.data)
    assert (buf[:4] == -7).all() and (buf[-4:] == -7).all()
    return buf[4:-4].reshape(nt, rows, n).copy()


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("stream", [0, 2 ** 30 - 1])
def test_fill_lane_equals_restatement(emu, ref, rows, stream):
    for t0 in (0, 2 ** 32 - 3):
        for lane0 in (0, 2 ** 32 - 2, 2 ** 40 + 1):
            want = ref.fill(SEED, stream, t0, 3, rows, lane0, 130)
            assert NR.same_bits(emu_fill(emu, SEED, stream, t0, 3, rows, lane0, 130), want), (t0, lane0)
            assert NR.same_bits(emu_fill(emu, SEED, stream, t0, 3, rows, lane0, 130, f32=True), want.astype(np.float32)), (t0, lane0)
    # 3 * 2 * 300 items = 8 workgroups of 256 lanes (the last ragged), one per launch
    want = ref.fill(SEED, stream, 1, 3, rows, 9, 300)
    assert NR.same_bits(emu_fill(emu, SEED, stream, 1, 3, rows, 9, 300, groups=1), want)


def test_one_draw_equals_restatement(emu, ref):
    want = ref.fill(SEED, 5, 2, 2, 3, 2 ** 33 + 1, 4)
    for t in range(2):
        for row in range(3):
            for l in range(4):
                got = emu.emu_normal_draw(SEED & 0xFFFFFFFF, SEED >> 32, 5, 2 + t, row, 2 ** 33 + 1 + l)
                assert got == want[t, row, l], (t, row, l)


@pytest.mark.parametrize("T,k0", [(6, 0), (6, 2), (3, 0), (3, 2)])
@pytest.mark.parametrize("clamp", [0, 1])
def test_sdraw_path_lane_generates_what_it_would_read(emu, ref, T, k0, clamp):
    from epidemicmodeling_amd import synth
    from tests import sdraw_ref as SR
    B, D = 3, 70
    w = synth.make_cfg3(B, T)
    case = SR.case_of(w, H.oracle_batch(w))
    big = [np.ascontiguousarray(case[k], dtype=np.float64) for k in SR.BIG]
    prm = np.ascontiguousarray(case["prm"], dtype=np.float64)
    z = ref.fill(SEED, 3, 0, T - k0, 3, 0, B * D)
    X = {}
    for mode in (1, 3):
        X[mode] = np.full((T - k0, 3, B * D), -7.0)
        emu.emu_sdraw_paths(B, T, D, k0, clamp, mode, SEED & 0xFFFFFFFF, SEED >> 32, 3, *[a.ctypes.data for a in big], prm.ctypes.data,
                            z.ctypes.data, X[mode].ctypes.data)
    assert NR.same_bits(X[1], X[3])
    assert np.isfinite(X[3]).all() and not (X[3] == -7.0).any()
    assert float(np.std(X[3][0, 2].reshape(B, D), axis=1).min()) > 0.0               # the draws of a chain differ: noise was added

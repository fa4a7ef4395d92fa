"""The kernels' source without a GPU: tests/sdraw_emu.cpp compiles csrc/smoother_draws.hpp for the host and runs both kernel
bodies one lane at a time; X, J, L, rank and status equal the restatement tests/sdraw_ref.py bit for bit -- classic layout and
8-chain blocks with B = 21 (the padding lanes hold NaN), float64 and float32 for the inputs, z and X, D = 1, 3, 64, 70, k0 and
clamp, the terminal law, the planted days, and a launch cut forced through a small bound."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import loglik_ref as LR
from tests import sdraw_ref as SR

NAMES = ("X", "rank", "status", "J", "L")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return SR.SdrawRef(tmp_path_factory.mktemp("sdraw_ref"))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.fail("no C++ compiler for tests/sdraw_emu.cpp")
    d = tmp_path_factory.mktemp("sdraw_emu")
    os.makedirs(d / "hip")
    (d / "hip" / "hip_runtime.h").write_text("#pragma once\n#define __device__\n#define __host__\n"
                                             "#define __forceinline__ inline __attribute__((always_inline))\n")
    so = str(d / "emu.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-I" + str(d),
                    "-I" + os.path.join(H.ROOT, "epidemicmodeling_amd", "csrc"), os.path.join(H.ROOT, "tests", "sdraw_emu.cpp"),
                    "-o", so], check=True)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def case21():
    """B = 21, T = 9: the first 21 chains and the last 9 days of a 45-day run would not be a filter run; a 9-day run is"""
    from epidemicmodeling_amd import synth
    w = synth.make_cfg3(21, 9)
    return w, SR.case_of(w, H.oracle_batch(w))


def run_emu(lib, case, D, z=None, s_term=None, P_term=None, k0=0, clamp=True, storage="f64", out_f32=False, blk=0, groups=1 << 20):
    B, T = case["B"], case["T"]
    dt = np.float32 if storage == "f32" else np.float64
    keep = []

    def arr(a, dtype=np.float64):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        keep.append(a)
        return a.ctypes.data_as(C.c_void_p)
    with np.errstate(over="ignore", invalid="ignore"):
        big = [case[k].astype(dt) for k in SR.BIG]
    if blk:
        big = [LR.to_blocked(a, blk, np.nan) for a in big]
    out = dict(X=np.full((T - k0, 3, B * D), -7, dtype=np.float32 if out_f32 else np.float64), rank=np.full((T, B), -7, dtype=np.int32),
               status=np.full(B, -7, dtype=np.int32), J=np.full((T, 9, B), -7.0), L=np.full((T, 9, B), -7.0))
    zm = 0 if z is None else (2 if z.dtype == np.float32 else 1)
    lib.emu_sdraw(B, T, D, int(k0), int(clamp), int(blk), int(storage == "f32"), zm, int(out_f32), int(groups), *[arr(a, dt) for a in big],
                  arr(case["prm"]), arr(z, None if z is None else z.dtype), arr(s_term), arr(P_term),
                  *[out[k].ctypes.data_as(C.c_void_p) for k in NAMES])
    return out


def _same(got, want, what):
    for k in NAMES:
        assert SR.same_bits(got[k], want[k]), (k, what)


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("name", SR.WORKLOADS)
def test_workloads(emu, ref, name, storage):
    w, case = SR.oracle_case(name)
    for D, k0, clamp, noise in ((1, 0, True, False), (3, 0, True, True), (3, 11, False, True), (70, 5, True, True)):
        z = SR.draws(w.T, k0, w.B, D, seed=D + k0) if noise else None
        want = ref.run(case, D, z, k0=k0, clamp=clamp, storage=storage)
        _same(run_emu(emu, case, D, z, k0=k0, clamp=clamp, storage=storage, blk=0 if D == 1 else 3), want, (D, k0, clamp))


@pytest.mark.parametrize("D", [1, 3, 64, 70])
@pytest.mark.parametrize("blk", [0, 8])
def test_b21_layouts_and_types(emu, ref, case21, D, blk):
    w, case = case21
    for storage, zt, of in (("f64", np.float64, False), ("f32", np.float64, False), ("f64", np.float32, True), ("f32", np.float32, False)):
        z = SR.draws(w.T, 0, w.B, D, seed=3, dtype=zt)
        want = ref.run(case, D, z, storage=storage, out_f32=of)
        _same(run_emu(emu, case, D, z, storage=storage, out_f32=of, blk=blk), want, (storage, zt, of))


def test_launch_cut_and_terminal(emu, ref, case21):
    w, case = case21
    z = SR.draws(w.T, 2, w.B, 70, seed=4)
    s_term, P_term = case["S_SMOOTH"][-1] * 1.001, case["P_SMOOTH"][-1] * 0.5
    want = ref.run(case, 70, z, s_term=s_term, P_term=P_term, k0=2)
    assert 21 * 70 > 2 * 256                                   # several launches of two workgroups
    _same(run_emu(emu, case, 70, z, s_term=s_term, P_term=P_term, k0=2, blk=8, groups=2), want, "cut")


def test_planted_days(emu, ref):
    case = SR.planted_case()
    for clamp in (True, False):
        z = SR.draws(case["T"], 0, case["B"], 3, seed=6)
        want = ref.run(case, 3, z, clamp=clamp)
        _same(run_emu(emu, case, 3, z, clamp=clamp, blk=2), want, clamp)

"""The kernels' source without a GPU: tests/loglik_emu.cpp compiles csrc/loglik.hpp for the host and runs every kernel body one
lane at a time; every output equals the restatement tests/loglik_ref.py bit for bit on the oracle's outputs of the seven
workloads -- classic layout and 40-chain blocks (70 is no multiple of 40; the padding lanes hold NaN and a poison that would
show in the sums), f64 and f32 storage, the windows, the planted days, the selection."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from epidemicmodeling_amd import layout as L
from tests import helpers as H
from tests import loglik_ref as LR


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return LR.LoglikRef(tmp_path_factory.mktemp("loglik_ref"))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.fail("no C++ compiler for tests/loglik_emu.cpp")
    d = tmp_path_factory.mktemp("loglik_emu")
    os.makedirs(d / "hip")
    (d / "hip" / "hip_runtime.h").write_text("#pragma once\n#define __device__\n#define __host__\n"
                                             "#define __forceinline__ inline __attribute__((always_inline))\n")
    so = str(d / "emu.so")
    subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-mfma", "-fPIC", "-shared", "-I" + str(d),
                    "-I" + os.path.join(H.ROOT, "epidemicmodeling_amd", "csrc"), os.path.join(H.ROOT, "tests", "loglik_emu.cpp"),
                    "-o", so], check=True)
    return C.CDLL(so)


def run_emu(lib, case, k0=0, k1=None, storage="f64", G=0, blk=0, names=None):
    m, flip, generic, fixed = LR.model_info(case["model"])
    B, T = case["B"], case["T"]
    dt = np.float32 if storage == "f32" else np.float64
    keep = []

    def arr(a, dtype=np.float64):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        keep.append(a)
        return a.ctypes.data_as(C.c_void_p)
    with np.errstate(over="ignore"):
        big = [case[k].astype(dt) for k in ("S_MINUS", "P_MINUS", "innovations")]
    if blk:
        big = [LR.to_blocked(a, blk, np.nan) for a in big]
    names = LR.ALL[:7] + (LR.SELECT if G else ()) if names is None else names
    shapes = {k: (B,) for k in LR.PER_CHAIN}
    shapes.update({k: (T, B) for k in LR.PER_DAY})
    shapes.update({k: (B // G if G else 0,) for k in LR.SELECT})
    out = {k: np.full(shapes[k], -7, dtype=np.int32 if k in ("n_valid", "status", "best") else np.float64) for k in names}
    lib.emu_loglik(m, int(flip), int(generic), 0 if fixed else L.OBS_IDS[case["obs_type"]], B, T, case["L"], case["x"].shape[1],
                   int(case["R_series"] is not None), int(storage == "f32"), int(k0), T if k1 is None else int(k1), int(G), int(blk),
                   *[arr(a, dt) for a in big], arr(case["x"]), arr(case["R_series"]), arr(case["R_scalar"]),
                   arr(case["x_series"], np.int32), arr(case["prm"]), *[arr_out(out, k) for k in LR.ALL])
    return out


def arr_out(out, k):
    return out[k].ctypes.data_as(C.c_void_p) if k in out else None


def _same(got, want, what):
    for k, v in got.items():
        assert LR.same_bits(v, want[k]), (k, what)


@pytest.mark.parametrize("storage", ["f64", "f32"])
@pytest.mark.parametrize("name", LR.WORKLOADS)
def test_seven_workloads(emu, ref, name, storage):
    w, case = LR.oracle_case(name)
    for k0, k1 in LR.WINDOWS:
        if (k1 or w.T) > w.T:
            continue
        want = ref.run(case, k0=k0, k1=k1, storage=storage)
        for blk in (0, 40) if w.B > 40 else (0, 3):
            _same(run_emu(emu, case, k0, k1, storage, blk=blk), want, (k0, k1, blk))


@pytest.mark.parametrize("name", ["cfg3", "cfg4", "row3", "cfg3_bwd"])
def test_planted_days(emu, ref, name):
    w = LR.with_missing_days(LR.oracle_case(name)[0])
    case = LR.with_bad_days(LR.case_of(w, H.oracle_batch(w)))
    for storage in ("f64", "f32"):
        want = ref.run(case, storage=storage)
        assert (want["status"] & 1).sum() >= 1 and (want["n_valid"] == 0).any()
        _same(run_emu(emu, case, storage=storage, blk=0 if w.B < 40 else 40), want, storage)


def test_single_outputs_and_selection(emu, ref):
    w, case = LR.oracle_case("cfg3")
    want = ref.run(case, G=14)
    _same(run_emu(emu, case, G=14, blk=40), want, "selection")
    for k in LR.ALL[:7]:
        _same(run_emu(emu, case, names=(k,)), want, k)
    _same(run_emu(emu, case, G=14, names=("R_used", "best")), want, "best without loglik")


def test_adaptive_chain_single_output_R_used(emu, ref):
    w, case = LR.oracle_case("row3")
    want = ref.run(case)
    _same(run_emu(emu, case, names=("R_used",)), want, "R_used")
    _same(run_emu(emu, case, names=("loglik",), blk=5), want, "loglik")

"""The plan query of tests/plan_query.cpp from Python: which kernel instances a call launches, and every instance any call can.

The query is plain C++17 around csrc/launch_plan.hpp (no HIP, no GPU, no sanitizer), built once per process with g++ into a
temporary shared object and loaded with ctypes; it takes the library's own descriptor structure (_lib.BatchDesc)."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

from epidemicmodeling_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "epidemicmodeling_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "plan_query.cpp")

SHAPES = {0: "auto", 1: "lane", 2: "quad", 3: "wave", 4: "hex"}
# ScheduleBits of csrc/launch_plan.hpp
SCHED = {"OVERLAP": 1, "TIME_PIPE": 2, "REVERSE_PIPE": 4, "FWD_RANGES": 8, "BWD_ROUNDS": 16, "BWD_HORIZON": 32}

_handle = None
_tmp = None


def sched_bits(names):
    """'OVERLAP|FWD_RANGES' or an iterable of names -> the schedule word; '' = serial."""
    if isinstance(names, str):
        names = [n for n in names.split("|") if n]
    v = 0
    for n in names:
        v |= SCHED[n]
    return v


def sched_names(v):
    return "|".join(n for n, b in SCHED.items() if v & b) or "serial"


def lib():
    """The loaded query (built on first use).  RuntimeError if there is no g++ or the build fails."""
    global _handle, _tmp
    if _handle is None:
        cxx = shutil.which("g++")
        if not cxx:
            raise RuntimeError("no g++ to build tests/plan_query.cpp")
        _tmp = tempfile.TemporaryDirectory(prefix="plan_query_")
        so = os.path.join(_tmp.name, "libplan_query.so")
        r = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unused-variable", "-fPIC", "-shared",
                            "-I" + CSRC, SRC, "-o", so], capture_output=True, text=True, stdin=subprocess.DEVNULL)
        if r.returncode != 0:
            raise RuntimeError("building tests/plan_query.cpp failed:\n" + r.stderr[-4000:])
        h = C.CDLL(so)
        h.epi_plan_query.restype = C.c_int
        h.epi_plan_query.argtypes = [C.POINTER(_lib.BatchDesc), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                     C.c_char_p, C.c_size_t]
        h.epi_plan_enumerate.restype = C.c_int
        h.epi_plan_enumerate.argtypes = [C.c_int, C.POINTER(C.c_int64), C.c_char_p, C.c_size_t]
        _handle = h
    return _handle


def query(desc, n_simds, extras=True, t_hist=None):
    """The launches of one call on `n_simds` SIMDs: desc a _lib.BatchDesc as the call passes it, extras = pinv_rank and status are
    outputs, t_hist = the sweep entry's (None: epi_ekf_run_device).  Returns dict shape (name), lw, schedule (bits), fwd_lds,
    launches [(role, name)] in launch order, names (set of the first pass), second (set of the dense second pass of
    exact_nonfinite, which does work only for chains whose status marks an overflow)."""
    facts = (C.c_int32 * 8)()
    buf = C.create_string_buffer(1 << 14)
    n = lib().epi_plan_query(C.byref(desc), int(bool(extras)), int(bool(extras)), int(n_simds), int(t_hist is not None),
                             int(t_hist or 0), facts, buf, len(buf))
    assert n >= 0 and not facts[5], (n, list(facts))
    launches = [tuple(l.split(" ", 1)) for l in buf.value.decode().splitlines()]
    return {"shape": SHAPES[facts[0]], "lw": int(facts[1]), "schedule": int(facts[2]), "fwd_lds": int(facts[3]), "launches": launches,
            "names": {n for r, n in launches if not r.startswith("second_")},
            "second": {n for r, n in launches if r.startswith("second_")}}


def enumerate_instances(n_simds):
    """(sorted names of every instance any plan on n_simds SIMDs can launch, number of plans walked)."""
    plans = C.c_int64(0)
    buf = C.create_string_buffer(1 << 16)
    n = lib().epi_plan_enumerate(int(n_simds), C.byref(plans), buf, len(buf))
    assert n > 0, n
    names = buf.value.decode().splitlines()
    assert len(names) == n
    return names, int(plans.value)

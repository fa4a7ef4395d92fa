"""The C ABI of the seeded draws without a GPU (every case is decided before a device is touched): the refusals of
epi_noise_validate and epi_noise_fill_*, of every *_seeded entry for a bad noise descriptor or a non-NULL z, the layout of
epi_noise_desc, the new symbols -- and the size of every structure the header had before, measured by a C compiler on the
header itself: additions only, ABI 6."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H

# sizeof of every structure of include/epiekf.h before the seeded draws were added (x86-64)
OLD_SIZES = {'epi_batch_desc': 92, 'epi_inputs': 96, 'epi_placement_report': 40, 'epi_outputs': 112, 'epi_sim_desc': 36, 'epi_mc_desc': 36,
             'epi_sweep_desc': 16, 'epi_prescribe_desc': 52, 'epi_prescribe_inputs': 104, 'epi_prescribe_outputs': 168,
             'epi_lookahead_desc': 52, 'epi_lookahead_inputs': 96, 'epi_lookahead_outputs': 88, 'epi_rtwin_desc': 40, 'epi_rtwin_outputs': 112,
             'epi_lasso_desc': 48, 'epi_lasso_outputs': 96, 'epi_ens_desc': 160, 'epi_ens_outputs': 48, 'epi_arfc_desc': 48,
             'epi_arfc_inputs': 72, 'epi_arfc_outputs': 32, 'epi_fuse_desc': 36, 'epi_fuse_inputs': 32, 'epi_fuse_outputs': 40,
             'epi_robfit_desc': 40, 'epi_robfit_outputs': 56, 'epi_ratemap_desc': 72, 'epi_ratemap_inputs': 48, 'epi_ratemap_outputs': 56,
             'epi_mldiv_desc': 32, 'epi_mldiv_inputs': 24, 'epi_mldiv_outputs': 56, 'epi_svr_desc': 40, 'epi_svr_inputs': 48,
             'epi_svr_outputs': 64, 'epi_rt_desc': 24, 'epi_rt_outputs': 72, 'epi_pre_desc': 32, 'epi_pre_outputs': 72, 'epi_nnls_desc': 20,
             'epi_loglik_desc': 56, 'epi_loglik_inputs': 64, 'epi_loglik_outputs': 72, 'epi_plan_desc': 40, 'epi_plan_inputs': 56,
             'epi_plan_outputs': 88, 'epi_sdraw_desc': 48, 'epi_sdraw_inputs': 64, 'epi_sdraw_outputs': 40, 'epi_escore_desc': 120,
             'epi_escore_inputs': 40, 'epi_escore_outputs': 112, 'epi_pathfn_desc': 48, 'epi_pathfn_inputs': 32, 'epi_pathfn_outputs': 104,
             'epi_ejoint_desc': 56, 'epi_ejoint_inputs': 40, 'epi_ejoint_outputs': 56}
NEW_SYMBOLS = ("epi_noise_validate", "epi_noise_fill_device", "epi_noise_fill_host", "epi_sdraw_run_device_seeded",
               "epi_sdraw_run_host_seeded", "epi_arfc_run_device_seeded", "epi_arfc_run_host_seeded", "epi_sialpha_sim_device_seeded",
               "epi_sialpha_score_device_seeded", "epi_sialpha_sim_host_seeded", "epi_random_npi_mc_device_seeded",
               "epi_random_npi_mc_host_seeded")


def _noise(seed=7, stream=0, abi=None):
    from epidemicmodeling_amd import _lib
    d = _lib.make_noise_desc(seed, stream)
    if abi is not None:
        d.abi_version = abi
    return d


def test_validate(hip_lib):
    err = C.create_string_buffer(256)
    assert hip_lib.epi_noise_validate(C.byref(_noise()), err) == 0
    assert hip_lib.epi_noise_validate(C.byref(_noise(2 ** 64 - 1, 2 ** 30 - 1)), err) == 0
    for d, msg in ((None, "NULL noise descriptor"), (C.byref(_noise(abi=5)), "ABI version mismatch"),
                   (C.byref(_noise(stream=2 ** 30)), "stream must be below 2^30"), (C.byref(_noise(stream=2 ** 32 - 1)), "stream must be below 2^30")):
        assert hip_lib.epi_noise_validate(d, err) == -5 and err.value.decode() == msg


FILL_BAD = [
    (dict(rows=2), "rows must be 1 or 3"), (dict(rows=0), "rows must be 1 or 3"), (dict(nt=0), "nt and n_lanes must be >= 1"),
    (dict(n_lanes=0), "nt and n_lanes must be >= 1"), (dict(t0=-1), "t is one counter word"),
    (dict(t0=2 ** 32 - 2), "t is one counter word"),            # nt = 3 from there leaves the 32-bit word
    (dict(t0=2 ** 40 + 1), "t is one counter word"), (dict(lane0=-1), "lane0 .. lane0 + n_lanes must lie in 0 .. 2^63"),
    (dict(lane0=2 ** 63 - 4), "lane0 .. lane0 + n_lanes must lie in 0 .. 2^63"), (dict(n_lanes=2 ** 61), "more than 2^62 elements"),
    (dict(out_f32=2), "out_f32 must be 0 (double) or 1 (float)"), (dict(groups=-1), "test_launch_groups must be >= 0"),
    (dict(out=None), "NULL out"), (dict(stream=2 ** 30), "stream must be below 2^30"),
]


@pytest.mark.parametrize("kw, msg", FILL_BAD)
def test_fill_refusals(hip_lib, kw, msg):
    buf = np.ones(64)
    a = dict(t0=0, nt=3, rows=3, lane0=0, n_lanes=5, out_f32=0, out=buf.ctypes.data, groups=0, stream=0)
    a.update(kw)
    d, err = _noise(stream=a["stream"]), C.create_string_buffer(256)
    head = (C.byref(d), a["t0"], a["nt"], a["rows"], a["lane0"], a["n_lanes"], a["out_f32"], a["out"])
    assert hip_lib.epi_noise_fill_device(*head, a["groups"], None, err) == -5 and msg in err.value.decode(), err.value
    if "groups" not in kw:
        assert hip_lib.epi_noise_fill_host(*head, 0, err) == -5 and msg in err.value.decode(), err.value
    # the last window that fits is accepted up to the pointer check
    assert hip_lib.epi_noise_fill_host(C.byref(_noise()), 2 ** 32 - 3, 3, 3, 2 ** 63 - 5, 5, 0, None, 0, err) == -5
    assert err.value.decode() == "NULL out"


def _seeded_calls(noise, z):
    """every *_seeded entry with `noise` and `z` and otherwise acceptable arguments: (name, rc, message)"""
    from epidemicmodeling_amd import _lib
    lib, err, buf = _lib.lib(), C.create_string_buffer(256), np.ones(4096)
    p = buf.ctypes.data
    np_ = None if noise is None else C.byref(noise)
    out = []
    sd = _lib.make_sdraw_desc(5, 6, 3)
    sin, sout = _lib.SdrawInputs(), _lib.SdrawOutputs()
    for k in _lib.SDRAW_IN_NAMES:
        setattr(sin, k, z if k == "z" else p)
    for k in _lib.SDRAW_OUT_NAMES:
        setattr(sout, k, p)
    out.append(("sdraw device", lib.epi_sdraw_run_device_seeded(C.byref(sd), np_, C.byref(sin), C.byref(sout), p, 1 << 20, None, err), err.value.decode()))
    out.append(("sdraw host", lib.epi_sdraw_run_host_seeded(C.byref(sd), np_, C.byref(sin), C.byref(sout), 0, err), err.value.decode()))
    ad = _lib.make_arfc_desc(2, 3, 20, 3, 5, 1.0)
    ain, aout = _lib.ArfcInputs(), _lib.ArfcOutputs()
    for k in ("seg", "beta", "s0", "i0"):
        setattr(ain, k, p)
    ain.z = z
    for k in _lib.ARFC_OUT_NAMES:
        setattr(aout, k, p)
    out.append(("arfc device", lib.epi_arfc_run_device_seeded(C.byref(ad), np_, C.byref(ain), C.byref(aout), None, err), err.value.decode()))
    out.append(("arfc host", lib.epi_arfc_run_host_seeded(C.byref(ad), np_, C.byref(ain), C.byref(aout), 0, err), err.value.decode()))
    sm = _lib.SimDesc()
    sm.abi_version, sm.B, sm.K, sm.Su, sm.n_npi, sm.noise, sm.with_cost = _lib.ABI_VERSION, 4, 5, 4, 2, 1, 1
    out.append(("sialpha_sim device", lib.epi_sialpha_sim_device_seeded(C.byref(sm), np_, None, p, p, z, p, p, p, p, p, None, err), err.value.decode()))
    out.append(("sialpha_score device", lib.epi_sialpha_score_device_seeded(C.byref(sm), np_, None, p, p, z, None, None, p, p, p, p, p, None, err),
                err.value.decode()))
    out.append(("sialpha_sim host", lib.epi_sialpha_sim_host_seeded(C.byref(sm), np_, None, p, p, z, p, p, p, p, p, 0, err), err.value.decode()))
    mc = _lib.McDesc()
    mc.abi_version, mc.R, mc.n_scen, mc.K, mc.n_npi, mc.noise = _lib.ABI_VERSION, 3, 4, 5, 2, 1
    out.append(("random_npi_mc device", lib.epi_random_npi_mc_device_seeded(C.byref(mc), np_, p, p, z, None, None, None, p, p, None, err), err.value.decode()))
    out.append(("random_npi_mc host", lib.epi_random_npi_mc_host_seeded(C.byref(mc), np_, p, p, z, None, None, None, p, p, 0, err), err.value.decode()))
    return out


def test_every_seeded_entry_refuses_a_z_and_a_bad_descriptor(hip_lib):
    z = np.ones(4096)
    got = _seeded_calls(_noise(), z.ctypes.data)
    assert len(got) == 9
    for name, rc, msg in got:
        assert rc == -5 and msg == "a seeded call takes no z: the draws have one source", (name, rc, msg)
    for noise, want in ((None, "NULL noise descriptor"), (_noise(abi=5), "ABI version mismatch"), (_noise(stream=2 ** 30), "stream must be below 2^30")):
        for name, rc, msg in _seeded_calls(noise, None):
            assert rc == -5 and msg == want, (name, rc, msg)


def test_layout_symbols_and_sizes(hip_lib, tmp_path):
    from epidemicmodeling_amd import _lib
    path = os.path.join(H.ROOT, "include", "epiekf.h")
    header = open(path).read()
    body = re.search(r"typedef struct epi_noise_desc \{(.*?)\} epi_noise_desc;", header, re.S).group(1)
    names = [n for decl in re.findall(r"\w+ [^;]*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) for n in re.findall(r"(\w+)\s*[,;]", decl)]
    assert names == [n for n, _ in _lib.NoiseDesc._fields_] == ["abi_version", "seed_lo", "seed_hi", "stream"]
    assert C.sizeof(_lib.NoiseDesc) == 16
    for sym in NEW_SYMBOLS:
        assert sym in _lib.ABI_SYMBOLS and hasattr(hip_lib, sym) and f"int {sym}(" in header, sym
    assert re.search(r"#define\s+EPIEKF_ABI_VERSION\s+6\b", header) and _lib.ABI_VERSION == 6
    # every structure the header had keeps its size; the only new one is epi_noise_desc
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler to measure the header's structures")
    structs = re.findall(r"typedef struct (epi_\w+) \{", header)
    src = '#include <stdio.h>\n#include "epiekf.h"\nint main(void) {\n' + "".join(
        '    printf("%s %%zu\\n", sizeof(%s));\n' % (n, n) for n in structs) + "    return 0;\n}\n"
    (tmp_path / "sizes.c").write_text(src)
    exe = str(tmp_path / "sizes")
    subprocess.run([cc, "-I" + os.path.dirname(path), str(tmp_path / "sizes.c"), "-o", exe], check=True, stdin=subprocess.DEVNULL)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, stdin=subprocess.DEVNULL).stdout
    sizes = {ln.split()[0]: int(ln.split()[1]) for ln in out.splitlines()}
    assert sizes == dict(OLD_SIZES, epi_noise_desc=16)
    mirror = {"epi_sim_desc": _lib.SimDesc, "epi_mc_desc": _lib.McDesc, "epi_arfc_desc": _lib.ArfcDesc, "epi_sdraw_desc": _lib.SdrawDesc,
              "epi_noise_desc": _lib.NoiseDesc}
    for n, t in mirror.items():
        assert C.sizeof(t) == sizes[n], n


def test_python_argument_checks(hip_lib):
    from epidemicmodeling_amd import _lib, hostapi
    assert _lib.noise_of(None, 0, None) is None
    d = _lib.noise_of(2 ** 40 + 3, 5, None)
    assert (d.seed_lo, d.seed_hi, d.stream, d.abi_version) == (3, 2 ** 8, 5, 6)
    with pytest.raises(ValueError, match="seed and z together"):
        _lib.noise_of(1, 0, np.zeros(3))
    with pytest.raises(ValueError, match="stream without seed"):
        _lib.noise_of(None, 1, None)
    with pytest.raises(ValueError, match="seed must lie in"):
        _lib.make_noise_desc(-1)
    T, B = 6, 4
    S, P, prm = np.zeros((T, 3, B)), np.zeros((T, 9, B)), np.zeros((61, B))
    with pytest.raises(ValueError, match="seed and z together"):
        hostapi.smoother_draws(S, P, S, P, prm, 2, z=np.zeros((T, 3, B * 2)), seed=1)
    with pytest.raises(ValueError, match="seed and z together"):
        hostapi.ar_forecast(np.zeros((20, 2)), np.zeros(2), np.zeros(2), np.zeros(2), 1.0, 3, 5, 3, z=np.zeros((5, 6)), seed=1)
    with pytest.raises(ValueError, match="seed and z together"):
        hostapi.random_npi_mc(np.zeros((48, 2)), np.zeros((2, 2)), 4, 5, z=np.zeros((5, 3, 8)), noise_seed=1)
    with pytest.raises(ValueError, match="rows must be 1 or 3"):
        hostapi.normal_draws(3, 2, 5, seed=1)
    with pytest.raises(ValueError, match="nt and lanes must be >= 1"):
        hostapi.normal_draws(0, 3, 5, seed=1)
    with pytest.raises(RuntimeError, match="stream must be below 2\\^30"):
        hostapi.normal_draws(3, 3, 5, seed=1, stream=2 ** 30)
    with pytest.raises(ValueError, match="dtype must be"):
        hostapi.normal_draws(3, 3, 5, seed=1, dtype=np.int32)

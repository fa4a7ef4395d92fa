"""The innovation whiteness diagnostics past 2^31 input elements, and the accuracy of the p-values on the device.

One run has 33 x (2^26 + 70) = 2.2e9 float32 innovations (8.9 GB; S = NULL, H = 2): element offsets beyond 2^31, a partial last
wavefront, one full and one partial block.  The series is generated on the device from a formula of (t, c), so the 256 sampled
chains -- the first and the last among them -- are rebuilt on the host and go through the restatement; every output word must
have left its poison.  The p-values: torch's gammaincc / gammainc on the device against scipy.stats.chi2 on the grid of
tests/test_innov_diag_ref.py, held to 50 x the worst relative error recorded in profiles/innov_diag/pvalues.json."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import innov_diag_ref as DR
from tests.test_gpu_innov_diag import FILL, GUARD, I32_FILL
from tests.test_innov_diag_ref import pvalue_errors

pytestmark = pytest.mark.gpu


def _series(t, c):
    """float32 innovation of day t, chain c: exact small integers over 8, so host and device agree to the bit; every 97th
    chain has a missing day 5, chain 3 an infinite day 20"""
    return (((c * 2654435761 + t * 40503 + (c >> 7) * t) % 257) - 128).astype(np.float32) / np.float32(8.0)


def test_more_than_2_31_input_elements(gpu_device, tmp_path_factory):
    import torch
    from epidemicmodeling_amd import _lib
    T, B, Hn = 33, 2 ** 26 + 70, 2
    assert T * B > 2 ** 31
    dev = torch.device(gpu_device)
    c = torch.arange(B, dtype=torch.int64, device=dev)
    e = torch.empty((T, B), dtype=torch.float32, device=dev)
    for t in range(T):
        e[t] = (((c * 2654435761 + t * 40503 + (c >> 7) * t) % 257) - 128).to(torch.float32) / 8.0
    e[5, ::97] = float("nan")
    e[20, 3] = float("inf")
    del c
    names = DR.ALL
    shapes = _lib.idiag_shapes(B, Hn)
    d = _lib.make_idiag_desc(B, T, Hn, 0, None, 0, 0, 1)
    ins = _lib.IdiagInputs()
    ins.e, ins.S = C.c_void_p(e.data_ptr()), None
    flat = {k: torch.full((int(np.prod(shapes[k])) + GUARD,), I32_FILL if k in DR.I32 else FILL,
                          dtype=torch.int32 if k in DR.I32 else torch.float64, device=dev) for k in names}
    outs = _lib.IdiagOutputs()
    for k in names:
        setattr(outs, k, C.c_void_p(flat[k].data_ptr()))
    err = C.create_string_buffer(256)
    n = C.c_size_t(0)
    _lib.check(_lib.lib().epi_idiag_workspace_bytes(C.byref(d), C.byref(n), err), err)
    ws = torch.full((n.value // 8 + GUARD,), FILL, dtype=torch.float64, device=dev)
    rc = _lib.lib().epi_idiag_run_device(C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(ws.data_ptr()), n.value,
                                         C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), err)
    _lib.check(rc, err)
    torch.cuda.synchronize(dev)
    assert bool((ws[n.value // 8:] == FILL).all()), "wrote behind the workspace"
    rng = np.random.default_rng(31)
    pick = np.unique(np.concatenate([[0, 3, 97, B - 71, B - 70, B - 1], rng.integers(0, B, 250)]))[:256]
    assert pick[0] == 0 and pick[-1] == B - 1
    host = np.stack([_series(np.int64(t), pick.astype(np.int64)) for t in range(T)]).astype(np.float64)
    host[5, pick % 97 == 0] = np.nan
    host[20, pick == 3] = np.inf
    idx = torch.as_tensor(pick, device=dev)
    assert DR.same_bits(e[:, idx].cpu().numpy().astype(np.float64), host)
    want = DR.InnovDiagRef(tmp_path_factory.mktemp("innov_diag_ref")).run(host, None, H=Hn)
    assert want["status"][1] == DR.BAD_DAY and want["n"][0] == T - 1 and want["n"][-1] == T
    for k in names:
        fill = I32_FILL if k in DR.I32 else FILL
        cnt = int(np.prod(shapes[k]))
        assert bool((flat[k][cnt:] == fill).all()), f"{k} wrote outside its elements"
        assert not bool((flat[k][:cnt] == fill).any()), f"{k} keeps poison"
        got = flat[k][:cnt].view(shapes[k])[..., idx].cpu().numpy()
        assert DR.same_bits(got, want[k]), k


def test_pvalues_on_the_device(gpu_device):
    recorded = json.load(open(os.path.join(H.ROOT, "profiles", "innov_diag", "pvalues.json")))
    err = pvalue_errors(gpu_device)
    print("worst relative errors on the device:", err)
    for k in ("lb_p", "nis_p"):
        assert recorded[k]["worst_relative_error"] <= 1e-6            # else the p-values would be computed on CPU tensors
        assert err[k] <= 50.0 * recorded[k]["worst_relative_error"], (k, err[k])

"""The direct optimal-NPI planner on the device (epi_plan_run_device / _host, batch.npi_plan, hostapi.npi_plan): every output
equals the C reading tests/npi_plan_ref.c of DESIGN.md §4.15 bit for bit -- any NaN equal to any NaN.  Every output starts as a
poison value and carries guard elements behind it; the workspace is poisoned too.  The shapes are the smallest that reach every
edge: the issue's grid (B = 32: chains of 1 to 16 iterations in one wavefront) at H = 1, 2, 30; B = 1, 65 = 5 x 13 and
257 = 1 x 257 (one lane; a region across the wavefront boundary; a region across four of them and a last wavefront of one lane)."""
import ctypes as C

import numpy as np
import pytest

from tests import npi_plan_ref as PR

pytestmark = pytest.mark.gpu

FILL, I32_FILL, GUARD = -98765.4321, -12345, 8


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return PR.PlanRef(tmp_path_factory.mktemp("npi_plan_ref"))


def _run_device(case, names=PR.ALL, device="cuda:0"):
    """epi_plan_run_device on poison-filled outputs with GUARD elements behind each and a poisoned workspace.  Returns (dict of
    NumPy arrays, dict name -> True if the guards still hold the poison)."""
    import torch
    from epidemicmodeling_amd import _lib
    dev = torch.device(device)
    up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
    tens = [up(case.get(k)) for k in _lib.PLAN_IN_NAMES]
    shapes = _lib.plan_shapes(case["R"], case["P"], case["H"], case["n"], case["max_iter"])
    d = _lib.make_plan_desc(case["R"], case["P"], case["H"], case["n"], case["prefix_days"], case["max_iter"], case["max_halvings"], case["tol"])
    ins = _lib.PlanInputs()
    for k, v in zip(_lib.PLAN_IN_NAMES, tens):
        setattr(ins, k, None if v is None else C.c_void_p(v.data_ptr()))
    flat = {k: torch.full((int(np.prod(shapes[k])) + GUARD,), I32_FILL if k in PR.I32 else FILL,
                          dtype=torch.int32 if k in PR.I32 else torch.float64, device=dev) for k in names}
    outs = _lib.PlanOutputs()
    for k in names:
        setattr(outs, k, C.c_void_p(flat[k].data_ptr()))
    err = C.create_string_buffer(256)
    n = C.c_size_t(0)
    _lib.check(_lib.lib().epi_plan_workspace_bytes(C.byref(d), C.byref(n), err), err)
    ws = torch.full((n.value // 8 + GUARD,), FILL, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev)
    rc = _lib.lib().epi_plan_run_device(C.byref(d), C.byref(ins), C.byref(outs), C.c_void_p(ws.data_ptr()), n.value,
                                        C.c_void_p(st.cuda_stream), err)
    _lib.check(rc, err)
    torch.cuda.synchronize(dev)
    res, clean = {}, {"workspace": bool((ws[n.value // 8:] == FILL).all())}
    for k in names:
        h = flat[k].cpu().numpy()
        cnt = int(np.prod(shapes[k]))
        clean[k] = bool((h[cnt:] == (I32_FILL if k in PR.I32 else FILL)).all())
        res[k] = h[:cnt].reshape(shapes[k])
    return res, clean


def _assert_equal(got, clean, want, what):
    assert clean["workspace"], f"{what}: wrote behind the workspace"
    for k, v in got.items():
        assert clean[k], f"{what}: {k} wrote outside its elements"
        assert PR.same_bits(v, want[k]), f"{what}: {k} differs from the C reading"
        assert not (v == (I32_FILL if k in PR.I32 else FILL)).any(), f"{what}: {k} keeps poison"


def _spread(P):
    """P cost weights from 1e-12 to 1 - 1e-12, dense near the small ones, where the iteration counts differ most"""
    return np.clip(np.linspace(0.0, 1.0, P) ** 4, 1e-12, 1.0 - 1e-12)


def _with_extras(case, seed):
    """held entries, a starting plan and a prefix on top of `case`"""
    rng = np.random.default_rng(seed)
    R, P, Hh, n = case["R"], case["P"], case["H"], case["n"]
    uf = np.full((Hh, n, R), np.nan)
    uf[rng.random(uf.shape) < 0.3] = 1.0
    return dict(case, u_fixed=uf, u_init=rng.integers(0, 3, (Hh, n, R * P)).astype(np.float64), J0_prefix=rng.random(R),
                J1_prefix=rng.random(R) * 100.0, prefix_days=40)


@pytest.mark.parametrize("horizon", PR.GRID_H)
def test_grid_bit_for_bit(gpu_device, ref, horizon):
    """the issue's grid: every output, then the optional ones absent; chains of 1 .. 16 iterations share the one wavefront"""
    case = PR.grid_case(horizon)
    want = ref.run(case)
    if horizon == 30:
        assert want["iters"].min() == 1 and want["iters"].max() == 16
    got, clean = _run_device(case)
    assert list(got) == list(PR.ALL)
    _assert_equal(got, clean, want, f"grid H={horizon}")
    got, clean = _run_device(case, PR.F64 + PR.I32)
    _assert_equal(got, clean, want, f"grid H={horizon}, optional outputs absent")
    got, clean = _run_device(case, PR.F64 + PR.I32 + ("mu",))
    _assert_equal(got, clean, want, f"grid H={horizon}, mu alone")


@pytest.mark.parametrize("R,P", [(1, 1), (5, 13), (1, 257)])
@pytest.mark.parametrize("horizon", PR.GRID_H)
def test_lane_wave_and_launch_boundaries(gpu_device, ref, R, P, horizon):
    regions = (150, 5, 20, 50, 100)[:R]
    case = dict(PR.region_case(regions, _spread(P) if P > 1 else (1e-3,), horizon), max_iter=20, max_halvings=8)
    want = ref.run(case)
    got, clean = _run_device(case)
    _assert_equal(got, clean, want, f"B={R * P} H={horizon}")
    if horizon == 30 and P > 1:
        assert len(set(want["iters"].tolist())) > 3         # mixed iteration counts in one wavefront


@pytest.mark.parametrize("n", [1, 11, 12])
def test_held_entries_start_plan_and_prefix(gpu_device, ref, n):
    case = _with_extras(dict(PR.region_case((5, 150, 100, 20, 50), _spread(13), 9, n=n), max_iter=12, max_halvings=6), n)
    want = ref.run(case)
    got, clean = _run_device(case)
    _assert_equal(got, clean, want, f"extras n={n}")
    held = np.repeat(~np.isnan(case["u_fixed"]), 13, axis=2)
    assert (got["plan"][held] == 1.0).all()
    got, clean = _run_device(case, PR.F64 + PR.I32 + ("F_trace",))
    _assert_equal(got, clean, want, f"extras n={n}, F_trace alone")


def test_cap_and_failed_search(gpu_device, ref):
    case = PR.region_case((150,), (1e-3,), 30)
    want = ref.run(case)
    assert want["status"][0] == 1
    got, clean = _run_device(case)
    _assert_equal(got, clean, want, "cap")
    rng = np.random.default_rng(11)
    case = dict(PR.grid_case(30), max_halvings=0, max_iter=40)
    case["u_init"] = np.where(rng.random((30, 12, 32)) < 0.5, 0.0, np.ones((30, 12, 32)) * 2.0)
    want = ref.run(case)
    assert (want["status"] & 2).any()
    got, clean = _run_device(case)
    _assert_equal(got, clean, want, "max_halvings = 0")


def test_python_entries_device_and_host_agree(gpu_device, ref):
    from epidemicmodeling_amd import batch, hostapi
    case = _with_extras(dict(PR.region_case((5, 150, 100, 20, 50), _spread(13), 9), max_iter=12, max_halvings=6), 3)
    want = ref.run(case)
    args = (case["sp"], case["u_min"], case["eps"], case["H"])
    kw = dict(u_fixed=case["u_fixed"], u_init=case["u_init"], J0_prefix=case["J0_prefix"], J1_prefix=case["J1_prefix"], prefix_days=40,
              max_iter=12, max_halvings=6, tol=case["tol"])
    dev = batch.npi_plan(*args, outputs=PR.OPTIONAL, device=gpu_device, **kw)
    host = hostapi.npi_plan(*args, outputs=PR.OPTIONAL, **kw)
    assert list(dev) == list(host) == list(PR.ALL)
    for k in PR.ALL:
        assert PR.same_bits(dev[k].cpu().numpy(), want[k]) and PR.same_bits(host[k], want[k]), k
    few = hostapi.npi_plan(*args, **kw)
    assert list(few) == list(PR.F64 + PR.I32) and all(PR.same_bits(few[k], want[k]) for k in few)

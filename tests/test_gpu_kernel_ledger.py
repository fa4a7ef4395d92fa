"""Every row of tests/kernel_ledger.py on the device: the call launches the kernel instances the row declares -- asked of the
launch plan with THIS device's SIMD count and the runner's own descriptor -- and every word those kernels write equals the C
oracle's.

Per row: the runner's descriptor equals the one tests/test_kernel_ledger.py planned, field by field; the plan on this device is the
declared one (the test fails with the numbers if the device has another SIMD count than the ledger assumes); outputs, workspace,
pinv_rank and status are poisoned; after the run no poison is left in any output; every selected output of EVERY chain, and
pinv_rank, equals the oracle bit for bit (fp32 storage: the oracle's value rounded once), and bit 0 of status is the oracle's
guard.  Sweep rows also hold (J0, J1), the front and I_opt against the separate scoring / Pareto calls on the same u_opt_smooth."""
import time

import numpy as np
import pytest

from tests import helpers as H
from tests import kernel_ledger as K
from tests import plan_probe as P
from tests.test_kernel_ledger import check_row

pytestmark = pytest.mark.gpu


def _need_bytes(w, names):
    from tests.test_gpu_addressing_limits import _need_bytes as need
    return need(w.B, w.T, w.m, w.n_npi, names, blocked_pad=1.05)


@pytest.mark.parametrize("rid", [r["id"] for r in K.LEDGER])
def test_row_runs_the_declared_kernels_and_equals_the_oracle(gpu_device, rid):
    import torch
    from epidemicmodeling_amd import batch
    row = K.BY_ID[rid]
    w = K.workload(row["workload"], row["flipped"])
    H.need_free(gpu_device, _need_bytes(w, row["runner"]["outputs"]))
    t0 = time.perf_counter()
    r = batch.EkfRunner(batch.DeviceWorkload(w, gpu_device), extras=True, **row["runner"])
    want, got = K.desc_fields(K.planned_desc(row, w)), K.desc_fields(r.desc)
    assert got == want, (rid, {k: (got[k], want[k]) for k in got if got[k] != want[k]})
    t_hist = row["t_hist"] if row["entry"] == "sweep" else None
    simds = 4 * torch.cuda.get_device_properties(gpu_device).multi_processor_count
    q = P.query(r.desc, simds, extras=True, t_hist=t_hist)
    bad = check_row(row, q)
    assert not bad, (rid, "the plan on this device (%d SIMDs, ledger: %d) is not the declared one" % (simds, K.S_LEDGER), w.B, w.T,
                     q["shape"], q["lw"], bad)
    H.poison_runner(r)
    t1 = time.perf_counter()
    if t_hist is None:
        r.run()
    else:
        from tests.test_gpu_npi_counts import _scoring_inputs
        sp, j0p, j1p = _scoring_inputs(w, np.random.default_rng(7))
        to = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(gpu_device)
        sp, j0p, j1p = to(sp), to(j0p), to(j1p)
        R = w.meta["regions"]
        sc = r.run_sweep(t_hist, sp, j0p, j1p, n_regions=R)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    left = H.surviving_poison(r)
    assert not left, (rid, "outputs that still hold the poison pattern (words)", left)
    stat = H.all_chains_equal_oracle(r, w, what=rid)
    assert stat["chains"] == w.B
    rank = r.unblocked("pinv_rank").cpu().numpy()              # (equal to the oracle's: compared just now)
    if not w.model.startswith("NewCase"):
        guard = H.oracle_guard_fired({"pinv_rank": rank}, w.model)
        assert np.array_equal((r.status.cpu().numpy() & 1).astype(bool), guard), (rid, "status bit 0 is not the oracle's guard")
        if row["guard"]:            # the dense second pass had a chain to run
            assert guard.any(), (rid, "no chain's guard fired: the second pass of exact_nonfinite had nothing to do")
    if t_hist is not None:
        J0, J1 = sc["J0"].clone(), sc["J1"].clone()
        sc2 = batch.score_sweep(r.out["u_opt_smooth"], t_hist, sp, j0p, j1p, B=w.B)
        assert torch.equal(J0, sc2["J0"]) and torch.equal(J1, sc2["J1"]), rid
        on2, io2 = batch.pareto_front(sc2["J0"], sc2["J1"], R)
        assert torch.equal(sc["on_front"].bool(), on2) and torch.equal(sc["i_opt"], io2), rid
    print("ledger row %s: %d chains x %d days; set-up %.2f s, call %.3f s, checks %.2f s"
          % (rid, w.B, w.T, t1 - t0, t2 - t1, time.perf_counter() - t2))

"""Every launchable kernel instance of the filter families is run by a named ledger row -- checked without a GPU.

(a) what the launch plan can launch (tests/plan_query.cpp's enumeration) plus NEVER_LAUNCHED is exactly what a host-only compile of
    csrc/epiekf.hip lists as kernels of these families: an instantiation added to a ladder, or a ladder the query no longer
    restates, fails here;
(b) NEVER_LAUNCHED is the six LDS-constant variants of the 3-state forward kernel and nothing else;
(c) every row of tests/kernel_ledger.py launches the instances and takes the schedule it declares, on S_LEDGER SIMDs;
(d) the rows together reach every launchable instance and every schedule bit, and none has gone missing."""
import collections
import os
import re
import shutil
import subprocess

import pytest

from tests import helpers as H
from tests import kernel_ledger as K
from tests import plan_probe as P

SRC = os.path.join(H.ROOT, "epidemicmodeling_amd", "csrc", "epiekf.hip")

# rows per group (the id up to its first "/"): a row that leaves the ledger is noticed even where another still reaches its kernels
ROWS_PER_GROUP = {"sia6": 44, "f32": 12, "sia3": 20, "newcase": 7, "lp": 9, "hex2": 6, "quad2": 4, "row3": 20, "sweep": 2}


@pytest.fixture(scope="module")
def query():
    try:
        P.lib()
    except RuntimeError as e:
        pytest.fail(str(e))
    return P.query


@pytest.fixture(scope="module")
def launchable(query):
    names, plans = P.enumerate_instances(K.S_LEDGER)
    assert plans > 10 ** 7, plans
    return names


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """The kernels of the filter families among the host stubs of a host-only compile (no device code is generated)."""
    from epidemicmodeling_amd import _build
    try:
        hipcc = _build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    nm = shutil.which("nm")
    if not nm:
        pytest.fail("no nm to list the kernels' host stubs")
    obj = str(tmp_path_factory.mktemp("host_only") / "epiekf_host.o")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "--cuda-host-only", "-c", SRC, "-o", obj], check=True,
                   stdin=subprocess.DEVNULL, capture_output=True, timeout=600)
    out = subprocess.run([nm, "-C", obj], check=True, capture_output=True, text=True, stdin=subprocess.DEVNULL).stdout
    stubs = [re.sub(r"\(.*", "", m.group(1)) for m in re.finditer(r"__device_stub__(.*)", out)]
    assert len(stubs) == len(set(stubs)) and len(stubs) > 200, len(stubs)
    return sorted(s for s in stubs if s.startswith(K.FAMILIES))


def test_launchable_plus_never_launched_is_what_is_compiled(launchable, compiled):
    assert not set(launchable) & set(K.NEVER_LAUNCHED)
    got, want = sorted(launchable + K.NEVER_LAUNCHED), compiled
    assert got == want, {"compiled, but no plan launches it and NEVER_LAUNCHED does not list it": sorted(set(want) - set(got)),
                         "a plan launches it, but it is not compiled": sorted(set(got) - set(want))}
    assert len(compiled) == 111 and len([n for n in compiled if not n.startswith("eks_pinv")]) == 107


def test_never_launched_is_the_six_lds_constant_variants_of_the_3_state_kernel():
    want = ["ekf_fwd_sym<3, 0, 1, 0, 0, 0>", "ekf_fwd_sym<3, 0, 1, 0, 0, 1>", "ekf_fwd_sym<3, 0, 1, 0, 1, 0>",
            "ekf_fwd_sym<3, 1, 1, 0, 0, 0>", "ekf_fwd_sym<3, 1, 1, 0, 0, 1>", "ekf_fwd_sym<3, 1, 1, 0, 1, 0>"]
    assert sorted(K.NEVER_LAUNCHED) == want


def check_row(row, q):
    """A row's declarations against a plan query's answer `q`; returns the list of what differs."""
    bad = []
    if sorted(q["names"]) != row["names"]:
        bad.append(("instances", sorted(q["names"]), "declared", row["names"]))
    if sorted(q["second"]) != row["second"]:
        bad.append(("second pass", sorted(q["second"]), "declared", row["second"]))
    if q["schedule"] != P.sched_bits(row["schedule"]):
        bad.append(("schedule", P.sched_names(q["schedule"]), "declared", row["schedule"] or "serial"))
    if row["bwd_order"] is not None and [n for r, n in q["launches"] if r == "bwd"] != row["bwd_order"]:
        bad.append(("smoother launches", [n for r, n in q["launches"] if r == "bwd"], "declared", row["bwd_order"]))
    if row["fwd_lds"] is not None and q["fwd_lds"] != row["fwd_lds"]:
        bad.append(("forward kernel's LDS bytes", q["fwd_lds"], "declared", row["fwd_lds"]))
    return bad


@pytest.mark.parametrize("rid", [r["id"] for r in K.LEDGER])
def test_row_launches_what_it_declares(query, rid):
    row = K.BY_ID[rid]
    d = K.planned_desc(row)
    q = query(d, K.S_LEDGER, extras=True, t_hist=row["t_hist"] if row["entry"] == "sweep" else None)
    bad = check_row(row, q)
    assert not bad, (rid, K.desc_fields(d), q["shape"], q["lw"], bad)


def test_sizes_of_the_rows_beyond_a_threshold_are_the_smallest_the_makers_give():
    S = K.S_LEDGER
    for wl, per_simd, n_eps in (("lp", 64, 16), ("lp-row3", 64, 16), ("lp-sweep", 64, 40), ("hex2", 10, 121), ("quad2", 16, 125)):
        B = K.workload(wl, False).B
        assert per_simd * S < B <= per_simd * S + n_eps and B % n_eps == 0, (wl, B)
    assert K.workload("lp", False).B == 65552 and K.workload("lp", False).T == 6 and K.workload("lp-sweep", False).T == 8
    # ragged last blocks / last waves on every layout the rows put these batches on
    assert K.workload("lp", False).B % 40 and K.workload("hex2", False).B % 10 and K.workload("quad2", False).B % 16
    # free controls over the horizon, so the bang-bang substitution runs
    import numpy as np
    for wl in ("lp", "lp-row3", "lp-sweep", "hex2", "quad2"):
        assert np.isnan(K.workload(wl, False).u[-2:]).all(), wl


def test_rows_reach_every_launchable_instance_and_schedule_bit(launchable):
    reached, bits = set(), {False: 0, True: 0}
    for r in K.LEDGER:
        reached |= set(r["names"])
        if r["guard"]:                       # the second pass has a marked chain to run
            reached |= set(r["second"])
        bits[r["flipped"]] |= P.sched_bits(r["schedule"])
    assert reached == set(launchable), {"launchable, in no row": sorted(set(launchable) - reached),
                                        "declared, not launchable": sorted(reached - set(launchable))}
    every = sum(P.SCHED.values())
    assert bits[False] == every, ("forward-model rows miss", P.sched_names(every & ~bits[False]))
    # the scoring tail belongs to the sweep entry, which runs the forward model only
    assert bits[True] == every & ~P.SCHED["BWD_HORIZON"], ("flipped-model rows miss", P.sched_names(every & ~bits[True]))
    # instances only a row beyond a SIMD-count threshold reaches are reached for both models
    for r in K.LEDGER:
        if r["flipped"] or r["entry"] == "sweep" or r["workload"] in ("cfg3-23", "cfg5-40", "row4", "row4-codegen", "row4-L5"):
            continue
        twin = r["id"].rsplit("/", 1)[0] + "/flipped"
        assert twin in K.BY_ID, (r["id"], "has no flipped-model row")
    per_group = collections.Counter(r["id"].split("/")[0] for r in K.LEDGER)
    assert dict(per_group) == ROWS_PER_GROUP, dict(per_group)
    # every row of SIA6_LAUNCHES is in, for both models
    from tests.test_gpu_npi_counts import SIA6_LAUNCHES
    for name, _, _ in SIA6_LAUNCHES:
        assert "sia6/%s/forward" % name in K.BY_ID and "sia6/%s/flipped" % name in K.BY_ID, name


def test_documents_quote_the_ledger():
    """The 'which test runs which kernel' paragraph of DESIGN.md 2 and the README's line are generated from the ledger."""
    design = open(os.path.join(H.ROOT, "DESIGN.md")).read()
    for line in K.coverage_table():
        assert line in design, line
    readme = open(os.path.join(H.ROOT, "README.md")).read()
    assert K.readme_line() in readme, K.readme_line()

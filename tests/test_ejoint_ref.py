"""The definition of the joint scores (include/epiekf.h) without a GPU: the NumPy restatement tests/ejoint_ref.py
and the sequential C restatement tests/ejoint_ref.c give the same bits; both agree with the energy score and the variogram score
computed another way (a broadcast NumPy double sum added with math.fsum) within the rounding of their sequential sums; and the
call tells joint draws from draws shuffled day by day, which ensemble_score cannot."""
import math

import numpy as np
import pytest

from tests import ejoint_ref as J
from tests import escore_ref as S

VS_CASES = ((1, 0), (1, 1), (1, 5), (2, 0), (2, 1), (2, 5))
# |es - brute| <= BOUND * truth_term: the sequential sums hold at most 45 000 terms at D = 300, whose n eps bound is 5e-12
BOUND = 1e-11


@pytest.fixture(scope="module")
def cref(tmp_path_factory):
    return J.EjointC(tmp_path_factory.mktemp("ejoint_ref"))


@pytest.mark.parametrize("W", J.CASE_W)
@pytest.mark.parametrize("D", J.CASE_D)
def test_restatements_agree(cref, D, W):
    for dtype in (np.float64, np.float32):
        for variant in (0, 1):
            c = J.case(D, W, dtype, variant)
            for k, (vs_order, max_lag) in enumerate(VS_CASES):
                want = J.joint(vs_order=vs_order, max_lag=max_lag, parts=("es", "vs") if k == 0 else ("vs",), **c)
                got = cref.joint(vs_order=vs_order, max_lag=max_lag, **c)
                for name in J.NAMES if k == 0 else ("vs", "n_members", "n_days", "truth_term", "member_dist"):
                    assert J.same_bits(got[name], want[name]), (name, dtype, variant, vs_order, max_lag)
            # what the case is there for: an undefined region of each kind, a defined one with a member absent
            assert (want["n_members"][:, 1] == 0).all() if variant == 0 else (want["n_days"][:, 1] == 0).all()
            assert (want["n_days"][:, 2] == 0).all() if variant == 0 else (want["n_days"][:, 2] == W).all()
            assert np.isnan(want["vs"][want["n_days"] == 0]).all() and np.isnan(want["member_dist"][:, D:2 * D]).all()
            if W > 1 and D > 1:
                assert want["n_members"][1, 0] == D - 1 and want["n_members"][0, 0] == D and want["n_members"][3, 0] == D - 1


@pytest.mark.parametrize("D", J.BIG_D)
def test_restatements_agree_at_16_32_and_64_registers(cref, D):
    """one D of each of NV = 16, 32, 64 (1 000: the workload's instantiation; 4 096: 64 blocks, 2 080 tiles), W = 2, both storages,
    the grid's case with its absent members in the last and in middle blocks.  NumPy takes about a second an item at 4 096."""
    assert {J.nv_of(d) for d in J.BIG_D} == {16, 32, 64}
    for dtype in (np.float64, np.float32):
        c = J.grid_case(D, 2, dtype, 1)
        for k, (vs_order, max_lag) in enumerate(((1, 0), (2, 5))):
            want = J.joint(vs_order=vs_order, max_lag=max_lag, parts=("es", "vs") if k == 0 else ("vs",), **c)
            got = cref.joint(vs_order=vs_order, max_lag=max_lag, **c)
            for name in J.NAMES if k == 0 else ("vs", "n_members", "n_days", "truth_term", "member_dist"):
                assert J.same_bits(got[name], want[name]), (name, dtype, vs_order, max_lag)
        assert want["n_members"][1, 0] == D - 3 and want["n_members"][0, 2] == D - 2 and (want["n_days"][:, 2] == 2).all()


def test_the_gpu_grid_reaches_every_instantiation():
    """What tests/test_gpu_ejoint.py's member-count grid (GRID_D of tests/test_gpu_ens_summary.py x both storages, every case
    asking for member_dist, es and vs) covers of ejoint_launch's dispatch (D <= 64: ejoint_members<1, S> and ejoint_vario<1, S>,
    <= 128: <2, S>, .. <= 2048: <32, S>, else <64, S>): all seven NV, each on its edge and one past the edge below it, so 7 x 2
    storages x 2 kernels = 28 instantiations; and ejoint_pairs at every block count its tile walk and mask reads differ at.  Thinning
    the grid fails here, without a device."""
    from tests.test_gpu_ens_summary import GRID_D
    assert {J.nv_of(D) for D in GRID_D} == {1, 2, 4, 8, 16, 32, 64}
    for edge in (64, 128, 256, 512, 1024, 2048):
        assert edge in GRID_D and edge + 1 in GRID_D and J.nv_of(edge + 1) == 2 * J.nv_of(edge), edge
    assert 1 in GRID_D and 4096 in GRID_D                                # validate's ends: 1 .. kEnsMaxD
    assert {1, 2, 3, 5, 16, 17, 33, 64} <= {J.nb_of(D) for D in GRID_D}  # 1, 3, 6, 15, 136, 153, 561, 2 080 tiles
    for n in (2, 8, 16, 32, 64):
        assert any(J.nv_of(D) == n and D % 64 for D in GRID_D), n        # with a partly filled last block
    for D in GRID_D:                                                     # the absent members: inside the item, the last block and,
        blocks = {e // 64 for _, _, e in J.grid_absent(D)}               # from three blocks on, one strictly between
        assert all(0 <= e < D for _, _, e in J.grid_absent(D)) and (D <= 64 or J.nb_of(D) - 1 in blocks and 0 not in blocks)
        assert J.nb_of(D) < 3 or len(blocks) == 3 or J.nb_of(D) == 3 and len(blocks) == 2
        assert D // 2 not in {e for _, _, e in J.grid_absent(D)}         # case()'s own absent member is another one


def brute(x, y, days, vs_order, max_lag):
    """x [W, n] the present members, y [W]: es, truth_term and vs by broadcast double sums added with math.fsum"""
    n = x.shape[1]
    tt = math.fsum(np.sqrt(((x - y[:, None]) ** 2).sum(axis=0))) / n
    dist = np.sqrt(((x[:, :, None] - x[:, None, :]) ** 2).sum(axis=0))
    es = tt - math.fsum(dist.reshape(-1)) / (2.0 * n * n)
    p = 0.5 if vs_order == 1 else 1.0
    terms = []
    for s in range(len(y)):
        for t in range(s + 1, len(y)):
            if max_lag == 0 or days[t] - days[s] <= max_lag:
                terms.append((abs(y[s] - y[t]) ** p - math.fsum(np.abs(x[s] - x[t]) ** p) / n) ** 2)
    return es, tt, math.fsum(terms)


@pytest.mark.parametrize("D", J.CASE_D)
def test_against_the_definition_computed_another_way(cref, D):
    for W in (2, 33):
        c = J.case(D, W, np.float64, 1)
        for vs_order, max_lag in ((1, 0), (2, 5)):
            got = cref.joint(vs_order=vs_order, max_lag=max_lag, **c)
            s = np.concatenate([c["src"], S.E.derived_row(c["src"], c["population"], c["R"], D)[:, None, :]], axis=1)
            checked = 0
            for row in range(4):
                for r in range(3):
                    if got["n_members"][row, r] == 0 or got["n_days"][row, r] == 0:
                        continue
                    ts = c["truth_series"][r]
                    days = [t for t in range(max(c["k0"], c["first_day"][r]), c["k1"]) if not np.isnan(c["truth"][t, row, ts])]
                    x = s[days, row, r * D:(r + 1) * D]
                    x = x[:, ~np.isnan(x).any(axis=0)]
                    es, tt, vs = brute(x, c["truth"][days, row, ts], days, vs_order, max_lag)
                    assert abs(got["es"][row, r] - es) <= BOUND * got["truth_term"][row, r], (row, r, got["es"][row, r], es)
                    assert abs(got["truth_term"][row, r] - tt) <= BOUND * tt
                    assert abs(got["vs"][row, r] - vs) <= BOUND * vs, (row, r, got["vs"][row, r], vs)
                    checked += 1
            assert checked >= 4


@pytest.mark.parametrize("D", J.CASE_D)
def test_one_day_is_the_crps(cref, D):
    c = J.case(D, 1, np.float64, 1)
    got = cref.joint(**c)
    sc = S.score(c["src"], c["truth"], 3, D, (), 0, population=c["population"], truth_series=c["truth_series"])
    checked = 0
    for row in range(3):                                                # the stored rows: values of order 1, as in that file's own check
        for r in range(3):
            if got["n_days"][row, r] == 1 and got["n_members"][row, r] > 0:
                t = [t for t in range(max(c["k0"], c["first_day"][r]), c["k1"]) if not np.isnan(c["truth"][t, row, c["truth_series"][r]])][0]
                # the members of the item are those of that one day, so the two calls score the same ensemble
                assert abs(got["es"][row, r] - sc["crps"][t, row, r]) <= 1e-12, (row, r)
                checked += 1
    assert checked >= 2


def test_one_member(cref):
    rng = np.random.default_rng(5)
    T, R = 7, 3
    src, truth = rng.standard_normal((T, 1, R)), rng.standard_normal((T, 1, R))
    for ref in (cref.joint, J.joint):
        got = ref(src, truth, R, 1, vs_order=2)
        for r in range(R):
            assert got["es"][0, r] == got["member_dist"][0, r] == got["truth_term"][0, r] and got["spread_term"][0, r] == 0.0
            assert got["n_members"][0, r] == 1 and got["n_days"][0, r] == T


def test_joint_draws_are_told_from_draws_shuffled_day_by_day(cref):
    """The property the call exists for: D = 64 paths constant in time against a constant truth, and a copy whose members are
    shuffled independently on every day.  ensemble_score gives every day the same bits for both (the marginals are the same);
    the variogram score is exactly 0.0 for the paths and positive for the shuffled copy, and the energy scores differ."""
    rng = np.random.default_rng(64)
    T, D = 12, 64
    c = rng.standard_normal(D)
    paths = np.repeat(c[None, None, :], T, axis=0)                       # [T, 1, D]
    shuffled = np.stack([rng.permutation(c) for _ in range(T)])[:, None, :]
    truth = np.full((T, 1, 1), 0.3)
    a, b = S.score(paths, truth, 1, D), S.score(shuffled, truth, 1, D)
    for k in ("crps", "wis", "ae", "rank", "ties", "cover", "count", "crps_mean", "wis_mean"):
        assert S.same_bits(a[k], b[k]), k
    for ref in (cref.joint, J.joint):
        for vs_order in (1, 2):
            ja, jb = ref(paths, truth, 1, D, vs_order=vs_order), ref(shuffled, truth, 1, D, vs_order=vs_order)
            assert ja["vs"][0, 0] == 0.0 and jb["vs"][0, 0] > 0.0
            assert ja["es"][0, 0] != jb["es"][0, 0]
            assert ja["n_members"][0, 0] == jb["n_members"][0, 0] == D and ja["n_days"][0, 0] == jb["n_days"][0, 0] == T


@pytest.mark.parametrize("D", (2, 65, 130))
def test_permuting_whole_members_moves_the_scores_only_within_the_bound(cref, D):
    """Unlike ensemble_score (§4.17), whose outputs are functions of each day's sorted members and so bit-invariant, es and vs
    are NOT bit-invariant under a permutation of the members: the tree and the tiles run over draws in the order given.  The
    same permutation on every day leaves n_members and n_days unchanged and moves es and vs only within the rounding bound."""
    c = J.case(D, 33, np.float64, 1)
    perm = np.random.default_rng(D).permutation(D)
    idx = np.concatenate([r * D + perm for r in range(3)])
    p = dict(c, src=np.ascontiguousarray(c["src"][:, :, idx]))
    a, b = cref.joint(vs_order=1, **c), cref.joint(vs_order=1, **p)
    assert np.array_equal(a["n_members"], b["n_members"]) and np.array_equal(a["n_days"], b["n_days"])
    on = (a["n_members"] > 0) & (a["n_days"] > 0)
    assert on.sum() >= 4
    assert (np.abs(a["es"][on] - b["es"][on]) <= BOUND * a["truth_term"][on]).all()
    assert (np.abs(a["vs"][on] - b["vs"][on]) <= BOUND * a["vs"][on]).all()
    md = a["member_dist"].reshape(4, 3, D)[:, :, perm].reshape(4, 3 * D)
    assert J.same_bits(md, b["member_dist"])                            # a member's own distance does not depend on its place

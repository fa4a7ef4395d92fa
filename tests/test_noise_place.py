"""Placing a chosen uniform under the seeded normal draws, without a GPU (tests/noise_place.py, DESIGN.md §4.21 "Where chance never
goes"): the inverse of Philox4x32-10 round-trips the Random123 known answers and random blocks through both restatements; every
placement of every target lies in the domain of epi_noise_fill_device, its window fits, and its forward uniform IS the target;
the target list holds both sides of the four branch boundaries and at least 40 far-tail points; every recorded far-tail seed
(tests/golden/noise_far_tail_seeds.json) is far-tail under both restatements, and the search tool (tests/noise_seed_search.c),
run over a small seed range that holds a recorded seed, reports it."""
from fractions import Fraction

import numpy as np
import pytest

from tests import noise_place as NP
from tests import noise_ref as NR

SEED = 0x13198A2E03707344


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return NR.NoiseRef(tmp_path_factory.mktemp("noise_ref"))


@pytest.fixture(scope="module")
def search(tmp_path_factory):
    return NP.SeedSearch(tmp_path_factory.mktemp("noise_seed_search"))


def test_inverse_round_trips(ref):
    kat = [([0] * 4, [0] * 2, [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, words in kat:
        assert list(NP.inv_philox(words, *key)) == ctr
    rng = np.random.default_rng(1)
    for _ in range(200):
        words = [int(v) for v in rng.integers(0, 2 ** 32, 4)]
        key = [int(v) for v in rng.integers(0, 2 ** 32, 2)]
        ctr = NP.inv_philox(words, *key)
        assert ref.philox(ctr, key) == words
        assert [int(v[0]) for v in NR.philox(*[[c] for c in ctr], *key)] == words
        assert list(NP.inv_philox(ref.philox(words, key), *key)) == words           # and the other way round


def _placements():
    rng = np.random.default_rng([SEED & 0xFFFFFFFF, SEED >> 32])
    for n in NP.targets():
        for slot in (0, 1):
            yield n, slot, False, NP.place(SEED, n, slot, rng)
        yield n, 0, True, NP.place(SEED, n, 0, rng, row0_only=True)


def test_placements_lie_in_the_domain_and_give_the_target(ref):
    rows_seen = set()
    for n, slot, row0, (stream, t, row, lane) in _placements():
        assert 0 <= stream < 2 ** 30 and 0 <= t < 2 ** 32 and 0 <= lane < 2 ** 63 and row in (0, 1, 2) and row & 1 == slot, (n, slot)
        assert row == 0 or not row0
        t0, lane0 = NP.window(t, lane)
        assert 0 <= t0 <= t < t0 + 3 <= 2 ** 32 and 0 <= lane0 <= lane < lane0 + 5 <= 2 ** 63, (n, slot)
        w = ref.philox([lane & 0xFFFFFFFF, lane >> 32, t, 0x80000000 | (stream << 1) | (row >> 1)], [SEED & 0xFFFFFFFF, SEED >> 32])
        assert ref.uniform(w[2 * slot], w[2 * slot + 1]) == NP.u_of(n), (n, slot)
        z = ref.fill(SEED, stream, t, 1, 3, lane, 1)[0, row, 0]                     # and through the restated fill
        assert z == ref.icdf([NP.u_of(n)])[0] == NR.fill(SEED, stream, t, 1, 3, lane, 1)[0, row, 0], (n, slot)
        rows_seen.add(row)
    assert rows_seen == {0, 1, 2}
    # deterministic for a given generator
    a = [p for *_, p in _placements()]
    assert a == [p for *_, p in _placements()]


def test_window_clips_to_the_domain():
    assert NP.window(0, 0) == (0, 0) and NP.window(2 ** 32 - 1, 2 ** 63 - 1) == (2 ** 32 - 3, 2 ** 63 - 5)
    assert NP.window(7, 9) == (6, 7)


def test_targets_hold_both_sides_of_every_boundary(ref):
    tg = NP.targets()
    assert len(tg) == len(set(tg)) and all(0 <= n <= NP.TOP for n in tg)
    for n in (0, 1, NP.TOP - 1, NP.TOP, 2 ** 51 - 1, 2 ** 51, *[2 ** k for k in range(52)]):
        assert n in tg
    assert NP.u_of(2 ** 51 - 1) < 0.5 < NP.u_of(2 ** 51) and NP.u_of(0) == 2.0 ** -53 and NP.u_of(NP.TOP) == 1.0 - 2.0 ** -53
    kind = {n: NP.classify(NP.u_of(n)) for n in tg}
    for v, (a, b) in zip(NP.boundaries(), (("near", "central"), ("central", "near"), ("far", "near"), ("near", "far"))):
        i = NP.boundary_index(v)
        ks = [kind[i + d] for d in (-1, 0, 1, 2)]
        print(v, i, ks)
        assert all(i + d in tg for d in (-1, 0, 1, 2))
        assert ks[0] == a and ks[-1] == b and set(ks) == {a, b}, (v, ks)              # a neighbour on either side
        assert NP.u_of(i) <= v < NP.u_of(i + 1)                                       # and the boundary between two of them
        # no lattice point sits ON |u - 1/2| = 0.425 (u - 1/2 is exact here), so `<=` against `<` cannot be told apart at one
        # point: the neighbours either side are what pins the boundary
        assert all(abs(Fraction(NP.u_of(i + d)) - Fraction(1, 2)) != Fraction(0.425) for d in (-1, 0, 1, 2))
    far = [n for n in tg if kind[n] == "far"]
    assert len(far) >= 40, len(far)
    # the far tail is n <= FAR_N or TOP - n <= FAR_N: what the search tool tests
    i = NP.boundary_index(NP.boundaries()[2])
    assert NP.FAR_N == i and kind[i] == "far" and kind[i + 1] == "near"
    j = NP.boundary_index(NP.boundaries()[3])
    assert kind[NP.TOP - NP.FAR_N] == "far" and NP.classify(NP.u_of(NP.TOP - NP.FAR_N - 1)) == "near" and j in (NP.TOP - NP.FAR_N - 1, NP.TOP - NP.FAR_N)
    # the restatements agree on every target, and the promise |z| < 8.2096 holds at the extremes
    u = np.array([NP.u_of(n) for n in tg])
    z = ref.icdf(u)
    assert NR.same_bits(z, NR.icdf(u)) and np.abs(z).max() < 8.2096 and z[tg.index(0)] == -z[tg.index(NP.TOP)]


def test_recorded_seeds_are_far_tail(ref):
    boxes = NP.recorded_seeds()
    assert set(boxes) == {"rows3", "row0"}
    for box, entries in boxes.items():
        assert {e["tail"] for e in entries} == {"lower", "upper"}, box
        for e in entries:
            assert e["stream"] == 0 and 0 <= e["t"] < NP.BOX_T and 0 <= e["lane"] < NP.BOX_LANES and e["row"] in ((0,) if box == "row0" else (0, 1, 2))
            u = NP.u_of(e["n"])
            assert NP.classify(u) == "far" and (u < 0.5) == (e["tail"] == "lower")
            rows = 1 if box == "row0" else 3
            for fill in (ref.fill, NR.fill):
                z = fill(e["seed"], 0, e["t"], 1, rows, e["lane"], 1)[0, e["row"], 0]
                assert z == ref.icdf([u])[0] and 5.0 < abs(z) < 8.2096 and (z < 0) == (e["tail"] == "lower"), (box, e)


@pytest.mark.parametrize("box", ["rows3", "row0"])
def test_search_tool_reports_a_recorded_seed(search, box):
    e = NP.recorded(box, "lower")
    hits = search.run(e["seed"] - 1000, 2000, 3 if box == "rows3" else 1, threads=2)
    assert e in hits, hits
    for h in hits:                                                                    # whatever else it reports is far-tail too
        assert NP.classify(NP.u_of(h["n"])) == "far"

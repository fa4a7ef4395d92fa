"""Putting a CHOSEN uniform under the seeded normal draws ("Where chance never goes").

Philox4x32-10 is a bijection of the counter for a fixed key and its rounds invert in closed form (the multipliers are odd, so
they have inverses mod 2^32; the key schedule is walked backwards).  So the output words -- and with them the lattice index n of
u = (n + 0.5) 2^-52 -- are chosen and the counter (lane, t, stream, row pair) that produces them is computed: `place`.  A fill
window of epi_noise_fill_device takes any t0 and lane0, so it can be put on that counter; the far-tail branch of the inverse
CDF (2.8e-11 per draw), both branch boundaries and the two extreme uniforms are then reached in a handful of lanes.

A consumer kernel starts its lanes and days at 0 and the key is not invertible, so a far-tail draw INSIDE a consumer is found
by walking seeds (tests/noise_seed_search.c, `SeedSearch`); tests/golden/noise_far_tail_seeds.json holds what the search found
(`recorded_seeds`).  No code is shared with csrc/noise.hpp."""
import json
import math
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEARCH_SRC = os.path.join(HERE, "noise_seed_search.c")
SEEDS_JSON = os.path.join(HERE, "golden", "noise_far_tail_seeds.json")

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
M0_INV, M1_INV = pow(M0, -1, 2 ** 32), pow(M1, -1, 2 ** 32)
MASK = 0xFFFFFFFF
TOP = 2 ** 52 - 1                                     # the largest lattice index
FAR_N = math.floor(math.exp(-25.0) * 2 ** 52 - 0.5)   # n <= FAR_N or TOP - n <= FAR_N: the far tail (test_noise_place.py checks it)
BOX_T, BOX_LANES = 3, 64                              # the box of the seed search: t < 3, lane < 64, stream 0


def inv_philox(words, k0, k1):
    """the counter (c0, c1, c2, c3) whose Philox4x32-10 block under the key (k0, k1) is `words`"""
    n0, n1, n2, n3 = (int(w) & MASK for w in words)
    for r in range(9, -1, -1):
        ka, kb = (int(k0) + r * W0) & MASK, (int(k1) + r * W1) & MASK
        c0, c2 = (n3 * M0_INV) & MASK, (n1 * M1_INV) & MASK
        c1 = n0 ^ ((M1 * c2) >> 32) ^ ka
        c3 = n2 ^ ((M0 * c0) >> 32) ^ kb
        n0, n1, n2, n3 = c0, c1, c2, c3
    return n0, n1, n2, n3


def place(seed, n, slot, rng, row0_only=False, max_trials=10000):
    """(stream, t, row, lane) at which the draw of `seed` has the lattice index n: u = (n + 0.5) 2^-52.  slot 0 / 1: the uniform of
    the output words (0, 1) / (2, 3), row = 2 q + slot with q the row pair the counter turns out to have; slot 1 only with q = 0
    (rows <= 3).  row0_only: q = 0 and slot 0, for windows of one row.  The six dropped low bits of the two words and the other
    two words come from rng (a numpy Generator), so the result is a function of the arguments and the generator's state."""
    seed, n = int(seed), int(n)
    assert 0 <= n <= TOP and slot in (0, 1) and not (row0_only and slot)
    for _ in range(max_trials):
        low = [int(v) for v in rng.integers(0, 64, 2)]
        other = [int(v) for v in rng.integers(0, 2 ** 32, 2)]
        pair = [((n >> 26) << 6) | low[0], ((n & (2 ** 26 - 1)) << 6) | low[1]]
        c0, c1, c2, c3 = inv_philox(pair + other if slot == 0 else other + pair, seed & MASK, seed >> 32)
        q = c3 & 1
        if not (c3 >> 31) or (c1 >> 31) or (q and (slot or row0_only)):
            continue
        return (c3 & 0x7FFFFFFF) >> 1, c2, 2 * q + slot, c0 | (c1 << 32)
    raise RuntimeError("no placement in %d trials" % max_trials)


def window(t, lane, nt=3, n_lanes=5):
    """(t0, lane0) of an nt x n_lanes fill window with (t, lane) inside it -- in the middle unless the domain (t < 2^32, lane <
    2^63) clips it"""
    return min(max(t - nt // 2, 0), 2 ** 32 - nt), min(max(lane - n_lanes // 2, 0), 2 ** 63 - n_lanes)


def targets():
    """the lattice indices the fill kernel is run at: the extremes and their neighbours, the two u next to 1/2 (where the sign of
    q = u - 1/2 flips), every power of two, and for each branch boundary v (|u - 1/2| = 0.425, min(u, 1 - u) = e^-25) the index
    floor(v 2^52 - 0.5) with the offsets -1 .. +2.  That list holds 24 far-tail points, all but five of them in the lower tail; the
    mirror images TOP - 2^k and the all-ones patterns 2^k - 1 bring the far tail to 53 points, both tails alike"""
    out = [0, 1, TOP - 1, TOP, 2 ** 51 - 1, 2 ** 51] + [2 ** k for k in range(52)]
    out += [TOP - 2 ** k for k in range(52)] + [2 ** k - 1 for k in range(1, 53)]
    for v in boundaries():
        out += [boundary_index(v) + d for d in (-1, 0, 1, 2)]
    seen, uniq = set(), []
    for n in out:
        if n not in seen:
            seen.add(n)
            uniq.append(n)
    return uniq


def boundaries():
    return (0.075, 0.925, math.exp(-25.0), 1.0 - math.exp(-25.0))


def boundary_index(v):
    # v 2^52 is exact in double (a power-of-two scaling); the subtraction is done on exact rationals
    from fractions import Fraction
    return math.floor(Fraction(v) * 2 ** 52 - Fraction(1, 2))


def u_of(n):
    """u = (n + 0.5) 2^-52, exact"""
    return (2 * int(n) + 1) * 2.0 ** -53


def classify(u):
    """'central' / 'near' / 'far' by the NumPy restatement's own rt"""
    from tests import noise_ref as NR
    u = float(u)
    q = u - 0.5
    if abs(q) <= 0.425:
        return "central"
    rt = float(np.sqrt(-NR.epi_log(np.float64(u if q < 0.0 else 1.0 - u))))
    return "near" if rt <= 5.0 else "far"


def recorded_seeds():
    """tests/golden/noise_far_tail_seeds.json: {"rows3": [...], "row0": [...]}, entries {seed, stream, t, row, lane, n, tail}"""
    with open(SEEDS_JSON) as f:
        return json.load(f)["boxes"]


def recorded(box, tail):
    """the first recorded entry of a box ('rows3' / 'row0') in a tail ('lower' / 'upper')"""
    return next(e for e in recorded_seeds()[box] if e["tail"] == tail)


class SeedSearch:
    """tests/noise_seed_search.c as a program in build_dir"""

    def __init__(self, build_dir):
        cc = shutil.which("gcc") or shutil.which("cc")
        if cc is None:
            raise RuntimeError("no C compiler for tests/noise_seed_search.c")
        self.exe = os.path.join(str(build_dir), "noise_seed_search")
        subprocess.check_call([cc, "-O3", "-pthread", SEARCH_SRC, "-o", self.exe])

    def run(self, start, count, box, threads=1):
        """the hits of the seeds [start, start + count) in box 3 (rows 0 .. 2) or 1 (row 0): dicts like the recorded entries"""
        out = subprocess.check_output([self.exe, str(int(start)), str(int(count)), str(int(box)), str(FAR_N), str(int(threads))], text=True)
        hits = []
        for line in out.splitlines():
            seed, stream, t, row, lane, n = (int(v) for v in line.split())
            hits.append(dict(seed=seed, stream=stream, t=t, row=row, lane=lane, n=n, tail="lower" if n <= FAR_N else "upper"))
        return sorted(hits, key=lambda e: (e["seed"], e["t"], e["row"], e["lane"]))

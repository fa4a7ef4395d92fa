"""The seeded standard-normal draws without a GPU: the C and the NumPy restatement (tests/noise_ref.c,
tests/noise_ref.py) give the same bits on windows that reach the high counter words; their Philox meets the Random123 known
answers and the oracle's; the uniform's two extremes; the inverse CDF against statistics.NormalDist().inv_cdf and
scipy.special.ndtri on a fixed list of u; the moments and correlations of 2^20 draws at a fixed seed inside five-sigma bounds."""
import math
import statistics

import numpy as np
import pytest

from tests import noise_ref as NR

SEED = 0x243F6A8885A308D3          # the first 64 bits of pi: the committed seed of the moment checks
# The largest relative difference of the restated inverse CDF to each reference over U_LIST, measured once, and the gate at four
# times that: the margin for ulp-level differences between epi_log and a libm (the two references differ from each other by the
# same order).  DESIGN.md §4.21 quotes both.
MEASURED_VS_STATISTICS = 5.634297790584442e-16
MEASURED_VS_SCIPY = 1.0284279997470381e-15


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return NR.NoiseRef(tmp_path_factory.mktemp("noise_ref"))


def u_list():
    """2^16 equispaced points, both branch boundaries +- 1 ulp (|u - 0.5| = 0.425; r = 5, that is min(u, 1 - u) = e^-25), and
    2^-53 2^k, k = 0 .. 52"""
    b = []
    for v in (0.075, 0.925, math.exp(-25.0), 1.0 - math.exp(-25.0)):
        b += [np.nextafter(v, 0.0), v, np.nextafter(v, 1.0)]
    return np.concatenate([(np.arange(2 ** 16) + 0.5) / 2 ** 16, b, 2.0 ** -53 * 2.0 ** np.arange(53)])


def test_philox_known_answers(ref):
    from oracle import oracle_lib as olib
    kat = [([0] * 4, [0] * 2, [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, want in kat:
        assert ref.philox(ctr, key) == want
        assert [int(v[0]) for v in NR.philox(*[[c] for c in ctr], *key)] == want
        assert olib.philox4x32_10(ctr, key) == want


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("stream", [0, 2 ** 30 - 1])
def test_restatements_agree_on_windows(ref, rows, stream):
    # nt = 3, 130 lanes: an odd pair count with rows = 3, a crossed 64-lane boundary.  t is ONE 32-bit counter word, so of the
    # offsets 0, 2^32 - 2, 2^40 + 1 the lane takes all three and t0 those whose window fits: 0 and 2^32 - 3 (the last that does)
    for t0 in (0, 2 ** 32 - 3):
        for lane0 in (0, 2 ** 32 - 2, 2 ** 40 + 1):
            a, b = ref.fill(SEED, stream, t0, 3, rows, lane0, 130), NR.fill(SEED, stream, t0, 3, rows, lane0, 130)
            assert NR.same_bits(a, b), (t0, lane0)
            assert np.isfinite(a).all() and len(np.unique(a)) == a.size
    # every index enters: another t0, lane0, stream, seed or row gives other draws
    base = NR.fill(SEED, stream, 5, 1, rows, 7, 130)
    for other in (NR.fill(SEED, stream, 6, 1, rows, 7, 130), NR.fill(SEED, stream, 5, 1, rows, 7 + 2 ** 32, 130),
                  NR.fill(SEED, stream ^ 1, 5, 1, rows, 7, 130), NR.fill(SEED ^ (1 << 40), stream, 5, 1, rows, 7, 130)):
        assert not (base == other).any()
    # a window is a window: lane0 = 7 + 64 of the same array
    assert NR.same_bits(base[:, :, 64:], NR.fill(SEED, stream, 5, 1, rows, 71, 66))
    if rows == 3:
        assert NR.same_bits(base[:, :1], NR.fill(SEED, stream, 5, 1, 1, 7, 130))      # row 0 of both shapes is one draw


def test_uniform_extremes(ref):
    assert ref.uniform(0, 0) == 2.0 ** -53 == float(NR.uniform(0, 0))
    assert ref.uniform(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53 == float(NR.uniform(0xffffffff, 0xffffffff))
    assert ref.uniform(0x3f, 0x3f) == 2.0 ** -53                                    # the low six bits of a word are dropped
    assert ref.uniform(0, 0x40) == 3 * 2.0 ** -53 and ref.uniform(0x40, 0) == (2.0 ** 26 + 0.5) * 2.0 ** -52
    z = ref.icdf([2.0 ** -53, 1.0 - 2.0 ** -53])
    assert z[0] == -z[1] and 8.2095 < z[1] < 8.2096                                  # |z| <= 8.2096 everywhere
    assert NR.same_bits(z, NR.icdf([2.0 ** -53, 1.0 - 2.0 ** -53]))


def test_inverse_cdf_against_two_references(ref):
    from scipy.special import ndtri
    u = u_list()
    z = ref.icdf(u)
    assert NR.same_bits(z, NR.icdf(u))
    assert np.isfinite(z).all() and (np.diff(z[:2 ** 16]) > 0).all() and np.abs(z).max() < 8.2096
    nd = statistics.NormalDist()
    zs, zp = np.array([nd.inv_cdf(float(v)) for v in u]), ndtri(u)
    nz = zs != 0.0                                                                    # u = 0.5 is not in the list; guard all the same
    d_stat = float(np.max(np.abs(z - zs)[nz] / np.abs(zs[nz])))
    d_scipy = float(np.max(np.abs(z - zp)[nz] / np.abs(zp[nz])))
    print("largest relative difference: to statistics %.17g, to scipy %.17g" % (d_stat, d_scipy))
    assert d_stat <= 4 * MEASURED_VS_STATISTICS, d_stat
    assert d_scipy <= 4 * MEASURED_VS_SCIPY, d_scipy


def _corr(a, b):
    return float(np.mean((a - a.mean()) * (b - b.mean())) / (a.std() * b.std()))


def test_moments_and_correlations():
    n = 2 ** 20
    a = NR.fill(SEED, 0, 0, 2, 3, 0, n)                                               # days 0, 1; rows 0 .. 2; lanes 0 .. n-1
    x = a[0, 0]
    got = {"mean": float(x.mean()), "var": float(x.var()), "lanes 2i / 2i+1": _corr(x[0::2], x[1::2]), "rows 0 / 1": _corr(x, a[0, 1]),
           "rows 0 / 2": _corr(x, a[0, 2]), "days t / t+1": _corr(x, a[1, 0]),
           "streams 0 / 1": _corr(x, NR.fill(SEED, 1, 0, 1, 1, 0, n)[0, 0]),
           "seeds one bit apart": _corr(x, NR.fill(SEED ^ 1, 0, 0, 1, 1, 0, n)[0, 0])}
    print(got)
    assert abs(got["mean"]) <= 5 / math.sqrt(n)
    assert abs(got["var"] - 1) <= 5 * math.sqrt(2 / n)
    for k in ("lanes 2i / 2i+1", "rows 0 / 1", "rows 0 / 2", "days t / t+1", "streams 0 / 1", "seeds one bit apart"):
        assert abs(got[k]) <= 5 / math.sqrt(n), k
    # the tails are there: 15 % of the draws take a tail branch, and the whole array is inside the bound
    assert 0.149 < float(np.mean(np.abs(a) > 1.4395314709384563)) < 0.151 and np.abs(a).max() < 8.2096

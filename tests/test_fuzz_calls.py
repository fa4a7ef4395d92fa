"""The random hunts of tests/test_gpu_fuzz_calls.py, as far as they go without a device: over every call's default seeds the
generators of tests/fuzz_calls.py reach every entry of the call's declared feature list (and nothing outside it), the two
restatements of a call agree bit for bit on every example -- a hunt of the references themselves -- and the restatement the
GPU test compares with answers every item of every example: no example is left out.  ar_forecast and smoother_draws carry
seeded twins (FZ.seeded_twin: the same example with its z made from a noise seed) among their default cases."""
import numpy as np
import pytest

from tests import fuzz_calls as FZ


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    return FZ.Refs(tmp_path_factory)


_WANT = {}


def want(refs, call):
    """(case, the reference's outputs) of every default seed and of every seeded twin, computed once per call and shared (read-only)"""
    if call not in _WANT:
        _WANT[call] = [(c, FZ.reference(refs, c)) for c in FZ.default_cases(call, refs)]
    return _WANT[call]


def _identical(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_identical(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and FZ.same_bits(a, b)
    return type(a) is type(b) and (a == b or (isinstance(a, float) and a != a and b != b))


@pytest.mark.parametrize("call", list(FZ.CALLS))
def test_a_generator_is_a_pure_function_of_its_seed(call):
    a, b = FZ.CALLS[call].make(3), FZ.CALLS[call].make(3)
    assert a.summary == b.summary and a.features == b.features and a.names == b.names and a.cut == b.cut and a.host == b.host
    assert _identical(a.kw, b.kw)
    assert FZ.CALLS[call].make(4).summary != a.summary


@pytest.mark.parametrize("call", list(FZ.CALLS))
def test_default_seeds_reach_every_declared_feature(refs, call):
    spec = FZ.CALLS[call]
    assert spec.n >= 20 and len(set(spec.features)) == len(spec.features)
    seen = set()
    for case, w in want(refs, call):
        seen |= case.features | spec.result_features(w)
    assert seen - set(spec.features) == set(), "features outside the declared list"
    assert set(spec.features) - seen == set(), "declared features the default seeds never reach"


@pytest.mark.parametrize("call", list(FZ.CALLS))
def test_the_reference_answers_every_item_of_every_example(refs, call):
    """no example is refused or left out: every output the example asks for comes back in the shape the library's own shape rule gives for the example, and
    where the restatement's loader pre-fills its outputs none of their words still holds the sentinel"""
    for case, w in want(refs, call):
        shapes = FZ.expected_shapes(case)
        for k in case.names:
            assert k in w and np.asarray(w[k]).dtype.kind in "if", (case.summary, k)
            a = np.asarray(w[k])
            assert a.shape == tuple(shapes[k]), (case.summary, k, a.shape, shapes[k])
            if call in FZ.SENTINELS:
                assert not (a == FZ.SENTINELS[call][0 if a.dtype.kind == "i" else 1]).any(), (case.summary, k)


@pytest.mark.parametrize("call", [c for c in FZ.CALLS if c not in FZ.ONE_READING])
def test_the_two_readings_agree_bit_for_bit(refs, call):
    for case, w in want(refs, call):
        other = FZ.second_reading(refs, case)
        assert other is not None
        for k in other:
            assert FZ.same_bits(w[k], other[k]), (case.summary, k)


@pytest.mark.parametrize("call", list(FZ.SEEDED_CALLS))
def test_seeded_twins(refs, call):
    """a twin follows its example, leaves it as it was, differs from it in z alone, and its z is the array of its noise seed
    under BOTH noise restatements, in the shape the call's z has"""
    from tests import noise_ref as NR
    plain, cases = FZ.default_cases(call), FZ.default_cases(call, refs)
    assert [c.summary for c in cases if c.noise is None] == [c.summary for c in plain]
    twins = [(cases[i - 1], c) for i, c in enumerate(cases) if c.noise is not None]
    assert 0 < len(twins) <= len(plain) // 2 and any(t.host for _, t in twins) and any(not t.host for _, t in twins)
    for case, twin in twins:
        assert case.noise is None and case.seed == twin.seed and case.seed % FZ.TWIN_EVERY == 0 and case.kw["z"] is not None
        assert "z:seeded" in twin.features and "z:seeded" not in case.features
        assert {f for f in twin.features if f[:2] != "z:"} == {f for f in case.features if f[:2] != "z:"}
        assert (twin.names, twin.cut, twin.host) == (case.names, case.cut, case.host)
        assert _identical(FZ.CALLS[call].make(case.seed).kw, case.kw)                     # the example itself: untouched
        assert _identical({k: v for k, v in twin.kw.items() if k != "z"}, {k: v for k, v in case.kw.items() if k != "z"})
        seed, stream = twin.noise
        assert 0 <= seed < 2 ** 64 and 0 <= stream < 2 ** 30 and twin.kw["z"].dtype == np.float64
        assert twin.kw["z"].shape == case.kw["z"].shape
        nt, lanes = twin.kw["z"].shape[0], twin.kw["z"].shape[-1]
        z = NR.fill(seed, stream, 0, nt, 1 if call == "ar_forecast" else 3, 0, lanes)
        assert NR.same_bits(twin.kw["z"], z[:, 0] if call == "ar_forecast" else z), twin.summary
    assert FZ.seeded_twin(refs, twins[0][1]) is None                                      # a twin has no twin

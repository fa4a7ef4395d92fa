"""pipeline.curve_boxplot and the curves= keyword of smoothed_fan / forecast_fan / forecast_outlook: without the keyword, and with
curves=None, the calls return exactly what they returned before it existed (the same keys, the same bits); with it the summary
gains `curves`, which equals the restatement tests/curve_depth_ref.py on the copied-back paths."""
import inspect

import numpy as np
import pytest

from tests import curve_depth_ref as S


def test_curves_defaults_to_none_everywhere():
    from epidemicmodeling_amd import pipeline
    for f in (pipeline.smoothed_fan, pipeline.forecast_fan, pipeline.forecast_outlook):
        assert inspect.signature(f).parameters["curves"].default is None, f.__name__
    sig = inspect.signature(pipeline.curve_boxplot).parameters
    assert (sig["alpha"].default, sig["fence_factor"].default, sig["fence_frac"].default) == ((0.5, 0.9), 1.5, 0.5)


@pytest.mark.gpu
def test_smoothed_fan_with_and_without_curves(gpu_device):
    from epidemicmodeling_amd import pipeline, synth
    B, T, D, k0 = 3, 40, 65, 8
    w = synth.make_cfg3(B, T)
    N = np.linspace(1e6, 5e6, B)
    _, X0, s0, _ = pipeline.smoothed_fan(w, D, population=N, seed=5, k0=k0, device=gpu_device)
    _, X1, s1, _ = pipeline.smoothed_fan(w, D, population=N, seed=5, k0=k0, device=gpu_device, curves=None)
    _, X2, s2, _ = pipeline.smoothed_fan(w, D, population=N, seed=5, k0=k0, device=gpu_device, curves=dict(alpha=(0.25, 0.5, 1.0)))
    assert list(s0) == list(s1) and "curves" not in s0 and list(s2) == list(s0) + ["curves"]
    for X, s in ((X1, s1), (X2, s2)):
        assert np.array_equal(X.cpu().numpy(), X0.cpu().numpy(), equal_nan=True)
        for k in s0:
            assert np.array_equal(s[k].cpu().numpy(), s0[k].cpu().numpy(), equal_nan=True), k
    cv = s2["curves"]
    want = S.statistics(X0.cpu().numpy(), B, D, alpha=(0.25, 0.5, 1.0), population=N)
    for k in S.NAMES:
        assert S.same_bits(cv["statistics"][k].cpu().numpy(), want[k]), k
    for k in ("median_curve", "env_lo", "env_hi", "whisk_lo", "whisk_hi", "n_outliers", "n_ranked"):
        assert cv[k] is cv["statistics"][k]
    # alpha = 1 is the ensemble's own min and max; the depth's summary counts the ranked paths
    assert np.array_equal(cv["env_lo"][:, 2].cpu().numpy(), s0["min"].cpu().numpy(), equal_nan=True)
    assert np.array_equal(cv["env_hi"][:, 2].cpu().numpy(), s0["max"].cpu().numpy(), equal_nan=True)
    assert tuple(cv["depth"]["quantiles"].shape) == (4, 5, B) and (cv["depth"]["count"].cpu().numpy() == want["n_ranked"]).all()

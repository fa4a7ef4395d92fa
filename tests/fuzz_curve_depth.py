"""The random hunt of the curve statistics: `draw(seed)` gives one example -- sizes, window, first_day, storage, derived row,
fractions, fences, an output subset, segments, a launch cut and planted values -- drawn from the seed alone, small enough that a
device example takes milliseconds.  tests/test_fuzz_curve_depth.py runs the examples through the host build of the lane-shaped
kernels and the NumPy restatement, tests/test_gpu_fuzz_curve_depth.py through the device (one in four also through hostapi); both
compare with the C restatement tests/curve_depth_ref.c bit for bit."""
import numpy as np

from tests import curve_depth_ref as S

DEFAULT_EXAMPLES = 48


def draw(seed):
    """{kw: the arguments of statistics() (src first), opt: alpha / fence_factor / fence_frac, outputs (None: all), segments,
    launch_groups, host: also through hostapi}"""
    rng = np.random.default_rng([20261021, 23, int(seed)])
    D = int(rng.choice([1, 2, 3, 5, 33, 63, 64, 65, 70, 129, 200, 257]))
    R = int(rng.choice([1, 2, 3]))
    T = int(rng.choice([1, 2, 5, 31, 32, 33, 40, 65, 70, 100]))
    derive = bool(rng.random() < 0.4)
    rows = 3 if derive else int(rng.choice([1, 2, 4]))
    k0 = int(rng.integers(0, T))
    k1 = int(rng.integers(k0 + 1, T + 1))
    if rng.random() < 0.4:
        k0, k1 = 0, T
    fd = None if rng.random() < 0.4 else rng.integers(0, T + 2, size=R).astype(np.int32)
    kind = rng.random()
    if kind < 0.3:
        src = rng.integers(0, 4, size=(T, rows, R * D)).astype(np.float64)          # ties everywhere
    else:
        src = rng.standard_normal((T, rows, R * D)) * 10.0 ** rng.uniform(-2, 2, size=(T, rows, 1))
    src[rng.random(src.shape) < rng.choice([0.0, 0.02, 0.5])] = np.nan
    if rng.random() < 0.3:
        src[:, int(rng.integers(0, rows)), int(rng.integers(0, R * D))] = np.nan    # a path that is NaN throughout
    if rng.random() < 0.3:
        src[int(rng.integers(0, T)), int(rng.integers(0, rows)), :] = np.nan        # a day without members
    for _ in range(int(rng.integers(0, 4))):
        src[int(rng.integers(0, T)), int(rng.integers(0, rows)), int(rng.integers(0, R * D))] = rng.choice([np.inf, -np.inf, 0.0, -0.0])
    if rng.random() < 0.3 and D > 1:
        r = int(rng.integers(0, R))
        src[:, :, r * D + D - 1] = src[:, :, r * D]                                  # identical paths
    storage = "f32" if rng.random() < 0.4 else "f64"
    if storage == "f32":
        src = src.astype(np.float32)
    pop = rng.uniform(1e3, 1e7, R) if derive else None
    na = int(rng.choice([0, 1, 2, 3, 8]))
    alpha = tuple(np.sort(rng.choice(np.arange(1, 41), size=na, replace=False)) / 40.0)
    ff = float(rng.choice([0.0, 0.5, 1.5, 3.0]))
    opt = dict(alpha=alpha, fence_factor=ff, fence_frac=float(rng.choice([0.05, 0.5, 1.0])))
    ok = [k for k in S.NAMES if (na or k not in S.ENV) and (ff > 0 or k not in S.NEED_FENCE)]
    outputs = None
    if rng.random() < 0.5:
        outputs = tuple(k for k in ok if rng.random() < 0.35) or ("depth",)
    nblk = (k1 - k0 + 31) // 32
    return dict(kw=dict(src=src, R=R, D=D, population=pop, first_day=fd, k0=k0, k1=k1), opt=opt, outputs=outputs, names=ok,
                segments=int(rng.integers(0, nblk + 1)), launch_groups=int(rng.choice([0, 0, 1, 2, 5])), host=seed % 4 == 0)


def coverage(n=DEFAULT_EXAMPLES):
    """what the first n seeds reach, for the assertion of tests/test_fuzz_curve_depth.py"""
    ex = [draw(s) for s in range(n)]
    return {"f32": sum(x["kw"]["src"].dtype == np.float32 for x in ex), "derive": sum(x["kw"]["population"] is not None for x in ex),
            "first_day": sum(x["kw"]["first_day"] is not None for x in ex), "subset": sum(x["outputs"] is not None for x in ex),
            "no_fence": sum(x["opt"]["fence_factor"] == 0 for x in ex), "no_alpha": sum(len(x["opt"]["alpha"]) == 0 for x in ex),
            "eight_alpha": sum(len(x["opt"]["alpha"]) == 8 for x in ex), "segments": sum(x["segments"] > 1 for x in ex),
            "cut": sum(x["launch_groups"] > 0 for x in ex), "blocks": sum((x["kw"]["k1"] - x["kw"]["k0"]) > 32 for x in ex),
            "two_registers": sum(x["kw"]["D"] > 64 for x in ex), "one_draw": sum(x["kw"]["D"] == 1 for x in ex),
            "host": sum(x["host"] for x in ex)}

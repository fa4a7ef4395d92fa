"""The random hunt of the innovation whiteness diagnostics: `draw(seed)` gives one example -- sizes, n_lags, window, layout,
storage, flip, S or none, an output subset and planted days -- drawn from the seed alone, small enough that a device example
takes milliseconds.  tests/test_fuzz_innov_diag.py runs the examples through the host build of the kernels' source,
tests/test_gpu_fuzz_innov_diag.py through the device (one in four also through hostapi); both compare with the restatement
tests/innov_diag_ref.py bit for bit."""
import numpy as np

from tests import innov_diag_ref as DR

DEFAULT_EXAMPLES = 48


def draw(seed):
    """{e [T, B], S or None, kw (H, k0, k1, flip, storage), blk, outputs (None: all), host: also through hostapi}"""
    rng = np.random.default_rng([20261021, int(seed)])
    T = int(rng.choice([1, 2, 31, 32, 33, 45, 64, 65, 97, 130]))
    B = int(rng.choice([1, 2, 63, 64, 65, 70, 129]))
    H = int(rng.choice([0, 1, 2, 10, 31, 32, 33, 40, 63, 64]))
    k0 = int(rng.integers(0, T + 1))
    k1 = int(rng.integers(k0, T + 1))
    if rng.random() < 0.5:
        k0, k1 = 0, T
    with_S = rng.random() < 0.7
    e, S = DR.series(T, B, seed=int(rng.integers(1 << 30)), with_S=with_S)
    tgt = S if with_S else e
    # missing days: scattered, whole blocks, whole chains
    tgt[rng.random((T, B)) < rng.choice([0.0, 0.05, 0.5])] = np.nan
    for _ in range(int(rng.integers(0, 3))):
        b = int(rng.integers(0, (T + 31) // 32))
        tgt[32 * b:32 * b + 32, int(rng.integers(0, B))] = np.nan
    if rng.random() < 0.3:
        tgt[:, int(rng.integers(0, B))] = np.nan
    # bad values, a constant chain, a huge and a tiny chain
    for _ in range(int(rng.integers(0, 4))):
        t, c = int(rng.integers(0, T)), int(rng.integers(0, B))
        if with_S and rng.random() < 0.6:
            S[t, c] = rng.choice([0.0, -1.0, np.inf, 1e-310, -np.inf])
        else:
            e[t, c] = rng.choice([np.inf, -np.inf] + ([np.nan] if with_S else []))
    if rng.random() < 0.3:
        c = int(rng.integers(0, B))
        e[:, c] = 3.0
        if with_S:
            S[:, c] = np.where(np.isnan(S[:, c]), np.nan, 9.0)
    if rng.random() < 0.2:
        e[:, int(rng.integers(0, B))] *= rng.choice([1e150, 1e-150, 1e30])
    blk = int(rng.choice([0, 0, 3, 40, 64])) if B > 1 else 0
    if blk >= B:
        blk = 0
    outputs = None
    if rng.random() < 0.5:
        outputs = tuple(k for k in DR.ALL if rng.random() < 0.35) or ("status",)
    return dict(e=e, S=S, kw=dict(H=H, k0=k0, k1=k1, flip=bool(rng.random() < 0.3), storage="f32" if rng.random() < 0.4 else "f64"),
                blk=blk, outputs=outputs, host=seed % 4 == 0)


def coverage(n=DEFAULT_EXAMPLES):
    """what the first n seeds reach, for the assertion of tests/test_fuzz_innov_diag.py"""
    ex = [draw(s) for s in range(n)]
    return {"blocked": sum(x["blk"] > 0 for x in ex), "f32": sum(x["kw"]["storage"] == "f32" for x in ex),
            "flip": sum(x["kw"]["flip"] for x in ex), "no_S": sum(x["S"] is None for x in ex),
            "subset": sum(x["outputs"] is not None for x in ex), "lags_64": sum(x["kw"]["H"] == 64 for x in ex),
            "no_lags": sum(x["kw"]["H"] == 0 for x in ex), "empty_window": sum(x["kw"]["k0"] == x["kw"]["k1"] for x in ex),
            "host": sum(x["host"] for x in ex), "multi_block": sum(x["e"].shape[0] > 64 for x in ex)}

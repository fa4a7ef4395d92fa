"""epi_lasso_validate and the argument checks of epi_lasso_run_host, through the C ABI (no GPU needed: every case is
rejected before a device is touched)."""
import ctypes as C

import numpy as np
import pytest

D_, N_, R_ = 20, 3, 4


def _call(fn="validate", **kw):
    from epidemicmodeling_amd import _lib
    args = dict(R=R_, D=D_, n=N_, K=5, num_lambda=100, lambda_ratio=1e-4, rel_tol=1e-4, max_iter=100000)
    args.update({k: v for k, v in kw.items() if k in args})
    d = _lib.make_lasso_desc(**args)
    if "abi_version" in kw:
        d.abi_version = kw["abi_version"]
    X, y = np.ones((D_, N_, R_)), np.ones((D_, R_))
    fold = kw.get("fold_array", np.tile((np.arange(D_) % 5)[:, None], (1, R_)).astype(np.int32))
    outs = _lib.LassoOutputs()
    bufs = {k: np.empty(sh, dtype=np.int32 if k in _lib.LASSO_OUT_I32 else np.float64)
            for k, sh in _lib.lasso_shapes(R_, D_, N_, 5, 100).items()}
    for k, v in bufs.items():
        setattr(outs, k, v.ctypes.data)
    for k in kw.get("null_outs", ()):
        setattr(outs, k, None)
    err = C.create_string_buffer(256)
    xp = None if kw.get("null_x") else X.ctypes.data
    yp = None if kw.get("null_y") else y.ctypes.data
    fp = None if kw.get("null_fold") else fold.ctypes.data
    op = None if kw.get("null_out") else C.byref(outs)
    dp = None if kw.get("null_desc") else C.byref(d)
    lib = _lib.lib()
    if fn == "validate":
        rc = lib.epi_lasso_validate(dp, xp, yp, fp, op, err)
    else:
        rc = lib.epi_lasso_run_host(dp, xp, yp, fp, op, 0, err)
    return rc, err.value.decode()


BAD = [
    (dict(null_desc=True), -5, "NULL descriptor"),
    (dict(abi_version=5), -5, "ABI"),
    (dict(R=0), -5, "R must be"),
    (dict(D=1, K=0), -5, "D must be"),
    (dict(n=0), -5, "n must be"),
    (dict(num_lambda=0), -5, "num_lambda must be"),
    (dict(K=1), -5, "K must be 0"),
    (dict(K=-2), -5, "K must be 0"),
    (dict(K=21), -5, "K must not exceed D"),
    (dict(lambda_ratio=0.0), -5, "lambda_ratio"),
    (dict(lambda_ratio=1.0), -5, "lambda_ratio"),
    (dict(rel_tol=0.0), -5, "rel_tol"),
    (dict(rel_tol=float("inf")), -5, "rel_tol"),
    (dict(rel_tol=float("nan")), -5, "rel_tol"),
    (dict(max_iter=0), -5, "max_iter"),
    (dict(null_x=True), -5, "NULL X"),
    (dict(null_y=True), -5, "NULL X"),
    (dict(null_out=True), -5, "NULL X"),
    (dict(null_fold=True), -5, "NULL fold"),
    (dict(null_outs=("status",)), -5, "NULL status"),
    (dict(null_outs=("a",)), -5, "NULL a / b"),
    (dict(null_outs=("b",)), -5, "NULL a / b"),
    (dict(n=13), -8, "n is limited to 12"),
    (dict(D=257), -8, "D is limited to 256"),
    (dict(D=256, K=64), -8, "K is limited to 63"),
    (dict(num_lambda=101), -8, "num_lambda is limited to 100"),
]


@pytest.mark.parametrize("kw, rc, msg", BAD)
def test_validate_rejects(hip_lib, kw, rc, msg):
    got, text = _call("validate", **kw)
    assert got == rc and msg in text, (got, text)
    got, text = _call("run_host", **kw)                     # the host entry validates first, before any device work
    assert got == rc and msg in text, (got, text)


def test_validate_accepts(hip_lib):
    assert _call("validate") == (0, "")
    assert _call("validate", K=0, null_fold=True, null_outs=("a", "b", "mse", "se", "idx_min_mse", "idx_1se"))[0] == 0
    assert _call("validate", D=256, K=63, n=12, num_lambda=100)[0] == 0
    assert _call("validate", num_lambda=1)[0] == 0


@pytest.mark.parametrize("mutate, msg", [
    (lambda f: f.__setitem__((0, 2), 5), "fold value outside"),
    (lambda f: f.__setitem__((0, 1), -1), "fold value outside"),
    (lambda f: f.__setitem__((f[:, 3] == 4, 3), 0), "empty fold"),
])
def test_run_host_rejects_bad_partitions(hip_lib, mutate, msg):
    fold = np.tile((np.arange(D_) % 5)[:, None], (1, R_)).astype(np.int32)
    mutate(fold)
    rc, text = _call("run_host", fold_array=fold)
    assert rc == -5 and msg in text, (rc, text)


def test_python_entry_points_check_partitions(hip_lib):
    from epidemicmodeling_amd import batch, hostapi
    X, y = np.ones((D_, N_, R_)), np.ones((D_, R_))
    fold = np.tile((np.arange(D_) % 5)[:, None], (1, R_)).astype(np.int32)
    fold[fold == 4] = 0
    with pytest.raises(ValueError, match="empty"):
        batch.lasso_cv(X, y, K=5, folds=fold, device="cpu")
    from epidemicmodeling_amd._lib import EpiError
    with pytest.raises(EpiError, match="empty fold"):
        hostapi.lasso_cv(X, y, K=5, folds=fold)

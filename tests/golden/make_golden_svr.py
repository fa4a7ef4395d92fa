"""Writes tests/golden/svr_sklearn.npz: scikit-learn's SVR (LIBSVM) on a handful of small cases of both kernels, inputs built
like the suite's (tests/svr_ref.plans: normalised synthetic plans), and the worst |fitted - SVR.predict| / max|y| of the NumPy
reading at the same tolerance, which tests/test_svr_ref.py gates at 8 x.  Needs scikit-learn; run from the repository root:
    python tests/golden/make_golden_svr.py"""
import os
import sys
import tempfile

import numpy as np
from sklearn.svm import SVR

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from tests import svr_ref as SV  # noqa: E402

TOL = 1e-6
# (seed, D, F, n_rows, kernel, box as a multiple of iqr / 1.349, kernel_scale)
CASES = [(1, 40, 5, 30, "linear", 1.0, 1.0), (2, 120, 49, 90, "linear", 1.0, 1.0), (3, 120, 49, 120, "linear", 4.0, 1.0),
         (4, 60, 13, 45, "gaussian", 1.0, 1.0), (5, 120, 49, 90, "gaussian", 1.0, 2.0), (6, 100, 25, 100, "gaussian", 4.0, 1.5)]


def main():
    ref = SV.SvrRef(tempfile.mkdtemp())
    out = {"n_cases": len(CASES), "tol": TOL}
    worst = 0.0
    for c, (seed, D, F, n, kernel, bf, scale) in enumerate(CASES):
        X, y = SV.plans(900 + seed, D, F, 1)
        X, y = X[:, :, 0], y[:, 0]
        q = float(SV.iqr(y[:n, None])[0])
        box, eps = q / 1.349 * bf, q / 13.49
        m = SVR(kernel="linear" if kernel == "linear" else "rbf", C=box, epsilon=eps, tol=TOL, gamma=1.0 / scale ** 2, shrinking=False,
                max_iter=-1).fit(X[:n], y[:n])
        pred = m.predict(X)
        o = SV.np_svr(X[:, :, None], y[:, None], (n,), kernel, box, eps, scale, TOL, SV.MAX_ITER, ref)
        assert o["status"][0, 0] == 0
        rel = np.abs(o["fitted"][0, :, 0] - pred).max() / np.abs(y).max()
        print(c, kernel, "n", n, "F", F, "C %.3g" % box, "ours", int(o["n_iter"][0, 0]), "libsvm", int(np.ravel(m.n_iter_)[0]), "rel %.3g" % rel)
        worst = max(worst, rel)
        out.update({f"X{c}": X, f"y{c}": y, f"n{c}": n, f"kernel{c}": SV.KERNELS.index(kernel), f"box{c}": box, f"eps{c}": eps,
                    f"scale{c}": scale, f"pred{c}": pred})
    out["measured"] = worst
    print("worst |fitted - sklearn| / max|y|:", worst)
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "svr_sklearn.npz"), **out)


if __name__ == "__main__":
    main()

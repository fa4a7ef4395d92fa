"""ctypes binding of libepiekf.so (the C ABI of include/epiekf.h).

There is NO CPU fallback: if the HIP library is missing or fails to load, importing the
compute API raises -- the product path never routes through oracle/ or NumPy."""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple

import numpy as np

from . import layout as L

HERE = os.path.dirname(os.path.abspath(__file__))
# EPIEKF_LIB: load another build of the same ABI instead (A/B measurements of kernel variants)
LIB_PATH = os.environ.get("EPIEKF_LIB") or os.path.join(HERE, "libepiekf.so")

ABI_VERSION = 6      # EPIEKF_ABI_VERSION of include/epiekf.h
ABI_SYMBOLS = [
    "epi_abi_version", "epi_status_string", "epi_model_dim", "epi_ekf_validate", "epi_ekf_workspace_bytes",
    "epi_ekf_precheck_device", "epi_ekf_time_stages_device", "epi_ekf_preferred_lane_block", "epi_ekf_run_device", "epi_ekf_run_host", "epi_ekf_run_host_multi", "epi_host_pool_release", "epi_sialpha_sim_device", "epi_sialpha_score_device", "epi_seirp_sim_device",
    "epi_random_npi_mc_device", "epi_pareto_front_device", "epi_npi_cost_device", "epi_si_controlled_device", "epi_si_controlled_host", "epi_sialpha_sim_host", "epi_seirp_sim_host", "epi_npi_cost_host", "epi_calib_copy_f64_device",
    "epi_rt_expfit_validate", "epi_rt_expfit_run_device", "epi_rt_expfit_run_host",
    "epi_preprocess_workspace_bytes", "epi_preprocess_device", "epi_nnls_affine_fit_device",
    "epi_sweep_run_device", "epi_sweep_prescribe_host", "epi_preprocess_host", "epi_nnls_affine_fit_host", "epi_random_npi_mc_host",
    "epi_sir_sim_device", "epi_sir_sim_host",
    "epi_lookahead_validate", "epi_lookahead_workspace_bytes", "epi_lookahead_run_device", "epi_lookahead_run_host",
    "epi_rtwin_validate", "epi_rtwin_run_device", "epi_rtwin_run_host",
    "epi_lasso_validate", "epi_lasso_run_device", "epi_lasso_run_host",
    "epi_ens_validate", "epi_ens_run_device", "epi_ens_run_host",
    "epi_arfc_validate", "epi_arfc_run_device", "epi_arfc_run_host",
    "epi_fuse_validate", "epi_fuse_run_device", "epi_fuse_run_host",
    "epi_robfit_validate", "epi_robfit_run_device", "epi_robfit_run_host",
    "epi_ratemap_validate", "epi_ratemap_run_device", "epi_ratemap_run_host",
    "epi_mldiv_validate", "epi_mldiv_run_device", "epi_mldiv_run_host",
    "epi_svr_validate", "epi_svr_run_device", "epi_svr_run_host",
    "epi_loglik_validate", "epi_loglik_workspace_bytes", "epi_loglik_run_device", "epi_loglik_run_host",
    "epi_idiag_validate", "epi_idiag_workspace_bytes", "epi_idiag_run_device", "epi_idiag_run_host",
    "epi_cdepth_validate", "epi_cdepth_workspace_bytes", "epi_cdepth_run_device", "epi_cdepth_run_host",
    "epi_plan_validate", "epi_plan_workspace_bytes", "epi_plan_run_device", "epi_plan_run_host",
    "epi_sdraw_validate", "epi_sdraw_workspace_bytes", "epi_sdraw_run_device", "epi_sdraw_run_host",
    "epi_escore_validate", "epi_escore_workspace_bytes", "epi_escore_run_device", "epi_escore_run_host",
    "epi_pathfn_validate", "epi_pathfn_workspace_bytes", "epi_pathfn_run_device", "epi_pathfn_run_host",
    "epi_ejoint_validate", "epi_ejoint_workspace_bytes", "epi_ejoint_run_device", "epi_ejoint_run_host",
    "epi_noise_validate", "epi_noise_fill_device", "epi_noise_fill_host",
    "epi_sdraw_run_device_seeded", "epi_sdraw_run_host_seeded", "epi_arfc_run_device_seeded", "epi_arfc_run_host_seeded",
    "epi_sialpha_sim_device_seeded", "epi_sialpha_score_device_seeded", "epi_sialpha_sim_host_seeded",
    "epi_random_npi_mc_device_seeded", "epi_random_npi_mc_host_seeded",
]


class EpiError(RuntimeError):
    """Raised for a negative epi_status; .status holds the code, the message is the reference's
    own error() text for the four reference errors (include/epiekf.h)."""

    def __init__(self, status: int, msg: str):
        super().__init__(msg)
        self.status = status


class BatchDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "model", "B", "T", "Sx", "Su", "n_npi", "L", "order",
                                          "obs_type", "r_mode", "q_mode")] + [
        ("out_mask", C.c_uint32), ("phase", C.c_int32), ("path_hint", C.c_int32), ("time_pipe", C.c_int32),
        ("lane_block", C.c_int32), ("shape", C.c_int32), ("storage", C.c_int32), ("exact_nonfinite", C.c_int32),
        ("placement_tries", C.c_int32),                                  # host-pointer entry points: candidate arenas (include/epiekf.h)
        ("test_window", C.c_int32), ("test_flags", C.c_int32)]           # test hooks, 0 in production


class Inputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("x_series", "u_series", "x", "u", "R_series", "R_scalar", "prm",
                                           "s_init", "Ps_init", "s_final", "Ps_final", "Q")]


class Outputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("u_opt", "u_opt_smooth", "S_MINUS", "S_PLUS", "S_SMOOTH", "P_MINUS",
                                           "P_PLUS", "P_SMOOTH", "K_GAIN", "innovations", "rho", "pinv_rank",
                                           "status", "placement")]


class PlacementReport(C.Structure):
    _fields_ = [("tries", C.c_int32), ("chosen", C.c_int32), ("ms", C.c_float * 8)]


class SweepDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "R", "P", "t_hist")]


class PrescribeDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "R", "P", "T", "t_hist", "n_npi", "L", "order", "obs_type")] + [
        ("out_mask", C.c_uint32), ("shape", C.c_int32), ("time_pipe", C.c_int32), ("placement_tries", C.c_int32)]


class PrescribeInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("x", "u", "R_series", "prm", "s_init", "Ps_init", "s_final", "Ps_final", "Q", "eps",
                                           "sp", "J0_prefix", "J1_prefix")]


class PrescribeOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("J0", "J1", "on_front", "i_opt", "u_opt", "S_opt")] + [("extras", Outputs), ("placement", C.c_void_p)]


class SimDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "B", "K", "Su", "n_npi", "noise", "with_cost", "prefix_days",
                                          "u_block")]


class McDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "R", "n_scen", "K", "n_npi", "noise", "prefix_days")] + [
        ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32)]


class NoiseDesc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("stream", C.c_uint32)]


def make_noise_desc(seed, stream=0) -> NoiseDesc:
    """The descriptor of the seeded draws (include/epiekf.h): seed a 64-bit integer (the Philox key), stream below 2^30"""
    seed, stream = int(seed), int(stream)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must lie in 0 .. 2^64 - 1")
    if not 0 <= stream < 1 << 32:
        raise ValueError("stream must lie in 0 .. 2^30 - 1")       # 2^30 .. 2^32 - 1 reach the library's own check
    d = NoiseDesc()
    d.abi_version, d.seed_lo, d.seed_hi, d.stream = ABI_VERSION, seed & 0xFFFFFFFF, seed >> 32, stream
    return d


def noise_of(seed, stream, z):
    """The seed= / stream= keywords of the Monte-Carlo calls -> a NoiseDesc, or None without a seed; seed and z together raise"""
    if seed is None:
        if stream:
            raise ValueError("stream without seed")
        return None
    if z is not None:
        raise ValueError("seed and z together: the draws have one source")
    return make_noise_desc(seed, stream)


class RtDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "B", "T", "Sx", "L", "order")]


RT_OUT_NAMES = ("S_MINUS", "S_PLUS", "P_MINUS", "P_PLUS", "K_GAIN", "S_SMOOTH", "P_SMOOTH", "innovations", "rho")


class RtOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in RT_OUT_NAMES]


class PreDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "S", "T", "n_npi", "W", "first_num_days")] + [("min_cases", C.c_double)]


PRE_OUT_NAMES = ("new_refined", "new_smoothed", "zero_lag", "x_new", "x_total", "R_v", "fatality", "I0", "ip_filled")


class PreOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in PRE_OUT_NAMES]


class LookaheadDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "model", "R", "LL", "F", "M", "n_npi", "L", "order", "obs_type", "r_mode",
                                          "shape", "placement_tries")]


LA_IN_NAMES = ("x", "u", "R_series", "R_scalar", "prm", "s_init", "Ps_init", "s_final", "Ps_final", "Q", "truth", "population")
LA_OUT_NAMES = ("est_plus", "est_smooth", "mean_plus", "median_plus", "std_plus", "mean_smooth", "median_smooth", "std_smooth",
                "S_PLUS", "S_SMOOTH", "status")


class LookaheadInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in LA_IN_NAMES]


class LookaheadOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in LA_OUT_NAMES]


def out_names(all_names, outputs, default):
    """the validated list of output names of a family call: `outputs`, or `default` when it is None"""
    names = list(default if outputs is None else outputs)
    bad = [k for k in names if k not in all_names]
    if bad:
        raise ValueError(f"unknown outputs {bad}")
    if not names:
        raise ValueError("no output requested")
    return names


class RtwinDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "R", "L", "wlen", "causal", "generation_period", "methods")] + \
        [("time_unit", C.c_double)]


RTWIN_METHODS = {"LogLinReg": 1, "GenRatios": 2, "NonlinLS": 4}
RTWIN_OUT_F64 = ("llr_Rt", "llr_A", "llr_Lambda", "llr_ExpFit", "gr_Rt", "gr_Lambda", "gr_RtSmoothed", "gr_LambdaSmoothed",
                 "nls_Rt", "nls_A", "nls_Lambda", "nls_ExpFit")
RTWIN_OUT_I32 = ("nls_status", "nls_iters")
RTWIN_OUT_NAMES = RTWIN_OUT_F64 + RTWIN_OUT_I32
RTWIN_STATUS = {"outside": 0, "tolx": 1, "tolfun": 2, "maxiter": 3, "stall": 4, "skipped": 5, "model_error": 6}


class RtwinOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in RTWIN_OUT_NAMES]


class LassoDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "R", "D", "n", "K", "num_lambda")] + \
        [("lambda_ratio", C.c_double), ("rel_tol", C.c_double), ("max_iter", C.c_int32)]


LASSO_OUT_NAMES = ("a", "b", "lambda", "B", "intercept", "df", "mse", "se", "iters", "idx_min_mse", "idx_1se", "status")
LASSO_OUT_I32 = ("df", "iters", "idx_min_mse", "idx_1se", "status")
LASSO_STATUS = {"ok": 0, "null_model": 1, "maxiter": 2, "nonfinite": 3, "bad_folds": 4}


class LassoOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in LASSO_OUT_NAMES]


def lasso_shapes(R, D, n, K, num_lambda):
    """shape of every output of epi_lasso_run_* (mse, se, a, b and the indices only with K >= 2)"""
    NL = int(num_lambda)
    sh = {"lambda": (NL, R), "B": (NL, n, R), "intercept": (NL, R), "df": (NL, R), "iters": (NL, R), "status": (R,)}
    if K >= 2:
        sh.update(a=(n, R), b=(R,), mse=(NL, R), se=(NL, R), idx_min_mse=(R,), idx_1se=(R,))
    return sh


def make_lasso_desc(R, D, n, K, num_lambda=100, lambda_ratio=1e-4, rel_tol=1e-4, max_iter=100000) -> LassoDesc:
    d = LassoDesc()
    d.abi_version = ABI_VERSION
    d.R, d.D, d.n, d.K, d.num_lambda = int(R), int(D), int(n), int(K), int(num_lambda)
    d.lambda_ratio, d.rel_tol, d.max_iter = float(lambda_ratio), float(rel_tol), int(max_iter)
    return d


class RobfitDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "R", "D", "n", "robust", "max_iter")] + \
        [("lower_a", C.c_double), ("upper_a", C.c_double)]


ROBFIT_OUT_NAMES = ("a", "b_item", "sigma", "iters", "status", "weights", "b")
ROBFIT_OUT_I32 = ("iters", "status")
ROBFIT_STATUS_BITS = {"nonfinite": 1, "const": 2, "slope_lost": 4, "maxiter": 8, "bound": 16}


class RobfitOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ROBFIT_OUT_NAMES]


def robfit_shapes(R, D, n):
    """shape of every output of epi_robfit_run_*"""
    return {"a": (n, R), "b_item": (n, R), "sigma": (n, R), "iters": (n, R), "status": (n, R), "weights": (D, n, R), "b": (R,)}


def make_robfit_desc(R, D, n, robust=1, max_iter=50, lower_a=0.0, upper_a=float("inf")) -> RobfitDesc:
    d = RobfitDesc()
    d.abi_version = ABI_VERSION
    d.R, d.D, d.n, d.robust, d.max_iter = int(R), int(D), int(n), int(robust), int(max_iter)
    d.lower_a, d.upper_a = float(lower_a), float(upper_a)
    return d


def robfit_out_names(outputs):
    """the validated list of output names (default: all but weights)"""
    return out_names(ROBFIT_OUT_NAMES, outputs, [k for k in ROBFIT_OUT_NAMES if k != "weights"])


class RatemapDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "T", "n", "R", "E", "K", "n_lags")] + [("lags", C.c_int32 * 3)] + \
        [(n, C.c_int32) for n in ("fit", "effect_lag")] + \
        [(n, C.c_double) for n in ("ridge", "lambda_threshold", "reduction_effect")]


RATEMAP_IN_NAMES = ("ip", "y", "new_smoothed", "extra", "lambda_in", "n_train")
RATEMAP_OUT_NAMES = ("map", "x_mx", "y_filled", "lambda_hat", "new_cases_est", "tracker", "status")
RATEMAP_OUT_I32 = ("status",)
RATEMAP_STATUS_BITS = {"leading_nan": 1, "not_pd": 2, "nonfinite": 4}


class RatemapInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in RATEMAP_IN_NAMES]


class RatemapOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in RATEMAP_OUT_NAMES]


def ratemap_shapes(T, n, R, E, K, n_lags):
    """shape of every output of epi_ratemap_run_*"""
    F = n * (1 + n_lags) + E
    return {"map": (K, F, R), "x_mx": (F, R), "y_filled": (T, R), "lambda_hat": (K, T, R), "new_cases_est": (K, T, R),
            "tracker": (T, R), "status": (K, R)}


def make_ratemap_desc(T, n, R, E, K, lags=(3, 5, 7), fit=1, effect_lag=3, ridge=1e-6, lambda_threshold=0.1,
                      reduction_effect=0.01) -> RatemapDesc:
    lags = [int(v) for v in lags]
    if len(lags) > 3:
        raise ValueError("at most 3 lags")
    d = RatemapDesc()
    d.abi_version = ABI_VERSION
    d.T, d.n, d.R, d.E, d.K, d.n_lags, d.fit, d.effect_lag = int(T), int(n), int(R), int(E), int(K), len(lags), int(fit), int(effect_lag)
    for i, v in enumerate(lags):
        d.lags[i] = v
    d.ridge, d.lambda_threshold, d.reduction_effect = float(ridge), float(lambda_threshold), float(reduction_effect)
    return d


def ratemap_out_names(outputs, fit, have_y):
    """the validated list of output names (default: all that the call can give)"""
    return out_names(RATEMAP_OUT_NAMES, outputs, [k for k in RATEMAP_OUT_NAMES if (fit or k != "map") and (have_y or k != "y_filled")])


def ratemap_n_train(n_train, K=None):
    """n_train as the int32 HOST array the call reads (a list of MATLAB-style train ends 1 .. T)"""
    a = np.ascontiguousarray(np.atleast_1d(np.asarray(n_train)), dtype=np.int32)
    if a.ndim != 1 or a.size < 1 or (K is not None and a.size != K):
        raise ValueError("n_train must be a list of K train ends")
    return a


class MldivDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "D", "F", "R", "K")] + [("tol_scale", C.c_double)]


MLDIV_IN_NAMES = ("X", "y", "n_rows")
MLDIV_OUT_NAMES = ("m", "rank", "perm", "rdiag", "resid", "fitted", "status")
MLDIV_OUT_I32 = ("rank", "perm", "status")
MLDIV_STATUS_BITS = {"rank_deficient": 1, "nonfinite_input": 2, "nonfinite": 4}
MLDIV_MAX_F, MLDIV_MAX_ELEMS = 96, 20000


class MldivInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in MLDIV_IN_NAMES]


class MldivOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in MLDIV_OUT_NAMES]


def mldiv_shapes(D, F, R, K):
    """shape of every output of epi_mldiv_run_*"""
    return {"m": (K, F, R), "rank": (K, R), "perm": (K, F, R), "rdiag": (K, F, R), "resid": (K, R), "fitted": (K, D, R),
            "status": (K, R)}


def make_mldiv_desc(D, F, R, K, tol_scale=1.0) -> MldivDesc:
    d = MldivDesc()
    d.abi_version = ABI_VERSION
    d.D, d.F, d.R, d.K, d.tol_scale = int(D), int(F), int(R), int(K), float(tol_scale)
    return d


def mldiv_out_names(outputs):
    """the validated list of output names (default: all)"""
    return out_names(MLDIV_OUT_NAMES, outputs, MLDIV_OUT_NAMES)


def mldiv_n_rows(n_rows, D):
    """n_rows as the int32 HOST array the call reads (default: all D rows)"""
    a = np.ascontiguousarray(np.atleast_1d(np.asarray(D if n_rows is None else n_rows)), dtype=np.int32)
    if a.ndim != 1 or a.size < 1:
        raise ValueError("n_rows must be a list of K row counts")
    return a


class SvrDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "D", "F", "R", "K", "kernel", "max_iter")] + [("tol", C.c_double)]


SVR_IN_NAMES = ("X", "y", "n_rows", "box", "epsilon", "kernel_scale")
SVR_OUT_NAMES = ("beta", "bias", "w", "fitted", "n_iter", "gap", "n_sv", "status")
SVR_OUT_I32 = ("n_iter", "n_sv", "status")
SVR_STATUS_BITS = {"not_converged": 1, "bad_input": 2, "nonfinite": 4}
SVR_KERNELS = {"linear": 0, "gaussian": 1}
SVR_MAX_F, SVR_MAX_ROWS, SVR_MAX_ELEMS, SVR_MAX_ITER = 96, 1024, 20000, 10000000


class SvrInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in SVR_IN_NAMES]


class SvrOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in SVR_OUT_NAMES]


def svr_shapes(D, F, R, K):
    """shape of every output of epi_svr_run_*"""
    return {"beta": (K, D, R), "bias": (K, R), "w": (K, F, R), "fitted": (K, D, R), "n_iter": (K, R), "gap": (K, R),
            "n_sv": (K, R), "status": (K, R)}


def svr_kernel(kernel):
    if kernel not in SVR_KERNELS:
        raise ValueError(f"kernel must be one of {tuple(SVR_KERNELS)}")
    return SVR_KERNELS[kernel]


def make_svr_desc(D, F, R, K, kernel="linear", tol=1e-3, max_iter=100000) -> SvrDesc:
    d = SvrDesc()
    d.abi_version = ABI_VERSION
    d.D, d.F, d.R, d.K, d.kernel, d.max_iter, d.tol = int(D), int(F), int(R), int(K), svr_kernel(kernel), int(max_iter), float(tol)
    return d


def svr_out_names(outputs, kernel):
    """the validated list of output names (default: all, w for the linear kernel only)"""
    return out_names(SVR_OUT_NAMES, outputs, [k for k in SVR_OUT_NAMES if k != "w" or kernel == "linear"])


def svr_defaults(y, kernel="linear"):
    """fitrsvm's documented defaults for the target(s) y [n] or [n, R] (the rows the fit will use; a NaN gives NaN):
    Epsilon = iqr(y) / 13.49, and 0.1 where the iqr is zero; BoxConstraint = iqr(y) / 1.349 for the Gaussian kernel, 1
    otherwise; KernelScale = 1.  iqr is MATLAB's: quantile(y, .75) - quantile(y, .25) with the sorted sample at the
    probabilities (i - 0.5) / n and linear interpolation between them.  Recalled from MATLAB's
    documentation, not taken from the reference: a convenience, the three are inputs.
    Returns a dict box, epsilon, kernel_scale of float64 arrays [R] (scalars for a 1-D y)."""
    svr_kernel(kernel)
    a = np.asarray(y, dtype=np.float64)
    if a.ndim not in (1, 2) or a.shape[0] < 1:
        raise ValueError("y must be [n] or [n, R]")
    s = np.sort(a.reshape(a.shape[0], -1), axis=0)
    n = s.shape[0]

    def quantile(p):
        pos = p * n - 0.5                                  # 0-based position among the sorted values
        if pos <= 0:
            return s[0].copy()
        if pos >= n - 1:
            return s[n - 1].copy()
        lo = int(np.floor(pos))
        return s[lo] + (pos - lo) * (s[lo + 1] - s[lo])

    iqr = quantile(0.75) - quantile(0.25)
    iqr = np.where(np.isnan(s).any(axis=0), np.nan, iqr)
    eps = np.where(iqr == 0.0, 0.1, iqr / 13.49)
    box = iqr / 1.349 if kernel == "gaussian" else np.ones_like(iqr)
    out = {"box": box, "epsilon": eps, "kernel_scale": np.ones_like(iqr)}
    return {k: (float(v[0]) if a.ndim == 1 else v) for k, v in out.items()}


def svr_region_array(v, R, name):
    """box / epsilon / kernel_scale as a float64 array [R]: a scalar is broadcast"""
    a = np.asarray(v, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(R, float(a))
    if a.shape != (R,):
        raise ValueError(f"{name} must be a scalar or an array [R]")
    return np.ascontiguousarray(a)


class EnsDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "T", "rows", "R", "D", "n_q", "storage", "derive_newcases")] + \
        [("q", C.c_double * 16)]


ENS_OUT_NAMES = ("mean", "std", "min", "max", "quantiles", "count")
ENS_DEFAULT_Q = (0.025, 0.25, 0.5, 0.75, 0.975)


class EnsOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ENS_OUT_NAMES]


def ens_shapes(T, rows, R, n_q, derive_newcases=0):
    """shape of every output of epi_ens_run_* (rows' = rows + derive_newcases)"""
    ro = int(rows) + int(derive_newcases)
    sh = {k: (T, ro, R) for k in ("mean", "std", "min", "max", "count")}
    sh["quantiles"] = (T, int(n_q), ro, R)
    return sh


def make_ens_desc(T, rows, R, D, q=ENS_DEFAULT_Q, storage=0, derive_newcases=0) -> EnsDesc:
    """storage: 0 / "f64" = double source, 1 / "f32" = float source.  More than 16 probabilities reach the library's own
    check as n_q = len(q) (only the first 16 fit the descriptor)."""
    d = EnsDesc()
    d.abi_version = ABI_VERSION
    d.T, d.rows, d.R, d.D = int(T), int(rows), int(R), int(D)
    q = [float(v) for v in np.atleast_1d(np.asarray(q, dtype=np.float64))]
    d.n_q = len(q)
    for k, v in enumerate(q[:16]):
        d.q[k] = v
    d.storage = {"f64": 0, "f32": 1}.get(storage, storage)
    d.derive_newcases = int(derive_newcases)
    return d


class ArfcDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "R", "D", "L", "p", "H", "fit", "nv_mode", "Sd", "reserved")] + \
        [("dt", C.c_double)]


ARFC_IN_NAMES = ("seg", "beta", "s0", "i0", "z", "drive", "drive_series", "A", "noise_var")
ARFC_OUT_NAMES = ("S", "A_out", "noise_var_out", "status")
ARFC_OK, ARFC_RANK_DEFICIENT, ARFC_BAD_INPUT = 0, 1, 2


class ArfcInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ARFC_IN_NAMES]


class ArfcOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ARFC_OUT_NAMES]


def arfc_shapes(R, D, L, p, H):
    """shape of every output of epi_arfc_run_*"""
    return {"S": (int(L) + int(H), 3, int(R) * int(D)), "A_out": (int(p), int(R)), "noise_var_out": (int(R),), "status": (int(R),)}


def make_arfc_desc(R, D, L, p, H, dt, fit=1, nv_mode=0, Sd=0) -> ArfcDesc:
    d = ArfcDesc()
    d.abi_version = ABI_VERSION
    d.R, d.D, d.L, d.p, d.H = int(R), int(D), int(L), int(p), int(H)
    d.fit, d.nv_mode, d.Sd, d.reserved, d.dt = int(fit), int(nv_mode), int(Sd), 0, float(dt)
    return d


class FuseDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "m", "B", "T", "lane_block", "storage", "form", "p_solver", "reserved")]


FUSE_IN_NAMES = ("sf", "Pf", "sb", "Pb")
FUSE_OUT_NAMES = ("s_out", "P_out", "d2", "rank", "status")
FUSE_NONFINITE, FUSE_SWEEP_CAP = 1, 2          # bits of status


class FuseInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in FUSE_IN_NAMES]


class FuseOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in FUSE_OUT_NAMES]


def fuse_shapes(m, B, T, lane_block=0):
    """shape of every array of epi_fuse_run_* (sf / sb as s_out, Pf / Pb as P_out): classic [T, rows, B], or chain-blocked
    [T, nblk, rows, blk] as EkfRunner allocates its outputs"""
    m, B, T, blk = int(m), int(B), int(T), int(lane_block)
    if blk <= 0 or blk >= B:
        vec, mat = (T, m, B), (T, m * m, B)
    else:
        nblk = (B + blk - 1) // blk
        vec, mat = (T, nblk, m, blk), (T, nblk, m * m, blk)
    return {"s_out": vec, "P_out": mat, "d2": (T, B), "rank": (T, B), "status": (B,)}


def make_fuse_desc(m, B, T, form, p_solver=0, lane_block=0, storage=0) -> FuseDesc:
    d = FuseDesc()
    d.abi_version = ABI_VERSION
    d.m, d.B, d.T, d.lane_block, d.storage = int(m), int(B), int(T), int(lane_block), int(storage)
    d.form, d.p_solver, d.reserved = int(form), int(p_solver), 0
    return d


class LoglikDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "model", "B", "T", "L", "obs_type", "r_mode", "Sx", "lane_block", "storage",
                                          "k0", "k1", "G", "reserved")]


LOGLIK_IN_NAMES = ("S_MINUS", "P_MINUS", "innovations", "x", "R_series", "R_scalar", "x_series", "prm")
LOGLIK_OUT_NAMES = ("loglik", "nis_mean", "n_valid", "status", "S", "nis", "R_used", "best", "best_loglik")
LOGLIK_OUT_I32 = ("n_valid", "status", "best")
LOGLIK_BAD_DAY, LOGLIK_ROUNDED_REPLAY = 1, 4          # bits of status


class LoglikInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in LOGLIK_IN_NAMES]


class LoglikOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in LOGLIK_OUT_NAMES]


def loglik_shapes(B, T, G=0):
    B, T, G = int(B), int(T), int(G)
    sh = {k: (B,) for k in ("loglik", "nis_mean", "n_valid", "status")}
    sh.update({k: (T, B) for k in ("S", "nis", "R_used")})
    sh.update({k: (B // G if G > 0 else 0,) for k in ("best", "best_loglik")})
    return sh


def loglik_out_names(outputs, G=0):
    """None -> the four per-chain outputs, and the two of the selection with G > 0; else the names given, in the ABI's order"""
    if outputs is None:
        return list(LOGLIK_OUT_NAMES[:4]) + (list(LOGLIK_OUT_NAMES[7:]) if int(G) > 0 else [])
    for k in outputs:
        if k not in LOGLIK_OUT_NAMES:
            raise ValueError(f"unknown output {k!r}")
    return [k for k in LOGLIK_OUT_NAMES if k in outputs]


def make_loglik_desc(model, B, T, L_, obs_type, r_mode, Sx, lane_block=0, storage=0, k0=0, k1=None, G=0) -> LoglikDesc:
    d = LoglikDesc()
    d.abi_version = ABI_VERSION
    d.model = L.MODEL_IDS[model] if isinstance(model, str) else int(model)
    d.B, d.T, d.L, d.r_mode, d.Sx = int(B), int(T), int(L_), int(r_mode), int(Sx)
    d.obs_type = L.OBS_IDS.get(obs_type, 99) if isinstance(obs_type, str) else int(obs_type)
    d.lane_block, d.storage, d.k0, d.k1, d.G, d.reserved = int(lane_block), int(storage), int(k0), 0 if k1 is None else int(k1), int(G), 0
    return d


class PlanDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "R", "P", "H", "n_npi", "prefix_days", "max_iter", "max_halvings")] + [
        ("tol", C.c_double)]


PLAN_IN_NAMES = ("sp", "u_min", "eps", "u_fixed", "u_init", "J0_prefix", "J1_prefix")
PLAN_OUT_NAMES = ("plan", "J0", "J1", "F", "gap", "iters", "halvings", "status", "states", "mu", "F_trace")
PLAN_OUT_I32 = ("iters", "halvings", "status")
PLAN_OPTIONAL = ("states", "mu", "F_trace")
PLAN_SIM_PRM_COUNT = 48                                 # EPI_SIM_PRM_COUNT
PLAN_STOP_CAP, PLAN_STOP_SEARCH, PLAN_STOP_NONFINITE = 1, 2, 4      # bits of status


class PlanInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in PLAN_IN_NAMES]


class PlanOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in PLAN_OUT_NAMES]


def plan_shapes(R, P, H, n, max_iter):
    B, H, n = int(R) * int(P), int(H), int(n)
    sh = {k: (B,) for k in ("J0", "J1", "F", "gap", "iters", "halvings", "status")}
    sh.update(plan=(H, n, B), states=(H, 3, B), mu=(H, 3, B), F_trace=(int(max_iter), B))
    return sh


def plan_out_names(outputs):
    """None -> the eight required outputs; else those and the optional ones named ("states", "mu", "F_trace"), in the ABI's order"""
    extra = () if outputs is None else tuple(outputs)
    for k in extra:
        if k not in PLAN_OUT_NAMES:
            raise ValueError(f"unknown output {k!r}")
    return [k for k in PLAN_OUT_NAMES if k not in PLAN_OPTIONAL or k in extra]


def make_plan_desc(R, P, H, n_npi, prefix_days=0, max_iter=64, max_halvings=30, tol=1e-9) -> PlanDesc:
    d = PlanDesc()
    d.abi_version = ABI_VERSION
    d.R, d.P, d.H, d.n_npi, d.prefix_days = int(R), int(P), int(H), int(n_npi), int(prefix_days)
    d.max_iter, d.max_halvings, d.tol = int(max_iter), int(max_halvings), float(tol)
    return d


class SdrawDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "model", "B", "T", "D", "k0", "clamp", "lane_block", "storage", "z_f32", "out_f32",
                                         "test_launch_groups")]


SDRAW_IN_NAMES = ("S_PLUS", "P_PLUS", "S_MINUS", "P_MINUS", "prm", "z", "s_term", "P_term")
SDRAW_OUT_NAMES = ("X", "rank", "status", "J", "L")
SDRAW_OUT_I32 = ("rank", "status")
SDRAW_DEFAULT = ("X", "rank", "status")
SDRAW_NONFINITE, SDRAW_RANK_DEFICIENT = 1, 2            # bits of status


class SdrawInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in SDRAW_IN_NAMES]


class SdrawOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in SDRAW_OUT_NAMES]


def sdraw_shapes(B, T, D, k0=0):
    B, T, D, k0 = int(B), int(T), int(D), int(k0)
    return dict(X=(T - k0, 3, B * D), rank=(T, B), status=(B,), J=(T, 9, B), L=(T, 9, B))


def make_sdraw_desc(B, T, D, k0=0, clamp=True, lane_block=0, storage=0, z_f32=0, out_f32=0, model="SIAlphaModelEKF",
                    test_launch_groups=0) -> SdrawDesc:
    d = SdrawDesc()
    d.abi_version = ABI_VERSION
    d.model = L.MODEL_IDS[model] if isinstance(model, str) else int(model)
    d.B, d.T, d.D, d.k0, d.clamp, d.lane_block = int(B), int(T), int(D), int(k0), int(clamp), int(lane_block)
    d.storage, d.z_f32, d.out_f32, d.test_launch_groups = int(storage), int(z_f32), int(out_f32), int(test_launch_groups)
    return d


class EscoreDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "T", "rows", "R", "D", "Rt", "n_a", "n_bins", "storage", "derive_newcases", "k0",
                                         "k1", "test_launch_items", "reserved")] + [("alpha", C.c_double * 8)]


ESCORE_IN_NAMES = ("src", "population", "truth", "truth_series", "first_day")
ESCORE_ITEM_NAMES = ("crps", "wis", "ae", "width", "rank", "ties", "cover", "count")
ESCORE_REGION_NAMES = ("crps_mean", "wis_mean", "ae_mean", "n_scored", "cover_frac", "pit_hist")
ESCORE_OUT_NAMES = ESCORE_ITEM_NAMES + ESCORE_REGION_NAMES
ESCORE_OUT_I32 = ("rank", "ties", "cover", "count", "n_scored", "pit_hist")
ESCORE_DEFAULT_ALPHA = (0.5, 0.05)


class EscoreInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ESCORE_IN_NAMES]


class EscoreOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ESCORE_OUT_NAMES]


def escore_shapes(T, rows, R, n_a, n_bins, derive_newcases=0):
    """shape of every output of epi_escore_run_* (rows' = rows + derive_newcases)"""
    ro, n_a, n_bins = int(rows) + int(derive_newcases), int(n_a), int(n_bins)
    sh = {k: (T, ro, R) for k in ESCORE_ITEM_NAMES}
    sh["width"] = (T, n_a, ro, R)
    sh.update({k: (ro, R) for k in ESCORE_REGION_NAMES})
    sh["cover_frac"], sh["pit_hist"] = (n_a, ro, R), (n_bins, ro, R)
    return sh


def escore_out_names(outputs, n_bins):
    """None -> every output (pit_hist only with n_bins > 0); else the names asked for, in the ABI's order"""
    default = [k for k in ESCORE_OUT_NAMES if k != "pit_hist" or int(n_bins) > 0]
    names = out_names(ESCORE_OUT_NAMES, outputs, default)
    return [k for k in ESCORE_OUT_NAMES if k in names]


def make_escore_desc(T, rows, R, D, Rt, alpha=ESCORE_DEFAULT_ALPHA, n_bins=0, storage=0, derive_newcases=0, k0=0, k1=None,
                     test_launch_items=0) -> EscoreDesc:
    """storage: 0 / "f64" = double source, 1 / "f32" = float source.  More than 8 levels reach the library's own check as
    n_a = len(alpha) (only the first 8 fit the descriptor).  k1 = None: T."""
    d = EscoreDesc()
    d.abi_version = ABI_VERSION
    d.T, d.rows, d.R, d.D, d.Rt = int(T), int(rows), int(R), int(D), int(Rt)
    alpha = [float(v) for v in np.atleast_1d(np.asarray(alpha, dtype=np.float64))]
    d.n_a, d.n_bins = len(alpha), int(n_bins)
    for k, v in enumerate(alpha[:8]):
        d.alpha[k] = v
    d.storage = {"f64": 0, "f32": 1}.get(storage, storage)
    d.derive_newcases = int(derive_newcases)
    d.k0, d.k1 = int(k0), int(T) if k1 is None else int(k1)
    d.test_launch_items = int(test_launch_items)
    return d


class PathfnDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "T", "rows", "R", "D", "n_thr", "storage", "derive_newcases", "k0", "k1",
                                         "test_segments", "test_launch_groups")]


PATHFN_IN_NAMES = ("src", "population", "thr", "first_day")
PATHFN_PATH_NAMES = ("peak_value", "peak_day", "min_value", "min_day", "total")
PATHFN_THR_NAMES = ("first_cross", "days_above", "longest_run")
PATHFN_REGION_NAMES = ("n_paths", "peak_day_hist", "n_cross", "cross_day_hist")
PATHFN_OUT_NAMES = PATHFN_PATH_NAMES + PATHFN_THR_NAMES + ("n_valid",) + PATHFN_REGION_NAMES
PATHFN_OUT_I32 = ("n_valid",) + PATHFN_REGION_NAMES
PATHFN_NEED_THR = PATHFN_THR_NAMES + ("n_cross", "cross_day_hist")


class PathfnInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in PATHFN_IN_NAMES]


class PathfnOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in PATHFN_OUT_NAMES]


def pathfn_shapes(rows, R, D, n_thr, W, derive_newcases=0):
    """shape of every output of epi_pathfn_run_* (rows' = rows + derive_newcases, W = k1 - k0)"""
    ro, N, n_thr, W = int(rows) + int(derive_newcases), int(R) * int(D), int(n_thr), int(W)
    sh = {k: (ro, N) for k in PATHFN_PATH_NAMES}
    sh.update({k: (n_thr, ro, N) for k in PATHFN_THR_NAMES})
    sh["n_valid"] = (ro, N)
    sh.update(n_paths=(ro, R), peak_day_hist=(W, ro, R), n_cross=(n_thr, ro, R), cross_day_hist=(W, n_thr, ro, R))
    return sh


def pathfn_out_names(outputs, n_thr):
    """None -> every output (those of the thresholds only with n_thr > 0); else the names asked for, in the ABI's order"""
    default = [k for k in PATHFN_OUT_NAMES if k not in PATHFN_NEED_THR or int(n_thr) > 0]
    names = out_names(PATHFN_OUT_NAMES, outputs, default)
    return [k for k in PATHFN_OUT_NAMES if k in names]


def make_pathfn_desc(T, rows, R, D, n_thr=0, storage=0, derive_newcases=0, k0=0, k1=None, test_segments=0,
                     test_launch_groups=0) -> PathfnDesc:
    """storage: 0 / "f64" = double source, 1 / "f32" = float source.  k1 = None: T."""
    d = PathfnDesc()
    d.abi_version = ABI_VERSION
    d.T, d.rows, d.R, d.D, d.n_thr = int(T), int(rows), int(R), int(D), int(n_thr)
    d.storage = {"f64": 0, "f32": 1}.get(storage, storage)
    d.derive_newcases = int(derive_newcases)
    d.k0, d.k1 = int(k0), int(T) if k1 is None else int(k1)
    d.test_segments, d.test_launch_groups = int(test_segments), int(test_launch_groups)
    return d


class EjointDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "T", "rows", "R", "D", "Rt", "storage", "derive_newcases", "k0", "k1", "vs_order",
                                         "max_lag", "test_launch_tiles", "reserved")]


EJOINT_IN_NAMES = ESCORE_IN_NAMES
EJOINT_OUT_NAMES = ("es", "truth_term", "spread_term", "vs", "n_members", "n_days", "member_dist")
EJOINT_OUT_I32 = ("n_members", "n_days")
EJOINT_VS_ORDERS = {0: 0, None: 0, 0.5: 1, 1: 2, 1.0: 2}        # the exponent p of the variogram score -> vs_order


class EjointInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in EJOINT_IN_NAMES]


class EjointOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in EJOINT_OUT_NAMES]


def ejoint_shapes(rows, R, D, derive_newcases=0):
    """shape of every output of epi_ejoint_run_* (rows' = rows + derive_newcases)"""
    ro = int(rows) + int(derive_newcases)
    sh = {k: (ro, R) for k in EJOINT_OUT_NAMES}
    sh["member_dist"] = (ro, R * D)
    return sh


def ejoint_out_names(outputs, vs_order):
    """None -> every output (vs only with vs_order > 0); else the names asked for, in the ABI's order"""
    default = [k for k in EJOINT_OUT_NAMES if k != "vs" or int(vs_order) > 0]
    names = out_names(EJOINT_OUT_NAMES, outputs, default)
    return [k for k in EJOINT_OUT_NAMES if k in names]


def make_ejoint_desc(T, rows, R, D, Rt, vs_order=0, max_lag=0, storage=0, derive_newcases=0, k0=0, k1=None, test_launch_tiles=0) -> EjointDesc:
    """storage: 0 / "f64" = double source, 1 / "f32" = float source.  vs_order: 0 (off), 1 (p = 0.5), 2 (p = 1).  k1 = None: T."""
    d = EjointDesc()
    d.abi_version = ABI_VERSION
    d.T, d.rows, d.R, d.D, d.Rt = int(T), int(rows), int(R), int(D), int(Rt)
    d.storage = {"f64": 0, "f32": 1}.get(storage, storage)
    d.derive_newcases = int(derive_newcases)
    d.k0, d.k1 = int(k0), int(T) if k1 is None else int(k1)
    d.vs_order, d.max_lag, d.test_launch_tiles = int(vs_order), int(max_lag), int(test_launch_tiles)
    return d


class IdiagDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "B", "T", "lane_block", "storage", "flip", "k0", "k1", "n_lags", "reserved")]


IDIAG_IN_NAMES = ("e", "S")
IDIAG_OUT_F64 = ("mean", "var", "skew", "kurt", "jb", "nis_sum", "nis_mean", "lb_q", "het", "cusumsq_max", "max_abs")
IDIAG_OUT_I32 = ("n", "lb_lags", "het_n1", "het_n2", "cusumsq_step", "max_abs_step", "status")
IDIAG_OUT_NAMES = IDIAG_OUT_F64 + IDIAG_OUT_I32 + ("acf",)
IDIAG_BAD_DAY, IDIAG_EMPTY, IDIAG_DEGENERATE, IDIAG_FEW_LAGS = 1, 2, 4, 8          # bits of status


class IdiagInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in IDIAG_IN_NAMES]


class IdiagOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in IDIAG_OUT_NAMES]


def idiag_shapes(B, H):
    sh = {k: (int(B),) for k in IDIAG_OUT_F64 + IDIAG_OUT_I32}
    sh["acf"] = (int(H), int(B))
    return sh


def idiag_out_names(outputs):
    """None -> every output; else the names given, in the ABI's order"""
    if outputs is None:
        return list(IDIAG_OUT_NAMES)
    for k in outputs:
        if k not in IDIAG_OUT_NAMES:
            raise ValueError(f"unknown output {k!r}")
    return [k for k in IDIAG_OUT_NAMES if k in outputs]


def make_idiag_desc(B, T, n_lags=10, k0=0, k1=None, flip=0, lane_block=0, storage=0) -> IdiagDesc:
    d = IdiagDesc()
    d.abi_version = ABI_VERSION
    d.B, d.T, d.lane_block, d.storage, d.flip = int(B), int(T), int(lane_block), int(storage), int(flip)
    d.k0, d.k1, d.n_lags, d.reserved = int(k0), int(T) if k1 is None else int(k1), int(n_lags), 0
    return d


class CdepthDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "T", "rows", "R", "D", "n_alpha", "storage", "derive_newcases", "k0", "k1",
                                         "test_segments", "test_launch_groups")] + [
        ("alpha", C.c_double * 8), ("fence_factor", C.c_double), ("fence_frac", C.c_double)]


CDEPTH_IN_NAMES = ("src", "population", "first_day")
CDEPTH_PATH_F64 = ("depth", "mhi", "band_count", "pair_total")
CDEPTH_PATH_I32 = ("n_valid", "depth_rank", "out_days")
CDEPTH_REGION_I32 = ("n_ranked", "median_path", "n_outliers")
CDEPTH_ENV_NAMES = ("env_lo", "env_hi")
CDEPTH_DAY_NAMES = ("median_curve", "whisk_lo", "whisk_hi")
CDEPTH_OUT_NAMES = CDEPTH_PATH_F64 + CDEPTH_PATH_I32 + CDEPTH_REGION_I32 + CDEPTH_ENV_NAMES + CDEPTH_DAY_NAMES
CDEPTH_OUT_I32 = CDEPTH_PATH_I32 + CDEPTH_REGION_I32
CDEPTH_NEED_FENCE = ("out_days", "n_outliers", "whisk_lo", "whisk_hi")
CDEPTH_DEFAULT_ALPHA, CDEPTH_DEFAULT_FENCE_FACTOR, CDEPTH_DEFAULT_FENCE_FRAC = (0.5, 0.9), 1.5, 0.5


class CdepthInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in CDEPTH_IN_NAMES]


class CdepthOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in CDEPTH_OUT_NAMES]


def cdepth_shapes(T, rows, R, D, n_alpha, derive_newcases=0):
    """shape of every output of epi_cdepth_run_* (rows' = rows + derive_newcases)"""
    ro, N, T, na, R = int(rows) + int(derive_newcases), int(R) * int(D), int(T), int(n_alpha), int(R)
    sh = {k: (ro, N) for k in CDEPTH_PATH_F64 + CDEPTH_PATH_I32}
    sh.update({k: (ro, R) for k in CDEPTH_REGION_I32})
    sh.update({k: (T, na, ro, R) for k in CDEPTH_ENV_NAMES})
    sh.update({k: (T, ro, R) for k in CDEPTH_DAY_NAMES})
    return sh


def cdepth_out_names(outputs, n_alpha, fence_factor):
    """None -> every output (the envelopes only with n_alpha > 0, the boxplot's only with fence_factor > 0); else the names asked
    for, in the ABI's order"""
    default = [k for k in CDEPTH_OUT_NAMES if (k not in CDEPTH_ENV_NAMES or int(n_alpha) > 0)
               and (k not in CDEPTH_NEED_FENCE or float(fence_factor) > 0.0)]
    names = out_names(CDEPTH_OUT_NAMES, outputs, default)
    return [k for k in CDEPTH_OUT_NAMES if k in names]


def make_cdepth_desc(T, rows, R, D, alpha=(), fence_factor=0.0, fence_frac=0.0, storage=0, derive_newcases=0, k0=0, k1=None,
                     test_segments=0, test_launch_groups=0) -> CdepthDesc:
    """storage: 0 / "f64" = double source, 1 / "f32" = float source.  k1 = None: T.  alpha: up to 8 fractions (more: ValueError)."""
    alpha = [float(a) for a in (() if alpha is None else np.atleast_1d(np.asarray(alpha, dtype=np.float64)))]
    if len(alpha) > 8:
        raise ValueError("at most 8 central regions (alpha)")
    d = CdepthDesc()
    d.abi_version = ABI_VERSION
    d.T, d.rows, d.R, d.D, d.n_alpha = int(T), int(rows), int(R), int(D), len(alpha)
    d.storage = {"f64": 0, "f32": 1}.get(storage, storage)
    d.derive_newcases = int(derive_newcases)
    d.k0, d.k1 = int(k0), int(T) if k1 is None else int(k1)
    d.test_segments, d.test_launch_groups = int(test_segments), int(test_launch_groups)
    for k, a in enumerate(alpha):
        d.alpha[k] = a
    d.fence_factor, d.fence_frac = float(fence_factor), float(fence_frac)
    return d


# A family: a batched device call with the three entry points epi_<prefix>_validate / _run_device / _run_host, which take
# (const desc *, args..., tail).  args: the argument types between the descriptor and the tail, the outputs structure last.
Family = namedtuple("Family", "prefix desc args out_names out_i32")
FAMILY_TAILS = {"validate": [C.c_char_p], "run_device": [C.c_void_p, C.c_char_p], "run_host": [C.c_int, C.c_char_p]}
FAMILIES = {f.prefix: f for f in (
    Family("rtwin", RtwinDesc, [C.c_void_p, C.POINTER(RtwinOutputs)], RTWIN_OUT_NAMES, RTWIN_OUT_I32),
    Family("lasso", LassoDesc, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(LassoOutputs)], LASSO_OUT_NAMES, LASSO_OUT_I32),
    Family("robfit", RobfitDesc, [C.c_void_p, C.c_void_p, C.POINTER(RobfitOutputs)], ROBFIT_OUT_NAMES, ROBFIT_OUT_I32),
    Family("ratemap", RatemapDesc, [C.POINTER(RatemapInputs), C.POINTER(RatemapOutputs)], RATEMAP_OUT_NAMES, RATEMAP_OUT_I32),
    Family("mldiv", MldivDesc, [C.POINTER(MldivInputs), C.POINTER(MldivOutputs)], MLDIV_OUT_NAMES, MLDIV_OUT_I32),
    Family("svr", SvrDesc, [C.POINTER(SvrInputs), C.POINTER(SvrOutputs)], SVR_OUT_NAMES, SVR_OUT_I32),
    Family("ens", EnsDesc, [C.c_void_p, C.c_void_p, C.POINTER(EnsOutputs)], ENS_OUT_NAMES, ("count",)),
    Family("arfc", ArfcDesc, [C.POINTER(ArfcInputs), C.POINTER(ArfcOutputs)], ARFC_OUT_NAMES, ("status",)),
    Family("fuse", FuseDesc, [C.POINTER(FuseInputs), C.POINTER(FuseOutputs)], FUSE_OUT_NAMES, ("rank", "status")),
)}


class NnlsDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("abi_version", "S", "D", "n", "max_iters")]


_lib = None


def _preload_torch_hip_runtime() -> None:
    """One HIP runtime per process.  PyTorch wheels bundle their own libamdhip64.so (same SONAME as
    /opt/rocm's); device pointers and streams handed to libepiekf.so come from torch, so the library
    must bind to torch's runtime, whichever of the two is loaded first.  Loading torch's copy by path
    here (no `import torch` needed) makes the dynamic linker resolve libepiekf.so's NEEDED
    libamdhip64.so.7 to it, and a later `import torch` reuses the same mapping.  Without torch in the
    environment (e.g. a MEX host) the system runtime is used."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.origin:
        return
    p = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(p):
        C.CDLL(p, mode=C.RTLD_GLOBAL)


def lib():
    """Load libepiekf.so; raises if absent (build it with __graft_entry__.build())."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found: build the HIP library first "
                              "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
        _preload_torch_hip_runtime()
        h = C.CDLL(LIB_PATH)
        h.epi_status_string.argtypes = [C.c_int]
        h.epi_model_dim.argtypes = [C.c_int]
        h.epi_ekf_validate.argtypes = [C.POINTER(BatchDesc), C.c_char_p]
        h.epi_ekf_workspace_bytes.argtypes = [C.POINTER(BatchDesc)]
        h.epi_ekf_precheck_device.argtypes = [C.POINTER(BatchDesc), C.POINTER(Inputs), C.c_void_p, C.POINTER(C.c_int),
                                              C.c_char_p]
        h.epi_ekf_preferred_lane_block.argtypes = [C.POINTER(BatchDesc)]
        h.epi_ekf_run_device.argtypes = [C.POINTER(BatchDesc), C.POINTER(Inputs), C.POINTER(Outputs), C.c_void_p,
                                         C.c_size_t, C.c_void_p, C.c_char_p]
        h.epi_ekf_time_stages_device.argtypes = [C.POINTER(BatchDesc), C.POINTER(Inputs), C.POINTER(Outputs), C.c_void_p,
                                                 C.c_size_t, C.c_void_p, C.c_double, C.POINTER(C.c_double), C.c_char_p]
        h.epi_ekf_run_host.argtypes = [C.POINTER(BatchDesc), C.POINTER(Inputs), C.POINTER(Outputs), C.c_int,
                                       C.c_char_p]
        h.epi_sialpha_sim_device.argtypes = [C.POINTER(SimDesc)] + [C.c_void_p] * 9 + [C.c_void_p, C.c_char_p]
        h.epi_sialpha_score_device.argtypes = [C.POINTER(SimDesc)] + [C.c_void_p] * 11 + [C.c_void_p, C.c_char_p]
        h.epi_seirp_sim_device.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p]
        h.epi_random_npi_mc_device.argtypes = [C.POINTER(McDesc)] + [C.c_void_p] * 8 + [C.c_void_p, C.c_char_p]
        h.epi_pareto_front_device.argtypes = [C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.c_void_p, C.c_char_p]
        h.epi_npi_cost_device.argtypes = [C.c_int32] * 5 + [C.c_void_p] * 6 + [C.c_void_p, C.c_char_p]
        h.epi_sialpha_sim_host.argtypes = [C.POINTER(SimDesc)] + [C.c_void_p] * 9 + [C.c_int, C.c_char_p]
        h.epi_seirp_sim_host.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p]
        h.epi_si_controlled_device.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_double] + [C.c_void_p] * 5 + [C.c_void_p, C.c_char_p]
        h.epi_si_controlled_host.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_double] + [C.c_void_p] * 5 + [C.c_int, C.c_char_p]
        h.epi_npi_cost_host.argtypes = [C.c_int32] * 5 + [C.c_void_p] * 6 + [C.c_int, C.c_char_p]
        h.epi_rt_expfit_validate.argtypes = [C.POINTER(RtDesc), C.c_char_p]
        h.epi_rt_expfit_run_device.argtypes = [C.POINTER(RtDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtOutputs),
                                               C.c_void_p, C.c_char_p]
        h.epi_rt_expfit_run_host.argtypes = [C.POINTER(RtDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtOutputs),
                                             C.c_int, C.c_char_p]
        h.epi_preprocess_workspace_bytes.argtypes = [C.POINTER(PreDesc)]
        h.epi_preprocess_device.argtypes = [C.POINTER(PreDesc)] + [C.c_void_p] * 4 + [C.POINTER(PreOutputs), C.c_void_p,
                                                                                        C.c_size_t, C.c_void_p, C.c_char_p]
        h.epi_nnls_affine_fit_device.argtypes = [C.POINTER(NnlsDesc)] + [C.c_void_p] * 7 + [C.c_void_p, C.c_char_p]
        h.epi_calib_copy_f64_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p]
        h.epi_ekf_run_host_multi.argtypes = [C.POINTER(BatchDesc), C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_char_p]
        h.epi_sweep_run_device.argtypes = [C.POINTER(BatchDesc), C.POINTER(Inputs), C.POINTER(Outputs), C.c_void_p, C.c_size_t,
                                           C.POINTER(SweepDesc)] + [C.c_void_p] * 7 + [C.c_void_p, C.c_char_p]
        h.epi_sweep_prescribe_host.argtypes = [C.POINTER(PrescribeDesc), C.POINTER(PrescribeInputs), C.POINTER(PrescribeOutputs),
                                               C.c_int, C.POINTER(C.c_int), C.c_char_p]
        h.epi_sir_sim_device.argtypes = [C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p]
        h.epi_sir_sim_host.argtypes = [C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p]
        h.epi_preprocess_host.argtypes = [C.POINTER(PreDesc)] + [C.c_void_p] * 4 + [C.POINTER(PreOutputs), C.c_int, C.c_char_p]
        h.epi_nnls_affine_fit_host.argtypes = [C.POINTER(NnlsDesc)] + [C.c_void_p] * 7 + [C.c_int, C.c_char_p]
        h.epi_random_npi_mc_host.argtypes = [C.POINTER(McDesc)] + [C.c_void_p] * 8 + [C.c_int, C.c_char_p]
        h.epi_lookahead_validate.argtypes = [C.POINTER(LookaheadDesc), C.c_char_p]
        h.epi_lookahead_workspace_bytes.argtypes = [C.POINTER(LookaheadDesc)]
        h.epi_lookahead_run_device.argtypes = [C.POINTER(LookaheadDesc), C.POINTER(LookaheadInputs), C.POINTER(LookaheadOutputs),
                                               C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p]
        h.epi_lookahead_run_host.argtypes = [C.POINTER(LookaheadDesc), C.POINTER(LookaheadInputs), C.POINTER(LookaheadOutputs),
                                             C.c_int, C.c_char_p]
        h.epi_loglik_validate.argtypes = [C.POINTER(LoglikDesc), C.c_char_p]
        h.epi_loglik_workspace_bytes.argtypes = [C.POINTER(LoglikDesc), C.POINTER(C.c_size_t), C.c_char_p]
        h.epi_loglik_run_device.argtypes = [C.POINTER(LoglikDesc), C.POINTER(LoglikInputs), C.POINTER(LoglikOutputs),
                                            C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p]
        h.epi_loglik_run_host.argtypes = [C.POINTER(LoglikDesc), C.POINTER(LoglikInputs), C.POINTER(LoglikOutputs),
                                          C.c_int, C.c_char_p]
        h.epi_plan_validate.argtypes = [C.POINTER(PlanDesc), C.c_char_p]
        h.epi_plan_workspace_bytes.argtypes = [C.POINTER(PlanDesc), C.POINTER(C.c_size_t), C.c_char_p]
        h.epi_plan_run_device.argtypes = [C.POINTER(PlanDesc), C.POINTER(PlanInputs), C.POINTER(PlanOutputs),
                                          C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p]
        h.epi_plan_run_host.argtypes = [C.POINTER(PlanDesc), C.POINTER(PlanInputs), C.POINTER(PlanOutputs), C.c_int, C.c_char_p]
        h.epi_sdraw_validate.argtypes = [C.POINTER(SdrawDesc), C.c_char_p]
        h.epi_sdraw_workspace_bytes.argtypes = [C.POINTER(SdrawDesc), C.POINTER(C.c_size_t), C.c_char_p]
        h.epi_sdraw_run_device.argtypes = [C.POINTER(SdrawDesc), C.POINTER(SdrawInputs), C.POINTER(SdrawOutputs),
                                           C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p]
        h.epi_sdraw_run_host.argtypes = [C.POINTER(SdrawDesc), C.POINTER(SdrawInputs), C.POINTER(SdrawOutputs), C.c_int, C.c_char_p]
        h.epi_escore_validate.argtypes = [C.POINTER(EscoreDesc), C.POINTER(EscoreInputs), C.POINTER(EscoreOutputs), C.c_char_p]
        h.epi_escore_workspace_bytes.argtypes = [C.POINTER(EscoreDesc), C.POINTER(C.c_size_t), C.c_char_p]
        h.epi_escore_run_device.argtypes = [C.POINTER(EscoreDesc), C.POINTER(EscoreInputs), C.POINTER(EscoreOutputs),
                                            C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p]
        h.epi_escore_run_host.argtypes = [C.POINTER(EscoreDesc), C.POINTER(EscoreInputs), C.POINTER(EscoreOutputs), C.c_int, C.c_char_p]
        h.epi_pathfn_validate.argtypes = [C.POINTER(PathfnDesc), C.POINTER(PathfnInputs), C.POINTER(PathfnOutputs), C.c_char_p]
        h.epi_pathfn_workspace_bytes.argtypes = [C.POINTER(PathfnDesc), C.POINTER(C.c_size_t), C.c_char_p]
        h.epi_pathfn_run_device.argtypes = [C.POINTER(PathfnDesc), C.POINTER(PathfnInputs), C.POINTER(PathfnOutputs),
                                            C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p]
        h.epi_pathfn_run_host.argtypes = [C.POINTER(PathfnDesc), C.POINTER(PathfnInputs), C.POINTER(PathfnOutputs), C.c_int, C.c_char_p]
        h.epi_ejoint_validate.argtypes = [C.POINTER(EjointDesc), C.POINTER(EjointInputs), C.POINTER(EjointOutputs), C.c_char_p]
        h.epi_ejoint_workspace_bytes.argtypes = [C.POINTER(EjointDesc), C.POINTER(C.c_size_t), C.c_char_p]
        h.epi_ejoint_run_device.argtypes = [C.POINTER(EjointDesc), C.POINTER(EjointInputs), C.POINTER(EjointOutputs),
                                            C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p]
        h.epi_ejoint_run_host.argtypes = [C.POINTER(EjointDesc), C.POINTER(EjointInputs), C.POINTER(EjointOutputs), C.c_int, C.c_char_p]
        h.epi_idiag_validate.argtypes = [C.POINTER(IdiagDesc), C.c_char_p]
        h.epi_idiag_workspace_bytes.argtypes = [C.POINTER(IdiagDesc), C.POINTER(C.c_size_t), C.c_char_p]
        h.epi_idiag_run_device.argtypes = [C.POINTER(IdiagDesc), C.POINTER(IdiagInputs), C.POINTER(IdiagOutputs),
                                           C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p]
        h.epi_idiag_run_host.argtypes = [C.POINTER(IdiagDesc), C.POINTER(IdiagInputs), C.POINTER(IdiagOutputs),
                                         C.c_int, C.c_char_p]
        h.epi_cdepth_validate.argtypes = [C.POINTER(CdepthDesc), C.POINTER(CdepthInputs), C.POINTER(CdepthOutputs), C.c_char_p]
        h.epi_cdepth_workspace_bytes.argtypes = [C.POINTER(CdepthDesc), C.POINTER(C.c_size_t), C.c_char_p]
        h.epi_cdepth_run_device.argtypes = [C.POINTER(CdepthDesc), C.POINTER(CdepthInputs), C.POINTER(CdepthOutputs),
                                            C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p]
        h.epi_cdepth_run_host.argtypes = [C.POINTER(CdepthDesc), C.POINTER(CdepthInputs), C.POINTER(CdepthOutputs), C.c_int, C.c_char_p]
        for f in FAMILIES.values():
            for kind, tail in FAMILY_TAILS.items():
                getattr(h, f"epi_{f.prefix}_{kind}").argtypes = [C.POINTER(f.desc)] + f.args + tail
        nd = C.POINTER(NoiseDesc)                   # the seeded siblings: the noise descriptor behind the call's own
        h.epi_noise_validate.argtypes = [nd, C.c_char_p]
        fill = [nd, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_void_p]
        h.epi_noise_fill_device.argtypes = fill + [C.c_int32, C.c_void_p, C.c_char_p]
        h.epi_noise_fill_host.argtypes = fill + [C.c_int, C.c_char_p]
        for name in ("epi_sdraw_run_device", "epi_sdraw_run_host", "epi_arfc_run_device", "epi_arfc_run_host", "epi_sialpha_sim_device",
                     "epi_sialpha_score_device", "epi_sialpha_sim_host", "epi_random_npi_mc_device", "epi_random_npi_mc_host"):
            at = getattr(h, name).argtypes
            getattr(h, name + "_seeded").argtypes = [at[0], nd] + list(at[1:])
        own = ("epi_status_string", "epi_host_pool_release", "epi_ekf_workspace_bytes", "epi_preprocess_workspace_bytes",
               "epi_lookahead_workspace_bytes")
        h.epi_status_string.restype = C.c_char_p
        h.epi_host_pool_release.restype = None
        h.epi_ekf_workspace_bytes.restype = h.epi_preprocess_workspace_bytes.restype = h.epi_lookahead_workspace_bytes.restype = C.c_size_t
        for name in ABI_SYMBOLS:                    # every other symbol returns an int
            if name not in own:
                getattr(h, name).restype = C.c_int
        if h.epi_abi_version() != ABI_VERSION:
            raise ImportError("libepiekf.so ABI version mismatch")
        _lib = h
    return _lib


def check(rc: int, err_buf) -> None:
    if rc != 0:
        msg = err_buf.value.decode(errors="replace") if err_buf is not None and err_buf.value else \
            lib().epi_status_string(rc).decode()
        raise EpiError(rc, msg)


def make_lookahead_desc(R, LL, F, M, n_npi, L_, order=1, obs_type="NEWCASES", r_mode=1, shape=0, placement_tries=0,
                        model="SIAlphaModelEKF") -> LookaheadDesc:
    d = LookaheadDesc()
    d.abi_version = ABI_VERSION
    d.model = L.MODEL_IDS[model] if isinstance(model, str) else int(model)
    d.R, d.LL, d.F, d.M, d.n_npi, d.L, d.order = int(R), int(LL), int(F), int(M), int(n_npi), int(L_), int(order)
    d.obs_type = L.OBS_IDS.get(obs_type, 99) if isinstance(obs_type, str) else int(obs_type)
    d.r_mode, d.shape, d.placement_tries = int(r_mode), int(shape), int(placement_tries)
    return d


def rtwin_methods(methods) -> int:
    """("LogLinReg", "GenRatios", "NonlinLS") names (any subset) or an int of EPI_RTWIN_* bits -> the bits"""
    if isinstance(methods, (int, np.integer)):
        return int(methods)
    if isinstance(methods, str):
        methods = (methods,)
    return sum(RTWIN_METHODS[m] for m in set(methods))


def make_rtwin_desc(R, L_, wlen, time_unit=1.0, causal=1, generation_period=None, methods=7) -> RtwinDesc:
    d = RtwinDesc()
    d.abi_version = ABI_VERSION
    d.R, d.L, d.wlen, d.causal = int(R), int(L_), int(wlen), int(causal)
    d.generation_period = 0 if generation_period is None else int(generation_period)
    d.methods = rtwin_methods(methods)
    d.time_unit = float(time_unit)
    return d


def make_desc(model, B, T, Sx, Su, n_npi, L_, order, obs_type, r_mode, out_mask, q_mode=0) -> BatchDesc:
    d = BatchDesc()
    d.abi_version = ABI_VERSION
    d.model = L.MODEL_IDS[model] if isinstance(model, str) else int(model)
    d.B, d.T, d.Sx, d.Su, d.n_npi, d.L, d.order = int(B), int(T), int(Sx), int(Su), int(n_npi), int(L_), int(order)
    if isinstance(obs_type, str):
        d.obs_type = L.OBS_IDS.get(obs_type, 99)   # unknown strings reach the library's own check
    else:
        d.obs_type = int(obs_type)
    d.r_mode, d.q_mode, d.out_mask, d.phase = int(r_mode), int(q_mode), int(out_mask), 0
    d.path_hint, d.time_pipe, d.lane_block, d.shape, d.storage, d.exact_nonfinite = 0, 0, 0, 0, 0, 0
    d.placement_tries, d.test_window, d.test_flags = 0, 0, 0
    return d

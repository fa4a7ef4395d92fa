/*
 * epiekf.h -- C ABI of libepiekf.so: the MI355X (gfx950) ensemble engine for the
 * reference's per-region EKF/EKS hot path.
 *
 * Drop-in boundary.  The reference's interface for this path is a family of
 * MATLAB functions with one signature (Tools/SIAlphaModelEKF.m:1,
 * Tools/SIAlphaModelEKFOptControlled.m:1, Tools/SIAlphaModelBackwardEKF.m:1,
 * Tools/SIAlphaModelBackwardEKFOptControlled.m:1,
 * Tools/NewCaseEKFEstimatorWithOptimalNPI.m:1):
 *
 *   [u_opt, u_opt_smooth, S_MINUS, S_PLUS, S_SMOOTH, P_MINUS, P_PLUS, P_SMOOTH,
 *    K_GAIN, innovations, rho] = F(u, x, params, s_init, Ps_init, s_final,
 *    Ps_final, w_bar, v_bar, Q_w, R_v, beta, gamma, inv_monitor_len, order)
 *
 * A MEX gateway / ctypes stub binds exactly the entry points below (see
 * INTEGRATION.md).  One call runs B independent filter chains ("chains" =
 * region x cost-factor x Monte-Carlo member); B = 1 with the identity series
 * maps reproduces one reference call, and with B = 1 every array below has
 * exactly MATLAB's column-major memory layout (u: n_npi x T, S: m x T,
 * P: m x m x T), so a gateway can pass mxGetPr() pointers straight through.
 *
 * Memory layout (batched, "SoA"): time-major, then row, then chain:
 *   x         [T][Sx]            observations; NaN = missing (GenericEKF.m:122)
 *   u         [T][n_npi][Su]     controls; NaN = "choose optimally" (OptControlled.m:49-58)
 *   R_series  [T][Sx]            R_v given as 1xT vector (fixed_R = false, GenericEKF.m:82-85)
 *   R_scalar  [B]                R_v given as a scalar   (fixed_R = true,  GenericEKF.m:79-81)
 *   prm       [EPI_PRM_COUNT][B] params struct + v_bar/beta/gamma (epiekf_layout.h)
 *   s_init    [m][B]   Ps_init [m*m][B]   s_final [m][B]   Ps_final [m*m][B]   Q [m*m][B]
 *   outputs   S_* [T][m][B], P_* [T][m*m][B] (element e = row + m*col), K_GAIN [T][m][B],
 *             u_opt* [T][n_npi][B], innovations/rho [T][B]
 * Chain c reads column x_series[c] of x / R_series and column u_series[c] of u
 * (NULL map = identity, then Sx resp. Su must equal B): the Pareto sweep's 250
 * cost factors of one region share that region's series
 * (Tools/TrainPredictPrescribeNPI.m:421-460).
 *
 * Ownership / threading / errors: the caller owns every buffer; the library
 * never frees or retains caller memory; every entry point may be called from
 * several threads at once; all device work of a *_device call is enqueued on
 * the caller's stream (stages that are off the critical path run on a helper
 * stream that is forked from and joined back into the caller's stream, so the
 * call behaves like work on that one stream, also under stream capture: a
 * helper stream that joined a caller's capture is not handed to any other call
 * afterwards -- it is retired until epi_host_pool_release()).
 * What the library keeps between calls, all of it freed by
 * epi_host_pool_release(): the CU count of each device it has seen, idle
 * helper streams (one per concurrent call and device, with their events), and
 * for the *_host entry points a pool of contexts per device (stream, device
 * arena, pinned staging buffer) and one worker thread per device used by the
 * *_multi calls.  EVERY *_host entry point, the simulators and small fits
 * included, runs on such a context: its kernels on the context's stream, which
 * alone it waits for, one copy each way, no allocation once the arena is large
 * enough, and the calling thread's current device as it found it.
 * Return value 0 or a negative epi_status; `err` (256 bytes,
 * may be NULL) receives the reference's own error() text for the four
 * reference errors.
 */
#ifndef EPIEKF_H
#define EPIEKF_H

#include <stddef.h>
#include <stdint.h>
#include "epiekf_layout.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EPIEKF_ABI_VERSION 6

/* which reference function the chain runs */
typedef enum epi_model {
    EPI_MODEL_SIA3 = 0,          /* Tools/SIAlphaModelEKF.m                      (m = 3) */
    EPI_MODEL_SIA6 = 1,          /* Tools/SIAlphaModelEKFOptControlled.m         (m = 6) */
    EPI_MODEL_SIA3_BWD = 2,      /* Tools/SIAlphaModelBackwardEKF.m              (m = 3) */
    EPI_MODEL_SIA6_BWD = 3,      /* Tools/SIAlphaModelBackwardEKFOptControlled.m (m = 6) */
    EPI_MODEL_NEWCASE6 = 4,      /* Tools/NewCaseEKFEstimatorWithOptimalNPI.m    (m = 6) */
    EPI_MODEL_NEWCASE6_CODEGEN = 5 /* MatlabCodeGenerator/NewCaseEKFEstimatorWithOptimalNPI.m */
} epi_model;

typedef enum epi_obs_type {      /* params.obs_type, Tools/SIAlphaModelEKF.m:52-58 */
    EPI_OBS_NEWCASES = 0,
    EPI_OBS_TOTALCASES = 1
} epi_obs_type;

typedef enum epi_status {
    EPI_OK = 0,
    EPI_ERR_UNDEFINED_ORDER = -1, /* 'Undefined order'  GenericExtendedKalmanFilter.m:111,151 */
    EPI_ERR_Q_MISMATCH = -2,      /* 'Process noise covariance noise mismatch'      :75 */
    EPI_ERR_R_MISMATCH = -3,      /* 'Observation noise covariance noise mismatch'  :90 */
    EPI_ERR_OBS_TYPE = -4,        /* 'unknown observation type'  SIAlphaModelEKF.m:57,87 */
    EPI_ERR_BAD_ARG = -5,         /* NULL / size / range error in the descriptor */
    EPI_ERR_WORKSPACE = -6,       /* workspace too small */
    EPI_ERR_HIP = -7,             /* HIP runtime failure (no device, launch error, ...) */
    EPI_ERR_UNSUPPORTED = -8
} epi_status;

/* output selection bits, in the order of the reference's output list */
typedef enum epi_out {
    EPI_OUT_U_OPT = 1 << 0,
    EPI_OUT_U_OPT_SMOOTH = 1 << 1,
    EPI_OUT_S_MINUS = 1 << 2,
    EPI_OUT_S_PLUS = 1 << 3,
    EPI_OUT_S_SMOOTH = 1 << 4,
    EPI_OUT_P_MINUS = 1 << 5,
    EPI_OUT_P_PLUS = 1 << 6,
    EPI_OUT_P_SMOOTH = 1 << 7,
    EPI_OUT_K_GAIN = 1 << 8,
    EPI_OUT_INNOVATIONS = 1 << 9,
    EPI_OUT_RHO = 1 << 10,
    EPI_OUT_ALL = (1 << 11) - 1
} epi_out;

typedef struct epi_batch_desc {
    int32_t abi_version;  /* EPIEKF_ABI_VERSION */
    int32_t model;        /* epi_model */
    int32_t B;            /* chains */
    int32_t T;            /* time samples  = size(x, 2) */
    int32_t Sx, Su;       /* distinct observation / control series */
    int32_t n_npi;        /* size(u, 1), 1..EPI_MAX_NPI */
    int32_t L;            /* inv_monitor_len */
    int32_t order;        /* 1 or 2 (2 is accepted: all SI-alpha Hessian callbacks are zero,
                             Tools/SIAlphaModelEKF.m:92-109) */
    int32_t obs_type;     /* epi_obs_type */
    int32_t r_mode;       /* 0: R_scalar[B] (scalar R_v, adaptive when beta != 1); 1: R_series */
    int32_t q_mode;       /* 0: fixed per-chain m x m Q_w, Q [m*m][B] (the only form the reference's callers use);
                             1: time-varying, Q [T][m*m][B] = Q(:,:,k) of filter step k (GenericEKF.m:63-73; a
                                length-T vector Q_w is q(k)*eye(m)); generic models only, dense kernels */
    uint32_t out_mask;    /* epi_out bits: which outputs are written */
    int32_t phase;        /* 0: forward EKF then backward EKS (one reference call).  For per-kernel timing a
                             caller may enqueue the stages one by one, in order, on the same buffers:
                             1 = forward kernel; 2 = smoother (3 then 4); 3 = pinv kernel; 4 = backward recursion */
    int32_t path_hint;    /* kernels of the generic (symmetrising) models: 0 = decide on the device (both the
                             symmetric-packed and the dense variant are enqueued, one returns at once);
                             1 = epi_ekf_precheck_device() said the batch qualifies for the symmetric-packed
                             kernels (Ps_init bit-wise symmetric, Q_w diagonal): enqueue only those;
                             2 = dense kernels only */
    int32_t time_pipe;    /* a full call (phase 0) of a generic model on the packed kernels (path_hint = 1, R_v a per-day
                             series, T >= 128) may run "pipelined in time": the forward kernel in four time segments (50, 35,
                             12, 3 % of the days), each followed by the eks_pinv grid of its days on a helper stream, so that
                             only the last days' pinv stands between the forward pass and the smoother.  0 = the library
                             decides (on when the batch leaves a quarter of the SIMDs idle -- the shards of the sweep on 2,
                             4, 8 GPUs), 1 = on, -1 = off.  Results are bit-identical either way. */
    int32_t lane_block;   /* layout of the OUTPUT arrays (and of the workspace) of epi_ekf_run_device.  0 or >= B: the
                             classic [T][rows][B].  blk in 1..B-1 (8 recommended): chain-blocked,
                             element (t, row, c) at ((t*nblk + c/blk)*rows + row)*blk + c%blk, nblk = ceil(B/blk) --
                             the rows of blk neighbouring chains form one contiguous block, which is what HBM wants
                             to see from ~100 concurrent stores per wave; arrays are then sized for
                             nblk*blk chains and one-row arrays (innovations, rho, pinv_rank) are [T][nblk*blk].
                             Inputs are never blocked.  epi_ekf_run_host accepts the classic layout only. */
    int32_t shape;        /* how the 6-state generic models are mapped to lanes (epi_shape): 0 = decide by batch size,
                             1 = one lane per chain (ekf_fwd_sym / eks_bwd_sym: least total work, what a batch that fills
                             the chip wants), 2 = four lanes per chain (ekf_fwd_quad / eks_bwd_quad: every 6 x 6 matrix as
                             a 2 x 2 grid of 3 x 3 blocks over a DPP quad; a ~2x shorter per-day instruction stream and
                             4x the wavefronts, what a batch that does NOT fill the chip wants -- DESIGN.md 4),
                             3 = one WAVEFRONT per chain (ekf_fwd_wave / eks_bwd_wave: lane e = i + 6 j owns element (i, j) of
                             every 6 x 6 matrix, operands exchanged through LDS; the shortest per-day latency, for batches of
                             at most one chain per SIMD -- the reference's own one-call-per-cost-weight loop; needs R_v as a
                             per-day series, else falls back to 2), 4 = SIX lanes per chain, ten chains per wavefront
                             (ekf_fwd_hex / eks_bwd_hex: lane j of a chain owns column j of every 6 x 6 matrix; the stored
                             covariances are symmetric bit for bit, so every product needs one transpose through LDS and the
                             Jacobian's zeros are skipped -- about half the quad shape's instructions per day; same conditions
                             as 3, except that a scalar R_v falls back to 2).  Auto: 3 up to 640 chains (up to 1 024 with a
                             scalar R_v, whose monitor the wave shape runs inline), 4 up to 20 480 (the 9 375-chain shard of the
                             headline sweep on one of 8 GPUs: 2.6 ms against 3.2 with 2 and 4.9 with 1), 2 up to 16 384 where 4
                             cannot run, then 1.
                             The 3-state generic models know 1 and 3 (there: SEVEN chains per wavefront, nine lanes each,
                             ekf_fwd_wave3 / eks_bwd_wave3; auto: 3 up to 2 048 chains).  Results are bit-identical in all
                             shapes.  NewCaseEKFEstimatorWithOptimalNPI knows 1 (the dense kernels) and 3 (auto: 3 up to 1 024 chains). */
    int32_t storage;      /* element type of the OUTPUT arrays: 0 = fp64 (the reference's), 1 = fp32 storage with fp64
                             register arithmetic (BASELINE config 5): every selected output is the fp64 result rounded
                             once to fp32; the forward quantities the smoother reads back stay fp64 in the workspace.
                             epi_ekf_run_device only. */
    int32_t exact_nonfinite; /* What happens to chains whose covariance overflows (status bit 0: the non-finite guard of
                             GenericEKF.m:211 fired).  The packed, quad and hex kernels skip products with structural zeros,
                             which is exact only for finite operands: after an overflow they may carry a finite number where
                             MATLAB has NaN.  0 (the default, ABI 5) = the reference's behaviour whenever the call runs the
                             smoother: the marked chains are run a second time by the dense kernels, in place, so that their
                             Inf / NaN pattern is the dense evaluation's -- the reference's, and the C oracle's -- at every
                             day; 1 = the same, and the smoother is run to find the chains even when no smoothed output is
                             selected; -1 = off, the outputs are what the fast kernels leave (`status` still tells which
                             chains).  Generic models, full call (phase 0), fixed Q_w, fp64 storage.  Cost when no chain is
                             marked: six small launches that return at once (~25 us; until ABI 4 the second pass's pinv grid
                             dispatched every (tile, step) workgroup -- 0.15 ms at 75 000 x 520 -- now it is 8 tiles wide and
                             walks the list of marked chains); (2 B + 1 + B) more int32 of workspace.  The *_host entry points
                             reach the same result without device-side launches: epi_ekf_run_host[_multi] look at the status
                             words that come back with the outputs and enqueue the second pass only when a chain is marked. */
    int32_t placement_tries; /* HOST-pointer entry points only (ABI 6; the device-pointer entry points ignore it: their caller owns
                             the allocation and can compare allocations with epi_ekf_time_stages_device).  Where the allocator
                             puts the ~14 arrays a pass streams concurrently changes the time of the forward kernel and of the
                             smoother by 5-15 % -- a property of the allocation, invisible to a caller who hands over host
                             arrays.  N > 1: when the call has to allocate a NEW device arena, its own kernels are timed on up to
                             N (<= EPI_PLACEMENT_MAX_TRIES) candidate arenas and the fastest is kept, with the pooled context,
                             for the calls that follow (epi_host_pool_release frees it); epi_outputs.placement receives the
                             report.  0 / 1 = off.  Cost: once per arena, ~N + 1 times the call's device time. */
    /* TEST HOOKS (ABI 6; until ABI 5 an environment variable read on every call).  Both are 0 in production: a default-
       constructed descriptor never sets them, nothing else in the library reads process-global state.  They only choose
       code paths that the batch size otherwise chooses, so that small tests reach them; results are identical for every value. */
    int32_t test_window;  /* > 0: the kernels that keep their buffer descriptors fixed over an addressing window of days (the hex
                             shape, ekf_hex.hpp; the one-lane kernels of ekf_lane6.hpp) use windows of at most that many days
                             (>= 2) instead of as many as fit 2 GiB.  It can only SHORTEN the window. */
    int32_t test_flags;   /* bit 0: a full call in the hex shape takes the reverse-time pipeline (pinv grids of the earlier days
                             beside the smoother's first launches) whatever the batch size and day count, which otherwise
                             engages beyond 768 hex wavefronts and 128 days only.
                             bit 1: the innovation monitor's scan kernel (ekf_monitor) replays rho whatever the batch size; below
                             65 537 chains the scan-free grid (ekf_monitor_par) otherwise does.
                             bit 2: a one-lane batch is cut into two chain ranges in the middle of its waves -- forward kernel,
                             pinv grid (the first range's beside the second forward launch) and, on the fixed-descriptor
                             smoother, the smoother with the monitor between its launches -- as batches of more waves than SIMDs
                             are cut after their first round of resident waves. */
} epi_batch_desc;

typedef enum epi_shape { EPI_SHAPE_AUTO = 0, EPI_SHAPE_LANE = 1, EPI_SHAPE_QUAD = 2, EPI_SHAPE_WAVE = 3, EPI_SHAPE_HEX = 4 } epi_shape;

typedef struct epi_inputs {
    const int32_t *x_series; /* [B] or NULL */
    const int32_t *u_series; /* [B] or NULL */
    const double *x, *u, *R_series, *R_scalar, *prm;
    const double *s_init, *Ps_init, *s_final, *Ps_final, *Q;
} epi_inputs;

#define EPI_PLACEMENT_MAX_TRIES 8
typedef struct epi_placement_report {
    int32_t tries;        /* candidate arenas timed; 0 = none (placement_tries <= 1, or the call reused a pooled arena) */
    int32_t chosen;       /* the one kept */
    float ms[EPI_PLACEMENT_MAX_TRIES];   /* device time of the call's kernels on each candidate */
} epi_placement_report;

typedef struct epi_outputs {
    double *u_opt, *u_opt_smooth;
    double *S_MINUS, *S_PLUS, *S_SMOOTH;
    double *P_MINUS, *P_PLUS, *P_SMOOTH;
    double *K_GAIN, *innovations, *rho;
    /* extras (not reference outputs; may be NULL) */
    int32_t *pinv_rank;   /* [T][B] rank kept by pinv at smoother step k (-1: not executed / guard) */
    int32_t *status;      /* [B] per-chain flags: bit0 non-finite P_MINUS guard hit (GenericEKF.m:211),
                             bit1 Jacobi sweep cap reached, bits 8.. minimum pinv rank seen */
    epi_placement_report *placement;   /* host-pointer entry points: what placement_tries > 1 did (may be NULL) */
} epi_outputs;

/* ---- EKF / EKS ---------------------------------------------------------- */
int epi_model_dim(int model);                                   /* 3, 6 or -1 */
int epi_ekf_validate(const epi_batch_desc *d, char *err);       /* descriptor checks only, no GPU */
size_t epi_ekf_workspace_bytes(const epi_batch_desc *d);        /* device scratch a run needs */
/* Synchronous: (forward + monitor, pinv grid, smoother) milliseconds -- ms[3] -- of this call on THESE device arrays, enqueued
 * stage by stage between HIP events on `stream`, averaged over as many rounds as fill `min_ms` of device time after one untimed
 * round.  For comparing ALLOCATIONS: the same arrays give the same times run after run, another allocation of the same arrays
 * may be 5-15 % slower (where its physical pages fall); a caller that will run many passes times one, allocates again while
 * holding the first, and keeps the faster (what placement_tries does for the host-pointer entry points). */
int epi_ekf_time_stages_device(const epi_batch_desc *d, const epi_inputs *in, const epi_outputs *out, void *workspace,
                               size_t workspace_bytes, void *stream, double min_ms, double *ms, char *err);
/* Synchronous: inspects Ps_init / Q (device pointers) and reports in *fast_ok whether path_hint = 1 is valid. */
int epi_ekf_precheck_device(const epi_batch_desc *d, const epi_inputs *in, void *stream, int *fast_ok, char *err);

/* The lane_block that matches the way epi_ekf_run_device will launch this batch on the current device: the number of
 * chains one wavefront handles (64, or fewer when the launch is split into equally full rounds; 16 where the 6-state
 * models run four lanes per chain, see `shape`).  With it every
 * wavefront's loads and stores of a step are one contiguous piece per array -- the fastest of the blocked layouts
 * (DESIGN.md 3).  Returns 0 for an invalid descriptor. */
int epi_ekf_preferred_lane_block(const epi_batch_desc *d);

/* All pointers in `in`/`out`/`workspace` are DEVICE pointers on the current HIP
 * device; `stream` is a hipStream_t (NULL = default stream).  Asynchronous:
 * returns after enqueueing.  Outputs not selected in out_mask may be NULL.
 * Alignment: every array needs the alignment of its element only (8 bytes for the fp64 arrays, 4 for int32 and fp32
 * storage), a slice of a larger allocation included.  The smoothers that fetch P_PLUS and X with 16-byte-per-lane LDS-DMA
 * (eks_bwd_lane6, eks_bwd_hex) give the same bits on arrays 8 bytes off a 16-byte boundary
 * (tests/test_gpu_addressing_limits.py).
 * Limits (epi_ekf_validate): B, Sx, Su and B rounded up to lane_block <= 2^23; each is run at its value there. */
int epi_ekf_run_device(const epi_batch_desc *d, const epi_inputs *in, const epi_outputs *out,
                       void *workspace, size_t workspace_bytes, void *stream, char *err);

/* Same call on HOST pointers (what a MEX gateway calls): copies in, runs, copies the selected outputs back and
 * synchronises.  Replaces one call of Tools/SIAlphaModelEKF.m:1 (B = 1) or a whole loop of them
 * (Tools/TrainPredictPrescribeNPI.m:421-460, B = 250 cost weights).  Classic layout only (lane_block = 0).
 * Device memory, a pinned staging buffer and a stream come from a per-device pool of contexts that lives as long as the
 * library (no hipMalloc / hipFree per call after the first): a call whose inputs + outputs fit the staging buffer
 * (64 MiB) moves them with ONE host-to-device and ONE device-to-host copy.  Thread-safe. */
int epi_ekf_run_host(const epi_batch_desc *d, const epi_inputs *in, const epi_outputs *out,
                     int device, char *err);

/* The same on SEVERAL GPUs of the node: the B chains are cut into n_devices contiguous blocks
 * (block r = chains [r * ceil(B / n_devices), ...), a shorter or empty last block), one host thread per block uploads
 * its chains, runs them on device_ids[r] (NULL: devices 0 .. n_devices-1) and writes the out_mask-selected outputs
 * straight into the caller's arrays -- chains are independent, so there is no exchange between the devices; this is the
 * loop over regions / cost weights of Tools/TrainPredictPrescribeNPI.m:93,421 spread over the GPUs.  A device may be
 * named more than once (two blocks then share it).  Returns the first error of any block. */
int epi_ekf_run_host_multi(const epi_batch_desc *d, const epi_inputs *in, const epi_outputs *out,
                           int n_devices, const int *device_ids, char *err);

/* Frees everything the library keeps between calls: pooled host contexts (device arenas, pinned buffers, streams), idle
 * helper streams and their events, and the *_multi worker threads.  Optional: call before unloading the library.  Not to be
 * called while another thread is inside a library call. */
void epi_host_pool_release(void);

/* ---- forward simulators and cost (Tools/SIalpha_Controlled.m, SEIRP.m, NPICost.m) ---- */
typedef struct epi_sim_desc {
    int32_t abi_version;
    int32_t B;        /* chains */
    int32_t K;        /* steps */
    int32_t Su;       /* distinct control series */
    int32_t n_npi;
    int32_t noise;    /* 0: noise-free; 1: z given [K][3][B] standard normal draws */
    int32_t with_cost;/* 1: also J0/J1 of NPICost over the simulated span */
    int32_t prefix_days; /* epi_sialpha_score_device: days already summed into J0_prefix / J1_prefix */
    int32_t u_block;  /* 0 or >= Su: u is [K][n_npi][Su]; otherwise u is chain-blocked like an output of
                         epi_ekf_run_device with lane_block = u_block (u_opt_smooth fed straight into the scoring) */
} epi_sim_desc;

/* SIalpha_Controlled.m:1-32 batched.  sp [EPI_SIM_PRM_COUNT][B]; u [K][n_npi][Su];
 * outputs s,i,alpha [K][B] (initial sample dropped, :30-32); J0,J1 [B] when with_cost:
 * J0 = mean(s.*i.*alpha), J1 = mean(weights.*u) with weights [n_npi][B] constant over time. */
enum {
    EPI_SIM_S0 = 0, EPI_SIM_I0, EPI_SIM_ALPHA0, EPI_SIM_ALPHA_MIN, EPI_SIM_ALPHA_MAX, EPI_SIM_GAMMA,
    EPI_SIM_B, EPI_SIM_BETA, EPI_SIM_S_STD, EPI_SIM_I_STD, EPI_SIM_ALPHA_STD, EPI_SIM_DT,
    EPI_SIM_A = 12,      /* a(1:12)     */
    EPI_SIM_U_MAX = 24,  /* u_max(1:12) */
    EPI_SIM_W = 36,      /* NPICost weights(1:12), constant over time */
    EPI_SIM_PRM_COUNT = 48
};
int epi_sialpha_sim_device(const epi_sim_desc *d, const int32_t *u_series, const double *u,
                           const double *sp, const double *z, double *s, double *i, double *alpha,
                           double *J0, double *J1, void *stream, char *err);

/* Scenario scoring of the Pareto sweep (Tools/TrainPredictPrescribeNPI.m:481-493): simulate the horizon under the
 * smoothed optimal control from the end-of-history state and return NPICost over [historic days, horizon days].
 * J0_prefix[B] / J1_prefix[B] hold the sequential sums over the `prefix_days` historic days of
 * s.*i.*alpha and of weights(:).*inputs(:) (column-major order); the kernel continues both sums in order, so
 * J0 = mean([newcases_hist, newcases_sim]) and J1 = mean(weights.*[u_hist, u_sim]) exactly as NPICost.m:6-10. */
int epi_sialpha_score_device(const epi_sim_desc *d, const int32_t *u_series, const double *u, const double *sp,
                             const double *z, const double *J0_prefix, const double *J1_prefix, double *s, double *i,
                             double *alpha, double *J0, double *J1, void *stream, char *err);

/* Tools/NPICost.m:1-10 batched over B chains: J0 = mean(newcases), J1 = mean(weights(:).*inputs(:)), both summed
 * sequentially in MATLAB's column-major element order (NPI index fastest, then time).  newcases [T][B];
 * inputs [T][n_npi][Su] with u_series [B] or NULL (identity, Su == B); weights [T][n_npi][B] when
 * weights_per_day != 0, else [n_npi][B] (the same weights every day, as TrainPredictPrescribeNPI.m:485-493 builds
 * them).  J0, J1 [B]. */
int epi_npi_cost_device(int32_t B, int32_t T, int32_t n_npi, int32_t Su, int32_t weights_per_day,
                        const int32_t *u_series, const double *newcases, const double *inputs, const double *weights,
                        double *J0, double *J1, void *stream, char *err);

/* Random-NPI Monte-Carlo scenarios of a region (Tools/TrainPredictPrescribeNPI.m:496-521): n_scen plans on the K
 * forecast days with u(jj,t) = randi([NPI_MINS(jj), NPI_MAXES(jj)]) -- scenarios with 1-based index < n_scen/2 are
 * constant over time (:502), the rest are redrawn every day -- each simulated with SIalpha_Controlled from the
 * end-of-history state and scored with NPICost over [historic days, forecast days] (u = cat(2, IP, u), :515-517).
 * Chain c = scenario * R + region.  sp [EPI_SIM_PRM_COUNT][R] per region (EPI_SIM_U_MAX rows are NPI_MAXES);
 * u_min [n_npi][R] = NPI_MINS; z [K][3][n_scen*R] standard-normal draws when noise != 0, else NULL;
 * J0_prefix/J1_prefix [R]: sequential sums over the prefix_days historic days (as for epi_sialpha_score_device;
 * NULL when prefix_days == 0); u_out [K][n_npi][n_scen*R] or NULL; J0, J1 [n_scen][R].
 * The integer draws come from Philox4x32-10 keyed by (seed_lo, seed_hi) with counter (region, scenario, NPI/4, day):
 * reproducible on any launch geometry and by the CPU oracle; MATLAB's own randi stream is not reproduced. */
typedef struct epi_mc_desc {
    int32_t abi_version;
    int32_t R;          /* regions */
    int32_t n_scen;     /* scenarios per region (500 in the reference) */
    int32_t K;          /* forecast days */
    int32_t n_npi;
    int32_t noise;
    int32_t prefix_days;
    uint32_t seed_lo, seed_hi;
} epi_mc_desc;
int epi_random_npi_mc_device(const epi_mc_desc *d, const double *sp, const double *u_min, const double *z,
                             const double *J0_prefix, const double *J1_prefix, double *u_out, double *J0, double *J1,
                             void *stream, char *err);

/* Pareto-front filter and optimum of the sweep (Tools/TrainPredictPrescribeNPI.m:624-633), per region:
 * on_front(ii) = (sum(J0 < J0(ii) & J1 < J1(ii)) == 0);  [~, I_opt] = min((J0/max(J0)).^2 + (J1/max(J1)).^2).
 * J0, J1 [R][P] (region-major -- the chain order of the sweep); on_front [R][P] (0/1) or NULL; i_opt [R] 0-based or
 * NULL.  P <= 8192 (the points of a region are staged in LDS); any R (one workgroup per region, launched in slices of 2^22
 * regions: the thread count of one launch is a 32-bit number). */
int epi_pareto_front_device(int32_t R, int32_t P, const double *J0, const double *J1, int32_t *on_front,
                            int32_t *i_opt, void *stream, char *err);

/* ---- the Pareto sweep over the NPI-cost weights as ONE call (Tools/TrainPredictPrescribeNPI.m:421-493, 624-633) ----
 * The reference walks `for ll = 1 : num_pareto_front_points` (:421): SIAlphaModelEKFOptControlled with
 * params.epsilon = human_npi_cost_factor(ll) (:460), SIalpha_Controlled over the horizon under opt_control_input_smooth from
 * the end-of-history state (:481), NPICost over [historic, horizon] (:493); after the loop the non-dominated points and
 * I_opt (:624-633).  epi_sweep_run_device is epi_ekf_run_device (same descriptor, inputs, outputs, workspace; model
 * EPI_MODEL_SIA6, phase ignored = full call, fp64 u_opt_smooth selected) followed by epi_sialpha_score_device on the last
 * T - t_hist days of the u_opt_smooth it wrote and, when on_front / i_opt are given, epi_pareto_front_device -- enqueued so
 * that scoring and filter run BESIDE the smoother's pass over the observed days (the horizon's u_opt_smooth is final after
 * the smoother's first T - 1 - t_hist steps; packed kernels, path_hint = 1; otherwise they follow it).  Results are
 * bit-identical to the three separate calls.
 *   sp [EPI_SIM_PRM_COUNT][B], J0_prefix / J1_prefix [B]: as for epi_sialpha_score_device (EPI_SIM_S0.. = s/i/alpha_historic
 *   (end), prefix_days = t_hist);  J0, J1 [B];  on_front [R][P] / i_opt [R] or NULL (both NULL: no filter -- a shard of the
 *   sweep that does not hold whole regions; then R, P are ignored). */
typedef struct epi_sweep_desc {
    int32_t abi_version;
    int32_t R;        /* regions of this call */
    int32_t P;        /* cost weights per region: chain c = region * P + ll, B == R * P */
    int32_t t_hist;   /* NumNPIdays: observed days; the T - t_hist days after them are the horizon, 1 <= t_hist < T */
} epi_sweep_desc;
int epi_sweep_run_device(const epi_batch_desc *d, const epi_inputs *in, const epi_outputs *out, void *workspace,
                         size_t workspace_bytes, const epi_sweep_desc *sd, const double *sp, const double *J0_prefix,
                         const double *J1_prefix, double *J0, double *J1, int32_t *on_front, int32_t *i_opt, void *stream,
                         char *err);

/* The same from HOST pointers and PER-REGION inputs, for all regions at once and on several GPUs (what a MEX gateway
 * binds: matlab/epiekf_pipeline_mex.cpp; replaces the two loops Tools/TrainPredictPrescribeNPI.m:93 and :421 around the
 * 6-state filter).  The host sends R columns (a few hundred KB), the device expands them to the R * P chains, runs
 * filter -> scoring -> front filter, and returns (J0, J1) per chain, the front, I_opt and the optimum's plan per region --
 * a few MB instead of the 5.6 - 49 GB of per-chain filter outputs.  Regions are cut into n_devices contiguous blocks (whole
 * regions, so the front filter needs no exchange); device_ids NULL = devices 0 .. n_devices-1.
 * Inputs (host, region-minor: a MATLAB R x rows matrix is the [rows][R] array):
 *   x [T][R], u [T][n_npi][R] (NaN over the horizon), R_series [T][R];
 *   prm [EPI_PRM_COUNT][R] (row EPI_PRM_EPSILON is ignored), s_init [6][R], Ps_init [36][R], s_final [6][R],
 *   Ps_final [36][R], Q [36][R];  eps [P] = human_npi_cost_factor;
 *   sp [EPI_SIM_PRM_COUNT][R], J0_prefix / J1_prefix [R]  (scoring inputs, see epi_sialpha_score_device).
 * Outputs (host; any may be NULL):
 *   J0, J1 [R][P];  on_front [R][P];  i_opt [R] (0-based);
 *   u_opt [T][n_npi][R] = u_opt_smooth of chain (r, i_opt[r]);  S_opt [T][6][R] = its S_SMOOTH;
 *   extras: per-chain filter outputs selected by out_mask, classic layout [T][rows][R * P] (pinv_rank / status are not
 *   returned); with out_mask != 0 the filter writes the classic layout and the call pays PCIe for what it selects. */
typedef struct epi_prescribe_desc {
    int32_t abi_version;
    int32_t R, P;            /* regions, cost weights per region */
    int32_t T, t_hist;       /* days incl. the horizon; observed days */
    int32_t n_npi, L, order, obs_type;
    uint32_t out_mask;       /* epi_out bits of the per-chain extras (0 = none) */
    int32_t shape, time_pipe;/* as in epi_batch_desc (0 = let the library decide) */
    int32_t placement_tries; /* as in epi_batch_desc: N > 1 = a new device arena is the fastest of up to N candidates */
} epi_prescribe_desc;
typedef struct epi_prescribe_inputs {
    const double *x, *u, *R_series;
    const double *prm, *s_init, *Ps_init, *s_final, *Ps_final, *Q;
    const double *eps;
    const double *sp, *J0_prefix, *J1_prefix;
} epi_prescribe_inputs;
typedef struct epi_prescribe_outputs {
    double *J0, *J1;
    int32_t *on_front, *i_opt;
    double *u_opt, *S_opt;
    epi_outputs extras;
    epi_placement_report *placement;   /* what placement_tries > 1 did on the first device's block (may be NULL) */
} epi_prescribe_outputs;
int epi_sweep_prescribe_host(const epi_prescribe_desc *d, const epi_prescribe_inputs *in, const epi_prescribe_outputs *out,
                             int n_devices, const int *device_ids, char *err);

/* ---- the forecast look-ahead error study (Tools/ForecastQualityAssessment.m:359-393, 428-449) as ONE call ----
 * For every region r and every start s = 1 .. F (F = num_forecast_days) the reference masks the last s observations with
 * NaN, runs SIAlphaModelEKF (the 3-state model, EPI_MODEL_SIA3) and compares N * s * i * alpha of S_PLUS and of S_SMOOTH with
 * the smoothed new cases over the hidden tail.  Here all R * F chains run as one batch: chain c = r * F + (s - 1) (the chain
 * order of synth.make_mask_ensemble); the device expands the per-region inputs, runs the filter and smoother, and reduces.
 * Inputs (region-minor, the layouts of epi_inputs with B = R):  x [LL][R] observations (NaN = missing), u [LL][n_npi][R]
 *   controls, R_series [LL][R] (r_mode 1) or R_scalar [R] (r_mode 0), prm [EPI_PRM_COUNT][R], s_init [3][R], Ps_init [9][R],
 *   s_final [3][R], Ps_final [9][R], Q [9][R];  truth [LL][R] = NewCasesSmoothed_ENTIRE (not normalised);  population [R].
 * Outputs:  est_plus / est_smooth [F][M][R] = EstError_PLUS / EstError_SMOOTH (M = MaxLookAheadDays): row s, column
 *   j = 1 .. min(s, M) is, at day t = LL - s + j - 1 (0-based), est = ((N * S(t,1)) * S(t,2)) * S(t,3) and
 *   (100 * |truth - est|) / truth (IEEE Inf / NaN where truth is 0 are kept); columns j > min(s, M) are 0 (`zeros`);
 *   mean_* / median_* / std_* [M][R]: statistics of each column over the rows s = M .. F (n = F - M + 1): mean = sum in
 *   increasing s / n, std = sqrt(sum((x - mean)^2) / (n - 1)) (0 for n = 1), median = NaN if any value is NaN, else the
 *   middle order statistic (odd n) or a + (b - a) / 2 of the two middle ones, (a + b) / 2 when they differ in sign or one is
 *   infinite (even n); n <= 0 (F < M) gives NaN in all three.
 *   Optional (NULL = not returned): S_PLUS / S_SMOOTH [LL][3][R * F] of every chain, status [R * F] (epi_outputs.status).
 * epi_lookahead_run_device takes DEVICE pointers and enqueues on `stream` (no host synchronisation); the workspace holds the
 * masked per-chain inputs (x, R_v and the per-chain columns of prm / s_init / ... / Q) and the filter's own workspace.
 * epi_lookahead_run_host takes HOST pointers and runs on a pooled context of `device` (as epi_ekf_run_host). */
typedef struct epi_lookahead_desc {
    int32_t abi_version;
    int32_t model;           /* EPI_MODEL_SIA3 (the reference's study runs SIAlphaModelEKF); anything else: EPI_ERR_UNSUPPORTED */
    int32_t R;               /* regions */
    int32_t LL;              /* days of the whole window */
    int32_t F;               /* num_forecast_days: starts 1 .. F, 1 <= F <= min(LL, 1024) */
    int32_t M;               /* MaxLookAheadDays, >= 1 */
    int32_t n_npi, L, order, obs_type, r_mode;   /* as in epi_batch_desc */
    int32_t shape;           /* lane mapping of the filter: 0 = the study decides, 1 = one lane per chain, 3 = seven chains per
                                wavefront (epi_batch_desc.shape; results are bit-identical) */
    int32_t placement_tries; /* as in epi_batch_desc (epi_lookahead_run_host only) */
} epi_lookahead_desc;
typedef struct epi_lookahead_inputs {
    const double *x, *u, *R_series, *R_scalar, *prm;
    const double *s_init, *Ps_init, *s_final, *Ps_final, *Q;
    const double *truth, *population;
} epi_lookahead_inputs;
typedef struct epi_lookahead_outputs {
    double *est_plus, *est_smooth;                              /* [F][M][R] */
    double *mean_plus, *median_plus, *std_plus;                 /* [M][R] */
    double *mean_smooth, *median_smooth, *std_smooth;           /* [M][R] */
    double *S_PLUS, *S_SMOOTH;                                  /* [LL][3][R * F] or NULL */
    int32_t *status;                                            /* [R * F] or NULL */
} epi_lookahead_outputs;
int epi_lookahead_validate(const epi_lookahead_desc *d, char *err);
size_t epi_lookahead_workspace_bytes(const epi_lookahead_desc *d);
int epi_lookahead_run_device(const epi_lookahead_desc *d, const epi_lookahead_inputs *in, const epi_lookahead_outputs *out,
                             void *workspace, size_t workspace_bytes, void *stream, char *err);
int epi_lookahead_run_host(const epi_lookahead_desc *d, const epi_lookahead_inputs *in, const epi_lookahead_outputs *out,
                           int device, char *err);

/* ---- the sliding-window growth-rate estimators Tools/Rt_ExpFitLogLinReg.m, Rt_ExpFitGenRatios.m, Rt_ExpFitNonlinLS.m ----
 * Any subset of the three over R series of L days in ONE call.  Input new_cases [L][R] (day-major, region-minor: the
 * new_smoothed layout of epi_preprocess_device).  Every output is [L][R]; NULL = not wanted.  Days mm are 1-based below.
 * Windows: causal n = -wlen+1 .. 0, mm = wlen .. L;  centred h = floor(wlen/2), n = -h .. h (2h + 1 samples, wlen + 1 for an
 * even wlen), mm = h+1 .. L-h.
 *   LogLinReg (bit 0): seg = log(window); En = mean(n), En2 = mean(n.^2), Det = En2 - En^2 (means: sequential sum / count);
 *     ALog = (mean(seg) En2 - mean(n.*seg) En) / Det, r = (mean(n.*seg) - mean(seg) En) / Det, 0 outside the windows;
 *     Rt = exp(r), A = exp(ALog), Lambda = r / time_unit, ExpFit = A .* Rt.  log(0) = -Inf and NaN propagate.
 *   GenRatios (bit 1): Lambda = [zeros(1,gp), log(x(1+gp:L) ./ x(1:L-gp))] / gp; LambdaSmoothed = filter(ones(1,wlen), wlen,
 *     Lambda) in the operation order of preprocessing's moving average; Rt = exp(Lambda time_unit), RtSmoothed = exp(
 *     LambdaSmoothed time_unit).  `causal` does not apply.
 *   NonlinLS (bit 2): A starts as filter([zeros(1,wlen-1),1], 1, x) (causal: 0 before day wlen) or x (centred), r as 0.  A
 *     window with fewer than wlen samples ~= 0 (NaN counts as non-zero) keeps A(mm) = x(mm), r(mm) = 0 (status SKIPPED);
 *     every other window is fitted with nlinfit's Levenberg-Marquardt (y = A exp(lambda t), t = n / time_unit, start
 *     [x(mm), 0], TolX = TolFun = 1e-6, MaxIter 250; NaN samples dropped; our reading in DESIGN.md §4.4).  Where MATLAB
 *     raises an error (the model is Inf / NaN, fewer than 2 samples left) the window's status is MODEL_ERROR and A = r = NaN.
 *     Rt = exp(r), Lambda = r / time_unit, ExpFit = A .* Rt; status / iters [L][R] int32 (iters = LM iterations run).
 * log and exp are evaluated in a fixed operation order (epi_log / epi_exp) that tests/rt_window_ref.c shares: results are
 * reproducible bit for bit.  epi_rtwin_run_device takes DEVICE pointers and enqueues on `stream` (no host synchronisation);
 * epi_rtwin_run_host takes HOST pointers and runs on a pooled context of `device`. */
enum { EPI_RTWIN_LOGLINREG = 1, EPI_RTWIN_GENRATIOS = 2, EPI_RTWIN_NONLINLS = 4 };
enum {
    EPI_RTWIN_OUTSIDE = 0,       /* day outside the window range: the initial A and r */
    EPI_RTWIN_TOLX = 1,          /* converged: norm(step) < TolX (sqrt(eps) + norm(beta)) */
    EPI_RTWIN_TOLFUN = 2,        /* converged: |sse - sseold| <= TolFun sse */
    EPI_RTWIN_MAXITER = 3,       /* 250 iterations reached */
    EPI_RTWIN_STALL = 4,         /* lambda passed 1e16 without an SSE that does not increase */
    EPI_RTWIN_SKIPPED = 5,       /* fewer than wlen non-zero samples: A = x(mm), r = 0 */
    EPI_RTWIN_MODEL_ERROR = 6    /* MATLAB's error (model Inf / NaN, too few samples): A = r = NaN */
};
typedef struct epi_rtwin_desc {
    int32_t abi_version;
    int32_t R;                   /* series (regions), >= 1 */
    int32_t L;                   /* days, >= 1 */
    int32_t wlen;                /* window length, 2 .. 31 (else EPI_ERR_UNSUPPORTED) */
    int32_t causal;              /* 1 causal, 0 centred (LogLinReg, NonlinLS) */
    int32_t generation_period;   /* GenRatios: 1 .. L */
    int32_t methods;             /* EPI_RTWIN_* bits, != 0 */
    double time_unit;
} epi_rtwin_desc;
typedef struct epi_rtwin_outputs {
    double *llr_Rt, *llr_A, *llr_Lambda, *llr_ExpFit;                        /* LogLinReg */
    double *gr_Rt, *gr_Lambda, *gr_RtSmoothed, *gr_LambdaSmoothed;           /* GenRatios */
    double *nls_Rt, *nls_A, *nls_Lambda, *nls_ExpFit;                        /* NonlinLS */
    int32_t *nls_status, *nls_iters;
} epi_rtwin_outputs;
/* no GPU needed: EPI_ERR_BAD_ARG for a bad descriptor or a NULL descriptor / new_cases / outputs, EPI_ERR_UNSUPPORTED for wlen
 * outside 2 .. 31 */
int epi_rtwin_validate(const epi_rtwin_desc *d, const double *new_cases, const epi_rtwin_outputs *out, char *err);
int epi_rtwin_run_device(const epi_rtwin_desc *d, const double *new_cases, const epi_rtwin_outputs *out, void *stream, char *err);
int epi_rtwin_run_host(const epi_rtwin_desc *d, const double *new_cases, const epi_rtwin_outputs *out, int device, char *err);

/* ---- REGRESSION_TYPE = 'LASSO' between the EKF rounds: [B, FitInfo] = lasso(X, y, 'CV', K), a = B(:, IndexMinMSE),
 * b = FitInfo.Intercept(IndexMinMSE) (TrainPredictPrescribeNPI.m:254-290, ForecastQualityAssessment.m:256-292) ----
 * For each of R regions: X [D][n][R] (= NPI_MAXES - InterventionPlans over the regression window, the layout of
 * epi_nnls_affine_fit_device), y [D][R], fold [D][R] int32 in 0 .. K-1 (the cross-validation partition, given by the
 * caller; may be NULL when K = 0).  Alpha = 1, Standardize = true, DFmax = Inf, no weights.  Our reading of lasso, point
 * by point and in the operation order the kernel and tests/lasso_ref.c share bit for bit, is DESIGN.md §4.5.
 * Outputs (NULL = not wanted, except status; a and b are required when K >= 2); lambda index k is ASCENDING (MATLAB's
 * order), indices are 0-based:
 *   lambda [NL][R], B [NL][n][R] (original scale), intercept [NL][R], df [NL][R] (non-zero B), iters [NL][R] (coordinate
 *   cycles of the full fit), mse / se [NL][R] (K >= 2), idx_min_mse / idx_1se [R], a [n][R], b [R], status [R].
 * A region whose X or y holds a non-finite value gets status NONFINITE, NaN outputs, df = iters = 0 and indices -1; so does
 * a region whose fold holds a value outside 0 .. K-1 or leaves a fold empty (BAD_FOLDS: epi_lasso_run_device cannot read
 * the partition without a host synchronisation; epi_lasso_run_host checks it first and returns EPI_ERR_BAD_ARG).
 * epi_lasso_run_device takes DEVICE pointers and enqueues one wavefront per region on `stream` (no host synchronisation);
 * epi_lasso_run_host takes HOST pointers and runs on a pooled context of `device`. */
enum {
    EPI_LASSO_OK = 0,
    EPI_LASSO_NULL_MODEL = 1,    /* lambdaMax = 0 (every column constant, or y constant): Lambda = 0, B = 0, Intercept = mean(y) */
    EPI_LASSO_MAXITER = 2,       /* some fit reached max_iter cycles at some lambda: its last iterate is kept */
    EPI_LASSO_NONFINITE = 3,     /* X or y holds Inf / NaN: NaN outputs */
    EPI_LASSO_BAD_FOLDS = 4      /* fold value outside 0 .. K-1, or an empty fold: NaN outputs */
};
typedef struct epi_lasso_desc {
    int32_t abi_version;
    int32_t R;                   /* regions, >= 1 */
    int32_t D;                   /* days, 2 .. 256 (else EPI_ERR_UNSUPPORTED above 256) */
    int32_t n;                   /* predictors (NPIs), 1 .. 12 */
    int32_t K;                   /* folds: 0 = path only, or 2 .. min(D, 63) (EPI_ERR_UNSUPPORTED above 63) */
    int32_t num_lambda;          /* NumLambda, 1 .. 100 (MATLAB's default 100) */
    double lambda_ratio;         /* LambdaRatio, in (0, 1) (1e-4) */
    double rel_tol;              /* RelTol, > 0 (1e-4) */
    int32_t max_iter;            /* MaxIter per lambda, >= 1 (1e5) */
} epi_lasso_desc;
typedef struct epi_lasso_outputs {
    double *a, *b;                          /* [n][R], [R]: the fit at IndexMinMSE */
    double *lambda, *B, *intercept;         /* [NL][R], [NL][n][R], [NL][R] */
    int32_t *df;                            /* [NL][R] */
    double *mse, *se;                       /* [NL][R] */
    int32_t *iters;                         /* [NL][R] */
    int32_t *idx_min_mse, *idx_1se;         /* [R] */
    int32_t *status;                        /* [R] EPI_LASSO_*, required */
} epi_lasso_outputs;
/* no GPU needed: EPI_ERR_BAD_ARG for a bad descriptor or a NULL descriptor / X / y / fold (K >= 2) / outputs / status /
 * a / b (K >= 2), EPI_ERR_UNSUPPORTED for n > 12, D > 256, K > 63 or num_lambda > 100 */
int epi_lasso_validate(const epi_lasso_desc *d, const double *X, const double *y, const int32_t *fold,
                       const epi_lasso_outputs *out, char *err);
int epi_lasso_run_device(const epi_lasso_desc *d, const double *X, const double *y, const int32_t *fold,
                         const epi_lasso_outputs *out, void *stream, char *err);
int epi_lasso_run_host(const epi_lasso_desc *d, const double *X, const double *y, const int32_t *fold,
                       const epi_lasso_outputs *out, int device, char *err);

/* ---- Monte-Carlo ensemble statistics: the distribution over the D draws of every region (BASELINE config 5) ----
 * src [T][rows][B] is an output array of the filter in the classic layout (S_SMOOTH, S_PLUS, ...: double, or float when the
 * filter ran with storage = 1), B = R * D chains, region-major: chain = r * D + d (synth.make_cfg5).  An item is one (day t,
 * row, region r) with the D members v[d] = src[t][row][r * D + d], widened to double.  With derive_newcases = 1 (rows >= 3,
 * population [R] given) one row is appended after the source's: ((N_r * v0) * v1) * v2 of rows 0, 1, 2 of the same chain and
 * day.  NaN members are excluded, n = the others (+-Inf take part); x(1 .. n) = the members ascending.  Per item:
 *   count = n;  min = x(1), max = x(n);
 *   quantile at p (MATLAB's quantile / prctile, NumPy's method="hazen"): h = n * p + 0.5, k = floor(h), g = h - k;
 *     x(1) if k < 1, x(n) if k >= n, else x(k) + g * (x(k+1) - x(k));
 *   mean = tree(v) / n, std = sqrt(tree(dev .* dev) / (n - 1)) with dev = v - mean (0 when n = 1), where tree() is the
 *     pairwise sum in draw order: excluded members and the padding to P (the power of two >= D) are +0.0, then
 *     a[i] = a[i] + a[i + h] for i < h, h = P/2, P/4, .., 1, and the sum is a[0];
 *   n = 0: every statistic is NaN.
 * One IEEE rounding per written operation: results are reproducible bit for bit, up to the sign of a zero.
 * Outputs (NULL = not wanted, except count): mean, std, min, max, count [T][rows'][R], quantiles [T][n_q][rows'][R],
 * rows' = rows + derive_newcases.  epi_ens_run_device takes DEVICE pointers and enqueues one wavefront per item on `stream`
 * (no host synchronisation); epi_ens_run_host takes HOST pointers and runs on a pooled context of `device`. */
typedef struct epi_ens_desc {
    int32_t abi_version;
    int32_t T;                   /* days, >= 1 */
    int32_t rows;                /* rows of src, >= 1 */
    int32_t R;                   /* regions, >= 1 */
    int32_t D;                   /* draws per region, 1 .. 4096; R * D <= INT32_MAX */
    int32_t n_q;                 /* quantiles, 1 .. 16 */
    int32_t storage;             /* element type of src: 0 = double, 1 = float (epi_batch_desc.storage) */
    int32_t derive_newcases;     /* 0, or 1: append the row ((N * row0) * row1) * row2 */
    double q[16];                /* probabilities, each finite and in [0, 1]; the first n_q are read */
} epi_ens_desc;
typedef struct epi_ens_outputs {
    double *mean, *std, *min, *max;         /* [T][rows'][R] */
    double *quantiles;                      /* [T][n_q][rows'][R] */
    int32_t *count;                         /* [T][rows'][R], required */
} epi_ens_outputs;
/* no GPU needed: EPI_ERR_BAD_ARG for anything outside the limits above or a NULL descriptor / src / population
 * (derive_newcases) / outputs / count */
int epi_ens_validate(const epi_ens_desc *d, const void *src, const double *population, const epi_ens_outputs *out, char *err);
int epi_ens_run_device(const epi_ens_desc *d, const void *src, const double *population, const epi_ens_outputs *out,
                       void *stream, char *err);
int epi_ens_run_host(const epi_ens_desc *d, const void *src, const double *population, const epi_ens_outputs *out,
                     int device, char *err);

/* ---- The autoregressive alpha forecaster as a Monte-Carlo batch: Tools/PrescribeNPI.m:204-215 ----
 *   ar_sys = ar(seg, p);  zi = filtic(sqrt(nv), A, seg(end:-1:1));  y = filter(sqrt(nv), A, randn(1, H), zi)';
 *   AlphaHat = [seg ; y + drive]';  AlphaHat(AlphaHat < 0) = 0;  [s, i] = SI_Controlled(AlphaHat, beta, s0, i0, L + H, dt)
 * for R regions x D draws, chain c = r * D + d (region-major: what epi_ens_run_* consumes), B = R * D, K = L + H.
 * Fit (fit = 1): ar's default, the forward-backward approach without windowing or mean removal.  A = [1, a_1 .. a_p]
 *   minimises sum_{t = p+1 .. L} (y(t) + sum_k a_k y(t-k))^2 + (y(t-p) + sum_k a_k y(t-p+k))^2, solved as ONE stacked
 *   least-squares problem of M = 2 (L - p) rows (forward rows first, t ascending, then the backward rows) by Householder QR,
 *   never by the normal equations.  A region with some |r_jj| <= max(M, p) * eps * (largest 2-norm of an original column)
 *   gets status EPI_ARFC_RANK_DEFICIENT: its A, noise variance and every row of S from day L on are NaN.  Nothing is thrown.
 *   Noise variance: nv_mode 0 = (forward RSS + backward RSS) / (2 (L - p)), 1 = forward RSS / (L - p).  WHICH VALUE MATLAB's
 *   ar RETURNS AS NoiseVariance IS NOT PINNED BY ANYTHING IN THE REFERENCE (its normalisation is undocumented); a caller who
 *   needs MATLAB's own model passes it in:
 * Given model (fit = 0): A [p][R] (a_1 .. a_p, without the leading 1) and noise_var [R] are inputs: get(ar_sys, 'A')(2:end),
 *   get(ar_sys, 'NoiseVariance').  A region whose model holds a non-finite number is NaN from day L on.
 * Forecast: b0 = sqrt(nv); y(t) = b0 z(t) - sum_{k=1..p} a_k y(t-k), one fma chain with k ascending, the past taken from the
 *   unclamped segment first: filter() with filtic()'s state to rounding, not bit for bit.  z [H][B] standard-normal draws are
 *   an INPUT (NULL = zeros: the deterministic continuation).  drive [H][Sd] (NULL = none), picked by drive_series [B] (NULL:
 *   Sd == B), is added to y before the clamp: the caller's gamma * (u' * a + b).  alpha_hat = [seg ; y + drive] with every
 *   negative entry set to 0.  Then SI_Controlled.m:19-22 statement for statement, in the same kernel.
 * A non-finite entry of seg gives status EPI_ARFC_BAD_INPUT and NaN in every row of S of the region on every day; its A_out and
 * noise_var_out are NaN with fit = 1 and, with fit = 0, the copies of the given model they always are in that mode.
 * The arithmetic is pinned (restated in tests/ar_forecast_ref.c): results are reproducible bit for bit.
 * Outputs: S [K][3][B], rows (s, i, alpha_hat), the filter outputs' layout (epi_ens_run_* with derive_newcases appends
 * ((N s) i) alpha unchanged); A_out [p][R], noise_var_out [R], status [R].  With fit = 1 the fit hands its model to the
 * simulation THROUGH A_out and noise_var_out (the call allocates nothing), so they are required then; with fit = 0 they are
 * optional copies of the inputs.  status is always optional.
 * Limits: 1 <= p <= 32, p + 1 <= L, L - p <= 256, 2 (L - p) >= p + 1, H >= 1, R * D <= INT32_MAX. */
#define EPI_ARFC_OK 0
#define EPI_ARFC_RANK_DEFICIENT 1
#define EPI_ARFC_BAD_INPUT 2
typedef struct epi_arfc_desc {
    int32_t abi_version;
    int32_t R, D;                /* regions, draws per region */
    int32_t L, p, H;             /* segment length, order, horizon */
    int32_t fit;                 /* 1 = fit the model on seg, 0 = A and noise_var are given */
    int32_t nv_mode;             /* fit = 1: 0 = (fRSS + bRSS) / (2 (L - p)), 1 = fRSS / (L - p) */
    int32_t Sd;                  /* series of drive (read when drive != NULL) */
    int32_t reserved;            /* 0 */
    double dt;
} epi_arfc_desc;
typedef struct epi_arfc_inputs {
    const double *seg;           /* [L][R] */
    const double *beta, *s0, *i0;/* [R] */
    const double *z;             /* [H][B] or NULL */
    const double *drive;         /* [H][Sd] or NULL */
    const int32_t *drive_series; /* [B], each in 0 .. Sd-1, or NULL (Sd == B) */
    const double *A;             /* [p][R] (fit = 0) */
    const double *noise_var;     /* [R] (fit = 0) */
} epi_arfc_inputs;
typedef struct epi_arfc_outputs {
    double *S;                   /* [L + H][3][B], required */
    double *A_out;               /* [p][R] */
    double *noise_var_out;       /* [R] */
    int32_t *status;             /* [R] */
} epi_arfc_outputs;
/* no GPU needed: EPI_ERR_BAD_ARG with a message for anything outside the limits or a missing array; nothing is clipped */
int epi_arfc_validate(const epi_arfc_desc *d, const epi_arfc_inputs *in, const epi_arfc_outputs *out, char *err);
/* DEVICE pointers; two kernels (ar_fit with fit = 1, ar_simulate) enqueued on `stream`: no host synchronisation, no allocation */
int epi_arfc_run_device(const epi_arfc_desc *d, const epi_arfc_inputs *in, const epi_arfc_outputs *out, void *stream, char *err);
/* HOST pointers, on a pooled context of `device` */
int epi_arfc_run_host(const epi_arfc_desc *d, const epi_arfc_inputs *in, const epi_arfc_outputs *out, int device, char *err);

/* ---- The forward-backward filter fusion: Tools/TrainPredictPrescribeNPI.m:464-478 ("Backward filtering (under test)") ----
 *   P_FRW_BCK(:,:,hh) = (P_PLUS_f + P_PLUS_b) \ (P_PLUS_f * P_PLUS_b);
 *   S_FRW_BCK(:,hh)   = pinv(P_PLUS_f + P_PLUS_b) * (P_PLUS_b * S_PLUS_f + P_PLUS_f * S_PLUS_b);
 * for every (chain c, day t) of two filter runs, m = 3 or 6, one independent item each: what the reverse-time models
 * (EPI_MODEL_*_BWD) exist for.  The call takes four arrays (sf, Pf) and (sb, Pb) and does not care which filter outputs they are:
 * forward S_PLUS / P_PLUS with backward S_MINUS / P_MINUS counts day t's observation once (the two-filter smoother's choice),
 * PLUS with PLUS is the reference's.
 * Off the commuting case the reference's two lines are NOT the two-filter smoother, P = Pf S^-1 Pb, s = Pb S^-1 sf + Pf S^-1 sb
 * with S = Pf + Pb: they write S^-1 (Pf Pb) and S^-1 (Pb sf + Pf sb), which agree with it only when Pf, Pb and S^-1 commute.
 * Both are built, and `form` is required (neither is a default of this ABI).
 * Arithmetic (pinned; restated in tests/two_filter_ref.py).  Double throughout, one rounding per written
 * operation; every inner product is acc = a_0 b_0, acc = acc + a_k b_k with k ascending (no fma).
 *   S(i,j) = Pf(i,j) + Pb(i,j) for i <= j, mirrored: only the upper triangles of Pf and Pb enter S.
 *   Any non-finite entry of S, sf or sb: every output of the item is NaN, rank = -1, bit 0 of status[c] is set and the
 *   pseudo-inverse is not evaluated.
 *   X = pinv(S): the smoother's symmetric pseudo-inverse (MATLAB's rule, tol = m eps(max singular value)), the two-sided Jacobi
 *   route for an S that is not positive semi-definite up to rounding; rank = the rank kept; bit 1 of status[c] is set if a Jacobi
 *   iteration hit its sweep cap.
 *   form 0:  w = Pb sf + Pf sb (two matrix-vector products over the matrices as stored, one add per row);  s = X w;
 *            C = Pf Pb;  P = S \ C evaluated as (C' / S')' by the library's mrdivide (p_solver 0) or P = X C (p_solver 1).
 *            P is not symmetrised: the reference does not.  PARITY UNPINNED: p_solver 0 is MATLAB's general square path (dgetf2 +
 *            dgetrs); for an exactly symmetric S with a positive diagonal MATLAB's backslash would try a Cholesky factorisation
 *            first, and nothing in the reference pins which path ran.
 *   form 1:  s = Pb (X sf) + Pf (X sb);  Y = X Pb;  P = Pf Y;  P = (P + P') / 2 (GenericExtendedKalmanFilter.m:138).
 *            p_solver must be 0.
 *   d2 = e' (X e), e = sf - sb, summed with i ascending: the squared Mahalanobis distance between the two estimates, the
 *   consistency check the forward-against-backward plots of :592-598 were drawn for.
 * Layout: sf, sb, s_out have m rows, Pf, Pb, P_out m*m rows (entry (i, j) in row i + m j), each in the filter outputs' layout,
 *   element (t, row, c) at ((t * nblk + c / blk) * rows + row) * blk + c % blk, blk = lane_block, nblk = ceil(B / blk);
 *   lane_block 0 or B is the classic [T][rows][B].  The chain-blocked outputs of epi_ekf_run_* are consumed in place.  The
 *   padding lanes of a last, partial block are never read; epi_fuse_run_device does not write them, epi_fuse_run_host (which
 *   moves whole arrays) overwrites them with zeros in s_out / P_out.  d2, rank are [T][B], status [B], never blocked.
 * storage 0 / 1: sf, Pf, sb, Pb, s_out, P_out are double / float arrays; a float is widened on load and a result rounded once on
 *   store.  d2, rank, status are always double / int32 / int32.  No output may overlap an input.
 * Every output is optional; at least one of s_out / P_out / d2 is required.  status is zeroed by the call and accumulated with
 * an atomic OR over the days. */
typedef struct epi_fuse_desc {
    int32_t abi_version;
    int32_t m;                   /* 3 or 6 */
    int32_t B, T;                /* chains, days */
    int32_t lane_block;          /* 0 or B: classic; else chains per layout block */
    int32_t storage;             /* 0 = double, 1 = float */
    int32_t form;                /* 0 = the reference as written, 1 = the information form; required */
    int32_t p_solver;            /* form 0: 0 = S \ C (LU), 1 = pinv(S) * C; form 1: 0 */
    int32_t reserved;            /* 0 */
} epi_fuse_desc;
typedef struct epi_fuse_inputs {
    const void *sf, *Pf;         /* [T][nblk][m][blk], [T][nblk][m*m][blk] */
    const void *sb, *Pb;
} epi_fuse_inputs;
typedef struct epi_fuse_outputs {
    void *s_out, *P_out;         /* as sf, Pf; each may be NULL */
    double *d2;                  /* [T][B] or NULL */
    int32_t *rank;               /* [T][B] or NULL */
    int32_t *status;             /* [B] or NULL */
} epi_fuse_outputs;
/* no GPU needed: EPI_ERR_BAD_ARG with a message for anything outside the limits or a missing array */
int epi_fuse_validate(const epi_fuse_desc *d, const epi_fuse_inputs *in, const epi_fuse_outputs *out, char *err);
/* DEVICE pointers; one kernel (in slices of 2^23 workgroups: 64 items each for m = 6, 256 for m = 3, i.e. beyond 2^29 /
 * 2^31 items) and the clearing of status enqueued on `stream`: no host
 * synchronisation, no allocation */
int epi_fuse_run_device(const epi_fuse_desc *d, const epi_fuse_inputs *in, const epi_fuse_outputs *out, void *stream, char *err);
/* HOST pointers, on a pooled context of `device` */
int epi_fuse_run_host(const epi_fuse_desc *d, const epi_fuse_inputs *in, const epi_fuse_outputs *out, int device, char *err);

/* ---- REGRESSION_TYPE = 'NONNEGATIVELS-ELEMENT-WISE' between the EKF rounds (TrainPredictPrescribeNPI.m:279-292, :340-353;
 * ForecastQualityAssessment.m:281-294, :342-355): for every NPI k on its own
 *     ffit = fit(X(:,k), y, fittype('a*x+b'), 'Robust','on', 'Lower',[0 -inf], 'Startpoint',[0 0]);  a(k) = ffit.a
 * and then b = mean(y - X*a), for every region in ONE call.  X [D][n][R] and y [D][R] as for epi_nnls_* / epi_lasso_*.
 * One item = (NPI k, region r).  The estimator is the documented one -- bisquare iteratively reweighted least squares,
 * residuals adjusted by leverage, scale from the median absolute deviation, every weighted sub-problem solved in closed
 * form with the slope clamped to [lower_a, upper_a] -- in the operation order of DESIGN.md §4.10, which the kernel,
 * tests/robust_fit_ref.c and tests/robust_fit_ref.py share bit for bit.  robust = 0 stops after the ordinary bounded
 * least-squares start (iters = 0, sigma = NaN, weights 1).
 * status [n][R] is a set of bits; an item with a non-finite x or y has NONFINITE alone, NaN a / b_item / sigma / weights,
 * iters = 0, and its region's b is NaN.
 * epi_robfit_run_device takes DEVICE pointers and enqueues one wavefront per item and then one per region on `stream` (no
 * host synchronisation, no allocation); epi_robfit_run_host takes HOST pointers and runs on a pooled context of `device`. */
enum {
    EPI_ROBFIT_NONFINITE = 1,    /* x or y holds Inf / NaN: NaN outputs */
    EPI_ROBFIT_CONST = 2,        /* max(x) == min(x): the slope is fixed at 0, the iteration gives the robust intercept */
    EPI_ROBFIT_SLOPE_LOST = 4,   /* x is not constant, but the final weights leave the slope unidentified: a = 0 */
    EPI_ROBFIT_MAXITER = 8,      /* max_iter reweightings without meeting the stop rule: the last iterate is kept */
    EPI_ROBFIT_BOUND = 16        /* the clamp to [lower_a, upper_a] changed the slope in the last solve */
};
typedef struct epi_robfit_desc {
    int32_t abi_version;
    int32_t R;                   /* regions, >= 1 */
    int32_t D;                   /* days, 3 .. 1024 (else EPI_ERR_UNSUPPORTED above 1024) */
    int32_t n;                   /* NPIs, 1 .. 12 */
    int32_t robust;              /* 1: 'Robust','on' (bisquare); 0: the least-squares start only */
    int32_t max_iter;            /* reweightings, 1 .. 100000 (robustfit's 50) */
    double lower_a, upper_a;     /* bounds of the slope, lower_a <= upper_a, +-Inf allowed (the reference: 0, +Inf) */
} epi_robfit_desc;
typedef struct epi_robfit_outputs {     /* each may be NULL, but not all of them */
    double *a, *b_item, *sigma;         /* [n][R]: ffit.a, the item's own intercept (the reference discards it), the last scale */
    int32_t *iters, *status;            /* [n][R] */
    double *weights;                    /* [D][n][R]: the final bisquare weights */
    double *b;                          /* [R]: mean(y - X a).  Without `a` the region's n fits run once more, one after the other */
} epi_robfit_outputs;
/* no GPU needed: EPI_ERR_BAD_ARG for a bad descriptor or a NULL descriptor / X / y / outputs / every output,
 * EPI_ERR_UNSUPPORTED for n > 12 or D > 1024 */
int epi_robfit_validate(const epi_robfit_desc *d, const double *X, const double *y, const epi_robfit_outputs *out, char *err);
int epi_robfit_run_device(const epi_robfit_desc *d, const double *X, const double *y, const epi_robfit_outputs *out,
                          void *stream, char *err);
int epi_robfit_run_host(const epi_robfit_desc *d, const double *X, const double *y, const epi_robfit_outputs *out,
                        int device, char *err);

/* ---- The NPI-to-growth-rate predictor of testScripts/test04FullFeatureExtMLpipeline.m (:292-404, :418-431, :576-642; the
 * same block in test01FitExponential.m:150-178, test03ExpfitVsIPRegression.m:147-196, test05DirectNewCasesLearning.m:160-186),
 * for every region and every train / test split in ONE call.  One item = (train end k, region r):
 *   target fill   y(jj) NaN / Inf takes y(jj-1), jj = 2 .. T; a NaN y(1) gives LEADING_NAN (the reference fails on it)
 *   features      [IP, lagged(lags[0]), .., extra], F = n (1 + n_lags) + E columns; a lagged block is 0 on its first lag days
 *   normalisation x_mx = max(abs(column)) over ALL T days, NaN ignored, 0 -> 1
 *   linear map    (X'X + ridge I) m = X'y over the days 1 .. n_train[k], by unblocked lower Cholesky (a pivot <= 0 or
 *                 non-finite gives NOT_PD; MATLAB's backslash would change its factorisation there, which is not restated)
 *   prediction    lambda_hat = [y(1:n_train); X(n_train+1:T, :) m], clipped to +-lambda_threshold on the test days only
 *   rebuild       new_cases_est = [new_smoothed(1:n_train); new_smoothed(n_train) exp(cumsum(lambda_hat(n_train+1:T)))]
 *   tracker       per region: a rise of the mean plan on day ii subtracts reduction_effect from the days
 *                 min(ii + effect_lag, T) .. T, a fall adds it
 * fit = 0 skips the features and the map and takes lambda_in as lambda_hat: LASSO's and the AR model's predictions go
 * through the same clip and rebuild (:586-598, :635-642).  The operation order is DESIGN.md §4.11; the kernels,
 * tests/rate_map_ref.c and tests/rate_map_ref.py share it bit for bit.  Arrays are region-fastest.
 * An item with LEADING_NAN or NOT_PD has that bit alone and NaN map / lambda_hat / new_cases_est; otherwise NONFINITE says
 * that an element of its map, lambda_hat or new_cases_est is Inf or NaN.
 * epi_ratemap_run_device takes DEVICE pointers -- except n_train, which is a HOST array like the descriptor: validate reads
 * it and the launches carry it by value -- and enqueues on `stream` (no host synchronisation, no allocation);
 * epi_ratemap_run_host takes HOST pointers and runs on a pooled context of `device`. */
enum {
    EPI_RATEMAP_LEADING_NAN = 1, /* y(1) is NaN: NaN outputs */
    EPI_RATEMAP_NOT_PD = 2,      /* a Cholesky pivot <= 0 or non-finite: NaN outputs */
    EPI_RATEMAP_NONFINITE = 4    /* a non-finite input reached a result, or a result overflowed */
};
typedef struct epi_ratemap_desc {
    int32_t abi_version;
    int32_t T;                   /* days, >= 1 */
    int32_t n;                   /* NPIs, 1 .. 24 */
    int32_t R;                   /* regions, >= 1 */
    int32_t E;                   /* caller-made extra columns, 0 .. 8 */
    int32_t K;                   /* train ends, >= 1; K * R < 2^31 */
    int32_t n_lags;              /* lagged copies of the plans, 0 .. 3; F = n (1 + n_lags) + E <= 96 */
    int32_t lags[3];             /* 1 <= lag < T (the reference: 3, 5, 7) */
    int32_t fit;                 /* 1: the linear map; 0: lambda_in is lambda_hat */
    int32_t effect_lag;          /* >= 0 (the reference: 3) */
    double ridge;                /* >= 0, finite (1e-6) */
    double lambda_threshold;     /* >= 0 (0.1) */
    double reduction_effect;     /* finite (0.01) */
} epi_ratemap_desc;
typedef struct epi_ratemap_inputs {
    const double *ip;            /* [T][n][R], N/A-filled (epi_preprocess's ip_filled) */
    const double *y;             /* [T][R] the growth rate; needed with fit = 1 or for y_filled */
    const double *new_smoothed;  /* [T][R] */
    const double *extra;         /* [T][E][R]; NULL with E = 0 */
    const double *lambda_in;     /* [K][T][R]; needed with fit = 0 */
    const int32_t *n_train;      /* [K], HOST memory in both entry points: 1 <= n_train[k] <= T */
} epi_ratemap_inputs;
typedef struct epi_ratemap_outputs {    /* each may be NULL, but not all of them */
    double *map;                        /* [K][F][R] in the normalised columns' units; fit = 1 only */
    double *x_mx;                       /* [F][R] */
    double *y_filled;                   /* [T][R] */
    double *lambda_hat, *new_cases_est; /* [K][T][R] */
    double *tracker;                    /* [T][R] */
    int32_t *status;                    /* [K][R] */
} epi_ratemap_outputs;
/* no GPU needed: EPI_ERR_BAD_ARG for a bad descriptor, a missing array or an element count of 2^31 or more,
 * EPI_ERR_UNSUPPORTED for n > 24, n_lags > 3, E > 8 or F > 96 */
int epi_ratemap_validate(const epi_ratemap_desc *d, const epi_ratemap_inputs *in, const epi_ratemap_outputs *out, char *err);
int epi_ratemap_run_device(const epi_ratemap_desc *d, const epi_ratemap_inputs *in, const epi_ratemap_outputs *out,
                           void *stream, char *err);
int epi_ratemap_run_host(const epi_ratemap_desc *d, const epi_ratemap_inputs *in, const epi_ratemap_outputs *out,
                         int device, char *err);

/* ---- MATLAB's rectangular backslash m = X \ y of testScripts/test01FitExponential.m:159, test03ExpfitVsIPRegression.m:169 and
 * test05DirectNewCasesLearning.m:185 (IPtoRateMap = X(1:train,:) \ y(1:train), the raw columns, no ridge), for every region
 * and every row count in ONE call.  One item = (row count k, region r) and uses the rows 1 .. n_rows[k] of X [D][F][R], y [D][R]:
 *   factorisation Householder QR with column pivoting of [X y], unblocked: the pivot is the remaining column of the largest
 *                 partial norm (ties: the lowest original index), the norms downdated as in LAPACK's dlaqp2 with its
 *                 recomputation safeguard at sqrt(eps), the reflectors in dlarfg's convention
 *   rank          the leading j with |R(j,j)| > tol_scale max(n_rows, F) eps |R(1,1)|: the rule MATLAB's lscov.m states; the
 *                 backslash's own tolerance is not documented, so tol_scale is an input (1 gives lscov's)
 *   solution      the basic one: m(perm(1:rank)) = R(1:rank,1:rank) \ (Q'y)(1:rank), every other entry +0
 *   fitted        X m over ALL D rows: the rows beyond n_rows[k] are the prediction
 * Every sum over rows is 8 interleaved fma chains (row i in chain i mod 8) added in ascending order, whatever the launch.  The
 * operation order is DESIGN.md §4.12; the kernel, tests/mldivide_ref.c and tests/mldivide_ref.py share it bit for bit.
 * n_rows < F and n_rows == F run the same route (for a square matrix MATLAB itself goes through LU: not this path).
 * Arrays are region-fastest.  An item with NONFINITE_INPUT has that bit alone, rank -1, perm 0 .. F-1 and NaN m / rdiag / resid /
 * fitted; otherwise RANK_DEFICIENT (MATLAB warns there; the outputs are valid) and NONFINITE may both be set.
 * epi_mldiv_run_device takes DEVICE pointers -- except n_rows, which is a HOST array like the descriptor: validate reads it
 * and the launches carry it by value -- and enqueues on `stream` (no host synchronisation, no allocation);
 * epi_mldiv_run_host takes HOST pointers and runs on a pooled context of `device`. */
enum {
    EPI_MLDIV_RANK_DEFICIENT = 1,  /* rank < min(n_rows, F) */
    EPI_MLDIV_NONFINITE_INPUT = 2, /* a NaN or Inf in the used rows of X or y: NaN outputs, rank -1 */
    EPI_MLDIV_NONFINITE = 4        /* an element of m, rdiag, resid or fitted is Inf or NaN */
};
typedef struct epi_mldiv_desc {
    int32_t abi_version;
    int32_t D;                   /* rows of X and y, >= 1 */
    int32_t F;                   /* columns, 1 .. 96 */
    int32_t R;                   /* regions, >= 1 */
    int32_t K;                   /* row counts, >= 1; K * R < 2^31 */
    double tol_scale;            /* finite, >= 0 (1: lscov's rule) */
} epi_mldiv_desc;
typedef struct epi_mldiv_inputs {
    const double *X;             /* [D][F][R] */
    const double *y;             /* [D][R] */
    const int32_t *n_rows;       /* [K], HOST memory in both entry points: 1 <= n_rows[k] <= D, max(n_rows) (F + 1) <= 20000 */
} epi_mldiv_inputs;
typedef struct epi_mldiv_outputs {      /* each may be NULL, but not all of them */
    double *m;                          /* [K][F][R] */
    int32_t *rank;                      /* [K][R] */
    int32_t *perm;                      /* [K][F][R]: the 0-based original column index in pivot order */
    double *rdiag;                      /* [K][F][R]: the signed R(j,j), +0 beyond min(n_rows, F) */
    double *resid;                      /* [K][R]: the 2-norm of (Q'y)(rank+1 : n_rows) */
    double *fitted;                     /* [K][D][R] */
    int32_t *status;                    /* [K][R] */
} epi_mldiv_outputs;
/* no GPU needed: EPI_ERR_BAD_ARG for a bad descriptor, a missing array, an n_rows outside 1 .. D or an element count of 2^31
 * or more, EPI_ERR_UNSUPPORTED for F > 96 or max(n_rows) (F + 1) > 20000 (the item's matrix stays in LDS) */
int epi_mldiv_validate(const epi_mldiv_desc *d, const epi_mldiv_inputs *in, const epi_mldiv_outputs *out, char *err);
int epi_mldiv_run_device(const epi_mldiv_desc *d, const epi_mldiv_inputs *in, const epi_mldiv_outputs *out,
                         void *stream, char *err);
int epi_mldiv_run_host(const epi_mldiv_desc *d, const epi_mldiv_inputs *in, const epi_mldiv_outputs *out,
                       int device, char *err);

/* ---- The two fitrsvm rows of the phase-I predictor block (testScripts/test05DirectNewCasesLearning.m:198-268,
 * test04FullFeatureExtMLpipeline.m:435-445, :623-624, test03ExpfitVsIPRegression.m:242-262): epsilon-insensitive support-vector
 * regression with a linear or a Gaussian kernel, for every region and every row count in ONE call.  One item = (row count k,
 * region r) fits the rows 1 .. n_rows[k] of X [D][F][R], y [D][R] and predicts all D rows:
 *   kernel        linear: K(a,b) = a.b; Gaussian: K(a,b) = exp(-|a - b|^2 / kernel_scale^2), both over f ascending by fma
 *   problem       LIBSVM's 2n-variable form: alpha_1..n, alpha*_1..n in [0, box], signs +1 / -1, linear term eps - y / eps + y
 *   solver        sequential minimal optimisation from alpha = 0: i the maximal violator, j by the second-order rule, a
 *                 non-positive curvature replaced by 1e-12, ties to the lowest index, LIBSVM's clipped two-variable step,
 *                 no shrinking; it stops when m(alpha) - M(alpha) < tol or after max_iter steps (NOT_CONVERGED: the outputs
 *                 are the iterate reached)
 *   bias          LIBSVM's rule: minus the mean of y_i G_i over the free variables, the midpoint of the bounds without one
 *   fitted        linear: x_t . w + bias with w = sum_i beta_i x_i; Gaussian: sum_i beta_i K(x_t, x_i) + bias; over ALL D rows:
 *                 the rows beyond n_rows[k] are the prediction
 * MATLAB's own solver stops at a gap tolerance of its own and its bias rule is not documented: this is the documented QP, not
 * fitrsvm's bits.  BoxConstraint, Epsilon and KernelScale are per-region inputs ('auto' and the hyper-parameter optimiser are
 * not here).  The operation order is DESIGN.md §4.13; the kernel, tests/svr_ref.c and tests/svr_ref.py share it bit for bit.
 * Arrays are region-fastest.  An item with BAD_INPUT has that bit alone, n_iter 0, n_sv 0 and NaN beta / bias / w / fitted / gap.
 * epi_svr_run_device takes DEVICE pointers -- except n_rows, which is a HOST array like the descriptor: validate reads it and
 * the launches carry it by value -- and enqueues on `stream` (no host synchronisation, no allocation); epi_svr_run_host takes
 * HOST pointers and runs on a pooled context of `device`. */
enum {
    EPI_SVR_NOT_CONVERGED = 1,   /* max_iter steps were taken and the gap is still >= tol */
    EPI_SVR_BAD_INPUT = 2,       /* a NaN or Inf in the used rows of X or y, or box / epsilon / kernel_scale outside its range */
    EPI_SVR_NONFINITE = 4        /* an element of beta, bias, w, fitted or gap is Inf or NaN */
};
enum { EPI_SVR_LINEAR = 0, EPI_SVR_GAUSSIAN = 1 };
typedef struct epi_svr_desc {
    int32_t abi_version;
    int32_t D;                   /* rows of X and y, >= 1 */
    int32_t F;                   /* columns, 1 .. 96 */
    int32_t R;                   /* regions, >= 1 */
    int32_t K;                   /* row counts, >= 1; K * R < 2^31 */
    int32_t kernel;              /* EPI_SVR_LINEAR or EPI_SVR_GAUSSIAN */
    int32_t max_iter;            /* 1 .. 10 000 000 */
    double tol;                  /* > 0, finite */
} epi_svr_desc;
typedef struct epi_svr_inputs {
    const double *X;             /* [D][F][R] */
    const double *y;             /* [D][R] */
    const int32_t *n_rows;       /* [K], HOST memory in both entry points: 1 <= n_rows[k] <= min(D, 1024),
                                    max(n_rows) ((F | 1) + 1) <= 20000 */
    const double *box;           /* [R]: finite, > 0 */
    const double *epsilon;       /* [R]: finite, >= 0 */
    const double *kernel_scale;  /* [R]: finite, > 0 (read for both kernels) */
} epi_svr_inputs;
typedef struct epi_svr_outputs {        /* each may be NULL, but not all of them */
    double *beta;                       /* [K][D][R]: alpha - alpha* on the rows used, +0 beyond them */
    double *bias;                       /* [K][R] */
    double *w;                          /* [K][F][R]: linear kernel only (must be NULL for the Gaussian kernel) */
    double *fitted;                     /* [K][D][R] */
    int32_t *n_iter;                    /* [K][R]: the pair steps taken */
    double *gap;                        /* [K][R]: m(alpha) - M(alpha) of the iterate returned */
    int32_t *n_sv;                      /* [K][R]: the rows with beta != 0 */
    int32_t *status;                    /* [K][R] */
} epi_svr_outputs;
/* no GPU needed: EPI_ERR_BAD_ARG for a bad descriptor, a missing array, w with the Gaussian kernel, an n_rows outside 1 .. D
 * or an element count of 2^31 or more, EPI_ERR_UNSUPPORTED for F > 96, n_rows > 1024 or max(n_rows) ((F | 1) + 1) > 20000 (the
 * item's rows stay in LDS, at the odd stride F | 1, with beta beside them) */
int epi_svr_validate(const epi_svr_desc *d, const epi_svr_inputs *in, const epi_svr_outputs *out, char *err);
int epi_svr_run_device(const epi_svr_desc *d, const epi_svr_inputs *in, const epi_svr_outputs *out,
                       void *stream, char *err);
int epi_svr_run_host(const epi_svr_desc *d, const epi_svr_inputs *in, const epi_svr_outputs *out,
                     int device, char *err);

/* ---- Tools/Rt_ExpFitEKF.m:1 -- 2-state exponential-fit EKF/EKS over the new-case counts, order 1 or 2 ----
 * [S_MINUS, S_PLUS, P_MINUS, P_PLUS, K_GAIN, S_SMOOTH, P_SMOOTH, innovations, rho] =
 *     Rt_ExpFitEKF(x, s_init, params, w_bar, v_bar, Ps_init, Q_w, R_v, beta, gamma, inv_monitor_len, order)
 * batched over B chains: x [T][Sx] (NaN = missing/forecast day), x_series [B] or NULL (identity, Sx == B),
 * rp [EPI_RT_PRM_COUNT][B] holding every other argument of the signature per chain.  Outputs [T][2][B] (S_*, K_GAIN),
 * [T][4][B] (P_*, column-major 2 x 2), [T][B] (innovations, rho).  S_MINUS, S_PLUS, P_MINUS, P_PLUS are required
 * (the smoother reads them back); the others may be NULL.  `order` other than 1 or 2 returns
 * EPI_ERR_UNDEFINED_ORDER ('Undefined order', Rt_ExpFitEKF.m:46,77).  exp/tanh are evaluated in a fixed operation
 * order (< 1 ulp / a few ulp from libm) that the CPU oracle shares: results are reproducible bit for bit. */
enum {
    EPI_RT_TIME_SCALE = 0, EPI_RT_ALPHA = 1, EPI_RT_SIGMA = 2,   /* params(1:3) */
    EPI_RT_W_BAR = 3,      /* w_bar(1:2) */
    EPI_RT_V_BAR = 5, EPI_RT_R_V = 6, EPI_RT_BETA_EKF = 7, EPI_RT_GAMMA_EKF = 8,
    EPI_RT_S_INIT = 9,     /* s_init(1:2) */
    EPI_RT_PS_INIT = 11,   /* Ps_init(:), column-major */
    EPI_RT_Q_W = 15,       /* Q_w(:), column-major */
    EPI_RT_PRM_COUNT = 19
};
typedef struct epi_rt_desc {
    int32_t abi_version;
    int32_t B, T, Sx;
    int32_t L;       /* inv_monitor_len, 1..106 */
    int32_t order;   /* 1 or 2 */
} epi_rt_desc;
typedef struct epi_rt_outputs {
    double *S_MINUS, *S_PLUS, *P_MINUS, *P_PLUS, *K_GAIN, *S_SMOOTH, *P_SMOOTH, *innovations, *rho;
} epi_rt_outputs;
int epi_rt_expfit_validate(const epi_rt_desc *d, char *err);
/* device pointers, enqueues on `stream` */
int epi_rt_expfit_run_device(const epi_rt_desc *d, const int32_t *x_series, const double *x, const double *rp,
                             const epi_rt_outputs *out, void *stream, char *err);
/* host pointers (what a MEX gateway calls): uploads, runs, downloads, synchronises */
int epi_rt_expfit_run_host(const epi_rt_desc *d, const int32_t *x_series, const double *x, const double *rp,
                           const epi_rt_outputs *out, int device, char *err);

/* ---- per-region preprocessing: data-set columns -> filter inputs (Tools/TrainPredictPrescribeNPI.m:142-198,201-202,240) ----
 * All series are [T][S] (day-major, region-minor) -- the x / R_series layout of epi_inputs; ip / ip_filled are
 * [T][n_npi][S] -- the u layout.  cases (and deaths, optional) are CUMULATIVE confirmed counts with NaN for missing
 * days; population [S].  For every region:
 *   new_refined  = diff([c(1); c]), negatives -> 0, a NaN last day <- last valid day, other NaN -> 0      (:166-178)
 *   new_smoothed = filter(ones(1,W), W, new_refined)                                                        (:173)
 *   zero_lag     = filtfilt(ones(1,W2), W2, new_refined), W2 = round(W/2)                                   (:174)
 *   x_new = new_smoothed / N;  x_total = cumsum(new_smoothed) / N                                           (:175-180)
 *   R_v   = 0.1 * ((zero_lag - new_refined) / N).^2                                                         (:240)
 *   fatality = cumsum(filter(.., deaths part)) ./ cumsum(new_smoothed), NaN -> 0                            (:183-197)
 *   I0    = max(min_cases, mean(first `first_num_days` positive samples of new_smoothed))                   (:201-202)
 *   ip_filled: N/A (NaN) levels take the previous day's level, leading N/A -> 0                            (:142-150)
 * Any output pointer may be NULL.  T must exceed 3*(W2-1) (filtfilt's 'Data length must be larger than ...'
 * error) and be >= 2 (:168 'Insufficient data'); 1 <= W <= 32. */
typedef struct epi_pre_desc {
    int32_t abi_version;
    int32_t S, T, n_npi;
    int32_t W;               /* SmoothingWinLen (7 in the reference) */
    int32_t first_num_days;  /* first_num_days_for_case_estimation */
    double min_cases;
} epi_pre_desc;
typedef struct epi_pre_outputs {
    double *new_refined, *new_smoothed, *zero_lag, *x_new, *x_total, *R_v, *fatality;   /* [T][S] */
    double *I0;                                                                         /* [S] */
    double *ip_filled;                                                                  /* [T][n_npi][S] */
} epi_pre_outputs;
size_t epi_preprocess_workspace_bytes(const epi_pre_desc *d);
int epi_preprocess_device(const epi_pre_desc *d, const double *cases, const double *deaths, const double *population,
                          const double *ip, const epi_pre_outputs *out, void *workspace, size_t workspace_bytes,
                          void *stream, char *err);

/* ---- regression between the EKF rounds (Tools/TrainPredictPrescribeNPI.m:251-276, 'NONNEGATIVELS') ----
 * For every region:  reg_coef_a = lsqnonneg(X, y); reg_coef_b = 0; then the loop :266-276 (at most max_iters = 100
 * passes: coef_temp = lsqnonneg(X, y - reg_coef_b), coef0_temp = mean(y - X*reg_coef_a), accepted while the squared
 * error decreases).  X [D][n][S] = NPI_MAXES - InterventionPlans over the regression window, y [D][S] = the smoothed
 * alpha estimate; outputs a [n][S], b [S], min_err [S] (may be NULL), iters [S] (accepted passes, may be NULL),
 * flag [S] (lsqnonneg exit flag of the first solve: 1, or 0 when its inner loop hit 3n iterations; may be NULL).
 * lsqnonneg = Lawson & Hanson's active-set algorithm with MATLAB's tolerance 10*eps*norm(X,1)*length(X), evaluated on
 * the normal equations with a diagonally pivoted Cholesky for the passive-set solves.  1 <= n <= 12. */
typedef struct epi_nnls_desc {
    int32_t abi_version;
    int32_t S, D, n;
    int32_t max_iters;   /* NONNEGATIVELS_IRERATIONS (100 in the reference) */
} epi_nnls_desc;
int epi_nnls_affine_fit_device(const epi_nnls_desc *d, const double *X, const double *y, double *a, double *b,
                               double *min_err, int32_t *iters, int32_t *flag, void *stream, char *err);

/* Host-pointer forms of the three stages around the filter (same arrays in host memory; staged through device `device`,
 * synchronous): what matlab/epiekf_pipeline_mex.cpp binds for TrainPredictPrescribeNPI.m:142-198 (preprocessing),
 * :251-276 (regression) and :496-521 (random-NPI Monte-Carlo). */
int epi_preprocess_host(const epi_pre_desc *d, const double *cases, const double *deaths, const double *population,
                        const double *ip, const epi_pre_outputs *out, int device, char *err);
int epi_nnls_affine_fit_host(const epi_nnls_desc *d, const double *X, const double *y, double *a, double *b,
                             double *min_err, int32_t *iters, int32_t *flag, int device, char *err);
int epi_random_npi_mc_host(const epi_mc_desc *d, const double *sp, const double *u_min, const double *z,
                           const double *J0_prefix, const double *J1_prefix, double *u_out, double *J0, double *J1,
                           int device, char *err);

/* SEIRP.m:1-32 / SEIRPSaturatedResource.m:1-38 batched: par [K][7][B] per-step parameter arrays in the
 * order alpha_e, alpha_i, kappa, rho, beta, mu, gamma (or constant-in-time: par [1][7][B], par_steps=1);
 * init [5][B] = s0,e0,i0,r0,p0; out [K][5][B].  saturated != 0: sat [6][B] = beta_0,beta_s,mu_0,mu_s,
 * sigma,i_0 and par rows 4,5 (beta, mu) are ignored.  integrator: 0 = explicit Euler (the reference,
 * parity), 1 = classical RK4 (extension; no reference oracle). */
int epi_seirp_sim_device(int32_t B, int32_t K, int32_t par_steps, double dt, int32_t saturated,
                         int32_t integrator, const double *par, const double *init, const double *sat,
                         double *out, void *stream, char *err);

/* Tools/SI_Controlled.m:1-23 batched: 2-state forward Euler with a time-dependent infection rate.  alpha [K-1][Sa]
 * (the loop reads alpha(1 : K-1)) with alpha_series [B] or NULL (identity, Sa == B); prm [3][B] = beta, s0, i0;
 * outputs s, i [K][B], the first sample being the initial condition (:15-16). */
int epi_si_controlled_device(int32_t B, int32_t K, int32_t Sa, double dt, const int32_t *alpha_series, const double *alpha,
                             const double *prm, double *s, double *i, void *stream, char *err);
int epi_si_controlled_host(int32_t B, int32_t K, int32_t Sa, double dt, const int32_t *alpha_series, const double *alpha,
                           const double *prm, double *s, double *i, int device, char *err);

/* testScripts/testSIR01.m:15-36 (BASELINE config 1) batched: the 3-compartment SIR with return flow r -> s, forward Euler
 * without clamps, s(t+1) = (-alpha s i + gamma r) dt + s etc.  prm [6][B] = alpha, beta, gamma, s0, i0, r0 per parameter set;
 * out [K][3][B] (rows s, i, r; the first sample is the initial state, :28-30). */
int epi_sir_sim_device(int32_t B, int32_t K, double dt, const double *prm, double *out, void *stream, char *err);
int epi_sir_sim_host(int32_t B, int32_t K, double dt, const double *prm, double *out, int device, char *err);

/* Host-pointer variants of the three entry points above (same arrays in host memory; the library stages them through
 * device `device` and synchronises): what a MEX gateway for SIalpha_Controlled.m / SEIRP.m / SEIRPSaturatedResource.m /
 * NPICost.m binds (matlab/epiekf_sim_mex.cpp). */
int epi_sialpha_sim_host(const epi_sim_desc *d, const int32_t *u_series, const double *u, const double *sp,
                         const double *z, double *s, double *i, double *alpha, double *J0, double *J1, int device,
                         char *err);
int epi_seirp_sim_host(int32_t B, int32_t K, int32_t par_steps, double dt, int32_t saturated, int32_t integrator,
                       const double *par, const double *init, const double *sat, double *out, int device, char *err);
int epi_npi_cost_host(int32_t B, int32_t T, int32_t n_npi, int32_t Su, int32_t weights_per_day, const int32_t *u_series,
                      const double *newcases, const double *inputs, const double *weights, double *J0, double *J1,
                      int device, char *err);

/* ---- The Gaussian innovation log-likelihood of every chain, from the arrays a filter run left on the device ----
 * Not a script of the reference: it hand-picks Q_w, R_v, gamma and beta (Tools/TrainPredictPrescribeNPI.m:12-22, :229-240);
 * this is the number that lets a batch of regions x candidates choose them.  It is the likelihood of the EKF's linearisation;
 * with the state clamps and gamma != 1 it is a score for comparing candidates of one region, not a calibrated probability.
 * Definition (pinned; restated in tests/loglik_ref.c).  Chain c, filter step k, day t = k (t = T-1-k for the
 * two *_BWD models), window k0 <= k < k1 (k1 = 0: T):
 *   C        ObsJacobian of S_MINUS(t), rows 0..2 (NEWCASES: s1 s2, s0 s2, s0 s1; TOTALCASES: -1, 0, 0)
 *   CP(j)    = C0 P(0,j), then fma(C1, P(1,j), .), fma(C2, P(2,j), .), j = 0..2, P = the upper-left 3 x 3 of P_MINUS(t), all nine
 *              elements read (entry (i, j) in row i + m j); CPC' = CP0 C0, fma(CP1, C1, .), fma(CP2, C2, .): the dense filter's
 *              order, whose 6-state terms with C(3..5) = 0 add nothing for a finite P
 *   S        = CPC' + gamma R(k), gamma = prm[EPI_PRM_GAMMA_EKF][c]: the denominator the filter divided by
 *   R(k)     r_mode 1: R_series[k][x_series[c]].  r_mode 0: the filter's own recursion from R_scalar[c], replayed from k = 0
 *              (whatever the window) over the stored innovations and the NaN mask of x: two L-sample windows summed newest
 *              first, mu = sum / cnt, cc = (e - mu)^2, and on a step with beta != 1 and x(t) observed (generic models: and
 *              k < T-1) R(k+1) = beta R(k) + (1 - beta) (sumC / cnt) -- NewCase models: beta R(k) + (1 - beta) sumC / cnt;
 *              on every other step the generic models fall back to R_scalar[c], the NewCase models keep R(k)
 *   valid    x(t) is not NaN and k0 <= k < k1.  bad: valid, and S NaN / infinite / below DBL_MIN or the innovation non-finite;
 *              a bad day enters no sum and sets bit 0 of status[c].  good: valid and not bad
 *   per good day   q = e e / S;  term = log(S) + q  (the library's fixed-order log)
 *   sums     in blocks of 32 filter steps aligned at k = 0: each block from 0.0 over its good days in ascending k, then the
 *              block sums from 0.0 in ascending block order (term, q and the count alike)
 *   n_valid  the number of good days;  loglik = -0.5 (sum_term + n_valid * 1.8378770664093453);  nis_mean = sum_q / n_valid
 *              (NaN for n_valid = 0)
 *   status   bit 0: a bad day;  bit 2: storage 1, r_mode 0 and beta != 1 -- R replayed from rounded innovations
 *   S, nis, R_used [T][B] by DAY: S of every valid day (NaN otherwise), nis = q of every good day (NaN otherwise), R_used =
 *              R(k) of every day
 *   G > 0    B = regions x G chains, region-major: best[r] = the lowest candidate index of the largest loglik among the
 *              candidates with status bit 0 clear and n_valid > 0, or -1;  best_loglik[r] = that value, or NaN
 * Layout: S_MINUS (m rows), P_MINUS (m*m rows), innovations (one row) as epi_ekf_run_* left them: element (t, row, c) at
 *   ((t * nblk + c / blk) * rows + row) * blk + c % blk, blk = lane_block (0 or B: the classic [T][rows][B]), doubles (storage
 *   0) or floats (storage 1, widened on load; all arithmetic is double).  Padding lanes are never read.  x [T][Sx] and R_series
 *   [T][Sx] (indexed by filter step) are the filter's inputs, x_series [B] or NULL (chain c reads column c), R_scalar [B], prm
 *   [EPI_PRM_COUNT][B] as the filter got it (rows EPI_PRM_GAMMA_EKF and EPI_PRM_BETA_EKF are read).
 * Every output may be NULL; at least one of loglik / nis_mean / S / nis / R_used is required, best / best_loglik need G > 0. */
typedef struct epi_loglik_desc {
    int32_t abi_version;
    int32_t model;               /* epi_model */
    int32_t B, T;                /* chains, days */
    int32_t L;                   /* the filter's inv_monitor_len (r_mode 0: the replay's window) */
    int32_t obs_type;            /* epi_obs_type (ignored by EPI_MODEL_NEWCASE6_CODEGEN, as by the filter) */
    int32_t r_mode;              /* 1 = R_series, 0 = R_scalar with the adaptive recursion */
    int32_t Sx;                  /* columns of x / R_series */
    int32_t lane_block;          /* 0 or B: classic; else chains per layout block */
    int32_t storage;             /* 0 = double, 1 = float (S_MINUS, P_MINUS, innovations) */
    int32_t k0, k1;              /* window of filter steps, k1 = 0: T */
    int32_t G;                   /* candidates per region (divides B) for best / best_loglik, or 0 */
    int32_t reserved;            /* 0 */
} epi_loglik_desc;
typedef struct epi_loglik_inputs {
    const void *S_MINUS, *P_MINUS, *innovations;
    const double *x;
    const double *R_series, *R_scalar;   /* the one r_mode names */
    const int32_t *x_series;             /* [B] or NULL */
    const double *prm;
} epi_loglik_inputs;
typedef struct epi_loglik_outputs {
    double *loglik, *nis_mean;           /* [B] */
    int32_t *n_valid, *status;           /* [B] */
    double *S, *nis, *R_used;            /* [T][B] */
    int32_t *best;                       /* [B / G] */
    double *best_loglik;                 /* [B / G] */
} epi_loglik_outputs;
/* no GPU needed: EPI_ERR_BAD_ARG with a message for anything outside the limits, EPI_ERR_OBS_TYPE for an unknown observation
 * type, EPI_ERR_UNSUPPORTED for an L whose two windows do not fit the LDS or B * ceil(T / 32) of 2^31 or more */
int epi_loglik_validate(const epi_loglik_desc *d, char *err);
/* bytes of device workspace epi_loglik_run_device needs (the block sums; r_mode 0: R(k) [T][B]) */
int epi_loglik_workspace_bytes(const epi_loglik_desc *d, size_t *bytes, char *err);
/* DEVICE pointers; up to four kernels enqueued on `stream`: no host synchronisation, no allocation, no second stream.
 * EPI_ERR_WORKSPACE for a workspace below epi_loglik_workspace_bytes */
int epi_loglik_run_device(const epi_loglik_desc *d, const epi_loglik_inputs *in, const epi_loglik_outputs *out, void *ws,
                          size_t ws_bytes, void *stream, char *err);
/* HOST pointers, on a pooled context of `device` (the workspace lives in its arena) */
int epi_loglik_run_host(const epi_loglik_desc *d, const epi_loglik_inputs *in, const epi_loglik_outputs *out, int device,
                        char *err);

/* ---- The direct optimal-NPI planner: the prescription's Pontryagin problem solved in its stable direction ----
 * Not a script of the reference: its sweep integrates the costates forward (SIAlphaModelEKFOptControlled.m:70-72), where they
 * grow like (1 + gamma dt)^T; this call runs the states forward and the adjoint backward from zero, the scheme the demos
 * testScripts/testSIModelOptimalControl01-03.m sketch.  It returns a stationary point of F with its Frank-Wolfe gap, not a
 * certificate of global optimality.
 * Definition (pinned; restated in tests/npi_plan_ref.c).  Chain c = region * P + l, eps = eps[l], ome = 1 - eps:
 *   forward    from (EPI_SIM_S0, _I0, _ALPHA0) of sp, per day t = 0 .. H-1 the scoring tail's day: SIalpha_Controlled's update
 *                with zero noise (the fma chain over gamma a(k) (u_max(k) - u(k)), k ascending, and the clamps), x(t) = the
 *                post-update (s, i, alpha), then NPICost's two running sums (s i alpha; w(k) u(k), k ascending), started from the
 *                first term:  F = ome * sum0 + eps * sum1.  J0, J1: the same sums continued from J0_prefix / J1_prefix when
 *                prefix_days > 0, divided by (H + prefix_days) and n_npi (H + prefix_days): epi_sialpha_score_device's values
 *   d(t)       three flags: x(t) strictly inside its clamp (0 < s < 1, 0 < i < 1, alpha_min < alpha < alpha_max)
 *   adjoint    t = H-1 .. 0:  mu(t) = ome (i al, s al, s i)  [t = H-1],  else  ome (..) + m  with v = d(t+1) ? mu(t+1) : 0 and
 *                m0 = fma(A10, v1, A00 v0), m1 = fma(A11, v1, A01 v0), m2 = fma(A22, v2, fma(A12, v1, A02 v0)), A the state block
 *                of StateJacobians at x(t) in the filter's own form: A00 = 1 - dt al i, A01 = -dt al s, A02 = -dt s i,
 *                A10 = dt i al, A11 = 1 + dt (s al - beta), A12 = dt s i, A22 = 1 - dt gamma (products left to right)
 *   gradient   g(k,t) = eps w(k) - dt (gamma a(k)) mu2(t) if d2(t), else eps w(k);  vertex u*(k,t) = u_min(k) if g > 0, else
 *                u_max(k) (the reference's tie rule);  held entries (u_fixed not NaN) keep their value and enter no sum
 *   gap        from 0.0, days descending, k ascending over the free entries: gap = gap + g (u - u*)
 *   iteration  F of the starting plan (free entries: u_init, or u_min without it); then repeat: F non-finite -> stop, status
 *                bit 2 (gap and mu NaN); F_trace[iters] = F, iters += 1, adjoint pass; gap <= tol |F| -> stop, status 0;
 *                iters == max_iter -> stop, bit 0; for j = 0 .. max_halvings, theta = 2^-j: the trial plan u + theta (u* - u)
 *                element by element, a full forward pass of it, accepted if F_trial < F (its plan, states and sums become the
 *                current ones), else halvings += 1; none accepted -> stop, bit 1.
 *   so the plan returned is always the one gap and mu belong to, F_trace is strictly decreasing, and F, J0, J1 are what the
 *   scoring tail gives for the plan returned.  F_trace beyond iters is NaN.
 * Layout: sp [EPI_SIM_PRM_COUNT][R] (pipeline.scoring_region_inputs), u_min [n_npi][R], eps [P], u_fixed [H][n_npi][R] or NULL
 *   (NaN = free), u_init [H][n_npi][R*P] or NULL, J0_prefix / J1_prefix [R] (needed for prefix_days > 0).  plan [H][n_npi][R*P],
 *   states and mu [H][3][R*P], F_trace [max_iter][R*P]; the rest [R*P].  states, mu and F_trace may be NULL. */
typedef struct epi_plan_desc {
    int32_t abi_version;
    int32_t R, P;                /* regions, cost weights: B = R * P chains */
    int32_t H;                   /* horizon in days, >= 1 */
    int32_t n_npi;               /* 1 .. EPI_MAX_NPI */
    int32_t prefix_days;         /* >= 0 */
    int32_t max_iter;            /* 1 .. 255 */
    int32_t max_halvings;        /* 0 .. 30 */
    double tol;                  /* >= 0, finite */
} epi_plan_desc;
typedef struct epi_plan_inputs {
    const double *sp, *u_min, *eps;
    const double *u_fixed, *u_init;          /* or NULL */
    const double *J0_prefix, *J1_prefix;     /* [R]; read for prefix_days > 0 */
} epi_plan_inputs;
typedef struct epi_plan_outputs {
    double *plan;                            /* [H][n_npi][B] */
    double *J0, *J1, *F, *gap;               /* [B] */
    int32_t *iters, *halvings, *status;      /* [B] */
    double *states, *mu;                     /* [H][3][B] or NULL */
    double *F_trace;                         /* [max_iter][B] or NULL */
} epi_plan_outputs;
/* no GPU needed: EPI_ERR_BAD_ARG with a message for R, P, H < 1, n_npi outside 1 .. 12, prefix_days < 0, max_iter outside
 * 1 .. 255, max_halvings outside 0 .. 30, a negative or non-finite tol; EPI_ERR_UNSUPPORTED where R * P, H * max(n_npi, 3) * R * P
 * or max_iter * R * P reaches 2^31 (the call is not cut into launches) */
int epi_plan_validate(const epi_plan_desc *d, char *err);
/* bytes of device workspace epi_plan_run_device needs (the second plan, the states of both sides, the vertex masks) */
int epi_plan_workspace_bytes(const epi_plan_desc *d, size_t *bytes, char *err);
/* DEVICE pointers; one kernel enqueued on `stream`: no host synchronisation, no allocation.  EPI_ERR_BAD_ARG for a NULL
 * required array, EPI_ERR_WORKSPACE for a workspace below epi_plan_workspace_bytes */
int epi_plan_run_device(const epi_plan_desc *d, const epi_plan_inputs *in, const epi_plan_outputs *out, void *ws, size_t ws_bytes,
                        void *stream, char *err);
/* HOST pointers, on a pooled context of `device` (the workspace lives in its arena) */
int epi_plan_run_host(const epi_plan_desc *d, const epi_plan_inputs *in, const epi_plan_outputs *out, int device, char *err);

/* ---- Joint posterior draws of the smoothed paths (backward simulation), from the arrays a 3-state filter run left ----
 * Not a script of the reference: its smoother returns the marginal law of every day (S_SMOOTH, P_SMOOTH); this call samples the
 * joint law over days whose mean and covariance recursions are Tools/GenericExtendedKalmanFilter.m:218 and :223.
 * Definition (pinned; restated in tests/sdraw_ref.c).  Chain c, day k, draw d, path p = c * D + d:
 *   A_k      StateJacobians of S_PLUS(k) (SIAlphaModelEKF.m:62-76; prm rows EPI_PRM_DT, _BETA, _GAMMA)
 *   J_k      k < T-1: (P_PLUS(k) A_k') pinv(P_MINUS(k+1)) in the smoother's own operation order (the fma chains of its products, the
 *              library's pinv on the upper triangle of P_MINUS): the bits the smoother forms.  0 where P_MINUS(k+1) holds a NaN
 *              or an Inf (:211), and for k = T-1
 *   Sigma_k  = P_PLUS(k) - (J_k P_MINUS(k+1)) J_k', products written (acc = a0 b0; acc = acc + ak bk, no fma), then (Sigma +
 *              Sigma') / 2.  Under the guard and for k = T-1: P_PLUS(k) (k = T-1: P_term when given), symmetrised the same way
 *   F_k      the factor of Sigma_k by a right-looking Cholesky with diagonal pivoting (the first largest remaining diagonal entry),
 *              stopped when that pivot is <= 3 eps max diag(Sigma_k) (eps = 2^-52) or not positive: column j = a(:, j) / sqrt(pivot),
 *              trailing block a(i, c) - l(i, j) l(c, j); the remaining columns are zero and the rows return to the original
 *              order, so F F' = Sigma up to rounding and F is a row-permuted lower triangle (nine entries).  rank = the columns kept
 *   x_{T-1}  = clamp(s_T + F z),  s_T = s_term when given, else S_PLUS(T-1)
 *   x_k      = clamp((S_PLUS(k) + J_k (x_{k+1} - S_MINUS(k+1))) + F_k z_k): J d first (d0 term, then fma for d1, d2: the
 *              smoother's :218), S_PLUS added, then F z as its own sum (written products) added.  z = NULL: the noise term is
 *              not formed, and with clamp = 1 the path is S_SMOOTH bit for bit
 *   clamp    StateHardMargins (SIAlphaModelEKF.m:27-31; prm rows EPI_PRM_S_MIN, _I_MIN, _ALPHA_MIN, _ALPHA_MAX) applied to every draw
 *              as :221 applies it to the mean, except that a NaN entry stays NaN.  clamp = 0: none (an exactly Gaussian law)
 *   a non-finite entry of S_PLUS(k) / P_PLUS(k) (k = T-1: of P_term): J_k and F_k are NaN, rank -1
 *   status   bit 0 (EPI_SDRAW_NONFINITE): a non-finite input entry met (the guard fired, or a NaN record);  bit 1
 *              (EPI_SDRAW_RANK_DEFICIENT): a rank below 3 on some day
 * Layout: S_PLUS, S_MINUS (3 rows), P_PLUS, P_MINUS (9 rows) as epi_ekf_run_* left them: element (t, row, c) at ((t * nblk + c /
 *   blk) * rows + row) * blk + c % blk, blk = lane_block (0 or B: the classic [T][rows][B]), doubles (storage 0) or floats (storage
 *   1, widened on load; all arithmetic is double).  Padding lanes are never read.  prm [EPI_PRM_COUNT][B]; s_term [3][B], P_term
 *   [9][B] doubles or NULL.  z and X [T - k0][3][B * D], path-minor (what epi_ens_run_* takes with R = B), each double or float
 *   (z_f32, out_f32; a float X is the double result rounded once).  J, L (= F) [T][9][B] column-major entries, rank [T][B], status
 *   [B].  Every output may be NULL. */
enum { EPI_SDRAW_NONFINITE = 1, EPI_SDRAW_RANK_DEFICIENT = 2 };
typedef struct epi_sdraw_desc {
    int32_t abi_version;
    int32_t model;               /* EPI_MODEL_SIA3 only */
    int32_t B, T;                /* chains, days */
    int32_t D;                   /* draws per chain, >= 1 */
    int32_t k0;                  /* first day returned, 0 <= k0 < T: the recursion stops there */
    int32_t clamp;               /* 1 = StateHardMargins on every draw, 0 = none */
    int32_t lane_block;          /* 0 or B: classic; else chains per layout block */
    int32_t storage;             /* 0 = double, 1 = float (S_PLUS, P_PLUS, S_MINUS, P_MINUS) */
    int32_t z_f32, out_f32;      /* element type of z / X: 0 = double, 1 = float */
    int32_t test_launch_groups;  /* 0; > 0: workgroups per launch (the tests cut small calls into several launches with it) */
} epi_sdraw_desc;
typedef struct epi_sdraw_inputs {
    const void *S_PLUS, *P_PLUS, *S_MINUS, *P_MINUS;
    const double *prm;
    const void *z;                       /* or NULL: the deterministic path */
    const double *s_term, *P_term;       /* or NULL */
} epi_sdraw_inputs;
typedef struct epi_sdraw_outputs {
    void *X;                             /* [T - k0][3][B * D] */
    int32_t *rank, *status;              /* [T][B], [B] */
    double *J, *L;                       /* [T][9][B] */
} epi_sdraw_outputs;
/* no GPU needed: EPI_ERR_UNSUPPORTED with a message for a model other than EPI_MODEL_SIA3 (the six-state models: their costate
 * block has no meaningful factor in fp64; the time-flipped models), EPI_ERR_BAD_ARG for B, T, D < 1, k0 outside 0 .. T-1, a
 * clamp, storage, z_f32 or out_f32 outside {0, 1}, a lane_block outside 0 .. B, a negative test_launch_groups */
int epi_sdraw_validate(const epi_sdraw_desc *d, char *err);
/* bytes of device workspace epi_sdraw_run_device needs (24 doubles per (day, chain)) */
int epi_sdraw_workspace_bytes(const epi_sdraw_desc *d, size_t *bytes, char *err);
/* DEVICE pointers; a memset of status and the two kernels (each cut into launches below 2^31 threads) enqueued on `stream`: no
 * host synchronisation, no allocation.  EPI_ERR_WORKSPACE for a workspace below epi_sdraw_workspace_bytes */
int epi_sdraw_run_device(const epi_sdraw_desc *d, const epi_sdraw_inputs *in, const epi_sdraw_outputs *out, void *ws, size_t ws_bytes,
                         void *stream, char *err);
/* HOST pointers, on a pooled context of `device` (the workspace lives in its arena) */
int epi_sdraw_run_host(const epi_sdraw_desc *d, const epi_sdraw_inputs *in, const epi_sdraw_outputs *out, int device, char *err);

/* ---- Probabilistic forecast scores of the Monte-Carlo ensembles (not a script of the reference) ----
 * src [T][rows][B], B = R * D, region-major, double or float, and the derived row, exactly as epi_ens_run_* take them; an item is
 * one (day t, row, region r) with its D members, NaN members absent, n the others.  The truth of the item is
 * y = truth[(t * rows' + row) * Rt + ts], ts = truth_series ? truth_series[r] : r (entries in 0 .. Rt-1; several regions may
 * share a column; without truth_series Rt = R).  Definition (pinned; restated in tests/escore_ref.py and tests/escore_ref.c):
 *   rank = #{members < y}, ties = #{members == y}, count = n
 *   x(1 .. n) the members ascending; Q(p) the quantile of epi_ens_run_* (h = n p + 0.5, k = floor(h), g = h - k; x(1) if k < 1,
 *     x(n) if k >= n, else x(k) + g (x(k+1) - x(k)));  med = Q(0.5), l_k = Q(alpha_k / 2), u_k = Q(1 - alpha_k / 2), the two
 *     probabilities formed once on the host in double
 *   ae = |y - med|;  width_k = u_k - l_k;  cover bit k = (l_k <= y and y <= u_k)
 *   IS_k = (width_k + c_k pos(l_k - y)) + c_k pos(y - u_k),  c_k = 2 / alpha_k,  pos(d) = d if d > 0 else 0
 *   wis = (...((0.5 ae) + (alpha_0 / 2) IS_0) + ... + (alpha_{n_a-1} / 2) IS_{n_a-1}) / (n_a + 0.5)
 *   crps = (2 / (n n)) tree(term),  term at sorted position i = 1 .. n: (x(i) - y) (((n if y < x(i) else 0) - i) + 0.5), +0.0
 *     at the positions n+1 .. P (selected by position), P the power of two >= max(D, 64), tree() the pairwise sum of
 *     epi_ens_run_* over the positions: the ensemble CRPS (1/n) sum |x_i - y| - (1/(2 n n)) sum sum |x_i - x_j|
 *   n = 0 or y NaN: every floating output of the item is NaN, rank = ties = -1, cover = 0 (count = n); non-finite members
 *     give what IEEE arithmetic gives in this order
 * Per (row, region), over the days k0 <= t < k1 with t >= first_day[r] (0 without first_day) and rank >= 0, ascending from 0.0:
 *   n_scored their number; crps_mean, wis_mean, ae_mean = sum / n_scored; cover_frac[k] = #{bit k set} / n_scored (NaN when
 *   n_scored = 0); pit_hist[b] = #{days with b = min(n_bins - 1, ((2 rank + ties + 1) n_bins) / (2 (count + 1)))} in 64-bit
 *   integer arithmetic (the bin of the non-randomised mid-rank)
 * Outputs (each may be NULL; at least one must not be): crps, wis, ae [T][rows'][R], width [T][n_a][rows'][R], rank, ties,
 *   cover, count [T][rows'][R] int32, crps_mean, wis_mean, ae_mean [rows'][R], n_scored [rows'][R] int32, cover_frac
 *   [n_a][rows'][R], pit_hist [n_bins][rows'][R] int32; rows' = rows + derive_newcases */
typedef struct epi_escore_desc {
    int32_t abi_version;
    int32_t T, rows, R;          /* days, rows of src, regions: each >= 1 */
    int32_t D;                   /* draws per region, 1 .. 4096; R * D <= INT32_MAX */
    int32_t Rt;                  /* columns of truth, >= 1 (= R without truth_series) */
    int32_t n_a;                 /* central intervals, 0 .. 8 */
    int32_t n_bins;              /* bins of pit_hist, 0 .. 32 (0: no histogram) */
    int32_t storage;             /* element type of src: 0 = double, 1 = float */
    int32_t derive_newcases;     /* 0, or 1: append the row ((N * row0) * row1) * row2 */
    int32_t k0, k1;              /* the window of the per-region outputs, 0 <= k0 <= k1 <= T */
    int32_t test_launch_items;   /* 0; > 0: items per launch (the tests cut small calls into several launches with it) */
    int32_t reserved;            /* 0 */
    double alpha[8];             /* levels, each in (0, 1), strictly descending; the first n_a are read */
} epi_escore_desc;
typedef struct epi_escore_inputs {
    const void *src;                     /* [T][rows][R * D] */
    const double *population;            /* [R] (derive_newcases) or NULL */
    const double *truth;                 /* [T][rows'][Rt] */
    const int32_t *truth_series;         /* [R] or NULL */
    const int32_t *first_day;            /* [R] or NULL */
} epi_escore_inputs;
typedef struct epi_escore_outputs {
    double *crps, *wis, *ae;             /* [T][rows'][R] */
    double *width;                       /* [T][n_a][rows'][R] */
    int32_t *rank, *ties, *cover, *count; /* [T][rows'][R] */
    double *crps_mean, *wis_mean, *ae_mean; /* [rows'][R] */
    int32_t *n_scored;                   /* [rows'][R] */
    double *cover_frac;                  /* [n_a][rows'][R] */
    int32_t *pit_hist;                   /* [n_bins][rows'][R] */
} epi_escore_outputs;
/* no GPU needed: EPI_ERR_BAD_ARG for T, rows, R, Rt < 1, D outside 1 .. 4096, R * D > INT32_MAX, n_a outside 0 .. 8, n_bins outside
 * 0 .. 32, an alpha outside (0, 1) or not strictly descending, k0 / k1 outside 0 <= k0 <= k1 <= T, storage or derive_newcases
 * outside {0, 1}, derive_newcases with rows < 3 or without population, a negative test_launch_items, a NULL src / truth, Rt != R
 * without truth_series, pit_hist with n_bins = 0, no output at all */
int epi_escore_validate(const epi_escore_desc *d, const epi_escore_inputs *in, const epi_escore_outputs *out, char *err);
/* bytes of device workspace epi_escore_run_device needs: the per-item arrays the per-region outputs are formed from (three
 * doubles and four int32 per item), whichever of them the caller also asks for */
int epi_escore_workspace_bytes(const epi_escore_desc *d, size_t *bytes, char *err);
/* DEVICE pointers; one wavefront per item (cut into launches below 2^31 threads), then one lane per (row, region) when a
 * per-region output is asked for, enqueued on `stream`: no host synchronisation, no allocation.  EPI_ERR_WORKSPACE for a
 * workspace below epi_escore_workspace_bytes when a per-region output is asked for (else ws may be NULL) */
int epi_escore_run_device(const epi_escore_desc *d, const epi_escore_inputs *in, const epi_escore_outputs *out, void *ws,
                          size_t ws_bytes, void *stream, char *err);
/* HOST pointers, on a pooled context of `device` (the workspace lives in its arena) */
int epi_escore_run_host(const epi_escore_desc *d, const epi_escore_inputs *in, const epi_escore_outputs *out, int device, char *err);

/* ---- Path functionals of the Monte-Carlo ensembles (not a script of the reference) ----
 * src [T][rows][N], N = R * D, region-major (path p = r * D + d), double or float, and the derived row ((N_r v0) v1) v2 as row
 * `rows`, exactly as epi_ens_run_* take them.  The window is k0 <= t < k1, W = k1 - k0.  Definition (pinned; restated in
 * tests/pathfn_ref.py and tests/pathfn_ref.c), per path p of region r and row q:
 *   day t is VALID if max(k0, first_day[r]) <= t < k1 (first_day 0 without the array) and the value v is not NaN; +Inf and -Inf
 *     are values.  One IEEE double operation per written operation, no fma(); a float value is widened once.
 *   peak_value = the maximum over the valid days, peak_day = the first t that attains it (ascending scan, update on strict >),
 *     the absolute day index of src as a double; min_value, min_day the same with <
 *   total: block j holds the days k0 + 32 j .. k0 + 32 j + 31 of the window; a block's sum starts at +0.0 and adds its valid
 *     days ascending (an invalid day is dropped by a select, not added as zero); total starts at +0.0 and adds the block sums
 *     for j ascending, every block of the window included
 *   per threshold j, thr = thr[(j * rows' + q) * R + r]: a day is ABOVE if it is valid and v >= thr; first_cross = the first
 *     such t (NaN: none), days_above their number, longest_run the longest run of consecutive above days (an invalid or a below
 *     day ends a run).  A NaN thr: the three are NaN ("not asked for this row and region")
 *   n_valid the number of valid days; n_valid = 0: every floating output of the (path, row) is NaN
 * Per (row, region) over the paths with n_valid > 0: n_paths; peak_day_hist[t - k0] = #{paths with peak_day = t}; n_cross[j] =
 *   #{paths with a first_cross}; cross_day_hist[t - k0][j] the same binned by first_cross.  Integer counts: no order involved.
 * Outputs (each may be NULL; at least one must not be): peak_value, peak_day, min_value, min_day, total [rows'][N];
 *   first_cross, days_above, longest_run [n_thr][rows'][N] (all double: each is itself a src of epi_ens_run_*); n_valid
 *   [rows'][N] int32; n_paths [rows'][R], peak_day_hist [W][rows'][R], n_cross [n_thr][rows'][R], cross_day_hist
 *   [W][n_thr][rows'][R] int32; rows' = rows + derive_newcases */
typedef struct epi_pathfn_desc {
    int32_t abi_version;
    int32_t T, rows, R;          /* days, rows of src (1 .. 4096), regions: each >= 1 */
    int32_t D;                   /* draws per region, >= 1; R * D <= INT32_MAX */
    int32_t n_thr;               /* thresholds, 0 .. 8 */
    int32_t storage;             /* element type of src: 0 = double, 1 = float */
    int32_t derive_newcases;     /* 0, or 1: append the row ((N * row0) * row1) * row2 */
    int32_t k0, k1;              /* the window, 0 <= k0 < k1 <= T */
    int32_t test_segments;       /* 0: the library's rule; > 0: time segments wanted, at most min(ceil(W / 32), 1024) (the tests) */
    int32_t test_launch_groups;  /* 0; > 0: workgroups per launch (the tests cut small calls into several launches with it) */
} epi_pathfn_desc;
typedef struct epi_pathfn_inputs {
    const void *src;                     /* [T][rows][R * D] */
    const double *population;            /* [R] (derive_newcases) or NULL */
    const double *thr;                   /* [n_thr][rows'][R] (NULL with n_thr = 0) */
    const int32_t *first_day;            /* [R] or NULL */
} epi_pathfn_inputs;
typedef struct epi_pathfn_outputs {
    double *peak_value, *peak_day, *min_value, *min_day, *total; /* [rows'][N] */
    double *first_cross, *days_above, *longest_run;              /* [n_thr][rows'][N] */
    int32_t *n_valid;                    /* [rows'][N] */
    int32_t *n_paths;                    /* [rows'][R] */
    int32_t *peak_day_hist;              /* [W][rows'][R] */
    int32_t *n_cross;                    /* [n_thr][rows'][R] */
    int32_t *cross_day_hist;             /* [W][n_thr][rows'][R] */
} epi_pathfn_outputs;
/* no GPU needed: EPI_ERR_BAD_ARG for T, R, D < 1, rows outside 1 .. 4096, R * D > INT32_MAX, n_thr outside 0 .. 8, k0 / k1 outside
 * 0 <= k0 < k1 <= T, storage or derive_newcases outside {0, 1}, derive_newcases with rows < 3 or without population,
 * test_segments outside 0 .. min(ceil(W / 32), 1024), a negative test_launch_groups, a NULL src, a NULL thr with n_thr > 0, a
 * threshold output with n_thr = 0, a histogram with W > 4096 (the bins of one histogram live in LDS), no output at all */
int epi_pathfn_validate(const epi_pathfn_desc *d, const epi_pathfn_inputs *in, const epi_pathfn_outputs *out, char *err);
/* bytes of device workspace epi_pathfn_run_device needs: peak_day and first_cross for the histograms (whichever of them the
 * caller also asks for), and with more than one time segment the segments' partial records */
int epi_pathfn_workspace_bytes(const epi_pathfn_desc *d, size_t *bytes, char *err);
/* DEVICE pointers; one lane per path (cut into launches of at most 2^22 workgroups), a combining pass when the days are cut into
 * segments, then one workgroup per (histogram, row, region) when a per-region output is asked for, enqueued on `stream`: no host
 * synchronisation, no allocation.  EPI_ERR_WORKSPACE for a workspace below epi_pathfn_workspace_bytes when the call needs one
 * (segments or a per-region output; else ws may be NULL) */
int epi_pathfn_run_device(const epi_pathfn_desc *d, const epi_pathfn_inputs *in, const epi_pathfn_outputs *out, void *ws,
                          size_t ws_bytes, void *stream, char *err);
/* HOST pointers, on a pooled context of `device` (the workspace lives in its arena) */
int epi_pathfn_run_host(const epi_pathfn_desc *d, const epi_pathfn_inputs *in, const epi_pathfn_outputs *out, int device, char *err);

/* ---- Joint scores of the Monte-Carlo ensembles: energy score and variogram score (not a script of the reference) ----
 * src [T][rows][B], B = R * D, region-major, double or float, the derived row, truth [T][rows'][Rt], truth_series and first_day
 * exactly as epi_escore_run_* take them.  An item is one (row, region r), item = row * R + r.  Definition (pinned; restated in
 * tests/ejoint_ref.py and tests/ejoint_ref.c; one IEEE double operation per written operation, sqrt correctly rounded):
 *   days of the item: the t in [max(k0, first_day[r]), k1) whose truth y_t = truth[(t * rows' + row) * Rt + ts] is not NaN
 *     (ts = truth_series ? truth_series[r] : r), ascending; W their number
 *   members of the item: member i is absent when x_it is NaN on any day of the item (with W = 0 nobody is); n the number present
 *   n = 0 or W = 0: every floating output of the item is NaN; n_members = n and n_days = W are still written
 *   d2(i, y) = sum over the item's days, ascending from 0.0, of (x_it - y_t) * (x_it - y_t);  e_i = sqrt(d2(i, y))
 *   d2(i, j) the same sum with x_jt in place of y_t;  dist_ij = sqrt(d2(i, j))
 *   truth_term = tree(e) / n: tree() the pairwise sum of epi_ens_run_* over P positions, P the power of two >= max(D, 64);
 *     absent members and the positions >= D count as +0.0, selected by position
 *   pair sum: members in blocks of 64, block I = members 64 I .. 64 I + 63; tile (I, J), I <= J.  Lane i of the tile (member
 *     64 I + i) forms s_i = (..((0.0 + c_i0) + c_i1) + .. + c_i63), c_ij = dist between members 64 I + i and 64 J + j when both are
 *     present (and below D) and, for I = J, j > i; else +0.0 (selected: the sum still adds it).  The tile sum is tree(s) over
 *     the 64 lanes.  pairsum = the tile sums added from 0.0 in the order I ascending, then J ascending from I.
 *   spread_term = pairsum / (n * n);  es = truth_term - spread_term: the ensemble energy score
 *     (1/n) sum ||x_i - y|| - (1/(2 n n)) sum sum ||x_i - x_j||; with W = 1 the ensemble CRPS
 *   variogram score, vs_order 1 (p = 0.5: g(a) = sqrt(fabs(a))) or 2 (p = 1: g(a) = fabs(a)); for days s < t of the item with
 *     t - s <= max_lag in calendar days (max_lag = 0: every pair): m_st = tree(g(x_is - x_it)) / n with absent members and
 *     positions >= D as +0.0;  term = g(y_s - y_t) - m_st;  v_s = sum over t ascending from 0.0 of term * term (0.0 for a day
 *     without a later one);  vs = sum over every day s of the item ascending from 0.0 of v_s
 *   non-finite members give what IEEE arithmetic gives in this order
 * Outputs (each may be NULL; at least one must not be): es, truth_term, spread_term, vs [rows'][R]; n_members, n_days [rows'][R]
 *   int32; member_dist [rows'][R * D], the e_i, NaN for absent members (region-major: itself a source of epi_ens_run_*);
 *   rows' = rows + derive_newcases */
typedef struct epi_ejoint_desc {
    int32_t abi_version;
    int32_t T, rows, R;          /* days, rows of src, regions: each >= 1; rows' * R <= INT32_MAX */
    int32_t D;                   /* draws per region, 1 .. 4096; R * D <= INT32_MAX */
    int32_t Rt;                  /* columns of truth, >= 1 (= R without truth_series) */
    int32_t storage;             /* element type of src: 0 = double, 1 = float */
    int32_t derive_newcases;     /* 0, or 1: append the row ((N * row0) * row1) * row2 */
    int32_t k0, k1;              /* the window, 0 <= k0 <= k1 <= T */
    int32_t vs_order;            /* 0: no variogram score; 1: p = 0.5; 2: p = 1 */
    int32_t max_lag;             /* >= 0: the largest t - s of a pair of days in the variogram score (0: every pair) */
    int32_t test_launch_tiles;   /* 0; > 0: units (items, tiles, days) per launch (the tests cut small calls into several launches) */
    int32_t reserved;            /* 0 */
} epi_ejoint_desc;
typedef struct epi_ejoint_inputs {
    const void *src;                     /* [T][rows][R * D] */
    const double *population;            /* [R] (derive_newcases) or NULL */
    const double *truth;                 /* [T][rows'][Rt] */
    const int32_t *truth_series;         /* [R] or NULL */
    const int32_t *first_day;            /* [R] or NULL */
} epi_ejoint_inputs;
typedef struct epi_ejoint_outputs {
    double *es, *truth_term, *spread_term, *vs; /* [rows'][R] */
    int32_t *n_members, *n_days;         /* [rows'][R] */
    double *member_dist;                 /* [rows'][R * D] */
} epi_ejoint_outputs;
/* no GPU needed: EPI_ERR_BAD_ARG for T, rows, R, Rt < 1, D outside 1 .. 4096, R * D or rows' * R > INT32_MAX, rows' * R *
 * max(tiles, k1 - k0) > 2^40 (tiles = nb (nb + 1) / 2, nb = ceil(D / 64): refused, not cut), k0 / k1 outside 0 <= k0 <= k1 <= T,
 * storage or derive_newcases outside {0, 1}, derive_newcases with rows < 3 or without population, vs_order outside 0 .. 2, a
 * negative max_lag or test_launch_tiles, a NULL src / truth, Rt != R without truth_series, vs with vs_order = 0, no output at all */
int epi_ejoint_validate(const epi_ejoint_desc *d, const epi_ejoint_inputs *in, const epi_ejoint_outputs *out, char *err);
/* bytes of device workspace epi_ejoint_run_device needs: per item a double, the tile sums, the v_s, the masks of present members
 * (a 64-bit word per block), n, W and the day list */
int epi_ejoint_workspace_bytes(const epi_ejoint_desc *d, size_t *bytes, char *err);
/* DEVICE pointers; a wavefront per item, then per (item, tile) when es or spread_term is asked for, then per (item, day) when vs
 * is, then a lane per (row, region), each cut into launches below 2^31 threads, enqueued on `stream`: no host synchronisation, no
 * allocation, no atomics.  EPI_ERR_WORKSPACE for a workspace below epi_ejoint_workspace_bytes */
int epi_ejoint_run_device(const epi_ejoint_desc *d, const epi_ejoint_inputs *in, const epi_ejoint_outputs *out, void *ws,
                          size_t ws_bytes, void *stream, char *err);
/* HOST pointers, on a pooled context of `device` (the workspace lives in its arena) */
int epi_ejoint_run_host(const epi_ejoint_desc *d, const epi_ejoint_inputs *in, const epi_ejoint_outputs *out, int device, char *err);

/* ---- Standard-normal draws from a seed, generated on the device (not a script of the reference) ----
 * The Monte-Carlo calls above take their draws as an input array z.  The *_seeded calls below generate the same draws in registers
 * where they are used: a seeded call gives, bit for bit, what its unseeded sibling gives when it is handed the array that
 * epi_noise_fill_* writes for the same descriptor.  Definition (pinned; restated in tests/noise_ref.c and tests/noise_ref.py).
 * Draw (t, row, lane) of a logical array [nt][rows][lanes], rows in {1, 3}, lane a 64-bit index, t a 32-bit index:
 *   block    one Philox4x32-10 block (Salmon et al., SC'11), key (seed_lo, seed_hi), counter
 *              (lane & 0xffffffff, lane >> 32, t, 0x80000000 | (stream << 1) | (row >> 1)),   stream < 2^30.
 *            The set top bit keeps these blocks apart from the integer draws of epi_random_npi_mc_*, whose fourth counter word is a
 *            day: the same seed may drive both
 *   uniform  j = row & 1 takes the output words w[2j], w[2j+1]:  n = (w[2j] >> 6) * 2^26 + (w[2j+1] >> 6),  u = (n + 0.5) * 2^-52,
 *            exact in double and strictly inside (0, 1)
 *   normal   z = the inverse normal CDF of u by Wichura's algorithm AS241 (PPND16) with the published coefficients: q = u - 0.5;
 *            |q| <= 0.425: r = 0.180625 - q q, z = (A(r) q) / B(r);  else r = sqrt(-epi_log(q < 0 ? u : 1 - u)), r <= 5: r - 1.6 and
 *            C / D, else r - 5 and E / F, negated for q < 0.  Every polynomial is Horner in written operations (acc = acc * r + c,
 *            no contraction), the logarithm is the library's own (fixed operation order), sqrt is correctly rounded, the quotient
 *            is one division.  |z| <= 8.2096 (u = 2^-53): a seeded call never draws beyond that, where an input array may
 *   t        the index in the array's own first dimension: the day k - k0 of epi_sdraw_*, the step of the simulators, the
 *            forecast day of epi_arfc_*;  lane: the path p of epi_sdraw_*, the chain c of the others
 *   rows 0 and 1 of a (t, lane) cost one block; row 2, and the single row of epi_arfc_*, use one block and discard half of it.
 *   Nothing depends on launch geometry, lane_block, launch cuts or k0 beyond the t above. */
typedef struct epi_noise_desc {
    int32_t abi_version;
    uint32_t seed_lo, seed_hi;   /* the Philox key */
    uint32_t stream;             /* < 2^30: independent arrays under one seed */
} epi_noise_desc;
/* no GPU needed: EPI_ERR_BAD_ARG for a NULL descriptor, another ABI version, stream >= 2^30 */
int epi_noise_validate(const epi_noise_desc *d, char *err);
/* The window [t0, t0 + nt) x rows x [lane0, lane0 + n_lanes) of the logical array into out [nt][rows][n_lanes], double (out_f32 = 0)
 * or float (1: the double draw rounded once).  DEVICE pointer; one kernel, cut into launches below 2^31 threads, enqueued on
 * `stream`.  EPI_ERR_BAD_ARG for rows outside {1, 3}, nt or n_lanes < 1, t0 < 0 or t0 + nt > 2^32 (t is one counter word), lane0 < 0 or
 * lane0 + n_lanes > 2^63, out_f32 outside {0, 1}, a NULL out, more than 2^62 elements.  test_launch_groups: 0; > 0: workgroups per
 * launch (the tests cut small calls into several launches with it) */
int epi_noise_fill_device(const epi_noise_desc *d, int64_t t0, int64_t nt, int32_t rows, int64_t lane0, int64_t n_lanes, int32_t out_f32,
                          void *out, int32_t test_launch_groups, void *stream, char *err);
/* HOST pointer, on a pooled context of `device` */
int epi_noise_fill_host(const epi_noise_desc *d, int64_t t0, int64_t nt, int32_t rows, int64_t lane0, int64_t n_lanes, int32_t out_f32,
                        void *out, int device, char *err);
/* The seeded siblings: the arguments of the unseeded call with `noise` behind the descriptor.  z must be NULL (EPI_ERR_BAD_ARG: the
 * draws have one source) and the descriptor's own noise / z_f32 field is not read: the noise term is always formed.  The host forms
 * copy no z. */
int epi_sdraw_run_device_seeded(const epi_sdraw_desc *d, const epi_noise_desc *noise, const epi_sdraw_inputs *in, const epi_sdraw_outputs *out,
                                void *ws, size_t ws_bytes, void *stream, char *err);
int epi_sdraw_run_host_seeded(const epi_sdraw_desc *d, const epi_noise_desc *noise, const epi_sdraw_inputs *in, const epi_sdraw_outputs *out,
                              int device, char *err);
int epi_arfc_run_device_seeded(const epi_arfc_desc *d, const epi_noise_desc *noise, const epi_arfc_inputs *in, const epi_arfc_outputs *out,
                               void *stream, char *err);
int epi_arfc_run_host_seeded(const epi_arfc_desc *d, const epi_noise_desc *noise, const epi_arfc_inputs *in, const epi_arfc_outputs *out,
                             int device, char *err);
int epi_sialpha_sim_device_seeded(const epi_sim_desc *d, const epi_noise_desc *noise, const int32_t *u_series, const double *u,
                                  const double *sp, const double *z, double *s, double *i, double *alpha, double *J0, double *J1,
                                  void *stream, char *err);
int epi_sialpha_score_device_seeded(const epi_sim_desc *d, const epi_noise_desc *noise, const int32_t *u_series, const double *u,
                                    const double *sp, const double *z, const double *J0_prefix, const double *J1_prefix, double *s,
                                    double *i, double *alpha, double *J0, double *J1, void *stream, char *err);
int epi_sialpha_sim_host_seeded(const epi_sim_desc *d, const epi_noise_desc *noise, const int32_t *u_series, const double *u,
                                const double *sp, const double *z, double *s, double *i, double *alpha, double *J0, double *J1,
                                int device, char *err);
int epi_random_npi_mc_device_seeded(const epi_mc_desc *d, const epi_noise_desc *noise, const double *sp, const double *u_min,
                                    const double *z, const double *J0_prefix, const double *J1_prefix, double *u_out, double *J0,
                                    double *J1, void *stream, char *err);
int epi_random_npi_mc_host_seeded(const epi_mc_desc *d, const epi_noise_desc *noise, const double *sp, const double *u_min,
                                  const double *z, const double *J0_prefix, const double *J1_prefix, double *u_out, double *J0,
                                  double *J1, int device, char *err);

/* ---- Whiteness diagnostics of the innovations of every chain ----
 * The definition and the structures epi_idiag_desc / _inputs / _outputs are in epiekf_idiag.h (tests/test_noise_abi.py pins the
 * set of structures this file itself defines, so a new call's structures get a header of their own). */
#ifdef __cplusplus
}
#endif
#include "epiekf_idiag.h"
#ifdef __cplusplus
extern "C" {
#endif
/* no GPU needed: EPI_ERR_BAD_ARG with a message for anything outside the limits, EPI_ERR_UNSUPPORTED for n_lags above 64, T of
 * 2^21 or more, or B * ceil(T / 32) of 2^31 or more */
int epi_idiag_validate(const epi_idiag_desc *d, char *err);
/* bytes of device workspace epi_idiag_run_device needs (the per-block records of the two passes) */
int epi_idiag_workspace_bytes(const epi_idiag_desc *d, size_t *bytes, char *err);
/* DEVICE pointers; four kernels enqueued on `stream`: no host synchronisation, no allocation, no second stream.
 * EPI_ERR_WORKSPACE for a workspace below epi_idiag_workspace_bytes */
int epi_idiag_run_device(const epi_idiag_desc *d, const epi_idiag_inputs *in, const epi_idiag_outputs *out, void *ws,
                         size_t ws_bytes, void *stream, char *err);
/* HOST pointers, on a pooled context of `device` (the workspace lives in its arena) */
int epi_idiag_run_host(const epi_idiag_desc *d, const epi_idiag_inputs *in, const epi_idiag_outputs *out, int device, char *err);

/* ---- Curve statistics of the Monte-Carlo ensembles: modified band depth, central envelopes, functional boxplot ----
 * The definition and the structures epi_cdepth_desc / _inputs / _outputs are in epiekf_cdepth.h. */
#ifdef __cplusplus
}
#endif
#include "epiekf_cdepth.h"
#ifdef __cplusplus
extern "C" {
#endif
/* no GPU needed: EPI_ERR_BAD_ARG for what epi_pathfn_validate refuses of T, rows, R, D, k0 / k1, storage, derive_newcases,
 * test_segments and test_launch_groups, and for D > 4096, n_alpha outside 0 .. 8, an alpha outside (0, 1] or not strictly
 * ascending, a negative or NaN fence_factor, with fence_factor > 0 a fence_frac outside (0, 1], env_lo / env_hi with n_alpha = 0,
 * out_days / n_outliers / whisk_lo / whisk_hi with fence_factor = 0, a NULL src, no output at all */
int epi_cdepth_validate(const epi_cdepth_desc *d, const epi_cdepth_inputs *in, const epi_cdepth_outputs *out, char *err);
/* bytes of device workspace epi_cdepth_run_device needs: the 32-day block records of every path and whatever a later pass reads
 * (depth, ranks, fence envelope, out_days), whether the caller asks for it or not */
int epi_cdepth_workspace_bytes(const epi_cdepth_desc *d, size_t *bytes, char *err);
/* DEVICE pointers; the depth pass (one wavefront per (row, region, 32-day block)), its combining pass, and as far as the
 * outputs asked for need them the rank, envelope, fence, outlier and whisker passes, enqueued on `stream` in launches of at most
 * 2^22 workgroups: no host synchronisation, no allocation.  EPI_ERR_WORKSPACE for a workspace below epi_cdepth_workspace_bytes */
int epi_cdepth_run_device(const epi_cdepth_desc *d, const epi_cdepth_inputs *in, const epi_cdepth_outputs *out, void *ws,
                          size_t ws_bytes, void *stream, char *err);
/* HOST pointers, on a pooled context of `device` (the workspace lives in its arena) */
int epi_cdepth_run_host(const epi_cdepth_desc *d, const epi_cdepth_inputs *in, const epi_cdepth_outputs *out, int device, char *err);

/* Measurement utility (not part of the reference's interface): copies n doubles src -> dst with the filter
 * kernels' access shape (8 B per lane); used to calibrate the HBM traffic counters on a known byte count. */
int epi_calib_copy_f64_device(const double *src, double *dst, size_t n, void *stream, char *err);

const char *epi_status_string(int status);
int epi_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif

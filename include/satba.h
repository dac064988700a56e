/*
 * satba.h -- C ABI of libsatba_hip.so: the bundle-adjustment least-squares hot path on MI355X (gfx950).
 *
 * The reference (centreborelli/sat-bundleadjust) has no FFI for this path: the boundary is the Python call
 * surface of bundle_adjust/ba_core.py and bundle_adjust/ba_params.py.  This header is what a native binding
 * of that surface needs; each entry point names the reference code it replaces (paths relative to the
 * reference tree, scipy paths relative to scipy 1.15.3).  The only caller in this repository is the ctypes
 * shim sat-bundleadjust_amd/satba/engine_hip.py; INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success or a negative SATBA_E_* code and never throws;
 *     satba_last_error() returns a thread-local description of the last failure.
 *   - "host" pointers are caller-owned host memory, copied before the call returns (after a stream sync for
 *     outputs).  "device" pointers are HIP device memory on the problem's device.
 *   - one solve per handle at a time (the reference is single-threaded and non-reentrant as well).
 *   - all arithmetic is IEEE float64; the only float32 is the optional rounding of RPC projections that
 *     mirrors ba_core.py:150.
 *
 * Variable vector (ba_params.py:152-172):  x = [cam 0 (n_params) | ... | cam M-1 | pt 0 (3) | ... | pt N-1 (3)]
 *   a camera's n_params entries are the first n_params of its cam_params row: angles (3), then T, then the intrinsics
 *   (affine fx fy skew, perspective fx fy skew cx cy; n_params 8 / 11 -- satba_version() >= 4)
 * Residual vector (ba_core.py:180-181):   r = [x0, y0, x1, y1, ...] = w_k * (projection_k - observation_k)
 *
 * Multi-GPU: one process and one handle per GPU.  Each handle holds ALL cameras and a contiguous shard of the
 * points with their observations.  Camera-side sums leave the device through the exchange buffer
 * (satba_bind_exchange), which the host all-reduces (RCCL through torch.distributed) between phases; `rank`
 * and `world` only decide who contributes the camera-only terms (rank 0) and which header slot a rank owns.
 */
#ifndef SATBA_H
#define SATBA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { SATBA_AFFINE = 0, SATBA_PERSPECTIVE = 1, SATBA_RPC = 2 };
/* losses of scipy.optimize.least_squares (scipy:optimize/_lsq/least_squares.py:172-207) */
enum { SATBA_LOSS_LINEAR = 0, SATBA_LOSS_SOFT_L1 = 1, SATBA_LOSS_HUBER = 2, SATBA_LOSS_CAUCHY = 3, SATBA_LOSS_ARCTAN = 4 };

enum {
    SATBA_OK = 0,
    SATBA_E_ARG = -1,      /* invalid argument (the Python shim raises ValueError)        */
    SATBA_E_HIP = -2,      /* HIP runtime error (RuntimeError)                             */
    SATBA_E_STATE = -3,    /* phase called out of order                                    */
    SATBA_E_NONFINITE = -4 /* non-finite residuals where the reference raises ValueError   */
};

/* per-camera RPC record: col_num[20] col_den[20] row_num[20] row_den[20]
 * lon_off lon_scale lat_off lat_scale alt_off alt_scale col_off col_scale row_off row_scale
 * (attribute names of rpcm.RPCModel; polynomial term order of ba_rpcfit.py:17-44 == c/rpc.c:285-289) */
#define SATBA_RPC_TABLE_LEN 90

/* exchange-buffer header: SATBA_HDR_FIXED scalars + one slot per rank, rounded up to an even count */
#define SATBA_HDR_FIXED 16
/* after satba_solve, header slots SATBA_HDR_KEEP .. +SATBA_KEEP_LEN-1 repeat the scalars of the earlier phases of the
 * same iteration: cost, |g|_inf, |g_h|^2, |J_h g_h|^2, |x_h|^2, damping used, trust radius used (0 unless
 * satba_schur_auto computed them), and SATBA_HDR_FX_BAD: non-zero when the fixed-point camera sums of the linearisation left
 * their range (the iteration is void: call satba_camera_sums_fallback and repeat it; satba_solve_lm / satba_lm_step and
 * satba/trf.py do) */
#define SATBA_HDR_KEEP 8
#define SATBA_KEEP_LEN 8
#define SATBA_HDR_FX_BAD 15
/* The fixed slots, per phase: every phase zeroes the header and then gives the low slots its own meaning (the same table, with the
 * same values, is satba/trf.py's; tests/test_host_logic.py holds the two together). */
/* left by satba_linearize (rank r also leaves |g_p|_inf of its shard in slot SATBA_HDR_FIXED + r): */
#define SATBA_HDR_COST 0
#define SATBA_HDR_FX 5      /* a term of the fixed-point camera sums exceeded its bound, or a free camera's diag U_c terms all lie below their unit (summed over ranks) */
#define SATBA_HDR_PREP_GH 6 /* point sums of |g_h|^2, |x_h|^2 when the linearisation did the point part of the prepare phase */
#define SATBA_HDR_PREP_XS 7
/* left by satba_prepare: |g_h|^2, |J_h g_h|^2, |x_h|^2, lead * |g_c|_inf */
#define SATBA_HDR_GH_SQ 1
#define SATBA_HDR_JG_SQ 2
#define SATBA_HDR_XS_SQ 3
#define SATBA_HDR_GC_INF 4
/* left by satba_solve and satba_solve_messages_end: Gram matrix of (g_h, gn_h), status word of the factorisation (written by rank 0
 * alone: headers are summed over the ranks), and the kept scalars in slots SATBA_HDR_KEEP + SATBA_KEEP_* (the last of them is
 * SATBA_HDR_FX_BAD) */
#define SATBA_HDR_GRAM_A 1
#define SATBA_HDR_GRAM_B 2
#define SATBA_HDR_GRAM_C 3
#define SATBA_HDR_CHOL_FAIL 4
#define SATBA_KEEP_COST 0
#define SATBA_KEEP_GINF 1
#define SATBA_KEEP_GH_SQ 2
#define SATBA_KEEP_JG_SQ 3
#define SATBA_KEEP_XS_SQ 4
#define SATBA_KEEP_LAM 5
#define SATBA_KEEP_DELTA 6
#define SATBA_KEEP_FX_BAD 7
/* bits of the status word in SATBA_HDR_CHOL_FAIL (0: factorised): the system is not positive definite; a wait timed out; that wait
 * was one BETWEEN the factorisation and the kernel producing its input beside it on another stream -- the two did not run at the same
 * time, the front is repeated one kernel after the other with the same damping (one rank: the word is >= SATBA_CHOL_BESIDE_WAIT) */
#define SATBA_CHOL_NOT_SPD 1
#define SATBA_CHOL_TIMEOUT 2
#define SATBA_CHOL_BESIDE_WAIT 4
/* left by satba_subspace: w.w, w.q1, g_h.w */
#define SATBA_HDR_WW 1
#define SATBA_HDR_WQ1 2
#define SATBA_HDR_GHW 6
/* left by satba_subspace_products: |J_h q1|^2, (J_h q1).(J_h w), |J_h w|^2 */
#define SATBA_HDR_B11 3
#define SATBA_HDR_B12 4
#define SATBA_HDR_B22 5
/* left by satba_trial and satba_trial_gn: cost at x_new, |step|^2, |x|^2 */
#define SATBA_HDR_COST_NEW 1
#define SATBA_HDR_STEP_SQ 2
#define SATBA_HDR_X_SQ 3

typedef struct satba_problem satba_problem;

/* satba_problem_desc.flags.  Every run is bitwise repeatable: all reductions of the library have a fixed order except the
 * per-camera sums of the linearisation, and those are accumulated in 64-bit fixed point (integer addition does not depend on the
 * order; csrc/satba_kernels.h, k_linearize).  CAMERA_MAJOR_SUMS (the former DETERMINISTIC flag, same value; environment
 * variable SATBA_DETERMINISTIC) selects the other route to the same property from the start: a camera-major pass in float64 with
 * a fixed order (k_cam_sums; one extra pass over the observations per linearisation, one lane per point) -- the route a solve
 * falls back to when a term leaves the fixed-point range (satba_camera_sums_fallback). */
#define SATBA_FLAG_DETERMINISTIC 1
#define SATBA_FLAG_CAMERA_MAJOR_SUMS 1

typedef struct satba_problem_desc {
    int32_t cam_model;      /* SATBA_AFFINE | SATBA_PERSPECTIVE | SATBA_RPC  (BundleAdjustmentParameters.cam_model) */
    int32_t n_cam;          /* M                                                                    */
    int32_t n_pts;          /* N: points held by this handle                                        */
    int32_t n_params;       /* optimised parameters per camera: 3 (R) | 5 (affine R+T) | 6 (R+T) |
                               8 (affine R+T+K) | 11 (perspective R+T+K)                              */
    int32_t cam_param_len;  /* columns of cam_params: 8 affine, 11 perspective, 9 rpc (ba_params.py:19-44) */
    int32_t n_cam_fix;      /* first n_cam_fix cameras are frozen (ba_params.py:246-249)             */
    int32_t n_pts_fix;      /* first n_pts_fix LOCAL points are frozen (ba_params.py:240-243)        */
    int32_t rank, world;    /* position of this shard; 0, 1 for a single GPU                        */
    int32_t rpc_store_f32;  /* non-zero: round RPC projections to float32 like ba_core.py:150        */
    int32_t device;         /* HIP device ordinal                                                    */
    int32_t flags;          /* SATBA_FLAG_* bits                                                     */
    int64_t n_obs;          /* K: observations held by this handle                                   */
    int64_t n_total;        /* size of the global variable vector (only used for default max_nfev)   */
    const double *cam_params;  /* host, M x cam_param_len, row-major (BundleAdjustmentParameters.cam_params) */
    const double *rpc_tables;  /* host, M x SATBA_RPC_TABLE_LEN, or NULL unless cam_model == SATBA_RPC */
    const int32_t *cam_ind;    /* host, K: camera of each observation                                */
    const int32_t *pts_ind;    /* host, K: LOCAL point of each observation, non-decreasing (point-major,
                                  the order ba_params.py:142-147 produces)                           */
    const double *pts2d;       /* host, K x 2 observed (col, row)                                    */
    const double *weights;     /* host, K (BundleAdjustmentParameters.pts2d_w)                       */
} satba_problem_desc;

const char *satba_last_error(void);
int satba_version(void);

/* Upload a problem (replaces the per-call numpy gathers of ba_core.py:72-81, 97-107, 147-153) and build its index structures
 * on the device: points sorted by track length into 64-point slices (sliced-ELL observation order), camera-major lists,
 * per-camera-pair lists of shared points (csrc/satba_layout.h).  pts_ind must be non-decreasing and the cameras of a point
 * strictly ascending -- the order ba_params.py:142-147 emits. */
int satba_problem_create(const satba_problem_desc *desc, satba_problem **out);
void satba_problem_destroy(satba_problem *p);

/* A handle launches everything on a stream of its own (created non-blocking with the handle).  satba_set_stream moves it to
 * `hip_stream` (a hipStream_t; NULL = the legacy default stream) -- e.g. the stream torch.distributed queues its collectives on --
 * or, with use_own != 0, back to its own. */
int satba_set_stream(satba_problem *p, void *hip_stream, int32_t use_own);

/* Length in doubles of the exchange buffer: header + max(M n_p^2 + M n_p, (M n_p)^2 + M n_p). */
int64_t satba_exchange_len(const satba_problem *p);
int64_t satba_header_len(const satba_problem *p);
/* Use caller-provided device memory (e.g. a torch tensor that torch.distributed will all-reduce) as the
 * exchange buffer; NULL restores the internally allocated one. */
int satba_bind_exchange(satba_problem *p, double *device_ptr, int64_t len);

/* The reduced camera system S is symmetric and only its lower triangle is formed and used: for the all-reduce between
 * ranks (no counterpart in the reference) the Schur payload [header | S (n_c^2) | rhs (n_c)] of the
 * exchange buffer is packed to [header | rhs | lower triangle, column-major, n_c (n_c + 1) / 2] in caller-provided device
 * memory (again typically a torch tensor), all-reduced there, and unpacked -- half the bytes over xGMI.
 * satba_packed_schur_len: length of that packed buffer in doubles. */
int64_t satba_packed_schur_len(const satba_problem *p);
int satba_pack_schur(satba_problem *p, double *packed_device_ptr);
int satba_unpack_schur(satba_problem *p, const double *packed_device_ptr);

/* The same exchange in MESSAGES, the dense factorisation beside it (round 6; replaces, for several ranks, the one LSMR call of
 * scipy:optimize/_lsq/trf.py:479-480 on the all-reduced system): the packed payload is cut at camera boundaries into
 * satba_solve_messages() pieces of about equal size -- bounds[m] .. bounds[m + 1] is the index range of message m, the first one
 * carries header and right-hand side; returns 0 when this handle solves its system in one piece (fewer than 129 or more than 1 024
 * unknowns: pack, all-reduce, unpack, satba_solve), -1 on a bad argument.  satba_solve_messages_begin packs the payload (unless
 * packed_already: satba_pack_schur has been called and the messages have ALL been reduced -- for collectives that block the host or
 * synchronise the device, e.g. gloo on device tensors, which would wait for the waiting factorisation) and launches
 * the factorisation on a stream of the handle's own, where it waits for tile columns; after the all-reduce of message m (a library
 * that queues it on the handle's stream: RCCL) satba_solve_messages_arrived unpacks its columns and releases the tiles they complete;
 * satba_solve_messages_end queues the rest of the solve phase (what satba_solve leaves behind: step and header).  Same arithmetic in
 * the same order as satba_solve on the unpacked system: the same bits.  _bind names the payload for the device-resident loop's parts
 * 10 (begin), 11 (arrived; the message index travels in lam_floor) and 12 (end) of satba_lm_part. */
int32_t satba_solve_messages(satba_problem *p, int64_t *bounds, int32_t cap);
int satba_solve_messages_bind(satba_problem *p, double *packed_device_ptr);
int satba_solve_messages_begin(satba_problem *p, double *packed_device_ptr, int32_t packed_already);
int satba_solve_messages_arrived(satba_problem *p, const double *packed_device_ptr, int32_t m);
int satba_solve_messages_end(satba_problem *p);

/* loss and f_scale of least_squares (ba_core.py:292-293). */
int satba_configure(satba_problem *p, int32_t loss, double f_scale);

int satba_set_x(satba_problem *p, const double *host_x);  /* n_cam*n_params + 3*n_pts doubles */
int satba_get_x(satba_problem *p, double *host_x);

/* ba_core.fun (ba_core.py:157-183) at the current x: residuals (2K doubles, may be NULL) and the cost
 * 0.5 * sum rho(f^2) (scipy:optimize/_lsq/trf.py:413-418). */
int satba_residuals(satba_problem *p, double *host_r, double *host_cost);

/* ---- phases of one trust-region iteration (satba/trf.py; scipy:optimize/_lsq/trf.py:450-551).
 * Each phase zeroes the exchange header, then writes its slots (SATBA_HDR_* above).                        */

/* residuals + analytic Jacobian -> normal-equation blocks at x.  Replaces scipy's finite-difference
 * Jacobian (scipy:optimize/_numdiff.py:628-705), compute_grad (common.py:590-595) and the robust
 * rescaling (common.py:720-731).  Exchange payload: U (M x n_p x n_p) | g_c (M x n_p); only diag(U_c) is
 * guaranteed (the off-diagonal entries are formed in the Schur phase by its camera-major pass).           */
int satba_linearize(satba_problem *p);
/* after the all-reduce: x_scale="jac" update (common.py:598-610), g_h, |J_h g_h|^2 for the Cauchy step
 * (trf.py:473-477).                                                                                       */
int satba_prepare(satba_problem *p, int32_t first);
/* local part of the reduced camera system  S = U + lam Dc^2 - sum_p W (V + lam Dp^2)^-1 W^T  and its
 * right-hand side; replaces LSMR (trf.py:479-480).  Exchange payload: S (n_c x n_c, column-major lower) | rhs. */
int satba_schur(satba_problem *p, double lam);
/* The same with the damping computed on the device from the (all-reduced) header of satba_prepare, exactly as the
 * host does it for satba_schur: scipy's Cauchy-step regulariser (scipy:optimize/_lsq/trf.py:473-477,
 * common.py:302-322) for the trust radius Delta, floored at lam_floor.  Delta <= 0 selects scipy's initial radius
 * |x_h| (trf.py:440-442).  linearize -> prepare -> schur_auto -> solve can then be queued without a host
 * round trip; satba_solve repeats the scalars the host would have read in between in header slots SATBA_HDR_KEEP.. */
int satba_schur_auto(satba_problem *p, double Delta, double lam_floor);
/* after the all-reduce: dense Cholesky solve, point back-substitution, Gram matrix of (g_h, gn_h).        */
int satba_solve(satba_problem *p);
/* basis of span{g_h, gn_h} (trf.py:481-482): q1 = inv_norm_g * g_h, w = gn_h - alpha * g_h, and their dots.
 * The quadratic model on that basis (trf.py:483-485) follows on the host from the normal equations,
 * J_h^T J_h gn_h = g_h - reg gn_h, without another pass over the observations (satba/trf.py);
 * satba_subspace_products computes the three products |J_h q1|^2, (J_h q1).(J_h w), |J_h w|^2 explicitly
 * (header slots SATBA_HDR_B11 .. _B22) for the ill-conditioned case and for the tests.                                      */
int satba_subspace(satba_problem *p, double alpha, double inv_norm_g);
int satba_subspace_products(satba_problem *p);
/* x_new = x + scale * (p0 q1 + p1 w); cost at x_new (trf.py:497-512).                                     */
int satba_trial(satba_problem *p, double p0, double p1);
/* the same step written on (g_h, gn_h): x_new = x + scale * (ca g_h + cb gn_h); needs no satba_subspace.           */
int satba_trial_gn(satba_problem *p, double ca, double cb);
int satba_accept(satba_problem *p);
/* Form the per-camera sums of the following linearisations with the camera-major float64 pass instead of the fixed-point LDS
 * table.  For callers that drive the phases themselves: call it when header slot SATBA_HDR_FX_BAD is non-zero after satba_solve
 * and repeat the iteration from satba_linearize.  (No counterpart in the reference.) */
int satba_camera_sums_fallback(satba_problem *p);
/* synchronise the stream and copy the exchange header to the host. */
int satba_read_header(satba_problem *p, double *host_hdr);

/* One fixed-work Levenberg-Marquardt iteration of a single-rank handle with the host side in C++: linearize, prepare, damped
 * Gauss-Newton step, 2-D trust-region subproblem, trial point, accept if the cost went down -- the body of satba_solve_lm's
 * loop without its termination tests (ref: scipy optimize/_lsq/trf.py:trf_no_bounds, one pass).  bench.py times this.
 * first != 0: first iteration (Jacobian scaling and trust radius are initialised; Delta is ignored).
 * out[8]: cost at x, cost at the trial point, new trust radius, accepted (0/1), interior Newton step (0/1), predicted reduction,
 * actual reduction, damping. */
int satba_lm_step(satba_problem* p, int32_t first, double Delta, double lam_floor, double* out);

/* The same iterations WITHOUT a host round trip (round 3; csrc/satba_lmdev.h): the loop's decisions -- scipy's top-of-loop tests,
 * damping escalation after a failed factorisation, the 2-D trust-region subproblem, radius update, accept / reject -- are taken by
 * one-thread kernels on the device, every kernel of an iteration reads a gate word of the loop's state in device memory, accepted
 * points are copied on the device, and the host only queues launches (a few iterations ahead of the device's progress reports in
 * pinned memory).  satba_lm_run performs n_iterations fixed-work iterations (no termination tests: satba_lm_step's semantics) from
 * the current x; cycle_len > 0: every cycle_len iterations the solve starts again from the point kept by satba_snapshot_x (what
 * bench.py does with the solve that the shipped tolerances end after that many iterations).  It returns when the device is done.
 * out (may be NULL; n_out >= 16), also returned by satba_lm_state: [0..7] as satba_lm_step for the last iteration ([3], [4]: totals
 * of accepted and interior steps), [8] phase (0 running, 1 finished, 2 stopped for the host), [9] scipy status, [10] nfev, [11] njev,
 * [12] iterations, [13] launch patterns ("ticks") executed, [14] reason of phase 2 (1 fixed-point overflow of the camera sums,
 * 2 factorisation failed ten times, 3 non-finite residuals at the start), [15] |g|_inf.  satba_solve_lm runs on the same
 * machinery with scipy's termination tests switched on.  Single-rank handles only. */
int satba_lm_run(satba_problem* p, int64_t n_iterations, int32_t cycle_len, double lam_floor, double* out, int32_t n_out);
int satba_lm_state(satba_problem* p, double* out, int32_t n);

/* The scalar side of the loop on its own, for tests of the two compilations this library carries of it (csrc/satba_lm.h): n rows
 * in = a b c g0 g1 Delta (host pointers, float64) of the model min 1/2 p^T [[a b] [b c]] p + g^T p, |p| <= Delta; per row
 * out = p0 p1 newton Delta_new ratio term -- the trust-region step and its Newton flag, then update_tr_radius and
 * check_termination fed from that step as the loop feeds them (satba_lm::lm_scalars_row).  device == 0: the host compilation (the
 * host loop's); device == 1: the device compilation (the decision kernels'), one thread per row on the default stream of the current
 * device.  No handle.  n == 0 returns 0 without a launch.  SATBA_E_ARG, before the device is touched: device not 0 or 1, n < 0 or
 * n > 2^24, a null pointer with n > 0. */
int satba_lm_scalars(int32_t device, int64_t n, const double *in, double *out);

/* ---- one-shot solve: the whole trust-region loop (scipy:optimize/_lsq/trf.py:401-560 as ba_core.py:284-297 configures it,
 * with the exact damped step of this library) below the ABI, for callers that do not want to drive the phases themselves.
 * Starts from the current x (satba_set_x), leaves the solution in the handle (satba_get_x, satba_residuals).  Single-rank
 * handles only (world == 1): with several ranks the exchange buffer must be all-reduced between the phases by the caller.
 * status, nfev: scipy's (0 max_nfev reached, 1 gtol, 2 ftol, 3 xtol, 4 ftol and xtol).  max_nfev <= 0: 100 * n_total. */
typedef struct satba_lm_opts {
    double ftol, xtol, gtol, f_scale;
    int64_t max_nfev;
    int32_t loss;     /* SATBA_LOSS_* */
    int32_t verbose;  /* 0 silent, 1 final message, 2 scipy's iteration table */
} satba_lm_opts;
typedef struct satba_lm_stats {
    double cost, initial_cost, optimality;
    int64_t nfev, njev, iterations;
    int32_t status, reserved;
} satba_lm_stats;
int satba_solve_lm(satba_problem *p, const satba_lm_opts *opts, satba_lm_stats *stats);

/* The device-resident loop for several ranks (replaces the host side of scipy:optimize/_lsq/trf.py:450-551 when the points are sharded,
 * north_star: "LM outer loop on device ... points shard across the 8 GPUs").  A tick is queued in parts with the caller's all-reduces
 * of the exchange buffer between them (torch.distributed on the handle's stream; satba/trf.py: trf_solve_sharded):
 *     0 | linearize payload | 1 | header | 2 | reduced system | 3 | header | 4 | header | 5
 * and the degenerate-subspace pattern  6 | header | 7 | header | 8 | header | 9.  Nothing waits for the device; the decisions are taken
 * by one-thread kernels on all-reduced scalars, identically on every rank.  satba_lm_begin: reset the loop (o: tolerances, loss;
 * never_stop / max_iterations / cycle_len as satba_lm_run).  satba_lm_poll (no wait): out[0] patterns executed, [1] phase (0 running,
 * 1 done, 2 needs the host, 3 paused for the subspace pattern), [2] pauses so far, [3] tick of the latest pause, [4] tick at which the
 * loop left the running phase (0: not yet).  Every rank must queue exactly out[4] + 3 patterns.  satba_lm_state returns the scalars. */
int satba_lm_begin(satba_problem* p, const satba_lm_opts* o, int32_t never_stop, int64_t max_iterations, int32_t cycle_len);
int satba_lm_part(satba_problem* p, int32_t part, double lam_floor);
int satba_lm_poll(satba_problem* p, int64_t* out, int32_t n);

/* ---- outlier rejection between the two solves of the pipeline (ba_outliers.py:14-58, 112-155): per-camera elbow threshold
 * on the reprojection errors of the current x and the observations above it.
 * err (host, K, caller's observation order, may be NULL: computed from the residuals at the current x as
 * ba_core.compute_reprojection_error does); predef_thr < 0: automatic (elbow) thresholds, NaN: SATBA_E_ARG (a caller that means a
 * negative threshold gets no silent elbow rule: the Python layer refuses both); outputs: cam_thr (host, M),
 * remove (host, K bytes: 1 = observation is an outlier), n_removed. */
int satba_outliers(satba_problem *p, const double *err, double predef_thr, double min_thr, double *cam_thr, uint8_t *remove,
                   int64_t *n_removed);

/* ba_core.compute_reprojection_error(ba_core.fun(x, p), p.pts2d_w) (ref:bundle_adjust/ba_core.py:335-349 on :157-183) at the current
 * x without the residual vector crossing the bus: host_err (K doubles, caller's observation order) = || f_k / w_k ||_2, the
 * reference's operations with their roundings (bit-identical to the host formula); host_cost (optional): 0.5 |f|^2.  What
 * ref:bundle_adjust/ba_core.py:277,303-304 computes before and after the solve.                                                  */
int satba_reprojection_errors(satba_problem *p, double *host_err, double *host_cost);
/* The same in two steps (round 6): _begin queues the error kernels at the current x into a device buffer of the handle and returns
 * without waiting; _fetch moves the K errors to host_err and may be called from ANOTHER host thread while this handle runs the solve
 * that follows -- the download of ref:bundle_adjust/ba_core.py:277's initial errors then overlaps the region :283-299 times.  One
 * _fetch per _begin; the values are those of the x at _begin whatever the handle has done since.                                  */
int satba_reprojection_errors_begin(satba_problem *p);
int satba_reprojection_errors_fetch(satba_problem *p, double *host_err);

/* device-side copy of the current point (no host transfer): restore == 0 keeps x, restore != 0 returns to the kept x, as
 * satba_set_x with the same vector would.  bench.py restarts its solve with it; a caller can use it to retry a solve. */
int satba_snapshot_x(satba_problem *p, int32_t restore);

/* ---- initial triangulation of the feature tracks, the step before the path.  Stand-alone: no problem handle.
 * cameras: n_cam x 12 (3 x 4 projection matrices, row-major; affine and perspective) or n_cam x SATBA_RPC_TABLE_LEN (rpc).
 *
 * satba_triangulate_pairwise replaces ft_triangulate.linear_triangulation_multiple_pts (ft_triangulate.py:18-34, the
 * cv2.triangulatePoints call) and ft_triangulate.rpc_triangulation (ft_triangulate.py:37-54 -> s2p/triangulation.py:82-135 ->
 * c/disp_to_h.c:40-64 `stereo_corresp_to_lonlatalt`): n correspondences (pts_i, pts_j: host, n x 2, (col, row)) between two
 * cameras -> pts3d (host, n x 3 float64, ECEF for rpc) and, for rpc, err (host, n float32, may be NULL: distance to the epipolar
 * curve in pixels).  kernel_ms (may be NULL): duration of the kernel from HIP events.
 *
 * satba_init_pts3d replaces ft_triangulate.init_pts3d (ft_triangulate.py:57-127): every track is triangulated from every listed
 * pair (pairs: host, n_pairs x 2, the reference's pairs_to_triangulate, processed in list order; pairs naming a camera >= n_cam
 * are skipped as at :99) whose two cameras observe it, and the results are folded into a float32 running mean with the
 * reference's sequence of float32 operations.  The tracks come as the observation lists of ba_params.py:142-147 instead of the
 * dense NaN-sparse C matrix: pt_ofs (host, n_pts + 1, pt_ofs[0] = 0), cam_ind (host, K), obs (host, K x 2).  Outputs: pts3d
 * (host, n_pts x 3 float32; zero where no pair applies, like the reference), n_tri (host, n_pts, may be NULL: triangulations
 * per track).  reps >= 1: the kernel is launched reps times (measurement), kernel_ms (may be NULL) = average duration. */
int satba_triangulate_pairwise(int32_t cam_model, const double *cam_i, const double *cam_j, int64_t n, const double *pts_i,
                               const double *pts_j, double *pts3d, float *err, int32_t device, float *kernel_ms);
int satba_init_pts3d(int32_t cam_model, int32_t n_cam, int64_t n_pts, const int64_t *pt_ofs, const int32_t *cam_ind,
                     const double *obs, const double *cameras, int32_t n_pairs, const int32_t *pairs, float *pts3d,
                     int32_t *n_tri, int32_t device, int32_t reps, float *kernel_ms);
/* The same on a problem handle's RESIDENT observations -- what ba_outliers.py:89-93 does right after the outlier rejection: the
 * tracks are not uploaded again.  remove (host, n_obs bytes in the caller's observation order, e.g. satba_outliers' mask; may be
 * NULL): observations to treat as absent.  cameras: host, n_cam x (12 | SATBA_RPC_TABLE_LEN) -- the caller's choice (the
 * reference passes p.cameras).  pts3d (host, n_pts x 3 float32) and n_tri (host, n_pts, may be NULL) in the caller's point order;
 * a track with n_tri = 0 is one ft_utils.filter_C_using_pairs_to_triangulate would drop.  Single-rank handles only. */
int satba_init_pts3d_resident(satba_problem *p, const uint8_t *remove, const double *cameras, int32_t n_pairs,
                              const int32_t *pairs, float *pts3d, int32_t *n_tri, float *kernel_ms);

/* ---- selection of the feature tracks, the step between the triangulation and the path (ft_ranking.py).  Stand-alone: no
 * problem handle.  The tracks come as the lists of the triangulation entry above: pt_ofs (host, n_pts + 1, pt_ofs[0] = 0), cam_ind
 * (host, K; cameras ascend strictly inside a track), plus scale and err (host, K: keypoint scale and reprojection error of every
 * observation; err == NULL: zeros, as ba_pipeline.py does while there are no 3-D points).
 *
 * satba_track_keys: the three ranking keys of ft_ranking.order_tracks (ft_ranking.py:145-147): length (observations), key_scale
 * (np.round of the mean scale to 2 decimals), key_cost (mean error); bit-identical to numpy's given the same inputs.
 *
 * satba_track_connectivity replaces ft_ranking.build_connectivity_matrix (ft_ranking.py:19-34): A (host, n_cam x n_cam int32) =
 * tracks seen by both cameras, zero diagonal, entries below min_matches zeroed (:32).  alive (host, n_pts bytes, may be NULL):
 * tracks with a zero byte are left out.
 *
 * satba_select_tracks replaces ft_ranking.select_best_tracks (ft_ranking.py:136-153 order_tracks, :232-263 get_tracks, :197-229
 * get_tracks_current_tree, :83-118 compute_camera_weights): K spanning trees over the camera graph, each taking the best-ranked
 * live tracks that reach new cameras.  priority: three codes, 0 length, 1 scale, 2 cost, -1 unused (the missing keys follow in
 * that order, numpy's rule for `order=`); exact ties in all three keys put the higher track index first.  Outputs: tree_of (host,
 * n_pts: the tree that took the track, or -1), n_selected, n_trees (trees that took at least one track; the loop ends after K
 * trees, when no track is left, or at the first empty tree), weights (host, K x n_cam, may be NULL: the camera weights every tree
 * started from, zero rows for trees that did not run), rank (host, n_pts, may be NULL: position of every track in the ranking),
 * kernel_ms (may be NULL: ranking + trees on the stream from HIP events, the per-layer status reads included). */
int satba_track_keys(int64_t n_pts, const int64_t *pt_ofs, const double *scale, const double *err, int32_t *length,
                     double *key_scale, double *key_cost, int32_t device);
int satba_track_connectivity(int32_t n_cam, int64_t n_pts, const int64_t *pt_ofs, const int32_t *cam_ind, const uint8_t *alive,
                             int32_t min_matches, int32_t *A, int32_t device);
int satba_select_tracks(int32_t n_cam, int64_t n_pts, const int64_t *pt_ofs, const int32_t *cam_ind, const double *scale,
                        const double *err, int32_t K, const int32_t *priority, int32_t *tree_of, int64_t *n_selected,
                        int32_t *n_trees, double *weights, int64_t *rank, int32_t device, float *kernel_ms);

/* ---- pairwise SIFT matching, the step in front of the track construction (ft_match.py:76-133 with the brute-force matcher of
 * 3rdparty/sift/simd/sift4ctypes.cpp:125-195).  Stand-alone: no problem handle; one call covers all pairs.  The entries are
 * detected by their presence; the version number stays.
 * features: host, n_cam pointers to n_kp[m] x 132 float32 (col, row, scale, orientation, 128 descriptor values); a row whose col is
 * NaN is padding: it stays a row and never matches.  utm: host, n_cam pointers to n_kp[m] x 2 float64 (east, north).  An image no
 * pair names is not read and may be NULL.  Images are uploaded and packed once and reused by every pair that names them.
 * Per pair (im_i, im_j) of pairs and per side, the keypoints whose utm lies strictly inside the pair's box (min_east, max_east,
 * min_north, max_north; infinite bounds are fine, NaN is an error) are selected, ascending; a NaN coordinate is outside.  For a
 * selected keypoint i of im_i over the selected j of im_j, ascending: d = sum (a - b)^2, +inf where the gate
 * fabs(xx_i - xx_j) < epi_thr fails, xx = (s[1] col + s[0] row) + s[2] in float32 in that order without fused multiply-add, s the
 * rectifying similarity of the side (linalg.c:108-138, in double from F5 = F[0,2], F[1,2], F[2,0], F[2,1], F[2,2] of the pair,
 * rounded to float32); F5 = NULL: no gate.  distA = the smallest d, among equals the lowest j; distB = the second smallest counted
 * with multiplicity.  (i, j) is a match when float32(distA) / float32(distB) (relative != 0) or float32(distA) (relative == 0) is
 * below float32(thr) * float32(thr): no match without a finite candidate or for 0 / 0, and a single finite candidate always
 * passes the relative test.  Matches come out pair by pair in the caller's order, i ascending inside a pair; kp_i / kp_j index the
 * images' rows.  Descriptors that are all integers in [0, 255] run on the int8 matrix cores and give the reference's bits
 * (d < 2^24 is exact in float32 in any order); anything else takes a float32 vector kernel that accumulates in index order.
 * counts (host, 4 x int64): matches, selected keypoints summed over pairs and sides, pairs with an empty side, the path that
 * ran (0 int8, 1 float32).  Argument errors (SATBA_E_ARG): an image index outside [0, n_cam), im_i == im_j, a NaN in a box,
 * thr <= 0.  kernel_ms (may be NULL): from the pack kernel to the last kernel, from HIP events (uploads outside, two reads of
 * counters inside).  Test switches, read at call time: SATBA_MATCH_FLOAT=1, SATBA_MATCH_CHUNK=<multiple of 16>. */
typedef struct satba_matches satba_matches;
int satba_match_pairs(int32_t n_cam, const int64_t *n_kp, const float *const *features, const double *const *utm, int32_t n_pairs,
                      const int32_t *pairs, const double *boxes, const double *F5, float thr, float epi_thr, int32_t relative,
                      satba_matches **out, int64_t *counts, int32_t device, float *kernel_ms);
/* any output may be NULL: pair_ofs (n_pairs + 1: the rows of pair p are pair_ofs[p] .. pair_ofs[p + 1] - 1), kp_i, kp_j (matches) */
int satba_matches_fetch(satba_matches *m, int64_t *pair_ofs, int32_t *kp_i, int32_t *kp_j);
void satba_matches_destroy(satba_matches *m);

/* ---- SIFT matching inside a UTM window, the matcher for pairs without a usable fundamental matrix (ft_match.py:151-160, 396-463,
 * locally_match_SIFT_utm_coords; its C routine is in neither tree, so the rule is fixed here).  Exactly as in satba_match_pairs: the
 * inputs, padding rows, the selection by the pair's box, the upload of each named image once, the satba_matches handle with
 * satba_matches_fetch / satba_matches_destroy, the output order, counts[0..3] (path: 0 integer, 1 float32), SATBA_MATCH_FLOAT=1,
 * kernel_ms and the argument errors.  Detected by its presence; the version number stays.
 * Per pair (im_i, im_j), for a selected keypoint i of im_i: its candidates are the selected keypoints j of im_j with
 * fabs(east_i - east_j) < rx and fabs(north_i - north_j) < ry, in float64, each difference rounded once, strict; a keypoint of im_j
 * outside the pair's box is no candidate however near it lies.  rx, ry may be +inf; NaN or a value <= 0 is SATBA_E_ARG.
 * d(i, j) = sum (a - b)^2 over the 128 descriptor values: exact in integers where all descriptors are integers in [0, 255],
 * otherwise in float32 accumulated in index order without fused multiply-add.  distA = the smallest d over the candidates, among
 * equals the lowest j (a reduction on the pair (d, j): the order of the visit does not matter).  (i, j) is a match when there is a
 * candidate and float32(distA) < float32(thr) * float32(thr); there is no relative test and no second nearest.  With rx = ry = +inf
 * this is satba_match_pairs with F5 = NULL and relative = 0.
 * counts (host, 5 x int64): [0..3] as above, [4] the (i, j) that passed the window test, summed over all pairs.
 * n_pairs == 0 returns 0 with an empty handle; fewer than 2^24 pairs per call. */
int satba_match_window(int32_t n_cam, const int64_t *n_kp, const float *const *features, const double *const *utm, int32_t n_pairs,
                       const int32_t *pairs, const double *boxes, double rx, double ry, float thr, satba_matches **out,
                       int64_t *counts /* 5 */, int32_t device, float *kernel_ms);

/* ---- SIFT detection and description of one image, the step in front of the matching (ref:s2p/sift.py keypoints_from_nparray,
 * i.e. sift() of ref:3rdparty/sift/simd/sift4ctypes.cpp:71-123: "Anatomy of the SIFT method" with delta_min 0.5, sigma_min 0.8,
 * sigma_in 0.5, 36 orientation bins, 4 x 4 x 8 descriptors, 5 interpolation steps, edge 10, lambda_ori 1.5, lambda_des 6, t 0.8).
 * image: height rows of width float32 pixels on the host, row_stride floats from one row to the next; nb_scales is the number of
 * scales per octave.  Rows come out as the reference lists them: by (octave, scale, row, column) of the discrete extremum, then
 * by orientation bin; a row is (col, row, sigma, theta, 128 integers 0 .. 255).  Two calls on one image return identical bytes.
 * counts (host, 6 x int64): rows, octaves, discrete extrema above 0.8 thr, survivors of the interpolation, survivors of the
 * border test (keypoints before their orientations), 1 when a pixel is not finite.  SATBA_E_ARG: a side shorter than 12 pixels,
 * nb_scales outside [1, 13], nb_octaves < 1, thresh_dog < 0 or NaN, row_stride < width.  SATBA_E_NONFINITE: a non-finite pixel.
 * keep_planes = 1 keeps the Gaussian planes for satba_sift_fetch_plane (plane `scale` of `octave`, 0 .. nb_scales + 2; plane may
 * be NULL to ask for the size only); with keep_planes = 0 that call returns SATBA_E_STATE.  kernel_ms (may be NULL): from the
 * seed kernel to the last kernel, from HIP events (the upload outside, three reads of counters inside). */
typedef struct satba_sift satba_sift;
int satba_sift_detect(const float *image, int32_t width, int32_t height, int64_t row_stride, float thresh_dog, int32_t nb_octaves,
                      int32_t nb_scales, int32_t keep_planes, satba_sift **out, int64_t *counts, int32_t device, float *kernel_ms);
int satba_sift_fetch(satba_sift *s, float *keypoints /* counts[0] x 132 */);
int satba_sift_fetch_plane(satba_sift *s, int32_t octave, int32_t scale, float *plane, int32_t *w, int32_t *h);
void satba_sift_destroy(satba_sift *s);

/* ---- feature tracks from pairwise matches, the step in front of the triangulation (ft_utils.py:65-182
 * feature_tracks_from_pairwise_matches with its baseline check :38-62 filter_C_using_pairs_to_triangulate, and the fixed-first
 * partition of ft_pipeline.py:175-179).  Stand-alone: no problem handle; no dense matrix is built.  Keypoint k of image m has
 * the global id kp_ofs[m] + k (kp_ofs: host, n_cam + 1, ascending from 0).  A track is a connected component (at least 2
 * keypoints) of the graph whose edges are the match rows; where several of its keypoints lie in one image the one written last by
 * the reference's fill wins (first-side keypoints of all rows in row order, then the second-side ones); a track stays if some
 * camera pair (i, j), i < j, of its observations is listed in pairs (a pair listed with i >= j or naming a camera >= n_cam
 * never matches).  Tracks are ordered by the smallest global id of their component; with n_adj > 0 the tracks without an
 * observation in a camera >= n_adj come first (n_pts_fix of them), both groups in that order.  The order of the match rows
 * changes nothing but the winners of contested cells, and two runs give identical bits.  A row with im_i > im_j is accepted
 * and is the same graph edge; im_i == im_j is an argument error, like an image >= n_cam, a keypoint index outside its image, or
 * 2^31 or more keypoints or matches.  The reference loses a union when a row names keypoint 0 of image 0 on its second side;
 * that is not reproduced (with im_i < im_j, what ft_match produces, it cannot occur).
 * kp: host, n_kp_total x 3 float32 (x, y, scale = columns 0..2 of the reference's keypoint arrays; NaN rows of padding are
 * fine, they are never matched).  matches: host, n_matches x 4 int32 (kp_i, kp_j, im_i, im_j).  pairs: host, n_pairs x 2.
 * counts (host, 5 x int64): n_tracks, n_obs, n_pts_fix, n_components (size >= 2, before the baseline check), n_conflicts
 * ((camera, track) cells with more than one claimant, before the baseline check).  kernel_ms (may be NULL): from the first kernel to
 * the last on the stream, from HIP events (the uploads are outside, two reads of counters inside). */
typedef struct satba_ftracks satba_ftracks;
int satba_ftracks_build(int32_t n_cam, const int64_t *kp_ofs, const float *kp, int64_t n_matches, const int32_t *matches,
                        int32_t n_pairs, const int32_t *pairs, int32_t n_adj, satba_ftracks **out, int64_t *counts,
                        int32_t device, float *kernel_ms);
/* the lists satba_init_pts3d and satba_select_tracks take; any output may be NULL: pt_ofs (n_tracks + 1), cam_ind (n_obs int32,
 * ascending strictly inside a track), kp_id (n_obs int32: index of the keypoint inside its image, the reference's C_v2), obs
 * (n_obs x 2 float64: the float32 coordinates widened exactly), scale (n_obs float64) */
int satba_ftracks_fetch(satba_ftracks *t, int64_t *pt_ofs, int32_t *cam_ind, int32_t *kp_id, double *obs, double *scale);
void satba_ftracks_destroy(satba_ftracks *t);
/* the baseline check alone, on lists (ft_utils.py:38-62): keep (host, n_pts bytes) = 1 where the track holds a listed pair */
int satba_tracks_have_pair(int32_t n_cam, int64_t n_pts, const int64_t *pt_ofs, const int32_t *cam_ind, int32_t n_pairs,
                           const int32_t *pairs, uint8_t *keep, int32_t device);

/* ---- RPC re-fit after the solve, the step behind the path.  Stand-alone: no problem handle.
 * satba_rpc_fit replaces ba_rpcfit.weighted_lsq (ba_rpcfit.py:88-153, with initialize_rpc / scaling_params :156-198), batched over
 * cameras: target (host, n_cam x n_samples x 2: col, row), locs (host, n_cam x n_samples x 3: lon, lat, alt) -> tables (host,
 * n_cam x SATBA_RPC_TABLE_LEN records of the fitted models), rmse (host, n_cam, may be NULL: the loop's last RMSE in pixels),
 * iters (host, n_cam, may be NULL: re-weighted passes that ran).  h, tol, max_iter: the reference's defaults are 1e-3, 1e-2, 20.
 * The loop stops when the RMSE of two consecutive RE-WEIGHTED passes differs by less than tol (at least two run when max_iter
 * allows): the unweighted solve's RMSE is no measure of the re-weighting's convergence.
 * satba_rpc_localization replaces rpcm.RPCModel.localization as ba_rpcfit.py:245,323 calls it: image points at given altitudes
 * -> lon, lat by inverting the projection of one camera (table: one record). */
int satba_rpc_fit(int32_t n_cam, int32_t n_samples, const double *target, const double *locs, double h, double tol,
                  int32_t max_iter, double *tables, double *rmse, int32_t *iters, int32_t device);
int satba_rpc_localization(const double *table, int64_t n, const double *col, const double *row, const double *alt, double *lon,
                           double *lat, int32_t device);

/* satba_rpc_refit replaces the loop of ba_pipeline.save_corrected_rpcs over ba_rpcfit.fit_Rt_corrected_rpc (ba_rpcfit.py:270-345,
 * ba_pipeline.py:406-423) for a batch of cameras, device resident: per camera the n_samples^3 mesh over its crop (+ margin) is built,
 * localised through the original RPC (tables_in: n_cam records), moved by global_transform (3 doubles or NULL), pushed through the
 * corrected projection x = P(R (X - T - C) + C) (rt: n_cam x 9 = Euler angles, T, C; the vector ba_params.reconstruct_vars keeps per
 * camera), fitted (satba_rpc_fit's loop) and checked: the margin (10 px at first) doubles until the convex hull of the mesh
 * re-projected through the FITTED model covers the crop (crops: n_cam x 4 = col0, row0, width, height) or exceeds 1000.
 * alt_ranges: n_cam x 2 (lowest, highest altitude of the mesh).  Outputs: tables_out (n_cam records), margins (n_cam: the last
 * margin), err (n_cam x n_samples^3 reprojection errors of the fitted model, check_errors; may be NULL), locs_out / target_out
 * (the last mesh: lon, lat, alt / col, row; may be NULL).  4 <= n_samples <= 16. */
int satba_rpc_refit(int32_t n_cam, const double *tables_in, const double *rt, const double *crops, const double *alt_ranges,
                    const double *global_transform, int32_t n_samples, double h, double tol, int32_t max_iter, double *tables_out, double *err,
                    double *margins, double *locs_out, double *target_out, int32_t device);

/* ---- cameras from RPCs, the step in front of the path (ba_pipeline.set_cameras / set_camera_centers).  Stand-alone: no problem
 * handle, float64, all cameras of a call in one launch.  These entries came after satba_version() 5 and left it unchanged: a caller
 * detects them by their presence in the library (dlsym), not by the version number.
 * satba_rpc_affine_approx replaces cam_utils.affine_rpc_approx (cam_utils.py:146-174): per camera the first-order expansion of
 * rpc.projection o ecef_to_latlon_custom at the ECEF point xyz (n_cam x 3; one point per camera), moved to the crop's origin
 * col0row0 (n_cam x 2): P_out (n_cam x 12, row-major 3 x 4) = [[J, q - J p - (col0, row0)], [0 0 0 1]].
 * satba_rpc_perspective_approx replaces cam_utils.perspective_rpc_approx / approx_rpc_as_proj_matrix (cam_utils.py:177-198, 234-277):
 * per camera the n_col x n_row x n_alt mesh (numpy.linspace over col_range / row_range / alt_range, n_cam x 2 each: first and last
 * sample; columns fastest, altitudes slowest) is localised through the RPC, taken to ECEF and resected.  crop0 (n_cam x 2: col0,
 * row0): the matrix is moved to the crop's origin and divided by P[2][3] (perspective_rpc_approx); NULL: the matrix as the
 * resection leaves it (approx_rpc_as_proj_matrix: unit Frobenius norm before the denormalisation, sign arbitrary).  mean_err (n_cam,
 * may be NULL): mean reprojection error over the mesh in pixels; centers (n_cam x 3, may be NULL): optical centres -M^-1 P[:, 3].
 * satba_camera_resection replaces cam_utils.camera_matrix (cam_utils.py:309-356, DLT with Hartley's normalisation) for n_cam sets of
 * n_pts correspondences X (n_cam x n_pts x 3) -> x (n_cam x n_pts x 2).
 * satba_rpc_mesh is the first phase alone: the ECEF nodes X_out (n_cam x n x 3), their image points x_out (n_cam x n x 2) and
 * altitudes alt_out (n_cam x n, may be NULL), n = n_col n_row n_alt.
 * SATBA_E_ARG: a null pointer, a negative count, fewer than 6 correspondences, fewer than 2 samples on an axis, more than 2^20
 * points per camera.  SATBA_E_NONFINITE: a non-finite input, or points no unique camera fits (a mesh axis of zero extent, coincident
 * or coplanar points: the second smallest eigenvalue of the DLT normal matrix is below 1e-12 of the largest), or an expansion point
 * on the polar axis; no output is written then -- a NaN matrix is never returned.  n_cam == 0 returns 0 without a device call. */
int satba_rpc_affine_approx(int32_t n_cam, const double *tables, const double *xyz, const double *col0row0, double *P_out, int32_t device);
int satba_rpc_perspective_approx(int32_t n_cam, const double *tables, const double *col_range, const double *row_range,
                                 const double *alt_range, int32_t n_col, int32_t n_row, int32_t n_alt, const double *crop0, double *P_out,
                                 double *mean_err, double *centers, int32_t device);
int satba_camera_resection(int32_t n_cam, int32_t n_pts, const double *X, const double *x, double *P_out, double *mean_err, int32_t device);
int satba_rpc_mesh(int32_t n_cam, const double *tables, const double *col_range, const double *row_range, const double *alt_range,
                   int32_t n_col, int32_t n_row, int32_t n_alt, double *X_out, double *x_out, double *alt_out, int32_t device);

/* ---- affine fundamental matrices of image pairs from their RPCs, the step between the choice of the pairs and their matching
 * under the epipolar gate (ft_pipeline.py:139-152, init_F_pair_to_match).  Stand-alone: no problem handle, float64, all pairs of a
 * call in one launch, the tables uploaded once.  Like the entries above it left the version number unchanged.
 * Per pair (i, j) of `pairs` (n_pairs x 2, indices into the n_cam tables) and its region of interest roi (n_pairs x 4: x, y, w, h in
 * image i) the matches of s2p.rpc_utils.matches_from_rpc (rpc_utils.py:199-246): an n x n x n mesh (numpy.linspace over columns
 * [x + w / 2n, x + (2n - 1) w / 2n], rows likewise, altitudes alt_offset -+ alt_scale of RPC i; columns fastest, altitudes
 * slowest) is localised through RPC i and projected through both RPCs -> rows x1, y1, x2, y2; then
 * s2p.estimation.affine_fundamental_matrix (estimation.py:114-154) of them: N, the right singular vector of the smallest singular
 * value of A = X - mean, X = (x2, y2, x1, y1), taken as the eigenvector of A^T A.  2 <= n <= 11 (the reference uses 5).
 * Outputs: F5 (n_pairs x 5) = F02, F12, F20, F21 = N of unit length and F22 = -N . mean, every other entry of the 3 x 3 matrix being
 * zero; sv (n_pairs x 4, may be NULL): the singular values of A, descending; matches (n_pairs x n^3 x 4, may be NULL).
 * Sign: the component of N with the largest magnitude is positive.  The sign the reference returns is an accident of LAPACK's SVD
 * and flips between crops of one pair; it means nothing, the epipolar gate of the match entry above is the same for F and -F.
 * Degenerate pairs (an image paired with itself, two identical RPCs: the second smallest eigenvalue of A^T A is not above 1e-12
 * of the largest, so no unique N exists): with degenerate == NULL the call returns SATBA_E_NONFINITE and writes no output; with
 * degenerate (n_pairs) given it succeeds, degenerate[p] = 1 marks those pairs and their F5 is NaN.
 * SATBA_E_ARG: a null pointer, a negative count, n outside 2..11, a pair index outside 0..n_cam-1, w <= 0 or h <= 0.
 * SATBA_E_NONFINITE: a non-finite table or region.  n_pairs == 0 returns 0 without a device call.
 * The kernel_ms entry returns the kernel time (HIP events, milliseconds) of the calling thread's last successful call. */
int satba_rpc_fundamental(int32_t n_cam, const double *tables, int32_t n_pairs, const int32_t *pairs, const double *roi, int32_t n,
                          double *F5, double *sv, double *matches, uint8_t *degenerate, int32_t device);
double satba_rpc_fundamental_kernel_ms(void);

/* ---- fundamental-matrix RANSAC of the pairwise matches (the filter of ref:bundle_adjust/s2p/sift.py:181-184 and of
 * ref:feature_tracks/ft_opencv.py:188-216).  Stand-alone: no problem handle, float64, all pairs of a call in
 * three launches.  The reference's RANSACs are random and in neither tree, so the rule is fixed here; it is deterministic, and a
 * pair's result depends on its rows, its index p in the call, n_trials, max_err and seed only.
 * Input per pair p: its M_p = pair_ofs[p + 1] - pair_ofs[p] matches as rows (x1, y1, x2, y2), in the caller's order.
 * 1. Small pairs.  M_p < 7: every match is kept, no model, best = (-1, M_p, 0).
 * 2. Normalisation.  Per pair and side Hartley's: translate to the centroid, scale so that the mean distance is sqrt(2); once, in
 *    float64, sums in the caller's order.  If a side's mean distance is 0 every match is kept and there is no model.
 * 3. Sampling, counter based.  Draw k of trial t of pair p is z = splitmix64(seed + 0x9E3779B97F4A7C15 * (1 + ((p * n_trials + t)
 *    * 64 + k))) in 64-bit wrap-around arithmetic (splitmix64: the finaliser z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27,
 *    z *= 0x94D049BB133111EB, z ^= z >> 31); the index is ((z >> 32) * M_p) >> 32.  Draws k = 0, 1, ... are taken until seven
 *    distinct indices are found, a repeat is skipped; after 64 draws without seven distinct indices the trial gives no model.  A
 *    sample in which two matches have a bit-identical (x1, y1) or a bit-identical (x2, y2) gives no model.
 * 4. Seven-point models.  The 7 x 9 matrix has the rows [x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1] of the normalised points;
 *    F1, F2 span its null space (Gauss-Jordan elimination with full pivoting, each vector of unit length); the real roots x of
 *    det(x F1 + (1 - x) F2) = 0 (closed form; three roots when the discriminant of the depressed cubic is negative, else one; a
 *    leading coefficient below 1e-12 of the largest drops the degree; then four Newton steps per root) give one to three models per
 *    trial, each denormalised (T2^T F T1) and scaled to unit Frobenius norm; a matrix that is not finite is no model.
 * 5. Error of a match under F: the larger of the two squared point-to-epipolar-line distances in pixel coordinates, as
 *    ref:ft_opencv.py:143-185 computes it, every operation rounded on its own.  Inlier iff err < max_err^2.
 * 6. Winner: the model with the most inliers; ties go to the lowest trial; ties between roots of one trial to the smaller sum of err
 *    over the model's inliers (then to the root written first).  The mask is the winner's inlier set; no refit.  If no trial gave a
 *    model every match is kept.
 * 7. The reference's values: n_trials = 1000 (sift.py:182), max_err = FT_ransac (0.3); seed is the caller's.
 * Outputs: inlier (n = pair_ofs[n_pairs]; 1 kept, 0 dropped); F (n_pairs x 9, may be NULL; zeros where there is no model); best
 * (n_pairs x 3, may be NULL) = winning trial (-1: no model), matches kept, models of the pair over all trials; kernel_ms (may be NULL):
 * HIP events around the three launches.
 * SATBA_E_ARG: a negative n_pairs, a pair_ofs that does not start at 0 or decreases, a non-finite coordinate, max_err <= 0 or not
 * finite, n_trials outside 1..65536, NULL pair_ofs (n_pairs > 0) or NULL xy / inlier (n > 0), n_pairs * n_trials above 2^26 or
 * n >= 2^31.  n_pairs == 0 and n == 0 return 0 without a device call. */
int satba_ransac_fundamental(int32_t n_pairs, const int64_t *pair_ofs, const double *xy, double max_err, int32_t n_trials, uint64_t seed,
                             uint8_t *inlier, double *F, int32_t *best, int32_t device, float *kernel_ms);
/* test entry: the models (step 4) of given samples, no sampling.  xy: the m rows of one pair (normalised as in step 2); idx
 * (n_samples x 7) indexes them -> n_models (n_samples), F (n_samples x 3 x 9, zeros behind the models).  A sample with repeated
 * points (step 3) or a pair without a normalisation gives 0 models.  SATBA_E_ARG: NULL, an index outside 0..m-1, a non-finite
 * coordinate. */
int satba_ransac_models(int64_t m, const double *xy, int32_t n_samples, const int32_t *idx, int32_t *n_models, double *F, int32_t device);

/* ---- the geographic side of the pairwise matching.  Stand-alone: no problem handle, float64.
 * satba_utm_filter is ref:feature_tracks/ft_match.py:220-247 (`filter_matches_inconsistent_utm_coords`) for the matches of all
 * pairs of a call: pair p owns the rows pair_ofs[p] : pair_ofs[p + 1] of utm (host, n x 4: east_i, north_i, east_j, north_j of the
 * match's two keypoints).  Per pair, over its matches with alive != 0 (alive NULL: all of them; a geometric filter's mask can be
 * handed in as it is):
 *   d = sqrt(dx * dx + dy * dy), every operation rounded on its own (what np.linalg.norm(..., axis=1) does on two columns);
 *   v = sort(d); (elbow, success) = get_elbow_value(v, 20) (ref:bundle_adjust/ba_outliers.py:14-58: the value farthest from the
 *   chord, first maximum; success iff elbow >= the 80th percentile, numpy's "linear" method); thr = success ? elbow + margin :
 *   v[last]; keep = d <= thr.  Index-exact against numpy, also where only rounding decides.
 * A match with alive == 0 gets keep = 0 and takes no part in the curve; a pair without an alive match gets thr = NaN, n_kept = 0.
 * Outputs (host): keep (n bytes, the caller's order), thr (n_pairs, may be NULL), n_kept (n_pairs, may be NULL); kernel_ms (may be
 * NULL): HIP events from the first kernel to the last.  margin: the reference's is 5.0 m.
 * SATBA_E_ARG: a negative n_pairs, a pair_ofs that does not start at 0 or decreases, n >= 2^31, a non-finite coordinate of an
 * alive match, a negative or non-finite margin, NULL pair_ofs (n_pairs > 0) or NULL utm / keep (n > 0).  n_pairs == 0 and n == 0
 * return 0 without a device call. */
int satba_utm_filter(int32_t n_pairs, const int64_t *pair_ofs, const double *utm /* n x 4: east_i, north_i, east_j, north_j */,
                     const uint8_t *alive /* n, or NULL: all */, double margin /* the reference's 5.0 m */,
                     uint8_t *keep /* n */, double *thr /* n_pairs, may be NULL */, int64_t *n_kept /* n_pairs, may be NULL */,
                     int32_t device, float *kernel_ms);
/* satba_keypoints_utm is ref:feature_tracks/ft_match.py:190-217 (`keypoints_to_utm_coords`) for all images of a call, in two
 * launches with a lane per row.  Per image c: the n_kp rows of features[c] (host, n_rows[c] x 132 float32) whose column is not NaN
 * are taken to lead the array, as the reference takes them; their (col + col0, row + row0) are localised at alt[c] through the
 * image's RPC record (the function satba_rpc_localization runs) and (lon, lat) are projected into the image's UTM zone by the
 * Krueger series to n^4 (k0 = 0.9996, false easting 500 000 m, southern northings negative; csrc/satba_utm_geom.h).  zone[c]:
 * 1..60, or 0 for the zone of the image's first keypoint (floor((lon + 180) / 6) mod 60 + 1), the reference's choice.  The rows
 * behind the first n_kp pass their two columns through, widened, to both outputs: NaN padding stays NaN.
 * Outputs (host, per image n_rows[c] x 2): utm_out = (easting, northing); lonlat_out (may be NULL) = (lon, lat) in degrees.
 * SATBA_E_ARG: a negative count, NULL arrays, a non-finite RPC record, offset or altitude, a zone outside 0..60, 2^31 rows or more. */
int satba_keypoints_utm(int32_t n_cam, const double *tables /* n_cam RPC records */, const int64_t *n_rows,
                        const float *const *features /* per image n_rows[c] x 132 */, const double *col0row0 /* n_cam x 2 */,
                        const double *alt /* n_cam */, const int32_t *zone /* n_cam; 0: zone of the image's first keypoint */,
                        double *const *utm_out /* per image n_rows[c] x 2 */, double *const *lonlat_out /* same shape, or NULL */,
                        int32_t device, float *kernel_ms);

/* ---- inspection entry points (parity tests; not used by the solver loop) */
/* index structures built by satba_problem_create, as int32 arrays (SATBA_LAY_PAIR_OFS: int64, SATBA_LAY_E_CAM8: uint8): n must equal
 * satba_layout_len */
enum { SATBA_LAY_PERM = 0, SATBA_LAY_RANK, SATBA_LAY_PT_CNT, SATBA_LAY_SLICE_BASE, SATBA_LAY_E_CAM, SATBA_LAY_OBS_POS, SATBA_LAY_CAM_OFS,
       SATBA_LAY_CM_PT, SATBA_LAY_CM_POS, SATBA_LAY_PAIR_OFS, SATBA_LAY_PAIR_PTS, SATBA_LAY_PAIR_PI, SATBA_LAY_PAIR_PJ, SATBA_LAY_PAIR_IJ, SATBA_LAY_CM_IO, SATBA_LAY_IPT_OFS,
       /* the merged records of the weighted / robust runs (affine, perspective; built by the first such linearisation, length -1 before):
        * piece offsets of the records' fixed parts (n_pts + 1: the last one is the all-zero record), of every point's first row scale,
        * the pair lists as (record, distances of the two scales in front of it), the camera-major lists as (record, scale piece), the
        * first camera-major entry of every diagonal item (+ 1 sentinel) */
       SATBA_LAY_W_FIX, SATBA_LAY_SC_OFS, SATBA_LAY_PAIR_REC, SATBA_LAY_PAIR_KK, SATBA_LAY_CM_REC, SATBA_LAY_CM_SC, SATBA_LAY_DG_OFS,
       /* the cameras of the ELL slots in one byte each (padding 0xFF), which the point kernels stream when there are at most 255 cameras
        * and SATBA_CAM_NARROW is not 0; length -1 where it is not built */
       SATBA_LAY_E_CAM8 };
int64_t satba_layout_len(const satba_problem *p, int32_t which);
int satba_get_layout(satba_problem *p, int32_t which, int64_t n, void *host_out);
/* n >= 16 doubles: [0..4] milliseconds since the start of satba_problem_create when the uploads were queued, the layout sizes were
 * known, the ELL + camera-major lists were queued, the pair lists were finished, the handle was complete; [5] padded ELL length,
 * [6] pair-list entries, [7] pair-list chunks, [8] unit weights, [9] camera constants in LDS, [10] RPC tables in LDS,
 * [11] camera sums by (fixed-point) LDS atomics, [12] camera-major sums requested, [13] chunks of the camera-major passes,
 * [14] workgroups of k_linearize, [15] fall-backs from the fixed-point sums so far, [16] satba_solve_lm runs on the
 * device-resident loop (n >= 17), [17] the last Schur + solve front had the factorisation running beside the pair
 * kernel (1), not (0), or that mode is switched off on this handle after a wait timed out (-1; it is tried again
 * after 128, 256, ... sequential fronts) (n >= 18), [18] such time-outs so far (n >= 19), [19] diagonal items per (camera,
 * chunk) of the weighted / robust pair kernel, 0 before the merged records exist (n >= 20), [20] log2 of the lanes per point
 * that the next launch of the point kernels uses with the loss configured now (n >= 21), [21] log2 of the replicas of
 * k_linearize's camera-sum table in LDS (n >= 22), [22] the first camera whose diagonal block and right-hand-side entries the
 * last Schur front produced BEHIND its pair kernel (csrc/satba_diag_split.h; the number of cameras: none; -1: no front yet) (n >= 23),
 * [23] the point kernels read the camera of an ELL slot from the one-byte array SATBA_LAY_E_CAM8 (1) or from SATBA_LAY_E_CAM (0) (n >= 24) */
int satba_get_info(const satba_problem *p, double *out, int32_t n);
/* normal-equation blocks of the last linearize: U (M n_p n_p), g_c (M n_p) as written to the exchange
 * payload, V (N x 6: xx xy xz yy yz zz), g_p (N x 3), points in the caller's order. Any pointer may be NULL.
 * U is formed by a camera-major pass (the solver itself only needs diag U_c before the Schur phase).       */
int satba_get_blocks(satba_problem *p, double *U, double *gc, double *V, double *gp);
/* materialised, weighted, row-scaled Jacobian blocks at x: Jc (K x 2 x n_p), Jp (K x 2 x 3).            */
int satba_get_jacobian(satba_problem *p, double *Jc, double *Jp);
/* copy n doubles of the exchange buffer starting at `offset`.                                            */
int satba_get_exchange(satba_problem *p, int64_t offset, int64_t n, double *host_out);
int satba_set_exchange(satba_problem *p, int64_t offset, int64_t n, const double *host_in);
/* state vectors, n_cam*n_params + 3*n_pts doubles: 0 g, 1 scale_inv, 2 gn_h, 3 q1, 4 w, 5 x_new, 6 g_h  */
int satba_get_vector(satba_problem *p, int32_t which, double *host_out);

/* ---- measurement: average duration in milliseconds of `reps` back-to-back launches of one phase's
 * dominant kernel, bracketed by HIP events on the handle's stream.
 * phase: 0 residual kernel, 1 linearize kernel (residual + Jacobian -> normal blocks), 2 Schur kernels,
 *        3 dense Cholesky solve, 4 back-substitution, 5 the Jacobian-vector product of the prepare phase */
int satba_time_kernel(satba_problem *p, int32_t phase, int32_t reps, float *ms_avg);

/* ---- measurement inside a running solve: with on != 0 every satba_linearize brackets its k_linearize launch with two HIP
 * events on the handle's stream (up to 4096 launches are kept); satba_profile_read waits for the stream, returns the number of
 * bracketed launches and the sum of their durations in milliseconds since the last read, and clears the record.  bench.py's
 * roofline figure is this average over the timed LM iterations. */
int satba_profile_linearize(satba_problem *p, int32_t on);
int satba_profile_read(satba_problem *p, int64_t *n_launches, double *ms_total);

#ifdef __cplusplus
}
#endif
#endif /* SATBA_H */

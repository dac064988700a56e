// satba_capi.hip -- C ABI of libsatba_hip.so (declared in include/satba.h) over the kernels of satba_kernels.h,
// satba_schur.h, satba_chol.h and the device-side layout builder of satba_layout.h.
//
// The handle owns every device array of one shard (all cameras, a contiguous range of points, their
// observations).  Phases are launched asynchronously on the handle's stream; the only synchronisation points
// are the functions that return data to the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/satba.h"
#include "satba_chol.h"
#include "satba_kernels.h"
#include "satba_layout.h"
#include "satba_lm.h"
#include "satba_lmdev.h"
#include "satba_outliers.h"
#include "satba_triangulate.h"
#include "satba_tracks.h"
#include "satba_ftracks.h"
#include "satba_match.h"
#include "satba_window.h"
#include "satba_sift.h"
#include "satba_rpcfit.h"
#include "satba_camapprox.h"
#include "satba_fundamental.h"
#include "satba_ransac.h"
#include "satba_utm.h"
#include "satba_schur.h"
#include "satba_schur_items.h"
#include "satba_diag_split.h"

#include <dlfcn.h>

// Range markers around the phases of an LM iteration (tracing): `rocprofv3 --marker-trace` shows the iteration
// structure -- linearize | prepare | schur | solve | trial | accept.  The marker library (ROCm's roctx) is looked up at run time, once:
// no link-time dependency, and a plain function-pointer test when it is absent.
namespace {
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        for (const char* name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
            if (void* h = dlopen(name, RTLD_LAZY | RTLD_GLOBAL)) {
                push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA"));
                pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
                if (push && pop) return;
                push = nullptr; pop = nullptr;
            }
        }
    }
};
inline const Roctx& roctx() { static const Roctx r; return r; }
struct Range {  // a phase's launches are queued between push and pop: the range covers the host side, the kernels follow on the stream
    bool on;
    explicit Range(const char* name) : on(roctx().push != nullptr) { if (on) roctx().push(name); }
    ~Range() { if (on) roctx().pop(); }
};
}  // namespace

using namespace satba;

static thread_local std::string g_err;

static int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(SATBA_E_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

constexpr int RED_SLOTS = 8, RED_MAX_GRID = 2048, RED_MAX_NV = 4;
// an item table of k_schur_pairs on the device: the items in dispatch order (satba_schur_items.h), the same flattened (k_schur_item_desc), workgroups of 4 items
struct SchurItems { int2* items = nullptr; SchurItem* desc = nullptr; int n_blocks = 0; };
static_assert(sizeof(SchurItemKey) == sizeof(int2) && offsetof(SchurItemKey, pair) == offsetof(int2, x) && offsetof(SchurItemKey, chunk) == offsetof(int2, y), "uploaded as int2");

struct satba_problem {
    int model = 0, M = 0, N = 0, NP = 0, c_p = 0, n_cam_fix = 0, n_pts_fix = 0, rank = 0, world = 1, f32 = 0, device = 0;
    long long K = 0, n_total = 0;
    int n_c = 0, n = 0, hdr = 0;
    int loss = 0;
    int camc_lds = 0, rpc_lds = 0;  // per-camera tables staged in LDS by the observation kernels
    int cam_sums_lds = 1;           // k_linearize accumulates diag U_c / g_c with LDS atomics (0: camera-major pass k_cam_sums)
    int lin_rep_shift = 0;          // log2 of the replicas of that LDS table (few cameras: same-address atomics serialise)
    int cam_narrow = 0;             // the point kernels stream the camera of a slot as one byte (Layout::e_cam8): at most 255 cameras
    int deterministic = 0;
    int split_env = -1;             // SATBA_SPLIT at satba_problem_create (experiments, tests): log2 of the lanes per point, -1 unset (slice_split)
    // fixed-point camera sums of k_linearize (satba_kernels.h): scales / bounds / inverse scales per slot, overflow flag, bounding
    // box of the points at the last satba_set_x, largest weight, most observations of one camera, and the cost of this shard at x
    // (linear loss: bound of a residual) with its copy for the trial point
    double *d_fx = nullptr, *d_bbox = nullptr, *d_fxcost = nullptr, *d_fxcost_new = nullptr, *d_fxcost0 = nullptr;
    int *d_fxflag = nullptr, *d_fxe = nullptr;
    bool fxcost_valid = false, fxcost_new_valid = false, fxcost0_valid = false;  // left by the pass that wrote the cost (or satba_accept), read by the next linearisation / snapshot
    double w_max = 1.0, n_max_cam = 1.0, fx_shrink = 1.0;
    int fx_fallbacks = 0;
    bool scales_by_tail = false;  // left by lm_launch_tail (the pattern ended with k_lm_accept_scales), read by the next lm_launch_tick, cleared by lm_drive
    bool gh_in_readers = false; // left by a linearisation that did NOT store g_h and g_h / scale_inv of the points (points_gh_stored): read by the launchers of their readers
    bool q1_points_unformed = false; // ... and the point entries of d_q1 = g_h / scale_inv are still not there: set by the prepare behind such a linearisation, cleared by the subspace phase (k_subspace_vec writes all of q1)
    bool prep_fused = false;   // left by a linearisation that did the point part of the prepare phase (PhaseCtx::fuse_prep), read by the prepare that follows
    struct LmDev* d_lm = nullptr;  // device-resident LM loop (satba_lmdev.h)
    struct LmSummary* h_lm = nullptr;  // pinned, mapped: the device posts the progress of the loop here
    struct LmSummary* h_lm_dev = nullptr;
    long long lm_ticks_queued = 0;
    hipStream_t own_stream = nullptr;   // created with the handle: the stream of every launch unless satba_set_stream names another
    double f_scale = 1.0, lead = 1.0;
    hipStream_t stream = nullptr;
    Layout L;
    int unit_weights = 0;
    double *d_cam_static = nullptr, *d_rpc = nullptr;
    // solver state (point parts in internal point order)
    double *d_x = nullptr, *d_xnew = nullptr, *d_camc = nullptr, *d_camc_new = nullptr;
    double *d_scale_inv = nullptr, *d_g = nullptr, *d_gh = nullptr, *d_gn = nullptr, *d_q1 = nullptr, *d_wv = nullptr;
    double *d_U = nullptr, *d_gc = nullptr, *d_V = nullptr, *d_PV = nullptr, *d_dc = nullptr, *d_dch = nullptr;
    double2 *d_f = nullptr, *d_ftmp = nullptr;  // residual pairs of the current linearisation / of satba_residuals, ELL order
    bool f_valid = false;                       // d_f holds the residuals of the current linearisation
    bool prof_lin = false;                      // satba_profile_linearize: event pairs around k_linearize
    std::vector<hipEvent_t> prof_ev;            // start, stop, start, stop, ...
    size_t prof_used = 0;
    double* d_Jpm = nullptr;                  // RPC: Jacobian blocks of the current linearisation, io order
    double *d_part = nullptr, *d_part3 = nullptr, *d_pair_part = nullptr;
    SchurItems items_chunked;  // (pair, chunk) work items of the Schur pair kernel
    SchurItems items_merged;   // one item per pair (all chunks), for the unit-weight kernels (schur_item_tables: not on every handle)
    // weighted / robust runs of the affine and perspective models (Layout::w_fix, built on first use by ensure_wlayout): the merged
    // records W and the item table with the diagonal items in front of every (camera row, chunk) group
    double2* d_W = nullptr;
    SchurItems items_w;
    int lin_grid = 0, cm_chunks = 1, cm_chunks_w = 1;  // chunks of the camera-major passes (unit weights and k_cam_sums | weighted / robust k_schur_diag)
    double* d_red = nullptr;  // RED_SLOTS x (RED_MAX_NV x RED_MAX_GRID doubles) partials of the deterministic grid sums
    unsigned* d_red_cnt = nullptr;
    double* d_stage = nullptr;  // staging for host transfers in the caller's order
    size_t stage_len = 0;
    int* d_fail = nullptr;
    double* d_dinv = nullptr;  // inverted 32 x 32 diagonal blocks of the factor (backward substitution)
    CholWork chol;             // scratch of the tile factorisation (satba_chol3.h)
    bool s_scaled = false;     // left by k_schur_finish's launcher when it handed the system over in scaled variables (FrontCtx::scale_in_finish), read by the solve
    // the factorisation beside the pair kernel (front_schur_solve): its stream, fork / join events, the producers' counters
    hipStream_t chol_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int* d_arrive = nullptr;   // (M + 2) x SCHUR_ARRIVE_STRIDE ints, zero between launches
    int* d_pair_cnt = nullptr; // weighted / robust runs: chunk items finished per camera pair (SchurArgs::pair_cnt), zero between launches
    int* d_dg_cnt = nullptr;   // ... and diagonal items finished per camera (SchurArgs::dg_cnt)
    long long* d_ts = nullptr; // (tools, -DC3_STAMPS: time stamps of the last factorisation beside the pair kernel, printed when the handle goes)
    int msg_epoch = 0;         // != 0 between satba_solve_messages_begin and _end: the epoch its factorisation waits for
    double* msg_packed = nullptr;  // the caller's packed payload of that exchange (device-resident loop: parts 10 - 12)
    bool beside_last = false;  // the last front ran that way
    int diag_split_last = -1;  // ... with the diagonal pass of the cameras from this one on behind the pair kernel (SchurRoute::c_split; M: none)
    bool beside_off = false;   // ... and timed out waiting for the pair kernel (kernels serialised by a tool, one hardware queue for both streams)
    int beside_clean = 0;      // sequential fronts QUEUED since the time-out (the device-resident loop also queues fronts that pass gated off:
                               // an upper bound of the ones that ran); the concurrent front is tried again after beside_retry_after of
    int beside_retry_after = 64;  // them, and the interval doubles with every further time-out (a profiler costs a handful of stalls, not one per front)
    int beside_timeouts = 0;
    double* d_scal = nullptr;  // 8 private scalars (costs of satba_residuals, timing sinks)
    double* d_keep = nullptr;  // SATBA_KEEP_LEN scalars of the running iteration that outlive the per-phase headers
    double* d_lam_used = nullptr;  // the damping of the last k_vinv, however it was chosen: k_backsub inverts V + lam Dp^2 with it again
    bool prepared = false;     // left by the prepare phase, read (and cleared) by satba_schur_auto
    double *d_xb_own = nullptr, *d_xb = nullptr;
    long long xb_len = 0;
    double* h_pin = nullptr;  // pinned staging for header reads
    bool dir_global = false;       // affine cameras whose direction tables (k_jvp, k_backsub) do not fit the LDS: d_dir_tab, built per launch
    double* d_dir_tab = nullptr;   // 2 x M x JVP_ROW
    void* h_stage = nullptr;  // pinned staging of the transfers between the caller's arrays and the device (copy_to_host)
    size_t h_stage_len = 0;
    // large transfers (round 6): COPY_LANES slices, each with a stream, a thread and two pinned chunks of its own (copy_big)
    struct CopyLane { char* pin = nullptr; hipEvent_t ev[2] = {nullptr, nullptr}; };
    CopyLane lanes[8];
    hipStream_t copy_stream = nullptr;
    bool lanes_ready = false;
    double* d_err_keep = nullptr;      // K per-observation errors kept for satba_reprojection_errors_fetch (caller's order)
    hipEvent_t ev_err = nullptr;       // ... complete on the device
    double* d_x0 = nullptr;   // satba_snapshot_x
    bool linearized = false, have_step = false;  // left by the linearisation / the solve, cleared by whatever moves x; read by the phases that need them
    double create_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<void*> allocs;

    double* payload() const { return d_xb + hdr; }
    RedBuf red(int slot) const { return RedBuf{d_red + (size_t)slot * RED_MAX_NV * RED_MAX_GRID, d_red_cnt + slot}; }
};
// What a caller wants of the phase it queues next.  The default value means "called from outside": nothing gated, nothing fused.
// The device-resident LM loop (satba_lmdev.h) passes `gate`, the word of its state that switches the kernels of the current part of
// the pattern on or off, and has the trust radius / first-iteration flag / trial coefficients read from the state (lm_ctx).
struct PhaseCtx {
    const int* gate = nullptr;
    const double *Delta_dev = nullptr, *coef_dev = nullptr, *lam_force_dev = nullptr, *sub_args_dev = nullptr;
    const int* first_dev = nullptr;
    int fuse_prep = -1;              // >= 0: k_linearize does the point part of the prepare phase (single-rank loops; value: `first`)
    bool skip_lin_scales = false;    // the previous tick's k_lm_accept_scales has done k_lin_scales' work (satba_problem::scales_by_tail)
    bool decide1a_in_trial = false;  // the trial's first launch carries k_lm_decide1a
    bool decide2_in_trial = false;   // the trial's residual kernel carries the loop's second decision
};
// ... and of a Schur phase: the front that queues it (front_schur_solve) and schur_impl fill it in
struct FrontCtx {
    int arrive_epoch = 0;          // != 0: the factorisation waits beside this stream (chol_front_launch) for this epoch
    bool scale_in_finish = false;  // k_schur_finish may hand the system over in scaled variables (the solve follows at once)
    double lam = 0.0;              // damping (k_schur_finish): value, or where k_vinv left it on the device
    const double* lam_dev = nullptr;
};
// RedBuf slots
enum { RB_RES = 0, RB_LIN = 1, RB_PREP = 2, RB_JVP = 3, RB_BS = 4, RB_SUB = 5, RB_TRIAL = 6, RB_MISC = 7 };

template <class T>
static int dev_alloc(satba_problem* p, T** out, size_t count) {
    void* ptr = nullptr;
    HIP_TRY(hipMalloc(&ptr, (count ? count : 1) * sizeof(T)));
    p->allocs.push_back(ptr);
    *out = static_cast<T*>(ptr);
    return 0;
}

#define TRY(expr)            \
    do {                     \
        int rc_ = (expr);    \
        if (rc_) return rc_; \
    } while (0)

#include "satba_devmem.h"

// dispatch on (camera model, parameters per camera, camera table in LDS, RPC table in LDS); valid pairs: affine {3,5,8},
// perspective {3,6,11}, rpc {3,6}
#define SATBA_CASE(key, M_, NP_, CL_, RL_, ...)                                                                    \
    case key: { constexpr int MODEL = M_, NP = NP_; constexpr bool CL = CL_, RL = RL_; (void)CL; (void)RL; __VA_ARGS__; } break;
#define SATBA_DISPATCH(p, ...)                                                                                    \
    do {                                                                                                          \
        const int key_ = (p)->model * 10 + (p)->NP + ((p)->camc_lds ? 100 : 0) + (((p)->model == RPC && (p)->rpc_lds) ? 1000 : 0); \
        switch (key_) {                                                                                           \
            SATBA_CASE(3, AFFINE, 3, false, false, __VA_ARGS__)                                                   \
            SATBA_CASE(5, AFFINE, 5, false, false, __VA_ARGS__)                                                   \
            SATBA_CASE(13, PERSPECTIVE, 3, false, false, __VA_ARGS__)                                             \
            SATBA_CASE(16, PERSPECTIVE, 6, false, false, __VA_ARGS__)                                             \
            SATBA_CASE(23, RPC, 3, false, false, __VA_ARGS__)                                                     \
            SATBA_CASE(26, RPC, 6, false, false, __VA_ARGS__)                                                     \
            SATBA_CASE(103, AFFINE, 3, true, false, __VA_ARGS__)                                                  \
            SATBA_CASE(105, AFFINE, 5, true, false, __VA_ARGS__)                                                  \
            SATBA_CASE(113, PERSPECTIVE, 3, true, false, __VA_ARGS__)                                             \
            SATBA_CASE(116, PERSPECTIVE, 6, true, false, __VA_ARGS__)                                             \
            SATBA_CASE(123, RPC, 3, true, false, __VA_ARGS__)                                                     \
            SATBA_CASE(126, RPC, 6, true, false, __VA_ARGS__)                                                     \
            SATBA_CASE(1123, RPC, 3, true, true, __VA_ARGS__)                                                     \
            SATBA_CASE(1126, RPC, 6, true, true, __VA_ARGS__)                                                     \
            SATBA_CASE(1023, RPC, 3, false, true, __VA_ARGS__)                                                    \
            SATBA_CASE(1026, RPC, 6, false, true, __VA_ARGS__)                                                    \
            SATBA_CASE(8, AFFINE, 8, false, false, __VA_ARGS__)                                                   \
            SATBA_CASE(21, PERSPECTIVE, 11, false, false, __VA_ARGS__)                                            \
            SATBA_CASE(108, AFFINE, 8, true, false, __VA_ARGS__)                                                  \
            SATBA_CASE(121, PERSPECTIVE, 11, true, false, __VA_ARGS__)                                            \
            default: return fail(SATBA_E_ARG, "unsupported (cam_model, n_params) = (%d, %d)", (p)->model, (p)->NP);           \
        }                                                                                                         \
    } while (0)

// weighted / robust runs with recomputed Jacobians (affine, perspective): row scales and point records share the merged records W
static bool unit_run(const satba_problem* p) { return p->loss == 0 && p->unit_weights; }  // every weight is 1 and the loss is linear
static bool wmode(const satba_problem* p) { return p->model != RPC && !unit_run(p); }
static bool merged_records(const satba_problem* p) { return wmode(p) && p->L.wl_ready; }  // ... and their layout is built: the kernels work on W
static bool pairs_run(const satba_problem* p) { return p->L.n_pairs > 0 && p->L.E > 0; }  // two cameras share a point: a Schur pair kernel runs

static ObsArgs obs_args(const satba_problem* p, bool at_new, const int* gate = nullptr) {
    ObsArgs a;
    const Layout& L = p->L;
    a.e_cam = L.e_cam; a.e_cam8 = L.e_cam8; a.e_obs = L.e_obs; a.e_w = L.e_w; a.slice_base = L.slice_base; a.pt_cnt = L.pt_cnt; a.perm = L.perm;
    a.ipt_ofs = L.ipt_ofs;
    a.x = at_new ? p->d_xnew : p->d_x;
    a.camc = at_new ? p->d_camc_new : p->d_camc;
    a.rpc = p->d_rpc;
    a.Jpm = at_new ? nullptr : p->d_Jpm;  // stored Jacobian blocks belong to the linearisation at x
    a.sc = nullptr;  // (RPC: the row scales ride in the stored D', ObsEval::store_jac)
    if (merged_records(p)) {  // the scales live in W: sc_ofs[q] + k instead of ipt_ofs[q] + k (null until the first linearisation has built the layout)
        a.sc = at_new ? nullptr : p->d_W;
        a.ipt_ofs = L.sc_ofs;
    }
    a.K = p->K; a.P = L.P; a.n_slices = L.n_slices; a.M = p->M; a.N = p->N; a.n_c = p->n_c;
    a.n_cam_fix = p->n_cam_fix; a.n_pts_fix = p->n_pts_fix; a.loss = p->loss; a.f32 = p->f32;
    a.f_scale = p->f_scale;
    a.unit = unit_run(p) ? 1 : 0;
    a.rep_shift = p->lin_rep_shift;
    a.fxe = p->d_fxe; a.fx_flag = p->d_fxflag; a.gate = gate;
    a.prep_scale = nullptr; a.prep_gh = nullptr; a.prep_ghs = nullptr; a.prep_first_dev = nullptr; a.prep_first = 0;
    a.dir_tab = p->d_dir_tab;
    a.sh = 0;  // lanes per point: set by the launchers of the kernels that support it
    return a;
}
// pt_rec: k_schur_diag on the merged records (SchurRoute::cm_rec) -- piece offsets instead of point indices
static CamMajor cam_major(const satba_problem* p, bool pt_rec = false) {
    return CamMajor{p->L.cam_ofs, pt_rec ? p->L.cm_rec : p->L.cm_pt, p->L.cm_pos, merged_records(p) ? p->L.cm_sc : p->L.cm_io};
}

static int grid_for(long long work, int block, int cap) {
    long long g = (work + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (int)g;
}

static size_t table_bytes(const satba_problem* p) {
    return sizeof(double) * ((p->camc_lds ? (size_t)p->M * CAMC : 0) + ((p->model == RPC && p->rpc_lds) ? (size_t)p->M * RPCS : 0));
}
static size_t lin_lds(const satba_problem* p) {
    return table_bytes(p) + (p->cam_sums_lds ? cam_sum_bytes(p->NP, (size_t)(p->M << p->lin_rep_shift)) : 0);
}
static size_t dir_table_bytes(const satba_problem* p) { return sizeof(double) * (size_t)p->M * JVP_ROW; }

template <class K>
static int raise_lds_limit(K kernel, size_t bytes) {
    if (bytes > 64 * 1024) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}

static int launch_cam_consts(satba_problem* p, bool at_new) {
    hipLaunchKernelGGL(k_cam_consts, dim3((p->M + 63) / 64), dim3(64), 0, p->stream, p->model, p->M, p->NP, p->c_p,
                       at_new ? p->d_xnew : p->d_x, p->d_cam_static, at_new ? p->d_camc_new : p->d_camc, (const int*)nullptr);
    HIP_TRY(hipGetLastError());
    return 0;
}

static int zero_header(satba_problem* p) {
    HIP_TRY(hipMemsetAsync(p->d_xb, 0, sizeof(double) * p->hdr, p->stream));
    return 0;
}

// grid of the thread-per-point kernels: `per_cu` workgroups per CU, all resident from the start (a later round of workgroups
// would run its slices alone at the end), every wave walking several slices (for_each_slice balances short and long tracks)
// log2 of the lanes per point of the slice kernels (SliceUnit): as many as it takes to give the chip ~8 waves per SIMD
static int slice_split(const satba_problem* p) {
    if (p->split_env >= 0) return std::min(p->split_env, 3);  // SATBA_SPLIT, read when the handle was created
    if (p->deterministic) return 0;  // the repeatability option keeps the summation order of the plain walk (goldens were made with it)
    int sh = 0;
    while (sh < 3 && ((long long)p->L.n_slices << sh) < 3000) ++sh;  // measured: 2 lanes per point at 100 k points, 8 at 5 k
    // weighted / robust runs: at least two lanes per point at every size (their linearize kernel keeps one record in flight instead of
    // two and sits at its register limit).  200 x 1M x 10M, soft_l1, LM it/s: 1 lane 455 / 455 / 455, 2 lanes 467 / 468 / 468, 4 lanes 459;
    // unit weights + linear loss: 841 / 822
    if (!unit_run(p)) sh = std::max(sh, 1);
    return sh;
}
// grid of k_linearize: one workgroup per CU (its LDS table is flushed once per workgroup; d_part holds 512 partial tables).  Depends on
// the lanes per point, i.e. on the configured loss: recomputed by satba_configure (round-5 advisor: a unit-weight handle later
// configured for a robust loss kept the grid of one lane per point -- half the workgroups on small problems)
static int lin_grid_for(const satba_problem* p) {
    return std::min(512, grid_for((long long)p->L.n_slices << slice_split(p), LinCfg<false>::WAVES, 256 * (1024 / LinCfg<false>::THREADS)));
}
static int slice_grid(const satba_problem* p, int waves_per_block, int per_cu, int sh = 0) {
    static const int env = getenv("SATBA_BPC") ? atoi(getenv("SATBA_BPC")) : 0;
    return grid_for((long long)p->L.n_slices << sh, waves_per_block, 256 * (env > 0 ? env : per_cu));
}

// direction of the slice walk per kernel (for_each_slice): bit 0 k_linearize, bit 1 k_backsub, bit 2 k_jvp, bit 3 k_residual.  Default 1: k_linearize
// walks from the middle of the slice list outwards, the trial evaluation in front of it from the ends to the middle -- it starts on the 200 MB of
// the ELL stream that the trial read last.  200 x 1M x 10M (profiles/r6_slice_direction.txt): k_linearize in the loop 0.124 -> 0.117 ms, 889 -> 902 it/s;
// the other kernels do not care (k_backsub, k_jvp: bound by their LDS reads; both directions the same: as before)
static int slice_rev(int bit) {
    static const int mask = getenv("SATBA_SLICE_REV") ? atoi(getenv("SATBA_SLICE_REV")) : 1;
    return (mask >> bit) & 1;
}
static int launch_residual(satba_problem* p, bool at_new, double2* f, double* cost, const int* gate = nullptr) {
    ObsArgs a = obs_args(p, at_new, gate);
    a.sh = slice_split(p);
    a.rev = slice_rev(3);
    const int grid = slice_grid(p, RES_THREADS / 64, 2, a.sh);
    const size_t lds = table_bytes(p);
    const TrialArgs t{};
    if (unit_run(p))
        SATBA_DISPATCH(p, hipLaunchKernelGGL((k_residual<MODEL, NP, CL, RL, true, false>), dim3(grid), dim3(RES_THREADS), lds, p->stream, a, f, p->red(RB_RES), cost, t));
    else
        SATBA_DISPATCH(p, hipLaunchKernelGGL((k_residual<MODEL, NP, CL, RL, false, false>), dim3(grid), dim3(RES_THREADS), lds, p->stream, a, f, p->red(RB_RES), cost, t));
    HIP_TRY(hipGetLastError());
    return 0;
}

// trial point + cost there + |step|^2, |x|^2 in one pass over the observations (k_residual<..., TRIAL>)
static int launch_trial(satba_problem* p, const PhaseCtx& c, double c0, double c1, const double* v0, const double* v1) {
    if (c.decide1a_in_trial) {  // device-resident loop: the decision kernel in front of the trial rides in this launch
        hipLaunchKernelGGL(k_lm_decide1a_trial_cams, dim3(1), dim3(256), 0, p->stream, p->d_lm, p->d_xb, p->model, p->M, p->NP, p->c_p, p->d_x, v0, v1,
                           p->d_scale_inv, p->d_cam_static, p->d_xnew, p->d_camc_new, p->d_xb, (int)p->hdr);
    } else
    hipLaunchKernelGGL(k_trial_cams, dim3((std::max(p->M, (int)p->hdr) + 63) / 64), dim3(64), 0, p->stream, p->model, p->M, p->NP, p->c_p, p->d_x, v0, v1,
                       p->d_scale_inv, c0, c1, p->d_cam_static, p->d_xnew, p->d_camc_new, p->d_xb, (int)p->hdr, c.coef_dev, c.gate);
    HIP_TRY(hipGetLastError());
    ObsArgs a = obs_args(p, true, c.gate);
    a.sh = slice_split(p);
    a.rev = slice_rev(3);
    const int grid = slice_grid(p, RES_THREADS / 64, 2, a.sh);
    const size_t lds = table_bytes(p);
    TrialArgs t{p->d_x, v0, v1, p->d_scale_inv, p->d_xnew, c0, c1, p->lead, p->d_xb + SATBA_HDR_STEP_SQ, p->d_xb + SATBA_HDR_X_SQ, p->d_fxcost_new, c.coef_dev};
    if (c.decide2_in_trial) { t.lm_st = p->d_lm; t.lm_sum = p->h_lm_dev; }  // (lm_launch_tail: one rank, device-resident loop)
    if (v0 == p->d_gh && p->gh_in_readers) t.g_pts = p->d_g;  // the point entries of g_h were not stored (points_gh_stored)
    p->fxcost_new_valid = true;
    double* cost = p->d_xb + SATBA_HDR_COST_NEW;
    if (unit_run(p))
        SATBA_DISPATCH(p, hipLaunchKernelGGL((k_residual<MODEL, NP, CL, RL, true, true>), dim3(grid), dim3(RES_THREADS), lds, p->stream, a, (double2*)nullptr, p->red(RB_RES), cost, t));
    else
        SATBA_DISPATCH(p, hipLaunchKernelGGL((k_residual<MODEL, NP, CL, RL, false, true>), dim3(grid), dim3(RES_THREADS), lds, p->stream, a, (double2*)nullptr, p->red(RB_RES), cost, t));
    HIP_TRY(hipGetLastError());
    return 0;
}

// which instantiation of k_linearize a run takes: 0 unit weights + linear loss (not RPC), 1 linear loss, 2 soft_l1 specialised at compile
// time, 3 generic robust
static int lin_variant(const satba_problem* p) {
    if (p->loss == 0) return (p->unit_weights && p->model != RPC) ? 0 : 1;
    return p->loss == SATBA_LOSS_SOFT_L1 ? 2 : 3;  // (RPC: the compile-time soft_l1 keeps the GENERIC formulas, robust(..., fast_soft = false): same bits, fewer registers)
}

template <int MODEL, int NP, bool CL, bool RL>
static int launch_lin(satba_problem* p, const ObsArgs& a) {
    double* gpv = p->d_g + p->n_c;
    double* cost = p->d_xb + SATBA_HDR_COST;
    double* gmax = p->d_xb + SATBA_HDR_FIXED + p->rank;
    const size_t lds = lin_lds(p);
    const RedBuf rb = p->red(RB_LIN);
    constexpr bool BIGL = MODEL == RPC || NP > 6;  // LinCfg of the linear-loss variants (k_linearize's own choice)
#define SATBA_LIN_LAUNCH(ROB, SOFT_, UNIT_, CS_, BIG_)                                                                                   \
    hipLaunchKernelGGL((k_linearize<MODEL, NP, ROB, CL, RL, SOFT_, UNIT_, CS_>), dim3(p->lin_grid), dim3(LinCfg<BIG_>::THREADS), lds, p->stream, \
                       a, (p->cam_sums_lds || MODEL != RPC) ? nullptr : p->d_f, p->d_V, gpv, p->d_part, rb, cost, gmax)
    const int v = lin_variant(p);
    if (p->cam_sums_lds) {
        if (v == 0) { if constexpr (MODEL != RPC) SATBA_LIN_LAUNCH(false, false, true, true, BIGL); }
        else if (v == 1) SATBA_LIN_LAUNCH(false, false, false, true, BIGL);
        else if (v == 2) SATBA_LIN_LAUNCH(true, true, false, true, BIGL);
        else SATBA_LIN_LAUNCH(true, false, false, true, true);
    } else {
        if (v == 0) { if constexpr (MODEL != RPC) SATBA_LIN_LAUNCH(false, false, true, false, BIGL); }
        else if (v == 1) SATBA_LIN_LAUNCH(false, false, false, false, BIGL);
        else if (v == 2) SATBA_LIN_LAUNCH(true, true, false, false, BIGL);
        else SATBA_LIN_LAUNCH(true, false, false, false, true);
    }
#undef SATBA_LIN_LAUNCH
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int MODEL, int NP, bool CL, bool RL>
static int raise_lin_limits(satba_problem* p) {
    const size_t lds = lin_lds(p);
    TRY(raise_lds_limit(k_linearize<MODEL, NP, false, CL, RL, false, false, true>, lds));
    TRY(raise_lds_limit(k_linearize<MODEL, NP, false, CL, RL, false, false, false>, lds));
    TRY(raise_lds_limit(k_linearize<MODEL, NP, true, CL, RL, false, false, true>, lds));
    TRY(raise_lds_limit(k_linearize<MODEL, NP, true, CL, RL, false, false, false>, lds));
    TRY(raise_lds_limit(k_linearize<MODEL, NP, true, CL, RL, true, false, true>, lds));
    TRY(raise_lds_limit(k_linearize<MODEL, NP, true, CL, RL, true, false, false>, lds));
    if constexpr (MODEL != RPC) {
        TRY(raise_lds_limit(k_linearize<MODEL, NP, false, CL, RL, false, true, true>, lds));
        TRY(raise_lds_limit(k_linearize<MODEL, NP, false, CL, RL, false, true, false>, lds));
    }
    TRY(raise_lds_limit(k_residual<MODEL, NP, CL, RL, true, false>, table_bytes(p)));
    TRY(raise_lds_limit(k_residual<MODEL, NP, CL, RL, false, false>, table_bytes(p)));
    TRY(raise_lds_limit(k_residual<MODEL, NP, CL, RL, true, true>, table_bytes(p)));
    TRY(raise_lds_limit(k_residual<MODEL, NP, CL, RL, false, true>, table_bytes(p)));
    const size_t dirb = p->dir_global ? 0 : dir_table_bytes(p);  // (global direction tables: those instantiations take no dynamic LDS)
    const size_t t = std::max(table_bytes(p), dirb);
    TRY(raise_lds_limit(k_jvp<MODEL, NP, 1, CL, RL, true>, t));
    TRY(raise_lds_limit(k_jvp<MODEL, NP, 1, CL, RL, false>, t));
    TRY(raise_lds_limit(k_jvp<MODEL, NP, 2, CL, RL, false>, std::max(t, 2 * dirb)));
    TRY(raise_lds_limit(k_backsub<MODEL, NP, CL, RL>, t));
    return 0;
}

// Whether a linearisation stores g_h and g_h / scale_inv of the points.  Not where it does the point part of the prepare phase itself on the
// default route (one rank, fixed-point camera sums, k_prepare_cams behind it): 48 MB of stores at 1 M points that every reader can form from
// g and scale_inv -- k_backsub, the trial's k_residual, k_jvp<PRE>, k_subspace_vec (point_gh, point_ghs in satba_kernels.h).  Several ranks,
// the phase entry points, more than 1 024 camera unknowns and the camera-major sums keep the arrays.
static bool points_gh_stored(const satba_problem* p, const PhaseCtx& c) {
    const char* e = getenv("SATBA_STORE_GH");  // A/B runs and the tests' comparison of the two forms (read per call): 1 stores everywhere
    const bool off = e && atoi(e) != 0;
    return off || !(c.fuse_prep >= 0 && p->world == 1 && p->n_c <= 1024 && p->cam_sums_lds);
}

static int launch_linearize_kernel(satba_problem* p, const PhaseCtx& c, bool store_gh) {
    ObsArgs a = obs_args(p, false, c.gate);
    a.sh = slice_split(p);
    a.rev = slice_rev(0);
    if (c.fuse_prep >= 0) {  // single-rank loops: the point part of the prepare phase rides in this kernel
        a.prep_scale = p->d_scale_inv;
        if (store_gh) { a.prep_gh = p->d_gh; a.prep_ghs = p->d_q1; }
        a.prep_first = c.fuse_prep; a.prep_first_dev = c.first_dev;
    }
    const bool prof = p->prof_lin && p->prof_used + 2 <= 2 * 4096;
    if (prof) {
        while (p->prof_ev.size() < p->prof_used + 2) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            p->prof_ev.push_back(e);
        }
        HIP_TRY(hipEventRecord(p->prof_ev[p->prof_used], p->stream));
    }
    SATBA_DISPATCH(p, TRY((launch_lin<MODEL, NP, CL, RL>(p, a))));
    if (prof) {
        HIP_TRY(hipEventRecord(p->prof_ev[p->prof_used + 1], p->stream));
        p->prof_used += 2;
    }
    return 0;
}

// camera-major camera sums of the stored linearisation -> U (full blocks), g_c
static int launch_cam_sums(satba_problem* p, const int* gate, double* U, double* gc) {
    ObsArgs a = obs_args(p, false, gate);
    CamMajor cm = cam_major(p);
    SATBA_DISPATCH(p, hipLaunchKernelGGL((k_cam_sums<MODEL, NP>), dim3(p->M, p->cm_chunks), dim3(LINC_THREADS), 0, p->stream, a, cm, p->d_f, p->d_part3));
    HIP_TRY(hipGetLastError());
    const int total = p->M * cam_acc_len(p->NP);
    hipLaunchKernelGGL(k_cam_sums_finish, dim3((total + 255) / 256), dim3(256), 0, p->stream, p->M, p->NP, p->cm_chunks, p->d_part3, U, gc, gate);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The host side of the Schur phase is satba_schur_api.inc; what the code in front of it needs of it.  launch_schur_kernel stays here: its
// dispatch is the first use of the Schur kernels, and a kernel's place in the code object follows the place of its first use.
namespace {
struct SchurRoute;
int schur_items_build(satba_problem* p, SchurTable kind, SchurItems* t, long long dg_weight);
int schur_item_tables(satba_problem* p);
template <int MODEL, int NP> int launch_schur(satba_problem* p, const FrontCtx& f, const SchurRoute& r, const ObsArgs& a, double* S, double* rhs);
}  // namespace
static int launch_schur_kernel(satba_problem* p, const int* gate, const FrontCtx& f, const SchurRoute& r) {
    ObsArgs a = obs_args(p, false, gate);
    double* S = p->payload();
    double* rhs = S + (size_t)p->n_c * p->n_c;
    SATBA_DISPATCH(p, TRY((launch_schur<MODEL, NP>(p, f, r, a, S, rhs))));
    return 0;
}

static int launch_backsub_kernel(satba_problem* p, const int* gate) {
    ObsArgs a = obs_args(p, false, gate);
    a.sh = slice_split(p);
    a.rev = slice_rev(1);
    const int grid = slice_grid(p, BS_THREADS / 64, 2, a.sh);
    const size_t lds = p->model == AFFINE ? dir_table_bytes(p) : table_bytes(p);
    if (p->dir_global) {
        SATBA_DISPATCH(p, if constexpr (MODEL == AFFINE) {
            hipLaunchKernelGGL((k_affine_dir_tab<NP>), dim3(1), dim3(1024), 0, p->stream, a, p->d_dc, (const double*)nullptr, (const double*)nullptr);
            hipLaunchKernelGGL((k_backsub<MODEL, NP, CL, RL, true>), dim3(grid), dim3(BS_THREADS), 0, p->stream, a, p->d_dc, p->d_dch, p->lead,
                               p->d_V, p->d_lam_used, p->d_g, p->d_scale_inv, p->d_gh, p->d_gn, p->red(RB_BS), p->d_xb, p->gh_in_readers ? nullptr : p->d_gh);
        });
    } else
    SATBA_DISPATCH(p, hipLaunchKernelGGL((k_backsub<MODEL, NP, CL, RL>), dim3(grid), dim3(BS_THREADS), lds, p->stream, a, p->d_dc, p->d_dch, p->lead,
                                         p->d_V, p->d_lam_used, p->d_g, p->d_scale_inv, p->d_gh, p->d_gn, p->red(RB_BS), p->d_xb, p->gh_in_readers ? nullptr : p->d_gh));
    HIP_TRY(hipGetLastError());
    return 0;
}

// pre: q1 is already in unscaled variables (nv == 1 only)
static int launch_jvp(satba_problem* p, const int* gate, int nv, const double* q1, const double* q2, double* out, bool pre = false) {
    ObsArgs a = obs_args(p, false, gate);
    a.sh = slice_split(p);
    a.rev = slice_rev(2);
    const int grid = slice_grid(p, JVP_THREADS / 64, 2, a.sh);
    const RedBuf rb = p->red(RB_JVP);
    const double* g_pre = (pre && p->gh_in_readers) ? p->d_g : nullptr;  // the point entries of q1 = g_h / scale_inv are formed in the kernel
    if (p->dir_global && (nv == 2 || pre)) {  // (affine) direction tables from global memory, built here
        SATBA_DISPATCH(p, if constexpr (MODEL == AFFINE) {
            hipLaunchKernelGGL((k_affine_dir_tab<NP>), dim3(1), dim3(1024), 0, p->stream, a, q1, nv == 2 ? q2 : nullptr, nv == 2 ? p->d_scale_inv : nullptr);
            if (nv == 1) hipLaunchKernelGGL((k_jvp<MODEL, NP, 1, CL, RL, true, true>), dim3(grid), dim3(JVP_THREADS), 0, p->stream, a, q1, q2, p->d_scale_inv, rb, out, g_pre);
            else hipLaunchKernelGGL((k_jvp<MODEL, NP, 2, CL, RL, false, true>), dim3(grid), dim3(JVP_THREADS), 0, p->stream, a, q1, q2, p->d_scale_inv, rb, out, g_pre);
        });
    } else if (nv == 1 && pre) {
        const size_t lds = p->model == AFFINE ? dir_table_bytes(p) : table_bytes(p);
        SATBA_DISPATCH(p, hipLaunchKernelGGL((k_jvp<MODEL, NP, 1, CL, RL, true>), dim3(grid), dim3(JVP_THREADS), lds, p->stream, a, q1, q2, p->d_scale_inv, rb, out, g_pre));
    } else if (nv == 1) {
        SATBA_DISPATCH(p, hipLaunchKernelGGL((k_jvp<MODEL, NP, 1, CL, RL, false>), dim3(grid), dim3(JVP_THREADS), table_bytes(p), p->stream, a, q1, q2,
                                             p->d_scale_inv, rb, out, g_pre));
    } else {
        const size_t lds = p->model == AFFINE ? std::max(table_bytes(p), 2 * dir_table_bytes(p)) : table_bytes(p);  // affine: two direction tables
        SATBA_DISPATCH(p, hipLaunchKernelGGL((k_jvp<MODEL, NP, 2, CL, RL, false>), dim3(grid), dim3(JVP_THREADS), lds, p->stream, a, q1, q2,
                                             p->d_scale_inv, rb, out, g_pre));
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// S z = rhs for the reduced system (S column-major lower, destroyed; b in place)
// unscaled (or null): set to whether the step in unscaled variables and the phase's header were written as well (k_unscale's work)
static int dense_solve(satba_problem* p, const int* gate, double* S, double* b, bool cleared = false, bool* unscaled = nullptr) {
    TrsvTail tail;
    tail.dc = p->d_dc; tail.scale_inv = p->d_scale_inv; tail.hdr = p->d_xb; tail.hdr_len = (int)p->hdr; tail.fail = p->d_fail; tail.lead = p->lead;
    tail.keep = p->d_keep; tail.keep_at = SATBA_HDR_KEEP; tail.keep_len = SATBA_KEEP_LEN;
    const bool done = cholesky_solve(S, p->n_c, b, p->d_fail, p->d_fail + 1, p->stream, p->chol, p->d_dinv, cleared, gate, nullptr,
                                     unscaled ? &tail : nullptr);  // clears d_fail and the flags unless the caller has
    if (unscaled) *unscaled = done;
    HIP_TRY(hipGetLastError());
    return 0;
}

// one-thread form of schur_lambda for problems without points (k_vinv is not launched then)
__global__ void k_lambda(const double* __restrict__ hdr, double Delta, double lam_floor, double* __restrict__ keep, const double* __restrict__ Delta_dev,
                         const double* __restrict__ lam_force, const int* gate) {
    SATBA_GATE(gate);
    if (Delta_dev) Delta = *Delta_dev;
    if (lam_force && *lam_force > 0.0) { keep[SATBA_KEEP_LAM] = *lam_force; return; }
    (void)schur_lambda(hdr, Delta, lam_floor, keep, true);
}

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The merged record layout of the weighted / robust runs (Layout::w_fix), built when the first such linearisation is queued: record
// offsets from the track lengths (one scan), the pair and camera-major lists re-expressed as piece offsets, the diagonal items.
static int ensure_wlayout(satba_problem* p) {
    Layout& L = p->L;
    if (L.wl_ready || !wmode(p)) return 0;
    const int N = p->N, M = p->M;
    hipStream_t st = p->stream;
    const size_t Nz = (size_t)N + 1;
    int *sz = nullptr, *wb = nullptr;
    char* cub = nullptr;
    size_t need = 0;
    // (round-5 advisor) the piece offsets are 32-bit: a record has at most track length + 13 pieces, so K + 13 N + 8 bounds the total
    // without waiting for the scan (whose int32 total could wrap to a positive value); pair_kk packs two track positions into 16 bits
    // each -- a track is at most M observations long (cameras strictly ascending inside a point)
    if ((long long)p->K + 13LL * N + 8 >= (1LL << 31)) return fail(SATBA_E_ARG, "the merged records of this shard exceed 2^31 pieces");
    if (M >= 65536) return fail(SATBA_E_ARG, "the merged record layout holds track positions in 16 bits: fewer than 65 536 cameras");
    DevAllocs tmp;  // sz, wb and cub: gone when this returns
    TRY(tmp.alloc(&sz, Nz + 1));
    TRY(tmp.alloc(&wb, Nz + 1));
    TRY(dev_alloc(p, &L.w_fix, Nz)); TRY(dev_alloc(p, &L.sc_ofs, Nz));
    HIP_TRY(hipMemsetAsync(sz, 0, sizeof(int) * (Nz + 1), st));
    hipLaunchKernelGGL(k_lay_wsize, dim3((unsigned)((Nz + 255) / 256)), dim3(256), 0, st, N, L.pt_cnt, sz);
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need, sz, wb, (int)(Nz + 1), st));
    TRY(tmp.alloc(&cub, need + 16));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(cub, need, sz, wb, (int)(Nz + 1), st));
    hipLaunchKernelGGL(k_lay_wfix, dim3((unsigned)((Nz + 255) / 256)), dim3(256), 0, st, N, L.pt_cnt, sz, wb, L.w_fix, L.sc_ofs);
    int h_len = 0, h_zero = 0;
    HIP_TRY(hipMemcpyAsync(&h_len, wb + Nz, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&h_zero, L.w_fix + N, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // (32-bit piece offsets: 2^31 pieces are 32 GB of records; a shard has fewer than 2^31 observations)
    if (h_len <= 0) return fail(SATBA_E_ARG, "the merged records of this shard exceed 2^31 pieces");
    L.W_len = h_len; L.zero_fix = h_zero;
    TRY(dev_alloc(p, &p->d_W, (size_t)L.W_len + 8));
    HIP_TRY(hipMemsetAsync(p->d_W, 0, sizeof(double2) * ((size_t)L.W_len + 8), st));  // pads, the zero record; scales are 0 until a linearisation
    const size_t Ez = (size_t)std::max<long long>(L.E, 1), Kz = (size_t)std::max<long long>(p->K, 1);
    TRY(dev_alloc(p, &L.pair_rec, Ez)); TRY(dev_alloc(p, &L.pair_kk, Ez)); TRY(dev_alloc(p, &L.cm_rec, Kz)); TRY(dev_alloc(p, &L.cm_sc, Kz));
    if (L.E > 0)
        hipLaunchKernelGGL(k_lay_pair_w, dim3(grid_for(L.E, 256, 8192)), dim3(256), 0, st, L.E, L.pair_pts, L.pair_pi, L.pair_pj, L.ipt_ofs, L.pt_cnt,
                           L.w_fix, L.pair_rec, L.pair_kk);
    if (p->K > 0)
        hipLaunchKernelGGL(k_lay_cm_w, dim3(grid_for(p->K, 256, 8192)), dim3(256), 0, st, p->K, L.cm_pt, L.cm_io, L.ipt_ofs, L.pt_cnt, L.w_fix,
                           L.cm_rec, L.cm_sc);
    // diagonal items: about 768 entries each (a dozen iterations of a wave; the pair items of the headline shape run five), at most 64
    // per camera (k_schur_finish adds a camera's partials with eight threads)
    const int C = L.C;
    const long long per_group = p->K / std::max(1, M) / std::max(1, C);
    int spc = (int)std::max<long long>(1, std::min<long long>((per_group + 767) / 768, std::max(1, 64 / C)));
    if (const char* e = getenv("SATBA_DIAG_SPC")) spc = std::max(1, std::min(atoi(e), std::max(1, 64 / C)));  // experiments
    L.dg_spc = spc; L.n_dg = C * spc;
    TRY(dev_alloc(p, &L.dg_ofs, (size_t)M * L.n_dg + 1));
    hipLaunchKernelGGL(k_lay_diag_items, dim3((unsigned)((M * C + 1 + 255) / 256)), dim3(256), 0, st, M, C, spc, std::max(N, 1), L.cam_ofs, L.cm_pt, L.dg_ofs);
    HIP_TRY(hipGetLastError());
    // what a camera's diagonal items weigh when the rows are dealt to the XCDs, in pair items: its entries over those of a pair
    const long long dg_weight = std::max<long long>(1, pairs_run(p) ? (long long)((double)p->K / M / ((double)L.E / L.n_pairs)) : 1);
    TRY(schur_items_build(p, SCHUR_ITEMS_WEIGHTED, &p->items_w, dg_weight));
    HIP_TRY(hipStreamSynchronize(st));
    L.wl_ready = true;
    return 0;
}

// ---------------------------------------------------------------------------------------------------- layout builder
// All index structures are derived on the device (satba_layout.h); the host sizes allocations from three scalars it reads
// back (padded ELL length, pair-list length, status flags).
static int build_layout(satba_problem* p, const satba_problem_desc* d) {
    Layout& L = p->L;
    const long long K = p->K;
    const int M = p->M, N = p->N;
    hipStream_t st = p->stream;
    L.M = M; L.N = N; L.K = K;
    L.n_slices = (N + 63) / 64;
    L.n_pairs = (long long)M * (M - 1) / 2;
    if (L.n_pairs >= (1ll << 31)) return fail(SATBA_E_ARG, "too many camera pairs");
    auto t0 = std::chrono::steady_clock::now();

    DevAllocs tmp;  // temporaries of the build: gone when this returns, before satba_problem_create allocates the solver's state
    int *o_cam = nullptr, *flags = nullptr, *o_ofs = nullptr, *cnt_o = nullptr, *iota = nullptr, *slots = nullptr;
    double2* o_obs = nullptr;
    double* o_w = nullptr;
    long long* hits = nullptr;
    const size_t Kz = (size_t)std::max<long long>(K, 1), Nz = (size_t)std::max(N, 1);
    TRY(tmp.alloc(&o_cam, Kz)); TRY(tmp.alloc(&o_obs, Kz)); TRY(tmp.alloc(&o_w, Kz)); TRY(tmp.alloc(&flags, 4));
    TRY(tmp.alloc(&o_ofs, Nz + 1)); TRY(tmp.alloc(&cnt_o, Nz)); TRY(tmp.alloc(&iota, Nz));
    TRY(tmp.alloc(&slots, L.n_slices + 1)); TRY(tmp.alloc(&hits, Nz + 1));
    TRY(dev_alloc(p, &L.ipt_ofs, Nz + 1)); TRY(dev_alloc(p, &L.cm_io, Kz));
    int* ipt_ofs = L.ipt_ofs;
    TRY(dev_alloc(p, &L.pts_ind, Kz)); TRY(dev_alloc(p, &L.obs_pos, Kz));
    TRY(dev_alloc(p, &L.perm, Nz)); TRY(dev_alloc(p, &L.rank, Nz)); TRY(dev_alloc(p, &L.pt_cnt, Nz));
    TRY(dev_alloc(p, &L.slice_base, L.n_slices + 1)); TRY(dev_alloc(p, &L.hit_ofs, Nz + 1));
    TRY(dev_alloc(p, &L.cam_ofs, M + 1)); TRY(dev_alloc(p, &L.cm_pt, Kz)); TRY(dev_alloc(p, &L.cm_pos, Kz));
    HIP_TRY(hipMemsetAsync(flags, 0, sizeof(int) * 4, st));
    if (K) {
        HIP_TRY(hipMemcpyAsync(o_cam, d->cam_ind, sizeof(int) * K, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(L.pts_ind, d->pts_ind, sizeof(int) * K, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(o_obs, d->pts2d, sizeof(double) * 2 * K, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(o_w, d->weights, sizeof(double) * K, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_lay_validate, dim3(grid_for(K, 256, 4096)), dim3(256), 0, st, K, M, N, o_cam, L.pts_ind, o_w, flags);
    }
    p->create_ms[0] = ms_since(t0);  // uploads queued (pageable host memory: the copies are synchronous in effect)
    // point CSR of the caller's order, track lengths, stable sort by length
    hipLaunchKernelGGL((k_lay_offsets<int>), dim3(grid_for(K + 1, 256, 4096)), dim3(256), 0, st, K, N, L.pts_ind, o_ofs);
    if (N) hipLaunchKernelGGL(k_lay_counts, dim3((N + 255) / 256), dim3(256), 0, st, N, o_ofs, cnt_o, iota);
    size_t cub_bytes = 0, need = 0;
    int bits_n = 1;
    while ((1ll << bits_n) <= M) ++bits_n;  // track lengths are <= M
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, need, cnt_o, L.pt_cnt, iota, L.perm, N, 0, bits_n, st));
    cub_bytes = std::max(cub_bytes, need);
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need, slots, L.slice_base, L.n_slices + 1, st));
    cub_bytes = std::max(cub_bytes, need);
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need, hits, L.hit_ofs, N + 1, st));
    cub_bytes = std::max(cub_bytes, need);
    int *io_cam = nullptr, *io_pos = nullptr, *io_pt = nullptr, *io_iota = nullptr, *cm_key = nullptr, *cm_io = L.cm_io;
    TRY(tmp.alloc(&io_cam, Kz)); TRY(tmp.alloc(&io_pos, Kz)); TRY(tmp.alloc(&io_pt, Kz)); TRY(tmp.alloc(&io_iota, Kz)); TRY(tmp.alloc(&cm_key, Kz));
    int bits_m = 1;
    while ((1ll << bits_m) < M) ++bits_m;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, need, io_cam, cm_key, io_iota, cm_io, (int)K, 0, bits_m, st));
    cub_bytes = std::max(cub_bytes, need);
    char* cub = nullptr;
    TRY(tmp.alloc(&cub, cub_bytes + 16));
    need = cub_bytes;
    if (N) HIP_TRY(hipcub::DeviceRadixSort::SortPairs(cub, need, cnt_o, L.pt_cnt, iota, L.perm, N, 0, bits_n, st));
    HIP_TRY(hipMemsetAsync(slots, 0, sizeof(int) * (L.n_slices + 1), st));
    HIP_TRY(hipMemsetAsync(hits, 0, sizeof(long long) * (Nz + 1), st));
    if (N) hipLaunchKernelGGL(k_lay_rank, dim3((N + 255) / 256), dim3(256), 0, st, N, L.perm, L.pt_cnt, L.rank, slots, hits);
    need = cub_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(cub, need, slots, L.slice_base, L.n_slices + 1, st));
    need = cub_bytes;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(cub, need, hits, L.hit_ofs, N + 1, st));
    // internal point-major CSR: exclusive sum of the sorted lengths (pt_cnt has N entries; one spare slot is read)
    {
        int* cnt_pad = nullptr;
        TRY(tmp.alloc(&cnt_pad, Nz + 1));
        HIP_TRY(hipMemsetAsync(cnt_pad, 0, sizeof(int) * (Nz + 1), st));
        if (N) HIP_TRY(hipMemcpyAsync(cnt_pad, L.pt_cnt, sizeof(int) * N, hipMemcpyDeviceToDevice, st));
        need = cub_bytes;
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(cub, need, cnt_pad, ipt_ofs, N + 1, st));
    }
    // sizes the host needs: padded ELL length, pair-list length, status
    int h_flags[4] = {0, 0, 0, 0}, h_P = 0;
    long long h_E = 0;
    HIP_TRY(hipMemcpyAsync(h_flags, flags, sizeof(int) * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&h_P, L.slice_base + L.n_slices, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&h_E, L.hit_ofs + N, sizeof(long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    switch (h_flags[0]) {
        case LAY_OK: break;
        case LAY_E_CAM: return fail(SATBA_E_ARG, "cam_ind out of range [0, %d)", M);
        case LAY_E_PT: return fail(SATBA_E_ARG, "pts_ind out of range [0, %d)", N);
        case LAY_E_ORDER: return fail(SATBA_E_ARG, "pts_ind must be non-decreasing (point-major order)");
        default: return fail(SATBA_E_ARG, "cameras must ascend strictly inside a point (ba_params.py:142-147 order)");
    }
    p->unit_weights = h_flags[1] ? 0 : 1;
    memcpy(&p->w_max, h_flags + 2, sizeof(double));  // largest |weight| (bound of the fixed-point camera sums)
    if (!(p->w_max > 0.0)) p->w_max = 1.0;
    L.P = h_P; L.E = h_E;
    if ((long long)L.P >= (1ll << 31) - 128 || L.E >= (1ll << 31)) return fail(SATBA_E_ARG, "observation or pair lists exceed 2^31 entries per shard");
    p->create_ms[1] = ms_since(t0);
    // sliced ELL
    const size_t Pz = (size_t)std::max(L.P, 1);
    TRY(dev_alloc(p, &L.e_cam, Pz + 64)); TRY(dev_alloc(p, &L.e_obs, Pz + 64)); TRY(dev_alloc(p, &L.e_w, Pz + 64));
    HIP_TRY(hipMemsetAsync(L.e_cam, 0xFF, sizeof(int) * (Pz + 64), st));
    if (p->cam_narrow) {  // the one-byte camera stream of the point kernels (Layout::e_cam8)
        TRY(dev_alloc(p, &L.e_cam8, Pz + 64));
        HIP_TRY(hipMemsetAsync(L.e_cam8, 0xFF, Pz + 64, st));
    }
    HIP_TRY(hipMemsetAsync(L.e_obs, 0, sizeof(double2) * (Pz + 64), st));
    HIP_TRY(hipMemsetAsync(L.e_w, 0, sizeof(double) * (Pz + 64), st));
    if (K) {
        hipLaunchKernelGGL(k_lay_fill_ell, dim3(grid_for(K, 256, 8192)), dim3(256), 0, st, K, o_cam, L.pts_ind, o_obs, o_w, o_ofs, L.rank,
                           L.slice_base, ipt_ofs, L.e_cam, L.e_cam8, L.e_obs, L.e_w, L.obs_pos, io_cam, io_pos, io_pt);
        // camera-major lists: stable sort of the internal point-major list by camera
        hipLaunchKernelGGL(k_lay_iota, dim3(grid_for(K, 256, 4096)), dim3(256), 0, st, K, io_iota);
        need = cub_bytes;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(cub, need, io_cam, cm_key, io_iota, cm_io, (int)K, 0, bits_m, st));
        hipLaunchKernelGGL(k_lay_gather2, dim3(grid_for(K, 256, 8192)), dim3(256), 0, st, K, cm_io, io_pos, io_pt, L.cm_pos, L.cm_pt);
    }
    hipLaunchKernelGGL((k_lay_offsets<int>), dim3(grid_for(K + 1, 256, 4096)), dim3(256), 0, st, K, M, cm_key, L.cam_ofs);
    HIP_TRY(hipGetLastError());
    p->create_ms[2] = ms_since(t0);
    // pair lists
    {
        // point-range chunks: 32 MB windows of the 128-byte point records and >= 256 entries per (pair, chunk) item on
        // average are the measured optimum between gather locality and the fixed cost per item at 200 x 1M x 10M; few
        // cameras: enough items to fill the chip (>= 8192 waves), at least 64 entries each
        int C = 1;
        if (L.n_pairs > 0 && L.E > 0) {
            C = (int)std::max<long long>(1, ((long long)N * 8 * PV_STRIDE + (32ll << 20) - 1) / (32ll << 20));
            // weighted / robust runs: an XCD works on one (camera, chunk) group at a time and gathers the records AND the row
            // scales of the camera's points in the chunk -- one merged record per point since round 5, ~256 bytes of lines (rounds 3-4:
            // record and scales apart, ~384); that set should sit in the XCD's 4 MB L2 with room to spare.  200 x 1M x 10M, LM it/s
            // of the soft_l1 loop with the merged records: 4 chunks 465, 5: 467, 6: 462, 7: 458, 8: 452, 10: 437, 12: 425, 16: 399
            // (round 4, separate arrays, pair kernel alone: 4 chunks 1.24 ms, 8: 1.02, 12: 1.04).  The unit-weight kernels use one
            // item per pair and do not look at the chunks
            C = (int)std::max<long long>(C, (K / std::max(M, 1) * 256 + 2800000 - 1) / 2800000);
            C = (int)std::max<long long>(1, std::min<long long>(C, L.E / L.n_pairs / 256));
            C = (int)std::max<long long>(C, std::min<long long>((8192 + L.n_pairs - 1) / L.n_pairs, std::max<long long>(1, L.E / L.n_pairs / 64)));
            if (const char* cs = getenv("SATBA_SCHUR_CHUNKS")) C = std::max(1, atoi(cs));
            C = std::min(C, 64);
            C = std::min(C, std::max(N, 1));
            while (C > 1 && L.n_pairs * (long long)(C + 1) > (1ll << 27)) --C;
        }
        L.C = C;
        const size_t n_ofs = (size_t)std::max<long long>(L.n_pairs, 1) * (C + 1) + 1;
        TRY(dev_alloc(p, &L.pair_ofs, n_ofs)); TRY(dev_alloc(p, &L.pair_ij, (size_t)std::max<long long>(L.n_pairs, 1)));
        const size_t Ez = (size_t)std::max<long long>(L.E, 1);
        TRY(dev_alloc(p, &L.pair_pts, Ez)); TRY(dev_alloc(p, &L.pair_pi, Ez)); TRY(dev_alloc(p, &L.pair_pj, Ez));
        if (M > 1) hipLaunchKernelGGL(k_lay_pair_ij, dim3(M - 1), dim3(64), 0, st, M, L.pair_ij);
        if (L.E > 0) {
            int *hk = nullptr, *hq = nullptr, *hpi = nullptr, *hpj = nullptr, *hi = nullptr, *hk_s = nullptr, *hi_s = nullptr;
            TRY(tmp.alloc(&hk, Ez)); TRY(tmp.alloc(&hq, Ez)); TRY(tmp.alloc(&hpi, Ez)); TRY(tmp.alloc(&hpj, Ez));
            TRY(tmp.alloc(&hi, Ez)); TRY(tmp.alloc(&hk_s, Ez)); TRY(tmp.alloc(&hi_s, Ez));
            hipLaunchKernelGGL(k_lay_hits, dim3((N + 255) / 256), dim3(256), 0, st, N, M, L.pt_cnt, L.slice_base, L.ipt_ofs, L.e_cam, L.hit_ofs, hk, hq, hpi, hpj);
            hipLaunchKernelGGL(k_lay_iota, dim3(grid_for(L.E, 256, 8192)), dim3(256), 0, st, L.E, hi);
            int bits_p = 1;
            while ((1ll << bits_p) < L.n_pairs) ++bits_p;
            size_t need2 = 0;
            HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, need2, hk, hk_s, hi, hi_s, (int)L.E, 0, bits_p, st));
            char* cub2 = nullptr;
            TRY(tmp.alloc(&cub2, need2 + 16));
            HIP_TRY(hipcub::DeviceRadixSort::SortPairs(cub2, need2, hk, hk_s, hi, hi_s, (int)L.E, 0, bits_p, st));  // stable: points stay ascending
            hipLaunchKernelGGL(k_lay_gather3, dim3(grid_for(L.E, 256, 8192)), dim3(256), 0, st, L.E, hi_s, hq, hpi, hpj, L.pair_pts, L.pair_pi, L.pair_pj);
            hipLaunchKernelGGL(k_lay_offsets_pair, dim3(grid_for(L.E + 1, 256, 8192)), dim3(256), 0, st, L.E, (long long)(n_ofs - 1), hk_s, L.pair_pts,
                               std::max(N, 1), C, L.pair_ofs);
        } else {
            HIP_TRY(hipMemsetAsync(L.pair_ofs, 0, sizeof(long long) * n_ofs, st));
        }
        HIP_TRY(hipGetLastError());
    }
    {   // most observations of one camera (range of the fixed-point camera sums)
        std::vector<int> h_ofs((size_t)M + 1);
        HIP_TRY(hipMemcpyAsync(h_ofs.data(), L.cam_ofs, sizeof(int) * (M + 1), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        int mx = 1;
        for (int c = 0; c < M; ++c) mx = std::max(mx, h_ofs[c + 1] - h_ofs[c]);
        p->n_max_cam = (double)mx;
    }
    p->create_ms[3] = ms_since(t0);
    return 0;
}

extern "C" {

const char* satba_last_error(void) { return g_err.c_str(); }
int satba_version(void) { return 5; }

int satba_problem_create(const satba_problem_desc* d, satba_problem** out) {
    Range range_("satba:problem_create");
    if (!d || !out) return fail(SATBA_E_ARG, "null argument");
    *out = nullptr;
    if (d->cam_model < 0 || d->cam_model > 2) return fail(SATBA_E_ARG, "cam_model must be 0, 1 or 2");
    const int c_p_expected = d->cam_model == SATBA_AFFINE ? 8 : (d->cam_model == SATBA_PERSPECTIVE ? 11 : 9);
    if (d->cam_param_len != c_p_expected) return fail(SATBA_E_ARG, "cam_param_len %d, expected %d", d->cam_param_len, c_p_expected);
    const int np_rt = d->cam_model == SATBA_AFFINE ? 5 : 6;
    const int np_rtk = d->cam_model == SATBA_AFFINE ? 8 : (d->cam_model == SATBA_PERSPECTIVE ? 11 : 0);  // + intrinsics (not rpc)
    if (d->n_params != 3 && d->n_params != np_rt && (np_rtk == 0 || d->n_params != np_rtk)) {
        if (np_rtk) return fail(SATBA_E_ARG, "n_params %d not in {3, %d, %d}", d->n_params, np_rt, np_rtk);
        return fail(SATBA_E_ARG, "n_params %d not in {3, %d}", d->n_params, np_rt);
    }
    if (d->n_cam <= 0 || d->n_pts < 0 || d->n_obs < 0) return fail(SATBA_E_ARG, "negative size");
    if (d->n_obs >= (1ll << 31) - 64) return fail(SATBA_E_ARG, "more than 2^31 observations per shard");
    if (!d->cam_params || (d->n_obs && (!d->cam_ind || !d->pts_ind || !d->pts2d || !d->weights)))
        return fail(SATBA_E_ARG, "null input array");
    if (d->cam_model == SATBA_RPC && !d->rpc_tables) return fail(SATBA_E_ARG, "rpc_tables required for cam_model rpc");
    if (d->n_cam_fix < 0 || d->n_cam_fix > d->n_cam || d->n_pts_fix < 0 || d->n_pts_fix > d->n_pts)
        return fail(SATBA_E_ARG, "n_cam_fix / n_pts_fix out of range");
    if (d->world < 1 || d->rank < 0 || d->rank >= d->world) return fail(SATBA_E_ARG, "bad rank / world");
    const long long K = d->n_obs;
    auto t_create = std::chrono::steady_clock::now();

    satba_problem* p = new (std::nothrow) satba_problem();
    if (!p) return fail(SATBA_E_ARG, "out of host memory");
    p->model = d->cam_model; p->M = d->n_cam; p->N = d->n_pts; p->NP = d->n_params; p->c_p = d->cam_param_len;
    p->n_cam_fix = d->n_cam_fix; p->n_pts_fix = d->n_pts_fix; p->rank = d->rank; p->world = d->world;
    p->f32 = d->rpc_store_f32; p->device = d->device; p->K = K; p->n_total = d->n_total;
    p->n_c = p->M * p->NP; p->n = p->n_c + 3 * p->N;
    p->hdr = SATBA_HDR_FIXED + p->world + (p->world & 1);
    p->lead = p->rank == 0 ? 1.0 : 0.0;
    p->deterministic = ((d->flags & SATBA_FLAG_DETERMINISTIC) || getenv("SATBA_DETERMINISTIC")) ? 1 : 0;
    if (const char* ss = getenv("SATBA_SPLIT")) p->split_env = atoi(ss);  // experiments, tests (negative: the rule, as unset)
    const char* cn = getenv("SATBA_CAM_NARROW");  // A/B runs, tests: 0 keeps the int stream
    p->cam_narrow = (p->M <= 255 && !(cn && atoi(cn) == 0)) ? 1 : 0;  // (0xFF, the padding, is then no camera)

    int rc = [&]() -> int {
        HIP_TRY(hipSetDevice(p->device));
        HIP_TRY(hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking));
        p->stream = p->own_stream;
        if (p->n_c > CH_NB * CH_MAX_STEPS) return fail(SATBA_E_ARG, "reduced camera system too large for the dense solver");
        cholesky_init();
        TRY(build_layout(p, d));
        // LDS budget of the observation kernels: camera-sum table first, then the camera constants, then the RPC tables
        const size_t budget = 150 * 1024;
        const size_t camc_b = sizeof(double) * (size_t)p->M * CAMC, rpc_b = sizeof(double) * (size_t)p->M * RPCS;
        // replicas of the camera-sum table: same-address and same-bank atomics of a wave spread over them.  Measured at 200 cameras
        // (k_linearize in the loop, fixed-point sums of round 3): 1 replica 0.112 ms, 2: 0.109, 4: 0.105 although only one workgroup
        // per CU fits then (the sums are integers: every replica count gives the same bits); at 50 cameras 16 replicas are as good as
        // or better than 4 (round 2, float atomics: C3 0.038 vs 0.040, P3 0.040 vs 0.047, C5 0.118 vs 0.119)
        while (p->lin_rep_shift < 4 && (p->M << (p->lin_rep_shift + 1)) <= 1024 &&
               cam_sum_bytes(p->NP, (size_t)(p->M << (p->lin_rep_shift + 1))) + camc_b <= 140 * 1024)
            ++p->lin_rep_shift;
        if (const char* rs = getenv("SATBA_LIN_REP")) p->lin_rep_shift = std::min(4, std::max(0, atoi(rs)));  // experiments
        const size_t acc_b = cam_sum_bytes(p->NP, (size_t)(p->M << p->lin_rep_shift));
        p->cam_sums_lds = (acc_b <= budget && !p->deterministic && !getenv("SATBA_CAM_SUMS") && p->n_max_cam <= (double)FX_MAX_OBS_PER_CAM) ? 1 : 0;
        size_t used = p->cam_sums_lds ? acc_b : 0;
        p->camc_lds = (camc_b <= 48 * 1024 && used + camc_b <= budget && !getenv("SATBA_CAMC_GLOBAL")) ? 1 : 0;
        used += p->camc_lds ? camc_b : 0;
        p->rpc_lds = (p->model == RPC && rpc_b <= 64 * 1024 && used + rpc_b <= budget && !getenv("SATBA_RPC_GLOBAL")) ? 1 : 0;
        // affine cameras: the direction tables of k_jvp (two for the explicit-products pattern) and k_backsub live in the LDS up to ~640
        // cameras, beyond that in global memory (k_affine_dir_tab in front of every such launch)
        p->dir_global = p->model == AFFINE && (2 * dir_table_bytes(p) > budget || getenv("SATBA_DIR_GLOBAL"));  // (the switch: tests)
        if (p->dir_global) TRY(dev_alloc(p, &p->d_dir_tab, (size_t)2 * p->M * JVP_ROW));
        SATBA_DISPATCH(p, TRY((raise_lin_limits<MODEL, NP, CL, RL>(p))));

        const size_t n = p->n, Pz = (size_t)std::max(p->L.P, 1) + 64;
        TRY(dev_alloc(p, &p->d_cam_static, (size_t)p->M * p->c_p));
        if (p->model == RPC) TRY(dev_alloc(p, &p->d_rpc, (size_t)p->M * SATBA_RPC_TABLE_LEN));
        TRY(dev_alloc(p, &p->d_x, n)); TRY(dev_alloc(p, &p->d_xnew, n)); TRY(dev_alloc(p, &p->d_scale_inv, n));
        TRY(dev_alloc(p, &p->d_g, n)); TRY(dev_alloc(p, &p->d_gh, n)); TRY(dev_alloc(p, &p->d_gn, n));
        TRY(dev_alloc(p, &p->d_q1, n)); TRY(dev_alloc(p, &p->d_wv, n));
        TRY(dev_alloc(p, &p->d_camc, (size_t)p->M * CAMC)); TRY(dev_alloc(p, &p->d_camc_new, (size_t)p->M * CAMC));
        TRY(dev_alloc(p, &p->d_U, (size_t)p->M * p->NP * p->NP)); TRY(dev_alloc(p, &p->d_gc, p->n_c));
        TRY(dev_alloc(p, &p->d_V, (size_t)6 * p->N));
        TRY(dev_alloc(p, &p->d_PV, (size_t)PV_STRIDE * (p->N + 1)));  // record N: all zeros, the target of lanes past the end of a pair list
        HIP_TRY(hipMemset(p->d_PV + (size_t)PV_STRIDE * p->N, 0, sizeof(double) * PV_STRIDE));
        TRY(dev_alloc(p, &p->d_dc, p->n_c)); TRY(dev_alloc(p, &p->d_dch, p->n_c));
        const size_t Kz = (size_t)std::max<long long>(K, 1) + 64;
        TRY(dev_alloc(p, &p->d_f, Pz)); TRY(dev_alloc(p, &p->d_ftmp, Pz));
        if (p->model == RPC) TRY(dev_alloc(p, &p->d_Jpm, Kz * jrow_stride(p->NP)));
        TRY(dev_alloc(p, &p->d_fail, 1 + CH_MAX_STEPS));  // [0] not-SPD flag, then the panel-step flags
        TRY(dev_alloc(p, &p->d_dinv, (size_t)((p->n_c + CH_NB - 1) / CH_NB) * CH_NB * CH_NB));
        {   // scratch of the tile factorisation: tile flags (zeroed once: they carry epochs), inverted 64 x 64 diagonal blocks, the tiles'
            // shares of the forward substitution, ticket counters
            const size_t T = (size_t)(p->n_c + 63) / 64;
            TRY(dev_alloc(p, &p->chol.flags, T * T + 1)); TRY(dev_alloc(p, &p->chol.Linv, T * 4096 + 1)); TRY(dev_alloc(p, &p->chol.Cc, T * T * 64 + 1));
            TRY(dev_alloc(p, &p->chol.ctr, 4));
            HIP_TRY(hipMemset(p->chol.flags, 0, sizeof(int) * (T * T + 1)));
            HIP_TRY(hipMemset(p->chol.ctr, 0, sizeof(int) * 4));
        }
        TRY(dev_alloc(p, &p->d_scal, 8));
        TRY(dev_alloc(p, &p->d_fx, fx_scales_len(p->NP))); TRY(dev_alloc(p, &p->d_fxe, fx_exps_len(p->NP)));  // (sized by NP: 8 and 11 need more than 6)
        TRY(dev_alloc(p, &p->d_bbox, 6)); TRY(dev_alloc(p, &p->d_fxflag, 1));
        TRY(dev_alloc(p, &p->d_fxcost, 1)); TRY(dev_alloc(p, &p->d_fxcost_new, 1)); TRY(dev_alloc(p, &p->d_fxcost0, 1));
        HIP_TRY(hipMemset(p->d_bbox, 0, sizeof(double) * 6));
        HIP_TRY(hipMemset(p->d_fxflag, 0, sizeof(int)));
        if (const char* fs = getenv("SATBA_FX_SHRINK")) p->fx_shrink = atof(fs);  // tests: shrink the bounds to force the fall-back
        TRY(dev_alloc(p, &p->d_lm, 1));
        HIP_TRY(hipMemset(p->d_lm, 0, sizeof(LmDev)));
        HIP_TRY(hipHostMalloc((void**)&p->h_lm, sizeof(LmSummary) + sizeof(LmDev), hipHostMallocMapped));
        memset(p->h_lm, 0, sizeof(LmSummary) + sizeof(LmDev));
        HIP_TRY(hipHostGetDevicePointer((void**)&p->h_lm_dev, p->h_lm, 0));
        TRY(dev_alloc(p, &p->d_keep, SATBA_KEEP_LEN));
        HIP_TRY(hipMemset(p->d_keep, 0, sizeof(double) * SATBA_KEEP_LEN));
        TRY(dev_alloc(p, &p->d_lam_used, 1));
        HIP_TRY(hipMemset(p->d_lam_used, 0, sizeof(double)));
        TRY(dev_alloc(p, &p->d_red, (size_t)RED_SLOTS * RED_MAX_NV * RED_MAX_GRID));
        TRY(dev_alloc(p, &p->d_red_cnt, RED_SLOTS));
        HIP_TRY(hipMemset(p->d_red_cnt, 0, sizeof(unsigned) * RED_SLOTS));
        // one workgroup per CU for the linearize kernel (its LDS table is flushed once per workgroup)
        p->lin_grid = lin_grid_for(p);
        TRY(dev_alloc(p, &p->d_part, (size_t)512 * p->M * cam_sum_len(p->NP)));
        {   // chunking of the camera-major passes (k_schur_diag, k_cam_sums): (camera, chunk) workgroups
            // Eight chunks, dealt to the eight XCDs (k_schur_diag: s.diag_xcd, a multiple of 8) -- more only where few cameras hold many
            // observations (>= 512 workgroups, >= 4 096 observations each), fewer where a workgroup would get less than 256 observations.
            // Round 5, LM it/s by chunk count (rounds 2-4 aimed at 2 048 workgroups of >= 512 observations: 40 chunks at 50 cameras, 16 at 200):
            //   50 x 100 k x 1 M    2: 3 123   4: 3 269   5: 3 295   8: 3 309   10: 3 300   12: 3 278   16: 3 265   40: 3 180
            //   perspective, same   4: 2 277   8: 2 333   12: 2 274   16: 2 281   40: 2 211
            //   200 x 1 M x 10 M    4: 831   6: 840   8: 840-847   10: 848   12: 841   16: 840-846   24: 833   32: 822   64: 776
            //   10 x 5 k x 30 k     1: 7 586   2: 7 758   3: 7 888   5: 7 958   8: 8 035
            // The weighted / robust pass (two lines per entry; only where the diagonal blocks are not items of the pair kernel) takes twice as many
            int chunks = 8;
            while (chunks < 64 && (long long)p->M * chunks < 512 && K / ((long long)p->M * (chunks + 8)) >= 4096) chunks += 8;
            while (chunks > 1 && K / ((long long)p->M * chunks) < 256) --chunks;
            int chunks_w = chunks;
            if (chunks >= 8) {
                chunks_w = std::min(64, 2 * chunks);
                while (chunks_w > chunks && K / ((long long)p->M * chunks_w) < 512) chunks_w -= 8;
            }
            if (const char* dc = getenv("SATBA_CM_CHUNKS")) chunks_w = chunks = std::max(1, std::min(256, atoi(dc)));  // experiments, tests
            p->cm_chunks = chunks; p->cm_chunks_w = chunks_w;
            // (+ NP: k_cam_sums' error words; 64: the diagonal items of the weighted / robust pair kernel, Layout::n_dg)
            TRY(dev_alloc(p, &p->d_part3, (size_t)p->M * std::max(64, std::max(chunks, chunks_w)) * (cam_acc_len(p->NP) + p->NP)));
        }
        if (p->L.C > 1) TRY(dev_alloc(p, &p->d_pair_part, (size_t)p->L.C * std::max<long long>(p->L.n_pairs, 1) * p->NP * p->NP));
        TRY(schur_item_tables(p));
        p->stage_len = std::max<size_t>(std::max<size_t>(n, 2 * (size_t)K), (size_t)6 * p->N) + 16;
        TRY(dev_alloc(p, &p->d_stage, p->stage_len));
        p->xb_len = satba_exchange_len(p);
        TRY(dev_alloc(p, &p->d_xb_own, p->xb_len));
        p->d_xb = p->d_xb_own;
        HIP_TRY(hipHostMalloc((void**)&p->h_pin, sizeof(double) * (p->hdr + 64)));
        HIP_TRY(hipMemset(p->d_xb, 0, sizeof(double) * p->xb_len));
        HIP_TRY(hipMemset(p->d_scale_inv, 0, sizeof(double) * n));
        HIP_TRY(hipMemset(p->d_x, 0, sizeof(double) * n));
        HIP_TRY(hipMemset(p->d_xnew, 0, sizeof(double) * n));
        HIP_TRY(hipMemcpy(p->d_cam_static, d->cam_params, sizeof(double) * p->M * p->c_p, hipMemcpyHostToDevice));
        if (p->model == RPC)
            HIP_TRY(hipMemcpy(p->d_rpc, d->rpc_tables, sizeof(double) * p->M * SATBA_RPC_TABLE_LEN, hipMemcpyHostToDevice));
        return 0;
    }();
    if (rc) {
        satba_problem_destroy(p);
        return rc;
    }
    p->create_ms[4] = ms_since(t_create);
    *out = p;
    return 0;
}

void satba_problem_destroy(satba_problem* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    (void)hipDeviceSynchronize();
#ifdef C3_STAMPS
    if (p->d_ts) {
        std::vector<long long> ts((size_t)20 * C3_TS);
        (void)hipMemcpy(ts.data(), p->d_ts, sizeof(long long) * ts.size(), hipMemcpyDeviceToHost);
        const int T = (p->n_c + 63) / 64;
        const long long t0 = ts[(size_t)T * C3_TS + 0];
        fprintf(stderr, "C3TS wait_begin 0 chain_start %.2f\n", (ts[(size_t)T * C3_TS + 1] - t0) * 0.01);
        for (int k = 0; k < T; ++k) {
            fprintf(stderr, "C3TS step %2d start %8.2f D_done %8.2f R %8.2f I %8.2f dnext %8.2f aux %8.2f nextD %8.2f | col arrived %8.2f handed %8.2f\n", k,
                    (ts[(size_t)k * C3_TS + 0] - t0) * 0.01, (ts[(size_t)k * C3_TS + 1] - t0) * 0.01, (ts[(size_t)k * C3_TS + 2] - t0) * 0.01,
                    (ts[(size_t)k * C3_TS + 3] - t0) * 0.01, (ts[(size_t)k * C3_TS + 4] - t0) * 0.01, (ts[(size_t)k * C3_TS + 5] - t0) * 0.01,
                    (ts[(size_t)k * C3_TS + 6] - t0) * 0.01, k >= 2 ? (ts[(size_t)T * C3_TS + k] - t0) * 0.01 : 0.0,
                    k >= 2 ? (ts[(size_t)(T + 1) * C3_TS + k] - t0) * 0.01 : 0.0);
        }
    }
#endif
    for (void* q : p->allocs) (void)hipFree(q);
    for (hipEvent_t e : p->prof_ev) (void)hipEventDestroy(e);
    if (p->h_pin) (void)hipHostFree(p->h_pin);
    if (p->h_stage) (void)hipHostFree(p->h_stage);
    for (auto& l : p->lanes) { if (l.pin) (void)hipHostFree(l.pin); for (hipEvent_t e : l.ev) if (e) (void)hipEventDestroy(e); }
    if (p->copy_stream) (void)hipStreamDestroy(p->copy_stream);
    if (p->ev_err) (void)hipEventDestroy(p->ev_err);
    if (p->h_lm) (void)hipHostFree(p->h_lm);
    if (p->own_stream) (void)hipStreamDestroy(p->own_stream);
    if (p->chol_stream) (void)hipStreamDestroy(p->chol_stream);
    if (p->ev_fork) (void)hipEventDestroy(p->ev_fork);
    if (p->ev_join) (void)hipEventDestroy(p->ev_join);
    delete p;
}

int satba_set_stream(satba_problem* p, void* hip_stream, int32_t use_own) {
    if (!p) return fail(SATBA_E_ARG, "null handle");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));  // nothing of this handle is left on the stream it moves away from
    p->stream = use_own ? p->own_stream : static_cast<hipStream_t>(hip_stream);
    return 0;
}

int64_t satba_header_len(const satba_problem* p) { return p ? p->hdr : 0; }

int64_t satba_exchange_len(const satba_problem* p) {
    if (!p) return 0;
    const long long lin = (long long)p->M * p->NP * p->NP + p->n_c;
    const long long sch = (long long)p->n_c * p->n_c + p->n_c;
    return p->hdr + (lin > sch ? lin : sch);
}

int satba_bind_exchange(satba_problem* p, double* device_ptr, int64_t len) {
    if (!p) return fail(SATBA_E_ARG, "null handle");
    if (!device_ptr) { p->d_xb = p->d_xb_own; return 0; }
    if (len < satba_exchange_len(p)) return fail(SATBA_E_ARG, "exchange buffer too small: %lld < %lld", (long long)len, (long long)satba_exchange_len(p));
    p->d_xb = device_ptr;
    return 0;
}

// lower triangle of S (column-major, n x n) <-> packed [header | rhs | column 0 | column 1 | ...]; block j = column j, block n = header and rhs.
// (Round 6: the right-hand side in FRONT of the columns, so that the first message of the pipelined exchange carries it.)
// c_lo, c_hi: only the columns in [c_lo, c_hi) (block n: only when c_lo == 0)
__global__ __launch_bounds__(256) void k_pack_lower(int n, int hdr, double* __restrict__ xb, double* __restrict__ packed, int unpack, int c_lo, int c_hi,
                                                    const int* gate) {
    SATBA_GATE(gate);
    const int j = blockIdx.x;
    if (j == n) {
        if (c_lo != 0) return;
        for (int i = threadIdx.x; i < hdr + n; i += 256) {
            double* a = i < hdr ? xb + i : xb + hdr + (size_t)n * n + (i - hdr);
            double* b = packed + i;
            if (unpack) __hip_atomic_store(a, __hip_atomic_load(b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else *b = *a;
        }
        return;
    }
    if (j < c_lo || j >= c_hi) return;
    double* col = xb + hdr + (size_t)j * n;
    double* pk = packed + hdr + n + ((long long)j * n - (long long)j * (j - 1) / 2) - j;  // pk[r] for r >= j
    for (int r = j + threadIdx.x; r < n; r += 256) {
        // (unpack: the payload may have come over a copy engine while kernels of this handle were running -- read past the caches,
        // system scope --, and a factorisation that is already waiting on the other stream reads S: write through)
        if (unpack) __hip_atomic_store(col + r, __hip_atomic_load(pk + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else pk[r] = col[r];
    }
}
// cameras [c_lo, c_hi) of the reduced system have arrived (k_chol_tiles waits for them: C3Args::arrive); first: the epoch word, too
__global__ void k_mark_arrived(int* __restrict__ arrive, int c_lo, int c_hi, int M, int epoch, int first, const int* gate) {
    SATBA_GATE(gate);
    const int c = c_lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (c < c_hi) __hip_atomic_store(arrive + (size_t)SCHUR_ARRIVE_STRIDE * c, M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (first && blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(arrive + (size_t)SCHUR_ARRIVE_STRIDE * M, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int64_t satba_packed_schur_len(const satba_problem* p) {
    return p ? p->hdr + (long long)p->n_c * (p->n_c + 1) / 2 + p->n_c : 0;
}

static int pack_schur_impl(satba_problem* p, double* packed, int unpack) {
    if (!p || !packed) return fail(SATBA_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    hipLaunchKernelGGL(k_pack_lower, dim3(p->n_c + 1), dim3(256), 0, p->stream, p->n_c, (int)p->hdr, p->d_xb, packed, unpack, 0, p->n_c, (const int*)nullptr);
    HIP_TRY(hipGetLastError());
    return 0;
}
int satba_pack_schur(satba_problem* p, double* packed) { return pack_schur_impl(p, packed, 0); }
int satba_unpack_schur(satba_problem* p, const double* packed) { return pack_schur_impl(p, const_cast<double*>(packed), 1); }

int satba_configure(satba_problem* p, int32_t loss, double f_scale) {
    if (!p) return fail(SATBA_E_ARG, "null handle");
    if (loss < 0 || loss > 4) return fail(SATBA_E_ARG, "unknown loss %d", loss);
    if (!(f_scale > 0.0)) return fail(SATBA_E_ARG, "f_scale must be positive");
    if (loss != p->loss || f_scale != p->f_scale) {
        p->linearized = false; p->have_step = false; p->prepared = false;
        p->fxcost_valid = false; p->fxcost_new_valid = false; p->fxcost0_valid = false;  // the kept costs belong to the old loss
    }
    p->loss = loss; p->f_scale = f_scale;
    p->lin_grid = lin_grid_for(p);
    return 0;
}

// Copies between the caller's (pageable) arrays and the device.  The runtime's first copy to or from a host range it has not seen
// costs 20 - 30 ms whatever its size (measured at 1 M observations, profiles/r5_e2e_C3.json: 28 ms for the 8 MB of errors, twice per
// call, where the transfer itself is 0.5 ms) -- and a caller's result arrays are new ranges every time.  Up to 32 MB the bytes go
// through a pinned buffer of the handle and one memcpy; larger transfers go direct (at 80 MB the direct copy runs at 15 GB/s and
// the extra memcpy would cost more than it saves).  Both wait for the stream.
constexpr size_t SATBA_STAGE_MAX = 32u << 20;
static int host_stage(satba_problem* p, size_t bytes) {
    if (p->h_stage_len >= bytes) return 0;
    if (p->h_stage) (void)hipHostFree(p->h_stage);
    p->h_stage = nullptr; p->h_stage_len = 0;
    HIP_TRY(hipHostMalloc((void**)&p->h_stage, bytes));
    p->h_stage_len = bytes;
    return 0;
}
// Large transfers (round 6; the drop-in call at 200 x 1M x 10M moves 208 MB: x up, x and two error vectors down).  A direct copy to or
// from a pageable array runs at ~15 GB/s -- the runtime's one staging thread: DMA into a bounce buffer, memcpy into pages that are
// touched for the first time -- and the bus does three times that.  Here copy_lanes() host threads share the memcpy side: thread t
// moves every copy_lanes()-th 4 MB chunk through two pinned halves of its own, the DMA of its next chunk under the memcpy of the
// current one.  ALL DMAs go through ONE extra stream (events tell a thread when its chunk has landed): the first version gave every
// thread a stream of its own, and with three or more streams alive beside the handle's the kernels of the LM loop ran 30 - 45 % slower
// for the rest of the process (200 x 1M x 10M: 594 against 859 it/s, a 5-evaluation solve 11.5 - 15 ms against 8.2; with one extra
// stream 8.1 - 8.3 -- profiles/r6_copy_lanes.txt).  `after`: an event the device-side data are complete at (else the caller has
// synchronised).  Does not touch p->stream or the staging buffer: safe beside a solve that another host thread drives on this handle
// (satba_reprojection_errors_fetch).
constexpr size_t COPY_CHUNK = 4u << 20, COPY_BIG_MIN = 8u << 20;
constexpr int COPY_LANES_MAX = 8;
static int copy_lanes() {  // SATBA_COPY_LANES: 1 .. 8 (experiments; default 4)
    static const int v = getenv("SATBA_COPY_LANES") ? std::max(1, std::min(COPY_LANES_MAX, atoi(getenv("SATBA_COPY_LANES")))) : 4;
    return v;
}
static int copy_lanes_init(satba_problem* p) {
    if (p->lanes_ready) return 0;
    HIP_TRY(hipStreamCreateWithFlags(&p->copy_stream, hipStreamNonBlocking));
    for (int t = 0; t < copy_lanes(); ++t) {
        HIP_TRY(hipHostMalloc((void**)&p->lanes[t].pin, 2 * COPY_CHUNK));
        for (int h = 0; h < 2; ++h) HIP_TRY(hipEventCreateWithFlags(&p->lanes[t].ev[h], hipEventDisableTiming));
    }
    p->lanes_ready = true;
    return 0;
}
static int copy_big(satba_problem* p, char* host, char* dev, size_t bytes, bool to_host, hipEvent_t after) {
    TRY(copy_lanes_init(p));
    const int T = copy_lanes();
    hipStream_t cs = p->copy_stream;
    if (after) HIP_TRY(hipStreamWaitEvent(cs, after, 0));  // (before any lane queues a chunk)
    std::atomic<int> err{0};
    const size_t n_chunks = (bytes + COPY_CHUNK - 1) / COPY_CHUNK;
    auto work = [&](int t) {
        if (hipSetDevice(p->device) != hipSuccess) { err = 1; return; }
        auto& L = p->lanes[t];
        // my chunks: t, t + T, ...; round i uses half i & 1
        size_t prev_off = 0, prev_len = 0;
        int i = 0;
        for (size_t c = t;; c += T, ++i) {
            const size_t off = c * COPY_CHUNK;
            const size_t len = c < n_chunks ? std::min(COPY_CHUNK, bytes - off) : 0;
            char* cur = L.pin + (size_t)(i & 1) * COPY_CHUNK;
            char* prv = L.pin + (size_t)((i + 1) & 1) * COPY_CHUNK;
            if (to_host) {
                if (len && (hipMemcpyAsync(cur, dev + off, len, hipMemcpyDeviceToHost, cs) != hipSuccess || hipEventRecord(L.ev[i & 1], cs) != hipSuccess)) err = 1;
                if (prev_len) memcpy(host + prev_off, prv, prev_len);  // (its event was waited for at the end of the previous round)
                if (len && hipEventSynchronize(L.ev[i & 1]) != hipSuccess) err = 1;
            } else {
                // chunk i goes into its pinned half while the DMA of chunk i - 1 (other half) runs; that half is free again when the DMA
                // of chunk i - 2 has finished: its event, waited for here
                if (len && i >= 2 && hipEventSynchronize(L.ev[i & 1]) != hipSuccess) err = 1;
                if (len) memcpy(cur, host + off, len);
                if (len && (hipMemcpyAsync(dev + off, cur, len, hipMemcpyHostToDevice, cs) != hipSuccess || hipEventRecord(L.ev[i & 1], cs) != hipSuccess)) err = 1;
            }
            prev_off = off; prev_len = len;
            if (err || !len) break;
        }
    };
    std::thread th[COPY_LANES_MAX];
    for (int t = 1; t < T; ++t) th[t] = std::thread(work, t);
    work(0);
    for (int t = 1; t < T; ++t) th[t].join();
    if (!to_host && hipStreamSynchronize(cs) != hipSuccess) err = 1;  // every upload has landed
    if (err) return fail(SATBA_E_HIP, "a chunk of a large host transfer failed");
    return 0;
}
static int copy_to_host(satba_problem* p, void* host, const void* dev, size_t bytes) {
    if (bytes == 0) { HIP_TRY(hipStreamSynchronize(p->stream)); return 0; }
    if (bytes >= COPY_BIG_MIN && !getenv("SATBA_COPY_DIRECT")) {
        HIP_TRY(hipStreamSynchronize(p->stream));
        return copy_big(p, static_cast<char*>(host), static_cast<char*>(const_cast<void*>(dev)), bytes, true, nullptr);
    }
    if (bytes > SATBA_STAGE_MAX) {
        HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return 0;
    }
    TRY(host_stage(p, bytes));
    HIP_TRY(hipMemcpyAsync(p->h_stage, dev, bytes, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    memcpy(host, p->h_stage, bytes);
    return 0;
}
static int copy_to_device_async(satba_problem* p, void* dev, const void* host, size_t bytes) {
    if (bytes == 0) return 0;
    if (bytes >= COPY_BIG_MIN && !getenv("SATBA_COPY_DIRECT")) {
        HIP_TRY(hipStreamSynchronize(p->stream));  // (whatever still reads the destination has passed; the lanes' streams are not ordered with it)
        return copy_big(p, static_cast<char*>(const_cast<void*>(host)), static_cast<char*>(dev), bytes, false, nullptr);  // complete on return
    }
    if (bytes > SATBA_STAGE_MAX) { HIP_TRY(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, p->stream)); return 0; }
    HIP_TRY(hipStreamSynchronize(p->stream));  // (an earlier copy out of the pinned buffer may still be queued)
    TRY(host_stage(p, bytes));
    memcpy(p->h_stage, host, bytes);
    HIP_TRY(hipMemcpyAsync(dev, p->h_stage, bytes, hipMemcpyHostToDevice, p->stream));
    return 0;
}

// host vector in the caller's point order -> device vector in internal order (and back); dim doubles per point
static int upload_permuted(satba_problem* p, const double* host, double* dev, int n_c, int dim) {
    const size_t len = (size_t)n_c + (size_t)p->N * dim;
    if (len > p->stage_len) return fail(SATBA_E_ARG, "staging buffer too small");
    TRY(copy_to_device_async(p, p->d_stage, host, sizeof(double) * len));
    hipLaunchKernelGGL(k_permute_vec, dim3(grid_for((long long)len, 256, 2048)), dim3(256), 0, p->stream, n_c, p->N, dim, p->L.perm, p->d_stage, dev, 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(p->stream));
    return 0;
}
static int download_permuted(satba_problem* p, const double* dev, double* host, int n_c, int dim) {
    const size_t len = (size_t)n_c + (size_t)p->N * dim;
    if (len > p->stage_len) return fail(SATBA_E_ARG, "staging buffer too small");
    hipLaunchKernelGGL(k_permute_vec, dim3(grid_for((long long)len, 256, 2048)), dim3(256), 0, p->stream, n_c, p->N, dim, p->L.perm, dev, p->d_stage, 1);
    HIP_TRY(hipGetLastError());
    return copy_to_host(p, host, p->d_stage, sizeof(double) * len);
}

int satba_set_x(satba_problem* p, const double* host_x) {
    if (!p || !host_x) return fail(SATBA_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    TRY(upload_permuted(p, host_x, p->d_x, p->n_c, 3));
    TRY(launch_cam_consts(p, false));
    hipLaunchKernelGGL(k_bbox, dim3(1), dim3(1024), 0, p->stream, p->N, p->d_x + p->n_c, p->d_bbox);
    HIP_TRY(hipGetLastError());
    p->linearized = false; p->have_step = false; p->prepared = false; p->fxcost_valid = false; p->fxcost_new_valid = false;
    return 0;
}

// device-side copy of the current point: restore == 0 keeps it, restore != 0 goes back to it (no host transfer)
int satba_snapshot_x(satba_problem* p, int32_t restore) {
    if (!p) return fail(SATBA_E_ARG, "null handle");
    HIP_TRY(hipSetDevice(p->device));
    if (!restore) {
        if (!p->d_x0) TRY(dev_alloc(p, &p->d_x0, p->n + 6 + (size_t)p->M * CAMC));  // x | bounding box of its points | camera constants
        HIP_TRY(hipMemcpyAsync(p->d_x0, p->d_x, sizeof(double) * p->n, hipMemcpyDeviceToDevice, p->stream));
        HIP_TRY(hipMemcpyAsync(p->d_x0 + p->n, p->d_bbox, sizeof(double) * 6, hipMemcpyDeviceToDevice, p->stream));
        HIP_TRY(hipMemcpyAsync(p->d_x0 + p->n + 6, p->d_camc, sizeof(double) * p->M * CAMC, hipMemcpyDeviceToDevice, p->stream));
        // the cost at the kept point travels with it (scales of the fixed-point camera sums, linear loss)
        if (p->loss == 0 && !p->fxcost_valid) {
            TRY(launch_residual(p, false, nullptr, p->d_fxcost));
            p->fxcost_valid = true;
        }
        p->fxcost0_valid = p->fxcost_valid;
        if (p->fxcost_valid) HIP_TRY(hipMemcpyAsync(p->d_fxcost0, p->d_fxcost, sizeof(double), hipMemcpyDeviceToDevice, p->stream));
        return 0;
    }
    if (!p->d_x0) return fail(SATBA_E_STATE, "restore before snapshot");
    HIP_TRY(hipMemcpyAsync(p->d_x, p->d_x0, sizeof(double) * p->n, hipMemcpyDeviceToDevice, p->stream));
    HIP_TRY(hipMemcpyAsync(p->d_bbox, p->d_x0 + p->n, sizeof(double) * 6, hipMemcpyDeviceToDevice, p->stream));
    TRY(launch_cam_consts(p, false));
    p->fxcost_valid = p->fxcost0_valid; p->fxcost_new_valid = false;
    if (p->fxcost0_valid) HIP_TRY(hipMemcpyAsync(p->d_fxcost, p->d_fxcost0, sizeof(double), hipMemcpyDeviceToDevice, p->stream));
    p->linearized = false; p->have_step = false; p->prepared = false; p->f_valid = false;
    return 0;
}

int satba_get_x(satba_problem* p, double* host_x) {
    if (!p || !host_x) return fail(SATBA_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    return download_permuted(p, p->d_x, host_x, p->n_c, 3);
}

int satba_residuals(satba_problem* p, double* host_r, double* host_cost) {
    Range range_("satba:residuals");
    if (!p) return fail(SATBA_E_ARG, "null handle");
    HIP_TRY(hipSetDevice(p->device));
    // the cost goes through a private scalar so the exchange header of a running solve is left alone; the residual pairs go
    // to their own buffer (d_f holds the residuals of the current linearisation) and from there, in the caller's observation
    // order, through the staging buffer
    double* slot = p->d_scal;
    double2* f_obs = reinterpret_cast<double2*>(p->d_stage);
    const bool want = host_r != nullptr && p->K > 0;
    TRY(launch_residual(p, false, want ? p->d_ftmp : nullptr, slot));
    HIP_TRY(hipMemcpyAsync(p->h_pin, slot, sizeof(double), hipMemcpyDeviceToHost, p->stream));
    if (want) {
        hipLaunchKernelGGL(k_gather_obs, dim3(grid_for(p->K, 256, 4096)), dim3(256), 0, p->stream, p->K, p->L.obs_pos, p->d_ftmp, f_obs);
        HIP_TRY(hipGetLastError());
        TRY(copy_to_host(p, host_r, f_obs, sizeof(double) * 2 * p->K));
    }
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (host_cost) *host_cost = p->h_pin[0];
    return 0;
}

// ---- the phases as the loops below queue them: a context per call, the state checks of the ABI (a loop may be driven from outside
// part by part: satba_lm_part), the range marker; the public entry points add the handle check and the device
static int linearize_impl(satba_problem* p, const PhaseCtx& c) {
    Range range_("satba:linearize");
    TRY(ensure_wlayout(p));
    const size_t nU = (size_t)p->M * p->NP * p->NP;
    const int n_clear = (int)(p->hdr + nU + p->n_c);  // header, U (only its diagonal is written), g_c
    if (p->cam_sums_lds) {
        // scales of the fixed-point camera sums: the linear loss bounds a residual by sqrt(2 cost(x)) -- the cost of the trial
        // evaluation that led here (satba_accept), else one cost-only pass
        if (p->loss == 0 && !p->fxcost_valid) {
            TRY(launch_residual(p, false, nullptr, p->d_fxcost, c.gate));
            p->fxcost_valid = true;
        }
        if (!c.skip_lin_scales)  // (device-resident loop on one rank: the previous tick's k_lm_accept_scales has done it)
        SATBA_DISPATCH(p, hipLaunchKernelGGL((k_lin_scales<MODEL, NP>), dim3(1), dim3(256), 0, p->stream, p->M, p->d_camc, p->d_rpc, p->d_bbox, p->w_max,
                                             p->loss, p->f_scale, p->d_fxcost, p->n_max_cam, p->fx_shrink, p->d_fx, p->d_fxe, p->d_fxflag, p->d_xb, n_clear, c.gate));
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemsetAsync(p->d_xb, 0, sizeof(double) * n_clear, p->stream));
    }
    const bool store_gh = points_gh_stored(p, c);  // (decided once per linearisation: the kernel and the readers' launchers must agree)
    TRY(launch_linearize_kernel(p, c, store_gh));
    double* U = p->payload();
    double* gc = U + nU;
    if (p->cam_sums_lds) {
        // unit weights + linear loss + affine R+T: the translation entries of diag(U_c) are (observation count) x constants
        // and were not accumulated by the kernel (lin_const_t in satba_kernels.h)
        const int const_t = lin_const_t(p->model, p->NP, p->loss != 0, unit_run(p)) && lin_variant(p) == 0;
        const int total = p->M * 2 * p->NP;
        hipLaunchKernelGGL(k_lin_finish, dim3((total + 63) / 64), dim3(1024), 0, p->stream, p->M, p->NP, p->lin_grid, p->d_part, U, gc,
                           p->L.cam_ofs, p->d_camc, p->n_cam_fix, const_t, p->d_fx, p->d_fxe, p->d_fxflag, p->d_xb + SATBA_HDR_FX, c.gate);
        HIP_TRY(hipGetLastError());
    } else {
        TRY(launch_cam_sums(p, c.gate, U, gc));  // camera-major pass, fixed summation order; fills the full blocks
    }
    p->linearized = true; p->have_step = false;
    p->f_valid = !p->cam_sums_lds && p->model == RPC;
    p->prep_fused = c.fuse_prep >= 0;
    p->gh_in_readers = !store_gh;
    p->q1_points_unformed = false;
    return 0;
}
int satba_linearize(satba_problem* p) {
    if (!p) return fail(SATBA_E_ARG, "null handle");
    HIP_TRY(hipSetDevice(p->device));
    return linearize_impl(p, PhaseCtx{});
}

static int prepare_impl(satba_problem* p, const PhaseCtx& c, int first) {
    Range range_("satba:prepare");
    if (!p->linearized) return fail(SATBA_E_STATE, "prepare before linearize");
    const size_t nU = (size_t)p->M * p->NP * p->NP;
    if (p->hdr > 1024) return fail(SATBA_E_ARG, "header too long");
    if (p->prep_fused && p->n_c <= 1024) {  // the point entries are done (k_linearize): stash and camera entries in one launch
        hipLaunchKernelGGL(k_prepare_cams, dim3(1), dim3(1024), 0, p->stream, (int)nU, p->n_c, p->NP, p->world, SATBA_HDR_FIXED, (int)p->hdr, first, p->lead,
                           p->d_xb, p->d_U, p->d_gc, p->d_keep, p->d_x, p->d_g, p->d_scale_inv, p->d_gh, p->d_q1, c.first_dev, c.gate);
        HIP_TRY(hipGetLastError());
        TRY(launch_jvp(p, c.gate, 1, p->d_q1, p->d_q1, p->d_xb + SATBA_HDR_JG_SQ, true));  // d_q1 is free until the subspace phase
        p->q1_points_unformed = p->gh_in_readers;  // (only the camera entries of q1 = g_h / scale_inv were written: satba_get_vector)
        p->prepared = true;
        return 0;
    }
    hipLaunchKernelGGL(k_prepare_stash, dim3(1), dim3(1024), 0, p->stream, (int)nU, p->n_c, p->world, SATBA_HDR_FIXED, (int)p->hdr, p->d_xb, p->d_U,
                       p->d_gc, p->d_keep, c.gate);
    HIP_TRY(hipGetLastError());
    const int n_prep = p->prep_fused ? p->n_c : p->n;  // fused: the point entries are done
    hipLaunchKernelGGL(k_prepare_vec, dim3(grid_for(n_prep, 256, 1024)),  // measured at 3 M entries: 512 workgroups 51 us, 1024: 45, 2048: 55
                       dim3(256), 0, p->stream, n_prep, p->n_c, p->NP, first,
                       p->lead, p->d_U, p->d_gc, p->d_V, p->d_x, p->d_g, p->d_scale_inv, p->d_gh, p->d_q1, p->red(RB_PREP), p->d_xb, p->d_keep, c.first_dev, c.gate);
    HIP_TRY(hipGetLastError());
    TRY(launch_jvp(p, c.gate, 1, p->d_q1, p->d_q1, p->d_xb + SATBA_HDR_JG_SQ, true));  // d_q1 is free until the subspace phase
    p->prepared = true;
    return 0;
}
int satba_prepare(satba_problem* p, int32_t first) {
    if (!p) return fail(SATBA_E_ARG, "null handle");
    HIP_TRY(hipSetDevice(p->device));
    return prepare_impl(p, PhaseCtx{}, first);
}

static int solve_impl(satba_problem* p, const PhaseCtx& c);
#include "satba_schur_api.inc"

static int solve_impl(satba_problem* p, const PhaseCtx& c) {
    Range range_("satba:solve");
    double* S = p->payload();
    double* rhs = S + (size_t)p->n_c * p->n_c;
    if (p->n_c <= CH_ONE_LAUNCH) {
        hipLaunchKernelGGL(k_solve_small, dim3(1), dim3(256), 0, p->stream, p->n_c, p->d_scale_inv, S, rhs, p->d_dch, p->d_dc, p->d_fail, 1 + CH_MAX_STEPS,
                           (int)p->hdr, p->d_xb, p->lead, p->d_keep, SATBA_HDR_KEEP, SATBA_KEEP_LEN, c.gate);
        HIP_TRY(hipGetLastError());
        TRY(launch_backsub_kernel(p, c.gate));
        p->have_step = true;
        return 0;
    }
    if (p->s_scaled) p->s_scaled = false;  // k_schur_finish has scaled the system and cleared the solver's status words
    else hipLaunchKernelGGL(k_scale_system, dim3(grid_for((long long)p->n_c * p->n_c, 256, 2048)), dim3(256), 0, p->stream, p->n_c,
                            p->d_scale_inv, S, rhs, p->d_dch, p->d_fail, 1 + CH_MAX_STEPS, c.gate, 0, p->n_c);
    HIP_TRY(hipGetLastError());
    bool unscaled = false;
    TRY(dense_solve(p, c.gate, S, p->d_dch, true, &unscaled));  // the not-SPD flag and the step flags were cleared by the scaling kernel
    if (!unscaled) {
        const int nu = std::max(p->n_c, (int)p->hdr);
        hipLaunchKernelGGL(k_unscale, dim3((nu + 255) / 256), dim3(256), 0, p->stream, p->n_c, p->d_scale_inv, p->d_dch, p->d_dc, (int)p->hdr,
                           p->d_xb, p->d_fail, p->lead, p->d_keep, SATBA_HDR_KEEP, SATBA_KEEP_LEN, c.gate);
        HIP_TRY(hipGetLastError());
    }
    TRY(launch_backsub_kernel(p, c.gate));
    p->have_step = true;
    return 0;
}
int satba_solve(satba_problem* p) {
    if (!p) return fail(SATBA_E_ARG, "null handle");
    HIP_TRY(hipSetDevice(p->device));
    return solve_impl(p, PhaseCtx{});
}

static int subspace_impl(satba_problem* p, const PhaseCtx& c, double alpha, double inv_norm_g) {
    Range range_("satba:subspace");
    if (!p->have_step) return fail(SATBA_E_STATE, "subspace before solve");
    if (!c.gate) TRY(zero_header(p));  // (the device-resident loop reads only the slots this phase writes)
    hipLaunchKernelGGL(k_subspace_vec, dim3(grid_for(p->n, 256, 512)), dim3(256), 0, p->stream, p->n, p->n_c, p->lead, alpha,
                       inv_norm_g, p->d_gh, p->d_gn, p->d_q1, p->d_wv, p->red(RB_SUB), p->d_xb, c.sub_args_dev, c.gate,
                       p->gh_in_readers ? p->d_g : nullptr, p->d_scale_inv);
    HIP_TRY(hipGetLastError());
    p->q1_points_unformed = false;  // (every entry of q1 is written)
    return 0;
}
int satba_subspace(satba_problem* p, double alpha, double inv_norm_g) {
    if (!p) return fail(SATBA_E_ARG, "null handle");
    HIP_TRY(hipSetDevice(p->device));
    return subspace_impl(p, PhaseCtx{}, alpha, inv_norm_g);
}

static int subspace_products_impl(satba_problem* p, const PhaseCtx& c) {
    Range range_("satba:subspace_products");
    if (!p->have_step) return fail(SATBA_E_STATE, "subspace_products before solve");
    if (!c.gate) TRY(zero_header(p));
    return launch_jvp(p, c.gate, 2, p->d_q1, p->d_wv, p->d_xb + SATBA_HDR_B11);
}
int satba_subspace_products(satba_problem* p) {
    if (!p) return fail(SATBA_E_ARG, "null handle");
    HIP_TRY(hipSetDevice(p->device));
    return subspace_products_impl(p, PhaseCtx{});
}

// the trial point x + c0 v0 + c1 v1: gn, along (g_h, gn_h) (satba_trial_gn), else along the subspace vectors (q1, w)
static int trial_impl(satba_problem* p, const PhaseCtx& c, bool gn, double c0, double c1) {
    Range range_("satba:trial");
    if (!p->have_step) return fail(SATBA_E_STATE, "trial before solve");
    return launch_trial(p, c, c0, c1, gn ? p->d_gh : p->d_q1, gn ? p->d_gn : p->d_wv);  // k_trial_cams clears the header
}
int satba_trial(satba_problem* p, double p0, double p1) {
    if (!p) return fail(SATBA_E_ARG, "null handle");
    HIP_TRY(hipSetDevice(p->device));
    return trial_impl(p, PhaseCtx{}, false, p0, p1);
}
int satba_trial_gn(satba_problem* p, double ca, double cb) {
    if (!p) return fail(SATBA_E_ARG, "null handle");
    HIP_TRY(hipSetDevice(p->device));
    return trial_impl(p, PhaseCtx{}, true, ca, cb);
}

int satba_accept(satba_problem* p) {
    Range range_("satba:accept");
    if (!p) return fail(SATBA_E_ARG, "null handle");
    std::swap(p->d_x, p->d_xnew);
    std::swap(p->d_camc, p->d_camc_new);
    std::swap(p->d_fxcost, p->d_fxcost_new);  // the cost of the trial evaluation is the cost at the new x
    p->fxcost_valid = p->fxcost_new_valid; p->fxcost_new_valid = false;
    p->linearized = false; p->have_step = false; p->prepared = false;
    return 0;
}

int satba_camera_sums_fallback(satba_problem* p) {
    if (!p) return fail(SATBA_E_ARG, "null handle");
    if (p->cam_sums_lds) { p->cam_sums_lds = 0; ++p->fx_fallbacks; }
    p->linearized = false; p->have_step = false; p->prepared = false;
    return 0;
}

int satba_read_header(satba_problem* p, double* host_hdr) {
    if (!p || !host_hdr) return fail(SATBA_E_ARG, "null argument");
    HIP_TRY(hipMemcpyAsync(p->h_pin, p->d_xb, sizeof(double) * p->hdr, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    memcpy(host_hdr, p->h_pin, sizeof(double) * p->hdr);
    return 0;
}

#include "satba_lm_api.inc"

// ---------------------------------------------------------------------------------------------------- inspection
int satba_get_blocks(satba_problem* p, double* U, double* gc, double* V, double* gp) {
    if (!p) return fail(SATBA_E_ARG, "null handle");
    if (!p->linearized) return fail(SATBA_E_STATE, "get_blocks before linearize");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    const size_t nU = (size_t)p->M * p->NP * p->NP;
    if (U) {
        // the linearize kernel only keeps diag(U_c): form the full blocks with the camera-major pass (inspection only)
        double *dU = nullptr, *dg = nullptr;
        DevAllocs tmp;
        TRY(tmp.alloc(&dU, nU));
        TRY(tmp.alloc(&dg, (size_t)p->n_c));
        if (!p->f_valid) {  // the default linearize kernel does not store the residuals: evaluate them for this view
            TRY(launch_residual(p, false, p->d_f, p->d_scal));
            p->f_valid = true;
        }
        TRY(launch_cam_sums(p, nullptr, dU, dg));
        HIP_TRY(hipStreamSynchronize(p->stream));
        HIP_TRY(hipMemcpy(U, dU, sizeof(double) * nU, hipMemcpyDeviceToHost));
    }
    if (gc) HIP_TRY(hipMemcpy(gc, p->payload() + nU, sizeof(double) * p->n_c, hipMemcpyDeviceToHost));
    if (V) TRY(download_permuted(p, p->d_V, V, 0, 6));
    if (gp) TRY(download_permuted(p, p->d_g + p->n_c, gp, 0, 3));
    return 0;
}

int satba_get_jacobian(satba_problem* p, double* Jc, double* Jp) {
    if (!p || !Jc || !Jp) return fail(SATBA_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    double *dJc = nullptr, *dJp = nullptr;
    DevAllocs tmp;
    TRY(tmp.alloc(&dJc, (size_t)(2 * p->K * p->NP + 1)));
    TRY(tmp.alloc(&dJp, (size_t)(6 * p->K + 1)));
    ObsArgs a = obs_args(p, false);
    SATBA_DISPATCH(p, hipLaunchKernelGGL((k_jacobian<MODEL, NP>), dim3(grid_for(p->K, 256, 1024)), dim3(256), 0, p->stream, a, p->L.pts_ind,
                                         p->L.rank, p->L.obs_pos, dJc, dJp));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(p->stream));
    HIP_TRY(hipMemcpy(Jc, dJc, sizeof(double) * 2 * p->K * p->NP, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(Jp, dJp, sizeof(double) * 6 * p->K, hipMemcpyDeviceToHost));
    return 0;
}

int satba_get_exchange(satba_problem* p, int64_t offset, int64_t n, double* host_out) {
    if (!p || !host_out) return fail(SATBA_E_ARG, "null argument");
    if (offset < 0 || n < 0 || offset + n > p->xb_len) return fail(SATBA_E_ARG, "exchange range out of bounds");
    HIP_TRY(hipStreamSynchronize(p->stream));
    HIP_TRY(hipMemcpy(host_out, p->d_xb + offset, sizeof(double) * n, hipMemcpyDeviceToHost));
    return 0;
}

int satba_set_exchange(satba_problem* p, int64_t offset, int64_t n, const double* host_in) {
    if (!p || !host_in) return fail(SATBA_E_ARG, "null argument");
    if (offset < 0 || n < 0 || offset + n > p->xb_len) return fail(SATBA_E_ARG, "exchange range out of bounds");
    HIP_TRY(hipStreamSynchronize(p->stream));
    HIP_TRY(hipMemcpy(p->d_xb + offset, host_in, sizeof(double) * n, hipMemcpyHostToDevice));
    return 0;
}

int satba_profile_linearize(satba_problem* p, int32_t on) {
    if (!p) return fail(SATBA_E_ARG, "null handle");
    p->prof_lin = on != 0;
    return 0;
}

int satba_profile_read(satba_problem* p, int64_t* n_launches, double* ms_total) {
    if (!p || !n_launches || !ms_total) return fail(SATBA_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    double tot = 0.0;
    for (size_t i = 0; i + 1 < p->prof_used; i += 2) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, p->prof_ev[i], p->prof_ev[i + 1]));
        tot += ms;
    }
    *n_launches = (int64_t)(p->prof_used / 2);
    *ms_total = tot;
    p->prof_used = 0;
    return 0;
}

int satba_get_vector(satba_problem* p, int32_t which, double* host_out) {
    if (!p || !host_out) return fail(SATBA_E_ARG, "null argument");
    const double* src[] = {p->d_g, p->d_scale_inv, p->d_gn, p->d_q1, p->d_wv, p->d_xnew, p->d_gh};
    if (which < 0 || which > 6) return fail(SATBA_E_ARG, "unknown vector id %d", which);
    HIP_TRY(hipSetDevice(p->device));
    // the loops' linearisation leaves the point entries of g_h -- and of q1 = g_h / scale_inv, until a subspace phase overwrites q1 -- to their readers: formed here
    const bool fill_gh = which == 6 && p->gh_in_readers, fill_q1 = which == 3 && p->gh_in_readers && p->q1_points_unformed;
    if (fill_gh || fill_q1) {
        hipLaunchKernelGGL(k_fill_point_gh, dim3(grid_for(p->n - p->n_c, 256, 1024)), dim3(256), 0, p->stream, (long long)p->n_c, (long long)p->n, p->d_g,
                           p->d_scale_inv, fill_gh ? p->d_gh : (double*)nullptr, fill_q1 ? p->d_q1 : (double*)nullptr);
        if (fill_q1) p->q1_points_unformed = false;
        HIP_TRY(hipGetLastError());
    }
    return download_permuted(p, src[which], host_out, p->n_c, 3);
}

int64_t satba_layout_len(const satba_problem* p, int32_t which) {
    if (!p) return -1;
    const Layout& L = p->L;
    switch (which) {
        case SATBA_LAY_PERM: case SATBA_LAY_RANK: case SATBA_LAY_PT_CNT: return L.N;
        case SATBA_LAY_SLICE_BASE: return L.n_slices + 1;
        case SATBA_LAY_E_CAM: return L.P;
        case SATBA_LAY_E_CAM8: return L.e_cam8 ? L.P : -1;
        case SATBA_LAY_OBS_POS: case SATBA_LAY_CM_PT: case SATBA_LAY_CM_POS: case SATBA_LAY_CM_IO: return L.K;
        case SATBA_LAY_IPT_OFS: return L.N + 1;
        case SATBA_LAY_CAM_OFS: return L.M + 1;
        case SATBA_LAY_PAIR_OFS: return L.n_pairs * (L.C + 1) + 1;
        case SATBA_LAY_PAIR_PTS: case SATBA_LAY_PAIR_PI: case SATBA_LAY_PAIR_PJ: return L.E;
        case SATBA_LAY_PAIR_IJ: return 2 * L.n_pairs;
        case SATBA_LAY_W_FIX: case SATBA_LAY_SC_OFS: return L.wl_ready ? L.N + 1 : -1;
        case SATBA_LAY_PAIR_REC: case SATBA_LAY_PAIR_KK: return L.wl_ready ? L.E : -1;
        case SATBA_LAY_CM_REC: case SATBA_LAY_CM_SC: return L.wl_ready ? L.K : -1;
        case SATBA_LAY_DG_OFS: return L.wl_ready ? (long long)L.M * L.n_dg + 1 : -1;
        default: return -1;
    }
}

int satba_get_layout(satba_problem* p, int32_t which, int64_t n, void* host_out) {
    if (!p || !host_out) return fail(SATBA_E_ARG, "null argument");
    const int64_t len = satba_layout_len(p, which);
    if (len < 0 || n != len) return fail(SATBA_E_ARG, "layout array %d has %lld entries, caller expects %lld", which, (long long)len, (long long)n);
    const Layout& L = p->L;
    const void* src = nullptr;
    size_t esz = sizeof(int);
    switch (which) {
        case SATBA_LAY_PERM: src = L.perm; break;
        case SATBA_LAY_RANK: src = L.rank; break;
        case SATBA_LAY_PT_CNT: src = L.pt_cnt; break;
        case SATBA_LAY_SLICE_BASE: src = L.slice_base; break;
        case SATBA_LAY_E_CAM: src = L.e_cam; break;
        case SATBA_LAY_E_CAM8: src = L.e_cam8; esz = 1; break;
        case SATBA_LAY_OBS_POS: src = L.obs_pos; break;
        case SATBA_LAY_CM_PT: src = L.cm_pt; break;
        case SATBA_LAY_CM_POS: src = L.cm_pos; break;
        case SATBA_LAY_CM_IO: src = L.cm_io; break;
        case SATBA_LAY_IPT_OFS: src = L.ipt_ofs; break;
        case SATBA_LAY_CAM_OFS: src = L.cam_ofs; break;
        case SATBA_LAY_PAIR_OFS: src = L.pair_ofs; esz = sizeof(long long); break;
        case SATBA_LAY_PAIR_PTS: src = L.pair_pts; break;
        case SATBA_LAY_PAIR_PI: src = L.pair_pi; break;
        case SATBA_LAY_PAIR_PJ: src = L.pair_pj; break;
        case SATBA_LAY_PAIR_IJ: src = L.pair_ij; break;
        case SATBA_LAY_W_FIX: src = L.w_fix; break;
        case SATBA_LAY_SC_OFS: src = L.sc_ofs; break;
        case SATBA_LAY_PAIR_REC: src = L.pair_rec; break;
        case SATBA_LAY_PAIR_KK: src = L.pair_kk; break;
        case SATBA_LAY_CM_REC: src = L.cm_rec; break;
        case SATBA_LAY_CM_SC: src = L.cm_sc; break;
        case SATBA_LAY_DG_OFS: src = L.dg_ofs; break;
        default: return fail(SATBA_E_ARG, "unknown layout array %d", which);
    }
    HIP_TRY(hipSetDevice(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (len) HIP_TRY(hipMemcpy(host_out, src, esz * (size_t)len, hipMemcpyDeviceToHost));
    return 0;
}

int satba_get_info(const satba_problem* p, double* out, int32_t n) {
    if (!p || !out || n < 16) return fail(SATBA_E_ARG, "bad argument");
    for (int i = 0; i < n; ++i) out[i] = 0.0;
    for (int i = 0; i < 5; ++i) out[i] = p->create_ms[i];
    out[5] = p->L.P; out[6] = (double)p->L.E; out[7] = p->L.C; out[8] = p->unit_weights; out[9] = p->camc_lds; out[10] = p->rpc_lds;
    out[11] = p->cam_sums_lds; out[12] = p->deterministic; out[13] = p->cm_chunks; out[14] = p->lin_grid; out[15] = p->fx_fallbacks;
    if (n > 16) out[16] = (lm_device_loop_ok(p) && lm_device_loop_pays(p)) ? 1.0 : 0.0;
    if (n > 17) out[17] = p->beside_off ? -1.0 : (p->beside_last ? 1.0 : 0.0);
    if (n > 18) out[18] = p->beside_timeouts;
    if (n > 19) out[19] = p->L.wl_ready ? p->L.dg_spc : 0;
    if (n > 20) out[20] = slice_split(p);
    if (n > 21) out[21] = p->lin_rep_shift;
    if (n > 22) out[22] = p->diag_split_last;
    if (n > 23) out[23] = p->cam_narrow;
    return 0;
}

int satba_time_kernel(satba_problem* p, int32_t phase, int32_t reps, float* ms_avg) {
    if (!p || !ms_avg || reps <= 0) return fail(SATBA_E_ARG, "bad argument");
    if (phase < 0 || phase > 5) return fail(SATBA_E_ARG, "unknown phase %d", phase);
    if (phase >= 2 && !p->linearized) return fail(SATBA_E_STATE, "time_kernel: linearize first");
    HIP_TRY(hipSetDevice(p->device));
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    // scratch outputs so a measurement never disturbs solver state that a later phase reads
    int rc = 0;
    auto once = [&]() -> int {
        switch (phase) {
            case 0: return launch_residual(p, false, p->d_f, p->d_scal);
            case 1: return launch_linearize_kernel(p, PhaseCtx{}, true);  // (not fused: the flag is not looked at)
            case 2: return launch_schur_kernel(p, nullptr, FrontCtx{}, schur_route(p, FrontCtx{}));
            case 3: {
                // factorising an already factorised matrix is meaningless numerically but identical in work
                return dense_solve(p, nullptr, p->payload(), p->d_dch);
            }
            case 4: return launch_backsub_kernel(p, nullptr);
            default: return launch_jvp(p, nullptr, 1, p->d_q1, p->d_q1, p->d_scal, true);  // the pass of the prepare phase
        }
    };
    rc = once();  // warm-up
    if (!rc) {
        (void)hipEventRecord(e0, p->stream);
        for (int i = 0; i < reps && !rc; ++i) rc = once();
        (void)hipEventRecord(e1, p->stream);
        (void)hipEventSynchronize(e1);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        *ms_avg = ms / reps;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    p->linearized = false; p->have_step = false;  // blocks / exchange payload were overwritten
    return rc;
}

#include "satba_outliers_api.inc"
#include "satba_triangulate_api.inc"
#include "satba_rpcfit_api.inc"
#include "satba_camapprox_api.inc"
#include "satba_fundamental_api.inc"
#include "satba_ransac_api.inc"
#include "satba_utm_api.inc"
#include "satba_tracks_api.inc"
#include "satba_ftracks_api.inc"
#include "satba_match_api.inc"
#include "satba_window_api.inc"
#include "satba_sift_api.inc"

}  // extern "C"

"""
Scenarios of the point kernels' two launch parameters (csrc/satba_kernels.h: SliceUnit, for_each_slice; csrc/satba_capi.hip:
slice_split, lin_rep_shift), shared by tests/test_lanes_cases_host.py and tests/test_gpu_lanes.py.  Nothing here needs a GPU: the
builders make the scenes at which the lanes of a point, the walk over the slices and the replicas of the camera-sum table can go
wrong, and restate the rules that pick the parameters from the constants of the code.

  lanes per point   2^sh lanes share a point's observations (slot g, g + 2^sh, ... of its track); sh comes from slice_split():
                    SATBA_SPLIT (0 .. 3) | 0 for deterministic handles | the smallest sh <= 3 with n_slices << sh >= 3000 |
                    at least 1 unless every weight is 1 and the loss is linear
  replicas          2^rep copies of k_linearize's fixed-point camera-sum table in LDS; rep comes from the camera count
                    (satba_problem_create) or SATBA_LIN_REP (0 .. 4)
"""
import functools
import os
import re

import numpy as np

import cases_intrinsics as CI
import cases_tri as CT
from satba import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sat-bundleadjust_amd", "csrc")

# ---------------------------------------------------------------------------------------------------------------------------------
# A. the grids of the five kernels, in waves
#
# k_residual (also its TRIAL form), k_jvp and k_backsub are launched with slice_grid(p, THREADS / 64, 2, sh):
#       workgroups = min(ceil(units / (THREADS / 64)), 256 * 2),    units = n_slices << sh,
# RES_THREADS = JVP_THREADS = BS_THREADS = 512 (satba_kernels.h): 8 waves per workgroup, at most 512 * 8 = 4 096 waves.
# k_linearize is launched with lin_grid_for(p) workgroups of LinCfg<BIG>::THREADS threads,
#       workgroups = min(512, min(ceil(units / LinCfg<false>::WAVES), 256 * (1024 / LinCfg<false>::THREADS))),
# LinCfg<false>::THREADS = SATBA_LIN_THREADS = 1024: at most 256 workgroups of 16 waves = 4 096 waves; the BIG variants (generic
# robust losses, RPC, intrinsics) run the same number of workgroups with 512 threads: at most 2 048 waves.
# for_each_slice gives wave w the units w, w + G, ... of the first half of the list (G waves in all) and with each its mirror image in
# the second half: a second round of that loop runs where ceil(units / 2) > G.
SLICE = 64
SIZE_RULE_UNITS = 3000  # slice_split: `while (sh < 3 && (n_slices << sh) < 3000) ++sh`
SH_MAX = 3
REP_MAX = 4
SLICE_PER_CU = 2        # the per_cu argument of the three slice_grid launches
CUS = 256               # `256 * per_cu`, `256 * (1024 / THREADS)`: one or two workgroups on each of the chip's 256 CUs
LIN_GRID_CAP = 512      # lin_grid_for's std::min(512, ...): d_part holds 512 partial tables


def source_constants():
    """The defaults the derivation above rests on, read from the sources: {"RES_THREADS": 512, ...}."""
    kernels = open(os.path.join(CSRC, "satba_kernels.h")).read()
    capi = open(os.path.join(CSRC, "satba_capi.hip")).read()
    out = {}
    for name in ("RES", "JVP", "BS", "LIN"):
        m = re.search(r"#ifndef SATBA_{0}_THREADS\s*\n\s*#define SATBA_{0}_THREADS (\d+)".format(name), kernels)
        out[name + "_THREADS"] = int(m.group(1))
    m = re.search(r"static constexpr int THREADS = BIG \? (\d+) : SATBA_LIN_THREADS;", kernels)
    out["LIN_THREADS_BIG"] = int(m.group(1))
    out["slice_per_cu"] = sorted(set(int(v) for v in re.findall(r"slice_grid\(p, (?:RES|JVP|BS)_THREADS / 64, (\d+), a\.sh\)", capi)))
    out["slice_launches"] = len(re.findall(r"slice_grid\(p, (?:RES|JVP|BS)_THREADS / 64, \d+, a\.sh\)", capi))
    m = re.search(r"return grid_for\(\(long long\)p->L\.n_slices << sh, waves_per_block, (\d+) \* \(env > 0 \? env : per_cu\)\);", capi)
    out["slice_cus"] = int(m.group(1))
    m = re.search(r"return std::min\((\d+), grid_for\(\(long long\)p->L\.n_slices << slice_split\(p\), LinCfg<false>::WAVES, "
                  r"(\d+) \* \((\d+) / LinCfg<false>::THREADS\)\)\);", capi)
    out["lin_cap"], out["lin_cus"], out["lin_threads_per_cu"] = (int(v) for v in m.groups())
    m = re.search(r"while \(sh < (\d+) && \(\(long long\)p->L\.n_slices << sh\) < (\d+)\) \+\+sh;", capi)
    out["sh_max"], out["size_rule_units"] = int(m.group(1)), int(m.group(2))
    m = re.search(r'getenv\("SATBA_LIN_REP"\)\) p->lin_rep_shift = std::min\((\d+), std::max\(0, atoi\(rs\)\)\);', capi)
    out["rep_max"] = int(m.group(1))
    return out


RES_THREADS = JVP_THREADS = BS_THREADS = 512
LIN_THREADS, LIN_THREADS_BIG = 1024, 512


def n_slices_of(n_pts):
    return (n_pts + SLICE - 1) // SLICE


def slice_grid(n_slices, sh, threads=RES_THREADS):
    """Workgroups of k_residual / k_jvp / k_backsub."""
    units = n_slices << sh
    return max(1, min((units + threads // 64 - 1) // (threads // 64), CUS * SLICE_PER_CU))


def lin_grid(n_slices, sh):
    """Workgroups of k_linearize (info()["lin_grid"])."""
    units, waves = n_slices << sh, LIN_THREADS // 64
    return min(LIN_GRID_CAP, max(1, min((units + waves - 1) // waves, CUS * (1024 // LIN_THREADS))))


def kernel_waves(n_slices, sh, big=False):
    """Waves of every grid: {"residual": .., "jvp": .., "backsub": .., "linearize": ..} (big: the 512-thread k_linearize variants)."""
    out = {name: slice_grid(n_slices, sh, t) * (t // 64) for name, t in (("residual", RES_THREADS), ("jvp", JVP_THREADS), ("backsub", BS_THREADS))}
    out["linearize"] = lin_grid(n_slices, sh) * ((LIN_THREADS_BIG if big else LIN_THREADS) // 64)
    return out


def walk_rounds(units, waves):
    """(rounds of for_each_slice's stride loop, iterations of the last round) for `units` units on `waves` waves."""
    half = (units + 1) // 2
    rounds = (half + waves - 1) // waves
    return rounds, half - (rounds - 1) * waves


def size_rule(n_slices, unit_run=True, deterministic=False, override=None):
    """slice_split() restated."""
    if override is not None and override >= 0:
        return min(override, SH_MAX)
    if deterministic:
        return 0
    sh = 0
    while sh < SH_MAX and (n_slices << sh) < SIZE_RULE_UNITS:
        sh += 1
    return sh if unit_run else max(sh, 1)


def rep_rule(n_cam, n_p):
    """lin_rep_shift of satba_problem_create restated: doubled while the rows stay <= 1 024 and the table with the camera constants
    <= 140 KB.  The table has cam_sum_stride(n_p) = (3 n_p) | 1 eight-byte slots per row (satba_kernels.h), rounded up to 16 bytes in
    all; the constants are CAMC = 26 doubles per camera (satba_models.h)."""
    def table(rows):
        return (rows * ((3 * n_p) | 1) * 8 + 15) & ~15

    rep = 0
    while rep < REP_MAX and (n_cam << (rep + 1)) <= 1024 and table(n_cam << (rep + 1)) + 8 * 26 * n_cam <= 140 * 1024:
        rep += 1
    return rep


# ---------------------------------------------------------------------------------------------------------------------------------
# B. MIXED: 12 cameras x 190 points, about 5 observations per point
#
# 190 points are three slices (odd: the unpaired middle unit of for_each_slice at sh = 0), the last one with 62 points (lanes without
# a point).  The seeds are the first per model whose track lengths hold what test_lanes_cases_host.py asserts: 2 and 3 (fewer
# observations than lanes at sh = 2), a length that is no multiple of 4 and one >= 9.
#
# Every family runs on synth's defaults: 12 px of initial error.  Two things follow from that size.
#
# huber at f_scale = 1.3 clamps 1 747 of the 1 928 Jacobian rows to sqrt(eps) of their weight (rho' + 2 rho'' z = 0 for z > 1), every
# row of 66 points and of five free cameras.  The diag U_c terms of those cameras lie 2^-52 below the largest possible term of their slot,
# under the unit of the fixed-point camera sums: k_linearize's route returned diag U_c = 0 for them -- an x_scale of 1 in the prepare
# phase where float64 has 1e-7 (|g_h|^2 = 3.896e18 against 1.2835e19, from a start moved by 1e-6 |x|) -- until k_lin_finish learnt to raise the header's FX slot for a
# free camera whose slot sums to less than its number of terms.  The caller then repeats the linearisation on the camera-major sums,
# as it does for a term above the range: FALLS_BACK names the families that do, and the GPU tests hold them to float64 after it.
#
# The trial point of _run_phases for soft_l1 lies 8e-4 |x| (affine) and 8e-3 |x| (perspective) away, at 100 and 160 times the cost.
# x_new = x + step is held to 1e-12 |x| while the vectors the step is made of are held to 1e-7 and 1e-8: consistent for steps below
# 1e-5 |x| only (measured at 12 px, perspective: x_new 3.2 .. 3.3e-12 at sh = 0 .. 3 with gn_h at 3.7e-10 and q1 at 6.5e-11 of their
# bounds' 1e-7 and 1e-8; affine: 2.2e-13).  The phase test therefore runs the families of NEAR_IN_PHASES on the NEAR variant of the
# scene, 1.2 px and 0.3 m from the truth, where the steps are 1e-7 and 9e-7 |x| (test_lanes_cases_host.py); every other test of those
# families runs at 12 px.
MIXED_CAMS, MIXED_PTS, MIXED_OPP = 12, 190, 5
MIXED_SEEDS = {"affine": 1, "perspective": 1, "rpc": 1}
NEAR_KW = {"sigma_theta": 1e-7, "pts_noise_m": 0.3}
MIXED_FIX = {"n_cam_fix": 2, "n_pts_fix": 9}  # the variant with frozen cameras and points

# name -> (model, options, loss, f_scale, rpc_f32, unit-weight run, 512-thread k_linearize)
FAMILIES = {
    "affine_RT": ("affine", {"correction_params": ["R", "T"]}, "linear", 1.0, True, True, False),
    "affine_R": ("affine", {"correction_params": ["R"]}, "linear", 1.0, True, True, False),
    "affine_RT_weighted": ("affine", {"correction_params": ["R", "T"], "ref_cam_weight": 2.5}, "linear", 1.0, True, False, False),
    "affine_RT_soft_l1": ("affine", {"correction_params": ["R", "T"]}, "soft_l1", 1.0, True, False, False),
    "affine_RT_huber": ("affine", {"correction_params": ["R", "T"]}, "huber", 1.3, True, False, True),
    "persp_RT": ("perspective", {"correction_params": ["R", "T"]}, "linear", 1.0, True, True, False),
    "persp_RT_soft_l1": ("perspective", {"correction_params": ["R", "T"]}, "soft_l1", 1.0, True, False, False),
    "rpc_R": ("rpc", {"correction_params": ["R"]}, "linear", 1.0, False, True, True),
    "affine_RTK": ("affine", {"correction_params": CI.RTK, "K_init": "camera"}, "linear", 1.0, True, True, True),
}
PHASES_ONLY_TO_PREPARE = ("affine_RT_huber",)  # tools/fuzz_solve.py: huber / cauchy past the Jacobian are reported, not asserted
REPLICA_FAMILIES = ("affine_RT", "affine_RT_soft_l1")
FALLS_BACK = ("affine_RT_huber",)
NEAR_IN_PHASES = ("affine_RT_soft_l1", "persp_RT_soft_l1")


@functools.lru_cache(maxsize=None)
def mixed_scene(model, near=False):
    return synth.make_scene(model, MIXED_CAMS, MIXED_PTS, MIXED_OPP, seed=MIXED_SEEDS[model], **(NEAR_KW if near else {}))


def family_params(name, fixed=False, near=False):
    """(params, start vector) of a family on MIXED (near: its NEAR variant); fixed: MIXED_FIX instead of one frozen camera."""
    from satba import ba_core

    model, opts = FAMILIES[name][:2]
    d = dict(opts, reduce=False, **(MIXED_FIX if fixed else {"n_cam_fix": 1}))
    p = synth.make_params(mixed_scene(model, near), d)
    return p, ba_core._frozen_vars(p.params_opt.copy(), p)


# ---------------------------------------------------------------------------------------------------------------------------------
# C. LONG: tracks longer than a wavefront, 90 cameras (three replicas by the rule)
LONG_ARGS = (90, 40, 80)
LONG_SEED = 5


def long_scene():
    return synth.make_affine_scene(*LONG_ARGS, seed=LONG_SEED)


# ---------------------------------------------------------------------------------------------------------------------------------
# D. ROUNDS: a second round of for_each_slice at eight lanes per point
#
# By section A every grid is capped at 4 096 waves (k_linearize<BIG>: 2 048), so at sh = 3 the second round starts where
# ceil(8 n_slices / 2) > 4 096: n_slices > 1 024.  61 copies of a 17-slice scene are 1 037 slices, 8 296 units, 4 148 iterations: a
# first round of 4 096 and a second of 52, fewer than there are waves.  The copies share cameras and observations, so every point
# of a copy has the inputs of its original; the handle sorts the points by track length, which spreads each copy over the slice list.
ROUNDS_CAMS, ROUNDS_BASE_PTS, ROUNDS_OPP, ROUNDS_SEED = 6, 1088, 4, 7
ROUNDS_TILES = 61
ROUNDS_SH = 3


def rounds_base_scene():
    return synth.make_affine_scene(ROUNDS_CAMS, ROUNDS_BASE_PTS, ROUNDS_OPP, seed=ROUNDS_SEED)


def tiled_scene(scene, reps):
    """`reps` copies of the scene's points (and of their initial values), one after the other, seen by the same cameras."""
    pts_ind, cam_ind, pts2d, n_pts = CT.tile_observations(scene, reps)
    d = dict(scene.__dict__, n_pts=n_pts, pts3d=np.tile(scene.pts3d, (reps, 1)), pts3d_true=np.tile(scene.pts3d_true, (reps, 1)),
             pts_ind=pts_ind, cam_ind=cam_ind, pts2d=pts2d)
    return synth.Scene(**d)


# ---------------------------------------------------------------------------------------------------------------------------------
# E. the size rule: the smallest scene that runs at four lanes per point (n_slices << 2 >= 3000: 750 slices)
RULE_SLICES = 750
RULE_PTS = (RULE_SLICES - 1) * SLICE + 1  # 47 937 points: the 750th slice holds one point
RULE_CAMS, RULE_OPP, RULE_SEED = 4, 2, 3


def rule_scene(n_pts=RULE_PTS):
    return synth.make_affine_scene(RULE_CAMS, n_pts, RULE_OPP, seed=RULE_SEED)


# ---------------------------------------------------------------------------------------------------------------------------------
# F. a camera step that is the same doubles on two handles
#
# The back-substitution takes dc from the dense solve, which works in scaled variables: with S = diag(s_i * s_i) and right-hand side r
# the scaled system is the identity (s_i * s_i is rounded once on both sides) and dc_i = fl(fl(r_i / s_i) / s_i).  Two handles with
# different camera scales s get the same dc only for chosen r: exact_rhs searches the doubles around d s^2 for one that lands on d, and
# moves d by an ulp where a handle has none.
def step_of(r, s):
    return (r / s) / s


def exact_rhs(d, scales, span=12, moves=64):
    """(d', [r per scale vector]) with step_of(r_k, scales_k) == d' bit for bit; d' is d moved by at most `moves` ulps."""
    d = np.array(d, dtype=np.float64)
    out = [np.zeros_like(d) for _ in scales]
    todo = np.ones(d.size, dtype=bool)
    for _ in range(moves):
        found = np.ones(d.size, dtype=bool)
        for k, s in enumerate(scales):
            r = d * s * s
            lo = r.copy()
            for _ in range(span):
                lo = np.nextafter(lo, -np.inf * np.sign(r))
            hit = np.zeros(d.size, dtype=bool)
            c = lo
            for _ in range(2 * span + 1):
                ok = (step_of(c, s) == d) & ~hit & todo
                out[k][ok] = c[ok]
                hit |= ok
                c = np.nextafter(c, np.inf * np.sign(r))
            found &= hit | ~todo
        todo &= ~found
        if not todo.any():
            return d, out
        d[todo] = np.nextafter(d[todo], np.inf)
    raise AssertionError("no exact right-hand side within {} ulps".format(moves))

"""
The scenarios of tests/cases_lanes.py on the CPU: each scene is what tests/test_gpu_lanes.py takes it for -- conditions on the inputs,
so that a GPU test cannot pass vacuously -- and the wave counts its second-round scene rests on follow from the constants in the
sources.
"""
import numpy as np
import pytest

import cases_lanes as CL
from oracle import lm_oracle as L
from satba import trf


def test_restated_grids_use_the_constants_of_the_sources():
    c = CL.source_constants()
    assert (c["RES_THREADS"], c["JVP_THREADS"], c["BS_THREADS"]) == (CL.RES_THREADS, CL.JVP_THREADS, CL.BS_THREADS) == (512, 512, 512)
    assert (c["LIN_THREADS"], c["LIN_THREADS_BIG"]) == (CL.LIN_THREADS, CL.LIN_THREADS_BIG) == (1024, 512)
    # k_residual, its TRIAL form, k_backsub and k_jvp: the same two workgroups per CU
    assert c["slice_launches"] == 4 and c["slice_per_cu"] == [CL.SLICE_PER_CU] and c["slice_cus"] == CL.CUS == 256
    assert (c["lin_cap"], c["lin_cus"], c["lin_threads_per_cu"]) == (CL.LIN_GRID_CAP, CL.CUS, 1024)
    assert (c["sh_max"], c["size_rule_units"], c["rep_max"]) == (CL.SH_MAX, CL.SIZE_RULE_UNITS, CL.REP_MAX) == (3, 3000, 4)
    # every capped grid is 4 096 waves, the 512-thread k_linearize variants 2 048
    big = 10 ** 6
    assert CL.kernel_waves(big, 0) == {"residual": 4096, "jvp": 4096, "backsub": 4096, "linearize": 4096}
    assert CL.kernel_waves(big, 0, big=True)["linearize"] == 2048
    assert CL.slice_grid(big, 0) == 512 and CL.lin_grid(big, 0) == 256
    # small problems: one wave per unit, rounded up to workgroups
    assert CL.slice_grid(3, 0) == 1 and CL.slice_grid(3, 3) == 3 and CL.lin_grid(3, 3) == 2 and CL.lin_grid(3, 0) == 1


def test_rules_restated():
    # the replica counts the suite's camera counts get (12 | 90 | 200 | 700 cameras)
    assert [CL.rep_rule(m, n) for m, n in ((12, 5), (12, 3), (12, 8), (7, 5), (90, 5), (200, 5), (700, 3))] == [4, 4, 4, 4, 3, 2, 0]
    assert CL.rep_rule(64, 5) == 4 and CL.rep_rule(65, 5) == 3  # 1 024 rows
    # lanes per point: eight below 750 slices (48 000 points), four below 1 500, two below 3 000
    assert [CL.size_rule(n) for n in (1, 749, 750, 1499, 1500, 2999, 3000, 10 ** 5)] == [3, 3, 2, 2, 1, 1, 0, 0]
    assert CL.size_rule(3000, unit_run=False) == 1 and CL.size_rule(750, unit_run=False) == 2
    assert CL.size_rule(3, deterministic=True) == 0 and CL.size_rule(3, deterministic=True, unit_run=False) == 0
    assert CL.size_rule(10 ** 5, override=2) == 2 and CL.size_rule(3, deterministic=True, override=7) == 3
    assert CL.size_rule(3, override=-1) == 3
    # the shapes bench.py times: 1 M points linear / soft_l1, 100 k points
    assert CL.size_rule(CL.n_slices_of(10 ** 6)) == 0 and CL.size_rule(CL.n_slices_of(10 ** 6), unit_run=False) == 1
    assert CL.size_rule(CL.n_slices_of(10 ** 5)) == 1 and CL.rep_rule(200, 5) == 2


@pytest.mark.parametrize("model", sorted(CL.MIXED_SEEDS))
def test_mixed_scene(model):
    scene = CL.mixed_scene(model)
    assert (scene.n_cam, scene.n_pts) == (12, 190) and scene.cam_model == model
    cnt = np.bincount(scene.pts_ind, minlength=scene.n_pts)
    assert cnt.min() == 2 and 3 in cnt           # fewer observations than the four lanes of sh = 2 (and the eight of sh = 3)
    assert np.any(cnt % 4 != 0) and cnt.max() >= 9   # a last iteration with idle lanes; more than one iteration at sh = 3
    assert scene.n_pts % 64 == 62                # the last slice has lanes without a point
    n_slices = CL.n_slices_of(scene.n_pts)
    assert n_slices == 3                         # odd: the middle unit of the walk at sh = 0 has no mirror image
    for sh in range(4):
        units = n_slices << sh
        assert CL.walk_rounds(units, CL.kernel_waves(n_slices, sh)["residual"])[0] == 1
        assert CL.size_rule(n_slices, override=sh) == sh
    assert CL.size_rule(n_slices) == 3 and CL.rep_rule(12, 5) == 4   # what the suite runs without the switches
    key = scene.pts_ind.astype(np.int64) * scene.n_cam + scene.cam_ind
    assert np.all(np.diff(key) > 0)              # point-major, cameras ascending


@pytest.mark.parametrize("name", sorted(CL.FAMILIES))
@pytest.mark.parametrize("fixed", [False, True])
def test_families(name, fixed):
    model, opts, loss, f_scale, rpc_f32, unit, big = CL.FAMILIES[name]
    p, v = CL.family_params(name, fixed=fixed)
    assert p.cam_model == model and p.n_params == {"affine_R": 3, "rpc_R": 3, "affine_RTK": 8}.get(name, 5 if model == "affine" else 6)
    assert (p.n_cam_fix, p.n_pts_fix) == ((2, 9) if fixed else (1, 0))
    assert loss in L.LOSSES and (loss == "linear" or not unit)
    assert bool(np.all(p.pts2d_w == 1.0)) == (name != "affine_RT_weighted")
    assert unit == (loss == "linear" and bool(np.all(p.pts2d_w == 1.0)))
    if name == "affine_RT_weighted":
        assert set(np.unique(p.pts2d_w)) == {1.0, 2.5}
    assert big == (loss not in ("linear", "soft_l1") or model == "rpc" or p.n_params > 6)  # LinCfg's choice
    assert v.shape == p.params_opt.shape and np.all(np.isfinite(v))
    n_c = p.n_cam * p.n_params
    assert np.array_equal(v[n_c:], p.params_opt[n_c:]) and np.array_equal(v[: p.n_cam_fix * p.n_params], p.cam_params[: p.n_cam_fix, : p.n_params].ravel())
    assert name not in CL.PHASES_ONLY_TO_PREPARE or loss == "huber"
    assert all(CL.FAMILIES[r][0] == "affine" for r in CL.REPLICA_FAMILIES)


def test_huber_family_has_cameras_with_clamped_rows_only():
    """What the fall-back from the fixed-point camera sums needs of the scene (cases_lanes.py section B): free cameras all of whose
    rows huber clamps to sqrt(eps), whose diag U_c is then 2^-52 of the slot's largest term -- and rows on the other branch too."""
    loss, f_scale = CL.FAMILIES["affine_RT_huber"][2:4]
    assert (loss, f_scale) == ("huber", 1.3) and CL.FALLS_BACK == ("affine_RT_huber",)
    p, v = CL.family_params("affine_RT_huber")
    f, _, _, Jc, _ = L.weighted_system(v, p, loss, f_scale)
    out = (np.abs(f) > f_scale).reshape(-1, 2)
    whole_pts = sum(bool(out[p.pts_ind == i].all()) for i in range(p.n_pts))
    whole_cams = [c for c in range(p.n_cam_fix, p.n_cam) if out[p.cam_ind == c].all()]
    print("clamped rows {} of {}, whole points {}, whole cameras {}".format(out.sum(), out.size, whole_pts, whole_cams))
    assert 1700 < out.sum() < out.size - 100 and whole_pts > 50 and len(whole_cams) >= 1
    U = np.zeros((p.n_cam, p.n_params))
    np.add.at(U, p.cam_ind, np.einsum("kri,kri->ki", Jc, Jc))
    assert 0 < U[whole_cams].max() < 2.0 ** -40 * U.max()  # far below the unit of a scale that holds the largest term in 50 bits


@pytest.mark.parametrize("name", CL.NEAR_IN_PHASES)
def test_soft_l1_trial_steps_are_small_enough_for_the_bound_on_x_new(name):
    """x_new is held to 1e-12 |x|, the vectors it is made of to 1e-7 and 1e-8: consistent for steps below 1e-5 |x| -- on the NEAR
    variant of the scene, not on the scene itself."""
    from test_gpu_parity import _run_phases

    def step(near):
        p, v = CL.family_params(name, near=near)
        ora = L.OracleEngine(p)
        ora.configure("soft_l1", 1.0)
        ora.set_x(v)
        out = _run_phases(ora, 1e-3)
        return np.abs(ora.x_new - v).max() / np.abs(v).max(), out["trial"][trf.COST_NEW] / out["lin"][trf.COST]

    (s, c), (s0, c0) = step(True), step(False)
    print("{}: step {:.2e} |x|, cost x {:.2f}; at synth's noise {:.2e} |x|, cost x {:.1f}".format(name, s, c, s0, c0))
    assert s < 1e-5 and c < 1.0 and s0 > 1e-4 and c0 > 10.0


def test_long_scene():
    scene = CL.long_scene()
    cnt = np.bincount(scene.pts_ind)
    assert (scene.n_cam, scene.n_pts) == (90, 40) and cnt.max() > 64 and cnt.min() > 8
    assert CL.rep_rule(90, 5) == 3 and CL.n_slices_of(40) == 1


def test_rounds_scene_needs_a_second_round_at_eight_lanes():
    base = CL.rounds_base_scene()
    assert base.n_pts == CL.ROUNDS_BASE_PTS == 17 * 64 and base.n_cam * 5 <= 63  # (the reduced system of one launch: k_solve_small)
    n_slices = CL.n_slices_of(base.n_pts * CL.ROUNDS_TILES)
    assert n_slices == 17 * 61 == 1037
    units = n_slices << CL.ROUNDS_SH
    waves = CL.kernel_waves(n_slices, CL.ROUNDS_SH)
    assert waves == {"residual": 4096, "jvp": 4096, "backsub": 4096, "linearize": 4096} and CL.lin_grid(n_slices, CL.ROUNDS_SH) == 256
    for name, w in waves.items():
        assert units > 2 * w and CL.walk_rounds(units, w) == (2, 52), name  # the second round carries fewer units than there are waves
    # ... and the base scene alone does not reach it
    assert CL.walk_rounds(17 << 3, CL.kernel_waves(17, 3)["residual"])[0] == 1
    tiled = CL.tiled_scene(base, 3)
    assert tiled.n_pts == 3 * base.n_pts and tiled.n_obs == 3 * base.n_obs and np.all(np.diff(tiled.pts_ind) >= 0)
    for r in range(3):
        o = slice(r * base.n_obs, (r + 1) * base.n_obs)
        assert np.array_equal(tiled.pts_ind[o] - r * base.n_pts, base.pts_ind) and np.array_equal(tiled.cam_ind[o], base.cam_ind)
        assert np.array_equal(tiled.pts2d[o], base.pts2d)
        assert np.array_equal(tiled.pts3d[r * base.n_pts: (r + 1) * base.n_pts], base.pts3d)
    assert tiled.cameras is base.cameras
    cnt = np.bincount(base.pts_ind)
    assert len(set(cnt)) >= 4 and cnt.min() == 2  # mixed lengths: sorted by length, the copies interleave in the slice list


def test_rule_scene_sits_on_the_threshold():
    assert CL.RULE_PTS == 47937 and CL.n_slices_of(CL.RULE_PTS) == 750 and CL.n_slices_of(CL.RULE_PTS - 1) == 749
    assert CL.size_rule(750) == 2 and CL.size_rule(749) == 3 and 750 << 2 == 3000
    scene = CL.rule_scene(200)
    assert scene.n_cam == CL.RULE_CAMS and np.bincount(scene.pts_ind).min() >= 2


def test_exact_rhs_lands_on_the_same_step():
    rng = np.random.default_rng(3)
    d0 = 1e-6 * rng.standard_normal(30)
    s1 = rng.uniform(1.0, 300.0, 30)
    s2 = s1 * np.sqrt(61.0) * (1 + 1e-13 * rng.standard_normal(30))
    d, (r1, r2) = CL.exact_rhs(d0, [s1, s2])
    assert np.array_equal(CL.step_of(r1, s1), d) and np.array_equal(CL.step_of(r2, s2), d)
    assert np.abs(d - d0).max() <= 64 * np.spacing(np.abs(d0).max()) and np.all(d != 0)
    assert not np.array_equal(CL.step_of(d0 * s1 * s1, s1), CL.step_of(d0 * s2 * s2, s2))  # the plain product does not

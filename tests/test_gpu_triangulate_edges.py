"""
The initial triangulation where its kernels change path (scenarios: tests/cases_tri.py, checked on the CPU by
tests/test_triangulate_cases_host.py; the pair and mean logic at ordinary shapes: tests/test_gpu_triangulate.py).

A  the three homes of the RPC tables in tri_run (csrc/satba_triangulate_api.inc): 48 KB of dynamic LDS, dynamic LDS above that
   after raising the kernel's limit, global memory -- 12 | 67 || 68 | 196 || 197 | 230 cameras (derivation: cases_tri.py, section A)
B  a second round of k_tri_points' grid-stride loop: more than 256 * 64 * 256 triangulations
C  the linear triangulation against numpy.longdouble at view separations from 0.3 rad down to 3e-5 rad
D  satba_init_pts3d_resident on tracks of up to 70 observations (a hundred refills of k_tri_list's sorted buffer) and on track
   lists of 1 and 64 n +- 1 tracks (the tails of the grids and of the handle's slices of 64 tracks)
"""
import functools

import numpy as np
import pytest

import cases_tri as CT
from oracle import triangulate_oracle as T
from satba import ft_triangulate as FT
from satba import synth
from test_gpu_triangulate import _assert_f32_close

pytestmark = pytest.mark.gpu


def _upload(scene, pairs):
    return FT.init_pts3d_from_observations(scene.pts_ind, scene.cam_ind, scene.pts2d, scene.n_pts, scene.cameras, scene.cam_model, pairs,
                                           return_info=True)


def _against_the_oracle(scene, pairs, got):
    """What test_running_mean_is_bit_exact asserts: the oracle's pair loop fed with the device's own pairwise triangulations gives
    the device's means bit for bit; the pairwise triangulations are the oracle's float64 chain at that file's tolerances; and the
    means are the oracle's own up to the float32 entries that sit on a rounding boundary.  Returns the means of the device-fed loop
    (the caller asserts equality)."""
    C = scene.to_dense_C()
    rpc = scene.cam_model == "rpc"
    chain, worst = {}, {"pts": 0.0, "err": 0.0}

    def dev_pair(c_i, c_j, oi, oj):
        if rpc:
            got_p, got_e = FT.rpc_triangulation(scene.cameras[c_i], scene.cameras[c_j], oi, oj)
            want_p, want_e = T.rpc_triangulation(scene.cameras[c_i], scene.cameras[c_j], oi, oj)
            worst["err"] = max(worst["err"], np.abs(got_e[:, 0] - want_e).max())
        else:
            got_p = FT.linear_triangulation_multiple_pts(scene.cameras[c_i], scene.cameras[c_j], oi, oj)
            want_p = T.linear_triangulation_multiple_pts(scene.cameras[c_i], scene.cameras[c_j], oi, oj)
        worst["pts"] = max(worst["pts"], np.abs(got_p - want_p).max())
        chain[(c_i, c_j)] = want_p
        return got_p
    fed = T.init_pts3d(C, scene.cameras, scene.cam_model, pairs, triangulate=dev_pair)
    own = T.init_pts3d(C, scene.cameras, scene.cam_model, pairs, triangulate=lambda c_i, c_j, oi, oj: chain[(c_i, c_j)])
    print("  pairwise: device - oracle {:.3g} m, {:.3g} px; means: {} of {} entries differ from the device-fed loop, {} from the oracle's"
          .format(worst["pts"], worst["err"], np.count_nonzero(got != fed), got.size, np.count_nonzero(got != own)))
    assert worst["pts"] < (1e-4 if rpc else 1e-6) and worst["err"] < 1e-5
    _assert_f32_close(got, own)
    return fed


# ------------------------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("M", CT.PLACEMENT_M)
def test_rpc_tables_in_each_of_their_homes(gpu, M):
    """120 tracks seen by all M cameras, 60 pairs that name the first and the last camera: the means are those of the oracle's loop
    fed with the device's pairwise triangulations (k_tri_pairwise: two tables in static LDS, whatever M is), bit for bit, in each of
    the three homes of the table -- the staging loop, the opt-in launch and the rows of the global table."""
    scene = CT.full_scene("rpc", M, CT.PLACEMENT_TRACKS, seed=23)
    pairs = CT.placement_pairs(M)
    got, info = _upload(scene, pairs)
    print("\nM = {} ({}), {} pairs, {} triangulations".format(M, CT.rpc_table_home(M), len(pairs), info["n_tri"].sum()))
    assert np.array_equal(info["n_tri"], CT.n_tri_reference(scene.pts_ind, scene.cam_ind, scene.n_pts, M, pairs))
    assert info["n_tri"].sum() == len(pairs) * CT.PLACEMENT_TRACKS
    fed = _against_the_oracle(scene, pairs, got)
    assert np.array_equal(got, fed)


# ------------------------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("model", list(CT.ROUNDS))
def test_second_round_of_the_grid_stride_loop(gpu, model):
    """293 tracks seen by 8 cameras, tiled until there are more triangulations than one round of k_tri_points' capped grid takes:
    every tile is the base run, bit for bit; the base run is checked like the runs of test_gpu_triangulate.py."""
    scene = CT.full_scene(model, CT.ROUNDS_CAMS, CT.ROUNDS_TRACKS, seed=29)
    pairs = CT.rounds_pairs(model)
    base, info_b = _upload(scene, pairs)
    assert np.array_equal(base, _against_the_oracle(scene, pairs, base))
    assert np.array_equal(info_b["n_tri"], np.full(scene.n_pts, len(pairs)))
    reps = CT.ROUNDS[model]
    pts_ind, cam_ind, pts2d, n_pts = CT.tile_observations(scene, reps)
    got, info = FT.init_pts3d_from_observations(pts_ind, cam_ind, pts2d, n_pts, scene.cameras, model, pairs, return_info=True)
    E = int(info["n_tri"].sum(dtype=np.int64))
    print("\n{}: {} tiles, E = {} triangulations ({} in the second round), {:.1f} ms".format(model, reps, E, E - CT.GRID_ROUND, info["kernel_ms"]))
    assert CT.GRID_ROUND < E <= 2 * CT.GRID_ROUND
    assert np.array_equal(info["n_tri"].reshape(reps, -1), np.broadcast_to(info_b["n_tri"], (reps, scene.n_pts)))
    tiles = got.reshape(reps, scene.n_pts, 3)
    bad = np.nonzero((tiles != base[None]).any(axis=(1, 2)))[0]
    assert bad.size == 0, "tiles {} ... differ from the base run".format(bad[:5])


# ------------------------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("model,delta,noise", CT.LINEAR_CLASSES)
def test_linear_triangulation_against_extended_precision(gpu, model, delta, noise):
    """100 points seen by two views `delta` rad apart: the device's points are as close to the null vector computed in
    numpy.longdouble as the float64 restatement of the same one-sided Jacobi method is, up to a factor 4 (two roundings of one
    backward-stable method: fused multiply-adds, rsqrt, the maximum over 100 samples) and never asked below 1e-9 m.  Cutting
    the sweeps to three misses it by factors of 1e3 to 1e7 at 0.3 and 3e-2 rad (tried); a Jacobi threshold of 1e-12 does not change a
    digit of any class (tried: the convergence is quadratic, the sweep that gets below 1e-12 ends far below 1e-16), so the threshold
    is not pinned by this test.
    Measured on an MI355X: device error / restatement error between 0.38 and 1.74 over the twenty classes (largest: affine,
    delta = 3e-4 rad, 0.3 px)."""
    P1, P2, a, b = CT.linear_class(model, delta, noise)
    ref = CT.triangulate_ld(P1, P2, a, b)
    restated = CT.restatement_error(P1, P2, a, b, ref)
    dev = CT.error_m(FT.linear_triangulation_multiple_pts(P1, P2, a, b), ref).max()
    print("\n{} delta {:g} noise {:g}: device {:.3g} m, float64 restatement {:.3g} m, ratio {:.2f}".format(model, delta, noise, dev, restated, dev / restated))
    assert restated <= 1e-8 / delta  # (the host test's law: the bound below is not a loose one)
    assert dev <= max(4.0 * restated, 1e-9)


# ------------------------------------------------------------------------------------------------------------------ D
def _params(scene):
    return synth.make_params(scene, {"correction_params": ["R"], "n_cam_fix": 1})


@pytest.mark.parametrize("general", [False, True])
def test_resident_triangulation_of_long_tracks(gpu, general, monkeypatch):
    """Tracks of 2 to 70 observations in one handle: the resident path walks the sliced layout to slot 69 and is the upload path bit
    for bit, without a mask and with a third of the observations removed; the counts are the reference loop's, and a sample of the
    upload path's rows (the hand-built tracks among them) is the oracle's."""
    scene = CT.long_track_scene()
    p = _params(scene)
    pairs = CT.long_pairs(general)
    if general:
        monkeypatch.setenv("SATBA_TRI_GENERAL", "1")
    up, info_u = _upload(scene, pairs)
    res, info_r = FT.init_pts3d_resident(p, pairs, return_info=True)
    print("\ngeneral = {}: {} pairs, up to {} triangulations on a track, upload {:.1f} ms, resident {:.1f} ms"
          .format(general, len(pairs), info_u["n_tri"].max(), info_u["kernel_ms"], info_r["kernel_ms"]))
    assert np.array_equal(info_u["n_tri"], CT.n_tri_reference(scene.pts_ind, scene.cam_ind, scene.n_pts, CT.LONG_CAMS, pairs))
    assert info_u["n_tri"][0] == len(pairs) and info_u["n_tri"][1] <= 3  # all 70 cameras: every listed pair; two cameras: one pair at most, however often listed
    assert np.array_equal(res, up) and np.array_equal(info_r["n_tri"], info_u["n_tri"])
    tracks = list(range(5)) + list(range(5, scene.n_pts, 20))
    _assert_f32_close(up[tracks], CT.batched_oracle(scene, pairs, tracks))
    remove = np.random.default_rng(5).random(p.n_obs) < 0.33
    keep = ~remove
    up, info_u = FT.init_pts3d_from_observations(p.pts_ind[keep], p.cam_ind[keep], p.pts2d[keep], p.n_pts, p.cameras, "affine", pairs, return_info=True)
    res, info_r = FT.init_pts3d_resident(p, pairs, remove=remove, return_info=True)
    assert np.array_equal(info_u["n_tri"], CT.n_tri_reference(p.pts_ind[keep], p.cam_ind[keep], p.n_pts, CT.LONG_CAMS, pairs))
    assert np.array_equal(res, up) and np.array_equal(info_r["n_tri"], info_u["n_tri"]) and info_u["n_tri"].max() > 24 * 24


@functools.lru_cache(maxsize=None)
def _prefix_full_run(general):
    scene = CT.long_track_scene(CT.PREFIX_BASE)
    pairs = CT.long_pairs(general, n=240 if general else None)
    full, info = _upload(scene, pairs)
    assert np.array_equal(info["n_tri"], CT.n_tri_reference(scene.pts_ind, scene.cam_ind, scene.n_pts, CT.LONG_CAMS, pairs))
    assert info["n_tri"][0] == len(pairs)
    return scene, pairs, (full, info)


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("N", CT.PREFIX_N)
def test_a_prefix_of_the_tracks_gives_a_prefix_of_the_points(gpu, N, general):
    """The first N tracks alone give the first N rows of the run on all 300, through the upload path and through a handle built from
    those N tracks: the last workgroups of k_tri_count, k_tri_list_ordered / k_tri_list (128 threads; general) and k_tri_mean and the
    last slice of the handle are partly filled at N = 1 and 64 n +- 1.  (The first track names all 70 cameras.)"""
    scene, pairs, (full, info) = _prefix_full_run(general)
    pre = CT.prefix_scene(scene, N)
    up, info_u = _upload(pre, pairs)
    assert up.shape == (N, 3) and np.array_equal(up, full[:N]) and np.array_equal(info_u["n_tri"], info["n_tri"][:N])
    res, info_r = FT.init_pts3d_resident(_params(pre), pairs, return_info=True)
    assert np.array_equal(res, full[:N]) and np.array_equal(info_r["n_tri"], info["n_tri"][:N])
    assert np.all((np.abs(up).max(axis=1) > 1e5) == (info_u["n_tri"] > 0)) and info_u["n_tri"][0] > 0

"""
The scenarios of tests/cases_tri.py on the CPU: each construction is what tests/test_gpu_triangulate_edges.py takes it for -- conditions
on the inputs, so that a GPU test cannot pass vacuously -- and the extended-precision triangulation is a yardstick: finer than
float64, equal to its scalar form, and telling the float64 Jacobi restatement from a bidiagonalising SVD.
"""
import numpy as np
import pytest

import cases_tri as CT
from oracle import triangulate_oracle as T


def test_rpc_table_homes_change_where_the_constants_say():
    """67 | 68 and 196 | 197: the camera counts on both sides of the two thresholds of tri_run, from its constants."""
    assert [CT.rpc_table_home(M) for M in CT.PLACEMENT_M] == ["lds", "lds", "lds_optin", "lds_optin", "global", "global"]
    assert 67 * 728 <= 48 * 1024 < 68 * 728 and 196 * 728 <= 160 * 1024 - 20 * 1024 < 197 * 728 and CT.TRI_RPC_STRIDE * 8 == 728
    # a device that only grants 64 KB keeps 61 cameras in LDS (61 * 728 = 44 408 <= 45 056 < 62 * 728)
    assert CT.rpc_table_home(61, 64 * 1024) == "lds" and CT.rpc_table_home(62, 64 * 1024) == "global"


@pytest.mark.parametrize("M", CT.PLACEMENT_M)
def test_placement_pairs(M):
    pairs = CT.placement_pairs(M)
    assert len(pairs) == (36 if M == 12 else CT.PLACEMENT_PAIRS) and pairs == sorted(set(pairs))
    assert all(0 <= i < j < M and (i + j) % 2 == 1 for i, j in pairs)
    assert (0, 1) in pairs and (M - 2, M - 1) in pairs and ((0, M - 1) in pairs or (1, M - 1) in pairs)
    assert pairs == CT.placement_pairs(M)


def test_full_scene_and_the_reference_count():
    scene = CT.full_scene("rpc", 68, 7, seed=4)
    assert np.array_equal(np.bincount(scene.pts_ind), np.full(7, 68)) and not np.isnan(scene.to_dense_C()).any()
    pairs = CT.placement_pairs(68)
    assert np.array_equal(CT.n_tri_reference(scene.pts_ind, scene.cam_ind, 7, 68, pairs), np.full(7, 60))
    # a missing observation takes the track out of the pairs of its camera, a pair naming a missing camera counts nothing
    keep = ~((scene.pts_ind == 3) & (scene.cam_ind == 0))
    n = CT.n_tri_reference(scene.pts_ind[keep], scene.cam_ind[keep], 7, 68, pairs + [(1, 70)])
    assert n[3] == 60 - sum(1 for i, j in pairs if i == 0) < 60 and np.all(np.delete(n, 3) == 60)


@pytest.mark.parametrize("model", list(CT.ROUNDS))
def test_tiled_scene_needs_a_second_grid_round(model):
    pairs = CT.rounds_pairs(model)
    assert len(pairs) == {"affine": 28, "rpc": 16}[model] and pairs == sorted(pairs)
    E = len(pairs) * CT.ROUNDS_TRACKS * CT.ROUNDS[model]
    assert CT.GRID_ROUND == 4194304 < E <= 2 * CT.GRID_ROUND
    assert CT.GRID_ROUND % (len(pairs) * CT.ROUNDS_TRACKS) != 0  # the first round ends inside a tile
    scene = CT.full_scene("affine", CT.ROUNDS_CAMS, CT.ROUNDS_TRACKS, seed=6)
    pts_ind, cam_ind, pts2d, n_pts = CT.tile_observations(scene, 3)
    assert n_pts == 3 * 293 and np.all(np.diff(pts_ind) >= 0) and pts_ind[-1] == n_pts - 1
    for r in range(3):
        sel = slice(r * scene.n_obs, (r + 1) * scene.n_obs)
        assert np.array_equal(pts_ind[sel] - r * 293, scene.pts_ind) and np.array_equal(cam_ind[sel], scene.cam_ind)
        assert np.array_equal(pts2d[sel], scene.pts2d)


def test_extended_precision_is_extended_and_the_vectorised_routine_is_the_scalar_one():
    assert np.finfo(np.longdouble).eps < 1e-18
    for cls in (("affine", 0.3, 0.0), ("affine", 3e-5, 0.3), ("perspective", 3e-3, 0.3), ("perspective", 3e-5, 0.0)):
        P1, P2, a, b = CT.linear_class(*cls)
        vec, sca = CT.triangulate_ld(P1, P2, a[:5], b[:5]), CT.triangulate_ld(P1, P2, a[:5], b[:5], scalar=True)
        assert vec.dtype == np.longdouble and np.array_equal(vec, sca)


@pytest.mark.parametrize("model,delta,noise", CT.LINEAR_CLASSES)
def test_linear_classes(model, delta, noise):
    """The pair is `delta` apart, the points are where the scene is, and the float64 Jacobi restatement stays inside 1e-8 m / delta of
    the extended-precision points (measured: 2e-9 m / delta) while numpy.linalg.svd does not at delta = 0.3."""
    P1, P2, a, b = CT.linear_class(model, delta, noise)
    assert a.shape == b.shape == (100, 2) and P1.shape == P2.shape == (3, 4)
    if model == "affine":
        d1, d2 = (np.cross(P[0, :3], P[1, :3]) for P in (P1, P2))
    else:
        d1, d2 = P1[2, :3], P2[2, :3]
    sep = np.arccos(np.clip(d1 @ d2 / np.linalg.norm(d1) / np.linalg.norm(d2), -1, 1))
    assert 0.85 * delta <= sep <= 1.01 * delta or (delta < 1e-4 and abs(sep - delta) < 3e-8)  # (cos(second Euler angle) >= 0.87; arccos near 1)
    ref = CT.triangulate_ld(P1, P2, a, b)
    assert np.abs(ref.astype(np.float64) - CT.synth.SCENE_CENTRE).max() < 5e3 + (40.0 * noise + 1e-3) / delta
    err = CT.restatement_error(P1, P2, a, b, ref)
    print("{} delta {:g} noise {:g}: float64 restatement {:.3g} m, bound {:.3g} m".format(model, delta, noise, err, 1e-8 / delta))
    assert 0 < err <= 1e-8 / delta
    if delta == 0.3:
        assert CT.error_m(CT.triangulate_lapack(P1, P2, a, b), ref).max() > 1e-8 / delta


def test_long_track_scene():
    scene = CT.long_track_scene()
    cnt = np.bincount(scene.pts_ind)
    assert scene.n_pts == 205 and tuple(cnt[:5]) == CT.LONG_HAND == (70, 2, 63, 64, 65) and 2 < cnt[5:].min() and cnt[5:].max() < 70
    key = scene.pts_ind * CT.LONG_CAMS + scene.cam_ind
    assert np.all(np.diff(key) > 0) and scene.cam_ind.max() == 69  # point-major, cameras ascending: what from_observations asks for
    assert np.array_equal(np.sort(scene.cam_ind[scene.pts_ind == 0]), np.arange(70))  # one track alone names every camera
    # sorted by length (the handle's internal order) the tracks fill three full slices of 64 and one of 13, of mixed lengths each
    order = np.sort(cnt)
    assert all(len(set(order[s:s + 64])) > 1 for s in range(0, 205, 64)) and order[0] == 2 and order[-1] == 70
    # the observations are projections of the points: the triangulated points are near them
    want = CT.batched_oracle(scene, CT.long_pairs(False, n=50), [0, 2, 3, 4, 100])
    assert np.abs(want - scene.pts3d_true[[0, 2, 3, 4, 100]]).max() < 20.0
    big = CT.long_track_scene(CT.PREFIX_BASE)
    assert big.n_pts == 300 > max(CT.PREFIX_N) and tuple(np.bincount(big.pts_ind)[:5]) == CT.LONG_HAND
    for n in CT.PREFIX_N:
        pre = CT.prefix_scene(big, n)
        assert pre.n_pts == n and pre.pts_ind.max() == n - 1 and pre.pts_ind.size == np.count_nonzero(big.pts_ind < n)
        assert np.array_equal(pre.pts2d, big.pts2d[:pre.n_obs]) and pre.pts3d.shape == (n, 3)


def test_long_pair_lists():
    full = CT.long_pairs(False)
    assert len(full) == 2415 and full == sorted(full) and CT.n_tri_reference([0] * 70, range(70), 1, 70, full)[0] == 2415 > 100 * 24
    gen = CT.long_pairs(True)
    assert len(gen) == 2417 and gen[:-2] != sorted(gen[:-2]) and set(gen[:-2]) == set(full)
    assert gen[-2] == gen[1] and gen[-1] == gen[3][::-1]
    sub = CT.long_pairs(True, n=240)
    assert len(sub) == 242 and set(sub[:-2]) < set(full) and sub[-1][0] > sub[-1][1]


def test_batched_oracle_is_the_oracle():
    scene = CT.long_track_scene()
    pairs = CT.long_pairs(True, n=30)
    tracks = [0, 1, 4, 77, 204]
    assert np.array_equal(CT.batched_oracle(scene, pairs, tracks), T.init_pts3d(scene.to_dense_C(), scene.cameras, "affine", pairs)[tracks])

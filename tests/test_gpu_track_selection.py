"""
Track selection on the device (satba.ft_ranking, csrc/satba_tracks.h) against what the reference's ft_ranking recorded in
tests/golden/track_selection.npz (tools/gen_golden_tracks.py).  The fixtures keep the reference's orderings strict with a margin
(tests/test_track_selection_host.py), so sets are compared exactly.
"""
import numpy as np
import pytest

import cases_tracks as CT
from satba import ft_ranking, synth

pytestmark = pytest.mark.gpu

_GOLDEN = {}


def case(name):
    """The stored arrays of one case (loaded once, never modified: arrays are handed out read-only)."""
    if not _GOLDEN:
        g = CT.load()
        for key in g.files:
            a = g[key]
            a.setflags(write=False)
            _GOLDEN[key] = a
    out = {k[len(name) + 1:]: v for k, v in _GOLDEN.items() if k.startswith(name + "_")}
    out["n_cam"], out["n_pts"], out["K"], out["n_trees"] = int(out["n_cam"]), int(out["n_pts"]), int(out["K"]), int(out["n_trees"])
    out["priority"] = [CT.PRIORITY_NAMES[i] for i in out["priority"]]
    return out


def run(g, **kw):
    args = dict(K=g["K"], priority=g["priority"], return_info=True)
    args.update(kw)
    return ft_ranking.select_best_tracks_from_observations(g["pts_ind"], g["cam_ind"], g["scale"], g["err"], g["n_cam"], g["n_pts"], **args)


def dense3(g):
    d = lambda v=None: CT.dense(g["pts_ind"], g["cam_ind"], g["n_cam"], g["n_pts"], v)  # noqa: E731
    return d(), d(g["scale"]), d(g["err"])


ALL = list(CT.SELECTION_CASES)


# ----------------------------------------------------------------------------- connectivity

@pytest.mark.parametrize("name", ALL)
def test_connectivity_matrix_equals_reference(gpu, name):
    g = case(name)
    C = CT.dense(g["pts_ind"], g["cam_ind"], g["n_cam"], g["n_pts"])
    for mm, key in ((0, "A0"), (10, "A10")):
        A = ft_ranking.build_connectivity_matrix(C, min_matches=mm)
        assert A.dtype == np.float64 and A.shape == (g["n_cam"], g["n_cam"])
        assert np.array_equal(A, g[key]), (name, mm)
    assert np.array_equal(ft_ranking.build_connectivity_matrix(C), g["A10"])  # the default is 10


def test_connectivity_alive_mask(gpu):
    g = case("c70_long")
    alive = (np.arange(g["n_pts"]) % 3 != 0)
    ofs, cam32 = ft_ranking._group(g["pts_ind"], g["cam_ind"], g["n_cam"], g["n_pts"])
    A = ft_ranking._connectivity(ofs, cam32, g["n_cam"], g["n_pts"], alive, 0, None)
    seen = ~np.isnan(CT.dense(g["pts_ind"], g["cam_ind"], g["n_cam"], g["n_pts"], g["scale"]))[:, alive]
    ref = seen.astype(np.int64) @ seen.T.astype(np.int64)
    np.fill_diagonal(ref, 0)
    assert np.array_equal(A, ref)


# ----------------------------------------------------------------------------- ranking

@pytest.mark.parametrize("name", ALL)
def test_track_keys_are_bit_identical_to_numpy(gpu, name):
    g = case(name)
    length, ks, kc = ft_ranking.track_keys_from_observations(g["pts_ind"], g["cam_ind"], g["scale"], g["err"], g["n_cam"], g["n_pts"])
    l_ref, ks_ref, kc_ref = CT.numpy_keys(g["pts_ind"], g["cam_ind"], g["scale"], g["err"], g["n_cam"], g["n_pts"])
    assert np.array_equal(length, l_ref)
    assert np.array_equal(ks.view(np.int64), ks_ref.view(np.int64))
    assert np.array_equal(kc.view(np.int64), kc_ref.view(np.int64))


@pytest.mark.parametrize("name", ALL)
def test_ranking_equals_reference(gpu, name):
    g = case(name)
    _, info = run(g, K=0)
    assert np.array_equal(info["rank"], g["rank"]), name
    ranked = ft_ranking.order_tracks(*dense3(g), priority=g["priority"])
    assert isinstance(ranked, dict) and len(ranked) == g["n_pts"]
    assert ranked == {int(t): int(r) for t, r in enumerate(g["rank"])}


def test_short_priority_is_completed_by_numpys_rule(gpu):
    g = case("c8_lsc")
    full = run(g, K=0, priority=["scale", "length", "cost"])[1]["rank"]
    assert np.array_equal(run(g, K=0, priority=["scale"])[1]["rank"], full)
    assert np.array_equal(run(g, K=0, priority=[])[1]["rank"], g["rank"])
    assert np.array_equal(run(g, K=0, priority=["cost"])[1]["rank"], case("c8_cls")["rank"])


def test_exact_ties_put_the_higher_track_index_first(gpu):
    pts = np.repeat(np.arange(5), 2)
    cam = np.tile([0, 1], 5)
    _, info = ft_ranking.select_best_tracks_from_observations(pts, cam, np.ones(10), None, 2, 5, K=0, return_info=True)
    assert np.array_equal(info["rank"], [4, 3, 2, 1, 0])


# ----------------------------------------------------------------------------- selection

@pytest.mark.parametrize("name", ALL)
def test_selection_equals_reference(gpu, name):
    g = case(name)
    S, info = run(g)
    assert np.array_equal(S, g["S"]), name
    assert info["n_trees"] == g["n_trees"]
    assert np.array_equal(info["tree_of"], g["tree_of"]), name  # the same track set per tree
    n = g["n_trees"]
    w, w_ref = info["weights"][:n], g["weights"][:n]
    rel = np.abs(w - w_ref).max() / np.abs(w_ref).max() if n else 0.0
    print(name, "weights: largest relative difference", rel)
    assert np.all(np.abs(w - w_ref) <= 1e-12 * np.abs(w_ref)), rel
    if g["weights"].shape[0] > n and n < g["K"] and g["S"].size < g["n_pts"]:
        # the empty tree that ended the loop started from the weights the reference's next (empty) tree started from
        assert np.all(np.abs(info["weights"][n] - g["weights"][n]) <= 1e-12 * np.abs(g["weights"][n]))
    assert not info["weights"][n + 1:].any()


@pytest.mark.parametrize("name", ["c8_scl", "c70_long", "c11_split"])
def test_dense_and_list_entry_points_agree(gpu, name):
    g = case(name)
    S = ft_ranking.select_best_tracks(*dense3(g), K=g["K"], priority=g["priority"])
    assert isinstance(S, np.ndarray) and np.array_equal(S, run(g)[0]) and np.array_equal(S, g["S"])
    w = ft_ranking.compute_camera_weights(dense3(g)[0], dense3(g)[2])
    assert isinstance(w, list) and len(w) == g["n_cam"]
    assert np.all(np.abs(np.array(w) - g["weights"][0]) <= 1e-12 * g["weights"][0])


def test_verbose_lines_are_the_reference_ones(gpu, capsys):
    g = case("c8_lsc")
    ft_ranking.select_best_tracks(*dense3(g), K=g["K"], priority=g["priority"], verbose=True)
    out = capsys.readouterr().out
    assert "Running feature tracks selection algorithm..." in out and "...done in " in out
    assert "Selected {} tracks out of 300 ({:.2f}%)".format(g["S"].size, g["S"].size / 3.0) in out
    assert "     - priority: ['length', 'scale', 'cost']" in out
    obs = np.bincount(g["cam_ind"], minlength=8)
    assert "     - obs per cam before: {}".format(obs) in out and "     - obs per cam after:  " in out


@pytest.mark.parametrize("name", ["c16_k60", "c70_long"])
def test_selection_does_not_depend_on_the_order_of_the_observations(gpu, name):
    g = case(name)
    perm = np.random.default_rng(4).permutation(g["pts_ind"].size)
    S, info = ft_ranking.select_best_tracks_from_observations(g["pts_ind"][perm], g["cam_ind"][perm], g["scale"][perm], g["err"][perm],
                                                              g["n_cam"], g["n_pts"], K=g["K"], priority=g["priority"], return_info=True)
    S0, info0 = run(g)
    assert np.array_equal(S, S0) and np.array_equal(info["tree_of"], info0["tree_of"]) and np.array_equal(info["rank"], info0["rank"])
    assert np.array_equal(info["weights"], info0["weights"])


def test_sensor_aware_selection_is_the_union_of_the_parts(gpu):
    g = case("c8_lsc")
    C, C_scale, C_reproj = dense3(g)

    class Im:
        def __init__(self, path):
            self.geotiff_path = path

    images = [Im("x/{}_{}.tif".format("d1" if i < 4 else "d2" if i < 7 else "d3", i)) for i in range(8)]
    S = ft_ranking.select_best_tracks_sensor_aware(images, C, C_scale, C_reproj, K=2)
    parts = [ft_ranking.select_best_tracks(C, C_scale, C_reproj, K=2)]
    seen = ~np.isnan(C[::2])
    for cams in (np.arange(0, 4), np.arange(4, 7)):  # the third sensor has one camera: skipped
        tracks = np.nonzero(seen[cams].sum(axis=0) >= 2)[0]
        rows = np.stack((2 * cams, 2 * cams + 1), axis=1).ravel()
        parts.append(tracks[ft_ranking.select_best_tracks(C[rows][:, tracks], C_scale[cams][:, tracks], C_reproj[cams][:, tracks], K=2)])
    assert S.dtype == np.int32 and np.array_equal(S, np.unique(np.concatenate(parts)))


# ----------------------------------------------------------------------------- end to end

@pytest.mark.parametrize("name", list(CT.E2E_CASES))
def test_end_to_end_from_the_device_errors(gpu, name):
    """compute_C_reproj at the tolerance tests/test_gpu_parity.py uses for `fun` of the camera model, and the selection made from it."""
    g = case(name)
    model, n_cam, n_pts, opp, K, kw = CT.E2E_CASES[name]
    sc = synth.make_scene(model, n_cam, n_pts, opp, seed=int(g["seed"]), **kw)
    assert np.array_equal(sc.pts_ind, g["pts_ind"]) and np.array_equal(sc.cam_ind, g["cam_ind"])
    C = sc.to_dense_C()
    C_reproj = ft_ranking.compute_C_reproj(C, sc.pts3d, sc.cameras, model, sc.pairs_to_triangulate, sc.camera_centers)
    ref = CT.dense(g["pts_ind"], g["cam_ind"], n_cam, n_pts, g["err"])
    assert C_reproj.shape == (n_cam, n_pts) and np.array_equal(np.isnan(C_reproj), np.isnan(ref))
    tol = 2.5e-4 if model == "rpc" else 1e-8
    diff = np.nanmax(np.abs(C_reproj - ref))
    print(name, "largest difference of the reprojection errors", diff)
    assert diff < tol, diff
    C_scale = CT.dense(g["pts_ind"], g["cam_ind"], n_cam, n_pts, g["scale"])
    S = ft_ranking.select_best_tracks(C, C_scale, C_reproj, K=K)
    assert np.array_equal(S, g["S"])


# ----------------------------------------------------------------------------- repeatability, edge cases

def test_two_runs_are_bit_identical(gpu):
    g = case("c16_k60")
    (S1, a), (S2, b) = run(g), run(g)
    assert np.array_equal(S1, S2) and np.array_equal(a["tree_of"], b["tree_of"]) and np.array_equal(a["rank"], b["rank"])
    assert np.array_equal(a["weights"].view(np.int64), b["weights"].view(np.int64))


def test_k_zero_selects_nothing(gpu):
    S, info = run(case("c8_lsc"), K=0)
    assert S.size == 0 and info["n_trees"] == 0 and np.all(info["tree_of"] == -1) and info["weights"].shape == (0, 8)


def test_k_larger_than_needed_stops_when_the_tracks_run_out(gpu):
    g = case("c7_exhaust")
    S, info = run(g, K=500)
    assert np.array_equal(S, np.arange(30)) and info["n_trees"] == g["n_trees"] < 60
    assert np.array_equal(info["tree_of"], g["tree_of"]) and not info["weights"][g["n_trees"]:].any()


def _components(n_cam, pts_ind, cam_ind, tracks):
    """Connected components of the cameras under the given tracks (labels)."""
    label = np.arange(n_cam)
    keep = np.isin(pts_ind, tracks)
    first = {}
    for t, c in zip(pts_ind[keep], cam_ind[keep]):
        first.setdefault(t, c)
    changed = True
    while changed:
        changed = False
        for t, c in zip(pts_ind[keep], cam_ind[keep]):
            a, b = label[first[t]], label[c]
            if a != b:
                label[label == max(a, b)] = min(a, b)
                changed = True
    return label


@pytest.mark.parametrize("name", ["c8_lsc", "c11_split", "c70_long"])
def test_without_errors_the_selection_spans_what_all_tracks_span(gpu, name):
    """err=None (no 3-D points yet): costs are zero and ties abound, so only the property is checked, not the reference's set."""
    g = case(name)
    S, info = ft_ranking.select_best_tracks_from_observations(g["pts_ind"], g["cam_ind"], g["scale"], None, g["n_cam"], g["n_pts"], K=1,
                                                              return_info=True)
    assert 0 < S.size < g["n_pts"] and np.array_equal(S, np.nonzero(info["tree_of"] == 0)[0])
    full = _components(g["n_cam"], g["pts_ind"], g["cam_ind"], np.arange(g["n_pts"]))
    root = int(np.argmax(info["weights"][0]))
    got = _components(g["n_cam"], g["pts_ind"], g["cam_ind"], S)
    assert np.array_equal(got == got[root], full == full[root])  # one tree reaches the whole component of its root


def test_sizes_off_the_wave_and_workgroup_size(gpu):
    """n_pts = 1, 63, 65, 129, 257 (no multiple of 64 or 256); 200 and 300 cameras take the pair table past the default LDS size and
    past LDS altogether.  With K = n_pts every track (all have two or more cameras) must be selected exactly once."""
    for n_cam, n_pts in ((2, 1), (5, 63), (9, 65), (200, 129), (300, 257)):
        pts, cam, sc, er = CT.random_tracks(n_cam, n_pts, 7, max_len=4)
        S, info = ft_ranking.select_best_tracks_from_observations(pts, cam, sc, er, n_cam, n_pts, K=n_pts, return_info=True)
        assert np.array_equal(S, np.arange(n_pts)), (n_cam, n_pts)
        assert np.array_equal(np.sort(info["rank"]), np.arange(n_pts))
        assert info["n_trees"] == info["tree_of"].max() + 1
    S = ft_ranking.select_best_tracks_from_observations([], [], [], None, 4, 0, K=3)
    assert S.size == 0

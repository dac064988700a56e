"""
Track construction on the device (satba.ft_utils, csrc/satba_ftracks.h) against what the reference's ft_utils recorded in
tests/golden/feature_tracks.npz (tools/gen_golden_ft.py) and, where nothing is stored, against the numpy rule of tests/cases_ft.py,
which tests/test_feature_tracks_host.py ties to the same file.  Everything is compared exactly.
"""
import numpy as np
import pytest

import cases_ft as CF
from satba import ft_triangulate, ft_utils, synth

pytestmark = pytest.mark.gpu

_GOLDEN = {}
_CACHE = {}


def stored(name):
    """The stored arrays of one case (loaded once, never modified: arrays are handed out read-only)."""
    if not _GOLDEN:
        g = CF.load()
        for key in g.files:
            a = g[key]
            a.setflags(write=False)
            _GOLDEN[key] = a
    return {k[len(name) + 1:]: v for k, v in _GOLDEN.items() if k.startswith(name + "_")}


def build(case, **kw):
    out = ft_utils.feature_tracks_from_matches(case["kp"], case["kp_ofs"], case["matches"], case["pairs"], return_info=True, **kw)
    keys = ("pts_ind", "cam_ind", "pts2d", "kp_id", "scale", "n_pts", "n_pts_fix", "info")
    return dict(zip(keys, out))


def dense_of(r, n_cam):
    return CF.dense(r["pts_ind"], r["cam_ind"], r["pts2d"], r["kp_id"], n_cam, r["n_pts"])


def check_lists(r, case):
    """The lists are what the triangulation and the selection take, and they agree with the keypoints they name."""
    n_obs = r["pts_ind"].size
    assert r["cam_ind"].dtype == np.int32 and r["kp_id"].dtype == np.int32 and r["pts2d"].dtype == np.float64 and r["scale"].dtype == np.float64
    assert r["cam_ind"].shape == r["kp_id"].shape == r["scale"].shape == (n_obs,) and r["pts2d"].shape == (n_obs, 2)
    ofs = r["info"]["pt_ofs"]
    assert ofs[0] == 0 and ofs[-1] == n_obs and ofs.size == r["n_pts"] + 1 and np.all(np.diff(ofs) >= 2)
    assert np.array_equal(r["pts_ind"], np.repeat(np.arange(r["n_pts"]), np.diff(ofs)))
    inside = np.diff(r["pts_ind"]) == 0
    assert np.all(np.diff(r["cam_ind"])[inside] > 0)  # cameras ascend strictly inside a track
    g = case["kp_ofs"][r["cam_ind"]] + r["kp_id"]
    assert np.all(r["kp_id"] >= 0) and np.all(g < case["kp_ofs"][r["cam_ind"] + 1])
    assert np.array_equal(r["pts2d"], case["kp"][g, :2].astype(np.float64)) and np.array_equal(r["scale"], case["kp"][g, 2].astype(np.float64))


def same_lists(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("pts_ind", "cam_ind", "pts2d", "kp_id", "scale")) and a["n_pts"] == b["n_pts"] \
        and a["n_pts_fix"] == b["n_pts_fix"]


def against_rule(r, case, **kw):
    ref = CF.rule(case["kp"], case["kp_ofs"], case["matches"], case["pairs"], **kw)
    assert same_lists(r, ref)
    assert r["info"]["n_components"] == ref["n_components"] and r["info"]["n_conflicts"] == ref["n_conflicts"]
    return ref


# ----------------------------------------------------------------------------- 1-3: the reference's matrices

@pytest.mark.parametrize("name", CF.SMALL_CASES)
def test_small_cases_equal_reference(gpu, name):
    case = stored(name)
    r = build(case)
    check_lists(r, case)
    C, V = dense_of(r, case["kp_ofs"].size - 1)
    print(name, "tracks", r["n_pts"], "components", r["info"]["n_components"], "conflicts", r["info"]["n_conflicts"])
    assert CF.same(C, V, case["C"], case["C_v2"])
    against_rule(r, case)


def test_scene_with_contended_parents_equals_reference(gpu):
    case = stored(CF.SCENE8[0])
    r = build(case)
    check_lists(r, case)
    C, V = dense_of(r, 8)
    assert CF.same(C, V, case["C"], case["C_v2"])
    ref = against_rule(r, case)
    print("scene8: tracks", r["n_pts"], "conflicts", r["info"]["n_conflicts"], "kernel_ms", r["info"]["kernel_ms"])
    assert r["info"]["n_conflicts"] > 0 and r["info"]["n_conflicts"] == ref["n_conflicts"]
    assert r["info"]["n_components"] == case["C_pre"].shape[1]


def test_chain_and_star_equal_reference(gpu):
    """Deep finds, the retry path, tracks of length 64 in the baseline check (2 016 pair tests per track)."""
    case = stored(CF.CHAIN)
    r = build(case)
    check_lists(r, case)
    C, V = dense_of(r, 64)
    assert CF.same(C, V, case["C"], case["C_v2"])
    assert r["n_pts"] == 4 and np.array_equal(np.diff(r["info"]["pt_ofs"]), [64] * 4) and r["info"]["n_conflicts"] == 0
    # either listed pair alone keeps all four tracks; a pair of the right cameras in the wrong order keeps none
    for pairs, n in (([(62, 63)], 4), ([(0, 5)], 4), ([(63, 62), (5, 0)], 0)):
        assert build(dict(case, pairs=np.array(pairs, dtype=np.int32)))["n_pts"] == n


def test_through_files_like_the_reference(gpu, tmp_path, capsys):
    """feature_tracks_from_pairwise_matches on keypoint files of different lengths and 132 columns; the reference's two prints."""
    case = stored("small06")
    n_cam = case["kp_ofs"].size - 1
    paths = []
    for m in range(n_cam):
        f = np.zeros((case["kp_ofs"][m + 1] - case["kp_ofs"][m], 132), dtype=np.float32)
        f[:, :3] = case["kp"][case["kp_ofs"][m]:case["kp_ofs"][m + 1]]
        paths.append(str(tmp_path / "{}.npy".format(m)))
        np.save(paths[-1], f)
    C, V = ft_utils.feature_tracks_from_pairwise_matches(paths, case["matches"], [tuple(p) for p in case["pairs"]])
    out = capsys.readouterr().out.splitlines()
    assert C.dtype == np.float64 and V.dtype == np.float64 and CF.same(C, V, case["C"], case["C_v2"])
    n_comp = CF.rule(case["kp"], case["kp_ofs"], case["matches"], case["pairs"])["n_components"]
    assert out[-2:] == ["C.shape before baseline check {}".format((2 * n_cam, n_comp)), "C.shape after baseline check {}".format(C.shape)]
    S = ft_utils.compute_C_scale(V, paths)
    seen = ~np.isnan(V)
    cams, trks = np.nonzero(seen)
    assert np.array_equal(np.isnan(S), ~seen)
    assert np.array_equal(S[cams, trks], case["kp"][case["kp_ofs"][cams] + V[cams, trks].astype(np.int64), 2].astype(np.float64))


# ----------------------------------------------------------------------------- 4: medium, against the rule

def scene12():
    if "scene12" not in _CACHE:
        case = CF.scene(**CF.SCENE12)
        for a in case.values():
            a.setflags(write=False)
        _CACHE["scene12"] = (case, CF.rule(**case))
    return _CACHE["scene12"]


def test_medium_scene_equals_the_rule(gpu):
    case, ref = scene12()
    r = build(case)
    print("12 x 20000: matches", case["matches"].shape[0], "tracks", r["n_pts"], "components", r["info"]["n_components"], "conflicts",
          r["info"]["n_conflicts"], "kernel_ms", r["info"]["kernel_ms"])
    assert case["matches"].shape[0] > 150000 and ref["n_conflicts"] > 0
    check_lists(r, case)
    assert same_lists(r, ref)
    assert r["info"]["n_components"] == ref["n_components"] and r["info"]["n_conflicts"] == ref["n_conflicts"]


# ----------------------------------------------------------------------------- 5: order independence, repeatability

def test_output_does_not_depend_on_the_order_of_the_rows(gpu):
    case = CF.scene(7, 1500, 1100, seed=21, false_frac=0.0)
    base = build(case)
    assert base["info"]["n_conflicts"] == 0 and base["n_pts"] > 0
    against_rule(base, case)
    for seed in (1, 2, 3):
        perm = np.random.default_rng(seed).permutation(case["matches"].shape[0])
        assert same_lists(build(dict(case, matches=case["matches"][perm])), base), seed
    flipped = case["matches"][:, [1, 0, 3, 2]]  # im_i > im_j: the same graph edges
    assert same_lists(build(dict(case, matches=flipped)), base)


@pytest.mark.parametrize("which", ["scene8", "scene12"])
def test_two_runs_are_bit_identical(gpu, which):
    case = stored(CF.SCENE8[0]) if which == "scene8" else scene12()[0]
    a, b = build(case), build(case)
    for k in ("pts_ind", "cam_ind", "pts2d", "kp_id", "scale"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.array_equal(a["info"]["pt_ofs"], b["info"]["pt_ofs"])
    assert (a["n_pts"], a["n_pts_fix"], a["info"]["n_components"], a["info"]["n_conflicts"]) == \
        (b["n_pts"], b["n_pts_fix"], b["info"]["n_components"], b["info"]["n_conflicts"])


# ----------------------------------------------------------------------------- 6: n_adj

def test_n_adj_puts_the_fixed_tracks_first(gpu):
    """ft_pipeline.py:175-179 applied to the n_adj = 0 result."""
    case = stored(CF.SCENE8[0])
    n_adj = 3
    r0, r3 = build(case), build(case, n_adj=n_adj)
    check_lists(r3, case)
    C0, V0 = dense_of(r0, 8)
    where_fix = np.sum(~np.isnan(C0[::2])[n_adj:], axis=0) == 0
    n_fix = int(where_fix.sum())
    assert 0 < n_fix < r0["n_pts"] and r3["n_pts_fix"] == n_fix and r0["n_pts_fix"] == 0 and r3["n_pts"] == r0["n_pts"]
    C3, V3 = dense_of(r3, 8)
    assert np.array_equal(C3, np.hstack([C0[:, where_fix], C0[:, ~where_fix]]), equal_nan=True)
    assert np.array_equal(V3, np.hstack([V0[:, where_fix], V0[:, ~where_fix]]), equal_nan=True)
    against_rule(r3, case, n_adj=n_adj)


# ----------------------------------------------------------------------------- 7: into the chain

def test_lists_feed_the_triangulation(gpu, tmp_path):
    n_cam, n_pts = 6, 300
    sc = synth.make_scene("affine", n_cam, n_pts, 3, seed=7)
    # one keypoint per observation, numbered inside each image by track; the tracks renumbered by (first camera, track) so that the
    # smallest global id of a track ascends with its number and the device's column order is the identity
    first_cam = np.full(n_pts, n_cam)
    np.minimum.at(first_cam, sc.pts_ind, sc.cam_ind)
    new_of = np.empty(n_pts, dtype=np.int64)
    new_of[np.lexsort((np.arange(n_pts), first_cam))] = np.arange(n_pts)
    pts_ind = new_of[sc.pts_ind]
    order = np.lexsort((sc.cam_ind, pts_ind))
    pts_ind, cam_ind, pts2d = pts_ind[order], sc.cam_ind[order], sc.pts2d[order]
    by_cam = np.lexsort((pts_ind, cam_ind))
    kp_ofs = np.concatenate([[0], np.cumsum(np.bincount(cam_ind, minlength=n_cam))]).astype(np.int64)
    kp_id = np.empty(pts_ind.size, dtype=np.int64)
    kp_id[by_cam] = np.arange(pts_ind.size) - kp_ofs[cam_ind[by_cam]]
    kp = np.zeros((pts_ind.size, 3), dtype=np.float32)
    kp[kp_ofs[cam_ind] + kp_id, :2] = pts2d
    kp[:, 2] = 2.0
    rows = [(kp_id[o], kp_id[o + 1], cam_ind[o], cam_ind[o + 1]) for o in range(pts_ind.size - 1) if pts_ind[o] == pts_ind[o + 1]]
    matches = np.array(rows, dtype=np.int32)[np.random.default_rng(7).permutation(len(rows))]
    pairs = [(i, j) for i in range(n_cam) for j in range(i + 1, n_cam)]

    r = build(dict(kp=kp, kp_ofs=kp_ofs, matches=matches, pairs=np.array(pairs, dtype=np.int32)))
    assert r["n_pts"] == n_pts and np.array_equal(r["pts_ind"], pts_ind) and np.array_equal(r["cam_ind"], cam_ind)
    assert np.array_equal(r["pts2d"], np.float32(pts2d).astype(np.float64)) and np.array_equal(r["kp_id"], kp_id)

    paths = []
    for m in range(n_cam):
        paths.append(str(tmp_path / "{}.npy".format(m)))
        np.save(paths[-1], kp[kp_ofs[m]:kp_ofs[m + 1]])
    C, _ = ft_utils.feature_tracks_from_pairwise_matches(paths, matches, pairs)
    from_lists = ft_triangulate.init_pts3d_from_observations(r["pts_ind"], r["cam_ind"], r["pts2d"], r["n_pts"], sc.cameras, "affine", pairs)
    from_dense = ft_triangulate.init_pts3d(C, sc.cameras, "affine", pairs)
    assert from_lists.shape == (n_pts, 3) and np.any(from_lists != 0) and from_lists.tobytes() == from_dense.tobytes()


# ----------------------------------------------------------------------------- 8: edges

def test_edges(gpu):
    case = stored("small03")
    n_cam = case["kp_ofs"].size - 1
    none = build(dict(case, matches=np.zeros((0, 4), dtype=np.int32)))
    assert none["n_pts"] == 0 and none["pts_ind"].size == 0 and np.array_equal(none["info"]["pt_ofs"], [0]) and none["info"]["n_components"] == 0
    dropped = build(dict(case, pairs=np.zeros((0, 2), dtype=np.int32)))
    assert dropped["n_pts"] == 0 and np.array_equal(dropped["info"]["pt_ofs"], [0]) and dropped["info"]["n_components"] == case["C_pre"].shape[1]
    listed = case["pairs"][case["pairs"][:, 0] < case["pairs"][:, 1]]
    assert build(dict(case, pairs=listed))["n_pts"] == case["C"].shape[1] > 0
    reversed_only = build(dict(case, pairs=listed[:, ::-1]))  # every pair only as (j, i) with j > i
    assert reversed_only["n_pts"] == 0
    allp = np.array([(i, j) for i in range(n_cam) for j in range(i + 1, n_cam)], dtype=np.int32)
    pre = build(dict(case, pairs=allp))
    C, V = dense_of(pre, n_cam)
    assert CF.same(C, V, case["C_pre"], case["C_v2_pre"])


@pytest.mark.parametrize("name", CF.PRE_CASES)
def test_baseline_check_alone_returns_the_reference_indices(gpu, name):
    case = stored(name)
    keep = ft_utils.filter_C_using_pairs_to_triangulate(case["C_pre"], [tuple(p) for p in case["pairs"]])
    assert np.array_equal(keep, case["keep"])
    assert ft_utils.filter_C_using_pairs_to_triangulate(case["C_pre"], []).size == 0
    assert ft_utils.filter_C_using_pairs_to_triangulate(case["C_pre"][:, :0], [(0, 1)]).size == 0


@pytest.mark.parametrize("n_cam", [800, 1200])
def test_baseline_check_with_many_cameras(gpu, n_cam):
    """800 cameras: the bit matrix (80 KB) needs more LDS than a kernel gets by default; 1200: it (180 KB) stays in global memory."""
    rng = np.random.default_rng(12)
    n_pts = 700
    cams = [np.sort(rng.permutation(n_cam)[: rng.integers(2, 6)]) for _ in range(n_pts)]
    pts_ind = np.repeat(np.arange(n_pts), [c.size for c in cams])
    cam_ind = np.concatenate(cams)
    pairs = np.sort(np.stack([rng.permutation(n_cam)[:2] for _ in range(150000)]), axis=1)
    keep = ft_utils.tracks_have_pair(pts_ind, cam_ind, n_cam, n_pts, pairs)
    expect = CF.has_pair(pts_ind, cam_ind, n_cam, n_pts, pairs)
    assert 0 < expect.sum() < n_pts and np.array_equal(keep, expect)

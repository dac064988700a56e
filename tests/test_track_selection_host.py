"""Track selection (satba.ft_ranking): what can be checked without a device -- the fixtures, the surface, the argument checks."""
import inspect

import numpy as np
import pytest

import cases_tracks as CT
from satba import engine_hip, ft_ranking


@pytest.fixture(scope="module")
def golden():
    return CT.load()


def test_golden_file_holds_only_numeric_arrays_of_every_case(golden):
    for key in golden.files:
        assert golden[key].dtype.kind in "iuf", key
    for name in list(CT.SELECTION_CASES) + list(CT.E2E_CASES):
        for field in ("pts_ind", "cam_ind", "scale", "err", "rank", "S", "tree_of", "n_trees", "weights", "A0", "A10", "priority", "K"):
            assert name + "_" + field in golden.files, (name, field)
    for name, (n_cam, n_pts, K, priority, _) in CT.SELECTION_CASES.items():
        assert (int(golden[name + "_n_cam"]), int(golden[name + "_n_pts"]), int(golden[name + "_K"])) == (n_cam, n_pts, K)
        assert np.array_equal(golden[name + "_priority"], CT.priority_codes(priority))
        assert golden[name + "_weights"].shape[1] == n_cam and golden[name + "_A0"].shape == (n_cam, n_cam)
        assert np.array_equal(np.sort(golden[name + "_rank"]), np.arange(n_pts))
        assert np.array_equal(golden[name + "_S"], np.nonzero(golden[name + "_tree_of"] >= 0)[0])
    # the shapes the issue asks for are really in there
    assert int(golden["c7_exhaust_n_trees"]) < 60 and golden["c7_exhaust_S"].size == 30  # K exhausts all tracks
    assert np.bincount(golden["c70_long_pts_ind"]).max() >= 30  # long tracks, more than 64 cameras
    A = golden["c11_split_A0"]
    assert not A[:5, 5:].any() and not A[10].any() and A[:5, :5].any() and A[5:10, 5:10].any()  # two groups, one empty camera
    for name in golden.files:
        if name.endswith("_n_pts"):
            assert int(golden[name]) % 64 != 0  # no fixture is a multiple of the wave or the workgroup size


@pytest.mark.parametrize("name", list(CT.SELECTION_CASES) + list(CT.E2E_CASES))
def test_golden_cases_keep_the_gaps_that_define_the_selection(golden, name):
    """The reference's orderings must be strict with a margin: camera weights inside a tree, costs of tracks that tie otherwise."""
    g = {k: golden[name + "_" + k] for k in ("pts_ind", "cam_ind", "scale", "err", "rank", "tree_of", "weights", "priority")}
    priority = [CT.PRIORITY_NAMES[i] for i in g["priority"]]
    w_gap, c_gap = CT.gaps(g["pts_ind"], g["cam_ind"], g["scale"], g["err"], int(golden[name + "_n_cam"]), int(golden[name + "_n_pts"]),
                           priority, g["rank"], g["tree_of"], g["weights"])
    need = CT.E2E_GAP if name in CT.E2E_CASES else CT.SELECTION_GAP
    print(name, "weight gap", w_gap, "cost gap", c_gap)
    assert w_gap >= need and c_gap >= need, (w_gap, c_gap)


def test_ft_ranking_exposes_the_reference_signatures():
    """Parameter names and defaults of ref:bundle_adjust/feature_tracks/ft_ranking.py (positional use must keep working)."""
    prio = ["length", "scale", "cost"]
    expected = {
        "build_connectivity_matrix": [("C", inspect.Parameter.empty), ("min_matches", 10)],
        "compute_C_reproj": [(n, inspect.Parameter.empty) for n in ("C", "pts3d", "cameras", "cam_model", "pairs_to_triangulate", "camera_centers")],
        "compute_camera_weights": [("C", inspect.Parameter.empty), ("C_reproj", inspect.Parameter.empty), ("connectivity_matrix", None)],
        "order_tracks": [("C", inspect.Parameter.empty), ("C_scale", inspect.Parameter.empty), ("C_reproj", inspect.Parameter.empty), ("priority", prio)],
        "select_best_tracks": [("C", inspect.Parameter.empty), ("C_scale", inspect.Parameter.empty), ("C_reproj", inspect.Parameter.empty),
                               ("K", 30), ("priority", prio), ("verbose", False)],
        "select_best_tracks_sensor_aware": [("images", inspect.Parameter.empty), ("C", inspect.Parameter.empty), ("C_scale", inspect.Parameter.empty),
                                            ("C_reproj", inspect.Parameter.empty), ("K", 30), ("priority", prio), ("verbose", False)],
    }
    for fname, params in expected.items():
        sig = inspect.signature(getattr(ft_ranking, fname))
        assert [(p.name, p.default) for p in sig.parameters.values()] == params, fname
    sig = inspect.signature(ft_ranking.select_best_tracks_from_observations)
    assert list(sig.parameters)[:9] == ["pts_ind", "cam_ind", "scale", "err", "n_cam", "n_pts", "K", "priority", "return_info"]
    assert sig.parameters["return_info"].default is False


def test_library_declares_the_track_entries_and_version_5():
    lib = engine_hip.load_library()
    assert lib.satba_version() == 5
    for sym in ("satba_track_keys", "satba_track_connectivity", "satba_select_tracks"):
        assert sym in engine_hip.SYMBOLS and hasattr(lib, sym)


def test_argument_errors_are_raised_on_the_host():
    """ValueError before a device is needed: these hold with or without a GPU."""
    f = ft_ranking.select_best_tracks_from_observations
    pts, cam, sc = [0, 0, 1, 1], [0, 1, 0, 2], [1.0, 2.0, 3.0, 4.0]
    with pytest.raises(ValueError):
        f(pts, cam, sc, None, 3, 2, K=2, priority=["length", "size"])  # unknown priority name
    with pytest.raises(ValueError):
        f(pts, cam, sc, None, 3, 2, K=2, priority=["cost", "cost"])
    with pytest.raises(ValueError):
        f(pts, cam[:3], sc, None, 3, 2, K=2)  # ragged lists
    with pytest.raises(ValueError):
        f(pts, cam, sc[:3], None, 3, 2, K=2)
    with pytest.raises(ValueError):
        f(pts, cam, sc, [0.1, 0.2], 3, 2, K=2)
    with pytest.raises(ValueError):
        f(pts, cam, sc, None, 3, 2, K=-1)  # K < 0
    with pytest.raises(ValueError):
        f(pts, [0, 1, 0, 3], sc, None, 3, 2, K=2)  # camera out of range
    with pytest.raises(ValueError):
        f([0, 0, 1, 2], cam, sc, None, 3, 2, K=2)  # track out of range
    with pytest.raises(ValueError):
        f([0, 0, 1, 1], [0, 0, 0, 2], sc, None, 3, 2, K=2)  # one observation twice
    C = CT.dense(np.array(pts), np.array(cam), 3, 2)
    with pytest.raises(ValueError):
        ft_ranking.select_best_tracks(C, np.zeros((3, 2)), CT.dense(np.array(pts), np.array(cam), 3, 2, np.ones(4)))  # C_scale without NaN
    with pytest.raises(ValueError):
        ft_ranking.build_connectivity_matrix(np.zeros((3, 2)))  # odd number of rows


def test_the_c_entries_validate_their_arguments():
    """SATBA_E_ARG (-1) from the entries themselves, before a device is touched."""
    import ctypes as C

    lib = engine_hip.load_library()
    lp, ip, dp = C.POINTER(C.c_int64), engine_hip._ip, engine_hip._dp
    ofs = np.array([0, 2, 4], dtype=np.int64)
    cam = np.array([0, 1, 0, 2], dtype=np.int32)
    sc = np.ones(4)
    tree = np.zeros(2, dtype=np.int32)
    n_sel, n_trees = C.c_int64(), C.c_int32()

    def select(ofs=ofs, cam=cam, K=2, prio=(0, 1, 2), n_cam=3):
        pr = np.array(prio, dtype=np.int32)
        return lib.satba_select_tracks(n_cam, 2, ofs.ctypes.data_as(lp), cam.ctypes.data_as(ip), sc.ctypes.data_as(dp), None, K,
                                       pr.ctypes.data_as(ip), tree.ctypes.data_as(ip), C.byref(n_sel), C.byref(n_trees), None, None, 0, None)

    assert select(K=-1) == -1
    assert select(prio=(0, 3, -1)) == -1 and select(prio=(1, 1, -1)) == -1
    assert select(cam=np.array([1, 0, 0, 2], dtype=np.int32)) == -1  # cameras must ascend inside a track
    assert select(cam=np.array([0, 1, 0, 3], dtype=np.int32)) == -1
    assert select(ofs=np.array([0, 3, 2], dtype=np.int64)) == -1
    assert select(n_cam=0) == -1
    A = np.zeros((3, 3), dtype=np.int32)
    assert lib.satba_track_connectivity(3, 2, ofs.ctypes.data_as(lp), cam.ctypes.data_as(ip), None, 0, None, 0) == -1
    assert lib.satba_track_connectivity(3, 2, np.array([1, 2, 4], dtype=np.int64).ctypes.data_as(lp), cam.ctypes.data_as(ip), None, 0,
                                        A.ctypes.data_as(ip), 0) == -1
    assert lib.satba_track_keys(2, ofs.ctypes.data_as(lp), None, None, tree.ctypes.data_as(ip), sc.ctypes.data_as(dp), sc.ctypes.data_as(dp), 0) == -1


def test_selection_fails_loudly_without_library_or_device(tmp_path, monkeypatch):
    """No CPU fallback: a missing library is an OSError, a missing device a runtime error -- never a silent result."""
    import torch

    pts, cam, sc, er = CT.random_tracks(5, 21, 3)
    if not torch.cuda.is_available():
        with pytest.raises((engine_hip.SatbaError, RuntimeError)):
            ft_ranking.select_best_tracks_from_observations(pts, cam, sc, er, 5, 21, K=2)
        with pytest.raises((engine_hip.SatbaError, RuntimeError)):
            ft_ranking.build_connectivity_matrix(CT.dense(pts, cam, 5, 21))
        with pytest.raises((engine_hip.SatbaError, RuntimeError)):
            ft_ranking.order_tracks(CT.dense(pts, cam, 5, 21), CT.dense(pts, cam, 5, 21, sc), CT.dense(pts, cam, 5, 21, er))
    monkeypatch.setattr(engine_hip, "_LIB", None)
    monkeypatch.setattr(engine_hip, "LIB_PATH", str(tmp_path / "libsatba_hip.so"))
    with pytest.raises(OSError):
        ft_ranking.select_best_tracks_from_observations(pts, cam, sc, er, 5, 21, K=2)

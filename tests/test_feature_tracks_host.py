"""Track construction (satba.ft_utils): what can be checked without a device -- the rule, the fixtures, the surface, the argument checks."""
import ctypes as C
import inspect

import numpy as np
import pytest

import cases_ft as CF
from satba import engine_hip, ft_utils

FT_SYMBOLS = ("satba_ftracks_build", "satba_ftracks_fetch", "satba_ftracks_destroy", "satba_tracks_have_pair")


@pytest.fixture(scope="module")
def golden():
    return CF.load()


def test_golden_file_holds_only_numeric_arrays_of_every_case(golden):
    for key in golden.files:
        assert golden[key].dtype.kind in "iuf", key
    for name in CF.GOLDEN_CASES:
        for field in ("kp", "kp_ofs", "matches", "pairs", "C", "C_v2"):
            assert name + "_" + field in golden.files, (name, field)
        assert golden[name + "_kp"].dtype == np.float32 and golden[name + "_kp"].shape[1] == 3
        m = golden[name + "_matches"]
        assert np.all(m[:, 2] < m[:, 3])  # what the reference's matcher produces
    for name in CF.PRE_CASES:
        assert golden[name + "_C_pre"].shape[1] > golden[name + "_C"].shape[1] == golden[name + "_keep"].size  # the check drops some


@pytest.mark.parametrize("name", CF.GOLDEN_CASES)
def test_generators_reproduce_the_stored_inputs(golden, name):
    made, stored = CF.make(name), CF.from_golden(golden, name)
    for k in stored:
        assert np.array_equal(made[k], stored[k]) and made[k].dtype == stored[k].dtype, k


@pytest.mark.parametrize("name", CF.GOLDEN_CASES)
def test_numpy_rule_reproduces_the_reference(golden, name):
    """Pins the rule of DESIGN.md section 4j on the reference, independently of any GPU: the arrays are equal after the canonical sort."""
    case = CF.from_golden(golden, name)
    n_cam = case["kp_ofs"].size - 1
    r = CF.rule(**case)
    Cm, V = CF.dense(r["pts_ind"], r["cam_ind"], r["pts2d"], r["kp_id"], n_cam, r["n_pts"])
    assert CF.same(Cm, V, golden[name + "_C"], golden[name + "_C_v2"])
    assert np.all(np.diff(r["pts_ind"]) >= 0)
    same_track = np.diff(r["pts_ind"]) == 0
    assert np.all(np.diff(r["cam_ind"])[same_track] > 0)  # cameras ascend strictly inside a track
    if name + "_C_pre" in golden.files:
        pre = CF.rule(**case, baseline=False)
        Cp, Vp = CF.dense(pre["pts_ind"], pre["cam_ind"], pre["pts2d"], pre["kp_id"], n_cam, pre["n_pts"])
        assert CF.same(Cp, Vp, golden[name + "_C_pre"], golden[name + "_C_v2_pre"])
        assert pre["n_pts"] == r["n_components"] == golden[name + "_C_pre"].shape[1]


def test_scenes_have_the_properties_the_gpu_tests_rely_on(golden):
    name = CF.SCENE8[0]
    r = CF.rule(**CF.from_golden(golden, name))
    assert r["n_conflicts"] > 0 and r["n_components"] > r["n_pts"] > 0
    assert golden[name + "_matches"].shape[0] > 40 * 256  # dozens of workgroups of match rows
    clean = CF.scene(6, 400, 300, seed=5, false_frac=0.0)
    assert CF.rule(**clean)["n_conflicts"] == 0
    ch = CF.from_golden(golden, CF.CHAIN)
    rc = CF.rule(**ch)
    assert rc["n_pts"] == 4 and np.array_equal(np.bincount(rc["pts_ind"]), [64] * 4)


def test_ft_utils_exposes_the_reference_signatures():
    """Parameter names and defaults of ref:bundle_adjust/feature_tracks/ft_utils.py:38,65 and ft_ranking.py:37."""
    empty = inspect.Parameter.empty
    expected = {
        "feature_tracks_from_pairwise_matches": [("feature_paths", empty), ("pairwise_matches", empty), ("pairs_to_triangulate", empty)],
        "filter_C_using_pairs_to_triangulate": [("C", empty), ("pairs_to_triangulate", empty)],
        "compute_C_scale": [("C_v2", empty), ("features", empty)],
    }
    for fname, params in expected.items():
        sig = inspect.signature(getattr(ft_utils, fname))
        assert [(p.name, p.default) for p in sig.parameters.values()] == params, fname
    sig = inspect.signature(ft_utils.feature_tracks_from_matches)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("kp", empty), ("kp_ofs", empty), ("pairwise_matches", empty), ("pairs_to_triangulate", empty), ("n_cam", None), ("n_adj", 0),
        ("device", None), ("return_info", False)]


def test_library_declares_the_track_construction_entries_and_version_5():
    lib = engine_hip.load_library()
    assert lib.satba_version() == 5
    for sym in FT_SYMBOLS:
        assert sym in engine_hip.SYMBOLS and hasattr(lib, sym), sym


def test_compute_C_scale_is_a_gather(tmp_path):
    rng = np.random.default_rng(3)
    paths, feats = [], []
    for m, n in enumerate((5, 9, 7)):
        f = rng.random((n, 6)).astype(np.float32)
        paths.append(str(tmp_path / "{}.npy".format(m)))
        np.save(paths[-1], f)
        feats.append(f)
    C_v2 = np.array([[0, np.nan, 4, 2], [8, 3, np.nan, np.nan], [np.nan, 6, 0, 1]], dtype=np.float64)
    S = ft_utils.compute_C_scale(C_v2, paths)
    assert S.dtype == np.float64 and np.array_equal(np.isnan(S), np.isnan(C_v2))
    for cam in range(3):
        for t in range(4):
            if not np.isnan(C_v2[cam, t]):
                assert S[cam, t] == np.float64(feats[cam][int(C_v2[cam, t]), 2])


def test_argument_errors_are_raised_on_the_host(tmp_path):
    """ValueError before a device is needed: these hold with or without a GPU."""
    f = ft_utils.feature_tracks_from_matches
    kp = np.zeros((7, 3), dtype=np.float32)
    ofs = [0, 3, 7]
    ok = [[0, 1, 0, 1]]
    pairs = [(0, 1)]
    with pytest.raises(ValueError):
        f(kp, ofs, [[3, 1, 0, 1]], pairs)  # a keypoint index outside its image
    with pytest.raises(ValueError):
        f(kp, ofs, [[0, 4, 0, 1]], pairs)
    with pytest.raises(ValueError):
        f(kp, ofs, [[0, 1, 0, 2]], pairs)  # an image >= n_cam
    with pytest.raises(ValueError):
        f(kp, ofs, [[0, 1, 1, 1]], pairs)  # im_i == im_j
    with pytest.raises(ValueError):
        f(kp, [0, 5, 3, 7], ok, pairs)  # kp_ofs not ascending
    with pytest.raises(ValueError):
        f(kp, [1, 3, 7], ok, pairs)  # ... from 0
    with pytest.raises(ValueError):
        f(kp, [0, 3, 6], ok, pairs)  # ragged: kp and kp_ofs disagree
    with pytest.raises(ValueError):
        f(kp, ofs, [[0, 1, 0]], pairs)  # a wrong column count
    with pytest.raises(ValueError):
        f(kp[:, :2], ofs, ok, pairs)
    with pytest.raises(ValueError):
        f(kp, ofs, [[0, -1, 0, 1]], pairs)  # negative indices
    with pytest.raises(ValueError):
        f(kp, ofs, [[0, 1, -1, 1]], pairs)
    with pytest.raises(ValueError):
        f(kp, ofs, ok, pairs, n_cam=3)
    with pytest.raises(ValueError):
        f(kp, ofs, ok, pairs, n_adj=-1)
    with pytest.raises(ValueError):
        ft_utils.filter_C_using_pairs_to_triangulate(np.zeros((3, 2)), pairs)  # odd number of rows
    path = str(tmp_path / "two_columns.npy")
    np.save(path, np.zeros((4, 2), dtype=np.float32))
    with pytest.raises(ValueError):
        ft_utils.feature_tracks_from_pairwise_matches([path, path], np.array(ok), pairs)


def test_the_c_entries_validate_their_arguments():
    """SATBA_E_ARG (-1) from the entries themselves, before anything is launched."""
    lib = engine_hip.load_library()
    lp, ip, fp = C.POINTER(C.c_int64), engine_hip._ip, C.POINTER(C.c_float)
    kp = np.zeros((7, 3), dtype=np.float32)
    pairs = np.array([[0, 1]], dtype=np.int32)
    counts = np.zeros(5, dtype=np.int64)

    def build(ofs=(0, 3, 7), row=(0, 1, 0, 1), n_cam=2, n_matches=1):
        ofs = np.array(ofs, dtype=np.int64)
        m = np.array([row], dtype=np.int32)
        h = C.c_void_p(None)
        rc = lib.satba_ftracks_build(n_cam, ofs.ctypes.data_as(lp), kp.ctypes.data_as(fp), n_matches, m.ctypes.data_as(ip), 1, pairs.ctypes.data_as(ip),
                                     0, C.byref(h), counts.ctypes.data_as(lp), 0, None)
        assert h.value is None or rc == 0
        return rc

    assert build(row=(3, 1, 0, 1)) == -1 and build(row=(0, 4, 0, 1)) == -1 and build(row=(-1, 1, 0, 1)) == -1
    assert build(row=(0, 1, 0, 2)) == -1 and build(row=(0, 1, -1, 1)) == -1
    assert build(row=(0, 1, 1, 1)) == -1
    assert b"image 1" in lib.satba_last_error()
    assert build(ofs=(0, 8, 7)) == -1 and build(ofs=(1, 3, 7)) == -1
    assert build(n_cam=0) == -1 and build(n_matches=-1) == -1
    assert build(ofs=(0, 3, 2 ** 31)) == -1 and build(n_matches=2 ** 31) == -1  # the limits, refused before any row is read
    assert b"2^31" in lib.satba_last_error()
    assert lib.satba_ftracks_fetch(None, None, None, None, None, None) == -1
    lib.satba_ftracks_destroy(None)
    ofs = np.array([0, 2, 4], dtype=np.int64)
    keep = np.zeros(2, dtype=np.uint8)
    bp = C.POINTER(C.c_uint8)

    def have(cam=(0, 1, 0, 2), ofs=ofs, n_cam=3, keep=keep):
        cam = np.array(cam, dtype=np.int32)
        return lib.satba_tracks_have_pair(n_cam, 2, ofs.ctypes.data_as(lp), cam.ctypes.data_as(ip), 1, pairs.ctypes.data_as(ip),
                                          keep.ctypes.data_as(bp) if keep is not None else None, 0)

    assert have(cam=(1, 0, 0, 2)) == -1 and have(cam=(0, 3, 0, 2)) == -1
    assert have(ofs=np.array([0, 3, 2], dtype=np.int64)) == -1 and have(n_cam=0) == -1 and have(keep=None) == -1


def test_construction_fails_loudly_without_library_or_device(tmp_path, monkeypatch):
    """No CPU fallback: a missing library is an OSError, a missing device a runtime error -- never a silent result."""
    import torch

    case = CF.random_small(2)
    if not torch.cuda.is_available():
        with pytest.raises((engine_hip.SatbaError, RuntimeError)):
            ft_utils.feature_tracks_from_matches(case["kp"], case["kp_ofs"], case["matches"], case["pairs"])
    monkeypatch.setattr(engine_hip, "_LIB", None)
    monkeypatch.setattr(engine_hip, "LIB_PATH", str(tmp_path / "libsatba_hip.so"))
    with pytest.raises(OSError):
        ft_utils.feature_tracks_from_matches(case["kp"], case["kp_ofs"], case["matches"], case["pairs"])

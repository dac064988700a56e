"""
Refinement of the intrinsics (correction_params ["R", "T", "K"], option K_init="camera"), host side: packing, unpacking, the
option checks and the outlier rebuilds, against the reference's own outputs (tests/golden/fun_*_RTK.npz,
tools/gen_golden_intrinsics.py).  No GPU.
"""
import numpy as np
import pytest

import cases_intrinsics as CI
from satba import ba_core, ba_outliers, ba_params, cam_utils, synth

N_K = {"affine": 3, "perspective": 5}


def _params(name, dense=True):
    return synth.make_params(CI.scene(name), CI.options(name), dense=dense)


def _host_fun(v, p):
    pts3d, cam_params = p.get_vars_ready_for_fun(v.copy())
    proj = (ba_core.project_affine if p.cam_model == "affine" else ba_core.project_perspective)(pts3d, cam_params, p.pts_ind, p.cam_ind)
    return np.repeat(p.pts2d_w, 2) * (proj - p.pts2d).ravel()


@pytest.mark.parametrize("name", list(CI.FUN_CASES))
def test_packing_starts_k_from_the_cameras(name):
    g = CI.golden("fun_" + name)
    p = _params(name)
    model = CI.FUN_CASES[name][0]
    assert p.n_params == int(g["n_params"]) == (8 if model == "affine" else 11)
    assert p.K_init == "camera"
    assert np.array_equal(p.pts_ind, g["pts_ind"]) and np.array_equal(p.cam_ind, g["cam_ind"])
    # (the camera decompositions agree to the last bits, not bit for bit)
    np.testing.assert_allclose(p.cam_params, g["cam_params"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(p.params_opt, g["v0"], rtol=1e-13, atol=0)
    assert np.array_equal(p.params_opt, CI.corrected_start(p.cam_params, p.pts3d, p.n_params))
    # the one deliberate deviation: the reference's start vector repeats T where K belongs
    n_c = p.n_cam * p.n_params
    differs = ~np.isclose(p.params_opt, g["params_opt"], rtol=1e-13, atol=0)
    cols = np.zeros((p.n_cam, p.n_params), dtype=bool)
    cols[:, p.n_params - N_K[model]:] = True
    assert not differs[n_c:].any()
    assert not differs[:n_c][~cols.ravel()].any()
    assert differs[:n_c][cols.ravel()].all()


@pytest.mark.parametrize("name", list(CI.FUN_CASES))
def test_sparse_entry_point_packs_the_same(name):
    pd, ps = _params(name, True), _params(name, False)
    assert ps.n_params == pd.n_params
    np.testing.assert_array_equal(ps.params_opt, pd.params_opt)


@pytest.mark.parametrize("name", list(CI.FUN_CASES))
def test_host_fun_matches_reference(name):
    g = CI.golden("fun_" + name)
    p = _params(name)
    for v, r in zip(g["v"], g["r"]):
        assert np.abs(_host_fun(v, p) - r).max() < 1e-8


@pytest.mark.parametrize("name", list(CI.FUN_CASES))
def test_sparsity_matches_reference(name):
    g = CI.golden("fun_" + name)
    A = ba_core.build_jacobian_sparsity(_params(name)).tocsr()
    assert tuple(A.shape) == tuple(g["A_shape"])
    np.testing.assert_array_equal(A.indptr, g["A_indptr"])
    np.testing.assert_array_equal(A.indices, g["A_indices"])


@pytest.mark.parametrize("name", list(CI.FUN_CASES))
def test_unpack_round_trip_and_cameras(name):
    g = CI.golden("fun_" + name)
    p = _params(name)
    v = g["v"][2].copy()
    pts3d, cam_params = p.get_vars_ready_for_fun(v.copy())
    n_c = p.n_cam * p.n_params
    opt = v[:n_c].reshape(p.n_cam, p.n_params).copy()
    opt[: p.n_cam_fix] = p.cam_params[: p.n_cam_fix, : p.n_params]
    np.testing.assert_array_equal(cam_params[:, : p.n_params], opt)
    np.testing.assert_array_equal(cam_params[:, p.n_params:], p.cam_params[:, p.n_params:])
    cams = [None] * p.n_cam
    _, cameras = p.reconstruct_vars(v.copy(), p.pts3d.copy(), cams)
    for i in range(p.n_cam):
        row = cam_params[i]
        R = ba_params.ba_rotate.euler_angles_to_R(*row[:3])
        if p.cam_model == "affine":
            P = cam_utils.compose_affine_camera(np.array([[row[5], row[7]], [0, row[6]]]), R, row[3:5])
        else:
            K = np.array([[row[6], row[8], row[9]], [0, row[7], row[10]], [0, 0, 1.0]])
            P = K @ np.hstack((R, row[3:6].reshape(3, 1)))
        np.testing.assert_allclose(cameras[i], P / P[2, 3], rtol=1e-12, atol=0)
        # the refined K comes back out of the composed camera
        back = ba_params.load_cam_params_from_camera(cameras[i], p.camera_centers[i], p.cam_model)
        np.testing.assert_allclose(back[3 + (2 if p.cam_model == "affine" else 3):], row[p.n_params - N_K[p.cam_model]: p.n_params], rtol=1e-7)
    assert set(p.estimated_params[0]) == {"R", "T"}


def test_options_that_stay_errors():
    sc = CI.scene("affine_RTK")
    d = {"correction_params": ["R", "T", "K"]}
    with pytest.raises(ba_params.Error, match="K_init"):  # no opt-in: the reference's start cannot be reproduced
        ba_params.BundleAdjustmentParameters.from_observations(sc.pts_ind, sc.cam_ind, sc.pts2d, sc.pts3d, sc.cameras, "affine",
                                                               sc.pairs_to_triangulate, sc.camera_centers, dict(d, verbose=False))
    for bad in ({"correction_params": ["R", "T", "K", "COMMON_K"], "K_init": "camera"},
                {"correction_params": ["R", "T", "K"], "K_init": "reference"},
                {"correction_params": ["R", "T"], "K_init": "nonsense"}):
        with pytest.raises(ba_params.Error):
            synth.make_params(sc, bad)
    rpc = synth.make_scene("rpc", 3, 40, 2, seed=7)
    with pytest.raises(ba_params.Error):
        synth.make_params(rpc, {"correction_params": ["R", "T", "K"], "K_init": "camera"})


def test_k_without_t_optimises_r_alone():
    sc = CI.scene("affine_RTK")
    p = synth.make_params(sc, {"correction_params": ["R", "K"], "K_init": "camera"})
    q = synth.make_params(sc, {"correction_params": ["R"]})
    assert p.n_params == 3
    np.testing.assert_array_equal(p.params_opt, q.params_opt)


@pytest.mark.parametrize("dense", [True, False])
def test_outlier_rebuilds_keep_k(dense):
    sc = synth.make_scene("affine", 5, 200, 4, seed=3, sigma_k=1e-3)
    p = synth.make_params(sc, {"correction_params": ["R", "T", "K"], "K_init": "camera", "n_cam_fix": 1}, dense=dense)
    assert ba_outliers._options_like(p, 0, False)["K_init"] == "camera"
    if dense:
        C = p.C.copy()
        C[:2, 0] = np.nan
        new_p = ba_outliers.reset_ba_params_after_outlier_removal(C, p, verbose=False, pts3d=p.pts3d)
        assert new_p.n_params == 8 and new_p.K_init == "camera"
        np.testing.assert_array_equal(new_p.params_opt[: new_p.n_cam * 8], p.params_opt[: p.n_cam * 8])


def test_scene_k_error_is_opt_in():
    for model in ("affine", "perspective"):
        a = synth.make_scene(model, 6, 300, 4, seed=9)
        b = synth.make_scene(model, 6, 300, 4, seed=9, sigma_k=1e-2)
        for k in ("pts3d", "pts2d", "pts_ind", "cam_ind"):
            assert np.array_equal(getattr(a, k), getattr(b, k))
        for ca, cb in zip(a.cameras, b.cameras):
            ra = ba_params.load_cam_params_from_camera(ca, np.zeros(3), model)
            rb = ba_params.load_cam_params_from_camera(cb, np.zeros(3), model)
            nt = 5 if model == "affine" else 6
            np.testing.assert_allclose(ra[:3], rb[:3], atol=1e-9)  # same rotation ...
            assert np.abs(ra[nt:] - rb[nt:]).max() > 0  # ... another K
        assert all(np.array_equal(x, y) for x, y in zip(a.cameras_true, b.cameras_true))
    assert "C3K" in synth.CONFIGS and synth.CONFIGS["P3K"][1] == ["R", "T", "K"]
    # the named K configs opt in by themselves (bench.py --shape C3K); a plain list does not
    assert synth.make_params(a, {"correction_params": synth.CONFIGS["P3K"][1]}).n_params == 11
    with pytest.raises(ba_params.Error):
        synth.make_params(a, {"correction_params": ["R", "T", "K"]})

"""
Host-side checks of the RPC -> affine / perspective camera approximation (no device): the numpy restatement of the device's
resection against the reference's vectors (the yardstick of the GPU tolerances, printed), the oracle composition of the affine
route against central differences, the argument checks of the C ABI and the Python wrappers' shape handling.
"""
import ctypes as C

import numpy as np
import pytest

import cases_camapprox as CC
from satba import cam_utils, engine_hip

E_ARG, E_NONFINITE = -1, -4


def test_restatement_matches_the_reference_vectors():
    """Reprojection of the stored points through both matrices and the optical centre.  These distances times 20 are the bounds of
    the device tests; they must leave the caps of 1e-6 px and 1e-2 m alone (measured: <= 1.2e-9 px, <= 1.8e-5 m)."""
    g = CC.load_golden()
    for name, (X, x, crop) in CC.resection_inputs().items():
        assert np.array_equal(X, g["res_{}_X".format(name)]) and np.array_equal(x, g["res_{}_x".format(name)]), name
        P, err, centre = CC.resect(X, x)
        Pg = g["res_{}_P".format(name)]
        d_px, d_m = CC.reprojection_distance(P, Pg, X), np.abs(centre - CC.centre_of(Pg)).max()
        print("resection {:8s} n = {:4d}: reprojection {:.3e} px, centre {:.3e} m, mean_err {:.3e} px".format(name, len(X), d_px, d_m, err))
        assert d_px <= CC.PX_CAP / CC.MARGIN and d_m <= CC.CENTRE_CAP / CC.MARGIN, (name, d_px, d_m)
    assert CC.resect(*CC.exact_camera())[1] < 1e-9
    for f, cname in CC.FULL_ROUTE:
        r, crop = CC.rpc(f), CC.CROPS[cname]
        X, x = CC.mesh_correspondences(r, *CC.perspective_ranges(r, crop))
        P, err, centre = CC.resect(X, x)
        key = "full_{}_{}".format(f, cname)
        d_img = CC.reprojection_distance(P, g[key + "_Pimg"], X)
        d_px = CC.reprojection_distance(CC.to_crop(P, crop), g[key + "_P"], X)
        d_m = np.abs(centre - g[key + "_centre"]).max()
        print("full route {:6s} {}: reprojection {:.3e} px (crop coordinates {:.3e}), centre {:.3e} m, mean_err {:.3e} vs {:.3e} px".format(
            cname, f, d_img, d_px, d_m, err, float(g[key + "_err"])))
        assert max(d_img, d_px) <= CC.PX_CAP / CC.MARGIN and d_m <= CC.CENTRE_CAP / CC.MARGIN, (key, d_img, d_px, d_m)
        assert abs(err - float(g[key + "_err"])) <= 1e-9


def test_normal_matrix_is_the_gram_matrix_of_the_reference_system():
    X, x, _ = CC.resection_inputs()["crop"]
    Xn, _ = cam_utils.normalize_3d_points(X)
    xn, _ = cam_utils.normalize_2d_points(x)
    # the system of ref:bundle_adjust/cam_utils.py:338-343: rows (0, -Xh, y Xh) and (Xh, 0, -x Xh) per correspondence
    Xh = np.hstack([Xn, np.ones((len(Xn), 1))])
    A = np.zeros((2 * len(Xn), 12))
    A[0::2, 4:8], A[0::2, 8:12] = -Xh, xn[:, 1:2] * Xh
    A[1::2, 0:4], A[1::2, 8:12] = Xh, -xn[:, 0:1] * Xh
    N = CC.normal_matrix(Xn, xn)
    assert np.abs(N - A.T @ A).max() <= 1e-13 * np.abs(N).max()
    lam, V = CC.jacobi_eigh(N)
    assert np.abs(V.T @ V - np.eye(12)).max() < 1e-14 and np.abs(V @ np.diag(lam) @ V.T - N).max() <= 1e-13 * np.abs(N).max()
    assert abs(np.mean(np.linalg.norm(Xn, axis=1)) - np.sqrt(3)) < 1e-14 and abs(np.mean(np.linalg.norm(xn, axis=1)) - np.sqrt(2)) < 1e-14


def test_affine_composition_against_central_differences():
    """The oracle's chained Jacobian is the derivative the reference takes with `ad`: central differences of the oracle projection
    agree within the bound derived from its third derivative and the rounding of one evaluation (cases_camapprox.fd_step_and_bound)."""
    for f in (0, 1):
        r = CC.rpc(f)
        for p in CC.expansion_points(r):
            h, bound = CC.fd_step_and_bound(r, p)
            Pe, Pf = CC.affine_expected(r, p), CC.affine_fd(r, p, h)
            d = np.abs(Pe[:2, :3] - Pf[:2, :3]).max()
            print("affine rpc {}: step {:.2f} m, |J - J_fd| = {:.3e} px/m (bound {:.3e}), yardstick {}".format(f, h, d, bound, CC.affine_yardstick(r, p)))
            assert d <= bound
            q = CC.rpc_oracle(r, p)[0][0]
            assert np.abs(Pe[:2, :3] @ p + Pe[:2, 3] - q).max() < 1e-8 and np.array_equal(Pe[2], [0, 0, 0, 1])
            Pc = CC.affine_expected(r, p, 120.0, 75.0)
            assert np.array_equal(Pc[:2, :3], Pe[:2, :3]) and np.abs(Pc[:2, 3] - (Pe[:2, 3] - [120.0, 75.0])).max() < 1e-8


def _lib():
    return engine_hip.load_library()


def _p(a):
    return engine_hip._ptr(np.ascontiguousarray(a, dtype=np.float64))


def test_c_abi_argument_errors_come_before_any_device_call():
    lib = _lib()
    tab = np.stack([CC.rpc(0).to_table(), CC.rpc(1).to_table()])
    cr, rr, ar = np.array([[0.0, 3200.0]] * 2), np.array([[0.0, 1350.0]] * 2), np.array([[3400.0, 3600.0]] * 2)
    P, err, cen = np.zeros((2, 12)), np.zeros(2), np.zeros((2, 3))
    xyz, c0 = np.array(CC.expansion_points(CC.rpc(0))), np.zeros((2, 2))

    def persp(n_cam=2, tables=tab, col=cr, row=rr, alt=ar, n=(10, 10, 10), crop0=c0, out=P):
        return lib.satba_rpc_perspective_approx(n_cam, _p(tables) if tables is not None else None, _p(col) if col is not None else None, _p(row), _p(alt),
                                                n[0], n[1], n[2], _p(crop0) if crop0 is not None else None, _p(out) if out is not None else None,
                                                _p(err), _p(cen), 0)

    assert persp(tables=None) == E_ARG and persp(col=None) == E_ARG and persp(out=None) == E_ARG
    assert persp(n_cam=-1) == E_ARG
    assert persp(n=(1, 10, 10)) == E_ARG and persp(n=(10, 1, 10)) == E_ARG and persp(n=(10, 10, 1)) == E_ARG and persp(n=(0, 0, 0)) == E_ARG
    assert persp(n=(1024, 1024, 2)) == E_ARG  # 2^21 nodes: above the documented 2^20
    assert b"1048576" in lib.satba_last_error()
    bad = tab.copy(); bad[1, 17] = np.nan
    assert persp(tables=bad) == E_NONFINITE
    assert persp(col=np.array([[0.0, 3200.0], [0.0, np.inf]])) == E_NONFINITE
    assert persp(crop0=np.array([[0.0, np.nan], [0.0, 0.0]])) == E_NONFINITE
    # degenerate: a mesh axis of zero extent (a zero-width crop) is refused, not resected
    assert persp(col=np.array([[0.0, 3200.0], [500.0, 500.0]])) == E_NONFINITE and b"Singular matrix" in lib.satba_last_error()
    assert persp(alt=np.array([[3500.0, 3500.0], [3400.0, 3600.0]])) == E_NONFINITE

    def affine(n_cam=2, tables=tab, pts=xyz, crop=c0, out=P):
        return lib.satba_rpc_affine_approx(n_cam, _p(tables) if tables is not None else None, _p(pts) if pts is not None else None,
                                           _p(crop) if crop is not None else None, _p(out) if out is not None else None, 0)

    assert affine(tables=None) == E_ARG and affine(pts=None) == E_ARG and affine(crop=None) == E_ARG and affine(out=None) == E_ARG
    assert affine(n_cam=-3) == E_ARG
    assert affine(tables=bad) == E_NONFINITE and affine(pts=np.array([[1.0, 2.0, np.inf], [1.0, 2.0, 3.0]])) == E_NONFINITE

    X, x = np.random.RandomState(0).rand(2, 6, 3), np.random.RandomState(1).rand(2, 6, 2)

    def resect(n_cam=2, n_pts=6, Xa=X, xa=x, out=P):
        return lib.satba_camera_resection(n_cam, n_pts, _p(Xa) if Xa is not None else None, _p(xa) if xa is not None else None,
                                          _p(out) if out is not None else None, None, 0)

    assert resect(Xa=None) == E_ARG and resect(xa=None) == E_ARG and resect(out=None) == E_ARG
    assert resect(n_cam=-1) == E_ARG and resect(n_pts=-1) == E_ARG and resect(n_pts=5) == E_ARG and resect(n_pts=0) == E_ARG
    Xb = X.copy(); Xb[1, 5, 2] = np.nan
    assert resect(Xa=Xb) == E_NONFINITE
    assert lib.satba_rpc_mesh(2, _p(tab), _p(cr), _p(rr), _p(ar), 10, 10, 1, _p(np.zeros(6)), _p(np.zeros(4)), None, 0) == E_ARG
    assert lib.satba_rpc_mesh(2, _p(tab), _p(cr), _p(rr), _p(ar), 2, 2, 2, None, _p(np.zeros(4)), None, 0) == E_ARG
    assert np.all(P == 0) and np.all(err == 0) and np.all(cen == 0)  # no output was touched


def test_empty_batch_returns_without_a_device():
    """n_cam == 0 is answered on the host (this test has no device to touch)."""
    lib = _lib()
    z = np.zeros(1)
    assert lib.satba_rpc_affine_approx(0, _p(z), _p(z), _p(z), _p(z), 0) == 0
    assert lib.satba_rpc_perspective_approx(0, _p(z), _p(z), _p(z), _p(z), 10, 10, 10, _p(z), _p(z), None, None, 0) == 0
    assert lib.satba_camera_resection(0, 6, _p(z), _p(z), _p(z), None, 0) == 0
    assert lib.satba_rpc_mesh(0, _p(z), _p(z), _p(z), _p(z), 2, 2, 2, _p(z), _p(z), None, 0) == 0
    assert cam_utils.approx_cameras([], [], "perspective") == [] and cam_utils.approx_cameras([], [], "affine", center=(1.0, 2.0, 3.0)) == []
    cams, info = cam_utils.approx_cameras([], [], "perspective", return_info=True)
    assert cams == [] and info["mean_err"].shape == (0,) and info["centers"].shape == (0, 3)
    assert cam_utils.camera_centers([], []).shape == (0, 3)
    assert cam_utils.camera_matrices(np.zeros((0, 6, 3)), np.zeros((0, 6, 2))).shape == (0, 3, 4)


def test_python_wrappers_check_shapes_and_broadcast():
    r, off = CC.rpc(0), CC.offset(CC.CROPS["full"])
    a = cam_utils._per_camera((1.0, 2.0, 3.0), 4, 3, "center")
    assert a.shape == (4, 3) and a.flags["C_CONTIGUOUS"] and np.array_equal(a[3], [1.0, 2.0, 3.0])
    b = np.arange(12.0).reshape(4, 3)
    assert np.array_equal(cam_utils._per_camera(b, 4, 3, "center"), b)
    for bad in (np.zeros(2), np.zeros((3, 3)), np.zeros((4, 2))):
        with pytest.raises(ValueError):
            cam_utils._per_camera(bad, 4, 3, "center")
    with pytest.raises(ValueError):
        cam_utils.approx_cameras([r, r], [off], "perspective")
    with pytest.raises(ValueError):
        cam_utils.approx_cameras([r], [off], "affine")  # no expansion point
    with pytest.raises(ValueError):
        cam_utils.approx_cameras([r, r], [off, off], "affine", center=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        cam_utils.approx_cameras([r], [off], "pinhole")
    rpcs = cam_utils.approx_cameras([r], [off], "rpc")
    assert rpcs[0] is not r and rpcs[0].col_num == r.col_num
    with pytest.raises(ValueError):
        cam_utils.camera_matrix(np.zeros((7, 3, 1)), np.zeros((7, 2)))
    with pytest.raises(ValueError):
        cam_utils.camera_matrices(np.zeros((1, 7, 3)), np.zeros((1, 8, 2)))
    with pytest.raises(ValueError):
        cam_utils.camera_matrix(np.zeros((5, 3)), np.zeros((5, 2)))  # fewer than 6 correspondences
    with pytest.raises(ValueError):
        cam_utils.approx_rpcs_as_proj_matrices([r, r], [[0, 10, 10], [0, 10, 9]], [0, 10, 10], [0, 10, 10])  # two sample counts in one call
    with pytest.raises(ValueError):
        cam_utils.approx_rpc_as_proj_matrix(r, [0, 10, 2.5], [0, 10, 10], [0, 10, 10])
    with pytest.raises((np.linalg.LinAlgError, ValueError)):
        cam_utils.perspective_rpc_approx(r, {"col0": 10.0, "row0": 0.0, "width": 0.0, "height": 100.0})
    # the mesh ranges of perspective_rpc_approx: 10 samples over the crop and +-100 m
    cr, rr, ar = cam_utils._perspective_ranges([r], [{"col0": 5.0, "row0": 7.0, "width": 100.0, "height": 50.0}])
    assert np.array_equal(cr, [[5.0, 105.0, 10.0]]) and np.array_equal(rr, [[7.0, 57.0, 10.0]]) and np.array_equal(ar, [[r.alt_offset - 100, r.alt_offset + 100, 10.0]])
    # host helpers
    pts = np.random.RandomState(3).rand(30, 3) * [4000.0, 3000.0, 200.0] + [1.9e6, -6.4e6, 1.4e6]
    n3, U = cam_utils.normalize_3d_points(pts)
    assert np.allclose(np.hstack([pts, np.ones((30, 1))]) @ U.T, np.hstack([n3, np.ones((30, 1))]), rtol=0, atol=1e-9)
    n2, T = cam_utils.normalize_2d_points(pts[:, :2])
    assert np.abs(n2.mean(0)).max() < 1e-9 and abs(np.mean(np.linalg.norm(n2, axis=1)) - np.sqrt(2)) < 1e-12 and T[2, 2] == 1.0
    assert list(cam_utils.check_projection_matrices([0.2, 1.5, 0.9, 3.0])) == [1, 3] and len(cam_utils.check_projection_matrices([0.2, 0.5], max_err=1.0)) == 0
    assert list(cam_utils.check_projection_matrices([0.2, 0.5], max_err=0.3)) == [1]


def test_new_symbols_are_declared_and_exported():
    lib = _lib()
    for sym in ("satba_rpc_affine_approx", "satba_rpc_perspective_approx", "satba_camera_resection", "satba_rpc_mesh"):
        assert sym in engine_hip.SYMBOLS and hasattr(lib, sym), sym
        assert getattr(lib, sym).argtypes[-1] is C.c_int32

"""
RPC -> affine / perspective cameras on the device (satba.cam_utils -> csrc/satba_camapprox.h) against the reference's vectors
(tests/golden/cam_approx.npz), the numpy restatement and the oracle composition of tests/cases_camapprox.py.

Bounds.  Resection: 20 x the distance of the restatement to the reference on the same points (two correct float64 routes to the
null vector; the margin covers another Jacobi sweep order and fused multiply-adds), capped at 1e-6 px and 1e-2 m; never on the raw
entries of P, whose scale and sign are arbitrary.  Full route against the reference: the device's localisation may differ from the
oracle's by the 1e-9 deg the project asserts, ~1.1e-4 m on the ground, at ~1 m ground sample 2e-4 px after rounding up.
"""
import functools

import numpy as np
import pytest

import cases_camapprox as CC
from satba import cam_utils, geo_utils

pytestmark = pytest.mark.gpu


def bounds(d_px, d_m):
    return min(CC.MARGIN * d_px, CC.PX_CAP), min(CC.MARGIN * d_m, CC.CENTRE_CAP)


@functools.lru_cache(maxsize=None)
def golden():
    return dict(CC.load_golden())


@functools.lru_cache(maxsize=None)
def resection_yardsticks():
    """name -> (reprojection [px], centre [m]) of the restatement against the reference; computed once"""
    out = {}
    for name, (X, x, _) in CC.resection_inputs().items():
        P, _, centre = CC.resect(X, x)
        Pg = golden()["res_{}_P".format(name)]
        out[name] = (CC.reprojection_distance(P, Pg, X), np.abs(centre - CC.centre_of(Pg)).max())
    return out


@functools.lru_cache(maxsize=None)
def full_route(f, cname):
    """oracle mesh, reference results and the restatement's distance to them for one full-route case; computed once"""
    r, crop = CC.rpc(f), CC.CROPS[cname]
    X, x = CC.mesh_correspondences(r, *CC.perspective_ranges(r, crop))
    P, _, centre = CC.resect(X, x)
    key = "full_{}_{}".format(f, cname)
    g = {k: golden()[key + "_" + k] for k in ("P", "Pimg", "err", "centre")}
    yard = (max(CC.reprojection_distance(P, g["Pimg"], X), CC.reprojection_distance(CC.to_crop(P, crop), g["P"], X)), np.abs(centre - g["centre"]).max())
    return r, crop, X, x, g, yard


@pytest.mark.parametrize("name", ["mesh6_0", "mesh6_1", "crop", "exact", "six"])
def test_camera_matrix_against_reference_vectors(gpu, name):
    X, x, _ = CC.resection_inputs()[name]
    Pg = golden()["res_{}_P".format(name)]
    b_px, b_m = bounds(*resection_yardsticks()[name])
    P, err = cam_utils.camera_matrices(X[None], x[None], return_info=True)
    assert np.array_equal(P[0], cam_utils.camera_matrix(X, x))
    d_px, d_m = CC.reprojection_distance(P[0], Pg, X), np.abs(CC.centre_of(P[0]) - CC.centre_of(Pg)).max()
    h = X @ Pg[:, :3].T + Pg[:, 3]
    err_g = np.mean(np.linalg.norm(x - h[:, :2] / h[:, 2:3], axis=1))
    print("{}: reprojection {:.3e} px (bound {:.3e}), centre {:.3e} m (bound {:.3e}), mean_err {:.3e} px (reference {:.3e})".format(name, d_px, b_px, d_m, b_m, err[0], err_g))
    assert d_px <= b_px and d_m <= b_m
    assert abs(err[0] - err_g) <= b_px + 1e-9  # (the reference's own evaluation of P X at these magnitudes is good to ~1e-9 px)
    if name == "exact":
        assert err[0] < 1e-9


@pytest.mark.parametrize("f,cname", [(0, "full"), (1, "c500"), (0, "c50")])
def test_full_route_equals_its_parts(gpu, f, cname):
    r, crop, _, _, _, yard = full_route(f, cname)
    ranges = CC.perspective_ranges(r, crop)
    P, err = cam_utils.approx_rpc_as_proj_matrix(r, *ranges)
    cols, rows, alts = cam_utils.generate_point_mesh(*ranges)
    Xd, xd, altd = cam_utils.rpc_point_mesh([r], *ranges)
    assert np.array_equal(altd[0], alts) and np.array_equal(xd[0, :, 0], cols) and np.array_equal(xd[0, :, 1], rows)
    lons, lats = r.localization(cols, rows, alts)
    X = np.vstack(geo_utils.latlon_to_ecef_custom(lats, lons, alts)).T
    assert np.abs(Xd[0] - X).max() <= 4e-9  # the same localisation; sincos of the device against numpy's: a few ulp of 6.4e6 m
    P_parts = cam_utils.camera_matrix(X, np.vstack([cols, rows]).T)
    d = CC.reprojection_distance(P, P_parts, X)
    print("{} {}: full route vs parts {:.3e} px (bound {:.3e}), mesh vs host ECEF {:.3e} m".format(f, cname, d, bounds(*yard)[0], np.abs(Xd[0] - X).max()))
    assert d <= bounds(*yard)[0]
    Pv, err_v = cam_utils.approx_rpc_as_proj_matrix(r, *ranges, verbose=True)  # (prints the reference's summary; the same call)
    assert np.array_equal(Pv, P) and err_v == err
    Pc, err_c = cam_utils.perspective_rpc_approx(r, CC.offset(crop))
    assert err_c == err and CC.reprojection_distance(Pc, CC.to_crop(P, crop), X) <= bounds(*yard)[0] and Pc[2, 3] == 1.0


@pytest.mark.parametrize("f,cname", CC.FULL_ROUTE)
def test_full_route_against_reference_vectors(gpu, f, cname):
    r, crop, X, x, g, _ = full_route(f, cname)
    cams, info = cam_utils.approx_cameras([r], [CC.offset(crop)], "perspective", return_info=True)
    d_px = CC.reprojection_distance(cams[0], g["P"], X)
    # centre: the restatement fed with the DEVICE's localisation against the reference (which used the oracle's), x 20
    Xd, xd, _ = cam_utils.rpc_point_mesh([r], *CC.perspective_ranges(r, crop))
    yard_m = np.abs(CC.resect(Xd[0], xd[0])[2] - g["centre"]).max()
    b_m = min(CC.MARGIN * yard_m, CC.CENTRE_CAP)
    d_m = np.abs(info["centers"][0] - g["centre"]).max()
    print("{} {}: reprojection {:.3e} px, mean_err {:.6e} vs {:.6e} px, centre {:.3e} m (bound {:.3e}), device vs oracle mesh {:.3e} m".format(
        f, cname, d_px, info["mean_err"][0], float(g["err"]), d_m, b_m, np.abs(Xd[0] - X).max()))
    assert d_px <= 2e-4 and abs(info["mean_err"][0] - float(g["err"])) <= 2e-4
    assert d_m <= b_m


@pytest.mark.parametrize("f", [0, 1])
def test_affine_against_oracle_composition(gpu, f):
    r = CC.rpc(f)
    rng = np.random.RandomState(5 + f)
    for p in CC.expansion_points(r):
        for col0, row0 in ((0.0, 0.0), (120.0, 75.0)):
            P = cam_utils.affine_rpc_approx(r, p[0], p[1], p[2], {"col0": col0, "row0": row0})
            Pe = CC.affine_expected(r, p, col0, row0)
            yJ, yT = CC.affine_yardstick(r, p, col0, row0)
            dJ, dT = np.abs(P[:2, :3] - Pe[:2, :3]).max() / np.abs(Pe[:2, :3]).max(), np.abs(P[:2, 3] - Pe[:2, 3]).max()
            print("rpc {} offset ({}, {}): J {:.3e} rel (bound {:.3e}), P[:2, 3] {:.3e} px (bound {:.3e})".format(f, col0, row0, dJ, CC.MARGIN * yJ, dT, CC.MARGIN * yT))
            assert dJ <= CC.MARGIN * yJ and dT <= CC.MARGIN * yT
            assert np.array_equal(P[2], [0.0, 0.0, 0.0, 1.0])
        # against the RPC itself within 500 m: the first neglected term, 0.5 d^T H d, with the oracle's second differences
        # (H moves by d / 6e5 m over the ball: 5 % on top)
        H = CC.hessian(r, p)
        d = rng.uniform(-1, 1, (200, 3))
        d *= (500.0 * rng.uniform(0.05, 1, 200) / np.linalg.norm(d, axis=1))[:, None]
        P = cam_utils.affine_rpc_approx(r, p[0], p[1], p[2])
        e = np.abs(cam_utils.apply_projection_matrix(P, p + d) - CC.rpc_oracle(r, p + d)[0])
        bound = 1.05 * 0.5 * np.linalg.norm(H.reshape(2, 9), axis=1)[None, :] * (np.linalg.norm(d, axis=1) ** 2)[:, None] + 1e-8
        print("rpc {}: affine vs RPC within 500 m: {:.3e} px at most (bound there {:.3e})".format(f, e.max(), bound.max()))
        assert np.all(e <= bound) and e.max() > 1e-4  # (the test points do leave the linear range: the bound is not idle)


def expansion_value_error(r, p, col0, row0, q):
    """|P (p, 1) - (q - (col0, row0))| of the device's matrix, the product taken in extended precision so that the figure is the
    matrix's and not this line's"""
    P = cam_utils.affine_rpc_approx(r, p[0], p[1], p[2], {"col0": col0, "row0": row0})
    back = P[:2, :3].astype(np.longdouble) @ p.astype(np.longdouble) + P[:2, 3].astype(np.longdouble)
    return float(np.abs(back - (np.asarray(q, dtype=np.longdouble) - np.array([col0, row0], dtype=np.longdouble))).max())


@pytest.mark.parametrize("f", [0, 1])
def test_affine_reproduces_the_expansion_value(gpu, f):
    """P (p, 1) == q - (col0, row0) to 1e-9 px, q the oracle's float64 projection at p (measured: 3.1e-10, 4.2e-10, 4.7e-10,
    1.9e-10 px at the four points; in the other octants tests/test_gpu_octants.py).

    This holds only because k_cam_affine takes the longitude correctly rounded (cam_atan2_rounded) and rounds it in degrees before
    the offset is taken off, as a float64 evaluation does: one ulp of a longitude of 73 deg
    is 1.6e-9 m on the ground and 2.2e-9 px in the column, and with the device's own atan2 the second point of rpc 0 was one ulp
    off (1.38e-9 px).  The other roundings of a float64 evaluation are worth 2 - 4e-10 px each (one ulp of the latitude or of the
    altitude's 6.4e6 m terms), so the oracle's own q sits 0.5 - 1.2e-9 px from the extended-precision value; the second assertion
    holds the matrix to that value within what one float64 evaluation is good to."""
    r = CC.rpc(f)
    worst = 0.0
    for p in CC.expansion_points(r):
        q = CC.rpc_oracle(r, p)[0][0]
        q_ext = CC.rpc_oracle_extended(r, p)
        eps_f = 4 * np.finfo(float).eps * np.linalg.norm(p) * np.abs(CC.rpc_oracle(r, p)[1][0]).max()  # cases_camapprox.fd_step_and_bound
        for col0, row0 in ((0.0, 0.0), (120.0, 75.0)):
            e, e_ext = expansion_value_error(r, p, col0, row0, q), expansion_value_error(r, p, col0, row0, q_ext)
            print("rpc {} offset ({}, {}): P (p, 1) - q {:.3e} px; against q in extended precision {:.3e} px (one float64 evaluation is good to {:.3e}), "
                  "the oracle's q against it {:.3e} px".format(f, col0, row0, e, e_ext, eps_f, float(np.abs(q - q_ext).max())))
            assert e_ext <= eps_f
            worst = max(worst, e)
    assert worst <= 1e-9


@functools.lru_cache(maxsize=None)
def alone(k):
    """camera k of the 257-camera batch, run alone: affine P, perspective P, mean_err, centre"""
    rpcs, offsets, centers = CC.batch(257)
    Pa = cam_utils.approx_cameras([rpcs[k]], [offsets[k]], "affine", center=centers[k])[0]
    cams, info = cam_utils.approx_cameras([rpcs[k]], [offsets[k]], "perspective", return_info=True)
    return Pa, cams[0], info["mean_err"][0], info["centers"][0]


@pytest.mark.parametrize("n", [1, 2, 65, 257])
def test_batches_are_bitwise_the_single_cameras(gpu, n):
    rpcs, offsets, centers = CC.batch(257)
    rpcs, offsets, centers = rpcs[:n], offsets[:n], centers[:n]
    for _ in range(2):  # and a second run repeats bitwise
        Pa = cam_utils.approx_cameras(rpcs, offsets, "affine", center=centers)
        Pp, info = cam_utils.approx_cameras(rpcs, offsets, "perspective", return_info=True)
        assert len(Pa) == n and len(Pp) == n
        for k in range(n):
            a = alone(k)
            assert np.array_equal(Pa[k], a[0]) and np.array_equal(Pp[k], a[1]), k
            assert info["mean_err"][k] == a[2] and np.array_equal(info["centers"][k], a[3]), k
    if n > 1:  # the cameras differ: a batch that repeated one result would have passed the loop otherwise
        assert not np.array_equal(Pa[0], Pa[1]) and not np.array_equal(Pp[0], Pp[1])
    shared = cam_utils.approx_cameras(rpcs, offsets, "affine", center=centers[0])  # one expansion point for all
    assert np.array_equal(shared[0], Pa[0]) and (n == 1 or not np.array_equal(shared[1], Pa[1]))


@pytest.mark.parametrize("size", CC.MESH_SIZES)
def test_mesh_sizes_against_the_restatement(gpu, size):
    """both RPCs in one launch, LDS-resident meshes and the slab in global memory; unequal axes catch a transposed index order"""
    rpcs = [CC.rpc(0), CC.rpc(1)]
    crop = (40.0, 25.0, 3000.0, 1200.0)
    ranges = [np.array([list(v) for v in rs]) for rs in zip(*[CC.perspective_ranges(r, crop, size) for r in rpcs])]
    P, err, cen = cam_utils.approx_rpcs_as_proj_matrices(rpcs, *ranges, return_centers=True)
    Xd, xd, altd = cam_utils.rpc_point_mesh(rpcs, *ranges)
    b_px, b_m = bounds(max(v[0] for v in resection_yardsticks().values()), max(v[1] for v in resection_yardsticks().values()))
    for k, r in enumerate(rpcs):
        cols, rows, alts = cam_utils.generate_point_mesh(*CC.perspective_ranges(r, crop, size))
        assert np.array_equal(altd[k], alts) and np.array_equal(xd[k, :, 0], cols) and np.array_equal(xd[k, :, 1], rows)
        Pr, err_r, cen_r = CC.resect(Xd[k], xd[k])
        d_px, d_m = CC.reprojection_distance(P[k], Pr, Xd[k]), np.abs(cen[k] - cen_r).max()
        print("mesh {} rpc {}: reprojection {:.3e} px (bound {:.3e}), centre {:.3e} m (bound {:.3e}), mean_err {:.3e} vs {:.3e}".format(size, k, d_px, b_px, d_m, b_m, err[k], err_r))
        assert d_px <= b_px and abs(err[k] - err_r) <= b_px and d_m <= b_m


def test_failures_raise_and_never_return_nan(gpu):
    r = CC.rpc(0)
    with pytest.raises((np.linalg.LinAlgError, ValueError)):
        cam_utils.perspective_rpc_approx(r, {"col0": 100.0, "row0": 0.0, "width": 0.0, "height": 1350.0})
    bad = r.copy()
    bad.row_num[3] = float("nan")
    with pytest.raises(ValueError):
        cam_utils.perspective_rpc_approx(bad, CC.offset(CC.CROPS["full"]))
    with pytest.raises(ValueError):
        cam_utils.affine_rpc_approx(bad, *CC.expansion_points(r)[0])
    X, x, _ = CC.resection_inputs()["crop"]
    with pytest.raises((np.linalg.LinAlgError, ValueError)):  # no extent: the normalisation divides by zero on the device
        cam_utils.camera_matrix(np.repeat(X[:1], 8, axis=0), np.repeat(x[:1], 8, axis=0))
    with pytest.raises((np.linalg.LinAlgError, ValueError)):  # 3-D points in one plane: a family of cameras fits them
        Xp = X.copy()
        Xp[:, 2] = 0.3 * Xp[:, 0] - 0.2 * Xp[:, 1] + 1.0e6
        cam_utils.camera_matrix(Xp, x)
    with pytest.raises((np.linalg.LinAlgError, ValueError)):  # on the polar axis there is no longitude
        cam_utils.affine_rpc_approx(r, 0.0, 0.0, 6.35e6)
    # one degenerate camera fails the batch; the good one alone passes and holds no NaN
    good = cam_utils.camera_matrices(X[None], x[None])
    assert np.isfinite(good).all()
    with pytest.raises((np.linalg.LinAlgError, ValueError)):
        cam_utils.camera_matrices(np.stack([X, np.repeat(X[:1], len(X), axis=0)]), np.stack([x, x]))


def test_camera_centres(gpu):
    rpcs = [CC.rpc(f) for f, _ in CC.FULL_ROUTE]
    offsets = [CC.offset(CC.CROPS[c]) for _, c in CC.FULL_ROUTE]
    centres = cam_utils.camera_centers(rpcs, offsets)
    cams = cam_utils.approx_cameras(rpcs, offsets, "perspective")
    assert centres.shape == (len(rpcs), 3)
    for k, (f, cname) in enumerate(CC.FULL_ROUTE):
        b_m = bounds(*full_route(f, cname)[5])[1]
        d = np.abs(centres[k] - CC.centre_of(cams[k])).max()
        _, _, alt = geo_utils.ecef_to_latlon_custom(centres[k][0], centres[k][1], centres[k][2])
        print("{} {}: centre vs host decomposition of the device P {:.3e} m (bound {:.3e}), {:.1f} km above the ellipsoid".format(f, cname, d, b_m, alt / 1e3))
        assert d <= b_m
        assert 400e3 <= alt <= 700e3

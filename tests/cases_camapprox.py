"""
Cases and yardsticks of the RPC -> affine / perspective camera approximation (satba.cam_utils, csrc/satba_camapprox.h), shared by
tools/gen_golden_camapprox.py (which records the reference's results into tests/golden/cam_approx.npz), the host test
(test_cam_approx_host.py) and the GPU tests (test_gpu_cam_approx.py).

* `resect` is a numpy restatement of the device's resection: Hartley normalisation, the four 4 x 4 moment matrices, the 12 x 12
  normal matrix, cyclic Jacobi, denormalisation, mean error and optical centre.  Its distance to the reference's SVD route on the
  stored points is the yardstick of the device tolerances.
* `affine_expected` composes the reference's affine_rpc_approx (value and exact first derivative of rpc.projection o
  ecef_to_latlon_custom; the reference takes the derivative with the `ad` package) from the two oracle Jacobians the project pins.
"""
import os

import numpy as np

from oracle import lm_oracle as L
from oracle import triangulate_oracle as T
from satba import cam_utils, geo_utils, synth
from satba.rpc_model import RPCModel

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cam_approx.npz")
IMAGE = (3200, 1350)  # the shipped images
# crops of the full-route cases: full image, 500^2, 50^2 (col0, row0, width, height)
CROPS = {"full": (0.0, 0.0, 3200.0, 1350.0), "c500": (1310.0, 420.0, 500.0, 500.0), "c50": (2210.0, 935.0, 50.0, 50.0)}
FULL_ROUTE = [(f, name) for f in (0, 1) for name in ("full", "c500", "c50")]
CAM_LDS_PTS = 1440  # csrc/satba_camapprox.h
# mesh sizes (n_col, n_row, n_alt): the smallest, unequal axes, the reference's, the largest LDS-resident one and the first that
# goes to the global slab (1441 = 11 x 131 has no three factors >= 2)
MESH_SIZES = [(2, 2, 2), (4, 3, 5), (10, 10, 10), (12, 12, 10), (7, 2, 103)]
assert 12 * 12 * 10 == CAM_LDS_PTS and 7 * 2 * 103 == CAM_LDS_PTS + 2
PX_CAP, CENTRE_CAP = 1e-6, 1e-2  # the project's parity level in pixels; metres for the optical centre
MARGIN = 20.0


def rpc(file_index):
    return RPCModel.from_file(synth.default_rpc_files()[file_index])


def offset(crop):
    return {"col0": crop[0], "row0": crop[1], "width": crop[2], "height": crop[3]}


def perspective_ranges(r, crop, n=(10, 10, 10)):
    """the mesh of the reference's perspective_rpc_approx"""
    return ([crop[0], crop[0] + crop[2], n[0]], [crop[1], crop[1] + crop[3], n[1]], [r.alt_offset - 100, r.alt_offset + 100, n[2]])


class OracleRpc:
    """an RPC whose localization is the oracle's restatement of the reference's C code (the device is held to it within 1e-9 deg)"""

    def __init__(self, r):
        self._r, self._c = r, T._Rpc(r, 0.1)
        self.alt_offset = r.alt_offset

    def localization(self, col, row, alt):
        return self._c.eval_rpc(np.asarray(col, float), np.asarray(row, float), np.asarray(alt, float))

    def projection(self, lon, lat, alt):
        return self._r.projection(lon, lat, alt)


def mesh_correspondences(r, col_range, row_range, alt_range, localization=None):
    """X (n, 3) ECEF, x (n, 2) of approx_rpc_as_proj_matrix's mesh; localization: callable (col, row, alt) -> lon, lat (default: oracle)"""
    cols, rows, alts = cam_utils.generate_point_mesh(col_range, row_range, alt_range)
    lons, lats = (localization or OracleRpc(r).localization)(cols, rows, alts)
    x, y, z = geo_utils.latlon_to_ecef_custom(lats, lons, alts)
    return np.vstack([x, y, z]).T, np.vstack([cols, rows]).T


# ------------------------------------------------------------------------------------------------ resection, restated
def jacobi_eigh(A, sweeps=40):
    """cyclic Jacobi as cam_jacobi12 runs it: eigenvalues (the diagonal) and eigenvectors (columns)"""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    V = np.eye(n)
    for _ in range(sweeps):
        rotated = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq, app, aqq = A[p, q], A[p, p], A[q, q]
                if not abs(apq) > 2.0 ** -56 * (abs(app) + abs(aqq)):
                    continue
                rotated = True
                d, g2 = aqq - app, 2.0 * apq
                t = np.copysign(1.0, d) * g2 / (abs(d) + np.sqrt(d * d + g2 * g2))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = c * t
                kp, kq = A[:, p].copy(), A[:, q].copy()
                A[:, p] = A[p, :] = c * kp - s * kq
                A[:, q] = A[q, :] = s * kp + c * kq
                A[p, p], A[q, q] = app - t * apq, aqq + t * apq
                A[p, q] = A[q, p] = 0.0
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
        if not rotated:
            break
    return np.diag(A).copy(), V


def normal_matrix(Xn, xn):
    """A^T A of the reference's 2n x 12 DLT matrix from the four moment matrices of Xh = (Xn, 1)"""
    Xh = np.hstack([Xn, np.ones((Xn.shape[0], 1))])
    x, y = xn[:, 0], xn[:, 1]
    S0 = Xh.T @ Xh
    Sx = Xh.T @ (x[:, None] * Xh)
    Sy = Xh.T @ (y[:, None] * Xh)
    Sr = Xh.T @ ((x * x + y * y)[:, None] * Xh)
    Z = np.zeros((4, 4))
    return np.block([[S0, Z, -Sx], [Z, S0, -Sy], [-Sx, -Sy, Sr]])


def resect(X, x):
    """P (3, 4) as camera_matrix returns it, mean reprojection error [px], optical centre (3,)"""
    Xn, U = cam_utils.normalize_3d_points(X)
    xn, Tm = cam_utils.normalize_2d_points(x)
    lam, V = jacobi_eigh(normal_matrix(Xn, xn))
    Pn = V[:, np.argmin(lam)].reshape(3, 4)
    P = np.linalg.inv(Tm) @ Pn @ U
    h = Xn @ Pn[:, :3].T + Pn[:, 3]
    err = np.mean(np.linalg.norm(xn - h[:, :2] / h[:, 2:3], axis=1)) / Tm[0, 0]
    centre = -np.linalg.solve(Pn[:, :3], Pn[:, 3]) / U[0, 0] - U[:3, 3] / U[0, 0]
    return P, err, centre


def to_crop(P, crop):
    """perspective_rpc_approx's last step (ref:bundle_adjust/cam_utils.py:195-197)"""
    Tr = np.array([[1.0, 0.0, -crop[0]], [0.0, 1.0, -crop[1]], [0.0, 0.0, 1.0]])
    Pc = Tr @ P
    return Pc / Pc[2, 3]


def reprojection_distance(Pa, Pb, X):
    """largest distance in pixels between the projections of X through two matrices"""
    return float(np.abs(cam_utils.apply_projection_matrix(Pa, X) - cam_utils.apply_projection_matrix(Pb, X)).max())


def centre_of(P):
    return cam_utils.decompose_perspective_camera(P)[3]


# ------------------------------------------------------------------------------------------------ resection cases of the golden file
def exact_camera():
    """a synthetic exact perspective camera 600 km above 4 x 4 x 3 points spread over 4 km in a local frame: X, x"""
    rng = np.random.RandomState(11)
    g = np.stack(np.meshgrid(np.linspace(-2000, 2000, 4), np.linspace(-1500, 2500, 4), np.linspace(-100, 300, 3), indexing="ij"), -1).reshape(-1, 3)
    X = g + rng.uniform(-50, 50, g.shape)
    a, b = 0.03, -0.02
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    K = np.array([[6.0e5, 12.0, 1500.0], [0.0, 6.1e5, 700.0], [0.0, 0.0, 1.0]])
    P = cam_utils.compose_perspective_camera(K, Rx @ Ry, np.array([2.0e4, -1.5e4, -6.0e5]))
    return X, cam_utils.apply_projection_matrix(P, X)


def six_points():
    """exactly 6 correspondences in general position (11 equations would do: the smallest legal set), of the first RPC's mesh"""
    X, x = mesh_correspondences(rpc(0), [100.0, 3000.0, 3], [50.0, 1300.0, 3], [3300.0, 3700.0, 3])
    pick = [0, 5, 7, 11, 19, 24]  # no four of them in a plane of the mesh, no three on a line
    return X[pick], x[pick]


def resection_inputs():
    """name -> (X, x, crop or None): what camera_matrix is run on, regenerated from the shipped RPCs"""
    out = {}
    for f in (0, 1):
        r = rpc(f)
        out["mesh6_{}".format(f)] = mesh_correspondences(r, [0.0, 3200.0, 6], [0.0, 1350.0, 6], [r.alt_offset - 100, r.alt_offset + 100, 6]) + (None,)
    crop = (1200.0, 300.0, 800.0, 600.0)
    r = rpc(1)
    out["crop"] = mesh_correspondences(r, *perspective_ranges(r, crop, (5, 4, 3))) + (crop,)
    out["exact"] = exact_camera() + (None,)
    out["six"] = six_points() + (None,)
    return out


def load_golden():
    return np.load(GOLDEN)


# ------------------------------------------------------------------------------------------------ affine route
def rpc_oracle(r, X):
    """(col, row) (n, 2) of ECEF points and d(col, row)/dX (n, 2, 3): the chain of the two pinned oracle Jacobians"""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    lat, lon, alt, G = L.geodetic_with_jacobian(X)
    q, D = L.rpc_project_with_jacobian(r, lat, lon, alt)
    return q, D @ G


def rpc_oracle_extended(r, X):
    """(col, row) of one ECEF point by the same two oracle functions in numpy's extended precision (64-bit mantissa on x86)"""
    lat, lon, alt, _ = L.geodetic_with_jacobian(np.atleast_2d(X).astype(np.longdouble))
    return L.rpc_project_with_jacobian(r, lat, lon, alt)[0][0]


def affine_expected(r, p, col0=0.0, row0=0.0):
    """affine_rpc_approx of the reference (ref:bundle_adjust/cam_utils.py:146-174) with the oracle's exact derivative"""
    p = np.asarray(p, dtype=np.float64)
    q, J = rpc_oracle(r, p)
    A = np.zeros((3, 4))
    A[:2, :3] = J[0]
    A[:2, 3] = q[0] - J[0] @ p
    A[2, 3] = 1.0
    Pc = np.array([[1.0, 0.0, -col0], [0.0, 1.0, -row0], [0.0, 0.0, 1.0]]) @ A
    return Pc / Pc[2, 3]


def expansion_points(r):
    """the RPC's own centre and a point 2 km off (east and north, 150 m up)"""
    out = []
    for dlon, dlat, dalt in ((0.0, 0.0, 0.0), (0.015, 0.012, 150.0)):
        out.append(np.array(geo_utils.latlon_to_ecef_custom(r.lat_offset + dlat, r.lon_offset + dlon, r.alt_offset + dalt), dtype=np.float64))
    return out


def hessian(r, p, h=200.0):
    """second derivatives d2(col, row)/dX_i dX_k [px / m^2], (2, 3, 3), from the oracle's analytic first derivative at p +- h e_k
    (a central difference of J: its error, O(h^2) times the fourth derivative, is far below the value)"""
    H = np.zeros((2, 3, 3))
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        H[:, :, k] = (rpc_oracle(r, p + e)[1][0] - rpc_oracle(r, p - e)[1][0]) / (2 * h)
    return H


def fd_step_and_bound(r, p, hj=1000.0):
    """Step h [m] of a central difference of the oracle projection at p along an axis and the bound on its distance to the exact
    derivative [px / m].  Truncation: h^2 M3 / 6 with M3 the largest third derivative d3(col, row)/dx_k^3, taken as the second
    difference of the oracle's analytic J over hj = 1 km (the curvature scale of the second derivative: the geodetic conversion
    bends the projection far faster than the sensor's distance would suggest).  Rounding: an evaluation of the projection is good to
    eps_f = 4 eps |p| |J| pixels (roundings of the ECEF coordinates and of the geodetic angles, each worth eps |p| metres on the
    ground), which the difference divides by h.  h balances the two; the bound is twice their sum at that h."""
    J0 = rpc_oracle(r, p)[1][0]
    M3 = 0.0
    for k in range(3):
        e = np.zeros(3)
        e[k] = hj
        M3 = max(M3, np.abs((rpc_oracle(r, p + e)[1][0] - 2 * J0 + rpc_oracle(r, p - e)[1][0])[:, k]).max() / (hj * hj))
    eps_f = 4 * np.finfo(float).eps * np.linalg.norm(p) * np.abs(J0).max()
    h = (3 * eps_f / M3) ** (1.0 / 3.0)
    return h, 2 * (h * h * M3 / 6 + eps_f / h)


def affine_fd(r, p, h, col0=0.0, row0=0.0):
    """affine_rpc_approx with the derivative taken by central differences of the oracle projection"""
    p = np.asarray(p, dtype=np.float64)
    q = rpc_oracle(r, p)[0][0]
    J = np.zeros((2, 3))
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        J[:, k] = (rpc_oracle(r, p + e)[0][0] - rpc_oracle(r, p - e)[0][0]) / (2 * h)
    P = np.zeros((3, 4))
    P[:2, :3] = J
    P[:2, 3] = q - J @ p - np.array([col0, row0])
    P[2, 3] = 1.0
    return P


def affine_yardstick(r, p, col0=0.0, row0=0.0):
    """distance of the oracle composition to its finite-difference version: relative on J (to its largest entry), absolute on P[:2, 3]"""
    h, _ = fd_step_and_bound(r, p)
    Pe, Pf = affine_expected(r, p, col0, row0), affine_fd(r, p, h, col0, row0)
    return np.abs(Pe[:2, :3] - Pf[:2, :3]).max() / np.abs(Pe[:2, :3]).max(), np.abs(Pe[:2, 3] - Pf[:2, 3]).max()


# ------------------------------------------------------------------------------------------------ batches
def batch(n):
    """n cameras: the two RPCs cycled, every camera with its own crop and expansion point.  Returns rpcs, offsets, centers (n, 3)"""
    rpcs, offsets, centers = [], [], []
    base = [rpc(0), rpc(1)]
    for k in range(n):
        r = base[k % 2]
        w, hgt = 3200.0 - 11.0 * (k % 97), 1350.0 - 5.0 * (k % 89)
        offsets.append({"col0": 3.0 * (k % 31), "row0": 2.0 * (k % 29), "width": w - 3.0 * (k % 31), "height": hgt - 2.0 * (k % 29)})
        centers.append(geo_utils.latlon_to_ecef_custom(r.lat_offset + 1e-4 * (k % 53), r.lon_offset - 1e-4 * (k % 47), r.alt_offset + k))
        rpcs.append(r)
    return rpcs, offsets, np.array(centers, dtype=np.float64)

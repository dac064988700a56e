"""
Camera helpers with the reference's names (ref:bundle_adjust/cam_utils.py).

The (de)composition helpers ba_params packs / unpacks camera matrices with (:45-75, 78-89, 92-143, 201-231) are host numpy.
The approximation of RPCs as affine or perspective cameras (:146-198, 234-277, 309-445: affine_rpc_approx, perspective_rpc_approx,
approx_rpc_as_proj_matrix, camera_matrix) runs on the device (csrc/satba_camapprox.h), for all cameras of a call in one launch;
approx_cameras / camera_centers are what ba_pipeline.set_cameras / set_camera_centers loop over.  There is no CPU fallback.
`rpc` is anything with the attribute names of rpcm.RPCModel (satba.rpc_model.rpc_to_table).
"""
import os

import numpy as np

from . import geo_utils
from .rpc_model import rpc_to_table


def decompose_perspective_camera(P):
    """
    P = K R [I | -oC] with K upper-triangular, positive diagonal (Hartley & Zisserman 6.2.4;
    ref:bundle_adjust/cam_utils.py:45-75).  Returns K, R, vecT = -R oC, oC.
    """
    from scipy.linalg import rq

    M = P[:, :3]
    K, R = rq(M)
    sgn = np.sign(np.diag(K))
    K = K * sgn[np.newaxis, :]  # K diag(sgn)
    R = sgn[:, np.newaxis] * R  # diag(sgn) R
    oC = -np.linalg.solve(M, P[:, 3])
    vecT = -(R @ oC)
    return K, R, vecT, oC


def compose_perspective_camera(K, R, oC):
    """P = K R [I | -oC]  (ref:bundle_adjust/cam_utils.py:78-89)."""
    return K @ R @ np.hstack((np.eye(3), -np.asarray(oC, dtype=np.float64).reshape(3, 1)))


def decompose_affine_camera(P):
    """
    Affine camera P = [[K, 0], [0, 1]] @ [[R[:2], vecT], [0, 1]], K = [[fx, s], [0, fy]]
    (Hartley & Zisserman 6.3.3; ref:bundle_adjust/cam_utils.py:92-126).  Returns K (2x2), R (3x3), vecT (2x1).
    """
    M = P[:2, :3]
    G = M @ M.T
    fy = np.sqrt(G[1, 1])
    s = G[1, 0] / fy
    fx = np.sqrt(G[0, 0] - s * s)
    K = np.array([[fx, s], [0.0, fy]])
    Kinv = np.linalg.inv(K)
    R2 = Kinv @ M
    R = np.vstack((R2, np.cross(R2[0], R2[1])))
    vecT = Kinv @ P[:2, 3:4]
    return K, R, vecT


def compose_affine_camera(K, R, vecT):
    """Inverse of decompose_affine_camera (ref:bundle_adjust/cam_utils.py:129-143)."""
    P = np.zeros((3, 4))
    P[:2, :3] = K @ R[:2]
    P[:2, 3] = K @ np.asarray(vecT, dtype=np.float64).reshape(2)
    P[2, 3] = 1.0
    return P


def apply_projection_matrix(P, pts3d):
    """Project Nx3 points with a 3x4 matrix (ref:bundle_adjust/cam_utils.py:201-214)."""
    h = pts3d @ P[:, :3].T + P[:, 3]
    return h[:, :2] / h[:, 2:3]


def apply_rpc_projection(rpc, pts3d):
    """ECEF -> geodetic -> rpc.projection (ref:bundle_adjust/cam_utils.py:217-231)."""
    lat, lon, alt = geo_utils.ecef_to_latlon_custom(pts3d[:, 0], pts3d[:, 1], pts3d[:, 2])
    col, row = rpc.projection(lon, lat, alt)
    return np.vstack((col, row)).T


def generate_point_mesh(col_range, row_range, alt_range):
    """(col, row, alt) coordinates of the n_col x n_row x n_alt grid given by three (min, max, n) triplets, flattened with the
    columns running fastest and the altitudes slowest (ref:bundle_adjust/cam_utils.py:280-306)."""
    cols, rows, alts = [np.linspace(v[0], v[1], int(v[2])) for v in (col_range, row_range, alt_range)]
    a, r, c = np.meshgrid(alts, rows, cols, indexing="ij")
    return c.reshape(-1), r.reshape(-1), a.reshape(-1)


# ---------------------------------------------------------------------------------------------- RPC -> affine / perspective camera
def _lib():
    from . import engine_hip as E

    return E, E.load_library(), int(os.environ.get("LOCAL_RANK", "0"))


def _checked(E, lib, rc):
    if rc == -4 and (lib.satba_last_error() or b"").startswith(b"Singular matrix"):
        # points no unique camera fits: the reference's numpy.linalg calls raise LinAlgError or return NaN there
        raise np.linalg.LinAlgError((lib.satba_last_error() or b"").decode())
    E._check(lib, rc)


def _tables(rpcs):
    if len(rpcs) == 0:
        return np.zeros((0, 90))
    return np.ascontiguousarray(np.stack([np.asarray(rpc_to_table(r), dtype=np.float64) for r in rpcs]))


def _per_camera(v, M, width, name):
    """(width,) shared by all cameras or (M, width) -> contiguous (M, width) float64"""
    a = np.asarray(v, dtype=np.float64)
    if a.shape == (width,):
        a = np.broadcast_to(a, (M, width))
    if a.shape != (M, width):
        raise ValueError("{} must have shape ({},) or ({}, {}), got {}".format(name, width, M, width, a.shape))
    return np.ascontiguousarray(a)


def normalize_2d_points(pts):
    """Centroid to the origin, mean distance to sqrt(2) (ref:bundle_adjust/cam_utils.py:359-404).  Returns new_pts (N, 2), T (3, 3)."""
    pts = np.asarray(pts, dtype=np.float64)
    c = np.array([np.mean(pts[:, 0]), np.mean(pts[:, 1])])
    new = pts - c
    s = np.sqrt(2) / np.mean(np.sqrt(new[:, 0] ** 2 + new[:, 1] ** 2))
    T = np.eye(3)
    T[0, 0] = T[1, 1] = s
    T[:2, 2] = -s * c
    return s * new, T


def normalize_3d_points(pts):
    """Centroid to the origin, mean distance to sqrt(3) (ref:bundle_adjust/cam_utils.py:407-452).  Returns new_pts (N, 3), U (4, 4)."""
    pts = np.asarray(pts, dtype=np.float64)
    c = np.array([np.mean(pts[:, 0]), np.mean(pts[:, 1]), np.mean(pts[:, 2])])
    new = pts - c
    s = np.sqrt(3) / np.mean(np.sqrt(new[:, 0] ** 2 + new[:, 1] ** 2 + new[:, 2] ** 2))
    U = np.eye(4)
    U[0, 0] = U[1, 1] = U[2, 2] = s
    U[:3, 3] = -s * c
    return s * new, U


def camera_matrices(X, x, return_info=False):
    """camera_matrix for M sets of n correspondences at once: X (M, n, 3), x (M, n, 2) -> P (M, 3, 4); with return_info also the mean
    reprojection error of every set in pixels (M,)."""
    E, lib, dev = _lib()
    X = np.ascontiguousarray(X, dtype=np.float64); x = np.ascontiguousarray(x, dtype=np.float64)
    if X.ndim != 3 or x.ndim != 3 or X.shape[2] != 3 or x.shape[2] != 2 or X.shape[:2] != x.shape[:2]:
        raise ValueError("X must be (M, n, 3) and x (M, n, 2), got {} and {}".format(X.shape, x.shape))
    M, n = X.shape[:2]
    P = np.zeros((M, 3, 4)); err = np.zeros(M)
    _checked(E, lib, lib.satba_camera_resection(M, n, E._ptr(X), E._ptr(x), E._ptr(P), E._ptr(err), dev))
    return (P, err) if return_info else P


def camera_matrix(X, x):
    """
    ref:bundle_adjust/cam_utils.py:309-356: the 3 x 4 projection matrix of the correspondences X (N, 3) -> x (N, 2) by the Direct
    Linear Transformation with Hartley's normalisation, on the device.  Scale and sign of the matrix are arbitrary, as in the reference.
    """
    X = np.asarray(X, dtype=np.float64); x = np.asarray(x, dtype=np.float64)
    if X.ndim != 2 or x.ndim != 2:
        raise ValueError("X must be (N, 3) and x (N, 2), got {} and {}".format(X.shape, x.shape))
    return camera_matrices(X[None], x[None])[0]


def _mesh_args(M, col_range, row_range, alt_range):
    n = []
    ranges = []
    for name, v in (("col_range", col_range), ("row_range", row_range), ("alt_range", alt_range)):
        a = np.asarray(v, dtype=np.float64)
        if a.shape == (3,):
            a = np.broadcast_to(a, (M, 3))
        if a.shape != (M, 3):
            raise ValueError("{} must be (min, max, n) or one such triplet per camera, got shape {}".format(name, a.shape))
        cnt = a[:, 2] if M else np.asarray(v, dtype=np.float64).reshape(-1)[2:3]
        if cnt.size and (np.any(cnt != cnt[0]) or cnt[0] != int(cnt[0])):
            raise ValueError("{}: all cameras of a call share one whole number of samples".format(name))
        n.append(int(cnt[0]) if cnt.size else 2)
        ranges.append(np.ascontiguousarray(a[:, :2]))
    return ranges, n


def rpc_point_mesh(rpcs, col_range, row_range, alt_range):
    """The correspondences approx_rpc_as_proj_matrix resects, for M cameras at once: generate_point_mesh, localisation through every
    RPC and latlon_to_ecef_custom on the device.  Ranges: (min, max, n) shared or one triplet per camera with a common n.
    Returns X (M, n, 3) ECEF, x (M, n, 2) col / row, alts (M, n)."""
    E, lib, dev = _lib()
    M = len(rpcs)
    (cr, rr, ar), (nc, nr, na) = _mesh_args(M, col_range, row_range, alt_range)
    tabs = _tables(rpcs)
    n = max(nc, 0) * max(nr, 0) * max(na, 0)
    X = np.zeros((M, n, 3)); x = np.zeros((M, n, 2)); alts = np.zeros((M, n))
    _checked(E, lib, lib.satba_rpc_mesh(M, E._ptr(tabs), E._ptr(cr), E._ptr(rr), E._ptr(ar), nc, nr, na, E._ptr(X), E._ptr(x), E._ptr(alts), dev))
    return X, x, alts


def approx_rpcs_as_proj_matrices(rpcs, col_range, row_range, alt_range, offsets=None, return_centers=False):
    """approx_rpc_as_proj_matrix for M cameras in one launch.  offsets: None (the matrices as the resection leaves them) or M crop
    dicts: the matrices are moved to (col0, row0) and divided by P[2, 3] as perspective_rpc_approx does.
    Returns P (M, 3, 4), mean_err (M,) [, centers (M, 3)]."""
    E, lib, dev = _lib()
    M = len(rpcs)
    (cr, rr, ar), (nc, nr, na) = _mesh_args(M, col_range, row_range, alt_range)
    tabs = _tables(rpcs)
    c0 = None
    if offsets is not None:
        if len(offsets) != M:
            raise ValueError("{} offsets for {} cameras".format(len(offsets), M))
        c0 = np.ascontiguousarray(np.array([[o["col0"], o["row0"]] for o in offsets], dtype=np.float64).reshape(M, 2))
    P = np.zeros((M, 3, 4)); err = np.zeros(M); cen = np.zeros((M, 3))
    _checked(E, lib, lib.satba_rpc_perspective_approx(M, E._ptr(tabs), E._ptr(cr), E._ptr(rr), E._ptr(ar), nc, nr, na,
                                                      E._ptr(c0) if c0 is not None else None, E._ptr(P), E._ptr(err),
                                                      E._ptr(cen) if return_centers else None, dev))
    return (P, err, cen) if return_centers else (P, err)


def approx_rpc_as_proj_matrix(rpc_model, col_range, lin_range, alt_range, verbose=False):
    """
    ref:bundle_adjust/cam_utils.py:234-277: least-squares approximation of the RPC as a projection matrix over the mesh given by the
    three (min, max, n) triplets.  Returns (P, mean_err): the matrix and its mean reprojection error over the mesh in pixels.
    verbose prints the reference's summary of the column and row differences (no histogram).
    """
    P, err = approx_rpcs_as_proj_matrices([rpc_model], col_range, lin_range, alt_range)
    if verbose:
        X, x, _ = rpc_point_mesh([rpc_model], col_range, lin_range, alt_range)
        d = x[0] - apply_projection_matrix(P[0], X[0])
        print("approximate_rpc_as_projective: (min, max, mean)")
        print("distance on cols:", np.min(d[:, 0]), np.max(d[:, 0]), np.mean(d[:, 0]))
        print("distance on rows:", np.min(d[:, 1]), np.max(d[:, 1]), np.mean(d[:, 1]))
    return P[0], float(err[0])


def _perspective_ranges(rpcs, offsets):
    """the mesh of perspective_rpc_approx (ref:bundle_adjust/cam_utils.py:193-194): 10 x 10 x 10 over the crop and +-100 m around alt_offset"""
    M = len(rpcs)
    if len(offsets) != M:
        raise ValueError("{} offsets for {} cameras".format(len(offsets), M))
    cr = np.array([[o["col0"], o["col0"] + o["width"], 10] for o in offsets], dtype=np.float64).reshape(M, 3)
    rr = np.array([[o["row0"], o["row0"] + o["height"], 10] for o in offsets], dtype=np.float64).reshape(M, 3)
    ar = np.array([[r.alt_offset - 100, r.alt_offset + 100, 10] for r in rpcs], dtype=np.float64).reshape(M, 3)
    return cr, rr, ar


def perspective_rpc_approx(rpc, offset):
    """
    ref:bundle_adjust/cam_utils.py:177-198: the RPC as a 3 x 4 perspective matrix in crop coordinates, by resection of a 10 x 10 x 10
    mesh over the crop (offset: dict col0 / row0 / width / height) and +-100 m around the RPC's altitude offset.
    Returns (P, mean_err).
    """
    P, info = approx_cameras([rpc], [offset], "perspective", return_info=True)
    return P[0], float(info["mean_err"][0])


def affine_rpc_approx(rpc, x, y, z, offset={"col0": 0.0, "row0": 0.0}):
    """
    ref:bundle_adjust/cam_utils.py:146-174: first-order Taylor approximation of the RPC projection at the ECEF point (x, y, z), in the
    coordinates of the crop `offset`.  Returns the 3 x 4 affine projection matrix.
    """
    return approx_cameras([rpc], [offset], "affine", center=(x, y, z))[0]


def approx_cameras(rpcs, offsets, cam_model, center=None, return_info=False):
    """
    The cameras ba_pipeline.set_cameras builds (ref:bundle_adjust/ba_pipeline.py:201-217), all in one launch.
    cam_model "affine": affine_rpc_approx of every RPC at `center`, the ECEF expansion point (3,) shared by all cameras (the
    pipeline's centre of the area of interest) or (M, 3); "perspective": perspective_rpc_approx; "rpc": copies of the RPCs.
    Returns the list of cameras; with return_info also a dict: perspective -> mean_err (M,) and centers (M, 3) optical centres.
    """
    M = len(rpcs)
    if len(offsets) != M:
        raise ValueError("{} offsets for {} cameras".format(len(offsets), M))
    info = {}
    if cam_model == "affine":
        if center is None:
            raise ValueError("the affine approximation needs the ECEF point `center` to expand at")
        E, lib, dev = _lib()
        xyz = _per_camera(center, M, 3, "center")
        c0 = np.ascontiguousarray(np.array([[o["col0"], o["row0"]] for o in offsets], dtype=np.float64).reshape(M, 2))
        tabs = _tables(rpcs)
        P = np.zeros((M, 3, 4))
        _checked(E, lib, lib.satba_rpc_affine_approx(M, E._ptr(tabs), E._ptr(xyz), E._ptr(c0), E._ptr(P), dev))
        cams = [P[k] for k in range(M)]
    elif cam_model == "perspective":
        cr, rr, ar = _perspective_ranges(rpcs, offsets)
        P, err, cen = approx_rpcs_as_proj_matrices(rpcs, cr, rr, ar, offsets, return_centers=True)
        cams = [P[k] for k in range(M)]
        info = {"mean_err": err, "centers": cen}
    elif cam_model == "rpc":
        import copy

        cams = [copy.copy(r) for r in rpcs]
    else:
        raise ValueError("cam_model must be affine, perspective or rpc, got {!r}".format(cam_model))
    return (cams, info) if return_info else cams


def camera_centers(rpcs, offsets):
    """What ba_pipeline.set_camera_centers computes (ref:bundle_adjust/ba_pipeline.py:185-199, cam_utils.py:29-34): the optical centre
    of the perspective approximation of every RPC, (M, 3) ECEF."""
    return approx_cameras(rpcs, offsets, "perspective", return_info=True)[1]["centers"]


def check_projection_matrices(err, max_err=1.0):
    """ref:bundle_adjust/ba_pipeline.py:174-183: warn about approximations whose mean reprojection error exceeds max_err pixels.
    Returns the indices of those cameras."""
    err = np.asarray(err, dtype=np.float64)
    err_cams = np.arange(len(err))[err > max_err]
    if len(err_cams) > 0:
        lines = " ".join(["\nCamera {}, error = {:.3f}".format(c, err[c]) for c in err_cams])
        print("WARNING: {} projection matrices with error larger than {} px\n{}".format(len(err_cams), max_err, lines), flush=True)
    return err_cams

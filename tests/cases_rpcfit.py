"""
Scenarios of the RPC re-fit's margin loop (satba.ba_rpcfit.fit_Rt_corrected_rpcs -> satba_rpc_refit) shared by the host test that pins
them (test_rpcfit_cases_host.py) and the GPU tests (test_gpu_rpcfit.py), and the extended-precision yardstick of the fit kernel.

A scenario is one camera: one of the two shipped RPC files, a crop, a correction Rt = [s * ANGLES, 0, C] with C 5e5 m above the
scene centre, and a global transform (None or GT).  `expected_margins` replays `ba_rpcfit._fit_with_growing_margin` with no device
(localisation by the oracle's restatement of the reference's C, the fit by the oracle's weighted_lsq, scipy's convex hull) and
returns the margin the loop ends at together with, per round, the signed distance in pixels of the worst crop corner to the hull
of the re-projected mesh (positive: outside, the margin doubles).

Two correct solvers differ by <= 2e-3 px in the fitted projection, so a scenario decides the same way on every correct
implementation only if that distance stays away from zero: MIN_SLACK (1 px) in every round.  That is a condition on the scenarios,
asserted for each of them on the CPU together with the literal margins below, not a tolerance of the device tests.
"""
import numpy as np

from oracle import rpcfit_oracle as F
from oracle import triangulate_oracle as T
from satba import cam_utils, geo_utils, synth
from satba.ba_core import adjust_pts3d
from satba.rpc_model import RPCModel

ANGLES = np.array([4e-6, -3e-6, 5e-6])
GT = np.array([30.0, -20.0, 10.0])
MIN_SLACK = 1.0
GIVE_UP = 1280  # the first margin above 1000: the loop returns whatever it has

# (file, s, global transform or None) -> margin the loop ends at, at n_samples = 10 and the full-image crop (CPU oracle)
FULL_IMAGE = {
    (0, 1, None): 10, (0, 10, None): 40, (0, 40, None): 160, (0, 150, None): 640, (0, 2000, None): GIVE_UP,
    (1, 1, None): 10, (1, 10, None): 40, (1, 40, None): 160, (1, 150, None): 640, (1, 2000, None): GIVE_UP,
    (0, 1, "gt"): 40, (0, 10, "gt"): 20, (0, 150, "gt"): 640, (0, 2000, "gt"): GIVE_UP,
    (1, 10, "gt"): 40, (1, 40, "gt"): 160, (1, 150, "gt"): 640, (1, 2000, "gt"): GIVE_UP,
}
# not usable (a corner within 1 px of the hull in some round): (0, 40, gt) and (1, 1, gt)

# the mixed batches of the GPU tests: alternating files, slots scattered in the later rounds
BATCH_NONE = [(0, 40, None), (1, 1, None), (0, 2000, None), (1, 10, None), (0, 1, None), (1, 150, None)]
BATCH_GT = [(0, 150, "gt"), (1, 10, "gt"), (0, 2000, "gt"), (1, 40, "gt"), (0, 10, "gt"), (1, 150, "gt"), (0, 1, "gt")]

# crops that do not start at (0, 0) and are smaller than the image: (file, s, gt, (col0, row0, width, height)) -> margin
CROP = (120, 75, 2400, 1000)  # the shipped images are 3200 x 1350
CROPPED = {
    (0, 40, None, CROP): 160, (1, 1, None, CROP): 10,
    (0, 10, "gt", CROP): 20, (1, 10, "gt", CROP): 40,
}

# other mesh sizes: (file, s, gt) -> margin at every n_samples of MESH_N.  16 and 15 put more than 48 KB of hull points into the
# LDS; 4 (64 samples, one staging tile of the fit) is the lower bound of satba_rpc_refit and the oracle's fit is regular on it:
# numpy.linalg.inv raises no LinAlgError at n_samples = 4 on the CPU.  s = 5 doubles once (the oracle's fit of a 16^3 mesh costs
# seconds per round on the CPU: the fewest rounds that still loop)
SMALLEST_N = 4
REFIT_MAX_N = 16  # csrc/satba_rpcfit.h
MESH_N = [16, 15, SMALLEST_N]
MESH_BATCH = [(0, 5, None), (1, 1, None)]
MESH_MARGINS = {(0, 5, None): 20, (1, 1, None): 10}


def rpc(file_index):
    return RPCModel.from_file(synth.default_rpc_files()[file_index])


def full_crop(r):
    return {"col0": 0, "row0": 0, "width": int(2 * r.col_scale), "height": int(2 * r.row_scale)}


def crop_dict(t):
    return {"col0": t[0], "row0": t[1], "width": t[2], "height": t[3]}


def correction(r, s):
    """(1, 9) [angles, T, C]: rotation by s * ANGLES about a centre 5e5 m above the scene centre"""
    c = np.array(geo_utils.latlon_to_ecef_custom(r.lat_offset, r.lon_offset, r.alt_offset))
    C = c + 5e5 * c / np.linalg.norm(c)
    return np.concatenate([s * ANGLES, np.zeros(3), C]).reshape(1, 9)


def gt_of(tag):
    return None if tag is None else GT.copy()


def scenario(key):
    """(rpc, Rt, crop, global transform) of a key (file, s, gt tag[, crop tuple])"""
    r = rpc(key[0])
    crop = crop_dict(key[3]) if len(key) > 3 and isinstance(key[3], tuple) else full_crop(r)
    return r, correction(r, key[1]), crop, gt_of(key[2])


def mesh(r, crop, margin, n_samples):
    """input_locs (n^3, 3) lon / lat / alt and the ECEF grid of the mesh over crop + margin, localised by the oracle"""
    x0, y0, w, h = crop["col0"], crop["row0"], crop["width"], crop["height"]
    cols, rows, alts = cam_utils.generate_point_mesh([x0 - margin, x0 + w + margin, n_samples], [y0 - margin, y0 + h + margin, n_samples],
                                                     [r.alt_offset - r.alt_scale, r.alt_offset + r.alt_scale, n_samples])
    lon, lat = T._Rpc(r, 0.1).eval_rpc(cols, rows, alts)
    grid = np.stack(geo_utils.latlon_to_ecef_custom(lat, lon, alts), 1)
    return np.stack([lon, lat, alts], 1), grid


def corner_distance(pts, crop):
    """largest signed distance (px) of the four crop corners to the convex hull of pts (n, 2): > 0 means a corner is outside"""
    from scipy.spatial import ConvexHull

    x0, y0, w, h = crop["col0"], crop["row0"], crop["width"], crop["height"]
    corners = np.array([[x0, y0], [x0, y0 + h], [x0 + w, y0 + h], [x0 + w, y0]], dtype=np.float64)
    eq = ConvexHull(np.asarray(pts, dtype=np.float64)).equations  # unit normals: a x + b y + c <= 0 inside
    return float((eq[:, :2] @ corners.T + eq[:, 2:3]).max())


def expected_margins(r, Rt, crop, gt, n_samples=10):
    """_fit_with_growing_margin on the CPU.  Returns (margin, [worst corner distance per round], [oracle iterations per round])."""
    margin, dist, iters = 10, [], []
    while True:
        locs, grid = mesh(r, crop, margin, n_samples)
        target = cam_utils.apply_rpc_projection(r, adjust_pts3d(grid + gt if gt is not None else grid, Rt))
        m, it = F.weighted_lsq(target, locs)
        la, lo, al = geo_utils.ecef_to_latlon_custom(grid[:, 0], grid[:, 1], grid[:, 2])  # the mesh WITHOUT the global transform
        d = corner_distance(np.stack(F.project(m, lo, la, al), 1), crop)
        dist.append(d); iters.append(it)
        if margin > 1000 or d <= 1e-9:
            return margin, dist, iters
        margin *= 2


# -------------------------------------------------------------------------------- the fit kernel against extended precision
EDGE_N = [39, 40, 63, 64, 65, 255, 256, 257, 1000]  # unknowns, +1, the tile of 64 and the workgroup of 256 with both neighbours
GOLDEN_FITS = ["rpc0", "rpc1", "affine"]
ETA_CAP = 32.0         # device <= ETA_CAP x numpy.linalg.solve on the same system
MIXED_PASSES_N = 257   # the size of the batch of different pass counts: one past the workgroup
ETA_SOLVE_MAX = 1e-14  # and numpy.linalg.solve itself must be this good, or the cap says nothing


def subset(g, name, n):
    """seeded n of the samples of a case of tests/golden/rpcfit.npz, ascending; all of them where it has no more than n (the RPC
    cases hold 1000 samples, the affine one 343: its "1000" is its whole set)"""
    t, x = g[name + "_target"], g[name + "_locs"]
    if n >= t.shape[0]:
        return t.copy(), x.copy()
    idx = np.sort(np.random.default_rng([GOLDEN_FITS.index(name), n]).permutation(t.shape[0])[:n])
    return np.ascontiguousarray(t[idx]), np.ascontiguousarray(x[idx])


def scaling_table(target, locs):
    """the record's last ten values (lon, lat, alt, col, row: offset, scale) by the reference's scaling_params: plain extrema"""
    tab = np.zeros(90)
    for q, v in enumerate((locs[:, 0], locs[:, 1], locs[:, 2], target[:, 0], target[:, 1])):
        tab[81 + 2 * q], tab[80 + 2 * q] = F.scaling_params(v)
    return tab


def model_dict(rpc):
    """an RPCModel as the dict the oracle's project / rmse_row_col take"""
    keys = ["col_num", "col_den", "row_num", "row_den"] + [a + b for a in ("lon", "lat", "alt", "col", "row") for b in ("_offset", "_scale")]
    return {k: np.asarray(getattr(rpc, k), dtype=np.float64) for k in keys}


def design_matrices(target, locs, table):
    """Per axis (col, row): M (n, 39) = [1, pv, -x pv] and b = x (n,) in numpy.longdouble, with the offsets / scales of `table`"""
    ld = np.longdouble
    t = np.asarray(table, dtype=np.float64)
    # normalisation in float64 like the kernel and the reference do it (these values are the fit's data), the rest extended
    L = ((locs[:, 0] - t[80]) / t[81]).astype(ld); P = ((locs[:, 1] - t[82]) / t[83]).astype(ld); H = ((locs[:, 2] - t[84]) / t[85]).astype(ld)
    pv = F.poly_vect(x=P, y=L, z=H).T
    out = []
    for a in range(2):
        x = ((target[:, a] - t[86 + 2 * a]) / t[87 + 2 * a]).astype(ld)
        out.append((np.hstack([np.ones((len(x), 1), dtype=ld), pv, -x[:, None] * pv]), x))
    return out


def unknowns(table, axis):
    """the 39 unknowns of an axis (0 col, 1 row) in the order of M's columns: num(20), den[1:](19)"""
    t = np.asarray(table, dtype=np.float64)
    num, den = (t[0:20], t[20:40]) if axis == 0 else (t[40:60], t[60:80])
    return np.concatenate([num, den[1:]])


def backward_error(M, b, x, w=None, h=0.0):
    """eta = |N x - r|_inf / (|N|_inf |x|_inf + |r|_inf) of the normal equations N = M' W M + h^2 I, r = M' W b, in longdouble"""
    ld = np.longdouble
    W = np.ones(len(b), dtype=ld) if w is None else np.asarray(w, dtype=ld)
    N = M.T @ (W[:, None] * M) + ld(h) * ld(h) * np.eye(M.shape[1], dtype=ld)
    r = M.T @ (W * b)
    x = np.asarray(x, dtype=ld)
    return float(np.abs(N @ x - r).max() / (np.abs(N).sum(axis=1).max() * np.abs(x).max() + np.abs(r).max()))


def solve_float64(M, b, w=None, h=0.0):
    """numpy.linalg.solve on the float64 normal equations of the same system: the yardstick"""
    M = np.asarray(M, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    W = np.ones(len(b)) if w is None else np.asarray(w, dtype=np.float64)
    return np.linalg.solve(M.T @ (W[:, None] * M) + h * h * np.eye(M.shape[1]), M.T @ (W * b))


def weights(M, x):
    """1 / den^2 of the model x on the samples of M (float64, the kernel's arithmetic up to the order of the sum)"""
    den = 1.0 + np.asarray(M[:, 1:20], dtype=np.float64) @ np.asarray(x[20:], dtype=np.float64)
    return 1.0 / (den * den)

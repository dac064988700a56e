"""
Scenarios of the initial triangulation (csrc/satba_triangulate.h, csrc/satba_triangulate_api.inc, satba/ft_triangulate.py) shared by
tests/test_triangulate_cases_host.py, tests/test_gpu_triangulate_edges.py and tools/tri_accuracy.py.  Nothing here needs a GPU or the
reference: the builders make the shapes at which the kernels change path -- the three homes of the RPC tables, a second round of the
grid-stride loop, long tracks and short track lists in a handle's sliced layout -- and `triangulate_ld` is the yardstick of the
linear triangulation, the null vector of the DLT matrix in numpy.longdouble.
"""
import numpy as np

from oracle import triangulate_oracle as T
from satba import ba_rotate, cam_utils, synth

# ---------------------------------------------------------------------------------------------------------------------------------
# A. where tri_run puts the RPC tables
#
# The device copy of the tables has TRI_RPC_STRIDE = 91 doubles per camera: 728 bytes.  tri_run keeps them in dynamic LDS without
# asking while they fit the 48 KB every launch may have,
#       67 * 728 = 48 776 <= 49 152 < 49 504 = 68 * 728                                       M <= 67,
# in dynamic LDS after raising the kernel's limit while they leave 20 KB of the workgroup's 160 KB (gfx950) to the kernel,
#       196 * 728 = 142 688 <= 163 840 - 20 480 = 143 360 < 143 416 = 197 * 728               68 <= M <= 196,
# and in global memory (k_tri_points<2, false>, TabGlobal, 90 doubles per camera) above that: M >= 197.
TRI_RPC_STRIDE = 91
LDS_DEFAULT = 48 * 1024
LDS_OPTIN_GFX950 = 160 * 1024
LDS_RESERVE = 20 * 1024
PLACEMENT_M = (12, 67, 68, 196, 197, 230)
PLACEMENT_TRACKS = 120
PLACEMENT_PAIRS = 60


def rpc_table_home(M, lds_optin=LDS_OPTIN_GFX950):
    """"lds" | "lds_optin" | "global": tri_run's choice restated from its constants."""
    tab_bytes = 8 * M * TRI_RPC_STRIDE
    if tab_bytes + LDS_RESERVE > lds_optin:
        return "global"
    return "lds" if tab_bytes <= LDS_DEFAULT else "lds_optin"


def placement_pairs(M, n=PLACEMENT_PAIRS, seed=0):
    """At most n pairs (i < j, i + j odd: the two shipped RPCs alternate and cameras of equal parity have no parallax) in ascending
    order, with (0, 1), (M - 2, M - 1) and a pair that joins camera 0 or 1 to camera M - 1 among them: the first and the last row of
    the table are read.  Twelve cameras only have 36 such pairs: all of them."""
    cand = [(i, j) for i in range(M) for j in range(i + 1, M) if (i + j) % 2 == 1]
    must = [(0, 1), (M - 2, M - 1), ((M - 1) % 2 ^ 1, M - 1)]
    assert all(pr in cand for pr in must)
    rest = [pr for pr in cand if pr not in must]
    rng = np.random.default_rng([seed, M])
    pick = rng.choice(len(rest), size=min(max(n - len(must), 0), len(rest)), replace=False)
    return sorted(must + [rest[int(k)] for k in pick])


def full_scene(model, M, N, seed, **kw):
    """Every camera sees every track (obs_per_pt = M makes the visibility draw certain)."""
    scene = synth.make_scene(model, M, N, M, seed=seed, **kw)
    assert scene.n_obs == M * N
    return scene


def n_tri_reference(pts_ind, cam_ind, n_pts, n_cam, pairs):
    """Triangulations per track as the reference's pair loop performs them (ref:ft_triangulate.py:96-106)."""
    seen = np.zeros((n_cam, n_pts), dtype=bool)
    seen[np.asarray(cam_ind), np.asarray(pts_ind)] = True
    n = np.zeros(n_pts, dtype=np.int64)
    for c_i, c_j in pairs:
        if c_i < n_cam and c_j < n_cam:
            n += seen[c_i] & seen[c_j]
    return n


# ---------------------------------------------------------------------------------------------------------------------------------
# B. more than one round of k_tri_points' grid-stride loop: its grid is capped at 256 * 64 workgroups of 256 threads
GRID_ROUND = 256 * 64 * 256  # 4 194 304 triangulations
ROUNDS_TRACKS = 293          # prime: the tiles straddle workgroups and lanes
ROUNDS_CAMS = 8
ROUNDS = {"affine": 512, "rpc": 900}  # tiles: 28 pairs x 293 x 512 = 4 200 448, 16 pairs x 293 x 900 = 4 219 200


def rounds_pairs(model):
    ok = (lambda i, j: (i + j) % 2 == 1) if model == "rpc" else (lambda i, j: True)
    return [(i, j) for i in range(ROUNDS_CAMS) for j in range(i + 1, ROUNDS_CAMS) if ok(i, j)]


def tile_observations(scene, reps):
    """(pts_ind, cam_ind, pts2d, n_pts) of `reps` copies of the scene's tracks, one after the other."""
    r = np.arange(reps, dtype=np.int64)[:, None]
    pts_ind = (scene.pts_ind[None, :] + r * scene.n_pts).ravel()
    return pts_ind, np.tile(scene.cam_ind, reps), np.tile(scene.pts2d, (reps, 1)), scene.n_pts * reps


# ---------------------------------------------------------------------------------------------------------------------------------
# C. the linear triangulation in extended precision
SEPARATIONS = (0.3, 3e-2, 3e-3, 3e-4, 3e-5)  # rad between the two views
NOISES = (0.0, 0.3)                          # px
LINEAR_CLASSES = [(model, delta, noise) for model in ("affine", "perspective") for delta in SEPARATIONS for noise in NOISES]
LD = np.longdouble
LD_THRESHOLD = 1e-19
LD_SWEEPS = 60


def _dlt(P1, P2, a, b, dtype):
    P1, P2, a, b = (np.asarray(v, dtype=np.float64).astype(dtype) for v in (P1, P2, a, b))
    return np.stack([a[:, 0:1] * P1[2] - P1[0], a[:, 1:2] * P1[2] - P1[1], b[:, 0:1] * P2[2] - P2[0], b[:, 1:2] * P2[2] - P2[1]], axis=1)


def null_vector_ld(A):
    """Right singular vector of the smallest singular value of every 4 x 4 matrix of A (n, 4, 4), numpy.longdouble: one-sided Jacobi
    rotations of the columns until every pair of columns is orthogonal to 1e-19 (at most 60 sweeps)."""
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    V = np.broadcast_to(np.eye(4, dtype=LD), (n, 4, 4)).copy()
    for _ in range(LD_SWEEPS):
        rotated = False
        for p in range(3):
            for q in range(p + 1, 4):
                al = (A[:, :, p] * A[:, :, p]).sum(axis=1); be = (A[:, :, q] * A[:, :, q]).sum(axis=1)
                ga = (A[:, :, p] * A[:, :, q]).sum(axis=1)
                act = (ga != 0) & ~(np.abs(ga) <= LD(LD_THRESHOLD) * np.sqrt(al * be))
                if not act.any():
                    continue
                rotated = True
                z = (be - al) / (2 * np.where(act, ga, LD(1)))
                t = np.where(z != 0, np.sign(z) / (np.abs(z) + np.sqrt(1 + z * z)), LD(1))
                c = np.where(act, 1 / np.sqrt(1 + t * t), LD(1))
                s = np.where(act, c * t, LD(0))
                for M in (A, V):
                    mp, mq = M[:, :, p].copy(), M[:, :, q].copy()
                    M[:, :, p] = c[:, None] * mp - s[:, None] * mq
                    M[:, :, q] = s[:, None] * mp + c[:, None] * mq
        if not rotated:
            break
    k = np.argmin((A * A).sum(axis=1), axis=1)
    return V[np.arange(n), :, k]


def null_vector_ld_scalar(A):
    """The same for one 4 x 4 matrix, written with scalars (what tools/tri_accuracy.py carried): the check of null_vector_ld."""
    A = np.array(A, dtype=LD)
    V = np.eye(4, dtype=LD)
    for _ in range(LD_SWEEPS):
        rot = False
        for p in range(3):
            for q in range(p + 1, 4):
                al, be, ga = (A[:, p] * A[:, p]).sum(), (A[:, q] * A[:, q]).sum(), (A[:, p] * A[:, q]).sum()
                if ga == 0 or abs(ga) <= LD(LD_THRESHOLD) * np.sqrt(al * be):
                    continue
                rot = True
                z = (be - al) / (2 * ga)
                t = np.sign(z) / (abs(z) + np.sqrt(1 + z * z)) if z != 0 else LD(1)
                c = 1 / np.sqrt(1 + t * t); s = c * t
                A[:, [p, q]] = np.stack([c * A[:, p] - s * A[:, q], s * A[:, p] + c * A[:, q]], 1)
                V[:, [p, q]] = np.stack([c * V[:, p] - s * V[:, q], s * V[:, p] + c * V[:, q]], 1)
        if not rot:
            break
    return V[:, int(np.argmin((A * A).sum(0)))]


def triangulate_ld(P1, P2, a, b, scalar=False):
    """linear_triangulation_multiple_pts in numpy.longdouble from the float64 inputs; (n, 3) longdouble."""
    A = _dlt(P1, P2, a, b, LD)
    X = np.stack([null_vector_ld_scalar(m) for m in A]) if scalar else null_vector_ld(A)
    return X[:, :3] / X[:, 3:4]


def triangulate_lapack(P1, P2, a, b):
    """The same null vector from numpy.linalg.svd (a bidiagonalising SVD): what the Jacobi method is preferred to."""
    vt = np.linalg.svd(_dlt(P1, P2, a, b, np.float64))[2][:, 3, :]
    return vt[:, :3] / vt[:, 3:4]


def error_m(X, ref):
    """Distance of every point to the extended-precision one, metres (float64)."""
    return np.sqrt((((np.asarray(X).astype(LD) - ref) ** 2).sum(axis=1))).astype(np.float64)


def affine_pair(delta, rng):
    """Two affine cameras of synth.make_affine_scene's kind; the second has the first's Euler angles but for the first, moved by delta."""
    c = synth.SCENE_CENTRE
    angles = rng.uniform(-0.5, 0.5, 3)
    cams = []
    for k in range(2):
        u = rng.uniform(-1.0, 1.0, 3)
        K = np.array([[1 + 0.05 * u[0], 0.01 * u[1]], [0.0, 1 + 0.05 * u[2]]])
        R = ba_rotate.euler_angles_to_R(*(angles + np.array([k * delta, 0.0, 0.0])))
        cams.append(cam_utils.compose_affine_camera(K, R, -R[:2] @ c + rng.uniform(2000.0, 4000.0, 2)))
    return cams


def perspective_pair(delta, rng):
    """Two pinhole cameras of synth.make_perspective_scene's kind, 600 km above the scene centre and looking at it; the second
    centre is the first moved by delta along the arc around the scene centre."""
    c = synth.SCENE_CENTRE
    up = c / np.linalg.norm(c)
    d = up + 0.3 * rng.uniform(-1, 1, 3)
    d /= np.linalg.norm(d)
    side = np.cross(d, rng.uniform(-1, 1, 3))
    side /= np.linalg.norm(side)
    cams = []
    for k in range(2):
        dk = np.cos(k * delta) * d + np.sin(k * delta) * side
        oC = c + 6.0e5 * dk
        fwd = -dk
        right = np.cross(fwd, rng.uniform(-1, 1, 3))
        right /= np.linalg.norm(right)
        R = np.vstack((right, np.cross(fwd, right), fwd))
        f = 6.0e5 * (1 + 0.05 * rng.uniform(-1, 1))
        K = np.array([[f, 10.0 * rng.uniform(-1, 1), 2000 + 100 * rng.uniform(-1, 1)],
                      [0.0, f * (1 + 0.01 * rng.uniform(-1, 1)), 2000 + 100 * rng.uniform(-1, 1)], [0, 0, 1.0]])
        P = K @ np.hstack((R, -(R @ oC).reshape(3, 1)))
        cams.append(P / P[2, 3])
    return cams


def linear_class(model, delta, noise, n=100):
    """(P1, P2, obs1, obs2): n points around the scene centre (ECEF magnitudes) seen by a pair `delta` rad apart, `noise` px added."""
    rng = np.random.default_rng([17, LINEAR_CLASSES.index((model, delta, noise))])
    P1, P2 = (affine_pair if model == "affine" else perspective_pair)(delta, rng)
    X = synth.SCENE_CENTRE + rng.uniform(-5e3, 5e3, (n, 3))
    obs = []
    for P in (P1, P2):
        h = X @ P[:, :3].T + P[:, 3]
        obs.append(h[:, :2] / h[:, 2:3] + rng.normal(0.0, 1.0, (n, 2)) * noise)
    return P1, P2, obs[0], obs[1]


def restatement_error(P1, P2, a, b, ref=None):
    """Largest distance of the float64 restatement (oracle.triangulate_oracle) to the extended-precision points."""
    ref = triangulate_ld(P1, P2, a, b) if ref is None else ref
    return error_m(T.linear_triangulation_multiple_pts(P1, P2, a, b), ref).max()


# ---------------------------------------------------------------------------------------------------------------------------------
# D. long tracks and short track lists for the resident path
LONG_CAMS = 70
LONG_HAND = (70, 2, 63, 64, 65)  # lengths of the hand-built tracks; they come first, so that the first track covers every camera
PREFIX_N = (1, 63, 64, 65, 127, 128, 129, 257)


PREFIX_BASE = 295  # 300 tracks with the hand-built ones: the longest prefix (257) is a proper one and ends inside a slice


def long_track_scene(n_base=200, seed=41):
    """synth.make_affine_scene(70, n_base, 60) behind five hand-built tracks of 70, 2, 63, 64 and 65 observations.  The handle sorts
    its tracks by length, so the slices of 64 tracks mix the lengths 2 and 52 - 68, and the last one ends with 70."""
    base = synth.make_affine_scene(LONG_CAMS, n_base, 60, seed=seed)
    rng = np.random.default_rng([seed, 1])
    n_hand = len(LONG_HAND)
    X = synth.SCENE_CENTRE + rng.uniform(-5e3, 5e3, (n_hand, 3))
    pts_ind, cam_ind = [], []
    for t, length in enumerate(LONG_HAND):
        cams = np.sort(rng.choice(LONG_CAMS, size=length, replace=False))
        pts_ind.append(np.full(length, t)); cam_ind.append(cams)
    pts_ind, cam_ind = np.concatenate(pts_ind), np.concatenate(cam_ind)
    Ps = np.stack(base.cameras_true)
    pts2d = np.einsum("kij,kj->ki", Ps[cam_ind][:, :2, :3], X[pts_ind]) + Ps[cam_ind][:, :2, 3] + rng.normal(0.0, 0.3, (pts_ind.size, 2))
    return synth.Scene(cam_model="affine", n_cam=LONG_CAMS, n_pts=base.n_pts + n_hand, cameras=base.cameras, cameras_true=base.cameras_true,
                       pts3d=np.vstack((X + rng.normal(0.0, 2.0, X.shape), base.pts3d)), pts3d_true=np.vstack((X, base.pts3d_true)),
                       pts_ind=np.concatenate((pts_ind, base.pts_ind + n_hand)), cam_ind=np.concatenate((cam_ind, base.cam_ind)),
                       pts2d=np.vstack((pts2d, base.pts2d)), camera_centers=base.camera_centers, pairs_to_triangulate=[(0, 1)])


def prefix_scene(scene, n):
    """The first n tracks of a scene (observation lists are point-major)."""
    k = int(np.searchsorted(scene.pts_ind, n))
    d = dict(scene.__dict__, n_pts=n, pts3d=scene.pts3d[:n], pts3d_true=scene.pts3d_true[:n], pts_ind=scene.pts_ind[:k],
             cam_ind=scene.cam_ind[:k], pts2d=scene.pts2d[:k])
    return synth.Scene(**d)


def long_pairs(general, n=None, seed=3):
    """Every pair (i < j) of the 70 cameras in ascending order (2 415: a track of 70 cameras lists them all, a hundred refills of the
    24-entry buffer), or -- general -- shuffled, with a duplicate and a reversed pair at the end.  n: only that many of them."""
    pairs = [(i, j) for i in range(LONG_CAMS) for j in range(i + 1, LONG_CAMS)]
    if n is not None:
        keep = np.sort(np.random.default_rng([seed, n]).choice(len(pairs), size=n, replace=False))
        pairs = [pairs[int(k)] for k in keep]
    if general:
        order = np.random.default_rng(seed).permutation(len(pairs))
        pairs = [pairs[int(k)] for k in order]
        pairs += [pairs[1], (pairs[3][1], pairs[3][0])]
    return pairs


def batched_oracle(scene, pairs, tracks):
    """Rows `tracks` of oracle.triangulate_oracle.init_pts3d of a linear scene, with the float64 triangulations of all pairs made in
    one call (the oracle's pair loop calls the Jacobi routine once per pair: too slow for thousands of pairs)."""
    C = scene.to_dense_C()[:, np.asarray(tracks)]
    seen = ~np.isnan(C[::2])
    P = np.stack([np.asarray(c, dtype=np.float64) for c in scene.cameras])
    todo = [(c_i, c_j, np.where(seen[c_i] & seen[c_j])[0]) for c_i, c_j in dict.fromkeys(pairs) if c_i < scene.n_cam and c_j < scene.n_cam]
    ci = np.concatenate([np.full(t.size, c_i) for c_i, _, t in todo]); cj = np.concatenate([np.full(t.size, c_j) for _, c_j, t in todo])
    tt = np.concatenate([t for _, _, t in todo])
    a = np.stack([C[2 * ci, tt], C[2 * ci + 1, tt]], axis=1); b = np.stack([C[2 * cj, tt], C[2 * cj + 1, tt]], axis=1)
    A = np.empty((tt.size, 4, 4))
    A[:, 0] = a[:, 0:1] * P[ci, 2] - P[ci, 0]; A[:, 1] = a[:, 1:2] * P[ci, 2] - P[ci, 1]
    A[:, 2] = b[:, 0:1] * P[cj, 2] - P[cj, 0]; A[:, 3] = b[:, 1:2] * P[cj, 2] - P[cj, 1]
    X = T._null_vector_jacobi(A)
    X = X[:, :3] / X[:, 3:4]
    ofs = np.concatenate(([0], np.cumsum([t.size for _, _, t in todo])))
    table = {(c_i, c_j): X[ofs[k]:ofs[k + 1]] for k, (c_i, c_j, _) in enumerate(todo)}
    return T.init_pts3d(C, scene.cameras, scene.cam_model, pairs, triangulate=lambda c_i, c_j, oi, oj: table[(c_i, c_j)])

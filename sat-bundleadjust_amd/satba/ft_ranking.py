"""
Selection of an optimal subset of feature tracks, on the device (the names of
ref:bundle_adjust/feature_tracks/ft_ranking.py; "Tracks selection for robust, efficient and scalable large-scale structure from
motion", Pattern Recognition 2017; DESIGN.md "Track selection").

`build_connectivity_matrix`, `compute_camera_weights`, `order_tracks`, `compute_C_reproj`, `select_best_tracks` and
`select_best_tracks_sensor_aware` keep the reference's signatures and return values.  The work is in csrc/satba_tracks.h behind
`satba_track_keys` / `satba_track_connectivity` / `satba_select_tracks` (include/satba.h); there is no CPU fallback: without
libsatba_hip.so or without a GPU the calls raise.

`select_best_tracks_from_observations` is the same selection for callers that hold observation lists (BundleAdjustmentParameters:
pts_ind / cam_ind) with one keypoint scale and one reprojection error per observation, and never build the dense matrices.

Not here: `compute_C_scale` (reads keypoint files: host I/O; see satba.ft_utils) and `print_quick_camera_weights`.
"""
import ctypes as ct
import timeit

import numpy as np

from . import engine_hip as E
from .ft_triangulate import _device
from .loader import flush_print

PRIORITY_NAMES = ("length", "scale", "cost")
_lp = ct.POINTER(ct.c_int64)


def _priority_codes(priority):
    """names -> the three codes of satba_select_tracks (-1: unused; the library completes the list by numpy's rule)."""
    names = list(priority)
    if len(names) > 3:
        raise ValueError("priority names at most three keys, got {}".format(names))
    codes = []
    for n in names:
        if n not in PRIORITY_NAMES:
            raise ValueError("unknown priority name {!r}: one of {}".format(n, list(PRIORITY_NAMES)))
        if PRIORITY_NAMES.index(n) in codes:
            raise ValueError("priority names {!r} twice".format(n))
        codes.append(PRIORITY_NAMES.index(n))
    return np.array(codes + [-1] * (3 - len(codes)), dtype=np.int32)


def _group(pts_ind, cam_ind, n_cam, n_pts, *per_obs):
    """Observations grouped by track with cameras ascending (as ft_triangulate.init_pts3d passes them): (pt_ofs, cam32, *per_obs)."""
    pts_ind = np.asarray(pts_ind); cam_ind = np.asarray(cam_ind)
    if pts_ind.ndim != 1 or cam_ind.shape != pts_ind.shape:
        raise ValueError("pts_ind and cam_ind must be vectors of one length")
    vals = []
    for v in per_obs:
        if v is not None:
            v = np.asarray(v, dtype=np.float64)
            if v.shape != pts_ind.shape:
                raise ValueError("one value per observation expected: {} values for {} observations".format(v.size, pts_ind.size))
        vals.append(v)
    n_pts, n_cam = int(n_pts), int(n_cam)
    if n_pts < 0 or n_cam <= 0:
        raise ValueError("n_cam must be positive and n_pts must not be negative")
    pts_ind = pts_ind.astype(np.int64); cam_ind = cam_ind.astype(np.int64)
    if pts_ind.size and (pts_ind.min() < 0 or pts_ind.max() >= n_pts):
        raise ValueError("pts_ind out of range")
    if cam_ind.size and (cam_ind.min() < 0 or cam_ind.max() >= n_cam):
        raise ValueError("cam_ind out of range")
    key = pts_ind * n_cam + cam_ind
    if np.any(key[1:] <= key[:-1]):
        order = np.argsort(key, kind="stable")
        key = key[order]
        if np.any(key[1:] == key[:-1]):
            raise ValueError("an observation (track, camera) is listed twice")
        pts_ind, cam_ind = pts_ind[order], cam_ind[order]
        vals = [None if v is None else v[order] for v in vals]
    ofs = np.zeros(n_pts + 1, dtype=np.int64)
    np.cumsum(np.bincount(pts_ind, minlength=n_pts), out=ofs[1:])
    return [ofs, np.ascontiguousarray(cam_ind, dtype=np.int32)] + [None if v is None else np.ascontiguousarray(v) for v in vals]


def _observations_of(C):
    """(pts_ind, cam_ind, seen) of a (2 n_cam, n_tracks) correspondence matrix: grouped by track, cameras ascending."""
    C = np.asarray(C)
    if C.ndim != 2 or C.shape[0] % 2:
        raise ValueError("C must have shape (2 * n_cam, n_tracks)")
    seen = ~np.isnan(C[::2])
    pts_ind, cam_ind = np.nonzero(seen.T)
    return pts_ind, cam_ind, seen


def _values_of(M, seen, pts_ind, cam_ind, name):
    M = np.asarray(M, dtype=np.float64)
    if M.shape != seen.shape:
        raise ValueError("{} must have shape (n_cam, n_tracks) = {}, got {}".format(name, seen.shape, M.shape))
    if not np.array_equal(~np.isnan(M), seen):
        raise ValueError("{} must hold a value exactly where C holds an observation".format(name))
    return M[cam_ind, pts_ind]


def _connectivity(ofs, cam32, n_cam, n_pts, alive, min_matches, device):
    lib = E.load_library()
    A = np.zeros((n_cam, n_cam), dtype=np.int32)
    a8 = None if alive is None else np.ascontiguousarray(alive, dtype=np.uint8)
    E._check(lib, lib.satba_track_connectivity(n_cam, n_pts, ofs.ctypes.data_as(_lp), E._ptr(cam32, E._ip),
                                               a8.ctypes.data_as(ct.POINTER(ct.c_uint8)) if a8 is not None else None,
                                               int(min_matches), E._ptr(A, E._ip), _device(device)))
    return A


def build_connectivity_matrix(C, min_matches=10):
    """
    ref:bundle_adjust/feature_tracks/ft_ranking.py:19-34: A (n_cam, n_cam) float64, A[i, j] = tracks seen in both cameras, zero
    where fewer than min_matches.
    """
    pts_ind, cam_ind, seen = _observations_of(C)
    n_cam, n_pts = seen.shape
    ofs, cam32 = _group(pts_ind, cam_ind, n_cam, n_pts)
    return _connectivity(ofs, cam32, n_cam, n_pts, None, min_matches, None).astype(np.float64)


def track_keys_from_observations(pts_ind, cam_ind, scale, err, n_cam, n_pts, device=None):
    """The ranking keys of every track: (length int32, scale float64 rounded to 2 decimals, cost float64)."""
    lib = E.load_library()
    ofs, cam32, sc, er = _group(pts_ind, cam_ind, n_cam, n_pts, scale, err)
    n_pts = ofs.size - 1
    length = np.zeros(n_pts, dtype=np.int32); ks = np.zeros(n_pts); kc = np.zeros(n_pts)
    E._check(lib, lib.satba_track_keys(n_pts, ofs.ctypes.data_as(_lp), E._ptr(sc), E._ptr(er) if er is not None else None,
                                       E._ptr(length, E._ip), E._ptr(ks), E._ptr(kc), _device(device)))
    return length, ks, kc


def select_best_tracks_from_observations(pts_ind, cam_ind, scale, err, n_cam, n_pts, K=30, priority=("length", "scale", "cost"),
                                         return_info=False, device=None):
    """
    select_best_tracks for observation lists: pts_ind (n_obs,), cam_ind (n_obs,), scale (n_obs,), err (n_obs,) or None (zeros), in
    any order (grouped by track, cameras ascending, here).  Returns the sorted indices of the selected tracks; with return_info
    also a dict: tree_of (n_pts,: the tree that took the track or -1), n_trees, weights (K, n_cam: the camera weights every tree
    started from), rank (n_pts,: position in the ranking), kernel_ms.
    """
    codes = _priority_codes(priority)
    K = int(K)
    if K < 0:
        raise ValueError("K must not be negative")
    if scale is None:
        raise ValueError("one keypoint scale per observation is required")
    ofs, cam32, sc, er = _group(pts_ind, cam_ind, n_cam, n_pts, scale, err)
    n_cam, n_pts = int(n_cam), int(n_pts)
    lib = E.load_library()
    tree_of = np.full(max(n_pts, 1), -1, dtype=np.int32)
    rank = np.zeros(max(n_pts, 1), dtype=np.int64)
    weights = np.zeros((K, n_cam))
    n_sel, n_trees, ms = ct.c_int64(0), ct.c_int32(0), ct.c_float(0.0)
    E._check(lib, lib.satba_select_tracks(n_cam, n_pts, ofs.ctypes.data_as(_lp), E._ptr(cam32, E._ip), E._ptr(sc),
                                          E._ptr(er) if er is not None else None, K, E._ptr(codes, E._ip), E._ptr(tree_of, E._ip),
                                          ct.byref(n_sel), ct.byref(n_trees), E._ptr(weights) if K else None, rank.ctypes.data_as(_lp),
                                          _device(device), ct.byref(ms)))
    tree_of, rank = tree_of[:n_pts], rank[:n_pts]
    S = np.nonzero(tree_of >= 0)[0]
    if S.size != n_sel.value:
        raise E.SatbaError("satba_select_tracks reported {} tracks but marked {}".format(n_sel.value, S.size))
    if return_info:
        return S, {"tree_of": tree_of, "n_trees": int(n_trees.value), "weights": weights, "rank": rank, "kernel_ms": ms.value}
    return S


def compute_camera_weights(C, C_reproj, connectivity_matrix=None):
    """
    ref:bundle_adjust/feature_tracks/ft_ranking.py:83-118: W(camera) = neighbours(camera) + exp(-cost(camera)), a list of n_cam
    floats.  These are the weights the first tree of the selection starts from (satba_select_tracks with K = 1); a connectivity
    matrix other than build_connectivity_matrix(C, 0) has no counterpart on the device.
    """
    pts_ind, cam_ind, seen = _observations_of(C)
    n_cam, n_pts = seen.shape
    if connectivity_matrix is not None:
        A0 = _connectivity(*_group(pts_ind, cam_ind, n_cam, n_pts), n_cam, n_pts, None, 0, None)
        if not np.array_equal(np.asarray(connectivity_matrix) > 0, A0 > 0):
            raise ValueError("connectivity_matrix must be build_connectivity_matrix(C, min_matches=0)")
    err = _values_of(C_reproj, seen, pts_ind, cam_ind, "C_reproj")
    if n_pts == 0:
        return [1.0] * n_cam
    _, info = select_best_tracks_from_observations(pts_ind, cam_ind, np.zeros(err.size), err, n_cam, n_pts, K=1, return_info=True)
    return [float(w) for w in info["weights"][0]]


def order_tracks(C, C_scale, C_reproj, priority=["length", "scale", "cost"]):
    """
    ref:bundle_adjust/feature_tracks/ft_ranking.py:136-153: ranking of the tracks in decreasing priority, a dict
    {index of the track in C: position in the ranking}.
    """
    pts_ind, cam_ind, seen = _observations_of(C)
    n_cam, n_pts = seen.shape
    scale = _values_of(C_scale, seen, pts_ind, cam_ind, "C_scale")
    err = _values_of(C_reproj, seen, pts_ind, cam_ind, "C_reproj")
    _, info = select_best_tracks_from_observations(pts_ind, cam_ind, scale, err, n_cam, n_pts, K=0, priority=priority, return_info=True)
    order = np.argsort(info["rank"], kind="stable")
    return dict(zip(order, np.arange(n_pts)))


def compute_C_reproj(C, pts3d, cameras, cam_model, pairs_to_triangulate, camera_centers):
    """
    ref:bundle_adjust/feature_tracks/ft_ranking.py:56-80: (n_cam, n_tracks) matrix with the reprojection error of every
    observation at the current parameters, NaN elsewhere.  The errors come from satba_reprojection_errors.
    """
    from . import ba_core
    from .ba_params import BundleAdjustmentParameters

    args = [C, pts3d, cameras, cam_model, pairs_to_triangulate, camera_centers]
    p = BundleAdjustmentParameters(*args, {"reduce": False, "verbose": False})
    eng = ba_core.get_engine(p)
    eng.configure("linear", 1.0)
    eng.set_x(ba_core._frozen_vars(np.array(p.params_opt, dtype=np.float64), p))
    err = eng.reprojection_errors()
    n_cam, n_pts = np.asarray(C).shape[0] // 2, np.asarray(C).shape[1]
    C_reproj = np.full((n_cam, n_pts), np.nan)
    C_reproj[p.cam_ind, p.pts_ind] = err
    return C_reproj


def select_best_tracks(C, C_scale, C_reproj, K=30, priority=["length", "scale", "cost"], verbose=False):
    """
    ref:bundle_adjust/feature_tracks/ft_ranking.py:266-289: ranks the tracks (order_tracks), then grows K spanning trees over the
    camera graph (get_tracks).  Returns the indices of the selected columns of C (sorted; the reference returns the same set in
    the iteration order of Python sets).
    """
    t0 = timeit.default_timer()
    if verbose:
        flush_print("\nRunning feature tracks selection algorithm...")
    pts_ind, cam_ind, seen = _observations_of(C)
    n_cam, n_pts = seen.shape
    scale = _values_of(C_scale, seen, pts_ind, cam_ind, "C_scale")
    err = _values_of(C_reproj, seen, pts_ind, cam_ind, "C_reproj")
    S = select_best_tracks_from_observations(pts_ind, cam_ind, scale, err, n_cam, n_pts, K=K, priority=priority)
    if verbose:
        obs_per_cam = seen.sum(axis=1)
        obs_per_cam_after = seen[:, S].sum(axis=1)
        flush_print("...done in {:.2f} seconds".format(timeit.default_timer() - t0))
        flush_print("Selected {} tracks out of {} ({:.2f}%)".format(len(S), n_pts, 100.0 * len(S) / n_pts))
        flush_print("     - priority: {}".format(priority))
        flush_print("     - obs per cam before: {}".format(obs_per_cam))
        flush_print("     - obs per cam after:  {}\n".format(obs_per_cam_after))
    return np.array(S)


def select_best_tracks_sensor_aware(images, C, C_scale, C_reproj, K=30, priority=["length", "scale", "cost"], verbose=False):
    """
    ref:bundle_adjust/feature_tracks/ft_ranking.py:292-316: the selection per SkySat sensor ("d1_", "d2_", "d3_" in the image's
    geotiff_path) over the tracks linking at least two of its cameras, united with the selection over all cameras.
    """
    C, C_scale, C_reproj = np.asarray(C), np.asarray(C_scale), np.asarray(C_reproj)
    seen = ~np.isnan(C[::2])
    kw = dict(K=K, priority=priority, verbose=verbose)
    picked = [select_best_tracks(C, C_scale, C_reproj, **kw)]
    for sensor in ("d1_", "d2_", "d3_"):
        cams = np.array([i for i, im in enumerate(images) if sensor in im.geotiff_path], dtype=np.int64)
        if cams.size < 2:
            continue
        tracks = np.nonzero(seen[cams].sum(axis=0) >= 2)[0]  # the tracks linking at least two cameras of this sensor
        rows = np.stack((2 * cams, 2 * cams + 1), axis=1).ravel()
        sub = select_best_tracks(C[np.ix_(rows, tracks)], C_scale[np.ix_(cams, tracks)], C_reproj[np.ix_(cams, tracks)], **kw)
        picked.append(tracks[sub])
    return np.unique(np.concatenate(picked).astype(np.int32))

"""
Feature tracks from pairwise matches, on the device (the names of ref:bundle_adjust/feature_tracks/ft_utils.py; DESIGN.md
"Track construction").

`feature_tracks_from_pairwise_matches` and `filter_C_using_pairs_to_triangulate` keep the reference's signatures and return
values; `compute_C_scale` is ref:bundle_adjust/feature_tracks/ft_ranking.py:37-53 as plain host code (a gather).  The work is in
csrc/satba_ftracks.h behind `satba_ftracks_build` / `satba_tracks_have_pair` (include/satba.h); there is no CPU fallback: without
libsatba_hip.so or without a GPU the calls raise.

`feature_tracks_from_matches` is the same construction for callers that hold the keypoints in memory and want observation lists
(what `ft_triangulate.init_pts3d_from_observations` and `ft_ranking.select_best_tracks_from_observations` take): the dense matrices
are never built.

The columns come in the order of the smallest global keypoint id of each track, not in the order of the reference's union-find
roots, which depends on the sequence of the match rows; nothing downstream uses that order.  A row with im_i > im_j is accepted as
the same graph edge; im_i == im_j is an error.

Not here: `check_pairs` / `check_correspondence_matrix` (O(n_cam) bookkeeping on the host) and the plotting helpers.
"""
import ctypes as ct

import numpy as np

from . import engine_hip as E
from .ft_ranking import _group, _observations_of
from .ft_triangulate import _device

_lp = ct.POINTER(ct.c_int64)
_fp = ct.POINTER(ct.c_float)
_bp = ct.POINTER(ct.c_uint8)


def _pairs_array(pairs_to_triangulate):
    pairs = np.asarray(list(pairs_to_triangulate), dtype=np.int64).reshape(-1, 2) if len(pairs_to_triangulate) else np.zeros((0, 2), np.int64)
    if pairs.size and (np.abs(pairs).max() >= 2 ** 31):
        raise ValueError("pairs_to_triangulate holds camera indices beyond 32 bits")
    return np.ascontiguousarray(pairs, dtype=np.int32)


def _check_inputs(kp, kp_ofs, pairwise_matches, n_cam):
    kp = np.asarray(kp)
    if kp.ndim != 2 or kp.shape[1] < 3:
        raise ValueError("kp must have shape (n_kp_total, >= 3): x, y, scale; got {}".format(kp.shape))
    kp_ofs = np.asarray(kp_ofs)
    if kp_ofs.ndim != 1 or kp_ofs.size < 2 or kp_ofs.dtype.kind not in "iu":
        raise ValueError("kp_ofs must be an integer vector of n_cam + 1 offsets")
    kp_ofs = kp_ofs.astype(np.int64)
    if n_cam is None:
        n_cam = kp_ofs.size - 1
    n_cam = int(n_cam)
    if kp_ofs.size != n_cam + 1:
        raise ValueError("kp_ofs must hold n_cam + 1 = {} offsets, got {}".format(n_cam + 1, kp_ofs.size))
    if kp_ofs[0] != 0 or np.any(np.diff(kp_ofs) < 0):
        raise ValueError("kp_ofs must ascend from 0")
    if kp_ofs[-1] != kp.shape[0]:
        raise ValueError("kp holds {} keypoints but kp_ofs ends at {}".format(kp.shape[0], kp_ofs[-1]))
    m = np.asarray(pairwise_matches)
    if m.size == 0:
        m = np.zeros((0, 4), dtype=np.int32)
    if m.ndim != 2 or m.shape[1] != 4:
        raise ValueError("pairwise_matches must have 4 columns (kp_i, kp_j, im_i, im_j), got shape {}".format(m.shape))
    if m.dtype.kind not in "iu":
        if not np.array_equal(m, np.floor(m)):
            raise ValueError("pairwise_matches must hold integers")
    m = m.astype(np.int64)
    if kp_ofs[-1] >= 2 ** 31 or m.shape[0] >= 2 ** 31:
        raise ValueError("fewer than 2^31 keypoints and matches are supported")
    if m.size:
        if m.min() < 0:
            raise ValueError("pairwise_matches holds a negative index")
        if m[:, 2:].max() >= n_cam:
            raise ValueError("pairwise_matches names image {} of {}".format(m[:, 2:].max(), n_cam))
        if np.any(m[:, 2] == m[:, 3]):
            raise ValueError("a match joins two keypoints of one image")
        sizes = np.diff(kp_ofs)
        if np.any(m[:, 0] >= sizes[m[:, 2]]) or np.any(m[:, 1] >= sizes[m[:, 3]]):
            raise ValueError("pairwise_matches names a keypoint outside its image")
    kp3 = np.ascontiguousarray(kp[:, :3], dtype=np.float32)
    return kp3, kp_ofs, np.ascontiguousarray(m, dtype=np.int32), n_cam


def feature_tracks_from_matches(kp, kp_ofs, pairwise_matches, pairs_to_triangulate, n_cam=None, n_adj=0, device=None, return_info=False):
    """
    kp (n_kp_total, >= 3: x, y, scale, the keypoints of all images one after the other), kp_ofs (n_cam + 1, ascending from 0: image m
    owns kp[kp_ofs[m]:kp_ofs[m + 1]]), pairwise_matches (n, 4: kp_i, kp_j, im_i, im_j, the keypoint indices inside their images),
    pairs_to_triangulate (list of (i, j)).  Returns pts_ind, cam_ind, pts2d, kp_id, scale, n_pts, n_pts_fix: the observations
    track-major with cameras ascending inside a track, pts2d (n_obs, 2) float64 and scale (n_obs,) float64 the keypoints' float32
    values, kp_id the keypoint's index inside its image.  With n_adj > 0 the n_pts_fix tracks without an observation in a camera
    >= n_adj come first.  With return_info also a dict: pt_ofs, n_components, n_conflicts, kernel_ms.
    """
    kp3, kp_ofs, m32, n_cam = _check_inputs(kp, kp_ofs, pairwise_matches, n_cam)
    pairs = _pairs_array(pairs_to_triangulate)
    n_adj = int(n_adj)
    if n_adj < 0:
        raise ValueError("n_adj must not be negative")
    lib = E.load_library()
    handle, ms = ct.c_void_p(None), ct.c_float(0.0)
    counts = np.zeros(5, dtype=np.int64)
    E._check(lib, lib.satba_ftracks_build(n_cam, kp_ofs.ctypes.data_as(_lp), kp3.ctypes.data_as(_fp), m32.shape[0], E._ptr(m32, E._ip),
                                          pairs.shape[0], E._ptr(pairs, E._ip), n_adj, ct.byref(handle), counts.ctypes.data_as(_lp),
                                          _device(device), ct.byref(ms)))
    try:
        n_pts, n_obs = int(counts[0]), int(counts[1])
        pt_ofs = np.zeros(n_pts + 1, dtype=np.int64)
        cam_ind = np.zeros(n_obs, dtype=np.int32); kp_id = np.zeros(n_obs, dtype=np.int32)
        pts2d = np.zeros((n_obs, 2)); scale = np.zeros(n_obs)
        E._check(lib, lib.satba_ftracks_fetch(handle, pt_ofs.ctypes.data_as(_lp), E._ptr(cam_ind, E._ip), E._ptr(kp_id, E._ip), E._ptr(pts2d),
                                              E._ptr(scale)))
    finally:
        lib.satba_ftracks_destroy(handle)
    pts_ind = np.repeat(np.arange(n_pts, dtype=np.int64), np.diff(pt_ofs))
    out = (pts_ind, cam_ind, pts2d, kp_id, scale, n_pts, int(counts[2]))
    if return_info:
        return out + ({"pt_ofs": pt_ofs, "n_components": int(counts[3]), "n_conflicts": int(counts[4]), "kernel_ms": ms.value},)
    return out


def feature_tracks_from_pairwise_matches(feature_paths, pairwise_matches, pairs_to_triangulate):
    """
    ref:bundle_adjust/feature_tracks/ft_utils.py:65-182.  feature_paths: one .npy keypoint file per image (rows = keypoints, columns
    0..2 = x, y, scale; only these are read, through a memory map, and the files may differ in length).  Returns C (2 n_cam, n_tracks)
    and C_v2 (n_cam, n_tracks), float64 with NaN where a track is not observed.
    """
    blocks = [np.load(path, mmap_mode="r") for path in feature_paths]
    for path, b in zip(feature_paths, blocks):
        if b.ndim != 2 or b.shape[1] < 3:
            raise ValueError("{}: a keypoint file must have shape (n, >= 3), got {}".format(path, b.shape))
    kp_ofs = np.concatenate([[0], np.cumsum([b.shape[0] for b in blocks])]).astype(np.int64)
    kp = np.empty((int(kp_ofs[-1]), 3), dtype=np.float32)
    for m, b in enumerate(blocks):
        kp[kp_ofs[m]:kp_ofs[m + 1]] = b[:, :3]
    del blocks
    n_cam = len(feature_paths)
    pts_ind, cam_ind, pts2d, kp_id, _, n_pts, _, info = feature_tracks_from_matches(kp, kp_ofs, pairwise_matches, pairs_to_triangulate,
                                                                                    n_cam=n_cam, return_info=True)
    C = np.full((2 * n_cam, n_pts), np.nan)
    C_v2 = np.full((n_cam, n_pts), np.nan)
    C[2 * cam_ind, pts_ind] = pts2d[:, 0]
    C[2 * cam_ind + 1, pts_ind] = pts2d[:, 1]
    C_v2[cam_ind, pts_ind] = kp_id
    print("C.shape before baseline check {}".format((2 * n_cam, info["n_components"])))
    print("C.shape after baseline check {}".format(C.shape))
    return C, C_v2


def tracks_have_pair(pts_ind, cam_ind, n_cam, n_pts, pairs_to_triangulate, device=None):
    """(n_pts,) bool: the track holds both cameras of a listed pair (i, j), i < j < n_cam (ft_utils.py:38-62 on observation lists)."""
    ofs, cam32 = _group(pts_ind, cam_ind, n_cam, n_pts)
    pairs = _pairs_array(pairs_to_triangulate)
    n_cam, n_pts = int(n_cam), int(n_pts)
    lib = E.load_library()
    keep = np.zeros(max(n_pts, 1), dtype=np.uint8)
    E._check(lib, lib.satba_tracks_have_pair(n_cam, n_pts, ofs.ctypes.data_as(_lp), E._ptr(cam32, E._ip), pairs.shape[0], E._ptr(pairs, E._ip),
                                             keep.ctypes.data_as(_bp), _device(device)))
    return keep[:n_pts].astype(bool)


def filter_C_using_pairs_to_triangulate(C, pairs_to_triangulate):
    """
    ref:bundle_adjust/feature_tracks/ft_utils.py:38-62: indices of the columns of C that hold both cameras of at least one pair of
    pairs_to_triangulate.
    """
    pts_ind, cam_ind, seen = _observations_of(C)
    n_cam, n_pts = seen.shape
    if n_pts == 0:
        return np.zeros(0, dtype=np.int64)
    return np.nonzero(tracks_have_pair(pts_ind, cam_ind, n_cam, n_pts, pairs_to_triangulate))[0]


def compute_C_scale(C_v2, features):
    """
    ref:bundle_adjust/feature_tracks/ft_ranking.py:37-53: (n_cam, n_tracks) matrix with the scale (column 2 of the keypoint file
    features[cam]) of every observation of C_v2, NaN elsewhere.  The observation path needs none of this: the build returns `scale`.
    """
    C_v2 = np.asarray(C_v2, dtype=np.float64)
    if C_v2.ndim != 2 or C_v2.shape[0] != len(features):
        raise ValueError("C_v2 must have one row per keypoint file")
    C_scale = np.full(C_v2.shape, np.nan)
    for cam, path in enumerate(features):
        cols = np.nonzero(~np.isnan(C_v2[cam]))[0]
        if cols.size:
            C_scale[cam, cols] = np.load(path, mmap_mode="r")[C_v2[cam, cols].astype(np.int64), 2]
    return C_scale

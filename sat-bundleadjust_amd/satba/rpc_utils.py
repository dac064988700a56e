"""
Affine fundamental matrices of image pairs from their RPCs (the names of ref:bundle_adjust/s2p/rpc_utils.py and
ref:bundle_adjust/s2p/estimation.py): what ref:bundle_adjust/feature_tracks/ft_pipeline.py:139-152
(init_F_pair_to_match) computes pair by pair on the host, here for all pairs of a call in one launch
(csrc/satba_fundamental.h behind `satba_rpc_fundamental`).  There is no CPU fallback: without libsatba_hip.so or without a GPU the
device calls raise.  `rpc` is anything with the attribute names of rpcm.RPCModel (satba.rpc_model.rpc_to_table).

Sign.  An affine fundamental matrix and its negative are the same matrix to every user (the rectifying similarities of -F negate
both rectified ordinates, so the epipolar gate |y1' - y2'| of the matching does not move).  The sign the reference returns is what
LAPACK's SVD happens to leave and flips between crops of one pair; the device fixes it: the entry of (F02, F12, F20, F21) with the
largest magnitude is positive.
"""
import ctypes as ct

import numpy as np

from . import engine_hip as E
from .ft_triangulate import _device
from .rpc_model import rpc_to_table

MAX_N = 11  # csrc/satba_fundamental.h, FND_MAX_N: n^3 matches stay in LDS


def _f3x3(f5):
    F = np.zeros((3, 3))
    F[0, 2], F[1, 2], F[2, 0], F[2, 1], F[2, 2] = f5
    return F


def _fundamental(tables, pairs, roi, n, device, want_matches):
    """satba_rpc_fundamental with the flags taken: F5 (P, 5), sv (P, 4), degenerate (P,) bool, matches (P, n^3, 4) or None, kernel_ms"""
    lib = E.load_library()
    tables = np.ascontiguousarray(tables, dtype=np.float64).reshape(-1, 90)
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    roi = np.ascontiguousarray(roi, dtype=np.float64).reshape(-1, 4)
    if roi.shape[0] != pairs.shape[0]:
        raise ValueError("one region of interest per pair")
    if n != int(n):
        raise ValueError("n must be a whole number, got {!r}".format(n))
    P, n = pairs.shape[0], int(n)
    F5, sv, deg = np.zeros((P, 5)), np.zeros((P, 4)), np.zeros(P, dtype=np.uint8)
    m = np.zeros((P, max(n, 0) ** 3, 4)) if want_matches else None
    E._check(lib, lib.satba_rpc_fundamental(tables.shape[0], E._ptr(tables), P, E._ptr(pairs, E._ip), E._ptr(roi), n, E._ptr(F5), E._ptr(sv),
                                            E._ptr(m) if want_matches else None, deg.ctypes.data_as(ct.POINTER(ct.c_uint8)), _device(device)))
    return F5, sv, deg.astype(bool), m, float(lib.satba_rpc_fundamental_kernel_ms())


def matches_from_rpc(rpc1, rpc2, x, y, w, h, n, device=None):
    """
    ref:bundle_adjust/s2p/rpc_utils.py:226-246 on the device: an n x n x n mesh over the region (x, y, w, h) of the first image and
    the altitude range alt_offset -+ alt_scale of rpc1 is localised through rpc1 and projected through both RPCs.  Returns the
    (n^3, 4) array of matches x1, y1, x2, y2 (x1, y1 is the re-projection through rpc1, as in the reference).  2 <= n <= 11.
    """
    tables = np.stack([np.asarray(rpc_to_table(r), dtype=np.float64) for r in (rpc1, rpc2)])
    return _fundamental(tables, [(0, 1)], [(x, y, w, h)], n, device, True)[3][0]


def affine_fundamental_matrix(matches):
    """
    ref:bundle_adjust/s2p/estimation.py:114-154, plain numpy on the host for callers that bring their own matches (N, 4) = x1, y1,
    x2, y2: the Gold Standard algorithm (Hartley & Zisserman, algorithm 14.1) by SVD, as the reference runs it.  The sign of the
    matrix is LAPACK's, that is arbitrary.
    """
    matches = np.asarray(matches, dtype=np.float64)
    if matches.ndim != 2 or matches.shape[1] != 4:
        raise ValueError("matches must be (N, 4) = x1, y1, x2, y2, got shape {}".format(matches.shape))
    X = matches[:, [2, 3, 0, 1]]
    XX = np.sum(X, axis=0) / len(X)
    N = np.linalg.svd(X - XX)[2][-1, :]
    return _f3x3(list(N) + [-np.dot(N, XX)])


def fundamental_matrices(pairs, rpcs, offsets, n=5, device=None, return_info=False):
    """
    One affine fundamental matrix per pair (i, j) of `pairs`, all in one device call: affine_fundamental_matrix(matches_from_rpc(
    rpcs[i], rpcs[j], 0, 0, offsets[i]["width"], offsets[i]["height"], n)), what ft_pipeline.init_F_pair_to_match and
    run_feature_matching compute (ref:bundle_adjust/feature_tracks/ft_pipeline.py:139-152).  The region is the crop's size at the
    origin: the reference evaluates the RPC at these coordinates as they are, without the crop's col0 / row0, and so does this.
    Returns the list of 3 x 3 matrices that match_stereo_pairs(..., F=...) takes; their sign follows the module's rule.
    A pair without a unique matrix (an image with itself, two identical RPCs) raises numpy.linalg.LinAlgError naming it; with
    return_info nothing is raised, the pair's matrix is NaN and the result is (matrices, info): sv (P, 4) singular values of the
    centred matches in descending order, degenerate (P,) bool, kernel_ms.
    """
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(offsets) != len(rpcs):
        raise ValueError("{} offsets for {} RPCs".format(len(offsets), len(rpcs)))
    if pairs.size and (pairs.min() < 0 or pairs.max() >= len(rpcs)):
        raise ValueError("a pair names an image outside 0..{}".format(len(rpcs) - 1))
    tables = np.stack([np.asarray(rpc_to_table(r), dtype=np.float64) for r in rpcs]) if len(rpcs) else np.zeros((0, 90))
    roi = np.array([[0.0, 0.0, offsets[i]["width"], offsets[i]["height"]] for i in pairs[:, 0]], dtype=np.float64).reshape(-1, 4)
    F5, sv, deg, _, ms = _fundamental(tables, pairs, roi, n, device, False)
    if deg.any() and not return_info:
        p = int(np.flatnonzero(deg)[0])
        raise np.linalg.LinAlgError("Singular matrix: pair {} (images {}, {}) has no unique affine fundamental matrix".format(p, pairs[p, 0], pairs[p, 1]))
    Fs = [_f3x3(f) for f in F5]
    return (Fs, {"sv": sv, "degenerate": deg, "kernel_ms": ms}) if return_info else Fs

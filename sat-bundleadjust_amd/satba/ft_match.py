"""
Pairwise matching of SIFT keypoints on the device (the names of ref:bundle_adjust/feature_tracks/ft_match.py; DESIGN.md "Pairwise
matching").

`match_stereo_pairs` returns the reference's M x 4 array (kp_i, kp_j, im_i, im_j), the input of `ft_utils`.  Per pair: the box of the
footprints' intersection, the device match of the keypoints inside it (csrc/satba_match.h behind `satba_match_pairs`: the rule of
ref:3rdparty/sift/simd/sift4ctypes.cpp:125-195, bit for bit on integer descriptors), the reference's renaming of matched keypoints,
and its UTM consistency filter.  All pairs go to the device in one call; there is no CPU fallback: without libsatba_hip.so or
without a GPU the calls raise.

The geographic side runs on the device too.  `keypoints_to_utm_coords_batch` gives the UTM coordinates of the
keypoints of all images in one call (satba_keypoints_utm: RPC localisation, then the Krueger series of csrc/satba_utm_geom.h).
`utm_filter` is the UTM consistency filter of all pairs in one call (satba_utm_filter), index-exact against
`filter_matches_inconsistent_utm_coords`; `match_stereo_pairs` renames all matches in one vectorised step and hands the geometric
mask to that call.  The single-image `keypoints_to_utm_coords` and the per-pair `filter_matches_inconsistent_utm_coords` are kept
as the host restatements.

The fundamental matrices of "epipolar_based" matching come from `fundamental_matrices` (satba/rpc_utils.py, re-exported here): one
matrix per pair from the two RPCs, all pairs in one device call.

Renaming.  ref:ft_s2p.s2p_match_SIFT maps a match back to indices by its coordinates (`list.index`), so a keypoint is named by the
first keypoint with the same (col, row) -- SIFT emits one keypoint per orientation at a location.  `canonical=True` (the default)
reproduces that with one index map per image (keypoints that share a location share their UTM coordinates, so they are inside a
box together); `canonical=False` returns the matched rows themselves.

Geometric filter.  ref:bundle_adjust/s2p/sift.py:181-184 and ref:feature_tracks/ft_opencv.py:188-216 filter every pair's matches by a
fundamental-matrix RANSAC (`ransac.find_fundamental_matrix` / `cv2.findFundamentalMat`) that is random and in neither tree.
`geometric_filter="ransac"` runs the deterministic rule of include/satba.h (satba_ransac_fundamental: counter-based samples,
seven-point models, the reference's error, most inliers wins; csrc/satba_ransac.h) on the device, all pairs of a call
in one device call, with max_err = FT_ransac (0.3), 1000 trials and `ransac_seed`.  A callable (pix_i, pix_j, matches_ij) ->
boolean mask is taken as before; None (the default) filters nothing.  `ransac_fundamental`, `geometric_filtering` and
`inliers_mask_from_fundamental_matrix` are the pieces on their own, the last two under the reference's names.

"local_window" (ref:ft_match.py:151-160, 396-463) is the matcher for pairs without a usable fundamental matrix: a keypoint is
compared only with the keypoints of the other image within FT_local_radius metres (30; the reference hard-codes it) on the ground,
under the absolute threshold FT_abs_thr (250), with no relative test.  `match_pairs_window` is the device call (satba_match_window:
the rule of include/satba.h, csrc/satba_window.h, DESIGN.md 4q -- the reference's C routine is in neither tree);
`locally_match_SIFT_utm_coords` is the one-pair function under the reference's name.

Not reproduced: the pairwise .npy cache files are not read or written, and of the reference's matching methods "flann" and
"lightglue" (foreign libraries) are not matched here.
"""
import ctypes as ct

import numpy as np

from . import engine_hip as E
from . import geo_utils
from .ba_outliers import get_elbow_value
from .ft_triangulate import _device
from .rpc_model import rpc_to_table
from .rpc_utils import affine_fundamental_matrix, fundamental_matrices, matches_from_rpc  # noqa: F401  (the pairs' matrices: the step in front)

_lp = ct.POINTER(ct.c_int64)
_fp = ct.POINTER(ct.c_float)
_bp = ct.POINTER(ct.c_uint8)
EPIPOLAR_THR = 20.0  # ref:ft_s2p.py:145
METHODS = ("epipolar_based", "bruteforce", "local_window")


# ----------------------------------------------------------------------------- convex polygons (in place of shapely)

def _ring(poly):
    """(n, 2) vertices of a footprint / geojson polygon / ring, the closing vertex dropped, counter-clockwise."""
    if isinstance(poly, dict):
        poly = poly["geojson"] if "geojson" in poly else poly
        poly = poly["coordinates"][0]
    elif hasattr(poly, "exterior"):
        poly = np.asarray(poly.exterior.coords)
    r = np.asarray(poly, dtype=np.float64).reshape(-1, 2)
    if len(r) > 1 and np.array_equal(r[0], r[-1]):
        r = r[:-1]
    return r[::-1] if _signed_area(r) < 0 else r


def _signed_area(r):
    if len(r) < 3:
        return 0.0
    x, y = r[:, 0], r[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


def polygon_area(poly):
    return abs(_signed_area(_ring(poly)))


def clip_convex(subject, clip):
    """Sutherland-Hodgman: the part of the convex polygon `subject` inside the convex polygon `clip`, (n, 2), n = 0 when disjoint."""
    out, c = [tuple(p) for p in _ring(subject)], _ring(clip)
    for k in range(len(c)):
        a, b = c[k], c[(k + 1) % len(c)]
        inp, out = out, []
        if not inp:
            break

        def side(p):
            return (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])

        for m in range(len(inp)):
            p, q = inp[m], inp[(m + 1) % len(inp)]
            sp, sq = side(p), side(q)
            if sp >= 0:
                out.append(p)
            if (sp > 0 and sq < 0) or (sp < 0 and sq > 0):
                t = sp / (sp - sq)
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return np.asarray(out, dtype=np.float64).reshape(-1, 2)


def footprint_intersection(poly_i, poly_j):
    """(area, box) of the intersection of two convex polygons; box = (min_east, max_east, min_north, max_north), None when the
    polygons share no area (disjoint, or touching along an edge or at a vertex)."""
    r = clip_convex(poly_i, poly_j)
    area = abs(_signed_area(r))
    if not area > 0.0:
        return 0.0, None
    return area, (r[:, 0].min(), r[:, 0].max(), r[:, 1].min(), r[:, 1].max())


def compute_pairs_to_match(init_pairs, footprints, optical_centers, min_overlap=0.1, min_baseline=1 / 4, orbit_alt=500000, verbose=True):
    """ref:ft_match.py:17-73: pairs whose footprints overlap by more than min_overlap of the first, and of those the pairs with a
    baseline above min_baseline * orbit_alt; pairs of a camera whose every pair has a short baseline are kept for triangulation."""

    def set_pair(i, j):
        return (min(i, j), max(i, j))

    pairs_to_match, pairs_to_triangulate = [], []
    for (i, j) in init_pairs:
        i, j = int(i), int(j)
        area, _ = footprint_intersection(footprints[i], footprints[j])
        if area / polygon_area(footprints[i]) > min_overlap:
            pairs_to_match.append(set_pair(i, j))
            baseline = np.linalg.norm(np.asarray(optical_centers[i]) - np.asarray(optical_centers[j]))
            if baseline / orbit_alt > min_baseline:
                pairs_to_triangulate.append(set_pair(i, j))
    in_match = set(int(c) for p in pairs_to_match for c in p)
    in_tri = set(int(c) for p in pairs_to_triangulate for c in p)
    cams_bad_baseline = list(in_match - in_tri)
    pairs_to_triangulate.extend([(i, j) for (i, j) in pairs_to_match if i in cams_bad_baseline or j in cams_bad_baseline])
    if verbose:
        print("     {} / {} pairs suitable to match".format(len(pairs_to_match), len(init_pairs)))
        print("     {} / {} pairs suitable to triangulate".format(len(pairs_to_triangulate), len(init_pairs)))
        if cams_bad_baseline:
            print("     WARNING: Found {} cameras with insufficient baseline w.r.t. all neighbor cameras".format(len(cams_bad_baseline)))
            print("              Concerned cameras are: {}".format(cams_bad_baseline))
    return pairs_to_match, pairs_to_triangulate


# ----------------------------------------------------------------------------- host pieces of the reference

def get_pt_indices_inside_utm_bbx(easts, norths, min_east, max_east, min_north, max_north):
    """ref:ft_match.py:76-90 (what the device's select kernel computes per pair and side)."""
    east_ok = (easts > min_east) & (easts < max_east)
    north_ok = (norths > min_north) & (norths < max_north)
    return np.where(east_ok & north_ok)[0]


def filter_matches_inconsistent_utm_coords(matches_ij, utm_i, utm_j):
    """ref:ft_match.py:220-247."""
    all_utm_distances = np.linalg.norm(utm_i[matches_ij[:, 0]] - utm_j[matches_ij[:, 1]], axis=1)
    utm_thr, success = get_elbow_value(all_utm_distances, max_outliers_percent=20, verbose=False)
    utm_thr = utm_thr + 5 if success else np.max(all_utm_distances)
    return matches_ij[all_utm_distances <= utm_thr]


def keypoints_to_utm_coords(im_features, im_rpc, im_offset, alt, zone=None):
    """ref:ft_match.py:190-217 with the localisation on the device; `zone` lets the images of a scene share one UTM zone (the
    reference takes the zone of each image's first keypoint).  The NaN padding of im_features is kept."""
    im_features = np.asarray(im_features)
    n_kp = int(np.sum(~np.isnan(im_features[:, 0])))
    utm_coords = np.full((im_features.shape[0], 2), np.nan)
    if n_kp:
        cols = im_features[:n_kp, 0].astype(np.float64) + im_offset["col0"]
        rows = im_features[:n_kp, 1].astype(np.float64) + im_offset["row0"]
        lon, lat = im_rpc.localization(cols, rows, np.full(n_kp, float(alt)))
        east, north = geo_utils.utm_from_lonlat(lon, lat, zone=zone)
        utm_coords[:n_kp, 0], utm_coords[:n_kp, 1] = east, north
    utm_coords[n_kp:] = im_features[n_kp:, :2]
    return utm_coords


def rectifying_similarities(F):
    """(s1, s2), float32[3] each: the similarities (a, b, q) that rectify the two images of an affine fundamental matrix F
    (Hartley & Zisserman p. 345), computed in double and rounded once, as ref:3rdparty/sift/simd/linalg.c:108-138 does."""
    c, d, a, b, e = _f5(F)
    r, s = np.sqrt(a * a + b * b), np.sqrt(c * c + d * d)
    z, t = np.sqrt(r / s), 0.5 * e / np.sqrt(r * s)
    zz = 1 / z
    return (np.array([z * b / r, z * a / r, t], dtype=np.float32), np.array([zz * -d / s, zz * -c / s, -t], dtype=np.float32))


def _f5(F):
    F = np.asarray(F, dtype=np.float64)
    if F.shape == (5,):
        return [np.float64(v) for v in F]
    if F.shape != (3, 3):
        raise ValueError("F must be a 3 x 3 fundamental matrix, got shape {}".format(F.shape))
    return [F[0, 2], F[1, 2], F[2, 0], F[2, 1], F[2, 2]]


def canonical_index_map(features):
    """index of the first keypoint with the same (col, row), per keypoint (what `list.index` finds in ref:ft_s2p.py:166-168)"""
    xy = np.ascontiguousarray(np.asarray(features)[:, :2], dtype=np.float32) + np.float32(0.0)  # -0.0 == 0.0
    key = xy.view(np.uint32).astype(np.uint64)
    key = (key[:, 0] << np.uint64(32)) | key[:, 1]
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    return first[inv.reshape(-1)]


# ----------------------------------------------------------------------------- the device match

def _load(a, dtype, cols):
    if isinstance(a, (str, bytes)) or hasattr(a, "__fspath__"):
        a = np.load(a, mmap_mode="r")
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.ndim != 2 or a.shape[1] != cols:
        raise ValueError("expected an array of shape (n, {}), got {}".format(cols, a.shape))
    return a


def _match_inputs(pairs, features, utm_coords, boxes):
    """the arguments that satba_match_pairs and satba_match_window share, checked and laid out for the call (the arrays are returned
    so that they outlive it)"""
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
    n_pairs, n_cam = pairs.shape[0], len(features)
    if len(utm_coords) != n_cam:
        raise ValueError("features and utm_coords must list the same images")
    if n_pairs and (pairs.min() < 0 or pairs.max() >= n_cam):
        raise ValueError("a pair names an image outside 0..{}".format(n_cam - 1))
    boxes = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64).reshape(-1, 4))
    if boxes.shape[0] != n_pairs:
        raise ValueError("one box per pair")
    used = set(int(c) for c in pairs.reshape(-1))
    feats = [_load(features[c], np.float32, 132) if c in used else None for c in range(n_cam)]
    utms = [_load(utm_coords[c], np.float64, 2) if c in used else None for c in range(n_cam)]
    n_kp = np.zeros(n_cam, dtype=np.int64)
    for c in used:
        if feats[c].shape[0] != utms[c].shape[0]:
            raise ValueError("image {}: {} keypoints but {} utm rows".format(c, feats[c].shape[0], utms[c].shape[0]))
        n_kp[c] = feats[c].shape[0]
    fptr = (ct.c_void_p * n_cam)(*[a.ctypes.data if a is not None else None for a in feats])
    uptr = (ct.c_void_p * n_cam)(*[a.ctypes.data if a is not None else None for a in utms])
    p32 = np.ascontiguousarray(pairs, dtype=np.int32)
    return n_cam, n_kp, fptr, uptr, n_pairs, p32, boxes, (feats, utms)


def _fetch_matches(lib, handle, n, n_pairs):
    try:
        pair_ofs = np.zeros(n_pairs + 1, dtype=np.int64)
        kp_i, kp_j = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        E._check(lib, lib.satba_matches_fetch(handle, pair_ofs.ctypes.data_as(_lp), E._ptr(kp_i, E._ip), E._ptr(kp_j, E._ip)))
    finally:
        lib.satba_matches_destroy(handle)
    return pair_ofs, kp_i, kp_j


def _match_info(counts, ms):
    return {"n_selected": int(counts[1]), "n_empty_pairs": int(counts[2]), "path": ("int8", "float32")[int(counts[3])], "kernel_ms": ms.value}


def match_pairs(pairs, features, utm_coords, boxes, F=None, thr=0.6, epi_thr=EPIPOLAR_THR, relative=True, device=None, return_info=False):
    """
    satba_match_pairs (include/satba.h): all pairs in one call.  pairs (n, 2) image indices; features / utm_coords: per image an
    (n_kp, 132) / (n_kp, 2) array or .npy path (images no pair names are not loaded); boxes (n, 4) = min_east, max_east, min_north,
    max_north; F: None (no gate) or per pair a 3 x 3 matrix (or its five coefficients).  Returns pair_ofs (n + 1), kp_i, kp_j: the
    matches of pair p are rows pair_ofs[p] : pair_ofs[p + 1], kp_i ascending.  With return_info also a dict: n_selected,
    n_empty_pairs, path ("int8" | "float32"), kernel_ms.
    """
    n_cam, n_kp, fptr, uptr, n_pairs, p32, boxes, _keep = _match_inputs(pairs, features, utm_coords, boxes)
    F5 = None
    if F is not None:
        if len(F) != n_pairs:
            raise ValueError("one fundamental matrix per pair")
        F5 = np.ascontiguousarray(np.array([_f5(f) for f in F], dtype=np.float64).reshape(-1, 5))
    lib = E.load_library()
    handle, ms = ct.c_void_p(None), ct.c_float(0.0)
    counts = np.zeros(4, dtype=np.int64)
    E._check(lib, lib.satba_match_pairs(n_cam, n_kp.ctypes.data_as(_lp), fptr, uptr, n_pairs, E._ptr(p32, E._ip), E._ptr(boxes),
                                        E._ptr(F5) if F5 is not None else None, float(thr), float(epi_thr), 1 if relative else 0, ct.byref(handle),
                                        counts.ctypes.data_as(_lp), _device(device), ct.byref(ms)))
    pair_ofs, kp_i, kp_j = _fetch_matches(lib, handle, int(counts[0]), n_pairs)
    if return_info:
        return pair_ofs, kp_i, kp_j, _match_info(counts, ms)
    return pair_ofs, kp_i, kp_j


def match_pairs_window(pairs, features, utm_coords, boxes, radius=30.0, thr=250.0, device=None, return_info=False):
    """
    satba_match_window (include/satba.h): the windowed match of all pairs in one call.  Arguments and results as `match_pairs`;
    radius: the window's half-width on the ground in metres, a scalar or (rx, ry), +inf allowed; thr: the absolute threshold on the
    descriptor distance.  A keypoint of the first image is compared with the keypoints of the second inside the pair's box whose
    easting differs by less than rx and whose northing by less than ry; the nearest matches when its distance is below thr ** 2.
    The info dict additionally holds n_candidates, the (i, j) that passed the window test summed over all pairs.
    """
    r = np.asarray(radius, dtype=np.float64).reshape(-1)
    if r.size not in (1, 2):
        raise ValueError("radius must be a scalar or (rx, ry), got {!r}".format(radius))
    rx, ry = float(r[0]), float(r[-1])
    n_cam, n_kp, fptr, uptr, n_pairs, p32, boxes, _keep = _match_inputs(pairs, features, utm_coords, boxes)
    lib = E.load_library()
    if not hasattr(lib, "satba_match_window"):
        raise OSError("libsatba_hip.so has no satba_match_window: rebuild it (make -C sat-bundleadjust_amd/csrc)")
    handle, ms = ct.c_void_p(None), ct.c_float(0.0)
    counts = np.zeros(5, dtype=np.int64)
    E._check(lib, lib.satba_match_window(n_cam, n_kp.ctypes.data_as(_lp), fptr, uptr, n_pairs, E._ptr(p32, E._ip), E._ptr(boxes), rx, ry, float(thr),
                                         ct.byref(handle), counts.ctypes.data_as(_lp), _device(device), ct.byref(ms)))
    pair_ofs, kp_i, kp_j = _fetch_matches(lib, handle, int(counts[0]), n_pairs)
    if return_info:
        return pair_ofs, kp_i, kp_j, dict(_match_info(counts, ms), n_candidates=int(counts[4]))
    return pair_ofs, kp_i, kp_j


def _match_by_method(method, pairs, feats, utms, boxes, Fs, tracks_config, device):
    """the device match of `pairs` by the configured method: (pair_ofs, kp_i, kp_j, info)"""
    if method == "local_window":
        return match_pairs_window(pairs, feats, utms, boxes, radius=tracks_config.get("FT_local_radius", 30.0), thr=tracks_config.get("FT_abs_thr", 250),
                                  device=device, return_info=True)
    return match_pairs(pairs, feats, utms, boxes, F=Fs, thr=tracks_config.get("FT_rel_thr", 0.6), device=device, return_info=True)


def _method(tracks_config):
    method = tracks_config.get("FT_sift_matching", "epipolar_based")
    if method not in METHODS:
        raise ValueError("FT_sift_matching must be one of {}, got {!r}".format(METHODS, method))
    return method


def ransac_fundamental(pair_ofs, xy, max_err=0.3, n_trials=1000, seed=0, device=None, return_info=False):
    """
    satba_ransac_fundamental (include/satba.h): the matches of all pairs, rows (x1, y1, x2, y2) in float64, pair p being rows
    pair_ofs[p] : pair_ofs[p + 1].  Returns the boolean mask of the matches kept; with return_info also a dict: F (n_pairs, 3, 3;
    zeros where a pair has no model), best (n_pairs, 3) = winning trial (-1: none), matches kept, models tried, and kernel_ms.
    """
    pair_ofs = np.ascontiguousarray(np.asarray(pair_ofs, dtype=np.int64).reshape(-1))
    xy = np.ascontiguousarray(np.asarray(xy, dtype=np.float64).reshape(-1, 4))
    if pair_ofs.size < 1 or pair_ofs[-1] != xy.shape[0]:
        raise ValueError("pair_ofs must hold n_pairs + 1 offsets that end at the number of matches ({}), got {}".format(xy.shape[0], pair_ofs[-1:]))
    n_pairs = pair_ofs.size - 1
    inlier = np.zeros(xy.shape[0], dtype=np.uint8)
    F, best = np.zeros((n_pairs, 9), dtype=np.float64), np.zeros((n_pairs, 3), dtype=np.int32)
    lib = E.load_library()
    ms = ct.c_float(0.0)
    E._check(lib, lib.satba_ransac_fundamental(n_pairs, pair_ofs.ctypes.data_as(_lp), E._ptr(xy), float(max_err), int(n_trials), int(seed) & (2 ** 64 - 1),
                                               inlier.ctypes.data_as(ct.POINTER(ct.c_uint8)), E._ptr(F), E._ptr(best, E._ip), _device(device), ct.byref(ms)))
    mask = inlier.astype(bool)
    if return_info:
        return mask, {"F": F.reshape(n_pairs, 3, 3), "best": best, "kernel_ms": ms.value}
    return mask


def inliers_mask_from_fundamental_matrix(F, m1, m2, ransac_thr):
    """ref:feature_tracks/ft_opencv.py:143-185: the matches (m1, m2: N x 2) whose larger squared distance to the epipolar lines of F
    is below ransac_thr ** 2 (None: 3.0, cv2's default); None when no match is."""
    F_ = np.asarray(F, dtype=np.float64).reshape(-1)
    m1, m2 = np.asarray(m1, dtype=np.float64), np.asarray(m2, dtype=np.float64)
    assert m1.shape[1] == 2 and m2.shape[1] == 2 and m1.shape == m2.shape
    ransac_thr = 3.0 if ransac_thr is None else ransac_thr
    with np.errstate(all="ignore"):
        a = F_[0] * m1[:, 0] + F_[1] * m1[:, 1] + F_[2]
        b = F_[3] * m1[:, 0] + F_[4] * m1[:, 1] + F_[5]
        c = F_[6] * m1[:, 0] + F_[7] * m1[:, 1] + F_[8]
        s2 = 1.0 / (a * a + b * b)
        d2 = m2[:, 0] * a + m2[:, 1] * b + c
        a = F_[0] * m2[:, 0] + F_[3] * m2[:, 1] + F_[6]
        b = F_[1] * m2[:, 0] + F_[4] * m2[:, 1] + F_[7]
        c = F_[2] * m2[:, 0] + F_[5] * m2[:, 1] + F_[8]
        s1 = 1.0 / (a * a + b * b)
        d1 = m1[:, 0] * a + m1[:, 1] * b + c
        inliers_mask = np.maximum(d1 * d1 * s1, d2 * d2 * s2) < ransac_thr ** 2
    return inliers_mask if inliers_mask.any() else None


def _match_coords(features_i, features_j, matches_ij):
    return np.concatenate([np.asarray(features_i)[matches_ij[:, 0], :2], np.asarray(features_j)[matches_ij[:, 1], :2]], axis=1).astype(np.float64)


def geometric_filtering(features_i, features_j, matches_ij, ransac_thr=0.3, return_mask=False, seed=0, device=None):
    """ref:feature_tracks/ft_opencv.py:188-216 with the device RANSAC in place of cv2's: the rows of matches_ij (M x 2) that the
    winning model keeps, None when there is none; ransac_thr=None means 3.0, cv2's default.  With return_mask also the M x 1 uint8
    mask (None with no match)."""
    matches_ij = np.asarray(matches_ij).reshape(-1, 2)
    mask = None
    if matches_ij.shape[0]:
        mask = ransac_fundamental([0, matches_ij.shape[0]], _match_coords(features_i, features_j, matches_ij),
                                  max_err=3.0 if ransac_thr is None else ransac_thr, seed=seed, device=device)
    matches_ij = matches_ij[mask] if mask is not None and mask.any() else None
    if return_mask:
        return matches_ij, (mask.astype(np.uint8).reshape(-1, 1) if mask is not None else None)
    return matches_ij


def _check_filter(geometric_filter):
    if not (geometric_filter is None or geometric_filter == "ransac" or callable(geometric_filter)):
        raise ValueError('geometric_filter must be None, "ransac" or a callable, got {!r}'.format(geometric_filter))


def utm_filter(pair_ofs, utm4, alive=None, margin=5.0, device=None, return_info=False):
    """
    satba_utm_filter (include/satba.h): `filter_matches_inconsistent_utm_coords` for the matches of all pairs in one device call.
    utm4: rows (east_i, north_i, east_j, north_j) of the matches' two keypoints, pair p being rows pair_ofs[p] : pair_ofs[p + 1];
    alive: None or a mask of the matches that take part (a geometric filter's), the others are dropped.  Returns the boolean mask of
    the matches kept; with return_info also a dict: thr (n_pairs; NaN where no match is alive), n_kept (n_pairs), kernel_ms.
    """
    pair_ofs = np.ascontiguousarray(np.asarray(pair_ofs, dtype=np.int64).reshape(-1))
    utm4 = np.ascontiguousarray(np.asarray(utm4, dtype=np.float64).reshape(-1, 4))
    n = utm4.shape[0]
    if pair_ofs.size < 1 or pair_ofs[-1] != n:
        raise ValueError("pair_ofs must hold n_pairs + 1 offsets that end at the number of matches ({}), got {}".format(n, pair_ofs[-1:]))
    if alive is not None:
        alive = np.ascontiguousarray(np.asarray(alive).reshape(-1) != 0, dtype=np.uint8)
        if alive.size != n:
            raise ValueError("alive must hold one entry per match ({}), got {}".format(n, alive.size))
    n_pairs = pair_ofs.size - 1
    keep = np.zeros(n, dtype=np.uint8)
    thr, n_kept = np.full(n_pairs, np.nan), np.zeros(n_pairs, dtype=np.int64)
    lib = E.load_library()
    ms = ct.c_float(0.0)
    E._check(lib, lib.satba_utm_filter(n_pairs, pair_ofs.ctypes.data_as(_lp), E._ptr(utm4), alive.ctypes.data_as(_bp) if alive is not None else None,
                                       float(margin), keep.ctypes.data_as(_bp), E._ptr(thr), n_kept.ctypes.data_as(_lp), _device(device), ct.byref(ms)))
    keep = keep.astype(bool)
    if return_info:
        return keep, {"thr": thr, "n_kept": n_kept, "kernel_ms": ms.value}
    return keep


def keypoints_to_utm_coords_batch(features, rpcs, offsets, alts, zone=None, device=None, return_lonlat=False, return_info=False):
    """
    satba_keypoints_utm (include/satba.h): `keypoints_to_utm_coords` for all images in one device call.  features: per image an
    (n, 132) array or .npy path; rpcs: per image an RPC model; offsets: per image a dict with "col0" and "row0"; alts: one altitude
    for all images or one per image.  zone=None takes, per image, the zone of its first keypoint, as the reference does; an integer
    1..60 makes all images share that zone (a sequence gives one per image).  Returns the list of (n, 2) arrays (easting, northing),
    the NaN padding of the features kept; with return_lonlat also the list of (n, 2) arrays (lon, lat) the localisation gave; with
    return_info also a dict: kernel_ms.
    """
    feats = [_load(f, np.float32, 132) for f in features]
    n_cam = len(feats)
    if len(rpcs) != n_cam or len(offsets) != n_cam:
        raise ValueError("features, rpcs and offsets must list the same images")
    tables = np.ascontiguousarray(np.array([rpc_to_table(r) for r in rpcs], dtype=np.float64).reshape(n_cam, 90))
    off = np.ascontiguousarray(np.array([[o["col0"], o["row0"]] for o in offsets], dtype=np.float64).reshape(n_cam, 2))
    alts = np.ascontiguousarray(np.broadcast_to(np.asarray(alts, dtype=np.float64), (n_cam,)))
    if zone is None:
        zones = np.zeros(n_cam, dtype=np.int32)
    else:
        zones = np.ascontiguousarray(np.broadcast_to(np.asarray(zone, dtype=np.int32), (n_cam,)))
        if n_cam and (zones.min() < 1 or zones.max() > 60):
            raise ValueError("a UTM zone lies in 1..60, got {!r}".format(zone))
    n_rows = np.array([f.shape[0] for f in feats], dtype=np.int64)
    utm = [np.zeros((f.shape[0], 2), dtype=np.float64) for f in feats]
    lonlat = [np.zeros((f.shape[0], 2), dtype=np.float64) for f in feats] if return_lonlat else None
    fptr = (ct.c_void_p * n_cam)(*[a.ctypes.data for a in feats])
    uptr = (ct.c_void_p * n_cam)(*[a.ctypes.data for a in utm])
    lptr = (ct.c_void_p * n_cam)(*[a.ctypes.data for a in lonlat]) if return_lonlat else None
    lib = E.load_library()
    ms = ct.c_float(0.0)
    E._check(lib, lib.satba_keypoints_utm(n_cam, E._ptr(tables), n_rows.ctypes.data_as(_lp), fptr, E._ptr(off), E._ptr(alts), E._ptr(zones, E._ip), uptr,
                                          lptr, _device(device), ct.byref(ms)))
    out = (utm,) + ((lonlat,) if return_lonlat else ()) + (({"kernel_ms": ms.value},) if return_info else ())
    return out if len(out) > 1 else utm


def _rename_all(ofs, kp_i, kp_j, sides, feats, canonical):
    """
    The renaming of the matches of all pairs in one vectorised step (sides: the two images of every pair; the matches of pair p are
    rows ofs[p] : ofs[p + 1]; host only).  Returns m_ij (n, 2) renamed through the images' index maps, im (n, 2) the images of every
    match, `used` the images in use, ascending, and `rows` (n, 2): where the two keypoints of a match stand when the arrays of the
    images in use are put behind one another.
    """
    sides = np.asarray(sides, dtype=np.int64).reshape(-1, 2)
    im = sides[np.repeat(np.arange(len(sides)), np.diff(ofs))]
    m_ij = np.stack([kp_i, kp_j], axis=1).astype(np.int64)
    used = np.unique(sides)
    base = np.zeros(len(feats) + 1, dtype=np.int64)
    base[used + 1] = [feats[c].shape[0] for c in used]
    base = np.cumsum(base)[:-1]
    rows = m_ij + base[im]
    if canonical and m_ij.shape[0]:
        rows = np.concatenate([canonical_index_map(feats[c]) + base[c] for c in used])[rows]
        m_ij = rows - base[im]
    return m_ij, im, used, rows


def _both_sides(arrays, used, rows):
    """(n, 2 k): the rows of the two keypoints of every match out of per-image (n_kp, k) arrays"""
    a = np.concatenate([np.asarray(arrays[c]) for c in used], axis=0)
    return np.concatenate([a[rows[:, 0]], a[rows[:, 1]]], axis=1)


def _rename_and_filter(ofs, kp_i, kp_j, sides, feats, utms, canonical, geometric_filter, tracks_config, ransac_seed, device):
    """
    What follows the device match, for all pairs at once: the renaming (`_rename_all`), the geometric filter ("ransac": one device
    call; a callable: called once per pair that has matches, in order) and the UTM filter (one device call, the geometric mask as
    its `alive`).  Returns m_ij (n, 2) renamed, im (n, 2), alive (n, bool; None without a geometric filter), keep (n, bool) and the
    kernel times.
    """
    m_ij, im, used, rows = _rename_all(ofs, kp_i, kp_j, sides, feats, canonical)
    n = m_ij.shape[0]
    info = {"utm_kernel_ms": 0.0}
    if geometric_filter == "ransac":
        info["ransac_kernel_ms"] = 0.0
    if n == 0:
        return m_ij, im, (None if geometric_filter is None else np.zeros(0, dtype=bool)), np.zeros(0, dtype=bool), info
    alive = None
    if geometric_filter == "ransac":
        xy = _both_sides([f[:, :2] if f is not None else None for f in feats], used, rows).astype(np.float64)
        alive, rinfo = ransac_fundamental(ofs, xy, max_err=tracks_config.get("FT_ransac", 0.3), seed=ransac_seed, device=device, return_info=True)
        info["ransac_kernel_ms"] = rinfo["kernel_ms"]
    elif geometric_filter is not None:
        alive = np.zeros(n, dtype=bool)
        for p, (i, j) in enumerate(np.asarray(sides, dtype=np.int64).reshape(-1, 2)):
            if ofs[p + 1] > ofs[p]:
                mask = geometric_filter(np.asarray(feats[i][:, :2]), np.asarray(feats[j][:, :2]), m_ij[ofs[p]:ofs[p + 1]])
                alive[ofs[p]:ofs[p + 1]] = np.asarray(mask, dtype=bool).reshape(-1)
    keep, uinfo = utm_filter(ofs, _both_sides(utms, used, rows), alive, device=device, return_info=True)
    info["utm_kernel_ms"] = uinfo["kernel_ms"]
    return m_ij, im, alive, keep, info


def _polygon_box(utm_polygon):
    r = _ring(utm_polygon)
    if len(r) == 0:
        return None
    return (r[:, 0].min(), r[:, 0].max(), r[:, 1].min(), r[:, 1].max())


def match_kp_within_utm_polygon(features_i, features_j, utm_i, utm_j, utm_polygon, tracks_config, F=None, canonical=True, geometric_filter=None,
                                device=None, ransac_seed=0):
    """ref:ft_match.py:93-187 for one pair.  utm_polygon: a ring (n, 2), a geojson polygon, or an object with .exterior.coords.
    Returns (matches_ij (M, 2) or None, n): n = [matched, after the geometric filter when there is one, after the UTM filter], or
    [0, 0, 0] when a side has no keypoint inside."""
    method = _method(tracks_config)
    _check_filter(geometric_filter)
    box = _polygon_box(utm_polygon)
    fi, fj, ui, uj = _load(features_i, np.float32, 132), _load(features_j, np.float32, 132), _load(utm_i, np.float64, 2), _load(utm_j, np.float64, 2)
    if box is None:
        return None, [0, 0, 0]
    Fs = [F] if method == "epipolar_based" else None
    if method == "epipolar_based" and F is None:
        raise ValueError("epipolar_based matching needs the fundamental matrix of the pair")
    ofs, kp_i, kp_j, info = _match_by_method(method, [(0, 1)], [fi, fj], [ui, uj], [box], Fs, tracks_config, device)
    if info["n_empty_pairs"]:
        return None, [0, 0, 0]
    m_ij, _, alive, keep, _ = _rename_and_filter(ofs, kp_i, kp_j, [(0, 1)], [fi, fj], [ui, uj], canonical, geometric_filter, tracks_config, ransac_seed,
                                                 device)
    n = [m_ij.shape[0]]
    if m_ij.shape[0] and alive is not None:
        n.append(int(alive.sum()))
    n.append(int(keep.sum()))
    m_ij = m_ij[keep]
    return (m_ij if m_ij.shape[0] else None), n


def locally_match_SIFT_utm_coords(features_i, features_j, utm_i, utm_j, radius=30, sift_thr=250, ransac_thr=0.3, seed=0, device=None):
    """ref:ft_match.py:396-463: the windowed match over all rows of two images (an infinite box), then `geometric_filtering` (the
    device RANSAC).  Returns (matches_ij (M, 2) or None, n_matches, n_matches_after_geofilt).  The reference adds 10e6 to every
    negative northing; so does this, on copies: the reference writes the shift, and then its registered coordinates, into its
    caller's arrays, which is not reproduced -- no argument is written to."""
    fi, fj = _load(features_i, np.float32, 132), _load(features_j, np.float32, 132)
    ui, uj = np.array(_load(utm_i, np.float64, 2)), np.array(_load(utm_j, np.float64, 2))  # copies
    for u in (ui, uj):
        with np.errstate(invalid="ignore"):
            u[u[:, 1] < 0, 1] += 10e6
    inf = np.inf
    ofs, kp_i, kp_j = match_pairs_window([(0, 1)], [fi, fj], [ui, uj], [(-inf, inf, -inf, inf)], radius=radius, thr=sift_thr, device=device)
    matches_ij = np.stack([kp_i, kp_j], axis=1).astype(np.int64)
    n_matches = matches_ij.shape[0]
    if n_matches == 0:
        return None, 0, 0
    matches_ij = geometric_filtering(fi, fj, matches_ij, ransac_thr, seed=seed, device=device)
    return matches_ij, n_matches, (0 if matches_ij is None else matches_ij.shape[0])


def match_stereo_pairs(pairs_to_match, features, footprints, utm_coords, tracks_config, F=None, canonical=True, geometric_filter=None,
                       device=None, return_info=False, ransac_seed=0):
    """
    ref:ft_match.py:250-339.  features / utm_coords: per image an array or a .npy path; footprints: per image a dict with a
    "geojson" polygon in UTM coordinates (convex).  F: per pair a 3 x 3 fundamental matrix ("epipolar_based"; "bruteforce" and
    "local_window" need none -- the latter reads FT_local_radius and FT_abs_thr).  Returns the M x 4
    int64 array (kp_i, kp_j, im_i, im_j), pairs in the given order; a pair whose footprints share no area gives no rows.
    geometric_filter: None, a callable per pair, or "ransac": the device RANSAC over all pairs in one call (module docstring), whose
    kernel time return_info reports as "ransac_kernel_ms".  The renaming and the UTM filter take all pairs at once; the filter is one
    device call (`utm_filter`), whose kernel time return_info reports as "utm_kernel_ms".
    """
    method = _method(tracks_config)
    _check_filter(geometric_filter)
    pairs = [(int(p[0]), int(p[1])) for p in pairs_to_match]
    if method == "epipolar_based" and (F is None or len(F) != len(pairs)):
        raise ValueError("epipolar_based matching needs one fundamental matrix per pair")
    boxes = [footprint_intersection(footprints[i], footprints[j])[1] for i, j in pairs]
    live = [k for k, b in enumerate(boxes) if b is not None]
    out = np.zeros((0, 4), dtype=np.int64)
    info = {"n_selected": 0, "n_empty_pairs": 0, "path": "int8", "kernel_ms": 0.0}
    times = {"utm_kernel_ms": 0.0}
    if live:
        Fs = [F[k] for k in live] if method == "epipolar_based" else None
        used = set(c for k in live for c in pairs[k])
        if used and not (0 <= min(used) and max(used) < min(len(features), len(utm_coords))):
            raise ValueError("a pair names an image outside 0..{}".format(len(features) - 1))
        feats = [_load(features[c], np.float32, 132) if c in used else None for c in range(len(features))]  # loaded once
        utms = [_load(utm_coords[c], np.float64, 2) if c in used else None for c in range(len(utm_coords))]
        ofs, kp_i, kp_j, info = _match_by_method(method, [pairs[k] for k in live], feats, utms, [boxes[k] for k in live], Fs, tracks_config, device)
        m_ij, im, _, keep, times = _rename_and_filter(ofs, kp_i, kp_j, [pairs[k] for k in live], feats, utms, canonical, geometric_filter, tracks_config,
                                                      ransac_seed, device)
        out = np.concatenate([m_ij, im], axis=1)[keep]
    info.update(times)
    return (out, info) if return_info else out

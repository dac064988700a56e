"""
Detection and description of SIFT keypoints on the device (the names of ref:bundle_adjust/feature_tracks/ft_s2p.py and
ref:bundle_adjust/s2p/sift.py; DESIGN.md "SIFT detection").

`keypoints_from_nparray` returns the (n, 132) rows (col, row, scale, orientation, 128 descriptor integers) that `ft_match`
consumes, as float32 (the reference returns the same values as float64): csrc/satba_sift.h behind `satba_sift_detect`, "Anatomy of
the SIFT method" as ref:3rdparty/sift/simd runs it.  `detect_features_image_sequence` adds the reference's mask, its stable sort
by scale and its truncation / NaN padding to FT_kp_max.  There is no CPU fallback: without libsatba_hip.so or without a GPU the
calls raise.

Not reproduced: the features/*.npy cache files are not read or written, and images too large for one device are not tiled.
"""
import ctypes as ct

import numpy as np

from . import engine_hip as E
from .ft_triangulate import _device

_lp = ct.POINTER(ct.c_int64)
_fp = ct.POINTER(ct.c_float)
THRESH_DOG, NB_OCTAVES, NB_SCALES = 0.0133, 8, 3  # ref:ft_s2p.py:42-44
FT_KP_MAX = 60000  # ref:ft_utils.init_feature_tracks_config


def _check_args(arr, thresh_dog, nb_octaves, nb_scales):
    arr = np.asarray(arr)
    if arr.ndim != 2:
        raise ValueError("expected a 2D image, got shape {}".format(arr.shape))
    if min(arr.shape) < 12:
        raise ValueError("the image must have at least 12 pixels a side, got {} x {}".format(arr.shape[1], arr.shape[0]))
    if int(nb_scales) < 1 or int(nb_scales) > 13:
        raise ValueError("nb_scales must be in [1, 13], got {}".format(nb_scales))
    if int(nb_octaves) < 1:
        raise ValueError("nb_octaves must be positive, got {}".format(nb_octaves))
    if not float(thresh_dog) >= 0.0:
        raise ValueError("thresh_dog must not be negative, got {}".format(thresh_dog))
    if arr.dtype != np.float32:
        arr = arr.astype(np.float32)
    if arr.strides[1] != 4 or arr.strides[0] < 4 * arr.shape[1] or arr.strides[0] % 4:
        arr = np.ascontiguousarray(arr)  # a view with whole rows a fixed distance apart goes as it is
    return arr


def sift_detect(arr, thresh_dog=THRESH_DOG, nb_octaves=NB_OCTAVES, nb_scales=NB_SCALES, device=None, planes=None):
    """satba_sift_detect (include/satba.h).  Returns (rows (n, 132) float32, info); planes: a list of (octave, scale) to fetch, returned
    as info["planes"][(octave, scale)]."""
    arr = _check_args(arr, thresh_dog, nb_octaves, nb_scales)
    lib = E.load_library()
    h, w = arr.shape
    handle, ms = ct.c_void_p(None), ct.c_float(0.0)
    counts = np.zeros(6, dtype=np.int64)
    E._check(lib, lib.satba_sift_detect(arr.ctypes.data_as(_fp), w, h, arr.strides[0] // 4, float(thresh_dog), int(nb_octaves), int(nb_scales),
                                        1 if planes else 0, ct.byref(handle), counts.ctypes.data_as(_lp), _device(device), ct.byref(ms)))
    try:
        rows = np.zeros((int(counts[0]), 132), dtype=np.float32)
        E._check(lib, lib.satba_sift_fetch(handle, rows.ctypes.data_as(_fp)))
        info = {"n_octaves": int(counts[1]), "n_extrema": int(counts[2]), "n_interpolated": int(counts[3]), "n_kept": int(counts[4]),
                "kernel_ms": ms.value, "counts": counts}
        if planes:
            info["planes"] = {}
            for o, s in planes:
                pw, ph = ct.c_int32(0), ct.c_int32(0)
                E._check(lib, lib.satba_sift_fetch_plane(handle, int(o), int(s), None, ct.byref(pw), ct.byref(ph)))
                p = np.zeros((ph.value, pw.value), dtype=np.float32)
                E._check(lib, lib.satba_sift_fetch_plane(handle, int(o), int(s), p.ctypes.data_as(_fp), None, None))
                info["planes"][(int(o), int(s))] = p
    finally:
        lib.satba_sift_destroy(handle)
    return rows, info


def keypoints_from_nparray(arr, thresh_dog=THRESH_DOG, nb_octaves=NB_OCTAVES, nb_scales=NB_SCALES, offset=None, device=None, return_info=False):
    """ref:s2p/sift.py:33-82.  (n, 132) float32 rows (col, row, scale, orientation, descriptor); offset (x, y) is added to the
    positions.  With return_info also a dict: the staged counts and kernel_ms."""
    rows, info = sift_detect(arr, thresh_dog, nb_octaves, nb_scales, device=device)
    if offset is not None:
        x, y = offset
        rows[:, 0] += x
        rows[:, 1] += y
    return (rows, info) if return_info else rows


def _load_image(image, offset=None):
    """an array, a .npy path, or (only where rasterio imports) a GeoTIFF path; offset: dict with col0, row0, width, height"""
    if isinstance(image, (str, bytes)) or hasattr(image, "__fspath__"):
        path = image.decode() if isinstance(image, bytes) else str(image)
        if path.lower().endswith(".npy"):
            image = np.load(path, mmap_mode="r")
        else:
            try:
                import rasterio
            except ImportError:
                raise ValueError("{}: only arrays and .npy files are read without rasterio".format(path))
            with rasterio.open(path) as f:
                image = f.read(1)
    image = np.asarray(image)
    if image.ndim != 2:
        raise ValueError("expected a 2D image, got shape {}".format(image.shape))
    if offset is not None:
        r0, c0 = int(offset["row0"]), int(offset["col0"])
        image = image[r0:r0 + int(offset["height"]), c0:c0 + int(offset["width"])]
    return image


def select_features(features_i, mask=None, max_kp=None):
    """ref:ft_s2p.py:68-81 on the rows of one image: keep the keypoints whose truncated (col, row) is inside the mask, sort by scale,
    descending and stable (equal scales keep their order, as Python's `sorted` leaves them), truncate and pad with NaN to max_kp."""
    features_i = np.asarray(features_i).reshape(-1, 132)
    if mask is not None:
        mask = np.asarray(mask)
        colrow = features_i[:, :2].astype(np.int64)
        features_i = features_i[mask[colrow[:, 1], colrow[:, 0]] > 0, :]
    features_i = features_i[np.argsort(-features_i[:, 2], kind="stable")]
    if max_kp is None:
        return features_i
    out = np.full((int(max_kp), 132), np.nan, dtype=features_i.dtype if features_i.dtype.kind == "f" else np.float64)
    n = min(features_i.shape[0], int(max_kp))
    out[:n] = features_i[:n]
    return out


def detect_features_image_sequence(images, mask_paths=None, offsets=None, tracks_config=None, device=None):
    """ref:ft_s2p.py:18-94.  images: per image an array or a .npy path (a GeoTIFF path only where rasterio imports); mask_paths: per
    image an array or a .npy path; offsets: per image a dict (col0, row0, width, height) that crops by slicing.  With a tracks_config
    the rows are truncated and NaN-padded to its FT_kp_max (60000 when it names none), as the reference does.  Returns the list of
    (n, 132) float32 arrays."""
    if mask_paths is not None and len(mask_paths) != len(images):
        raise ValueError("one mask per image")
    if offsets is not None and len(offsets) != len(images):
        raise ValueError("one offset per image")
    max_kp = None if tracks_config is None else int(tracks_config.get("FT_kp_max", FT_KP_MAX))
    if max_kp is not None and max_kp < 0:
        raise ValueError("FT_kp_max must not be negative, got {}".format(max_kp))
    features = []
    for i, image in enumerate(images):
        arr = _load_image(image, None if offsets is None else offsets[i])
        rows = keypoints_from_nparray(arr, THRESH_DOG, NB_OCTAVES, NB_SCALES, None, device=device)
        mask = None
        if mask_paths is not None:
            mask = mask_paths[i]
            if isinstance(mask, (str, bytes)) or hasattr(mask, "__fspath__"):
                mask = np.load(mask)
        features.append(select_features(rows, mask, max_kp))
    return features


def detect_features_image_sequence_multiprocessing(images, mask_paths=None, offsets=None, tracks_config=None, n_proc=5, device=None):
    """ref:ft_s2p.py:97-124: the same call; the device is the parallelism (n_proc is accepted and ignored)."""
    return detect_features_image_sequence(images, mask_paths, offsets, tracks_config, device=device)

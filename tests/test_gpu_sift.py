"""SIFT detection on the device (satba.ft_s2p, csrc/satba_sift.h) against the float64 rule of tests/cases_sift.py and the reference's
stored rows (tests/golden/ft_sift.npz).

Tolerances.  The fixture stores `spread_*`: the largest differences between the reference and the rule over all paired keypoints of
all cases (column, row, sigma relative, theta, descriptor L-inf and L2) and the largest error of the reference's Gaussian planes
relative to a plane's largest value.  The device works in the reference's float32 with another summation order and other exp /
atan2: against the rule it must stay within 2 x each spread (two independent errors of that size add to sqrt(2) of it, rounded up),
against the reference's rows within 3 x (1 + 2, the triangle inequality), its planes against the rule's planes within 2 x the
plane spread.  Keypoints pair one to one inside a window of 0.05 px, 2 % of sigma and 0.05 rad; an unpaired keypoint on either
side is allowed only at a candidate the rule marks fragile, per case and per octave."""
import ctypes as ct

import numpy as np
import pytest

import cases_sift as CS

pytestmark = pytest.mark.gpu
_cache = {}


@pytest.fixture(scope="module")
def golden():
    return CS.load()


@pytest.fixture(scope="module")
def spread(golden):
    return np.array([float(golden["spread_" + k]) for k in CS.SPREAD_KEYS])


def _run(golden, name):
    """the device's rows, info and every plane of one case, computed once"""
    if name not in _cache:
        from satba import ft_s2p

        c = CS.case(golden, name)
        img = c["image"].astype(np.float32)
        g = CS.geometry(img.shape[1], img.shape[0], c["nb_octaves"], 3, c["thresh_dog"])
        want = [(o, s) for o in range(g["n_oct"]) for s in range(g["n_planes"])]
        rows, info = ft_s2p.sift_detect(img, c["thresh_dog"], c["nb_octaves"], 3, planes=want)
        _cache[name] = (c, g, rows, info)
    return _cache[name]


@pytest.mark.parametrize("name", list(CS.CASES))
def test_planes_against_the_rule(gpu, golden, name):
    c, g, rows, info = _run(golden, name)
    planes = CS.gaussian_planes(c["image"], g)
    tol = 2 * float(golden["spread_plane"])
    worst = 0.0
    for o in range(g["n_oct"]):
        for s in range(g["n_planes"]):
            dev = info["planes"][(o, s)]
            assert dev.shape == (g["h"][o], g["w"][o])
            worst = max(worst, float(np.abs(dev - planes[o][s]).max() / np.abs(planes[o][s]).max()))
    print(name, "planes: largest error", worst, "of", tol)
    assert worst <= tol


def _check_pairs(dev, other, other_fragile_rows, other_octave, cand, fragile, delta, tol, what):
    """dev rows against `other` rows (rule or reference): spreads within tol; unpaired rows only at fragile candidates"""
    ia, ib = CS.pair_rows(dev, other)
    sp = CS.spreads(dev[ia].astype(np.float64), other[ib].astype(np.float64))
    print(what, "paired", len(ia), "of", len(dev), "/", len(other), "differences / tolerance", np.array2string(sp / tol, precision=3))
    for k in np.setdiff1d(np.arange(len(other)), ib):
        if other_fragile_rows is not None:
            assert other_fragile_rows[k], "{}: row {} (octave {}) is missing on the device".format(what, k, other_octave[k])
        else:
            assert CS.fragile_near(cand, fragile, delta, other[k]), "{}: row {} is missing on the device".format(what, k)
    for k in np.setdiff1d(np.arange(len(dev)), ia):
        assert CS.fragile_near(cand, fragile, delta, dev[k]), "{}: row {} of the device is not a keypoint".format(what, k)
    assert np.all(np.diff(ib) > 0), "{}: the device lists its keypoints in another order".format(what)
    assert np.all(sp <= tol), (what, sp, tol)
    return ia, ib


@pytest.mark.parametrize("name", list(CS.CASES))
def test_counts_and_keypoints(gpu, golden, spread, name):
    c, g, rows, info = _run(golden, name)
    n_fragile = int(c["fragile"].sum())
    counts = info["counts"]
    print(name, "device counts", counts.tolist(), "rule", c["counts"].tolist(), "fragile", n_fragile)
    assert counts[1] == c["counts"][1] == g["n_oct"] and counts[5] == 0
    for k in (2, 3, 4):  # a fragile candidate may go either way at one stage and so at every later one
        assert abs(int(counts[k]) - int(c["counts"][k])) <= n_fragile
    if not n_fragile:
        assert counts[:5].tolist() == c["counts"].tolist()
    assert rows.shape == (counts[0], 132) and rows.dtype == np.float32
    assert np.all(rows[:, 4:] == np.rint(rows[:, 4:])) and np.all((rows[:, 4:] >= 0) & (rows[:, 4:] <= 255))
    row_fragile = c["fragile"][c["rule_cand"]] if len(c["rule"]) else np.zeros(0, bool)
    ia, ib = _check_pairs(rows, c["rule"], row_fragile, c["rule_octave"], c["cand"], c["fragile"], g["delta"], 2 * spread, name + " vs rule")
    for o in range(g["n_oct"]):  # per octave: every solid keypoint of the rule is there
        solid = np.nonzero((c["rule_octave"] == o) & ~row_fragile)[0]
        assert set(solid.tolist()) <= set(ib.tolist()), "octave {}".format(o)
    _check_pairs(rows, c["ref"], None, None, c["cand"], c["fragile"], g["delta"], 3 * spread, name + " vs reference")


def test_constant_image_has_no_keypoints(gpu, golden):
    from satba import ft_s2p

    c, g, rows, info = _run(golden, "flat")
    assert rows.shape == (0, 132) and info["counts"][:5].tolist() == [0, g["n_oct"], 0, 0, 0]
    out = ft_s2p.keypoints_from_nparray(np.full((33, 47), 3000.0, dtype=np.float32))
    assert out.shape == (0, 132) and out.dtype == np.float32
    assert ft_s2p.keypoints_from_nparray(np.zeros((12, 12), dtype=np.float64)).shape == (0, 132)


def test_order_is_the_reference_list_order(gpu, golden):
    """(octave, scale, row, column) of the discrete extremum, then orientations ascending by bin"""
    c, g, rows, info = _run(golden, "s208x300")
    ia, ib = CS.pair_rows(rows, c["rule"])
    assert len(ia) >= 0.98 * len(rows) and np.all(np.diff(ib) > 0)
    octave = c["rule_octave"][ib]
    assert np.all(np.diff(octave) >= 0) and octave.max() == c["rule_octave"].max() >= 3
    cand = c["rule_cand"][ib]
    key = c["cand"][cand][:, :4]  # octave, scale, row, column of the discrete extremum
    assert np.all(np.diff(cand) >= 0)
    same = np.nonzero(np.diff(cand) == 0)[0]  # orientations of one keypoint: same place, bins ascending
    assert len(same) > 0
    for k in same:
        a, b = rows[ia[k]], rows[ia[k + 1]]
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
        assert np.mod(a[3], 2 * np.pi) < np.mod(b[3], 2 * np.pi)  # bin b holds [b, b + 1) * 10 degrees of [0, 360)
    flat = ((key[:, 0] * 16 + key[:, 1]) * 4096 + key[:, 2]) * 4096 + key[:, 3]
    assert np.all(np.diff(flat) >= 0)


def test_two_calls_give_identical_bytes(gpu, golden):
    from satba import ft_s2p

    for name in ("s128x200", "s208x300"):
        c, g, rows, info = _run(golden, name)
        again, info2 = ft_s2p.sift_detect(c["image"].astype(np.float32), c["thresh_dog"], c["nb_octaves"], 3)
        assert again.tobytes() == rows.tobytes() and info2["counts"].tolist() == info["counts"].tolist()


def test_strided_view_equals_contiguous(gpu, golden):
    from satba import ft_s2p

    c, g, rows, info = _run(golden, "s61x83")
    big = np.full((70, 101), np.nan, dtype=np.float32)  # what lies around the view must not be read into the result
    big[5:66, 9:92] = c["image"]
    view = big[5:66, 9:92]
    assert not view.flags["C_CONTIGUOUS"] and view.strides == (404, 4)
    out = ft_s2p.keypoints_from_nparray(view)
    assert out.tobytes() == rows.tobytes()
    seq = ft_s2p.detect_features_image_sequence([big], offsets=[{"row0": 5, "col0": 9, "width": 83, "height": 61}])
    assert len(seq) == 1 and np.array_equal(seq[0], rows[np.argsort(-rows[:, 2], kind="stable")])
    moved = ft_s2p.keypoints_from_nparray(view, offset=(9, 5))
    assert np.array_equal(moved[:, 2:], rows[:, 2:]) and np.array_equal(moved[:, 0], rows[:, 0] + np.float32(9))


def test_sequence_masks_sorts_and_pads(gpu, golden):
    from satba import ft_s2p

    c, g, rows, info = _run(golden, "s61x83")
    mask = np.zeros((61, 83), dtype=np.uint8)
    mask[:, :40] = 1
    out = ft_s2p.detect_features_image_sequence([c["image"]], mask_paths=[mask], tracks_config={"FT_kp_max": 25})[0]
    kept = rows[rows[:, 0].astype(np.int64) < 40]
    kept = kept[np.argsort(-kept[:, 2], kind="stable")]
    assert out.shape == (25, 132)
    n = min(len(kept), 25)
    assert n > 5 and np.array_equal(out[:n], kept[:n]) and np.isnan(out[n:]).all()
    both = ft_s2p.detect_features_image_sequence_multiprocessing([c["image"], c["image"]])
    assert len(both) == 2 and np.array_equal(both[0], both[1]) and both[0].shape == rows.shape


def _detect_code(img, w, h, stride, nb_scales=3, keep=0):
    from satba import engine_hip as E

    lib = E.load_library()
    handle, counts = ct.c_void_p(None), np.zeros(6, dtype=np.int64)
    rc = lib.satba_sift_detect(img.ctypes.data_as(ct.POINTER(ct.c_float)), w, h, stride, CS.THRESH_DOG, 8, nb_scales, keep, ct.byref(handle),
                               counts.ctypes.data_as(ct.POINTER(ct.c_int64)), 0, None)
    return lib, rc, handle, counts


def test_error_codes(gpu, golden):
    from satba import ft_s2p

    img = np.ascontiguousarray(CS.image("s52"), dtype=np.float32)
    for w, h in ((11, 52), (52, 11)):
        lib, rc, handle, counts = _detect_code(img, w, h, 52)
        assert rc == -1 and not handle.value and b"12" in lib.satba_last_error()
    lib, rc, handle, counts = _detect_code(img, 52, 52, 52, nb_scales=0)
    assert rc == -1 and not handle.value
    lib, rc, handle, counts = _detect_code(img, 52, 52, 40)
    assert rc == -1 and not handle.value
    for bad in (np.nan, np.inf, -np.inf):
        poisoned = img.copy()
        poisoned[51, 51] = bad  # the last pixel: every pixel is looked at
        lib, rc, handle, counts = _detect_code(poisoned, 52, 52, 52)
        assert rc == -4 and not handle.value and counts[5] == 1
        with pytest.raises(ValueError):
            ft_s2p.keypoints_from_nparray(poisoned)
    lib, rc, handle, counts = _detect_code(img, 52, 52, 52, keep=0)
    assert rc == 0 and handle.value
    w, h = ct.c_int32(0), ct.c_int32(0)
    assert lib.satba_sift_fetch_plane(handle, 0, 0, None, ct.byref(w), ct.byref(h)) == -3  # the planes were not kept
    lib.satba_sift_destroy(handle)
    lib, rc, handle, counts = _detect_code(img, 52, 52, 52, keep=1)
    assert rc == 0 and lib.satba_sift_fetch_plane(handle, 0, 0, None, ct.byref(w), ct.byref(h)) == 0 and (w.value, h.value) == (104, 104)
    assert lib.satba_sift_fetch_plane(handle, 4, 0, None, None, None) == -1 and lib.satba_sift_fetch_plane(handle, 0, 6, None, None, None) == -1
    lib.satba_sift_destroy(handle)
    lib.satba_sift_destroy(None)

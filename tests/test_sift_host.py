"""SIFT detection, the parts that need no device: the float64 rule of tests/cases_sift.py against the reference's stored rows (with the
conditions on the fixture re-checked from tests/golden/ft_sift.npz), the geometry header csrc/satba_sift_geom.h against the rule's
geometry (tests/host/sift_geom_dump.cpp), and the host side of satba/ft_s2p.py."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sat-bundleadjust_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cases_sift as CS  # noqa: E402

CSRC = os.path.join(ROOT, "sat-bundleadjust_amd", "csrc")
SIDES = [12, 13, 24, 25, 52, 61, 83, 208, 4001]
SHAPES = [(s, s) for s in SIDES] + [(61, 83), (83, 61), (208, 300), (4001, 12), (13, 4001)]  # (width, height)


@pytest.fixture(scope="module")
def golden():
    return CS.load()


@pytest.fixture(scope="module")
def rules(golden):
    """the rule run on every stored image, once"""
    return {name: CS.detect(golden[name + "_image"], CS.CASES[name][3], CS.CASES[name][4]) for name in CS.CASES}


# ----------------------------------------------------------------------------- the rule and the fixture

@pytest.mark.parametrize("name", list(CS.CASES))
def test_fixture_holds_the_cases_images(golden, name):
    assert np.array_equal(golden[name + "_image"], CS.image(name))
    assert golden[name + "_image"].shape == CS.CASES[name][:2]
    assert "-ffp-contract=off" in str(golden["flags"]) and "-mavx" in str(golden["flags"])


@pytest.mark.parametrize("name", list(CS.CASES))
def test_rule_is_the_stored_rule(golden, rules, name):
    c, r = CS.case(golden, name), rules[name]
    assert np.array_equal(r["counts"], c["counts"])
    assert np.array_equal(r["rows"][:, 4:], c["rule"][:, 4:])
    assert np.array_equal(r["rows"][:, :4], c["rule"][:, :4])
    assert np.array_equal(r["fragile"], c["fragile"]) and np.array_equal(r["row_octave"], c["rule_octave"])


@pytest.mark.parametrize("name", CS.PARITY_CASES)
def test_fixture_conditions(golden, rules, name):
    c, g = CS.case(golden, name), rules[name]["geom"]
    assert min(min(g["w"]), min(g["h"])) >= 13  # below, the reference's blur reads what it never wrote
    real_fragile = int((c["fragile"] & (c["cand"][:, 4] > 0)).sum())
    assert real_fragile <= 0.02 * len(c["rule"])
    assert len(c["rule"]) >= 20
    assert 2 * float(golden["spread_dog"]) <= CS.EXT_EPS


def test_octave_counts_of_the_cases(rules):
    assert rules["s208x300"]["geom"]["n_oct"] == 6 and rules["s128x200_oct2"]["geom"]["n_oct"] == 2
    assert rules["s128x200"]["geom"]["n_oct"] == 5 and rules["s52"]["geom"]["n_oct"] == 4
    assert rules["s61x83_half"]["counts"][0] > rules["s61x83"]["counts"][0]
    assert rules["flat"]["counts"][0] == 0 and rules["flat"]["rows"].shape == (0, 132)


@pytest.mark.parametrize("name", CS.PARITY_CASES)
def test_rule_against_the_reference(golden, rules, name):
    """away from fragile candidates the reference and the rule name the same keypoints, in the same order, per octave"""
    c, r = CS.case(golden, name), rules[name]
    ref = c["ref"].astype(np.float64)
    ia, ib = CS.pair_rows(ref, r["rows"])
    for k in np.setdiff1d(np.arange(len(r["rows"])), ib):
        assert r["fragile"][r["row_cand"][k]], "row {} of the rule (octave {}) is not in the reference".format(k, r["row_octave"][k])
    for k in np.setdiff1d(np.arange(len(ref)), ia):
        assert CS.fragile_near(r["cand"], r["fragile"], r["geom"]["delta"], ref[k]), "row {} of the reference is not in the rule".format(k)
    assert np.all(np.diff(ib) > 0)
    for o in range(r["geom"]["n_oct"]):  # no octave hides in a percentage
        in_o = np.nonzero(r["row_octave"] == o)[0]
        solid = [k for k in in_o if not r["fragile"][r["row_cand"][k]]]
        assert set(solid) <= set(ib.tolist())
    sp = CS.spreads(ref[ia], r["rows"][ib])
    stored = np.array([float(golden["spread_" + k]) for k in CS.SPREAD_KEYS])
    assert np.all(sp <= stored), (sp, stored)


def test_transposed_image_gives_transposed_keypoints(rules):
    a, b = rules["s61x83"], rules["s83x61"]
    assert a["counts"].tolist() == b["counts"].tolist()
    ka = np.sort(np.round(a["rows"][:, [0, 1, 2]], 6), axis=0)
    kb = np.sort(np.round(b["rows"][:, [1, 0, 2]], 6), axis=0)
    assert np.allclose(ka, kb, atol=1e-5)


# ----------------------------------------------------------------------------- the geometry header

def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler ($CXX, g++, /opt/rocm/lib/llvm/bin/clang++)")
    exe = str(tmp_path_factory.mktemp("sift_geom") / "sift_geom_dump")
    base = [cxx, "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "host", "sift_geom_dump.cpp"), "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    return exe


def _geom(dump, w, h, nb_octaves, nb_scales, thresh):
    r = subprocess.run([dump, str(w), str(h), str(nb_octaves), str(nb_scales), repr(float(thresh))], capture_output=True)
    if r.returncode == 2:
        return None
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()
    words = np.frombuffer(r.stdout, dtype=np.int32)
    f = words.view(np.float32)
    n, ns, p = int(words[0]), int(words[1]), 3
    g = {"n_oct": n, "n_planes": ns, "thr": f[2], "w": [], "h": [], "delta": [], "sigma": [], "inc": [], "taps": []}
    for _ in range(n):
        g["w"].append(int(words[p])); g["h"].append(int(words[p + 1])); g["delta"].append(f[p + 2])
        g["sigma"].append(f[p + 3:p + 3 + ns].copy()); g["inc"].append(f[p + 3 + ns:p + 3 + 2 * ns].copy())
        p += 3 + 2 * ns
        taps = []
        for _ in range(ns):
            r_ = int(words[p])
            taps.append(f[p + 1:p + 2 + r_].copy())
            p += 2 + r_
        g["taps"].append(taps)
    assert p == len(words)
    return g


@pytest.mark.parametrize("nb_octaves,nb_scales,thresh", [(8, 3, CS.THRESH_DOG), (2, 3, CS.THRESH_DOG / 2), (8, 2, 0.02), (8, 5, CS.THRESH_DOG)])
@pytest.mark.parametrize("shape", SHAPES)
def test_geometry_header_against_the_rule(dump, shape, nb_octaves, nb_scales, thresh):
    w, h = shape
    g, e = _geom(dump, w, h, nb_octaves, nb_scales, thresh), CS.geometry(w, h, nb_octaves, nb_scales, thresh)
    assert g is not None and g["n_oct"] == e["n_oct"] >= 1 and g["n_planes"] == e["n_planes"] == nb_scales + 3
    assert g["w"] == e["w"] and g["h"] == e["h"]
    assert g["thr"].tobytes() == np.float32(e["thr"]).tobytes()
    for o in range(e["n_oct"]):
        assert g["delta"][o] == e["delta"][o]
        assert g["sigma"][o].tobytes() == e["sigma"][o].tobytes()  # float32, exactly
        assert g["inc"][o].tobytes() == e["inc"][o].tobytes()
        for s in range(e["n_planes"]):
            assert g["taps"][o][s].tobytes() == CS.taps(e["inc"][o, s]).tobytes(), (o, s)


def test_geometry_numbers(dump):
    """the numbers DESIGN.md quotes: octave counts from the integer division, sizes from integer division, radii at the defaults"""
    counts = {side: CS.octave_count(side, side, 8) for side in SIDES}
    assert counts == {12: 2, 13: 2, 24: 3, 25: 3, 52: 4, 61: 4, 83: 4, 208: 6, 4001: 8}
    assert CS.octave_count(11, 50, 8) == 1 and CS.octave_count(5, 50, 8) == 0
    assert _geom(dump, 5, 50, 8, 3, CS.THRESH_DOG) is None
    g = CS.geometry(61, 83, 8, 3)
    assert g["w"] == [122, 61, 30, 15] and g["h"] == [166, 83, 41, 20]
    radii = [len(CS.taps(s)) - 1 for s in g["inc"][0]]
    assert radii == [5, 5, 7, 8, 10, 13] and max(len(CS.taps(s)) - 1 for s in g["inc"].ravel()) == 13
    assert float(g["thr"]) == float(np.float32(CS.THRESH_DOG))  # nb_scales = 3: the conversion is the identity
    last = CS.geometry(97, 131, 8, 3)
    assert min(last["w"][-1], last["h"][-1]) == 12  # a size the fixture must not use


# ----------------------------------------------------------------------------- the host wrapper

def _rows(scales, tag0=0):
    rows = np.zeros((len(scales), 132), dtype=np.float32)
    rows[:, 2] = scales
    rows[:, 0] = np.arange(len(scales)) + 0.75  # col
    rows[:, 1] = 2 * np.arange(len(scales)) + 0.5  # row
    rows[:, 4] = tag0 + np.arange(len(scales))  # a tag that shows the order
    return rows


def test_select_sorts_stably_by_scale_descending():
    from satba import ft_s2p

    rows = _rows([1.0, 3.0, 1.0, 2.0, 3.0, 1.0])
    out = ft_s2p.select_features(rows)
    assert out[:, 4].tolist() == [1, 4, 3, 0, 2, 5]  # equal scales keep their order, as Python's sorted(reverse=True) leaves them
    expected = np.array(sorted(rows.tolist(), key=lambda kp: kp[2], reverse=True))
    assert np.array_equal(out, expected.astype(np.float32))


def test_select_truncates_and_pads():
    from satba import ft_s2p

    rows = _rows([1.0, 3.0, 1.0, 2.0])
    cut = ft_s2p.select_features(rows, max_kp=3)
    assert cut.shape == (3, 132) and cut[:, 4].tolist() == [1, 3, 0]
    pad = ft_s2p.select_features(rows, max_kp=6)
    assert pad.shape == (6, 132) and pad[:4, 4].tolist() == [1, 3, 0, 2] and np.isnan(pad[4:]).all()
    none = ft_s2p.select_features(np.zeros((0, 132), np.float32), max_kp=2)
    assert none.shape == (2, 132) and np.isnan(none).all()
    assert ft_s2p.select_features(np.zeros((0, 132), np.float32)).shape == (0, 132)


def test_select_masks_by_truncated_position():
    from satba import ft_s2p

    rows = _rows([1.0, 1.0, 1.0, 1.0])  # (col, row) = (0.75, 0.5), (1.75, 2.5), (2.75, 4.5), (3.75, 6.5)
    mask = np.zeros((8, 5), dtype=np.uint8)
    mask[2, 1] = 1  # keeps row 1: int(1.75) = 1, int(2.5) = 2
    mask[6, 3] = 7  # keeps row 3
    mask[4, 3] = 1  # (col 3, row 4) is nobody's truncated position
    out = ft_s2p.select_features(rows, mask)
    assert out[:, 4].tolist() == [1, 3]


@pytest.mark.parametrize("kwargs", [dict(arr=np.zeros((11, 40), np.float32)), dict(arr=np.zeros((40, 11), np.float32)),
                                    dict(arr=np.zeros((40, 40), np.float32), nb_scales=0), dict(arr=np.zeros((40, 40), np.float32), nb_scales=14),
                                    dict(arr=np.zeros((40, 40), np.float32), nb_octaves=0), dict(arr=np.zeros((40, 40), np.float32), thresh_dog=-1.0),
                                    dict(arr=np.zeros((40, 40), np.float32), thresh_dog=float("nan")), dict(arr=np.zeros((4, 40, 40), np.float32))])
def test_argument_errors_raise_before_any_device_call(monkeypatch, kwargs):
    from satba import engine_hip, ft_s2p

    def no_device(*a, **k):
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(engine_hip, "load_library", no_device)
    with pytest.raises(ValueError):
        ft_s2p.keypoints_from_nparray(**kwargs)


def test_sequence_argument_errors(monkeypatch):
    from satba import engine_hip, ft_s2p

    monkeypatch.setattr(engine_hip, "load_library", lambda *a, **k: (_ for _ in ()).throw(AssertionError("the library was loaded")))
    img = np.zeros((40, 40), np.float32)
    with pytest.raises(ValueError):
        ft_s2p.detect_features_image_sequence([img, img], mask_paths=[None])
    with pytest.raises(ValueError):
        ft_s2p.detect_features_image_sequence([img], offsets=[])
    with pytest.raises(ValueError):
        ft_s2p.detect_features_image_sequence(["scene.tif"]) if not _has("rasterio") else ft_s2p.detect_features_image_sequence([np.zeros(5)])
    with pytest.raises(ValueError):
        ft_s2p.detect_features_image_sequence([img], offsets=[{"row0": 0, "col0": 0, "width": 40, "height": 5}])  # the crop is too short


def _has(module):
    try:
        __import__(module)
        return True
    except ImportError:
        return False


def test_symbols_are_declared():
    from satba import engine_hip

    header = open(os.path.join(ROOT, "include", "satba.h")).read()
    for s in ("satba_sift_detect", "satba_sift_fetch", "satba_sift_fetch_plane", "satba_sift_destroy"):
        assert s in engine_hip.SYMBOLS and s + "(" in header

"""
Pairwise matching on the device (satba.ft_match, csrc/satba_match.h) against the numpy rule of tests/cases_match.py, which
tests/test_match_host.py ties to what the reference's compiled `matching` returned (tests/golden/ft_match.npz), and against the
stored index pairs themselves.  Everything is compared exactly: on integer descriptors the rule allows no tolerance.
"""
import numpy as np
import pytest

import cases_match as CM
from satba import ft_match, ft_utils

pytestmark = pytest.mark.gpu

GRID = [(name, v) for name in CM.CASES for v in CM.VARIANTS]
GRID_IDS = ["{}-{}".format(name, v[0]) for name, v in GRID]
SWITCHES = ("SATBA_MATCH_CHUNK", "SATBA_MATCH_FLOAT")
_GOLDEN, _CASES, _RULE = {}, {}, {}


def golden():
    if not _GOLDEN:
        g = CM.load()
        _GOLDEN.update({k: g[k] for k in g.files})
    return _GOLDEN


def case_of(name):
    if name not in _CASES:
        _CASES[name] = CM.from_golden(golden(), name)
    return _CASES[name]


def rule_of(name, variant):
    """computed once per (case, variant), shared and never modified"""
    key = (name, variant[0])
    if key not in _RULE:
        _RULE[key] = CM.rule(case_of(name), variant[1], variant[2], variant[3])
        for a in _RULE[key]:
            a.setflags(write=False)
    return _RULE[key]


def device(case, variant, only=None, **kw):
    _, gate, relative, thr = variant
    idx = list(range(len(case["pairs"]))) if only is None else list(only)
    return ft_match.match_pairs(case["pairs"][idx], case["feats"], case["utm"], case["boxes"][idx], F=[case["F"][p] for p in idx] if gate else None,
                                thr=CM.variant_thr(case, thr, relative), epi_thr=CM.EPI_THR, relative=relative, return_info=True, **kw)


def same(a, b):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(a[:3], b[:3]))


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("name,variant", GRID, ids=GRID_IDS)
def test_device_equals_the_rule_and_the_reference(gpu, name, variant):
    case = case_of(name)
    out = device(case, variant)
    assert same(out, rule_of(name, variant))
    info = out[3]
    assert info["path"] == ("float32" if name == "float" else "int8")
    sel = golden()["{}_{}_sel".format(name, variant[0])]
    assert info["n_selected"] == sel.sum() and info["n_empty_pairs"] == int((sel == 0).any(axis=1).sum())
    assert np.array_equal(out[0], golden()["{}_{}_ofs".format(name, variant[0])])
    if name not in ("same_coords", "ties", "extremes"):  # no two keypoints share a location: the reference's index pairs as stored
        assert np.array_equal(np.stack([out[1], out[2]], axis=1), golden()["{}_{}_renamed".format(name, variant[0])])


@pytest.mark.parametrize("switch", [("SATBA_MATCH_CHUNK", "16"), ("SATBA_MATCH_CHUNK", "64"), ("SATBA_MATCH_FLOAT", "1")], ids=["chunk16", "chunk64", "float"])
@pytest.mark.parametrize("name", CM.INT_CASES)
def test_switches_change_no_match_on_integer_data(gpu, monkeypatch, name, switch):
    monkeypatch.setenv(*switch)
    for variant in CM.VARIANTS:
        out = device(case_of(name), variant)
        assert same(out, rule_of(name, variant)), variant[0]
        assert out[3]["path"] == ("float32" if switch[0] == "SATBA_MATCH_FLOAT" else "int8")


@pytest.mark.parametrize("chunk", ["16", "64"])
def test_float_case_across_chunks(gpu, monkeypatch, chunk):
    monkeypatch.setenv("SATBA_MATCH_CHUNK", chunk)
    for variant in CM.VARIANTS:
        out = device(case_of("float"), variant)
        assert same(out, rule_of("float", variant)) and out[3]["path"] == "float32"


def test_bad_chunk_is_an_argument_error(gpu, monkeypatch):
    monkeypatch.setenv("SATBA_MATCH_CHUNK", "24")
    with pytest.raises(ValueError):
        device(case_of("tiny"), CM.VARIANTS[0])


@pytest.mark.parametrize("variant", CM.VARIANTS, ids=[v[0] for v in CM.VARIANTS])
def test_scene_in_one_call_equals_its_pairs_one_at_a_time(gpu, variant):
    case = case_of("scene")
    ofs, ki, kj, _ = device(case, variant)
    for p in range(len(case["pairs"])):
        o1, i1, j1, _ = device(case, variant, only=[p])
        assert np.array_equal(i1, ki[ofs[p]:ofs[p + 1]]) and np.array_equal(j1, kj[ofs[p]:ofs[p + 1]]) and o1.tolist() == [0, ofs[p + 1] - ofs[p]]
    # pairs in the caller's order, whatever it is
    order = [3, 0, 4, 2, 1]
    o2, i2, j2, _ = device(case, variant, only=order)
    assert np.array_equal(np.diff(o2), np.diff(ofs)[order])
    assert np.array_equal(i2, np.concatenate([ki[ofs[p]:ofs[p + 1]] for p in order]))
    assert np.array_equal(j2, np.concatenate([kj[ofs[p]:ofs[p + 1]] for p in order]))


def test_two_runs_give_identical_bits(gpu):
    for name in ("small", "scene", "float"):
        a, b = device(case_of(name), CM.VARIANTS[0]), device(case_of(name), CM.VARIANTS[0])
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))


def _footprints(case):
    """rectangles whose pairwise intersections are the case's boxes: every image BOX but image 2, which carries the cut"""
    def rect(b):
        return {"geojson": {"type": "Polygon", "coordinates": [[[b[0], b[2]], [b[1], b[2]], [b[1], b[3]], [b[0], b[3]], [b[0], b[2]]]]}}
    return [rect(case["boxes"][1] if m == 2 else CM.BOX) for m in range(len(case["feats"]))]


def test_match_stereo_pairs_feeds_the_track_builder(gpu, tmp_path):
    """the reference's M x 4 rows -- device match, renaming, UTM filter -- equal the stored ones, and ft_utils builds from them the
    tracks it builds from the rule's matches"""
    case, g = case_of("scene"), golden()
    cfg = {"FT_sift_matching": "epipolar_based", "FT_rel_thr": 0.6}
    pairs = [tuple(int(v) for v in p) for p in case["pairs"]]
    rows = ft_match.match_stereo_pairs(pairs, case["feats"], _footprints(case), case["utm"], cfg, F=case["F"])
    fofs, filt = g["scene_gate_rel_fofs"], g["scene_gate_rel_filt"]
    want = np.concatenate([np.concatenate([filt[fofs[p]:fofs[p + 1]], np.tile([pairs[p]], (fofs[p + 1] - fofs[p], 1))], axis=1) for p in range(len(pairs))])
    assert rows.dtype == np.int64 and np.array_equal(rows, want)
    # the same from .npy paths, and without the gate
    paths_f, paths_u = [], []
    for m, (f, u) in enumerate(zip(case["feats"], case["utm"])):
        paths_f.append(str(tmp_path / "f{}.npy".format(m))); paths_u.append(str(tmp_path / "u{}.npy".format(m)))
        np.save(paths_f[-1], f); np.save(paths_u[-1], u)
    assert np.array_equal(ft_match.match_stereo_pairs(pairs, paths_f, _footprints(case), paths_u, cfg, F=case["F"]), rows)
    free = ft_match.match_stereo_pairs(pairs, case["feats"], _footprints(case), case["utm"], dict(cfg, FT_sift_matching="bruteforce"))
    assert np.array_equal(free[:, :2], g["scene_free_rel_filt"])
    # canonical=False returns the matched rows themselves; a geometric filter that keeps every other match is applied per pair
    raw = ft_match.match_stereo_pairs(pairs, case["feats"], _footprints(case), case["utm"], cfg, F=case["F"], canonical=False)
    ofs, ki, kj = rule_of("scene", CM.VARIANTS[0])
    assert set(map(tuple, raw[:, :2])) <= set(zip(ki.tolist(), kj.tolist()))
    half = ft_match.match_stereo_pairs(pairs, case["feats"], _footprints(case), case["utm"], cfg, F=case["F"],
                                       geometric_filter=lambda pi, pj, m: np.arange(len(m)) % 2 == 0)
    assert 0 < len(half) <= (len(ki) + len(pairs)) // 2 + len(pairs)

    kp = np.concatenate([f[:, :3] for f in case["feats"]])
    kp_ofs = np.concatenate([[0], np.cumsum([f.shape[0] for f in case["feats"]])]).astype(np.int64)
    got = ft_utils.feature_tracks_from_matches(kp, kp_ofs, rows, pairs)
    ref = ft_utils.feature_tracks_from_matches(kp, kp_ofs, want, pairs)
    assert got[5] > 0 and got[5] == ref[5] and all(np.array_equal(a, b) for a, b in zip(got[:5], ref[:5]))


def test_one_pair_entry_and_same_coords(gpu):
    """match_kp_within_utm_polygon: the reference's per-pair call; keypoints that share a location are named by the first"""
    case, g = case_of("same_coords"), golden()
    ring = np.array([[CM.BOX[0], CM.BOX[2]], [CM.BOX[1], CM.BOX[2]], [CM.BOX[1], CM.BOX[3]], [CM.BOX[0], CM.BOX[3]]])
    cfg = {"FT_sift_matching": "epipolar_based", "FT_rel_thr": 0.6}
    m, n = ft_match.match_kp_within_utm_polygon(case["feats"][0], case["feats"][1], case["utm"][0], case["utm"][1], ring, cfg, F=case["F"][0])
    assert np.array_equal(m, g["same_coords_gate_rel_filt"]) and n == [len(g["same_coords_gate_rel_renamed"]), len(m)]
    raw, _ = ft_match.match_kp_within_utm_polygon(case["feats"][0], case["feats"][1], case["utm"][0], case["utm"][1], ring, cfg, F=case["F"][0], canonical=False)
    ofs, ki, kj = rule_of("same_coords", CM.VARIANTS[0])
    assert not np.array_equal(raw, m) and set(map(tuple, raw)) <= set(zip(ki.tolist(), kj.tolist()))
    b = case_of("boxes")
    empty = np.array([[b["boxes"][0][0], 0.0], [b["boxes"][0][1], 0.0], [b["boxes"][0][1], 9e3], [b["boxes"][0][0], 9e3]])
    assert ft_match.match_kp_within_utm_polygon(b["feats"][0], b["feats"][1], b["utm"][0], b["utm"][1], empty, cfg, F=b["F"][0]) == (None, [0, 0, 0])


def test_keypoints_to_utm_coords_keeps_the_padding(gpu):
    import os

    from satba import geo_utils
    from satba.rpc_model import RPCModel

    rpc = RPCModel.from_file(os.path.join(os.path.dirname(CM.GOLDEN), "rpc", "20200413_151408_ssc4d2_0011_basic_panchromatic_dn.rpc"))
    f = case_of("padded")["feats"][0]
    n, off = int(np.sum(~np.isnan(f[:, 0]))), {"col0": 100.0, "row0": 50.0}
    assert 0 < n < len(f)
    u = ft_match.keypoints_to_utm_coords(f, rpc, off, 30.0)
    lon, lat = rpc.localization(f[:n, 0].astype(np.float64) + 100.0, f[:n, 1].astype(np.float64) + 50.0, np.full(n, 30.0))
    east, north = geo_utils.utm_from_lonlat(lon, lat)
    assert u.shape == (len(f), 2) and np.array_equal(u[:n], np.stack([east, north], axis=1)) and np.isnan(u[n:]).all()
    assert np.isfinite(u[:n]).all()
    zone = geo_utils.utm_zone_from_lonlat(lon[0], lat[0])
    assert np.array_equal(ft_match.keypoints_to_utm_coords(f, rpc, off, 30.0, zone=zone), u, equal_nan=True)
    assert not np.array_equal(ft_match.keypoints_to_utm_coords(f, rpc, off, 30.0, zone=zone + 1)[:n], u[:n])


def test_argument_errors_raise(gpu):
    c = case_of("tiny")
    one = dict(pairs=[(0, 1)], features=c["feats"], utm_coords=c["utm"], boxes=[CM.BOX])
    for bad in (dict(one, pairs=[(0, 6)]), dict(one, pairs=[(-1, 1)]), dict(one, pairs=[(1, 1)]), dict(one, boxes=[(0.0, np.nan, 0.0, 1.0)]),
                dict(one, thr=0.0), dict(one, thr=-0.6), dict(one, thr=float("nan"))):
        with pytest.raises(ValueError):
            ft_match.match_pairs(**bad)
    ofs, ki, kj = ft_match.match_pairs([], c["feats"], c["utm"], np.zeros((0, 4)))
    assert ofs.tolist() == [0] and ki.size == 0 and kj.size == 0

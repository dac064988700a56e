"""
Pairwise matching without a GPU: the numpy rule of tests/cases_match.py against what the reference's compiled `matching` returned
(tests/golden/ft_match.npz, tools/gen_golden_match.py), and the host pieces of satba.ft_match -- renaming, UTM filter, similarities,
the convex clipper, compute_pairs_to_match -- against the reference's stored results and hand-computed cases.
"""
import numpy as np
import pytest

import cases_match as CM
from satba import engine_hip, ft_match

GRID = [(name, v) for name in CM.CASES for v in CM.VARIANTS]
GRID_IDS = ["{}-{}".format(name, v[0]) for name, v in GRID]


@pytest.fixture(scope="module")
def golden():
    return CM.load()


@pytest.fixture(scope="module")
def cases(golden):
    return {name: CM.from_golden(golden, name) for name in CM.CASES}


@pytest.mark.parametrize("name", CM.CASES)
def test_generators_reproduce_the_stored_cases(cases, name):
    made, stored = CM.make(name), cases[name]
    for k in ("feats", "utm", "F"):
        assert len(made[k]) == len(stored[k])
        for a, b in zip(made[k], stored[k]):
            assert np.array_equal(a, b, equal_nan=True), k
    assert np.array_equal(made["pairs"], stored["pairs"]) and np.array_equal(made["boxes"], stored["boxes"])


@pytest.mark.parametrize("name,variant", GRID, ids=GRID_IDS)
def test_rule_equals_the_reference_matching(golden, cases, name, variant):
    """same selection, same number of matches per pair, the coordinates `matching` returned; where no two keypoints share a
    location also the same index pairs"""
    vname, gate, relative, thr = variant
    case, key = cases[name], "{}_{}_".format(name, vname)
    ofs, ki, kj = CM.rule(case, gate, relative, thr)
    assert np.array_equal(ofs, golden[key + "ofs"])
    sel = [(len(CM.inside(case["utm"][i], b)), len(CM.inside(case["utm"][j], b))) for (i, j), b in zip(case["pairs"], case["boxes"])]
    assert np.array_equal(np.array(sel).reshape(-1, 2), golden[key + "sel"])
    coords = []
    for p, (i, j) in enumerate(case["pairs"]):
        s = slice(ofs[p], ofs[p + 1])
        coords.append(np.concatenate([case["feats"][i][ki[s], :2], case["feats"][j][kj[s], :2]], axis=1))
    assert np.array_equal(np.concatenate(coords), golden[key + "coords"])
    if name != "same_coords" and name != "ties" and name != "extremes":
        assert np.array_equal(np.stack([ki, kj], axis=1), golden[key + "renamed"])


def test_cases_hold_what_they_are_for(golden, cases):
    """the edges the cases were built for are met, by the reference's own output"""
    c = cases["ties"]
    d = CM.distances(c["feats"][0][CM.inside(c["utm"][0], CM.BOX)], c["feats"][1][CM.inside(c["utm"][1], CM.BOX)], None)
    dA, jA, dB = CM.nearest_two(d)
    assert dA[0] == 0 and dB[0] == 0 and jA[0] == 10            # 0 / 0: no match
    assert dA[1] == dB[1] > 0 and jA[1] == 10 and d[1, 290] == dA[1]  # equally near: the lowest j, distB == distA
    assert dA[2] == 0 and dB[2] > 0 and jA[2] == 20
    ren = golden["ties_free_rel_renamed"]
    assert 0 not in ren[:, 0] and 1 not in ren[:, 0] and [2, 20] in ren.tolist()
    e = cases["extremes"]
    assert CM.distances(e["feats"][0][:1], e["feats"][1][:1], None)[0, 0] == 128 * 255 ** 2
    assert golden["boxes_gate_rel_sel"].min() == 0 and (golden["boxes_gate_rel_sel"] > 0).all(axis=1).sum() == 2
    assert golden["tiny_gate_rel_sel"].tolist() == [[1, 1], [1, 17], [17, 1], [6, 17], [17, 6]]
    assert np.diff(golden["tiny_gate_rel_ofs"]).tolist()[3:] == [0, 1]  # all gated out | a single finite candidate
    assert np.isnan(cases["padded"]["feats"][0][-13:]).all() and np.isnan(cases["padded"]["utm"][1][-30:]).all()
    s = cases["same_coords"]["feats"][0]
    assert len(np.unique(s[:, :2], axis=0)) < len(s)


@pytest.mark.parametrize("variant", CM.VARIANTS, ids=[v[0] for v in CM.VARIANTS])
def test_float_case_has_no_query_inside_the_margins(cases, variant):
    """recomputed in float64: no query within 1e-4 (relative) of thr^2, no two nearest within 1e-4 (relative); none is left out"""
    _, gate, relative, thr = variant
    assert CM.margins(cases["float"], gate, relative, thr) == (0, 0)


@pytest.mark.parametrize("name,variant", GRID, ids=GRID_IDS)
def test_renaming_and_utm_filter_equal_the_reference(golden, cases, name, variant):
    vname, gate, relative, thr = variant
    case, key = cases[name], "{}_{}_".format(name, vname)
    ofs, ki, kj = CM.rule(case, gate, relative, thr)
    maps = [ft_match.canonical_index_map(f) for f in case["feats"]]
    fofs = [0]
    filt = []
    for p, (i, j) in enumerate(case["pairs"]):
        s = slice(ofs[p], ofs[p + 1])
        m = np.stack([maps[i][ki[s]], maps[j][kj[s]]], axis=1).astype(np.int64)
        assert np.array_equal(m, golden[key + "renamed"][s])
        # the reference's own renaming, on the selected set: first keypoint there with the same coordinates
        si = CM.inside(case["utm"][i], case["boxes"][p])
        assert np.array_equal(si[CM.first_index_by_coords(case["feats"][i][si], np.searchsorted(si, ki[s]))], m[:, 0])
        f = ft_match.filter_matches_inconsistent_utm_coords(m, case["utm"][i], case["utm"][j]) if len(m) else m
        filt.append(f)
        fofs.append(fofs[-1] + len(f))
    assert np.array_equal(fofs, golden[key + "fofs"])
    assert np.array_equal(np.concatenate(filt), golden[key + "filt"])


@pytest.mark.parametrize("name", CM.CASES)
def test_similarities_equal_the_reference_bit_for_bit(golden, cases, name):
    for p, F in enumerate(cases[name]["F"]):
        s1, s2 = ft_match.rectifying_similarities(F)
        assert s1.dtype == np.float32 and s2.dtype == np.float32
        assert np.concatenate([s1, s2]).tobytes() == golden[name + "_sim"][p].tobytes()
        r1, r2 = CM.similarities(F)
        assert np.concatenate([r1, r2]).tobytes() == golden[name + "_sim"][p].tobytes()
        assert np.concatenate(ft_match.rectifying_similarities([F[0, 2], F[1, 2], F[2, 0], F[2, 1], F[2, 2]])).tobytes() == golden[name + "_sim"][p].tobytes()


def _rect(x0, x1, y0, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


def test_clipper_on_hand_computed_polygons():
    fi = ft_match.footprint_intersection
    area, box = fi(_rect(0, 10, 0, 8), _rect(2, 5, 1, 3))  # nested
    assert area == 6.0 and box == (2.0, 5.0, 1.0, 3.0)
    assert fi(_rect(2, 5, 1, 3), _rect(0, 10, 0, 8)) == (6.0, (2.0, 5.0, 1.0, 3.0))
    area, box = fi(_rect(0, 4, 0, 4), _rect(2, 9, -3, 2))  # overlapping corners
    assert area == 4.0 and box == (2.0, 4.0, 0.0, 2.0)
    # a square of diagonal 4 (rotated by 45 degrees) centred on a square of side 2 .. covers it; on one of side 3: an octagon
    diamond = [(0, -2), (2, 0), (0, 2), (-2, 0)]
    area, box = fi(_rect(-1, 1, -1, 1), diamond)
    assert area == 4.0 and box == (-1.0, 1.0, -1.0, 1.0)
    area, box = fi(diamond, _rect(-1.5, 1.5, -1.5, 1.5))
    assert abs(area - (9.0 - 4 * 0.5)) < 1e-12 and box == (-1.5, 1.5, -1.5, 1.5)  # four corner triangles of legs 1 are cut off
    # clockwise input and a closed geojson ring give the same
    closed = {"geojson": {"type": "Polygon", "coordinates": [[[0, 0], [0, 8], [10, 8], [10, 0], [0, 0]]]}}
    assert fi(closed, _rect(2, 5, 1, 3)) == (6.0, (2.0, 5.0, 1.0, 3.0)) and ft_match.polygon_area(closed) == 80.0
    assert fi(_rect(0, 1, 0, 1), _rect(1, 2, 0, 1)) == (0.0, None)  # touching along an edge
    assert fi(_rect(0, 1, 0, 1), _rect(1, 2, 1, 2)) == (0.0, None)  # touching at a vertex
    assert fi(_rect(0, 1, 0, 1), _rect(3, 4, 0, 1)) == (0.0, None)  # disjoint
    assert fi(_rect(0, 1, 0, 1), diamond_at(5, 5)) == (0.0, None)


def diamond_at(x, y):
    return [(x, y - 2), (x + 2, y), (x, y + 2), (x - 2, y)]


def test_compute_pairs_to_match_on_a_hand_case():
    """five footprints in a row; cameras 3 and 4 are close to each other and 4 sees nothing else: the exception keeps (3, 4)"""
    fp = [{"geojson": {"type": "Polygon", "coordinates": [[list(p) for p in _rect(x0, x0 + 10, 0, 10)]]}} for x0 in (0, 5, 9.5, 14, 18)]
    centers = [np.array([0.0, 0.0, 5e5]), np.array([2e5, 0.0, 5e5]), np.array([4e5, 0.0, 5e5]), np.array([6e5, 0.0, 5e5]), np.array([6.1e5, 0.0, 5e5])]
    init = [(0, 1), (2, 0), (1, 2), (0, 3), (2, 3), (4, 3), (1, 1 + 3)]
    m, t = ft_match.compute_pairs_to_match(init, fp, centers, verbose=False)
    # overlaps of the first: (0,1) 50 %, (2,0) 5 % of 2 -> out, (1,2) 55 %, (0,3) none, (2,3) 55 %, (4,3) 60 %, (1,4) none
    assert m == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert t == [(0, 1), (1, 2), (2, 3), (3, 4)]  # (3, 4): baseline 1e4 / 5e5 < 1/4, kept for camera 4
    m, t = ft_match.compute_pairs_to_match([(0, 1), (3, 4)], fp, centers, verbose=False)
    assert m == [(0, 1), (3, 4)] and t == [(0, 1), (3, 4), ]
    m, t = ft_match.compute_pairs_to_match([(0, 1), (2, 3), (3, 4)], fp, centers, min_baseline=0.5, verbose=False)
    assert m == [(0, 1), (2, 3), (3, 4)] and t == [(0, 1), (2, 3), (3, 4)]  # every baseline too short: all kept by the exception


def test_selection_and_argument_checks_need_no_device(cases):
    c = cases["boxes"]
    for p, (i, j) in enumerate(c["pairs"]):
        u = c["utm"][i]
        assert np.array_equal(ft_match.get_pt_indices_inside_utm_bbx(u[:, 0], u[:, 1], *c["boxes"][p]), CM.inside(u, c["boxes"][p]))
    with pytest.raises(ValueError):
        ft_match.match_stereo_pairs([(0, 1)], c["feats"], [None] * 3, c["utm"], {"FT_sift_matching": "flann", "FT_rel_thr": 0.6})
    with pytest.raises(ValueError):
        ft_match.match_stereo_pairs([(0, 1)], c["feats"], [None] * 3, c["utm"], {"FT_sift_matching": "epipolar_based", "FT_rel_thr": 0.6}, F=None)
    with pytest.raises(ValueError):
        ft_match.match_pairs([(0, 3)], c["feats"], c["utm"], [CM.BOX])


def test_library_declares_the_matching_entries_and_keeps_its_version():
    lib = engine_hip.load_library()
    assert lib.satba_version() == 5
    for sym in ("satba_match_pairs", "satba_matches_fetch", "satba_matches_destroy"):
        assert sym in engine_hip.SYMBOLS and hasattr(lib, sym), sym

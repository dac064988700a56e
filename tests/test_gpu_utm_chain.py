"""
The device UTM filter and the vectorised renaming in the place the chain uses them: the tail of match_stereo_pairs.  The two-view
scene of tests/test_gpu_ransac_chain.py, rebuilt from the same helpers, with two more pairs: one whose footprints share no area,
and one between the first view and a third image -- the second view with every keypoint moved 3 .. 15 px off its epipolar line,
matches that pass the rectified gate and that no fundamental matrix explains.  The device RANSAC cannot leave a pair without a match
(its winner keeps its own sample), so it cuts that pair down; the callable empties it.  What match_stereo_pairs returns is compared
with the host composition pair by pair: match_pairs, canonical_index_map, the mask, filter_matches_inconsistent_utm_coords.
"""
import functools

import numpy as np
import pytest

import cases_camapprox as CC
import cases_fundamental as CF
import cases_match as CM
from satba import ft_match, ft_utils

pytestmark = pytest.mark.gpu
N_PTS, N_OUT = 300, 60
CASE = CF.CASES[0]
CFG = {"FT_sift_matching": "epipolar_based", "FT_ransac": 0.3}
PAIRS = [(0, 1), (0, 2), (0, 3)]


def _footprint(box):
    ring = [[box[0], box[2]], [box[1], box[2]], [box[1], box[3]], [box[0], box[3]], [box[0], box[2]]]
    return {"geojson": {"type": "Polygon", "coordinates": [ring]}}


@functools.lru_cache(maxsize=None)
def scene():
    """features (4 x (N_PTS, 132) float32), utm (4 x (N_PTS, 2)), footprints, F per pair: images 0 and 1 are the views of
    test_gpu_ransac_chain.py, image 2 lies elsewhere, image 3 is image 1 off its epipolar lines"""
    rng = np.random.default_rng([22, 11])
    r0, r1 = CC.rpc(0), CC.rpc(1)
    Fg = CF.load_golden()[CF.key(CASE) + "_F"]
    desc, _, utm = CM._points(rng, N_PTS)
    col, row = rng.uniform(50.0, 3150.0, N_PTS), rng.uniform(50.0, 1300.0, N_PTS)
    alt = r0.alt_offset + rng.uniform(-0.1, 0.1, N_PTS) * r0.alt_scale
    lon, lat = CF.Rpc(r0).localization(col, row, alt)
    x1, y1 = r0.projection(lon, lat, alt)
    x2, y2 = r1.projection(lon, lat, alt)
    pts = np.vstack([x1, y1, x2, y2]).T
    outliers = np.sort(rng.permutation(N_PTS)[:N_OUT])
    nrm = np.array([Fg[0, 2], Fg[1, 2]]) / np.hypot(Fg[0, 2], Fg[1, 2])
    shift = rng.uniform(3.0, 15.0, N_OUT) * rng.choice([-1.0, 1.0], N_OUT)
    pts[outliers, 2:] += shift[:, None] * nrm[None, :]
    assert np.abs(CF.residual(Fg, pts)).max() < 20.0  # every match passes the gate
    feats, utms = [], []
    for v in range(2):
        f = np.zeros((N_PTS, 132), dtype=np.float32)
        f[:, :2], f[:, 2], f[:, 3] = pts[:, 2 * v: 2 * v + 2], 1.0 + rng.integers(0, 16, N_PTS) / 4.0, rng.integers(0, 360, N_PTS)
        f[:, 4:] = np.clip(desc + np.rint(4.0 * rng.standard_normal((N_PTS, 128))).astype(np.int64), 0, 255)
        feats.append(f)
        utms.append(utm + v * np.array([3.0, -2.0]) + 0.5 * rng.standard_normal((N_PTS, 2)))
    # image 2: the first view, 5 km to the east: no overlap
    feats.append(feats[0].copy())
    utms.append(utms[0] + np.array([5000.0, 0.0]))
    # image 3: the second view, every keypoint off its epipolar line
    f3 = feats[1].copy()
    f3[:, :2] += ((rng.uniform(3.0, 15.0, N_PTS) * rng.choice([-1.0, 1.0], N_PTS))[:, None] * nrm[None, :]).astype(np.float32)
    feats.append(f3)
    utms.append(utms[1] + 0.5 * rng.standard_normal((N_PTS, 2)))
    b = CM.BOX
    footprints = [_footprint(b), _footprint(b), _footprint((b[0] + 5000.0, b[1] + 5000.0, b[2], b[3])), _footprint(b)]
    return feats, utms, footprints, [Fg] * len(PAIRS)


def empties_the_third_pair(pix_i, pix_j, m_ij):
    """every other match, and none between image 0 and image 3"""
    if np.array_equal(pix_j, scene()[0][3][:, :2]):
        return np.zeros(len(m_ij), dtype=bool)
    return np.arange(len(m_ij)) % 2 == 0


def by_hand(feats, utms, footprints, F, geometric_filter, seed=0):
    """the host composition, pair by pair; the RANSAC masks come from one call over the live pairs, as a pair's samples depend on
    its place in the call"""
    boxes = [ft_match.footprint_intersection(footprints[i], footprints[j])[1] for i, j in PAIRS]
    live = [k for k, b in enumerate(boxes) if b is not None]
    ofs, kp_i, kp_j = ft_match.match_pairs([PAIRS[k] for k in live], feats, utms, [boxes[k] for k in live], F=[F[k] for k in live])
    maps = [ft_match.canonical_index_map(f) for f in feats]
    pairs = []
    for m, k in enumerate(live):
        i, j = PAIRS[k]
        s = slice(ofs[m], ofs[m + 1])
        pairs.append(np.stack([maps[i][kp_i[s]], maps[j][kp_j[s]]], axis=1).astype(np.int64))
    masks = [np.ones(len(m_ij), dtype=bool) for m_ij in pairs]
    if geometric_filter == "ransac":
        xy = np.concatenate([np.concatenate([feats[PAIRS[k][0]][m_ij[:, 0], :2], feats[PAIRS[k][1]][m_ij[:, 1], :2]], axis=1)
                             for k, m_ij in zip(live, pairs)]).astype(np.float64)
        mask = ft_match.ransac_fundamental(ofs, xy, CFG["FT_ransac"], seed=seed)
        masks = [mask[ofs[m]:ofs[m + 1]] for m in range(len(live))]
    elif geometric_filter is not None:
        masks = [np.asarray(geometric_filter(feats[PAIRS[k][0]][:, :2], feats[PAIRS[k][1]][:, :2], m_ij), dtype=bool) for k, m_ij in zip(live, pairs)]
    rows, counts = [], []
    for k, m_ij, mask in zip(live, pairs, masks):
        i, j = PAIRS[k]
        m_ij = m_ij[mask]
        if len(m_ij):
            m_ij = ft_match.filter_matches_inconsistent_utm_coords(m_ij, utms[i], utms[j])
        rows.append(np.concatenate([m_ij, np.tile(np.array([[i, j]], dtype=np.int64), (len(m_ij), 1))], axis=1))
        counts.append((len(mask), int(mask.sum()), len(m_ij)))
    return np.concatenate(rows, axis=0), live, counts


@pytest.mark.parametrize("geometric_filter", [None, "ransac", empties_the_third_pair], ids=["none", "ransac", "callable"])
def test_match_stereo_pairs_equals_the_host_composition(gpu, geometric_filter):
    feats, utms, footprints, F = scene()
    rows, info = ft_match.match_stereo_pairs(PAIRS, feats, footprints, utms, CFG, F=F, geometric_filter=geometric_filter, return_info=True)
    want, live, counts = by_hand(feats, utms, footprints, F, geometric_filter)
    assert live == [0, 2]  # the second pair's footprints share no area
    assert rows.dtype == np.int64 and rows.shape[1] == 4 and np.array_equal(rows, want)
    assert info["utm_kernel_ms"] > 0 and ("ransac_kernel_ms" in info) == (geometric_filter == "ransac")
    assert counts[0][0] >= 0.9 * N_PTS and counts[1][0] >= 0.85 * N_PTS  # both live pairs were matched
    assert (rows[:, 2] == 0).all() and set(rows[:, 3].tolist()) <= {1, 3} and (rows[:, 3] == 1).sum() == counts[0][2]
    if geometric_filter is None:
        assert counts[1][2] >= 0.65 * N_PTS  # nothing but the UTM filter looks at the third pair
    elif geometric_filter == "ransac":
        assert 7 <= counts[1][1] <= 0.2 * counts[1][0]  # no matrix explains the third pair: few matches are left to the UTM filter
        assert counts[0][1] >= 0.7 * counts[0][0]
    else:
        assert counts[1][1] == 0 and not (rows[:, 3] == 3).any() and counts[0][1] == (counts[0][0] + 1) // 2
    # the one-pair entry goes the same way
    ring = np.array(footprints[0]["geojson"]["coordinates"][0])
    m, n = ft_match.match_kp_within_utm_polygon(feats[0], feats[1], utms[0], utms[1], ring, CFG, F=F[0], geometric_filter=geometric_filter)
    assert np.array_equal(m, want[want[:, 3] == 1, :2])  # (a pair's RANSAC samples depend on its place in the call: pair 0 in both)
    assert n == ([counts[0][0], counts[0][2]] if geometric_filter is None else [counts[0][0], counts[0][1], counts[0][2]])


def test_no_live_pair_and_no_match(gpu):
    feats, utms, footprints, F = scene()
    rows, info = ft_match.match_stereo_pairs([(0, 2)], feats, footprints, utms, CFG, F=F[:1], geometric_filter="ransac", return_info=True)
    assert rows.shape == (0, 4) and rows.dtype == np.int64 and info["utm_kernel_ms"] == 0.0
    # a live pair without a match: the second view moved 5 000 px across the epipolar lines, all candidates fail the gate
    blank = [f.copy() for f in feats]
    blank[1][:, :2] += (5000.0 * np.array([F[0][0, 2], F[0][1, 2]]) / np.hypot(F[0][0, 2], F[0][1, 2])).astype(np.float32)
    for geometric_filter in (None, "ransac", empties_the_third_pair):
        rows, info = ft_match.match_stereo_pairs([(0, 1)], blank, footprints, utms, CFG, F=F[:1], geometric_filter=geometric_filter, return_info=True)
        assert rows.shape == (0, 4) and rows.dtype == np.int64 and info["utm_kernel_ms"] == 0.0


def test_utm_coordinates_of_the_batch_feed_the_chain(gpu):
    """keypoints_to_utm_coords_batch in front: the keypoints of the two views through their RPCs, the footprint around what came
    out, match_stereo_pairs with the device RANSAC and filter, and ft_utils behind"""
    feats, _, _, F = scene()
    feats = feats[:2]
    r0, r1 = CC.rpc(0), CC.rpc(1)
    utms = ft_match.keypoints_to_utm_coords_batch(feats, [r0, r1], [{"col0": 0.0, "row0": 0.0}] * 2, [r0.alt_offset, r1.alt_offset])
    single = [ft_match.keypoints_to_utm_coords(f, r, {"col0": 0.0, "row0": 0.0}, r.alt_offset) for f, r in zip(feats, (r0, r1))]
    assert all(np.abs(a - b).max() < 1e-6 for a, b in zip(utms, single))
    both = np.concatenate(utms)
    fp = _footprint((both[:, 0].min() - 10.0, both[:, 0].max() + 10.0, both[:, 1].min() - 10.0, both[:, 1].max() + 10.0))
    rows, info = ft_match.match_stereo_pairs([(0, 1)], feats, [fp, fp], utms, CFG, F=F[:1], geometric_filter="ransac", return_info=True)
    ofs, kp_i, kp_j = ft_match.match_pairs([(0, 1)], feats, utms, [ft_match.footprint_intersection(fp, fp)[1]], F=F[:1])
    m_ij = np.stack([kp_i, kp_j], axis=1).astype(np.int64)
    xy = np.concatenate([feats[0][m_ij[:, 0], :2], feats[1][m_ij[:, 1], :2]], axis=1).astype(np.float64)
    mask = ft_match.ransac_fundamental(ofs, xy, CFG["FT_ransac"])
    want = ft_match.filter_matches_inconsistent_utm_coords(m_ij[mask], utms[0], utms[1])
    assert info["utm_kernel_ms"] > 0 and len(want) >= 0.5 * N_PTS
    assert np.array_equal(rows[:, :2], want) and np.all(rows[:, 2] == 0) and np.all(rows[:, 3] == 1)
    kp = np.concatenate([f[:, :3] for f in feats])
    kp_ofs = np.array([0, N_PTS, 2 * N_PTS], dtype=np.int64)
    got = ft_utils.feature_tracks_from_matches(kp, kp_ofs, rows, [(0, 1)])
    assert got[5] > 0

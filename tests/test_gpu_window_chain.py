"""
The windowed matching in the place the chain uses it: match_stereo_pairs with FT_sift_matching = "local_window" on the scene of
tests/test_gpu_utm_chain.py (two views, an image elsewhere, the second view off its epipolar lines), against the composition by
hand: the numpy rule of tests/cases_window.py on the boxed keypoints, the vectorised renaming, the device RANSAC's mask where one is
asked for, and filter_matches_inconsistent_utm_coords pair by pair.  And locally_match_SIFT_utm_coords, the one-pair function under
the reference's name.
"""
import numpy as np
import pytest

import cases_window as W
import test_gpu_utm_chain as UC
from satba import ft_match

pytestmark = pytest.mark.gpu
CFG = {"FT_sift_matching": "local_window", "FT_ransac": 0.3}
PAIRS = UC.PAIRS


def by_hand(feats, utms, footprints, cfg, geometric_filter, seed=0):
    boxes = [ft_match.footprint_intersection(footprints[i], footprints[j])[1] for i, j in PAIRS]
    live = [k for k, b in enumerate(boxes) if b is not None]
    sides = [PAIRS[k] for k in live]
    case = dict(feats=feats, utm=utms, pairs=np.asarray(sides, dtype=np.int32), boxes=np.asarray([boxes[k] for k in live], dtype=np.float64))
    r = cfg.get("FT_local_radius", 30.0)
    ofs, ki, kj, _ = W.rule_window(case, r, r, cfg.get("FT_abs_thr", 250))
    m_ij, im, used, rows = ft_match._rename_all(ofs, ki, kj, sides, feats, True)
    mask = np.ones(len(m_ij), dtype=bool)
    if geometric_filter == "ransac":
        xy = ft_match._both_sides([f[:, :2] for f in feats], used, rows).astype(np.float64)
        mask = ft_match.ransac_fundamental(ofs, xy, cfg["FT_ransac"], seed=seed)
    out, counts = [], []
    for m, (i, j) in enumerate(sides):
        s = slice(ofs[m], ofs[m + 1])
        kept = m_ij[s][mask[s]]
        if len(kept):
            kept = ft_match.filter_matches_inconsistent_utm_coords(kept, utms[i], utms[j])
        out.append(np.concatenate([kept, np.tile(np.array([[i, j]], dtype=np.int64), (len(kept), 1))], axis=1))
        counts.append((int(ofs[m + 1] - ofs[m]), int(mask[s].sum()), len(kept)))
    return np.concatenate(out, axis=0), live, counts


@pytest.mark.parametrize("geometric_filter", [None, "ransac"], ids=["none", "ransac"])
@pytest.mark.parametrize("cfg", [CFG, dict(CFG, FT_local_radius=4.0, FT_abs_thr=60)], ids=["defaults", "4m-thr60"])
def test_match_stereo_pairs_equals_the_host_composition(gpu, cfg, geometric_filter):
    feats, utms, footprints, _ = UC.scene()
    rows, info = ft_match.match_stereo_pairs(PAIRS, feats, footprints, utms, cfg, geometric_filter=geometric_filter, return_info=True)
    want, live, counts = by_hand(feats, utms, footprints, cfg, geometric_filter)
    print(cfg, geometric_filter, counts, info)
    assert live == [0, 2]  # the second pair's footprints share no area
    assert rows.dtype == np.int64 and rows.shape[1] == 4 and np.array_equal(rows, want)
    assert info["path"] == "int8" and info["n_candidates"] > 0 and info["utm_kernel_ms"] > 0
    assert ("ransac_kernel_ms" in info) == (geometric_filter == "ransac")
    if cfg is CFG:
        assert counts[0][0] >= 0.9 * UC.N_PTS  # the views lie 3.6 m apart on the ground: a 30 m window holds every true match
    else:
        assert 0 < counts[0][0] < by_hand(feats, utms, footprints, CFG, None)[2][0][0]  # the key and the threshold are read
    # the one-pair entry goes the same way
    ring = np.array(footprints[0]["geojson"]["coordinates"][0])
    m, n = ft_match.match_kp_within_utm_polygon(feats[0], feats[1], utms[0], utms[1], ring, cfg, geometric_filter=geometric_filter)
    assert np.array_equal(m, want[want[:, 3] == 1, :2])
    assert n == ([counts[0][0], counts[0][2]] if geometric_filter is None else list(counts[0]))


def test_locally_match_SIFT_utm_coords(gpu):
    feats, utms, _, _ = UC.scene()
    args = [feats[0].copy(), feats[1].copy(), utms[0].copy(), utms[1] - np.array([0.0, 1e7])]  # the second image's northings are negative
    before = [a.copy() for a in args]
    m, n, n_geo = ft_match.locally_match_SIFT_utm_coords(*args, radius=30, sift_thr=250, ransac_thr=0.3)
    assert all(np.array_equal(a, b) for a, b in zip(args, before))  # the reference writes into its arguments; this does not
    shifted = before[3].copy()
    shifted[shifted[:, 1] < 0, 1] += 10e6
    case = dict(feats=feats[:2], utm=[before[2], shifted], pairs=np.array([[0, 1]], dtype=np.int32), boxes=np.array([W.EVERYWHERE]))
    ofs, ki, kj, _ = W.rule_window(case, 30.0, 30.0, 250.0)
    assert n == ofs[-1] >= 0.9 * UC.N_PTS and m is not None and n_geo == len(m) and 8 <= n_geo <= n
    assert m.shape[1] == 2 and set(map(tuple, m.tolist())) <= set(zip(ki.tolist(), kj.tolist()))
    mask = ft_match.ransac_fundamental([0, n], ft_match._match_coords(feats[0], feats[1], np.stack([ki, kj], axis=1)), max_err=0.3)
    assert np.array_equal(m, np.stack([ki, kj], axis=1)[mask])
    # without the shift the images lie 10 000 km apart: no window holds a candidate
    far = [a.copy() for a in before]
    far[2][:, 1] += 3e7
    assert ft_match.locally_match_SIFT_utm_coords(*far) == (None, 0, 0)

"""
The device RANSAC in the place the chain uses it: the geometric filter of match_stereo_pairs, between the renaming and the UTM
filter.  The two-view scene of tests/test_gpu_fundamental_chain.py -- ground points projected through both shipped RPCs, descriptors
of the cases_match generator -- with planted wrong matches that only geometry can find: their partner stays inside the box, passes
the +-20 px rectified gate and lies 3 .. 15 px off its epipolar line.  Heights stay within a tenth of the RPC's altitude scale, where
one fundamental matrix describes the pair to 0.12 px (the restatement of tests/cases_ransac.py keeps all 240 planted inliers there).
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


@functools.lru_cache(maxsize=None)
def scene():
    """features (2 x (N_PTS, 132) float32), utm (2 x (N_PTS, 2)), the indices of the planted wrong matches, footprints, F"""
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
    b = CM.BOX
    ring = [[b[0], b[2]], [b[1], b[2]], [b[1], b[3]], [b[0], b[3]], [b[0], b[2]]]
    return feats, utms, outliers, [{"geojson": {"type": "Polygon", "coordinates": [ring]}}] * 2, [Fg]


def _same(rows):
    return set(int(k) for k in rows[rows[:, 0] == rows[:, 1], 0])


def test_ransac_filter_in_match_stereo_pairs(gpu):
    feats, utms, outliers, footprints, F = scene()
    inliers = np.setdiff1d(np.arange(N_PTS), outliers)
    plain = ft_match.match_stereo_pairs([(0, 1)], feats, footprints, utms, CFG, F=F)
    rows, info = ft_match.match_stereo_pairs([(0, 1)], feats, footprints, utms, CFG, F=F, geometric_filter="ransac", return_info=True)
    assert rows.dtype == np.int64 and rows.shape[1] == 4 and info["ransac_kernel_ms"] > 0
    # without the filter the planted wrong matches are there (the UTM filter may cut a few of the widest matches of either kind)
    assert len(_same(plain) & set(outliers.tolist())) >= 0.9 * N_OUT and len(_same(plain) & set(inliers.tolist())) >= 0.9 * len(inliers)
    # with it none of them is ...
    assert not (_same(rows) & set(outliers.tolist()))
    # ... and the filter itself loses no planted inlier: the matches in front of it, its mask, and the UTM filter behind it
    ofs, kp_i, kp_j = ft_match.match_pairs([(0, 1)], feats, utms, [CM.BOX], F=F)
    m_ij = np.stack([kp_i, kp_j], axis=1).astype(np.int64)
    xy = np.concatenate([feats[0][m_ij[:, 0], :2], feats[1][m_ij[:, 1], :2]], axis=1).astype(np.float64)
    mask = ft_match.ransac_fundamental([0, len(m_ij)], xy, CFG["FT_ransac"])
    true = m_ij[:, 0] == m_ij[:, 1]
    assert true[np.isin(m_ij[:, 0], inliers)].sum() >= 0.95 * len(inliers)  # the matcher found the planted pairs
    assert mask[true & np.isin(m_ij[:, 0], inliers)].all() and not mask[true & np.isin(m_ij[:, 0], outliers)].any()
    assert (true & np.isin(m_ij[:, 0], outliers)).sum() >= 0.9 * N_OUT
    want = ft_match.filter_matches_inconsistent_utm_coords(m_ij[mask], utms[0], utms[1])
    assert np.array_equal(rows[:, :2], want) and np.all(rows[:, 2] == 0) and np.all(rows[:, 3] == 1)

    def by_hand(pix_i, pix_j, m_ij):
        kept, mask = ft_match.geometric_filtering(pix_i, pix_j, m_ij, CFG["FT_ransac"], return_mask=True)
        return mask.ravel().astype(bool)

    assert np.array_equal(ft_match.match_stereo_pairs([(0, 1)], feats, footprints, utms, CFG, F=F, geometric_filter=by_hand), rows)
    # another seed is another sequence of samples (the planted matches are as clear to it)
    other = ft_match.match_stereo_pairs([(0, 1)], feats, footprints, utms, CFG, F=F, geometric_filter="ransac", ransac_seed=7)
    assert not (_same(other) & set(outliers.tolist()))
    with pytest.raises(ValueError):
        ft_match.match_stereo_pairs([(0, 1)], feats, footprints, utms, CFG, F=F, geometric_filter="lmeds")

    kp = np.concatenate([f[:, :3] for f in feats])
    kp_ofs = np.array([0, N_PTS, 2 * N_PTS], dtype=np.int64)
    got = ft_utils.feature_tracks_from_matches(kp, kp_ofs, rows, [(0, 1)])
    assert got[5] > 0


def test_one_pair_entry_counts_the_filter(gpu):
    feats, utms, outliers, footprints, F = scene()
    ring = np.array(footprints[0]["geojson"]["coordinates"][0])
    m0, n0 = ft_match.match_kp_within_utm_polygon(feats[0], feats[1], utms[0], utms[1], ring, CFG, F=F[0])
    m1, n1 = ft_match.match_kp_within_utm_polygon(feats[0], feats[1], utms[0], utms[1], ring, CFG, F=F[0], geometric_filter="ransac")
    assert len(n0) == 2 and len(n1) == 3 and n1[0] == n0[0] and n1[0] - n1[1] >= 0.9 * N_OUT and n1[2] == len(m1)
    rows = ft_match.match_stereo_pairs([(0, 1)], feats, footprints, utms, CFG, F=F, geometric_filter="ransac")
    assert np.array_equal(rows[:, :2], m1)

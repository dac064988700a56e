"""
The device's fundamental matrix in the place the chain uses it: the epipolar gate of the pairwise matching.  A two-view scene of
ground points projected through both shipped RPCs, descriptors of the cases_match generator, and planted outliers whose partner
lies more than 20 px off its epipolar line: matching gated with fundamental_matrices' F returns exactly what it returns with the
reference's F (tests/golden/ft_fundamental.npz), keeps every planted inlier and drops every planted outlier.
"""
import functools

import numpy as np
import pytest

import cases_camapprox as CC
import cases_fundamental as CF
import cases_match as CM
from satba import ft_match

pytestmark = pytest.mark.gpu
N_PTS, N_OUT = 300, 60
CASE = CF.CASES[0]  # pair (0, 1), the full image, n = 5: the region fundamental_matrices takes


@functools.lru_cache(maxsize=None)
def scene():
    """features (2 x (N_PTS, 132) float32), utm (2 x (N_PTS, 2)), the indices of the planted outliers"""
    rng = np.random.default_rng([21, 11])
    r0, r1 = CC.rpc(0), CC.rpc(1)
    Fg = CF.load_golden()[CF.key(CASE) + "_F"]
    desc, _, utm = CM._points(rng, N_PTS)
    col, row = rng.uniform(50.0, 3150.0, N_PTS), rng.uniform(50.0, 1300.0, N_PTS)
    alt = r0.alt_offset + rng.uniform(-0.5, 0.5, N_PTS) * r0.alt_scale
    lon, lat = CF.Rpc(r0).localization(col, row, alt)
    x1, y1 = r0.projection(lon, lat, alt)
    x2, y2 = r1.projection(lon, lat, alt)
    pts = np.vstack([x1, y1, x2, y2]).T
    assert np.abs(CF.residual(Fg, pts)).max() < 10.0  # true correspondences lie within the RPCs' non-linearity of their lines
    outliers = np.sort(rng.permutation(N_PTS)[:N_OUT])
    # an outlier's partner moves 30 .. 300 px along the normal of its epipolar line in image 1
    nrm = np.array([Fg[0, 2], Fg[1, 2]]) / np.hypot(Fg[0, 2], Fg[1, 2])
    shift = rng.uniform(30.0, 300.0, N_OUT) * rng.choice([-1.0, 1.0], N_OUT)
    pts[outliers, 2:] += shift[:, None] * nrm[None, :]
    assert np.abs(CF.residual(Fg, pts[outliers])).min() > 20.0
    feats, utms = [], []
    for v in range(2):
        f = np.zeros((N_PTS, 132), dtype=np.float32)
        f[:, :2], f[:, 2], f[:, 3] = pts[:, 2 * v: 2 * v + 2], 1.0 + rng.integers(0, 16, N_PTS) / 4.0, rng.integers(0, 360, N_PTS)
        f[:, 4:] = np.clip(desc + np.rint(4.0 * rng.standard_normal((N_PTS, 128))).astype(np.int64), 0, 255)
        feats.append(f)
        utms.append(utm + v * np.array([3.0, -2.0]) + 0.5 * rng.standard_normal((N_PTS, 2)))
    return feats, utms, outliers


def test_matching_gated_with_the_device_matrix_equals_the_reference_matrix(gpu):
    feats, utms, outliers = scene()
    rpcs, offs = [CC.rpc(0), CC.rpc(1)], [CC.offset(CC.CROPS["full"])] * 2
    F_dev = ft_match.fundamental_matrices([(0, 1)], rpcs, offs)
    Fg = CF.load_golden()[CF.key(CASE) + "_F"]
    runs = {}
    for name, F in (("device", F_dev), ("reference", [Fg]), ("negated", [-F_dev[0]]), ("none", None)):
        ofs, kp_i, kp_j = ft_match.match_pairs([(0, 1)], feats, utms, [CM.BOX], F=F)
        runs[name] = np.stack([kp_i, kp_j], axis=1)
        assert ofs[0] == 0 and ofs[1] == len(kp_i)
    assert np.array_equal(runs["device"], runs["reference"]) and np.array_equal(runs["device"], runs["negated"])
    inliers = np.setdiff1d(np.arange(N_PTS), outliers)
    got = {tuple(m) for m in runs["device"]}
    assert all((k, k) in got for k in inliers)  # every planted inlier survives
    assert not any((k, k) in got for k in outliers)  # (a query whose gate leaves one candidate matches it: a few false pairs remain)
    free = {tuple(m) for m in runs["none"]}
    assert all((k, k) in free for k in outliers)  # ... which only the gate removes
    print("{} matches with the gate ({} inliers planted), {} without".format(len(got), len(inliers), len(free)))


def test_the_chain_runs_on_this_tree_alone(gpu):
    """fundamental_matrices' list is what match_stereo_pairs takes"""
    feats, utms, outliers = scene()
    rpcs, offs = [CC.rpc(0), CC.rpc(1)], [CC.offset(CC.CROPS["full"])] * 2
    b = CM.BOX
    ring = [[b[0], b[2]], [b[1], b[2]], [b[1], b[3]], [b[0], b[3]], [b[0], b[2]]]
    footprints = [{"geojson": {"type": "Polygon", "coordinates": [ring]}}] * 2
    cfg = {"FT_sift_matching": "epipolar_based"}
    F_dev = ft_match.fundamental_matrices([(0, 1)], rpcs, offs)
    out = ft_match.match_stereo_pairs([(0, 1)], feats, footprints, utms, cfg, F=F_dev)
    ref = ft_match.match_stereo_pairs([(0, 1)], feats, footprints, utms, cfg, F=[CF.load_golden()[CF.key(CASE) + "_F"]])
    assert np.array_equal(out, ref) and out.shape[1] == 4 and np.all(out[:, 2] == 0) and np.all(out[:, 3] == 1)
    true = out[out[:, 0] == out[:, 1], 0]
    assert not np.intersect1d(true, outliers).size and true.size >= 0.9 * (N_PTS - N_OUT)  # (the UTM filter may cut a few of the widest)

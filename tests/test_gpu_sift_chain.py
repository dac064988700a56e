"""Detection feeding the matching: the two views of tests/cases_sift.py (one scene, cut twice, VIEW_SHIFT whole pixels apart) go
through satba.ft_s2p.keypoints_from_nparray and satba.ft_match.match_pairs.

The scene is constant for VIEW_MARGIN = 40 pixels and more around its texture in either view, and the shift is a multiple of the
sample spacing of the octaves used, so wherever no blur reaches from the texture across a border and back (twice the margin, 80
pixels) the two views' planes are the same function of the scene.  The chain runs VIEW_OCTAVES = 2 octaves: the blurs of octave 0
reach 23 pixels (the sum of their radii, 47 samples of half a pixel), those of octave 1 start from plane 3 of octave 0 (12 pixels)
and add 47 samples of one pixel, 59 pixels in all.  There a keypoint of one view is the same keypoint of the other, displaced by
the shift: every match must show that within 2 x the position spread of the fixture."""
import numpy as np
import pytest

import cases_sift as CS

pytestmark = pytest.mark.gpu


def test_two_views_match_with_the_known_shift(gpu):
    from satba import ft_match, ft_s2p

    z = CS.load()
    a, b = z["view_a_image"], z["view_b_image"]
    dr, dc = CS.VIEW_SHIFT
    assert np.array_equal(a[dr:, dc:], b[:a.shape[0] - dr, :a.shape[1] - dc])
    fa = ft_s2p.keypoints_from_nparray(a, nb_octaves=CS.VIEW_OCTAVES)
    fb = ft_s2p.keypoints_from_nparray(b, nb_octaves=CS.VIEW_OCTAVES)
    assert len(fa) >= 40 and len(fb) >= 40
    # "UTM" coordinates: the position in the scene, one box around everything
    ua = fa[:, :2].astype(np.float64)
    ub = fb[:, :2].astype(np.float64) + np.array([dc, dr], dtype=np.float64)
    box = (-1000.0, 1000.0, -1000.0, 1000.0)
    ofs, kp_i, kp_j = ft_match.match_pairs([(0, 1)], [fa, fb], [ua, ub], [box], F=None)
    assert ofs.tolist() == [0, len(kp_i)]
    # the overlap in view a: what view b sees too
    inside = (fa[:, 0] >= dc) & (fa[:, 1] >= dr)
    matched = np.zeros(len(fa), bool)
    matched[kp_i] = True
    share = matched[inside].sum() / max(inside.sum(), 1)
    d_col = fa[kp_i, 0].astype(np.float64) - fb[kp_j, 0].astype(np.float64) - dc
    d_row = fa[kp_i, 1].astype(np.float64) - fb[kp_j, 1].astype(np.float64) - dr
    tol_col, tol_row = 2 * float(z["spread_col"]), 2 * float(z["spread_row"])
    print("keypoints", len(fa), len(fb), "inside the overlap", int(inside.sum()), "matched", len(kp_i), "share", share,
          "largest displacement error", np.abs(d_col).max(), np.abs(d_row).max(), "of", tol_col, tol_row)
    assert inside.sum() >= 40 and share >= 0.5
    assert np.all(np.abs(d_col) <= tol_col) and np.all(np.abs(d_row) <= tol_row)

"""
Affine fundamental matrices from RPCs on the device (satba.rpc_utils -> csrc/satba_fundamental.h) against the reference's vectors
(tests/golden/ft_fundamental.npz) and numpy's SVD, in the metric of tests/cases_fundamental.py (what the epipolar gate sees, px).

Bounds.
* Matches: the device localisation is held to the oracle's within 1e-9 deg per angle by the project's tests; a projection moves by
  at most col_scale / lon_scale (... row_scale / lat_scale) pixels per degree of normalised extent, so a coordinate may differ by
  2 x 1e-9 deg x the largest of the four ratios of the projecting RPC (cases_fundamental.match_tolerance: 3.2e-6 px here).
* Eigen-solve: the device's F against numpy.linalg.svd on the device's own matches, 10 x the yardstick of
  test_fundamental_host.py (the float64 restatement against the reference on the same case): the device differs from the
  restatement in summation order and fused multiply-adds only.  The product stays far below the parity level of 1e-6 px.
* Whole route against the reference's F: the sum of the two.

Measured on an MI355X: matches <= 1.6e-6 px (the reference's own stopping error of the localisation, which the device iterates
past: DESIGN.md 4n), eigen-solve 7e-13 .. 1.1e-11 px, whole route 6e-11 .. 1.1e-8 px, other hemispheres <= 2.6e-12 px.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import cases_camapprox as CC
import cases_fundamental as CF
import cases_octants as CO
from satba import engine_hip, rpc_utils

pytestmark = pytest.mark.gpu
E_NONFINITE = -4


@functools.lru_cache(maxsize=None)
def golden():
    return dict(CF.load_golden())


@functools.lru_cache(maxsize=None)
def solve_tolerance(case):
    tol = CF.SOLVE_MARGIN * CF.yardstick(golden(), case)
    assert tol <= CF.PX_CAP
    return tol


@functools.lru_cache(maxsize=None)
def tables():
    return np.stack([CC.rpc(0).to_table(), CC.rpc(1).to_table()])


def device(pairs, roi, n=5, matches=True, tabs=None):
    """F5 (P, 5), sv (P, 4), degenerate (P,), matches (P, n^3, 4) or None"""
    return rpc_utils._fundamental(tables() if tabs is None else tabs, pairs, roi, n, None, matches)[:4]


@functools.lru_cache(maxsize=None)
def device_case(case):
    i, j, _, n = case
    F5, sv, deg, m = device([(i, j)], [CF.roi(case)], n)
    assert not deg[0]
    return F5[0], sv[0], m[0]


@pytest.mark.parametrize("case", CF.CASES, ids=CF.key)
def test_matches_against_reference_vectors(gpu, case):
    i, j, _, n = case
    ri, rj = CC.rpc(i), CC.rpc(j)
    m = rpc_utils.matches_from_rpc(ri, rj, *CF.roi(case), n)
    assert m.shape == (n ** 3, 4) and np.array_equal(m, device_case(case)[2])  # the wrapper's two tables or the batch's: one kernel
    d = np.abs(m - golden()[CF.key(case) + "_matches"]).max(axis=0)
    tol = np.array([CF.match_tolerance(ri)] * 2 + [CF.match_tolerance(rj)] * 2)
    print("{}: matches against the reference x1 {:.3e} y1 {:.3e} x2 {:.3e} y2 {:.3e} px (bounds {:.3e}, {:.3e})".format(CF.key(case), *d, tol[0], tol[2]))
    assert np.all(d <= tol)
    # x1, y1 is the re-projection of the localised node: close to the node, not the node
    col, row, _ = CF.mesh(ri, CF.roi(case), n)
    assert np.abs(m[:, 0] - col).max() <= 1e-5 and np.abs(m[:, 1] - row).max() <= 1e-5


@pytest.mark.parametrize("case", CF.CASES, ids=CF.key)
def test_eigen_solve_against_svd_of_the_device_matches(gpu, case):
    F5, sv, m = device_case(case)
    tol, pts = solve_tolerance(case), CF.metric_points(golden(), case)
    d = CF.distance(F5, CF.svd_f5(m), pts)
    print("{}: device F against SVD of its matches {:.3e} px (bound {:.3e}), N {:.3e}".format(CF.key(case), d, tol, CF.vector_distance(F5, CF.svd_f5(m))))
    assert d <= tol
    # the sign rule, the unit length, F22 = -N . mean, the singular values
    assert F5[np.argmax(np.abs(F5[:4]))] > 0.0 and abs(np.linalg.norm(F5[:4]) - 1.0) <= 4 * np.finfo(float).eps
    X = m[:, [2, 3, 0, 1]]
    assert abs(F5[4] + F5[:4] @ X.mean(axis=0)) <= 64 * np.finfo(float).eps * np.abs(X).max()
    s = np.linalg.svd(X - X.mean(axis=0), compute_uv=False)
    assert np.all(np.diff(sv) <= 0) and np.abs(sv ** 2 - s ** 2).max() <= 64 * np.finfo(float).eps * s[0] ** 2


@pytest.mark.parametrize("case", CF.CASES, ids=CF.key)
def test_whole_route_against_reference_vectors(gpu, case):
    i, j, crop, n = case
    F5 = device_case(case)[0]
    Fg, pts = golden()[CF.key(case) + "_F"], CF.metric_points(golden(), case)
    tol = max(CF.match_tolerance(CC.rpc(i)), CF.match_tolerance(CC.rpc(j))) + solve_tolerance(case)
    d = CF.distance(F5, Fg, pts)
    print("{}: device F against the reference's {:.3e} px (bound {:.3e}), N {:.3e}".format(CF.key(case), d, tol, CF.vector_distance(F5, Fg)))
    assert d <= tol
    if crop == "full":  # the region fundamental_matrices takes: the crop's size at the origin
        Fs, info = rpc_utils.fundamental_matrices([(i, j)], [CC.rpc(0), CC.rpc(1)], [CC.offset(CC.CROPS[crop])] * 2, n=n, return_info=True)
        assert Fs[0].shape == (3, 3) and np.array_equal(CF.f5(Fs[0]), F5) and np.count_nonzero(Fs[0]) == 5
        assert not info["degenerate"][0] and np.array_equal(info["sv"][0], device_case(case)[1]) and info["kernel_ms"] > 0.0
        assert np.array_equal(rpc_utils.fundamental_matrices([(i, j)], [CC.rpc(0), CC.rpc(1)], [CC.offset(CC.CROPS[crop])] * 2, n=n)[0], Fs[0])


def test_sample_counts_and_regions_at_their_limits(gpu):
    r0, r1 = CC.rpc(0), CC.rpc(1)
    for n in (1, CF.MAX_N + 1):
        with pytest.raises(ValueError):
            rpc_utils.matches_from_rpc(r0, r1, 0, 0, 3200, 1350, n)
    with pytest.raises(ValueError):
        device([(0, 1)], [(0.0, 0.0, 0.0, 1350.0)])
    # a region of 1 x 1 px: the two smallest singular values are 3.2 and 2.7 px apart from 5e4, still a matrix.  A normal matrix
    # is good to eps lambda_1 / (lambda_3 - lambda_4) = 2e-7 in N there, times the 3 px extent: inside the parity level
    for region in ((1600.0, 700.0, 1.0, 1.0), (0.0, 0.0, 1.0, 1.0)):
        F5, sv, deg, m = device([(0, 1)], [region])
        d = CF.distance(F5[0], CF.svd_f5(m[0]), m[0])
        print("region {}: singular values {}, device F against SVD of its matches {:.3e} px".format(region, sv[0], d))
        assert not deg[0] and np.isfinite(F5).all() and d <= CF.PX_CAP
        # no residual above the whole set's root sum of squares (sigma_4 = |A N|, in the metric's normalisation)
        assert np.abs(CF.residual(F5[0], m[0])).max() <= sv[0][3] / np.hypot(F5[0][0], F5[0][1])


@functools.lru_cache(maxsize=None)
def singles():
    """every pair of the largest batch on its own: one call each"""
    pairs, roi = CF.batch(257)
    return [device(pairs[k:k + 1], roi[k:k + 1]) for k in range(len(pairs))]


@pytest.mark.parametrize("n_pairs", [1, 2, 65, 257])
def test_a_pair_does_not_depend_on_its_batch(gpu, n_pairs):
    pairs, roi = CF.batch(n_pairs)
    assert len({tuple(r) for r in roi[:6]}) == min(n_pairs, 6)
    F5, sv, deg, m = device(pairs, roi)
    again = device(pairs, roi)
    for a, b in zip((F5, sv, deg, m), again):
        assert np.array_equal(a, b)  # two calls repeat bitwise
    assert not deg.any() and np.isfinite(F5).all()
    for k in range(n_pairs):
        f1, s1, _, m1 = singles()[k]
        assert np.array_equal(F5[k], f1[0]) and np.array_equal(sv[k], s1[0]) and np.array_equal(m[k], m1[0]), k
    # the outputs nobody asked for change nothing
    assert np.array_equal(device(pairs, roi, matches=False)[0], F5)


def test_degenerate_pair_is_flagged_and_its_neighbours_are_untouched(gpu):
    pairs, roi = [(0, 1), (0, 0), (1, 0)], [CC.CROPS["full"]] * 3
    F5, sv, deg, m = device(pairs, roi)
    assert list(deg) == [False, True, False] and np.isnan(F5[1]).all() and np.isfinite(m).all()
    assert np.array_equal(m[1][:, :2], m[1][:, 2:]) and sv[1][2] ** 2 <= CF.RANK_TOL * sv[1][0] ** 2
    print("pair of an image with itself: singular values", sv[1])
    for k in (0, 2):
        f1, s1, _, m1 = device(pairs[k:k + 1], roi[k:k + 1])
        assert np.array_equal(F5[k], f1[0]) and np.array_equal(sv[k], s1[0]) and np.array_equal(m[k], m1[0])
    # two tables with the same content are as degenerate as one table named twice
    same = np.stack([tables()[0], tables()[0]])
    assert device([(0, 1)], roi[:1], tabs=same)[2][0]
    # without the flags: an error code, and no output is written
    lib = engine_hip.load_library()
    p, r = np.ascontiguousarray(pairs, dtype=np.int32), np.ascontiguousarray(roi, dtype=np.float64)
    outF, outS, outM = np.full((3, 5), 7.0), np.full((3, 4), 7.0), np.full((3, 125, 4), 7.0)
    rc = lib.satba_rpc_fundamental(2, engine_hip._ptr(tables()), 3, engine_hip._ptr(p, engine_hip._ip), engine_hip._ptr(r), 5, engine_hip._ptr(outF),
                                   engine_hip._ptr(outS), engine_hip._ptr(outM), None, 0)
    assert rc == E_NONFINITE and b"Singular matrix: pair 1 (images 0, 0)" in lib.satba_last_error()
    assert np.all(outF == 7.0) and np.all(outS == 7.0) and np.all(outM == 7.0)
    # ... and the same call without the degenerate pair succeeds
    keep = np.ascontiguousarray(p[[0, 2]])
    assert lib.satba_rpc_fundamental(2, engine_hip._ptr(tables()), 2, engine_hip._ptr(keep, engine_hip._ip), engine_hip._ptr(r), 5, engine_hip._ptr(outF),
                                     None, None, None, 0) == 0
    assert np.array_equal(outF[:2], F5[[0, 2]]) and np.all(outF[2] == 7.0)
    # the Python wrapper
    rpcs, offs = [CC.rpc(0), CC.rpc(1)], [CC.offset(CC.CROPS["full"])] * 2
    with pytest.raises(np.linalg.LinAlgError, match=r"pair 1 \(images 0, 0\)"):
        rpc_utils.fundamental_matrices(pairs, rpcs, offs)
    Fs, info = rpc_utils.fundamental_matrices(pairs, rpcs, offs, return_info=True)
    assert list(info["degenerate"]) == [False, True, False] and np.isnan(Fs[1][0, 2]) and np.array_equal(CF.f5(Fs[2]), F5[2])


@pytest.mark.parametrize("placement", CO.PLACEMENTS[1:], ids=CO.placement_id)
def test_other_hemispheres(gpu, placement):
    """The chain's exact symmetries move the ground, not the images: F of a moved pair is F of the original pair.
    The original pair is the moved one taken back.  At a shift of -90 degrees the two longitude offsets (-72.7 -> -162.7, the next
    binade) are ROUNDED by the move, each on its own, so the moved pair is the exact image of a pair whose offsets sit up to one
    ulp of 163 degrees (2.8e-14 deg, 3e-9 m on the ground between the two images) from the shipped ones: against the shipped pair
    itself F22 differs by 4.4e-9 px, which is that displacement and no error of the kernel.  Every other placement takes back to
    the shipped pair bit for bit."""
    rpcs_moved = CO.rpcs(*placement)
    rpcs_back = [CO.moved_rpc(r, -placement[0], placement[1]) for r in rpcs_moved]
    for back, mv, shipped in zip(rpcs_back, rpcs_moved, (CC.rpc(0), CC.rpc(1))):
        assert np.array_equal(CO.moved_rpc(back, *placement).to_table(), mv.to_table())  # the move of the original is exact
        t = back.to_table() - shipped.to_table()
        assert not np.delete(t, 80).any() and abs(t[80]) <= (2.0 ** -45 if placement[0] == -90.0 else 0.0)
    pairs, roi = [(0, 1), (1, 0)], [CC.CROPS["full"]] * 2
    F5, _, deg, m = device(pairs, roi, tabs=np.stack([r.to_table() for r in rpcs_moved]))
    F0, _, deg0, m0 = device(pairs, roi, tabs=np.stack([r.to_table() for r in rpcs_back]))
    assert not deg.any() and not deg0.any()
    for k, case in enumerate((CF.CASES[0], CF.CASES[3])):
        assert case[:3] == (pairs[k][0], pairs[k][1], "full")
        if placement[0] != -90.0:
            assert np.array_equal(F0[k], device_case(case)[0])
        d = CF.distance(F5[k], F0[k], CF.metric_points(golden(), case))
        print("{} {}: F against the original placement {:.3e} px (bound {:.3e}), matches {:.3e} px; against the shipped pair {:.3e} px".format(
            CO.placement_id(placement), CF.key(case), d, solve_tolerance(case), np.abs(m[k] - m0[k]).max(),
            CF.distance(F5[k], device_case(case)[0], CF.metric_points(golden(), case))))
        assert d <= solve_tolerance(case)

"""
The scenarios of tests/cases_outliers.py on the CPU: `rule` (the yardstick of tests/test_gpu_outliers.py) against vectors of the
reference's own compute_obs_to_remove (tests/golden/outliers_edges.npz), each scenario being what its name says -- conditions on the
inputs, so that a GPU test cannot pass vacuously --, and the rm_outliers golden against the CPU oracle's triangulation.
"""
import numpy as np
import pytest

import cases
import cases_outliers as CO
from satba import ba_outliers

SHAPED_N = [n for lay in CO.LAYOUTS for n in CO.counts(lay) if n >= CO.SHAPED_MIN_N]  # 255 ... 1025, 70 001, and twelve of 1 000 to 3 000


@pytest.fixture(scope="module")
def golden():
    g = cases.golden("outliers_edges")
    return {k: g[k] for k in g.files}


def test_layouts_have_the_prescribed_counts():
    assert CO.counts("edges") == (0, 1, 2, 3, 255, 256, 257, 511, 512, 513, 1025, 70001)
    assert all(1000 <= c <= 3000 for c in CO.counts("bulk")) and len(CO.counts("bulk")) == CO.N_CAM
    for lay in CO.LAYOUTS:
        L = CO.layout(lay)
        assert np.array_equal(np.bincount(L["cam_ind"], minlength=CO.N_CAM), CO.counts(lay))
        key = L["pts_ind"] * CO.N_CAM + L["cam_ind"]
        assert np.all(np.diff(key) > 0) and L["pts_ind"].max() + 1 == L["pts3d"].shape[0]  # point-major, cameras ascending, no gaps
        p = CO.layout_params(lay)
        assert p.C is None and p.n_obs == sum(CO.counts(lay)) and p.n_cam == CO.N_CAM
    # the builders are deterministic, finite, non-negative and do not arrive sorted
    for pat in CO.PATTERNS:
        for n in (0, 1, 2, 3, 257, 1025):
            v = CO.errors(pat, n, 5)
            assert v.shape == (n,) and np.array_equal(v, CO.errors(pat, n, 5)) and np.all(np.isfinite(v)) and np.all(v >= 0)
            if n > 3 and not pat.startswith("equal"):
                assert not np.array_equal(v, np.sort(v)) and not np.array_equal(v, CO.errors(pat, n, 6))


def test_rule_equals_the_reference_on_every_scenario(golden):
    """ref:bundle_adjust/ba_outliers.py:112-155 (golden) against `rule`: thresholds bit-equal, removed set index-exact, on every case
    the reference can run -- all but the camera without observations, which `rule` gives 0.0 and an empty set."""
    seen = 0
    for key, lay, pattern, predef_thr, min_thr in CO.edge_cases():
        L = CO.layout(lay)
        err = CO.layout_errors(lay, pattern)
        thr, remove = CO.rule(err, L["cam_ind"], CO.N_CAM, predef_thr, min_thr)
        has = np.asarray(L["counts"]) > 0
        assert np.array_equal(thr[has], golden[key + "/thr"]), key
        if predef_thr is None:
            assert np.all(thr[~has] == 0.0)
        assert np.array_equal(remove, np.unpackbits(golden[key + "/removed"], count=err.size).astype(bool)), key
        seen += 1
    assert seen == len(CO.LAYOUTS) * (len(CO.PATTERNS) * len(CO.MIN_THRS) + len(CO.PREDEF_THRS)) == len(golden) // 2


def test_plateau_is_decided_by_rounding():
    """In every plateau vector the two largest float64 distances differ by at most 4 ulp (measured: at most 2), the elbow counts
    (success), and an evaluation in longdouble -- every product and sum rounded elsewhere, like a contracted one -- ends at another
    rounded threshold in at least 80 % of them (measured: 136 of 144 over these sizes with 12 seeds each; the layouts' own 19 below)."""
    other, total = 0, 0
    for lay in CO.LAYOUTS:
        for c, n in enumerate(CO.counts(lay)):
            if n < CO.SHAPED_MIN_N:
                continue
            v = CO.errors("plateau", n, c)
            d, _ = CO.chord_distances(v)
            top = np.sort(d)[-2:]
            assert top[1] - top[0] <= 4 * np.spacing(top[1]), (lay, n)
            elbow, success = ba_outliers.get_elbow_value(v)
            assert success
            a, b = int(0.85 * n), int(0.95 * n)
            s = np.sort(v)
            assert s[a] <= elbow <= s[b - 1] and s[b - 1] - s[a] > 1.5  # the candidates span pixels, not ulps
            t64, tld = CO.threshold_in(v, np.float64, 0.0), CO.threshold_in(v, np.longdouble, 0.0)
            assert t64 == np.round(elbow, 2)
            other += t64 != tld
            total += 1
    assert total == len(SHAPED_N) == 20
    if np.finfo(np.longdouble).nmant > 52:  # (a platform whose longdouble is float64 has no second evaluation to offer)
        assert other >= 0.8 * total, (other, total)


def test_each_scenario_is_what_its_name_says():
    for n in SHAPED_N:
        for seed in (0, 7):
            elbow, success = ba_outliers.get_elbow_value(CO.errors("no_elbow", n, seed))
            assert not success
            v = CO.errors("min_thr", n, seed)
            elbow, success = ba_outliers.get_elbow_value(v)
            assert success and 0.35 < elbow < 1.0
            for m in (1.0, 2.75):  # one error equal to the binding min_thr, one a double above
                assert np.sum(v == m) == 1 and np.sum(v == np.nextafter(m, np.inf)) == 1
            for pat, E in CO.HALF_ELBOWS.items():
                v = CO.errors(pat, n, seed)
                elbow, success = ba_outliers.get_elbow_value(v)
                assert success and elbow == E, (pat, n, elbow)
                R = np.round(E, 2)
                assert np.sum(v == R) == 1 and np.sum(v == np.nextafter(R, np.inf)) == 1
            v = CO.errors("wide", n, seed)
            d, u = CO.chord_distances(v)
            s = np.sort(v)
            # the square of the value range overflows and the unit chord comes out as (0, 0): the distance of point i degenerates to
            # |(i, v_i - v_0)|, infinite from the first value whose own square overflows on; np.argmax takes that first one.  (With a
            # finite range no distance is NaN: the chord is x / inf = 0, never inf / inf.)
            with np.errstate(over="ignore"):
                assert np.isinf((s[-1] - s[0]) ** 2) and np.all(u == 0.0) and not np.isnan(d).any()
                first = int(np.argmax(d))
                assert np.isinf(d[first]) and np.all(np.isfinite(d[:first])) and np.isinf(s[first] ** 2) and np.isfinite(s[first - 1] ** 2)
            assert s[0] < np.finfo(np.float64).tiny  # a subnormal smallest value
    # the halves: thr * 100 has the fractional part exactly 0.5 where the decimal value survives the product, and rint goes to even
    for E, frac, R in ((0.125, 0.5, 0.12), (2.675, 0.5, 2.68), (1e6 + 0.005, 0.5, 1e6)):
        assert (E * 100.0) % 1.0 == frac and np.round(E, 2) == R
    # ... and just below it where the product rounds down: the threshold goes down although the decimal value is a half
    for E, R in ((0.285, 0.28), (1.005, 1.0)):
        assert 0.4999 < (E * 100.0) % 1.0 < 0.5 and np.round(E, 2) == R
    for n in (1, 2, 3, 255, 70001):  # all equal: every distance is 0 (n = 1: NaN), the argmax is 0, the threshold max(value, min_thr)
        for pat, val in (("equal_0", 0.0), ("equal_2.5", 2.5)):
            v = CO.errors(pat, n, 0)
            assert np.all(v == val) and ba_outliers.get_elbow_value(v) == (val, True)
            thr, remove = CO.rule(v, np.zeros(n, dtype=int), 1, None, 1.0)
            assert thr[0] == max(val, 1.0) and not remove.any()  # (err > thr: equal stays)


def test_the_two_mistakes_the_scenarios_are_for_change_a_threshold():
    """
    What tests/test_gpu_outliers.py would see if k_out_elbow made one of the two mistakes random vectors cannot show, replayed on the
    CPU per camera of each layout (segments up to 5 000 values: the fused product is evaluated in rational arithmetic).
    A fused multiply-add in the scalar product: another threshold on 3 of 7 (edges) and 6 of 12 (bulk) plateau vectors, on no random one.
    The last of the tied maxima instead of the first: another threshold on 4 of 7 and 11 of 12 plateau vectors (their top distances tie
    exactly) and on every wide one (all distances from the first overflowing square on are inf) -- and on no `equal` vector: there every
    candidate carries the same value, so `equal` guards the count and the comparison, not the tie-break.
    """
    for lay in CO.LAYOUTS:
        changed = {}
        for pattern in ("plateau", "wide", "equal_2.5", "random"):
            for mutation in ("fma", "last"):
                k = 0
                for c, n in enumerate(CO.counts(lay)):
                    if CO.SHAPED_MIN_N <= n <= 5000:
                        v = CO.errors(pattern, n, c)
                        k += CO.threshold_mutated(v, mutation) != CO.threshold_in(v, np.float64, 0.0)
                changed[pattern, mutation] = int(k)
        n_vec = sum(CO.SHAPED_MIN_N <= n <= 5000 for n in CO.counts(lay))
        assert changed["plateau", "fma"] >= 3 and changed["plateau", "last"] >= 3, changed
        assert changed["wide", "last"] == n_vec and changed["wide", "fma"] == 0, changed
        assert changed["random", "fma"] == changed["random", "last"] == changed["equal_2.5", "fma"] == changed["equal_2.5", "last"] == 0, changed


def test_rule_on_the_smallest_segments():
    """n = 0, 1, 2, 3 by hand."""
    cam = np.array([1, 2, 2, 3, 3, 3])
    err = np.array([7.0, 0.5, 9.0, 0.25, 0.5, 30.0])
    thr, remove = CO.rule(err, cam, 4, None, 1.0)
    # one value: the chord is a point, distances NaN, argmax 0 -> the value itself; two: both on the chord, argmax 0 -> the smaller one,
    # below the 80th percentile -> no success -> the maximum; three: the middle one is the elbow, below the percentile -> the maximum
    assert thr.tolist() == [0.0, 7.0, 9.0, 30.0] and not remove.any()


def test_negative_or_nan_predef_thr_is_refused():
    """The C ABI spells "no predefined threshold" as a negative value: a caller's negative or NaN threshold must not select the elbow
    rule silently (the reference would apply it as given).  The check comes before any device work."""
    from satba.engine_hip import HipEngine, check_predef_thr

    p = CO.layout_params("bulk")
    err = np.zeros(p.n_obs)
    for bad in (-1.0, -1e-300, float("nan"), -np.inf, np.float64("nan")):
        with pytest.raises(ValueError):
            ba_outliers.compute_obs_mask(err, p, predef_thr=bad)
        with pytest.raises(ValueError):
            ba_outliers.compute_obs_to_remove(err, p, predef_thr=bad)
        with pytest.raises(ValueError):
            ba_outliers.rm_outliers(err, p, predef_thr=bad)
        with pytest.raises(ValueError):
            HipEngine.outliers(None, err, predef_thr=bad)  # (raises before it touches the handle)
    for good in (None, 0.0, 1e-3, 3.14159, np.inf):
        check_predef_thr(good)


# ------------------------------------------------------------------------------------------------------------------ rm_outliers
@pytest.mark.parametrize("name", list(CO.RM_CASES))
def test_rm_outliers_golden_is_consistent_with_the_oracle(name):
    """
    tests/golden/rm_outliers.npz (the reference's own rm_outliers) restated on the CPU: `rule` on the stored errors gives the stored
    thresholds and, with the host's track filters, the stored observation lists, pts_prev_indices and n_pts_fix; and the CPU oracle's
    init_pts3d on the surviving observations stays within the criterion the GPU test applies to the device's (at most 4 float32 ulp,
    at most 0.5 % of the entries different) -- the condition on the scene that criterion needs.
    """
    from oracle import triangulate_oracle as T

    g = cases.golden("rm_outliers")
    g = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "/")}
    scene, d, kw = CO.rm_case(name)
    from satba import synth

    p = synth.make_params(scene, d, dense=True)
    thr, remove = CO.rule(g["err"], p.cam_ind, p.n_cam, kw.get("predef_thr"), kw.get("min_thr", 1.0))
    assert np.array_equal(thr, g["cam_thr"]) and int(remove.sum()) == int(g["n_detected"])
    assert bool(g["same_object"]) == (remove.sum() == 0) == (name == "clean")
    if name == "clean":
        assert np.array_equal(g["pts_ind"], p.pts_ind) and np.array_equal(g["pts2d"], p.pts2d)
        return
    assert 0.03 * p.n_obs < remove.sum() < 0.15 * p.n_obs
    keep = ~remove
    ok = ba_outliers._surviving_tracks(p.pts_ind[keep], p.cam_ind[keep], p.n_pts, p.n_cam, p.pairs_to_triangulate)
    left = np.nonzero(ok)[0]
    assert np.array_equal(left, g["pts_prev_indices"]) and left.size < p.n_pts
    assert int(g["n_pts_fix"]) == int(np.sum(left < p.n_pts_fix))
    two = np.bincount(p.pts_ind[keep], minlength=p.n_pts) >= 2
    if name == "affine":  # fixed points go too, and tracks are dropped for lack of a listed pair, not only for lack of observations
        assert int(g["n_pts_fix"]) == p.n_pts_fix - 2 and np.sum(two & ~ok) > 0
        assert any(a > b for a, b in p.pairs_to_triangulate)
    new_index = np.full(p.n_pts, -1)
    new_index[left] = np.arange(left.size)
    sel = ok[p.pts_ind] & keep
    assert np.array_equal(g["pts_ind"], new_index[p.pts_ind[sel]]) and np.array_equal(g["cam_ind"], p.cam_ind[sel])
    assert np.array_equal(g["pts2d"], p.pts2d[sel])
    C_left = np.full((2 * p.n_cam, left.size), np.nan)
    C_left[2 * g["cam_ind"], g["pts_ind"]] = g["pts2d"][:, 0]
    C_left[2 * g["cam_ind"] + 1, g["pts_ind"]] = g["pts2d"][:, 1]
    pts = T.init_pts3d(C_left, scene.cameras, scene.cam_model, p.pairs_to_triangulate)
    n_fix = int(g["n_pts_fix"])
    assert np.array_equal(g["pts3d"][:n_fix], np.asarray(p.pts3d)[left[:n_fix]]) and g["pts3d"].dtype == np.float32
    a = pts[n_fix:].view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(g["pts3d"][n_fix:]).view(np.int32).astype(np.int64)
    assert np.abs(a - b).max() <= 4 and np.mean(a != b) <= 0.005

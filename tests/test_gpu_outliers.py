"""
The outlier rejection on the device (satba_outliers: the k_out_* kernels of csrc/satba_outliers.h, satba/ba_outliers.py) at its edges,
against `rule` -- the numpy restatement of ref:bundle_adjust/ba_outliers.py:112-155 in tests/cases_outliers.py, which
tests/test_outliers_cases_host.py pins on vectors of the reference's own function -- and rm_outliers against the reference's own
(tests/golden/rm_outliers.npz).

Every comparison of thresholds, masks, counts and index lists is exact (np.array_equal): the contract is bit-equal thresholds and an
index-exact removed set.  The only tolerance is the one tests/test_gpu_triangulate.py applies to re-triangulated float32 points.
"""
import ctypes

import numpy as np
import pytest

import cases
import cases_outliers as CO
from satba import ba_core, ba_outliers, synth
from satba.engine_hip import HipEngine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def layouts(gpu):
    """Per layout: the object built from the observation lists, the one built through the dense matrix, and an engine of the first."""
    out = {}
    for lay in CO.LAYOUTS:
        p, p_dense = CO.layout_params(lay), CO.layout_params(lay, dense=True)
        assert np.array_equal(p.pts_ind, p_dense.pts_ind) and np.array_equal(p.cam_ind, p_dense.cam_ind)
        out[lay] = (p, p_dense, ba_core.get_engine(p))
    yield out
    for p, p_dense, eng in out.values():
        for q in (p, p_dense):
            for e in q.__dict__.get(ba_core._ENGINE_ATTR, {}).values():
                e.close()


def _check_all_routes(layouts, lay, err, predef_thr, min_thr, tag):
    p, p_dense, eng = layouts[lay]
    thr, remove = CO.rule(err, p.cam_ind, p.n_cam, predef_thr, min_thr)
    got_thr, got_rm, got_n = eng.outliers(err, predef_thr=predef_thr, min_thr=min_thr)
    assert np.array_equal(got_thr, thr), (tag, "engine.outliers", got_thr, thr)
    assert np.array_equal(got_rm, remove) and got_n == int(remove.sum()), (tag, "engine.outliers", got_n, int(remove.sum()))
    rm2, thr2, n2 = ba_outliers.compute_obs_mask(err, p, predef_thr=predef_thr, min_thr=min_thr)
    assert np.array_equal(np.array(thr2), thr) and np.array_equal(rm2, remove) and n2 == int(remove.sum()), (tag, "compute_obs_mask")
    C_new, thr3, n3 = ba_outliers.compute_obs_to_remove(err, p_dense, predef_thr=predef_thr, min_thr=min_thr)
    assert np.array_equal(np.array(thr3), thr) and n3 == int(remove.sum()), (tag, "compute_obs_to_remove")
    assert np.array_equal(np.isnan(C_new[2 * p.cam_ind, p.pts_ind]), remove) and np.array_equal(np.isnan(C_new[2 * p.cam_ind + 1, p.pts_ind]), remove)
    assert int(np.isnan(C_new[::2]).sum() - np.isnan(p_dense.C[::2]).sum()) == n3  # nothing else was blanked
    return thr, remove


@pytest.mark.parametrize("pattern", CO.PATTERNS)
@pytest.mark.parametrize("lay", list(CO.LAYOUTS))
def test_errors_handed_in(layouts, lay, pattern):
    """Every pattern on both layouts at min_thr 0.0 / 1.0 / 2.75, through engine.outliers, compute_obs_mask and compute_obs_to_remove:
    thresholds, mask and count equal `rule`'s.  plateau: only the reference's sequence of roundings finds the index; equal: the first
    of 70 001 tied maxima; edges: segments of 0, 1, 2, 3 and around 256 / 512 / 1024 values, and one of 70 001 for the segmented sort."""
    err = CO.layout_errors(lay, pattern)
    removed = []
    for min_thr in CO.MIN_THRS:
        thr, remove = _check_all_routes(layouts, lay, err, None, min_thr, (lay, pattern, min_thr))
        removed.append(int(remove.sum()))
    if pattern.startswith("equal"):
        assert removed == [0, 0, 0]  # the threshold is max(value, min_thr): an error equal to it stays
    if pattern == "min_thr":
        assert removed[0] > removed[1] > removed[2] > 0  # each min_thr binds


@pytest.mark.parametrize("lay", list(CO.LAYOUTS))
def test_predefined_thresholds(layouts, lay):
    """np.round(predef_thr, 2) for thresholds whose hundredfold lies on or next to a half (2.675 -> 2.68, 0.125 -> 0.12,
    1e6 + 0.005 -> 1e6), one that rounds to 0.0, and the one the existing golden uses."""
    err = CO.layout_errors(lay, "random")
    want = {3.14159: 3.14, 2.675: 2.68, 0.125: 0.12, 1e-3: 0.0, 1e6 + 0.005: 1e6}
    for t in CO.PREDEF_THRS:
        thr, remove = _check_all_routes(layouts, lay, err, t, 1.0, (lay, "predef", t))
        assert np.all(thr == want[t])
    assert remove.sum() == 0 and want[1e-3] == 0.0
    # an error equal to the rounded threshold stays, the next double goes
    p = layouts[lay][0]
    err2 = err.copy()
    k = np.nonzero(p.cam_ind == 5)[0][:2]
    err2[k] = [2.68, np.nextafter(2.68, np.inf)]
    thr, remove = _check_all_routes(layouts, lay, err2, 2.675, 1.0, (lay, "predef", "tie"))
    assert not remove[k[0]] and remove[k[1]]


def test_negative_or_nan_threshold_is_an_error(layouts):
    """Python refuses a negative or NaN predef_thr (the C ABI would read it as "none"); the C entry point itself refuses NaN, which is
    neither "sort and take the elbow" nor "skip the elbow"."""
    p, _, eng = layouts["bulk"]
    err = CO.layout_errors("bulk", "random")
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            eng.outliers(err, predef_thr=bad)
        with pytest.raises(ValueError):
            ba_outliers.compute_obs_mask(err, p, predef_thr=bad)
    thr = np.empty(p.n_cam)
    rm = np.zeros(p.n_obs, dtype=np.uint8)
    n = ctypes.c_int64()
    dp = ctypes.POINTER(ctypes.c_double)
    for predef, min_thr in ((float("nan"), 1.0), (-1.0, float("nan"))):
        rc = eng.lib.satba_outliers(eng._h, err.ctypes.data_as(dp), predef, min_thr, thr.ctypes.data_as(dp),
                                    rm.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(n))
        assert rc != 0 and b"NaN" in eng.lib.satba_last_error()


def test_two_calls_on_one_handle_are_bit_identical(layouts):
    for lay in CO.LAYOUTS:
        eng = layouts[lay][2]
        for pattern in ("plateau", "random"):
            err = CO.layout_errors(lay, pattern)
            a, b = eng.outliers(err, min_thr=0.0), eng.outliers(err, min_thr=0.0)
            assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ------------------------------------------------------------------------------------------------------- errors from the device
DEVICE_CASES = {
    "affine_weighted": ("affine", 8, 900, 5, {"correction_params": ["R"], "n_cam_fix": 2, "ref_cam_weight": 3.0}, {}),
    "perspective_RT": ("perspective", 6, 700, 4, {"correction_params": ["R", "T"], "n_cam_fix": 1}, {}),
    "rpc_R": ("rpc", 4, 400, 4, {"correction_params": ["R"], "n_cam_fix": 1}, {"sigma_theta": 5e-6}),
}


def _device_case(name):
    model, M, N, opp, d, kw = DEVICE_CASES[name]
    scene = synth.make_scene(model, M, N, opp, seed=17, **kw)
    rng = np.random.default_rng(29)
    bad = rng.random(scene.n_obs) < 0.05
    scene.pts2d = scene.pts2d.copy()
    scene.pts2d[bad] += rng.normal(0.0, 25.0, (int(bad.sum()), 2))
    return scene, (lambda: synth.make_params(scene, dict(d, reduce=False))), bad


@pytest.mark.parametrize("loss", ["linear", "soft_l1"])
@pytest.mark.parametrize("name", list(DEVICE_CASES))
def test_errors_from_the_device(gpu, name, loss):
    """err = None: engine.outliers() = rule(engine.reprojection_errors()) = rule(compute_reprojection_error(fun(x), pts2d_w)), with
    weighted observations, on the three camera models, and whatever loss the handle is configured for -- which stays in force."""
    scene, make_p, bad = _device_case(name)
    p = make_p()
    if "ref_cam_weight" in DEVICE_CASES[name][4]:
        assert np.sum(p.pts2d_w == 3.0) > 0 and np.sum(p.pts2d_w == 1.0) > 0
    x = ba_core._frozen_vars(p.params_opt.copy(), p)
    err_host = ba_core.compute_reprojection_error(ba_core.fun(x.copy(), p), p.pts2d_w)  # (the cached engine of p, linear)
    eng = HipEngine(p)
    try:
        eng.configure(loss, 1.0)
        eng.set_x(x)
        _, cost_before = eng.residuals(with_cost=True)
        err_dev = eng.reprojection_errors()
        assert np.array_equal(err_dev, err_host)
        for min_thr in (1.0, 0.0):
            thr, remove = CO.rule(err_dev, p.cam_ind, p.n_cam, None, min_thr)
            got = eng.outliers(min_thr=min_thr)
            assert np.array_equal(got[0], thr) and np.array_equal(got[1], remove) and got[2] == int(remove.sum())
        assert remove[bad].mean() > 0.6 and 0 < remove.sum() < 0.3 * p.n_obs  # the injected errors are what goes
        got = eng.outliers(predef_thr=2.675)
        thr, remove = CO.rule(err_dev, p.cam_ind, p.n_cam, 2.675, 1.0)
        assert np.array_equal(got[0], thr) and np.array_equal(got[1], remove) and got[2] == int(remove.sum())
        _, cost_after = eng.residuals(with_cost=True)
        assert cost_after == cost_before
        eng.configure("linear", 1.0)
        _, cost_linear = eng.residuals(with_cost=True)
        assert (cost_linear == cost_before) == (loss == "linear")  # the gross errors make soft_l1 a different number
    finally:
        eng.close()


@pytest.mark.parametrize("loss", ["linear", "soft_l1"])
def test_the_handle_solves_as_if_the_call_had_not_happened(gpu, loss):
    """solve_lm after outliers() (errors from the device, and errors handed in) returns the bits a fresh handle returns."""
    _, make_p, _, _ = cases.solve_case("affine_small_R")
    runs = []
    for call in (False, True):
        p = make_p()
        eng = HipEngine(p)
        try:
            eng.configure(loss, 1.0)
            eng.set_x(p.params_opt.copy())
            if call:
                a = eng.outliers()
                b = eng.outliers(eng.reprojection_errors(), min_thr=0.0)
                assert a[2] >= 0 and b[2] >= a[2]
            st = eng.solve_lm(max_nfev=12, loss=loss)
            runs.append(((st.cost, st.initial_cost, st.optimality, st.nfev, st.njev, st.iterations, st.status), eng.get_x()))
            if call:  # ... and the call after a solve sees the solve's end point
                e = eng.reprojection_errors()
                thr, remove = CO.rule(e, p.cam_ind, p.n_cam, None, 1.0)
                got = eng.outliers()
                assert np.array_equal(got[0], thr) and np.array_equal(got[1], remove)
        finally:
            eng.close()
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])
    assert runs[0][0][3] > 2 and runs[0][0][0] < runs[0][0][1]  # a solve that did something


# ------------------------------------------------------------------------------------------------------------------ rm_outliers
def _close_engines(*objs):
    for q in objs:
        for e in q.__dict__.pop(ba_core._ENGINE_ATTR, {}).values():
            e.close()


def _ulp_diff(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


@pytest.mark.parametrize("route", ["dense", "resident", "upload"])
@pytest.mark.parametrize("name", list(CO.RM_CASES))
def test_rm_outliers_against_the_reference(gpu, name, route, monkeypatch):
    """
    The object rm_outliers returns against the one the reference's own rm_outliers returned for the same errors
    (tests/golden/rm_outliers.npz): observation lists, pts2d, pts_prev_indices and n_pts_fix equal; fixed points keep their
    coordinates bit for bit; the re-triangulated points within the criterion of tests/test_gpu_triangulate.py (at most 4 float32 ulp,
    at most 0.5 % of the entries different: tests/test_outliers_cases_host.py asserts the CPU oracle meets it on these scenes).
    Routes: the dense matrix; the observation lists with a cached engine (the handle's resident tracks where the pair list is written
    i < j -- the affine scene writes one pair reversed and takes the host filter); the observation lists with SATBA_TRI_UPLOAD=1.
    """
    g = cases.golden("rm_outliers")
    g = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "/")}
    scene, d, kw = CO.rm_case(name)
    p = synth.make_params(scene, d, dense=(route == "dense"))
    assert (p.C is not None) == (route == "dense")
    if route == "resident":
        ba_core.get_engine(p)
        assert ba_core.cached_engine(p) is not None
    if route == "upload":
        monkeypatch.setenv("SATBA_TRI_UPLOAD", "1")
    else:
        monkeypatch.delenv("SATBA_TRI_UPLOAD", raising=False)
    new_p = None
    try:
        new_p = ba_outliers.rm_outliers(g["err"], p, **kw)
        if name == "clean":
            assert bool(g["same_object"]) and new_p is p  # nothing detected: the object itself
            return
        assert new_p is not p and (new_p.C is not None) == (route == "dense")
        assert np.array_equal(new_p.pts_ind, g["pts_ind"]) and np.array_equal(new_p.cam_ind, g["cam_ind"])
        assert np.array_equal(new_p.pts2d, g["pts2d"])
        assert np.array_equal(new_p.pts_prev_indices, g["pts_prev_indices"])
        n_fix = int(g["n_pts_fix"])
        assert new_p.n_pts_fix == n_fix and new_p.n_pts == g["pts3d"].shape[0] and new_p.n_obs == g["pts_ind"].size
        assert new_p.n_pts_opt == new_p.n_pts - n_fix and new_p.n_cam_fix == p.n_cam_fix and new_p.ref_cam_weight == p.ref_cam_weight
        pts = np.asarray(new_p.pts3d)
        assert pts.dtype == np.float32 and pts.shape == g["pts3d"].shape
        assert np.array_equal(pts[:n_fix], np.asarray(p.pts3d)[g["pts_prev_indices"][:n_fix]])
        assert np.array_equal(pts[:n_fix], g["pts3d"][:n_fix])
        diff = _ulp_diff(pts[n_fix:], g["pts3d"][n_fix:])
        print(name, route, "re-triangulated entries that differ: {} of {} (max {} ulp)".format(int((diff > 0).sum()), diff.size, int(diff.max())))
        assert diff.max() <= 4, "float32 means differ by {} ulp".format(diff.max())
        assert np.mean(diff > 0) <= 0.005, "{:.2%} of the float32 entries differ".format(np.mean(diff > 0))
        # a second round on the result works, and takes away no more than it holds
        err2 = ba_core.compute_reprojection_error(ba_core.fun(new_p.params_opt.copy(), new_p), new_p.pts2d_w)
        again = ba_outliers.rm_outliers(err2, new_p, **kw)
        thr2, remove2 = CO.rule(err2, new_p.cam_ind, new_p.n_cam, kw.get("predef_thr"), kw.get("min_thr", 1.0))
        assert again.n_obs <= new_p.n_obs - int(remove2.sum()) and again.n_pts <= new_p.n_pts
        assert (again is new_p) == (remove2.sum() == 0)
        if again is not new_p:
            prev = np.asarray(again.pts_prev_indices)
            assert np.all(np.diff(prev) > 0) and np.all(np.isin(prev, np.asarray(new_p.pts_prev_indices)))
            _close_engines(again)
    finally:
        _close_engines(*(q for q in (p, new_p) if q is not None))

"""
RPC re-fit on the device (satba.ba_rpcfit -> satba_rpc_fit / satba_rpc_localization) against the oracle and the vectors of the
reference function (tests/golden/rpcfit.npz).  SURVEY section 8f #4.

Tolerances.  The normal matrices of this fit are ill-conditioned (cond 1e13 - 1e17; for an affine camera the unregularised first
solve is rank deficient in exact arithmetic): replacing numpy.linalg.inv by another correct solver moves the reference's own
fitted projection by 5e-5 px (RPC cases) to 7e-4 px (affine case) and may change the number of re-weighted passes.  What is
asserted is therefore the fitted PROJECTION against the reference's (2e-3 px) and the fit error against the target (same level
as the reference's), not the coefficients.

The margin loop of satba_rpc_refit runs on scenarios with a known number of doublings (tests/cases_rpcfit.py, pinned without a device
by test_rpcfit_cases_host.py); the solve of k_rpc_fit is held against numpy.longdouble through its backward error, which does not
depend on the condition number.  DESIGN.md section 4b lists what is covered and what the MI355X measured.
"""
import functools

import numpy as np
import pytest

import cases
import cases_rpcfit as K
from oracle import rpcfit_oracle as F
from oracle import triangulate_oracle as T
from satba import ba_rpcfit, cam_utils, geo_utils, synth
from satba.rpc_model import RPCModel

pytestmark = pytest.mark.gpu


def _golden():
    import os

    return np.load(os.path.join(cases.GOLDEN, "rpcfit.npz"))


@pytest.mark.parametrize("name", ["rpc0", "rpc1", "affine"])
def test_weighted_lsq_against_reference_vectors(gpu, name):
    g = _golden()
    target, locs = g[name + "_target"], g[name + "_locs"]
    rpc = ba_rpcfit.weighted_lsq(target, locs)
    ref = RPCModel.from_table(g[name + "_table"])
    # offsets and scales are plain extrema: exact
    assert np.array_equal(rpc.to_table()[80:], ref.to_table()[80:])
    assert rpc.col_den[0] == 1.0 and rpc.row_den[0] == 1.0
    p_dev = np.stack(rpc.projection(*locs.T), 1); p_ref = np.stack(ref.projection(*locs.T), 1)
    assert np.abs(p_dev - p_ref).max() < 2e-3
    err = ba_rpcfit.check_errors(rpc, locs, target)
    assert err.max() < 1.05 * g[name + "_err"].max() + 2e-3 and np.median(err) < 1.05 * np.median(g[name + "_err"]) + 1e-3
    # against points the fit has not seen: half-way between the grid nodes, inside the box
    mid = 0.5 * (locs[:-1] + locs[1:])
    assert np.abs(np.stack(rpc.projection(*mid.T), 1) - np.stack(ref.projection(*mid.T), 1)).max() < 2e-3


def test_batch_equals_single_fits(gpu):
    g = _golden()
    t = np.stack([g["rpc0_target"], g["rpc1_target"]]); x = np.stack([g["rpc0_locs"], g["rpc1_locs"]])
    rpcs, info = ba_rpcfit.weighted_lsq_batch(t, x, return_info=True)
    for k in range(2):
        one = ba_rpcfit.weighted_lsq(t[k], x[k])
        assert np.array_equal(one.to_table(), rpcs[k].to_table())
        m, it = F.weighted_lsq(t[k], x[k])
        assert info["iters"][k] == it and abs(info["rmse"][k] - F.rmse_row_col(m, x[k], t[k])) < 1e-3
    with pytest.raises(ValueError):
        ba_rpcfit.weighted_lsq(t[0][:10], x[0][:10])  # fewer samples than unknowns
    flat = x[0].copy(); flat[:, 2] = 100.0  # constant altitude: zero scale, singular normal equations
    with pytest.raises(np.linalg.LinAlgError):
        ba_rpcfit.weighted_lsq(t[0], flat)
    assert ba_rpcfit.weighted_lsq_batch(t[:0], x[:0]) == []
    bad = t[0].copy(); bad[3, 0] = np.nan
    with pytest.raises(ValueError):
        ba_rpcfit.weighted_lsq(bad, x[0])


def test_localization_inverts_the_projection(gpu):
    """image points over the whole image (and a margin) at altitudes over the model's range -> lon / lat -> projection: back on the
    image points; and the same root as the oracle's restatement of the reference's C localisation (ref:c/rpc.c:372-408)."""
    rng = np.random.default_rng(5)
    for path in synth.default_rpc_files():
        r = RPCModel.from_file(path)
        n = 3000
        col = r.col_offset + rng.uniform(-1.02, 1.02, n) * r.col_scale; row = r.row_offset + rng.uniform(-1.02, 1.02, n) * r.row_scale
        alt = r.alt_offset + rng.uniform(-1, 1, n) * r.alt_scale
        lo, la = r.localization(col, row, alt)
        assert np.isfinite(lo).all() and np.isfinite(la).all()
        c2, r2 = r.projection(lo, la, alt)
        assert np.abs(c2 - col).max() < 1e-5 and np.abs(r2 - row).max() < 1e-5  # the iteration stops at 1e-9 of the image scale
        o = T._Rpc(r, 0.1)
        lo2, la2 = o.eval_rpc(col[:300], row[:300], alt[:300])
        assert np.abs(lo[:300] - lo2).max() < 1e-9 and np.abs(la[:300] - la2).max() < 1e-9  # degrees: 0.1 mm on the ground
        assert r.localization(np.zeros((0,)), np.zeros((0,)), np.zeros((0,)))[0].shape == (0,)
        g = r.localization(np.full((2, 3), r.col_offset), np.full((2, 3), r.row_offset), r.alt_offset)  # broadcasting like numpy
        assert g[0].shape == (2, 3) and abs(g[0][0, 0] - r.lon_offset) < 0.05


def test_fit_Rt_corrected_rpc_reproduces_the_corrected_projection(gpu):
    """ref:bundle_adjust/ba_rpcfit.py:270-345 end to end: grid over the image, localisation through the original RPC, corrected
    projection, fit, coverage check.  The fitted RPC must reproduce x = P(R (X - C) + C) on fresh points."""
    from satba import ba_core
    from satba.ba_core import adjust_pts3d

    r = RPCModel.from_file(synth.default_rpc_files()[0])
    crop = {"col0": 0, "row0": 0, "width": int(2 * r.col_scale), "height": int(2 * r.row_scale)}
    lon0, lat0 = r.lon_offset, r.lat_offset
    c = np.array(geo_utils.latlon_to_ecef_custom(lat0, lon0, r.alt_offset))
    C = c + 5e5 * c / np.linalg.norm(c)
    Rt = np.concatenate([[4e-6, -3e-6, 5e-6], np.zeros(3), C]).reshape(1, 9)
    rng = np.random.default_rng(1)
    # ground points under the image (the RPC's lon / lat box is far larger than the footprint)
    alt = r.alt_offset + rng.uniform(-0.5, 0.5, 500) * r.alt_scale
    lo, la = r.localization(rng.uniform(0, crop["width"], 500), rng.uniform(0, crop["height"], 500), alt)
    pts = np.stack(geo_utils.latlon_to_ecef_custom(la, lo, alt), 1)
    rpc, err, margin = ba_rpcfit.fit_Rt_corrected_rpc(Rt, None, r, crop, pts)
    assert margin in (10, 20, 40, 80, 160, 320, 640, 1280) and err.shape == (1000,) and err.max() < 0.5
    want = cam_utils.apply_rpc_projection(r, adjust_pts3d(pts, Rt))
    got = cam_utils.apply_rpc_projection(rpc, pts)
    assert np.abs(got - want).max() < 0.05  # pixels; the correction itself moves the points by tens of pixels
    assert np.abs(cam_utils.apply_rpc_projection(r, pts) - want).max() > 1.0
    # several cameras in one launch: the same models as one by one
    r1 = RPCModel.from_file(synth.default_rpc_files()[1])
    crop1 = {"col0": 0, "row0": 0, "width": int(2 * r1.col_scale), "height": int(2 * r1.row_scale)}
    # several cameras at once, device resident (satba_rpc_refit: mesh, localisation, corrected projection, fit, errors and coverage
    # test on the device): the same margins, the same mesh, and -- the fit is ill-conditioned, so its coefficients
    # answer to the last bits of the samples -- the same PROJECTION as the host-driven route camera by camera
    Rt1 = Rt * np.r_[2.0 * np.ones(3), np.ones(6)]
    many, info = ba_rpcfit.fit_Rt_corrected_rpcs([Rt, Rt1], None, [r, r1], [crop, crop1], return_info=True)
    one = ba_rpcfit.fit_Rt_corrected_rpc(Rt1, None, r1, crop1, pts)
    for (rpc_d, err_d, margin_d), (rpc_h, err_h, margin_h), rr, RT, k in ((many[0], (rpc, err, margin), r, Rt, 0), (many[1], one, r1, Rt1, 1)):
        assert margin_d == margin_h and err_d.shape == err_h.shape
        locs_d, target_d = info["input_locs"][k], info["target"][k]
        cr = crop if k == 0 else crop1
        cols, rows, alts = cam_utils.generate_point_mesh([-margin_h, cr["width"] + margin_h, 10], [-margin_h, cr["height"] + margin_h, 10],
                                                         [rr.alt_offset - rr.alt_scale, rr.alt_offset + rr.alt_scale, 10])
        assert np.abs(locs_d[:, 2] - alts).max() == 0.0  # numpy.linspace's arithmetic
        lon_h, lat_h = rr.localization(cols, rows, alts)
        assert np.abs(locs_d[:, 0] - lon_h).max() < 1e-11 and np.abs(locs_d[:, 1] - lat_h).max() < 1e-11
        X = np.stack(geo_utils.latlon_to_ecef_custom(lat_h, lon_h, alts), 1)
        assert np.abs(target_d - cam_utils.apply_rpc_projection(rr, ba_core.adjust_pts3d(X, RT))).max() < 1e-6
        assert np.abs(np.stack(rpc_d.projection(*locs_d.T), 1) - np.stack(rpc_h.projection(*locs_d.T), 1)).max() < 2e-3
        assert np.abs(err_d - err_h).max() < 2e-3 and np.abs(err_d - ba_rpcfit.check_errors(rpc_d, locs_d, target_d)).max() < 1e-9
    # the affine route (ba_rpcfit.py:201-267): an RPC copying a projection matrix that maps into a crop at (col0, row0)
    scene = synth.make_scene("affine", 2, 300, 2, seed=3)
    P = np.asarray(scene.cameras[0], dtype=np.float64).copy()
    X = scene.pts3d_true
    proj = cam_utils.apply_projection_matrix(P, X)
    P[0] -= proj[:, 0].min() * P[2]; P[1] -= proj[:, 1].min() * P[2]  # crop coordinates start at (0, 0)
    proj = cam_utils.apply_projection_matrix(P, X)
    crop = {"col0": 120, "row0": 75, "width": int(np.ceil(proj[:, 0].max())), "height": int(np.ceil(proj[:, 1].max()))}
    shift = np.array([crop["col0"], crop["row0"]], dtype=np.float64)
    la, lo, al = geo_utils.ecef_to_latlon_custom(*X.T)
    # the "original" RPC of that image, needed to localise the grid: fitted on a box around the scene
    glon, glat, galt = [v.reshape(-1) for v in np.meshgrid(np.linspace(lo.min() - 0.01, lo.max() + 0.01, 8), np.linspace(la.min() - 0.01, la.max() + 0.01, 8),
                                                           np.linspace(al.min() - 9000, al.max() + 9000, 8), indexing="ij")]
    G = np.stack(geo_utils.latlon_to_ecef_custom(glat, glon, galt), 1)
    base = ba_rpcfit.weighted_lsq(cam_utils.apply_projection_matrix(P, G) + shift, np.stack([glon, glat, galt], 1))
    rpc2, err2, margin2 = ba_rpcfit.fit_rpc_from_projection_matrix(P, None, base, crop, X, n_samples=8)
    assert err2.shape == (512,) and err2.max() < 0.05 and margin2 >= 10  # the regularised fit (h = 1e-3) leaves ~1e-2 px on this box
    assert np.abs(cam_utils.apply_rpc_projection(rpc2, X) - (proj + shift)).max() < 0.05


def test_rpc_pipeline_from_tracks_to_refitted_rpcs(gpu, tmp_path):
    """The reference's main use (tests/config1.json: cam_model "rpc") through the drop-in names, ref:bundle_adjust/ba_pipeline.py:700-728
    minus feature tracking: triangulate the tracks -> BundleAdjustmentParameters -> soft L1 -> outlier rejection (re-triangulates) ->
    L2 -> reconstruct_vars -> re-fit one RPC per camera -> write / read .rpc_adj.  The re-fitted RPCs, applied to the adjusted points
    with no correction, must explain the observations as well as the corrected cameras do."""
    from satba import ba_core, ba_outliers, ba_params, ft_triangulate, loader

    M = 4
    scene = synth.make_scene("rpc", M, 1200, 4, seed=12, sigma_theta=5e-6)
    rng = np.random.default_rng(2)
    bad = rng.random(scene.n_obs) < 0.02
    scene.pts2d[bad] += rng.normal(0, 25.0, (int(bad.sum()), 2))
    C = scene.to_dense_C()
    pairs = [(i, j) for i in range(M) for j in range(i + 1, M) if (i + j) % 2 == 1]  # the two shipped models alternate
    pts0 = ft_triangulate.init_pts3d(C, scene.cameras, "rpc", pairs)
    keep = np.abs(pts0).max(axis=1) > 0  # tracks seen only by same-model cameras have no pair
    C, pts0 = C[:, keep], pts0[keep]
    d = {"n_cam_fix": 0, "n_pts_fix": 0, "ref_cam_weight": 1.0, "correction_params": ["R"], "verbose": False}
    p = ba_params.BundleAdjustmentParameters(C, pts0, scene.cameras, "rpc", pairs, scene.camera_centers, d)
    _, sol, e0, e1, _ = ba_core.run_ba_optimization(p, {"loss": "soft_l1", "f_scale": 1.0, "max_iter": 300, "verbose": 0}, False, False)
    p.reconstruct_vars(sol, pts0, scene.cameras)
    n_before = p.n_obs
    p = ba_outliers.rm_outliers(e1, p, verbose=False)
    assert 0.3 * bad[np.isin(scene.pts_ind, np.nonzero(keep)[0])].sum() < n_before - p.n_obs
    _, sol, e2, e3, _ = ba_core.run_ba_optimization(p, None, False, False)
    pts_ba, cams_ba = p.reconstruct_vars(sol, np.asarray(pts0, dtype=np.float64), list(scene.cameras))
    assert e3.mean() < 0.5 and e3.mean() < 0.2 * e0.mean()
    crops = [{"col0": 0, "row0": 0, "width": int(2 * r.col_scale), "height": int(2 * r.row_scale)} for r in scene.cameras]
    fits = ba_rpcfit.fit_Rt_corrected_rpcs([np.asarray(c).reshape(1, 9) for c in cams_ba], None, scene.cameras, crops)
    names = [str(tmp_path / "rpcs_adj" / "im{}.rpc_adj".format(k)) for k in range(M)]
    loader.save_rpcs(names, [f[0] for f in fits])
    loader.write_point_cloud_ply(str(tmp_path / "pts3d_adj.ply"), p.pts3d_ba)
    loader.save_estimated_params(str(tmp_path), ["im{}".format(k) for k in range(M)], p.estimated_params)
    new_rpcs = [RPCModel.from_file(fn) for fn in names]
    # the observations through the re-fitted models, no correction any more
    err_new = np.zeros(p.n_obs)
    for k in range(M):
        sel = p.cam_ind == k
        proj = cam_utils.apply_rpc_projection(new_rpcs[k], p.pts3d_ba[p.pts_ind[sel]])
        err_new[sel] = np.linalg.norm(proj - p.pts2d[sel], axis=1)
        assert fits[k][1].max() < 0.05
    assert abs(err_new.mean() - e3.mean()) < 0.02, (err_new.mean(), e3.mean())
    assert np.abs(loader.read_point_cloud_ply(str(tmp_path / "pts3d_adj.ply")) - p.pts3d_ba).max() < 1e-6


# ------------------------------------------------------------------------------ the margin loop of satba_rpc_refit (cases_rpcfit.py)
# Scenarios whose number of doublings is known from the CPU oracle (test_rpcfit_cases_host.py pins every margin below and that, in
# every round, the worst crop corner is >= 1 px away from the hull: two correct fits differ by <= 2e-3 px, so they decide alike).
@functools.lru_cache(maxsize=None)
def _refit(keys, n_samples=10):
    """one fit_Rt_corrected_rpcs call over the scenarios `keys` (they share one global transform); computed once, read-only"""
    sc = [K.scenario(k) for k in keys]
    assert all((s[3] is None) == (sc[0][3] is None) for s in sc)
    out, info = ba_rpcfit.fit_Rt_corrected_rpcs([s[1] for s in sc], sc[0][3], [s[0] for s in sc], [s[2] for s in sc], n_samples=n_samples,
                                                return_info=True)
    for a in [o[1] for o in out] + list(info.values()):
        a.setflags(write=False)
    return out, info


def _margin_of(key):
    return K.CROPPED[key] if len(key) > 3 else K.FULL_IMAGE[key]


_BATCHES = {"none": tuple(K.BATCH_NONE), "gt": tuple(K.BATCH_GT)}


@pytest.mark.parametrize("tag", ["none", "gt"])
def test_margin_loop_ends_at_the_oracles_margins(gpu, tag):
    """One call over cameras whose margins end at 10 ... 640 and one that is never covered: later rounds hold scattered slots (round
    2 of the first batch: {0, 2, 3, 5}, round 4: {0, 2, 5}), so the coverage test, the compaction to the front of the device list,
    the launches per run of consecutive slots and the give-up above 1000 all decide the result."""
    out, info = _refit(_BATCHES[tag])
    assert [o[2] for o in out] == [K.FULL_IMAGE[k] for k in _BATCHES[tag]]
    assert K.GIVE_UP in [o[2] for o in out]
    for (rpc, err, margin), k in zip(out, range(len(out))):
        assert err.shape == (1000,) and np.isfinite(rpc.to_table()).all()
        assert np.abs(err - ba_rpcfit.check_errors(rpc, info["input_locs"][k], info["target"][k])).max() < 1e-9  # no stale err or table


@pytest.mark.parametrize("tag", ["none", "gt"])
def test_every_camera_of_the_batch_equals_the_camera_alone(gpu, tag):
    """Nothing in these kernels depends on the other workgroups of a launch or on arrival order: table, err, margin, mesh and target
    of every camera are those of the same camera run alone, bit for bit."""
    keys = _BATCHES[tag]
    out, info = _refit(keys)
    for k, key in enumerate(keys):
        out1, info1 = _refit((key,))
        rpc1, err1, margin1 = out1[0]
        assert out[k][2] == margin1, key
        assert np.array_equal(out[k][0].to_table(), rpc1.to_table()), key
        assert np.array_equal(out[k][1], err1), key
        assert np.array_equal(info["input_locs"][k], info1["input_locs"][0]) and np.array_equal(info["target"][k], info1["target"][0]), key


_SCENARIO_IDS = dict(ids=lambda k: "file{}-s{}-{}{}".format(k[0], k[1], k[2], "-crop" if len(k) > 3 else ""))


@functools.lru_cache(maxsize=None)
def _host_route(key):
    """fit_Rt_corrected_rpc (numpy mesh, one localisation and one fit launch per round, scipy's hull) on a scenario"""
    r, Rt, crop, gt = K.scenario(key)
    lo, la = r.localization(np.array([crop["col0"] + 0.5 * crop["width"]]), np.array([crop["row0"] + 0.5 * crop["height"]]), np.array([r.alt_offset]))
    pts = np.stack(geo_utils.latlon_to_ecef_custom(la, lo, np.array([r.alt_offset])), 1) + (gt if gt is not None else 0.0)
    return ba_rpcfit.fit_Rt_corrected_rpc(Rt, gt, r, crop, pts)


@pytest.mark.parametrize("key", list(K.FULL_IMAGE) + list(K.CROPPED), **_SCENARIO_IDS)
def test_device_route_equals_host_driven_route(gpu, key):
    """satba_rpc_refit against the host-driven fit_Rt_corrected_rpc with the same global transform and crop offset: the same margin
    (the oracle's), the same mesh, and err is the error of the returned model on the returned mesh."""
    r, Rt, crop, gt = K.scenario(key)
    out, info = _refit((key,))
    rpc_d, err_d, margin_d = out[0]
    locs_d, target_d = info["input_locs"][0], info["target"][0]
    rpc_h, err_h, margin_h = _host_route(key)
    assert margin_d == margin_h == _margin_of(key)
    cols, rows, alts = cam_utils.generate_point_mesh([crop["col0"] - margin_h, crop["col0"] + crop["width"] + margin_h, 10],
                                                     [crop["row0"] - margin_h, crop["row0"] + crop["height"] + margin_h, 10],
                                                     [r.alt_offset - r.alt_scale, r.alt_offset + r.alt_scale, 10])
    assert np.array_equal(locs_d[:, 2], alts)
    lon_h, lat_h = r.localization(cols, rows, alts)
    assert np.abs(locs_d[:, 0] - lon_h).max() < 1e-11 and np.abs(locs_d[:, 1] - lat_h).max() < 1e-11
    assert err_d.shape == err_h.shape
    assert np.abs(err_d - ba_rpcfit.check_errors(rpc_d, locs_d, target_d)).max() < 1e-9


@pytest.mark.parametrize("key", list(K.FULL_IMAGE) + list(K.CROPPED), **_SCENARIO_IDS)
def test_device_route_projection_equals_host_driven_route(gpu, key):
    """
    The fitted projection and err of the two routes on the mesh, within the 2e-3 px this file uses between two correct fits.

    This test found a defect.  Both routes run the same k_rpc_fit on the same mesh, bit for bit; their targets differ by 3.5e-9 px
    (the corrected projection in the kernel against numpy's).  With the reference's stopping rule taken literally -- the first
    re-weighted pass is compared with the unweighted solve -- the kernel, whose unweighted solve is accurate (RMSE ~1e-4 px at once),
    stopped after ONE re-weighted pass in 19 of the 22 scenarios.  That pass is weighted by the denominators of the unregularised
    solve, rounding noise in the near-null space of the normal matrix: the routes differed by 2.8e-3 px (file 0, s = 10) and 4.9e-3 px
    (file 1, s = 40), the fit error was up to 4 x the oracle's (4.4e-3 against 1.0e-3 px) and the model up to 3.7e-3 px away from the
    oracle's, which runs 2 - 3 passes on every one of these inputs because numpy.linalg.inv leaves its first model's RMSE far above
    tol.  Since k_rpc_fit judges convergence between two re-weighted passes, measured on an MI355X over the 22 scenarios: routes
    1.7e-8 - 1.1e-5 px apart, fit error equal to the oracle's to 2 digits, model within 3.2e-4 px of the oracle's.
    """
    out, info = _refit((key,))
    rpc_d, err_d, margin_d = out[0]
    locs_d = info["input_locs"][0]
    rpc_h, err_h, margin_h = _host_route(key)
    assert margin_d == margin_h
    d = np.abs(np.stack(rpc_d.projection(*locs_d.T), 1) - np.stack(rpc_h.projection(*locs_d.T), 1)).max()
    print("routes {}: projection {:.2e} px, err {:.2e} px".format(key, d, np.abs(err_d - err_h).max()))
    assert d < 2e-3
    assert np.abs(err_d - err_h).max() < 2e-3


def test_target_under_a_global_transform(gpu):
    """k_refit_grid adds the global transform before the corrected projection; the coverage test projects the mesh without it (the
    margins of the gt batch, which differ from those of the same cameras without it, say so: file 0, s = 10 ends at 20, not 40)."""
    from satba.ba_core import adjust_pts3d

    keys = _BATCHES["gt"]
    out, info = _refit(keys)
    for k, key in enumerate(keys):
        r, Rt, crop, gt = K.scenario(key)
        locs = info["input_locs"][k]
        X = np.stack(geo_utils.latlon_to_ecef_custom(locs[:, 1], locs[:, 0], locs[:, 2]), 1)
        assert np.abs(info["target"][k] - cam_utils.apply_rpc_projection(r, adjust_pts3d(X + gt, Rt))).max() < 1e-6
        assert np.abs(info["target"][k] - cam_utils.apply_rpc_projection(r, adjust_pts3d(X, Rt))).max() > 1.0
    assert K.FULL_IMAGE[(0, 10, "gt")] != K.FULL_IMAGE[(0, 10, None)] and K.FULL_IMAGE[(0, 1, "gt")] != K.FULL_IMAGE[(0, 1, None)]


@pytest.mark.parametrize("n", K.MESH_N)
def test_mesh_sizes(gpu, n):
    """n_samples 16 and 15: the hull's points take more than 48 KB of dynamic LDS (64 KB at 16, beside the static arrays); 4: the
    lower bound, 64 samples, one staging tile of the fit (the oracle's fit is regular there).  One camera doubles once."""
    keys = tuple(K.MESH_BATCH)
    out, info = _refit(keys, n)
    assert [o[2] for o in out] == [K.MESH_MARGINS[k] for k in keys] and out[0][2] > 10
    for k, key in enumerate(keys):
        r, Rt, crop, gt = K.scenario(key)
        rpc, err, margin = out[k]
        locs, target = info["input_locs"][k], info["target"][k]
        assert err.shape == (n ** 3,) and locs.shape == (n ** 3, 3) and target.shape == (n ** 3, 2)
        assert np.array_equal(locs[:, 2], np.repeat(np.linspace(r.alt_offset - r.alt_scale, r.alt_offset + r.alt_scale, n), n * n))
        cols, rows, alts = cam_utils.generate_point_mesh([-margin, crop["width"] + margin, n], [-margin, crop["height"] + margin, n],
                                                         [r.alt_offset - r.alt_scale, r.alt_offset + r.alt_scale, n])
        lon_h, lat_h = r.localization(cols, rows, alts)
        assert np.abs(locs[:, 0] - lon_h).max() < 1e-11 and np.abs(locs[:, 1] - lat_h).max() < 1e-11
        assert np.abs(err - ba_rpcfit.check_errors(rpc, locs, target)).max() < 1e-9


@pytest.mark.parametrize("n", [3, K.REFIT_MAX_N + 1])
def test_mesh_sizes_out_of_range_raise_and_leave_the_outputs(gpu, n):
    from satba import engine_hip as E

    keys = K.MESH_BATCH
    sc = [K.scenario(k) for k in keys]
    with pytest.raises(ValueError):
        ba_rpcfit.fit_Rt_corrected_rpcs([s[1] for s in sc], None, [s[0] for s in sc], [s[2] for s in sc], n_samples=n)
    lib = E.load_library()
    M, n3 = len(sc), n ** 3
    tabs = np.ascontiguousarray(np.stack([s[0].to_table() for s in sc])); rt = np.ascontiguousarray(np.stack([s[1].reshape(9) for s in sc]))
    crops = np.array([[s[2]["col0"], s[2]["row0"], s[2]["width"], s[2]["height"]] for s in sc], dtype=np.float64)
    alts = np.array([[s[0].alt_offset - s[0].alt_scale, s[0].alt_offset + s[0].alt_scale] for s in sc], dtype=np.float64)
    outs = [np.full(shape, -7.25) for shape in ((M, 90), (M, n3), (M,), (M, n3, 3), (M, n3, 2))]
    rc = lib.satba_rpc_refit(M, E._ptr(tabs), E._ptr(rt), E._ptr(crops), E._ptr(alts), None, n, 1e-3, 1e-2, 20, *[E._ptr(o) for o in outs], 0)
    assert rc == -1  # SATBA_E_ARG
    assert all((o == -7.25).all() for o in outs)


# ------------------------------------------------------------------------------ k_rpc_fit against extended precision
def _eta_rows(name):
    """per (n, axis, pass): eta of the device's solve and of numpy.linalg.solve on the same normal equations, in longdouble"""
    g = _golden()
    rows = []
    for n in K.EDGE_N:
        t, x = K.subset(g, name, n)
        r0, i0 = ba_rpcfit.weighted_lsq_batch(t[None], x[None], max_iter=0, return_info=True)
        r1, i1 = ba_rpcfit.weighted_lsq_batch(t[None], x[None], max_iter=1, return_info=True)
        assert i0["iters"][0] == 0 and i1["iters"][0] == 1
        tab0, tab1 = r0[0].to_table(), r1[0].to_table()
        want = K.scaling_table(t, x)
        assert np.array_equal(tab0[80:], want[80:]) and np.array_equal(tab1[80:], want[80:])  # plain extrema: exact at every n
        assert tab0[20] == 1.0 and tab0[60] == 1.0 and tab1[20] == 1.0 and tab1[60] == 1.0
        for a, (M, b) in enumerate(K.design_matrices(t, x, want)):
            x0, x1 = K.unknowns(tab0, a), K.unknowns(tab1, a)
            w = K.weights(M, x0)  # the weights of the kernel's pass 1: its pass 0 is the max_iter = 0 call (runs repeat bitwise)
            rows.append((len(t), a, 0, K.backward_error(M, b, x0), K.backward_error(M, b, K.solve_float64(M, b))))
            rows.append((len(t), a, 1, K.backward_error(M, b, x1, w, 1e-3), K.backward_error(M, b, K.solve_float64(M, b, w, 1e-3), w, 1e-3)))
    return rows


@pytest.mark.parametrize("name", K.GOLDEN_FITS)
def test_fit_backward_error_at_the_sample_count_edges(gpu, name):
    """
    The unweighted solve (max_iter = 0) and the first re-weighted one (max_iter = 1, weights 1 / den^2 of the first, + h^2 I) on
    seeded subsets of n = 39 (the unknowns), 40, 63 / 64 / 65 (the staging tile), 255 / 256 / 257 (the workgroup) and all samples:
    eta = |N x - r|_inf / (|N|_inf |x|_inf + |r|_inf) with N, r summed over ALL n samples in numpy.longdouble.  It does not depend on
    the condition number (1e7 - 1e18 here); a dropped or doubled sample, a wrong weight, a missing h^2 or a lost elimination update
    moves it by orders of magnitude.  Bound: ETA_CAP (32) x the eta of numpy.linalg.solve on the float64 normal equations of the same
    system -- two correct float64 solvers were measured within a factor 9 of each other on the CPU (summation order) -- and that
    yardstick itself < 1e-14 (on the CPU: 1.2e-17 ... 5.8e-16, test_rpcfit_cases_host.py).
    Measured on an MI355X over the 108 (case, n, axis, pass) systems: device / solve between 0.25 and 6.86, median 1.17 (the largest at
    n = 1000, pass 0: the order of 1000 terms per sum); the yardstick itself 5.5e-18 ... 5.8e-16.
    """
    rows = _eta_rows(name)
    for n, a, p, dev, ref in rows:
        print("eta {} n={} axis={} pass={} device {:.2e} solve {:.2e} ratio {:.2f}".format(name, n, a, p, dev, ref, dev / ref))
    for n, a, p, dev, ref in rows:
        assert ref < K.ETA_SOLVE_MAX, (name, n, a, p, ref)
        assert dev <= K.ETA_CAP * ref, (name, n, a, p, dev, ref)


@pytest.mark.parametrize("name", K.GOLDEN_FITS)
def test_rmse_is_the_returned_models(gpu, name):
    """the converged default call at every edge size: info["rmse"] is the RMSE of the returned coefficients (the same formula on the
    same numbers: 1e-9 px), the scaling parameters are exact"""
    g = _golden()
    for n in K.EDGE_N:
        t, x = K.subset(g, name, n)
        rpcs, info = ba_rpcfit.weighted_lsq_batch(t[None], x[None], return_info=True)
        assert np.array_equal(rpcs[0].to_table()[80:], K.scaling_table(t, x)[80:])
        assert 2 <= info["iters"][0] <= 20  # convergence is judged between two re-weighted passes
        assert abs(info["rmse"][0] - F.rmse_row_col(K.model_dict(rpcs[0]), x, t)) < 1e-9, (name, n)


def test_batch_of_different_pass_counts_equals_single_fits(gpu):
    """cameras that stop after different numbers of passes in one launch (the three cases and the first with 0.3 px of seeded noise
    on its target): each is the single fit, bit for bit.  At the default tol all of them converge in two passes; tighter ones spread
    the counts, and at least one of those tried must."""
    g = _golden()
    n = K.MIXED_PASSES_N
    sub = [K.subset(g, name, n) for name in K.GOLDEN_FITS]
    sub.append((sub[0][0] + np.random.default_rng(7).normal(0.0, 0.3, sub[0][0].shape), sub[0][1]))
    t = np.stack([s[0] for s in sub]); x = np.stack([s[1] for s in sub])
    mixed = 0
    for tol in (1e-2, 1e-5, 1e-7, 1e-9):
        rpcs, info = ba_rpcfit.weighted_lsq_batch(t, x, tol=tol, return_info=True)
        print("passes at n = {}, tol = {:.0e}: {}".format(n, tol, info["iters"]))
        mixed += len(set(info["iters"].tolist())) > 1
        for k in range(len(sub)):
            one, i1 = ba_rpcfit.weighted_lsq_batch(t[k][None], x[k][None], tol=tol, return_info=True)
            assert np.array_equal(one[0].to_table(), rpcs[k].to_table())
            assert i1["iters"][0] == info["iters"][k] and i1["rmse"][0] == info["rmse"][k]
    assert mixed >= 1  # or no batch mixes pass counts any more

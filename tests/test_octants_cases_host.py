"""The eight placements of tests/cases_octants.py, pinned on the CPU oracle.  The GPU tests (test_gpu_octants.py) hold the device to
the oracle in the moved frames, and the oracle is pinned to the reference in the original octant only: here the oracle in a moved
frame is held to the oracle in the original one through the two exact symmetries of the chain.  Every bound is MARGIN x the distance
measured on the pinned seed (the constants of cases_octants.py, each with its measurement): distances of the oracle to itself."""
import functools

import numpy as np
import pytest

import cases_octants as CO
from oracle import ba_oracle as O
from oracle import lm_oracle as L
from oracle import triangulate_oracle as T
from satba import synth
from satba.rpc_model import RPCModel, _POLYS, _SCALARS

PLACED = pytest.mark.parametrize("placement", CO.PLACEMENTS, ids=CO.placement_id)


@functools.lru_cache(maxsize=None)
def scene0():
    """one draw, in the original frame: 4 cameras x 300 points x 4 observations per point"""
    return synth.make_rpc_scene(4, 300, 4, seed=7)


def chain(r, X):
    """(col, row) (n, 2) and d(col, row)/dX (n, 2, 3) by the two pinned oracle Jacobians"""
    lat, lon, alt, G = L.geodetic_with_jacobian(X)
    q, D = L.rpc_project_with_jacobian(r, lat, lon, alt)
    return q, D @ G


@PLACED
def test_moved_rpc_round_trips_through_the_file_format(placement, tmp_path):
    """(a)"""
    files = CO.moved_files(tmp_path, *placement)
    assert len(files) == 2 and files[0] != files[1]
    for path, r in zip(files, CO.rpcs(*placement)):
        assert r.to_table().shape == (90,) and np.isfinite(r.to_table()).all()
        back = RPCModel.from_file(path)
        for _, attr in _SCALARS + _POLYS:  # 12 decimals
            assert np.abs(np.asarray(getattr(back, attr)) - np.asarray(getattr(r, attr))).max() <= 0.5000001e-12, attr
    r0, m = RPCModel.from_file(synth.default_rpc_files()[0]), CO.rpcs(*placement)[0]
    assert m.lon_offset == r0.lon_offset + placement[0] and m.lat_offset == (-r0.lat_offset if placement[1] else r0.lat_offset)
    changed = [k for k in range(20) if m.col_num[k] != r0.col_num[k]]
    assert changed == ([k for k in CO.ODD_IN_P if r0.col_num[k] != 0.0] if placement[1] else [])
    if placement == CO.ORIGINAL:
        assert np.array_equal(m.to_table(), r0.to_table())


def test_the_eight_sign_patterns_are_distinct_and_kept():
    """(b)"""
    seen = set()
    for placement in CO.PLACEMENTS:
        X = CO.moved_points(scene0().pts3d_true, *placement)
        sx, sy, sz, steep = CO.promised_signs(placement)
        assert np.all(np.sign(X[:, 0]) == sx) and np.all(np.sign(X[:, 1]) == sy) and np.all(np.sign(X[:, 2]) == sz), placement
        assert np.all((np.abs(X[:, 1]) > np.abs(X[:, 0])) == steep), placement
        assert np.array_equal(CO.original_points(X, *placement), scene0().pts3d_true)  # (a signed permutation: exact)
        # a scene drawn around the moved files lies in the same octant and under its cameras
        lat, lon, _ = O.ecef_to_latlon(*X.T)
        r = CO.rpcs(*placement)[0]
        assert np.abs(lon - r.lon_offset).max() < 0.011 and np.abs(lat - r.lat_offset).max() < 0.006
        seen.add((sx, sy, sz))
    assert len(seen) == 8 and CO.PLACEMENTS[0] == (0.0, False)
    # the four longitudes take every branch of the arctangent both ways: |x| >= |y| or not, x < 0 or not, y < 0 or not
    assert {(s[0], s[1], s[2]) for s in CO.LON_SIGNS.values()} == {(1, -1, True), (1, 1, False), (-1, 1, True), (-1, -1, False)}


@PLACED
def test_moved_rpc_projects_moved_points_to_the_same_pixels(placement):
    """(c) and (d)"""
    X = scene0().pts3d_true
    Xm = CO.moved_points(X, *placement)
    n = X.shape[0]
    base = [RPCModel.from_file(f) for f in synth.default_rpc_files()]
    moved = CO.rpcs(*placement)
    zero = np.zeros((2, 9))  # identity correction
    pts_ind, cam_ind = np.tile(np.arange(n), 2), np.repeat(np.arange(2), n)
    d_ba = np.abs(O.project_rpc(Xm, moved, zero, pts_ind, cam_ind, np.float64) - O.project_rpc(X, base, zero, pts_ind, cam_ind, np.float64)).max()
    d_px = d_jac = 0.0
    for r, m in zip(base, moved):
        q, J = chain(r, X)
        qm, Jm = chain(m, Xm)
        d_px = max(d_px, np.abs(qm - q).max())
        d_jac = max(d_jac, np.abs(CO.original_jacobian(Jm, *placement) - J).max() / np.abs(J).max())
        assert np.abs(q - np.stack(r.projection(*[L.geodetic_with_jacobian(X)[k] for k in (1, 0, 2)]), 1)).max() < 1e-8  # (the chain is the projection)
    print("{}: projection {:.3e} px (chain), {:.3e} px (ba_oracle), Jacobian {:.3e} rel".format(CO.placement_id(placement), d_px, d_ba, d_jac))
    assert d_px <= CO.MARGIN * CO.PROJ_CHAIN_PX and d_ba <= CO.MARGIN * CO.PROJ_BA_PX
    assert d_jac <= CO.MARGIN * CO.JAC_REL
    if placement[0] == 0.0:  # the pure mirror changes no longitude: only signs, which round to the same bits
        assert d_px == 0.0 and d_ba == 0.0


@PLACED
@pytest.mark.parametrize("corr", [["R"], ["R", "T"]], ids=["R", "RT"])
def test_residual_vector_of_a_moved_scene(placement, corr):
    """(e) one draw in the original frame, moved with cases_octants.moved_scene; corrections that turn about Z (and translate) at
    perturbed points, so that neither the residuals nor the corrections are trivial"""
    d = {"correction_params": corr, "n_cam_fix": 0, "reduce": False}
    p0, pm = synth.make_params(scene0(), d), synth.make_params(CO.moved_scene(scene0(), *placement), d)
    assert np.array_equal(pm.pts2d, p0.pts2d) and np.array_equal(pm.pts_ind, p0.pts_ind) and np.array_equal(pm.cam_ind, p0.cam_ind)
    rng = np.random.default_rng(3)
    v = p0.params_opt.copy()
    cam = v[: p0.n_cam * p0.n_params].reshape(p0.n_cam, p0.n_params)
    cam[:, 2] += rng.normal(0.0, 3e-6, p0.n_cam)
    if "T" in corr:
        cam[:, 3:6] += rng.normal(0.0, 2.0, (p0.n_cam, 3))
    v[p0.n_cam * p0.n_params:] += rng.normal(0.0, 1.0, 3 * p0.n_pts)
    f0 = O.fun(v, p0, np.float64)
    fm = O.fun(CO.moved_variables(v, p0.n_cam, p0.n_params, *placement), pm, np.float64)
    dist = np.abs(fm - f0).max()
    print("{} {}: residual vector {:.3e} px (|f| up to {:.2f} px)".format(CO.placement_id(placement), "".join(corr), dist, np.abs(f0).max()))
    assert np.abs(f0).max() > 1.0 and np.abs(f0 - O.fun(p0.params_opt, p0, np.float64)).max() > 0.5
    assert dist <= CO.MARGIN * CO.FUN_PX


@PLACED
def test_oracle_localisation_in_the_moved_frame(placement):
    """(f)"""
    rng = np.random.default_rng(5)
    d_lon = d_lat = 0.0
    for r, m in zip([RPCModel.from_file(f) for f in synth.default_rpc_files()], CO.rpcs(*placement)):
        n = 300
        col, row = r.col_offset + rng.uniform(-1.02, 1.02, n) * r.col_scale, r.row_offset + rng.uniform(-1.02, 1.02, n) * r.row_scale
        alt = r.alt_offset + rng.uniform(-1, 1, n) * r.alt_scale
        lon, lat = T._Rpc(r, 0.1).eval_rpc(col, row, alt)
        lon_m, lat_m = T._Rpc(m, 0.1).eval_rpc(col, row, alt)
        d_lon = max(d_lon, np.abs(lon_m - (lon + placement[0])).max())
        d_lat = max(d_lat, np.abs(lat_m - (-lat if placement[1] else lat)).max())
        assert np.abs(lon - r.lon_offset).max() < 0.1 and np.abs(lat - r.lat_offset).max() < 0.1
    print("{}: localisation {:.3e} deg (lon), {:.3e} deg (lat)".format(CO.placement_id(placement), d_lon, d_lat))
    assert d_lon <= CO.MARGIN * CO.LOC_LON_DEG and d_lat <= CO.MARGIN * CO.LOC_LAT_DEG

"""
Every RPC kernel family in every octant of the globe.  The shipped RPCs sit at 11.02 N, 72.71 W: x > 0, y < 0, z > 0, |y| > |x| for
every ECEF point the rest of the suite feeds an RPC kernel.  The eight placements of tests/cases_octants.py move the same two
cameras to the longitudes -72.7, 17.3, 107.3 and -162.7 degrees in both hemispheres by the chain's two exact symmetries; the
original placement stays in as the control.  The device is held to the CPU oracle IN the moved frame (test_octants_cases_host.py
pins the oracle there), with the tolerance the suite asserts for the same quantity in the original octant -- the magnitudes do not
change under the move -- and, for the camera approximations, to its own result in the original frame taken through the move, within
MARGIN x the distance of the two oracle results to each other.  Every yardstick is computed from the oracle and printed beside the
device's distance.
"""
import functools

import numpy as np
import pytest

import cases
import cases_camapprox as CC
import cases_octants as CO
from oracle import lm_oracle as L
from oracle import triangulate_oracle as T
from satba import ba_core, ba_rpcfit, cam_utils, geo_utils, synth, trf
from satba import ft_triangulate as FT
from satba.engine_hip import HipEngine
from test_gpu_cam_approx import bounds, expansion_value_error, resection_yardsticks
from test_gpu_parity import _run_phases, rel
from test_gpu_triangulate import _assert_f32_close

pytestmark = pytest.mark.gpu
PLACED = pytest.mark.parametrize("placement", CO.PLACEMENTS, ids=CO.placement_id)
OFFSETS = ((0.0, 0.0), (120.0, 75.0))  # the crop offsets of test_affine_against_oracle_composition


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """placement -> a scene of 6 cameras x 300 points x 4 (or opp) observations per point around the moved RPC files; built once"""
    made = {}

    def get(placement, opp=4, **kw):
        key = (placement, opp) + tuple(sorted(kw.items()))
        if key not in made:
            made[key] = CO.scene(placement, tmp_path_factory.mktemp("octant"), 6, 300, opp, seed=7, **kw)
        return made[key]
    return get


def in_octant(X, placement):
    sx, sy, sz, steep = CO.promised_signs(placement)
    return bool(np.all(np.sign(X[:, 0]) == sx) and np.all(np.sign(X[:, 1]) == sy) and np.all(np.sign(X[:, 2]) == sz)
                and np.all((np.abs(X[:, 1]) > np.abs(X[:, 0])) == steep))


def perturbed(p, seed=3):
    """the initial variables moved off the identity correction: angles ~ 3e-6 rad (1.5 px from 500 km), T and the points ~ 1 m"""
    rng = np.random.default_rng(seed)
    v = p.params_opt.copy()
    cam = v[: p.n_cam * p.n_params].reshape(p.n_cam, p.n_params)
    cam[:, :3] += rng.normal(0.0, 3e-6, (p.n_cam, 3))
    if p.n_params == 6:
        cam[:, 3:6] += rng.normal(0.0, 1.0, (p.n_cam, 3))
    v[p.n_cam * p.n_params:] += rng.normal(0.0, 1.0, 3 * p.n_pts)
    return ba_core._frozen_vars(v, p)


# ----------------------------------------------------------------------------- residuals, Jacobian, normal blocks, phases, a solve
@PLACED
@pytest.mark.parametrize("corr", [["R"], ["R", "T"]], ids=["R", "RT"])
@pytest.mark.parametrize("loss", ["linear", "soft_l1"])
def test_residuals_and_jacobian(gpu, scenes, placement, corr, loss):
    """geodetic<true>, rpc_project<true> and the rotation chain in the residual and linearisation kernels"""
    scene = scenes(placement)
    assert in_octant(scene.pts3d, placement)
    p = synth.make_params(scene, {"correction_params": corr, "n_cam_fix": 1, "reduce": False})
    v = perturbed(p)
    eng = HipEngine(p, rpc_f32=False)
    eng.configure(loss, 1.3)
    eng.set_x(v)
    Jc, Jp = eng.get_jacobian()
    f, _, _, Jc_o, Jp_o = L.weighted_system(v, p, loss, 1.3, rpc_f32=False)
    d_f = np.abs(eng.residuals() - f).max()
    print("{} {} {}: Jc {:.3e} rel, Jp {:.3e} rel, residuals {:.3e} px".format(CO.placement_id(placement), "".join(corr), loss, rel(Jc, Jc_o), rel(Jp, Jp_o), d_f))
    assert rel(Jc, Jc_o) < 1e-8 and rel(Jp, Jp_o) < 1e-8  # test_gpu_parity.test_jacobian_blocks
    assert d_f < 1e-8
    assert np.abs(f).max() > 1.0  # (not at a minimum, and not the identity correction)
    eng.close()


@PLACED
def test_residuals_with_the_float32_store(gpu, scenes, placement):
    """the reference's float32 store of the projections on, the bound of test_gpu_parity.test_normal_blocks: one float32 ulp of a
    pixel coordinate (a projection within ~1e-8 px of a rounding boundary lands on either side: of these eight scenes the one of
    lon-90_north has one such residual, 3.05e-5 px apart, the others agree bit for bit)"""
    p = synth.make_params(scenes(placement), {"correction_params": ["R", "T"], "n_cam_fix": 1, "reduce": False})
    v = perturbed(p, seed=4)
    eng = HipEngine(p)
    eng.configure("linear", 1.0)
    eng.set_x(v)
    d_f = np.abs(eng.residuals() - L.weighted_system(v, p)[0]).max()
    print("{}: residuals (float32 store) {:.3e} px".format(CO.placement_id(placement), d_f))
    assert d_f < 2.5e-4 * p.pts2d_w.max()
    eng.close()


@PLACED
@pytest.mark.parametrize("loss", ["linear", "soft_l1"])
def test_normal_blocks(gpu, scenes, placement, loss):
    """test_gpu_parity.test_normal_blocks and its tolerances, on the smooth function (no float32 store, as test_phases_match_oracle_engine
    compares it): with the store on, ONE residual that rounds to the other float32 changes the soft_l1 weights of its point and V by
    ~1e-6 relative (seen in lon-90_north, see test_residuals_with_the_float32_store), which a bound of 1e-8 cannot tell from a defect"""
    p = synth.make_params(scenes(placement), {"correction_params": ["R", "T"], "n_cam_fix": 1, "reduce": False})
    v = perturbed(p, seed=4)
    eng = HipEngine(p, rpc_f32=False)
    eng.configure(loss, 1.0)
    eng.set_x(v)
    eng.linearize()
    U, gc, V, gp = eng.get_blocks()
    hdr = eng.read_header()
    f, cost, fs, Jc, Jp = L.weighted_system(v, p, loss, 1.0, rpc_f32=False)
    U_o, gc_o, V_o, gp_o = L.normal_blocks(fs, Jc, Jp, p)
    V_o6 = V_o[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    print("{} {}: U {:.3e}, V {:.3e}, gc {:.3e}, gp {:.3e} rel".format(CO.placement_id(placement), loss, rel(U, U_o), rel(V, V_o6), rel(gc, gc_o), rel(gp, gp_o)))
    assert rel(U, U_o) < 1e-8 and rel(V, V_o6) < 1e-8
    assert rel(gc, gc_o) < 1e-6 and rel(gp, gp_o) < 1e-6
    assert abs(hdr[trf.COST] - cost) < 1e-6 * cost
    assert abs(hdr[eng.HDR_FIXED] - np.abs(gp_o).max()) < 1e-6 * np.abs(gp_o).max()
    eng.close()


@PLACED
@pytest.mark.parametrize("loss", ["linear", "soft_l1"])
def test_phases_match_oracle_engine(gpu, scenes, placement, loss):
    """test_gpu_parity.test_phases_match_oracle_engine: one outer iteration at lam = 1e-3, header slots to 1e-7, the vectors as there"""
    p = synth.make_params(scenes(placement), {"correction_params": ["R"], "n_cam_fix": 1, "reduce": False})
    v = perturbed(p, seed=5)
    dev, ora = HipEngine(p, rpc_f32=False), L.OracleEngine(p, rpc_f32=False)
    for e in (dev, ora):
        e.configure(loss, 1.0)
        e.set_x(v)
    a, b = _run_phases(dev, 1e-3), _run_phases(ora, 1e-3)
    assert abs(a["natural_lam"] - b["natural_lam"]) < 1e-7 * b["natural_lam"]
    for phase, slots in (("lin", [trf.COST, dev.HDR_FIXED]), ("prep", [trf.GH_SQ, trf.JG_SQ, trf.XS_SQ, trf.GC_INF]),
                         ("solve", [trf.GRAM_A, trf.GRAM_B, trf.GRAM_C, trf.CHOL_FAIL]), ("sub", [trf.WW]), ("prod", [trf.B11, trf.B12, trf.B22]),
                         ("trial", [trf.COST_NEW, trf.STEP_SQ, trf.X_SQ])):
        for s in slots:
            assert abs(a[phase][s] - b[phase][s]) <= 1e-7 * abs(b[phase][s]) + 1e-300, (phase, s, a[phase][s], b[phase][s])
    assert rel(dev.get_vector("scale_inv"), ora.scale_inv) < 1e-9
    assert rel(dev.get_vector("g_h"), ora.g_h) < 1e-8
    assert rel(dev.get_vector("gn_h"), ora.gn_h) < 1e-7
    assert rel(dev.get_vector("q1"), ora.q1) < 1e-8
    assert rel(dev.get_vector("x_new"), ora.x_new) < 1e-12
    dev.close()


@PLACED
def test_solve_ends_where_the_oracle_ends(gpu, scenes, placement):
    """test_gpu_parity.test_random_problems_end_where_the_oracle_ends: the trial kernels' geodetic<false> run a whole solve.  Every
    camera sees every point here (6 observations per point, the corrections of solve_rpc_small_R): the two shipped RPCs alternate,
    and with 4 of 6 cameras a point in fourteen is seen by cameras of one parity only and has no parallax -- on that scene the
    ORACLE's loop runs into max_nfev at these tolerances (status 0 in 2 of 3 placements tried), which says nothing about an octant"""
    p = synth.make_params(scenes(placement, opp=6, sigma_theta=5e-6), {"correction_params": ["R"], "n_cam_fix": 1})
    res = []
    for e, native in ((HipEngine(p, rpc_f32=False), True), (L.OracleEngine(p, rpc_f32=False), False)):
        e.configure("soft_l1", 1.0)
        e.set_x(p.params_opt.copy())
        res.append(trf.trf_solve(e, ftol=1e-9, xtol=1e-12, gtol=1e-10, max_nfev=200, loss="soft_l1", f_scale=1.0, native=native))
    rd, ro = res
    print("{}: cost {:.10e} (device, {} evaluations) {:.10e} (oracle, {}), {:.3e} rel".format(CO.placement_id(placement), rd.cost, rd.nfev, ro.cost, ro.nfev, abs(rd.cost - ro.cost) / ro.cost))
    assert rd.status > 0 and ro.status > 0, (rd.status, ro.status)
    assert abs(rd.cost - ro.cost) <= 1e-8 * ro.cost


# ----------------------------------------------------------------------------- triangulation, localisation, re-fit
@PLACED
def test_triangulation(gpu, scenes, placement):
    """tri_localize and the RPC triangulation: test_gpu_triangulate.test_pairwise_against_oracle_float64's bounds for the pair, the
    float32 means of init_pts3d as test_init_pts3d_against_reference_vectors compares them"""
    scene = scenes(placement)
    C = scene.to_dense_C()
    t = np.where(~np.isnan(C[0]) & ~np.isnan(C[2]))[0]
    oi, oj = C[0:2, t].T, C[2:4, t].T
    want, werr = T.rpc_triangulation(scene.cameras[0], scene.cameras[1], oi, oj)
    got, gerr = FT.rpc_triangulation(scene.cameras[0], scene.cameras[1], oi, oj)
    print("{}: {} pairs, points {:.3e} m, errors {:.3e}".format(CO.placement_id(placement), len(t), np.abs(got - want).max(), np.abs(gerr[:, 0] - werr).max()))
    assert len(t) > 100 and np.isfinite(got).all() and np.isfinite(gerr).all()
    assert np.abs(gerr[:, 0] - werr).max() < 1e-5 and np.abs(got - want).max() < 1e-4
    assert in_octant(got, placement) and np.abs(got - scene.pts3d_true[t]).max() < 50.0
    pairs = [(0, 1), (2, 3)]
    pts = FT.init_pts3d(C, scene.cameras, "rpc", pairs)
    _assert_f32_close(pts, T.init_pts3d(C, scene.cameras, "rpc", pairs))
    done = pts.any(axis=1)
    assert np.isfinite(pts).all() and done.sum() > 150 and in_octant(pts[done].astype(np.float64), placement)


@PLACED
def test_localization(gpu, placement):
    """test_gpu_rpcfit.test_localization_inverts_the_projection in the moved frame"""
    rng = np.random.default_rng(5)
    for r in CO.rpcs(*placement):
        n = 3000
        col, row = r.col_offset + rng.uniform(-1.02, 1.02, n) * r.col_scale, r.row_offset + rng.uniform(-1.02, 1.02, n) * r.row_scale
        alt = r.alt_offset + rng.uniform(-1, 1, n) * r.alt_scale
        lo, la = r.localization(col, row, alt)
        assert np.isfinite(lo).all() and np.isfinite(la).all()
        c2, r2 = r.projection(lo, la, alt)
        lo2, la2 = T._Rpc(r, 0.1).eval_rpc(col[:300], row[:300], alt[:300])
        print("{}: back on the image points within {:.3e} px, the oracle's root within {:.3e} deg (lon) {:.3e} deg (lat)".format(
            CO.placement_id(placement), max(np.abs(c2 - col).max(), np.abs(r2 - row).max()), np.abs(lo[:300] - lo2).max(), np.abs(la[:300] - la2).max()))
        assert np.abs(c2 - col).max() < 1e-5 and np.abs(r2 - row).max() < 1e-5
        assert np.abs(lo[:300] - lo2).max() < 1e-9 and np.abs(la[:300] - la2).max() < 1e-9
        assert np.abs(lo - r.lon_offset).max() < 0.1 and np.abs(la - r.lat_offset).max() < 0.1  # (under the moved camera)


@PLACED
def test_refit(gpu, placement):
    """the first half of test_gpu_rpcfit.test_fit_Rt_corrected_rpc_reproduces_the_corrected_projection in the moved frame: the centre
    of the correction 500 km above the moved RPC's centre (the affine route of that test has no RPC geometry)"""
    r, r1 = CO.rpcs(*placement)
    crop = {"col0": 0, "row0": 0, "width": int(2 * r.col_scale), "height": int(2 * r.row_scale)}
    c = np.array(geo_utils.latlon_to_ecef_custom(r.lat_offset, r.lon_offset, r.alt_offset))
    assert in_octant(c[None], placement)
    C = c + 5e5 * c / np.linalg.norm(c)
    Rt = np.concatenate([[4e-6, -3e-6, 5e-6], np.zeros(3), C]).reshape(1, 9)
    rng = np.random.default_rng(1)
    alt = r.alt_offset + rng.uniform(-0.5, 0.5, 500) * r.alt_scale
    lo, la = r.localization(rng.uniform(0, crop["width"], 500), rng.uniform(0, crop["height"], 500), alt)
    pts = np.stack(geo_utils.latlon_to_ecef_custom(la, lo, alt), 1)
    rpc, err, margin = ba_rpcfit.fit_Rt_corrected_rpc(Rt, None, r, crop, pts)
    want = cam_utils.apply_rpc_projection(r, ba_core.adjust_pts3d(pts, Rt))
    got = cam_utils.apply_rpc_projection(rpc, pts)
    print("{}: margin {}, err {:.3e} px, fitted against corrected projection {:.3e} px, the correction {:.2f} px".format(
        CO.placement_id(placement), margin, err.max(), np.abs(got - want).max(), np.abs(cam_utils.apply_rpc_projection(r, pts) - want).max()))
    assert margin in (10, 20, 40, 80, 160, 320, 640, 1280) and err.shape == (1000,) and err.max() < 0.5
    assert np.abs(got - want).max() < 0.05
    assert np.abs(cam_utils.apply_rpc_projection(r, pts) - want).max() > 1.0
    crop1 = {"col0": 0, "row0": 0, "width": int(2 * r1.col_scale), "height": int(2 * r1.row_scale)}
    Rt1 = Rt * np.r_[2.0 * np.ones(3), np.ones(6)]
    many, info = ba_rpcfit.fit_Rt_corrected_rpcs([Rt, Rt1], None, [r, r1], [crop, crop1], return_info=True)
    one = ba_rpcfit.fit_Rt_corrected_rpc(Rt1, None, r1, crop1, pts)
    for (rpc_d, err_d, margin_d), (rpc_h, err_h, margin_h), rr, RT, cr, k in ((many[0], (rpc, err, margin), r, Rt, crop, 0), (many[1], one, r1, Rt1, crop1, 1)):
        assert margin_d == margin_h and err_d.shape == err_h.shape
        locs_d, target_d = info["input_locs"][k], info["target"][k]
        cols, rows, alts = cam_utils.generate_point_mesh([-margin_h, cr["width"] + margin_h, 10], [-margin_h, cr["height"] + margin_h, 10],
                                                         [rr.alt_offset - rr.alt_scale, rr.alt_offset + rr.alt_scale, 10])
        assert np.abs(locs_d[:, 2] - alts).max() == 0.0
        lon_h, lat_h = rr.localization(cols, rows, alts)
        assert np.abs(locs_d[:, 0] - lon_h).max() < 1e-11 and np.abs(locs_d[:, 1] - lat_h).max() < 1e-11
        X = np.stack(geo_utils.latlon_to_ecef_custom(lat_h, lon_h, alts), 1)
        assert np.abs(target_d - cam_utils.apply_rpc_projection(rr, ba_core.adjust_pts3d(X, RT))).max() < 1e-6
        assert np.abs(np.stack(rpc_d.projection(*locs_d.T), 1) - np.stack(rpc_h.projection(*locs_d.T), 1)).max() < 2e-3
        assert np.abs(err_d - err_h).max() < 2e-3 and np.abs(err_d - ba_rpcfit.check_errors(rpc_d, locs_d, target_d)).max() < 1e-9


# ----------------------------------------------------------------------------- affine approximation
def affine_device(r, p, col0, row0):
    return cam_utils.affine_rpc_approx(r, p[0], p[1], p[2], {"col0": col0, "row0": row0})


@PLACED
def test_affine_against_oracle_composition(gpu, placement):
    """test_gpu_cam_approx.test_affine_against_oracle_composition at the moved RPCs' own expansion points, the yardstick evaluated
    in the moved frame"""
    for f, r in enumerate(CO.rpcs(*placement)):
        for p in CC.expansion_points(r):
            assert in_octant(p[None], placement)
            for col0, row0 in OFFSETS:
                P = affine_device(r, p, col0, row0)
                Pe = CC.affine_expected(r, p, col0, row0)
                yJ, yT = CC.affine_yardstick(r, p, col0, row0)
                dJ, dT = np.abs(P[:2, :3] - Pe[:2, :3]).max() / np.abs(Pe[:2, :3]).max(), np.abs(P[:2, 3] - Pe[:2, 3]).max()
                print("{} rpc {} offset ({}, {}): J {:.3e} rel (bound {:.3e}), P[:2, 3] {:.3e} px (bound {:.3e})".format(
                    CO.placement_id(placement), f, col0, row0, dJ, CC.MARGIN * yJ, dT, CC.MARGIN * yT))
                assert dJ <= CC.MARGIN * yJ and dT <= CC.MARGIN * yT
                assert np.array_equal(P[2], [0.0, 0.0, 0.0, 1.0])


def lon_ulp_factor(r):
    """ulp of the moved longitude over the ulp of the shipped one (72.7 deg): 1 up to 128 deg, 2 beyond"""
    return max(1.0, np.spacing(abs(r.lon_offset)) / np.spacing(72.7))


@functools.lru_cache(maxsize=None)
def expansion_values(placement):
    """[(rpc, point, offset, |P (p, 1) - q| against the oracle's float64 q, against q in extended precision, eps_f, the oracle's
    own |q - q_ext|, ulp factor)] of the device's affine matrices at the moved RPCs' expansion points; computed once"""
    out = []
    for f, r in enumerate(CO.rpcs(*placement)):
        for k, p in enumerate(CC.expansion_points(r)):
            q = CC.rpc_oracle(r, p)[0][0]
            q_ext = CC.rpc_oracle_extended(r, p)
            eps_f = 4 * np.finfo(float).eps * np.linalg.norm(p) * np.abs(CC.rpc_oracle(r, p)[1][0]).max()  # cases_camapprox.fd_step_and_bound
            for col0, row0 in OFFSETS:
                out.append((f, k, (col0, row0), expansion_value_error(r, p, col0, row0, q), expansion_value_error(r, p, col0, row0, q_ext), eps_f,
                            float(np.abs(q - q_ext).max()), lon_ulp_factor(r)))
    return out


@PLACED
def test_affine_expansion_value_in_extended_precision(gpu, placement):
    """P (p, 1) == q - (col0, row0), q the oracle's projection at p in extended precision, within what one float64 evaluation is
    good to (eps_f ~ 8e-9 px: the second assertion of test_gpu_cam_approx.test_affine_reproduces_the_expansion_value), everywhere.
    This is the test that runs every branch of cam_atan2_rounded on the device: |x| >= |y| at 17.3 and -162.7 degrees, the
    subtraction from pi at 107.3 and -162.7.  Measured, the largest per longitude (north / south): -72.7: 1.58e-9 / 1.58e-9,
    17.3: 7.1e-10 / 7.1e-10, 107.3: 8.7e-10 / 7.8e-10, -162.7: 2.39e-9 / 2.26e-9 px -- the oracle's own float64 q is as far from
    that value (1.16e-9, 3.4e-10, 8.3e-10, 2.35e-9 px), since both round the longitude in degrees to the same float64."""
    for f, k, off, e, e_ext, eps_f, e_oracle, _ in expansion_values(placement):
        print("{} rpc {} point {} offset {}: against q in extended precision {:.3e} px (bound {:.3e}); the oracle's float64 q against it {:.3e} px".format(
            CO.placement_id(placement), f, k, off, e_ext, eps_f, e_oracle))
        assert e_ext <= eps_f


@PLACED
def test_affine_expansion_value_against_the_float64_oracle(gpu, placement):
    """P (p, 1) == q - (col0, row0), q the oracle's FLOAT64 projection at p, within 1e-9 px x max(1, ulp(|lon'|) / ulp(72.7)): the
    1e-9 px of test_gpu_cam_approx.test_affine_reproduces_the_expansion_value where an ulp of the longitude is that of 72.7 degrees
    (up to 128 degrees), twice that at -162.7.

    Measured, the largest of the four points (bound): lon+0_north 4.67e-10 (1e-9), lon+90_north 9.08e-10 (1e-9), lon+180_north
    4.89e-10 (1e-9), lon-90_north 5.39e-10 (2e-9), lon+0_south 4.67e-10 (1e-9), lon+90_south 9.08e-10 (1e-9), lon+180_south
    2.00e-10 (1e-9), lon-90_south 5.21e-10 (2e-9) px.

    This test found a defect.  k_cam_affine took rad * (180 / pi) - lon_offset as ONE fused multiply-add: the longitude in degrees
    was never rounded, so q carried the rounding of the radians alone while the float64 value it is compared with rounds the
    degrees as well (the correctly rounded radians times 180 / pi give the oracle's longitude bit for bit at all 32 points, on a
    host build).  The two sat up to half an ulp of the longitude apart -- 1.1e-9 px at 107 degrees, 2.2e-9 px at -162.7 -- and
    the figures read 1.42e-9, 2.29e-9, 1.007e-9, 1.135e-9 and 2.14e-9 px in lon+180_north, lon-90_north, lon+0_south,
    lon+180_south and lon-90_south (7.39e-10 px at the shipped points: below the bound by luck).  The kernel now rounds the
    product before the offset is taken off."""
    worst = 0.0
    for f, k, off, e, e_ext, eps_f, e_oracle, factor in expansion_values(placement):
        print("{} rpc {} point {} offset {}: P (p, 1) - q {:.3e} px (bound {:.1e}); the matrix against q in extended precision {:.3e} px, the oracle's q against it {:.3e} px".format(
            CO.placement_id(placement), f, k, off, e, 1e-9 * factor, e_ext, e_oracle))
        worst = max(worst, e / factor)
    assert worst <= 1e-9


@functools.lru_cache(maxsize=None)
def affine_of_placement(placement):
    """device P (3, 4) and oracle composition at the ORIGINAL expansion points taken to the placement: [(f, point, offset)] -> (P, Pe)"""
    out = {}
    for f, (r0, r) in enumerate(zip(CO.rpcs(*CO.ORIGINAL), CO.rpcs(*placement))):
        for k, p0 in enumerate(CC.expansion_points(r0)):
            p = CO.moved_points(p0, *placement)
            for col0, row0 in OFFSETS:
                out[f, k, col0] = (affine_device(r, p, col0, row0), CC.affine_expected(r, p, col0, row0))
    return out


@PLACED
def test_affine_taken_back_is_the_original(gpu, placement):
    """metamorphic: J of the moved camera at the moved point, taken back through the rotation and the mirror, against the device's
    own J in the original frame, within MARGIN x the distance of the two oracle compositions to each other.  Both distances are
    the largest over the placement's four expansion points: at a single point the numpy composition can be EXACTLY symmetric
    (distance 0 at five of the twelve rotated points of the northern placements; x * x + y * y rounds alike when x and y swap) where the device's fused
    x * x + y * y does not, so a point's own yardstick can be zero while the placement's is 9e-16 .. 1e-14.  The pure mirror is
    exact on both sides."""
    moved, orig = affine_of_placement(placement), affine_of_placement(CO.ORIGINAL)
    d = yard = 0.0
    for key in orig:
        (P, Pe), (P0, Pe0) = moved[key], orig[key]
        scale = np.abs(Pe0[:2, :3]).max()
        d_k = np.abs(CO.original_jacobian(P[:2, :3], *placement) - P0[:2, :3]).max() / scale
        y_k = np.abs(CO.original_jacobian(Pe[:2, :3], *placement) - Pe0[:2, :3]).max() / scale
        print("{} {}: J taken back against the original {:.3e} rel (device), {:.3e} rel (oracle)".format(CO.placement_id(placement), key, d_k, y_k))
        d, yard = max(d, d_k), max(yard, y_k)
        assert np.array_equal(P[2], [0.0, 0.0, 0.0, 1.0])
    print("{}: {:.3e} rel (device), bound {:.3e}".format(CO.placement_id(placement), d, CO.MARGIN * yard))
    assert d <= CO.MARGIN * yard


# ----------------------------------------------------------------------------- perspective approximation and centres
def stacked_ranges(rpcs, crop):
    return [np.array([list(v) for v in rs]) for rs in zip(*[CC.perspective_ranges(r, crop) for r in rpcs])]


@functools.lru_cache(maxsize=None)
def perspective_of_placement(placement, cname):
    """device cameras and centres of both RPCs in one launch, and the restatement's centres on the oracle's mesh"""
    rpcs, crop = CO.rpcs(*placement), CC.CROPS[cname]
    cams, info = cam_utils.approx_cameras(rpcs, [CC.offset(crop)] * 2, "perspective", return_info=True)
    restated = [CC.resect(*CC.mesh_correspondences(r, *CC.perspective_ranges(r, crop)))[2] for r in rpcs]
    return cams, info, restated


@PLACED
@pytest.mark.parametrize("cname", ["full", "c50"])
def test_perspective_and_centres(gpu, placement, cname):
    """k_cam_resect (mesh, localisation, ECEF, resection, centre) in the moved frame: against the restatement on the device's own
    mesh within the bounds of test_gpu_cam_approx.test_mesh_sizes_against_the_restatement, the mesh against the host's as in
    test_full_route_equals_its_parts, the centre against the original placement's through the move"""
    rpcs, crop = CO.rpcs(*placement), CC.CROPS[cname]
    cams, info, restated = perspective_of_placement(placement, cname)
    _, info0, restated0 = perspective_of_placement(CO.ORIGINAL, cname)
    Xd, xd, altd = cam_utils.rpc_point_mesh(rpcs, *stacked_ranges(rpcs, crop))
    b_px, b_m = bounds(max(v[0] for v in resection_yardsticks().values()), max(v[1] for v in resection_yardsticks().values()))
    for k, r in enumerate(rpcs):
        cols, rows, alts = cam_utils.generate_point_mesh(*CC.perspective_ranges(r, crop))
        assert np.array_equal(altd[k], alts) and np.array_equal(xd[k, :, 0], cols) and np.array_equal(xd[k, :, 1], rows)
        lons, lats = r.localization(cols, rows, alts)
        X = np.vstack(geo_utils.latlon_to_ecef_custom(lats, lons, alts)).T
        assert in_octant(Xd[k], placement)
        assert np.abs(Xd[k] - X).max() <= 4e-9
        Pr, err_r, cen_r = CC.resect(Xd[k], xd[k])
        d_px, d_m = CC.reprojection_distance(cams[k], CC.to_crop(Pr, crop), Xd[k]), np.abs(info["centers"][k] - cen_r).max()
        _, _, alt_c = geo_utils.ecef_to_latlon_custom(*info["centers"][k])
        back = CO.original_points(info["centers"][k], *placement)
        d_back = np.abs(back - info0["centers"][k]).max()
        yard = np.abs(CO.original_points(restated[k], *placement) - restated0[k]).max()
        print("{} {} rpc {}: reprojection {:.3e} px (bound {:.3e}), centre {:.3e} m (bound {:.3e}), mean_err {:.3e} vs {:.3e}, mesh vs host {:.3e} m, {:.1f} km up; "
              "centre taken back against the original {:.3e} m (device), {:.3e} m (restatement), bound {:.3e}".format(
                  CO.placement_id(placement), cname, k, d_px, b_px, d_m, b_m, info["mean_err"][k], err_r, np.abs(Xd[k] - X).max(), alt_c / 1e3, d_back, yard, CO.MARGIN * yard))
        assert d_px <= b_px and abs(info["mean_err"][k] - err_r) <= b_px and d_m <= b_m
        assert 400e3 <= alt_c <= 700e3
        assert d_back <= CO.MARGIN * yard
        alone, info_a = cam_utils.approx_cameras([r], [CC.offset(crop)], "perspective", return_info=True)
        assert np.array_equal(alone[0], cams[k]) and info_a["mean_err"][0] == info["mean_err"][k] and np.array_equal(info_a["centers"][0], info["centers"][k])
    assert not np.array_equal(cams[0], cams[1])


# ----------------------------------------------------------------------------- the pipeline's sequence
@pytest.mark.parametrize("placement", [(180.0, True), (-90.0, False)], ids=CO.placement_id)
def test_rpc_pipeline_sequence_config1(gpu, placement):
    """test_gpu_parity.test_rpc_pipeline_sequence_config1, its size and its assertions, on that test's scene taken to the two
    placements farthest from the original (the same draws: the reference's errors of the original scene still apply)"""
    g = cases.golden("solve_rpc_config1")
    scene = CO.moved_scene(synth.make_rpc_scene(2, 2000, 2, seed=1, sigma_theta=5e-6), *placement)
    assert in_octant(scene.pts3d, placement)
    p = synth.make_params(scene, {"correction_params": ["R"], "reduce": False})
    _, v1, e0, e1, it1 = ba_core.run_ba_optimization(p, {"loss": "soft_l1", "f_scale": 1.0, "max_iter": 300, "verbose": 0}, False, False)
    p.params_opt = v1.copy()
    _, v2, _, e2, it2 = ba_core.run_ba_optimization(p, {"verbose": 0}, False, False)
    print("{}: initial errors {:.3e} px from the reference's, soft_l1 mean {:.3e}, l2 mean {:.3e} from the reference's".format(
        CO.placement_id(placement), np.abs(e0 - g["err_init"]).max(), abs(e1.mean() - g["err_softl1"].mean()), abs(e2.mean() - g["err_l2"].mean())))
    assert np.abs(e0 - g["err_init"]).max() < 2.5e-4
    assert abs(e1.mean() - g["err_softl1"].mean()) < 5e-3 and abs(e2.mean() - g["err_l2"].mean()) < 5e-3
    assert e2.mean() < 0.05 * e0.mean()
    pts3d, cams = p.reconstruct_vars(v2, scene.pts3d, scene.cameras)
    assert len(p.estimated_params) == 2 and set(p.estimated_params[0]) == {"R", "C"}

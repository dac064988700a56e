"""
The one-byte camera stream of the point kernels (csrc/satba_layout.h: Layout::e_cam8; csrc/satba_kernels.h: CamStream) and the two
per-point reads they skip when nothing needs them (perm without fixed points: point_mask; ipt_ofs without row scales or stored
RPC rows).

With at most 255 cameras a handle builds e_cam8 beside e_cam and k_linearize (but for its perspective weighted / robust and RPC
variants, which keep the int array), k_jvp, k_backsub and k_residual read the camera of a slot from it; from 256 cameras on, or under SATBA_CAM_NARROW=0, they read the int array as before.  Every other test of the suite
has fewer than 256 cameras and so runs on the narrow route: this file is what runs the wide one.  The two routes load the same
camera index, so everything downstream is compared bit for bit.

  1. the array: e_cam8 == e_cam at every slot (0xFF <-> -1 in the padding), M = 3, 40, 255; absent at M = 256 and under the switch
  2. the two routes, phase by phase (linearize -> prepare -> schur -> solve -> subspace -> trial), at 1, 2, 4 and 8 lanes per point
     (SATBA_SPLIT, as tests/test_gpu_lanes.py sets it): affine and perspective R+T with unit weights, affine soft_l1 with a weighted
     camera (merged records: row scales indexed by ipt_ofs), RPC (stored Jacobian rows indexed by ipt_ofs)
  3. n_pts_fix = 0 (perm is not read) and 7 (it is): fixed points stay, their blocks are zero, the free points' blocks are float64's
  4. 256 cameras: the wide route by rule solves to where the Python loop does; 255 cameras: both routes, identical solves
  5. the device-resident loop on both routes: identical statistics and solution

Tolerances against float64 are those of tests/test_gpu_lanes.py (V 1e-8, g_p 1e-6 of the largest entry), those of the loop
comparison are test_solve_lm_matches_python_loop's (tests/test_gpu_layout.py: cost 1e-14, x 1e-12 relative, same counts).
"""
import functools

import numpy as np
import pytest

from oracle import lm_oracle as L
from satba import ba_core, synth, trf
from satba.engine_hip import HipEngine
from test_gpu_parity import _run_phases, rel

pytestmark = pytest.mark.gpu

SWITCHES = ("SATBA_CAM_NARROW", "SATBA_SPLIT", "SATBA_HOST_LOOP", "SATBA_DEVICE_LOOP")
LAM = 1e-3  # damping of the phase comparison (tests/test_gpu_parity.py)


@functools.lru_cache(maxsize=None)
def tracks_scene(model, n_cam, n_pts, lo, hi, seed=1):
    """A scene of synth with every camera seeing every point, thinned to tracks of lo .. hi observations: point q keeps the cameras
    2 q and 2 q + 1 (mod n_cam; the first only for a track of one), so that every camera is observed once n_pts >= n_cam / 2, and
    random others up to its length; the lengths cycle through lo .. hi in an order that does not follow the point index."""
    scene = synth.make_scene(model, n_cam, n_pts, n_cam, seed=seed)
    assert scene.n_obs == n_cam * n_pts and np.array_equal(scene.cam_ind[:n_cam], np.arange(n_cam))  # point-major, all visible
    rng = np.random.default_rng([seed, n_cam, n_pts])
    lengths = lo + rng.permutation(n_pts) % (hi - lo + 1)
    keep = np.zeros((n_pts, n_cam), dtype=bool)
    for q in range(n_pts):
        first = [(2 * q) % n_cam, (2 * q + 1) % n_cam][: lengths[q]]
        rest = [c for c in rng.permutation(n_cam) if c not in first]
        keep[q, first + rest[: lengths[q] - len(first)]] = True
    assert np.array_equal(keep.sum(axis=1), lengths)
    k = keep.ravel()
    d = dict(scene.__dict__, pts_ind=scene.pts_ind[k], cam_ind=scene.cam_ind[k], pts2d=scene.pts2d[k])
    return synth.Scene(**d)


def engine(monkeypatch, p, narrow=True, rpc_f32=True, **env):
    """A handle created on the narrow route (the rule) or under SATBA_CAM_NARROW=0, with the other switches as given."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    if not narrow:
        monkeypatch.setenv("SATBA_CAM_NARROW", "0")
    eng = HipEngine(p, rpc_f32=rpc_f32)
    monkeypatch.delenv("SATBA_CAM_NARROW", raising=False)
    assert eng.info()["cam_narrow"] == (1 if narrow and p.n_cam <= 255 else 0), eng.info()
    return eng


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ----------------------------------------------------------------------------- 1. the array

@pytest.mark.parametrize("n_cam,lo,hi", [(3, 1, 3), (40, 2, 8), (255, 2, 8)])
def test_narrow_array_is_the_int_array(gpu, monkeypatch, n_cam, lo, hi):
    """130 points are three slices, the last with two points; at least three track lengths, so slices hold padded slots."""
    p = synth.make_params(tracks_scene("affine", n_cam, 130, lo, hi), {"correction_params": ["R"], "n_cam_fix": 1})
    assert np.unique(np.bincount(p.pts_ind, minlength=130)).size >= 3
    eng = engine(monkeypatch, p)
    wide, narrow = eng.get_layout("e_cam"), eng.get_layout("e_cam8")
    assert narrow.dtype == np.uint8 and narrow.shape == wide.shape == (int(eng.info()["ell_len"]),)
    pad = wide < 0
    assert pad.any() and np.all(wide[pad] == -1) and np.all(narrow[pad] == 0xFF)
    assert np.array_equal(narrow[~pad].astype(np.int32), wide[~pad]) and wide[~pad].max() == n_cam - 1
    assert np.count_nonzero(~pad) == p.n_obs
    eng.close()


def test_narrow_array_is_absent_from_256_cameras_on_and_under_the_switch(gpu, monkeypatch):
    p = synth.make_params(tracks_scene("affine", 256, 130, 2, 8), {"correction_params": ["R"], "n_cam_fix": 1})
    eng = engine(monkeypatch, p)
    assert eng.info()["cam_narrow"] == 0 and eng.get_layout("e_cam").max() == 255
    with pytest.raises(ValueError):
        eng.get_layout("e_cam8")
    eng.close()
    p = synth.make_params(tracks_scene("affine", 40, 130, 2, 8), {"correction_params": ["R"], "n_cam_fix": 1})
    eng = engine(monkeypatch, p, narrow=False)
    assert eng.info()["cam_narrow"] == 0
    with pytest.raises(ValueError):
        eng.get_layout("e_cam8")
    eng.close()


# ----------------------------------------------------------------------------- 2. the routes, kernel by kernel

# name -> (model, options, loss, rpc_f32, unit-weight run)
FAMILIES = {
    "affine_RT": ("affine", {"correction_params": ["R", "T"]}, "linear", True, True),
    "persp_RT": ("perspective", {"correction_params": ["R", "T"]}, "linear", True, True),
    "affine_RT_weighted_soft_l1": ("affine", {"correction_params": ["R", "T"], "ref_cam_weight": 2.5}, "soft_l1", True, False),
    "rpc_R": ("rpc", {"correction_params": ["R"]}, "linear", False, True),
}
SMALL_SEED = 3


@functools.lru_cache(maxsize=None)
def small_params(name, n_pts_fix=0):
    """12 cameras x 300 points, tracks of 2 .. 8: five slices, the last with 44 points."""
    model, opts = FAMILIES[name][:2]
    p = synth.make_params(tracks_scene(model, 12, 300, 2, 8, seed=SMALL_SEED), dict(opts, n_cam_fix=1, n_pts_fix=n_pts_fix, reduce=False))
    return p, ba_core._frozen_vars(p.params_opt.copy(), p)


def walk(eng, loss, v):
    """One iteration through the phase entry points; everything the kernels in question leave behind."""
    eng.configure(loss, 1.0)
    eng.set_x(v)
    out = dict(_run_phases(eng, LAM))
    model = out.pop("model")
    out["model"] = np.array(model)
    out["natural_lam"] = np.array(out["natural_lam"])
    _, _, out["V"], out["gp"] = eng.get_blocks()
    for k in ("g", "scale_inv", "gn_h", "q1", "w", "x_new"):
        out["vec_" + k] = eng.get_vector(k)
    return out


@pytest.mark.parametrize("sh", [0, 1, 2, 3])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_routes_are_equal_kernel_by_kernel(gpu, monkeypatch, name, sh):
    """V, g (cameras and points), scale_inv, the headers of every phase (cost, |g_h|^2, the Gram entries, the trial cost, |step|^2,
    |x|^2, ...), the camera and point step gn_h and the trial point: the same bits on both routes."""
    loss, rpc_f32, unit = FAMILIES[name][2:5]
    p, v = small_params(name)
    assert np.bincount(p.pts_ind).min() == 2 and np.bincount(p.pts_ind).max() == 8 and bool(np.all(p.pts2d_w == 1.0)) == (name != "affine_RT_weighted_soft_l1")
    got = []
    for narrow in (True, False):
        eng = engine(monkeypatch, p, narrow=narrow, rpc_f32=rpc_f32, SATBA_SPLIT=sh)
        info = eng.info()
        assert info["lanes_log2"] == sh and info["cam_sums_lds"] == 1
        got.append(walk(eng, loss, v))
        assert eng.info()["unit_weights"] == (1 if np.all(p.pts2d_w == 1.0) else 0) and eng.info()["fx_fallbacks"] == 0
        if not unit:
            eng.get_layout("sc_ofs")  # the merged records exist: the row scales were stored and read through them
        eng.close()
    a, b = got
    assert a.keys() == b.keys()
    assert a["trial"][trf.COST_NEW] > 0.0 and a["trial"][trf.STEP_SQ] > 0.0 and np.any(a["vec_gn_h"] != 0.0) and np.any(a["V"] != 0.0)
    for k in a:
        assert same_bits(a[k], b[k]), (k, np.abs(np.asarray(a[k]) - np.asarray(b[k])).max())


# ----------------------------------------------------------------------------- 3. fixed points

@pytest.mark.parametrize("narrow", [True, False], ids=["narrow", "wide"])
@pytest.mark.parametrize("n_fix", [0, 7])
def test_fixed_points(gpu, monkeypatch, n_fix, narrow):
    p, v = small_params("affine_RT", n_fix)
    assert p.n_pts_fix == n_fix
    eng = engine(monkeypatch, p, narrow=narrow)
    eng.configure("linear", 1.0)
    eng.set_x(v)
    eng.linearize()
    _, _, V, gp = eng.get_blocks()
    f, cost, fs, Jc, Jp = L.weighted_system(v, p)
    _, _, V_o, gp_o = L.normal_blocks(fs, Jc, Jp, p)
    V6_o = V_o[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    assert np.all(V[:n_fix] == 0.0) and np.all(gp[:n_fix] == 0.0)
    assert np.all(V[n_fix:, [0, 3, 5]] > 0.0)
    print("V {:.3g} g_p {:.3g}".format(rel(V[n_fix:], V6_o[n_fix:]), rel(gp[n_fix:], gp_o[n_fix:])))
    assert rel(V[n_fix:], V6_o[n_fix:]) < 1e-8 and rel(gp[n_fix:], gp_o[n_fix:]) < 1e-6
    st = eng.solve_lm(max_nfev=200, loss="linear")
    x = eng.get_x()
    n_c = p.n_cam * p.n_params
    assert st.status > 0 and st.cost < 0.5 * st.initial_cost
    assert np.array_equal(x[n_c: n_c + 3 * n_fix], v[n_c: n_c + 3 * n_fix])
    moved = np.any((x[n_c:] != v[n_c:]).reshape(-1, 3), axis=1)
    assert moved[n_fix:].all() and not moved[:n_fix].any()
    eng.close()


# ----------------------------------------------------------------------------- 4. the wide route by rule

def rule_params(n_cam, corr):
    p = synth.make_params(tracks_scene("affine", n_cam, 700, 2, 5), {"correction_params": corr, "n_cam_fix": 1})
    assert np.unique(p.cam_ind).size == n_cam  # every camera is observed
    return p


def test_256_cameras_solve_on_the_wide_route(gpu, monkeypatch):
    """satba_solve_lm -- as the handle runs it by its rules, and with the decisions on the host (SATBA_HOST_LOOP) -- against the
    Python loop of satba/trf.py."""
    tol = dict(ftol=1e-4, xtol=1e-10, gtol=1e-8)
    outs = []
    for how in ("python", "native", "native_host_loop"):
        p = rule_params(256, ["R"])
        eng = engine(monkeypatch, p, **({"SATBA_HOST_LOOP": 1} if how == "native_host_loop" else {}))
        assert eng.info()["cam_narrow"] == 0
        res = trf.trf_solve(eng, max_nfev=300, loss="linear", native=(how != "python"), **tol)
        outs.append((res, eng.get_x()))
        eng.close()
    (ra, xa) = outs[0]
    p = rule_params(256, ["R"])
    assert ra.status > 0 and ra.cost < 0.1 * 0.5 * np.sum(ba_core.fun(p.params_opt.copy(), p) ** 2)  # (the solve went somewhere)
    for rb, xb in outs[1:]:
        print("cost {:.17g} vs {:.17g}, nfev {} vs {}".format(ra.cost, rb.cost, ra.nfev, rb.nfev))
        assert ra.nfev == rb.nfev and ra.status == rb.status and ra.njev == rb.njev and ra.iterations == rb.iterations
        assert abs(ra.cost - rb.cost) <= 1e-14 * ra.cost
        assert np.abs(xa - xb).max() <= 1e-12 * np.abs(xa).max()


def test_255_cameras_solve_the_same_on_both_routes(gpu, monkeypatch):
    outs = []
    for narrow in (True, False):
        eng = engine(monkeypatch, rule_params(255, ["R", "T"]), narrow=narrow)
        st = eng.solve_lm(max_nfev=60, loss="linear", ftol=1e-10, xtol=1e-12, gtol=1e-10)
        outs.append(((st.cost, st.nfev, st.njev, st.iterations, st.status, st.optimality, st.initial_cost), eng.get_x()))
        eng.close()
    assert outs[0][0][4] >= 0 and outs[0][0][0] < 0.5 * outs[0][0][6]
    assert outs[0][0] == outs[1][0], (outs[0][0], outs[1][0])
    assert same_bits(outs[0][1], outs[1][1])


# ----------------------------------------------------------------------------- 5. the device-resident loop

@pytest.mark.parametrize("name", ["affine_RT", "affine_RT_weighted_soft_l1"])
def test_device_resident_loop_is_the_same_on_both_routes(gpu, monkeypatch, name):
    loss = FAMILIES[name][2]
    p, v = small_params(name)
    outs = []
    for narrow in (True, False):
        eng = engine(monkeypatch, p, narrow=narrow, SATBA_DEVICE_LOOP=1)
        assert eng.info()["device_loop"] == 1
        eng.set_x(v)
        st = eng.solve_lm(max_nfev=60, loss=loss, ftol=1e-12, xtol=1e-12, gtol=1e-12)
        outs.append(((st.cost, st.nfev, st.njev, st.iterations, st.status, st.optimality, st.initial_cost), eng.get_x()))
        eng.close()
    assert outs[0][0][1] > 3 and outs[0][0][0] < 0.5 * outs[0][0][6]
    assert outs[0][0] == outs[1][0], (outs[0][0], outs[1][0])
    assert same_bits(outs[0][1], outs[1][1])

"""
The five kernels that walk the sliced point list (k_residual and its TRIAL form, k_linearize, k_jvp with one and two vectors,
k_backsub) at every number of lanes per point (SATBA_SPLIT = 0 .. 3) and every replica count of k_linearize's camera-sum table
(SATBA_LIN_REP = 0 .. 4), against the float64 oracle and against each other.  Without the switches the small problems of the suite
all run at sh = 3, rep = 4 (90 cameras: 3), and what bench.py times -- sh = 0 | 1, rep = 2 -- was only reached at full size, where
nothing is compared with float64.  The scenes and the rules restated are in tests/cases_lanes.py, their preconditions in
tests/test_lanes_cases_host.py.  The huber family leaves the fixed-point camera sums on this scene (cameras with clamped rows only:
the header's FX slot, `linearize` below) and is held to float64 on the camera-major sums it falls back to.

Tolerances are those of tests/test_gpu_parity.py: test_phases_match_oracle_engine (headers 1e-7 relative, scale_inv 1e-9, g_h 1e-8,
gn_h 1e-7, q1 1e-8, x_new 1e-12), test_normal_blocks (U, V 1e-8, g_c, g_p 1e-6 of the largest entry; residuals 1e-8 px, RPC without
the float32 store 1e-7 px), test_fun_cost_matches_residual_norm (cost against the residuals: 1e-10, robust 1e-12) and
test_points_with_more_than_64_observations.
"""
import functools

import numpy as np
import pytest

import cases_lanes as CL
from oracle import lm_oracle as L
from satba import ba_core, synth, trf
from satba.engine_hip import HipEngine
from test_gpu_intrinsics import jacobian_blocks_k
from test_gpu_parity import _run_phases, rel

pytestmark = pytest.mark.gpu

SWITCHES = ("SATBA_SPLIT", "SATBA_LIN_REP", "SATBA_DETERMINISTIC", "SATBA_CAM_SUMS", "SATBA_BPC", "SATBA_SLICE_REV", "SATBA_FX_SHRINK")
FIXED_FAMILIES = ("affine_RT", "affine_R", "affine_RT_weighted", "affine_RT_soft_l1", "persp_RT")
GRID = [(name, False) for name in CL.FAMILIES] + [(name, True) for name in FIXED_FAMILIES]
GRID_IDS = [name + ("-fixed" if fixed else "") for name, fixed in GRID]
HDR_FX = 5  # SATBA_HDR_FX (include/satba.h): left by the linearisation when its fixed-point camera sums are void
LAM = 1e-3  # damping of the phase comparisons (tests/test_gpu_parity.py: the reduced system is well conditioned there)


def engine(monkeypatch, p, sh=None, rep=None, rpc_f32=True, unit=None, **env):
    """A handle created under SATBA_SPLIT = sh / SATBA_LIN_REP = rep (None: unset), checked to run at what it was asked for."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(env, SATBA_SPLIT=sh, SATBA_LIN_REP=rep).items():
        if v is not None:
            monkeypatch.setenv(k, str(v))
    eng = HipEngine(p, rpc_f32=rpc_f32)
    info = eng.info()
    n_slices = eng.get_layout("slice_base").size - 1
    assert n_slices == CL.n_slices_of(p.n_pts)
    assert info["lin_rep_shift"] == (CL.rep_rule(p.n_cam, p.n_params) if rep is None else rep), info
    if sh is not None:
        assert info["lanes_log2"] == min(sh, CL.SH_MAX) and info["lin_grid"] == CL.lin_grid(n_slices, min(sh, CL.SH_MAX)), info
    if unit is not None:
        assert info["unit_weights"] == (1 if unit else 0), info
    return eng


def configured(eng, name, v):
    loss, f_scale = CL.FAMILIES[name][2:4]
    eng.configure(loss, f_scale)
    eng.set_x(v)
    return eng


def report(test, eng, extra=""):
    info = eng.info()
    print("{}: (sh, rep) = ({:d}, {:d}), lin_grid {:d}{}".format(test, int(info["lanes_log2"]), int(info["lin_rep_shift"]), int(info["lin_grid"]), extra))


def linearize(eng, name):
    """The linearisation as a caller that drives the phases itself has to run it: when the header's FX slot is raised the fixed-point
    camera sums are void, the handle is switched to the camera-major sums and the linearisation repeated.  Exactly the families of
    cases_lanes.FALLS_BACK do that (cameras whose diag U_c terms all lie under the unit of the fixed-point scale), once."""
    eng.linearize()
    fell = eng.read_header()[HDR_FX] != 0.0
    assert fell == (name in CL.FALLS_BACK), (name, fell)
    if fell:
        assert eng.info()["cam_sums_lds"] == 1 and eng.camera_sums_fallback()
        eng.linearize()
        assert eng.read_header()[HDR_FX] == 0.0 and eng.info()["cam_sums_lds"] == 0
    assert eng.info()["fx_fallbacks"] == (1 if fell else 0)
    return fell


def phases(eng, to_prepare, name=None):
    """name: a device engine of that family (the oracle engine has no routes to switch)."""
    if not to_prepare:
        return _run_phases(eng, LAM)
    out = {}
    if name is None:
        eng.linearize()
    else:
        out["fell_back"] = linearize(eng, name)
        out["diagU"] = lin_payload(eng)[0]
    out["lin"] = eng.read_header()
    eng.prepare(True)
    out["prep"] = eng.read_header()
    return out


def lin_payload(eng):
    """diag U_c (M, n_p) and g_c (M, n_p) as k_linearize's route left them in the exchange payload (call between linearize and prepare)."""
    M, n_p = eng.n_cam, eng.n_p
    pay = eng.get_exchange(eng.hdr, M * n_p * n_p + M * n_p)
    U = pay[: M * n_p * n_p].reshape(M, n_p, n_p)
    return U[:, np.arange(n_p), np.arange(n_p)].copy(), pay[M * n_p * n_p:].reshape(M, n_p).copy()


@functools.lru_cache(maxsize=None)
def oracle(name, fixed=False, near=False):
    """The float64 side of a family, computed once: phases of the oracle engine, its vectors, the normal blocks."""
    loss, f_scale, rpc_f32 = CL.FAMILIES[name][2:5]
    p, v = CL.family_params(name, fixed=fixed, near=near)
    saved = L.jacobian_blocks
    L.jacobian_blocks = jacobian_blocks_k  # (the intrinsics' columns; the oracle's own blocks for every other n_params)
    try:
        ora = configured(L.OracleEngine(p, rpc_f32=rpc_f32), name, v)
        out = {"p": p, "v": v, "phases": phases(ora, name in CL.PHASES_ONLY_TO_PREPARE)}
        for k in ("scale_inv", "g_h", "gn_h", "q1", "x_new"):
            out[k] = None if getattr(ora, k, None) is None else np.array(getattr(ora, k))
        f, cost, fs, Jc, Jp = L.weighted_system(v, p, loss, f_scale, rpc_f32=rpc_f32)
        U, gc, V, gp = L.normal_blocks(fs, Jc, Jp, p)
    finally:
        L.jacobian_blocks = saved
    out.update(f=f, cost=cost, U=U, gc=gc, V6=V[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]], gp=gp)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def check_blocks(eng, o, diagU, gc_pay, U, gc, V, gp):
    n_p = eng.n_p
    assert rel(U, o["U"]) < 1e-8 and rel(V, o["V6"]) < 1e-8, (rel(U, o["U"]), rel(V, o["V6"]))
    assert rel(gc, o["gc"]) < 1e-6 and rel(gp, o["gp"]) < 1e-6, (rel(gc, o["gc"]), rel(gp, o["gp"]))
    assert np.array_equal(gc, gc_pay)
    assert rel(diagU, o["U"][:, np.arange(n_p), np.arange(n_p)]) < 1e-8  # what the solver itself uses of U


# ----------------------------------------------------------------------------- A. phases against the oracle engine

@pytest.mark.parametrize("sh", [0, 1, 2, 3])
@pytest.mark.parametrize("name,fixed", GRID, ids=GRID_IDS)
def test_phases_at_every_lanes_per_point(gpu, monkeypatch, name, fixed, sh):
    o = oracle(name, fixed, near=name in CL.NEAR_IN_PHASES)  # (the bound on x_new: cases_lanes.py section B)
    p, b = o["p"], o["phases"]
    short = name in CL.PHASES_ONLY_TO_PREPARE
    dev = configured(engine(monkeypatch, p, sh=sh, rpc_f32=CL.FAMILIES[name][4], unit=bool(np.all(p.pts2d_w == 1.0))), name, o["v"])
    assert dev.info()["cam_sums_lds"] == 1
    report("phases {}{}".format(name, " fixed" if fixed else ""), dev)
    a = phases(dev, short, name)
    assert a["lin"][HDR_FX] == 0.0 and short == (name in CL.FALLS_BACK)
    if short:  # what the prepare phase scales by: the sums of the route the handle fell back to, entry by entry of the largest
        n_p = dev.n_p
        print("  fell back: {}, diag U_c {:.3g}".format(a["fell_back"], rel(a["diagU"], o["U"][:, np.arange(n_p), np.arange(n_p)])))
        assert a["fell_back"] and rel(a["diagU"], o["U"][:, np.arange(n_p), np.arange(n_p)]) < 1e-8
    checks = [("lin", [trf.COST, dev.HDR_FIXED]), ("prep", [trf.GH_SQ, trf.JG_SQ, trf.XS_SQ, trf.GC_INF])]
    if not short:
        assert abs(a["natural_lam"] - b["natural_lam"]) < 1e-7 * b["natural_lam"]
        checks += [("solve", [trf.GRAM_A, trf.GRAM_B, trf.GRAM_C, trf.CHOL_FAIL]), ("sub", [trf.WW]), ("prod", [trf.B11, trf.B12, trf.B22]),
                   ("trial", [trf.COST_NEW, trf.STEP_SQ, trf.X_SQ])]
    for phase, slots in checks:
        for s in slots:
            print("  {} [{}] {:.17g} oracle {:.17g}".format(phase, s, a[phase][s], b[phase][s]))
            assert abs(a[phase][s] - b[phase][s]) <= 1e-7 * abs(b[phase][s]) + 1e-300, (phase, s, a[phase][s], b[phase][s])
    tols = {"scale_inv": 1e-9, "g_h": 1e-8} if short else {"scale_inv": 1e-9, "g_h": 1e-8, "gn_h": 1e-7, "q1": 1e-8, "x_new": 1e-12}
    for k, tol in tols.items():
        err = rel(dev.get_vector(k), o[k])
        print("  {} {:.3g} (bound {:g})".format(k, err, tol))
        assert err < tol, (k, err)
    if fixed and not short:
        gn = dev.get_vector("gn_h")
        assert np.all(gn[: 2 * dev.n_p] == 0.0) and np.all(gn[dev.n_c: dev.n_c + 27] == 0.0)  # frozen cameras / points do not move
    dev.close()


# ----------------------------------------------------------------------------- B. blocks against float64

@pytest.mark.parametrize("sh", [0, 1, 2, 3])
@pytest.mark.parametrize("name,fixed", GRID, ids=GRID_IDS)
def test_blocks_at_every_lanes_per_point(gpu, monkeypatch, name, fixed, sh):
    o = oracle(name, fixed)
    p = o["p"]
    loss, f_scale, rpc_f32 = CL.FAMILIES[name][2:5]
    dev = configured(engine(monkeypatch, p, sh=sh, rpc_f32=rpc_f32), name, o["v"])
    report("blocks {}{}".format(name, " fixed" if fixed else ""), dev)
    linearize(dev, name)
    diagU, gc_pay = lin_payload(dev)
    check_blocks(dev, o, diagU, gc_pay, *dev.get_blocks())
    r, cost = dev.residuals(with_cost=True)
    assert np.abs(r - o["f"]).max() < (1e-8 if rpc_f32 or p.cam_model != "rpc" else 1e-7)
    assert abs(cost - L.robust_cost(r, loss, f_scale)) < (1e-10 if loss == "linear" else 1e-12) * cost
    dev.close()


# ----------------------------------------------------------------------------- C. replicas of the camera-sum table

@pytest.mark.parametrize("sh", [0, 3])
@pytest.mark.parametrize("name", CL.REPLICA_FAMILIES)
def test_camera_sums_at_every_replica_count(gpu, monkeypatch, name, sh):
    """The sums are integers: every replica count gives the same bits, and they are the oracle's to the tolerance of the blocks."""
    o = oracle(name)
    got = []
    for rep in range(CL.REP_MAX + 1):
        dev = configured(engine(monkeypatch, o["p"], sh=sh, rep=rep), name, o["v"])
        assert dev.info()["cam_sums_lds"] == 1
        report("replicas {}".format(name), dev)
        linearize(dev, name)
        got.append(lin_payload(dev))
        check_blocks(dev, o, *got[-1], *dev.get_blocks())
        assert dev.info()["fx_fallbacks"] == 0
        dev.close()
    for rep in range(1, CL.REP_MAX + 1):
        assert np.array_equal(got[rep][0], got[0][0]) and np.array_equal(got[rep][1], got[0][1]), rep


# ----------------------------------------------------------------------------- D. camera sums across the lanes per point

@pytest.mark.parametrize("name", list(CL.FAMILIES))
def test_camera_sums_do_not_depend_on_the_lanes_per_point(gpu, monkeypatch, name):
    """Integer addition does not care which lane adds: diag U_c and g_c of the fixed-point route are the same bits at sh = 0 .. 3
    (the exponents come from bounds that see the cost after rounding to a power of two).  V and g_p change with the order of the
    xor-shuffles: to the oracle's tolerance only -- as do the camera sums of a family that leaves the fixed-point route
    (cases_lanes.FALLS_BACK: float64 sums of the camera-major pass), which falls back at every sh."""
    o = oracle(name)
    got = []
    n_p = o["p"].n_params
    for sh in range(4):
        dev = configured(engine(monkeypatch, o["p"], sh=sh, rpc_f32=CL.FAMILIES[name][4]), name, o["v"])
        assert dev.info()["cam_sums_lds"] == 1
        report("across sh {}".format(name), dev)
        linearize(dev, name)
        got.append(lin_payload(dev))
        _, _, V, gp = dev.get_blocks()
        assert rel(V, o["V6"]) < 1e-8 and rel(gp, o["gp"]) < 1e-6
        assert rel(got[-1][0], o["U"][:, np.arange(n_p), np.arange(n_p)]) < 1e-8 and rel(got[-1][1], o["gc"]) < 1e-6
        dev.close()
    for sh in range(1, 4):
        print("  sh {} vs 0: diag U_c {:.3g}, g_c {:.3g}".format(sh, rel(got[sh][0], got[0][0]), rel(got[sh][1], got[0][1])))
    for sh in range(1, 4):
        assert name in CL.FALLS_BACK or (np.array_equal(got[sh][0], got[0][0]) and np.array_equal(got[sh][1], got[0][1])), sh


# ----------------------------------------------------------------------------- E. tracks longer than a wavefront

@functools.lru_cache(maxsize=None)
def long_oracle():
    p = synth.make_params(CL.long_scene(), {"correction_params": ["R", "T"], "n_cam_fix": 1})
    assert np.bincount(p.pts_ind).max() > 64
    ora = L.OracleEngine(p)
    ora.configure("linear", 1.0)
    ora.set_x(p.params_opt.copy())
    return p, _run_phases(ora, LAM), np.array(ora.gn_h)


@pytest.mark.parametrize("sh", [0, 1, 2])
def test_long_tracks_at_fewer_lanes(gpu, monkeypatch, sh):
    """test_points_with_more_than_64_observations (which runs at sh = 3) at one, two and four lanes per point; three replicas."""
    p, b, gn_o = long_oracle()
    dev = engine(monkeypatch, p, sh=sh)
    assert dev.info()["lin_rep_shift"] == 3
    report("long tracks", dev)
    dev.configure("linear", 1.0)
    dev.set_x(p.params_opt.copy())
    a = _run_phases(dev, LAM)
    for phase, slots in (("lin", [trf.COST, dev.HDR_FIXED]), ("prep", [trf.GH_SQ, trf.JG_SQ]),
                         ("solve", [trf.GRAM_A, trf.GRAM_B, trf.GRAM_C]), ("sub", [trf.WW]), ("prod", [trf.B11, trf.B12, trf.B22])):
        for s in slots:
            assert abs(a[phase][s] - b[phase][s]) <= 1e-7 * abs(b[phase][s]), (phase, s)
    assert rel(dev.get_vector("gn_h"), gn_o) < 1e-6
    dev.close()


# ----------------------------------------------------------------------------- F. the second round of the walk

def _walk(eng, v):
    """Linearise, then everything of the iteration that does not need the camera step."""
    eng.configure("linear", 1.0)
    eng.set_x(v)
    eng.linearize()
    out = {"cost": eng.read_header()[trf.COST]}
    out["diagU"], out["gc"] = lin_payload(eng)
    _, _, out["V"], out["gp"] = eng.get_blocks()
    eng.prepare(True)
    eng.schur(LAM)  # (the damped inverses of the point blocks for the back-substitution)
    out["s"] = eng.get_vector("scale_inv")[: eng.n_c]
    return out


def _step(eng, out, r):
    """The camera step of cases_lanes.exact_rhs through the solve phase, then a trial point along (g_h, gn_h)."""
    s, n_c = out["s"], eng.n_c
    eng.set_exchange(eng.hdr, np.diag(s * s).ravel())
    eng.set_exchange(eng.hdr + n_c * n_c, r)
    eng.solve()
    out["gn_h"] = eng.get_vector("gn_h")
    assert eng.read_header()[trf.CHOL_FAIL] == 0
    eng.trial_gn(-0.25, -0.5)
    out["cost_new"] = eng.read_header()[trf.COST_NEW]
    out["x_new"] = eng.get_vector("x_new")


def test_second_round_of_the_walk_gives_every_point_the_same_bits(gpu, monkeypatch):
    """61 copies of a 1 088-point scene at eight lanes per point: 8 296 units on 4 096 waves, a second round of 52.  A point's lanes and
    the order of their sums do not depend on where its slice sits in the walk, so V, g_p, the point part of gn_h (for the same camera
    step) and of the trial point are, copy by copy, the bits of the scene run alone -- which test_phases_at_every_lanes_per_point
    holds against float64.  The camera sums and the costs are 61 times the scene's to 1e-12 (other exponents: no bits)."""
    base_scene = CL.rounds_base_scene()
    T, N = CL.ROUNDS_TILES, base_scene.n_pts
    opts = {"correction_params": ["R", "T"], "n_cam_fix": 1, "reduce": False}
    pb, pt = synth.make_params(base_scene, opts), synth.make_params(CL.tiled_scene(base_scene, T), opts)
    n_c = pb.n_cam * pb.n_params
    rng = np.random.default_rng(11)
    vb = ba_core._frozen_vars(pb.params_opt + 1e-6 * rng.standard_normal(pb.params_opt.size) * np.abs(pb.params_opt).clip(1.0), pb)
    vt = np.concatenate((vb[:n_c], np.tile(vb[n_c:], T)))
    eb, et = engine(monkeypatch, pb, sh=CL.ROUNDS_SH, unit=True), engine(monkeypatch, pt, sh=CL.ROUNDS_SH, unit=True)
    n_slices = CL.n_slices_of(pt.n_pts)
    assert et.info()["lin_grid"] == CL.lin_grid(n_slices, CL.ROUNDS_SH) == 256
    assert CL.walk_rounds(n_slices << CL.ROUNDS_SH, 4096) == (2, 52) and CL.walk_rounds(CL.n_slices_of(N) << CL.ROUNDS_SH, 17 * 8)[0] == 1
    report("second round, the scene", eb)
    report("second round, {} copies".format(T), et)
    b, t = _walk(eb, vb), _walk(et, vt)
    d, (rb, rt) = CL.exact_rhs(1e-7 * rng.standard_normal(n_c) * np.abs(vb[:n_c]).clip(1.0), [b["s"], t["s"]])
    _step(eb, b, rb)
    _step(et, t, rt)
    for o, r in ((b, rb), (t, rt)):  # the solve was exact: both handles back-substitute the same camera step d
        assert np.array_equal(o["gn_h"][:n_c], r / o["s"]) and np.array_equal(o["gn_h"][:n_c] / o["s"], d)
    for k, width in (("V", 6), ("gp", 3)):
        assert t[k].shape == (T * N, width) and np.array_equal(t[k].reshape(T, N, width), np.broadcast_to(b[k], (T, N, width))), k
    for k in ("gn_h", "x_new"):
        assert np.any(b[k][n_c:] != 0.0)
        assert np.array_equal(t[k][n_c:].reshape(T, 3 * N), np.broadcast_to(b[k][n_c:], (T, 3 * N))), k
    assert np.any(b["x_new"][n_c:] != vb[n_c:])
    for k in ("diagU", "gc"):
        print("  {}: {:.3g}".format(k, rel(t[k], T * b[k])))
        assert rel(t[k], T * b[k]) <= 1e-12, k
    for k in ("cost", "cost_new"):
        print("  {}: {:.17g} vs {} x {:.17g}".format(k, t[k], T, b[k]))
        assert abs(t[k] - T * b[k]) <= 1e-12 * T * b[k], k
    eb.close()
    et.close()


# ----------------------------------------------------------------------------- G. the rule itself

def test_rule_on_a_small_problem(gpu, monkeypatch):
    p, v = CL.family_params("affine_RT")
    dev = engine(monkeypatch, p, unit=True)
    info = dev.info()
    report("rule, small", dev)
    assert info["lanes_log2"] == 3 == CL.size_rule(3) and info["lin_rep_shift"] == 4 and info["lin_grid"] == CL.lin_grid(3, 3) == 2
    dev.close()
    dev = engine(monkeypatch, p, SATBA_DETERMINISTIC=1)
    report("rule, deterministic", dev)
    assert dev.info()["deterministic"] == 1 and dev.info()["lanes_log2"] == 0 and dev.info()["lin_grid"] == CL.lin_grid(3, 0) == 1
    dev.configure("soft_l1", 1.0)  # the repeatability option comes before "two lanes for robust runs"
    assert dev.info()["lanes_log2"] == 0
    dev.close()
    dev = engine(monkeypatch, p, sh=7, SATBA_DETERMINISTIC=1)  # the switch wins and is clamped
    report("rule, deterministic, SATBA_SPLIT=7", dev)
    assert dev.info()["lanes_log2"] == 3
    dev.close()


@pytest.mark.parametrize("n_slices,sh", [(749, 3), (750, 2)])
def test_rule_at_the_threshold_of_four_lanes(gpu, monkeypatch, n_slices, sh):
    scene = CL.rule_scene((n_slices - 1) * 64 + 1)
    p = synth.make_params(scene, {"correction_params": ["R"], "n_cam_fix": 1})
    dev = engine(monkeypatch, p, unit=True)
    report("rule, {} slices".format(n_slices), dev)
    assert dev.get_layout("slice_base").size - 1 == n_slices and (n_slices << 2 >= CL.SIZE_RULE_UNITS) == (sh == 2)
    assert dev.info()["lanes_log2"] == sh == CL.size_rule(n_slices)
    assert dev.info()["lin_grid"] == CL.lin_grid(n_slices, sh)
    dev.close()


def test_rule_follows_the_configured_loss(gpu, monkeypatch):
    """One lane per point from 3 000 slices on -- unless the run is weighted or robust: a handle created for the linear loss and
    configured for soft_l1 afterwards runs at two lanes, and k_linearize's grid follows (it once kept the grid of one lane)."""
    n_slices = CL.SIZE_RULE_UNITS
    scene = CL.rule_scene((n_slices - 1) * 64 + 1)
    p = synth.make_params(scene, {"correction_params": ["R"], "n_cam_fix": 1})
    dev = engine(monkeypatch, p, unit=True)
    report("rule, linear", dev)
    assert dev.get_layout("slice_base").size - 1 == n_slices
    assert dev.info()["lanes_log2"] == 0 == CL.size_rule(n_slices) and dev.info()["lin_grid"] == CL.lin_grid(n_slices, 0) == 188
    dev.configure("soft_l1", 1.0)
    report("rule, soft_l1", dev)
    assert dev.info()["lanes_log2"] == 1 == CL.size_rule(n_slices, unit_run=False) and dev.info()["lin_grid"] == CL.lin_grid(n_slices, 1) == 256
    dev.configure("linear", 1.0)
    assert dev.info()["lanes_log2"] == 0 and dev.info()["lin_grid"] == 188
    dev.close()

"""
Refinement of the intrinsics (n_params 8 affine, 11 perspective) on the device: residuals, Jacobian blocks, normal blocks and
the reduced camera system against the reference's goldens (tests/golden/fun_*_RTK.npz) and a numpy restatement of the K
columns; end-to-end solves, repeatability and the two loops.
"""
import numpy as np
import pytest

import cases_intrinsics as CI
from oracle import lm_oracle as L
from satba import ba_core, synth, trf
from satba.engine_hip import HipEngine

pytestmark = pytest.mark.gpu
LOSSES = ["linear", "soft_l1", "huber", "cauchy", "arctan"]


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def jacobian_blocks_k(v, p, _base=L.jacobian_blocks):
    """The oracle's blocks with the intrinsics' columns appended (affine (q0, 0, q1 | 0, q1, 0), perspective (q0, 0, q1, q2, 0 | ...) / q2)."""
    n_p = p.n_params
    if n_p not in (8, 11):
        return _base(v, p)
    pts3d, cam_params = p.get_vars_ready_for_fun(v.copy())
    cp = cam_params[p.cam_ind]
    q = ba_core.rotate_euler(pts3d[p.pts_ind], cp[:, :3])
    # the R+T blocks of the oracle at the same cameras: K (and the frozen rows) come from the unpacked rows, not from the start
    saved, saved_cp = p.n_params, p.cam_params
    p.n_params, p.cam_params = (5 if n_p == 8 else 6), cam_params
    try:
        v_rt = np.hstack((cam_params[:, : p.n_params].ravel(), v[saved * p.n_cam:]))
        proj, Jc, Jp = _base(v_rt, p)
    finally:
        p.n_params, p.cam_params = saved, saved_cp
    K = q.shape[0]
    if n_p == 8:
        q = q[:, :2] + cp[:, 3:5]
        Jk = np.zeros((K, 2, 3))
        Jk[:, 0, 0], Jk[:, 0, 2], Jk[:, 1, 1] = q[:, 0], q[:, 1], q[:, 1]
    else:
        q = q + cp[:, 3:6]
        Jk = np.zeros((K, 2, 5))
        Jk[:, 0, 0], Jk[:, 0, 2], Jk[:, 0, 3] = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2], 1.0
        Jk[:, 1, 1], Jk[:, 1, 4] = q[:, 1] / q[:, 2], 1.0
    return proj, np.concatenate((Jc, Jk), axis=2), Jp


@pytest.fixture
def koracle(monkeypatch):
    monkeypatch.setattr(L, "jacobian_blocks", jacobian_blocks_k)
    return L


def fun_case(name):
    return synth.make_params(CI.scene(name), CI.options(name), dense=True), CI.golden("fun_" + name)


@pytest.mark.parametrize("name", list(CI.FUN_CASES))
def test_residuals_match_reference(gpu, name):
    p, g = fun_case(name)
    for v, r in zip(g["v"], g["r"]):
        assert np.abs(ba_core.fun(v.copy(), p) - r).max() < 1e-8


@pytest.mark.parametrize("name", list(CI.FUN_CASES))
@pytest.mark.parametrize("loss", LOSSES)
def test_jacobian_blocks(gpu, koracle, name, loss):
    p, g = fun_case(name)
    v = ba_core._frozen_vars(g["v"][1].copy(), p)
    eng = HipEngine(p)
    eng.configure(loss, 1.0)
    eng.set_x(v)
    eng.linearize()
    Jc, Jp = eng.get_jacobian()
    _, _, _, Jc_o, Jp_o = koracle.weighted_system(v, p, loss, 1.0)
    assert rel(Jc, Jc_o) < 1e-8 and rel(Jp, Jp_o) < 1e-8
    if loss == "linear":  # 3-point differences of the reference's own fun (frozen columns are zero on the device)
        mc = (p.cam_ind >= p.n_cam_fix)[:, None, None]
        mp = (p.pts_ind >= p.n_pts_fix)[:, None, None]
        assert rel(Jc, g["Jc"] * mc) < 1e-6 and rel(Jp, g["Jp"] * mp) < 1e-6
    eng.close()


@pytest.mark.parametrize("name", list(CI.FUN_CASES))
@pytest.mark.parametrize("loss", ["linear", "soft_l1"])
def test_normal_blocks(gpu, koracle, name, loss):
    p, g = fun_case(name)
    v = ba_core._frozen_vars(g["v"][2].copy(), p)
    eng = HipEngine(p)
    eng.configure(loss, 1.0)
    eng.set_x(v)
    eng.linearize()
    U, gc, V, gp = eng.get_blocks()
    f, cost, fs, Jc, Jp = koracle.weighted_system(v, p, loss, 1.0)
    U_o, gc_o, V_o, gp_o = koracle.normal_blocks(fs, Jc, Jp, p)
    V_o6 = V_o[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]
    assert rel(U, U_o) < 1e-8 and rel(V, V_o6) < 1e-8
    assert rel(gc, gc_o) < 1e-6 and rel(gp, gp_o) < 1e-6
    assert abs(eng.read_header()[trf.COST] - cost) < 1e-6 * cost
    eng.close()


def _schur_case(name):
    if name in CI.FUN_CASES:
        p = fun_case(name)[0]
        return p, ba_core._frozen_vars(CI.golden("fun_" + name)["v"][1].copy(), p)
    # past the LDS tables: 120 perspective cameras, 1320 unknowns in the reduced system
    sc = synth.make_scene("perspective", 120, 3000, 6, seed=4, sigma_k=1e-3)
    p = synth.make_params(sc, {"correction_params": ["R", "T", "K"], "K_init": "camera", "n_cam_fix": 1})
    return p, p.params_opt.copy()


@pytest.mark.parametrize("name", list(CI.FUN_CASES) + ["persp_120"])
@pytest.mark.parametrize("loss", ["linear", "soft_l1"])
def test_schur_matrix_and_rhs(gpu, koracle, name, loss):
    p, v = _schur_case(name)
    dev, ora = HipEngine(p), koracle.OracleEngine(p)
    for e in (dev, ora):
        e.configure(loss, 1.0)
        e.set_x(v)
        e.linearize()
        e.prepare(True)
        e.schur(0.37)
    n_c = dev.n_c
    S = dev.get_exchange(dev.hdr, n_c * n_c).reshape(n_c, n_c).T
    rhs = dev.get_exchange(dev.hdr + n_c * n_c, n_c)
    S_o = ora._xb[ora.hdr: ora.hdr + n_c * n_c].reshape(n_c, n_c)
    rhs_o = ora._xb[ora.hdr + n_c * n_c: ora.len_schur]
    low = np.tril_indices(n_c)
    assert rel(S[low], S_o[low]) < 1e-9
    assert rel(rhs, rhs_o) < 1e-9
    dev.close()


def _k_scene(model, seed=2):
    sc = synth.make_scene(model, 8, 2000, 5, seed=seed, sigma_k=1e-2 if model == "affine" else 2e-3)
    return sc, synth.make_params(sc, {"correction_params": ["R", "T", "K"], "K_init": "camera", "n_cam_fix": 1, "n_pts_fix": 30})


def _k_err(p, cameras, cams_true):
    from satba import ba_params

    n0 = p.n_params - (3 if p.cam_model == "affine" else 5)
    e = []
    for c, t in zip(cameras[p.n_cam_fix:], cams_true[p.n_cam_fix:]):
        a = ba_params.load_cam_params_from_camera(c, np.zeros(3), p.cam_model)[n0:]
        b = ba_params.load_cam_params_from_camera(t, np.zeros(3), p.cam_model)[n0:]
        e.append(np.abs(a - b) / np.maximum(np.abs(b), 1.0))
    return np.mean(e)


@pytest.mark.parametrize("model", ["affine", "perspective"])
def test_end_to_end_solve_with_k_error(gpu, model):
    sc, p = _k_scene(model)
    out = ba_core.run_ba_optimization(p, {"loss": "linear", "verbose": 0, "max_iter": 200}, False, False)
    vars_init, vars_ba, err_init, err_ba = out[:4]
    assert err_ba.mean() < 0.5 * err_init.mean()
    if model == "affine":
        # (perspective cameras 600 km away from a 10 km scene: the focal lengths trade against the distance along the optical axis --
        # the intrinsics are not identifiable there, only the reprojection error is compared)
        _, cams = p.reconstruct_vars(vars_ba.copy(), p.pts3d.copy(), list(p.cameras))
        assert _k_err(p, cams, sc.cameras_true) < _k_err(p, p.cameras, sc.cameras_true)


def _solve_stats(st):
    return (st.cost, st.nfev, st.njev, st.iterations, st.status, st.optimality, st.initial_cost)


@pytest.mark.parametrize("model", ["affine", "perspective"])
@pytest.mark.parametrize("loss", ["linear", "soft_l1"])
def test_runs_repeat_bitwise_and_loops_agree(gpu, monkeypatch, model, loss):
    """Two device-resident solves repeat bit for bit; the same solve with the decisions on the host (SATBA_HOST_LOOP) is identical."""
    sc, _ = _k_scene(model, seed=3)
    outs = []
    for host in (False, False, True):
        if host:
            monkeypatch.setenv("SATBA_HOST_LOOP", "1")
        eng = HipEngine(synth.make_params(sc, {"correction_params": ["R", "T", "K"], "K_init": "camera", "n_cam_fix": 1, "n_pts_fix": 30}))
        st = eng.solve_lm(max_nfev=40, loss=loss, ftol=1e-12, xtol=1e-12, gtol=1e-12)
        outs.append((_solve_stats(st), eng.get_x()))
        eng.close()
    assert outs[0][0] == outs[1][0] == outs[2][0]
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][1], outs[2][1])
    assert outs[0][0][0] < outs[0][0][6]


@pytest.mark.parametrize("model,M,N,opp", [("perspective", 30, 3000, 5), ("affine", 24, 3000, 6)])
@pytest.mark.parametrize("loop,loss", [("host", "linear"), ("device", "linear"), ("host", "soft_l1"), ("device", "soft_l1")])
def test_factorisation_beside_the_pair_kernel_is_the_sequential_solve(gpu, monkeypatch, model, M, N, opp, loop, loss):
    """
    The factorisation beside the pair kernel (n_c 330 / 192: more than two tile columns) takes every tile when the producers of its
    columns have counted themselves in -- at NP = 11 through the wide epilogue of the pair items (passes of 64 totals), at NP = 8 / 11 in
    soft_l1 through the diagonal items in passes of 64.  Same arithmetic in the same order as the sequential front (SATBA_CHOL_BESIDE=0):
    identical to the last bit, in both loops.
    """
    scene = synth.make_scene(model, M, N, opp, seed=11, sigma_k=1e-3)
    if loop == "host":
        monkeypatch.setenv("SATBA_HOST_LOOP", "1")
    monkeypatch.setenv("SATBA_SCHUR_MERGE", "1")
    outs = []
    for beside in ("1", "0", "1"):
        monkeypatch.setenv("SATBA_CHOL_BESIDE", beside)
        eng = HipEngine(synth.make_params(scene, {"correction_params": ["R", "T", "K"], "K_init": "camera", "n_cam_fix": 1, "n_pts_fix": 20}))
        assert eng.n_c > 128
        st = eng.solve_lm(max_nfev=30, loss=loss, ftol=1e-12, xtol=1e-12, gtol=1e-12)
        outs.append((_solve_stats(st), eng.get_x()))
        assert int(eng.info()["chol_beside"]) == int(beside)
        eng.close()
    assert outs[0][0] == outs[1][0] == outs[2][0]
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][1], outs[2][1])
    assert outs[0][0][0] < 0.5 * outs[0][0][6]


@pytest.mark.parametrize("model", ["affine", "perspective"])
@pytest.mark.parametrize("native", [True, False])
def test_fixed_point_overflow_falls_back_to_camera_major_sums(gpu, monkeypatch, model, native):
    """
    The range check of k_linearize's fixed-point camera sums at NP = 8 / 11: SATBA_FX_SHRINK makes the bounds 1e9 times too small, a term
    beyond its bound raises K_FX_BAD, the loop switches the handle to the camera-major sums and repeats the iteration -- and ends where
    the run without the overflow ends.
    """
    sc, _ = _k_scene(model, seed=4)
    opts = {"correction_params": ["R", "T", "K"], "K_init": "camera", "n_cam_fix": 1, "n_pts_fix": 30}
    kw = dict(ftol=1e-12, xtol=1e-12, gtol=1e-12, max_nfev=40, loss="linear")
    ref = HipEngine(synth.make_params(sc, opts))
    res_ref = trf.trf_solve(ref, native=native, **kw)
    x_ref = ref.get_x()
    assert ref.info()["fx_fallbacks"] == 0
    ref.close()
    monkeypatch.setenv("SATBA_FX_SHRINK", "1e-9")
    eng = HipEngine(synth.make_params(sc, opts))
    assert eng.info()["cam_sums_lds"] == 1
    res = trf.trf_solve(eng, native=native, **kw)
    info = eng.info()
    assert info["fx_fallbacks"] == 1 and info["cam_sums_lds"] == 0
    # (the two routes differ in the order of their sums.  The perspective intrinsics trade against the distance along the optical axis
    # -- a flat valley that 40 evaluations do not leave (status 0, max_nfev) --, and there rounding-level differences grow to 3e-8 of
    # the cost; the affine solve ends where the reference run ends to 1e-10)
    tol = (1e-10, 1e-8) if model == "affine" else (1e-6, 1e-6)
    assert res.status == res_ref.status and abs(res.cost - res_ref.cost) < tol[0] * res_ref.cost
    assert np.abs(eng.get_x() - x_ref).max() < tol[1] * np.abs(x_ref).max()
    eng.close()


# ----------------------------------------------------------------------------- against the reference's own solves

@pytest.mark.parametrize("name", list(CI.SOLVE_CASES))
@pytest.mark.parametrize("route", ["default", "camera_major"])
def test_tight_solve_matches_reference(gpu, monkeypatch, name, route):
    """
    The reference's least_squares from the corrected start under the tight3 protocol (tools/gen_golden_intrinsics.py): cost to 1e-9;
    linear loss: residual vector to 1e-6 of its norm and camera parameters to 1e-6 where the gauge is fixed (one frozen camera and 8
    frozen points).  soft_l1: the reference's run stops on xtol at optimality 1e2 -- not a stationary point: this solver ends at the
    same cost (5e-11), 1.7e-5 of |f| away along a flat direction; the residual vector is compared at 1e-4.
    """
    if route == "camera_major":
        monkeypatch.setenv("SATBA_DETERMINISTIC", "1")
    g = CI.golden("solve_intrinsics")
    for loss in CI.SOLVE_CASES[name][7]:
        p = synth.make_params(CI.scene(name), CI.options(name))
        key = name + "_" + loss
        assert np.allclose(p.params_opt, g["x0_" + key], rtol=1e-13, atol=0)
        out = ba_core.run_ba_optimization(p, {"loss": loss, "ftol": 1e-15, "xtol": 1e-15, "gtol": 1e-15, "max_iter": 300,
                                              "verbose": 0, "return_result": True}, False, False)
        vars_ba, res = out[1], out[5]
        x3, f3, s3 = g["x_" + key], g["fun_" + key], g["stats_" + key]
        assert res.status in (2, 3, 4)
        assert abs(res.cost - s3[0]) < 1e-9 * s3[0], (res.cost, s3[0])
        ftol_ = 1e-6 if loss == "linear" else 1e-4
        assert np.linalg.norm(res.fun - f3) < ftol_ * np.linalg.norm(f3), np.linalg.norm(res.fun - f3) / np.linalg.norm(f3)
        if name not in CI.GAUGE_FREE_CASES and loss == "linear":
            n_c = p.n_cam * p.n_params
            assert rel(vars_ba[:n_c], x3[:n_c]) < 1e-6, rel(vars_ba[:n_c], x3[:n_c])


def _two_rank_k_worker(rank, world, port, model, loss, out_dir):
    import os
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(os.path.dirname(here), "sat-bundleadjust_amd"), os.path.dirname(here), here]
    import torch
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from satba import sharding as sh, synth as sy, trf as tr
    from satba.engine_hip import HipEngine as Eng

    sc = sy.make_scene(model, 12, 3000, 5, seed=11, sigma_k=1e-3)
    p = sy.make_params(sc, {"correction_params": ["R", "T", "K"], "K_init": "camera", "n_cam_fix": 1, "n_pts_fix": 20})
    comm = tr.TorchComm()
    shard = sh.make_shard(p, comm.rank, comm.world)
    eng = Eng(p, shard)
    res = tr.trf_solve(eng, comm, loss=loss, ftol=1e-12, xtol=1e-12, gtol=1e-12, max_nfev=40)
    x = sh.assemble_x(p, shard, eng.get_x(), comm)
    r = sh.assemble_residuals(p, shard, eng.residuals(), comm)
    np.savez(os.path.join(out_dir, "rank{}.npz".format(rank)), x=x, r=r, cost=res.cost, nfev=res.nfev, status=res.status)
    eng.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("model", ["affine", "perspective"])
@pytest.mark.parametrize("loss", ["linear", "soft_l1"])
def test_two_ranks_on_one_gpu(gpu, tmp_path, model, loss):
    """Two processes share this GPU, each with one shard of the points, the exchange (NP = 8 / 11 camera blocks) all-reduced over
    gloo: both ranks end on the same point, and where one rank ends (the sums differ in their order only)."""
    import socket

    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_two_rank_k_worker, args=(2, port, model, loss, str(tmp_path)), nprocs=2, join=True)
    outs = [np.load(str(tmp_path / "rank{}.npz".format(r))) for r in range(2)]
    assert np.array_equal(outs[0]["x"], outs[1]["x"]) and int(outs[0]["nfev"]) == int(outs[1]["nfev"])
    sc = synth.make_scene(model, 12, 3000, 5, seed=11, sigma_k=1e-3)
    p = synth.make_params(sc, {"correction_params": ["R", "T", "K"], "K_init": "camera", "n_cam_fix": 1, "n_pts_fix": 20})
    eng = HipEngine(p)
    res = trf.trf_solve(eng, loss=loss, ftol=1e-12, xtol=1e-12, gtol=1e-12, max_nfev=40)
    f1 = eng.residuals()
    eng.close()
    # (two shards sum the camera blocks in another order than one; 40 evaluations end inside the flat valleys of these R+T+K problems
    # (status 0), where such differences have grown to 1e-6 of the cost: a wrong exchange is off by orders of magnitude more)
    assert int(outs[0]["nfev"]) == res.nfev
    assert abs(float(outs[0]["cost"]) - res.cost) < 1e-5 * res.cost
    assert np.linalg.norm(outs[0]["r"] - f1) < 1e-3 * np.linalg.norm(f1)
    assert float(outs[0]["cost"]) < 0.1 * res.initial_cost

"""
The linearisation of the single-rank loops and its readers (issue "fold x <- x_new into k_linearize; form g_h in its readers").

What is built: on the default route of the single-rank loops k_linearize no longer stores g_h and g_h / scale_inv of the points; k_backsub,
the trial's k_residual, k_jvp<PRE> and k_subspace_vec form them from g and scale_inv (csrc/satba_kernels.h: point_gh, point_ghs).  The
accept copy folded into k_linearize was built, measured and taken out again (docs/experiments/accept_in_linearize.diff,
profiles/accept_in_linearize_ab.txt); the cases written for it -- rejected trials, fixed-work runs with restarts, termination straight after
an accepted step, get_x / snapshot_x between runs, several ranks, the host loop -- stay: they hold the device-resident loop and the
loop with the decisions on the host together at every point where the current point changes hands.

Every comparison is BITWISE: the device-resident loop against the loop with the decisions on the host (SATBA_HOST_LOOP, or satba_lm_step
for the fixed-work runs), and the readers' g_h against the stored one (SATBA_STORE_GH=1): same operations on the same operands.
"""
import os
import socket

import numpy as np
import pytest

import cases
from oracle import lm_oracle
from satba import synth, trf
from satba.engine_hip import HipEngine

RT = {"correction_params": ["R", "T"], "n_cam_fix": 1}
TIGHT = dict(ftol=1e-12, xtol=1e-12, gtol=1e-12)
# (cameras, points, observations per point): one slice unit per wave / several workgroups, neither a multiple of the 64-point slice
SHAPES = {"6x300": (6, 300, 6), "12x2000": (12, 2000, 8)}


def affine_rt(shape, seed=3, sigma_theta=2e-5):
    M, N, opp = SHAPES[shape]
    scene = synth.make_affine_scene(M, N, opp, seed=seed, sigma_theta=sigma_theta)
    return lambda: synth.make_params(scene, RT)


def stats(st):
    return (st.cost, st.nfev, st.njev, st.iterations, st.status, st.optimality, st.initial_cost)


def solve_both_loops(monkeypatch, make_p, env=None, **kw):
    """satba_solve_lm on the device-resident loop and with the decisions on the host: [(stats, x, ticks)] * 2."""
    outs = []
    for host in (False, True):
        monkeypatch.delenv("SATBA_HOST_LOOP", raising=False)
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        if host:
            monkeypatch.setenv("SATBA_HOST_LOOP", "1")
        eng = HipEngine(make_p())
        st = eng.solve_lm(**kw)
        outs.append((stats(st), eng.get_x(), int(eng.lm_state()["ticks"]), eng.info()))
        eng.close()
    monkeypatch.delenv("SATBA_HOST_LOOP", raising=False)
    return outs


def host_steps(eng, n, cycle_len=0):
    """n fixed-work iterations driven from the host (satba_lm_step: x and x_new swapped on the host), back to the kept point every
    cycle_len iterations -- what satba_lm_run(n, cycle_len) does on the device."""
    first, Delta, accepted = True, -1.0, 0
    for i in range(n):
        if cycle_len and i and i % cycle_len == 0:
            eng.snapshot_x(True)
            first = True
        r = eng.lm_step(first, Delta, 1e-14)
        first, Delta = False, r["Delta"]
        accepted += int(r["accepted"])
    return accepted


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("sh", [0, 1, 2, 3])
def test_every_lane_count_matches_the_host_loop(gpu, monkeypatch, shape, sh):
    """Lanes per point 1, 2, 4, 8 (SATBA_SPLIT): the lane of slot 0 forms the point's g_h in k_backsub, every lane in k_residual and k_jvp."""
    (sa, xa, ticks, info), (sb, xb, ticks_b, _) = solve_both_loops(monkeypatch, affine_rt(shape), env={"SATBA_SPLIT": str(sh)}, max_nfev=12,
                                                                   loss="linear", **TIGHT)
    assert int(info["lanes_log2"]) == sh and int(info["unit_weights"]) == 1
    assert ticks >= sa[1] - 1 and ticks_b == 0  # the device-resident loop ran / did not run
    assert sa[3] >= 2 and sa[0] < 0.5 * sa[6]  # accepted steps: the solve went somewhere
    assert sa == sb and np.array_equal(xa, xb)


# rotations 0.1 rad off: the Gauss-Newton step inside scipy's first radius |x_h| overshoots, the first trial is rejected, the radius shrinks
REJECT = dict(shape="6x300", seed=1, sigma_theta=0.1, max_nfev=8)


def oracle_decisions(p, max_nfev):
    """The sequence of trial evaluations ("t") and accepted steps ("a") of the reference loop (satba/trf.py on the CPU oracle)."""
    eng = lm_oracle.OracleEngine(p)
    seq = []
    trial_gn, accept = eng.trial_gn, eng.accept
    eng.trial_gn = lambda *a: (seq.append("t"), trial_gn(*a))[1]
    eng.accept = lambda: (seq.append("a"), accept())[1]
    trf.trf_solve(eng, max_nfev=max_nfev, loss="linear", **TIGHT)
    return "".join(seq)


def test_oracle_rejects_then_accepts_for_the_chosen_start():
    """(no GPU) the start of the next test makes the reference loop reject a trial and accept the one behind it -- otherwise that
    test would silently cover accepted steps only."""
    seq = oracle_decisions(affine_rt(REJECT["shape"], REJECT["seed"], REJECT["sigma_theta"])(), REJECT["max_nfev"])
    assert seq.startswith("tta"), seq


@pytest.mark.gpu
def test_rejected_trial_then_accepted_one(gpu, monkeypatch):
    """After a rejected trial the front is switched off: the second trial forms g_h again from the g and scale_inv of the kept linearisation."""
    make_p = affine_rt(REJECT["shape"], REJECT["seed"], REJECT["sigma_theta"])
    (sa, xa, ticks, _), (sb, xb, _, _) = solve_both_loops(monkeypatch, make_p, max_nfev=REJECT["max_nfev"], loss="linear", **TIGHT)
    assert sa[1] - 1 > sa[3] >= 1, sa  # more trial evaluations than iterations: a rejected trial; and an accepted step
    assert sa == sb and np.array_equal(xa, xb)


@pytest.mark.gpu
@pytest.mark.parametrize("n,cycle_len", [(1, 0), (1, 3), (3, 1), (5, 2), (3, 2), (7, 3), (4, 3)])
def test_fixed_work_runs_end_at_the_host_loops_point(gpu, n, cycle_len):
    """satba_lm_run against satba_lm_step: the accepted point is copied on the device / swapped on the host, and at a restart the kept
    point comes back.  n = cycle_len + 1: the run ends one step after a restart."""
    make_p = affine_rt("12x2000")
    xs, acc = [], []
    for device in (False, True):
        eng = HipEngine(make_p())
        eng.configure("linear", 1.0)
        eng.snapshot_x(False)
        if device:
            ls = eng.lm_run(n, cycle_len=cycle_len, lam_floor=1e-14)
            assert int(ls["iterations"]) == n and int(ls["phase"]) == 1
            acc.append(int(ls["accepted"]))
        else:
            acc.append(host_steps(eng, n, cycle_len))
        xs.append(eng.get_x())
        eng.close()
    assert acc[0] == acc[1] and acc[0] >= 1
    assert np.array_equal(xs[0], xs[1])


@pytest.mark.gpu
def test_termination_straight_after_an_accepted_step(gpu, monkeypatch):
    """Loose ftol: the step that satisfies it is accepted and the loop ends behind the linearisation at the accepted point."""
    (sa, xa, _, _), (sb, xb, _, _) = solve_both_loops(monkeypatch, affine_rt("12x2000"), max_nfev=50, loss="linear", ftol=1e-2, xtol=1e-15,
                                                      gtol=1e-15)
    assert sa[4] == 2 and sa[3] >= 1 and sa[2] == sa[3] + 1, sa  # ftol; every iteration accepted and linearised again
    assert sa == sb and np.array_equal(xa, xb)


@pytest.mark.gpu
def test_snapshot_and_get_x_between_two_runs(gpu):
    """get_x and snapshot_x(False) behind a fixed-work run see the run's last accepted point; the next run restarts from it."""
    make_p = affine_rt("6x300")
    outs = []
    for device in (False, True):
        eng = HipEngine(make_p())
        eng.configure("linear", 1.0)
        step = (lambda n, c=0: eng.lm_run(n, cycle_len=c, lam_floor=1e-14)) if device else (lambda n, c=0: host_steps(eng, n, c))
        step(1)  # (far from converged: the steps of the second run are accepted ones)
        x1 = eng.get_x()
        eng.snapshot_x(False)
        step(5, 2)  # ends on the first step after a restart at the point kept above
        x2 = eng.get_x()
        eng.snapshot_x(True)
        x3 = eng.get_x()
        outs.append((x1, x2, x3))
        eng.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert np.array_equal(outs[1][0], outs[1][2]) and not np.array_equal(outs[1][0], outs[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("name,loss", [("affine_small_R", "soft_l1"), ("rpc_small_R", "linear"), ("persp_small_RT", "linear")])
def test_robust_rpc_and_perspective_routes(gpu, monkeypatch, name, loss):
    """Robust loss, RPC and perspective cameras on the device-resident loop: results unchanged against the host loop."""
    _, make_p, _, _ = cases.solve_case(name)
    (sa, xa, ticks, _), (sb, xb, _, _) = solve_both_loops(monkeypatch, make_p, max_nfev=40, loss=loss, **TIGHT)
    assert ticks >= sa[1] - 1 and sa[3] >= 2
    assert sa == sb and np.array_equal(xa, xb)


@pytest.mark.gpu
def test_device_loop_switched_off(gpu, monkeypatch):
    """SATBA_DEVICE_LOOP=0: the host loop -- same result as both other drivers."""
    make_p = affine_rt("12x2000")
    (sa, xa, _, _), (sb, xb, _, _) = solve_both_loops(monkeypatch, make_p, max_nfev=12, loss="linear", **TIGHT)
    monkeypatch.setenv("SATBA_DEVICE_LOOP", "0")
    eng = HipEngine(make_p())
    st = eng.solve_lm(max_nfev=12, loss="linear", **TIGHT)
    assert int(eng.lm_state()["ticks"]) == 0
    assert stats(st) == sa == sb and np.array_equal(eng.get_x(), xa) and np.array_equal(xa, xb)
    eng.close()


@pytest.mark.gpu
def test_two_ranks_keep_the_stored_arrays(gpu, tmp_path):
    """Two gloo ranks on this GPU: the prepare phase is not fused, k_prepare_vec stores g_h and g_h / scale_inv and the readers take the
    stored form -- the device-resident loop equals the host loop on the same two shards."""
    import torch.multiprocessing as mp

    from test_gpu_parity import _two_rank_worker

    outs = {}
    for loop in ("device", "host"):
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        d = tmp_path / loop
        d.mkdir()
        mp.spawn(_two_rank_worker, args=(2, port, "affine_small_RT", "linear", str(d), "gloo", {"SATBA_HOST_LOOP": "1"} if loop == "host" else {}),
                 nprocs=2, join=True)
        outs[loop] = [np.load(os.path.join(str(d), "rank{}.npz".format(r))) for r in range(2)]
    a, b = outs["device"], outs["host"]
    assert int(a[0]["ticks"]) >= int(a[0]["nfev"]) - 1 and int(b[0]["ticks"]) == 0
    assert int(a[0]["nfev"]) == int(b[0]["nfev"]) and float(a[0]["cost"]) == float(b[0]["cost"])
    assert np.array_equal(a[0]["x"], a[1]["x"]) and np.array_equal(a[0]["x"], b[0]["x"]) and np.array_equal(a[0]["r"], b[0]["r"])


# g_h and g_h / scale_inv of the points: formed in their readers on the default route of the single-rank loops, stored everywhere under
# SATBA_STORE_GH=1 -- the same two divisions on the same operands, so the same bits (csrc/satba_kernels.h: point_gh, point_ghs)
@pytest.mark.gpu
@pytest.mark.parametrize("case,loss", [("12x2000", "linear"), ("6x300", "linear"), ("affine_small_R", "soft_l1"), ("persp_small_RT", "linear"),
                                       ("rpc_small_R", "soft_l1")])
@pytest.mark.parametrize("host", [False, True])
def test_g_h_formed_in_its_readers_is_the_stored_g_h(gpu, monkeypatch, case, loss, host):
    """k_backsub, the trial's k_residual, k_jvp<PRE> (affine table form and the generic one) and, with soft_l1, k_subspace_vec."""
    make_p = affine_rt(case) if case in SHAPES else cases.solve_case(case)[1]
    if host:
        monkeypatch.setenv("SATBA_HOST_LOOP", "1")
    outs = []
    for store in ("0", "1"):
        monkeypatch.setenv("SATBA_STORE_GH", store)
        eng = HipEngine(make_p())
        st = eng.solve_lm(max_nfev=25, loss=loss, **TIGHT)
        outs.append((stats(st), eng.get_x(), eng.get_vector("g_h"), eng.get_vector("gn_h")))
        assert int(eng.lm_state()["ticks"]) == 0 if host else int(eng.lm_state()["ticks"]) >= st.nfev - 1
        eng.close()
    assert outs[0][0] == outs[1][0] and outs[0][0][3] >= 2
    for a, b in zip(outs[0][1:], outs[1][1:]):
        assert np.array_equal(a, b)
    assert np.abs(outs[0][2][-3:]).max() > 0  # (the point entries of g_h are there in both forms)


@pytest.mark.gpu
def test_get_vector_forms_the_entries_that_were_not_stored(gpu, monkeypatch):
    """satba_get_vector behind an iteration of the host-driven loop: g_h, and q1 = g_h / scale_inv until a subspace phase overwrites q1,
    are formed on demand where k_linearize did not store them -- equal to the stored arrays, and to g / scale_inv of the same handle."""
    outs = []
    for store in ("0", "1"):
        monkeypatch.setenv("SATBA_STORE_GH", store)
        eng = HipEngine(affine_rt("12x2000")())
        eng.configure("linear", 1.0)
        eng.lm_step(True, -1.0, 1e-14)
        eng.lm_step(False, 1.0, 1e-14)
        outs.append({k: eng.get_vector(k) for k in ("q1", "g_h", "g", "scale_inv")})
        eng.close()
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
    gh = outs[0]["g"] / outs[0]["scale_inv"]
    assert np.array_equal(outs[0]["g_h"], gh) and np.array_equal(outs[0]["q1"], gh / outs[0]["scale_inv"])
    assert np.abs(outs[0]["q1"][-3:]).max() > 0

"""The unit-weight front beside the factorisation with its diagonal pass cut in two (csrc/satba_diag_split.h, SchurRoute::c_split): the
cameras [c*, M) get their diagonal blocks and right-hand-side entries BEHIND the pair kernel, every camera's last chunk workgroup
adding the camera's partials up and counting the camera in (C3Args::arr_extra), the cameras [0, c*) in front of it as before.  Chunk
boundaries, per-chunk sums and the order the partials are added in are those of the sequential front, so every split -- wherever it
sits, in either placement of the late part -- gives the sequential solve to the last bit."""
import numpy as np
import pytest

from satba import synth
from satba.engine_hip import HipEngine

pytestmark = pytest.mark.gpu

# the smallest shapes of test_factorisation_beside_the_pair_kernel_is_the_sequential_solve where the split can sit in every position
# (3, 4, 6 tile columns; 3 and 5 unknowns per camera: cameras that straddle a tile boundary), and one at 200 cameras (16 tile columns)
SHAPES = {
    "affine_RT_27": ("affine", 27, 2000, 6, ["R", "T"]),
    "affine_RT_40": ("affine", 40, 4000, 6, ["R", "T"]),
    "affine_R_70": ("affine", 70, 5000, 5, ["R"]),
    "affine_RT_200": ("affine", 200, 20000, 8, ["R", "T"]),
}
LATE_ENV = ("SATBA_DIAG_LATE_FROM", "SATBA_DIAG_LATE_COLS", "SATBA_DIAG_LATE_PLACE")
_scenes, _refs = {}, {}


def _solve(monkeypatch, shape, loop, env, twice=False):
    """[(statistics, x, info)] of one (twice: two) solve(s) of a fresh handle under `env`"""
    model, M, N, opp, corr = SHAPES[shape]
    if shape not in _scenes:
        _scenes[shape] = synth.make_scene(model, M, N, opp, seed=11)
    monkeypatch.setenv("SATBA_SCHUR_MERGE", "1")  # one item per camera pair for the few cameras of a test, too
    if loop == "host":
        monkeypatch.setenv("SATBA_HOST_LOOP", "1")
    else:
        monkeypatch.delenv("SATBA_HOST_LOOP", raising=False)
    for k in LATE_ENV + ("SATBA_CHOL_BESIDE",):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = synth.make_params(_scenes[shape], {"correction_params": corr, "n_cam_fix": 1})
    x0 = p.params_opt.copy()
    eng = HipEngine(p)
    outs = []
    for _ in range(2 if twice else 1):
        eng.set_x(x0)
        st = eng.solve_lm(max_nfev=30, loss="linear", ftol=1e-12, xtol=1e-12, gtol=1e-12)
        outs.append(((st.cost, st.nfev, st.njev, st.iterations, st.status, st.optimality, st.initial_cost), eng.get_x(), eng.info()))
    eng.close()
    return outs


def _reference(monkeypatch, shape, loop):
    """the sequential front (SATBA_CHOL_BESIDE=0) and the undivided diagonal pass (SATBA_DIAG_LATE_COLS=0), once per (shape, loop)"""
    if (shape, loop) not in _refs:
        seq = _solve(monkeypatch, shape, loop, {"SATBA_CHOL_BESIDE": "0"})[0]
        whole = _solve(monkeypatch, shape, loop, {"SATBA_DIAG_LATE_COLS": "0"})[0]
        assert int(seq[2]["chol_beside"]) == 0 and int(whole[2]["chol_beside"]) == 1
        assert int(whole[2]["diag_late_from"]) == SHAPES[shape][1]  # nothing late
        assert seq[0][0] < 0.5 * seq[0][6]  # (the solve went somewhere)
        seq[1].setflags(write=False)
        whole[1].setflags(write=False)
        _refs[shape, loop] = (seq, whole)
    return _refs[shape, loop]


@pytest.mark.parametrize("split", ["0", "1", "half", "last", "default", "cols2"])
@pytest.mark.parametrize("loop", ["device", "host"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_late_diagonal_cameras_give_the_sequential_solve(gpu, monkeypatch, shape, loop, split):
    """
    Forced splits c* = 0 (every camera late, the fixed one included: it publishes zeros and counts itself in), 1, M // 2, M - 1, the
    default rule and two late tile columns; the late part as a launch of its own behind the pair kernel (a) and as trailing workgroups
    of the pair launch (b); the device-resident loop and the one with the decisions on the host.  Statistics and point identical to
    the sequential front's and to the undivided diagonal pass's, no arrival time-out, and a second solve on the same handle repeats
    the first one: the per-camera counters are back at zero after every front.
    """
    M = SHAPES[shape][1]
    seq, whole = _reference(monkeypatch, shape, loop)
    forced = {"0": 0, "1": 1, "half": M // 2, "last": M - 1}.get(split)
    env = {"default": {}, "cols2": {"SATBA_DIAG_LATE_COLS": "2"}}.get(split, {"SATBA_DIAG_LATE_FROM": str(forced)})
    for place in ("a", "b"):
        outs = _solve(monkeypatch, shape, loop, dict(env, SATBA_DIAG_LATE_PLACE=place), twice=True)
        for stats, x, info in outs:
            assert int(info["chol_beside"]) == 1 and int(info["chol_beside_timeouts"]) == 0, (place, info)
            if forced is not None:
                assert int(info["diag_late_from"]) == forced, (place, info)
            if split == "cols2":
                assert 0 < int(info["diag_late_from"]) < M, (place, info)
            assert stats == seq[0] == whole[0], (place, stats, seq[0], whole[0])
            assert np.array_equal(x, seq[1]) and np.array_equal(x, whole[1]), place

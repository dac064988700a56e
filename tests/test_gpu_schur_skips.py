"""
What the Schur phase and the back-substitution no longer do, and what must not change because of it.

  * k_vinv stores the point blocks' inverses in the records of the Schur kernels only; k_backsub inverts V + lam Dp^2 again with the
    damping k_vinv left on the device.  A stale damping there shows when one handle is damped twice without a new linearisation.
  * Pair items and diagonal walks of a fixed camera skip their hit lists: the blocks are zero, but the items still write them and
    still count themselves in for the factorisation that waits beside the pair kernel.

Shapes (affine cameras, R + T, unit weights, linear loss): 13 cameras x 400 points x 4 observations -- 78 pairs, the sequential front,
n_c = 65: two tile columns; 130 cameras x 3 000 points x 6 observations -- 8 385 pairs, from 8 192 on the pair kernel has one item per
pair and the factorisation may run beside it (n_c = 650, eleven tile columns).

Tolerances: S and rhs 1e-10 relative to the largest entry, the bound of the other Schur tests against the float64 oracle.  The step
gn_h 1e-7, the bound the parity tests hold it to at a damping of 1e-3; the dampings here (0.37, 3.7 in scaled variables, where the
diagonal of J_h^T J_h is 1) leave the system better conditioned, and a step taken with the other damping is off by tens of per cent.
"""
import numpy as np
import pytest

from oracle import lm_oracle as L
from satba import synth
from satba.engine_hip import HipEngine

pytestmark = pytest.mark.gpu

SHAPES = {"small": (13, 400, 4), "large": (130, 3000, 6)}
LAMS = (0.37, 3.7)
_CACHE = {}


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _params(shape, n_cam_fix, n_pts_fix):
    n_cam, n_pts, opp = SHAPES[shape]
    if shape not in _CACHE:
        _CACHE[shape] = synth.make_scene("affine", n_cam, n_pts, opp, seed=17)
    return synth.make_params(_CACHE[shape], {"correction_params": ["R", "T"], "n_cam_fix": n_cam_fix, "n_pts_fix": n_pts_fix,
                                              "reduce": False})


def _oracle(shape, n_cam_fix, n_pts_fix):
    """S, rhs and gn_h of the float64 oracle at x0 for both dampings (computed once per case, read-only afterwards)."""
    key = (shape, n_cam_fix, n_pts_fix)
    if key not in _CACHE:
        ora = L.OracleEngine(_params(*key))
        ora.configure("linear", 1.0)
        ora.linearize()
        ora.prepare(True)
        out = {}
        for lam in LAMS:
            ora.schur(lam)
            n_c = ora.n_c
            S = ora._xb[ora.hdr: ora.hdr + n_c * n_c].reshape(n_c, n_c).copy()
            rhs = ora._xb[ora.hdr + n_c * n_c: ora.len_schur].copy()
            ora.solve()
            for a in (S, rhs, ora.gn_h):
                a.setflags(write=False)
            out[lam] = (S, rhs, ora.gn_h)
        _CACHE[key] = out
    return _CACHE[key]


def _device_system(dev):
    n_c = dev.n_c
    S = dev.get_exchange(dev.hdr, n_c * n_c).reshape(n_c, n_c).T  # column-major on the device, lower triangle
    return S, dev.get_exchange(dev.hdr + n_c * n_c, n_c)


@pytest.mark.parametrize("n_cam_fix", [1, 3])
@pytest.mark.parametrize("shape", ["small", "large"])
def test_fixed_cameras_schur_system(gpu, shape, n_cam_fix):
    """S (lower triangle) and rhs against the oracle; the off-diagonal blocks of the fixed cameras are exactly zero.  At the large
    shape also one front with the factorisation beside the pair kernel: every item of a fixed camera has to count itself in or the
    factorisation's wait times out -- and the factor's columns of the fixed cameras stay zero below their diagonal blocks."""
    p = _params(shape, n_cam_fix, 0)
    S_o, rhs_o, gn_o = _oracle(shape, n_cam_fix, 0)[LAMS[0]]
    dev = HipEngine(p)
    dev.configure("linear", 1.0)
    dev.linearize(); dev.prepare(True); dev.schur(LAMS[0])
    S, rhs = _device_system(dev)
    n_c, n_p = dev.n_c, dev.n_c // p.n_cam
    low = np.tril_indices(n_c)
    print("S", rel(S[low], S_o[low]), "rhs", rel(rhs, rhs_o))
    assert rel(S[low], S_o[low]) < 1e-10
    assert rel(rhs, rhs_o) < 1e-10
    nf = n_cam_fix * n_p
    off = np.tril(S, -1)
    for c in range(n_cam_fix):
        off[c * n_p:(c + 1) * n_p, c * n_p:(c + 1) * n_p] = 0.0  # (the camera's own diagonal block: lam Dc^2)
    assert np.all(off[:, :nf] == 0.0) and np.all(off[:nf, :] == 0.0)
    if shape == "large":
        out = dev.lm_step(True, 0.0, LAMS[0])  # the damping of the Cauchy step lies far below the floor
        assert out["lam"] == LAMS[0]
        info = dev.info()
        assert int(info["chol_beside"]) == 1 and int(info["chol_beside_timeouts"]) == 0
        print("gn_h", rel(dev.get_vector("gn_h"), gn_o))
        assert rel(dev.get_vector("gn_h"), gn_o) < 1e-7
        Lf = np.tril(_device_system(dev)[0], -1)  # the factor, in place
        for c in range(n_cam_fix):
            Lf[c * n_p:(c + 1) * n_p, c * n_p:(c + 1) * n_p] = 0.0
        assert np.all(Lf[:, :nf] == 0.0)
    dev.close()


@pytest.mark.parametrize("n_pts_fix", [0, 7])
@pytest.mark.parametrize("shape", ["small", "large"])
def test_gauss_newton_step_follows_the_damping(gpu, shape, n_pts_fix):
    """schur(lam) + solve() with 0.37 and then 3.7 on one handle, one linearisation: the second step is the oracle's for 3.7."""
    p = _params(shape, 1, n_pts_fix)
    ora = _oracle(shape, 1, n_pts_fix)
    dev = HipEngine(p)
    dev.configure("linear", 1.0)
    dev.linearize(); dev.prepare(True)
    for lam in LAMS:
        dev.schur(lam); dev.solve()
        gn = dev.get_vector("gn_h")
        print("lam", lam, "gn_h", rel(gn, ora[lam][2]))
        assert rel(gn, ora[lam][2]) < 1e-7
        assert np.all(gn[dev.n_c: dev.n_c + 3 * n_pts_fix] == 0.0)  # frozen points do not move
    assert rel(ora[LAMS[0]][2], ora[LAMS[1]][2]) > 0.1  # (a step left over from the first damping would not pass for the second)
    dev.close()


def test_loops_agree_bit_for_bit(gpu, monkeypatch):
    """One solve from x0 with the device-resident loop and one with the decisions on the host: same statistics, same solution."""
    outs = []
    for host in (False, True):
        if host:
            monkeypatch.setenv("SATBA_HOST_LOOP", "1")
        eng = HipEngine(_params("small", 1, 0))
        st = eng.solve_lm(max_nfev=30, loss="linear", ftol=1e-12, xtol=1e-12, gtol=1e-12)
        outs.append(((st.cost, st.nfev, st.njev, st.iterations, st.status, st.optimality, st.initial_cost), eng.get_x()))
        eng.close()
    assert outs[0][0] == outs[1][0] and np.array_equal(outs[0][1], outs[1][1])
    assert outs[0][0][1] > 2 and outs[0][0][0] < outs[0][0][6]

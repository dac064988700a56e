"""
Affine fundamental matrices from RPCs, the parts that need no GPU: the host's affine_fundamental_matrix against the reference's
vectors (tests/golden/ft_fundamental.npz), the yardstick of the device tolerances (the numpy restatement of the device route
against the reference's SVD route), the sign-invariance of the epipolar gate, the rank test and the argument checks of the C ABI.

Yardstick measured here (px, cases_fundamental.yardstick: the larger of the restatement's two solvers), pair i j / crop / n:
  0 1 full 5: 1.4e-11   0 1 c500 5: 5.6e-12   0 1 c50 5: 1.4e-10   1 0 full 5: 3.1e-12   1 0 c500 5: 1.3e-11   1 0 c50 5: 4.0e-10
  0 1 full 2: 1.5e-11   0 1 full 3: 8.7e-12   0 1 full 7: 9.7e-12   0 1 full 11: 6.4e-12
The components of N differ by 3e-16 .. 5e-12 (the c50 crops, where the gap of the two smallest singular values is smallest).
"""
import ctypes as C

import numpy as np
import pytest

import cases_camapprox as CC
import cases_fundamental as CF
from satba import engine_hip, ft_match, rpc_utils

E_ARG, E_NONFINITE = -1, -4
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def golden():
    return dict(CF.load_golden())


@pytest.mark.parametrize("case", CF.CASES, ids=CF.key)
def test_host_matrix_reproduces_the_reference_up_to_sign(golden, case):
    k = CF.key(case)
    m, Fg, sv = golden[k + "_matches"], golden[k + "_F"], golden[k + "_sv"]
    assert m.shape == (case[3] ** 3, 4)
    F = rpc_utils.affine_fundamental_matrix(m)
    assert F.shape == (3, 3) and not F[:2, :2].any() and abs(np.linalg.norm(CF.f5(F)[:4]) - 1.0) <= 4 * EPS
    assert ft_match.affine_fundamental_matrix is rpc_utils.affine_fundamental_matrix
    # SVD repeatability: a backward error of a few eps sigma_1 in A turns N by that over the gap to the next singular value
    tol = 64 * EPS * sv[0] / (sv[2] - sv[3])
    d = CF.vector_distance(F, Fg)
    print("{}: N against the stored one {:.3e} (bound {:.3e})".format(k, d, tol))
    assert d <= tol
    assert abs(abs(F[2, 2]) - abs(Fg[2, 2])) <= tol * np.abs(m).max() * 4
    with pytest.raises(ValueError):
        rpc_utils.affine_fundamental_matrix(m[:, :3])


@pytest.mark.parametrize("case", CF.CASES, ids=CF.key)
def test_yardstick_restatement_against_reference(golden, case):
    """two-pass normal matrix + Jacobi / eigh on the oracle's matches against the reference's SVD: what float64 leaves between two
    correct routes.  Ten times this is the device's tolerance and has to stay below the project's parity level."""
    k = CF.key(case)
    i, j, _, n = case
    m = CF.restate_matches(CC.rpc(i), CC.rpc(j), CF.roi(case), n)
    assert np.abs(m - golden[k + "_matches"]).max() <= 1e-9  # the same oracle, the same numpy: equal up to the build of numpy
    pts = CF.metric_points(golden, case)
    for solver in ("jacobi", "eigh"):
        F, sv, deg = CF.restate(m, solver)
        print("{} {:6s}: {:.3e} px, N {:.3e}, largest residual of the reference's F {:.2f} px".format(
            k, solver, CF.distance(F, golden[k + "_F"], pts), CF.vector_distance(F, golden[k + "_F"]), np.abs(CF.residual(golden[k + "_F"], pts)).max()))
        assert not deg and F[np.argmax(np.abs(F[:4]))] > 0.0 and abs(np.linalg.norm(F[:4]) - 1.0) <= 4 * EPS
        # eigenvalues of A^T A are good to a few eps of the largest
        assert np.abs(sv ** 2 - golden[k + "_sv"] ** 2).max() <= 64 * EPS * golden[k + "_sv"][0] ** 2
    y = CF.yardstick(golden, case)
    print("{}: yardstick {:.3e} px".format(k, y))
    assert CF.SOLVE_MARGIN * y <= CF.PX_CAP
    assert 0.0 < y


def test_conditioning_of_the_cases(golden):
    """the null direction is separated: sigma_4 is pixels of RPC non-linearity, the healthy ratio lambda_3 / lambda_1 sits far above
    the rank tolerance"""
    for case in CF.CASES:
        sv = golden[CF.key(case) + "_sv"]
        print(CF.key(case), sv, "lambda_3 / lambda_1 = {:.2e}".format((sv[2] / sv[0]) ** 2))
        assert sv[3] > 1.0 and sv[2] > 20 * sv[3] and (sv[2] / sv[0]) ** 2 >= 5e-6 > 1e6 * CF.RANK_TOL


def test_sign_of_the_reference_is_arbitrary_and_the_gate_ignores_it(golden):
    """the reference's sign flips between crops of one pair; the rectifying similarities of -F negate both rectified ordinates"""
    signs = set()
    for case in CF.HEALTHY:
        k = CF.key(case)
        F, m = golden[k + "_F"], golden[k + "_matches"].astype(np.float32)
        signs.add((case[0], bool(F[0, 2] > 0)))
        (s1, s2), (t1, t2) = ft_match.rectifying_similarities(F), ft_match.rectifying_similarities(-F)
        assert np.array_equal(t1, -s1) and np.array_equal(t2, -s2)
        y1, y2 = (s1[1] * m[:, 0] + s1[0] * m[:, 1]) + s1[2], (s2[1] * m[:, 2] + s2[0] * m[:, 3]) + s2[2]
        z1, z2 = (t1[1] * m[:, 0] + t1[0] * m[:, 1]) + t1[2], (t2[1] * m[:, 2] + t2[0] * m[:, 3]) + t2[2]
        assert np.array_equal(z1, -y1) and np.array_equal(z2, -y2) and np.array_equal(np.abs(z1 - z2), np.abs(y1 - y2))
        assert np.abs(y1 - y2).max() < ft_match.EPIPOLAR_THR  # the pair's own matches pass the gate
    assert len(signs) > 2  # both signs occur for at least one ordered pair


def test_restatement_flags_a_pair_of_an_image_with_itself():
    r = CC.rpc(0)
    F, sv, deg = CF.restate(CF.restate_matches(r, r, CC.CROPS["full"], 5))
    assert deg and np.isnan(F).all() and sv[2] ** 2 <= CF.RANK_TOL * sv[0] ** 2
    for i, j, c, n in CF.HEALTHY:
        assert not CF.restate(CF.restate_matches(CC.rpc(i), CC.rpc(j), CC.CROPS[c], n))[2]


def test_c_abi_argument_errors_come_before_any_device_call():
    lib = engine_hip.load_library()
    tab = np.stack([CC.rpc(0).to_table(), CC.rpc(1).to_table()])
    F5, sv, deg = np.zeros((2, 5)), np.zeros((2, 4)), np.zeros(2, dtype=np.uint8)

    def call(n_cam=2, tables=tab, n_pairs=2, pairs=((0, 1), (1, 0)), roi=((0, 0, 3200, 1350), (0, 0, 3200, 1350)), n=5, out=F5):
        p = np.ascontiguousarray(pairs, dtype=np.int32) if pairs is not None else None
        r = np.ascontiguousarray(roi, dtype=np.float64) if roi is not None else None
        t = np.ascontiguousarray(tables, dtype=np.float64) if tables is not None else None
        return lib.satba_rpc_fundamental(n_cam, engine_hip._ptr(t) if t is not None else None, n_pairs, engine_hip._ptr(p, engine_hip._ip) if p is not None else None,
                                         engine_hip._ptr(r) if r is not None else None, n, engine_hip._ptr(out) if out is not None else None,
                                         engine_hip._ptr(sv), None, deg.ctypes.data_as(C.POINTER(C.c_uint8)), 0)

    assert call(tables=None) == E_ARG and call(pairs=None) == E_ARG and call(roi=None) == E_ARG and call(out=None) == E_ARG
    assert call(n_cam=-1) == E_ARG and call(n_pairs=-1) == E_ARG
    assert call(n=1) == E_ARG and call(n=0) == E_ARG and call(n=-5) == E_ARG
    assert call(n=CF.MAX_N + 1) == E_ARG and b"11" in lib.satba_last_error()
    assert call(pairs=((0, 1), (1, 2))) == E_ARG and call(pairs=((-1, 1), (1, 0))) == E_ARG
    assert call(roi=((0, 0, 0, 1350), (0, 0, 3200, 1350))) == E_ARG and call(roi=((0, 0, 3200, 1350), (0, 0, 3200, -1))) == E_ARG
    assert call(roi=((0, 0, np.nan, 1350), (0, 0, 3200, 1350))) == E_NONFINITE and call(roi=((np.inf, 0, 3200, 1350), (0, 0, 3200, 1350))) == E_NONFINITE
    bad = tab.copy(); bad[1, 85] = np.nan
    assert call(tables=bad) == E_NONFINITE
    assert call(n_pairs=0) == 0 and call(n_cam=0, n_pairs=0) == 0  # an empty batch is answered on the host
    assert not F5.any() and not sv.any() and not deg.any()  # no output was touched
    assert rpc_utils.fundamental_matrices([], [], []) == []
    for sym in ("satba_rpc_fundamental", "satba_rpc_fundamental_kernel_ms"):
        assert sym in engine_hip.SYMBOLS and hasattr(lib, sym), sym


def test_python_wrappers_check_their_arguments():
    r, off = CC.rpc(0), CC.offset(CC.CROPS["full"])
    with pytest.raises(ValueError):
        rpc_utils.fundamental_matrices([(0, 1)], [r], [off])  # a pair names an image that is not there
    with pytest.raises(ValueError):
        rpc_utils.fundamental_matrices([(0, 1)], [r, r], [off])
    with pytest.raises(ValueError):
        rpc_utils.fundamental_matrices([(0, 1)], [r, CC.rpc(1)], [off, off], n=1)
    with pytest.raises(ValueError):
        rpc_utils.fundamental_matrices([(0, 1)], [r, CC.rpc(1)], [off, off], n=CF.MAX_N + 1)
    with pytest.raises(ValueError):
        rpc_utils.fundamental_matrices([(0, 1)], [r, CC.rpc(1)], [off, off], n=2.5)
    with pytest.raises(ValueError):
        rpc_utils.matches_from_rpc(r, CC.rpc(1), 0, 0, 0, 1350, 5)
    assert rpc_utils.MAX_N == CF.MAX_N and ft_match.fundamental_matrices is rpc_utils.fundamental_matrices
    assert ft_match.matches_from_rpc is rpc_utils.matches_from_rpc

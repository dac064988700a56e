"""
The dense solve of the reduced camera system (csrc/satba_chol.h, satba_chol3.h) on the systems of tests/cases_dense.py, through the C
ABI: ill-conditioned, clustered and graded SPD systems at every size where the solver takes another path, pivots that fail late in the
matrix, special right-hand sides and the state a solve leaves in its handle.

A system is planted as test_dense_cholesky_solve (test_gpu_parity.py) does it -- linearize, prepare, schur, then the payload is
overwritten -- and everything is measured in the scaled variables the device factorises in (cases_dense.py: M_eff, b_eff).  The
bounds are LAPACK's own constants times 8 (forward) and 16 (backward, factor): cases_dense.bounds; tests/test_dense_cases_host.py
shows that LAPACK meets them with margin 1.  What the device and LAPACK give on every case is written down in
profiles/dense_accuracy.json (tools/dense_accuracy.py).

Routes: up to 63 unknowns k_solve_small; above, k_chol_tiles with k_trsv_back_mw (up to 1024 unknowns) or k_trsv_back.
"""
import numpy as np
import pytest

import cases_dense as D
from satba import synth, trf
from satba.engine_hip import HipEngine

pytestmark = pytest.mark.gpu

SATBA_CHOL_NOT_SPD = 1  # include/satba.h
ALL_SIZES = {**D.SIZES, **D.EXTRA_SIZES}
_ENGINES = {}


def open_engine(n):
    """a handle with n unknowns in its reduced system, a reduced system formed once (the solve phase expects one), and its scale_inv"""
    model, n_cam, corr = ALL_SIZES[n]
    kw, opts = {}, {"correction_params": list(corr)}
    if corr == "RTK":
        kw["sigma_k"] = 1e-2 if model == "affine" else 2e-3
        opts["K_init"] = "camera"
    scene = synth.make_scene(model, n_cam, 4 * n_cam, min(n_cam, 4), seed=3, **kw)
    eng = HipEngine(synth.make_params(scene, opts))
    eng.configure("linear", 1.0)
    eng.linearize()
    eng.prepare(True)
    eng.schur(1.0)
    assert eng.n_c == n
    s = eng.get_vector("scale_inv")[:n].copy()
    assert np.isfinite(s).all() and (s > 0).all()
    return eng, s


def _engine(n):
    if n not in _ENGINES:
        _ENGINES[n] = open_engine(n)
    return _ENGINES[n]


@pytest.fixture(scope="module", autouse=True)
def _engines(gpu):
    yield
    for eng, _ in _ENGINES.values():
        eng.close()
    _ENGINES.clear()


def solve(eng, S_p, rhs, upper=0.0):
    """plant, solve; (status word, solution in scaled variables)"""
    n = eng.n_c
    eng.set_exchange(eng.hdr, D.payload(S_p, upper))
    eng.set_exchange(eng.hdr + n * n, rhs)
    eng.solve()
    flag = eng.read_header()[trf.CHOL_FAIL]
    return flag, eng.get_vector("gn_h")[:n].copy()


def read_factor(eng):
    """the payload after a solve on the tile routes: L in the lower triangle, (n <= 1024) L^T in the strict upper one"""
    n = eng.n_c
    return eng.get_exchange(eng.hdr, n * n).reshape(n, n).T.copy()  # column-major on the device


# ------------------------------------------------------------------------------------------------------------- a. accuracy

@pytest.mark.parametrize("family", D.SPD_FAMILIES)
@pytest.mark.parametrize("n", list(D.SIZES))
def test_accuracy(n, family):
    """forward error <= 8 C_FWD u kappa_2(M_eff) for every family; backward error <= 16 C_BWD u where kappa <= 1e4 (above, the
    explicitly inverted diagonal blocks may cost backward stability: recorded in profiles/dense_accuracy.json, not asserted)"""
    eng, s = _engine(n)
    c = D.Case(family, n, s)
    flag, z = solve(eng, c.S_p, c.rhs)
    assert flag == 0 and np.isfinite(z).all()
    c.check(c.measure(z), "device")


# ------------------------------------------------------------------------------------------------------------- b. the factor

@pytest.mark.parametrize("family", D.SPD_FAMILIES)
@pytest.mark.parametrize("n", [n for n in D.SIZES if n >= 64])
def test_factor(n, family):
    """|L L^T - M_eff|_F / |M_eff|_F <= 16 C_FAC u where kappa <= 1e4; and the strict upper triangle is L^T bit for bit wherever
    k_trsv_back_mw reads it (its load_block: every entry outside the 32 x 32 diagonal blocks)"""
    eng, s = _engine(n)
    c = D.Case(family, n, s)
    flag, z = solve(eng, c.S_p, c.rhs)
    assert flag == 0
    A = read_factor(eng)
    L = np.tril(A)
    assert np.isfinite(L).all() and (np.diag(L) > 0).all()
    fac = D.factor_residual(L, c.M_eff)
    bound = D.bounds(family, 0.0)[2]
    print("device n={} {}: factor residual {:.3e} (bound {})".format(n, family, fac, bound))
    if bound is not None:
        assert fac <= bound
    if n <= 1024:
        blk = np.arange(n) // 32
        read = blk[:, None] < blk[None, :]  # row block above column block: read by the substitution as L^T
        assert np.array_equal(A[read], L.T[read])


# ------------------------------------------------------------------------------------------------------------- c. failing pivots

_CLEAN = {}


def _wishart_on_a_fresh_handle(n):
    """the wishart system's solution on a handle that never saw a failed factorisation"""
    if n not in _CLEAN:
        eng, s = open_engine(n)
        c = D.Case("wishart", n, s)
        flag, z = solve(eng, c.S_p, c.rhs)
        eng.close()
        assert flag == 0
        _CLEAN[n] = (s, z)
    return _CLEAN[n]


@pytest.mark.parametrize("n,j,kind", D.fail_cases())
def test_failing_pivot_raises_the_flag_and_leaves_the_handle_clean(n, j, kind):
    """Pivot j fails -- after the updates only ("negative"), or by a NaN / inf in row j -- in every wave quarter, micro-panel, tile and
    in the ragged last tile: the status word is exactly SATBA_CHOL_NOT_SPD (no time-out bits: the kernels keep going after a bad
    pivot, none of their waits depends on a value), and the next solve on the handle has the bits of a handle that never failed."""
    eng, s = _engine(n)
    bad = D.Case("wishart", n, s, M=D.indefinite(D.spd("wishart", n), j, kind))
    flag, _ = solve(eng, bad.S_p, bad.rhs)
    assert int(flag) == SATBA_CHOL_NOT_SPD and flag == SATBA_CHOL_NOT_SPD
    s_clean, z_clean = _wishart_on_a_fresh_handle(n)
    assert np.array_equal(s, s_clean)
    good = D.Case("wishart", n, s)
    flag, z = solve(eng, good.S_p, good.rhs)
    assert flag == 0
    assert z.tobytes() == z_clean.tobytes()


@pytest.mark.parametrize("n", [22, 63, 130, 1026])
def test_tiny_pivots_are_no_failure(n):
    """the counter-case: spectrum12 has pivots down to ~1e-12"""
    eng, s = _engine(n)
    c = D.Case("spectrum12", n, s)
    flag, z = solve(eng, c.S_p, c.rhs)
    assert flag == 0 and np.isfinite(z).all()


# ------------------------------------------------------------------------------------------------------------- d. right-hand sides

RHS_SIZES = [22, 130, 1026]


@pytest.mark.parametrize("n", RHS_SIZES)
def test_zero_right_hand_side(n):
    eng, s = _engine(n)
    c = D.Case("spectrum4", n, s, b=np.zeros(n))
    flag, z = solve(eng, c.S_p, c.rhs)
    assert flag == 0 and np.array_equal(z, np.zeros(n))  # (+0 or -0, no NaN)


@pytest.mark.parametrize("n", RHS_SIZES)
def test_right_hand_side_scaled_by_a_power_of_two(n):
    """every operation on the right-hand side is linear and no exponent comes near the limits (|z| ~ 1e4 x 2^+-40; k_solve_small
    carries the right-hand side as row 63 under a corner of 1e200): the same bits, shifted"""
    eng, s = _engine(n)
    c = D.Case("spectrum4", n, s)
    flag, z = solve(eng, c.S_p, c.rhs)
    assert flag == 0 and np.abs(z).max() < 1e8
    for e in (40, -40):
        flag, ze = solve(eng, c.S_p, np.ldexp(c.rhs, e))
        assert flag == 0
        assert ze.tobytes() == np.ldexp(z, e).tobytes(), e


@pytest.mark.parametrize("n", RHS_SIZES)
def test_unit_right_hand_sides(n):
    """e_0, e_(n-1) and e_k at the edges of the 64-row tiles and the 128-row superblocks of the substitution, each held to the bounds
    of test_accuracy (spectrum4: forward and backward)"""
    eng, s = _engine(n)
    base = D.Case("spectrum4", n, s)
    for k in sorted({0, n - 1} | {k for k in (63, 64, 127, 128, 1023, 1024) if k < n}):
        c = D.Case("spectrum4", n, s, b=np.eye(n)[k])
        c.__dict__["kappa"] = base.kappa  # (the same matrix)
        assert c.b_eff[k] == 1.0
        flag, z = solve(eng, c.S_p, c.rhs)
        assert flag == 0
        c.check(c.measure(z), "device e_{}".format(k))


# ------------------------------------------------------------------------------------------------------------- e. state

@pytest.mark.parametrize("n", list(D.SIZES))
def test_same_bits_twice_and_upper_triangle_ignored(n):
    """the same system twice on one handle: the same bits; NaN in the strict upper triangle of the payload (ignored on input by
    contract -- in production it holds the previous solve's L^T): the same bits again"""
    eng, s = _engine(n)
    c = D.Case("spectrum8", n, s)
    flag, z1 = solve(eng, c.S_p, c.rhs)
    assert flag == 0
    flag, z2 = solve(eng, c.S_p, c.rhs)
    assert flag == 0 and z2.tobytes() == z1.tobytes()
    flag, z3 = solve(eng, c.S_p, c.rhs, upper=np.nan)
    assert flag == 0 and z3.tobytes() == z1.tobytes()

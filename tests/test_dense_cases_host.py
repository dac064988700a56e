"""
The systems of tests/cases_dense.py without a device: the families have the condition numbers they are named for, `truth` is far
more accurate than anything it is compared with, every indefinite case fails where it is meant to, and LAPACK's float64 Cholesky --
measured on every (size, family) the device is tested on -- is inside the device's bounds with margin 1 instead of 8 and 16: the
constants C_FWD, C_BWD, C_FAC of cases_dense.py are LAPACK's, not a fit to the device.

The scale_inv of a handle is replaced by a synthetic one spanning 1e-6 .. 1e3.
"""
import mpmath
import numpy as np
import pytest

import cases_dense as D


def _case(family, n):
    return D.Case(family, n, D.synthetic_scale(n))


@pytest.fixture(scope="module")
def lapack_table():
    """LAPACK on every (size, family): {(n, family): (case's kappa, measures, last refinement correction)}"""
    out = {}
    for n in D.SIZES:
        for family in D.SPD_FAMILIES:
            c = _case(family, n)
            z, L = D.lapack(c.M_eff, c.b_eff)
            out[n, family] = (c.measure(z, L), c.truth_info["last"], np.diag(c.M_eff).copy())
    return out


def test_families_have_their_condition_numbers(lapack_table):
    for (n, family), (m, _, diag) in lapack_table.items():
        k = m["kappa_scaled"] if family == "graded" else m["kappa"]
        assert D.KAPPA[family] / 3 < k < 3 * D.KAPPA[family], (n, family, k)
        if family in D.UNIT_DIAGONAL:
            assert np.abs(diag - 1.0).max() <= 1e-12, (n, family)
        if family == "graded":
            assert 1e12 / 3 < diag.max() / diag.min() < 3e12, (n, diag.min(), diag.max())


def test_effective_system_is_the_scaling_kernels_arithmetic():
    """M_eff is S_p[r, c] / (s[r] * s[c]) -- one product, one division, in float64 -- and differs from M by two roundings"""
    n = 22
    M, s = D.spd("spectrum8", n), D.synthetic_scale(n)
    S_p, rhs, M_eff, b_eff = D.planted(M, D.rhs_for("spectrum8", n), s)
    for r, c in ((0, 0), (5, 3), (21, 20), (3, 17)):
        assert M_eff[r, c] == np.float64(S_p[r, c]) / (np.float64(s[r]) * np.float64(s[c]))
    assert b_eff[7] == rhs[7] / s[7]
    assert np.array_equal(M_eff, M_eff.T)
    assert 0 < np.abs(M_eff - M).max() <= 4 * 2.0 ** -53 * np.abs(M).max()
    P = D.payload(S_p, np.nan).reshape(n, n)  # column-major: P[c, r] = S_p[r, c]
    assert P[3, 5] == S_p[5, 3] and np.isnan(P[5, 3]) and P[4, 4] == S_p[4, 4]


def _mp_solve(M, b):
    mpmath.mp.prec = 200
    z = mpmath.lu_solve(mpmath.matrix(M.tolist()), mpmath.matrix(b.tolist()))
    return [z[i] for i in range(len(b))]


def _mp(v):
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(v - D.LD(hi)))


@pytest.mark.parametrize("family", D.SPD_FAMILIES)
@pytest.mark.parametrize("n", [22, 66])
def test_truth_against_mpmath(family, n):
    c = _case(family, n)
    z_mp = _mp_solve(c.M_eff, c.b_eff)
    z = c.z_true
    err = max(abs(_mp(z[i]) - z_mp[i]) for i in range(n)) / max(abs(v) for v in z_mp)
    fwd, _, _ = D.bounds(family, c.kappa)
    assert err <= 0.01 * fwd, (float(err), fwd)
    if family == "graded":  # the bound asserted for graded systems is the one in the variables d o z
        ks, d = c.scaled
        err = max(abs(_mp(z[i]) - z_mp[i]) * d[i] for i in range(n)) / max(abs(z_mp[i]) * d[i] for i in range(n))
        assert err <= 0.01 * D.FWD_MARGIN * D.C_FWD * D.U * ks, float(err)


def test_truth_converges_at_every_size(lapack_table):
    """beyond what mpmath checks: the last correction of the refinement -- the size of what is left -- is below 1 / 100 of the smallest
    tolerance asserted for the family"""
    for (n, family), (m, last, _) in lapack_table.items():
        tol = D.bounds(family, m["kappa"])[0]
        if family == "graded":
            tol = D.FWD_MARGIN * D.C_FWD * D.U * m["kappa_scaled"]
        assert last <= 0.01 * tol, (n, family, last, tol)


def test_factor_residual_is_exact():
    """the sliced product against a longdouble product, rows spread over ten orders of magnitude"""
    n = 130
    L = np.tril(np.random.default_rng(1).normal(size=(n, n))) * 10.0 ** np.random.default_rng(2).uniform(-5, 5, size=(n, 1))
    M = L @ L.T
    Ll = L.astype(D.LD)
    R = Ll @ Ll.T - M
    ref = float(np.sqrt((R * R).sum()) / np.sqrt((M.astype(D.LD) ** 2).sum()))
    got = D.factor_residual(L, M)
    assert 1e-17 < ref < 1e-15 and abs(got - ref) <= 0.02 * ref  # (the longdouble product rounds at 2^-64 itself)


def test_lapack_is_inside_the_devices_bounds_with_margin_one(lapack_table):
    worst = {"fwd": (0, None), "bwd": (0, None), "fac": (0, None), "fwd_scaled": (0, None)}
    for key, (m, _, _) in lapack_table.items():
        for name, v in (("fwd", m["fwd"] / (D.U * m["kappa"])), ("bwd", m["bwd"] / D.U), ("fac", m["fac"] / D.U)):
            worst[name] = max(worst[name], (v, key))
        if key[1] == "graded":
            worst["fwd_scaled"] = max(worst["fwd_scaled"], (m["fwd_scaled"] / (D.U * m["kappa_scaled"]), key))
    print("LAPACK float64 Cholesky, worst over sizes x families:", worst)
    assert worst["fwd"][0] <= D.C_FWD and worst["fwd_scaled"][0] <= D.C_FWD
    assert worst["bwd"][0] <= D.C_BWD
    assert worst["fac"][0] <= D.C_FAC
    # ... and the constants are LAPACK's own, not an allowance: at least half of each is used
    assert worst["fwd"][0] >= 0.5 * D.C_FWD and worst["bwd"][0] >= 0.5 * D.C_BWD and worst["fac"][0] >= 0.5 * D.C_FAC


def test_spectrum12_factorises():
    """the counter-case of the failing pivots: pivots down to ~1e-12 are no failure"""
    for n in (22, 63, 130, 1026):
        c = _case("spectrum12", n)
        L = np.linalg.cholesky(c.M_eff)
        assert 1e-8 < np.diag(L).min() < 1e-4 and D.cholesky_ld(c.M_eff)[1] == n


@pytest.mark.parametrize("n,j,kind", D.fail_cases())
def test_indefinite_cases_fail_at_their_pivot(n, j, kind):
    s = D.synthetic_scale(n)
    M = D.indefinite(D.spd("wishart", n), j, kind)
    c = D.Case("wishart", n, s, M=M)
    if kind == "negative":
        with pytest.raises(np.linalg.LinAlgError):
            np.linalg.cholesky(c.M_eff)
    else:
        # (numpy's Cholesky does not test its pivots for NaN or inf: with the OpenBLAS build it raises on some of these and hands back
        # a factor full of NaN on others -- the very behaviour the device's flag exists to prevent.  Either is a failure.)
        try:
            assert not np.isfinite(np.linalg.cholesky(c.M_eff)).all()
        except np.linalg.LinAlgError:
            pass
    if kind == "negative" and j > 0:
        assert c.M_eff[j, j] > 0  # only the updates make the pivot negative
    # in extended precision: the leading minor of order j is positive definite, the one of order j + 1 is not
    L, first_bad = D.cholesky_ld(c.M_eff[: j + 1, : j + 1])
    assert first_bad == j
    if kind == "negative":
        pivot = c.M_eff[j, j] - (L[j, :j] * L[j, :j]).sum() if j else c.M_eff[0, 0]
        assert -0.51 < pivot < -0.49, pivot
    # everything but row / column j is the SPD matrix's
    keep = np.ones(n, dtype=bool)
    keep[j] = False
    if kind == "nan_offdiag" and j > 0:
        assert np.isnan(c.M_eff[j, j // 2]) and np.isfinite(np.delete(c.M_eff[j], j // 2)).all()
    assert np.array_equal(c.M_eff[np.ix_(keep, keep)], D.Case("wishart", n, s).M_eff[np.ix_(keep, keep)])

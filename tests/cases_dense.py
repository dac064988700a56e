"""
Systems for the dense solve of the reduced camera system (csrc/satba_chol.h, satba_chol3.h: k_solve_small up to 63 unknowns,
k_chol_tiles + k_trsv_back_mw up to 1024, k_chol_tiles + k_trsv_back above), their solution to better than float64 and the error
measures.  numpy / scipy only.  Shared by tests/test_dense_cases_host.py (which shows that LAPACK in float64 meets every bound the
device is held to), tests/test_gpu_dense.py and tools/dense_accuracy.py.

What the device factorises.  A test plants S_p and rhs in the exchange payload; k_scale_system / k_solve_small first form, in float64,
    M_eff[r, c] = S_p[r, c] / (scale_inv[r] * scale_inv[c]),    b_eff = rhs / scale_inv
and the solution z of M_eff z = b_eff is what get_vector("gn_h") returns.  A family is built as the matrix M wanted in these scaled
variables, planted as S_p = M o (s s^T) (`plant`), and M_eff, b_eff are recomputed here with the same two operations in the same order
(`effective`).  M_eff differs from M by two roundings per entry; every truth and every measure is formed from M_eff and b_eff.

Families (SPD_FAMILIES, each seeded and built for any n; KAPPA: the nominal 2-norm condition number):
  wishart      A A^T + n I, A standard normal: condition ~5 (the only kind of input the suite had before)
  spectrum4 / spectrum8 / spectrum12
               Q diag(logspace(0, -k, n)) Q^T, Q random orthogonal, rescaled symmetrically to unit diagonal (production hands the
               solver a unit diagonal up to the damping).  spectrum12 has pivots down to ~1e-12 and must still factorise.
  cluster9     n - 7 eigenvalues at 1 and seven at 1e-9 (n < 14: n // 2 of them), unit diagonal: the flat valley / gauge directions
  graded       D spectrum4 D, D = diag(logspace(-3, 3, n)) in random order: the diagonal spans 1e-6 .. 1e6 (the pivot limits 1e-300,
               1e300 of the solver are absolute).  Its 2-norm condition number is 1e12 .. 1e16 and has no closed form: KAPPA holds
               the condition number after rescaling to unit diagonal (1e4), and `kappa2` computes the true one.
`indefinite(M, j, kind)`: row j of an SPD matrix changed so that the leading minor of order j stays positive definite and pivot j
fails -- "negative": M[j, j] = sum_k L[j, k]^2 - 0.5 (the diagonal entry stays positive for j > 0: only the updates make the pivot
negative), "nan_diag", "inf_diag", "nan_offdiag" (NaN at M[j, j // 2]).

Constants C_FWD, C_BWD, C_FAC: what LAPACK's float64 Cholesky (scipy.linalg.cho_factor / cho_solve) needs on every (size, family) of
SIZES x SPD_FAMILIES, in units of u kappa_2 (forward error) and u (backward error, factor residual), u = 2^-53, rounded up.
tests/test_dense_cases_host.py re-measures them and fails if LAPACK exceeds them; profiles/dense_accuracy.json holds the measured
values.  The device is allowed 8 x (forward) and 16 x (backward, factor) as much: a different summation order, a square root from
v_rsq_f64 + two Goldschmidt steps (a few ulp) and explicitly inverted, well-conditioned diagonal blocks.
"""
import functools

import numpy as np
import scipy.linalg as sl
import scipy.sparse.linalg as ssl

U = 2.0 ** -53
LD = np.longdouble

SPD_FAMILIES = ("wishart", "spectrum4", "spectrum8", "spectrum12", "cluster9", "graded")
KAPPA = {"wishart": 5.0, "spectrum4": 1e4, "spectrum8": 1e8, "spectrum12": 1e12, "cluster9": 1e9, "graded": 1e4}
UNIT_DIAGONAL = ("spectrum4", "spectrum8", "spectrum12", "cluster9")
BACKWARD_STABLE = ("wishart", "spectrum4")  # kappa <= 1e4: backward error and factor residual are asserted, elsewhere recorded

# (unknowns) -> (camera model, cameras, correction_params): cameras x n_params, n_params = 3 (R), 5 / 6 (R, T affine / perspective),
# 8 / 11 (R, T, K affine / perspective)
SIZES = {
    # k_solve_small; 56 / 57: the eighth micro-panel, and with it the padded corner, enters the factorisation
    6: ("affine", 2, "R"), 16: ("affine", 2, "RTK"), 22: ("perspective", 2, "RTK"), 55: ("perspective", 5, "RTK"),
    56: ("affine", 7, "RTK"), 57: ("affine", 19, "R"), 63: ("affine", 21, "R"),
    # k_chol_tiles + k_trsv_back_mw; 64: one tile; 1024: the last size the multi-workgroup substitution takes
    64: ("affine", 8, "RTK"), 65: ("affine", 13, "RT"), 88: ("perspective", 8, "RTK"), 126: ("affine", 42, "R"),
    128: ("affine", 16, "RTK"), 129: ("affine", 43, "R"), 255: ("affine", 85, "R"), 256: ("affine", 32, "RTK"),
    258: ("affine", 86, "R"), 704: ("perspective", 64, "RTK"), 1020: ("affine", 340, "R"), 1023: ("affine", 341, "R"),
    1024: ("affine", 128, "RTK"),
    # k_chol_tiles + k_trsv_back; 1056: a whole number of 32-blocks
    1025: ("affine", 205, "RT"), 1026: ("affine", 342, "R"), 1056: ("perspective", 96, "RTK"),
}
EXTRA_SIZES = {130: ("affine", 26, "RT")}  # failing pivots and right-hand sides only

# (n, j) of the failing pivots; the non-finite kinds at one interior and at the last position of each size
FAIL_POSITIONS = {22: (0, 7, 8, 15, 16, 21), 63: (56, 62), 130: (0, 63, 64, 71, 127, 128, 129), 258: (200, 257), 1026: (1024, 1025)}
FAIL_NONFINITE_AT = {22: (8, 21), 63: (56, 62), 130: (71, 129), 258: (200, 257), 1026: (1024, 1025)}
FAIL_KINDS = ("negative", "nan_diag", "inf_diag", "nan_offdiag")

# LAPACK's own constants over SIZES x SPD_FAMILIES (see the module comment).  Measured with `synthetic_scale`: 1.39 (wishart, 1056
# unknowns), 2.03 (cluster9, 1023), 14.2 (cluster9, 1056); with the handles' own scale_inv 1.41, 1.74, 14.2 -- and the device's own
# 2.22, 1.57, 14.4 -- (profiles/dense_accuracy.json, "constants").
C_FWD = 1.5
C_BWD = 2.25
C_FAC = 15.0
FWD_MARGIN, BWD_MARGIN, FAC_MARGIN = 8.0, 16.0, 16.0  # what the device may take of them


def bounds(family, kappa):
    """(forward, backward, factor) bounds of the device for a system of that family and condition number; None: recorded only"""
    stable = family in BACKWARD_STABLE
    return FWD_MARGIN * C_FWD * U * kappa, BWD_MARGIN * C_BWD * U if stable else None, FAC_MARGIN * C_FAC * U if stable else None


def fail_cases():
    out = []
    for n, js in FAIL_POSITIONS.items():
        for j in js:
            out.append((n, j, "negative"))
            if j in FAIL_NONFINITE_AT[n]:
                out += [(n, j, kind) for kind in FAIL_KINDS[1:]]
    return out


# ---------------------------------------------------------------------------------------------------------------- families

def _seed(family, n, seed):
    return [SPD_FAMILIES.index(family), n, seed]


def _orthogonal(rng, n):
    Q, R = np.linalg.qr(rng.normal(size=(n, n)))
    return Q * np.sign(np.diag(R))


def _unit_diagonal(M):
    d = 1.0 / np.sqrt(np.diag(M))
    M = M * d[:, None] * d[None, :]
    M = 0.5 * (M + M.T)
    np.fill_diagonal(M, 1.0)
    return M


def _with_spectrum(rng, lam):
    """Q diag(lam) Q^T rescaled to unit diagonal.  The rescaling moves the condition number: by a few per cent at n = 1000, by a factor
    of five at n = 6 when one entry of the dominant eigenvector is small.  Up to n = 64 Q is therefore drawn again (same generator)
    until the condition number is within a factor 2 of the spectrum's own."""
    n, want = lam.size, lam.max() / lam.min()
    for _ in range(100):
        Q = _orthogonal(rng, n)
        M = _unit_diagonal((Q * lam) @ Q.T)
        if n > 64:
            return M
        ev = np.linalg.eigvalsh(M)
        if ev[0] > 0 and 0.5 * want < ev[-1] / ev[0] < 2.0 * want:
            return M
    raise RuntimeError("no draw with the wanted condition number")


@functools.lru_cache(maxsize=8)
def spd(family, n, seed=0):
    """The matrix M of a family in scaled variables (read-only: cached)."""
    rng = np.random.default_rng(_seed(family, n, seed))
    if family == "wishart":
        A = rng.normal(size=(n, n))
        M = A @ A.T + n * np.eye(n)
    elif family.startswith("spectrum"):
        M = _with_spectrum(rng, np.logspace(0, -int(family[8:]), n))
    elif family == "cluster9":
        lam = np.ones(n)
        lam[: min(7, n // 2)] = 1e-9
        M = _with_spectrum(rng, rng.permutation(lam))
    elif family == "graded":
        M = _with_spectrum(rng, np.logspace(0, -4, n))
        d = rng.permutation(np.logspace(-3, 3, n))
        M = M * d[:, None] * d[None, :]
    else:
        raise KeyError(family)
    M.setflags(write=False)
    return M


def rhs_for(family, n, seed=0):
    return np.random.default_rng(_seed(family, n, seed) + [1]).normal(size=n)


def synthetic_scale(n, seed=0):
    """A scale_inv spanning 1e-6 .. 1e3 (the host test's stand-in for a handle's)."""
    return 10.0 ** np.random.default_rng([n, seed, 2]).uniform(-6.0, 3.0, size=n)


def plant(M, s):
    """S_p = M o (s s^T): what goes into the payload for the device to see (about) M."""
    return M * (s[:, None] * s[None, :])


def effective(S_p, rhs, s):
    """M_eff, b_eff: k_scale_system's arithmetic, operation for operation (the product of the two scales first, then one division)."""
    M_eff = S_p / (s[:, None] * s[None, :])
    return M_eff, rhs / s


def planted(M, b, s):
    """S_p, rhs as planted, and the M_eff, b_eff the device then factorises; rhs is chosen so that b_eff is b up to one rounding"""
    S_p = plant(M, s)
    rhs = b * s
    return (S_p, rhs) + effective(S_p, rhs, s)


def payload(S_p, upper=0.0):
    """the n x n payload of a symmetric S_p: column-major lower triangle, `upper` in the strict upper triangle (ignored on input)"""
    P = np.tril(S_p).T.copy()  # row-major view of the column-major matrix: P[c, r] = S_p[r, c], r >= c
    if upper != 0.0 or np.isnan(upper):
        P[np.tril_indices(S_p.shape[0], -1)] = upper
    return P.ravel()


# ---------------------------------------------------------------------------------------------------------------- truth

def truth(M, b, max_iter=12, info=None):
    """z with M z = b to (about) 2^-64 kappa: float64 Cholesky, iterative refinement with the residual and the sum in longdouble.
    info (a dict): "last" = |last correction|_inf / |z|_inf, "iterations"."""
    c = sl.cho_factor(M, lower=True)
    Ml, bl = M.astype(LD), b.astype(LD)
    z = sl.cho_solve(c, b).astype(LD)
    last = np.inf
    for it in range(max_iter):
        r = bl - Ml @ z
        dz = sl.cho_solve(c, r.astype(np.float64))
        z = z + dz
        rel = float(np.abs(dz).max() / np.abs(z).max())
        stalled = rel > 0.25 * last  # no longer contracting: the corrections are the rounding of the longdouble residual, ~2^-64 kappa
        last = rel
        if stalled or rel < 2.0 ** -66:
            break
    if info is not None:
        info["last"], info["iterations"] = last, it + 1
    return z


def kappa2(M):
    """|M|_2 |M^-1|_2.  The inverse's norm comes from the Cholesky factor, which is accurate for graded matrices too (eigvalsh of M
    itself loses the small eigenvalues of `graded` in the rounding of the large ones)."""
    n = M.shape[0]
    c = sl.cho_factor(M, lower=True)
    if n <= 300:
        inv = sl.cho_solve(c, np.eye(n))
        return float(np.linalg.eigvalsh(M)[-1] * np.linalg.eigvalsh(0.5 * (inv + inv.T))[-1])
    # Lanczos (a dense eigenvalue routine takes most of a second at n = 1000); a Ritz value at tol 1e-3 is far inside what a
    # condition number is used for here
    v0 = np.ones(n)
    top = ssl.eigsh(M, k=1, which="LA", v0=v0, tol=1e-3, return_eigenvectors=False)[0]
    op = ssl.LinearOperator((n, n), matvec=lambda x: sl.cho_solve(c, x), dtype=np.float64)
    top_inv = ssl.eigsh(op, k=1, which="LA", v0=v0, tol=1e-3, return_eigenvectors=False)[0]
    return float(top * top_inv)


def unit_scaled(M):
    """(D^-1 M D^-1, d) with d = sqrt(diag M): the matrix whose condition number governs a Cholesky solve of a graded M"""
    d = np.sqrt(np.diag(M))
    return M / (d[:, None] * d[None, :]), d


# ---------------------------------------------------------------------------------------------------------------- measures

def forward_error(z, z_true, d=1.0):
    """|z - z*|_inf / |z*|_inf; d: of d o z instead (the variables in which a graded system has a unit diagonal)"""
    z_true = np.asarray(z_true, dtype=LD) * d
    return float(np.abs(np.asarray(z, dtype=LD) * d - z_true).max() / np.abs(z_true).max())


def backward_error(M, b, z):
    """normwise: eta = |b - M z|_inf / (|M|_inf |z|_inf + |b|_inf), the residual in longdouble"""
    zl = np.asarray(z, dtype=LD)
    r = b.astype(LD) - M.astype(LD) @ zl
    return float(np.abs(r).max() / (np.abs(M).sum(axis=1).max() * np.abs(zl).max() + np.abs(b).max()))


def _slices(L, bits=20, count=3):
    """L = sum_k I_k[i, j] 2^(e[i] - (k + 1) bits) + (a remainder below 2^(e[i] - count bits)), I_k integers below 2^bits in float64"""
    big = np.abs(L).max(axis=1)
    e = np.where(big > 0, np.frexp(big)[1], 0)
    rest = np.ldexp(L, -e[:, None])  # |.| < 1, exact
    out = []
    for _ in range(count):
        rest = np.ldexp(rest, bits)
        top = np.trunc(rest)
        out.append(top)
        rest = rest - top  # exact
    return out, e


def factor_residual(L, M):
    """|L L^T - M|_F / |M|_F with the product formed exactly: a float64 product at n = 1000 carries rounding of the size of what is
    measured, and a longdouble product takes seconds.  The rows of L are cut into 20-bit integer slices under a row exponent; the
    product of two slices is a sum of n integers below 2^40, exact in float64 in any order for n < 8192 (BLAS); the slice products are
    added in longdouble.  Dropped: products of slices beyond 2^-60 of a row's largest entry."""
    n = L.shape[0]
    assert n < 8192
    L = np.tril(L)
    (s0, s1, s2), e = _slices(L)
    p01, p02 = s0 @ s1.T, s0 @ s2.T
    acc = (s0 @ s0.T).astype(LD)
    acc += np.ldexp((p01 + p01.T).astype(LD), -20)
    acc += np.ldexp((s1 @ s1.T + p02 + p02.T).astype(LD), -40)  # (the float64 sum here rounds at 2^-93 of the leading term)
    acc = np.ldexp(acc, (e[:, None] + e[None, :] - 40).astype(np.int32))
    R = acc - M.astype(LD)
    return float(np.sqrt((R * R).sum()) / np.sqrt((M.astype(LD) ** 2).sum()))


class Case:
    """One planted system: S_p, rhs for the payload; M_eff, b_eff as the device forms them; truth and condition number on demand.
    s: the scale_inv the device will divide by."""

    def __init__(self, family, n, s, M=None, b=None):
        self.family, self.n, self.s = family, n, np.asarray(s, dtype=np.float64)
        M = spd(family, n) if M is None else M
        b = rhs_for(family, n) if b is None else b
        self.S_p, self.rhs, self.M_eff, self.b_eff = planted(M, b, self.s)
        self.truth_info = {}

    @functools.cached_property
    def z_true(self):
        return truth(self.M_eff, self.b_eff, info=self.truth_info)

    @functools.cached_property
    def kappa(self):
        return kappa2(self.M_eff)

    @functools.cached_property
    def scaled(self):
        """(kappa_2 of M_eff rescaled to unit diagonal, the scaling d): graded systems"""
        Ms, d = unit_scaled(self.M_eff)
        return kappa2(Ms), d

    def measure(self, z, L=None):
        """the measures of a computed solution z (and factor L): fwd, bwd, fac (None without L), kappa; graded: also fwd_scaled, the
        forward error of d o z, and kappa_scaled"""
        out = {"kappa": self.kappa, "fwd": forward_error(z, self.z_true), "bwd": backward_error(self.M_eff, self.b_eff, z),
               "fac": None if L is None else factor_residual(L, self.M_eff)}
        if self.family == "graded":
            ks, d = self.scaled
            out["kappa_scaled"], out["fwd_scaled"] = ks, forward_error(z, self.z_true, d)
        return out

    def check(self, m, what=""):
        """assert the device's bounds on measures m (see `bounds`); prints the figures first"""
        fwd, bwd, fac = bounds(self.family, m["kappa"])
        print("{} n={} {}: kappa {:.3e} fwd {:.3e} (bound {:.3e}) bwd {:.3e} (bound {}) fac {} (bound {})".format(
            what, self.n, self.family, m["kappa"], m["fwd"], fwd, m["bwd"], bwd, m["fac"], fac))
        assert m["fwd"] <= fwd
        if bwd is not None:
            assert m["bwd"] <= bwd
        if fac is not None and m["fac"] is not None:
            assert m["fac"] <= fac
        if self.family == "graded":
            # The 2-norm bound is void here (u kappa_2 > 1).  A Cholesky solve of D M D is as accurate in the variables d o z as one of
            # the unit-diagonal M (van der Sluis; Demmel 1989): the same bound with that matrix's condition number, on d o z.
            print("    scaled: kappa {:.3e} fwd {:.3e}".format(m["kappa_scaled"], m["fwd_scaled"]))
            assert m["fwd_scaled"] <= FWD_MARGIN * C_FWD * U * m["kappa_scaled"]


def lapack(M, b):
    """LAPACK's float64 solve and factor: (z, L)"""
    c, _ = sl.cho_factor(M, lower=True)
    return sl.cho_solve((c, True), b), np.tril(c)


# ---------------------------------------------------------------------------------------------------------------- failing systems

def cholesky_ld(M):
    """Cholesky in longdouble, column by column: (L, j) with j the first pivot that is not a positive finite number (n: none)"""
    n = M.shape[0]
    L = np.zeros((n, n), dtype=LD)
    A = np.asarray(M, dtype=LD)
    for k in range(n):
        col = A[k:, k] - L[k:, :k] @ L[k, :k]
        if not (col[0] > 0 and np.isfinite(col[0])):
            return L, k
        L[k:, k] = col / np.sqrt(col[0])
    return L, n


def indefinite(M, j, kind):
    """A copy of the SPD matrix M whose leading minor of order j is untouched and whose pivot j fails (see the module comment).
    "negative": sum_k L[j, k]^2 = m^T A^-1 m (A the leading minor, m = M[j, :j]) comes from `truth`, i.e. in extended precision."""
    M = np.array(M)
    if kind == "negative":
        s = LD(0.0)
        if j > 0:
            m = M[j, :j]
            s = (m.astype(LD) * truth(M[:j, :j], m)).sum()
        M[j, j] = float(s - LD(0.5))
    elif kind == "nan_diag":
        M[j, j] = np.nan
    elif kind == "inf_diag":
        M[j, j] = np.inf
    elif kind == "nan_offdiag":
        M[j, j // 2] = M[j // 2, j] = np.nan
    else:
        raise KeyError(kind)
    return M

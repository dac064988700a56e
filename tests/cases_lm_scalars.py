"""
Models for the scalar side of the trust-region loop (csrc/satba_lm.h, satba/trf.py): rows (a, b, c, g0, g1, Delta) of
min q(p) = 0.5 p^T B p + g^T p, |p| <= Delta, B = [[a, b], [b, c]], by family, with a 400-bit solver of the same problem
as the reference, and grids of special values for update_tr_radius and check_termination.  Shared by
tests/test_lm_scalars_host.py (which recomputes the reference) and tests/test_gpu_lm_scalars.py (which reads it from
tests/golden/lm_scalars.npz, written by tools/gen_golden_lm_scalars.py and checked against the recomputation by the host test).

Families (FAMILIES; `corpus()` returns the rows and the family index of each):

ordinary   A A^T and A + A^T with cond(B) <= 1e8, |g| over 1e-12 .. 1e6, Delta over 1e-8 .. 1e4: Newton steps that fit, steps that
           do not, and radii within 1e-12 (relative) of the Newton step's length, on both sides and on it.
hard       the hard case and its neighbours, built from small integers and powers of two so that every quantity is exact:
           indefinite and negative definite B with g exactly along the larger eigenvector (interior part shorter and longer than
           Delta), B = lambda I for every sign of lambda, b = 0 with a > c, a < c, a == c, g = 0, the zero matrix.
stall      diag(-L, L2) and rotations of it with |g| / Delta = 2^-60 .. 2^-40 of L: the secular bracket [-l1, |g| / Delta - l1]
           is a handful of floats wide or a single one.  Row 0 is diag(-1, 1), g = (1e-20, 0), Delta = 1.
singular   rank-one B = s v v^T (entries rounded) with g = -t v in its range; the same with a second eigenvalue of +-2^-50 .. 2^-30
           of the first; exact versions from small integers and powers of two (det == 0 exactly).  g stays in the range of B up to
           rounding: with a large component of g along a direction whose curvature is rounding noise the optimum is not determined
           by the float64 inputs.
scales     moderate rows (entries of B within 1e-2 .. 1e2, |g_i| and Delta within 1e-2 .. 1e2) with the objective multiplied by 1e+-150
           (B and g), with the step's unit multiplied by 1e+-150 (Delta, and B divided), and with B, g, Delta times 1e+-50, 1e+-150,
           1e+-100.  All of them are expected to stay finite, feasible and optimal: every square and product the functions need for
           the result (a c, b b, d^2 + b^2, Delta^2, |p|^2, c g, |g| / Delta) stays a normal float64, i.e. every entry stays within
           1e-153 .. 1e153.  |p|^3 in the secular derivative does overflow or underflow at Delta ~ 1e+-150: the iteration then
           bisects, and the rows show that it still ends on the optimum.  Not generated, because no formula that squares B's entries
           can hold there: entries of B (or g, or Delta) beyond 1e+-153, where a c and d^2 + b^2 overflow or go subnormal.
radius     Delta = 0 (the step is exactly (0, 0), no Newton flag); the smallest subnormal with diagonal B and g along an axis (the
           only models whose optimum is representable at that radius: its components are 0 or +-Delta); Delta = 2^-1000 and
           2^-600 on moderate models; Delta = inf with positive definite B (the Newton step).
nonfinite  NaN or +-inf in any slot of moderate models (Delta = inf only with B that is not positive definite: the minimum is
           unbounded).  Nothing is asserted but that the function returns without the Newton flag.
"""
import functools
import hashlib
import itertools
import os

import numpy as np

FAMILIES = ("ordinary", "hard", "stall", "singular", "scales", "radius", "nonfinite")
EPS = 2.0 ** -52
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm_scalars.npz")


def _sym(l1, l2, th):
    """R diag(l1, l2) R^T in float64, R the rotation by th"""
    cs, sn = np.cos(th), np.sin(th)
    return l1 * sn * sn + l2 * cs * cs, (l2 - l1) * cs * sn, l1 * cs * cs + l2 * sn * sn


def _vec(rng, norm):
    th = rng.uniform(0, 2 * np.pi)
    return norm * np.cos(th), norm * np.sin(th)


def _ordinary_B(rng):
    while True:
        A = rng.normal(size=(2, 2)) * 10 ** rng.uniform(-2, 2, size=(2, 1))
        B = A @ A.T if rng.random() < 0.7 else A + A.T
        if rng.random() < 0.3:  # spread the condition numbers over 1 .. 1e8, which A A^T alone rarely reaches
            l2 = 10 ** rng.uniform(-3, 3)
            a, b, c = _sym(l2 * 10 ** -rng.uniform(0, 7.9) * rng.choice([1, 1, -1]), l2, rng.uniform(0, np.pi))
            B = np.array([[a, b], [b, c]])
        w = np.abs(np.linalg.eigvalsh(B))
        if w.min() > 0 and w.max() / w.min() <= 1e8:
            return B[0, 0], B[0, 1], B[1, 1]


def ordinary_rows(rng, n=2600, n_edge=135):
    rows = []
    for _ in range(n):
        a, b, c = _ordinary_B(rng)
        g0, g1 = _vec(rng, 10 ** rng.uniform(-12, 6))
        rows.append((a, b, c, g0, g1, 10 ** rng.uniform(-8, 4)))
    offs = (0.0, 1e-12, -1e-12, 4e-16, -4e-16, 1e-8, -1e-8, 1e-6, -1e-6)
    k = 0
    while k < n_edge:
        a, b, c = _ordinary_B(rng)
        if not (a > 0 and a * c - b * b > 0):
            continue
        g0, g1 = _vec(rng, 10 ** rng.uniform(-6, 6))
        p = np.linalg.solve(np.array([[a, b], [b, c]]), [-g0, -g1])
        rows.append((a, b, c, g0, g1, np.hypot(*p) * (1 + offs[k % len(offs)])))
        k += 1
    return np.array(rows)


def hard_rows(rng):
    rows = []
    vs = [(1, 0), (0, 1), (1, 1), (1, 2), (3, 1), (2, -3), (-5, 2), (4, 7)]
    for (m, n), (l1, l2), t, D in itertools.product(vs, [(-2, 3), (-4, -1), (-1, 0), (0, 2), (-3, -3), (-8, 0.5)], (2.0 ** -3, -2.0 ** -30),
                                                    (2.0 ** -6, 1.0, 64.0)):
        # B = l1 v1 v1^T + l2 v2 v2^T with v2 = (m, n), v1 = (-n, m): integers, exact; g = t v2 exactly along the larger eigenvector
        rows.append((l1 * n * n + l2 * m * m, (l2 - l1) * m * n, l1 * m * m + l2 * n * n, t * m, t * n, D))
    for lam, (g0, g1), D in itertools.product((-3.0, -2.0 ** -20, 0.0, 2.0 ** -20, 5.0), [(0, 0), (1, 0), (0, -2), (3, 4), (1e-9, -1e-9), (-7e5, 2e5)],
                                              (1e-3, 1.0, 1e3)):
        rows.append((lam, 0.0, lam, g0, g1, D))  # lambda I (lambda = 0: the zero matrix)
    for (a, c), (g0, g1), D in itertools.product([(2, 1), (1, 2), (2, 2), (-1, -2), (-2, -1), (1, -1), (-1, 1), (0, 1), (1, 0), (0, -1), (-1, 0)],
                                                 [(0, 0), (1, 0), (0, 1), (-1, 1e-3), (1e-3, -1), (0.3, 0.4)], (0.01, 0.7, 30.0)):
        rows.append((a, 0.0, c, g0, g1, D))  # b = 0
    for _ in range(150):  # g = 0 on every kind of B
        kind = rng.integers(4)
        l2 = 10 ** rng.uniform(-3, 3)
        l1 = l2 * (10 ** -rng.uniform(0, 6) if kind == 0 else -10 ** rng.uniform(-6, 1) if kind == 1 else 0.0)
        a, b, c = _sym(l1, l2, rng.uniform(0, np.pi)) if kind < 3 else _sym(-l2, -l2 * 10 ** -rng.uniform(0, 3), rng.uniform(0, np.pi))
        rows.append((a, b, c, 0.0, 0.0, 10 ** rng.uniform(-6, 3)))
    return np.array(rows, dtype=np.float64)


def stall_rows(rng, n=360):
    rows = [(-1.0, 0.0, 1.0, 1e-20, 0.0, 1.0)]
    while len(rows) < n:
        L = 10 ** rng.uniform(-3, 8)
        L2 = L * 10 ** rng.uniform(-2, 2) * rng.choice([1, 1, 1, -1e-3])  # (the last: both eigenvalues negative, L2 > -L)
        D = 10 ** rng.uniform(-6, 3)
        gn = L * D * 2.0 ** -rng.uniform(40, 60)
        kind = len(rows) % 3
        a, b, c = (-L, 0.0, L2) if kind == 0 else (L2, 0.0, -L) if kind == 1 else _sym(-L, L2, rng.uniform(0, np.pi))
        g0, g1 = _vec(rng, gn)
        if rng.random() < 0.2:  # along one axis
            g0, g1 = (gn, 0.0) if rng.random() < 0.5 else (0.0, -gn)
        rows.append((a, b, c, g0, g1, D))
    return np.array(rows)


def singular_rows(rng, n_rank1=100, n_second=140, n_exact=60):
    rows = []
    for k in range(n_rank1 + n_second):
        v = rng.normal(size=2)
        B = np.outer(v, v)
        if k >= n_rank1:
            w = np.array([-v[1], v[0]])
            B = B + np.outer(w, w) * (rng.choice([-1, 1]) * 2.0 ** -rng.uniform(30, 50))
        B = B * 10 ** rng.uniform(-6, 6)
        g = -v * 10 ** rng.uniform(-9, 3)
        rows.append((B[0, 0], B[0, 1], B[1, 1], g[0], g[1], 10 ** rng.uniform(-8, 4)))
    for _ in range(n_exact):  # small integers and powers of two: det == 0 exactly, g exactly in the range
        m, n = rng.integers(-9, 10, size=2)
        if m == 0 and n == 0:
            m = 1
        s, t = 2.0 ** rng.integers(-20, 21), rng.choice([-1, 1]) * 2.0 ** rng.integers(-30, 11)
        D = 2.0 ** rng.integers(-26, 14) * rng.choice([1.0, 1.5, 1.0 + 2.0 ** -30])
        rows.append((s * m * m, s * m * n, s * n * n, t * m, t * n, D))
    return np.array(rows, dtype=np.float64)


def scales_rows(rng, n=60):
    rows = []
    for _ in range(n):
        l2 = 10 ** rng.uniform(-1, 1.5)
        a, b, c = _sym(l2 * 10 ** -rng.uniform(0, 1) * rng.choice([1, 1, -1]), l2, rng.uniform(0.2, 1.3))  # entries within 1e-2 .. 1e2
        g0, g1 = _vec(rng, 10 ** rng.uniform(-1.5, 1.5))
        g0, g1 = np.sign(g0) * max(abs(g0), 1e-2), np.sign(g1) * max(abs(g1), 1e-2)
        D = 10 ** rng.uniform(-2, 2)
        for s in (1e150, 1e-150):
            rows.append((a * s, b * s, c * s, g0 * s, g1 * s, D))  # the objective times s
        for u in (1e150, 1e-150):
            rows.append((a / u, b / u, c / u, g0, g1, D * u))  # the step's unit times u
        rows.append((a * 1e50, b * 1e50, c * 1e50, g0 * 1e150, g1 * 1e150, D * 1e100))
        rows.append((a * 1e-50, b * 1e-50, c * 1e-50, g0 * 1e-150, g1 * 1e-150, D * 1e-100))
    return np.array(rows)


def _moderate(rng):
    l2 = 10 ** rng.uniform(-1, 1)
    kind = rng.integers(3)
    l1 = l2 * (10 ** -rng.uniform(0, 2) if kind == 0 else -10 ** rng.uniform(-2, 1) if kind == 1 else 0.3)
    return _sym(l1, l2, rng.uniform(0, np.pi)) + _vec(rng, 10 ** rng.uniform(-2, 2))


def radius_rows(rng):
    rows = [_moderate(rng) + (0.0,) for _ in range(20)]
    rows += [(1.0, 0.0, 1.0, 0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (-1.0, 0.0, 1.0, 1e-20, 0.0, 0.0), (-1.0, 0.5, -2.0, 0.0, 0.0, 0.0)]
    sub = 5e-324
    for (a, c), (g0, g1) in itertools.product([(2.0, 1.0), (1.0, 2.0), (-1.0, 3.0), (3.0, -1.0), (0.0, 0.0), (-2.0, -2.0)],
                                              [(1.0, 0.0), (-1e-3, 0.0), (0.0, 7.0), (0.0, -1e5)]):
        rows.append((a, 0.0, c, g0, g1, sub))
    for D in (2.0 ** -1000, 2.0 ** -600, 2.0 ** -481, 2.0 ** -480):
        rows += [_moderate(rng) + (D,) for _ in range(12)]
    while len(rows) < 130:  # no radius at all: the Newton step of a positive definite model
        r = _moderate(rng)
        if r[0] > 0 and r[0] * r[2] - r[1] * r[1] > 1e-3 * r[0] * r[2]:
            rows.append(r + (np.inf,))
    return np.array(rows)


def nonfinite_rows(rng):
    rows = []
    for base in ((2.0, 0.5, 1.0, 0.3, -0.4, 1.0), (2.0, 0.5, 1.0, 30.0, -40.0, 1.0), (-1.0, 0.5, 2.0, 0.3, -0.4, 1.0), (1.0, 1.0, 1.0, -1.0, -1.0, 2.0),
                 (0.0, 0.0, 0.0, 0.0, 0.0, 1.0)):
        for slot, v in itertools.product(range(6), (np.nan, np.inf, -np.inf)):
            if slot == 5 and v == np.inf and base[0] > 0 and base[0] * base[2] - base[1] * base[1] > 0:
                continue  # (a radius edge: family `radius`)
            r = list(base)
            r[slot] = v
            rows.append(tuple(r))
    for v, w in itertools.product((np.nan, np.inf, -np.inf), repeat=2):  # two slots at once, the radius among them
        rows += [(v, 0.0, w, 1.0, 1.0, 1.0), (1.0, 0.0, 1.0, v, w, np.inf), (1.0, v, 1.0, 1.0, 1.0, w), (v, v, v, w, w, np.inf)]
    return np.array(rows)


@functools.lru_cache(maxsize=None)
def corpus():
    """(rows [n, 6], family index [n]): the same arrays for every caller of a session, read-only"""
    gens = (ordinary_rows, hard_rows, stall_rows, singular_rows, scales_rows, radius_rows, nonfinite_rows)
    parts = [g(np.random.default_rng(1000 + k)) for k, g in enumerate(gens)]
    rows = np.ascontiguousarray(np.concatenate(parts), dtype=np.float64)
    fam = np.concatenate([np.full(len(p), k) for k, p in enumerate(parts)])
    rows.setflags(write=False)
    fam.setflags(write=False)
    return rows, fam


def corpus_digest():
    return hashlib.sha256(corpus()[0].tobytes()).hexdigest()


def checked(rows):
    """rows whose values are compared: finite B and g, Delta > 0; Delta = inf only where B is positive definite (family `radius`)"""
    with np.errstate(invalid="ignore"):
        pd = (rows[:, 0] > 0) & (rows[:, 0] * rows[:, 2] - rows[:, 1] * rows[:, 1] > 1e-3 * rows[:, 0] * rows[:, 2])
    return np.isfinite(rows[:, :5]).all(1) & (rows[:, 5] > 0) & (np.isfinite(rows[:, 5]) | pd)


SPECIAL = (0.0, -0.0, 5e-324, -5e-324, 1.0, -1.0, np.inf, -np.inf, np.nan)


@functools.lru_cache(maxsize=None)
def radius_grid():
    """Delta, actual, predicted, step_norm, bound_hit over the special values"""
    return np.array([v + (float(h),) for v in itertools.product(SPECIAL, repeat=4) for h in (0, 1)])


@functools.lru_cache(maxsize=None)
def term_grid():
    """dF, F, dx_norm, x_norm, ratio over the special values (and 0.25, the threshold of the ratio), ftol and xtol over 0, tiny, 1e-8, 1, inf, NaN"""
    tol = (0.0, 5e-324, 1e-8, 1.0, np.inf, np.nan)
    rng = np.random.default_rng(7)
    full = np.array(list(itertools.product(SPECIAL, SPECIAL, SPECIAL, SPECIAL, SPECIAL + (0.25, 0.5), (1e-8,), (1e-8,))))
    pick = np.array(list(itertools.product(tol, tol)))
    some = full[rng.choice(len(full), 6000, replace=False)].copy()
    some[:, 5:] = pick[rng.integers(len(pick), size=len(some))]
    return np.concatenate([full, some])


# ----------------------------------------------------------------------------- the 400-bit reference

def reference(row):
    """
    (q*, scale, flag) of one row with finite B, g and Delta > 0 (mpmath numbers, flag an int), in 400-bit arithmetic (mpmath): the Newton step when B is positive
    definite and it fits, otherwise the eigen-decomposition and the root of the secular equation (bracketed Newton on
    1 / |p(mu)| - 1 / Delta, which is concave and increasing; bisection when an iterate leaves the bracket), the hard case (no
    component of g along v1, interior part no longer than Delta) explicitly.  scale = |g| Delta + max |B| Delta^2 / 2.
    flag: 1 / 0 where exact arithmetic's answer to "a Newton step that fits?" is decisive, -1 where either value is accepted.
    Decisive for "yes or no by the radius": l1 / l2 > 1e-12 and | |p_newton| / Delta - 1 | > 1e-9.  Decisive "no": B exactly zero, or
    l1 < -1e-12 max(|l1|, |l2|) (not positive definite by a margin no rounding bridges).  Everything between is undecided.
    """
    import mpmath as mp

    with mp.workprec(400):
        a, b, c, g0, g1, D = (mp.mpf(float(v)) for v in row)
        h, d = (a + c) / 2, (a - c) / 2
        r = mp.sqrt(d * d + b * b)
        l1, l2 = h - r, h + r
        if r == 0:
            v1 = (mp.mpf(1), mp.mpf(0))
        elif d > 0:
            n = mp.sqrt((d + r) ** 2 + b * b)
            v1 = (-b / n, (d + r) / n)
        else:
            n = mp.sqrt((d - r) ** 2 + b * b)
            v1 = ((d - r) / n, b / n)
        v2 = (-v1[1], v1[0])
        det = a * c - b * b  # exact: two 53-bit factors
        if a > 0 and det > 0:
            l1 = det / l2  # (h - r cancels: a thin B keeps its relative accuracy this way)
        elif det == 0:
            l1 = mp.mpf(0) if h >= 0 else l1
            l2 = l2 if h >= 0 else mp.mpf(0)
        c1, c2 = g0 * v1[0] + g1 * v1[1], g0 * v2[0] + g1 * v2[1]
        gn = mp.sqrt(c1 * c1 + c2 * c2)
        # a component 2^-350 of |g| is the eigenvectors' own rounding at 400 bits (float64 inputs give exactly 0 or far more): g exactly
        # along an eigenvector has none along the other
        c1 = c1 if abs(c1) > mp.mpf(2) ** -350 * gn else mp.mpf(0)
        c2 = c2 if abs(c2) > mp.mpf(2) ** -350 * gn else mp.mpf(0)
        scale = gn * D + max(abs(a), abs(b), abs(c)) * D * D / 2 if D != mp.inf else mp.inf
        big = max(abs(l1), abs(l2))

        def q(q1, q2):
            return (l1 * q1 * q1 + l2 * q2 * q2) / 2 + c1 * q1 + c2 * q2

        flag = -1
        if big == 0 or l1 < -mp.mpf("1e-12") * big:
            flag = 0
        if l1 > 0:
            n1, n2 = -c1 / l1, -c2 / l2
            nn = mp.sqrt(n1 * n1 + n2 * n2)
            fits = nn <= D
            if l1 / l2 > mp.mpf("1e-12") and (D == mp.inf or abs(nn / D - 1) > mp.mpf("1e-9")):
                flag = int(fits)
            if fits:
                return q(n1, n2), scale, flag
        assert D != mp.inf
        lo = max(mp.mpf(0), -l1)
        if gn == 0:
            return l1 * D * D / 2 if l1 < 0 else mp.mpf(0), scale, flag
        if c1 == 0 and (l2 + lo == 0 or abs(c2) <= (l2 + lo) * D):
            if l2 + lo == 0:  # lambda I, lambda <= 0: straight down the gradient
                return l1 * D * D / 2 - gn * D, scale, flag
            q2 = -c2 / (l2 + lo)
            return q(mp.sqrt(D * D - q2 * q2), q2), scale, flag

        def at(mu):
            q1 = c1 / (l1 + mu) if c1 != 0 else mp.mpf(0)
            q2 = c2 / (l2 + mu) if c2 != 0 else mp.mpf(0)
            return q1, q2, mp.sqrt(q1 * q1 + q2 * q2)

        mu_lo, mu_hi = lo, lo + gn / D  # |p(mu_hi)| <= |g| / (l1 + mu_hi) <= Delta; at mu_lo (a pole, or the long interior part) |p| > Delta
        mu = mu_hi
        for _ in range(3000):
            q1, q2, nrm = at(mu)
            if nrm > D:
                mu_lo = mu
            else:
                mu_hi = mu
            if mu_hi - mu_lo <= mp.mpf(2) ** -380 * mu_hi:
                break
            dphi = ((q1 * q1 / (l1 + mu) if c1 != 0 else 0) + (q2 * q2 / (l2 + mu) if c2 != 0 else 0)) / nrm ** 3
            new = mu - (1 / nrm - 1 / D) / dphi
            if not mu_lo < new < mu_hi:
                new = (mu_lo + mu_hi) / 2
            elif abs(new - mu) <= mp.mpf(2) ** -390 * mu_hi:  # converged from one side: close the bracket around the root
                side = new + (mu_hi - mu_lo) * mp.mpf(2) ** -200 if nrm > D else new - (mu_hi - mu_lo) * mp.mpf(2) ** -200
                new = side if mu_lo < side < mu_hi else new
            mu = new
        else:
            raise AssertionError("the reference's secular iteration did not converge: {}".format(tuple(map(float, row))))
        q1, q2, nrm = at(mu_hi)
        assert abs(nrm / D - 1) < mp.mpf(2) ** -300, (tuple(map(float, row)), float(nrm / D - 1))
        return q(-q1, -q2), scale, flag


def model_value(row, p):
    """q(p) of the float64 step p in 400-bit arithmetic"""
    import mpmath as mp

    with mp.workprec(400):
        a, b, c, g0, g1, _ = (mp.mpf(float(v)) for v in row)
        p0, p1 = mp.mpf(float(p[0])), mp.mpf(float(p[1]))
        return (a * p0 * p0 + 2 * b * p0 * p1 + c * p1 * p1) / 2 + g0 * p0 + g1 * p1


def compute_reference():
    """(qrel, qstar, flag) for every row of the corpus: q* / scale and q* as float64 (hi, lo) pairs (q* itself is used only where
    Delta = inf, scale with it; at subnormal radii it is no float64), NaN and -1 on the rows that are not compared"""
    import mpmath as mp

    rows, _ = corpus()
    ok = checked(rows)
    qs = np.full((len(rows), 2), np.nan)
    qrel = np.full((len(rows), 2), np.nan)
    flag = np.full(len(rows), -1, dtype=np.int64)
    with mp.workprec(400):
        for i in np.flatnonzero(ok):
            qstar, sc, fl = reference(rows[i])
            for dst, v in ((qs, qstar), (qrel, qstar / sc if sc != mp.inf and sc != 0 else mp.mpf(0))):
                hi = float(v)
                dst[i] = hi, float(v - mp.mpf(hi))
            flag[i] = fl
    return qrel, qs, flag


@functools.lru_cache(maxsize=None)
def golden_reference():
    g = np.load(GOLDEN)
    assert str(g["digest"]) == corpus_digest(), "tests/golden/lm_scalars.npz belongs to another corpus: run tools/gen_golden_lm_scalars.py"
    return g["qrel"], g["qstar"], g["flag"]


def check_rows(rows, fam, out, ref, name, tol=None):
    """
    The four properties on `out` (p0, p1, newton per row) against ref = (qrel, qstar, flag): finite, feasible
    (|p| <= Delta (1 + 8 eps)), optimal (q(p) - q* <= tol eps scale, tol = 64 unless TOL names the family) and the Newton flag where it
    is decisive; on the rows that are not compared only that the flag is down.  Returns {family: worst (q(p) - q*) / (eps scale)}
    and the number of rows whose flag was undecided; raises AssertionError with every failing row's index.
    """
    import mpmath as mp

    qrel, qstar, flag = ref
    ok = checked(rows)
    worst = {f: 0.0 for f in FAMILIES}
    bad = []
    with mp.workprec(400):
        for i in range(len(rows)):
            p0, p1, nt = out[i, 0], out[i, 1], out[i, 2]
            f = FAMILIES[fam[i]]
            if not ok[i]:
                if rows[i, 5] == 0 and np.isfinite(rows[i]).all():
                    if not (p0 == 0 and p1 == 0 and nt == 0):
                        bad.append((i, f, "Delta = 0 gives {} {} {}".format(p0, p1, nt)))
                elif nt != 0:
                    bad.append((i, f, "Newton flag on a non-finite model"))
                continue
            if not (np.isfinite(p0) and np.isfinite(p1)):
                bad.append((i, f, "step {} {}".format(p0, p1)))
                worst[f] = np.inf
                continue
            D = mp.mpf(float(rows[i, 5]))
            nrm = mp.sqrt(mp.mpf(float(p0)) ** 2 + mp.mpf(float(p1)) ** 2)
            if nrm > D * (1 + 8 * mp.mpf(EPS)):
                bad.append((i, f, "|p| / Delta - 1 = {:.3e}".format(float(nrm / D - 1))))
            if np.isfinite(rows[i, 5]):
                a, b, c, g0, g1 = (mp.mpf(float(v)) for v in rows[i, :5])
                scale = mp.sqrt(g0 * g0 + g1 * g1) * D + max(abs(a), abs(b), abs(c)) * D * D / 2
                if scale == 0:  # the zero model: every step is optimal
                    continue
                exc = float((model_value(rows[i], (p0, p1)) / scale - mp.mpf(float(qrel[i, 0])) - mp.mpf(float(qrel[i, 1]))) / mp.mpf(EPS))
            else:  # Delta = inf: the Newton step itself, to 64 eps of |q*|
                qs = mp.mpf(float(qstar[i, 0])) + mp.mpf(float(qstar[i, 1]))
                exc = float((model_value(rows[i], (p0, p1)) - qs) / (mp.mpf(EPS) * max(abs(qs), mp.mpf(2) ** -1000)))
            worst[f] = max(worst[f], exc)
            if not exc <= (tol or TOL).get(f, 64.0):
                bad.append((i, f, "q(p) - q* = {:.4g} eps scale".format(exc)))
            if flag[i] >= 0 and int(nt) != flag[i]:
                bad.append((i, f, "Newton flag {} where exact arithmetic says {}".format(int(nt), flag[i])))
    if bad:
        raise AssertionError("{}: {} rows fail, worst per family (eps scale) {}\n".format(name, len(bad), worst) + "\n".join(
            "row {} ({}) {}: {}".format(i, f, tuple(rows[i]), why) for i, f, why in bad[:40]))
    return worst


# tolerance of q(p) - q* in eps scale per family where it is not 64 (none: every family holds 64)
TOL = {}


# ----------------------------------------------------------------------------- the stand-alone host compilation

def build_dump(directory, sanitize):
    """tests/host/lm_scalars_dump.cpp -> (path, whether it carries the address and undefined-behaviour sanitizers), None without a compiler.
    A sanitizer build that does not link, or that cannot start here (an empty run fails), gives way to a plain one."""
    import shutil
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = next((shutil.which(c) for c in (os.environ.get("CXX"), "g++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    if cxx is None:
        return None
    exe = os.path.join(str(directory), "lm_scalars_dump")
    base = [cxx, "-std=c++17", "-O1", "-I", os.path.join(root, "sat-bundleadjust_amd", "csrc"), os.path.join(root, "tests", "host", "lm_scalars_dump.cpp"), "-o", exe]
    if sanitize:
        r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
        if r.returncode == 0 and subprocess.run([exe, "rows"], input=b"", capture_output=True).returncode == 0:
            return exe, True
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe, False


def run_dump(exe, mode, rows):
    import subprocess

    r = subprocess.run([exe, mode], input=np.ascontiguousarray(rows, dtype=np.float64).tobytes(), capture_output=True)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-3000:]
    return np.frombuffer(r.stdout, dtype=np.float64).reshape(len(rows), -1)

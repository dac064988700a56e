"""
Cases, restatement and metrics of the affine fundamental matrices from RPCs (satba.rpc_utils, csrc/satba_fundamental.h), shared by
tools/gen_golden_fundamental.py (which records the reference's matches_from_rpc and affine_fundamental_matrix into
tests/golden/ft_fundamental.npz), the host test (test_fundamental_host.py) and the GPU tests (test_gpu_fundamental*.py).

* Cases: both ordered pairs of the two shipped RPCs x the three crops of cases_camapprox.CROPS at n = 5, and the (0, 1) full crop
  at n = 2, 3, 7 and MAX_N (7^3 = 343 nodes: more than one pass of the 256 lanes).
* `restate` is a numpy restatement of the device route on a set of matches: means, the two-pass centred scatter matrix, cyclic
  Jacobi (or numpy.linalg.eigh), the sign rule and the rank test.  `restate_matches` builds the matches with the oracle's
  localisation.  The distance of the restatement to the reference's SVD route is the yardstick of the device tolerances.
* Metric.  Scale and sign of a fundamental matrix mean nothing, so matrices are compared by what the epipolar gate sees: the signed
  residual in pixels (F20 x1 + F21 y1 + F02 x2 + F12 y2 + F22) / hypot(F02, F12) on the stored matches of the case and on the four
  corners of the region paired with their stored partners, the global sign aligned first.
"""
import os

import numpy as np

import cases_camapprox as CC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ft_fundamental.npz")
MAX_N = 11            # csrc/satba_fundamental.h, FND_MAX_N
RANK_TOL = 1e-12      # csrc/satba_camapprox.h, CAM_RANK_TOL
PX_CAP = CC.PX_CAP    # the project's parity level in pixels
SOLVE_MARGIN = 10.0   # device against SVD on its own matches: one decimal order over the yardstick (summation order, fma)
LOC_TOL_DEG = 1e-9    # the device localisation is held to the oracle within this (test_gpu_rpcfit.py, test_gpu_octants.py)
# (image i, image j, crop, n)
CASES = [(i, 1 - i, c, 5) for i in (0, 1) for c in ("full", "c500", "c50")] + [(0, 1, "full", n) for n in (2, 3, 7, MAX_N)]
HEALTHY = CASES[:6]


def key(case):
    return "p{}{}_{}_n{}".format(*case)


class Rpc(CC.OracleRpc):
    """cases_camapprox.OracleRpc with the attribute matches_from_rpc reads besides alt_offset"""

    def __init__(self, r):
        super().__init__(r)
        self.alt_scale = r.alt_scale


def roi(case):
    """(x, y, w, h) of the case in image i"""
    return CC.CROPS[case[2]]


def mesh(r, region, n):
    """col, row, alt of the n^3 nodes (columns fastest, altitudes slowest): ref:bundle_adjust/s2p/rpc_utils.py:218-221, 241"""
    x, y, w, h = region
    cols = np.linspace(x + (1.0 / (2 * n)) * w, x + ((2 * n - 1.0) / (2 * n)) * w, n)
    rows = np.linspace(y + (1.0 / (2 * n)) * h, y + ((2 * n - 1.0) / (2 * n)) * h, n)
    alts = np.linspace(r.alt_offset - r.alt_scale, r.alt_offset + r.alt_scale, n)
    a, ro, c = np.meshgrid(alts, rows, cols, indexing="ij")
    return c.reshape(-1), ro.reshape(-1), a.reshape(-1)


def restate_matches(ri, rj, region, n, localization=None):
    """(n^3, 4) x1, y1, x2, y2; localization: callable (col, row, alt) -> lon, lat (default: the oracle's, through ri)"""
    col, row, alt = mesh(ri, region, n)
    lon, lat = (localization or Rpc(ri).localization)(col, row, alt)
    x1, y1 = ri.projection(lon, lat, alt)
    x2, y2 = rj.projection(lon, lat, alt)
    return np.vstack([x1, y1, x2, y2]).T


def corner_matches(ri, rj, region):
    """the four corners of the region at alt_offset of ri (x1, y1: the corner itself) and their partners in image j"""
    x, y, w, h = region
    col, row = np.array([x, x + w, x, x + w]), np.array([y, y, y + h, y + h])
    alt = np.full(4, ri.alt_offset)
    lon, lat = Rpc(ri).localization(col, row, alt)
    x2, y2 = rj.projection(lon, lat, alt)
    return np.vstack([col, row, x2, y2]).T


def f5(F):
    F = np.asarray(F, dtype=np.float64)
    return F if F.shape == (5,) else np.array([F[0, 2], F[1, 2], F[2, 0], F[2, 1], F[2, 2]])


def scatter(matches):
    """mean (4,) and A^T A (4, 4) of X = (x2, y2, x1, y1), the second pass after the means"""
    X = np.asarray(matches, dtype=np.float64)[:, [2, 3, 0, 1]]
    mean = np.sum(X, axis=0) / len(X)
    A = X - mean
    return mean, A.T @ A


def restate(matches, solver="jacobi"):
    """F5 (NaN when flagged), singular values (descending), degenerate: the device route on given matches"""
    mean, S = scatter(matches)
    if solver == "jacobi":
        lam, V = CC.jacobi_eigh(S)
    else:
        lam, V = np.linalg.eigh(S)
    k0 = int(np.argmin(lam))
    N = V[:, k0] / np.linalg.norm(V[:, k0])
    if N[np.argmax(np.abs(N))] < 0.0:
        N = -N
    l2 = np.min(np.delete(lam, k0))
    degenerate = not (np.isfinite(lam.sum()) and l2 > RANK_TOL * lam.max())
    F = np.concatenate([N, [-np.dot(N, mean)]])
    return (np.full(5, np.nan) if degenerate else F), np.sqrt(np.maximum(np.sort(lam)[::-1], 0.0)), degenerate


def svd_f5(matches):
    """the reference's route (ref:bundle_adjust/s2p/estimation.py:114-154) on given matches, as five coefficients"""
    X = np.asarray(matches, dtype=np.float64)[:, [2, 3, 0, 1]]
    XX = np.sum(X, axis=0) / len(X)
    N = np.linalg.svd(X - XX)[2][-1, :]
    return np.concatenate([N, [-np.dot(N, XX)]])


def align(F, Fref):
    """F5 with the global sign of Fref"""
    a, b = f5(F), f5(Fref)
    return -a if np.dot(a[:4], b[:4]) < 0.0 else a


def residual(F, pts):
    """signed epipolar residual in pixels of the matches pts (m, 4) = x1, y1, x2, y2"""
    f = f5(F)
    return (f[2] * pts[:, 0] + f[3] * pts[:, 1] + f[0] * pts[:, 2] + f[1] * pts[:, 3] + f[4]) / np.hypot(f[0], f[1])


def distance(Fa, Fb, pts):
    """largest difference in pixels of what the gate sees of two matrices over pts, the signs aligned"""
    return float(np.abs(residual(align(Fa, Fb), pts) - residual(Fb, pts)).max())


def vector_distance(Fa, Fb):
    """largest difference of the four components of N, the signs aligned"""
    return float(np.abs(align(Fa, Fb)[:4] - f5(Fb)[:4]).max())


def load_golden():
    return np.load(GOLDEN)


def metric_points(g, case):
    """the stored matches of the case and the four corners with their partners"""
    return np.concatenate([g[key(case) + "_matches"], g[key(case) + "_corners"]])


def yardstick(g, case):
    """The distance in pixels of the restatement on the oracle's matches to the reference's F of the case: two correct float64
    routes to one null vector (normal matrix against SVD).  The larger of the restatement's two solvers, Jacobi and
    numpy.linalg.eigh: both are the device route in float64, and what one of them hits by luck of its roundings the other need not."""
    i, j, _, n = case
    m = restate_matches(CC.rpc(i), CC.rpc(j), roi(case), n)
    Fg, pts = g[key(case) + "_F"], metric_points(g, case)
    return max(distance(restate(m, solver)[0], Fg, pts) for solver in ("jacobi", "eigh"))


def match_tolerance(r):
    """bound in pixels on a projection through r of a point localised within LOC_TOL_DEG in each angle: LOC_TOL_DEG x the largest
    d(col, row)/d(lon, lat) scale ratio of r, x 2 for the two angles"""
    return 2.0 * LOC_TOL_DEG * max(r.col_scale / r.lon_scale, r.col_scale / r.lat_scale, r.row_scale / r.lon_scale, r.row_scale / r.lat_scale)


def batch(n_pairs):
    """n_pairs pairs cycling through the six healthy cases, every one with a region of its own.  Returns pairs (n, 2), roi (n, 4)"""
    pairs, regions = [], []
    for k in range(n_pairs):
        i, j, c, _ = HEALTHY[k % 6]
        x, y, w, h = CC.CROPS[c]
        pairs.append((i, j))
        regions.append((x + 3.0 * (k % 7), y + 2.0 * (k % 5), w - 3.0 * (k % 7) - 0.5 * (k % 11), h - 2.0 * (k % 5) - 0.25 * (k % 13)))
    return np.array(pairs, dtype=np.int32), np.array(regions, dtype=np.float64)

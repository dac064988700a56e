"""
The fundamental-matrix RANSAC of include/satba.h (satba_ransac_fundamental) restated in numpy float64, and the scenes its tests use.

The restatement follows the rule draw for draw with tools of its own: the null space of the 7 x 9 matrix is numpy.linalg.svd's, the
cubic det(x F1 + (1 - x) F2) is interpolated from four determinants and solved by numpy.roots; only the count of real roots is taken
the way the rule states it (the sign of the depressed cubic's discriminant), so that both sides drop the same complex pairs.  The
scoring part (`errors`) takes a dtype and also runs in numpy.longdouble: that run measures the rounding of the float64 scoring
(profiles/ft_ransac.json, `measure_rounding`).

Scenes (`scenes()`): two perspective cameras 500 km away with 1 m pixels, 12 and 14 degrees off nadir; points in a 1.8 km square with
heights 0 .. 100 m; Gaussian noise on both sides; a planted share of second-side points displaced uniformly by +-20 px.
"""
import functools

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
MIN_MATCHES, MAX_DRAWS, NEWTON_STEPS = 7, 64, 4
# Rounding of the scoring: the largest |err_float64 - err_longdouble| / max(err, max_err^2) over every (model, match) of the scenes
# below (10.1 million evaluations; measure_rounding(), recorded in profiles/ft_ransac.json), and the band the device gets: eight times
# that, the slack the SIFT tests give to the same arithmetic in another order.
SCORE_ROUNDING = 1.8e-10  # measured: 1.751e-10
BAND = 8 * SCORE_ROUNDING
# Models: the largest entry-wise difference between the float64 restatement's unit-norm matrices and the same samples solved in
# numpy.longdouble (`models_of_sample(..., dtype=numpy.longdouble)`: elimination with full pivoting, Newton on the float64 roots), over
# the first 48 trials of every scene (measure_rounding(), profiles/ft_ransac.json); the device gets eight times that.
MODEL_ROUNDING = 6.7e-12  # measured: 6.64e-12
MODEL_TOL = 8 * MODEL_ROUNDING


# ----------------------------------------------------------------------------- sampling

def splitmix64(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, p, n_trials, t, k, m):
    z = splitmix64(seed + GOLDEN * (1 + ((p * n_trials + t) * 64 + k)))
    return ((z >> 32) * m) >> 32


def sample(seed, p, n_trials, t, m):
    """the seven distinct indices of trial t in the order drawn, or None after 64 draws"""
    idx = []
    for k in range(MAX_DRAWS):
        v = draw(seed, p, n_trials, t, k, m)
        if v not in idx:
            idx.append(v)
            if len(idx) == 7:
                return idx
    return None


def repeats(rows):
    """two rows with a bit-identical (x1, y1) or a bit-identical (x2, y2)"""
    b = np.ascontiguousarray(rows, dtype=np.float64).view(np.uint64)
    for side in (0, 2):
        if len(set((int(r[side]), int(r[side + 1])) for r in b)) < len(b):
            return True
    return False


# ----------------------------------------------------------------------------- normalisation, models, errors

def normalise(xy):
    """(cx1, cy1, s1, cx2, cy2, s2), or None when a side's mean distance to its centroid is 0"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 4)
    if xy.shape[0] == 0:
        return None
    T = []
    for side in (0, 2):
        c = xy[:, side:side + 2].mean(axis=0)
        mean = np.sqrt(((xy[:, side:side + 2] - c) ** 2).sum(axis=1)).mean()
        if not mean > 0:
            return None
        T += [c[0], c[1], np.sqrt(2.0) / mean]
    return np.array(T)


def _T3(c0, c1, s, dtype):
    return np.array([[s, 0, -s * c0], [0, s, -s * c1], [0, 0, 1]], dtype=dtype)


def _null_space_ld(A):
    """two null vectors of the 7 x 9 matrix in its own dtype: Gauss-Jordan with full pivoting"""
    A = A.copy()
    perm = list(range(9))
    for c in range(7):
        sub = np.abs(A[c:, c:])
        r, k = np.unravel_index(np.argmax(sub), sub.shape)
        r, k = r + c, k + c
        A[[c, r]] = A[[r, c]]
        A[:, [c, k]] = A[:, [k, c]]
        perm[c], perm[k] = perm[k], perm[c]
        A[c] = A[c] / A[c, c]
        for q in range(7):
            if q != c:
                A[q] = A[q] - A[q, c] * A[c]
    out = []
    for j in (7, 8):
        v = np.zeros(9, dtype=A.dtype)
        v[perm[j]] = 1
        for q in range(7):
            v[perm[q]] = -A[q, j]
        out.append(v / np.sqrt((v * v).sum()))
    return out


def _det3(F):
    return (F[0, 0] * (F[1, 1] * F[2, 2] - F[1, 2] * F[2, 1]) - F[0, 1] * (F[1, 0] * F[2, 2] - F[1, 2] * F[2, 0])
            + F[0, 2] * (F[1, 0] * F[2, 1] - F[1, 1] * F[2, 0]))


def models_of_sample(rows, T, dtype=np.float64):
    """(n, 9), n = 0 .. 3: the unit-norm matrices of seven matches (pixel coordinates) under the pair's normalisation T"""
    rows = np.asarray(rows, dtype=np.float64).reshape(7, 4)
    if T is None or repeats(rows):
        return np.zeros((0, 9))
    r, T = rows.astype(dtype), np.asarray(T).astype(dtype)
    x1, y1, x2, y2 = (r[:, 0] - T[0]) * T[2], (r[:, 1] - T[1]) * T[2], (r[:, 2] - T[3]) * T[5], (r[:, 3] - T[4]) * T[5]
    A = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones(7, dtype=dtype)], axis=1)
    with np.errstate(all="ignore"):
        if dtype == np.float64:
            vt = np.linalg.svd(A)[2]
            F1, F2 = vt[7].reshape(3, 3), vt[8].reshape(3, 3)
        else:
            F1, F2 = (v.reshape(3, 3) for v in _null_space_ld(A))
        # det(x F1 + (1 - x) F2) = c3 x^3 + c2 x^2 + c1 x + c0 through x = -1, 0, 1, 2
        xs = np.array([-1, 0, 1, 2], dtype=dtype)
        d = np.array([_det3(x * F1 + (1 - x) * F2) for x in xs], dtype=dtype)
        c0 = d[1]
        c2 = (d[2] + d[0]) / 2 - c0
        c3 = (d[3] - 2 * d[2] - 2 * c2 + c0) / 6
        c1 = d[2] - c0 - c2 - c3
        c = np.array([c3, c2, c1, c0])
        big = np.abs(c).max()
        if not (big > 0 and np.isfinite(big)):
            return np.zeros((0, 9))
        tiny = 1e-12 * big
        if abs(c3) > tiny:
            a, b, e = c2 / c3, c1 / c3, c0 / c3
            p, q = b - a * a / 3, 2 * a * a * a / 27 - a * b / 3 + e
            n_real = 3 if q * q / 4 + p * p * p / 27 < 0 else 1
            poly = c
        elif abs(c2) > tiny:
            n_real = 2 if c1 * c1 - 4 * c2 * c0 >= 0 else 0
            poly = c[1:]
        elif abs(c1) > tiny:
            n_real, poly = 1, c[2:]
        else:
            return np.zeros((0, 9))
        roots = np.roots(poly.astype(np.float64))
        roots = roots[np.argsort(np.abs(roots.imag), kind="stable")][:n_real].real.astype(dtype)
        out = []
        for x in roots:
            for _ in range(NEWTON_STEPS):
                f, g = ((c3 * x + c2) * x + c1) * x + c0, (3 * c3 * x + 2 * c2) * x + c1
                if g != 0 and np.isfinite(f / g):
                    x = x - f / g
            F = _T3(T[3], T[4], T[5], dtype).T @ (x * F1 + (1 - x) * F2) @ _T3(T[0], T[1], T[2], dtype)
            nrm = np.sqrt((F * F).sum())
            if nrm > 0 and np.all(np.isfinite(F / nrm)):
                out.append((F / nrm).reshape(9))
    return np.array(out, dtype=dtype).reshape(-1, 9)


def errors(F, xy, dtype=np.float64):
    """ref:bundle_adjust/feature_tracks/ft_opencv.py:143-185 before the threshold: the larger of the two squared distances"""
    F_ = np.asarray(F).reshape(9).astype(dtype)
    xy = np.asarray(xy).reshape(-1, 4).astype(dtype)
    m1, m2 = xy[:, :2], xy[:, 2:]
    with np.errstate(all="ignore"):
        a = F_[0] * m1[:, 0] + F_[1] * m1[:, 1] + F_[2]
        b = F_[3] * m1[:, 0] + F_[4] * m1[:, 1] + F_[5]
        c = F_[6] * m1[:, 0] + F_[7] * m1[:, 1] + F_[8]
        s2 = 1.0 / (a * a + b * b)
        d2 = m2[:, 0] * a + m2[:, 1] * b + c
        a = F_[0] * m2[:, 0] + F_[3] * m2[:, 1] + F_[6]
        b = F_[1] * m2[:, 0] + F_[4] * m2[:, 1] + F_[7]
        c = F_[2] * m2[:, 0] + F_[5] * m2[:, 1] + F_[8]
        s1 = 1.0 / (a * a + b * b)
        d1 = m1[:, 0] * a + m1[:, 1] * b + c
        return np.maximum(d1 * d1 * s1, d2 * d2 * s2)  # NaN stays NaN: never an inlier


# ----------------------------------------------------------------------------- the rule

def ransac_pair(xy, p=0, max_err=0.3, n_trials=1000, seed=0, band=BAND):
    """
    One pair.  Returns a dict: mask (M bool), F (9; zeros without a model), best (trial, kept, models), and the table of every
    model: trial, F, count, sum, in_band (matches whose error lies within band * max_err^2 of max_err^2), winner (its row, or -1).
    """
    xy = np.ascontiguousarray(np.asarray(xy, dtype=np.float64).reshape(-1, 4))
    m, thr2 = xy.shape[0], max_err * max_err
    res = {"mask": np.ones(m, dtype=bool), "F": np.zeros(9), "best": (-1, m, 0), "trial": np.zeros(0, int), "models": np.zeros((0, 9)),
           "count": np.zeros(0, int), "sum": np.zeros(0), "in_band": np.zeros(0, int), "winner": -1, "samples": []}
    T = normalise(xy) if m >= MIN_MATCHES else None
    if T is None:
        return res
    trial, models, count, total, in_band, samples = [], [], [], [], [], []
    for t in range(n_trials):
        idx = sample(seed, p, n_trials, t, m)
        samples.append(idx)
        if idx is None:
            continue
        for F in models_of_sample(xy[idx], T):
            err = errors(F, xy)
            inl = err < thr2
            trial.append(t); models.append(F); count.append(int(inl.sum())); total.append(float(err[inl].sum()))
            in_band.append(int((np.abs(err - thr2) <= band * thr2).sum()))
    res.update(trial=np.array(trial, int), models=np.array(models).reshape(-1, 9), count=np.array(count, int), sum=np.array(total),
               in_band=np.array(in_band, int), samples=samples)
    if not trial:
        return res
    w = min(range(len(trial)), key=lambda k: (-count[k], trial[k], total[k], k))
    res.update(winner=w, F=models[w], mask=errors(models[w], xy) < thr2, best=(trial[w], count[w], len(trial)))
    return res


def ransac(pair_ofs, xy, max_err=0.3, n_trials=1000, seed=0, band=BAND):
    """all pairs of a call: mask (n), F (n_pairs, 9), best (n_pairs, 3), the per-pair dicts of ransac_pair"""
    pair_ofs = np.asarray(pair_ofs, dtype=np.int64)
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 4)
    pairs = [ransac_pair(xy[pair_ofs[p]:pair_ofs[p + 1]], p, max_err, n_trials, seed, band) for p in range(len(pair_ofs) - 1)]
    mask = np.concatenate([r["mask"] for r in pairs]) if pairs else np.zeros(0, bool)
    return mask, np.array([r["F"] for r in pairs]).reshape(-1, 9), np.array([r["best"] for r in pairs], dtype=np.int32).reshape(-1, 3), pairs


def match_models(got, want):
    """largest entry-wise difference between each matrix of `got` and the nearest of `want`, signs aligned; inf when the counts differ"""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1, 9), np.asarray(want, dtype=np.float64).reshape(-1, 9)
    if len(got) != len(want):
        return np.inf
    worst = 0.0
    for g in got:
        worst = max(worst, min(min(np.abs(g - w).max(), np.abs(g + w).max()) for w in want))
    return worst


# ----------------------------------------------------------------------------- scenes

def _camera(theta_deg, phi_deg):
    th, ph = np.radians(theta_deg), np.radians(phi_deg)
    d = np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])  # from the scene to the camera
    z = -d
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z]), 500e3 * d


def _project(X, cam, affine):
    R, C = cam
    if affine:
        return X @ R[:2].T + 900.0
    Xc = (X - C) @ R.T
    return 500e3 * Xc[:, :2] / Xc[:, 2:3] + 900.0  # 1 m pixels at 500 km


def make_scene(m, outlier_share, sigma, seed, affine=False):
    """(xy (m, 4), planted (m) bool: True where the match was not displaced)"""
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.uniform(-900, 900, (m, 2)), rng.uniform(0, 100, (m, 1))], axis=1)
    a = _project(X, _camera(12.0, 20.0), affine) + sigma * rng.standard_normal((m, 2))
    b = _project(X, _camera(14.0, 200.0), affine) + sigma * rng.standard_normal((m, 2))
    n_out = int(round(outlier_share * m))
    planted = np.ones(m, dtype=bool)
    out = rng.permutation(m)[:n_out]
    planted[out] = False
    b[out] += rng.uniform(-20, 20, (n_out, 2))
    return np.ascontiguousarray(np.concatenate([a, b], axis=1)), planted


# name -> (M, outlier share, sigma): the table of planted scenes
PLANTED = {"m7": (7, 0.0, 0.02), "m8": (8, 0.125, 0.02), "m64": (64, 0.30, 0.02), "m200": (200, 0.40, 0.03), "m1000": (1000, 0.50, 0.03),
           "m200_noisy": (200, 0.40, 0.1)}


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> dict(pair_ofs, xy, planted or None); every scene is one call"""
    out = {}
    for k, (name, (m, share, sigma)) in enumerate(PLANTED.items()):
        # at 8 matches every sample of seven has seven inliers (its own), so the rule's tie goes to trial 0 whatever the scene: seed
        # 307 displaces match 5, the one trial 0 of pair 0 (seed 0: draws 7, 3, 0, 2, 1, 6, 4) leaves out
        xy, planted = make_scene(m, share, sigma, seed=307 if name == "m8" else 100 + k)
        out[name] = dict(pair_ofs=np.array([0, m], dtype=np.int64), xy=xy, planted=planted)
    for m in (0, 1, 6):
        out["m%d" % m] = dict(pair_ofs=np.array([0, m], dtype=np.int64), xy=make_scene(m, 0.0, 0.02, seed=200 + m)[0], planted=None)
    xy = make_scene(20, 0.0, 0.02, seed=210)[0]
    xy[:, :2] = xy[0, :2]  # one side collapsed: no normalisation
    out["one_side_constant"] = dict(pair_ofs=np.array([0, 20], dtype=np.int64), xy=xy, planted=None)
    xy = np.repeat(make_scene(20, 0.0, 0.02, seed=211)[0], 2, axis=0)  # most samples hold a repeated row: no model
    out["rows_doubled"] = dict(pair_ofs=np.array([0, 40], dtype=np.int64), xy=np.ascontiguousarray(xy), planted=None)
    xy = make_scene(9, 0.0, 0.02, seed=212)[0]
    xy[7:] = xy[:2]
    out["m9_two_repeats"] = dict(pair_ofs=np.array([0, 9], dtype=np.int64), xy=xy, planted=None)
    parts = [make_scene(m, 0.3 if m > 8 else 0.0, 0.02, seed=220 + k)[0] for k, m in enumerate((7, 300, 0, 64, 2049))]
    out["five_pairs"] = dict(pair_ofs=np.cumsum([0] + [len(q) for q in parts]).astype(np.int64), xy=np.ascontiguousarray(np.concatenate(parts)), planted=None)
    xy, planted = make_scene(64, 0.30, 0.02, seed=230, affine=True)
    out["affine"] = dict(pair_ofs=np.array([0, 64], dtype=np.int64), xy=xy, planted=planted)
    return out


# (scene, n_trials, seed) of every run the tests make
RUNS = [(name, 1000, 0) for name in ("m7", "m8", "m64", "m200", "m1000", "m200_noisy", "m0", "m1", "m6", "one_side_constant", "rows_doubled",
                                      "m9_two_repeats", "five_pairs", "affine")]
RUNS += [("m64", 1, 0), ("m64", 3, 0), ("m64", 1000, 12345), ("m200", 1000, 12345)]


@functools.lru_cache(maxsize=None)
def reference(name, n_trials=1000, seed=0, max_err=0.3):
    """the restatement's result of a run, computed once and shared: (mask, F, best, per-pair dicts)"""
    s = scenes()[name]
    return ransac(s["pair_ofs"], s["xy"], max_err, n_trials, seed)


def measure_rounding(n_model_trials=48, max_err=0.3):
    """(scoring, models, evaluations): the figures behind SCORE_ROUNDING and MODEL_ROUNDING, over every run of RUNS"""
    thr2, score, model, n_eval = max_err * max_err, 0.0, 0.0, 0
    for name, n_trials, seed in RUNS:
        s = scenes()[name]
        for p, r in enumerate(reference(name, n_trials, seed)[3]):
            xy = s["xy"][s["pair_ofs"][p]:s["pair_ofs"][p + 1]]
            for F in r["models"]:
                e64, eld = errors(F, xy), errors(F, xy, np.longdouble)
                ok = np.isfinite(eld)
                score = max(score, float((np.abs(e64[ok] - eld[ok]) / np.maximum(eld[ok], thr2)).max()))
                n_eval += len(e64)
            T = normalise(xy) if len(xy) >= MIN_MATCHES else None
            for idx in r["samples"][:n_model_trials]:
                if idx is not None:
                    a, b = models_of_sample(xy[idx], T), models_of_sample(xy[idx], T, np.longdouble)
                    if len(a) == len(b):  # a discriminant at rounding distance of 0 would differ in count: none does
                        model = max(model, match_models(a, b.astype(np.float64)))
                    else:
                        model = np.inf
    return score, model, n_eval

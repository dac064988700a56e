"""
Cases of the pairwise matching (satba.ft_match) shared by tools/gen_golden_match.py, which runs the reference's compiled `matching`
and its UTM filter on them and writes tests/golden/ft_match.npz, and by the tests, which only read that file.

A case is a handful of images -- keypoint rows of 132 float32 (col, row, scale, orientation, 128 descriptor values) with UTM
coordinates -- and pairs with a box and an affine fundamental matrix each.  Images of a case see the same scene points: descriptors
are a point's descriptor plus noise of a wide range of amplitudes (so the ratios spread around the threshold), coordinates are
displaced along and across the epipolar lines (so the gate cuts some true pairs and nearly all false ones).  Every case is run in
four variants: gate on / off x relative (thr 0.6) / absolute (thr 250).

`rule` restates in numpy what the device computes (include/satba.h, satba_match_pairs): the host test ties it to the reference's
output, the GPU tests compare the device with it.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ft_match.npz")
INT_CASES = ["small", "ties", "extremes", "tiny", "padded", "boxes", "same_coords", "scene"]
CASES = INT_CASES + ["float"]
VARIANTS = [("gate_rel", True, True, 0.6), ("gate_abs", True, False, 250.0), ("free_rel", False, True, 0.6), ("free_abs", False, False, 250.0)]
EPI_THR = 20.0
BOX = (1000.0, 2000.0, 5000.0, 6500.0)
FLOAT_SCALE = 512.0
MARGIN = 1e-4


def load():
    return np.load(GOLDEN)


def variant_thr(case, thr, relative):
    """the absolute threshold follows the descriptors' scale"""
    return thr if relative else thr / case.get("scale", 1.0)


def fundamental(seed):
    """an affine fundamental matrix: epipolar lines close to the image rows"""
    rng = np.random.default_rng([seed, 7])
    a, b, c, d, e = 0.02 * rng.standard_normal(), 1.0, 0.03 * rng.standard_normal(), -1.0 - 0.02 * rng.random(), 8.0 * rng.standard_normal()
    F = np.zeros((3, 3))
    F[0, 2], F[1, 2], F[2, 0], F[2, 1], F[2, 2] = c, d, a, b, e
    return F


def _points(rng, n):
    """scene points: integer descriptors, quarter-pixel coordinates, UTM inside BOX"""
    desc = rng.integers(0, 256, (n, 128)) * (rng.random((n, 128)) < 0.7)
    xy = rng.integers(0, 8000, (n, 2)) / 4.0
    utm = np.stack([rng.uniform(BOX[0] + 50, BOX[1] - 50, n), rng.uniform(BOX[2] + 50, BOX[3] - 50, n)], axis=1)
    return desc, xy, utm


def _view(rng, pts, idx, F=None, first=True, n_out=0, pad=0):
    """An image that sees the scene points idx (in that order), n_out keypoints outside BOX mixed in, `pad` NaN rows behind."""
    desc, xy, utm = pts
    n = len(idx)
    amp = rng.choice([0, 2, 10, 40, 90, 140], n)[:, None]
    d = np.clip(desc[idx] + np.rint(amp * rng.standard_normal((n, 128))).astype(np.int64), 0, 255)
    c = xy[idx].copy()
    if not first and F is not None:  # put the point near its epipolar line: c col2 + d row2 + a col1 + b row1 + e = 0
        col2 = c[:, 0] + rng.integers(-200, 200, n) / 4.0
        row2 = -(F[0, 2] * col2 + F[2, 0] * c[:, 0] + F[2, 1] * c[:, 1] + F[2, 2]) / F[1, 2]
        c = np.stack([col2, np.rint(4.0 * row2) / 4.0 + rng.integers(-120, 120, n) / 4.0], axis=1)
    u = utm[idx] + (0.0 if first else np.array([3.0, -2.0])) + 0.5 * rng.standard_normal((n, 2))
    wild = rng.random(n) < 0.04  # a few keypoints far from where their point is: the UTM filter's outliers
    u[wild] += rng.uniform(-30, 30, (int(wild.sum()), 2))
    f = np.zeros((n + n_out, 132), dtype=np.float32)
    um = np.zeros((n + n_out, 2))
    slot = np.sort(rng.permutation(n + n_out)[:n])
    outside = np.setdiff1d(np.arange(n + n_out), slot)
    f[slot, :2], f[slot, 2], f[slot, 3], f[slot, 4:] = c, 1.0 + rng.integers(0, 16, n) / 4.0, rng.integers(0, 360, n), d
    um[slot] = u
    f[outside, :2] = rng.integers(0, 8000, (n_out, 2)) / 4.0
    f[outside, 4:] = rng.integers(0, 256, (n_out, 128))
    um[outside] = np.stack([rng.uniform(BOX[1], BOX[1] + 500, n_out), rng.uniform(BOX[2], BOX[3], n_out)], axis=1)
    um[outside[::2], 0] = BOX[0]  # on the box's edge: strictly inside fails
    if pad:
        f = np.concatenate([f, np.full((pad, 132), np.nan, dtype=np.float32)])
        um = np.concatenate([um, np.full((pad, 2), np.nan)])
    return f, um


def _case(feats, utm, pairs, boxes, seeds, **kw):
    return dict(feats=list(feats), utm=list(utm), pairs=np.asarray(pairs, dtype=np.int32).reshape(-1, 2),
                boxes=np.asarray(boxes, dtype=np.float64).reshape(-1, 4), F=[fundamental(s) for s in seeds], **kw)


def _two(seed, n_i, n_j, n_common, n_out=(0, 0), pad=(0, 0)):
    """two images of n_i / n_j keypoints inside BOX, n_common scene points seen by both"""
    rng = np.random.default_rng([seed, 11])
    F = fundamental(seed)
    pts = _points(rng, n_i + n_j - n_common)
    idx_i = rng.permutation(n_i)
    idx_j = rng.permutation(np.concatenate([np.arange(n_common), np.arange(n_i, n_i + n_j - n_common)]))
    a = _view(rng, pts, idx_i, F, True, n_out[0], pad[0])
    b = _view(rng, pts, idx_j, F, False, n_out[1], pad[1])
    return a, b


def make(name):
    if name == "small":  # 257 x 300 selected of 290 x 341: 16-row and 16-column tiles with remainders
        a, b = _two(1, 257, 300, 180, n_out=(33, 41))
        return _case([a[0], b[0]], [a[1], b[1]], [(0, 1)], [BOX], [1])
    if name == "ties":
        a, b = _two(2, 40, 300, 30)
        fa, fb = a[0], b[0]
        fb[290, 4:] = fb[10, 4:]          # one descriptor at j = 10 and j = 290 ...
        fa[0, 4:] = fb[10, 4:]            # ... and a query at distance 0 of both: 0 / 0
        fa[0, :2], fb[290, :2] = (100.0, 200.0), fb[10, :2]
        fa[1, 4:] = np.clip(fb[10, 4:] + 3.0 * (np.arange(128) % 2), 0, 255)  # equally near to both: distB == distA > 0
        fa[1, :2] = fa[0, :2]
        fa[2, 4:] = fb[20, 4:]            # an exact copy once: distA = 0 < distB
        F = fundamental(2)                # the copies' partners lie on the epipolar lines of the queries
        for j in (10, 290, 20):
            src = fa[0] if j != 20 else fa[2]
            fb[j, 0] = src[0] + 5.0
            fb[j, 1] = np.rint(-4.0 * (F[0, 2] * fb[j, 0] + F[2, 0] * src[0] + F[2, 1] * src[1] + F[2, 2]) / F[1, 2]) / 4.0
        return _case([fa, fb], [a[1], b[1]], [(0, 1)], [BOX], [2])
    if name == "extremes":  # the signed shift and the int32 range
        a, b = _two(3, 24, 37, 20)
        fa, fb = a[0], b[0]
        fa[0, 4:], fa[1, 4:], fa[2, 4:] = 0.0, 255.0, np.where(np.arange(128) % 2, 255.0, 0.0)
        fb[0, 4:], fb[1, 4:], fb[2, 4:], fb[3, 4:] = 255.0, 0.0, np.where(np.arange(128) % 2, 0.0, 255.0), np.where(np.arange(128) % 3, 0.0, 255.0)
        fa[:3, :2] = fb[:3, :2] = (50.0, 60.0)
        return _case([fa, fb], [a[1], b[1]], [(0, 1)], [BOX], [3])
    if name == "tiny":  # 1 x 1, 1 x 17, 17 x 1, a single finite candidate, a query whose candidates are all gated out
        rng = np.random.default_rng([4, 11])
        pts = _points(rng, 40)
        F = fundamental(4)
        one = _view(rng, pts, np.array([0]), F, True)
        one_b = _view(rng, pts, np.array([0]), F, False)
        many = _view(rng, pts, np.arange(17), F, True)
        many_b = _view(rng, pts, np.arange(17), F, False)
        far = _view(rng, pts, np.arange(20, 26), F, True)
        far[0][:, 1] += 5000.0   # rows far from every epipolar line of image 3: all gated out
        near = _view(rng, pts, np.arange(20, 26), F, False)
        near[0][1:, 1] += 9000.0  # ... and for the queries of image 2 only candidate 0 can pass the gate
        feats, utm = zip(one, one_b, many, many_b, far, near)
        return _case(feats, utm, [(0, 1), (0, 3), (2, 1), (4, 3), (2, 5)], [BOX] * 5, [4] * 5)
    if name == "padded":
        a, b = _two(5, 50, 70, 40, n_out=(5, 9), pad=(13, 30))
        return _case([a[0], b[0]], [a[1], b[1]], [(0, 1)], [BOX], [5])
    if name == "boxes":  # an empty side, a box that cuts both images, infinite bounds
        a, b = _two(6, 90, 110, 70, n_out=(10, 10))
        empty = (BOX[1] + 600.0, BOX[1] + 700.0, BOX[2], BOX[3])
        left = (BOX[0] + 50.0, BOX[0] + 50.0 + 300.0, BOX[2], BOX[3])
        cut = (BOX[0] + 300.0, BOX[0] + 700.0, BOX[2] + 200.0, BOX[3] - 300.0)
        inf = (-np.inf, np.inf, -np.inf, BOX[3] - 500.0)
        c = _view(np.random.default_rng(66), _points(np.random.default_rng(67), 8), np.arange(8), None, True)
        c[1][:, 0] += 5000.0  # image 2 lies outside `left`: that pair has one empty side
        return _case([a[0], b[0], c[0]], [a[1], b[1], c[1]], [(0, 1), (0, 2), (0, 1), (1, 0)], [empty, left, cut, inf], [6, 6, 6, 7])
    if name == "same_coords":  # several orientations at one location share (col, row) and the UTM coordinates
        a, b = _two(8, 80, 90, 60)
        for f, u in (a, b):
            for k in range(5, f.shape[0], 7):
                f[k, :2], u[k] = f[k - 3, :2], u[k - 3]
                f[k, 3] += 90.0
        return _case([a[0], b[0]], [a[1], b[1]], [(0, 1)], [BOX], [8])
    if name == "scene":  # 4 images, 5 pairs of unequal sizes in one call, F per pair
        rng = np.random.default_rng([9, 11])
        pts = _points(rng, 400)
        sizes, views = (130, 201, 77, 310), []
        for m, n in enumerate(sizes):
            views.append(_view(rng, pts, rng.permutation(400)[:n], fundamental(9), m == 0, n_out=7 * m, pad=3 * m))
        feats, utm = zip(*views)
        cut = (BOX[0] + 100.0, BOX[1] - 200.0, BOX[2] + 100.0, BOX[3] - 100.0)
        return _case(feats, utm, [(0, 1), (0, 2), (1, 3), (2, 3), (0, 3)], [BOX, cut, BOX, cut, BOX], [9, 9, 10, 11, 9])
    if name == "float":  # descriptors that are no integers: the float path
        a, b = _two(12, 70, 95, 55, n_out=(4, 6))
        for f in (a[0], b[0]):
            f[:, 4:] /= np.float32(FLOAT_SCALE)
        return _case([a[0], b[0]], [a[1], b[1]], [(0, 1)], [BOX], [12], scale=FLOAT_SCALE)
    raise KeyError(name)


def from_golden(g, name):
    """the case as tools/gen_golden_match.py stored it (descriptors as uint8 with their scale, padding rows by their NaN head)"""
    ofs = np.concatenate([[0], np.cumsum(g[name + "_sizes"])])
    scale = float(g[name + "_scale"])
    f = np.concatenate([g[name + "_head"], g[name + "_desc"].astype(np.float32) / np.float32(scale)], axis=1).astype(np.float32)
    f[np.isnan(f[:, 0])] = np.nan
    case = dict(feats=[f[a:b].copy() for a, b in zip(ofs[:-1], ofs[1:])], utm=[g[name + "_utm"][a:b].copy() for a, b in zip(ofs[:-1], ofs[1:])],
                pairs=g[name + "_pairs"], boxes=g[name + "_boxes"], F=list(g[name + "_F"]))
    if scale != 1.0:
        case["scale"] = scale
    return case


# ----------------------------------------------------------------------------- the rule

def similarities(F):
    """(s1, s2) float32[3]: include/satba.h, satba_match_pairs; the formulas of the affine rectification (H&Z p. 345) in double"""
    c, d, a, b, e = F[0, 2], F[1, 2], F[2, 0], F[2, 1], F[2, 2]
    r, s = np.sqrt(a * a + b * b), np.sqrt(c * c + d * d)
    z, t = np.sqrt(r / s), 0.5 * e / np.sqrt(r * s)
    zz = 1 / z
    return np.array([z * b / r, z * a / r, t], dtype=np.float32), np.array([zz * -d / s, zz * -c / s, -t], dtype=np.float32)


def inside(utm, box):
    e, n = utm[:, 0], utm[:, 1]
    return np.where((e > box[0]) & (e < box[1]) & (n > box[2]) & (n < box[3]))[0]


def distances(fi, fj, F, epi_thr=EPI_THR, exact=np.int64):
    """d (n_i, n_j) float64: the exact squared distances, +inf where the gate fails (gate in float32, in the reference's order)"""
    a, b = fi[:, 4:].astype(np.float64), fj[:, 4:].astype(np.float64)
    if exact is np.int64:
        ai, bi = a.astype(np.int64), b.astype(np.int64)
        d = ((ai * ai).sum(1)[:, None] + (bi * bi).sum(1)[None, :] - 2 * (ai @ bi.T)).astype(np.float64)
    else:
        d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(2)  # float64: the float case is small
    if F is not None:
        s1, s2 = similarities(F)
        xx1 = (s1[1] * fi[:, 0] + s1[0] * fi[:, 1]) + s1[2]
        xx2 = (s2[1] * fj[:, 0] + s2[0] * fj[:, 1]) + s2[2]
        assert xx1.dtype == np.float32 and xx2.dtype == np.float32
        d = np.where(np.abs(xx1[:, None] - xx2[None, :]) < np.float32(epi_thr), d, np.inf)
    return d


def nearest_two(d):
    """distA, indexA (lowest j among equals), distB (with multiplicity)"""
    n_i, n_j = d.shape
    jA = np.argmin(d, axis=1)
    dA = d[np.arange(n_i), jA]
    dB = np.partition(d, 1, axis=1)[:, 1] if n_j > 1 else np.full(n_i, np.inf)
    return dA, jA, dB


def rule_match(fi, fj, F, thr, relative, epi_thr=EPI_THR, exact=np.int64):
    """(i, j) int64 (M, 2) of the matches between two sets of selected keypoints, i ascending"""
    if fi.shape[0] == 0 or fj.shape[0] == 0:
        return np.zeros((0, 2), dtype=np.int64)
    dA, jA, dB = nearest_two(distances(fi, fj, F, epi_thr, exact))
    with np.errstate(invalid="ignore", divide="ignore"):
        val = dA.astype(np.float32) / dB.astype(np.float32) if relative else dA.astype(np.float32)
        ok = val < np.float32(thr) * np.float32(thr)
    i = np.where(ok)[0]
    return np.stack([i, jA[i]], axis=1).astype(np.int64)


def rule(case, gate, relative, thr, only=None):
    """pair_ofs, kp_i, kp_j of the whole case (or of the pairs `only`), as satba_matches_fetch returns them"""
    ofs, ki, kj = [0], [], []
    exact = np.float64 if "scale" in case else np.int64
    for p in (range(len(case["pairs"])) if only is None else only):
        i, j = case["pairs"][p]
        si, sj = inside(case["utm"][i], case["boxes"][p]), inside(case["utm"][j], case["boxes"][p])
        m = rule_match(case["feats"][i][si], case["feats"][j][sj], case["F"][p] if gate else None, variant_thr(case, thr, relative), relative, exact=exact)
        ki.append(si[m[:, 0]]); kj.append(sj[m[:, 1]])
        ofs.append(ofs[-1] + len(m))
    return np.asarray(ofs, dtype=np.int64), np.concatenate(ki).astype(np.int32), np.concatenate(kj).astype(np.int32)


def margins(case, gate, relative, thr):
    """queries of the float case, recomputed in float64, whose value lies within MARGIN (relative) of thr^2, or whose two nearest
    are closer than MARGIN (relative) without being equal copies: both counts must be zero for the float path to be comparable"""
    near_thr = near_tie = 0
    t2 = float(variant_thr(case, thr, relative)) ** 2
    for p, (i, j) in enumerate(case["pairs"]):
        si, sj = inside(case["utm"][i], case["boxes"][p]), inside(case["utm"][j], case["boxes"][p])
        if not len(si) or not len(sj):
            continue
        dA, jA, dB = nearest_two(distances(case["feats"][i][si], case["feats"][j][sj], case["F"][p] if gate else None, exact=np.float64))
        fin = np.isfinite(dA)
        with np.errstate(invalid="ignore", divide="ignore"):
            val = np.where(np.isfinite(dB), dA / dB, 0.0) if relative else dA
            near_thr += int(np.sum(fin & (np.abs(val - t2) < MARGIN * t2)))
            near_tie += int(np.sum(fin & np.isfinite(dB) & (dB - dA < MARGIN * dB)))
    return near_thr, near_tie


def first_index_by_coords(feats_sel, m):
    """the reference's renaming (`list.index` of the matched coordinates, ref:ft_s2p.py:164-168) on a selected set"""
    allp = feats_sel[:, :2].tolist()
    return np.array([allp.index(allp[k]) for k in m], dtype=np.int64)

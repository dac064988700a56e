"""
Cases of the windowed matching (satba.ft_match.match_pairs_window, include/satba.h: satba_match_window) and the rule in numpy.

A case is what a case of tests/cases_match.py is -- images of 132-float32 keypoint rows with UTM coordinates, pairs with a box
each -- plus, where the case fixes them, the window "radius" (rx, ry) and the thresholds "thrs" it is run with.  The cases of
cases_match hold a handful of candidates per window; these are dense where it matters.  Coordinates lie on a quarter-metre lattice
(every difference is exact) except where a case places a value by `nextafter`.

`rule_window` is brute force: all distances, a boolean window mask in float64, argmin (the lowest j among equals).  At an infinite
radius it is cases_match.rule without gate under the absolute threshold, which tests/golden/ft_match.npz pins on the reference's
compiled `matching` (tests/test_window_host.py).
"""
import functools

import numpy as np

import cases_match as CM

INF = np.inf
EVERYWHERE = (-INF, INF, -INF, INF)
RADII = [(30.0, 30.0), (6.0, 2.0), (0.25, 0.25), (INF, INF)]
CASES = ["edge", "cells", "sparse", "dense", "ties", "extremes", "boxed", "float"]
THR = 250.0


def radii_of(case):
    return [case["radius"]] if "radius" in case else RADII


def thrs_of(case):
    return case.get("thrs", [THR])


# ----------------------------------------------------------------------------- the rule

def window_mask(ui, uj, rx, ry):
    """(n_i, n_j) bool: fabs(east_i - east_j) < rx and fabs(north_i - north_j) < ry in float64, each difference rounded once"""
    with np.errstate(over="ignore"):
        return (np.abs(ui[:, None, 0] - uj[None, :, 0]) < rx) & (np.abs(ui[:, None, 1] - uj[None, :, 1]) < ry)


def rule_pair(case, p, rx, ry, thr):
    """(si, sj, mask, d): selected rows of both sides, the window mask and the distances between them"""
    i, j = case["pairs"][p]
    si, sj = CM.inside(case["utm"][i], case["boxes"][p]), CM.inside(case["utm"][j], case["boxes"][p])
    exact = np.float64 if "scale" in case else np.int64
    mask = window_mask(case["utm"][i][si], case["utm"][j][sj], rx, ry)
    d = CM.distances(case["feats"][i][si], case["feats"][j][sj], None, exact=exact) if len(si) and len(sj) else np.zeros((len(si), len(sj)))
    return si, sj, mask, d


def rule_window(case, rx, ry, thr, only=None):
    """pair_ofs, kp_i, kp_j as satba_matches_fetch returns them, and n_candidates; thr follows the descriptors' scale as in
    cases_match.rule"""
    ofs, ki, kj, n_cand = [0], [], [], 0
    t2 = np.float32(CM.variant_thr(case, thr, False)) * np.float32(CM.variant_thr(case, thr, False))
    for p in (range(len(case["pairs"])) if only is None else only):
        si, sj, mask, d = rule_pair(case, p, rx, ry, thr)
        n_cand += int(mask.sum())
        m = np.zeros((0, 2), dtype=np.int64)
        if len(si) and len(sj):
            d = np.where(mask, d, np.inf)
            jA = np.argmin(d, axis=1)
            dA = d[np.arange(len(si)), jA]
            ok = mask.any(axis=1) & (dA.astype(np.float32) < t2)
            q = np.where(ok)[0]
            m = np.stack([q, jA[q]], axis=1)
        ki.append(si[m[:, 0]]); kj.append(sj[m[:, 1]])
        ofs.append(ofs[-1] + len(m))
    return np.asarray(ofs, dtype=np.int64), np.concatenate(ki).astype(np.int32), np.concatenate(kj).astype(np.int32), n_cand


def window_counts(case, p, rx, ry):
    """candidates per selected query of pair p"""
    return rule_pair(case, p, rx, ry, THR)[2].sum(axis=1)


# ----------------------------------------------------------------------------- building blocks

def _lattice(rng, n, lo, hi):
    """n points on the quarter-metre lattice in [lo, hi] x [lo, hi] (or per axis: lo, hi pairs)"""
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=np.float64), (2,)), np.broadcast_to(np.asarray(hi, dtype=np.float64), (2,))
    return np.stack([rng.integers(int(4 * lo[k]), int(4 * hi[k]) + 1, n) / 4.0 for k in range(2)], axis=1)


def _image(rng, utm, desc, pad=0):
    n = len(utm)
    f = np.zeros((n, 132), dtype=np.float32)
    f[:, :2] = rng.integers(0, 8000, (n, 2)) / 4.0
    f[:, 2], f[:, 3] = 1.0 + rng.integers(0, 16, n) / 4.0, rng.integers(0, 360, n)
    f[:, 4:] = desc
    u = np.asarray(utm, dtype=np.float64).reshape(n, 2).copy()
    if pad:
        f = np.concatenate([f, np.full((pad, 132), np.nan, dtype=np.float32)])
        u = np.concatenate([u, np.full((pad, 2), np.nan)])
    return f, u


def _desc(rng, n):
    return rng.integers(0, 256, (n, 128)) * (rng.random((n, 128)) < 0.7)


def _noisy(rng, desc, amps=(0, 1, 2, 3, 6)):
    """descriptors near `desc`: d up to 128 * 36, far below 250^2, and far from every other random descriptor"""
    amp = rng.choice(amps, len(desc))[:, None]
    return np.clip(desc + rng.integers(-1, 2, desc.shape) * amp, 0, 255)


def _views(rng, n, lo, hi, jitter=2.0, extra=0):
    """two images of the same n scene points: the second displaced by up to `jitter` metres on the lattice, in another order, with
    `extra` keypoints of its own"""
    pts, desc = _lattice(rng, n, lo, hi), _desc(rng, n)
    a = _image(rng, pts, _noisy(rng, desc))
    order = rng.permutation(n)
    moved = pts[order] + rng.integers(int(-4 * jitter), int(4 * jitter) + 1, (n, 2)) / 4.0
    ub = np.concatenate([moved, _lattice(rng, extra, lo, hi)])
    db = np.concatenate([_noisy(rng, desc[order]), _desc(rng, extra)])
    mix = rng.permutation(n + extra)
    b = _image(rng, ub[mix], db[mix])
    return a, b


def _case(images, pairs, boxes=None, **kw):
    feats, utm = zip(*images)
    boxes = [EVERYWHERE] * len(pairs) if boxes is None else boxes
    return dict(feats=list(feats), utm=list(utm), pairs=np.asarray(pairs, dtype=np.int32).reshape(-1, 2),
                boxes=np.asarray(boxes, dtype=np.float64).reshape(-1, 4), **kw)


# ----------------------------------------------------------------------------- the cases

@functools.lru_cache(maxsize=None)
def make(name):
    rng = np.random.default_rng([sum(map(ord, name)), 23])
    if name == "edge":
        # around each query: keypoints at |dx| == rx (out; they carry the query's descriptor, so taking one in shows), at
        # nextafter(rx, 0) (in; noisy copies), the same for dy, and the corners; rx != ry.  Query 0 sits at the origin, where
        # nextafter(r, 0) is a coordinate; query 1 on the lattice, where fl(e - e_j) rounds: 7.75 / 4.75 are the last lattice steps in
        rx, ry = 8.0, 5.0
        bx, by = np.nextafter(rx, 0.0), np.nextafter(ry, 0.0)
        D = _desc(rng, 2)
        uq = np.array([[0.0, 0.0], [4096.25, 8192.5]])
        out0 = [(rx, 0), (-rx, 0), (0, ry), (0, -ry), (rx, by), (-bx, -ry), (rx, ry)]
        in0 = [(bx, 0), (-bx, 0), (0, by), (0, -by), (bx, by), (-bx, -by), (bx, -by)]
        out1 = [(8.0, 0), (-8.0, 0), (0, 5.0), (0, -5.0), (8.0, 4.75), (-7.75, 5.0), (np.nextafter(4096.25 + 8.0, 0.0) - 4096.25, 0)]
        in1 = [(7.75, 0), (-7.75, 0), (0, 4.75), (0, -4.75), (7.75, 4.75), (-7.75, -4.75)]
        uj, dj = [], []
        for q, (outs, ins) in enumerate(((out0, in0), (out1, in1))):
            for o in outs:
                uj.append(uq[q] + np.array(o)); dj.append(D[q])
            for o in ins:
                uj.append(uq[q] + np.array(o)); dj.append(_noisy(rng, D[q][None], amps=(2, 3))[0])
        mix = rng.permutation(len(uj))
        a = _image(rng, uq, D)
        b = _image(rng, np.array(uj)[mix], np.array(dj)[mix])
        return _case([a, b], [(0, 1), (1, 0)], radius=(rx, ry))
    if name == "cells":
        # r = 4 over keypoints in [0, 40]^2: queries on cell corners, on the grid's outer edge and corners, outside the grid and far
        # from it; candidates in all nine neighbouring cells; a second image whose grid is one cell, and one of a single keypoint
        r = 4.0
        a, b = _views(rng, 700, 0.0, 40.0, jitter=1.0, extra=100)
        corners = np.array([(4.0 * k, 4.0 * l) for k in (0, 1, 5, 9, 10) for l in (0, 2, 5, 10)] + [(-2.0, -2.0), (-4.0, 20.0), (44.0, 20.0), (43.75, 43.75),
                                                                                                   (1000.0, 1000.0), (20.0, -1e7)])
        near = np.array([np.argmin(np.abs(b[1] - c).sum(axis=1)) for c in corners])
        qa = _image(rng, corners, _noisy(rng, b[0][near, 4:].astype(np.int64)))
        fa, ua = np.concatenate([qa[0], a[0]]), np.concatenate([qa[1], a[1]])
        one = _image(rng, _lattice(rng, 30, (10.0, 10.0), (13.0, 13.0)), _noisy(rng, a[0][:30, 4:].astype(np.int64)))
        single = _image(rng, np.array([[20.0, 20.0]]), a[0][200:201, 4:])
        return _case([(fa, ua), b, one, single], [(0, 1), (1, 0), (0, 2), (0, 3), (3, 1)], radius=(r, r))
    if name == "sparse":
        # two clusters 10^6 m apart with r = 0.25: on the lattice only a keypoint at the very same place is a candidate
        r = 0.25
        c0, c1 = np.array([500000.0, 4000000.0]), np.array([1500000.0, 5000000.0])
        pts = np.concatenate([c0 + _lattice(rng, 60, 0.0, 6.0), c1 + _lattice(rng, 60, 0.0, 6.0)])
        desc = _desc(rng, len(pts))
        a = _image(rng, pts, _noisy(rng, desc))
        shift = rng.choice([0.0, 0.25, -0.25], (len(pts), 2), p=[0.6, 0.2, 0.2])
        order = rng.permutation(len(pts))
        b = _image(rng, (pts + shift)[order], _noisy(rng, desc)[order])
        return _case([a, b], [(0, 1), (1, 0)], radius=(r, r))
    if name == "dense":
        # r = 30: windows of exactly 63, 64 and 65 candidates, one of about 5 000, and near-duplicate descriptors whose distance is
        # 250^2 - 1, 250^2 and 250^2 + 1, so that thr = 250 decides
        r = 30.0
        centres = np.array([[1000.0, 1000.0], [2000.0, 1000.0], [3000.0, 1000.0], [1000.0, 3000.0], [3000.0, 3000.0], [5000.0, 5000.0], [5000.0, 1000.0]])
        sizes = [63, 64, 65, 5000, 300, 65, 64]
        D = _desc(rng, len(centres))
        D[:, :8] = 0
        uj, dj = [], []
        for c, n, d in zip(centres, sizes, D):
            uj.append(c + _lattice(rng, n, -29.75, 29.75))
            dj.append(_desc(rng, n))
        # the windows' own nearest: 62 499 (a match), 62 500 (none: strict), 62 501 (none), and both 62 499 and an exact copy
        below, at, above = np.array([249, 22, 3, 2, 1, 0, 0, 0]), np.array([250, 0, 0, 0, 0, 0, 0, 0]), np.array([250, 1, 0, 0, 0, 0, 0, 0])
        for k, delta in ((0, below), (1, at), (2, above), (3, below), (5, at), (6, above)):
            dj[k][sizes[k] // 2] = np.concatenate([delta, D[k][8:]])
        dj[3][4321] = D[3]
        dj[5][7], dj[5][40] = np.concatenate([below[::-1], D[5][8:]]), np.concatenate([below, D[5][8:]])  # equal d at two j
        b = _image(rng, np.concatenate(uj), np.concatenate(dj))
        # queries: the centres (their window holds the whole cluster), and keypoints of the clusters themselves seen again
        again = rng.permutation(len(b[1]))[:120]
        ua = np.concatenate([centres, b[1][again] + rng.integers(-8, 9, (120, 2)) / 4.0])
        da = np.concatenate([D, _noisy(rng, b[0][again, 4:].astype(np.int64))])
        a = _image(rng, ua, da)
        return _case([a, b], [(0, 1)], radius=(r, r))
    if name == "ties":
        # per query: its descriptor at several j inside the window (the lowest j wins), once more at a lower j outside (must not
        # win), and, for the second half of the queries, nothing but a far descriptor inside: the match goes to nobody although a
        # copy lies outside
        r = 10.0
        n_q = 12
        uq = np.array([[100.0 * (k + 1), 50.0 * (k % 3)] for k in range(n_q)])
        D = _desc(rng, n_q)
        uj, dj = [], []
        for k in range(n_q):  # the outside copies first: lower j
            uj.append(uq[k] + np.array([r, 0.0]) * (1 if k % 2 else -1) + np.array([0.0, 0.25 * k])); dj.append(D[k])
        for k in range(n_q):
            if k < n_q // 2:
                for o in ((3.0, 1.0), (-9.75, 9.75), (0.0, 0.0), (9.75, -2.5)):
                    uj.append(uq[k] + np.array(o)); dj.append(D[k])
            else:
                uj.append(uq[k] + np.array([1.0, 1.0])); dj.append(_desc(rng, 1)[0])
        a = _image(rng, uq, D)
        b = _image(rng, np.array(uj), np.array(dj))
        return _case([a, b], [(0, 1), (1, 0)], radius=(r, r))
    if name == "extremes":
        # all-0 against all-255: d = 8 323 200, the largest there is; thr^2 in float32 just above and just below it
        r = 5.0
        pattern = np.where(np.arange(128) % 2, 255, 0)
        ua = np.array([[10.0, 10.0], [100.0, 10.0], [200.0, 10.0], [300.0, 10.0]])
        da = np.array([np.zeros(128), np.full(128, 255), pattern, np.zeros(128)])
        ub = np.array([[11.0, 11.0], [101.0, 9.0], [200.25, 10.0], [300.0, 10.25], [304.75, 14.75]])
        db = np.array([np.full(128, 255), np.zeros(128), 255 - pattern, np.full(128, 255), np.concatenate([[1], np.full(127, 255)])])
        t = np.sqrt(np.float32(8323200.0))
        lo, hi = t, t
        while np.float32(lo) * np.float32(lo) >= np.float32(8323200.0):
            lo = np.nextafter(np.float32(lo), np.float32(0.0))
        while np.float32(hi) * np.float32(hi) <= np.float32(8323200.0):
            hi = np.nextafter(np.float32(hi), np.float32(INF))
        return _case([_image(rng, ua, da), _image(rng, ub, db)], [(0, 1), (1, 0)], radius=(r, r), thrs=[float(lo), float(hi), THR])
    if name == "boxed":
        # boxes that cut through windows (a keypoint outside the box is no candidate however near), an empty side, NaN padding rows,
        # and the same images in several pairs of one call with different boxes
        a, b = _views(rng, 500, 1000.0, 1100.0, jitter=1.5, extra=60)
        a = (np.concatenate([a[0], np.full((11, 132), np.nan, dtype=np.float32)]), np.concatenate([a[1], np.full((11, 2), np.nan)]))
        b = (np.concatenate([b[0][:200], np.full((5, 132), np.nan, dtype=np.float32), b[0][200:]]), np.concatenate([b[1][:200], np.full((5, 2), np.nan), b[1][200:]]))
        c = _views(rng, 90, 1040.0, 1060.0, jitter=1.0)[1]
        boxes = [(1000.0, 1100.0, 1000.0, 1100.0), (1030.0, 1070.5, 1020.25, 1081.0), (1050.0, 1050.25, 1000.0, 1100.0), (2000.0, 2100.0, 1000.0, 1100.0),
                 (1049.0, INF, -INF, 1062.0), (1030.0, 1070.5, 1020.25, 1081.0), EVERYWHERE]
        return _case([a, b, c], [(0, 1), (0, 1), (0, 1), (0, 1), (1, 0), (2, 0), (1, 2)], boxes)
    if name == "float":
        a, b = _views(rng, 300, 0.0, 80.0, jitter=1.5, extra=40)
        for f in (a[0], b[0]):
            f[:, 4:] /= np.float32(CM.FLOAT_SCALE)
        return _case([a, b], [(0, 1), (1, 0)], scale=CM.FLOAT_SCALE)
    raise KeyError(name)

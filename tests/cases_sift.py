"""
Cases of the SIFT detection (satba.ft_s2p) shared by tools/gen_golden_sift.py, which runs the reference's compiled `sift` on them
and writes tests/golden/ft_sift.npz, and by the tests, which only read that file.

`detect` restates in numpy float64 the whole chain that the device runs in float32 (include/satba.h, satba_sift_detect; DESIGN.md
section 4m): geometry and tap tables as the reference's floats, then oversampling, blurs, discrete extrema, interpolation, the
discards, orientations and descriptors in float64.  It reports the staged counts of the device's `counts` and, per candidate, a
margin: the smallest relative distance of any decision the candidate went through from that decision's threshold --

    the two value thresholds (0.8 thr before, thr after the interpolation), the 0.6 offsets, the edge ratio, the four border
    comparisons, a secondary orientation peak against 0.8 max,

and, apart from those, the strictness of the discrete extremum as an absolute DoG difference.  A candidate is *fragile* when the
relative margin is below MARGIN = 1e-3 or the strictness below EXT_EPS.  The offsets count at every interpolation step, not only at
the last: a step that moves in one arithmetic and converges in the other changes the keypoint just as the last one does.
EXT_EPS = 2e-6 comes from the reference's own error: a DoG sample formed from its Gaussian planes differs from the rule's by at most
3.5e-7 (`spread_dog` of the fixture; the generator asserts 2 spread_dog <= EXT_EPS), a comparison u - v by twice that, and two float32
chains from each other by twice that again, 1.4e-6.
The candidate list also holds the samples that miss being a candidate by less than those margins (`real` false): a float32
chain may keep them.  Unpaired keypoints are allowed only at fragile candidates.
"""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ft_sift.npz")
MARGIN = 1e-3
EXT_EPS = 2e-6
THRESH_DOG = 0.0133
DELTA_MIN, SIGMA_MIN, SIGMA_IN = np.float32(0.5), np.float32(0.8), np.float32(0.5)
OFF_MAX, EDGE, LAMBDA_ORI, LAMBDA_DES, T_ORI = 0.6, 10.0, 1.5, 6.0, 0.8
N_BINS, N_HIST, N_ORI, MAX_ITER = 36, 4, 8, 5
PAIR_PX, PAIR_SIGMA, PAIR_THETA = 0.05, 0.02, 0.05
SPREAD_KEYS = ("col", "row", "sigma", "theta", "desc_inf", "desc_l2")

# name -> (height, width, seed, thresh_dog, nb_octaves); "flat" is the constant image, view_a / view_b the chain test's pair
CASES = {
    "s52": (52, 52, 20, THRESH_DOG, 8),
    "s61x83": (61, 83, 20, THRESH_DOG, 8),
    "s83x61": (83, 61, 20, THRESH_DOG, 8),
    "s128x200": (128, 200, 20, THRESH_DOG, 8),
    "s208x300": (208, 300, 20, THRESH_DOG, 8),
    "s61x83_half": (61, 83, 20, THRESH_DOG / 2, 8),
    "s128x200_oct2": (128, 200, 20, THRESH_DOG, 2),
    "flat": (40, 56, 0, THRESH_DOG, 8),
    "view_a": (160, 220, 22, THRESH_DOG, 8),
    "view_b": (160, 220, 22, THRESH_DOG, 8),
}
PARITY_CASES = [c for c in CASES if c != "flat"]
VIEW_SHIFT = (8, 16)  # view_b[r, c] = scene[r + 8, c + 16]: a keypoint of view_a at (col, row) is at (col - 16, row - 8) in view_b
VIEW_MARGIN = 40     # either view is constant for at least this many pixels from each of its borders
VIEW_OCTAVES = 2     # octaves of the chain test: their blurs reach 59 pixels, less than twice the margin


# ----------------------------------------------------------------------------- geometry, as the reference's floats

def octave_count(w, h, nb_octaves):
    h0 = int(np.float32(min(w, h)) / DELTA_MIN)
    q = h0 // 12
    if q < 1:
        return 0
    return min(int(nb_octaves), int(math.log(q) / math.log(2.0)) + 1)


def threshold(thresh_dog, nb_scales):
    k_nspo = np.float32(math.exp(math.log(2.0) / float(np.float32(nb_scales))))
    k_3 = np.float32(math.exp(math.log(2.0) / 3.0))
    return np.float32((k_nspo - np.float32(1)) / (k_3 - np.float32(1)) * np.float32(thresh_dog))


def geometry(w, h, nb_octaves=8, nb_scales=3, thresh_dog=THRESH_DOG):
    """dict: n_oct, n_planes, w, h (per octave), delta, sigma (n_oct, n_planes), inc (n_oct, n_planes), thr; all float32"""
    n = octave_count(w, h, nb_octaves)
    ns = nb_scales + 3
    h0, w0 = int(np.float32(h) / DELTA_MIN), int(np.float32(w) / DELTA_MIN)
    g = {"n_oct": n, "n_planes": ns, "w": [], "h": [], "delta": np.zeros(n, np.float32), "sigma": np.zeros((n, ns), np.float32),
         "inc": np.zeros((n, ns), np.float32), "thr": threshold(thresh_dog, nb_scales)}
    for o in range(n):
        dn = np.float32(DELTA_MIN * np.float32(1 << o))
        g["delta"][o] = dn
        g["h"].append(h0 // (1 << o))
        g["w"].append(w0 // (1 << o))
        for s in range(ns):
            g["sigma"][o, s] = np.float32(float(np.float32(dn / DELTA_MIN) * SIGMA_MIN) * math.pow(2.0, float(np.float32(s) / np.float32(nb_scales))))
        for s in range(1, ns):
            sp, sn = g["sigma"][o, s - 1], g["sigma"][o, s]
            g["inc"][o, s] = np.sqrt(np.float32(sn * sn) - np.float32(sp * sp)) / dn
    if n:
        s0 = g["sigma"][0, 0]
        g["inc"][0, 0] = np.sqrt(np.float32(s0 * s0) - np.float32(SIGMA_IN * SIGMA_IN)) / DELTA_MIN
    return g


def taps(sigma):
    """normalised float32 taps ker[0 .. ceil(4 sigma)]"""
    sigma = np.float32(sigma)
    r = int(np.ceil(np.float32(4) * sigma))
    ker = np.zeros(r + 1, np.float32)
    ker[0] = 1
    if sigma > 0:
        total = np.float32(1)
        for k in range(1, r + 1):
            ker[k] = np.float32(math.exp(-0.5 * float(k) * float(k) / float(sigma) / float(sigma)))
            total = np.float32(total + np.float32(2) * ker[k])
        ker = (ker / total).astype(np.float32)
    return ker


# ----------------------------------------------------------------------------- the planes

def _mirror(idx, n):
    m = np.mod(idx, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def blur(p, sigma):
    ker = taps(sigma).astype(np.float64)
    r = len(ker) - 1
    for axis in (0, 1):  # columns first, as the reference
        n = p.shape[axis]
        e = np.take(p, _mirror(np.arange(-r, n + r), n), axis=axis)
        out = ker[0] * np.take(e, np.arange(r, r + n), axis=axis)
        for k in range(1, r + 1):
            out = out + ker[k] * (np.take(e, np.arange(r - k, r - k + n), axis=axis) + np.take(e, np.arange(r + k, r + k + n), axis=axis))
        p = out
    return p


def oversample(img, ho, wo):
    hi, wi = img.shape
    x, y = np.arange(ho) * 0.5, np.arange(wo) * 0.5
    dx, dy = x.astype(np.int64), y.astype(np.int64)
    im, ip = np.where(dx >= hi, 2 * hi - 1 - dx, dx), np.where(dx + 1 >= hi, 2 * hi - 2 - dx, dx + 1)
    jm, jp = np.where(dy >= wi, 2 * wi - 1 - dy, dy), np.where(dy + 1 >= wi, 2 * wi - 2 - dy, dy + 1)
    fx, fy = (x - np.floor(x))[:, None], (y - np.floor(y))[None, :]
    return fx * (fy * img[np.ix_(ip, jp)] + (1 - fy) * img[np.ix_(ip, jm)]) + (1 - fx) * (fy * img[np.ix_(im, jp)] + (1 - fy) * img[np.ix_(im, jm)])


def gaussian_planes(img, g):
    """per octave an (n_planes, h, w) float64 array"""
    img = np.asarray(img, dtype=np.float64) / 256.0
    out = []
    for o in range(g["n_oct"]):
        planes = np.zeros((g["n_planes"], g["h"][o], g["w"][o]))
        if o == 0:
            planes[0] = blur(oversample(img, g["h"][0], g["w"][0]), g["inc"][0, 0])
        else:
            planes[0] = out[o - 1][g["n_planes"] - 3][0:2 * g["h"][o]:2, 0:2 * g["w"][o]:2]
        for s in range(1, g["n_planes"]):
            planes[s] = blur(planes[s - 1], g["inc"][o, s])
        out.append(planes)
    return out


def gradient(p):
    """(gx along the rows' index, gy along the columns'): centred inside, one-sided and not halved on the border"""
    gx, gy = np.zeros_like(p), np.zeros_like(p)
    gy[:, 1:-1] = (p[:, 2:] - p[:, :-2]) * 0.5
    gy[:, 0], gy[:, -1] = p[:, 1] - p[:, 0], p[:, -1] - p[:, -2]
    gx[1:-1] = (p[2:] - p[:-2]) * 0.5
    gx[0], gx[-1] = p[1] - p[0], p[-1] - p[-2]
    return gx, gy


# ----------------------------------------------------------------------------- candidates

def _rel(a, b):
    return abs(a / b - 1.0) if b != 0 else np.inf


def _taylor(D, s, i, j):
    c = D[s, i, j]
    hXX = D[s, i - 1, j] + D[s, i + 1, j] - 2 * c
    hYY = D[s, i, j + 1] + D[s, i, j - 1] - 2 * c
    hSS = D[s - 1, i, j] + D[s + 1, i, j] - 2 * c
    hXY = 0.25 * ((D[s, i + 1, j + 1] - D[s, i + 1, j - 1]) - (D[s, i - 1, j + 1] - D[s, i - 1, j - 1]))
    hXS = 0.25 * ((D[s + 1, i + 1, j] - D[s + 1, i - 1, j]) - (D[s - 1, i + 1, j] - D[s - 1, i - 1, j]))
    hYS = 0.25 * ((D[s + 1, i, j + 1] - D[s + 1, i, j - 1]) - (D[s - 1, i, j + 1] - D[s - 1, i, j - 1]))
    gX, gY, gS = 0.5 * (D[s, i + 1, j] - D[s, i - 1, j]), 0.5 * (D[s, i, j + 1] - D[s, i, j - 1]), 0.5 * (D[s + 1, i, j] - D[s - 1, i, j])
    det = hXX * hYY * hSS - hXX * hYS * hYS - hXY * hXY * hSS + 2 * hXY * hXS * hYS - hXS * hXS * hYY
    with np.errstate(divide="ignore", invalid="ignore"):
        aa, ab, ac = (hYY * hSS - hYS * hYS) / det, (hXS * hYS - hXY * hSS) / det, (hXY * hYS - hXS * hYY) / det
        bb, bc, cc = (hXX * hSS - hXS * hXS) / det, (hXY * hXS - hXX * hYS) / det, (hXX * hYY - hXY * hXY) / det
        oi, oj, os_ = -aa * gX - ab * gY - ac * gS, -ab * gX - bb * gY - bc * gS, -ac * gX - bc * gY - cc * gS
        return oi, oj, os_, c + 0.5 * (gX * oi + gY * oj + gS * os_)


def _refine(D, g, o, s, i, j, img_h, img_w, c):
    """follows one candidate through interpolation, discards, edge and border tests; fills c (stage, margin, x, y, sigma, s)"""
    ns, h, w = D.shape
    delta, thr = float(g["delta"][o]), float(g["thr"])
    ic, jc, sc, conv = i, j, s, False
    oi = oj = os_ = val = 0.0
    for _ in range(MAX_ITER):
        if 0 < ic < h - 1 and 0 < jc < w - 1:
            oi, oj, os_, val = _taylor(D, sc, ic, jc)
            for off in (oi, oj, os_):
                if np.isfinite(off):
                    c["margin"] = min(c["margin"], _rel(abs(off), OFF_MAX))
        else:
            oi = oj = os_ = 5.0
        if abs(oi) < OFF_MAX and abs(oj) < OFF_MAX and abs(os_) < OFF_MAX:
            conv = True
            break
        if oi > OFF_MAX and ic + 1 < h - 1:
            ic += 1
        if oj > OFF_MAX and jc + 1 < w - 1:
            jc += 1
        if oi < -OFF_MAX and ic - 1 > 0:
            ic -= 1
        if oj < -OFF_MAX and jc - 1 > 0:
            jc -= 1
        if os_ > OFF_MAX and sc + 1 < ns - 1:
            sc += 1
        if os_ < -OFF_MAX and sc - 1 > 0:
            sc -= 1
    if not conv:
        return
    c["stage"] = 2
    ratio = float(g["sigma"][0, 1]) / float(g["sigma"][0, 0])
    x, y, sigma = (ic + oi) * delta, (jc + oj) * delta, float(g["sigma"][o, sc]) * ratio ** os_
    c["margin"] = min(c["margin"], _rel(abs(val), thr))
    if not abs(val) > thr:
        return
    cc = D[sc, ic, jc]
    hXX = D[sc, ic - 1, jc] + D[sc, ic + 1, jc] - 2 * cc
    hYY = D[sc, ic, jc + 1] + D[sc, ic, jc - 1] - 2 * cc
    hXY = ((D[sc, ic + 1, jc + 1] - D[sc, ic + 1, jc - 1]) - (D[sc, ic - 1, jc + 1] - D[sc, ic - 1, jc - 1])) / 4.0
    with np.errstate(divide="ignore", invalid="ignore"):
        edge = (hXX + hYY) * (hXX + hYY) / (hXX * hYY - hXY * hXY)
    e_thr = (EDGE + 1) * (EDGE + 1) / EDGE
    if np.isfinite(edge):
        c["margin"] = min(c["margin"], _rel(abs(edge), e_thr))
    if abs(edge) > e_thr:
        return
    for a, b in ((x, sigma), (x + sigma, float(img_h)), (y, sigma), (y + sigma, float(img_w))):
        c["margin"] = min(c["margin"], _rel(a, b))
    if x <= sigma or x + sigma >= img_h or y <= sigma or y + sigma >= img_w:
        return
    c.update(stage=3, x=x, y=y, sigma=sigma, s=sc)


def _orientations(gx, gy, c, delta):
    h, w = gx.shape
    xk, yk, sk = c["x"] / delta, c["y"] / delta, c["sigma"] / delta
    R = 3 * LAMBDA_ORI * sk
    i0, j0 = max(0, int(xk - R + 0.5)), max(0, int(yk - R + 0.5))
    i1, j1 = min(int(xk + R + 0.5), h - 1), min(int(yk + R + 0.5), w - 1)
    hist = np.zeros(N_BINS)
    if i1 >= i0 and j1 >= j0:
        si, sj = np.meshgrid(np.arange(i0, i1 + 1), np.arange(j0, j1 + 1), indexing="ij")
        sX, sY = (si - xk) / sk, (sj - yk) / sk
        dx, dy = gx[i0:i1 + 1, j0:j1 + 1], gy[i0:i1 + 1, j0:j1 + 1]
        ori = np.mod(np.arctan2(dy, dx), 2 * np.pi)
        m = np.hypot(dx, dy) * np.exp(-(sX * sX + sY * sY) / (2 * LAMBDA_ORI * LAMBDA_ORI))
        b = (ori / (2 * np.pi) * N_BINS + 0.5).astype(np.int64) % N_BINS
        np.add.at(hist, b.ravel(), m.ravel())
    for _ in range(6):
        hist = (np.roll(hist, 1) + hist + np.roll(hist, -1)) / 3.0
    mx, thetas = hist.max(), []
    for b in range(N_BINS):
        hc, hp, hn = hist[b], hist[(b - 1) % N_BINS], hist[(b + 1) % N_BINS]
        if hc > hp and hc > hn:
            if hc != mx:
                c["margin"] = min(c["margin"], _rel(hc, T_ORI * mx))
            if hc > T_ORI * mx:
                di = (hp - hn) / (2 * (hp + hn - 2 * hc))
                ori = (b + di + 0.5) * 2 * np.pi / N_BINS
                thetas.append(ori - 2 * np.pi if ori > np.pi else ori)
    return thetas


def _descriptor(gx, gy, c, delta, theta):
    h, w = gx.shape
    xk, yk, sk = c["x"] / delta, c["y"] / delta, c["sigma"] / delta
    cosT, sinT = np.cos(-theta), np.sin(-theta)
    t2 = 1.0 / (2.0 * (LAMBDA_DES * sk) ** 2)
    R = (1 + 1 / N_HIST) * LAMBDA_DES * sk
    Rp = np.sqrt(2.0) * R
    i0, j0 = max(0, int(xk - Rp + 0.5)), max(0, int(yk - Rp + 0.5))
    i1, j1 = min(int(xk + Rp + 0.5), h - 1), min(int(yk + Rp + 0.5), w - 1)
    d = np.zeros(N_HIST * N_HIST * N_ORI)
    if i1 > i0 and j1 > j0:  # the reference's loops stop one short of i1 / j1
        si, sj = np.meshgrid(np.arange(i0, i1), np.arange(j0, j1), indexing="ij")
        X, Y = cosT * (si - xk) - sinT * (sj - yk), sinT * (si - xk) + cosT * (sj - yk)
        ok = (np.abs(X) < R) & (np.abs(Y) < R)
        X, Y, dx, dy = X[ok], Y[ok], gx[i0:i1, j0:j1][ok], gy[i0:i1, j0:j1][ok]
        ori = np.mod(np.arctan2(dy, dx) - theta, 2 * np.pi)
        M = np.hypot(dx, dy) * np.exp(-(X * X + Y * Y) * t2)
        alpha, beta = X / (2 * LAMBDA_DES * sk / N_HIST) + (N_HIST - 1.0) / 2.0, Y / (2 * LAMBDA_DES * sk / N_HIST) + (N_HIST - 1.0) / 2.0
        gamma = ori / (2 * np.pi) * N_ORI
        fi, fj, fg = np.floor(alpha), np.floor(beta), np.floor(gamma)
        v0, v1 = np.where(fi < 0, 0.0, 1.0 - np.abs(fi - alpha)), np.where(fi > N_HIST - 2, 0.0, 1.0 - np.abs(fi + 1 - alpha))
        v2, v3 = np.where(fj < 0, 0.0, 1.0 - np.abs(fj - beta)), np.where(fj > N_HIST - 2, 0.0, 1.0 - np.abs(fj + 1 - beta))
        gl, gr = 1.0 - (gamma - fg), 1.0 - (fg + 1 - gamma)
        ia = np.clip(fi.astype(np.int64), 0, N_HIST - 1)
        ja = np.clip(fj.astype(np.int64), 0, N_HIST - 1)
        ib, jb = np.minimum(ia + 1, N_HIST - 1), np.minimum(ja + 1, N_HIST - 1)
        bl, br = fg.astype(np.int64) % N_ORI, (fg.astype(np.int64) + 1) % N_ORI
        for a, va in ((ia, v0), (ib, v1)):
            for b, vb in ((ja, v2), (jb, v3)):
                np.add.at(d, (a * N_HIST + b) * N_ORI + bl, gl * va * vb * M)
                np.add.at(d, (a * N_HIST + b) * N_ORI + br, gr * va * vb * M)
    thresh = np.sqrt(np.sum(d * d)) * 0.2
    d = np.minimum(d, thresh)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = d * (512.0 / np.sqrt(np.sum(d * d)))
    return np.minimum(np.nan_to_num(q).astype(np.int64), 255).astype(np.float64)


def detect(img, thresh_dog=THRESH_DOG, nb_octaves=8, nb_scales=3):
    """
    The float64 rule.  Returns a dict:
      rows (n, 132) float64, in the reference's list order;  row_cand (n,) index into the candidate list;  row_octave (n,)
      counts: rows, octaves, discrete extrema above 0.8 thr, survivors of the interpolation, survivors of the border test
      cand: (m, 8) float64 per candidate: octave, scale, row, column of the discrete extremum, real (0 / 1), stage reached
            (1 extremum, 2 interpolated, 3 kept), relative margin, strictness
      fragile (m,) bool;  planes: per octave (n_planes, h, w);  geom
    """
    img = np.asarray(img, dtype=np.float64)
    img_h, img_w = img.shape
    g = geometry(img_w, img_h, nb_octaves, nb_scales, thresh_dog)
    planes = gaussian_planes(img, g)
    thr = float(g["thr"])
    rows, row_cand, row_oct, cand = [], [], [], []
    for o in range(g["n_oct"]):
        G = planes[o]
        D = G[1:] - G[:-1]
        delta = float(g["delta"][o])
        grads = {}
        c0 = D[1:-1, 1:-1, 1:-1]
        lo, hi = np.full(c0.shape, np.inf), np.full(c0.shape, np.inf)  # smallest u - v and smallest v - u over the 26 neighbours
        for ds in (0, 1, 2):
            for di in (0, 1, 2):
                for dj in (0, 1, 2):
                    if (ds, di, dj) == (1, 1, 1):
                        continue
                    u = D[ds:ds + c0.shape[0], di:di + c0.shape[1], dj:dj + c0.shape[2]]
                    lo, hi = np.minimum(lo, u - c0), np.minimum(hi, c0 - u)
        strict = np.maximum(lo, hi)  # > 0: a strict extremum
        near = (strict > -EXT_EPS) & (np.abs(c0) > 0.8 * thr * (1 - MARGIN))
        for s, i, j in np.argwhere(near) + 1:
            v = D[s, i, j]
            c = {"o": o, "s": int(s), "s0": int(s), "i": int(i), "j": int(j), "stage": 0, "strict": float(strict[s - 1, i - 1, j - 1]),
                 "margin": _rel(abs(v), 0.8 * thr)}
            c["real"] = c["strict"] > 0 and abs(v) > 0.8 * thr
            cand.append(c)
            if not c["real"]:
                continue
            c["stage"] = 1
            _refine(D, g, o, int(s), int(i), int(j), img_h, img_w, c)
            if c["stage"] < 3:
                continue
            if c["s"] not in grads:
                grads[c["s"]] = gradient(G[c["s"]])
            gx, gy = grads[c["s"]]
            for theta in _orientations(gx, gy, c, delta):
                rows.append(np.concatenate([[c["y"], c["x"], c["sigma"], theta], _descriptor(gx, gy, c, delta, theta)]))
                row_cand.append(len(cand) - 1)
                row_oct.append(o)
    table = np.array([[c["o"], c["s0"], c["i"], c["j"], float(c["real"]), c["stage"], c["margin"], c["strict"]] for c in cand],
                     dtype=np.float64).reshape(-1, 8)
    fragile = (table[:, 6] < MARGIN) | (np.abs(table[:, 7]) < EXT_EPS) if len(cand) else np.zeros(0, bool)
    stage = table[:, 5] if len(cand) else np.zeros(0)
    counts = np.array([len(rows), g["n_oct"], int(np.sum(stage >= 1)), int(np.sum(stage >= 2)), int(np.sum(stage >= 3))], dtype=np.int64)
    return {"rows": np.array(rows, dtype=np.float64).reshape(-1, 132), "row_cand": np.array(row_cand, dtype=np.int64),
            "row_octave": np.array(row_oct, dtype=np.int64), "counts": counts, "cand": table, "fragile": fragile, "planes": planes, "geom": g}


# ----------------------------------------------------------------------------- pairing and spreads

def theta_diff(a, b):
    d = np.abs(a - b) % (2 * np.pi)
    return np.minimum(d, 2 * np.pi - d)


def pair_rows(a, b, px=PAIR_PX, rel_sigma=PAIR_SIGMA, rad=PAIR_THETA):
    """one-to-one pairing of keypoint rows inside the window; returns (ia, ib) index arrays, nearest first come first served"""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 132), np.asarray(b, dtype=np.float64).reshape(-1, 132)
    used, ia, ib = np.zeros(len(b), bool), [], []
    for k in range(len(a)):
        if not len(b):
            break
        ok = (np.abs(b[:, 0] - a[k, 0]) <= px) & (np.abs(b[:, 1] - a[k, 1]) <= px) & (np.abs(b[:, 2] - a[k, 2]) <= rel_sigma * a[k, 2])
        ok &= (theta_diff(b[:, 3], a[k, 3]) <= rad) & ~used
        idx = np.nonzero(ok)[0]
        if len(idx):
            m = idx[np.argmin(np.hypot(b[idx, 0] - a[k, 0], b[idx, 1] - a[k, 1]) + theta_diff(b[idx, 3], a[k, 3]))]
            used[m] = True
            ia.append(k)
            ib.append(m)
    return np.array(ia, dtype=np.int64), np.array(ib, dtype=np.int64)


def spreads(a, b):
    """largest differences over paired rows a[k] ~ b[k]: col, row, sigma (relative), theta, descriptor L-inf, descriptor L2"""
    if not len(a):
        return np.zeros(6)
    d = np.abs(a[:, 4:] - b[:, 4:])
    return np.array([np.abs(a[:, 0] - b[:, 0]).max(), np.abs(a[:, 1] - b[:, 1]).max(), (np.abs(a[:, 2] - b[:, 2]) / b[:, 2]).max(),
                     theta_diff(a[:, 3], b[:, 3]).max(), d.max(), np.sqrt((d * d).sum(axis=1)).max()])


# ----------------------------------------------------------------------------- images

def _noise(rng, h, w, sigma):
    p = rng.standard_normal((h, w))
    k = np.exp(-0.5 * (np.arange(-int(4 * sigma), int(4 * sigma) + 1) / sigma) ** 2)
    k /= k.sum()
    p = np.apply_along_axis(lambda r: np.convolve(np.pad(r, len(k) // 2, mode="wrap"), k, mode="valid"), 0, p)
    p = np.apply_along_axis(lambda r: np.convolve(np.pad(r, len(k) // 2, mode="wrap"), k, mode="valid"), 1, p)
    return p / p.std()


def texture(h, w, seed):
    """smoothed noise at three scales, integers 0 .. 255 (uint8)"""
    rng = np.random.default_rng([seed, 2024])
    t = _noise(rng, h, w, 2.5) + _noise(rng, h, w, 6.0) + _noise(rng, h, w, 14.0)
    t = (t - t.min()) / (t.max() - t.min())
    return np.rint(255.0 * t).astype(np.uint8)


def view_scene(h, w, seed):
    """The scene both views are cut from: texture inside a window, the constant 128 for VIEW_MARGIN pixels and more around it in
    either view.  A blur mirrors a view at its border; with a flat margin what it mirrors in is what the other view sees there, so
    away from the border by less than twice the margin the two views' planes are the same function of the scene."""
    H, W = h + VIEW_SHIFT[0], w + VIEW_SHIFT[1]
    m0, m1 = VIEW_MARGIN + VIEW_SHIFT[0], VIEW_MARGIN + VIEW_SHIFT[1]

    def ramp(n, m):  # 0 up to m, a raised cosine over 12 samples, 1 inside
        d = np.minimum(np.arange(n) - m, n - 1 - m - np.arange(n))
        return np.where(d <= 0, 0.0, np.where(d >= 12, 1.0, 0.5 - 0.5 * np.cos(np.pi * np.clip(d, 0, 12) / 12.0)))

    win = ramp(H, m0)[:, None] * ramp(W, m1)[None, :]
    return np.rint(128.0 + (texture(H, W, seed).astype(np.float64) - 128.0) * win).astype(np.uint8)


def image(name):
    h, w, seed = CASES[name][:3]
    if name == "flat":
        return np.full((h, w), 97, dtype=np.uint8)
    if name in ("view_a", "view_b"):
        scene = view_scene(h, w, seed)
        return scene[:h, :w].copy() if name == "view_a" else scene[VIEW_SHIFT[0]:, VIEW_SHIFT[1]:].copy()
    if name == "s83x61":
        return texture(61, 83, seed).T.copy()
    return texture(h, w, seed)


def load():
    return np.load(GOLDEN)


def pack(name, img, ref, rule):
    """the arrays of one case as the fixture stores them: descriptors as uint8, the candidate table as small integers"""
    ref = np.asarray(ref).reshape(-1, 132)
    c = rule["cand"]
    return {name + "_image": img, name + "_ref_kp": ref[:, :4].astype(np.float32), name + "_ref_desc": ref[:, 4:].astype(np.uint8),
            name + "_rule_kp": rule["rows"][:, :4], name + "_rule_desc": rule["rows"][:, 4:].astype(np.uint8),
            name + "_rule_octave": rule["row_octave"].astype(np.int8), name + "_rule_cand": rule["row_cand"].astype(np.int32),
            name + "_counts": rule["counts"], name + "_cand": c[:, :6].astype(np.int16), name + "_cand_margin": c[:, 6:].astype(np.float32),
            name + "_fragile": rule["fragile"]}


def case(z, name):
    """one case of the fixture: image, ref (n, 132) float32, rule (m, 132) float64, rule_octave, rule_cand, counts, cand, fragile"""
    get = lambda k: z[name + "_" + k]  # noqa: E731
    return {"image": get("image"), "ref": np.concatenate([get("ref_kp"), get("ref_desc").astype(np.float32)], axis=1),
            "rule": np.concatenate([get("rule_kp"), get("rule_desc").astype(np.float64)], axis=1), "rule_octave": get("rule_octave").astype(np.int64),
            "rule_cand": get("rule_cand").astype(np.int64), "counts": get("counts"),
            "cand": np.concatenate([get("cand").astype(np.float64), get("cand_margin").astype(np.float64)], axis=1), "fragile": get("fragile"),
            "thresh_dog": CASES[name][3], "nb_octaves": CASES[name][4]}


def fragile_near(cand, fragile, delta, row, reach=6.0):
    """is a fragile candidate within `reach` samples (of its octave) of the keypoint row?  delta: per octave"""
    for c in cand[fragile]:
        d = float(delta[int(c[0])])
        if abs(c[2] * d - row[1]) <= reach * d and abs(c[3] * d - row[0]) <= reach * d:
            return True
    return False

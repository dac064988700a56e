"""
Scenarios of the outlier rejection (csrc/satba_outliers.h, satba/ba_outliers.py) shared by tests/test_outliers_cases_host.py,
tests/test_gpu_outliers.py and tools/gen_golden.py (sections outliers_edges and rm_outliers).  Nothing here needs a GPU or the
reference: `rule` restates ref:bundle_adjust/ba_outliers.py:112-155 with numpy, the builders make the error vectors on which that
rule is fragile, and `layout` cuts observation lists with prescribed per-camera counts out of an affine scene.
"""
import numpy as np

from satba import ba_outliers, synth

# ---------------------------------------------------------------------------------------------------------------------------------
# the rule


def rule(err, cam_ind, n_cam, predef_thr=None, min_thr=1.0):
    """
    (cam_thr (n_cam,) float64, remove (K,) bool): ref:bundle_adjust/ba_outliers.py:112-155 line for line, per camera, with the host
    get_elbow_value (pinned on reference vectors in tests/test_host_logic.py).  A camera without observations gets the threshold 0.0
    and removes nothing (the device's choice; the reference raises IndexError there).
    """
    err = np.asarray(err, dtype=np.float64)
    cam_ind = np.asarray(cam_ind)
    cam_thr = []
    for cam_idx in range(n_cam):
        if predef_thr is None:
            e = err[cam_ind == cam_idx]
            if e.size == 0:
                cam_thr.append(0.0)
                continue
            elbow_value, success = ba_outliers.get_elbow_value(e)
            thr = max(elbow_value, min_thr) if success else np.max(e)
            cam_thr.append(np.round(thr, 2))
        else:
            cam_thr.append(np.round(float(predef_thr), 2))
    remove = np.zeros(err.size, dtype=bool)
    for cam_idx, thr in enumerate(cam_thr):
        sel = cam_ind == cam_idx
        remove[sel] = err[sel] > thr
    return np.array(cam_thr, dtype=np.float64), remove


def chord_distances(v, dtype=np.float64):
    """Distances of the sorted values to their chord, the operations of get_elbow_value evaluated in `dtype` (np.longdouble stands in
    for a contracted or re-ordered evaluation: every product and sum rounds differently)."""
    v = np.sort(np.asarray(v, dtype=np.float64)).astype(dtype)
    n = v.size
    line = np.array([n - 1.0, v[-1] - v[0]], dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u = line / np.sqrt(np.sum(line ** 2))
        px, py = np.arange(n).astype(dtype), v - v[0]
        sp = px * u[0] + py * u[1]
        return np.sqrt((px - sp * u[0]) ** 2 + (py - sp * u[1]) ** 2), u


def threshold_in(v, dtype, min_thr=1.0):
    """The rounded threshold of one vector when the distances are evaluated in `dtype` (everything after the argmax in float64)."""
    s = np.sort(np.asarray(v, dtype=np.float64))
    d, _ = chord_distances(s, dtype)
    elbow = s[int(np.argmax(d))] if not np.all(np.isnan(d)) else s[0]
    success = not (elbow < np.percentile(s, 80))
    return np.round(max(elbow, min_thr) if success else s[-1], 2)


def threshold_mutated(v, mutation, min_thr=0.0):
    """
    The rounded threshold of one vector under one of the two mistakes a kernel can make without a random vector noticing:
    "fma": the scalar product evaluated as fma(px, ux, py * uy) -- exactly (rational arithmetic, one rounding) --, everything else as
    the reference has it; "last": the last of the tied maxima instead of the first.
    """
    from fractions import Fraction

    s = np.sort(np.asarray(v, dtype=np.float64))
    n = s.size
    line = np.array([n - 1.0, s[-1] - s[0]])
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u = line / np.sqrt(np.sum(line ** 2))
        px, py = np.arange(n, dtype=np.float64), s - s[0]
        t = py * u[1]
        if mutation == "fma":
            ux = Fraction(float(u[0]))
            sp = np.array([float(Fraction(float(px[i])) * ux + Fraction(float(t[i]))) for i in range(n)])
        else:
            sp = px * u[0] + t
        d = np.sqrt((px - sp * u[0]) ** 2 + (py - sp * u[1]) ** 2)
    arg = int(np.argmax(d)) if mutation == "fma" else int(n - 1 - np.argmax(d[::-1]))
    elbow = s[arg]
    success = not (elbow < np.percentile(s, 80))
    return np.round(max(elbow, min_thr) if success else s[-1], 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# error vectors: deterministic from (pattern, n, seed), finite and non-negative

HALF_ELBOWS = {"half_0.125": 0.125, "half_0.285": 0.285, "half_1.005": 1.005, "half_2.675": 2.675, "half_1e6": 1e6 + 0.005}
PATTERNS = ("random", "equal_0", "equal_2.5", "plateau", "no_elbow", "min_thr") + tuple(HALF_ELBOWS) + ("wide",)
MIN_THRS = (0.0, 1.0, 2.75)
PREDEF_THRS = (3.14159, 2.675, 0.125, 1e-3, 1e6 + 0.005)
SHAPED_MIN_N = 250  # below it the shaped patterns (plateau, no_elbow, min_thr, half_*) have no room: they fall back to "random"


def _rng(pattern, n, seed):
    return np.random.default_rng([PATTERNS.index(pattern), int(n), int(seed)])


def _random(rng, n):
    """|N(0, 1)| plus 10 % gross errors: the vectors of tools/gen_golden.py golden_outliers."""
    return np.abs(rng.normal(0, 1, n)) + (rng.random(n) < 0.1) * rng.uniform(5, 50, n)


def _plateau(rng, n):
    """
    Sorted curve with a stretch parallel to the chord: with the chord's slope s = V / (n - 1), v[i] = v0 + s i - h on [a, b) =
    [0.85 n, 0.95 n), a slow linear ramp from v0 up to v[a] before it and a linear rise to v0 + V after it.  Every point of the stretch
    is at the same distance from the chord mathematically, so rounding alone picks the argmax, and the candidates' values differ by
    0.1 V = 2 to 8 px.
    """
    V, v0 = rng.uniform(20.0, 80.0), rng.uniform(0.0, 0.5)
    a, b = int(0.85 * n), int(0.95 * n)
    s = V / (n - 1)
    h = rng.uniform(0.7, 0.95) * s * a
    i = np.arange(n, dtype=np.float64)
    v = np.empty(n)
    v[a:b] = v0 + s * i[a:b] - h
    v[:a] = v0 + (v[a] - v0) * i[:a] / a
    v[b:] = v[b - 1] + (v0 + V - v[b - 1]) * (i[b:] - (b - 1)) / (n - b)
    return v


def _no_elbow(rng, n):
    """A step at half the length: the point farthest from the chord is the last one before the step, far below the 80th percentile."""
    v = np.concatenate([rng.uniform(0.0, 0.2, n // 2), rng.uniform(10.0, 10.2, n - n // 2)])
    return v


def _min_thr(rng, n):
    """Bulk (88 %) below 0.4 px, then a tail that rises quadratically to 12.4 px: the elbow sits at the knee, about 0.4 to 0.6 px, so
    min_thr = 1.0 and 2.75 bind and 0.0 does not.  The vector holds 1.0 and 2.75 and their upper neighbours: an error equal to a binding
    min_thr stays, the next double goes."""
    nt = n - int(0.88 * n)
    tail = 0.4 + 12.0 * np.linspace(0.0, 1.0, nt) ** 2
    planted = [1.0, np.nextafter(1.0, np.inf), 2.75, np.nextafter(2.75, np.inf)]
    return np.concatenate([rng.uniform(0.0, 0.4, n - nt - 4), planted, tail])


def _half(rng, n, E):
    """
    An L whose knee is the single value E, with one value equal to R = round(E, 2) and one a double above it.
    R < E (the product E * 100 lies at or below the half and rint goes down): a sharp L -- the bulk (88 %) below E, holding R and its
    neighbour, then E, then a tail that starts at 40 E + 5 and rises to 100 E + 40.
    R > E (2.675 * 100 is 267.5 exactly in float64 and rint goes to the even 268): R and its neighbour come right after E, and any
    point between the knee and a steep rise would be the knee itself.  So the chord is made flat, slope s = 0.4 (R - E) per index: the
    bulk approaches E at 0.3 s per index, the step from E to R is 2.5 s, and the tail rises at about 6 s.
    """
    R = np.round(E, 2)
    nb = int(0.88 * n)
    if R < E:
        bulk = rng.uniform(0.0, E, nb)
        bulk[:2] = [R, np.nextafter(R, np.inf)]
        tail = np.linspace(40.0 * E + 5.0, 100.0 * E + 40.0, n - nb - 1) + rng.uniform(0.0, 1e-3, n - nb - 1)
        return np.concatenate([bulk, [E], tail])
    s = 0.4 * (R - E)
    bulk = E - 0.3 * s * (nb - np.arange(nb) + rng.uniform(-0.1, 0.1, nb))
    nt = n - nb - 3
    tail = np.linspace(R + 2.0 * (R - E), bulk[0] + s * (n - 1), nt)
    return np.concatenate([bulk, [E, R, np.nextafter(R, np.inf)], tail])


def _wide(rng, n):
    """Log-uniform from 1e-300 to 1e200, a subnormal below: the square of the value range overflows."""
    v = 10.0 ** rng.uniform(-300.0, 200.0, n)
    v[0] = 1e200
    if n > 1:
        v[1] = 1e-300
    if n > 2:
        v[2] = 1e-310
    return v


def errors(pattern, n, seed):
    """(n,) float64 error values of a pattern, in shuffled (not sorted) order."""
    if pattern not in PATTERNS:
        raise KeyError(pattern)
    rng = _rng(pattern, n, seed)
    if n == 0:
        return np.zeros(0)
    if pattern.startswith("equal_"):
        return np.full(n, float(pattern[len("equal_"):]))
    if pattern == "wide":
        v = _wide(rng, n)
    elif pattern == "random" or n < SHAPED_MIN_N:
        v = _random(rng, n)
    elif pattern == "plateau":
        v = _plateau(rng, n)
    elif pattern == "no_elbow":
        v = _no_elbow(rng, n)
    elif pattern == "min_thr":
        v = _min_thr(rng, n)
    else:
        v = _half(rng, n, HALF_ELBOWS[pattern])
    return v[rng.permutation(n)]


# ---------------------------------------------------------------------------------------------------------------------------------
# problems with prescribed per-camera observation counts

N_CAM = 12
# EDGES: nothing, a point, a chord without an interior, one interior point, one pass of the 256 threads of k_out_elbow short of / exactly /
# beyond full, two passes, four passes and one more, and a segment in the range hipcub's segmented radix sort hands to its large-segment
# kernel (the bench shape has 50 000 per camera).  BULK: every camera in the range the pipeline's small runs have.
LAYOUTS = {"edges": (0, 1, 2, 3, 255, 256, 257, 511, 512, 513, 1025, 70001), "bulk": None}
_layout_cache = {}


def counts(name):
    if name == "bulk":
        return tuple(int(c) for c in np.random.default_rng(77).integers(1000, 3001, N_CAM))
    return LAYOUTS[name]


def layout(name):
    """
    dict(scene, pts_ind, cam_ind, pts2d, pts3d, counts): observation lists, point-major with cameras ascending, in which camera c has
    exactly counts(name)[c] observations -- cut from an affine synth scene of 12 cameras in which every camera sees every point (camera c
    keeps a seeded random subset of the points; points nobody keeps are dropped and the rest renumbered).
    """
    if name in _layout_cache:
        return _layout_cache[name]
    cnt = counts(name)
    n_pts = max(cnt)
    scene = synth.make_affine_scene(N_CAM, n_pts, N_CAM, seed=19, sigma_theta=2e-6)
    assert scene.n_obs == N_CAM * n_pts  # full visibility: observation (q, c) is entry q * N_CAM + c
    rng = np.random.default_rng([23, list(LAYOUTS).index(name)])
    keep = np.zeros((n_pts, N_CAM), dtype=bool)
    for c, k in enumerate(cnt):
        keep[rng.choice(n_pts, size=k, replace=False), c] = True
    used = keep.any(axis=1)
    new_index = np.cumsum(used) - 1
    flat = keep.ravel()
    out = dict(scene=scene, counts=cnt, pts_ind=new_index[scene.pts_ind[flat]], cam_ind=scene.cam_ind[flat], pts2d=scene.pts2d[flat],
               pts3d=scene.pts3d[used])
    assert np.array_equal(np.bincount(out["cam_ind"], minlength=N_CAM), cnt)
    _layout_cache[name] = out
    return out


def layout_params(name, dense=False):
    """BundleAdjustmentParameters of a layout: from the observation lists, or (dense) through the correspondence matrix."""
    from satba.ba_params import BundleAdjustmentParameters

    L = layout(name)
    s = L["scene"]
    d = {"correction_params": ["R"], "n_cam_fix": 0, "reduce": False, "verbose": False}
    if dense:
        C = np.full((2 * N_CAM, L["pts3d"].shape[0]), np.nan)
        C[2 * L["cam_ind"], L["pts_ind"]] = L["pts2d"][:, 0]
        C[2 * L["cam_ind"] + 1, L["pts_ind"]] = L["pts2d"][:, 1]
        return BundleAdjustmentParameters(C, L["pts3d"], s.cameras, "affine", s.pairs_to_triangulate, s.camera_centers, d)
    return BundleAdjustmentParameters.from_observations(L["pts_ind"], L["cam_ind"], L["pts2d"], L["pts3d"], s.cameras, "affine",
                                                        s.pairs_to_triangulate, s.camera_centers, d)


def layout_errors(name, pattern, seed=0):
    """(K,) errors of a layout: camera c's observations carry errors(pattern, counts[c], seed + c), already shuffled by the builder (the
    point-major order scatters them over the vector anyway; the shuffle keeps a camera's values from arriving sorted)."""
    L = layout(name)
    err = np.zeros(L["cam_ind"].size)
    for c, k in enumerate(L["counts"]):
        err[L["cam_ind"] == c] = errors(pattern, k, seed + c)
    return err


def edge_cases():
    """(key, layout, pattern, predef_thr, min_thr) of every case of the golden outliers_edges: all patterns on both layouts at the three
    min_thr, and the predefined thresholds on the random errors."""
    out = []
    for lay in LAYOUTS:
        for pat in PATTERNS:
            for m in MIN_THRS:
                out.append(("{}/{}/min{}".format(lay, pat, m), lay, pat, None, m))
        for k, t in enumerate(PREDEF_THRS):
            out.append(("{}/random/predef{}".format(lay, k), lay, "random", t, 1.0))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# rm_outliers against the reference's own (tools/gen_golden.py golden_rm_outliers, tests/golden/rm_outliers.npz)

# name: (camera model, cameras, tracks, observations per track, scene seed, options, share of gross errors, rm_outliers keywords)
RM_CASES = {
    # fixed points (float32 coordinates: the reference writes them into the float32 array its triangulation returns) and a pair list
    # that omits some camera pairs and writes one reversed (it never matches a track's pairs, which are written i < j)
    "affine": ("affine", 7, 400, 4, 41, {"correction_params": ["R"], "n_cam_fix": 1, "n_pts_fix": 12, "ref_cam_weight": 2.0}, 0.05, {}),
    "persp": ("perspective", 6, 300, 3, 42, {"correction_params": ["R", "T"], "n_cam_fix": 1}, 0.05, {}),
    "rpc": ("rpc", 6, 300, 4, 43, {"correction_params": ["R"], "n_cam_fix": 1}, 0.05, {"min_thr": 2.0}),
    # nothing detected: no gross errors and a predefined threshold above every error
    "clean": ("affine", 5, 200, 3, 44, {"correction_params": ["R"], "n_cam_fix": 0}, 0.0, {"predef_thr": 1000.0}),
}


def rm_pairs(name, M):
    if name == "affine":
        pairs = [(i, j) for i in range(M) for j in range(i + 1, M) if (i * 5 + j) % 7 != 0]
        pairs[4] = (pairs[4][1], pairs[4][0])
        return pairs
    if name == "rpc":  # the scene cycles two RPCs over its cameras: only pairs of different models have a baseline
        return [(i, j) for i in range(M) for j in range(i + 1, M) if (i + j) % 2 == 1]
    return [(i, j) for i in range(M) for j in range(i + 1, M)]


def rm_case(name):
    """(scene, options, rm_outliers keywords): the seeded scene with its gross errors injected into pts2d and its pair list set."""
    model, M, N, opp, seed, d, frac, kw = RM_CASES[name]
    scene = synth.make_scene(model, M, N, opp, seed=seed, **({"sigma_theta": 1e-6} if model == "rpc" else {}))
    scene.pts3d = scene.pts3d.astype(np.float32)
    rng = np.random.default_rng(seed + 100)
    bad = rng.random(scene.n_obs) < frac
    scene.pts2d = scene.pts2d.copy()
    scene.pts2d[bad] += rng.normal(0.0, 25.0, (int(bad.sum()), 2))
    if d.get("n_pts_fix", 0) > 7:  # a fixed point that loses every observation and one that keeps a single one: n_pts_fix must shrink
        for q, spare in ((3, 0), (7, 1)):
            scene.pts2d[np.nonzero(scene.pts_ind == q)[0][spare:]] += 60.0
    scene.pairs_to_triangulate = rm_pairs(name, M)
    return scene, dict(d, reduce=False, verbose=False), dict(kw)

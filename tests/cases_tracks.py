"""
Cases of the track selection (satba.ft_ranking) shared by tools/gen_golden_tracks.py, which runs the reference on them and writes
tests/golden/track_selection.npz, and by the tests, which only read that file.

A selection case is a random set of tracks (observation lists with one keypoint scale and one reprojection error per observation);
an end-to-end case is a `synth` scene whose errors come from compute_C_reproj.  The selection is only defined where the reference's
orderings are strict, so every case must keep two gaps (`gaps`) above a threshold: the tool searches seeds until they hold and the
host test checks the stored file again.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "track_selection.npz")
PRIORITY_NAMES = ("length", "scale", "cost")
ROTATIONS = (("length", "scale", "cost"), ("scale", "cost", "length"), ("cost", "length", "scale"))

# name: (n_cam, n_pts, K, priority, generator options)
SELECTION_CASES = {
    "c8_lsc": (8, 300, 5, ROTATIONS[0], {}),
    "c8_scl": (8, 300, 5, ROTATIONS[1], {}),
    "c8_cls": (8, 300, 5, ROTATIONS[2], {}),
    "c16_k60": (16, 1000, 60, ROTATIONS[0], {}),
    "c7_exhaust": (7, 30, 60, ROTATIONS[0], {}),
    "c70_long": (70, 600, 4, ROTATIONS[0], {"max_len": 35}),
    # cameras 0-4 and 5-9 share no track, camera 10 has no observation
    "c11_split": (11, 200, 6, ROTATIONS[0], {"groups": ((0, 5), (5, 10))}),
}
SELECTION_GAP = 1e-9
# name: (cam_model, n_cam, n_pts, obs_per_pt, K, synth options); the initial points are 0.3 m off and the cameras 5e-8 rad: with synth's defaults the costs
# are several pixels, exp(-cost) is ~1e-8 and no seed separates the camera weights
E2E_CASES = {
    "e2e_affine": ("affine", 8, 300, 3, 5, {"pts_noise_m": 0.3, "sigma_theta": 5e-8}),
    "e2e_rpc": ("rpc", 8, 300, 3, 5, {"pts_noise_m": 0.3, "sigma_theta": 5e-8}),
}
E2E_GAP = 1e-5
FIRST_SEED = 100


def random_tracks(n_cam, n_pts, seed, max_len=6, groups=None):
    """(pts_ind, cam_ind, scale, err): tracks of 2 .. max_len cameras drawn inside one of `groups` (camera ranges; default: all)."""
    rng = np.random.default_rng(seed)
    groups = groups or ((0, n_cam),)
    pts_ind, cam_ind = [], []
    for t in range(n_pts):
        g0, g1 = groups[rng.integers(len(groups))]
        hi = min(max_len, g1 - g0)
        n = 2 + int(rng.integers(0, hi - 1) * rng.random() ** 2)  # short tracks are the common ones
        cams = np.sort(rng.choice(np.arange(g0, g1), size=min(n, hi), replace=False))
        pts_ind.append(np.full(cams.size, t)); cam_ind.append(cams)
    pts_ind, cam_ind = np.concatenate(pts_ind), np.concatenate(cam_ind)
    scale = rng.uniform(1.0, 6.0, pts_ind.size)
    err = np.abs(rng.normal(0.0, 0.6, pts_ind.size)) * (1.0 + 0.5 * rng.random(n_cam))[cam_ind]
    return pts_ind, cam_ind, scale, err


def dense(pts_ind, cam_ind, n_cam, n_pts, values=None):
    """(n_cam, n_pts) matrix of one value per observation, NaN elsewhere; values None: the (2 n_cam, n_pts) matrix C of ones."""
    if values is None:
        C = np.full((2 * n_cam, n_pts), np.nan)
        C[2 * cam_ind, pts_ind] = 1.0
        C[2 * cam_ind + 1, pts_ind] = 1.0
        return C
    M = np.full((n_cam, n_pts), np.nan)
    M[cam_ind, pts_ind] = values
    return M


def priority_codes(priority):
    return np.array([PRIORITY_NAMES.index(n) for n in priority], dtype=np.int32)


def numpy_keys(pts_ind, cam_ind, scale, err, n_cam, n_pts):
    """The three keys as ft_ranking.order_tracks forms them (ref:bundle_adjust/feature_tracks/ft_ranking.py:145-147)."""
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        length = np.bincount(pts_ind, minlength=n_pts).astype(np.int32)
        ks = np.round(np.nanmean(dense(pts_ind, cam_ind, n_cam, n_pts, scale), axis=0), 2).astype(np.float64)
        kc = np.nanmean(dense(pts_ind, cam_ind, n_cam, n_pts, err), axis=0).astype(np.float64)
    return length, ks, kc


def gaps(pts_ind, cam_ind, scale, err, n_cam, n_pts, priority, rank, tree_of, weights):
    """
    (weight gap, cost gap) of a recorded selection.
    weight gap: in every tree that ran, the smallest difference between the weights of two cameras that both see a live track.
    cost gap: the smallest difference between the cost keys of two tracks that are neighbours in the ranking and agree in every key
    the priority puts before the cost (for the default priority: equal length and scale).
    """
    length, ks, kc = numpy_keys(pts_ind, cam_ind, scale, err, n_cam, n_pts)
    keys = {"length": length.astype(np.float64), "scale": ks, "cost": kc}
    before = list(priority)[: list(priority).index("cost")]
    order = np.argsort(rank)
    same = np.ones(n_pts - 1, dtype=bool)
    for name in before:
        same &= keys[name][order][1:] == keys[name][order][:-1]
    d = np.abs(np.diff(kc[order]))[same]
    cost_gap = d.min() if d.size else np.inf
    w_gap = np.inf
    for k in range(weights.shape[0]):
        live = (tree_of < 0) | (tree_of >= k)
        cams = np.unique(cam_ind[live[pts_ind]])
        if cams.size > 1:
            w_gap = min(w_gap, np.diff(np.sort(weights[k][cams])).min())
    return w_gap, cost_gap


def load():
    return np.load(GOLDEN)

"""
Cases of the track construction (satba.ft_utils) shared by tools/gen_golden_ft.py, which runs the reference on them and writes
tests/golden/feature_tracks.npz, and by the tests, which only read that file.

A case is a set of keypoints (x, y, scale per keypoint, images of different sizes), match rows (kp_i, kp_j, im_i, im_j) with
im_i < im_j, and a list of camera pairs good for triangulation.  `rule` restates in numpy what the device computes (DESIGN.md
section 4j): the host test ties it to the reference's matrices, the GPU tests compare the device with it where no golden is stored.
Columns of two results are brought into one order by `canonical`.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "feature_tracks.npz")
SMALL_CASES = ["small{:02d}".format(i) for i in range(12)]
SCENE8 = ("scene8", dict(n_img=8, n_kp=3000, n_tracks=2000, seed=8))
SCENE12 = dict(n_img=12, n_kp=20000, n_tracks=17600, seed=12)  # regenerated from its seed, never stored
CHAIN = "chain"
GOLDEN_CASES = SMALL_CASES + [SCENE8[0], CHAIN]
# cases whose matrix before the baseline check and the reference's surviving indices are stored too
PRE_CASES = ["small03", SCENE8[0]]


def load():
    return np.load(GOLDEN)


def _keypoints(rng, n):
    """x, y on a quarter-pixel grid and a scale on an eighth: exact in float32, and the golden file compresses."""
    kp = np.empty((n, 3), dtype=np.float32)
    kp[:, :2] = rng.integers(0, 20000, (n, 2)) / 4.0
    kp[:, 2] = rng.integers(8, 48, n) / 8.0
    return kp


def _all_pairs(n_img):
    return np.array([(i, j) for i in range(n_img) for j in range(i + 1, n_img)], dtype=np.int32).reshape(-1, 2)


def random_small(seed):
    """2-7 images of 3-39 keypoints, 1-119 matches: many tracks name several keypoints of one image."""
    rng = np.random.default_rng([seed, 41])
    n_img = int(rng.integers(2, 8))
    sizes = rng.integers(3, 40, n_img)
    kp_ofs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = int(rng.integers(1, 120))
    im = np.sort(np.stack([rng.permutation(n_img)[:2] for _ in range(n)]), axis=1)
    matches = np.stack([rng.integers(0, sizes[im[:, 0]]), rng.integers(0, sizes[im[:, 1]]), im[:, 0], im[:, 1]], axis=1).astype(np.int32)
    allp = _all_pairs(n_img)
    pairs = allp[rng.random(len(allp)) < 0.5]
    if rng.random() < 0.5:  # pairs the check must ignore: reversed, and one naming a camera that does not exist
        pairs = np.concatenate([pairs, [[n_img - 1, 0], [0, n_img]]]).astype(np.int32)
    return dict(kp=_keypoints(rng, int(kp_ofs[-1])), kp_ofs=kp_ofs, matches=matches, pairs=pairs.reshape(-1, 2).astype(np.int32))


def scene(n_img, n_kp, n_tracks, seed, false_frac=0.02, pair_frac=0.7, max_len=8, keep_pairs=0.6):
    """
    True tracks over random camera subsets (every keypoint belongs to at most one), pair_frac of each track's camera pairs matched
    (at least a spanning chain, so the track stays one component), false_frac of the rows false matches between random keypoints,
    rows shuffled.  With false matches components merge and cells get several claimants.
    """
    rng = np.random.default_rng([seed, 43])
    kp_ofs = (np.arange(n_img + 1) * n_kp).astype(np.int64)
    free = [list(rng.permutation(n_kp)) for _ in range(n_img)]
    rows = []
    for _ in range(n_tracks):
        L = int(rng.integers(2, min(n_img, max_len) + 1))
        cams = np.sort(rng.permutation(n_img)[:L])
        kps = [free[c].pop() for c in cams]
        take = rng.random((L, L)) < pair_frac
        for a in range(L):
            for b in range(a + 1, L):
                if b == a + 1 or take[a, b]:
                    rows.append((kps[a], kps[b], cams[a], cams[b]))
    n_false = int(round(false_frac * len(rows)))
    for _ in range(n_false):
        i, j = np.sort(rng.permutation(n_img)[:2])
        rows.append((rng.integers(0, n_kp), rng.integers(0, n_kp), i, j))
    matches = np.array(rows, dtype=np.int32)[rng.permutation(len(rows))]
    allp = _all_pairs(n_img)
    listed = rng.random(len(allp)) < keep_pairs
    listed[0] = True  # (0, 1): some tracks that see only the first cameras survive the check (the n_adj cases need them)
    pairs = allp[listed]
    return dict(kp=_keypoints(rng, int(kp_ofs[-1])), kp_ofs=kp_ofs, matches=matches, pairs=pairs.astype(np.int32))


def chain_and_star():
    """
    64 images x 4 keypoints.  Tracks 0-2 are paths image k -> k + 1 through all 64 images, track 3 is a star from image 0; rows
    shuffled with a fixed seed, a tenth of them listed twice; only (62, 63) and (0, 5) are good for triangulation.
    """
    rng = np.random.default_rng(64)
    n_img = 64
    rows = [(t, t, k, k + 1) for t in range(3) for k in range(n_img - 1)] + [(3, 3, 0, j) for j in range(1, n_img)]
    rows = np.array(rows, dtype=np.int32)
    rows = np.concatenate([rows, rows[rng.permutation(len(rows))[: len(rows) // 10]]])
    return dict(kp=_keypoints(rng, 4 * n_img), kp_ofs=(np.arange(n_img + 1) * 4).astype(np.int64), matches=rows[rng.permutation(len(rows))],
                pairs=np.array([[62, 63], [0, 5]], dtype=np.int32))


def make(name):
    if name in SMALL_CASES:
        return random_small(SMALL_CASES.index(name))
    if name == SCENE8[0]:
        return scene(**SCENE8[1])
    if name == CHAIN:
        return chain_and_star()
    raise KeyError(name)


def from_golden(g, name):
    return {k: g[name + "_" + k] for k in ("kp", "kp_ofs", "matches", "pairs")}


# ---------------------------------------------------------------------------------------------------------------- the rule
def has_pair(pts_ind, cam_ind, n_cam, n_pts, pairs):
    """(n_pts,) bool: the track holds both cameras of a listed pair (i, j) with i < j < n_cam."""
    seen = np.zeros((n_cam, n_pts), dtype=bool)
    seen[cam_ind, pts_ind] = True
    keep = np.zeros(n_pts, dtype=bool)
    for i, j in np.asarray(pairs).reshape(-1, 2):
        if 0 <= i < j < n_cam:
            keep |= seen[i] & seen[j]
    return keep


def rule(kp, kp_ofs, matches, pairs, n_adj=0, baseline=True):
    """
    DESIGN.md section 4j in numpy.  Returns a dict: pts_ind, cam_ind, kp_id (observation lists, track-major, cameras ascending),
    pts2d (float64), scale (float64), n_pts, n_pts_fix, n_components, n_conflicts.
    """
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    kp_ofs = np.asarray(kp_ofs, dtype=np.int64)
    m = np.asarray(matches, dtype=np.int64).reshape(-1, 4)
    n_cam, n_kp, n = kp_ofs.size - 1, int(kp_ofs[-1]), m.shape[0]
    a, b = kp_ofs[m[:, 2]] + m[:, 0], kp_ofs[m[:, 3]] + m[:, 1]                 # 1. global ids
    _, comp = connected_components(coo_matrix((np.ones(n), (a, b)), shape=(n_kp, n_kp)), directed=False)
    size = np.bincount(comp)                                                  # 2. components of at least 2
    first = np.full(size.size, n_kp, dtype=np.int64)
    np.minimum.at(first, comp, np.arange(n_kp))
    valid = np.nonzero(size >= 2)[0]
    valid = valid[np.argsort(first[valid])]                                   # 5. ascending smallest id
    track_of = np.full(size.size, -1, dtype=np.int64)
    track_of[valid] = np.arange(valid.size)
    wkey = np.zeros(n_kp, dtype=np.int64)                                     # 3. the last write wins
    np.maximum.at(wkey, a, np.arange(n) + 1)
    np.maximum.at(wkey, b, n + np.arange(n) + 1)
    ids = np.nonzero(wkey)[0]
    cell = track_of[comp[ids]] * n_cam + (np.searchsorted(kp_ofs, ids, side="right") - 1)
    order = np.lexsort((wkey[ids], cell))
    cell, ids = cell[order], ids[order]
    last = np.r_[cell[1:] != cell[:-1], True] if cell.size else np.zeros(0, dtype=bool)
    head = np.r_[True, cell[1:] != cell[:-1]] if cell.size else np.zeros(0, dtype=bool)
    n_conflicts = int(np.sum(~(head & last) & last))
    cell, ids = cell[last], ids[last]
    pts_ind, cam_ind = cell // n_cam, cell % n_cam
    n_pts = valid.size
    keep = has_pair(pts_ind, cam_ind, n_cam, n_pts, pairs) if baseline else np.ones(n_pts, dtype=bool)  # 4.
    fixed = np.ones(n_pts, dtype=bool) if n_adj > 0 else np.zeros(n_pts, dtype=bool)
    if n_adj > 0:
        fixed[pts_ind[cam_ind >= n_adj]] = False
    new = np.full(n_pts, -1, dtype=np.int64)
    sel = np.concatenate([np.nonzero(keep & fixed)[0], np.nonzero(keep & ~fixed)[0]])
    new[sel] = np.arange(sel.size)
    o = np.nonzero(new[pts_ind] >= 0)[0]
    o = o[np.argsort(new[pts_ind[o]], kind="stable")]
    kp = np.asarray(kp)
    return dict(pts_ind=new[pts_ind[o]], cam_ind=cam_ind[o], kp_id=ids[o] - kp_ofs[cam_ind[o]], pts2d=kp[ids[o], :2].astype(np.float64),
                scale=kp[ids[o], 2].astype(np.float64), n_pts=int(sel.size), n_pts_fix=int(np.sum(keep & fixed)), n_components=int(n_pts),
                n_conflicts=n_conflicts)


def dense(pts_ind, cam_ind, pts2d, kp_id, n_cam, n_pts):
    """The reference's (C, C_v2) of observation lists."""
    C = np.full((2 * n_cam, n_pts), np.nan)
    C_v2 = np.full((n_cam, n_pts), np.nan)
    C[2 * cam_ind, pts_ind] = pts2d[:, 0]
    C[2 * cam_ind + 1, pts_ind] = pts2d[:, 1]
    C_v2[cam_ind, pts_ind] = kp_id
    return C, C_v2


def canonical(C, C_v2):
    """Both matrices with their columns in one order: np.lexsort over the rows of C_v2, NaN as -1."""
    order = np.lexsort(np.where(np.isnan(C_v2), -1.0, C_v2))
    return C[:, order], C_v2[:, order]


def same(Ca, Va, Cb, Vb):
    Ca, Va = canonical(Ca, Va)
    Cb, Vb = canonical(Cb, Vb)
    return Ca.shape == Cb.shape and np.array_equal(Ca, Cb, equal_nan=True) and np.array_equal(Va, Vb, equal_nan=True)

"""
Golden vectors of the track selection (satba.ft_ranking) -- runs ONLY where the reference is mounted, like tools/gen_golden.py,
whose reference import it reuses.  Writes tests/golden/track_selection.npz (numeric arrays only).

Per case of tests/cases_tracks.py: the observation lists with their scale and err, the reference's ranking, its sorted selection,
the tree that took every track and the weights every tree started from (recorded by wrapping the reference's
get_tracks_current_tree, not by restating its loop) and its connectivity matrix at min_matches 0 and 10.  The selection is only
defined where the reference's orderings are strict: seeds are searched from cases_tracks.FIRST_SEED until both gaps of
cases_tracks.gaps hold, and the gaps found are printed.

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_tracks.py
"""
import importlib
import os
import sys
import warnings

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_golden as G  # noqa: E402  (imports the reference)
import cases_tracks as CT  # noqa: E402

R = importlib.import_module("bundle_adjust.feature_tracks.ft_ranking")
synth = G.synth


def run_reference(pts_ind, cam_ind, scale, err, n_cam, n_pts, K, priority):
    """The reference's select_best_tracks on the dense matrices, with every tree's weights and track set recorded."""
    C = CT.dense(pts_ind, cam_ind, n_cam, n_pts)
    C_scale = CT.dense(pts_ind, cam_ind, n_cam, n_pts, scale)
    C_reproj = CT.dense(pts_ind, cam_ind, n_cam, n_pts, err)
    trees, weights = [], []
    inner = R.get_tracks_current_tree

    def recorder(A, V, cam_weights, cam_indices_per_track, inverted_track_list):
        Sk = inner(A, V, cam_weights, cam_indices_per_track, inverted_track_list)
        weights.append(np.array(cam_weights, dtype=np.float64))
        trees.append(sorted(int(t) for t in Sk))
        return Sk

    R.get_tracks_current_tree = recorder
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            S = R.select_best_tracks(C, C_scale, C_reproj, K=K, priority=list(priority))
            ranked = R.order_tracks(C, C_scale, C_reproj, priority=list(priority))
    finally:
        R.get_tracks_current_tree = inner
    rank = np.zeros(n_pts, dtype=np.int64)
    for t, r in ranked.items():
        rank[int(t)] = int(r)
    tree_of = np.full(n_pts, -1, dtype=np.int32)
    for k, Sk in enumerate(trees):
        assert np.all(tree_of[Sk] == -1)
        tree_of[Sk] = k
    S = np.sort(np.asarray(S, dtype=np.int64))
    assert np.array_equal(S, np.nonzero(tree_of >= 0)[0])
    n_trees = sum(1 for Sk in trees if Sk)
    assert all(Sk for Sk in trees[:n_trees]) and not any(trees[n_trees:])  # the empty trees come last
    out = dict(pts_ind=pts_ind.astype(np.int64), cam_ind=cam_ind.astype(np.int64), scale=scale, err=err, n_cam=np.int64(n_cam),
               n_pts=np.int64(n_pts), K=np.int64(K), priority=CT.priority_codes(priority), rank=rank, S=S, tree_of=tree_of,
               n_trees=np.int64(n_trees), weights=np.array(weights).reshape(len(weights), n_cam),
               A0=R.build_connectivity_matrix(C, min_matches=0).astype(np.int32),
               A10=R.build_connectivity_matrix(C, min_matches=10).astype(np.int32))
    return out, CT.gaps(pts_ind, cam_ind, scale, err, n_cam, n_pts, priority, rank, tree_of, out["weights"])


def main():
    arrays = {}
    for name, (n_cam, n_pts, K, priority, opts) in CT.SELECTION_CASES.items():
        for seed in range(CT.FIRST_SEED, CT.FIRST_SEED + 200):
            out, (w_gap, c_gap) = run_reference(*CT.random_tracks(n_cam, n_pts, seed, **opts), n_cam, n_pts, K, priority)
            print("{} seed {}: weight gap {:.3e}, cost gap {:.3e}, {} tracks in {} trees".format(name, seed, w_gap, c_gap, out["S"].size,
                                                                                              int(out["n_trees"])), flush=True)
            if min(w_gap, c_gap) >= CT.SELECTION_GAP:
                break
        else:
            raise SystemExit("no seed keeps the gaps of " + name)
        out["seed"] = np.int64(seed)
        arrays.update({name + "_" + k: v for k, v in out.items()})
    for name, (model, n_cam, n_pts, opp, K, kw) in CT.E2E_CASES.items():
        for seed in range(CT.FIRST_SEED, CT.FIRST_SEED + 200):
            sc = synth.make_scene(model, n_cam, n_pts, opp, seed=seed, **kw)
            C = sc.to_dense_C()
            C_reproj = R.compute_C_reproj(C, sc.pts3d, sc.cameras, model, sc.pairs_to_triangulate, sc.camera_centers)
            assert np.array_equal(np.isnan(C_reproj), np.isnan(C[::2]))
            scale = np.random.default_rng([seed, 5]).uniform(1.0, 6.0, sc.pts_ind.size)
            err = C_reproj[sc.cam_ind, sc.pts_ind]
            out, (w_gap, c_gap) = run_reference(sc.pts_ind, sc.cam_ind, scale, err, n_cam, n_pts, K, CT.ROTATIONS[0])
            print("{} seed {}: weight gap {:.3e}, cost gap {:.3e}, {} tracks in {} trees".format(name, seed, w_gap, c_gap, out["S"].size,
                                                                                              int(out["n_trees"])), flush=True)
            if min(w_gap, c_gap) >= CT.E2E_GAP:
                break
        else:
            raise SystemExit("no seed keeps the gaps of " + name)
        out["seed"] = np.int64(seed)
        arrays.update({name + "_" + k: v for k, v in out.items()})
    for k, v in arrays.items():
        assert np.asarray(v).dtype.kind in "iuf", k
    G.save("track_selection", **arrays)


if __name__ == "__main__":
    main()

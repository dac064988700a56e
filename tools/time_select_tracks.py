"""
Times of the track selection (satba.ft_ranking.select_best_tracks_from_observations, K = 60) at the two `synth` visibility shapes the
benchmarks use, 50 cameras x 100 000 tracks and 200 cameras x 1 000 000 tracks (10 observations per track), and of the reference's
select_best_tracks on this machine's CPU at the largest shape of a ladder it finishes within a minute.

    python tools/time_select_tracks.py device       # needs a GPU; writes / updates profiles/select_tracks.json
    python tools/time_select_tracks.py reference    # needs the reference mounted (tools/gen_golden.py); no GPU
    (a second argument names another output file)

Each mode fills its own part of the file and keeps the other.  Keypoint scales are uniform in [1, 6], errors |N(0, 0.6)| pixels:
the selection's cost depends on the lists, not on how the errors were produced.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sat-bundleadjust_amd"))
OUT = os.path.join(ROOT, "profiles", "select_tracks.json")
K = 60


def lists(n_cam, n_pts, opp, seed=1):
    from satba import synth

    rng = np.random.default_rng(seed)
    pts_ind, cam_ind = synth._visibility(rng, n_cam, n_pts, opp)
    return pts_ind, cam_ind, rng.uniform(1.0, 6.0, pts_ind.size), np.abs(rng.normal(0.0, 0.6, pts_ind.size))


def device():
    from satba import ft_ranking

    rows = []
    for n_cam, n_pts in ((50, 100000), (200, 1000000)):
        pts_ind, cam_ind, scale, err = lists(n_cam, n_pts, 10)
        best = None
        for rep in range(3):  # the first call also loads the code object
            t0 = time.perf_counter()
            S, info = ft_ranking.select_best_tracks_from_observations(pts_ind, cam_ind, scale, err, n_cam, n_pts, K=K, return_info=True)
            wall = time.perf_counter() - t0
            if best is None or wall < best["wall_s"]:
                best = {"n_cam": n_cam, "n_tracks": n_pts, "n_obs": int(pts_ind.size), "K": K, "wall_s": wall,
                        "device_ms": info["kernel_ms"], "n_selected": int(S.size), "n_trees": info["n_trees"]}
        print(best, flush=True)
        rows.append(best)
    return rows


def reference():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import importlib
    import warnings

    import gen_golden  # noqa: F401  (imports the reference)
    import cases_tracks as CT

    R = importlib.import_module("bundle_adjust.feature_tracks.ft_ranking")
    rows = []
    for n_cam, n_pts in ((20, 2000), (50, 5000), (50, 20000), (50, 100000)):
        pts_ind, cam_ind, scale, err = lists(n_cam, n_pts, 10)
        C, Cs, Cr = (CT.dense(pts_ind, cam_ind, n_cam, n_pts, v) for v in (None, scale, err))
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            S = R.select_best_tracks(C, Cs, Cr, K=K)
        wall = time.perf_counter() - t0
        rows.append({"n_cam": n_cam, "n_tracks": n_pts, "n_obs": int(pts_ind.size), "K": K, "wall_s": wall, "n_selected": int(len(S))})
        print(rows[-1], flush=True)
        if wall * (4 if n_pts < 20000 else 5) > 60.0:  # the next rung would not finish within a minute
            break
    return rows


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "device"
    if len(sys.argv) > 2:
        OUT = sys.argv[2]
    out = json.load(open(OUT)) if os.path.exists(OUT) else {}
    out[mode] = device() if mode == "device" else reference()
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", OUT)

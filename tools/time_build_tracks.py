"""
Times of the track construction (satba.ft_utils.feature_tracks_from_matches) and of the reference's
feature_tracks_from_pairwise_matches on this machine's CPU, on synthetic matches.

    python tools/time_build_tracks.py device       # needs a GPU; writes / updates profiles/build_tracks.json
    python tools/time_build_tracks.py reference    # needs the reference mounted (tools/gen_golden_ft.py); no GPU
    python tools/time_build_tracks.py one 200      # one device call at the shape of 200 cameras, for a profiler
    (device / reference: a second argument names another output file)

Each mode fills its own part of the file and keeps the other.  Shapes: the two scenes of tests/cases_ft.py (8 x 3 000 and
12 x 20 000 keypoints), and two `large` scenes, 50 cameras x 100 000 tracks and 200 cameras x 60 000 keypoints x 1 000 000 tracks with
about 10 observations per track.  A large scene takes its tracks from synth's visibility, gives every observation its own keypoint,
matches every observation with its predecessor in the track and, with probability 1/2, with one more earlier observation, adds 2 %
false matches between random keypoints and shuffles the rows.  The device times are the median of 5 calls after one warm-up:
`kernel_ms` from HIP events inside the entry, `wall_s` around the whole Python call (argument checks, both copies, the fetch).
"""
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sat-bundleadjust_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "build_tracks.json")
LARGE = {50: (50, 100000, None), 200: (200, 1000000, 60000)}


def large(n_cam, n_tracks, n_kp_per_image, opp=10, seed=1):
    from satba import synth

    rng = np.random.default_rng(seed)
    pts_ind, cam_ind = synth._visibility(rng, n_cam, n_tracks, opp)  # track-major, cameras ascending
    n_obs = pts_ind.size
    per_cam = np.bincount(cam_ind, minlength=n_cam)
    size = int(per_cam.max()) if n_kp_per_image is None else int(n_kp_per_image)
    assert per_cam.max() <= size
    kp_ofs = (np.arange(n_cam + 1) * size).astype(np.int64)
    by_cam = np.argsort(cam_ind, kind="stable")
    kp_id = np.empty(n_obs, dtype=np.int64)
    kp_id[by_cam] = np.arange(n_obs) - np.concatenate([[0], np.cumsum(per_cam)])[cam_ind[by_cam]]
    start = np.concatenate([[0], np.cumsum(np.bincount(pts_ind, minlength=n_tracks))])[pts_ind]
    o = np.arange(n_obs)
    a = o[o > start]                                             # every observation but the first of its track: its predecessor
    extra = o[(o > start + 1) & (rng.random(n_obs) < 0.5)]        # and, for half of them, one more earlier observation
    prev = start[extra] + (rng.random(extra.size) * (extra - 1 - start[extra])).astype(np.int64)
    i = np.concatenate([a - 1, prev])
    j = np.concatenate([a, extra])
    rows = np.stack([kp_id[i], kp_id[j], cam_ind[i], cam_ind[j]], axis=1)
    n_false = int(0.02 * rows.shape[0])
    im = np.stack([rng.integers(0, n_cam, n_false), rng.integers(0, n_cam - 1, n_false)], axis=1)
    im[:, 1] += im[:, 1] >= im[:, 0]                             # two different images
    im.sort(axis=1)
    false = np.stack([rng.integers(0, size, n_false), rng.integers(0, size, n_false), im[:, 0], im[:, 1]], axis=1)
    matches = np.concatenate([rows, false]).astype(np.int32)[rng.permutation(rows.shape[0] + n_false)]
    kp = np.empty((n_cam * size, 3), dtype=np.float32)
    kp[:, :2] = rng.random((n_cam * size, 2), dtype=np.float32) * 5000.0
    kp[:, 2] = 1.0 + 5.0 * rng.random(n_cam * size, dtype=np.float32)
    pairs = np.array([(p, q) for p in range(n_cam) for q in range(p + 1, n_cam)], dtype=np.int32)
    pairs = pairs[rng.random(pairs.shape[0]) < 0.6]
    return dict(kp=kp, kp_ofs=kp_ofs, matches=np.ascontiguousarray(matches), pairs=pairs)


def shapes(which):
    import cases_ft as CF

    if which in ("scene8", "all"):
        yield "8 x 3000", CF.scene(**CF.SCENE8[1])
    if which in ("scene12", "all"):
        yield "12 x 20000", CF.scene(**CF.SCENE12)
    for key, args in LARGE.items():
        if which in (str(key), "all"):
            yield "{} x {} tracks".format(args[0], args[1]), large(*args)


def describe(name, case):
    return {"shape": name, "n_cam": int(case["kp_ofs"].size - 1), "n_keypoints": int(case["kp_ofs"][-1]), "n_matches": int(case["matches"].shape[0]),
            "n_pairs": int(case["pairs"].shape[0])}


def call(case):
    from satba import ft_utils

    t0 = time.perf_counter()
    out = ft_utils.feature_tracks_from_matches(case["kp"], case["kp_ofs"], case["matches"], case["pairs"], return_info=True)
    return time.perf_counter() - t0, out


def device(which="all"):
    rows = []
    for name, case in shapes(which):
        call(case)  # warm-up: the first call also loads the code object
        walls, kernels = [], []
        for _ in range(5):
            wall, out = call(case)
            walls.append(wall)
            kernels.append(out[-1]["kernel_ms"])
        row = dict(describe(name, case), n_tracks=int(out[5]), n_obs=int(out[0].size), n_components=out[-1]["n_components"],
                   n_conflicts=out[-1]["n_conflicts"], wall_s=float(np.median(walls)), kernel_ms=float(np.median(kernels)))
        print(row, flush=True)
        rows.append(row)
    return rows


def reference():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_golden_ft as GF

    rows = []
    for name, case in shapes("all"):
        n_cam, size = case["kp_ofs"].size - 1, int(np.diff(case["kp_ofs"]).max())
        if rows and (rows[-1]["wall_s"] * case["matches"].shape[0] / rows[-1]["n_matches"] > 60.0 or n_cam * size * 132 * 4 > 2 << 30):
            break  # this rung would not finish within a minute, or its stacked keypoint files would not fit
        with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
            paths = GF.keypoint_files(case, tmp)
            pairs = [tuple(int(v) for v in p) for p in case["pairs"]]
            t0 = time.perf_counter()
            C, _ = GF.R.feature_tracks_from_pairwise_matches(paths, case["matches"], pairs)
            wall = time.perf_counter() - t0
        rows.append(dict(describe(name, case), n_tracks=int(C.shape[1]), wall_s=wall))
        print(rows[-1], flush=True)
    return rows


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "device"
    if mode == "one":
        name, case = next(shapes(sys.argv[2]))
        call(case)
        print(name, call(case)[0], "s")
        sys.exit(0)
    if len(sys.argv) > 2:
        OUT = sys.argv[2]
    out = json.load(open(OUT)) if os.path.exists(OUT) else {}
    out[mode] = device() if mode == "device" else reference()
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", OUT)

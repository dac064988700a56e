"""
Times of the windowed matching (satba.ft_match.match_pairs_window) on synthetic keypoints, beside the brute-force device path that
could serve the same method (match_pairs without gate under the absolute threshold, every n_i x n_j distance on the matrix cores).

    python tools/time_window.py device        # needs a GPU; writes profiles/ft_window.json (a second argument names another file)
    python tools/time_window.py one sparse    # one device call (sparse | dense), for a profiler

Shapes: one pair of 60 000 x 60 000 keypoints (FT_kp_max), all inside the box, scattered over a square whose side puts about 30
("sparse": 2 683 m) or about 1 000 ("dense": 465 m) keypoints of the second image into a 30 m window; the second image sees the
first one's scene points 3 m away with noise on the descriptors.  Nothing is read from disk.  `kernel_ms` from HIP events inside
the entries (median of 5 calls after one warm-up), `wall_s` around the Python call with both copies.  `quotient` = brute force /
window: above 1 the window path is the faster one.  The brute-force path returns the global nearest, not the nearest inside the
window: `same_matches` says how many of its matches the window path shares on these inputs.

The "lanes_per_query" part of the file holds the same rows from builds of the library with another WN_LANES (csrc/satba_window.h):
    make -C sat-bundleadjust_amd/csrc OUT=/tmp/lanes64/libsatba_hip.so EXTRA=-DWN_LANES=64
    SATBA_LIB=/tmp/lanes64/libsatba_hip.so python tools/time_window.py device /tmp/lanes64.json
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sat-bundleadjust_amd"))
OUT = os.path.join(ROOT, "profiles", "ft_window.json")
N_KP, RADIUS, THR = 60000, 30.0, 250.0
SIDES = {"sparse": 2683.0, "dense": 465.0}
EVERYWHERE = (-np.inf, np.inf, -np.inf, np.inf)


def images(side, n_kp=N_KP, seed=1):
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0.0, side, (n_kp, 2)) + np.array([500000.0, 4600000.0])
    desc = rng.integers(0, 256, (n_kp, 128)) * (rng.random((n_kp, 128)) < 0.7)
    feats, utm = [], []
    for v in range(2):
        order = rng.permutation(n_kp)
        f = np.empty((n_kp, 132), dtype=np.float32)
        f[:, 0], f[:, 1] = rng.integers(0, 8000, n_kp) / 4.0, rng.integers(0, 8000, n_kp) / 4.0
        f[:, 2], f[:, 3] = 1.0, 0.0
        f[:, 4:] = np.clip(desc[order] + rng.integers(-6, 7, (n_kp, 128)), 0, 255)
        feats.append(f)
        utm.append(pts[order] + v * np.array([3.0, -2.0]) + 0.5 * rng.standard_normal((n_kp, 2)))
    return feats, utm


def call(which, feats, utm):
    from satba import ft_match

    t0 = time.perf_counter()
    if which == "window":
        out = ft_match.match_pairs_window([(0, 1)], feats, utm, [EVERYWHERE], radius=RADIUS, thr=THR, return_info=True)
    else:
        out = ft_match.match_pairs([(0, 1)], feats, utm, [EVERYWHERE], F=None, thr=THR, relative=False, return_info=True)
    return time.perf_counter() - t0, out


def device():
    rows = []
    for shape, side in SIDES.items():
        feats, utm = images(side)
        row = {"shape": "1 pair {} x {}, {} m square, radius {} m".format(N_KP, N_KP, side, RADIUS), "name": shape}
        outs = {}
        for which in ("window", "brute_force"):
            call(which, feats, utm)  # warm-up: the first call also loads the code object
            walls, kernels = [], []
            for _ in range(5):
                wall, out = call(which, feats, utm)
                walls.append(wall)
                kernels.append(out[3]["kernel_ms"])
            outs[which] = out
            row[which] = {"kernel_ms": float(np.median(kernels)), "kernel_ms_all": [float(k) for k in kernels], "wall_s": float(np.median(walls)),
                          "path": out[3]["path"], "n_matches": int(out[0][-1])}
        info = outs["window"][3]
        row["candidates_per_query"] = info["n_candidates"] / float(N_KP)
        row["quotient"] = row["brute_force"]["kernel_ms"] / row["window"]["kernel_ms"]
        a = set(zip(outs["window"][1].tolist(), outs["window"][2].tolist()))
        b = set(zip(outs["brute_force"][1].tolist(), outs["brute_force"][2].tolist()))
        row["same_matches"] = len(a & b)
        print(row, flush=True)
        rows.append(row)
    return rows


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "device"
    if mode == "one":
        feats, utm = images(SIDES[sys.argv[2]])
        call("window", feats, utm)
        wall, out = call("window", feats, utm)
        print(sys.argv[2], wall, "s", out[3])
        sys.exit(0)
    if len(sys.argv) > 2:
        OUT = sys.argv[2]
    out = json.load(open(OUT)) if os.path.exists(OUT) else {}
    out["device"] = device()  # the "lanes_per_query" part is kept
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", OUT)

"""
Times of the pairwise matching (satba.ft_match.match_pairs) on synthetic keypoints.

    python tools/time_match.py device        # needs a GPU; writes / updates the "device" part of profiles/ft_match.json
    python tools/time_match.py one pair      # one device call (pair | scene), for a profiler
    (device: a second argument names another output file)

The "reference" part of the file -- single-thread seconds of the reference's `matching` at 5 000 x 5 000 on a CPU host -- is
written by tools/gen_golden_match.py where the reference is mounted; each tool keeps the other's part.

Shapes: one pair of 60 000 x 60 000 keypoints (FT_kp_max, every keypoint inside the box), gated (epi_thr 20 on rows up to 2 000: a
few percent of the candidates pass) and ungated; a scene of 50 images and 200 pairs with 20 000 selected keypoints per side, gated.
Both paths: int8 (matrix cores) and float32 (SATBA_MATCH_FLOAT=1) -- the float path only at the sizes it finishes in seconds.
`kernel_ms` from HIP events inside the entry (median of 3 calls after one warm-up), `wall_s` around the Python call with both
copies; `int8_ops_per_s` = 2 * 128 * queries * candidates / kernel time, beside the matrix-core peak for int8 (2 x the ~2.5 PFLOP/s
dense BF16 of the MI355X).
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sat-bundleadjust_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "profiles", "ft_match.json")
INT8_PEAK = 5.0e15
BOX = (0.0, 1000.0, 0.0, 1000.0)


def images(n_img, n_kp, seed=1):
    rng = np.random.default_rng(seed)
    feats, utm = [], []
    for _ in range(n_img):
        f = np.empty((n_kp, 132), dtype=np.float32)
        f[:, 0], f[:, 1] = rng.integers(0, 8000, n_kp) / 4.0, rng.integers(0, 8000, n_kp) / 4.0
        f[:, 2], f[:, 3] = 1.0, 0.0
        f[:, 4:] = rng.integers(0, 256, (n_kp, 128), dtype=np.uint8)
        feats.append(f)
        utm.append(rng.uniform(1.0, 999.0, (n_kp, 2)))
    return feats, utm


def shapes(which):
    import cases_match as CM

    if which in ("pair", "all"):
        feats, utm = images(2, 60000)
        yield "1 pair 60000 x 60000, ungated", feats, utm, [(0, 1)], None, True
        yield "1 pair 60000 x 60000, gated", feats, utm, [(0, 1)], [CM.fundamental(1)], True
    if which in ("scene", "all"):
        feats, utm = images(50, 20000)
        rng = np.random.default_rng(2)
        allp = [(i, j) for i in range(50) for j in range(i + 1, 50)]
        pairs = [allp[k] for k in np.sort(rng.permutation(len(allp))[:200])]
        yield "50 images, 200 pairs, 20000 x 20000 each, gated", feats, utm, pairs, [CM.fundamental(k) for k in range(200)], False


def call(feats, utm, pairs, F):
    from satba import ft_match

    t0 = time.perf_counter()
    out = ft_match.match_pairs(pairs, feats, utm, [BOX] * len(pairs), F=F, thr=0.6, return_info=True)
    return time.perf_counter() - t0, out


def device(which="all"):
    rows = []
    for name, feats, utm, pairs, F, both in shapes(which):
        work = float(sum(feats[i].shape[0] * feats[j].shape[0] for i, j in pairs))
        for path in (("int8", "float32") if both else ("int8",)):
            os.environ.pop("SATBA_MATCH_FLOAT", None)
            if path == "float32":
                os.environ["SATBA_MATCH_FLOAT"] = "1"
            call(feats, utm, pairs, F)  # warm-up: the first call also loads the code object
            walls, kernels = [], []
            for _ in range(3):
                wall, out = call(feats, utm, pairs, F)
                walls.append(wall)
                kernels.append(out[3]["kernel_ms"])
            assert out[3]["path"] == path
            ms = float(np.median(kernels))
            row = {"shape": name, "path": path, "n_pairs": len(pairs), "n_selected": out[3]["n_selected"], "n_matches": int(out[0][-1]),
                   "kernel_ms": ms, "wall_s": float(np.median(walls)), "int8_ops_per_s": 2.0 * 128 * work / (ms * 1e-3), "int8_peak_ops_per_s": INT8_PEAK}
            row["fraction_of_peak"] = row["int8_ops_per_s"] / INT8_PEAK
            print(row, flush=True)
            rows.append(row)
        os.environ.pop("SATBA_MATCH_FLOAT", None)
    return rows


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "device"
    if mode == "one":
        name, feats, utm, pairs, F, _ = next(shapes(sys.argv[2]))
        call(feats, utm, pairs, F)
        print(name, call(feats, utm, pairs, F)[0], "s")
        sys.exit(0)
    if len(sys.argv) > 2:
        OUT = sys.argv[2]
    out = json.load(open(OUT)) if os.path.exists(OUT) else {}
    out["device"] = device()
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", OUT)

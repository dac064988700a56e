"""
Times of the affine fundamental matrices from RPCs (satba.rpc_utils.fundamental_matrices) for 1 pair, 200 pairs and 19 900 pairs
(all pairs of 200 images), n = 5.

    python tools/time_fundamental.py [output.json]     # needs a GPU; writes profiles/ft_fundamental.json by default

The 200 images are the two shipped RPCs cycled, every image with a crop size of its own; pairs of two images with the same RPC are
degenerate (flagged, NaN) and cost what any pair costs, so they stay in the batch.  Per workload: the kernel time from the
library's HIP events and the wall time around the whole Python call (tables, one launch, the copy back, the list of matrices),
medians of 3 calls after one warm-up.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (os.path.join(ROOT, "sat-bundleadjust_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, path)
OUT = os.path.join(ROOT, "profiles", "ft_fundamental.json")
N_IMAGES = 200


def main(out_path):
    import cases_camapprox as CC
    from satba import rpc_utils

    base = [CC.rpc(0), CC.rpc(1)]
    rpcs = [base[k % 2] for k in range(N_IMAGES)]
    offsets = [{"col0": 0.0, "row0": 0.0, "width": 3200.0 - 11.0 * (k % 97), "height": 1350.0 - 5.0 * (k % 89)} for k in range(N_IMAGES)]
    all_pairs = [(i, j) for i in range(N_IMAGES) for j in range(i + 1, N_IMAGES)]
    rows = {"n": 5, "n_images": N_IMAGES}
    for name, pairs in (("1_pair", all_pairs[:1]), ("200_pairs", all_pairs[:200]), ("19900_pairs", all_pairs)):
        rpc_utils.fundamental_matrices(pairs, rpcs, offsets, return_info=True)  # warm-up: the first call also loads the code object
        walls, kernels = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            Fs, info = rpc_utils.fundamental_matrices(pairs, rpcs, offsets, return_info=True)
            walls.append(time.perf_counter() - t0)
            kernels.append(info["kernel_ms"])
        healthy = ~info["degenerate"]
        assert len(Fs) == len(pairs) and all(np.isfinite(Fs[k]).all() for k in np.flatnonzero(healthy))
        assert np.array_equal(info["degenerate"], np.array([(i - j) % 2 == 0 for i, j in pairs]))
        rows[name] = {"pairs": len(pairs), "degenerate": int((~healthy).sum()), "kernel_ms": float(np.median(kernels)),
                      "python_call_ms": 1e3 * float(np.median(walls))}
    print(json.dumps(rows), flush=True)
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)

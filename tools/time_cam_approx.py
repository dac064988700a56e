"""
Times of the camera approximation (satba.cam_utils.approx_cameras) for 200 cameras, both models, against the numpy restatement of
tests/cases_camapprox.py on this machine's CPU.

    python tools/time_cam_approx.py [output.json]     # needs a GPU; writes profiles/cam_approx.json by default

The 200 cameras are the two shipped RPCs cycled with different crops and expansion points (cases_camapprox.batch).  Device: the
median wall time of 5 calls after one warm-up, around the whole Python call (tables, one launch, the copy back).  Host: the
restatement (`resect`: moments, 12 x 12, Jacobi in Python; `affine_expected`: the oracle's chained Jacobian) on the first 20
cameras, scaled to 200; the perspective figure leaves the mesh out (it is the device's), so it is the resection alone.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (os.path.join(ROOT, "sat-bundleadjust_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, path)
OUT = os.path.join(ROOT, "profiles", "cam_approx.json")
N_CAM, N_HOST = 200, 20


def main(out_path):
    import cases_camapprox as CC
    from satba import cam_utils

    rpcs, offsets, centers = CC.batch(N_CAM)
    rows = {"n_cam": N_CAM}
    for model, kw in (("affine", {"center": centers}), ("perspective", {})):
        cam_utils.approx_cameras(rpcs, offsets, model, **kw)  # warm-up: the first call also loads the code object
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            cams = cam_utils.approx_cameras(rpcs, offsets, model, **kw)
            walls.append(time.perf_counter() - t0)
        assert len(cams) == N_CAM and all(np.isfinite(c).all() for c in cams)
        rows[model + "_device_wall_s"] = float(np.median(walls))
    cr, rr, ar = cam_utils._perspective_ranges(rpcs[:N_HOST], offsets[:N_HOST])
    X, x, _ = cam_utils.rpc_point_mesh(rpcs[:N_HOST], cr, rr, ar)
    t0 = time.perf_counter()
    for k in range(N_HOST):
        CC.resect(X[k], x[k])
    rows["perspective_host_restatement_s"] = (time.perf_counter() - t0) * N_CAM / N_HOST
    t0 = time.perf_counter()
    for k in range(N_HOST):
        CC.affine_expected(rpcs[k], centers[k], offsets[k]["col0"], offsets[k]["row0"])
    rows["affine_host_oracle_s"] = (time.perf_counter() - t0) * N_CAM / N_HOST
    print(json.dumps(rows), flush=True)
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)

"""
Golden vectors of the RPC -> perspective camera approximation -- runs ONLY in the build container, where the reference is mounted.

Imports the reference's cam_utils in place (tools/gen_golden.py stubs the absent third-party modules) and records into
tests/golden/cam_approx.npz what its camera_matrix and approx_rpc_as_proj_matrix / perspective_rpc_approx return on the cases of
tests/cases_camapprox.py.  rpc.localization is the oracle's restatement of the reference's C localisation
(oracle.triangulate_oracle._Rpc(r, 0.1).eval_rpc).  The reference's affine route needs the `ad` package, which is absent: its
expected values are composed in tests/cases_camapprox.py instead.

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_camapprox.py
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_golden as G  # noqa: E402  (imports the reference)
import cases_camapprox as CC  # noqa: E402

RC = G.ref.cam_utils


def main():
    out = {}
    # resection cases: the stored correspondences and the reference's camera_matrix on them
    for name, (X, x, crop) in CC.resection_inputs().items():
        P = RC.camera_matrix(X, x)
        out["res_{}_X".format(name)], out["res_{}_x".format(name)], out["res_{}_P".format(name)] = X, x, P
        s = np.linalg.svd(np.asarray(_dlt_matrix(X, x)), compute_uv=False)
        h = X @ P[:, :3].T + P[:, 3]
        err = np.mean(np.linalg.norm(x - h[:, :2] / h[:, 2:3], axis=1))
        print("{:8s} n = {:4d}  smallest singular values {:.3e} {:.3e}  mean_err {:.3e} px".format(name, len(X), s[-1], s[-2], err))
    # full-route cases: only the results are stored, the inputs are the shipped RPC files
    for f, cname in CC.FULL_ROUTE:
        r, crop = CC.OracleRpc(CC.rpc(f)), CC.CROPS[cname]
        P, err = RC.perspective_rpc_approx(r, CC.offset(crop))
        P_img, err_img = RC.approx_rpc_as_proj_matrix(r, *CC.perspective_ranges(r, crop))
        assert err == err_img
        key = "full_{}_{}".format(f, cname)
        out[key + "_P"], out[key + "_Pimg"], out[key + "_err"] = P, P_img, np.float64(err)
        out[key + "_centre"] = RC.decompose_perspective_camera(P)[3]
        print("{:12s} mean_err {:.3e} px  centre {}".format(key, err, out[key + "_centre"]))
    np.savez_compressed(CC.GOLDEN, **out)
    print("wrote", CC.GOLDEN, os.path.getsize(CC.GOLDEN), "bytes")


def _dlt_matrix(X, x):
    """the reference's A of the normalised points (for the printed conditioning figures only)"""
    Xn, _ = RC.normalize_3d_points(X)
    xn, _ = RC.normalize_2d_points(x)
    Xh = np.hstack([Xn, np.ones((len(Xn), 1))])
    A = np.zeros((2 * len(Xn), 12))
    A[0::2, 4:8], A[0::2, 8:12] = -Xh, xn[:, 1:2] * Xh
    A[1::2, 0:4], A[1::2, 8:12] = Xh, -xn[:, 0:1] * Xh
    return A


if __name__ == "__main__":
    main()

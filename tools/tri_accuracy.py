"""Runs ON the GPU box: how far the device's, the oracle's and LAPACK's linear triangulations are from the exact null vector of the
DLT matrix (one-sided Jacobi in numpy.longdouble: tests/cases_tri.py, the reference of tests/test_gpu_triangulate_edges.py), in
metres, on a wide-baseline scene.   usage: python tools/tri_accuracy.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sat-bundleadjust_amd"), ROOT, os.path.join(ROOT, "tests")]
import cases_tri as CT  # noqa: E402
from oracle import triangulate_oracle as T  # noqa: E402
from satba import ft_triangulate as FT  # noqa: E402
from satba import synth  # noqa: E402

for model in ("affine", "perspective"):
    scene = synth.make_scene(model, 4, 1500, 4, seed=9)
    C = scene.to_dense_C()
    t = np.where(~np.isnan(C[0]) & ~np.isnan(C[2]))[0][:300]
    oi, oj = C[0:2, t].T, C[2:4, t].T
    P1, P2 = np.asarray(scene.cameras[0], float), np.asarray(scene.cameras[1], float)
    ex = CT.triangulate_ld(P1, P2, oi, oj).astype(np.float64)
    dev = FT.linear_triangulation_multiple_pts(P1, P2, oi, oj)
    orc = T.linear_triangulation_multiple_pts(P1, P2, oi, oj)
    lap = CT.triangulate_lapack(P1, P2, oi, oj)
    e = lambda x, y: np.linalg.norm(x - y, axis=1)
    print(model, "n", len(t), "| device - exact: median %.3g max %.3g m | oracle (Jacobi) - exact: max %.3g m | numpy.linalg.svd - exact: median %.3g max %.3g m"
          % (np.median(e(dev, ex)), e(dev, ex).max(), e(orc, ex).max(), np.median(e(lap, ex)), e(lap, ex).max()))

"""
Cases of the intrinsics' refinement (correction_params ["R", "T", "K"] with K_init="camera"), shared by
tools/gen_golden_intrinsics.py (which runs the reference on them) and the tests.

R + T + K with free points has a gauge freedom: the 12-parameter affine group (affine cameras) or the 15-parameter
projective group (perspective cameras); one frozen camera removes 8 or 11 of those.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
RTK = ["R", "T", "K"]

# name -> (model, n_cam, n_pts, obs_per_pt, seed, options, scene keywords)
FUN_CASES = {
    "affine_RTK": ("affine", 4, 60, 3, 7, {"correction_params": RTK, "n_cam_fix": 1, "n_pts_fix": 6, "ref_cam_weight": 2.5}, {}),
    "persp_RTK": ("perspective", 4, 50, 3, 7, {"correction_params": RTK, "n_cam_fix": 0}, {}),
}

# name -> (model, n_cam, n_pts, obs_per_pt, seed, options, scene keywords, losses): the reference's own least_squares from the corrected
# start under the tight3 protocol (tools/gen_golden_intrinsics.py -> solve_intrinsics.npz).  The parameter-compared cases freeze one
# camera and 8 points (in general position: uniform in a 10 km cube); GAUGE_FREE_CASES are compared on gauge-invariant outputs only.
# No perspective case: at the synthetic geometry (600 km to a 10 km scene) the focal lengths trade against the distance along the optical
# axis, and neither the reference's run (417 evaluations and restarts) nor this solver (300) reaches a stationary point to compare.
SOLVE_CASES = {
    "affine_small_RTK": ("affine", 5, 300, 4, 5, {"correction_params": RTK, "n_cam_fix": 1, "n_pts_fix": 8},
                         {"sigma_k": 1e-4}, ["linear", "soft_l1"]),
    "affine_small_RTK_free": ("affine", 5, 300, 4, 6, {"correction_params": RTK, "n_cam_fix": 0}, {"sigma_k": 1e-4}, ["linear"]),
}
GAUGE_FREE_CASES = ("affine_small_RTK_free",)


def _case(name):
    return FUN_CASES[name] if name in FUN_CASES else SOLVE_CASES[name]


def scene(name):
    from satba import synth

    model, M, N, opp, seed, _, kw = _case(name)[:7]
    return synth.make_scene(model, M, N, opp, seed=seed, **kw)


def options(name):
    return dict(_case(name)[5], K_init="camera", reduce=False, verbose=False)


def corrected_start(cam_params, pts3d, n_params):
    """The start vector of K_init="camera": [cam_params[:, :n_params] per camera | points]."""
    return np.hstack((np.asarray(cam_params)[:, :n_params].ravel(), np.asarray(pts3d, dtype=np.float64).ravel()))


def golden(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"))

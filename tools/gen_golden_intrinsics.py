"""
Golden vectors of the intrinsics' refinement (correction_params ["R", "T", "K"], K_init="camera") -- runs ONLY where the
reference is mounted, like tools/gen_golden.py, whose reference import, `ref_params` and `fd3_jacobian_blocks` it reuses.

The reference starts K from the T columns (ref:bundle_adjust/ba_params.py:163); everything else of its K machinery
(get_vars_ready_for_fun, fun) is sound.  So the reference's parameters object is built as it is, its own params_opt is stored,
and every evaluation and solve starts from the corrected vector v0 = [cam_params[:, :n_params] | pts3d].

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_intrinsics.py [fun] [solve]
"""
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_golden as G  # noqa: E402  (imports the reference)
import cases_intrinsics as CI  # noqa: E402

ref = G.ref


def golden_fun():
    for name in CI.FUN_CASES:
        sc = CI.scene(name)
        p = G.ref_params(sc, CI.options(name))
        n_c = p.n_cam * p.n_params
        v0 = CI.corrected_start(p.cam_params, p.pts3d, p.n_params)
        rng = np.random.default_rng(11)
        vs, rs = [], []
        scale = np.abs(v0[:n_c]).reshape(p.n_cam, p.n_params)
        for k in range(3):
            v = v0.copy()
            if k > 0:  # angles 1e-6, T and K 1e-6 relative, points 1 m
                dc = rng.normal(0, 1e-6, (p.n_cam, p.n_params))
                dc[:, 3:] *= np.maximum(scale[:, 3:], 1.0)
                v[:n_c] += dc.ravel()
                v[n_c:] += rng.normal(0, 1.0, v.size - n_c)
            vs.append(v.copy())
            rs.append(ref.ba_core.fun(v.copy(), p))
        Jc, Jp = G.fd3_jacobian_blocks(lambda v, p=p: ref.ba_core.fun(v.copy(), p), vs[1], p, p.n_params)
        A = ref.ba_core.build_jacobian_sparsity(p).tocsr()
        G.save("fun_" + name, v=np.array(vs), r=np.array(rs), v0=v0, params_opt=p.params_opt, cam_params=p.cam_params,
               pts_ind=p.pts_ind, cam_ind=p.cam_ind, pts2d=p.pts2d, pts2d_w=p.pts2d_w, pts3d=sc.pts3d, n_params=p.n_params,
               Jc=Jc, Jp=Jp, A_indices=A.indices, A_indptr=A.indptr, A_shape=np.array(A.shape))


def golden_solve():
    """The reference's own least_squares call (its sparsity, x_scale="jac", trf) from v0 under tools/gen_golden.py's tight3 protocol."""
    from scipy.optimize import least_squares

    out = {}
    for name, case in CI.SOLVE_CASES.items():
        sc = CI.scene(name)
        for loss in case[7]:
            p = G.ref_params(sc, CI.options(name))
            p.params_opt = CI.corrected_start(p.cam_params, p.pts3d, p.n_params)
            A = ref.ba_core.build_jacobian_sparsity(p)
            kw = dict(jac="3-point", jac_sparsity=A, x_scale="jac", method="trf", loss=loss, f_scale=1.0, args=(p,),
                      tr_options={"atol": 1e-12, "btol": 1e-12}, ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=600)
            res = least_squares(ref.ba_core.fun, p.params_opt.copy(), **kw)
            for restart in range(8):  # restarted from its own end point until it returns its start (tools/gen_golden.py: golden_tight3)
                nxt = least_squares(ref.ba_core.fun, res.x.copy(), **kw)
                if np.array_equal(nxt.x, res.x):
                    break
                nxt.nfev += res.nfev
                res = nxt
            print(name, loss, "status", res.status, "nfev", res.nfev, "cost %.12f" % res.cost, "optimality %.3e" % res.optimality, flush=True)
            key = name + "_" + loss
            out.update({"x_" + key: res.x, "fun_" + key: res.fun, "x0_" + key: p.params_opt,
                        "stats_" + key: np.array([res.cost, res.nfev, res.status, res.optimality])})
    G.save("solve_intrinsics", **out)


if __name__ == "__main__":
    which = sys.argv[1:] or ["fun", "solve"]
    if "fun" in which:
        golden_fun()
    if "solve" in which:
        golden_solve()

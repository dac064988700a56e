"""
Golden vectors of the affine fundamental matrices from RPCs -- runs ONLY in the build container, where the reference is mounted.

Imports the reference's s2p/rpc_utils.py and s2p/estimation.py in place (tools/gen_golden.py stubs the absent third-party modules;
here also bundle_adjust.s2p as a namespace package and a stub of its geographiclib, which rpc_utils imports at module level and
never uses on this path) and records into tests/golden/ft_fundamental.npz what matches_from_rpc and affine_fundamental_matrix
return on the cases of tests/cases_fundamental.py.  rpc.localization is the oracle's restatement of the reference's C localisation
(cases_camapprox.OracleRpc).  Per case: the matches (n^3, 4), F (3, 3), the singular values of the centred matches (4,), and the
four corners of the region with their partners (cases_fundamental.corner_matches: the points the metric adds to the matches).

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_fundamental.py
"""
import importlib
import os
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_golden as G  # noqa: E402, F401  (imports the reference and stubs the third-party modules)
import cases_camapprox as CC  # noqa: E402
import cases_fundamental as CF  # noqa: E402


def import_s2p():
    base = sys.modules["bundle_adjust"].__path__[0]
    pkg = types.ModuleType("bundle_adjust.s2p")
    pkg.__path__ = [os.path.join(base, "s2p")]
    sys.modules["bundle_adjust.s2p"] = pkg
    sys.modules["bundle_adjust.s2p.geographiclib"] = types.ModuleType("bundle_adjust.s2p.geographiclib")
    return importlib.import_module("bundle_adjust.s2p.rpc_utils"), importlib.import_module("bundle_adjust.s2p.estimation")


def main():
    RU, ES = import_s2p()
    out = {}
    for case in CF.CASES:
        i, j, _, n = case
        ri, rj = CC.rpc(i), CC.rpc(j)
        x, y, w, h = CF.roi(case)
        m = RU.matches_from_rpc(CF.Rpc(ri), CF.Rpc(rj), x, y, w, h, n)
        F = ES.affine_fundamental_matrix(m)
        X = m[:, [2, 3, 0, 1]]
        sv = np.linalg.svd(X - np.sum(X, axis=0) / len(X), compute_uv=False)
        k = CF.key(case)
        out[k + "_matches"], out[k + "_F"], out[k + "_sv"], out[k + "_corners"] = m, F, sv, CF.corner_matches(ri, rj, (x, y, w, h))
        print("{:18s} {:5d} matches  singular values {:.3e} {:.3e} {:.3e} {:.3e}  N {}".format(k, len(m), *sv, CF.f5(F)[:4]))
    np.savez_compressed(CF.GOLDEN, **out)
    print("wrote", CF.GOLDEN, os.path.getsize(CF.GOLDEN), "bytes")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""
Accuracy of the dense solve of the reduced camera system on every (size, family) of tests/cases_dense.py, the device beside LAPACK's
float64 Cholesky on the same M_eff, b_eff:

    python tools/dense_accuracy.py [profiles/dense_accuracy.json]

Per case: the condition number kappa_2(M_eff); forward error |z - z*|_inf / |z*|_inf, normwise backward error and factor residual
|L L^T - M|_F / |M|_F of both (the factor of k_solve_small, up to 63 unknowns, never leaves the chip: null); for the graded family also
the forward error in the variables with a unit diagonal and that matrix's condition number.  "constants": LAPACK's worst forward
error / (u kappa_2), backward error / u and factor residual / u over all cases (u = 2^-53) -- what C_FWD, C_BWD, C_FAC of
tests/cases_dense.py are rounded up from -- and the same three figures for the device.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sat-bundleadjust_amd"), ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import cases_dense as D  # noqa: E402
import test_gpu_dense as G  # noqa: E402  (the handles and the planting are the tests')


def main(out_path):
    rows = []
    worst = {who: {"fwd": 0.0, "bwd": 0.0, "fac": 0.0} for who in ("lapack", "device")}
    for n in D.SIZES:
        eng, s = G.open_engine(n)
        for family in D.SPD_FAMILIES:
            c = D.Case(family, n, s)
            flag, z = G.solve(eng, c.S_p, c.rhs)
            L = np.tril(G.read_factor(eng)) if n >= 64 else None
            z_l, L_l = D.lapack(c.M_eff, c.b_eff)
            row = {"n": n, "family": family, "route": "small" if n < 64 else "tiles+trsv_mw" if n <= 1024 else "tiles+trsv", "flag": int(flag)}
            for who, m in (("device", c.measure(z, L)), ("lapack", c.measure(z_l, L_l))):
                row["kappa"] = m["kappa"]
                row[who] = {k: m[k] for k in ("fwd", "bwd", "fac")}
                if family == "graded":
                    row["kappa_scaled"], row[who]["fwd_scaled"] = m["kappa_scaled"], m["fwd_scaled"]
                w = worst[who]
                w["fwd"], w["bwd"] = max(w["fwd"], m["fwd"] / (D.U * m["kappa"])), max(w["bwd"], m["bwd"] / D.U)
                if m["fac"] is not None:
                    w["fac"] = max(w["fac"], m["fac"] / D.U)
            rows.append(row)
            print(json.dumps(row), flush=True)
        eng.close()
    doc = {"u": D.U, "constants": {"C_fwd": worst["lapack"]["fwd"], "C_bwd": worst["lapack"]["bwd"], "C_fac": worst["lapack"]["fac"],
                                   "device_fwd": worst["device"]["fwd"], "device_bwd": worst["device"]["bwd"], "device_fac": worst["device"]["fac"]},
           "asserted": {"C_FWD": D.C_FWD, "C_BWD": D.C_BWD, "C_FAC": D.C_FAC, "margins": [D.FWD_MARGIN, D.BWD_MARGIN, D.FAC_MARGIN]},
           "cases": rows}
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["constants"]))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "dense_accuracy.json"))

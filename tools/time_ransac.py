"""
Figures of the fundamental-matrix RANSAC (satba.ft_match.ransac_fundamental) in profiles/ft_ransac.json.

    python tools/time_ransac.py [output.json]              # needs a GPU: the "times" section
    python tools/time_ransac.py --rounding [output.json]   # CPU only: the "rounding" section

times: n_trials = 1000, max_err = 0.3, scenes of tests/cases_ransac.py (40 % of the matches displaced), medians of 3 calls after one
warm-up: the kernel time from the library's HIP events (three launches) and the wall time around the whole Python call, at 200 pairs x
500 matches and at 1 pair x 5 000 matches; 200 pairs x 8 matches stands for the model kernel alone (there is next to nothing to score).
restatement_cpu_ms is the numpy restatement of tests/cases_ransac.py for one pair of 500 matches on the host: numpy, not the
reference's C (`ransac` / cv2), which is not available.

rounding: tests/cases_ransac.py measure_rounding(): the float64 restatement against its numpy.longdouble run, the figures behind the
band and the model tolerance of tests/test_gpu_ransac.py.

The section that is not measured is kept as the output file has it.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (os.path.join(ROOT, "sat-bundleadjust_amd"), os.path.join(ROOT, "tests"), ROOT):
    sys.path.insert(0, path)
OUT = os.path.join(ROOT, "profiles", "ft_ransac.json")


def rounding():
    import cases_ransac as R

    score, model, n_eval = R.measure_rounding()
    return {"what": "tests/cases_ransac.py measure_rounding(): float64 restatement against its numpy.longdouble run over every run of RUNS, on the CPU",
            "score_float64_vs_longdouble": float(score), "models_float64_vs_longdouble": float(model), "evaluations": int(n_eval), "device_factor": 8}


def times():
    import cases_ransac as R
    from satba import ft_match

    rows = {"n_trials": 1000, "max_err": 0.3}
    for name, n_pairs, m in (("200_pairs_x_500", 200, 500), ("1_pair_x_5000", 1, 5000), ("200_pairs_x_8", 200, 8)):
        parts = [R.make_scene(m, 0.4 if m > 8 else 0.125, 0.03, seed=1000 + p)[0] for p in range(n_pairs)]
        ofs, xy = np.arange(n_pairs + 1, dtype=np.int64) * m, np.concatenate(parts)
        ft_match.ransac_fundamental(ofs, xy, return_info=True)  # warm-up: the first call also loads the code object
        walls, kernels = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            mask, info = ft_match.ransac_fundamental(ofs, xy, return_info=True)
            walls.append(time.perf_counter() - t0)
            kernels.append(info["kernel_ms"])
        rows[name] = {"pairs": n_pairs, "matches_per_pair": m, "kept": int(mask.sum()), "models": int(info["best"][:, 2].sum()),
                      "kernel_ms": float(np.median(kernels)), "python_call_ms": 1e3 * float(np.median(walls))}
    xy = R.make_scene(500, 0.4, 0.03, seed=1000)[0]
    t0 = time.perf_counter()
    R.ransac_pair(xy)
    rows["restatement_cpu_ms"] = {"what": "numpy restatement (tests/cases_ransac.py) of one pair of 500 matches on the host; not the reference's C",
                                  "ms": 1e3 * (time.perf_counter() - t0)}
    return rows


def main(argv):
    only_rounding = "--rounding" in argv
    paths = [a for a in argv if not a.startswith("--")]
    out_path = paths[0] if paths else OUT
    doc = {}
    for src in (OUT, out_path):
        if os.path.exists(src):
            with open(src) as f:
                doc.update(json.load(f))
    if only_rounding:
        doc["rounding"] = rounding()
    else:
        doc["times"] = times()
    print(json.dumps(doc), flush=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1:])

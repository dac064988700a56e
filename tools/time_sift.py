"""
Times of the SIFT detection (satba.ft_s2p.keypoints_from_nparray) on smoothed-noise images of 1 000 x 1 000 and 4 000 x 4 000.

    python tools/time_sift.py device [FILE]       # needs a GPU; writes / updates the "device" part of profiles/ft_sift.json (or FILE)
    python tools/time_sift.py reference [DIR]     # needs the reference tree (default /root/reference); the "reference" part
    python tools/time_sift.py one SIZE            # one size on the device, one JSON line (what `device` starts per size)
    python tools/time_sift.py ref_one SO SIZE     # one size through a compiled reference library, one JSON line

device: per size a fresh process under its own time limit; after a warm-up call the median of 3 calls of `kernel_ms` (HIP events
inside the entry: from the seed kernel to the last kernel, three reads of counters inside) and of the wall time of the whole call
(upload, kernels, download of the rows).  If a size fails the tool stops there.  reference: the reference's library, compiled
by the tool into a temporary directory as tools/gen_golden_sift.py compiles it, with OMP_NUM_THREADS = 1 and = 16; the median of 3
calls at 1 000 x 1 000, one call at 4 000 x 4 000.  Each tool mode keeps the other's part of the file.
"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "sat-bundleadjust_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "profiles", "ft_sift.json")
SIZES = (1000, 4000)
LIMIT = {1000: 120, 4000: 400}  # seconds per child process


def image(size):
    import cases_sift as CS

    return CS.texture(size, size, 5).astype(np.float32)


def one(size):
    from satba import ft_s2p

    img = image(size)
    ft_s2p.keypoints_from_nparray(img, return_info=True)  # warm-up: the first call also loads the code object
    walls, kernels = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        rows, info = ft_s2p.keypoints_from_nparray(img, return_info=True)
        walls.append(time.perf_counter() - t0)
        kernels.append(info["kernel_ms"])
    return {"size": size, "n_keypoints": int(rows.shape[0]), "n_octaves": info["n_octaves"], "n_extrema": info["n_extrema"],
            "kernel_ms": float(np.median(kernels)), "wall_s": float(np.median(walls))}


def ref_one(so, size):
    import gen_golden_sift as G
    import ctypes

    lib = ctypes.CDLL(so)
    lib.sift.restype = ctypes.POINTER(ctypes.c_float)
    lib.delete_buffer.argtypes = [ctypes.POINTER(ctypes.c_float)]
    img = image(size)
    times = []
    for _ in range(3 if size <= 1000 else 1):
        t0 = time.perf_counter()
        rows = G.reference_rows(lib, img, 0.0133, 8)
        times.append(time.perf_counter() - t0)
    return {"size": size, "threads": int(os.environ.get("OMP_NUM_THREADS", "0")), "n_keypoints": int(rows.shape[0]), "wall_s": float(np.median(times))}


def children(argv_of, limit_of, env_of=lambda size: None):
    rows = []
    for size in SIZES:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv_of(size), capture_output=True, text=True, timeout=limit_of(size),
                               env=env_of(size))
        except subprocess.TimeoutExpired:
            print("size", size, "ran into its time limit: stopping", flush=True)
            break
        if r.returncode != 0:
            print("size", size, "failed with", r.returncode, r.stderr[-2000:], "stopping", flush=True)
            break
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(rows[-1], flush=True)
    return rows


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "device"
    if mode == "one":
        print(json.dumps(one(int(sys.argv[2]))))
        sys.exit(0)
    if mode == "ref_one":
        print(json.dumps(ref_one(sys.argv[2], int(sys.argv[3]))))
        sys.exit(0)
    out = json.load(open(OUT)) if os.path.exists(OUT) else {}
    dest = sys.argv[2] if mode == "device" and len(sys.argv) > 2 else OUT
    if mode == "device":
        out["device"] = children(lambda size: ["one", str(size)], lambda size: LIMIT[size])
    elif mode == "reference":
        import gen_golden_sift as G

        with tempfile.TemporaryDirectory() as tmp:
            G.build(sys.argv[2] if len(sys.argv) > 2 else "/root/reference", tmp, G.FLAGS)
            so = os.path.join(tmp, "libsift_ref.so")
            out["reference"] = {"flags": " ".join(G.FLAGS), "host_cpus": os.cpu_count(), "runs": []}
            for threads in (1, 16):
                env = dict(os.environ, OMP_NUM_THREADS=str(threads))
                out["reference"]["runs"] += children(lambda size: ["ref_one", so, str(size)], lambda size: 1800, lambda size: env)
    else:
        sys.exit("unknown mode " + mode)
    os.makedirs(os.path.dirname(os.path.abspath(dest)), exist_ok=True)
    with open(dest, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", dest)

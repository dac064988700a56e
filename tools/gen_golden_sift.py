#!/usr/bin/env python
"""
Writes tests/golden/ft_sift.npz: the cases of tests/cases_sift.py run through the reference's compiled SIFT library
(ref:3rdparty/sift/simd, entry `sift` of sift4ctypes.cpp) and through the float64 rule of tests/cases_sift.py.

    python tools/gen_golden_sift.py [--reference /path/to/reference] [--march-native]

The library is compiled into a temporary directory (Utilities.cpp includes png.h and tiffio.h without using them: two empty files
of those names on the include path are enough) and nothing compiled is kept.  Per case the file stores the image (uint8), the
reference's rows, the rule's staged counts and rows, the candidate table with its fragile flags, and once the flags of the build
and the spreads: the largest differences between the reference and the rule over all paired keypoints of all cases, and the
largest error of the reference's Gaussian planes (its own oversampling and blur routines, driven through a few lines of C++ written
here, against the rule's planes, relative to a plane's largest magnitude).

The generator asserts the conditions the tests lean on (every octave side >= 13, fragile share <= 2 %, the reference and the rule
name the same keypoints away from fragile candidates) and fails when one does not hold: change the seed in tests/cases_sift.py.
"""
import argparse
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
from numpy.ctypeslib import ndpointer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cases_sift as CS  # noqa: E402

FLAGS = ["-O2", "-mavx", "-ffp-contract=off", "-fpic", "-shared", "-w", "-fopenmp"]
SOURCES = ["sift4ctypes.cpp", "LibImages/LibImages.cpp", "LibSSE/LibSSE.cpp", "LibSift/KeyPoint.cpp", "LibSift/LibSift.cpp", "LibSift/Octave.cpp",
           "LibSift/ScaleSpace.cpp", "Utilities/Memory.cpp", "Utilities/Parameters.cpp", "Utilities/Time.cpp", "Utilities/Utilities.cpp"]
# the reference's own image routines behind a C interface, so that its planes can be measured (its `sift` does not return them)
DRIVER = r"""
#include "LibImages/LibImages.h"
extern "C" void planes_oversample(const float* in, size_t w, size_t h, float* out) {
    Image a(in, w, h, 1), b(2 * w, 2 * h, 1);
    a.overSample(b, 0.5f, 0, 0);
    for (size_t i = 0; i < 2 * h; ++i) for (size_t j = 0; j < 2 * w; ++j) out[i * 2 * w + j] = b.getPtr(0, i)[j];
}
extern "C" void planes_blur(const float* in, size_t w, size_t h, float sigma, float* out) {
    Image a(in, w, h, 1), b(w, h, 1);
    a.applyGaussianBlur(b, sigma, 0, 0);
    for (size_t i = 0; i < h; ++i) for (size_t j = 0; j < w; ++j) out[i * w + j] = b.getPtr(0, i)[j];
}
"""


def build(reference, tmp, flags):
    simd = os.path.join(reference, "3rdparty", "sift", "simd")
    stub = os.path.join(tmp, "stub")
    os.makedirs(stub)
    for name in ("png.h", "tiffio.h"):
        open(os.path.join(stub, name), "w").close()
    with open(os.path.join(tmp, "planes_driver.cpp"), "w") as f:
        f.write(DRIVER)
    so = os.path.join(tmp, "libsift_ref.so")
    cmd = ["g++"] + flags + ["-I", stub, "-I", simd] + [os.path.join(simd, s) for s in SOURCES] + [os.path.join(tmp, "planes_driver.cpp"), "-o", so]
    subprocess.run(cmd, check=True)
    lib = ctypes.CDLL(so)
    lib.sift.restype = ctypes.POINTER(ctypes.c_float)
    lib.delete_buffer.argtypes = [ctypes.POINTER(ctypes.c_float)]
    f2 = ndpointer(dtype=np.float32, ndim=2, flags="C_CONTIGUOUS")
    lib.planes_oversample.argtypes = [f2, ctypes.c_size_t, ctypes.c_size_t, f2]
    lib.planes_blur.argtypes = [f2, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_float, f2]
    return lib


def reference_rows(lib, img, thresh_dog, nb_octaves, nb_scales=3):
    h, w = img.shape
    lib.sift.argtypes = (ndpointer(dtype=ctypes.c_float, shape=(h, w)), ctypes.c_uint, ctypes.c_uint, ctypes.c_float, ctypes.c_uint, ctypes.c_uint,
                         ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint))
    size, n = ctypes.c_uint(), ctypes.c_uint()
    ptr = lib.sift(np.ascontiguousarray(img, dtype=np.float32), w, h, thresh_dog, nb_octaves, nb_scales, ctypes.byref(size), ctypes.byref(n))
    rows = np.ctypeslib.as_array(ptr, shape=(n.value * size.value,)).copy().reshape(n.value, size.value) if n.value else np.zeros((0, 132), np.float32)
    lib.delete_buffer(ptr)
    return rows.astype(np.float32)


def reference_planes(lib, img, g):
    """the reference's oversampling and blur routines run along the chain of the geometry"""
    out = []
    scaled = np.ascontiguousarray(img.astype(np.float32) * np.float32(1.0 / 256.0))
    for o in range(g["n_oct"]):
        h, w = g["h"][o], g["w"][o]
        planes = np.zeros((g["n_planes"], h, w), np.float32)
        if o == 0:
            seed = np.zeros((h, w), np.float32)
            lib.planes_oversample(scaled, img.shape[1], img.shape[0], seed)
            lib.planes_blur(seed, w, h, float(g["inc"][0, 0]), planes[0])
        else:
            planes[0] = out[o - 1][g["n_planes"] - 3][0:2 * h:2, 0:2 * w:2]
        for s in range(1, g["n_planes"]):
            lib.planes_blur(np.ascontiguousarray(planes[s - 1]), w, h, float(g["inc"][o, s]), planes[s])
        out.append(planes)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--march-native", action="store_true", help="build with -march=native instead of -mavx -ffp-contract=off (not for the fixture)")
    ap.add_argument("--out", default=CS.GOLDEN)
    a = ap.parse_args()
    flags = ["-O2", "-march=native", "-fpic", "-shared", "-w", "-fopenmp"] if a.march_native else FLAGS
    out = {"flags": np.array(" ".join(flags)), "cases": np.array(list(CS.CASES))}
    spread, plane_err, dog_err = np.zeros(6), 0.0, 0.0
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(a.reference, tmp, flags)
        for name, (h, w, seed, thresh, n_oct) in CS.CASES.items():
            img = CS.image(name)
            ref = reference_rows(lib, img, thresh, n_oct)
            rule = CS.detect(img, thresh, n_oct)
            g = rule["geom"]
            if name != "flat":
                assert min(min(g["w"]), min(g["h"])) >= 13, (name, g["w"], g["h"])
            n_frag = int((rule["fragile"] & (rule["cand"][:, 4] > 0)).sum())  # of the rule's own candidates
            assert n_frag <= 0.02 * max(len(rule["rows"]), 1) or name == "flat", (name, n_frag, len(rule["rows"]))
            ia, ib = CS.pair_rows(ref, rule["rows"])
            un_ref = np.setdiff1d(np.arange(len(ref)), ia)
            un_rule = np.setdiff1d(np.arange(len(rule["rows"])), ib)
            for k in un_rule:
                assert rule["fragile"][rule["row_cand"][k]], (name, "the rule's row", k, "is not in the reference")
            for k in un_ref:
                assert CS.fragile_near(rule["cand"], rule["fragile"], g["delta"], ref[k]), (name, "the reference's row", k, "is not in the rule")
            assert np.all(np.diff(ib) > 0), (name, "the reference lists its keypoints in another order than the rule")
            sp = CS.spreads(ref[ia].astype(np.float64), rule["rows"][ib])
            spread = np.maximum(spread, sp)
            for pr, pq in zip(reference_planes(lib, img, g), rule["planes"]):
                for s in range(g["n_planes"]):
                    plane_err = max(plane_err, float(np.abs(pr[s] - pq[s]).max() / np.abs(pq[s]).max()))
                dog_err = max(dog_err, float(np.abs((pr[1:] - pr[:-1]).astype(np.float64) - (pq[1:] - pq[:-1])).max()))
            print("{:14s} {:3d} x {:3d}: {} octaves, reference {} rows, rule {} rows, counts {}, fragile {}, unpaired {} / {}, spread {}".format(
                name, h, w, g["n_oct"], len(ref), len(rule["rows"]), rule["counts"].tolist(), n_frag, len(un_ref), len(un_rule),
                np.array2string(sp, precision=3)))
            out.update(CS.pack(name, img, ref, rule))
    for k, key in enumerate(CS.SPREAD_KEYS):
        out["spread_" + key] = np.float64(spread[k])
    out["spread_plane"] = np.float64(plane_err)
    out["spread_dog"] = np.float64(dog_err)  # absolute, of a DoG sample formed in float32 from the reference's planes
    assert 2 * dog_err <= CS.EXT_EPS, ("EXT_EPS of tests/cases_sift.py is below twice the reference's DoG error", dog_err)
    print("spreads:", {k: float(out["spread_" + k]) for k in CS.SPREAD_KEYS + ("plane", "dog")})
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")
    assert os.path.getsize(a.out) <= 1000000


if __name__ == "__main__":
    main()

"""
Golden vectors of the pairwise matching (satba.ft_match) -- runs ONLY where the reference is mounted, like tools/gen_golden_ft.py.
Writes tests/golden/ft_match.npz (numeric arrays only; descriptors as uint8) and the reference's line of profiles/ft_match.json.

The reference's matcher is `matching` of 3rdparty/sift/simd/sift4ctypes.cpp.  It needs nothing but its own translation unit, which
is compiled here into a temporary directory (the other objects of that library need png.h; `matching` does not call them):

    g++ -O2 -fpic -shared -w -I <simd dir> sift4ctypes.cpp -o <tmp>/libmatch.so      (no -march, no fast-math)

and loaded lazily.  Nothing compiled and no reference text is kept.  Per case of tests/cases_match.py and per variant (gate on / off
x relative / absolute), per pair: the reference's selection (ft_match.get_pt_indices_inside_utm_bbx), the coordinates `matching`
returns, the index pairs that ft_s2p.s2p_match_SIFT's `list.index` makes of them (mapped back to the images' rows), and what the
reference's filter_matches_inconsistent_utm_coords keeps of those; per pair also the similarities of the reference's
rectifying_similarities_from_affine_fundamental_matrix.

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_match.py            # golden + timing line
    ... python tools/gen_golden_match.py golden | time
"""
import ctypes
import importlib
import json
import os
import platform
import subprocess
import sys
import tempfile
import time
import types

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_golden as G  # noqa: E402  (imports the reference)
import cases_match as CM  # noqa: E402

SIMD = "/root/reference/3rdparty/sift/simd"
PROFILE = os.path.join(ROOT, "profiles", "ft_match.json")


def reference_ft_match():
    """the reference's ft_match module; its matchers' imports (cv2, the prebuilt sift library) are stubbed: nothing here calls them"""
    ft = types.ModuleType("bundle_adjust.feature_tracks")
    ft.__path__ = ["/root/reference/bundle_adjust/feature_tracks"]
    sys.modules.setdefault("bundle_adjust.feature_tracks", ft)
    for name in ("bundle_adjust.feature_tracks.ft_opencv", "bundle_adjust.feature_tracks.ft_s2p"):
        sys.modules.setdefault(name, types.ModuleType(name))
    loader = types.ModuleType("bundle_adjust.loader")
    loader.flush_print, loader.get_id = print, (lambda p: p)
    sys.modules.setdefault("bundle_adjust.loader", loader)
    sys.modules.pop("bundle_adjust.feature_tracks.ft_match", None)
    return importlib.import_module("bundle_adjust.feature_tracks.ft_match")


def compile_matching(tmp):
    path = os.path.join(tmp, "libmatch.so")
    subprocess.run(["g++", "-O2", "-fpic", "-shared", "-w", "-I", SIMD, os.path.join(SIMD, "sift4ctypes.cpp"), "-o", path], check=True)
    lib = ctypes.CDLL(path, mode=os.RTLD_LAZY)
    fp, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
    lib.matching.argtypes = (fp, fp, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_float, ctypes.c_float, dp, ctypes.c_bool,
                             ctypes.c_bool, ctypes.POINTER(ctypes.c_uint))
    lib.matching.restype = fp
    lib.delete_buffer.argtypes = (fp,)
    lib.delete_buffer.restype = None
    name = "rectifying_similarities_from_affine_fundamental_matrix"
    sim = getattr(lib, "_Z{}{}PfS_Pd".format(len(name), name))  # C++ linkage: (float*, float*, double*)
    sim.argtypes, sim.restype = (fp, fp, dp), None
    return lib, sim


def run_matching(lib, k1, k2, F, thr, relative):
    """the call of ref:bundle_adjust/s2p/sift.py:189-235 -> (M, 4) float32 coordinates"""
    k1, k2 = np.ascontiguousarray(k1, dtype=np.float32), np.ascontiguousarray(k2, dtype=np.float32)
    coeff = np.zeros(5) if F is None else np.asarray([F[0, 2], F[1, 2], F[2, 0], F[2, 1], F[2, 2]], dtype=np.float64)
    n = ctypes.c_uint()
    fp, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
    ptr = lib.matching(k1.ctypes.data_as(fp), k2.ctypes.data_as(fp), 128, 4, len(k1), len(k2), thr, CM.EPI_THR, coeff.ctypes.data_as(dp), F is not None,
                       bool(relative), ctypes.byref(n))
    out = np.ctypeslib.as_array(ptr, shape=(max(n.value, 1) * 4,))[: n.value * 4].copy().reshape(-1, 4)
    lib.delete_buffer(ptr)
    return out


def stored_inputs(case):
    """numeric arrays from which cases_match.from_golden rebuilds the case"""
    scale = case.get("scale", 1.0)
    sizes = np.array([f.shape[0] for f in case["feats"]], dtype=np.int64)
    head = np.concatenate([f[:, :4] for f in case["feats"]]).astype(np.float32)
    desc = np.concatenate([np.where(np.isnan(f[:, 4:]), 0.0, f[:, 4:] * np.float32(scale)) for f in case["feats"]])
    assert np.array_equal(desc, np.rint(desc)) and desc.min() >= 0 and desc.max() <= 255
    return dict(sizes=sizes, head=head, desc=desc.astype(np.uint8), utm=np.concatenate(case["utm"]), pairs=case["pairs"], boxes=case["boxes"],
                F=np.stack(case["F"]), scale=np.float64(scale))


def golden():
    R = reference_ft_match()
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        lib, sim = compile_matching(tmp)
        for name in CM.CASES:
            case = CM.make(name)
            arrays.update({"{}_{}".format(name, k): v for k, v in stored_inputs(case).items()})
            sims = np.zeros((len(case["pairs"]), 6), dtype=np.float32)
            fp = ctypes.POINTER(ctypes.c_float)
            for p, F in enumerate(case["F"]):
                coeff = np.asarray([F[0, 2], F[1, 2], F[2, 0], F[2, 1], F[2, 2]], dtype=np.float64)
                sim(sims[p, :3].ctypes.data_as(fp), sims[p, 3:].ctypes.data_as(fp), coeff.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
            arrays[name + "_sim"] = sims
            for vname, gate, relative, thr in CM.VARIANTS:
                ofs, coords, renamed, fofs, filt, sel = [0], [], [], [0], [], []
                for p, (i, j) in enumerate(case["pairs"]):
                    box = case["boxes"][p]
                    si = R.get_pt_indices_inside_utm_bbx(case["utm"][i][:, 0], case["utm"][i][:, 1], *box)
                    sj = R.get_pt_indices_inside_utm_bbx(case["utm"][j][:, 0], case["utm"][j][:, 1], *box)
                    sel.append((len(si), len(sj)))
                    c, m, f = np.zeros((0, 4), np.float32), np.zeros((0, 2), np.int64), np.zeros((0, 2), np.int64)
                    if len(si) and len(sj):
                        fi, fj = case["feats"][i][si], case["feats"][j][sj]
                        c = run_matching(lib, fi, fj, case["F"][p] if gate else None, CM.variant_thr(case, thr, relative), relative)
                        if len(c):  # ref:ft_s2p.py:163-168, then ref:ft_match.py:175-181
                            all_i, all_j = fi[:, :2].tolist(), fj[:, :2].tolist()
                            m = np.array([[all_i.index(a), all_j.index(b)] for a, b in zip(c[:, :2].tolist(), c[:, 2:].tolist())], dtype=np.int64)
                            m = np.stack([si[m[:, 0]], sj[m[:, 1]]], axis=1)
                            f = R.filter_matches_inconsistent_utm_coords(m, case["utm"][i], case["utm"][j])
                    coords.append(c); renamed.append(m); filt.append(f)
                    ofs.append(ofs[-1] + len(m)); fofs.append(fofs[-1] + len(f))
                key = "{}_{}_".format(name, vname)
                arrays.update({key + "ofs": np.array(ofs, dtype=np.int64), key + "coords": np.concatenate(coords), key + "renamed": np.concatenate(renamed),
                               key + "fofs": np.array(fofs, dtype=np.int64), key + "filt": np.concatenate(filt), key + "sel": np.array(sel, dtype=np.int64)})
                print("{} {}: selected {} -> {} matches, {} after the UTM filter".format(name, vname, sel, np.diff(ofs).tolist(), np.diff(fofs).tolist()), flush=True)
    for k, v in arrays.items():
        assert np.asarray(v).dtype.kind in "iuf", k
    np.savez_compressed(os.path.join(G.OUT, "ft_match.npz"), **arrays)
    print("wrote ft_match.npz:", len(arrays), "arrays")
    size = os.path.getsize(os.path.join(G.OUT, "ft_match.npz"))
    assert size < 1 << 20, size


def timing(n=5000):
    """single-thread seconds of the reference's `matching` at n x n, gated and ungated, on this host's CPU"""
    rng = np.random.default_rng(5)
    k = [np.concatenate([rng.integers(0, 8000, (n, 2)) / 4.0, np.ones((n, 2)), rng.integers(0, 256, (n, 128))], axis=1).astype(np.float32) for _ in range(2)]
    row = {"shape": "{0} x {0}".format(n), "host": "{} ({}), one thread, g++ -O2".format(platform.processor() or platform.machine(), platform.system())}
    with tempfile.TemporaryDirectory() as tmp:
        lib, _ = compile_matching(tmp)
        for label, F in (("ungated_s", None), ("gated_s", CM.fundamental(1))):
            t0 = time.perf_counter()
            m = run_matching(lib, k[0], k[1], F, 0.6, True)
            row[label] = time.perf_counter() - t0
            row[label.replace("_s", "_matches")] = int(len(m))
    row["ungated_ops_per_s"] = 2.0 * 128 * n * n / row["ungated_s"]
    out = json.load(open(PROFILE)) if os.path.exists(PROFILE) else {}
    out["reference"] = [row]
    with open(PROFILE, "w") as f:
        json.dump(out, f, indent=1)
    print(row, "->", PROFILE)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    if mode in ("all", "golden"):
        golden()
    if mode in ("all", "time"):
        timing()

"""
Golden vectors of the track construction (satba.ft_utils) -- runs ONLY where the reference is mounted, like
tools/gen_golden_tracks.py, whose reference import it reuses.  Writes tests/golden/feature_tracks.npz (numeric arrays only).

Per case of tests/cases_ft.py: the keypoints (x, y, scale), their offsets, the matches, the pairs, and the (C, C_v2) that the
reference's feature_tracks_from_pairwise_matches returns for them, called unchanged on temporary keypoint files of equal length
(the reference stacks them; the shorter images are padded with NaN rows, which no match names).  For cases_ft.PRE_CASES also the
matrices before the baseline check (the same call with every pair listed) and the indices the reference's
filter_C_using_pairs_to_triangulate keeps of it.

    MPLBACKEND=Agg PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_ft.py
"""
import contextlib
import importlib
import io
import os
import sys
import tempfile
import types

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_golden as G  # noqa: E402  (imports the reference)
import cases_ft as CF  # noqa: E402

# the real ft_match needs cv2; nothing on this path calls it
sys.modules["bundle_adjust.feature_tracks.ft_match"] = types.ModuleType("bundle_adjust.feature_tracks.ft_match")
R = importlib.import_module("bundle_adjust.feature_tracks.ft_utils")


def keypoint_files(case, tmp):
    """One 132-column keypoint file per image, all of the length of the longest image (NaN rows behind the image's own)."""
    kp, kp_ofs = case["kp"], case["kp_ofs"]
    sizes = np.diff(kp_ofs)
    paths = []
    for m in range(sizes.size):
        f = np.full((int(sizes.max()), 132), np.nan, dtype=np.float32)
        f[: sizes[m], :3] = kp[kp_ofs[m]:kp_ofs[m + 1]]
        f[: sizes[m], 3:] = 0.0
        paths.append(os.path.join(tmp, "{:03d}.npy".format(m)))
        np.save(paths[-1], f)
    return paths


def run_reference(case, pairs):
    with tempfile.TemporaryDirectory() as tmp:
        paths = keypoint_files(case, tmp)
        with contextlib.redirect_stdout(io.StringIO()):
            C, C_v2 = R.feature_tracks_from_pairwise_matches(paths, case["matches"], [tuple(int(v) for v in p) for p in pairs])
    return C, C_v2


def main():
    arrays = {}
    for name in CF.GOLDEN_CASES:
        case = CF.make(name)
        C, C_v2 = run_reference(case, case["pairs"])
        out = dict(case, C=C, C_v2=C_v2)
        if name in CF.PRE_CASES:
            n_img = case["kp_ofs"].size - 1
            C_pre, C_v2_pre = run_reference(case, [(i, j) for i in range(n_img) for j in range(i + 1, n_img)])
            keep = R.filter_C_using_pairs_to_triangulate(C_pre, [tuple(int(v) for v in p) for p in case["pairs"]])
            assert np.array_equal(C_pre[:, keep], C, equal_nan=True)
            out.update(C_pre=C_pre, C_v2_pre=C_v2_pre, keep=np.asarray(keep, dtype=np.int64))
        print("{}: {} images, {} keypoints, {} matches, {} pairs -> {} tracks".format(name, case["kp_ofs"].size - 1, int(case["kp_ofs"][-1]),
                                                                                    len(case["matches"]), len(case["pairs"]), C.shape[1]), flush=True)
        arrays.update({name + "_" + k: v for k, v in out.items()})
    for k, v in arrays.items():
        assert np.asarray(v).dtype.kind in "iuf", k
    G.save("feature_tracks", **arrays)


if __name__ == "__main__":
    main()

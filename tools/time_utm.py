"""
Figures of the geographic side of the pairwise matching (satba.ft_match.utm_filter, keypoints_to_utm_coords_batch, the tail of
match_stereo_pairs) in profiles/ft_utm.json.

    python tools/time_utm.py --rounding [output.json]                  # CPU only: the "rounding" section
    python tools/time_utm.py [--label NAME] [--package DIR] [output.json]   # needs a GPU: one line of the "times" section

rounding: e_host, the largest absolute error [m] of geo_utils.utm_from_lonlat against the mpmath evaluation of the same series
(tests/cases_utm.py: utm_truth, 40 digits) over lonlat_samples(), and the band 8 x e_host that tests/test_utm_host.py and
tests/test_gpu_utm.py hold the device's projection to.

times, medians of 3 after one warm-up, wall times around the Python calls:
  tail_ms        what match_stereo_pairs does behind the device match and its fetch, at 2 000 pairs of 2 000 matches between 64
                 images of 20 000 keypoints, no geometric filter: renaming through the index maps, UTM filter, the M x 4 array.
                 The index maps (canonical_index_map, host, unchanged) are timed apart as index_maps_ms.
  utm_filter_kernel_ms / utm_filter_call_ms   the filter's device call inside the tail (HIP events / wall)
  keypoints_kernel_ms / keypoints_call_ms     the UTM coordinates of 64 images of 20 000 keypoints (13 of them padding)
--package DIR imports the package from DIR instead of this tree (a checkout of another commit beside the same library); where
the package has no `utm_filter` the tail is the per-pair loop that commit runs (its _rename and _after_match, in its
match_stereo_pairs' order) and the keypoints go through its single-image keypoints_to_utm_coords, image by image.  Both lines are
kept: the section that is not measured stays as the output file has it.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "ft_utm.json")
N_PAIRS, N_MATCHES, N_IMAGES, N_KP = 2000, 2000, 64, 20000


def rounding():
    import cases_utm as U

    lon, lat, zone = U.lonlat_samples()
    e_host = U.host_rounding(lon, lat, zone)
    return {"what": "tests/cases_utm.py host_rounding(): geo_utils.utm_from_lonlat in float64 against utm_truth (mpmath, 40 digits) over "
                    "lonlat_samples(), largest absolute error of an easting or a northing, on the CPU",
            "points": int(lon.size), "e_host_m": float(e_host), "device_factor": 8, "band_m": 8.0 * float(e_host)}


def inputs():
    rng = np.random.default_rng([44, 1])
    feats = [np.rint(4.0 * rng.uniform(0.0, 3000.0, (N_KP, 2))).astype(np.float32) / np.float32(4.0) for _ in range(N_IMAGES)]
    ground = rng.uniform([300000.0, 4000000.0], [310000.0, 4010000.0], (N_KP, 2))
    utms = [ground + rng.normal(0.0, 1.5, (N_KP, 2)) + (rng.random((N_KP, 1)) < 0.05) * rng.uniform(-60.0, 60.0, (N_KP, 2)) for _ in range(N_IMAGES)]
    sides = np.stack([rng.integers(0, N_IMAGES - 1, N_PAIRS), np.zeros(N_PAIRS, dtype=np.int64)], axis=1)
    sides[:, 1] = sides[:, 0] + 1 + rng.integers(0, N_IMAGES - 1 - sides[:, 0])
    ofs = np.arange(N_PAIRS + 1, dtype=np.int64) * N_MATCHES
    kp = np.sort(rng.integers(0, N_KP, (N_PAIRS, N_MATCHES)), axis=1).reshape(-1).astype(np.int32)  # a match joins the same ground point
    return feats, utms, sides, ofs, kp, kp.copy()


def median_ms(fn, n=3):
    fn()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        out = fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t)), out


def times():
    from satba import ft_match
    from satba.rpc_model import RPCModel

    feats, utms, sides, ofs, kp_i, kp_j = inputs()
    row = {"pairs": N_PAIRS, "matches_per_pair": N_MATCHES, "images": N_IMAGES, "keypoints_per_image": N_KP}
    row["index_maps_ms"], maps = median_ms(lambda: [ft_match.canonical_index_map(f) for f in feats])
    if hasattr(ft_match, "utm_filter"):
        def tail():
            m_ij, im, _, keep, info = ft_match._rename_and_filter(ofs, kp_i, kp_j, sides, feats, utms, True, None, {}, 0, None)
            return np.concatenate([m_ij, im], axis=1)[keep], info
        row["tail_ms"], (out, info) = median_ms(tail)
        row["tail_ms"] -= row["index_maps_ms"]  # _rename_and_filter builds the maps itself
        row["utm_filter_kernel_ms"] = info["utm_kernel_ms"]
        m_ij, _, used, rows = ft_match._rename_all(ofs, kp_i, kp_j, sides, feats, True)
        utm4 = ft_match._both_sides(utms, used, rows)
        row["utm_filter_call_ms"], _ = median_ms(lambda: ft_match.utm_filter(ofs, utm4))
    else:
        def tail():  # the loop of that commit's match_stereo_pairs, the maps given
            jobs = []
            for m in range(N_PAIRS):
                i, j = sides[m]
                m_ij = np.stack([kp_i[ofs[m]:ofs[m + 1]], kp_j[ofs[m]:ofs[m + 1]]], axis=1).astype(np.int64)
                jobs.append((ft_match._rename(m_ij, (maps[i], maps[j]), True), feats[i], feats[j]))
            rows = []
            for (m_ij, _, _), m in zip(jobs, range(N_PAIRS)):
                i, j = sides[m]
                m_ij, _ = ft_match._after_match(m_ij, feats[i], feats[j], utms[i], utms[j], None, None)
                if m_ij.shape[0]:
                    rows.append(np.concatenate([m_ij, np.tile(np.array([[i, j]], dtype=np.int64), (m_ij.shape[0], 1))], axis=1))
            return np.concatenate(rows, axis=0), None
        row["tail_ms"], (out, _) = median_ms(tail)
    row["rows_kept"] = int(out.shape[0])
    row["rows_checksum"] = int(out.astype(np.uint64).sum() % (1 << 61))  # the two lines computed the same rows
    # keypoints to UTM: the two shipped RPCs in turn, quarter pixels over the image, 13 rows of padding
    rng = np.random.default_rng([44, 2])
    rpc_dir = os.path.join(ROOT, "tests", "golden", "rpc")
    rpcs = [RPCModel.from_file(os.path.join(rpc_dir, f)) for f in sorted(os.listdir(rpc_dir)) if f.endswith(".rpc")]
    rpcs = [rpcs[c % 2] for c in range(N_IMAGES)]
    full = []
    for r in rpcs:
        f = np.zeros((N_KP, 132), dtype=np.float32)
        f[:, 0], f[:, 1] = rng.integers(0, int(8 * r.col_offset), N_KP) / 4.0, rng.integers(0, int(8 * r.row_offset), N_KP) / 4.0
        f[-13:] = np.nan
        full.append(f)
    offsets, alts = [{"col0": 0.0, "row0": 0.0}] * N_IMAGES, [r.alt_offset for r in rpcs]
    if hasattr(ft_match, "keypoints_to_utm_coords_batch"):
        row["keypoints_call_ms"], (u, info) = median_ms(lambda: ft_match.keypoints_to_utm_coords_batch(full, rpcs, offsets, alts, return_info=True))
        row["keypoints_kernel_ms"] = info["kernel_ms"]
    else:
        row["keypoints_call_ms"], u = median_ms(lambda: [ft_match.keypoints_to_utm_coords(f, r, o, a) for f, r, o, a in zip(full, rpcs, offsets, alts)])
    row["keypoints_mean_easting"] = float(np.mean([np.nanmean(x[:, 0]) for x in u]))
    return row


def main(argv):
    args, flags = [], {}
    it = iter(argv)
    for a in it:
        if a in ("--label", "--package"):
            flags[a] = next(it)
        elif a.startswith("--"):
            flags[a] = True
        else:
            args.append(a)
    for path in (flags.get("--package", os.path.join(ROOT, "sat-bundleadjust_amd")), os.path.join(ROOT, "tests"), ROOT):
        sys.path.insert(0, path)
    out_path = args[0] if args else OUT
    doc = {}
    for src in (OUT, out_path):
        if os.path.exists(src):
            with open(src) as f:
                doc.update(json.load(f))
    if "--rounding" in flags:
        doc["rounding"] = rounding()
    else:
        doc.setdefault("times", {})[flags.get("--label", "this_commit")] = times()
    print(json.dumps(doc), flush=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1:])

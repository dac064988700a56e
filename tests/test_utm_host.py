"""The geographic side of the pairwise matching on the host: tests/host/utm_dump.cpp, built with the address and undefined-behaviour
sanitizers, runs the functions of csrc/satba_utm_geom.h and csrc/satba_elbow.h -- the code the kernels of satba_utm.h and
k_out_elbow run -- as a program of its own.  The filter is compared with `filter_matches_inconsistent_utm_coords` pair by pair,
exactly, and, behind the vectorised renaming of satba.ft_match, with the reference's stored results; the projection with an mpmath
evaluation of the same series."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cases_match as CM
import cases_utm as U
from satba import ft_match, geo_utils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sat-bundleadjust_amd", "csrc")
GRID = [(name, v) for name in CM.CASES for v in CM.VARIANTS]
GRID_IDS = ["{}-{}".format(name, v[0]) for name, v in GRID]


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


@pytest.fixture(scope="session")
def dump(tmp_path_factory):
    """(path of the dump program, whether it carries the sanitizers, a directory for its inputs)"""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler ($CXX, g++, /opt/rocm/lib/llvm/bin/clang++)")
    tmp = tmp_path_factory.mktemp("utm_dump")
    exe = str(tmp / "utm_dump")
    # no contraction, as on the device (the pragmas of the headers are clang's; x86-64 without -mfma fuses nothing either way)
    base = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "host", "utm_dump.cpp"), "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode == 0:
        return exe, True, str(tmp)
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe, False, str(tmp)


def run_dump(dump, values):
    path = os.path.join(dump[2], "in.bin")
    np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in values]).tofile(path)
    r = subprocess.run([dump[0], path], capture_output=True)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()
    return np.frombuffer(r.stdout, dtype=np.float64)


def host_filter(dump, pair_ofs, utm4, alive=None, margin=U.MARGIN):
    """(keep, thr, n_kept) of the device's functions run sequentially"""
    n, n_pairs = len(utm4), len(pair_ofs) - 1
    a = np.ones(n) if alive is None else np.asarray(alive, dtype=np.float64)
    out = run_dump(dump, [[0, margin, n_pairs], pair_ofs, utm4, a])
    assert out.size == n + 2 * n_pairs
    return out[:n] != 0, out[n:n + n_pairs], out[n + n_pairs:].astype(np.int64)


@pytest.fixture(scope="module")
def truth():
    """the mpmath truth on the samples, once"""
    lon, lat, zone = U.lonlat_samples()
    return lon, lat, zone, U.utm_truth(lon, lat, zone)


def test_dump_program_carries_the_sanitizers(dump):
    if not dump[1]:
        pytest.skip("the sanitizer runtimes do not link with this compiler: the code was checked on a build without them")


def test_new_symbols_are_declared():
    from satba import engine_hip

    header = open(os.path.join(ROOT, "include", "satba.h")).read()
    for sym in ("satba_utm_filter", "satba_keypoints_utm"):
        assert re.search(r"\b%s\s*\(" % sym, header) and sym in engine_hip.SYMBOLS, sym
    lib = engine_hip.load_library()
    for sym in ("satba_utm_filter", "satba_keypoints_utm"):
        assert hasattr(lib, sym), sym
    assert callable(ft_match.utm_filter) and callable(ft_match.keypoints_to_utm_coords_batch)


def test_cases_hold_what_they_are_for():
    """the curves do what their comments say, by the host restatement"""
    cases = U.filter_cases()
    keep, thr, n_kept = U.filter_reference(cases["curves_in_order"])
    by = dict(zip(U.CURVES, range(len(U.CURVES))))
    ofs = cases["curves_in_order"]["pair_ofs"]
    assert thr[by["two_points"]] == 9.0 + 5.0                       # the elbow only rounding decides
    assert thr[by["equal"]] == 12.0 and thr[by["zero"]] == 5.0 and n_kept[by["zero"]] == 10
    assert thr[by["L"]] == 11.0 and n_kept[by["L"]] == 41 and len(U.L_CURVE) == 43  # 11 == thr is kept, 50 and 60 are not
    d = np.array(U.L_CURVE_JUST_ABOVE)
    assert thr[by["L_just_above"]] == 11.0 and np.array_equal(keep[ofs[by["L_just_above"]]:ofs[by["L_just_above"] + 1]], d <= 11.0)
    assert np.sum(d == 11.0) == 1 and np.sum(d == 11.25) == 1
    assert thr[by["concave"]] == 46.0 and n_kept[by["concave"]] == 11  # the elbow fails: thr is the maximum and all are kept
    v = np.array(U.CURVES["elbow_is_percentile"])
    assert ft_match.get_elbow_value(v)[0] == np.percentile(v, 80) == 1.0 and thr[by["elbow_is_percentile"]] == 6.0
    assert sorted(np.diff(cases["sizes_L"]["pair_ofs"]).tolist()) == sorted(U.SIZES)
    a = cases["alive_patterns"]
    counts = [int(a["alive"][a["pair_ofs"][p]:a["pair_ofs"][p + 1]].sum()) for p in range(5)]
    assert counts == [43, 0, 1, 22, 39]  # all, none, one, alternating, exactly the matches up to the elbow
    # plateaus: more than one point at the largest distance from the chord, in exact arithmetic
    v = U._plateau(257)
    s = (v[-1] - v[0]) / (len(v) - 1)
    gap = s * np.arange(len(v)) - (v - v[0])
    assert np.sum(gap == gap.max()) > 10


@pytest.mark.parametrize("name", list(U.filter_cases()))
def test_filter_equals_the_reference_pair_by_pair(dump, name):
    case = U.filter_cases()[name]
    keep, thr, n_kept = host_filter(dump, case["pair_ofs"], case["utm4"], case["alive"], case["margin"])
    want = U.filter_reference(case)
    assert np.array_equal(keep, want[0])
    assert np.array_equal(thr, want[1], equal_nan=True)
    assert np.array_equal(n_kept, want[2])


def test_elbow_core_equals_get_elbow_value(dump):
    """the shared core alone, on the curves and on the error vectors the outlier rejection is tested with"""
    import cases_outliers as CO

    curves = [np.sort(np.asarray(v, dtype=np.float64)) for v in U.CURVES.values()] + [U._plateau(n) for n in (255, 257, 5000)]
    curves += [np.sort(CO.errors(p, n, 0)) for p in ("random", "plateau", "no_elbow", "equal_2.5") for n in (1, 2, 3, 257, 1000)]
    for v in curves:
        elbow, success = ft_match.get_elbow_value(v)
        got = run_dump(dump, [[3, len(v)], v])
        assert got[0] == elbow and bool(got[1]) == success and got[2] == v[-1], len(v)


@pytest.fixture(scope="module")
def golden():
    return CM.load()


@pytest.mark.parametrize("name,variant", GRID, ids=GRID_IDS)
def test_vectorised_renaming_and_filter_equal_the_reference(dump, golden, name, variant):
    """the rewired tail of match_stereo_pairs -- one renaming step over all pairs, one filter call -- on the reference's own results"""
    vname, gate, relative, thr = variant
    case, key = CM.from_golden(golden, name), "{}_{}_".format(name, vname)
    ofs, ki, kj = CM.rule(case, gate, relative, thr)
    m_ij, im, used, rows = ft_match._rename_all(ofs, ki, kj, case["pairs"], case["feats"], True)
    assert m_ij.dtype == np.int64 and np.array_equal(m_ij, golden[key + "renamed"])
    assert np.array_equal(im, np.repeat(case["pairs"], np.diff(ofs), axis=0))
    utm4 = ft_match._both_sides(case["utm"], used, rows)
    for p, (i, j) in enumerate(case["pairs"]):
        s = slice(ofs[p], ofs[p + 1])
        assert np.array_equal(utm4[s], np.concatenate([case["utm"][i][m_ij[s, 0]], case["utm"][j][m_ij[s, 1]]], axis=1))
    keep, _, n_kept = host_filter(dump, ofs, utm4)
    assert np.array_equal(np.concatenate([[0], np.cumsum(n_kept)]), golden[key + "fofs"])
    assert np.array_equal(m_ij[keep], golden[key + "filt"])
    raw = ft_match._rename_all(ofs, ki, kj, case["pairs"], case["feats"], False)[0]
    assert np.array_equal(raw, np.stack([ki, kj], axis=1))


def test_zone_rule(dump):
    lon = np.array([-180.0, -179.999, -174.0, -72.0000001, -72.0, -71.9999, -6.0, -1e-9, 0.0, 5.999, 6.0, 107.29, 174.0, 179.999, 180.0, 185.0, -186.0])
    want = [geo_utils.utm_zone_from_lonlat(v, 0.0) for v in lon]
    assert run_dump(dump, [[2, len(lon)], lon]).astype(int).tolist() == want
    assert min(want) == 1 and max(want) == 60


def test_band_is_what_was_measured(truth):
    """profiles/ft_utm.json holds e_host, the rounding of geo_utils.utm_from_lonlat against the truth, and the band 8 x e_host (the
    factor of the RANSAC tests over the restatement's own rounding); recomputed here.  Below 1 um as a condition: one ulp of a
    northing is 2 nm, a band of micrometres would mean another series."""
    lon, lat, zone, _ = truth
    prof = json.load(open(os.path.join(ROOT, "profiles", "ft_utm.json")))["rounding"]
    e_host = U.host_rounding(lon, lat, zone)
    print("e_host {:.6e} m, committed {:.6e} m, band {:.6e} m".format(e_host, prof["e_host_m"], prof["band_m"]))
    assert prof["band_m"] == 8.0 * prof["e_host_m"] == U.band()
    assert e_host <= prof["e_host_m"] <= 2.0 * e_host  # the one measured (another libm may round a last bit differently)
    assert 0.0 < prof["band_m"] < 1e-6


def test_projection_lies_within_the_band(dump, truth):
    lon, lat, zone, (te, tn) = truth
    out = run_dump(dump, [[1, len(lon)], np.stack([lon, lat, zone.astype(np.float64)], axis=1)]).reshape(-1, 2)
    worst = max(np.abs(out[:, 0] - te).max(), np.abs(out[:, 1] - tn).max())
    print("host-compiled satba_utm_geom.h against the truth: {:.6e} m (band {:.6e} m)".format(worst, U.band()))
    assert worst <= U.band()
    # the samples are what they are for: both hemispheres, both signs of longitude, points on either side of a zone's edge
    assert (lat > 0).any() and (lat < 0).any() and (lon > 0).any() and (lon < 0).any() and (tn < 0).any()
    assert (te < 200000.0).any() or (te > 800000.0).any()

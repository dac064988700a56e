"""The windowed matching on the host: the numpy rule of tests/cases_window.py against cases_match.rule and the reference's stored
results at an infinite radius; the cases against what their comments promise; and csrc/satba_window_cells.h -- the cells the kernels
of satba_window.h order and visit the keypoints by -- run as a program of its own (tests/host/window_cells_dump.cpp) under the
address and undefined-behaviour sanitizers: every candidate of the rule lies in a cell its query visits, the cell of a coordinate is
monotone, and the grid's dimensions keep their cap."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cases_match as CM
import cases_window as W
from satba import ft_match

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sat-bundleadjust_amd", "csrc")
MAX_DIM = 1 << 20


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


@pytest.fixture(scope="module")
def golden():
    return CM.load()


@pytest.mark.parametrize("name", CM.CASES)
def test_rule_at_infinite_radius_is_the_free_absolute_rule(golden, name):
    case = CM.from_golden(golden, name)
    ofs, ki, kj, n_cand = W.rule_window(case, np.inf, np.inf, 250.0)
    want = CM.rule(case, False, False, 250.0)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip((ofs, ki, kj), want))
    assert np.array_equal(ofs, golden[name + "_free_abs_ofs"])
    sel = golden[name + "_free_abs_sel"]
    assert n_cand == int((sel[:, 0] * sel[:, 1]).sum())  # every selected pair of keypoints is a candidate


def test_smaller_windows_keep_fewer_matches(golden):
    got = {name: [int(W.rule_window(CM.from_golden(golden, name), r, r, 250.0)[0][-1]) for r in (np.inf, 30.0, 6.0, 2.0)] for name in ("small", "ties", "scene")}
    assert got == {"small": [46, 45, 42, 2], "ties": [11, 8, 8, 0], "scene": [76, 76, 69, 32]}
    assert [W.rule_window(CM.from_golden(golden, "scene"), r, r, 250.0)[3] for r in (np.inf, 30.0, 6.0, 2.0)] == [145068, 840, 368, 196]


def test_cases_hold_what_they_are_for():
    c = W.make("edge")
    rx, ry = c["radius"]
    ui, uj = c["utm"][0], c["utm"][1]
    dx, dy = np.abs(ui[:, None, 0] - uj[None, :, 0]), np.abs(ui[:, None, 1] - uj[None, :, 1])
    assert rx != ry and (dx == rx).sum() >= 4 and (dy == ry).sum() >= 4                       # on the edge: out
    assert (dx == np.nextafter(rx, 0)).sum() >= 4 and (dy == np.nextafter(ry, 0)).sum() >= 4  # one step inside: in
    ofs, ki, kj, n_cand = W.rule_window(c, rx, ry, W.THR)
    assert n_cand == 2 * 13 + 2 and ofs[1] == 2  # 7 + 6 keypoints per query (one "out" of query 1 rounds in), both queries matched
    assert W.rule_window(c, np.nextafter(rx, np.inf), np.nextafter(ry, np.inf), W.THR)[3] > n_cand

    c = W.make("cells")
    counts = W.window_counts(c, 0, 4.0, 4.0)
    assert counts[:20].min() > 0 and counts[24] == 0 and counts[25] == 0  # corners of the grid have neighbours, far queries have none
    assert np.ptp(c["utm"][2], axis=0).max() < 4.0 and len(c["utm"][3]) == 1  # a grid of one cell, a single keypoint

    c = W.make("sparse")
    assert np.ptp(c["utm"][1][:, 0]) >= 1e6 and c["radius"] == (0.25, 0.25)
    assert 0 < W.rule_window(c, 0.25, 0.25, W.THR)[0][1] < len(c["utm"][0])

    c = W.make("dense")
    counts = W.window_counts(c, 0, 30.0, 30.0)
    assert sorted(counts[:7].tolist()) == [63, 64, 64, 65, 65, 300, 5000]
    ofs, ki, kj, _ = W.rule_window(c, 30.0, 30.0, W.THR)
    matched = dict(zip(ki.tolist(), kj.tolist()))
    assert 0 in matched and 3 in matched and 1 not in matched and 2 not in matched and 4 not in matched and 6 not in matched  # thr decides
    base = np.concatenate([[0], np.cumsum([63, 64, 65, 5000, 300, 65, 64])])
    assert matched[3] == base[3] + 4321 and matched[5] == base[5] + 7  # the exact copy beats 62 499; of two equal d the lower j

    c = W.make("ties")
    ofs, ki, kj, _ = W.rule_window(c, 10.0, 10.0, W.THR)
    first = [12 + 4 * k for k in range(6)]
    assert ki[:ofs[1]].tolist() == list(range(6)) and kj[:ofs[1]].tolist() == first  # the lowest j inside, not the copy outside
    assert W.rule_window(c, np.inf, np.inf, W.THR)[2][:12].tolist() == list(range(12))  # which wins without a window

    c = W.make("extremes")
    lo, hi, _ = c["thrs"]
    assert np.float32(lo) ** 2 < 8323200 < np.float32(hi) ** 2 and np.nextafter(np.float32(lo), np.float32(np.inf)) == np.float32(hi)
    assert W.rule_window(c, 5.0, 5.0, lo)[0].tolist() == [0, 1, 2] and W.rule_window(c, 5.0, 5.0, hi)[0].tolist() == [0, 4, 9]

    c = W.make("boxed")
    i, j = c["pairs"][1]
    out = np.setdiff1d(np.where(~np.isnan(c["utm"][j][:, 0]))[0], CM.inside(c["utm"][j], c["boxes"][1]))
    si = CM.inside(c["utm"][i], c["boxes"][1])
    assert W.window_mask(c["utm"][i][si], c["utm"][j][out], 6.0, 2.0).any()  # outside the box, inside a selected query's window
    assert any(len(CM.inside(c["utm"][c["pairs"][p][1]], c["boxes"][p])) == 0 for p in range(len(c["pairs"])))
    assert np.isnan(c["utm"][0][-1]).all() and np.isnan(c["utm"][1][200]).all()
    assert len(set(map(tuple, c["pairs"].tolist()))) < len(c["pairs"])

    c = W.make("float")
    assert c["scale"] == CM.FLOAT_SCALE and (c["feats"][0][:, 4:] != np.trunc(c["feats"][0][:, 4:])).any()


# ----------------------------------------------------------------------------- the cells

@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """(path of the dump program, whether it carries the sanitizers, a directory for its inputs)"""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler ($CXX, g++, /opt/rocm/lib/llvm/bin/clang++)")
    tmp = tmp_path_factory.mktemp("window_cells_dump")
    exe = str(tmp / "window_cells_dump")
    base = [cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-I", CSRC, os.path.join(ROOT, "tests", "host", "window_cells_dump.cpp"), "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode == 0:
        return exe, True, str(tmp)
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe, False, str(tmp)


def cells(dump, uj, ui, rx, ry):
    """grid (x.o, x.w, x.n, y.o, y.w, y.n), the cells (n_j, 2) of the keypoints, the ranges (n_i, 4) of the queries"""
    path = os.path.join(dump[2], "in.bin")
    uj, ui = np.asarray(uj, dtype=np.float64).reshape(-1, 2), np.asarray(ui, dtype=np.float64).reshape(-1, 2)
    np.concatenate([[rx, ry, len(uj), len(ui)], uj.reshape(-1), ui.reshape(-1)]).tofile(path)
    r = subprocess.run([dump[0], path], capture_output=True)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()
    out = np.frombuffer(r.stdout, dtype=np.float64)
    assert out.size == 6 + 2 * len(uj) + 4 * len(ui)
    return out[:6], out[6:6 + 2 * len(uj)].reshape(-1, 2).astype(np.int64), out[6 + 2 * len(uj):].reshape(-1, 4).astype(np.int64)


def check_cells(dump, uj, ui, rx, ry, tight=False):
    uj, ui = np.asarray(uj, dtype=np.float64).reshape(-1, 2), np.asarray(ui, dtype=np.float64).reshape(-1, 2)
    grid, cj, rng = cells(dump, uj, ui, rx, ry)
    # the cap, and cells no narrower than the window
    assert 1 <= grid[2] <= MAX_DIM and 1 <= grid[5] <= MAX_DIM and grid[1] >= rx and grid[4] >= ry
    assert (cj >= 0).all() and (cj[:, 0] < grid[2]).all() and (cj[:, 1] < grid[5]).all()
    assert (rng >= 0).all() and (rng[:, 1] < grid[2]).all() and (rng[:, 3] < grid[5]).all()
    # monotone in the coordinate
    for k in range(2):
        order = np.argsort(uj[:, k], kind="stable")
        assert (np.diff(cj[order, k]) >= 0).all()
    # coverage: every candidate of the rule lies in a visited cell
    mask = W.window_mask(ui, uj, rx, ry)
    qi, kj = np.where(mask)
    assert (rng[qi, 0] <= cj[kj, 0]).all() and (cj[kj, 0] <= rng[qi, 1]).all()
    assert (rng[qi, 2] <= cj[kj, 1]).all() and (cj[kj, 1] <= rng[qi, 3]).all()
    if tight:  # coordinates whose spacing is far below the window: at most four cells per axis, three but for rounding
        assert (rng[:, 1] - rng[:, 0] <= 3).all() and (rng[:, 3] - rng[:, 2] <= 3).all()
    return grid, cj, rng, int(mask.sum())


def test_dump_program_carries_the_sanitizers(dump):
    if not dump[1]:
        pytest.skip("the sanitizer runtimes do not link with this compiler: the code was checked on a build without them")


@pytest.mark.parametrize("name", W.CASES)
def test_cells_cover_the_rule_on_the_cases(dump, name):
    case = W.make(name)
    total = 0
    for rx, ry in W.radii_of(case):
        for p, (i, j) in enumerate(case["pairs"]):
            si, sj = CM.inside(case["utm"][i], case["boxes"][p]), CM.inside(case["utm"][j], case["boxes"][p])
            total += check_cells(dump, case["utm"][j][sj], case["utm"][i][si], rx, ry, tight=True)[3]
    assert total == sum(W.rule_window(case, rx, ry, W.THR)[3] for rx, ry in W.radii_of(case))


def test_sparse_case_meets_the_cap(dump):
    case = W.make("sparse")
    grid = check_cells(dump, case["utm"][1], case["utm"][0], 0.25, 0.25)[0]
    assert np.ptp(case["utm"][1][:, 0]) / 0.25 > MAX_DIM and grid[2] == MAX_DIM and grid[5] == MAX_DIM and grid[1] > 0.25


@pytest.mark.parametrize("r", [30.0, 0.1, 1e-3, 1.0 / 3.0, 4.0, np.inf])
def test_cells_cover_where_rounding_decides(dump, r):
    """keypoints one unit in the last place either side of e +- r, for queries of several magnitudes: fl(e - r) can lie above e - r
    with a candidate between the two"""
    rng = np.random.default_rng(5)
    e = np.concatenate([[0.0, 500000.3, 4649776.22482, -7.1, 1e9 + 0.7], rng.uniform(2e5, 8e5, 40), rng.uniform(-1e7, 1e7, 40)])
    ui = np.stack([e, e[::-1]], axis=1)
    rows = [ui]
    if np.isfinite(r):
        def steps(v):
            return [v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf), np.nextafter(np.nextafter(v, -np.inf), -np.inf),
                    np.nextafter(np.nextafter(v, np.inf), np.inf)]

        for sign in (-1.0, 1.0):  # beside the window's edge on one axis, at the query on the other
            rows += [np.stack([v, ui[:, 1]], axis=1) for v in steps(ui[:, 0] + sign * r)]
            rows += [np.stack([ui[:, 0], v], axis=1) for v in steps(ui[:, 1] + sign * r)]
            rows += [np.stack([v, w], axis=1) for v, w in zip(steps(ui[:, 0] + sign * r), steps(ui[:, 1] - sign * r))]
        edges = e.min() + r * np.arange(0, 64)  # and beside the edges of the cells themselves
        rows += [np.stack([v, np.full(64, ui[np.argmin(e), 1])], axis=1) for v in steps(edges)]
    uj = np.concatenate(rows)
    n_cand = check_cells(dump, uj, ui, r, r)[3]
    assert n_cand > len(e)
    check_cells(dump, uj, ui, r, 2.5 * r if np.isfinite(r) else 1.0)


def test_huge_extents_one_keypoint_and_none(dump):
    for uj in ([[-1e15, 3.0], [1e15, 4.0], [0.0, 3.5]], [[-1e300, -1e308], [1e300, 1e308], [0.0, 0.0]], [[5.0, 5.0]], np.zeros((0, 2)),
               [[2.0 ** 52, 1.0], [2.0 ** 52 + 1.0, 1.0], [2.0 ** 53, 1.0]]):
        ui = np.array([[0.0, 3.5], [1e15, 4.0], [-1e300, 0.0], [5.0, 5.0], [2.0 ** 52, 1.0], [1e308, -1e308]])
        for r in (0.25, 30.0, 1e6, np.inf):
            grid = check_cells(dump, uj, ui, r, r)[0]
            if len(uj) <= 1:
                assert grid[2] == 1 and grid[5] == 1


# ----------------------------------------------------------------------------- the public interface

def test_local_window_is_a_method_and_the_foreign_ones_still_raise():
    from satba import engine_hip

    assert "local_window" in ft_match.METHODS and ft_match._method({"FT_sift_matching": "local_window"}) == "local_window"
    for method in ("flann", "lightglue"):
        with pytest.raises(ValueError):
            ft_match._method({"FT_sift_matching": method})
    header = open(os.path.join(ROOT, "include", "satba.h")).read()
    assert re.search(r"\bsatba_match_window\s*\(", header) and "satba_match_window" in engine_hip.SYMBOLS
    assert callable(ft_match.match_pairs_window) and callable(ft_match.locally_match_SIFT_utm_coords)
    with pytest.raises(ValueError):
        ft_match.match_pairs_window([(0, 1)], [None, None], [None, None], [W.EVERYWHERE], radius=(1.0, 2.0, 3.0))

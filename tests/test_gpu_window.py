"""
The windowed matching on the device (satba.ft_match.match_pairs_window, csrc/satba_window.h) against the numpy rule of
tests/cases_window.py -- exactly: offsets, indices, dtypes and the number of candidates -- and, at an infinite radius, against
match_pairs without gate under the absolute threshold and the reference's stored results (tests/golden/ft_match.npz).
"""
import numpy as np
import pytest

import cases_match as CM
import cases_window as W
from satba import ft_match

pytestmark = pytest.mark.gpu

SWITCHES = ("SATBA_MATCH_CHUNK", "SATBA_MATCH_FLOAT")
GRID = [(name, r, thr) for name in W.CASES for r in W.radii_of(W.make(name)) for thr in W.thrs_of(W.make(name))]
GRID_IDS = ["{}-{:g}x{:g}-{:.8g}".format(name, r[0], r[1], thr) for name, r, thr in GRID]
_GOLDEN, _CASES, _RULE = {}, {}, {}


def golden():
    if not _GOLDEN:
        g = CM.load()
        _GOLDEN.update({k: g[k] for k in g.files})
    return _GOLDEN


def match_case(name):
    if name not in _CASES:
        _CASES[name] = CM.from_golden(golden(), name)
    return _CASES[name]


def rule_of(name, r, thr):
    """computed once per (case, radius, thr), shared and never modified"""
    key = (name, r, thr)
    if key not in _RULE:
        _RULE[key] = W.rule_window(W.make(name), r[0], r[1], thr)
        for a in _RULE[key][:3]:
            a.setflags(write=False)
    return _RULE[key]


def device(case, r, thr, only=None, **kw):
    idx = list(range(len(case["pairs"]))) if only is None else list(only)
    return ft_match.match_pairs_window(case["pairs"][idx], case["feats"], case["utm"], case["boxes"][idx], radius=r, thr=CM.variant_thr(case, thr, False),
                                       return_info=True, **kw)


def same(out, want):
    return all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(out[:3], want[:3])) and out[3]["n_candidates"] == want[3]


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("name,r,thr", GRID, ids=GRID_IDS)
def test_device_equals_the_rule(gpu, name, r, thr):
    case = W.make(name)
    out, want = device(case, r, thr), rule_of(name, r, thr)
    print(name, r, thr, "matches", int(out[0][-1]), "of", int(want[0][-1]), "candidates", out[3]["n_candidates"], "of", want[3], out[3]["path"])
    assert same(out, want)
    assert out[3]["path"] == ("float32" if name == "float" else "int8")
    sel = [(len(CM.inside(case["utm"][i], b)), len(CM.inside(case["utm"][j], b))) for (i, j), b in zip(case["pairs"], case["boxes"])]
    assert out[3]["n_selected"] == sum(a + b for a, b in sel) and out[3]["n_empty_pairs"] == sum(1 for a, b in sel if not a or not b)


@pytest.mark.parametrize("name", CM.CASES)
def test_infinite_radius_equals_match_pairs_and_the_reference(gpu, name):
    case, g = match_case(name), golden()
    thr = CM.variant_thr(case, 250.0, False)
    out = ft_match.match_pairs_window(case["pairs"], case["feats"], case["utm"], case["boxes"], radius=np.inf, thr=thr, return_info=True)
    brute = ft_match.match_pairs(case["pairs"], case["feats"], case["utm"], case["boxes"], F=None, thr=thr, relative=False, return_info=True)
    assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(out[:3], brute[:3]))
    assert all(out[3][k] == brute[3][k] for k in ("n_selected", "n_empty_pairs", "path"))
    assert np.array_equal(out[0], g[name + "_free_abs_ofs"])
    sel = g[name + "_free_abs_sel"]
    assert out[3]["n_candidates"] == int((sel[:, 0] * sel[:, 1]).sum())
    if name not in ("same_coords", "ties", "extremes"):  # as tests/test_gpu_match.py: no two keypoints share a location
        assert np.array_equal(np.stack([out[1], out[2]], axis=1), g[name + "_free_abs_renamed"])
    # a scalar and a pair are the same window where they say the same
    assert all(np.array_equal(x, y) for x, y in zip(out[:3], ft_match.match_pairs_window(case["pairs"], case["feats"], case["utm"], case["boxes"],
                                                                                         radius=(np.inf, np.inf), thr=thr)))


@pytest.mark.parametrize("name", [n for n in W.CASES if n != "float"])
def test_float_switch_changes_no_match_on_integer_data(gpu, monkeypatch, name):
    monkeypatch.setenv("SATBA_MATCH_FLOAT", "1")
    case = W.make(name)
    r, thr = W.radii_of(case)[0], W.thrs_of(case)[-1]
    out = device(case, r, thr)
    assert same(out, rule_of(name, r, thr)) and out[3]["path"] == "float32"


def test_float_case_reports_its_path(gpu):
    out = device(W.make("float"), (30.0, 30.0), W.THR)
    assert out[3]["path"] == "float32" and out[0][-1] > 0


@pytest.mark.parametrize("name,r", [("boxed", (6.0, 2.0)), ("cells", (4.0, 4.0))])
def test_a_subset_of_the_pairs_is_a_slice_of_the_full_call(gpu, name, r):
    case = W.make(name)
    ofs, ki, kj, _ = device(case, r, W.THR)
    n = len(case["pairs"])
    for only in ([p] for p in range(n)):
        o1, i1, j1, info = device(case, r, W.THR, only=only)
        p = only[0]
        assert np.array_equal(i1, ki[ofs[p]:ofs[p + 1]]) and np.array_equal(j1, kj[ofs[p]:ofs[p + 1]]) and o1.tolist() == [0, ofs[p + 1] - ofs[p]]
        assert info["n_candidates"] == W.rule_window(case, r[0], r[1], W.THR, only=only)[3]
    order = list(range(n))[::-1]  # pairs in the caller's order, whatever it is
    o2, i2, j2, info = device(case, r, W.THR, only=order)
    assert np.array_equal(np.diff(o2), np.diff(ofs)[order])
    assert np.array_equal(i2, np.concatenate([ki[ofs[p]:ofs[p + 1]] for p in order]))
    assert np.array_equal(j2, np.concatenate([kj[ofs[p]:ofs[p + 1]] for p in order]))
    assert info["n_candidates"] == rule_of(name, r, W.THR)[3]


def test_two_runs_give_identical_bits(gpu):
    for name in ("dense", "boxed", "float"):
        case = W.make(name)
        r = W.radii_of(case)[0]
        a, b = device(case, r, W.THR), device(case, r, W.THR)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3])) and a[3]["n_candidates"] == b[3]["n_candidates"]


def test_argument_errors_raise(gpu):
    c = W.make("extremes")
    one = dict(pairs=[(0, 1)], features=c["feats"], utm_coords=c["utm"], boxes=[W.EVERYWHERE])
    for bad in (dict(one, radius=0.0), dict(one, radius=-30.0), dict(one, radius=(30.0, 0.0)), dict(one, radius=(-np.inf, 1.0)), dict(one, radius=float("nan")),
                dict(one, radius=(30.0, float("nan"))), dict(one, thr=0.0), dict(one, thr=-250.0), dict(one, thr=float("nan")), dict(one, pairs=[(1, 1)]),
                dict(one, pairs=[(0, 2)]), dict(one, boxes=[(0.0, np.nan, 0.0, 1.0)])):
        with pytest.raises(ValueError):
            ft_match.match_pairs_window(**bad)
    ofs, ki, kj, info = ft_match.match_pairs_window([], c["feats"], c["utm"], np.zeros((0, 4)), return_info=True)
    assert ofs.tolist() == [0] and ki.size == 0 and kj.size == 0 and info["n_candidates"] == 0

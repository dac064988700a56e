"""The scalar side of the trust-region loop (csrc/satba_lm.h as a host compiler builds it: tests/host/lm_scalars_dump.cpp, with the address
and undefined-behaviour sanitizers; satba/trf.py) on the models of tests/cases_lm_scalars.py, against a 400-bit solver of the same problem.
With q(p) = p^T B p / 2 + g^T p, q* the reference's optimum, eps = 2^-52 and scale = |g| Delta + max |B| Delta^2 / 2, every row with
finite inputs and Delta > 0 must give a step that is
  finite;
  feasible   |p| <= Delta (1 + 8 eps): the final rescale and the rotation into the eigenbasis;
  optimal    q(p) - q* <= 64 eps scale: a relative perturbation of a few eps in p moves q by a few eps scale;
  flagged    as a Newton step exactly where exact arithmetic says so decisively (cases_lm_scalars.reference).
Measured (worst q(p) - q* in eps scale; C++ | trf.py | scipy | the C++ before the singular models were handled):
  ordinary 3.7 | 2.7 | 2.2 | NaN steps (6 rows)      hard 2.6 | 2.6 | 4.5e15 and 39 rows scipy raises on or misses | 2.6
  stall 2.4 | 2.5 | 2.7e11 | NaN steps (34 rows)      singular 0.9 | 0.9 | 0.9 | 4.5e15 (= 1.0 scale: no decrease at all)
  scales 2.1 | 1.1 | 1.0 | 2.1                        radius 0.7 | 0.7 | raises | NaN steps
No family needs more than the 64 eps."""
import numpy as np
import pytest

import cases_lm_scalars as K
from satba import engine_hip, trf


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """(path of the dump program, whether it carries the sanitizers)"""
    d = K.build_dump(tmp_path_factory.mktemp("lm_scalars"), sanitize=True)
    if d is None:
        pytest.skip("no C++ compiler ($CXX, g++, /opt/rocm/lib/llvm/bin/clang++)")
    return d


@pytest.fixture(scope="module")
def ref():
    """the reference, recomputed"""
    return K.compute_reference()


@pytest.fixture(scope="module")
def cpp(dump):
    return K.run_dump(dump[0], "rows", K.corpus()[0])


def _steps(solve):
    rows, _ = K.corpus()
    out = np.zeros((len(rows), 3))
    for i, r in enumerate(rows):
        p, newton = solve(np.array([[r[0], r[1]], [r[1], r[2]]]), r[3:5].copy(), r[5])
        out[i] = p[0], p[1], newton
    return out


def test_dump_program_carries_the_sanitizers(dump):
    if not dump[1]:
        pytest.skip("the sanitizer runtimes do not link or start with this compiler: the scalars were checked on a build without them")


def test_reference_is_the_stored_one_and_decides_the_flag_on_most_rows(ref):
    rows, fam = K.corpus()
    assert len(rows) % 256 != 0 and fam[K.corpus()[0][:, 5] == 0].size > 0
    for got, want in zip(ref, K.golden_reference()):
        assert np.array_equal(got, want, equal_nan=True)
    ok = K.checked(rows)
    undecided = int((ref[2][ok] < 0).sum())
    print("Newton flag undecided on {} of {} compared rows ({:.1%})".format(undecided, ok.sum(), undecided / ok.sum()))
    assert undecided < 0.10 * ok.sum() and undecided < 0.10 * len(rows)


def test_cpp_steps_are_finite_feasible_optimal_and_flagged(cpp, ref):
    rows, fam = K.corpus()
    worst = K.check_rows(rows, fam, cpp, ref, "satba_lm.h")
    print("satba_lm.h, worst q(p) - q* in eps scale:", {k: round(v, 2) for k, v in worst.items()})


def test_cpp_on_the_models_that_gave_nan(cpp):
    rows, fam = K.corpus()
    i = int(np.flatnonzero(fam == K.FAMILIES.index("stall"))[0])
    assert tuple(rows[i]) == (-1.0, 0.0, 1.0, 1e-20, 0.0, 1.0)
    assert tuple(cpp[i, :3]) == (-1.0, 0.0, 0.0)  # the boundary point along v1, down what there is of a gradient
    zero = (rows[:, 5] == 0) & np.isfinite(rows).all(1)
    assert zero.sum() >= 20 and not cpp[zero, :3].any()
    assert np.isfinite(cpp[K.checked(rows)]).all()  # ... and the helpers behind the step: Delta_new, ratio, term


def test_trf_py_meets_the_same_properties(cpp, ref):
    rows, fam = K.corpus()
    out = _steps(trf.solve_trust_region_2d)  # raises nothing, non-finite models included
    worst = K.check_rows(rows, fam, out, ref, "trf.py")
    ok = K.checked(rows) & np.isfinite(rows[:, 5])
    diff = np.abs(out[ok, :2] - cpp[ok, :2]).max(1) / rows[ok, 5]
    print("trf.py, worst q(p) - q* in eps scale:", {k: round(v, 2) for k, v in worst.items()})
    print("trf.py against satba_lm.h (math.hypot against sqrt(a a + b b)): {} of {} steps differ, at most {:.3g} Delta".format(
        int((diff > 0).sum()), ok.sum(), diff.max()))


def test_scipy_agrees_on_ordinary_models(cpp, ref):
    """the same flag wherever it is decisive and no better a model value than the C++'s beyond the tolerance; nothing about scipy elsewhere"""
    from scipy.optimize._lsq import common as sc
    import mpmath as mp

    rows, fam = K.corpus()
    sel = np.flatnonzero(fam == K.FAMILIES.index("ordinary"))
    worst_sc = worst_cpp = 0.0
    with mp.workprec(400):
        for i in sel:
            r = rows[i]
            p, newton = sc.solve_trust_region_2d(np.array([[r[0], r[1]], [r[1], r[2]]]), r[3:5].copy(), r[5])
            if ref[2][i] >= 0:
                assert bool(newton) == bool(cpp[i, 2]) == bool(ref[2][i]), (i, tuple(r))
            scale = mp.mpf(K.EPS) * (mp.sqrt(mp.mpf(r[3]) ** 2 + mp.mpf(r[4]) ** 2) * r[5] + max(abs(r[:3])) * mp.mpf(r[5]) ** 2 / 2)
            q_sc, q_cpp = K.model_value(r, p), K.model_value(r, cpp[i, :2])
            qs = (mp.mpf(ref[0][i, 0]) + mp.mpf(ref[0][i, 1])) * scale / mp.mpf(K.EPS)
            assert q_cpp - q_sc <= 64 * scale, (i, tuple(r), float((q_cpp - q_sc) / scale))
            worst_sc, worst_cpp = max(worst_sc, float((q_sc - qs) / scale)), max(worst_cpp, float((q_cpp - qs) / scale))
    print("ordinary models, worst q(p) - q* in eps scale: scipy {:.2f}, satba_lm.h {:.2f}".format(worst_sc, worst_cpp))
    assert worst_cpp <= 64


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def test_radius_and_termination_helpers_are_scipys_on_special_values(dump):
    from scipy.optimize._lsq import common as sc

    grid = K.radius_grid()
    got = K.run_dump(dump[0], "radius", grid)
    for row, g in zip(grid, got):
        args = tuple(float(v) for v in row[:4]) + (bool(row[4]),)
        want = sc.update_tr_radius(*args)
        assert _same(g, want), (args, tuple(g), want)
        assert _same(trf.update_tr_radius(*args), want), args
    grid = K.term_grid()
    got = K.run_dump(dump[0], "term", grid)
    for row, g in zip(grid, got):
        args = tuple(float(v) for v in row)
        want = sc.check_termination(*args)
        assert g[0] == (want or 0), (args, g[0], want)  # scipy's None is the C++ 0
        assert trf.check_termination(*args) == want, args


def test_library_host_compilation_is_the_stand_alone_one(cpp):
    """satba_lm_scalars(device = 0), the header as the library's host side carries it, against the dump program: bit for bit, NaN equal to NaN"""
    rows, _ = K.corpus()
    host = engine_hip.lm_scalars(rows, device=False)
    assert np.array_equal(np.isnan(host), np.isnan(cpp))
    assert np.array_equal(host[~np.isnan(host)].view(np.uint64), cpp[~np.isnan(cpp)].view(np.uint64))


def test_arguments_are_checked_before_the_device_is_touched():
    lib = engine_hip.load_library()
    buf = np.zeros(6)
    ptr = engine_hip._ptr
    assert lib.satba_lm_scalars(2, 1, ptr(buf), ptr(buf)) == -1 and lib.satba_lm_scalars(1, -1, ptr(buf), ptr(buf)) == -1
    assert lib.satba_lm_scalars(1, 1, None, ptr(buf)) == -1 and lib.satba_lm_scalars(1, 1 << 25, ptr(buf), ptr(buf)) == -1
    assert lib.satba_lm_scalars(1, 0, None, None) == 0

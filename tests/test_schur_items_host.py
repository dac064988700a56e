"""Dispatch order of the work items of k_schur_pairs (csrc/satba_schur_items.h), checked on the host: tests/host/schur_items_dump.cpp,
built with the address and undefined-behaviour sanitizers, writes a table; every table is compared with a restatement of the order in
numpy and, independently of that, against what the kernels lean on.  Beside the factorisation the item of a pair's last chunk and the
last diagonal item of a camera WAIT for the pair's / camera's other items (satba_schur.h: SchurArgs::pair_cnt, dg_cnt): a table that
starts one of those after the item that waits for it hangs the device instead of failing a test."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sat-bundleadjust_amd", "csrc")
CHUNKED, MERGED, WEIGHTED = 0, 1, 2
XCDS, WAVES = 8, 4  # workgroup b runs on XCD b % 8 and takes 4 items


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


@pytest.fixture(scope="session")
def dump(tmp_path_factory):
    """(path of the dump program, whether it carries the sanitizers)"""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler ($CXX, g++, /opt/rocm/lib/llvm/bin/clang++)")
    exe = str(tmp_path_factory.mktemp("schur_items") / "schur_items_dump")
    base = [cxx, "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "host", "schur_items_dump.cpp"), "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode == 0:
        return exe, True
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe, False


def test_dump_program_carries_the_sanitizers(dump):
    if not dump[1]:
        pytest.skip("the sanitizer runtimes do not link with this compiler: the item tables were checked on a build without them")


def _table(dump, kind, M, C, spc, w):
    r = subprocess.run([dump[0], str(kind), str(M), str(C), str(spc), str(w)], capture_output=True)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()
    return np.frombuffer(r.stdout, dtype=np.int32).reshape(-1, 2)


def _expected(kind, M, C, spc, w):
    """(A) the order as satba_schur_items.h describes it"""
    weighted, merged = kind == WEIGHTED, kind == MERGED
    per, load = [[] for _ in range(XCDS)], [0] * XCDS
    for i in range(M if weighted else M - 1):
        x = load.index(min(load))  # least loaded XCD, the lowest index wins ties
        load[x] += M - 1 - i + (w if weighted else 0)
        first = i * M - i * (i + 1) // 2  # index of pair (i, i + 1)
        for ch in range(1 if merged else C):
            diag = np.stack([np.full(spc, -2 - i), ch * spc + np.arange(spc)], 1) if weighted else np.zeros((0, 2), int)
            pairs = np.stack([first + np.arange(M - 1 - i), np.full(M - 1 - i, -1 if merged else ch)], 1)
            pad = np.tile([-1, 0], ((-len(diag) - len(pairs)) % WAVES, 1))
            per[x].append(np.concatenate([diag, pairs, pad]))
    groups = [np.concatenate(g).reshape(-1, WAVES, 2) if g else np.zeros((0, WAVES, 2), int) for g in per]
    slots = max(len(g) for g in groups)
    if slots == 0:
        return np.tile([-1, 0], (WAVES, 1)).astype(np.int32)
    table = np.tile([-1, 0], (slots, XCDS, WAVES, 1))
    for x, g in enumerate(groups):
        table[: len(g), x] = g
    return table.reshape(-1, 2).astype(np.int32)


def _check_invariants(t, kind, M, C, spc):
    """(B) what the kernels and the factorisation beside them lean on; nothing here uses _expected"""
    weighted, merged = kind == WEIGHTED, kind == MERGED
    n_pairs = M * (M - 1) // 2
    assert len(t) % WAVES == 0
    block = np.arange(len(t)) // WAVES
    is_pair, is_diag = t[:, 0] >= 0, t[:, 0] <= -2
    # 1. coverage: every item exactly once, everything else padding, whole rounds of the 8 XCDs
    assert np.all(t[~is_pair & ~is_diag] == [-1, 0])
    pairs = t[is_pair]
    if merged:
        assert np.all(pairs[:, 1] == -1) and np.array_equal(np.sort(pairs[:, 0]), np.arange(n_pairs))
    else:
        assert np.all((pairs[:, 1] >= 0) & (pairs[:, 1] < C)) and np.all(pairs[:, 0] < n_pairs)
        assert np.array_equal(np.sort(pairs[:, 0].astype(np.int64) * C + pairs[:, 1]), np.arange(n_pairs * C))
    diags = np.stack([-2 - t[is_diag, 0], t[is_diag, 1]], 1)  # (camera, slot)
    if weighted:
        assert np.all((diags[:, 0] < M) & (diags[:, 1] >= 0) & (diags[:, 1] < C * spc))
        assert np.array_equal(np.sort(diags[:, 0].astype(np.int64) * C * spc + diags[:, 1]), np.arange(M * C * spc))
    else:
        assert len(diags) == 0
    if len(pairs) + len(diags) == 0:
        assert len(t) == WAVES
        return
    assert len(t) % (XCDS * WAVES) == 0
    # camera row and chunk of every item (paddings: -1)
    ii, _ = np.triu_indices(M, 1)  # pair index -> camera i: the pairs (i, j > i) row by row
    row = np.full(len(t), -1)
    chunk = np.full(len(t), -1)
    row[is_pair] = ii[t[is_pair, 0]]
    chunk[is_pair] = np.maximum(t[is_pair, 1], 0)
    row[is_diag] = diags[:, 0]
    chunk[is_diag] = diags[:, 1] // max(spc, 1)
    real = row >= 0
    key = row.astype(np.int64) * C + chunk  # ascends with (row, chunk)
    # 2. one (row, chunk) group per workgroup
    kb = np.where(real, key, -1).reshape(-1, WAVES)
    kmax = kb.max(1)
    assert np.all((kb == kmax[:, None]) | (kb == -1))
    # 3. one XCD per row
    xcd = block % XCDS
    row_xcd = np.full(M, -1)
    row_xcd[row[real]] = xcd[real]
    assert np.all(row_xcd[row[real]] == xcd[real])
    # 4. inside an XCD the workgroups ascend with (row, chunk): the rows of the pair triangle are finished from the top, the columns of S from the left
    for x in range(XCDS):
        kx = kmax[x::XCDS]
        kx = kx[kx >= 0]
        assert np.all(np.diff(kx) >= 0)
    if weighted:  # ... and the diagonal items of (i, chunk) come no later than its pair items
        last_diag = np.full(M * C, -1)
        np.maximum.at(last_diag, key[is_diag], block[is_diag])
        assert np.all(last_diag[key[is_pair]] <= block[is_pair])
    # 5. the item that waits for the others is the last one started
    if C > 1 and not merged and len(pairs):
        blk = np.full((n_pairs, C), -1)
        blk[t[is_pair, 0], t[is_pair, 1]] = block[is_pair]
        assert np.all(blk[:, : C - 1] < blk[:, C - 1 :])
    if weighted:
        blk = np.full((M, C * spc), -1)
        blk[diags[:, 0], diags[:, 1]] = block[is_diag]
        assert np.all(blk <= blk[:, -1:])


def _cases():
    for M, C in itertools.product((1, 2, 3, 5, 9, 10, 33, 70), (1, 2, 5)):
        yield CHUNKED, M, C, 0, 0
        yield MERGED, M, C, 0, 0
        for spc, w in itertools.product((1, 3), (1, 7)):
            yield WEIGHTED, M, C, spc, w
    yield CHUNKED, 200, 5, 0, 0  # the headline shape
    yield MERGED, 200, 5, 0, 0
    yield WEIGHTED, 200, 5, 3, 50


@pytest.mark.parametrize("kind", (CHUNKED, MERGED, WEIGHTED), ids=("chunked", "merged", "weighted"))
def test_item_tables_in_dispatch_order(dump, kind):
    n = 0
    for k, M, C, spc, w in _cases():
        if k != kind:
            continue
        t = _table(dump, k, M, C, spc, w)
        case = f"kind {k} M {M} C {C} spc {spc} dg_weight {w}"
        assert np.array_equal(t, _expected(k, M, C, spc, w)), case
        try:
            _check_invariants(t, k, M, C, spc)
        except AssertionError as e:
            raise AssertionError(case) from e
        n += 1
    assert n == (97 if kind == WEIGHTED else 25)


def test_invariants_notice_a_broken_order():
    """the checks of (B) are not vacuous: a pair's last chunk started first, and a camera's last diagonal item started first, are caught"""
    t = _expected(WEIGHTED, 9, 2, 3, 1)
    _check_invariants(t, WEIGHTED, 9, 2, 3)
    a, b = np.flatnonzero((t[:, 0] == 5) & (t[:, 1] == 0))[0], np.flatnonzero((t[:, 0] == 5) & (t[:, 1] == 1))[0]
    bad = t.copy()
    bad[[a, b]] = bad[[b, a]]
    with pytest.raises(AssertionError):
        _check_invariants(bad, WEIGHTED, 9, 2, 3)
    a, b = np.flatnonzero((t[:, 0] == -2 - 4) & (t[:, 1] == 0))[0], np.flatnonzero((t[:, 0] == -2 - 4) & (t[:, 1] == 5))[0]
    bad = t.copy()
    bad[[a, b]] = bad[[b, a]]
    with pytest.raises(AssertionError):
        _check_invariants(bad, WEIGHTED, 9, 2, 3)

"""Where the unit-weight front beside the factorisation cuts its diagonal pass (csrc/satba_diag_split.h), checked on the host:
tests/host/diag_split_dump.cpp, built with the address and undefined-behaviour sanitizers where they link, prints c* for every number
of late tile columns.

The rule, stated here independently of the header: the reduced system has M cameras x NP unknowns in T = ceil(M NP / 64) tile columns
of 64; camera c owns columns c NP .. c NP + NP - 1.  With `late` late tile columns the boundary is column b = 64 (T - late).  A camera
is LATE when it has a column at or behind b -- a camera that straddles b is late --, and c* is the first late camera.  Hence every
camera >= c* has a column in the last `late` tile columns (all of them, or it straddles b), and every camera < c* has none there."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sat-bundleadjust_amd", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler ($CXX, g++, /opt/rocm/lib/llvm/bin/clang++)")
    exe = str(tmp_path_factory.mktemp("diag_split") / "diag_split_dump")
    base = [cxx, "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "host", "diag_split_dump.cpp"), "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(exe, M, NP, applies=1):
    r = subprocess.run([exe, str(M), str(NP), str(applies)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    cols, forced = [], {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "default":
            forced["default"] = int(w[1])
        elif w[0] == "from":
            forced[int(w[1])] = int(w[2])
        else:
            cols.append(tuple(int(v) for v in w))
    return cols, forced


@pytest.mark.parametrize("M,NP", list(itertools.product((27, 40, 70, 128, 200), (3, 5, 8))))
def test_split_camera_for_every_number_of_late_columns(dump, M, NP):
    cols, forced = _run(dump, M, NP)
    T = (M * NP + 63) // 64
    assert [c[0] for c in cols] == list(range(T + 2)) and all(c[2] == T for c in cols)
    cstar = [c[1] for c in cols]
    assert all(0 <= c <= M for c in cstar)
    assert cstar[0] == M  # no late column: today's front
    assert all(a >= b for a, b in zip(cstar, cstar[1:]))  # more late columns: never fewer late cameras
    assert cstar[T] == 0 and cstar[T + 1] == 0  # every column late: every camera late
    for late in range(T + 1):
        b = 64 * (T - late)  # first late column
        cs = cstar[late]
        for c in range(M):
            last_col = c * NP + NP - 1
            if c >= cs:
                assert late > 0 and last_col >= b, (late, c)  # all its columns late, or it straddles the boundary
            else:
                assert last_col < b, (late, c)  # none of its columns in a late tile column
        if 0 < late < T:
            assert cs == b // NP
    # the default: 3 late tile columns of 16, scaled with T and rounded down -- never every column
    assert forced.pop("default") == 3 * T // 16 < T
    # the forced split: clamped to [0, M]
    assert forced == {f: min(max(f, 0), M) for f in range(-1, M + 2)}


@pytest.mark.parametrize("M,NP", [(27, 5), (200, 5)])
def test_no_split_where_the_route_does_not_apply(dump, M, NP):
    cols, forced = _run(dump, M, NP, applies=0)
    forced.pop("default")
    assert all(c[1] == M for c in cols) and all(v == M for v in forced.values())

"""cam_atan2_rounded (csrc/satba_camapprox.h), the double-double arctangent behind the longitude of k_cam_affine, on its own: the
function is __host__ __device__, tests/host/atan2_dump.hip calls it on the host (built whole -- the header's kernels want their fat
binary -- with the address and undefined-behaviour sanitizers on the host side where they link; it calls no HIP API and needs no
device).  Every result is compared bit for bit with the correctly rounded value of mpmath at 200 bits, and with numpy's arctan2 in
extended precision within half an ulp (the only check where mpmath is missing).  The inputs cover the four quadrants, both sides of
|y| = |x|, of the axes and of the cut at +-pi: every combination of the function's three branches."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEAMS = [0.0, math.pi / 4, -math.pi / 4, math.pi / 2, -math.pi / 2, 3 * math.pi / 4, -3 * math.pi / 4]
# (y, x)
EXACT = [(0.0, 1.0), (0.0, -1.0), (1.0, 0.0), (-1.0, 0.0), (1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0), (1e-300, 1.0), (1.0, 1e-300)]


def _hipcc():
    for cxx in (os.environ.get("HIPCC"), "hipcc", "/opt/rocm/bin/hipcc"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


@pytest.fixture(scope="session")
def dump(tmp_path_factory):
    """(path of the dump program, whether it carries the sanitizers)"""
    hipcc = _hipcc()
    assert hipcc is not None, "no hipcc ($HIPCC, hipcc, /opt/rocm/bin/hipcc): the library itself cannot be built either"
    exe = str(tmp_path_factory.mktemp("atan2") / "atan2_dump")
    base = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "sat-bundleadjust_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
            os.path.join(ROOT, "tests", "host", "atan2_dump.hip"), "-o", exe]
    r = subprocess.run(base + ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"], capture_output=True, text=True)
    if r.returncode == 0:
        return exe, True
    r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe, False


def test_dump_program_carries_the_sanitizers(dump):
    if not dump[1]:
        pytest.skip("the sanitizer runtimes do not link with this compiler: the arctangent was checked on a build without them")


def _run(dump, y, x):
    """cam_atan2_rounded(y, x) of the host build, bit for bit (hex floats both ways)"""
    text = "".join("{} {}\n".format(float(a).hex(), float(b).hex()) for a, b in zip(y, x))
    # (the HIP runtime's own start-up allocations are not this program's: no leak report at exit)
    r = subprocess.run([dump[0]], input=text, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and not r.stderr, r.stderr
    out = np.array([float("nan") if "nan" in t else float.fromhex(t) for t in r.stdout.split()])
    assert out.shape == (len(y),)
    return out


def _inputs():
    """y, x: 20 000 points over the full circle at ECEF radii, 2 000 within 1e-6 rad of each seam, 1 000 around +-pi, the exact cases"""
    rng = np.random.default_rng(20)
    ang = [rng.uniform(-math.pi, math.pi, 20000)] + [s + rng.uniform(-1e-6, 1e-6, 2000) for s in SEAMS] + [math.pi + rng.uniform(-1e-6, 1e-6, 1000)]
    ang = np.concatenate(ang)
    rad = rng.uniform(3.2e6, 6.4e6, ang.size)
    y, x = rad * np.sin(ang), rad * np.cos(ang)
    return np.concatenate([y, [e[0] for e in EXACT]]), np.concatenate([x, [e[1] for e in EXACT]])


def _mpmath_rounded(y, x):
    """atan2 correctly rounded to float64, or None without mpmath"""
    try:
        import mpmath
    except ImportError:
        return None
    with mpmath.workprec(200):
        # 200 bits: the nearest float64 is decided unless the value sits within 2^-147 relative of a rounding boundary
        return np.array([float(mpmath.atan2(mpmath.mpf(float(a)), mpmath.mpf(float(b)))) for a, b in zip(y, x)])


def test_inputs_reach_every_branch():
    y, x = _inputs()
    assert y.size == 20000 + 7 * 2000 + 1000 + len(EXACT)
    for flat in (False, True):  # |x| >= |y| or not, in each of the four quadrants
        for sx in (-1, 1):
            for sy in (-1, 1):
                assert np.sum(((np.abs(x) >= np.abs(y)) == flat) & (np.sign(x) == sx) & (np.sign(y) == sy)) > 1000
    ref = np.arctan2(y, x)
    for s in SEAMS:  # both sides of every seam, within 1e-6 rad
        near = np.abs(ref - s) < 1.1e-6
        assert np.sum(near & (ref < s)) > 500 and np.sum(near & (ref > s)) > 500
    assert np.sum(ref > math.pi - 1.1e-6) > 200 and np.sum(ref < -math.pi + 1.1e-6) > 200


def test_arctangent_is_correctly_rounded(dump):
    y, x = _inputs()
    got = _run(dump, y, x)
    assert np.isfinite(got).all()
    # numpy in extended precision (64-bit mantissa on x86: its own error is below 2^-63 relative); where long double is double the
    # bound still holds and is simply wider than needed.  A libm's float64 atan2 is NOT a reference at this level: numpy.arctan2 in
    # float64 differed from the rounded value on 227 of these 35 010 arguments where this was written (printed below)
    ref = np.arctan2(y.astype(np.longdouble), x.astype(np.longdouble))
    err = np.abs(got.astype(np.longdouble) - ref)
    bound = np.longdouble(0.5) * np.spacing(np.abs(ref.astype(np.float64))).astype(np.longdouble) + np.longdouble(2.0) ** -63 * np.abs(ref)
    assert np.all(err <= bound), "{} of {} beyond half an ulp".format(int(np.sum(err > bound)), y.size)
    exact = _mpmath_rounded(y, x)
    if exact is not None:
        differ = np.flatnonzero(got != exact)
        print("{} inputs, {} differ from mpmath's rounded value; numpy.arctan2 in float64 differs on {}".format(y.size, differ.size, int(np.sum(np.arctan2(y, x) != exact))))
        assert differ.size == 0, [(y[k].hex(), x[k].hex(), got[k].hex(), exact[k].hex()) for k in differ[:5]]


def test_zeros(dump):
    got = _run(dump, [0.0, -0.0, 0.0, -0.0], [0.0, -1.0, -1.0, 1.0])
    assert np.isnan(got[0])  # a point on the polar axis has no longitude
    # the function tests y < 0.0, which a negative zero is not: +pi where IEEE's atan2 gives -pi (a zero without a sign, as
    # mpmath takes it), and +0 on the positive x axis
    assert got[1] == math.pi and got[2] == math.pi and got[3] == 0.0 and not np.signbit(got[3])

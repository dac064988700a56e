"""The scalar side of the trust-region loop as the device runs it (satba_lm_scalars: one thread per model through csrc/satba_lm.h's
solve_trust_region_2d, update_tr_radius and check_termination) on the models of tests/cases_lm_scalars.py -- the hard case, stalled
secular brackets, singular and thin B, radii of 0, subnormal and inf, non-finite inputs: the branches no whole solve takes.
  bit identity  device compilation == the library's host compilation == a stand-alone host build (tests/host/lm_scalars_dump.cpp), NaN
                equal to NaN: the header's claim that the host loop and the decision kernels take the same decisions;
  values        finite, feasible, optimal to 64 eps scale and flagged as tests/test_lm_scalars_host.py states them, against the stored
                400-bit optima (tests/golden/lm_scalars.npz);
  shapes        1, 255, 256, 257 rows, the whole corpus (no multiple of the workgroup's 256), and none."""
import numpy as np
import pytest

import cases_lm_scalars as K
from satba import engine_hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_rows():
    return engine_hip.lm_scalars(K.corpus()[0], device=True)


def _same(a, b):
    """bit for bit, NaN equal to NaN"""
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))


def test_device_host_and_stand_alone_compilations_agree_bit_for_bit(device_rows, tmp_path):
    rows, fam = K.corpus()
    host = engine_hip.lm_scalars(rows, device=False)
    bad = np.flatnonzero([not _same(d, h) for d, h in zip(device_rows, host)])
    assert bad.size == 0, [(int(i), K.FAMILIES[fam[i]], tuple(rows[i]), tuple(device_rows[i]), tuple(host[i])) for i in bad[:10]]
    d = K.build_dump(tmp_path, sanitize=False)
    if d is None:
        pytest.fail("no C++ compiler ($CXX, g++, /opt/rocm/lib/llvm/bin/clang++) for the stand-alone host build")
    alone = K.run_dump(d[0], "rows", rows)
    bad = np.flatnonzero([not _same(a, h) for a, h in zip(alone, host)])
    assert bad.size == 0, [(int(i), K.FAMILIES[fam[i]], tuple(rows[i]), tuple(alone[i]), tuple(host[i])) for i in bad[:10]]


def test_device_steps_are_finite_feasible_optimal_and_flagged(device_rows):
    rows, fam = K.corpus()
    worst = K.check_rows(rows, fam, device_rows, K.golden_reference(), "satba_lm.h on the device")
    print("device, worst q(p) - q* in eps scale:", {k: round(v, 2) for k, v in worst.items()})
    i = int(np.flatnonzero(fam == K.FAMILIES.index("stall"))[0])
    assert tuple(rows[i]) == (-1.0, 0.0, 1.0, 1e-20, 0.0, 1.0) and tuple(device_rows[i, :3]) == (-1.0, 0.0, 0.0)
    assert np.isfinite(device_rows[K.checked(rows)]).all()


@pytest.mark.parametrize("n", (0, 1, 255, 256, 257))
def test_row_counts_around_the_workgroup(device_rows, n):
    rows, _ = K.corpus()
    assert len(rows) % 256 != 0
    pick = np.arange(n) * 17 % len(rows)  # across the families
    got = engine_hip.lm_scalars(rows[pick], device=True)
    assert got.shape == (n, 6) and _same(got, device_rows[pick])

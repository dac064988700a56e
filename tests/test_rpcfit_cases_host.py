"""
The scenarios of the RPC re-fit's margin loop (tests/cases_rpcfit.py), pinned on the CPU: every scenario ends at the margin its
table names, so it keeps exercising the branch it was chosen for, and in every round the worst crop corner is at least
cases_rpcfit.MIN_SLACK (1 px) away from the hull of the re-projected mesh, so that every correct implementation of the fit (they
differ by <= 2e-3 px in the projection) takes the same decisions.  No device: the replay is cases_rpcfit.expected_margins.
"""
import numpy as np
import pytest

import cases
import cases_rpcfit as K


def _check(key, n_samples, want):
    r, Rt, crop, gt = K.scenario(key)
    margin, dist, iters = K.expected_margins(r, Rt, crop, gt, n_samples)
    print(key, n_samples, margin, np.round(dist, 2), iters)
    assert margin == want
    assert len(dist) == int(np.log2(margin // 10)) + 1
    assert min(abs(d) for d in dist) >= K.MIN_SLACK, dist
    # every round but the last one doubled because a corner was outside; the last one is covered unless the loop gave up
    assert all(d > 0 for d in dist[:-1])
    assert dist[-1] < 0 or margin == K.GIVE_UP


@pytest.mark.parametrize("key", list(K.FULL_IMAGE), ids=lambda k: "file{}-s{}-{}".format(*k))
def test_full_image_scenarios_end_at_their_margins(key):
    _check(key, 10, K.FULL_IMAGE[key])


@pytest.mark.parametrize("key", list(K.CROPPED), ids=lambda k: "file{}-s{}-{}".format(*k[:3]))
def test_cropped_scenarios_end_at_their_margins(key):
    assert key[3][0] != 0 and key[3][1] != 0
    r = K.rpc(key[0])
    assert key[3][0] + key[3][2] < 2 * r.col_scale and key[3][1] + key[3][3] < 2 * r.row_scale  # smaller than the image
    _check(key, 10, K.CROPPED[key])


@pytest.mark.parametrize("n_samples", K.MESH_N)
@pytest.mark.parametrize("key", K.MESH_BATCH, ids=lambda k: "file{}-s{}".format(*k[:2]))
def test_mesh_size_scenarios_end_at_their_margins(key, n_samples):
    _check(key, n_samples, K.MESH_MARGINS[key])


def test_the_batches_scatter_their_slots():
    """what the mixed batches are for: later rounds hold non-consecutive slots, a run of length 1 beside one of length 2, and one
    camera gives up"""
    for batch in (K.BATCH_NONE, K.BATCH_GT):
        margins = [K.FULL_IMAGE[k] for k in batch]
        assert [k[0] for k in batch] == [i % 2 for i in range(len(batch))]  # the two shipped files alternate
        assert K.GIVE_UP in margins and len(set(margins)) >= 4
        rounds = [[i for i, m in enumerate(margins) if m >= mg] for mg in (20, 40, 80, 160, 320, 640, 1280)]
        gaps = [any(b - a > 1 for a, b in zip(r[:-1], r[1:])) for r in rounds]
        assert sum(gaps) >= 3
    assert [i for i, k in enumerate(K.BATCH_NONE) if K.FULL_IMAGE[k] >= 20] == [0, 2, 3, 5]
    assert [i for i, k in enumerate(K.BATCH_NONE) if K.FULL_IMAGE[k] >= 80] == [0, 2, 5]


def test_smallest_mesh_is_the_lower_bound():
    """n_samples = 4 is the smallest mesh the device accepts, and the oracle's fit is regular on it (no LinAlgError): the test of
    test_mesh_size_scenarios covers it; below it the 27 samples are fewer than the 39 unknowns"""
    assert K.SMALLEST_N == 4 and 3 ** 3 < 39 <= K.SMALLEST_N ** 3


def test_eta_of_the_yardstick_on_every_edge_size():
    """numpy.linalg.solve on the float64 normal equations, the yardstick of the device's backward error, is itself below
    ETA_SOLVE_MAX on every (case, n, axis), unweighted and in the first re-weighted pass: the cap of the GPU test cannot hide a
    failure behind a bad reference."""
    import os

    g = np.load(os.path.join(cases.GOLDEN, "rpcfit.npz"))
    worst = 0.0
    for name in K.GOLDEN_FITS:
        for n in K.EDGE_N:
            t, x = K.subset(g, name, n)
            assert t.shape == (min(n, len(g[name + "_target"])), 2) and x.shape == (t.shape[0], 3)
            for M, b in K.design_matrices(t, x, K.scaling_table(t, x)):
                s0 = K.solve_float64(M, b)
                e0 = K.backward_error(M, b, s0)
                w = K.weights(M, s0)
                e1 = K.backward_error(M, b, K.solve_float64(M, b, w, 1e-3), w, 1e-3)
                worst = max(worst, e0, e1)
                assert e0 < K.ETA_SOLVE_MAX and e1 < K.ETA_SOLVE_MAX, (name, n, e0, e1)
    print("largest eta of numpy.linalg.solve: {:.2e}".format(worst))

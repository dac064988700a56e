"""
Cases of the geographic side of the pairwise matching (satba.ft_match.utm_filter, keypoints_to_utm_coords_batch), shared by the host
test (test_utm_host.py), which runs the kernels' own arithmetic compiled for the CPU, and the GPU tests (test_gpu_utm.py).  numpy
only (the truth of the projection needs mpmath, imported where it is used).

Filter cases are lists of pairs with chosen curves of distances.  A match's first keypoint sits at integer UTM coordinates and its
second one at an offset with few fractional bits, along an axis or along a 3-4-5 triangle, so that the subtraction, the squares and
the root are exact and the distance is the chosen number (`exact` cases; the random curves need no exactness: device and host read
the same coordinates).
"""
import functools

import numpy as np

from satba import ft_match, geo_utils
from satba.ba_outliers import get_elbow_value

MARGIN = 5.0  # ref:ft_match.py:246
SIZES = (0, 1, 2, 3, 255, 256, 257, 5000)  # either side of a workgroup's stride and of the segmented sort's small / large segments

# the curve of the issue: elbow 6, success, thr = 11: 41 of 43 kept, 11 == thr kept, 50 and 60 dropped
L_CURVE = [5.0] * 30 + [6.0] * 9 + [10.0, 11.0, 50.0, 60.0]
# ... and with a match a quarter of a metre above the threshold (same elbow: 41 of 44)
L_CURVE_JUST_ABOVE = [5.0] * 30 + [6.0] * 9 + [10.0, 11.0, 11.25, 50.0, 60.0]
CURVES = {
    "two_points": [1.0, 9.0],                 # both distances to the chord are rounding noise: numpy's elbow is 9, not 1
    "equal": [7.0] * 10,
    "zero": [0.0] * 10,
    "one_zero": [0.0],
    "one": [3.0],
    "tent": [0.0, 0.0, 0.0, 0.0, 10.0, 10.0, 10.0, 10.0],  # (3, 0) and (4, 10) mirror each other across the chord: the first wins
    "L": L_CURVE,
    "L_just_above": L_CURVE_JUST_ABOVE,
    "concave": [0.0, 10.0, 20.0, 30.0, 40.0, 41.0, 42.0, 43.0, 44.0, 45.0, 46.0],  # the elbow (40) is below the percentile: all kept
    "ramp": [0.25 * k for k in range(50)],    # uniform: every point lies on the chord, rounding picks the elbow
    "elbow_is_percentile": [0.0, 0.0, 0.0, 0.0, 1.0, 100.0],  # n = 6: the 80th percentile is v[4], and v[4] is the elbow
}


def _plateau(n):
    """a stretch parallel to the chord (tests/cases_outliers.py `_plateau`, in quarter metres): its points are equally far from the
    chord and only rounding and the index order tell the maxima apart"""
    v = np.zeros(n)
    a, b = int(0.85 * n), int(0.95 * n)
    s = 0.25
    v[:a] = np.floor(np.linspace(0.0, 4.0 * (s * a - 20.0), a)) / 4.0
    v[a:b] = s * np.arange(a, b) - 20.0
    v[b:] = np.rint(4.0 * np.linspace(v[b - 1] + 0.25, s * (n - 1), n - b)) / 4.0
    return np.sort(np.maximum(v, 0.0))


def _l_random(rng, n):
    """most matches within a few metres, one in ten tens of metres off, in quarter metres, unsorted"""
    return np.rint(4.0 * (rng.uniform(0.0, 8.0, n) + (rng.random(n) < 0.1) * rng.uniform(30.0, 200.0, n))) / 4.0


def coords(d, rng, exact=True):
    """utm4 (n, 4) whose distances are d: the first keypoint on the integer grid, the second one off by d along an axis, or along a
    3-4-5 triangle where d / 5 has few fractional bits"""
    d = np.asarray(d, dtype=np.float64)
    n = d.size
    p = np.stack([rng.integers(300000, 700000, n), rng.integers(1000000, 5000000, n)], axis=1).astype(np.float64)
    off = np.zeros((n, 2))
    t = d / 5.0
    tri = (t * 5.0 == d) & (np.rint(t * 1024.0) == t * 1024.0)
    axis = rng.integers(0, 2, n)
    off[np.arange(n), axis] = d
    swap = rng.integers(0, 2, n).astype(bool)
    off[tri] = np.where(swap[tri, None], np.stack([3.0 * t[tri], 4.0 * t[tri]], axis=1), np.stack([4.0 * t[tri], 3.0 * t[tri]], axis=1))
    off *= rng.choice([-1.0, 1.0], (n, 2))
    utm4 = np.concatenate([p, p - off], axis=1)
    if exact:
        assert np.array_equal(np.linalg.norm(utm4[:, :2] - utm4[:, 2:], axis=1), d)
    return utm4


def _case(curves, alive=None, shuffle=True, seed=0, margin=MARGIN):
    """pairs from their curves (one array of distances each); alive: None or one mask (or None) per pair"""
    rng = np.random.default_rng([41, seed])
    ofs, rows, masks = [0], [], []
    for k, d in enumerate(curves):
        d = np.asarray(d, dtype=np.float64)
        order = rng.permutation(d.size) if shuffle else np.arange(d.size)
        rows.append(coords(d[order], rng))
        a = None if alive is None else alive[k]
        masks.append(np.ones(d.size, dtype=bool) if a is None else np.asarray(a, dtype=bool)[order])
        ofs.append(ofs[-1] + d.size)
    return dict(pair_ofs=np.array(ofs, dtype=np.int64), utm4=np.concatenate(rows, axis=0).reshape(-1, 4),
                alive=None if alive is None else np.concatenate(masks), margin=margin)


@functools.lru_cache(maxsize=None)
def filter_cases():
    rng = np.random.default_rng([41, 99])
    cases = {}
    cases["curves"] = _case(list(CURVES.values()))
    cases["curves_in_order"] = _case(list(CURVES.values()), shuffle=False, seed=1)
    cases["sizes_L"] = _case([_l_random(rng, n) for n in SIZES], seed=2)
    cases["sizes_equal"] = _case([np.full(n, 12.5) for n in SIZES], seed=3)
    cases["sizes_ramp"] = _case([0.25 * np.arange(n) for n in SIZES], seed=4)
    cases["plateaus"] = _case([_plateau(n) for n in (255, 256, 257, 5000)], seed=5)
    cases["one_pair"] = _case([L_CURVE], seed=6)
    cases["empty_pairs"] = _case([[], [], L_CURVE, [], [1.0, 9.0], []], seed=7)
    # alive patterns over the L curve (43 matches; above its elbow: 10, 11, 50, 60), and over the sizes
    L = np.array(L_CURVE)
    one = np.zeros(L.size, dtype=bool)
    one[17] = True
    patterns = [np.ones(L.size, dtype=bool), np.zeros(L.size, dtype=bool), one, np.arange(L.size) % 2 == 0, L <= 6.0]
    cases["alive_patterns"] = _case([L_CURVE] * len(patterns), alive=patterns, seed=8)
    cases["alive_alternating_sizes"] = _case([_l_random(rng, n) for n in SIZES], alive=[np.arange(n) % 2 == 1 for n in SIZES], seed=9)
    cases["alive_random_sizes"] = _case([_l_random(rng, n) for n in SIZES], alive=[rng.random(n) < 0.7 for n in SIZES], seed=10)
    cases["alive_none_at_all"] = _case([_l_random(rng, n) for n in (3, 257)], alive=[np.zeros(n, dtype=bool) for n in (3, 257)], seed=11)
    # a dead match may hold anything: it is not read
    c = _case([L_CURVE, [1.0, 9.0]], alive=[L <= 11.0, [True, True]], shuffle=False, seed=12)
    c["utm4"][np.where(~c["alive"])[0][0]] = np.nan
    cases["dead_match_not_finite"] = c
    cases["margin_quarter"] = _case([L_CURVE_JUST_ABOVE, _l_random(rng, 257)], seed=13, margin=0.25)
    return cases


def filter_reference(case):
    """(keep, thr, n_kept): `filter_matches_inconsistent_utm_coords` pair by pair on the alive subset; the threshold restates its
    three lines (they return no threshold), and the rows it keeps are checked against it"""
    ofs, utm4, alive = case["pair_ofs"], case["utm4"], case["alive"]
    n_pairs = len(ofs) - 1
    keep, thr, n_kept = np.zeros(len(utm4), dtype=bool), np.full(n_pairs, np.nan), np.zeros(n_pairs, dtype=np.int64)
    for p in range(n_pairs):
        idx = np.arange(ofs[p], ofs[p + 1])
        if alive is not None:
            idx = idx[alive[idx]]
        if not idx.size:
            continue
        u_i, u_j = utm4[idx, :2], utm4[idx, 2:]
        d = np.linalg.norm(u_i - u_j, axis=1)
        elbow, success = get_elbow_value(d, max_outliers_percent=20)
        thr[p] = elbow + case["margin"] if success else np.max(d)
        kept = idx[d <= thr[p]]
        if case["margin"] == MARGIN:
            m = np.stack([np.arange(idx.size)] * 2, axis=1)
            assert np.array_equal(idx[ft_match.filter_matches_inconsistent_utm_coords(m, u_i, u_j)[:, 0]], kept)
        keep[kept] = True
        n_kept[p] = kept.size
    return keep, thr, n_kept


def bad_filter_arguments():
    """keyword arguments of ft_match.utm_filter that must raise ValueError (n >= 2^31 is tested on the C entry: no array that large)"""
    c = filter_cases()["one_pair"]
    ok = dict(pair_ofs=c["pair_ofs"], utm4=c["utm4"])
    n = len(c["utm4"])
    bad = {}
    for name, v in (("nan", np.nan), ("inf", np.inf), ("minus_inf", -np.inf)):
        for col in range(4):
            u = c["utm4"].copy()
            u[5, col] = v
            bad["coordinate_{}_{}".format(name, col)] = dict(ok, utm4=u)
    u = c["utm4"].copy()
    u[5, 0] = np.nan
    alive = np.zeros(n, dtype=bool)
    alive[5] = True
    bad["coordinate_nan_only_alive"] = dict(ok, utm4=u, alive=alive)
    bad["pair_ofs_decreases"] = dict(ok, pair_ofs=[0, 30, 20, n])
    bad["pair_ofs_starts_late"] = dict(ok, pair_ofs=[3, n])
    bad["pair_ofs_negative_start"] = dict(ok, pair_ofs=[-1, n])
    bad["pair_ofs_ends_early"] = dict(ok, pair_ofs=[0, n - 1])
    bad["alive_short"] = dict(ok, alive=np.ones(n - 1, dtype=bool))
    for name, v in (("negative", -1.0), ("nan", np.nan), ("inf", np.inf)):
        bad["margin_" + name] = dict(ok, margin=v)
    return bad


# ---------------------------------------------------------------------------------------------------- keypoints to UTM
KP_SIZES = (0, 1, 64, 65, 257, 5000)  # either side of the kernels' block of 64 lanes, more than one block, many blocks


def _features(rng, rpc, n_kp, pad=0):
    """(n_kp + pad, 132) float32: keypoints in quarter pixels over the image of the RPC, `pad` NaN rows behind"""
    f = np.zeros((n_kp + pad, 132), dtype=np.float32)
    f[:n_kp, 0] = rng.integers(0, int(8 * rpc.col_offset), n_kp) / 4.0
    f[:n_kp, 1] = rng.integers(0, int(8 * rpc.row_offset), n_kp) / 4.0
    f[:n_kp, 2:] = rng.random((n_kp, 130))
    f[n_kp:] = np.nan
    return f


def straddling_rpc(r):
    """the RPC moved along its parallel until its centre lies on the meridian 72 W, between the zones 18 and 19"""
    import cases_octants as CO

    return CO.moved_rpc(r, -72.0 - r.lon_offset, False)


@functools.lru_cache(maxsize=None)
def kp_cases():
    """name -> dict(features, rpcs, offsets, alts, zone)"""
    import cases_octants as CO

    rng = np.random.default_rng([43, 7])
    shipped = CO.rpcs(*CO.ORIGINAL)
    cases = {}

    def case(rpcs, sizes, pads=None, zone=None, offsets=None, alts=None):
        pads = pads or [0] * len(rpcs)
        return dict(features=[_features(rng, r, n, p) for r, n, p in zip(rpcs, sizes, pads)], rpcs=list(rpcs),
                    offsets=offsets or [{"col0": 0.0, "row0": 0.0}] * len(rpcs),
                    alts=alts if alts is not None else [r.alt_offset for r in rpcs], zone=zone)

    cases["sizes"] = case([shipped[k % 2] for k in range(len(KP_SIZES))], KP_SIZES)
    cases["padded"] = case([shipped[0], shipped[1], shipped[0]], [0, 100, 64], pads=[7, 13, 1],
                           offsets=[{"col0": 0.0, "row0": 0.0}, {"col0": 100.0, "row0": 50.0}, {"col0": -20.5, "row0": 300.25}], alts=30.0)
    moved = [r for placement in CO.PLACEMENTS for r in CO.rpcs(*placement)]
    cases["octants"] = case(moved, [65] * len(moved))
    zone = geo_utils.utm_zone_from_lonlat(shipped[0].lon_offset, shipped[0].lat_offset)
    cases["shared_zone"] = case(shipped, [65, 33], zone=zone)
    cases["neighbour_zone"] = case(shipped, [65, 33], zone=zone + 1)
    cases["straddle"] = case([straddling_rpc(r) for r in shipped], [257, 65])
    return cases


def lonlat_samples():
    """(lon, lat, zone) float64 / int arrays for the host test, which cannot localise: points over the footprints of the RPCs of
    kp_cases() -- the shipped ones in all eight placements and the ones on the zone's edge --, in the zone the batch would pick
    (that of an image's first point) and, for the shipped pair, the neighbouring zone"""
    import cases_octants as CO

    rng = np.random.default_rng([43, 8])
    lon, lat, zone = [], [], []
    shipped = CO.rpcs(*CO.ORIGINAL)
    groups = [(r, 0) for placement in CO.PLACEMENTS for r in CO.rpcs(*placement)] + [(straddling_rpc(r), 0) for r in shipped] + [(r, 1) for r in shipped]
    for r, dz in groups:
        lo = r.lon_offset + r.lon_scale * rng.uniform(-1.0, 1.0, 150)
        la = r.lat_offset + r.lat_scale * rng.uniform(-1.0, 1.0, 150)
        z = (geo_utils.utm_zone_from_lonlat(lo[0], la[0]) - 1 + dz) % 60 + 1
        lon.append(lo); lat.append(la); zone.append(np.full(150, z))
    return np.concatenate(lon), np.concatenate(lat), np.concatenate(zone)


def utm_truth(lon, lat, zone, dps=40):
    """(east, north) float64, rounded once from an evaluation of the series of geo_utils.utm_from_lonlat with `dps` digits: the same
    truncation (to n^4), so that what is measured against it is rounding alone.  cos, sin, cosh, sinh of the multiples of xi and eta
    come from those of 2 xi and 2 eta by the addition theorems (exact identities: another evaluation of the same terms)"""
    import mpmath as mp

    lon, lat, zone = np.broadcast_arrays(np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64), np.asarray(zone))
    east, north = np.zeros(lon.shape), np.zeros(lon.shape)
    with mp.workdps(dps):
        f = 1 / mp.mpf("298.257223563")
        n = f / (2 - f)
        A = mp.mpf(6378137) / (1 + n) * (1 + n ** 2 / 4 + n ** 4 / 64)
        al = [n / 2 - 2 * n ** 2 / 3 + 5 * n ** 3 / 16 + 41 * n ** 4 / 180, 13 * n ** 2 / 48 - 3 * n ** 3 / 5 + 557 * n ** 4 / 1440,
              61 * n ** 3 / 240 - 103 * n ** 4 / 140, 49561 * n ** 4 / 161280]
        e = mp.sqrt(f * (2 - f))
        k0A = mp.mpf("0.9996") * A
        rad = mp.pi / 180
        for k in np.ndindex(lon.shape):
            phi, dl = mp.mpf(float(lat[k])) * rad, (mp.mpf(float(lon[k])) - (6 * int(zone[k]) - 183)) * rad
            sp = mp.sin(phi)
            t = mp.sinh(mp.atanh(sp) - e * mp.atanh(e * sp))
            xi = mp.atan2(t, mp.cos(dl))
            eta = mp.atanh(mp.sin(dl) / mp.sqrt(1 + t * t))
            c1, s1 = mp.cos_sin(2 * xi)
            ex = mp.exp(2 * eta)
            ch1, sh1 = (ex + 1 / ex) / 2, (ex - 1 / ex) / 2
            c, s, ch, sh = c1, s1, ch1, sh1
            x, y = eta, xi
            for a in al:
                x += a * c * sh
                y += a * s * ch
                c, s = c * c1 - s * s1, s * c1 + c * s1
                ch, sh = ch * ch1 + sh * sh1, sh * ch1 + ch * sh1
            east[k], north[k] = float(500000 + k0A * x), float(k0A * y)
    return east, north


def band():
    """the tolerance of the projection [m]: 8 x e_host as profiles/ft_utm.json records it (tools/time_utm.py measures it,
    test_utm_host.py holds the file to the measurement)"""
    import json
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return float(json.load(open(os.path.join(root, "profiles", "ft_utm.json")))["rounding"]["band_m"])


def host_rounding(lon=None, lat=None, zone=None):
    """e_host: the largest absolute error [m] of geo_utils.utm_from_lonlat against the truth over lonlat_samples()"""
    if lon is None:
        lon, lat, zone = lonlat_samples()
    te, tn = utm_truth(lon, lat, zone)
    worst = 0.0
    for z in np.unique(zone):
        m = zone == z
        e, n = geo_utils.utm_from_lonlat(lon[m], lat[m], zone=int(z))
        worst = max(worst, float(np.abs(e - te[m]).max()), float(np.abs(n - tn[m]).max()))
    return worst

"""
The geographic side of the pairwise matching on the device: satba.ft_match.utm_filter (satba_utm_filter) against
`filter_matches_inconsistent_utm_coords` pair by pair, exactly, and keypoints_to_utm_coords_batch (satba_keypoints_utm) against the
localisation of RPCModel.localization, bit for bit, and the mpmath truth of the projection on the kernel's own (lon, lat), within
the band of profiles/ft_utm.json (8 x the rounding of the numpy restatement; tests/test_utm_host.py holds the file to its
measurement).  The cases are those of tests/cases_utm.py.
"""
import ctypes as ct
import functools

import numpy as np
import pytest

import cases_utm as U
from satba import engine_hip as E
from satba import ft_match, geo_utils

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(U.filter_cases()))
def test_filter_equals_the_reference_pair_by_pair(gpu, name):
    case = U.filter_cases()[name]
    keep, info = ft_match.utm_filter(case["pair_ofs"], case["utm4"], case["alive"], margin=case["margin"], return_info=True)
    want = U.filter_reference(case)
    assert keep.dtype == bool and np.array_equal(keep, want[0])
    assert np.array_equal(info["thr"], want[1], equal_nan=True)
    assert info["n_kept"].dtype == np.int64 and np.array_equal(info["n_kept"], want[2])
    assert info["kernel_ms"] > 0 or len(case["utm4"]) == 0
    assert np.array_equal(ft_match.utm_filter(case["pair_ofs"], case["utm4"], case["alive"], margin=case["margin"]), keep)
    if case["alive"] is None:  # a mask of ones is no mask
        assert np.array_equal(ft_match.utm_filter(case["pair_ofs"], case["utm4"], np.ones(len(keep), dtype=np.uint8), margin=case["margin"]), keep)


def test_filter_without_matches(gpu):
    keep, info = ft_match.utm_filter([0], np.zeros((0, 4)), return_info=True)
    assert keep.shape == (0,) and info["thr"].shape == (0,) and info["n_kept"].shape == (0,)
    keep, info = ft_match.utm_filter([0, 0, 0], np.zeros((0, 4)), return_info=True)
    assert keep.shape == (0,) and np.isnan(info["thr"]).all() and info["n_kept"].tolist() == [0, 0]


@pytest.mark.parametrize("name", list(U.bad_filter_arguments()))
def test_bad_filter_arguments_raise(gpu, name):
    with pytest.raises(ValueError):
        ft_match.utm_filter(**U.bad_filter_arguments()[name])


def test_too_many_matches_is_an_argument_error(gpu):
    """n >= 2^31 is refused before an array is read (none that large is made here): the C entry, with nothing behind its pointers"""
    lib = E.load_library()
    ofs = np.array([0, 2 ** 31], dtype=np.int64)
    rc = lib.satba_utm_filter(1, ofs.ctypes.data_as(ct.POINTER(ct.c_int64)), None, None, 5.0, None, None, None, 0, None)
    with pytest.raises(ValueError, match="2\\^31"):
        E._check(lib, rc)
    ofs[1] = 2 ** 40
    with pytest.raises(ValueError):
        E._check(lib, lib.satba_utm_filter(1, ofs.ctypes.data_as(ct.POINTER(ct.c_int64)), None, None, 5.0, None, None, None, 0, None))


# ---------------------------------------------------------------------------------------------------- keypoints to UTM
@functools.lru_cache(maxsize=None)
def batch(name):
    """(utm, lonlat, kernel_ms) of a case, one device call"""
    c = U.kp_cases()[name]
    utm, lonlat, info = ft_match.keypoints_to_utm_coords_batch(c["features"], c["rpcs"], c["offsets"], c["alts"], zone=c["zone"], return_lonlat=True,
                                                               return_info=True)
    return utm, lonlat, info["kernel_ms"]


def _n_kp(f):
    return int(np.sum(~np.isnan(f[:, 0])))


def _alts(c):
    return np.broadcast_to(np.asarray(c["alts"], dtype=np.float64), (len(c["features"]),))


@pytest.mark.parametrize("name", list(U.kp_cases()))
def test_localisation_is_rpc_localization_bit_for_bit(gpu, name):
    c = U.kp_cases()[name]
    utm, lonlat, ms = batch(name)
    assert len(utm) == len(lonlat) == len(c["features"]) and ms > 0
    for f, r, o, a, u, ll in zip(c["features"], c["rpcs"], c["offsets"], _alts(c), utm, lonlat):
        n = _n_kp(f)
        assert u.shape == ll.shape == (len(f), 2) and u.dtype == ll.dtype == np.float64
        if n:
            lon, lat = r.localization(f[:n, 0].astype(np.float64) + o["col0"], f[:n, 1].astype(np.float64) + o["row0"], np.full(n, float(a)))
            assert np.array_equal(ll[:n, 0], lon) and np.array_equal(ll[:n, 1], lat)
        # the rows behind the keypoints come back as the reference leaves them: their two columns, here NaN
        assert np.array_equal(u[n:], f[n:, :2].astype(np.float64), equal_nan=True) and np.isnan(u[n:]).all()
        assert np.array_equal(ll[n:], f[n:, :2].astype(np.float64), equal_nan=True)


@pytest.mark.parametrize("name", list(U.kp_cases()))
def test_projection_lies_within_the_band_of_the_truth(gpu, name):
    """the mpmath truth on the kernel's own (lon, lat), in the zone the kernel had to take"""
    c = U.kp_cases()[name]
    utm, lonlat, _ = batch(name)
    lon, lat, zone, got = [], [], [], []
    for f, u, ll in zip(c["features"], utm, lonlat):
        n = _n_kp(f)
        if n:
            z = c["zone"] if c["zone"] is not None else geo_utils.utm_zone_from_lonlat(ll[0, 0], ll[0, 1])
            lon.append(ll[:n, 0]); lat.append(ll[:n, 1]); zone.append(np.full(n, z)); got.append(u[:n])
    lon, lat, zone, got = np.concatenate(lon), np.concatenate(lat), np.concatenate(zone), np.concatenate(got)
    assert np.isfinite(got).all()
    te, tn = U.utm_truth(lon, lat, zone)
    worst = max(np.abs(got[:, 0] - te).max(), np.abs(got[:, 1] - tn).max())
    print("{}: {} keypoints, worst distance to the truth {:.6e} m (band {:.6e} m)".format(name, len(lon), worst, U.band()))
    assert worst <= U.band()
    if name == "octants":  # both hemispheres (southern northings negative) and both signs of longitude
        assert (got[:, 1] < 0).any() and (got[:, 1] > 0).any() and (lon < 0).any() and (lon > 0).any() and len(np.unique(zone)) >= 4
    if name == "straddle":  # keypoints on both sides of the meridian 72 W, all in the zone of the image's first one
        own = np.array([geo_utils.utm_zone_from_lonlat(v, 0.0) for v in lon])
        assert set(own.tolist()) == {18, 19} and (own != zone).any()
        east = got[own != zone, 0]  # beyond the zone's edge: 3 degrees of longitude at 11 N are 327.7 km
        assert ((east < 173000.0) | (east > 827000.0)).all()


def test_zone_none_against_an_explicit_zone(gpu):
    """what test_keypoints_to_utm_coords_keeps_the_padding expects of the single-image function, of the batch: zone=None is the zone
    of each image's first keypoint, another zone gives other coordinates; and the batch agrees with the single-image function"""
    c = U.kp_cases()["padded"]
    utm, lonlat, _ = batch("padded")
    zones = [geo_utils.utm_zone_from_lonlat(ll[0, 0], ll[0, 1]) for f, ll in zip(c["features"], lonlat) if _n_kp(f)]
    assert len(set(zones)) == 1
    same = ft_match.keypoints_to_utm_coords_batch(c["features"], c["rpcs"], c["offsets"], c["alts"], zone=zones[0])
    other = ft_match.keypoints_to_utm_coords_batch(c["features"], c["rpcs"], c["offsets"], c["alts"], zone=zones[0] + 1)
    per_image = ft_match.keypoints_to_utm_coords_batch(c["features"], c["rpcs"], c["offsets"], c["alts"], zone=[zones[0]] * len(utm))
    for f, r, o, a, u, s, x, p in zip(c["features"], c["rpcs"], c["offsets"], _alts(c), utm, same, other, per_image):
        n = _n_kp(f)
        assert np.array_equal(u, s, equal_nan=True) and np.array_equal(u, p, equal_nan=True)
        assert np.array_equal(np.isnan(u), np.isnan(x)) and (n == 0 or not np.array_equal(u[:n], x[:n]))
        single = ft_match.keypoints_to_utm_coords(f, r, o, a)
        assert np.array_equal(np.isnan(single), np.isnan(u)) and (n == 0 or np.abs(single[:n] - u[:n]).max() <= U.band() + U.band() / 8)
    # the explicit zones of the cases were taken: the neighbouring zone moves the eastings by hundreds of kilometres
    a, b = batch("shared_zone")[0], batch("neighbour_zone")[0]
    assert all(np.abs(x[:, 0] - y[:, 0]).min() > 1e5 for x, y in zip(a, b))


def test_bad_keypoint_arguments_raise(gpu):
    c = U.kp_cases()["shared_zone"]
    ok = dict(features=c["features"], rpcs=c["rpcs"], offsets=c["offsets"], alts=c["alts"])
    assert len(ft_match.keypoints_to_utm_coords_batch([], [], [], [])) == 0
    for bad in (dict(ok, zone=0), dict(ok, zone=61), dict(ok, zone=-3), dict(ok, alts=np.nan), dict(ok, alts=[30.0, np.inf]),
                dict(ok, offsets=[{"col0": np.nan, "row0": 0.0}] * 2), dict(ok, rpcs=c["rpcs"][:1]), dict(ok, features=[f[:, :100] for f in c["features"]])):
        with pytest.raises(ValueError):
            ft_match.keypoints_to_utm_coords_batch(**bad)

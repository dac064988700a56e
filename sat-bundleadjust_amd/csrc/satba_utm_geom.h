// Geographic coordinates to UTM: the Krueger n-series of the transverse Mercator projection to n^4, term for
// term what satba/geo_utils.py:utm_from_lonlat evaluates in numpy -- k0 = 0.9996, false easting 500 000 m, no false northing
// (southern northings are negative), the zones of the standard 6-degree grid without the Norway / Svalbard exceptions.  Plain C++17
// in float64 that compiles on the host on its own (tests/host/utm_dump.cpp); k_kp_project of satba_utm.h runs the same function.
#pragma once
#include <cmath>
#include <cstdint>

#include "satba_elbow.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define UTM_HD __host__ __device__ inline
#else
#define UTM_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define UTM_SQRT_RN(x) __dsqrt_rn(x)
#else
#define UTM_SQRT_RN(x) std::sqrt(x)
#endif

constexpr double UTM_WGS84_A = 6378137.0;
constexpr double UTM_WGS84_FINV = 298.257223563;
constexpr double UTM_K0 = 0.9996;
constexpr double UTM_FALSE_EASTING = 500000.0;
constexpr double UTM_DEG = 3.141592653589793 / 180.0;  // numpy's deg2rad multiplies by this constant

// distance on the ground between the two keypoints of a match, row = (east_i, north_i, east_j, north_j), as
// np.linalg.norm(utm_i - utm_j, axis=1) rounds it: two squares, one sum, one root, nothing fused (the UTM filter is index-exact)
UTM_HD double utm_distance(const double* row) {
#pragma clang fp contract(off)
    const double dx = row[0] - row[2], dy = row[1] - row[3];
    const double xx = dx * dx, yy = dy * dy;
    return UTM_SQRT_RN(xx + yy);
}

// the UTM filter's last step on the elbow of a pair's sorted distances (ref:feature_tracks/ft_match.py:245-246)
UTM_HD double utm_threshold(const satba::Elbow& e, double margin) { return e.success ? e.elbow + margin : e.last; }

// geo_utils.utm_zone_from_lonlat: 1..60 for every finite longitude (Python's % is never negative)
UTM_HD int utm_zone(double lon_deg) {
    const long long z = (long long)std::floor((lon_deg + 180.0) / 6.0);
    return (int)(((z % 60) + 60) % 60) + 1;
}

// (lon, lat) in degrees -> (easting, northing) in metres in the given zone
UTM_HD void utm_project(double lon_deg, double lat_deg, int zone, double& east, double& north) {
    const double lam0 = (6.0 * zone - 183.0) * UTM_DEG;
    const double f = 1.0 / UTM_WGS84_FINV;
    const double n = f / (2.0 - f);
    const double n2 = n * n, n3 = n2 * n, n4 = n2 * n2;
    const double A = UTM_WGS84_A / (1.0 + n) * (1.0 + n2 / 4.0 + n4 / 64.0);
    const double al[4] = {n / 2.0 - 2.0 * n2 / 3.0 + 5.0 * n3 / 16.0 + 41.0 * n4 / 180.0,
                          13.0 * n2 / 48.0 - 3.0 * n3 / 5.0 + 557.0 * n4 / 1440.0,
                          61.0 * n3 / 240.0 - 103.0 * n4 / 140.0,
                          49561.0 * n4 / 161280.0};
    const double phi = lat_deg * UTM_DEG, lam = lon_deg * UTM_DEG;
    const double e = std::sqrt(f * (2.0 - f));
    const double sp = std::sin(phi);
    const double t = std::sinh(std::atanh(sp) - e * std::atanh(e * sp));
    const double dl = lam - lam0;
    const double xi = std::atan2(t, std::cos(dl));
    const double eta = std::atanh(std::sin(dl) / std::sqrt(1.0 + t * t));
    double x = eta, y = xi;
    for (int j = 1; j <= 4; ++j) {
        const double a = al[j - 1], w = 2.0 * j;
        x += a * std::cos(w * xi) * std::sinh(w * eta);
        y += a * std::sin(w * xi) * std::cosh(w * eta);
    }
    east = UTM_FALSE_EASTING + UTM_K0 * A * x;
    north = UTM_K0 * A * y;
}

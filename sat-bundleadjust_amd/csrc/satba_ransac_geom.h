// Geometry of the fundamental-matrix RANSAC (the rule is stated in include/satba.h, satba_ransac_fundamental):
// the counter-based sampler, Hartley's normalisation, the seven-point solver and the error of a match under a matrix.  Plain C++17
// in float64 that compiles on the host on its own (tests/host/ransac_geom_dump.cpp); the kernels of satba_ransac.h run the same
// functions.  Every array below is indexed by loop counters whose bounds are constants, so that a device compiler that unrolls
// the loops keeps the 7 x 9 block in registers: no loop here has a bound that depends on the data, except the 64 draws of a sample.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RSC_HD __host__ __device__ inline
#define RSC_UNROLL _Pragma("unroll")
#else
#define RSC_HD inline
#define RSC_UNROLL
#endif

constexpr int RSC_MIN_MATCHES = 7;    // ref:bundle_adjust/s2p/sift.py:181
constexpr int RSC_MAX_DRAWS = 64;     // draws of one trial
constexpr int RSC_NEWTON_STEPS = 4;   // on every root of the cubic
constexpr uint64_t RSC_GOLDEN = 0x9E3779B97F4A7C15ull;

// ---------------------------------------------------------------------------------------------------- sampling
RSC_HD uint64_t rsc_splitmix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// draw k of trial t of pair p: an index below m
RSC_HD int64_t rsc_draw(uint64_t seed, uint64_t p, uint64_t n_trials, uint64_t t, uint64_t k, uint64_t m) {
    const uint64_t z = rsc_splitmix64(seed + RSC_GOLDEN * (1ull + ((p * n_trials + t) * 64ull + k)));
    return (int64_t)(((z >> 32) * m) >> 32);
}

struct RscSample {
    int64_t i[7];
};

// seven distinct indices below m, in the order drawn; false after RSC_MAX_DRAWS draws without them
RSC_HD bool rsc_sample(uint64_t seed, uint64_t p, uint64_t n_trials, uint64_t t, uint64_t m, RscSample* s) {
    int found = 0;
    RSC_UNROLL
    for (int j = 0; j < 7; ++j) s->i[j] = -1;
    for (int k = 0; k < RSC_MAX_DRAWS && found < 7; ++k) {
        const int64_t v = rsc_draw(seed, p, n_trials, t, (uint64_t)k, m);
        bool seen = false;
        RSC_UNROLL
        for (int j = 0; j < 7; ++j) seen = seen || s->i[j] == v;  // the slots not yet filled hold -1
        if (seen) continue;
        RSC_UNROLL
        for (int j = 0; j < 7; ++j)
            if (j == found) s->i[j] = v;
        ++found;
    }
    return found == 7;
}

RSC_HD uint64_t rsc_bits(double v) {
    uint64_t u;
    __builtin_memcpy(&u, &v, sizeof u);
    return u;
}

// rows of a sample as (x1, y1, x2, y2); true when two rows share a bit-identical (x1, y1) or a bit-identical (x2, y2)
struct RscRows {
    double v[7][4];
};

RSC_HD bool rsc_rows_repeat(const RscRows& r) {
    bool rep = false;
    RSC_UNROLL
    for (int a = 0; a < 7; ++a) {
        RSC_UNROLL
        for (int b = a + 1; b < 7; ++b) {
            rep = rep || (rsc_bits(r.v[a][0]) == rsc_bits(r.v[b][0]) && rsc_bits(r.v[a][1]) == rsc_bits(r.v[b][1]));
            rep = rep || (rsc_bits(r.v[a][2]) == rsc_bits(r.v[b][2]) && rsc_bits(r.v[a][3]) == rsc_bits(r.v[b][3]));
        }
    }
    return rep;
}

// ---------------------------------------------------------------------------------------------------- normalisation
// Hartley's, of one pair: T = (cx1, cy1, s1, cx2, cy2, s2), a point maps to ((x - cx) s, (y - cy) s).  Sums run over the matches in
// the caller's order.  false when a side's mean distance to its centroid is 0 (or the pair is empty).
inline bool rsc_normalise(const double* xy, int64_t m, double* T) {
    if (m <= 0) return false;
    for (int side = 0; side < 2; ++side) {
        double sx = 0.0, sy = 0.0, sd = 0.0;
        for (int64_t i = 0; i < m; ++i) {
            sx += xy[4 * i + 2 * side];
            sy += xy[4 * i + 2 * side + 1];
        }
        const double cx = sx / (double)m, cy = sy / (double)m;
        for (int64_t i = 0; i < m; ++i) {
            const double dx = xy[4 * i + 2 * side] - cx, dy = xy[4 * i + 2 * side + 1] - cy;
            sd += std::sqrt(dx * dx + dy * dy);
        }
        const double mean = sd / (double)m;
        if (!(mean > 0.0)) return false;
        T[3 * side] = cx;
        T[3 * side + 1] = cy;
        T[3 * side + 2] = std::sqrt(2.0) / mean;
    }
    return true;
}

// ---------------------------------------------------------------------------------------------------- seven-point models
struct RscModels {
    int n;
    double F[3][9];
};

RSC_HD double rsc_det3(const double* a, const double* b, const double* c) {  // rows a, b, c
    return a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}

// Two vectors that span the null space of the 7 x 9 matrix A (destroyed): Gauss-Jordan elimination with full pivoting; the
// column order is kept in `perm`, every swap is a chain of selects over constant indices.  Each vector has unit length.
RSC_HD void rsc_null_space(double (&A)[7][9], double* f1, double* f2) {
    int perm[9];
    RSC_UNROLL
    for (int k = 0; k < 9; ++k) perm[k] = k;
    RSC_UNROLL
    for (int c = 0; c < 7; ++c) {
        int pr = c, pk = c;
        double best = -1.0;
        RSC_UNROLL
        for (int r = c; r < 7; ++r) {
            RSC_UNROLL
            for (int k = c; k < 9; ++k) {
                const double v = std::fabs(A[r][k]);
                if (v > best) { best = v; pr = r; pk = k; }
            }
        }
        RSC_UNROLL
        for (int r = c + 1; r < 7; ++r) {
            const bool sw = pr == r;
            RSC_UNROLL
            for (int k = 0; k < 9; ++k) {
                const double u = A[c][k], w = A[r][k];
                A[c][k] = sw ? w : u;
                A[r][k] = sw ? u : w;
            }
        }
        RSC_UNROLL
        for (int k = c + 1; k < 9; ++k) {
            const bool sw = pk == k;
            RSC_UNROLL
            for (int r = 0; r < 7; ++r) {
                const double u = A[r][c], w = A[r][k];
                A[r][c] = sw ? w : u;
                A[r][k] = sw ? u : w;
            }
            const int pu = perm[c], pw = perm[k];
            perm[c] = sw ? pw : pu;
            perm[k] = sw ? pu : pw;
        }
        const double inv = 1.0 / A[c][c];  // a rank-deficient sample gives non-finite vectors; rsc_seven_point drops them
        RSC_UNROLL
        for (int k = c; k < 9; ++k) A[c][k] *= inv;
        RSC_UNROLL
        for (int r = 0; r < 7; ++r) {
            if (r == c) continue;
            const double g = A[r][c];
            RSC_UNROLL
            for (int k = c; k < 9; ++k) A[r][k] -= g * A[c][k];
        }
    }
    // in the permuted order the null vectors are (-A[:, 7], 1, 0) and (-A[:, 8], 0, 1)
    double n1 = 1.0, n2 = 1.0;
    RSC_UNROLL
    for (int r = 0; r < 7; ++r) {
        n1 += A[r][7] * A[r][7];
        n2 += A[r][8] * A[r][8];
    }
    n1 = 1.0 / std::sqrt(n1);
    n2 = 1.0 / std::sqrt(n2);
    RSC_UNROLL
    for (int o = 0; o < 9; ++o) {
        double a = 0.0, b = 0.0;
        RSC_UNROLL
        for (int r = 0; r < 7; ++r) {
            a = perm[r] == o ? -A[r][7] : a;
            b = perm[r] == o ? -A[r][8] : b;
        }
        a = perm[7] == o ? 1.0 : a;
        b = perm[8] == o ? 1.0 : b;
        f1[o] = a * n1;
        f2[o] = b * n2;
    }
}

// real roots of c3 x^3 + c2 x^2 + c1 x + c0, 0 to 3 of them in `x`; the degree drops when the leading coefficient is below 1e-12
// of the largest.  The count comes from the sign of the discriminant; every root then takes RSC_NEWTON_STEPS Newton steps.
RSC_HD int rsc_real_roots(double c3, double c2, double c1, double c0, double* x) {
    const double big = std::fmax(std::fmax(std::fabs(c3), std::fabs(c2)), std::fmax(std::fabs(c1), std::fabs(c0)));
    int n = 0;
    if (!(big > 0.0) || !(big < INFINITY)) return 0;
    const double tiny = 1e-12 * big;
    if (std::fabs(c3) > tiny) {
        const double a = c2 / c3, b = c1 / c3, c = c0 / c3;
        const double p = b - a * a / 3.0, q = 2.0 * a * a * a / 27.0 - a * b / 3.0 + c;
        const double disc = 0.25 * q * q + p * p * p / 27.0;
        if (disc < 0.0) {  // p < 0
            const double m = 2.0 * std::sqrt(-p / 3.0);
            double arg = 3.0 * q / (p * m);
            arg = arg > 1.0 ? 1.0 : (arg < -1.0 ? -1.0 : arg);
            const double th = std::acos(arg) / 3.0;
            x[0] = m * std::cos(th) - a / 3.0;
            x[1] = m * std::cos(th - 2.0943951023931953) - a / 3.0;
            x[2] = m * std::cos(th - 4.1887902047863905) - a / 3.0;
            n = 3;
        } else {
            const double sq = std::sqrt(disc);
            const double u = q > 0.0 ? -std::cbrt(0.5 * q + sq) : std::cbrt(-0.5 * q + sq);
            x[0] = (u != 0.0 ? u - p / (3.0 * u) : 0.0) - a / 3.0;
            n = 1;
        }
    } else if (std::fabs(c2) > tiny) {
        const double disc = c1 * c1 - 4.0 * c2 * c0;
        if (disc >= 0.0) {
            const double s = -0.5 * (c1 + (c1 < 0.0 ? -std::sqrt(disc) : std::sqrt(disc)));
            x[0] = s / c2;
            x[1] = s != 0.0 ? c0 / s : x[0];
            n = 2;
        }
    } else if (std::fabs(c1) > tiny) {
        x[0] = -c0 / c1;
        n = 1;
    }
    RSC_UNROLL
    for (int r = 0; r < 3; ++r) {
        if (r < n) {
            double v = x[r];
            RSC_UNROLL
            for (int it = 0; it < RSC_NEWTON_STEPS; ++it) {
                const double f = ((c3 * v + c2) * v + c1) * v + c0, d = (3.0 * c3 * v + 2.0 * c2) * v + c1;
                const double step = f / d;
                v = (d != 0.0 && std::fabs(step) < INFINITY) ? v - step : v;
            }
            x[r] = v;
        }
    }
    return n;
}

// the models of seven matches (pixel coordinates) under the normalisation T of their pair: each denormalised, of unit Frobenius
// norm; a root whose matrix is not finite gives none
RSC_HD void rsc_seven_point(const RscRows& rows, const double* T, RscModels* out) {
    double A[7][9];
    RSC_UNROLL
    for (int r = 0; r < 7; ++r) {
        const double x1 = (rows.v[r][0] - T[0]) * T[2], y1 = (rows.v[r][1] - T[1]) * T[2];
        const double x2 = (rows.v[r][2] - T[3]) * T[5], y2 = (rows.v[r][3] - T[4]) * T[5];
        A[r][0] = x2 * x1; A[r][1] = x2 * y1; A[r][2] = x2;
        A[r][3] = y2 * x1; A[r][4] = y2 * y1; A[r][5] = y2;
        A[r][6] = x1; A[r][7] = y1; A[r][8] = 1.0;
    }
    double f1[9], f2[9], d[9];
    rsc_null_space(A, f1, f2);
    RSC_UNROLL
    for (int k = 0; k < 9; ++k) d[k] = f1[k] - f2[k];
    // det(f2 + x d)
    const double c0 = rsc_det3(f2, f2 + 3, f2 + 6), c3 = rsc_det3(d, d + 3, d + 6);
    const double c1 = rsc_det3(d, f2 + 3, f2 + 6) + rsc_det3(f2, d + 3, f2 + 6) + rsc_det3(f2, f2 + 3, d + 6);
    const double c2 = rsc_det3(d, d + 3, f2 + 6) + rsc_det3(d, f2 + 3, d + 6) + rsc_det3(f2, d + 3, d + 6);
    double x[3] = {0.0, 0.0, 0.0};
    const int n = rsc_real_roots(c3, c2, c1, c0, x);
    double H[3][9];
    bool ok[3];
    RSC_UNROLL
    for (int r = 0; r < 3; ++r) {
        double G[9];
        RSC_UNROLL
        for (int k = 0; k < 9; ++k) G[k] = f2[k] + x[r] * d[k];
        // T2^T G T1 with T = [[s, 0, -s cx], [0, s, -s cy], [0, 0, 1]]
        const double s1 = T[2], s2 = T[5], tx1 = -T[2] * T[0], ty1 = -T[2] * T[1], tx2 = -T[5] * T[3], ty2 = -T[5] * T[4];
        double B[9];  // G T1
        RSC_UNROLL
        for (int i = 0; i < 3; ++i) {
            B[3 * i] = G[3 * i] * s1;
            B[3 * i + 1] = G[3 * i + 1] * s1;
            B[3 * i + 2] = G[3 * i] * tx1 + G[3 * i + 1] * ty1 + G[3 * i + 2];
        }
        double nrm = 0.0;
        RSC_UNROLL
        for (int k = 0; k < 3; ++k) {
            H[r][k] = s2 * B[k];
            H[r][3 + k] = s2 * B[3 + k];
            H[r][6 + k] = tx2 * B[k] + ty2 * B[3 + k] + B[6 + k];
        }
        RSC_UNROLL
        for (int k = 0; k < 9; ++k) nrm += H[r][k] * H[r][k];
        const double inv = 1.0 / std::sqrt(nrm);
        ok[r] = r < n && nrm > 0.0 && inv < INFINITY && inv > 0.0;
        RSC_UNROLL
        for (int k = 0; k < 9; ++k) H[r][k] *= inv;
    }
    // the models that exist move to the front, in the order of their roots (selects on values: no indexed store)
    out->n = (ok[0] ? 1 : 0) + (ok[1] ? 1 : 0) + (ok[2] ? 1 : 0);
    RSC_UNROLL
    for (int k = 0; k < 9; ++k) {
        out->F[0][k] = ok[0] ? H[0][k] : (ok[1] ? H[1][k] : H[2][k]);
        out->F[1][k] = (ok[0] && ok[1]) ? H[1][k] : H[2][k];
        out->F[2][k] = H[2][k];
    }
}

// ---------------------------------------------------------------------------------------------------- error of a match
// ref:bundle_adjust/feature_tracks/ft_opencv.py:143-185: the larger of the two squared distances to the epipolar lines, every
// operation rounded on its own, in the reference's order.  A match is an inlier iff the value is below max_err^2 (NaN: never).
RSC_HD double rsc_error(const double* F, double x1, double y1, double x2, double y2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double a = F[0] * x1 + F[1] * y1 + F[2];
    double b = F[3] * x1 + F[4] * y1 + F[5];
    double c = F[6] * x1 + F[7] * y1 + F[8];
    const double s2 = 1.0 / (a * a + b * b);
    const double d2 = x2 * a + y2 * b + c;
    a = F[0] * x2 + F[3] * y2 + F[6];
    b = F[1] * x2 + F[4] * y2 + F[7];
    c = F[2] * x2 + F[5] * y2 + F[8];
    const double s1 = 1.0 / (a * a + b * b);
    const double d1 = x1 * a + y1 * b + c;
    const double e1 = d1 * d1 * s1, e2 = d2 * d2 * s2;
    return (e1 != e1 || e2 != e2) ? NAN : (e1 > e2 ? e1 : e2);
}

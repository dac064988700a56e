// satba_camapprox.h -- affine and perspective cameras from RPCs, the step that hands the solver its cameras and camera centres:
//   ref:bundle_adjust/cam_utils.py:146-174  affine_rpc_approx: first-order Taylor expansion of rpc.projection o ecef_to_latlon_custom at
//       an ECEF point (the reference differentiates with the `ad` package; k_cam_affine chains the two analytic Jacobians of
//       satba_models.h, which is the same derivative; the value is taken at the correctly rounded longitude, cam_atan2_rounded)
//   ref:bundle_adjust/cam_utils.py:177-198, 234-277  perspective_rpc_approx / approx_rpc_as_proj_matrix: a mesh over the crop and an
//       altitude range is localised through the RPC, taken to ECEF and resected
//   ref:bundle_adjust/cam_utils.py:309-445  camera_matrix (DLT with Hartley's normalisation), normalize_{2d,3d}_points
//
// k_cam_resect, one workgroup per camera: (a) mesh, localisation, ECEF; (b) centroids and mean distances of both point sets;
// (c) the 12 x 12 normal matrix A^T A of the reference's 2n x 12 matrix A from 40 sums -- four symmetric 4 x 4 moment matrices of
// Xh = (X, 1): S0 = sum Xh Xh^T, Sx = sum x Xh Xh^T, Sy = sum y Xh Xh^T, Sr = sum (x^2 + y^2) Xh Xh^T and
// A^T A = [[S0, 0, -Sx], [0, S0, -Sy], [-Sx, -Sy, Sr]]; (d) its eigenvector of the smallest eigenvalue by cyclic Jacobi; (e)
// P = T^-1 P U; (f) mean reprojection error; (g) crop translation and division by P[2][3]; (h) optical centre.
// The null vector of A is well separated (smallest singular value 1e-6 .. 9e-5 against 4.8 .. 21 for the next), so
// the normal matrix loses nothing that matters: no QR of the 2n x 12 matrix.
// Every sum runs in a fixed order (per-thread strided partial sums, a butterfly inside the wave, the four waves in order) and
// there are no floating-point atomics: a camera's result depends on nothing around it, and runs repeat bitwise.
// What bounds it: three passes over the points (LDS resident up to CAM_LDS_PTS of them) and then ONE lane running the 12 x 12
// Jacobi sweeps (~1e5 dependent float64 operations); the kernel is latency bound by that lane, the cameras run side by side.
#pragma once
#include <hip/hip_runtime.h>
#include "satba_models.h"
#include "satba_rpcfit.h"

namespace satba {

constexpr int CAM_THREADS = 256;
constexpr int CAM_LDS_PTS = 1440;       // points kept in LDS (5 doubles each: 57.6 KB); the reference's mesh has 1000
constexpr int CAM_MAX_PTS = 1 << 20;    // points per camera (mesh nodes or correspondences)
constexpr int CAM_SWEEPS = 40;          // Jacobi sweeps at most (6 - 9 run)
constexpr double CAM_RANK_TOL = 1e-12;  // second smallest / largest eigenvalue of A^T A below this: no unique camera

// sum_k v[k] over the workgroup for N values at once -> s_out[0 .. N - 1]; s_part: 4 N doubles
template <int N>
__device__ inline void cam_block_sums(const double (&v)[N], double* s_part, double* s_out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double t = v[k];
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
        if (lane == 0) s_part[4 * k + wave] = t;
    }
    __syncthreads();
    if (threadIdx.x < N) s_out[threadIdx.x] = (s_part[4 * threadIdx.x] + s_part[4 * threadIdx.x + 1]) + (s_part[4 * threadIdx.x + 2] + s_part[4 * threadIdx.x + 3]);
    __syncthreads();
}

// node i of the n_col x n_row x n_alt mesh (columns fastest, altitudes slowest; numpy.linspace's arithmetic): p = X Y Z col row
template <class T>
__device__ inline void cam_mesh_node(const T& tab, const double* cr, const double* rr, const double* ar, int n_col, int n_row, int n_alt, int i,
                                     double (&p)[5], double& alt) {
    const int ic = i % n_col, ir = (i / n_col) % n_row, ia = i / (n_col * n_row);
    p[3] = refit_linspace(cr[0], cr[1], n_col, ic);
    p[4] = refit_linspace(rr[0], rr[1], n_row, ir);
    alt = refit_linspace(ar[0], ar[1], n_alt, ia);
    double lon, lat;
    tri_localize(tab, p[3], p[4], alt, lon, lat);
    refit_to_ecef(lat, lon, alt, p[0], p[1], p[2]);
}

// eigenvectors (columns of V) and eigenvalues (diagonal of A) of the symmetric N x N matrix A by cyclic Jacobi, one lane (12 x 12:
// the resection below, "cam_jacobi12" in tests/cases_camapprox.py; 4 x 4: satba_fundamental.h).  A rotation is skipped once |a_pq| is below 2^-56 of the two diagonal entries:
// what is left moves an eigenvector by less than one rounding of the gap to its neighbour.  (A^T A is only positive semi-definite
// up to rounding: its smallest eigenvalue may come out negative, so the test is on the absolute values.)
template <int N>
__device__ inline void cam_jacobi(double (*A)[N], double (*V)[N]) {
    for (int r = 0; r < N; ++r)
        for (int c = 0; c < N; ++c) V[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < CAM_SWEEPS; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < N - 1; ++p)
            for (int q = p + 1; q < N; ++q) {
                const double apq = A[p][q], app = A[p][p], aqq = A[q][q];
                if (!(fabs(apq) > 0x1p-56 * (fabs(app) + fabs(aqq)))) continue;  // (also: a NaN rotates nothing and stays)
                rotated = true;
                // t = sign(theta) / (|theta| + sqrt(theta^2 + 1)), theta = (a_qq - a_pp) / (2 a_pq), with one division and one square root
                const double d = aqq - app, g2 = 2.0 * apq;
                const double t = copysign(1.0, d) * g2 / (fabs(d) + sqrt(d * d + g2 * g2));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                for (int k = 0; k < N; ++k) {
                    if (k != p && k != q) {
                        const double akp = A[k][p], akq = A[k][q];
                        A[k][p] = A[p][k] = c * akp - s * akq;
                        A[k][q] = A[q][k] = s * akp + c * akq;
                    }
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
                A[p][p] = app - t * apq; A[q][q] = aqq + t * apq;
                A[p][q] = A[q][p] = 0.0;
            }
        if (!rotated) break;
    }
}

// x = -M^-1 b for the 3 x 3 matrix M (rows m[0..2]) by Gaussian elimination with partial pivoting (what numpy.linalg.solve does)
__device__ inline void cam_centre3(double (&m)[3][4], double (&x)[3]) {  // m: [M | b], destroyed
    for (int k = 0; k < 3; ++k) {
        int piv = k;
        for (int r = k + 1; r < 3; ++r)
            if (fabs(m[r][k]) > fabs(m[piv][k])) piv = r;
        for (int c = 0; c < 4; ++c) { const double t = m[k][c]; m[k][c] = m[piv][c]; m[piv][c] = t; }
        for (int r = k + 1; r < 3; ++r) {
            const double f = m[r][k] / m[k][k];
            for (int c = k; c < 4; ++c) m[r][c] -= f * m[k][c];
        }
    }
    for (int k = 2; k >= 0; --k) {
        double v = m[k][3];
        for (int c = k + 1; c < 3; ++c) v -= m[k][c] * x[c];
        x[k] = v / m[k][k];
    }
    for (int k = 0; k < 3; ++k) x[k] = -x[k];
}

struct CamResectArgs {
    int n_pts;                  // per camera: mesh nodes or correspondences
    int n_col, n_row, n_alt;    // mesh route
    const double* tables;       // n_cam x 90: mesh route (phase a); null: the correspondences X, x are the caller's
    const double *col_range, *row_range, *alt_range;  // n_cam x 2 each
    double *X, *x;              // n_cam x n_pts x 3 / x 2: the caller's correspondences, or the slab of a mesh that does not fit the LDS
    const double* crop0;        // n_cam x 2 (col0, row0), or null: P as the resection leaves it (no translation, no division)
    double *P, *mean_err, *centers, *alts;  // n_cam x 12 | n_cam | n_cam x 3 | n_cam x n_pts; all but P may be null
};

// MESH_ONLY: phase (a) alone -- the mesh goes to X, x, alts (satba_rpc_mesh)
template <bool MESH_ONLY>
__global__ __launch_bounds__(CAM_THREADS) void k_cam_resect(const CamResectArgs a) {
    extern __shared__ double s_pts[];  // 5 x n_pts (X Y Z col row, one array each) when n_pts <= CAM_LDS_PTS
    __shared__ double s_tab[TRI_RPC_STRIDE];
    __shared__ double s_part[160], s_sum[40];
    __shared__ double s_A[12][12], s_V[12][12];
    __shared__ double s_Pn[12];
    const int cam = blockIdx.x, tid = threadIdx.x, n = a.n_pts;
    const bool lds = !MESH_ONLY && n <= CAM_LDS_PTS;
    double* Xg = a.X ? a.X + (size_t)cam * n * 3 : nullptr;
    double* xg = a.x ? a.x + (size_t)cam * n * 2 : nullptr;
    // ---- (a) the points
    if (a.tables) {
        if (tid < 90) s_tab[tid] = a.tables[(size_t)cam * 90 + tid];
        __syncthreads();
        for (int i = tid; i < n; i += CAM_THREADS) {
            double p[5], alt;
            cam_mesh_node(TabLds{s_tab}, a.col_range + 2 * cam, a.row_range + 2 * cam, a.alt_range + 2 * cam, a.n_col, a.n_row, a.n_alt, i, p, alt);
            if (lds) {
#pragma unroll
                for (int k = 0; k < 5; ++k) s_pts[k * n + i] = p[k];
            } else {
                Xg[3 * (size_t)i] = p[0]; Xg[3 * (size_t)i + 1] = p[1]; Xg[3 * (size_t)i + 2] = p[2];
                xg[2 * (size_t)i] = p[3]; xg[2 * (size_t)i + 1] = p[4];
            }
            if (MESH_ONLY && a.alts) a.alts[(size_t)cam * n + i] = alt;
        }
    } else if (lds) {
        for (int i = tid; i < n; i += CAM_THREADS) {
            s_pts[i] = Xg[3 * (size_t)i]; s_pts[n + i] = Xg[3 * (size_t)i + 1]; s_pts[2 * n + i] = Xg[3 * (size_t)i + 2];
            s_pts[3 * n + i] = xg[2 * (size_t)i]; s_pts[4 * n + i] = xg[2 * (size_t)i + 1];
        }
    }
    if (MESH_ONLY) return;
    __syncthreads();  // (a slab in global memory is read back by other lanes of this workgroup only)
    auto point = [&](int i, double (&p)[5]) {
        if (lds) {
#pragma unroll
            for (int k = 0; k < 5; ++k) p[k] = s_pts[k * n + i];
        } else {
            p[0] = Xg[3 * (size_t)i]; p[1] = Xg[3 * (size_t)i + 1]; p[2] = Xg[3 * (size_t)i + 2];
            p[3] = xg[2 * (size_t)i]; p[4] = xg[2 * (size_t)i + 1];
        }
    };
    // ---- (b) Hartley normalisation: centroids, then the mean distances to them scaled to sqrt(3) and sqrt(2)
    double c5[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += CAM_THREADS) {
        double p[5];
        point(i, p);
#pragma unroll
        for (int k = 0; k < 5; ++k) c5[k] += p[k];
    }
    cam_block_sums<5>(c5, s_part, s_sum);
    double cen[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) cen[k] = s_sum[k] / (double)n;
    double d2[2] = {0.0, 0.0};
    for (int i = tid; i < n; i += CAM_THREADS) {
        double p[5];
        point(i, p);
#pragma unroll
        for (int k = 0; k < 5; ++k) p[k] -= cen[k];
        d2[0] += sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
        d2[1] += sqrt(p[3] * p[3] + p[4] * p[4]);
    }
    cam_block_sums<2>(d2, s_part, s_sum);
    const double s3 = sqrt(3.0) / (s_sum[0] / (double)n), s2 = sqrt(2.0) / (s_sum[1] / (double)n);
    // ---- (c) the moments of the normalised points
    double acc[40];
#pragma unroll
    for (int k = 0; k < 40; ++k) acc[k] = 0.0;
    for (int i = tid; i < n; i += CAM_THREADS) {
        double p[5];
        point(i, p);
        const double h[4] = {s3 * (p[0] - cen[0]), s3 * (p[1] - cen[1]), s3 * (p[2] - cen[2]), 1.0};
        const double x = s2 * (p[3] - cen[3]), y = s2 * (p[4] - cen[4]), rr = x * x + y * y;
        int e = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = r; c < 4; ++c) {
                const double m = h[r] * h[c];
                acc[e] += m; acc[10 + e] += x * m; acc[20 + e] += y * m; acc[30 + e] += rr * m;
                ++e;
            }
    }
    cam_block_sums<40>(acc, s_part, s_sum);
    if (tid < 144) {
        const int r = tid / 12, c = tid % 12, br = r / 4, bc = c / 4;
        const int i0 = r % 4 < c % 4 ? r % 4 : c % 4, i1 = r % 4 < c % 4 ? c % 4 : r % 4;
        const int e = i0 * 4 - i0 * (i0 - 1) / 2 + (i1 - i0);  // index of (i0 <= i1) in the upper triangle, row by row
        double v = 0.0;
        if (br == bc) v = br < 2 ? s_sum[e] : s_sum[30 + e];
        else if (br == 2 || bc == 2) v = -s_sum[((br == 2 ? bc : br) == 0 ? 10 : 20) + e];
        s_A[r][c] = v;
    }
    __syncthreads();
    // ---- (d) the eigenvector of the smallest eigenvalue, (e) P = T^-1 Pn U
    if (tid == 0) {
        cam_jacobi<12>(s_A, s_V);
        int k0 = 0;
        double lmax = s_A[0][0], l2 = INFINITY, sum = 0.0;
        for (int k = 0; k < 12; ++k) {
            sum += s_A[k][k];
            if (s_A[k][k] < s_A[k0][k0]) k0 = k;
            lmax = fmax(lmax, s_A[k][k]);
        }
        for (int k = 0; k < 12; ++k)
            if (k != k0) l2 = fmin(l2, s_A[k][k]);
        // no unique camera (points in a plane, fewer than 6 distinct ones) or a non-finite sum (no extent: the scales are infinite)
        const bool ok = isfinite(sum) && isfinite(s2) && isfinite(s3) && l2 > CAM_RANK_TOL * lmax;
        for (int k = 0; k < 12; ++k) s_Pn[k] = ok ? s_V[k][k0] : NAN;
    }
    __syncthreads();
    double Pn[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Pn[k] = s_Pn[k];
    // ---- (f) mean reprojection error, taken in the normalised frame (pixels = normalised / s2): T^-1 is affine, so this is the
    // distance the reference measures, without the cancellation of P X at ECEF magnitudes
    double es[1] = {0.0};
    for (int i = tid; i < n; i += CAM_THREADS) {
        double p[5];
        point(i, p);
        const double X = s3 * (p[0] - cen[0]), Y = s3 * (p[1] - cen[1]), Z = s3 * (p[2] - cen[2]);
        const double w = Pn[8] * X + Pn[9] * Y + Pn[10] * Z + Pn[11];
        const double u = (Pn[0] * X + Pn[1] * Y + Pn[2] * Z + Pn[3]) / w, v = (Pn[4] * X + Pn[5] * Y + Pn[6] * Z + Pn[7]) / w;
        es[0] += hypot(s2 * (p[3] - cen[3]) - u, s2 * (p[4] - cen[4]) - v);
    }
    cam_block_sums<1>(es, s_part, s_sum);
    if (tid == 0) {
        double Q[3][4], P[3][4];
        for (int c = 0; c < 4; ++c) {
            Q[0][c] = Pn[c] / s2 + cen[3] * Pn[8 + c];
            Q[1][c] = Pn[4 + c] / s2 + cen[4] * Pn[8 + c];
            Q[2][c] = Pn[8 + c];
        }
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) P[r][c] = s3 * Q[r][c];
            P[r][3] = Q[r][3] - s3 * (Q[r][0] * cen[0] + Q[r][1] * cen[1] + Q[r][2] * cen[2]);
        }
        // ---- (g) the crop's corner becomes the origin, P[2][3] = 1 (cam_utils.py:195-197)
        if (a.crop0) {
            const double col0 = a.crop0[2 * cam], row0 = a.crop0[2 * cam + 1];
            for (int c = 0; c < 4; ++c) { P[0][c] -= col0 * P[2][c]; P[1][c] -= row0 * P[2][c]; }
            const double d = P[2][3];
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 4; ++c) P[r][c] /= d;
        }
        for (int k = 0; k < 12; ++k) a.P[(size_t)cam * 12 + k] = P[k / 4][k % 4];
        if (a.mean_err) a.mean_err[cam] = s_sum[0] / (double)n / s2;
        // ---- (h) optical centre -M^-1 P[:, 3]: solved in the normalised frame (the centre is the same point whatever T and the crop
        // translation are) and taken back through U
        if (a.centers) {
            double m[3][4], cn[3];
            for (int k = 0; k < 12; ++k) m[k / 4][k % 4] = Pn[k];
            cam_centre3(m, cn);
            for (int k = 0; k < 3; ++k) a.centers[(size_t)cam * 3 + k] = cn[k] / s3 + cen[k];
        }
    }
}

// ---- the longitude, correctly rounded.  One ulp of a longitude in degrees (73 deg: 1.4e-14 deg, 1.6e-9 m on the ground) moves the
// column of the shipped sensors by 2.2e-9 px; the device's atan2 is good to an ulp or two, and a host libm's float64 atan2 is
// not correctly rounded either (numpy.arctan2 missed the rounded value on 227 of 35 010 arguments, tests/test_atan2_host.py).  The
// value q of the affine expansion is the one quantity compared at the 1e-9 px level, so k_cam_affine takes atan2(y, x) in
// double-double arithmetic (error-free sums and fma products, ~1e-30 relative) and rounds it once: bit for bit the rounded value of
// a 200-bit evaluation on those arguments, in all four quadrants and across every seam of the three branches below.
struct CamDD { double hi, lo; };
__host__ __device__ inline CamDD cam_dd_norm(double a, double b) {  // |a| >= |b|
#pragma clang fp contract(off)
    const double s = a + b;
    return CamDD{s, b - (s - a)};
}
__host__ __device__ inline CamDD cam_dd_add(CamDD a, CamDD b) {
#pragma clang fp contract(off)
    const double s = a.hi + b.hi, bb = s - a.hi;
    const double e = ((a.hi - (s - bb)) + (b.hi - bb)) + (a.lo + b.lo);
    return cam_dd_norm(s, e);
}
__host__ __device__ inline CamDD cam_dd_neg(CamDD a) { return CamDD{-a.hi, -a.lo}; }
__host__ __device__ inline CamDD cam_dd_mul(CamDD a, CamDD b) {
#pragma clang fp contract(off)
    const double p = a.hi * b.hi;
    const double e = fma(a.hi, b.hi, -p) + (a.hi * b.lo + a.lo * b.hi);
    return cam_dd_norm(p, e);
}
__host__ __device__ inline CamDD cam_dd_div(CamDD a, CamDD b) {
#pragma clang fp contract(off)
    const double q1 = a.hi / b.hi;
    CamDD r = cam_dd_add(a, cam_dd_neg(cam_dd_mul(b, CamDD{q1, 0.0})));
    const double q2 = r.hi / b.hi;
    r = cam_dd_add(r, cam_dd_neg(cam_dd_mul(b, CamDD{q2, 0.0})));
    const double q3 = r.hi / b.hi;
    return cam_dd_add(cam_dd_norm(q1, q2), CamDD{q3, 0.0});
}
__host__ __device__ inline CamDD cam_dd_sqrt(CamDD a) {
#pragma clang fp contract(off)
    const double x = sqrt(a.hi);
    const CamDD r = cam_dd_add(a, cam_dd_neg(cam_dd_mul(CamDD{x, 0.0}, CamDD{x, 0.0})));
    return cam_dd_add(CamDD{x, 0.0}, CamDD{r.hi / (2.0 * x), 0.0});
}
// atan(t), 0 <= t <= 1: three half-angle steps t <- t / (1 + sqrt(1 + t^2)) bring t below 0.0985, then 13 terms of the series
__host__ __device__ inline CamDD cam_dd_atan01(CamDD t) {
    const CamDD one{1.0, 0.0};
    for (int k = 0; k < 3; ++k) t = cam_dd_div(t, cam_dd_add(one, cam_dd_sqrt(cam_dd_add(one, cam_dd_mul(t, t)))));
    const CamDD u = cam_dd_neg(cam_dd_mul(t, t));
    CamDD poly = cam_dd_div(one, CamDD{25.0, 0.0});
    for (int k = 11; k >= 0; --k) poly = cam_dd_add(cam_dd_div(one, CamDD{(double)(2 * k + 1), 0.0}), cam_dd_mul(u, poly));
    const CamDD a = cam_dd_mul(t, poly);
    return CamDD{8.0 * a.hi, 8.0 * a.lo};
}
__host__ __device__ inline double cam_atan2_rounded(double y, double x) {
    const double ax = fabs(x), ay = fabs(y);
    const CamDD pi{3.141592653589793116, 1.224646799147353207e-16}, half_pi{1.570796326794896558, 6.123233995736766036e-17};
    CamDD a = ax >= ay ? cam_dd_atan01(cam_dd_div(CamDD{ay, 0.0}, CamDD{ax, 0.0}))
                       : cam_dd_add(half_pi, cam_dd_neg(cam_dd_atan01(cam_dd_div(CamDD{ax, 0.0}, CamDD{ay, 0.0}))));
    if (x < 0.0) a = cam_dd_add(pi, cam_dd_neg(a));
    return y < 0.0 ? -a.hi : a.hi;  // (0, 0): NaN, as the longitude of a point on the polar axis should be
}

// q - J p - c0 rounded once: the products and the partial sums are carried exactly (error-free product by fma, two-sum), because
// J p is ~1e6 pixels (|p| = 6.4e6 m) and every rounding at that size is 1e-10 .. 5e-10 px
__device__ inline double cam_affine_offset(double q, const double (&J)[3], const double (&p)[3], double c0) {
#pragma clang fp contract(off)
    double hi = q, lo = 0.0;
    for (int k = 0; k < 4; ++k) {
        double t, te = 0.0;
        if (k < 3) { t = -J[k] * p[k]; te = fma(-J[k], p[k], -t); }
        else t = -c0;
        const double s = hi + t, b = s - hi;
        lo += ((hi - (s - b)) + (t - b)) + te;
        hi = s;
    }
    return hi + lo;
}

// one lane per camera: P = [[J, q - J p - (col0, row0)], [0 0 0 1]], q = (col, row) and J = d(col, row)/dX at p = xyz[cam]
__global__ __launch_bounds__(CAM_THREADS) void k_cam_affine(int n_cam, const double* __restrict__ tables, const double* __restrict__ xyz,
                                                            const double* __restrict__ col0row0, double* __restrict__ P) {
    const int cam = blockIdx.x * CAM_THREADS + threadIdx.x;
    if (cam >= n_cam) return;
    const double p[3] = {xyz[3 * (size_t)cam], xyz[3 * (size_t)cam + 1], xyz[3 * (size_t)cam + 2]};
    const double* tab = tables + (size_t)cam * 90;
    double q[2], D[2][3], geo[3], G[3][3];
    rpc_project<true>(tab, p[0], p[1], p[2], q[0], q[1], D);  // J: the chain of the two analytic Jacobians
    geodetic<false>(p[0], p[1], p[2], geo, G);                // q: the same projection at the correctly rounded longitude
    double L;
    {
        // The longitude in degrees is ROUNDED before the offset is taken off, as a float64 evaluation of the reference's formula
        // rounds it.  Contracted into fma(rad, 180 / pi, -offset) the product keeps its extra bits, q then carries the rounding of
        // the radians only and sits up to half an ulp of the longitude (1.1e-9 px at 107 deg, 2.2e-9 px at 163 deg) from the
        // float64 value it is compared with: below 1e-9 px at the four shipped points by luck, beyond it in five of the eight
        // octant placements (tests/test_gpu_octants.py).
#pragma clang fp contract(off)
        geo[1] = cam_atan2_rounded(p[1], p[0]) * (180.0 / M_PI);
        L = (geo[1] - tab[80]) / tab[81];
    }
    const double La = (geo[0] - tab[82]) / tab[83], H = (geo[2] - tab[84]) / tab[85];
    double* o = P + (size_t)cam * 12;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        double num, den, u0, u1, u2;
        rpc_poly<false>(tab + 40 * k, L, La, H, L * L, La * La, H * H, L * La, L * H, La * H, num, u0, u1, u2);
        rpc_poly<false>(tab + 40 * k + 20, L, La, H, L * L, La * La, H * H, L * La, L * H, La * H, den, u0, u1, u2);
        q[k] = num / den * tab[87 + 2 * k] + tab[86 + 2 * k];
        o[4 * k] = D[k][0]; o[4 * k + 1] = D[k][1]; o[4 * k + 2] = D[k][2];
        o[4 * k + 3] = cam_affine_offset(q[k], D[k], p, col0row0[2 * cam + k]);
    }
    o[8] = 0.0; o[9] = 0.0; o[10] = 0.0; o[11] = 1.0;
}

}  // namespace satba

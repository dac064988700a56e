// satba_fundamental.h -- one affine fundamental matrix per image pair from the two RPCs, the step between the choice of the pairs
// and their matching under the epipolar gate (ref:bundle_adjust/feature_tracks/ft_pipeline.py:139-152, init_F_pair_to_match):
//   ref:bundle_adjust/s2p/rpc_utils.py:199-246  matches_from_rpc: an n x n x n mesh over the region of interest of image i and the
//       altitude range alt_offset -+ alt_scale of RPC i is localised through RPC i and projected through RPC i AND RPC j (x1, y1 is
//       the re-projection, not the mesh node)
//   ref:bundle_adjust/s2p/estimation.py:114-154  affine_fundamental_matrix: X = (x2, y2, x1, y1), A = X - mean; N = the right singular
//       vector of the smallest singular value of A; F02, F12, F20, F21 = N, F22 = -N . mean (Hartley & Zisserman, algorithm 14.1)
//
// k_fundamental, one workgroup per pair: (a) both tables to LDS; (b) the n^3 matches, LDS resident (one array per coordinate);
// (c) the four means; (d) the ten centred second moments A^T A, a SECOND pass after the means (the coordinates are ~1e3 px, the
// smallest singular value a few px: sum of squares minus square of sum would lose it); (e) one lane: cyclic Jacobi on the 4 x 4
// matrix, the column of the smallest eigenvalue, normalised, and F22.
// The null direction is separated (singular values 5e4, 2e2 .. 1e4, 1.6e2 .. 4e3 against 3.5 .. 14, pixels of RPC
// non-linearity over the altitude range), so the normal matrix loses nothing that matters, as in the resection (satba_camapprox.h).
// Sign: N and -N are the same matrix to every user (the rectifying similarities of -F negate both rectified ordinates, the gate
// |y1' - y2'| of satba_match.h does not move), and the sign the reference returns is whatever LAPACK's SVD leaves: it flips
// between crops of one pair.  Here the component of N with the largest magnitude is positive (the first of equals).
// Degenerate pairs (an image with itself, two identical RPCs): the null space of A is two-dimensional and any vector of it would
// be an accident.  When the second smallest eigenvalue is not above CAM_RANK_TOL times the largest (healthy pairs: 9e-6 and above;
// identical RPCs: below 1e-30) the pair's status is 1 and its F5 is NaN.
// Every sum runs in a fixed order (per-lane strided partial sums, a butterfly inside the wave, the four waves in order) and there
// are no floating-point atomics: a pair's result depends on nothing around it, and runs repeat bitwise.
// What bounds it: n^3 / 256 localisations per lane (a Newton iteration each), three block reductions, then ONE lane running the
// 4 x 4 Jacobi sweeps: 22 us for one pair as for 200, the pairs run side by side; 1.3 ms for 19 900 pairs.
#pragma once
#include <hip/hip_runtime.h>
#include "satba_camapprox.h"
#include "satba_rpcfit.h"
#include "satba_triangulate.h"

namespace satba {

constexpr int FND_THREADS = CAM_THREADS;
constexpr int FND_MAX_N = 11;  // samples per axis: 11^3 = 1331 matches of 4 doubles are 42.6 KB of LDS (CAM_LDS_PTS = 1440 is the
                               // budget of the resection); the reference uses 5
// The localisation runs past the reference's stopping rule (squared normalised residual 1e-18: a node localised to 1e-9 of the
// image scale, ~1e-6 px) down to 1e-26.  Where the reference stops depends on the path its Newton iteration took, and an RPC
// mirrored to the other hemisphere takes another one (the start -delta in the normalised latitude becomes +delta): F of a
// mirrored pair then sat 1.6e-9 px from F of the original pair, ten times the distance between two float64 routes to N.  One
// or two more steps cost a third of phase (b) and leave 2e-12 px (tests/test_gpu_fundamental.py, test_other_hemispheres); the
// matches stay within 1e-6 px of the reference's, far inside what the project asserts of a localisation (1e-9 deg).
constexpr double FND_LOC_TOL2 = 1e-26;
static_assert(FND_MAX_N * FND_MAX_N * FND_MAX_N <= CAM_LDS_PTS && (FND_MAX_N + 1) * (FND_MAX_N + 1) * (FND_MAX_N + 1) > CAM_LDS_PTS, "n^3 matches stay LDS resident");

struct FundamentalArgs {
    int n;                  // samples per axis
    const double* tables;   // n_cam x 90
    const int* pairs;       // n_pairs x 2: images i, j
    const double* ranges;   // n_pairs x 6: first and last column, row, altitude of the mesh
    double *F5, *sv;        // n_pairs x 5: F02 F12 F20 F21 F22 | n_pairs x 4: singular values of A, descending
    double* matches;        // n_pairs x n^3 x 4 (x1 y1 x2 y2), or null
    int* status;            // n_pairs: 1 = no unique matrix (F5 is NaN)
};

__global__ __launch_bounds__(FND_THREADS) void k_fundamental(const FundamentalArgs a) {
    extern __shared__ double s_m[];  // 4 x n^3: x1, y1, x2, y2, one array each
    __shared__ double s_tab[2 * TRI_RPC_STRIDE];
    __shared__ double s_part[40], s_sum[10];
    __shared__ double s_A[4][4], s_V[4][4];
    const int pair = blockIdx.x, tid = threadIdx.x, n = a.n, n3 = n * n * n;
    // ---- (a) the tables of image i and image j
    for (int k = tid; k < 180; k += FND_THREADS) s_tab[(k / 90) * TRI_RPC_STRIDE + k % 90] = a.tables[(size_t)a.pairs[2 * pair + k / 90] * 90 + k % 90];
    __syncthreads();
    const TabLds ti{s_tab}, tj{s_tab + TRI_RPC_STRIDE};
    // ---- (b) the matches: columns fastest, altitudes slowest
    const double* rg = a.ranges + 6 * (size_t)pair;
    for (int i = tid; i < n3; i += FND_THREADS) {
        const double col = refit_linspace(rg[0], rg[1], n, i % n), row = refit_linspace(rg[2], rg[3], n, (i / n) % n);
        const double alt = refit_linspace(rg[4], rg[5], n, i / (n * n));
        double lon, lat, m[4];
        tri_localize(ti, col, row, alt, lon, lat, FND_LOC_TOL2);
        tri_project(ti, lon, lat, alt, m[0], m[1]);
        tri_project(tj, lon, lat, alt, m[2], m[3]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s_m[k * n3 + i] = m[k];
            if (a.matches) a.matches[((size_t)pair * n3 + i) * 4 + k] = m[k];
        }
    }
    // ---- (c) the means, in the reference's order of X: x2, y2, x1, y1
    auto point = [&](int i, double (&x)[4]) { x[0] = s_m[2 * n3 + i]; x[1] = s_m[3 * n3 + i]; x[2] = s_m[i]; x[3] = s_m[n3 + i]; };
    double c4[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n3; i += FND_THREADS) {  // (the barrier that makes the matches visible opens cam_block_sums)
        double x[4];
        point(i, x);
#pragma unroll
        for (int k = 0; k < 4; ++k) c4[k] += x[k];
    }
    cam_block_sums<4>(c4, s_part, s_sum);
    double mean[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) mean[k] = s_sum[k] / (double)n3;
    // ---- (d) the centred second moments (upper triangle, row by row)
    double acc[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[k] = 0.0;
    for (int i = tid; i < n3; i += FND_THREADS) {
        double x[4];
        point(i, x);
#pragma unroll
        for (int k = 0; k < 4; ++k) x[k] -= mean[k];
        int e = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = r; c < 4; ++c) acc[e++] += x[r] * x[c];
    }
    cam_block_sums<10>(acc, s_part, s_sum);
    // ---- (e) the eigenvector of the smallest eigenvalue
    if (tid == 0) {
        int e = 0;
        for (int r = 0; r < 4; ++r)
            for (int c = r; c < 4; ++c) s_A[r][c] = s_A[c][r] = s_sum[e++];
        cam_jacobi<4>(s_A, s_V);
        int k0 = 0;
        double lam[4], lmax = s_A[0][0], l2 = INFINITY, sum = 0.0;
        for (int k = 0; k < 4; ++k) {
            lam[k] = s_A[k][k];
            sum += lam[k];
            if (lam[k] < lam[k0]) k0 = k;
            lmax = fmax(lmax, lam[k]);
        }
        for (int k = 0; k < 4; ++k)
            if (k != k0) l2 = fmin(l2, lam[k]);
        const bool ok = isfinite(sum) && l2 > CAM_RANK_TOL * lmax;
        double N[4], nn = 0.0, big = 0.0, e22 = 0.0;
        for (int k = 0; k < 4; ++k) { N[k] = s_V[k][k0]; nn += N[k] * N[k]; }
        for (int k = 0; k < 4; ++k)
            if (fabs(N[k]) > fabs(big)) big = N[k];
        const double s = (big < 0.0 ? -1.0 : 1.0) / sqrt(nn);
        for (int k = 0; k < 4; ++k) { N[k] *= s; e22 -= N[k] * mean[k]; }
        double* F = a.F5 + 5 * (size_t)pair;
        for (int k = 0; k < 4; ++k) F[k] = ok ? N[k] : NAN;
        F[4] = ok ? e22 : NAN;
        a.status[pair] = ok ? 0 : 1;
        // singular values of A: the square roots of the eigenvalues, descending (A^T A is positive semi-definite up to rounding only)
        for (int k = 1; k < 4; ++k)
            for (int m = k; m > 0 && lam[m] > lam[m - 1]; --m) { const double t = lam[m]; lam[m] = lam[m - 1]; lam[m - 1] = t; }
        for (int k = 0; k < 4; ++k) a.sv[4 * (size_t)pair + k] = sqrt(fmax(lam[k], 0.0));
    }
}

}  // namespace satba

// satba_utm.h -- the geographic side of the pairwise matching on the device:
//   * the UTM consistency filter of ref:feature_tracks/ft_match.py:220-247 for the matches of all pairs in one call
//     (satba_utm_filter): distance of a match's two keypoints on the ground, per pair the elbow of the sorted distances
//     (satba_elbow.h), matches at most elbow + margin away are kept;
//   * the UTM coordinates of the keypoints of all images in one call (satba_keypoints_utm, ref:ft_match.py:190-217): RPC
//     localisation at the image's altitude (tri_localize of satba_triangulate.h, what k_rpc_localize runs), then the projection
//     of satba_utm_geom.h in the image's zone.
// The filter must come out index-exact against numpy, so its distances and its threshold round where numpy's do: no contraction.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "satba_elbow.h"
#include "satba_triangulate.h"
#include "satba_utm_geom.h"

namespace satba {

constexpr int UTM_THREADS = 256;     // the filter's kernels
constexpr int UTM_KP_THREADS = 64;   // the keypoint kernels: one wave, so that small images spread over the CUs

// ---------------------------------------------------------------------------------------------------- the filter
// d[i] = | (east_i, north_i) - (east_j, north_j) | as np.linalg.norm(..., axis=1) rounds it (two squares, one sum, one root);
// flag[i] = alive (the input of the exclusive scan)
__global__ __launch_bounds__(UTM_THREADS) void k_utm_dist(long long n, const double* __restrict__ utm, const unsigned char* __restrict__ alive,
                                                          double* __restrict__ d, int* __restrict__ flag) {
    for (long long i = (long long)blockIdx.x * UTM_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * UTM_THREADS) {
        d[i] = utm_distance(utm + 4 * i);
        flag[i] = (!alive || alive[i]) ? 1 : 0;
    }
}

// the alive distances pair by pair (pos: the exclusive scan of flag; n >= 1) and the pairs' offsets among them: the scan read at
// pair_ofs[p], behind the last match the number alive
__global__ __launch_bounds__(UTM_THREADS) void k_utm_compact(long long n, int n_pairs, const long long* __restrict__ pair_ofs,
                                                             const double* __restrict__ d, const int* __restrict__ flag,
                                                             const int* __restrict__ pos, double* __restrict__ dc, int* __restrict__ cofs) {
    const long long stride = (long long)gridDim.x * UTM_THREADS, t0 = (long long)blockIdx.x * UTM_THREADS + threadIdx.x;
    for (long long i = t0; i < n; i += stride)
        if (flag[i]) dc[pos[i]] = d[i];
    for (long long p = t0; p <= n_pairs; p += stride) {
        const long long o = pair_ofs[p];
        cofs[p] = o < n ? pos[o] : pos[n - 1] + flag[n - 1];
    }
}

// one workgroup per pair over its ascending alive distances: thr = success ? elbow + margin : v[n - 1] (NaN without an alive
// match), then the pair's matches in the caller's order: keep = alive and d <= thr, and their count
__global__ __launch_bounds__(UTM_THREADS) void k_utm_threshold(const long long* __restrict__ pair_ofs, const int* __restrict__ cofs,
                                                               const double* __restrict__ sorted, const double* __restrict__ d,
                                                               const int* __restrict__ flag, double margin, unsigned char* __restrict__ keep,
                                                               double* __restrict__ thr_out, long long* __restrict__ n_kept) {
    const int p = blockIdx.x;
    const int b = cofs[p], m = cofs[p + 1] - b;
    __shared__ double s_thr;
    __shared__ int s_cnt;
    if (m > 0) {
        const Elbow e = elbow_block<UTM_THREADS>(sorted + b, m);
        if (threadIdx.x == 0) s_thr = utm_threshold(e, margin);
    } else if (threadIdx.x == 0) {
        s_thr = __longlong_as_double(0x7ff8000000000000ll);
    }
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const double thr = s_thr;
    int cnt = 0;
    for (long long i = pair_ofs[p] + threadIdx.x; i < pair_ofs[p + 1]; i += UTM_THREADS) {
        const unsigned char k = (flag[i] && d[i] <= thr) ? 1 : 0;
        keep[i] = k;
        cnt += k;
    }
    for (int s = 32; s > 0; s >>= 1) cnt += __shfl_down(cnt, s);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    if (threadIdx.x == 0) { thr_out[p] = thr; n_kept[p] = s_cnt; }
}

// ---------------------------------------------------------------------------------------------------- keypoints to UTM
struct KpImage {     // per image, device memory
    long long base;  // first row of the image in the concatenated arrays
    int n_rows, n_kp;  // rows, and the leading ones that are keypoints (ref:ft_match.py:203: the rows whose column is no NaN)
    double col0, row0, alt;
    int zone, pad;   // 0: the zone of the image's first keypoint
};

// lane = row of a block's image (blocks: image, first row of the block inside it): keypoints are localised at the image's altitude,
// padding rows pass their two columns through (ref:ft_match.py:216)
__global__ __launch_bounds__(UTM_KP_THREADS) void k_kp_localize(const int2* __restrict__ blocks, const KpImage* __restrict__ images,
                                                                const double* __restrict__ tables, const float2* __restrict__ xy,
                                                                double2* __restrict__ lonlat) {
    __shared__ double s_tab[TRI_RPC_STRIDE];
    const int2 blk = blocks[blockIdx.x];
    const KpImage im = images[blk.x];
    for (int k = threadIdx.x; k < 90; k += UTM_KP_THREADS) s_tab[k] = tables[(size_t)blk.x * 90 + k];
    __syncthreads();
    const int r = blk.y + threadIdx.x;
    if (r >= im.n_rows) return;
    const float2 q = xy[im.base + r];
    double lo = (double)q.x, la = (double)q.y;
    if (r < im.n_kp) tri_localize(TabLds{s_tab}, (double)q.x + im.col0, (double)q.y + im.row0, im.alt, lo, la);
    lonlat[im.base + r] = make_double2(lo, la);
}

__global__ __launch_bounds__(UTM_KP_THREADS) void k_kp_project(const int2* __restrict__ blocks, const KpImage* __restrict__ images,
                                                               const double2* __restrict__ lonlat, double2* __restrict__ utm) {
    const int2 blk = blocks[blockIdx.x];
    const KpImage im = images[blk.x];
    const int r = blk.y + threadIdx.x;
    if (r >= im.n_rows) return;
    const double2 g = lonlat[im.base + r];
    double2 o = g;
    if (r < im.n_kp) {
        const int zone = im.zone ? im.zone : utm_zone(lonlat[im.base].x);
        utm_project(g.x, g.y, zone, o.x, o.y);
    }
    utm[im.base + r] = o;
}

}  // namespace satba

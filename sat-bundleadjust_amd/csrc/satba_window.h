// satba_window.h -- SIFT matching inside a UTM window (ref:bundle_adjust/feature_tracks/ft_match.py:396-463,
// locally_match_SIFT_utm_coords; the rule is in include/satba.h, satba_match_window).  Host side:
// satba_window_api.inc.  Pack, select, emit, the slot space and MatchPair are those of satba_match.h; the cells are satba_window_cells.h.
//
// The walk.  The selected keypoints of every pair's second side are sorted once by (pair, cell_y, cell_x) (rocprim, stable) and what
// a query reads per candidate is gathered into that order.  A query visits the grid rows of its window; in the sorted order the cells
// cx0 .. cx1 of one row are one contiguous range, found by two binary searches.  WN_LANES lanes share a query: each takes every
// WN_LANES-th keypoint of a range, tests the window in float64, and gathers the 128-byte record of a candidate that passes.  A range
// of any length is walked by the loop: nothing assumes that a window fits a tile.  The lanes reduce (d << 32) | j to its minimum,
// so the winner does not depend on the order of the visit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "satba_match.h"
#include "satba_window_cells.h"

namespace satba {

#ifndef WN_LANES
#define WN_LANES 16  // lanes per query: 16 (four queries per wave) or 64 (DESIGN.md 4q has the measurement)
#endif
constexpr int WN_THREADS = 256;

// One workgroup per pair: the extent of the second side's selected keypoints, and from it the pair's grid.
__global__ __launch_bounds__(WN_THREADS) void k_window_grid(const MatchPair* __restrict__ pairs, const double2* __restrict__ utm, const int* __restrict__ sel,
                                                            double rx, double ry, WcGrid* __restrict__ grids) {
    __shared__ double red[4][WN_THREADS / 64];
    const MatchPair& P = pairs[blockIdx.x];
    const int n = P.n[1], ofs = P.ofs[1], tid = threadIdx.x;
    double e0 = INFINITY, e1 = -INFINITY, n0 = INFINITY, n1 = -INFINITY;
    for (int k = tid; k < n; k += WN_THREADS) {
        const double2 u = utm[sel[ofs + k]];
        e0 = fmin(e0, u.x); e1 = fmax(e1, u.x);
        n0 = fmin(n0, u.y); n1 = fmax(n1, u.y);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        e0 = fmin(e0, __shfl_xor(e0, m)); e1 = fmax(e1, __shfl_xor(e1, m));
        n0 = fmin(n0, __shfl_xor(n0, m)); n1 = fmax(n1, __shfl_xor(n1, m));
    }
    if ((tid & 63) == 0) {
        red[0][tid >> 6] = e0; red[1][tid >> 6] = e1; red[2][tid >> 6] = n0; red[3][tid >> 6] = n1;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < WN_THREADS / 64; ++w) {
            e0 = fmin(e0, red[0][w]); e1 = fmax(e1, red[1][w]);
            n0 = fmin(n0, red[2][w]); n1 = fmax(n1, red[3][w]);
        }
        WcGrid g;
        g.x = wc_axis(e0, e1, rx);
        g.y = wc_axis(n0, n1, ry);
        grids[blockIdx.x] = g;
    }
}

// Sort keys of the second sides: blockIdx.x = pair, the pair's selected keypoints strided over blockIdx.y.  seg[p] is the first
// position of pair p among all pairs' second-side selections; val = the keypoint's position j inside its side.
__global__ __launch_bounds__(WN_THREADS) void k_window_keys(const MatchPair* __restrict__ pairs, const double2* __restrict__ utm, const int* __restrict__ sel,
                                                            const WcGrid* __restrict__ grids, const int* __restrict__ seg, unsigned long long* __restrict__ keys,
                                                            int* __restrict__ vals) {
    const int p = blockIdx.x;
    const MatchPair& P = pairs[p];
    const WcGrid g = grids[p];
    const int n = P.n[1], ofs = P.ofs[1], s0 = seg[p];
    for (int k = blockIdx.y * WN_THREADS + threadIdx.x; k < n; k += gridDim.y * WN_THREADS) {
        const double2 u = utm[sel[ofs + k]];
        keys[s0 + k] = wc_key(p, wc_cell(g.y, u.y), wc_cell(g.x, u.x));
        vals[s0 + k] = k;
    }
}

// What a query reads per keypoint of a range, in the sorted order: coordinates, global row, squared norm of the int8 record.
__global__ __launch_bounds__(WN_THREADS) void k_window_gather(int n, const MatchPair* __restrict__ pairs, const unsigned long long* __restrict__ keys,
                                                              const int* __restrict__ w_j, const int* __restrict__ sel, const double2* __restrict__ utm,
                                                              const int* __restrict__ nrm, double2* __restrict__ w_utm, int* __restrict__ w_row,
                                                              int* __restrict__ w_nrm) {
    const int k = blockIdx.x * WN_THREADS + threadIdx.x;
    if (k >= n) return;
    const int p = (int)(keys[k] >> (2 * WC_DIM_BITS));
    const int row = sel[pairs[p].ofs[1] + w_j[k]];
    w_utm[k] = utm[row];
    w_row[k] = row;
    w_nrm[k] = nrm[row];
}

// first position in [a, b) whose key is not below / is above `key`
__device__ __forceinline__ int wn_lower(const unsigned long long* __restrict__ keys, int a, int b, unsigned long long key) {
    while (a < b) {
        const int m = a + ((b - a) >> 1);
        if (keys[m] < key) a = m + 1; else b = m;
    }
    return a;
}
__device__ __forceinline__ int wn_upper(const unsigned long long* __restrict__ keys, int a, int b, unsigned long long key) {
    while (a < b) {
        const int m = a + ((b - a) >> 1);
        if (keys[m] <= key) a = m + 1; else b = m;
    }
    return a;
}

// squared distance of two keypoint rows as the upper half of the reduction key (non-negative, so the bits order as the values do)
// integer path: |a'|^2 + |b'|^2 - 2 a'.b' on the packed int8 records, exact
__device__ __forceinline__ unsigned wn_dist_i8(const int (&q)[MT_DESC / 4], int nq, const signed char* __restrict__ rec, int row, int nb) {
    const mt_v4i* r = reinterpret_cast<const mt_v4i*>(rec + (long long)row * MT_DESC);
    int dot = 0;
#pragma unroll
    for (int v = 0; v < MT_DESC / 16; ++v) {
        const mt_v4i c = r[v];
#pragma unroll
        for (int e = 0; e < 4; ++e) dot = __builtin_amdgcn_sdot4(q[4 * v + e], c[e], dot, false);
    }
    return (unsigned)(nq + nb - 2 * dot);
}
// float path: float32 in index order, nothing fused
__device__ __forceinline__ unsigned wn_dist_f32(const float* __restrict__ feat, int row_i, int row_j) {
    const float4* a = reinterpret_cast<const float4*>(feat + (long long)row_i * MT_ROW + 4);
    const float4* b = reinterpret_cast<const float4*>(feat + (long long)row_j * MT_ROW + 4);
    float d = 0.0f;
    for (int v = 0; v < MT_DESC / 4; ++v) {
        const float4 x = a[v], y = b[v];
        float t = __fsub_rn(x.x, y.x); d = __fadd_rn(d, __fmul_rn(t, t));
        t = __fsub_rn(x.y, y.y); d = __fadd_rn(d, __fmul_rn(t, t));
        t = __fsub_rn(x.z, y.z); d = __fadd_rn(d, __fmul_rn(t, t));
        t = __fsub_rn(x.w, y.w); d = __fadd_rn(d, __fmul_rn(t, t));
    }
    return __float_as_uint(d);
}

// WN_LANES lanes per first-side slot.  Slots of a second side, past a side's selection, or of a pair with an empty side idle through
// the loops (no early return: all lanes meet at the reduction).  hit / kp_j are those k_match_emit reads.
template <int LPQ, bool F32>
__global__ __launch_bounds__(WN_THREADS) void k_window_nearest(long long n_slots, const MatchPair* __restrict__ pairs, const int* __restrict__ slot_pair,
                                                               const WcGrid* __restrict__ grids, const int* __restrict__ seg, const int* __restrict__ sel,
                                                               const double2* __restrict__ utm, const int* __restrict__ nrm_s,
                                                               const unsigned long long* __restrict__ keys, const double2* __restrict__ w_utm,
                                                               const int* __restrict__ w_row, const int* __restrict__ w_j, const int* __restrict__ w_nrm,
                                                               const signed char* __restrict__ rec, const float* __restrict__ feat, double rx, double ry,
                                                               float thr2, int* __restrict__ hit, int* __restrict__ kp_j, unsigned long long* __restrict__ n_cand) {
    static_assert(LPQ == 16 || LPQ == 32 || LPQ == 64, "lanes per query");
    const int sub = threadIdx.x % LPQ;
    long long slot = (long long)blockIdx.x * (WN_THREADS / LPQ) + threadIdx.x / LPQ;
    if (LPQ == 64) slot = (long long)blockIdx.x * (WN_THREADS / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // uniform: the record by scalar loads
    int p = -1, q = 0;
    if (slot < n_slots) p = slot_pair[slot / MT_TILE];
    bool active = p >= 0;
    if (active) {
        q = (int)(slot - pairs[p].ofs[0]);
        active = q < pairs[p].n[0] && pairs[p].n[1] > 0;
    }
    unsigned long long best = ~0ull;
    unsigned cand = 0;
    if (active) {
        const int row_i = sel[slot];
        const double2 ui = utm[row_i];
        const WcGrid g = grids[p];
        int cx0, cx1, cy0, cy1;
        wc_range(g.x, ui.x, rx, cx0, cx1);
        wc_range(g.y, ui.y, ry, cy0, cy1);
        int qv[MT_DESC / 4], nq = 0;
        if (!F32) {
            const mt_v4i* r = reinterpret_cast<const mt_v4i*>(rec + (long long)row_i * MT_DESC);
#pragma unroll
            for (int v = 0; v < MT_DESC / 16; ++v) {
                const mt_v4i c = r[v];
                qv[4 * v] = c[0]; qv[4 * v + 1] = c[1]; qv[4 * v + 2] = c[2]; qv[4 * v + 3] = c[3];
            }
            nq = nrm_s[slot];
        }
        int a = seg[p];
        const int s1 = seg[p + 1];
        for (int cy = cy0; cy <= cy1; ++cy) {
            a = wn_lower(keys, a, s1, wc_key(p, cy, cx0));
            const int b = wn_upper(keys, a, s1, wc_key(p, cy, cx1));
            for (int k = a + sub; k < b; k += LPQ) {
                const double2 uj = w_utm[k];
                if (fabs(ui.x - uj.x) < rx && fabs(ui.y - uj.y) < ry) {
                    ++cand;
                    unsigned d;
                    if (F32) d = wn_dist_f32(feat, row_i, w_row[k]);
                    else d = wn_dist_i8(qv, nq, rec, w_row[k], w_nrm[k]);
                    const unsigned long long key = ((unsigned long long)d << 32) | (unsigned)w_j[k];
                    best = key < best ? key : best;
                }
            }
            a = b;
        }
    }
#pragma unroll
    for (int m = LPQ / 2; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(best, m);
        best = o < best ? o : best;
        cand += __shfl_xor(cand, m);
    }
    if (active && sub == 0) {
        int found = 0, out = -1;
        if (cand) {
            const unsigned d = (unsigned)(best >> 32);
            const float dA = F32 ? __uint_as_float(d) : (float)(int)d;
            if (dA < thr2) {
                found = 1;
                out = sel[pairs[p].ofs[1] + (int)(unsigned)best] - pairs[p].base[1];
            }
            atomicAdd(n_cand, (unsigned long long)cand);
        }
        hit[slot] = found;
        kp_j[slot] = out;
    }
}

}  // namespace satba

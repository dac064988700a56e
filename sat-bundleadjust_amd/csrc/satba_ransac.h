// Fundamental-matrix RANSAC of the pairwise matches (the rule: include/satba.h, satba_ransac_fundamental).
// Three kernels, each launched once for all pairs of a call, nothing passes between workgroups of one launch:
//   k_ransac_models  one lane per (pair, trial): sample, seven-point models (satba_ransac_geom.h), up to three matrices and their count
//   k_ransac_score   one workgroup per (pair, 16 trials): the pair's matches go through LDS tile by tile, a wave owns a model slot
//                    at a time and its lanes stride over the tile; (inlier count, error sum over the inliers) per slot
//   k_ransac_pick    one workgroup per pair: the best slot under a strict total order, then the mask, the matrix and `best`
// Sums of errors are taken in one order (lane-local in match order, a butterfly over the wave, tiles in order), the winner is the
// maximum of a total order: two runs give the same bytes.
#pragma once
#include <hip/hip_runtime.h>

#include "satba_ransac_geom.h"

constexpr int RSC_MODEL_THREADS = 64;
constexpr int RSC_SCORE_THREADS = 256;                              // 4 waves
constexpr int RSC_ITEM_TRIALS = 16;                                 // trials of one score item
constexpr int RSC_ITEM_SLOTS = 3 * RSC_ITEM_TRIALS;                 // model slots of one score item
constexpr int RSC_WAVE_SLOTS = RSC_ITEM_SLOTS / (RSC_SCORE_THREADS / 64);
constexpr int RSC_TILE = 2048;                                      // matches per LDS tile: 64 KB, two workgroups per CU
constexpr int RSC_PICK_THREADS = 256;

struct RansacArgs {
    const double* xy;            // n x 4
    const long long* ofs;        // n_pairs + 1
    const double* T;             // n_pairs x 6: the normalisation
    const unsigned char* live;   // n_pairs: 7 matches or more and a normalisation
    int n_pairs, n_trials;
    unsigned long long seed;
    double thr2;                 // max_err^2
    double* models;              // (n_pairs n_trials) x 3 x 9
    int* nmod;                   // n_pairs n_trials
    const int2* items;           // (pair, first trial) of every score item
    int tile;                    // matches per tile of this launch (<= RSC_TILE)
    int* cnt;                    // (n_pairs n_trials) x 3, -1: no model in the slot
    double* sum;
    unsigned char* inlier;       // n
    double* F;                   // n_pairs x 9
    int* best;                   // n_pairs x 3
};

__device__ inline void rsc_store_models(const RscModels& m, double* models, int* nmod, long long g) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        if (r < m.n) {
#pragma unroll
            for (int k = 0; k < 9; ++k) models[(g * 3 + r) * 9 + k] = m.F[r][k];
        }
    }
    nmod[g] = m.n;
}

__global__ __launch_bounds__(RSC_MODEL_THREADS) void k_ransac_models(RansacArgs a) {
    const long long g = (long long)blockIdx.x * RSC_MODEL_THREADS + threadIdx.x;
    if (g >= (long long)a.n_pairs * a.n_trials) return;
    const int p = (int)(g / a.n_trials), t = (int)(g % a.n_trials);
    if (!a.live[p]) { a.nmod[g] = 0; return; }
    const long long base = a.ofs[p], m = a.ofs[p + 1] - base;
    RscSample s;
    if (!rsc_sample(a.seed, (uint64_t)p, (uint64_t)a.n_trials, (uint64_t)t, (uint64_t)m, &s)) { a.nmod[g] = 0; return; }
    RscRows rows;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const double* q = a.xy + (base + s.i[j]) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) rows.v[j][e] = q[e];
    }
    if (rsc_rows_repeat(rows)) { a.nmod[g] = 0; return; }
    RscModels out;
    rsc_seven_point(rows, a.T + 6 * (long long)p, &out);
    rsc_store_models(out, a.models, a.nmod, g);
}

// test entry: the models of given samples of one pair (idx: n_samples x 7, checked by the host)
__global__ __launch_bounds__(RSC_MODEL_THREADS) void k_ransac_models_idx(const double* xy, const double* T, const int* idx, int n_samples,
                                                                          double* models, int* nmod) {
    const int g = blockIdx.x * RSC_MODEL_THREADS + threadIdx.x;
    if (g >= n_samples) return;
    RscRows rows;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
        const double* q = xy + (long long)idx[7 * g + j] * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) rows.v[j][e] = q[e];
    }
    if (rsc_rows_repeat(rows)) { nmod[g] = 0; return; }
    RscModels out;
    rsc_seven_point(rows, T, &out);
    rsc_store_models(out, models, nmod, g);
}

__global__ __launch_bounds__(RSC_SCORE_THREADS) void k_ransac_score(RansacArgs a) {
    extern __shared__ double rsc_lds[];  // 4 x tile: x1 | y1 | x2 | y2
    const int2 it = a.items[blockIdx.x];
    const int p = it.x, t0 = it.y, tile = a.tile;
    const long long base = a.ofs[p];
    const int m = (int)(a.ofs[p + 1] - base);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long g0 = (long long)p * a.n_trials;
    int cnt[RSC_WAVE_SLOTS];
    double sum[RSC_WAVE_SLOTS];
#pragma unroll
    for (int j = 0; j < RSC_WAVE_SLOTS; ++j) { cnt[j] = 0; sum[j] = 0.0; }
    for (int m0 = 0; m0 < m; m0 += tile) {
        const int rows = min(tile, m - m0);
        __syncthreads();  // the tile before this one has been read
        for (int i = threadIdx.x; i < rows; i += RSC_SCORE_THREADS) {
            const double2* q = reinterpret_cast<const double2*>(a.xy + (base + m0 + i) * 4);
            const double2 u = q[0], v = q[1];
            rsc_lds[i] = u.x; rsc_lds[tile + i] = u.y; rsc_lds[2 * tile + i] = v.x; rsc_lds[3 * tile + i] = v.y;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < RSC_WAVE_SLOTS; ++j) {
            const int slot = wave + (RSC_SCORE_THREADS / 64) * j, t = t0 + slot / 3, r = slot % 3;
            if (t >= a.n_trials || r >= a.nmod[g0 + t]) continue;  // the same for every lane of the wave
            const double* Fg = a.models + ((g0 + t) * 3 + r) * 9;
            double F[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) F[k] = Fg[k];
            double s = 0.0;
            int c = 0;
            for (int i0 = 0; i0 < rows; i0 += 64) {
                const int i = i0 + lane;
                bool in = false;
                double e = 0.0;
                if (i < rows) {
                    e = rsc_error(F, rsc_lds[i], rsc_lds[tile + i], rsc_lds[2 * tile + i], rsc_lds[3 * tile + i]);
                    in = e < a.thr2;
                }
                c += __popcll(__ballot(in));
                s += in ? e : 0.0;
            }
#pragma unroll
            for (int w = 32; w >= 1; w >>= 1) s += __shfl_xor(s, w, 64);
            cnt[j] += c;
            sum[j] += s;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < RSC_WAVE_SLOTS; ++j) {
            const int slot = wave + (RSC_SCORE_THREADS / 64) * j, t = t0 + slot / 3, r = slot % 3;
            if (t >= a.n_trials) continue;
            const bool has = r < a.nmod[g0 + t];
            a.cnt[(g0 + t) * 3 + r] = has ? cnt[j] : -1;
            a.sum[(g0 + t) * 3 + r] = has ? sum[j] : 0.0;
        }
    }
}

struct RscBest {
    int cnt, slot;  // slot = 3 trial + root
    double sum;
};

// the order of the rule: more inliers; then the lower trial; then, inside a trial, the smaller error sum; then the lower slot
__device__ inline bool rsc_better(const RscBest& x, const RscBest& y) {
    if (x.cnt != y.cnt) return x.cnt > y.cnt;
    if (x.slot / 3 != y.slot / 3) return x.slot / 3 < y.slot / 3;
    if (x.sum != y.sum) return x.sum < y.sum;
    return x.slot < y.slot;
}

__global__ __launch_bounds__(RSC_PICK_THREADS) void k_ransac_pick(RansacArgs a) {
    __shared__ int s_cnt[RSC_PICK_THREADS], s_slot[RSC_PICK_THREADS], s_n[RSC_PICK_THREADS];
    __shared__ double s_sum[RSC_PICK_THREADS];
    const int p = blockIdx.x, tid = threadIdx.x;
    const long long base = a.ofs[p];
    const int m = (int)(a.ofs[p + 1] - base);
    const long long g0 = (long long)p * a.n_trials;
    RscBest b{-1, 0x7fffffff, 0.0};
    int n_models = 0;
    if (a.live[p]) {
        for (int s = tid; s < 3 * a.n_trials; s += RSC_PICK_THREADS) {
            const RscBest x{a.cnt[g0 * 3 + s], s, a.sum[g0 * 3 + s]};
            if (x.cnt >= 0 && rsc_better(x, b)) b = x;
        }
        for (int t = tid; t < a.n_trials; t += RSC_PICK_THREADS) n_models += a.nmod[g0 + t];
    }
    s_cnt[tid] = b.cnt; s_slot[tid] = b.slot; s_sum[tid] = b.sum; s_n[tid] = n_models;
    __syncthreads();
    for (int w = RSC_PICK_THREADS / 2; w >= 1; w >>= 1) {
        if (tid < w) {
            const RscBest x{s_cnt[tid], s_slot[tid], s_sum[tid]}, y{s_cnt[tid + w], s_slot[tid + w], s_sum[tid + w]};
            if (y.cnt >= 0 && (x.cnt < 0 || rsc_better(y, x))) { s_cnt[tid] = y.cnt; s_slot[tid] = y.slot; s_sum[tid] = y.sum; }
            s_n[tid] += s_n[tid + w];
        }
        __syncthreads();
    }
    const int win_cnt = s_cnt[0], win_slot = s_slot[0];
    n_models = s_n[0];
    double F[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = win_cnt >= 0 ? a.models[(g0 * 3 + win_slot) * 9 + k] : 0.0;
    for (int i = tid; i < m; i += RSC_PICK_THREADS) {
        const double* q = a.xy + (base + i) * 4;
        a.inlier[base + i] = win_cnt < 0 ? 1 : (rsc_error(F, q[0], q[1], q[2], q[3]) < a.thr2 ? 1 : 0);
    }
    if (tid < 9) a.F[9 * (long long)p + tid] = win_cnt >= 0 ? a.models[(g0 * 3 + win_slot) * 9 + tid] : 0.0;
    if (tid == 0) {
        a.best[3 * p] = win_cnt >= 0 ? win_slot / 3 : -1;
        a.best[3 * p + 1] = win_cnt >= 0 ? win_cnt : m;
        a.best[3 * p + 2] = n_models;
    }
}

// satba_match.h -- pairwise SIFT matching (ref:bundle_adjust/feature_tracks/ft_match.py:76-133 and the matching() of
// ref:3rdparty/sift/simd/sift4ctypes.cpp:125-195): pack, select, nearest / second nearest, threshold.  Host side: satba_match_api.inc;
// DESIGN.md "Pairwise matching".
//
// The rule.  For a query i and the selected candidates j in ascending order: d(i, j) = sum (a - b)^2, +inf where the epipolar gate
// fails; distA the smallest d (lowest j among equals), distB the second smallest counted with multiplicity; a match when
// distA / distB (relative) or distA (absolute) < thr^2, all in float32.  Descriptors that are integers 0..255 give d <= 8 323 200 < 2^24:
// the reference's float32 sum is exact in any order, so the integer path computes d = |a'|^2 + |b'|^2 - 2 a'.b' in int32 with
// a' = a - 128 as int8 on the matrix cores and agrees bit for bit.
//
// Slots.  Every (pair, side) owns MT_TILE-aligned `cap` slots of one slot space: sel (global row of the selected keypoint, ascending),
// nrm_s (its squared norm), xx_s (its rectified coordinate).  A query's results live at its slot.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

namespace satba {

constexpr int MT_DESC = 128, MT_ROW = 132;  // descriptor length, floats per keypoint row
constexpr int MT_TILE = 16;                 // one MFMA tile: 16 candidates x 16 queries
constexpr int MT_QT = 4;                    // query tiles a wave keeps in registers
constexpr int MT_WQ = MT_TILE * MT_QT;      // queries per work item
constexpr int MT_WAVES = 4;                 // work items (waves) per workgroup of k_match_i8
constexpr int MT_SEL_THREADS = 1024;

struct MatchPair {
    int n[2];            // selected keypoints per side (filled on the device by k_match_select)
    int ofs[2];          // first slot per side, multiple of MT_TILE
    int cap[2];          // slots per side: keypoints of the image rounded up to MT_TILE
    int base[2];         // first global row of the side's image
    int cnt[2];          // keypoints of the side's image
    float s[2][3];       // rectifying similarities (a, b, q) of the two images
    double box[4];       // min_east, max_east, min_north, max_north
    long long part_ofs;  // first partial of the pair: [chunk][cap[0]]
    int n_chunks, pad_;
};
struct MatchItem { int pair, q0, c0, chunk; };
struct MatchPart { float dA, dB; int jA; };  // jA: candidate position inside the pair's second side, -1 none

using mt_v4i = __attribute__((ext_vector_type(4))) int;

// ---------------------------------------------------------------------------------------------------- pack
// One wave per keypoint row: int8 record of value - 128, squared norm of the record, (col, row).  flag |= 1 where a row that is not
// padding (col is NaN) holds a descriptor value that is not an integer in [0, 255].
__global__ __launch_bounds__(256) void k_match_pack(long long n_rows, const float* __restrict__ feat, signed char* __restrict__ rec, int* __restrict__ nrm,
                                                    float2* __restrict__ xy, int* __restrict__ flag) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= n_rows) return;
    const float* f = feat + row * MT_ROW;
    const float col = f[0];
    const bool padding = col != col;
    int sq = 0, bad = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int k = lane + 64 * h;
        const float v = f[4 + k];
        const bool ok = v >= 0.0f && v <= 255.0f && v == truncf(v);
        const int q = (ok && !padding) ? (int)v - 128 : 0;
        bad |= (!ok && !padding) ? 1 : 0;
        rec[row * MT_DESC + k] = (signed char)q;
        sq += q * q;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        sq += __shfl_xor(sq, m);
        bad |= __shfl_xor(bad, m);
    }
    if (lane == 0) {
        nrm[row] = sq;
        xy[row] = make_float2(col, f[1]);
        if (bad) atomicOr(flag, 1);
    }
}

// ---------------------------------------------------------------------------------------------------- select
// One workgroup per (pair, side): the keypoints strictly inside the box, ascending (an ordered compaction, tile by tile), with
// what the match kernels read per selected keypoint.  A NaN coordinate fails every comparison.
__global__ __launch_bounds__(MT_SEL_THREADS) void k_match_select(MatchPair* __restrict__ pairs, const double2* __restrict__ utm, const float2* __restrict__ xy,
                                                                 const int* __restrict__ nrm, int* __restrict__ sel, int* __restrict__ nrm_s,
                                                                 float* __restrict__ xx_s, int gate) {
    __shared__ int wave_cnt[MT_SEL_THREADS / 64];
    __shared__ int base_sh;
    MatchPair& P = pairs[blockIdx.x >> 1];
    const int side = blockIdx.x & 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = P.cnt[side], row0 = P.base[side], ofs = P.ofs[side];
    const double e0 = P.box[0], e1 = P.box[1], n0 = P.box[2], n1 = P.box[3];
    const float sa = P.s[side][0], sb = P.s[side][1], sq = P.s[side][2];
    if (tid == 0) base_sh = 0;
    __syncthreads();
    for (int t0 = 0; t0 < n; t0 += MT_SEL_THREADS) {
        const int k = t0 + tid;
        bool in = false;
        if (k < n) {
            const double2 u = utm[row0 + k];
            in = (u.x > e0) && (u.x < e1) && (u.y > n0) && (u.y < n1);
        }
        const unsigned long long mask = __ballot(in);
        if (lane == 0) wave_cnt[wave] = __popcll(mask);
        __syncthreads();
        int before = base_sh, total = 0;
        for (int w = 0; w < MT_SEL_THREADS / 64; ++w) {
            const int c = wave_cnt[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (in) {
            const int pos = before + __popcll(mask & ((1ull << lane) - 1ull));  // pos <= k < cap
            const int row = row0 + k;
            sel[ofs + pos] = row;
            nrm_s[ofs + pos] = nrm[row];
            const float2 p = xy[row];
            // xx = b * col + a * row + q, float32, in the reference's order and without contraction
            xx_s[ofs + pos] = gate ? __fadd_rn(__fadd_rn(__fmul_rn(sb, p.x), __fmul_rn(sa, p.y)), sq) : 0.0f;
        }
        __syncthreads();
        if (tid == 0) base_sh += total;
        __syncthreads();
    }
    if (tid == 0) P.n[side] = base_sh;
}

// ---------------------------------------------------------------------------------------------------- nearest two
// keep the two smallest of {a, b} + {oa, ob} (a <= b, oa <= ob), the first ordered by (d, j)
template <class T>
__device__ __forceinline__ void mt_merge(T& a, T& b, int& j, T oa, T ob, int oj) {
    if (oa < a || (oa == a && oj < j)) {
        b = a < ob ? a : ob;
        a = oa;
        j = oj;
    } else {
        b = b < oa ? b : oa;
    }
}

// Integer path.  A wave owns MT_WQ queries (B operand: column = lane & 15 of each tile, kept in registers for the whole item) and
// walks its chunk of candidates 16 at a time (A operand: row = lane & 15).  Both operands put bytes 16 g .. 16 g + 15 of a 64-byte
// K-step into lane group g = lane >> 4: whatever k the hardware gives those bytes, it is the same k on both sides, and a dot product
// does not care about the order.  Result tile: column (query) = lane & 15, row (candidate) = 4 g + register, so a lane sees its
// candidates in ascending order and the strict `<` of the reference keeps the lowest j; the four lane groups are merged by (d, j).
template <bool GATE>
__global__ __launch_bounds__(64 * MT_WAVES) void k_match_i8(int n_items, const MatchItem* __restrict__ items, const MatchPair* __restrict__ pairs,
                                                            const signed char* __restrict__ rec, const int* __restrict__ sel, const int* __restrict__ nrm_s,
                                                            const float* __restrict__ xx_s, int chunk, float epi_thr, MatchPart* __restrict__ part) {
    const int lane = threadIdx.x & 63, it = blockIdx.x * MT_WAVES + (threadIdx.x >> 6);
    if (it >= n_items) return;
    const MatchItem w = items[it];
    const MatchPair& P = pairs[w.pair];
    const int n_i = P.n[0], n_j = P.n[1], ofs_i = P.ofs[0], ofs_j = P.ofs[1];
    const int col = lane & 15, g = lane >> 4;

    mt_v4i bq[MT_QT][2];
    int nq[MT_QT], bA[MT_QT], bB[MT_QT], jA[MT_QT];
    float xq[MT_QT];
#pragma unroll
    for (int t = 0; t < MT_QT; ++t) {
        const int q = min(w.q0 + MT_TILE * t + col, n_i - 1);
        const mt_v4i* r = reinterpret_cast<const mt_v4i*>(rec + (long long)sel[ofs_i + q] * MT_DESC);
        bq[t][0] = r[g];
        bq[t][1] = r[4 + g];
        nq[t] = nrm_s[ofs_i + q];
        xq[t] = xx_s[ofs_i + q];
        bA[t] = INT_MAX; bB[t] = INT_MAX; jA[t] = -1;
    }
    const int c_end = min(w.c0 + chunk, n_j);
    for (int c = w.c0; c < c_end; c += MT_TILE) {
        const mt_v4i* r = reinterpret_cast<const mt_v4i*>(rec + (long long)sel[ofs_j + min(c + col, n_j - 1)] * MT_DESC);
        const mt_v4i a0 = r[g], a1 = r[4 + g];
        const int jb = c + 4 * g;  // this lane's four candidates; slots up to the side's cap exist, those past n_j are masked
        const int4 nb = *reinterpret_cast<const int4*>(nrm_s + ofs_j + jb);
        const int nbv[4] = {nb.x, nb.y, nb.z, nb.w};
        float xbv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (GATE) {
            const float4 xb = *reinterpret_cast<const float4*>(xx_s + ofs_j + jb);
            xbv[0] = xb.x; xbv[1] = xb.y; xbv[2] = xb.z; xbv[3] = xb.w;
        }
#pragma unroll
        for (int t = 0; t < MT_QT; ++t) {
            mt_v4i acc = {0, 0, 0, 0};
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, bq[t][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, bq[t][1], acc, 0, 0, 0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bool ok = jb + e < c_end;
                if (GATE) ok = ok && fabsf(__fsub_rn(xq[t], xbv[e])) < epi_thr;
                const int d = ok ? nq[t] + nbv[e] - 2 * acc[e] : INT_MAX;
                if (d < bA[t]) {
                    bB[t] = bA[t]; bA[t] = d; jA[t] = jb + e;
                } else if (d < bB[t]) {
                    bB[t] = d;
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < MT_QT; ++t) {
#pragma unroll
        for (int m = 16; m <= 32; m <<= 1) {
            const int oa = __shfl_xor(bA[t], m), ob = __shfl_xor(bB[t], m), oj = __shfl_xor(jA[t], m);
            mt_merge(bA[t], bB[t], jA[t], oa, ob, oj);
        }
        const int q = w.q0 + MT_TILE * t + col;
        if (g == 0 && q < n_i) {
            MatchPart o;
            o.dA = bA[t] == INT_MAX ? INFINITY : (float)bA[t];
            o.dB = bB[t] == INT_MAX ? INFINITY : (float)bB[t];
            o.jA = jA[t];
            part[P.part_ofs + (long long)w.chunk * P.cap[0] + q] = o;
        }
    }
}

// Float path: descriptors that are not all integers (or SATBA_MATCH_FLOAT=1).  One thread per query, the reference's loop as it
// stands: float32 accumulation in index order, no contraction.  Not tuned.
template <bool GATE>
__global__ __launch_bounds__(MT_WQ) void k_match_f32(int n_items, const MatchItem* __restrict__ items, const MatchPair* __restrict__ pairs,
                                                     const float* __restrict__ feat, const int* __restrict__ sel, const float* __restrict__ xx_s, int chunk,
                                                     float epi_thr, MatchPart* __restrict__ part) {
    __shared__ float qs[MT_DESC][MT_WQ];     // [k][query]: conflict-free
    __shared__ float cs[MT_TILE][MT_DESC];   // [candidate][k]: broadcast reads
    const MatchItem w = items[blockIdx.x];
    const MatchPair& P = pairs[w.pair];
    const int n_i = P.n[0], n_j = P.n[1], ofs_i = P.ofs[0], ofs_j = P.ofs[1], tid = threadIdx.x;
    for (int e = tid; e < MT_WQ * MT_DESC; e += MT_WQ) {
        const int q = e / MT_DESC, k = e % MT_DESC;
        qs[k][q] = feat[(long long)sel[ofs_i + min(w.q0 + q, n_i - 1)] * MT_ROW + 4 + k];
    }
    const int q = w.q0 + tid;
    const float xq = xx_s[ofs_i + min(q, n_i - 1)];
    float dA = INFINITY, dB = INFINITY;
    int jA = -1;
    const int c_end = min(w.c0 + chunk, n_j);
    for (int c = w.c0; c < c_end; c += MT_TILE) {
        __syncthreads();
        for (int e = tid; e < MT_TILE * MT_DESC; e += MT_WQ) {
            const int r = e / MT_DESC, k = e % MT_DESC;
            cs[r][k] = feat[(long long)sel[ofs_j + min(c + r, n_j - 1)] * MT_ROW + 4 + k];
        }
        __syncthreads();
        const int m = min(MT_TILE, c_end - c);
        for (int r = 0; r < m; ++r) {
            float d = INFINITY;
            if (!GATE || fabsf(__fsub_rn(xq, xx_s[ofs_j + c + r])) < epi_thr) {
                d = 0.0f;
                for (int k = 0; k < MT_DESC; ++k) {
                    const float t = __fsub_rn(qs[k][tid], cs[r][k]);
                    d = __fadd_rn(d, __fmul_rn(t, t));
                }
            }
            if (d < dA) {
                dB = dA; dA = d; jA = c + r;
            } else if (d < dB) {
                dB = d;
            }
        }
    }
    if (q < n_i) {
        MatchPart o;
        o.dA = dA; o.dB = dB; o.jA = jA;
        part[P.part_ofs + (long long)w.chunk * P.cap[0] + q] = o;
    }
}

// One thread per first-side slot: the chunks' partials merged in ascending order by (d, j), the threshold, the matched keypoint.
__global__ __launch_bounds__(256) void k_match_finish(int n_pairs, const MatchPair* __restrict__ pairs, const int* __restrict__ slot_pair, long long n_slots,
                                                      const int* __restrict__ sel, const MatchPart* __restrict__ part, float thr2, int relative,
                                                      int* __restrict__ hit, int* __restrict__ kp_j) {
    const long long slot = (long long)blockIdx.x * 256 + threadIdx.x;
    if (slot >= n_slots) return;
    int found = 0, out = -1;
    const int p = slot_pair[slot / MT_TILE];  // >= 0: the slot belongs to the first side of pair p
    if (p >= 0) {
        const MatchPair& P = pairs[p];
        const int q = (int)(slot - P.ofs[0]);
        if (q < P.n[0] && P.n[1] > 0) {
            float dA = INFINITY, dB = INFINITY;
            int jA = -1;
            for (int c = 0; c < P.n_chunks; ++c) {
                const MatchPart o = part[P.part_ofs + (long long)c * P.cap[0] + q];
                if (o.jA >= 0) {
                    if (jA < 0) { dA = o.dA; dB = o.dB; jA = o.jA; }
                    else mt_merge(dA, dB, jA, o.dA, o.dB, o.jA);
                }
            }
            const float val = relative ? __fdiv_rn(dA, dB) : dA;
            if (jA >= 0 && val < thr2) {
                found = 1;
                out = sel[P.ofs[1] + jA] - P.base[1];
            }
        }
    }
    hit[slot] = found;
    kp_j[slot] = out;
}

// the matches in slot order (pairs in the caller's order, queries ascending): pos = exclusive scan of hit
__global__ __launch_bounds__(256) void k_match_emit(long long n_slots, const MatchPair* __restrict__ pairs, const int* __restrict__ slot_pair,
                                                    const int* __restrict__ sel, const int* __restrict__ hit, const int* __restrict__ pos,
                                                    const int* __restrict__ kp_j, int* __restrict__ out_i, int* __restrict__ out_j) {
    const long long slot = (long long)blockIdx.x * 256 + threadIdx.x;
    if (slot >= n_slots || !hit[slot]) return;
    const MatchPair& P = pairs[slot_pair[slot / MT_TILE]];
    out_i[pos[slot]] = sel[slot] - P.base[0];
    out_j[pos[slot]] = kp_j[slot];
}

}  // namespace satba

// Feature tracks from pairwise matches on the device (ref:bundle_adjust/feature_tracks/ft_utils.py:65-182 with its baseline check
// :38-62; DESIGN.md "Track construction").  gfx950.  Stand-alone like satba_tracks.h: no problem handle, rocPRIM for the scans and
// the sort (satba_ftracks_api.inc).  Keypoint k of image m has the global id kp_ofs[m] + k; a match row (kp_i, kp_j, im_i, im_j) is
// an edge between two ids.  im_i > im_j is accepted and is the same edge; im_i == im_j is rejected by the entry (the reference's
// matcher only produces im_i < im_j).
//
//   k_ft_init        parent[i] = i, write key 0 (never matched), component size 0
//   k_ft_union       lane = match row: lock-free union-find, the larger root is hooked under the smaller by compare-and-swap
//   k_ft_keys        lane = match row: 64-bit atomic max of the write key per keypoint (row + 1 first side, n + row + 1 second side)
//   k_ft_flatten     lane = keypoint: final label = smallest id of its component, component sizes by integer atomics
//   k_ft_flags       lane = keypoint: "root of a component of >= 2" (its exclusive scan numbers the tracks) and "was matched"
//   k_ft_candidates  lane = keypoint: the matched keypoints, in id order, with the sort key track * n_cam + camera
//   k_ft_heads / k_ft_winners   runs of one (track, camera) cell in the sorted list: the keypoint with the largest write key wins
//   k_ft_has_pair    lane = track: does any camera pair (i < j) of the track have its bit in the matrix of listed pairs
//   k_ft_lengths / k_ft_emit    surviving tracks (fixed ones first for n_adj > 0) -> pt_ofs, cam_ind, kp_id, obs, scale
//
// Nothing is summed in floating point and nothing depends on arrival order: what meets across lanes is an integer add, an integer
// max, or a compare-and-swap whose outcome (the smallest id of the component) is the same for every schedule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define FT_THREADS 256

// While k_ft_union runs, other workgroups (on other XCDs, behind other L2s) change the parent array: every access to it is an
// agent-scope relaxed atomic, which is served by the coherent level.  No lane waits for another one: the loops below are the walk
// to the root and the retry after a lost compare-and-swap.
__device__ __forceinline__ int ft_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x, halving the path on the way.  A parent is always smaller than its child (roots are only ever hooked under smaller
// roots), so the walk ends; a halving store replaces a parent by an ancestor, which no concurrent hook can invalidate because hooks
// change roots only and x is not one.
__device__ __forceinline__ int ft_find(int* parent, int x) {
    for (;;) {
        const int p = ft_load(parent + x);
        if (p == x) return x;
        const int g = ft_load(parent + p);
        if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
    }
}

__global__ __launch_bounds__(FT_THREADS) void k_ft_init(int n_kp, int* __restrict__ parent, int* __restrict__ cnt,
                                                       unsigned long long* __restrict__ wkey) {
    const int i = blockIdx.x * FT_THREADS + threadIdx.x;
    if (i >= n_kp) return;
    parent[i] = i;
    cnt[i] = 0;
    wkey[i] = 0ull;
}

// global ids of the two sides of a row (validated on the host: images and keypoints in range, im_i != im_j)
__device__ __forceinline__ void ft_row_ids(const int* __restrict__ kp_ofs, const int* __restrict__ matches, int r, int& a, int& b) {
    const int4 m = reinterpret_cast<const int4*>(matches)[r];
    a = kp_ofs[m.z] + m.x;
    b = kp_ofs[m.w] + m.y;
}

__global__ __launch_bounds__(FT_THREADS) void k_ft_union(int n, const int* __restrict__ kp_ofs, const int* __restrict__ matches, int* parent) {
    const int r = blockIdx.x * FT_THREADS + threadIdx.x;
    if (r >= n) return;
    int a, b;
    ft_row_ids(kp_ofs, matches, r, a, b);
    for (;;) {
        a = ft_find(parent, a);
        b = ft_find(parent, b);
        if (a == b) break;
        const int lo = a < b ? a : b;
        int hi = a < b ? b : a;
        // hi was a root when it was read; if it still is, it becomes a child of lo.  Otherwise somebody hooked it: find again.
        if (__hip_atomic_compare_exchange_strong(parent + hi, &hi, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
    }
}

// The reference writes the first-side keypoints of all rows and then the second-side ones; inside one side the later row wins.
__global__ __launch_bounds__(FT_THREADS) void k_ft_keys(int n, const int* __restrict__ kp_ofs, const int* __restrict__ matches,
                                                       unsigned long long* __restrict__ wkey) {
    const int r = blockIdx.x * FT_THREADS + threadIdx.x;
    if (r >= n) return;
    int a, b;
    ft_row_ids(kp_ofs, matches, r, a, b);
    atomicMax(wkey + a, (unsigned long long)r + 1ull);
    atomicMax(wkey + b, (unsigned long long)n + (unsigned long long)r + 1ull);
}

// a launch of its own: k_ft_union has finished, the parents no longer change (the walk does not write them either)
__global__ __launch_bounds__(FT_THREADS) void k_ft_flatten(int n_kp, const int* __restrict__ parent, int* __restrict__ label, int* __restrict__ cnt) {
    const int i = blockIdx.x * FT_THREADS + threadIdx.x;
    if (i >= n_kp) return;
    int x = i;
    for (int p = parent[x]; p != x; p = parent[x]) x = p;
    label[i] = x;
    atomicAdd(cnt + x, 1);
}

// is_root / is_matched have n_kp + 1 entries, the last one 0: their exclusive scans end with the totals
__global__ __launch_bounds__(FT_THREADS) void k_ft_flags(int n_kp, const int* __restrict__ label, const int* __restrict__ cnt,
                                                        const unsigned long long* __restrict__ wkey, int* __restrict__ is_root,
                                                        int* __restrict__ is_matched) {
    const int i = blockIdx.x * FT_THREADS + threadIdx.x;
    if (i > n_kp) return;
    is_root[i] = i < n_kp && label[i] == i && cnt[i] >= 2;
    is_matched[i] = i < n_kp && wkey[i] != 0ull;
}

// image of a global id: the last m with kp_ofs[m] <= id (images without keypoints repeat an offset and are skipped by "last")
__device__ __forceinline__ int ft_image_of(const int* __restrict__ kp_ofs, int n_cam, int id) {
    int lo = 0, hi = n_cam;  // kp_ofs[lo] <= id < kp_ofs[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (kp_ofs[mid] <= id) lo = mid;
        else hi = mid;
    }
    return lo;
}

// A matched keypoint belongs to a component of at least 2 (its row's two sides differ), so its root has a track number.
__global__ __launch_bounds__(FT_THREADS) void k_ft_candidates(int n_kp, int n_cam, const int* __restrict__ kp_ofs, const int* __restrict__ label,
                                                             const int* __restrict__ track_of_root, const int* __restrict__ is_matched,
                                                             const int* __restrict__ pos, unsigned long long* __restrict__ key, int* __restrict__ id) {
    const int i = blockIdx.x * FT_THREADS + threadIdx.x;
    if (i >= n_kp || !is_matched[i]) return;
    const int q = pos[i];
    key[q] = (unsigned long long)track_of_root[label[i]] * (unsigned long long)n_cam + (unsigned long long)ft_image_of(kp_ofs, n_cam, i);
    id[q] = i;
}

// head[s] = 1 where a (track, camera) cell begins in the sorted list (n_c + 1 entries, the last one 0)
__global__ __launch_bounds__(FT_THREADS) void k_ft_heads(int n_c, const unsigned long long* __restrict__ key, int* __restrict__ head) {
    const int s = blockIdx.x * FT_THREADS + threadIdx.x;
    if (s > n_c) return;
    head[s] = s < n_c && (s == 0 || key[s] != key[s - 1]);
}

// lane = head of a cell: the claimant with the largest write key is the observation (write keys are distinct: one per row and side).
// The cells come out track-major with cameras ascending strictly: cell_pos is the exclusive scan of head.  tr_ofs (n_tr + 1).
__global__ __launch_bounds__(FT_THREADS) void k_ft_winners(int n_c, int n_cam, int n_tr, const unsigned long long* __restrict__ key,
                                                          const int* __restrict__ id, const int* __restrict__ head, const int* __restrict__ cell_pos,
                                                          const unsigned long long* __restrict__ wkey, int* __restrict__ cell_trk,
                                                          int* __restrict__ cell_cam, int* __restrict__ cell_kp, int* __restrict__ tr_ofs,
                                                          int* __restrict__ n_conflicts) {
    const int s = blockIdx.x * FT_THREADS + threadIdx.x;
    if (s >= n_c || !head[s]) return;
    const unsigned long long k = key[s];
    int best = id[s];
    unsigned long long bw = wkey[best];
    int e = s + 1;
    for (; e < n_c && key[e] == k; ++e) {
        const int c = id[e];
        const unsigned long long w = wkey[c];
        if (w > bw) { bw = w; best = c; }
    }
    if (e - s > 1) atomicAdd(n_conflicts, 1);
    const int t = (int)(k / (unsigned long long)n_cam);
    const int q = cell_pos[s];
    cell_trk[q] = t;
    cell_cam[q] = (int)(k % (unsigned long long)n_cam);
    cell_kp[q] = best;
    if (s == 0 || (int)(key[s - 1] / (unsigned long long)n_cam) != t) tr_ofs[t] = q;
    if (s == 0) tr_ofs[n_tr] = cell_pos[n_c];
}

// Baseline check (ft_utils.py:38-62).  bits: n_cam * n_cam bits, bit i * n_cam + j set for every listed pair with i < j < n_cam
// (built on the host, so a pair listed as (j, i) or naming a camera >= n_cam never matches).  L (L - 1) / 2 tests for a track of
// length L, ended by the first hit.  LDS: the matrix is copied into dynamic LDS first.
// group (2 * n_tr + 1 entries, the last one 0; may be null): with n_adj > 0 a surviving track flags slot t if none of its cameras is
// >= n_adj ("fixed") and slot n_tr + t otherwise, so that one exclusive scan is the stable fixed-first partition; n_adj == 0 puts
// every survivor in the second half.
template <bool LDS>
__global__ __launch_bounds__(FT_THREADS) void k_ft_has_pair(int n_tr, int n_cam, int n_adj, const int* __restrict__ tr_ofs, const int* __restrict__ cell_cam,
                                                           const unsigned* __restrict__ bits, long long n_words, unsigned char* __restrict__ keep,
                                                           int* __restrict__ group) {
    extern __shared__ unsigned ft_lds[];
    if (LDS) {
        for (long long w = threadIdx.x; w < n_words; w += FT_THREADS) ft_lds[w] = bits[w];
        __syncthreads();
    }
    const unsigned* tab = LDS ? ft_lds : bits;
    for (int t = blockIdx.x * FT_THREADS + threadIdx.x; t < n_tr; t += gridDim.x * FT_THREADS) {
        const int o0 = tr_ofs[t], o1 = tr_ofs[t + 1];
        int found = 0;
        for (int a = o0; a < o1 && !found; ++a) {
            const long long row = (long long)cell_cam[a] * n_cam;
            for (int b = a + 1; b < o1; ++b) {
                const long long bit = row + cell_cam[b];  // cameras ascend strictly inside a track: i < j
                if ((tab[bit >> 5] >> (bit & 31)) & 1u) { found = 1; break; }
            }
        }
        if (keep) keep[t] = (unsigned char)found;
        if (group) {
            const int fixed = n_adj > 0 && cell_cam[o1 - 1] < n_adj;  // the last camera is the largest
            group[t] = found && fixed;
            group[n_tr + t] = found && !fixed;
            if (t == 0) group[2 * n_tr] = 0;
        }
    }
}

// new_len has n_out + 1 entries (zeroed before): its exclusive scan is pt_ofs
__global__ __launch_bounds__(FT_THREADS) void k_ft_lengths(int n_tr, const int* __restrict__ tr_ofs, const int* __restrict__ group,
                                                          const int* __restrict__ slot, int* __restrict__ new_trk, int* __restrict__ new_len) {
    const int t = blockIdx.x * FT_THREADS + threadIdx.x;
    if (t >= n_tr) return;
    int q = -1;
    if (group[t]) q = slot[t];
    else if (group[n_tr + t]) q = slot[n_tr + t];
    new_trk[t] = q;
    if (q >= 0) new_len[q] = tr_ofs[t + 1] - tr_ofs[t];
}

// lane = cell before the check.  kp: n_kp x 3 float32 (x, y, scale), widened exactly.
__global__ __launch_bounds__(FT_THREADS) void k_ft_emit(int n_cells, const int* __restrict__ cell_trk, const int* __restrict__ cell_cam,
                                                       const int* __restrict__ cell_kp, const int* __restrict__ tr_ofs, const int* __restrict__ new_trk,
                                                       const int* __restrict__ pt_ofs, const int* __restrict__ kp_ofs, const float* __restrict__ kp,
                                                       int* __restrict__ cam_ind, int* __restrict__ kp_id, double* __restrict__ obs,
                                                       double* __restrict__ scale) {
    const int c = blockIdx.x * FT_THREADS + threadIdx.x;
    if (c >= n_cells) return;
    const int t = cell_trk[c];
    const int q = new_trk[t];
    if (q < 0) return;
    const int o = pt_ofs[q] + (c - tr_ofs[t]);
    const int cam = cell_cam[c], g = cell_kp[c];
    cam_ind[o] = cam;
    kp_id[o] = g - kp_ofs[cam];
    obs[2 * (size_t)o] = (double)kp[3 * (size_t)g];
    obs[2 * (size_t)o + 1] = (double)kp[3 * (size_t)g + 1];
    scale[o] = (double)kp[3 * (size_t)g + 2];
}

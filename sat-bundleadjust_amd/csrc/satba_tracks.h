// Feature-track selection on the device (ref:bundle_adjust/feature_tracks/ft_ranking.py; DESIGN.md "Track selection").
// gfx950, lane = track as in satba_kernels.h.  The tracks come as the observation lists satba_init_pts3d takes: pt_ofs (N + 1),
// cam_ind (K, cameras ascending strictly inside a track) plus one keypoint scale and one reprojection error per observation.
//
//   k_trk_keys        the three ranking keys of every track (ft_ranking.py:145-147) and their order-preserving integer images
//   k_trk_iota_desc / k_trk_scatter_rank   around the three stable radix sorts of the ranking (rocPRIM, satba_tracks_api.inc)
//   k_trk_connect     pair counts of the live tracks, integer atomics (LDS table per workgroup when it fits)   (:19-34)
//   k_trk_connect_finish   symmetric matrix with the entries below min_matches zeroed (satba_track_connectivity)
//   k_trk_weights     per camera: neighbours, mean and population deviation of the live tracks' costs -> weight  (:83-118)
//   k_trk_tree_begin  root = first camera of maximal weight, empty reached / layer sets                          (:204-207)
//   k_trk_claim       one layer: 64-bit atomic min of (layer order * N + rank) per camera not yet reached        (:211-222)
//   k_trk_commit      claimants -> selected, new cameras -> reached, next layer by decreasing weight             (:224-227)
//
// Nothing here sums floating-point numbers in an order that depends on the schedule: the per-camera sums walk the camera's track
// list (ascending track index) with a fixed assignment of entries to threads and a fixed tree over the threads; everything
// else that meets across threads is an integer add or an integer min.
#pragma once
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#include <stdint.h>

#define TRK_THREADS 256
#define TRK_NONE 0xffffffffffffffffull

// ascending unsigned order == ascending order of the doubles (-0.0 is folded onto 0.0 first: numpy's `<` does not tell them apart)
__device__ __forceinline__ unsigned long long trk_image(double v) {
    v = v + 0.0;
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// length = observations, scale = rint(mean * 100) / 100 (np.round(., 2)), cost = mean; the sums run in ascending camera order and
// are divided by the count, which is np.nanmean over a column of a C-ordered matrix.  err == nullptr: zeros.
// img (3 x N, may be null): complemented images of (length, -scale, -cost): sorting them ASCENDING is the reference's ranking.
__global__ __launch_bounds__(TRK_THREADS) void k_trk_keys(int N, const int* __restrict__ pt_ofs, const double* __restrict__ scale,
                                                         const double* __restrict__ err, int* __restrict__ len, double* __restrict__ k_scale,
                                                         double* __restrict__ k_cost, unsigned long long* __restrict__ img) {
    const int t = blockIdx.x * TRK_THREADS + threadIdx.x;
    if (t >= N) return;
    const int o0 = pt_ofs[t], o1 = pt_ofs[t + 1];
    double s = 0.0, e = 0.0;
    for (int o = o0; o < o1; ++o) {
        s += scale[o];
        if (err) e += err[o];
    }
    const double n = (double)(o1 - o0);
    const double ms = s / n, mc = e / n;  // 0 / 0 = NaN for a track without observations, like np.nanmean
    const double rs = rint(ms * 100.0) / 100.0;
    len[t] = o1 - o0;
    k_scale[t] = rs;
    k_cost[t] = mc;
    if (img) {
        img[t] = ~(unsigned long long)(unsigned)(o1 - o0);
        img[(size_t)N + t] = ~trk_image(-rs);
        img[2 * (size_t)N + t] = ~trk_image(-mc);
    }
}

// the sorts are stable and ascending: starting from N-1 .. 0 puts the higher track index first among exact ties
__global__ __launch_bounds__(TRK_THREADS) void k_trk_iota_desc(int N, int* __restrict__ idx) {
    const int t = blockIdx.x * TRK_THREADS + threadIdx.x;
    if (t < N) idx[t] = N - 1 - t;
}

__global__ __launch_bounds__(TRK_THREADS) void k_trk_gather(int N, const int* __restrict__ idx, const unsigned long long* __restrict__ src,
                                                           unsigned long long* __restrict__ dst) {
    const int t = blockIdx.x * TRK_THREADS + threadIdx.x;
    if (t < N) dst[t] = src[idx[t]];
}

__global__ __launch_bounds__(TRK_THREADS) void k_trk_scatter_rank(int N, const int* __restrict__ order, int* __restrict__ rank) {
    const int r = blockIdx.x * TRK_THREADS + threadIdx.x;
    if (r < N) rank[order[r]] = r;
}

// the track of every observation (the values of the sort that groups the observations by camera)
__global__ __launch_bounds__(TRK_THREADS) void k_trk_obs_track(int N, const int* __restrict__ pt_ofs, int* __restrict__ obs_trk) {
    const int t = blockIdx.x * TRK_THREADS + threadIdx.x;
    if (t >= N) return;
    for (int o = pt_ofs[t]; o < pt_ofs[t + 1]; ++o) obs_trk[o] = t;
}

// packed upper triangle: (i, j), i < j
__device__ __forceinline__ int trk_tri(int M, int i, int j) { return i * M - (i * (i + 1)) / 2 + (j - i - 1); }

// pair counts over the live tracks (alive == nullptr: all; otherwise alive[t] < 0 is live -- tree_of doubles as the mask -- or, with
// alive_is_mask, alive[t] != 0).  LDS: the packed triangle lives in dynamic LDS per workgroup and is flushed with one integer
// atomic per non-zero entry; otherwise the atomics go to the global triangle directly.  Integer adds commute: the counts do not
// depend on the schedule.
template <bool LDS>
__global__ __launch_bounds__(TRK_THREADS) void k_trk_connect(int N, int M, const int* __restrict__ pt_ofs, const int* __restrict__ cam_ind,
                                                            const int* __restrict__ alive, int alive_is_mask, int* __restrict__ tri) {
    extern __shared__ int trk_lds[];
    const int n_tri = M * (M - 1) / 2;
    if (LDS) {
        for (int i = threadIdx.x; i < n_tri; i += TRK_THREADS) trk_lds[i] = 0;
        __syncthreads();
    }
    for (int t = blockIdx.x * TRK_THREADS + threadIdx.x; t < N; t += gridDim.x * TRK_THREADS) {
        if (alive && (alive_is_mask ? alive[t] == 0 : alive[t] >= 0)) continue;
        const int o0 = pt_ofs[t], o1 = pt_ofs[t + 1];
        for (int a = o0; a < o1; ++a) {
            const int ci = cam_ind[a];
            for (int b = a + 1; b < o1; ++b) {
                const int e = trk_tri(M, ci, cam_ind[b]);  // cameras ascend strictly inside a track (checked on the host)
                if (LDS) atomicAdd(&trk_lds[e], 1);
                else atomicAdd(&tri[e], 1);
            }
        }
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < n_tri; i += TRK_THREADS) {
            const int v = trk_lds[i];
            if (v) atomicAdd(&tri[i], v);
        }
    }
}

__global__ __launch_bounds__(TRK_THREADS) void k_trk_connect_finish(int M, const int* __restrict__ tri, int min_matches, int* __restrict__ A) {
    const int e = blockIdx.x * TRK_THREADS + threadIdx.x;
    if (e >= M * M) return;
    const int i = e / M, j = e % M;
    int v = 0;
    if (i != j) v = tri[trk_tri(M, i < j ? i : j, i < j ? j : i)];
    A[e] = v < min_matches ? 0 : v;
}

// fixed tree over the workgroup's threads
__device__ __forceinline__ double trk_block_sum(double v, double* sh) {
    __syncthreads();
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = TRK_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

// one workgroup per camera c: neighbours = cameras sharing a live track (tri > 0), cost statistics over the live tracks it sees
// (cm_trk[cam_ofs[c] .. cam_ofs[c+1]): its tracks, ascending); weight = neighbours + exp(-(mean + 3 std)), 1.0 without neighbours.
// `cost` is the key of the whole track (k_trk_keys): the reference does not recompute it per tree either (ft_ranking.py:109).
__global__ __launch_bounds__(TRK_THREADS) void k_trk_weights(int M, const int* __restrict__ cam_ofs, const int* __restrict__ cm_trk,
                                                            const int* __restrict__ tree_of, const double* __restrict__ cost,
                                                            const int* __restrict__ tri, double* __restrict__ w, double* __restrict__ w_out) {
    __shared__ double sh[TRK_THREADS];
    const int c = blockIdx.x;
    double nb = 0.0;
    for (int j = threadIdx.x; j < M; j += TRK_THREADS)
        if (j != c && tri[trk_tri(M, j < c ? j : c, j < c ? c : j)] > 0) nb += 1.0;
    nb = trk_block_sum(nb, sh);
    double weight = 1.0;
    if (nb > 0.0) {  // uniform over the workgroup
        const int o0 = cam_ofs[c], o1 = cam_ofs[c + 1];
        double s = 0.0, n = 0.0;
        for (int o = o0 + threadIdx.x; o < o1; o += TRK_THREADS) {
            const int t = cm_trk[o];
            if (tree_of[t] < 0) { s += cost[t]; n += 1.0; }
        }
        s = trk_block_sum(s, sh);
        n = trk_block_sum(n, sh);
        const double mean = s / n;
        double q = 0.0;
        for (int o = o0 + threadIdx.x; o < o1; o += TRK_THREADS) {
            const int t = cm_trk[o];
            if (tree_of[t] < 0) { const double d = cost[t] - mean; q += d * d; }
        }
        q = trk_block_sum(q, sh);
        weight = nb + exp(-(mean + 3.0 * sqrt(q / n)));
    }
    if (threadIdx.x == 0) {
        w[c] = weight;
        if (w_out) w_out[c] = weight;
    }
}

// status words of the tree loop (read back once per layer)
enum { TRK_ST_NEW = 0, TRK_ST_REACHED, TRK_ST_SELECTED, TRK_ST_TREE_SELECTED, TRK_ST_LEN };

// one workgroup: root = first camera of maximal weight (np.argmax), layer = {root}, reached = {root}, every slot empty
__global__ __launch_bounds__(TRK_THREADS) void k_trk_tree_begin(int M, const double* __restrict__ w, int* __restrict__ reached,
                                                               int* __restrict__ layer_pos, unsigned long long* __restrict__ slot,
                                                               int* __restrict__ status) {
    __shared__ double sh_w[TRK_THREADS];
    __shared__ int sh_i[TRK_THREADS];
    double bw = -1.0;
    int bi = M;
    for (int c = threadIdx.x; c < M; c += TRK_THREADS)
        if (w[c] > bw) { bw = w[c]; bi = c; }  // ascending c: the first maximum of this thread's cameras
    sh_w[threadIdx.x] = bw; sh_i[threadIdx.x] = bi;
    __syncthreads();
    for (int s = TRK_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const double ow = sh_w[threadIdx.x + s];
            const int oi = sh_i[threadIdx.x + s];
            if (ow > sh_w[threadIdx.x] || (ow == sh_w[threadIdx.x] && oi < sh_i[threadIdx.x])) { sh_w[threadIdx.x] = ow; sh_i[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    const int root = sh_i[0];
    for (int c = threadIdx.x; c < M; c += TRK_THREADS) {
        reached[c] = c == root;
        layer_pos[c] = c == root ? 0 : -1;
        slot[c] = TRK_NONE;
    }
    if (threadIdx.x == 0) { status[TRK_ST_NEW] = 0; status[TRK_ST_REACHED] = 1; status[TRK_ST_TREE_SELECTED] = 0; }
}

// One layer.  A live track that sees a layer camera is visited first at (lowest layer order among its cameras, its rank); it is
// taken iff it is the first visitor of a camera not yet reached, i.e. iff it holds the minimum of that camera's slot.
__global__ __launch_bounds__(TRK_THREADS) void k_trk_claim(int N, const int* __restrict__ pt_ofs, const int* __restrict__ cam_ind,
                                                          const int* __restrict__ tree_of, const int* __restrict__ rank,
                                                          const int* __restrict__ layer_pos, const int* __restrict__ reached,
                                                          unsigned long long* __restrict__ slot) {
    const int t = blockIdx.x * TRK_THREADS + threadIdx.x;
    if (t >= N || tree_of[t] >= 0) return;
    const int o0 = pt_ofs[t], o1 = pt_ofs[t + 1];
    int lo = 0x7fffffff, open = 0;
    for (int o = o0; o < o1; ++o) {
        const int c = cam_ind[o];
        const int lp = layer_pos[c];
        if (lp >= 0 && lp < lo) lo = lp;
        open |= !reached[c];
    }
    if (lo == 0x7fffffff || !open) return;
    const unsigned long long key = (unsigned long long)lo * (unsigned long long)N + (unsigned long long)rank[t];
    for (int o = o0; o < o1; ++o) {
        const int c = cam_ind[o];
        if (!reached[c]) atomicMin(&slot[c], key);
    }
}

// one workgroup: the claimants are selected into tree k, their cameras are reached, and these cameras, by decreasing weight (the
// lower index first among equal weights), are the next layer.  Works for any M: the sets are arrays, not bit masks.
__global__ __launch_bounds__(TRK_THREADS) void k_trk_commit(int M, int N, int k, const double* __restrict__ w, const int* __restrict__ order,
                                                           int* __restrict__ tree_of, int* __restrict__ reached, int* __restrict__ layer_pos,
                                                           unsigned long long* __restrict__ slot, int* __restrict__ status) {
    __shared__ int n_new, n_sel;
    if (threadIdx.x == 0) { n_new = 0; n_sel = 0; }
    __syncthreads();
    int my_new = 0, my_sel = 0;
    for (int c = threadIdx.x; c < M; c += TRK_THREADS) {
        const unsigned long long s = slot[c];
        if (s == TRK_NONE) continue;
        const int t = order[(int)(s % (unsigned long long)N)];
        if (atomicCAS(&tree_of[t], -1, k) == -1) ++my_sel;  // one claimant may hold several cameras: counted once
        ++my_new;
    }
    if (my_new) atomicAdd(&n_new, my_new);
    if (my_sel) atomicAdd(&n_sel, my_sel);
    __syncthreads();
    for (int c = threadIdx.x; c < M; c += TRK_THREADS) {
        int pos = -1;
        if (slot[c] != TRK_NONE) {
            pos = 0;
            const double wc = w[c];
            for (int d = 0; d < M; ++d)
                if (slot[d] != TRK_NONE && (w[d] > wc || (w[d] == wc && d < c))) ++pos;
        }
        layer_pos[c] = pos;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < M; c += TRK_THREADS)
        if (slot[c] != TRK_NONE) { reached[c] = 1; slot[c] = TRK_NONE; }
    if (threadIdx.x == 0) {
        status[TRK_ST_NEW] = n_new;
        status[TRK_ST_REACHED] += n_new;
        status[TRK_ST_SELECTED] += n_sel;
        status[TRK_ST_TREE_SELECTED] += n_sel;
    }
}

// satba_track_keys / satba_track_connectivity / satba_select_tracks (include/satba.h): part of the extern "C" block of satba_capi.hip.
// Stand-alone entry points (no problem handle), like satba_init_pts3d: the selection runs before a BundleAdjustmentParameters
// object for the selected tracks exists.  Kernels: satba_tracks.h.
extern "C++" {
namespace {
// the observation lists on the host: checked (offsets monotone, cameras in range and strictly ascending inside a track), narrowed to
// 32 bits; cam_cnt (may be null): observations per camera
int trk_check_lists(int32_t n_cam, int64_t n_pts, const int64_t* pt_ofs, const int32_t* cam_ind, std::vector<int>& ofs32, std::vector<int>* cam_cnt) {
    if (n_cam <= 0 || n_pts < 0 || !pt_ofs) return fail(SATBA_E_ARG, "null or negative argument");
    if (n_cam >= 46341) return fail(SATBA_E_ARG, "the pair table holds fewer than 46 341 cameras");
    TRY(dev_check_offsets(n_pts, pt_ofs, cam_ind != nullptr, ofs32));
    if (cam_cnt) cam_cnt->assign((size_t)n_cam, 0);
    for (int64_t i = 0; i < n_pts; ++i)
        for (int64_t o = pt_ofs[i]; o < pt_ofs[i + 1]; ++o) {
            if (cam_ind[o] < 0 || cam_ind[o] >= n_cam) return fail(SATBA_E_ARG, "camera index %d out of range", cam_ind[o]);
            if (o > pt_ofs[i] && cam_ind[o] <= cam_ind[o - 1]) return fail(SATBA_E_ARG, "cameras must ascend strictly inside a track (track %lld)", (long long)i);
            if (cam_cnt) ++(*cam_cnt)[(size_t)cam_ind[o]];
        }
    return 0;
}

// pair counts of the live tracks into the packed triangle d_tri (zeroed here)
int trk_connect(DevRun& s, int N, int M, const int* d_ofs, const int* d_cam, const int* d_alive, int alive_is_mask, int* d_tri, int lds_optin) {
    const size_t tri_bytes = sizeof(int) * (size_t)std::max(M * (M - 1) / 2, 1);
    HIP_TRY(hipMemsetAsync(d_tri, 0, tri_bytes, s.stream));
    if (!N || M < 2) return 0;
    const unsigned blocks = (unsigned)std::min<long long>(((long long)N + TRK_THREADS - 1) / TRK_THREADS, 1024);
    if ((long long)tri_bytes + 1024 <= (long long)lds_optin) {
        if (tri_bytes > 48 * 1024)
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_trk_connect<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tri_bytes));
        hipLaunchKernelGGL(k_trk_connect<true>, dim3(blocks), dim3(TRK_THREADS), tri_bytes, s.stream, N, M, d_ofs, d_cam, d_alive, alive_is_mask, d_tri);
    } else {
        hipLaunchKernelGGL(k_trk_connect<false>, dim3(blocks), dim3(TRK_THREADS), 0, s.stream, N, M, d_ofs, d_cam, d_alive, alive_is_mask, d_tri);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// priority: up to three of 0 length, 1 scale, 2 cost (-1: unused); the missing ones follow in that order (numpy's rule for `order=`)
int trk_priority(const int32_t* priority, int out[3]) {
    int n = 0;
    bool seen[3] = {false, false, false};
    for (int i = 0; i < 3 && priority; ++i) {
        const int q = priority[i];
        if (q == -1) continue;
        if (q < 0 || q > 2) return fail(SATBA_E_ARG, "priority names are 0 length, 1 scale, 2 cost (or -1); got %d", q);
        if (seen[q]) return fail(SATBA_E_ARG, "priority names key %d twice", q);
        seen[q] = true;
        out[n++] = q;
    }
    for (int q = 0; q < 3; ++q)
        if (!seen[q]) out[n++] = q;
    return 0;
}
}  // namespace
}  // extern "C++"

int satba_track_keys(int64_t n_pts, const int64_t* pt_ofs, const double* scale, const double* err, int32_t* length, double* key_scale,
                     double* key_cost, int32_t device) {
    if (n_pts < 0 || !pt_ofs || (n_pts && (!length || !key_scale || !key_cost))) return fail(SATBA_E_ARG, "null or negative argument");
    std::vector<int> ofs32;
    TRY(dev_check_offsets(n_pts, pt_ofs, scale != nullptr, ofs32));
    const int64_t K = pt_ofs[n_pts];
    DevRun s;
    TRY(s.begin(device));
    int *d_ofs, *d_len;
    double *d_scale, *d_err = nullptr, *d_ks, *d_kc;
    TRY(s.upload(&d_ofs, ofs32.data(), ofs32.size())); TRY(s.upload(&d_scale, scale, (size_t)K));
    if (err) TRY(s.upload(&d_err, err, (size_t)K));
    TRY(s.alloc(&d_len, (size_t)n_pts)); TRY(s.alloc(&d_ks, (size_t)n_pts));
    TRY(s.alloc(&d_kc, (size_t)n_pts));
    if (n_pts) {
        hipLaunchKernelGGL(k_trk_keys, dim3((unsigned)((n_pts + TRK_THREADS - 1) / TRK_THREADS)), dim3(TRK_THREADS), 0, s.stream, (int)n_pts, d_ofs,
                           d_scale, d_err, d_len, d_ks, d_kc, (unsigned long long*)nullptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(length, d_len, sizeof(int) * n_pts, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipMemcpyAsync(key_scale, d_ks, sizeof(double) * n_pts, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipMemcpyAsync(key_cost, d_kc, sizeof(double) * n_pts, hipMemcpyDeviceToHost, s.stream));
    }
    HIP_TRY(hipStreamSynchronize(s.stream));
    return 0;
}

int satba_track_connectivity(int32_t n_cam, int64_t n_pts, const int64_t* pt_ofs, const int32_t* cam_ind, const uint8_t* alive,
                             int32_t min_matches, int32_t* A, int32_t device) {
    if (!A) return fail(SATBA_E_ARG, "null argument");
    std::vector<int> ofs32;
    TRY(trk_check_lists(n_cam, n_pts, pt_ofs, cam_ind, ofs32, nullptr));
    const int64_t K = pt_ofs[n_pts];
    DevRun s;
    TRY(s.begin(device));
    int *d_ofs, *d_cam, *d_alive = nullptr, *d_tri, *d_A;
    TRY(s.upload(&d_ofs, ofs32.data(), ofs32.size())); TRY(s.upload(&d_cam, cam_ind, (size_t)K));
    if (alive) {
        std::vector<int> a32((size_t)n_pts);
        for (int64_t i = 0; i < n_pts; ++i) a32[(size_t)i] = alive[i] != 0;
        TRY(s.upload(&d_alive, a32.data(), a32.size()));
        HIP_TRY(hipStreamSynchronize(s.stream));  // a32 leaves scope
    }
    const int M = n_cam;
    TRY(s.alloc(&d_tri, (size_t)std::max(M * (M - 1) / 2, 1))); TRY(s.alloc(&d_A, (size_t)M * M));
    TRY(trk_connect(s, (int)n_pts, M, d_ofs, d_cam, d_alive, 1, d_tri, dev_lds_limit(device)));
    hipLaunchKernelGGL(k_trk_connect_finish, dim3((unsigned)(((long long)M * M + TRK_THREADS - 1) / TRK_THREADS)), dim3(TRK_THREADS), 0, s.stream, M,
                       d_tri, (int)min_matches, d_A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(A, d_A, sizeof(int) * (size_t)M * M, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    return 0;
}

int satba_select_tracks(int32_t n_cam, int64_t n_pts, const int64_t* pt_ofs, const int32_t* cam_ind, const double* scale, const double* err,
                        int32_t K, const int32_t* priority, int32_t* tree_of, int64_t* n_selected, int32_t* n_trees, double* weights,
                        int64_t* rank, int32_t device, float* kernel_ms) {
    if (K < 0) return fail(SATBA_E_ARG, "K must not be negative");
    if (!priority || !n_selected || !n_trees || (n_pts > 0 && !tree_of)) return fail(SATBA_E_ARG, "null argument");
    int prio[3];
    TRY(trk_priority(priority, prio));
    std::vector<int> ofs32, cam_cnt;
    TRY(trk_check_lists(n_cam, n_pts, pt_ofs, cam_ind, ofs32, &cam_cnt));
    const int64_t n_obs = pt_ofs[n_pts];
    if (n_obs && !scale) return fail(SATBA_E_ARG, "null observations");
    const int M = n_cam, N = (int)n_pts;
    *n_selected = 0; *n_trees = 0;
    if (weights) std::fill(weights, weights + (size_t)K * M, 0.0);
    std::vector<int> cam_ofs((size_t)M + 1, 0);
    for (int c = 0; c < M; ++c) cam_ofs[(size_t)c + 1] = cam_ofs[(size_t)c] + cam_cnt[(size_t)c];

    DevRun s;
    TRY(s.begin(device));
    const int lds_optin = dev_lds_limit(device);
    int *d_ofs, *d_cam, *d_len, *d_idx_a, *d_idx_b, *d_rank, *d_tree, *d_cam_ofs, *d_cm_trk, *d_cam_sorted, *d_obs_trk, *d_tri, *d_reached, *d_layer, *d_status;
    double *d_scale, *d_err = nullptr, *d_ks, *d_kc, *d_w, *d_wout = nullptr;
    unsigned long long *d_img, *d_key_a, *d_key_b, *d_slot;
    TRY(s.upload(&d_ofs, ofs32.data(), ofs32.size())); TRY(s.upload(&d_cam, cam_ind, (size_t)n_obs));
    TRY(s.upload(&d_scale, scale, (size_t)n_obs));
    if (err) TRY(s.upload(&d_err, err, (size_t)n_obs));
    TRY(s.upload(&d_cam_ofs, cam_ofs.data(), cam_ofs.size()));
    TRY(s.alloc(&d_len, (size_t)N)); TRY(s.alloc(&d_ks, (size_t)N));
    TRY(s.alloc(&d_kc, (size_t)N)); TRY(s.alloc(&d_img, 3 * (size_t)N));
    TRY(s.alloc(&d_key_a, (size_t)N)); TRY(s.alloc(&d_key_b, (size_t)N));
    TRY(s.alloc(&d_idx_a, (size_t)N)); TRY(s.alloc(&d_idx_b, (size_t)N));
    TRY(s.alloc(&d_rank, (size_t)N)); TRY(s.alloc(&d_tree, (size_t)N));
    TRY(s.alloc(&d_cm_trk, (size_t)n_obs)); TRY(s.alloc(&d_cam_sorted, (size_t)n_obs));
    TRY(s.alloc(&d_obs_trk, (size_t)n_obs));
    TRY(s.alloc(&d_tri, (size_t)std::max(M * (M - 1) / 2, 1)));
    TRY(s.alloc(&d_reached, (size_t)M)); TRY(s.alloc(&d_layer, (size_t)M));
    TRY(s.alloc(&d_slot, (size_t)M)); TRY(s.alloc(&d_w, (size_t)M));
    TRY(s.alloc(&d_status, (size_t)TRK_ST_LEN));
    if (weights && K) TRY(s.alloc(&d_wout, (size_t)K * M));
    HIP_TRY(hipMemsetAsync(d_tree, 0xff, sizeof(int) * (size_t)std::max(N, 1), s.stream));  // -1: not selected
    HIP_TRY(hipMemsetAsync(d_status, 0, sizeof(int) * TRK_ST_LEN, s.stream));
    if (d_wout) HIP_TRY(hipMemsetAsync(d_wout, 0, sizeof(double) * (size_t)K * M, s.stream));

    // temporary storage of the radix sorts (rocPRIM: stable, ascending)
    size_t tmp_a = 0, tmp_b = 0;
    if (N) HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp_a, d_key_a, d_key_b, d_idx_a, d_idx_b, (size_t)N, 0, 64, s.stream));
    if (n_obs) HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp_b, d_cam, d_cam_sorted, d_obs_trk, d_cm_trk, (size_t)n_obs, 0, 32, s.stream));
    char* d_tmp;
    const size_t tmp_bytes = std::max(tmp_a, tmp_b) + 16;
    TRY(s.alloc(&d_tmp, tmp_bytes));

    const dim3 gN((unsigned)((N + TRK_THREADS - 1) / TRK_THREADS)), blk(TRK_THREADS);
    HIP_TRY(hipEventRecord(s.e0, s.stream));
    if (N) {
        // ---- keys and ranking (ft_ranking.py:136-153)
        hipLaunchKernelGGL(k_trk_keys, gN, blk, 0, s.stream, N, d_ofs, d_scale, d_err, d_len, d_ks, d_kc, d_img);
        hipLaunchKernelGGL(k_trk_iota_desc, gN, blk, 0, s.stream, N, d_idx_a);
        HIP_TRY(hipGetLastError());
        for (int pass = 2; pass >= 0; --pass) {  // least significant key first
            const int key = prio[pass];
            hipLaunchKernelGGL(k_trk_gather, gN, blk, 0, s.stream, N, d_idx_a, d_img + (size_t)key * N, d_key_a);
            HIP_TRY(hipGetLastError());
            size_t tb = tmp_bytes;
            HIP_TRY(rocprim::radix_sort_pairs(d_tmp, tb, d_key_a, d_key_b, d_idx_a, d_idx_b, (size_t)N, 0, 64, s.stream));
            std::swap(d_idx_a, d_idx_b);
        }
        hipLaunchKernelGGL(k_trk_scatter_rank, gN, blk, 0, s.stream, N, d_idx_a, d_rank);  // d_idx_a: order (rank -> track)
        HIP_TRY(hipGetLastError());
    }
    if (n_obs) {
        // ---- every camera's tracks, ascending: the stable sort of the (track-major) observations by camera
        hipLaunchKernelGGL(k_trk_obs_track, gN, blk, 0, s.stream, N, d_ofs, d_obs_trk);
        HIP_TRY(hipGetLastError());
        size_t tb = tmp_bytes;
        HIP_TRY(rocprim::radix_sort_pairs(d_tmp, tb, d_cam, d_cam_sorted, d_obs_trk, d_cm_trk, (size_t)n_obs, 0, 32, s.stream));
    }
    // ---- the trees (ft_ranking.py:232-263)
    int st[TRK_ST_LEN] = {0, 0, 0, 0};
    int trees = 0;
    for (int k = 0; k < K && st[TRK_ST_SELECTED] < N; ++k) {
        TRY(trk_connect(s, N, M, d_ofs, d_cam, d_tree, 0, d_tri, lds_optin));
        hipLaunchKernelGGL(k_trk_weights, dim3((unsigned)M), blk, 0, s.stream, M, d_cam_ofs, d_cm_trk, d_tree, d_kc, d_tri, d_w,
                           d_wout ? d_wout + (size_t)k * M : (double*)nullptr);
        hipLaunchKernelGGL(k_trk_tree_begin, dim3(1), blk, 0, s.stream, M, d_w, d_reached, d_layer, d_slot, d_status);
        HIP_TRY(hipGetLastError());
        for (;;) {  // the layers (ft_ranking.py:209-227): at most M - 1 of them reach a new camera
            hipLaunchKernelGGL(k_trk_claim, gN, blk, 0, s.stream, N, d_ofs, d_cam, d_tree, d_rank, d_layer, d_reached, d_slot);
            hipLaunchKernelGGL(k_trk_commit, dim3(1), blk, 0, s.stream, M, N, k, d_w, d_idx_a, d_tree, d_reached, d_layer, d_slot, d_status);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(st, d_status, sizeof(st), hipMemcpyDeviceToHost, s.stream));
            HIP_TRY(hipStreamSynchronize(s.stream));
            if (st[TRK_ST_NEW] == 0 || st[TRK_ST_REACHED] >= M) break;
        }
        if (st[TRK_ST_TREE_SELECTED] == 0) break;  // an empty tree: the live set did not change, every later tree would be empty too
        ++trees;
    }
    HIP_TRY(hipEventRecord(s.e1, s.stream));
    std::vector<int> rank32((size_t)(rank ? N : 0));
    if (N) HIP_TRY(hipMemcpyAsync(tree_of, d_tree, sizeof(int) * (size_t)N, hipMemcpyDeviceToHost, s.stream));
    if (N && rank) HIP_TRY(hipMemcpyAsync(rank32.data(), d_rank, sizeof(int) * (size_t)N, hipMemcpyDeviceToHost, s.stream));
    if (d_wout) HIP_TRY(hipMemcpyAsync(weights, d_wout, sizeof(double) * (size_t)K * M, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    for (size_t i = 0; i < rank32.size(); ++i) rank[i] = rank32[i];
    *n_selected = st[TRK_ST_SELECTED];
    *n_trees = trees;
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, s.e0, s.e1));
    return 0;
}

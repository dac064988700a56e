// satba_ftracks_build / _fetch / _destroy and satba_tracks_have_pair (include/satba.h): part of the extern "C" block of satba_capi.hip.
// Stand-alone entry points (no problem handle): the tracks are built before anything else exists.  Kernels: satba_ftracks.h.
struct satba_ftracks {
    int device = 0;
    int64_t n_tracks = 0, n_obs = 0;
    int *pt_ofs = nullptr, *cam_ind = nullptr, *kp_id = nullptr;
    double *obs = nullptr, *scale = nullptr;
    DevAllocs mem;  // owns the arrays
};

extern "C++" {
namespace {
// bit i * n_cam + j for every listed pair with i < j < n_cam
void ft_pair_bits(int32_t n_cam, int32_t n_pairs, const int32_t* pairs, std::vector<unsigned>& bits) {
    const long long n_bits = (long long)n_cam * n_cam;
    bits.assign((size_t)((n_bits + 31) / 32), 0u);
    for (int32_t p = 0; p < n_pairs; ++p) {
        const long long i = pairs[2 * p], j = pairs[2 * p + 1];
        if (i < 0 || i >= j || j >= n_cam) continue;
        const long long b = i * n_cam + j;
        bits[(size_t)(b >> 5)] |= 1u << (b & 31);
    }
}

template <class T>
int ft_scan(DevRun& s, void* d_tmp, size_t tmp_bytes, const T* in, T* out, size_t n) {
    HIP_TRY(rocprim::exclusive_scan(d_tmp, tmp_bytes, in, out, T(0), n, rocprim::plus<T>(), s.stream));
    return 0;
}

int ft_has_pair(DevRun& s, int n_tr, int n_cam, int n_adj, const int* d_ofs, const int* d_cam, const unsigned* d_bits, long long n_words,
                unsigned char* d_keep, int* d_group, int lds_optin) {
    if (!n_tr) return 0;
    const unsigned blocks = (unsigned)std::min<long long>(((long long)n_tr + FT_THREADS - 1) / FT_THREADS, 2048);
    const long long lds_bytes = n_words * (long long)sizeof(unsigned);
    if (lds_bytes + 1024 <= (long long)lds_optin) {
        if (lds_bytes > 48 * 1024)
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ft_has_pair<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        hipLaunchKernelGGL(k_ft_has_pair<true>, dim3(blocks), dim3(FT_THREADS), (size_t)lds_bytes, s.stream, n_tr, n_cam, n_adj, d_ofs, d_cam, d_bits,
                           n_words, d_keep, d_group);
    } else {
        hipLaunchKernelGGL(k_ft_has_pair<false>, dim3(blocks), dim3(FT_THREADS), 0, s.stream, n_tr, n_cam, n_adj, d_ofs, d_cam, d_bits, n_words, d_keep,
                           d_group);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

void ft_free(satba_ftracks* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    delete t;
}

int ft_build(satba_ftracks* t, int32_t n_cam, const std::vector<int>& ofs32, const float* kp, int64_t n_matches, const int32_t* matches,
             const std::vector<unsigned>& bits, int32_t n_adj, int64_t* counts, int32_t device, float* kernel_ms) {
    const int n_kp = ofs32[(size_t)n_cam], n = (int)n_matches;
    DevRun s;
    TRY(s.begin(device));
    t->device = device;
    const dim3 blk(FT_THREADS);
    auto grid = [](long long m) { return dim3((unsigned)((m + FT_THREADS - 1) / FT_THREADS)); };

    int *d_kp_ofs, *d_matches, *d_parent, *d_label, *d_cnt, *d_is_root, *d_is_matched, *d_track_of_root, *d_pos, *d_conf;
    float* d_kp;
    unsigned long long* d_wkey;
    unsigned* d_bits;
    TRY(s.upload(&d_kp_ofs, ofs32.data(), ofs32.size())); TRY(s.upload(&d_kp, kp, 3 * (size_t)n_kp));
    TRY(s.upload(&d_matches, matches, 4 * (size_t)n)); TRY(s.upload(&d_bits, bits.data(), bits.size()));
    TRY(s.alloc(&d_parent, (size_t)n_kp)); TRY(s.alloc(&d_label, (size_t)n_kp));
    TRY(s.alloc(&d_cnt, (size_t)n_kp)); TRY(s.alloc(&d_wkey, (size_t)n_kp));
    TRY(s.alloc(&d_is_root, (size_t)n_kp + 1)); TRY(s.alloc(&d_is_matched, (size_t)n_kp + 1));
    TRY(s.alloc(&d_track_of_root, (size_t)n_kp + 1)); TRY(s.alloc(&d_pos, (size_t)n_kp + 1));
    TRY(s.alloc(&d_conf, 1));
    HIP_TRY(hipMemsetAsync(d_conf, 0, sizeof(int), s.stream));
    size_t tmp_scan = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tmp_scan, d_is_root, d_track_of_root, 0, (size_t)n_kp + 1, rocprim::plus<int>(), s.stream));
    char* d_tmp_scan;
    TRY(s.alloc(&d_tmp_scan, tmp_scan + 16));

    // ---- components (ft_utils.py:115-149)
    HIP_TRY(hipEventRecord(s.e0, s.stream));
    int tot[2] = {0, 0};  // components of >= 2, matched keypoints
    if (n_kp) {
        hipLaunchKernelGGL(k_ft_init, grid(n_kp), blk, 0, s.stream, n_kp, d_parent, d_cnt, d_wkey);
        if (n) {
            hipLaunchKernelGGL(k_ft_union, grid(n), blk, 0, s.stream, n, d_kp_ofs, d_matches, d_parent);
            hipLaunchKernelGGL(k_ft_keys, grid(n), blk, 0, s.stream, n, d_kp_ofs, d_matches, d_wkey);
        }
        hipLaunchKernelGGL(k_ft_flatten, grid(n_kp), blk, 0, s.stream, n_kp, d_parent, d_label, d_cnt);
        hipLaunchKernelGGL(k_ft_flags, grid((long long)n_kp + 1), blk, 0, s.stream, n_kp, d_label, d_cnt, d_wkey, d_is_root, d_is_matched);
        HIP_TRY(hipGetLastError());
        TRY(ft_scan(s, d_tmp_scan, tmp_scan, d_is_root, d_track_of_root, (size_t)n_kp + 1));
        TRY(ft_scan(s, d_tmp_scan, tmp_scan, d_is_matched, d_pos, (size_t)n_kp + 1));
        HIP_TRY(hipMemcpyAsync(&tot[0], d_track_of_root + n_kp, sizeof(int), hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipMemcpyAsync(&tot[1], d_pos + n_kp, sizeof(int), hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipStreamSynchronize(s.stream));
    }
    const int n_tr = tot[0], n_c = tot[1];

    // ---- one winner per (track, camera) cell (ft_utils.py:159-170)
    int res[3] = {0, 0, 0};  // fixed survivors, survivors, their observations
    int conflicts = 0;
    if (n_tr) {
        unsigned long long *d_key_a, *d_key_b;
        int *d_id_a, *d_id_b, *d_head, *d_cell_pos, *d_cell_trk, *d_cell_cam, *d_cell_kp, *d_tr_ofs, *d_group, *d_slot, *d_new_trk, *d_new_len, *d_pt_ofs;
        TRY(s.alloc(&d_key_a, (size_t)n_c)); TRY(s.alloc(&d_key_b, (size_t)n_c));
        TRY(s.alloc(&d_id_a, (size_t)n_c)); TRY(s.alloc(&d_id_b, (size_t)n_c));
        TRY(s.alloc(&d_head, (size_t)n_c + 1)); TRY(s.alloc(&d_cell_pos, (size_t)n_c + 1));
        TRY(s.alloc(&d_cell_trk, (size_t)n_c)); TRY(s.alloc(&d_cell_cam, (size_t)n_c));
        TRY(s.alloc(&d_cell_kp, (size_t)n_c)); TRY(s.alloc(&d_tr_ofs, (size_t)n_tr + 1));
        TRY(s.alloc(&d_group, 2 * (size_t)n_tr + 1)); TRY(s.alloc(&d_slot, 2 * (size_t)n_tr + 1));
        TRY(s.alloc(&d_new_trk, (size_t)n_tr)); TRY(s.alloc(&d_new_len, (size_t)n_tr + 1));
        TRY(s.alloc(&d_pt_ofs, (size_t)n_tr + 1));
        int key_bits = 1;
        while (key_bits < 64 && ((unsigned long long)n_tr * (unsigned long long)n_cam) >> key_bits) ++key_bits;
        size_t tmp_sort = 0, tmp_scan2 = 0;
        HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp_sort, d_key_a, d_key_b, d_id_a, d_id_b, (size_t)n_c, 0, key_bits, s.stream));
        HIP_TRY(rocprim::exclusive_scan(nullptr, tmp_scan2, d_head, d_cell_pos, 0, (size_t)std::max(n_c, 2 * n_tr) + 1, rocprim::plus<int>(), s.stream));
        const size_t tmp_bytes = std::max(tmp_sort, tmp_scan2) + 16;
        char* d_tmp;
        TRY(s.alloc(&d_tmp, tmp_bytes));

        hipLaunchKernelGGL(k_ft_candidates, grid(n_kp), blk, 0, s.stream, n_kp, (int)n_cam, d_kp_ofs, d_label, d_track_of_root, d_is_matched, d_pos, d_key_a,
                           d_id_a);
        HIP_TRY(hipGetLastError());
        size_t tb = tmp_bytes;
        // stable: inside a cell the claimants stay in id order (the winner does not depend on it: write keys are distinct)
        HIP_TRY(rocprim::radix_sort_pairs(d_tmp, tb, d_key_a, d_key_b, d_id_a, d_id_b, (size_t)n_c, 0, key_bits, s.stream));
        hipLaunchKernelGGL(k_ft_heads, grid((long long)n_c + 1), blk, 0, s.stream, n_c, d_key_b, d_head);
        HIP_TRY(hipGetLastError());
        TRY(ft_scan(s, d_tmp, tmp_bytes, d_head, d_cell_pos, (size_t)n_c + 1));
        hipLaunchKernelGGL(k_ft_winners, grid(n_c), blk, 0, s.stream, n_c, (int)n_cam, n_tr, d_key_b, d_id_b, d_head, d_cell_pos, d_wkey, d_cell_trk,
                           d_cell_cam, d_cell_kp, d_tr_ofs, d_conf);
        HIP_TRY(hipGetLastError());

        // ---- baseline check and the fixed-first partition (ft_utils.py:38-62, ft_pipeline.py:175-179)
        TRY(ft_has_pair(s, n_tr, n_cam, n_adj, d_tr_ofs, d_cell_cam, d_bits, (long long)bits.size(), nullptr, d_group, dev_lds_limit(device)));
        TRY(ft_scan(s, d_tmp, tmp_bytes, d_group, d_slot, 2 * (size_t)n_tr + 1));
        HIP_TRY(hipMemsetAsync(d_new_len, 0, sizeof(int) * ((size_t)n_tr + 1), s.stream));
        hipLaunchKernelGGL(k_ft_lengths, grid(n_tr), blk, 0, s.stream, n_tr, d_tr_ofs, d_group, d_slot, d_new_trk, d_new_len);
        HIP_TRY(hipGetLastError());
        TRY(ft_scan(s, d_tmp, tmp_bytes, d_new_len, d_pt_ofs, (size_t)n_tr + 1));
        int n_cells = 0;
        HIP_TRY(hipMemcpyAsync(&res[0], d_slot + n_tr, sizeof(int), hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipMemcpyAsync(&res[1], d_slot + 2 * (size_t)n_tr, sizeof(int), hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipMemcpyAsync(&n_cells, d_cell_pos + n_c, sizeof(int), hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipMemcpyAsync(&conflicts, d_conf, sizeof(int), hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipStreamSynchronize(s.stream));
        HIP_TRY(hipMemcpyAsync(&res[2], d_pt_ofs + res[1], sizeof(int), hipMemcpyDeviceToHost, s.stream));  // survivors fill slots 0 .. res[1] - 1
        HIP_TRY(hipStreamSynchronize(s.stream));

        // ---- the lists, in the handle's own memory
        TRY(t->mem.alloc(&t->pt_ofs, (size_t)res[1] + 1));
        TRY(t->mem.alloc(&t->cam_ind, (size_t)std::max(res[2], 1)));
        TRY(t->mem.alloc(&t->kp_id, (size_t)std::max(res[2], 1)));
        TRY(t->mem.alloc(&t->obs, 2 * (size_t)std::max(res[2], 1)));
        TRY(t->mem.alloc(&t->scale, (size_t)std::max(res[2], 1)));
        HIP_TRY(hipMemcpyAsync(t->pt_ofs, d_pt_ofs, sizeof(int) * ((size_t)res[1] + 1), hipMemcpyDeviceToDevice, s.stream));
        if (res[2]) {
            hipLaunchKernelGGL(k_ft_emit, grid(n_cells), blk, 0, s.stream, n_cells, d_cell_trk, d_cell_cam, d_cell_kp, d_tr_ofs, d_new_trk, d_pt_ofs,
                               d_kp_ofs, d_kp, t->cam_ind, t->kp_id, t->obs, t->scale);
            HIP_TRY(hipGetLastError());
        }
    } else {
        TRY(t->mem.alloc(&t->pt_ofs, 1));
        HIP_TRY(hipMemsetAsync(t->pt_ofs, 0, sizeof(int), s.stream));
    }
    HIP_TRY(hipEventRecord(s.e1, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, s.e0, s.e1));
    t->n_tracks = res[1];
    t->n_obs = res[2];
    counts[0] = res[1]; counts[1] = res[2]; counts[2] = res[0]; counts[3] = n_tr; counts[4] = conflicts;
    return 0;
}
}  // namespace
}  // extern "C++"

int satba_ftracks_build(int32_t n_cam, const int64_t* kp_ofs, const float* kp, int64_t n_matches, const int32_t* matches, int32_t n_pairs,
                        const int32_t* pairs, int32_t n_adj, satba_ftracks** out, int64_t* counts, int32_t device, float* kernel_ms) {
    if (!out || !counts || !kp_ofs || n_cam <= 0 || n_matches < 0 || n_pairs < 0 || n_adj < 0) return fail(SATBA_E_ARG, "null or negative argument");
    *out = nullptr;
    if (n_cam >= 46341) return fail(SATBA_E_ARG, "the pair table holds fewer than 46 341 cameras");
    if ((n_matches && !matches) || (n_pairs && !pairs)) return fail(SATBA_E_ARG, "null matches or pairs");
    if (kp_ofs[0] != 0) return fail(SATBA_E_ARG, "kp_ofs must start at 0");
    for (int32_t m = 0; m < n_cam; ++m)
        if (kp_ofs[m + 1] < kp_ofs[m]) return fail(SATBA_E_ARG, "kp_ofs must not decrease (image %d)", m);
    if (kp_ofs[n_cam] >= (int64_t)1 << 31 || n_matches >= (int64_t)1 << 31)
        return fail(SATBA_E_ARG, "fewer than 2^31 keypoints and matches are supported (%lld, %lld)", (long long)kp_ofs[n_cam], (long long)n_matches);
    if (kp_ofs[n_cam] && !kp) return fail(SATBA_E_ARG, "null keypoints");
    for (int64_t r = 0; r < n_matches; ++r) {
        const int32_t *m = matches + 4 * r;
        if (m[2] < 0 || m[2] >= n_cam || m[3] < 0 || m[3] >= n_cam) return fail(SATBA_E_ARG, "match %lld names an image outside 0..%d", (long long)r, n_cam - 1);
        if (m[2] == m[3]) return fail(SATBA_E_ARG, "match %lld joins two keypoints of image %d", (long long)r, m[2]);
        if (m[0] < 0 || m[0] >= kp_ofs[m[2] + 1] - kp_ofs[m[2]] || m[1] < 0 || m[1] >= kp_ofs[m[3] + 1] - kp_ofs[m[3]])
            return fail(SATBA_E_ARG, "match %lld names a keypoint outside its image", (long long)r);
    }
    std::vector<int> ofs32((size_t)n_cam + 1);
    for (int32_t m = 0; m <= n_cam; ++m) ofs32[(size_t)m] = (int)kp_ofs[m];
    std::vector<unsigned> bits;
    ft_pair_bits(n_cam, n_pairs, pairs, bits);
    satba_ftracks* t = new (std::nothrow) satba_ftracks();
    if (!t) return fail(SATBA_E_ARG, "out of host memory");
    const int rc = ft_build(t, n_cam, ofs32, kp, n_matches, matches, bits, n_adj, counts, device, kernel_ms);
    if (rc) {
        ft_free(t);
        return rc;
    }
    *out = t;
    return 0;
}

int satba_ftracks_fetch(satba_ftracks* t, int64_t* pt_ofs, int32_t* cam_ind, int32_t* kp_id, double* obs, double* scale) {
    if (!t) return fail(SATBA_E_ARG, "null handle");
    HIP_TRY(hipSetDevice(t->device));
    if (pt_ofs) {
        std::vector<int> o32((size_t)t->n_tracks + 1);
        HIP_TRY(hipMemcpy(o32.data(), t->pt_ofs, sizeof(int) * o32.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < o32.size(); ++i) pt_ofs[i] = o32[i];
    }
    const size_t K = (size_t)t->n_obs;
    if (K && cam_ind) HIP_TRY(hipMemcpy(cam_ind, t->cam_ind, sizeof(int) * K, hipMemcpyDeviceToHost));
    if (K && kp_id) HIP_TRY(hipMemcpy(kp_id, t->kp_id, sizeof(int) * K, hipMemcpyDeviceToHost));
    if (K && obs) HIP_TRY(hipMemcpy(obs, t->obs, sizeof(double) * 2 * K, hipMemcpyDeviceToHost));
    if (K && scale) HIP_TRY(hipMemcpy(scale, t->scale, sizeof(double) * K, hipMemcpyDeviceToHost));
    return 0;
}

void satba_ftracks_destroy(satba_ftracks* t) { ft_free(t); }

int satba_tracks_have_pair(int32_t n_cam, int64_t n_pts, const int64_t* pt_ofs, const int32_t* cam_ind, int32_t n_pairs, const int32_t* pairs,
                           uint8_t* keep, int32_t device) {
    if (n_pairs < 0 || (n_pairs && !pairs) || (n_pts > 0 && !keep)) return fail(SATBA_E_ARG, "null or negative argument");
    std::vector<int> ofs32;
    TRY(trk_check_lists(n_cam, n_pts, pt_ofs, cam_ind, ofs32, nullptr));
    if (!n_pts) return 0;
    std::vector<unsigned> bits;
    ft_pair_bits(n_cam, n_pairs, pairs, bits);
    DevRun s;
    TRY(s.begin(device));
    int *d_ofs, *d_cam;
    unsigned* d_bits;
    unsigned char* d_keep;
    TRY(s.upload(&d_ofs, ofs32.data(), ofs32.size())); TRY(s.upload(&d_cam, cam_ind, (size_t)pt_ofs[n_pts]));
    TRY(s.upload(&d_bits, bits.data(), bits.size())); TRY(s.alloc(&d_keep, (size_t)n_pts));
    TRY(ft_has_pair(s, (int)n_pts, n_cam, 0, d_ofs, d_cam, d_bits, (long long)bits.size(), d_keep, nullptr, dev_lds_limit(device)));
    HIP_TRY(hipMemcpyAsync(keep, d_keep, (size_t)n_pts, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    return 0;
}

// satba_triangulate_pairwise / satba_init_pts3d (include/satba.h): part of the extern "C" block of satba_capi.hip.
// Stand-alone entry points (no problem handle): the triangulation runs before a BundleAdjustmentParameters object exists.
extern "C++" {
namespace {
int tri_cam_len(int model) { return model == SATBA_RPC ? SATBA_RPC_TABLE_LEN : 12; }
}  // namespace
}  // extern "C++"

int satba_triangulate_pairwise(int32_t cam_model, const double* cam_i, const double* cam_j, int64_t n, const double* pts_i, const double* pts_j,
                               double* pts3d, float* err, int32_t device, float* kernel_ms) {
    if (!cam_i || !cam_j || n < 0 || (n && (!pts_i || !pts_j || !pts3d))) return fail(SATBA_E_ARG, "null argument");
    if (cam_model != SATBA_AFFINE && cam_model != SATBA_PERSPECTIVE && cam_model != SATBA_RPC) return fail(SATBA_E_ARG, "unknown camera model");
    DevRun s;
    TRY(s.begin(device));
    const int len = tri_cam_len(cam_model);
    double *d_ci, *d_cj, *d_pi, *d_pj, *d_out;
    float* d_err = nullptr;
    TRY(s.upload(&d_ci, cam_i, (size_t)len)); TRY(s.upload(&d_cj, cam_j, (size_t)len));
    TRY(s.upload(&d_pi, pts_i, (size_t)2 * n)); TRY(s.upload(&d_pj, pts_j, (size_t)2 * n));
    TRY(s.alloc(&d_out, (size_t)3 * n));
    if (err) TRY(s.alloc(&d_err, (size_t)n));
    HIP_TRY(hipEventRecord(s.e0, s.stream));
    if (n) {
        const dim3 grid((unsigned)((n + 255) / 256)), block(256);
        if (cam_model == SATBA_RPC) hipLaunchKernelGGL(k_tri_pairwise<2>, grid, block, 0, s.stream, (long long)n, d_ci, d_cj, d_pi, d_pj, d_out, d_err);
        else hipLaunchKernelGGL(k_tri_pairwise<0>, grid, block, 0, s.stream, (long long)n, d_ci, d_cj, d_pi, d_pj, d_out, d_err);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(s.e1, s.stream));
    if (n) HIP_TRY(hipMemcpyAsync(pts3d, d_out, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, s.stream));
    if (n && err) HIP_TRY(hipMemcpyAsync(err, d_err, sizeof(float) * n, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, s.e0, s.e1));
    return 0;
}

extern "C++" {
namespace {
// the four passes over prepared arguments (a: pt_ofs, cam_ind, obs and, for a handle's layout, slice_base / removed / perm set by the
// caller; the pair tables, outputs and work lists are set up here); results to the host
int tri_run(DevRun& s, TriArgs a, int32_t cam_model, int32_t n_cam, int64_t n_pts, bool ordered, const double* cameras, int32_t n_pairs,
            const int32_t* pairs, const std::vector<int>& first, const std::vector<int>& next, float* pts3d, int32_t* n_tri, int32_t device,
            int32_t reps, float* kernel_ms) {
    a.M = n_cam; a.N = (int)n_pts; a.n_pairs = n_pairs; a.cam_len = tri_cam_len(cam_model); a.ordered = ordered;
    int *d_first, *d_next, *d_pairs, *d_ntri, *d_tofs, *d_ntri_out = nullptr;
    double* d_cams;
    float* d_out;
    TRY(s.upload(&d_cams, cameras, (size_t)n_cam * a.cam_len)); TRY(s.upload(&d_first, first.data(), first.size()));
    TRY(s.upload(&d_next, next.data(), next.size())); TRY(s.upload(&d_pairs, pairs, (size_t)2 * n_pairs));
    TRY(s.alloc(&d_out, (size_t)3 * n_pts));
    TRY(s.alloc(&d_ntri, (size_t)n_pts + 1)); TRY(s.alloc(&d_tofs, (size_t)n_pts + 1));
    if (a.perm && n_tri) TRY(s.alloc(&d_ntri_out, (size_t)n_pts));
    HIP_TRY(hipMemsetAsync(d_ntri, 0, sizeof(int) * ((size_t)n_pts + 1), s.stream));
    a.cams = d_cams; a.pair_first = d_first; a.pair_next = d_next; a.pairs = d_pairs;
    a.out = d_out; a.n_tri = d_ntri; a.tri_ofs = d_tofs; a.n_tri_out = d_ntri_out;
    const size_t tab_bytes = sizeof(double) * (size_t)n_cam * TRI_RPC_STRIDE;
    // the RPC tables go to dynamic LDS when the device's opt-in limit allows (160 KB per workgroup on gfx950; the limit is asked,
    // not assumed: the Makefile's ARCH can be overridden), with 20 KB left for the kernel's own arrays
    const int lds_optin = dev_lds_limit(device);
    const bool tab_lds = cam_model == SATBA_RPC && (long long)tab_bytes + 20 * 1024 <= (long long)lds_optin;
    if (tab_lds && tab_bytes > 48 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k_tri_points<2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tab_bytes));
    char* d_cub = nullptr;
    size_t cub_bytes = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, d_ntri, d_tofs, (int)n_pts + 1, s.stream));
    TRY(s.alloc(&d_cub, cub_bytes + 16));
    const dim3 g256((unsigned)((n_pts + 255) / 256)), gl((unsigned)((n_pts + TRI_THREADS - 1) / TRI_THREADS));
    auto count_pass = [&]() -> int {
        hipLaunchKernelGGL(k_tri_count, g256, dim3(256), 0, s.stream, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_cub, cub_bytes, d_ntri, d_tofs, (int)n_pts + 1, s.stream));
        return 0;
    };
    long long E = 0;
    if (n_pts) {  // size of the work list (untimed: the timed passes below repeat the count)
        TRY(count_pass());
        int total = 0;
        HIP_TRY(hipMemcpyAsync(&total, d_tofs + n_pts, sizeof(int), hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipStreamSynchronize(s.stream));
        if (total < 0) return fail(SATBA_E_ARG, "more than 2^31 triangulations");
        E = total;
    }
    int2* d_entries;
    float* d_res;
    TRY(s.alloc(&d_entries, (size_t)E)); TRY(s.alloc(&d_res, (size_t)3 * E));
    a.entries = d_entries; a.res = d_res;
    reps = std::max(reps, 1);
    HIP_TRY(hipEventRecord(s.e0, s.stream));
    for (int r = 0; r < reps && n_pts; ++r) {
        TRY(count_pass());
        if (ordered) hipLaunchKernelGGL(k_tri_list_ordered, g256, dim3(256), 0, s.stream, a);
        else hipLaunchKernelGGL(k_tri_list, gl, dim3(TRI_THREADS), 0, s.stream, a);
        if (E) {
            const dim3 gp((unsigned)std::min<long long>((E + 255) / 256, 256 * 64));
            if (tab_lds) hipLaunchKernelGGL((k_tri_points<2, true>), gp, dim3(256), tab_bytes, s.stream, a, (int)E);
            else if (cam_model == SATBA_RPC) hipLaunchKernelGGL((k_tri_points<2, false>), gp, dim3(256), 0, s.stream, a, (int)E);
            else hipLaunchKernelGGL((k_tri_points<0, false>), gp, dim3(256), 0, s.stream, a, (int)E);
        }
        hipLaunchKernelGGL(k_tri_mean, g256, dim3(256), 0, s.stream, a);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(s.e1, s.stream));
    if (n_pts) HIP_TRY(hipMemcpyAsync(pts3d, d_out, sizeof(float) * 3 * n_pts, hipMemcpyDeviceToHost, s.stream));
    if (n_pts && n_tri) HIP_TRY(hipMemcpyAsync(n_tri, d_ntri_out ? d_ntri_out : d_ntri, sizeof(int) * n_pts, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    if (kernel_ms) { HIP_TRY(hipEventElapsedTime(kernel_ms, s.e0, s.e1)); *kernel_ms /= (float)reps; }
    return 0;
}

// ordered pair -> list indices, ascending (a pair may be listed more than once: every occurrence triangulates again, like
// the reference's loop); pairs naming a camera the problem does not have are skipped (ft_triangulate.py:99).
// ordered (in/out): stays true if the pairs are listed in ascending lexicographic order with c_i < c_j
int tri_pair_tables(int32_t n_cam, int32_t n_pairs, const int32_t* pairs, std::vector<int>& first, std::vector<int>& next, bool& ordered) {
    for (int id = 0; id < n_pairs && ordered; ++id) {
        const int ci = pairs[2 * id], cj = pairs[2 * id + 1];
        ordered = ci < cj && (id == 0 || pairs[2 * id - 2] < ci || (pairs[2 * id - 2] == ci && pairs[2 * id - 1] < cj));
    }
    first.assign((size_t)n_cam * n_cam, -1); next.assign((size_t)std::max(n_pairs, 1), -1);
    for (int id = n_pairs - 1; id >= 0; --id) {
        const int ci = pairs[2 * id], cj = pairs[2 * id + 1];
        if (ci < 0 || cj < 0) return fail(SATBA_E_ARG, "negative camera index in pair %d", id);
        if (ci == cj) return fail(SATBA_E_ARG, "pair %d names one camera twice", id);
        if (ci >= n_cam || cj >= n_cam) continue;
        next[(size_t)id] = first[(size_t)ci * n_cam + cj];
        first[(size_t)ci * n_cam + cj] = id;
    }
    return 0;
}
}  // namespace
}  // extern "C++"

int satba_init_pts3d(int32_t cam_model, int32_t n_cam, int64_t n_pts, const int64_t* pt_ofs, const int32_t* cam_ind, const double* obs,
                     const double* cameras, int32_t n_pairs, const int32_t* pairs, float* pts3d, int32_t* n_tri, int32_t device,
                     int32_t reps, float* kernel_ms) {
    if (n_cam <= 0 || n_pts < 0 || n_pairs < 0 || !pt_ofs || !cameras || (n_pts && !pts3d) || (n_pairs && !pairs))
        return fail(SATBA_E_ARG, "null or negative argument");
    if (cam_model != SATBA_AFFINE && cam_model != SATBA_PERSPECTIVE && cam_model != SATBA_RPC) return fail(SATBA_E_ARG, "unknown camera model");
    std::vector<int> ofs32;
    TRY(dev_check_offsets(n_pts, pt_ofs, cam_ind && obs, ofs32));
    const int64_t K = pt_ofs[n_pts];
    for (int64_t o = 0; o < K; ++o)
        if (cam_ind[o] < 0 || cam_ind[o] >= n_cam) return fail(SATBA_E_ARG, "camera index %d out of range", cam_ind[o]);
    // the common case: pairs listed in ascending lexicographic order with c_i < c_j, every track's cameras ascending
    bool ordered = getenv("SATBA_TRI_GENERAL") == nullptr;
    std::vector<int> first, next;
    TRY(tri_pair_tables(n_cam, n_pairs, pairs, first, next, ordered));
    for (int64_t i = 0; i < n_pts && ordered; ++i)
        for (int64_t o = pt_ofs[i] + 1; o < pt_ofs[i + 1]; ++o)
            if (cam_ind[o] <= cam_ind[o - 1]) { ordered = false; break; }
    DevRun s;
    TRY(s.begin(device));
    TriArgs a{};
    int *d_ofs, *d_cam;
    double* d_obs;
    TRY(s.upload(&d_ofs, ofs32.data(), ofs32.size())); TRY(s.upload(&d_cam, cam_ind, (size_t)K)); TRY(s.upload(&d_obs, obs, (size_t)2 * K));
    a.pt_ofs = d_ofs; a.cam_ind = d_cam; a.obs = d_obs;
    return tri_run(s, a, cam_model, n_cam, n_pts, ordered, cameras, n_pairs, pairs, first, next, pts3d, n_tri, device, reps, kernel_ms);
}

int satba_init_pts3d_resident(satba_problem* p, const uint8_t* remove, const double* cameras, int32_t n_pairs, const int32_t* pairs, float* pts3d,
                              int32_t* n_tri, float* kernel_ms) {
    if (!p || !cameras || n_pairs < 0 || (n_pairs && !pairs) || (p->N && !pts3d)) return fail(SATBA_E_ARG, "null or negative argument");
    if (p->world != 1) return fail(SATBA_E_ARG, "satba_init_pts3d_resident: the handle holds a shard (world = %d)", p->world);
    // the handle's cameras ascend inside every track (k_lay_validate): the direct list pass applies whenever the pairs are listed in order
    bool ordered = getenv("SATBA_TRI_GENERAL") == nullptr;
    std::vector<int> first, next;
    TRY(tri_pair_tables(p->M, n_pairs, pairs, first, next, ordered));
    DevRun s;
    TRY(s.begin(p->device));
    HIP_TRY(hipStreamSynchronize(p->stream));  // (the layout is static, but a caller may still have work queued on the handle)
    const Layout& L = p->L;
    TriArgs a{};
    a.pt_ofs = L.ipt_ofs; a.cam_ind = L.e_cam; a.obs = reinterpret_cast<const double*>(L.e_obs);
    a.slice_base = L.slice_base; a.perm = L.perm;
    if (remove && p->K) {
        unsigned char *d_rm, *d_rm_ell;
        TRY(s.upload(&d_rm, (const unsigned char*)remove, (size_t)p->K));
        TRY(s.alloc(&d_rm_ell, (size_t)std::max(L.P, 1) + 64));
        HIP_TRY(hipMemsetAsync(d_rm_ell, 0, (size_t)std::max(L.P, 1) + 64, s.stream));
        hipLaunchKernelGGL(k_tri_mask_ell, dim3((unsigned)((p->K + 255) / 256)), dim3(256), 0, s.stream, p->K, L.obs_pos, d_rm, d_rm_ell);
        HIP_TRY(hipGetLastError());
        a.removed = d_rm_ell;
    }
    return tri_run(s, a, p->model, p->M, p->N, ordered, cameras, n_pairs, pairs, first, next, pts3d, n_tri, p->device, 1, kernel_ms);
}

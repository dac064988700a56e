// satba_utm_filter / satba_keypoints_utm (include/satba.h): part of the extern "C" block of satba_capi.hip; stand-alone (no
// handle).  The host checks the arguments and packs them; everything else is the kernels of satba_utm.h, a scan and a segmented sort.
int satba_utm_filter(int32_t n_pairs, const int64_t* pair_ofs, const double* utm, const uint8_t* alive, double margin, uint8_t* keep, double* thr,
                     int64_t* n_kept, int32_t device, float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.f;
    if (n_pairs < 0) return fail(SATBA_E_ARG, "negative pair count");
    if (!(margin >= 0.0) || !std::isfinite(margin)) return fail(SATBA_E_ARG, "margin must be finite and not negative");
    if (n_pairs == 0) return 0;
    if (!pair_ofs) return fail(SATBA_E_ARG, "null pair_ofs");
    if (pair_ofs[0] != 0) return fail(SATBA_E_ARG, "pair_ofs must start at 0");
    for (int p = 0; p < n_pairs; ++p)
        if (pair_ofs[p + 1] < pair_ofs[p]) return fail(SATBA_E_ARG, "pair_ofs decreases at pair %d", p);
    const int64_t n = pair_ofs[n_pairs];
    if (n >= (int64_t)1 << 31) return fail(SATBA_E_ARG, "more than 2^31 matches in one call");
    if (n && (!utm || !keep)) return fail(SATBA_E_ARG, "null utm or keep");
    for (int64_t i = 0; i < n; ++i)
        if ((!alive || alive[i]) && !cam_all_finite(utm + 4 * i, 4)) return fail(SATBA_E_ARG, "match %lld has a non-finite coordinate", (long long)i);
    const size_t np = (size_t)n_pairs;
    if (n == 0) {  // nothing for the device to do
        for (size_t p = 0; p < np; ++p) {
            if (thr) thr[p] = std::nan("");
            if (n_kept) n_kept[p] = 0;
        }
        return 0;
    }
    DevRun s;
    TRY(s.begin(device));
    static_assert(sizeof(long long) == sizeof(int64_t), "pair_ofs is uploaded as it is");
    double *d_utm, *d_d, *d_dc, *d_sorted, *d_thr;
    long long *d_ofs, *d_cnt;
    unsigned char *d_alive = nullptr, *d_keep;
    int *d_flag, *d_pos, *d_cofs;
    char *d_scan, *d_sort;
    TRY(s.upload(&d_utm, utm, (size_t)n * 4)); TRY(s.upload(&d_ofs, (const long long*)pair_ofs, np + 1));
    if (alive) TRY(s.upload(&d_alive, (const unsigned char*)alive, (size_t)n));
    TRY(s.alloc(&d_d, (size_t)n)); TRY(s.alloc(&d_dc, (size_t)n)); TRY(s.alloc(&d_sorted, (size_t)n)); TRY(s.alloc(&d_thr, np));
    TRY(s.alloc(&d_cnt, np)); TRY(s.alloc(&d_keep, (size_t)n)); TRY(s.alloc(&d_flag, (size_t)n)); TRY(s.alloc(&d_pos, (size_t)n));
    TRY(s.alloc(&d_cofs, np + 1));
    // the alive matches are at most n: the sort is sized for n and sorts what the compacted offsets delimit
    size_t need_scan = 0, need_sort = 0;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, need_scan, d_flag, d_pos, (int)n, s.stream));
    HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, need_sort, d_dc, d_sorted, (int)n, n_pairs, d_cofs, d_cofs + 1, 0, 64, s.stream));
    TRY(s.alloc(&d_scan, need_scan + 16)); TRY(s.alloc(&d_sort, need_sort + 16));
    const unsigned grid = (unsigned)grid_for(std::max<long long>(n, (long long)np + 1), UTM_THREADS, 4096);
    HIP_TRY(hipEventRecord(s.e0, s.stream));
    hipLaunchKernelGGL(k_utm_dist, dim3(grid), dim3(UTM_THREADS), 0, s.stream, (long long)n, d_utm, d_alive, d_d, d_flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_scan, need_scan, d_flag, d_pos, (int)n, s.stream));
    hipLaunchKernelGGL(k_utm_compact, dim3(grid), dim3(UTM_THREADS), 0, s.stream, (long long)n, n_pairs, d_ofs, d_d, d_flag, d_pos, d_dc, d_cofs);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortKeys(d_sort, need_sort, d_dc, d_sorted, (int)n, n_pairs, d_cofs, d_cofs + 1, 0, 64, s.stream));
    hipLaunchKernelGGL(k_utm_threshold, dim3(n_pairs), dim3(UTM_THREADS), 0, s.stream, d_ofs, d_cofs, d_sorted, d_d, d_flag, margin, d_keep, d_thr, d_cnt);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s.e1, s.stream));
    std::vector<double> h_thr(np);
    std::vector<long long> h_cnt(np);
    HIP_TRY(hipMemcpyAsync(keep, d_keep, (size_t)n, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipMemcpyAsync(h_thr.data(), d_thr, sizeof(double) * np, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipMemcpyAsync(h_cnt.data(), d_cnt, sizeof(long long) * np, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s.e0, s.e1));
    if (thr) memcpy(thr, h_thr.data(), sizeof(double) * np);
    if (n_kept) memcpy(n_kept, h_cnt.data(), sizeof(int64_t) * np);
    if (kernel_ms) *kernel_ms = ms;
    return 0;
}

int satba_keypoints_utm(int32_t n_cam, const double* tables, const int64_t* n_rows, const float* const* features, const double* col0row0,
                        const double* alt, const int32_t* zone, double* const* utm_out, double* const* lonlat_out, int32_t device, float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.f;
    if (n_cam < 0) return fail(SATBA_E_ARG, "negative image count");
    if (n_cam == 0) return 0;
    if (!tables || !n_rows || !features || !col0row0 || !alt || !zone || !utm_out) return fail(SATBA_E_ARG, "null argument");
    if (!cam_all_finite(tables, (size_t)n_cam * 90)) return fail(SATBA_E_ARG, "non-finite RPC record");
    if (!cam_all_finite(col0row0, (size_t)n_cam * 2) || !cam_all_finite(alt, (size_t)n_cam)) return fail(SATBA_E_ARG, "non-finite offset or altitude");
    int64_t total = 0;
    for (int c = 0; c < n_cam; ++c) {
        if (n_rows[c] < 0) return fail(SATBA_E_ARG, "image %d: negative row count", c);
        if (zone[c] < 0 || zone[c] > 60) return fail(SATBA_E_ARG, "image %d: zone %d outside 0..60", c, zone[c]);
        if (n_rows[c] && (!features[c] || !utm_out[c] || (lonlat_out && !lonlat_out[c]))) return fail(SATBA_E_ARG, "image %d: null array", c);
        total += n_rows[c];
        if (total >= (int64_t)1 << 31) return fail(SATBA_E_ARG, "more than 2^31 rows in one call");
    }
    if (total == 0) return 0;
    // the two columns the kernels read, of all images, and per image the number of keypoints in front of the padding
    std::vector<float2> xy((size_t)total);
    std::vector<KpImage> images((size_t)n_cam);
    std::vector<int2> blocks;
    int64_t base = 0;
    for (int c = 0; c < n_cam; ++c) {
        KpImage& im = images[c];
        im.base = base; im.n_rows = (int)n_rows[c]; im.n_kp = 0;
        im.col0 = col0row0[2 * c]; im.row0 = col0row0[2 * c + 1]; im.alt = alt[c]; im.zone = zone[c]; im.pad = 0;
        for (int64_t r = 0; r < n_rows[c]; ++r) {
            const float* f = features[c] + 132 * r;
            xy[(size_t)(base + r)] = make_float2(f[0], f[1]);
            im.n_kp += f[0] == f[0] ? 1 : 0;
        }
        for (int r = 0; r < im.n_rows; r += UTM_KP_THREADS) blocks.push_back(make_int2(c, r));
        base += n_rows[c];
    }
    DevRun s;
    TRY(s.begin(device));
    float2* d_xy;
    KpImage* d_images;
    int2* d_blocks;
    double* d_tab;
    double2 *d_ll, *d_utm;
    TRY(s.upload(&d_xy, (const float2*)xy.data(), xy.size())); TRY(s.upload(&d_images, (const KpImage*)images.data(), images.size()));
    TRY(s.upload(&d_blocks, (const int2*)blocks.data(), blocks.size())); TRY(s.upload(&d_tab, tables, (size_t)n_cam * 90));
    TRY(s.alloc(&d_ll, (size_t)total)); TRY(s.alloc(&d_utm, (size_t)total));
    HIP_TRY(hipEventRecord(s.e0, s.stream));
    hipLaunchKernelGGL(k_kp_localize, dim3((unsigned)blocks.size()), dim3(UTM_KP_THREADS), 0, s.stream, d_blocks, d_images, d_tab, d_xy, d_ll);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_kp_project, dim3((unsigned)blocks.size()), dim3(UTM_KP_THREADS), 0, s.stream, d_blocks, d_images, d_ll, d_utm);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s.e1, s.stream));
    std::vector<double2> h_utm((size_t)total), h_ll(lonlat_out ? (size_t)total : 0);
    HIP_TRY(hipMemcpyAsync(h_utm.data(), d_utm, sizeof(double2) * (size_t)total, hipMemcpyDeviceToHost, s.stream));
    if (lonlat_out) HIP_TRY(hipMemcpyAsync(h_ll.data(), d_ll, sizeof(double2) * (size_t)total, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s.e0, s.e1));
    for (int c = 0; c < n_cam; ++c) {
        if (!n_rows[c]) continue;
        memcpy(utm_out[c], h_utm.data() + images[c].base, sizeof(double2) * (size_t)n_rows[c]);
        if (lonlat_out) memcpy(lonlat_out[c], h_ll.data() + images[c].base, sizeof(double2) * (size_t)n_rows[c]);
    }
    if (kernel_ms) *kernel_ms = ms;
    return 0;
}

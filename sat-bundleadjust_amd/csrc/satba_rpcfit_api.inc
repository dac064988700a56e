// satba_rpc_fit / satba_rpc_localization (include/satba.h): part of the extern "C" block of satba_capi.hip; stand-alone (no handle)
int satba_rpc_fit(int32_t n_cam, int32_t n_samples, const double* target, const double* locs, double h, double tol, int32_t max_iter,
                  double* tables, double* rmse, int32_t* iters, int32_t device) {
    if (n_cam < 0 || n_samples < FIT_N || !target || !locs || !tables || max_iter < 0) return fail(SATBA_E_ARG, "bad argument (at least %d samples)", FIT_N);
    if (!cam_all_finite(target, (size_t)n_cam * n_samples * 2)) return fail(SATBA_E_NONFINITE, "non-finite target");
    if (!cam_all_finite(locs, (size_t)n_cam * n_samples * 3)) return fail(SATBA_E_NONFINITE, "non-finite location");
    if (n_cam == 0) return 0;
    DevRun s;
    TRY(s.begin(device));
    double *d_t, *d_l, *d_tab, *d_rmse;
    int* d_it;
    TRY(s.upload(&d_t, target, (size_t)n_cam * n_samples * 2)); TRY(s.upload(&d_l, locs, (size_t)n_cam * n_samples * 3));
    TRY(s.alloc(&d_tab, (size_t)n_cam * 90)); TRY(s.alloc(&d_rmse, (size_t)n_cam));
    TRY(s.alloc(&d_it, (size_t)n_cam));
    hipLaunchKernelGGL(k_rpc_fit, dim3(n_cam), dim3(FIT_THREADS), 0, s.stream, n_samples, d_t, d_l, h, tol, max_iter, d_tab, d_rmse, d_it);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(tables, d_tab, sizeof(double) * 90 * n_cam, hipMemcpyDeviceToHost, s.stream));
    if (rmse) HIP_TRY(hipMemcpyAsync(rmse, d_rmse, sizeof(double) * n_cam, hipMemcpyDeviceToHost, s.stream));
    if (iters) HIP_TRY(hipMemcpyAsync(iters, d_it, sizeof(int) * n_cam, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    return 0;
}

int satba_rpc_localization(const double* table, int64_t n, const double* col, const double* row, const double* alt, double* lon, double* lat,
                           int32_t device) {
    if (!table || n < 0 || (n && (!col || !row || !alt || !lon || !lat))) return fail(SATBA_E_ARG, "null argument");
    if (n == 0) return 0;
    DevRun s;
    TRY(s.begin(device));
    double *d_tab, *d_c, *d_r, *d_a, *d_lo, *d_la;
    TRY(s.upload(&d_tab, table, (size_t)90)); TRY(s.upload(&d_c, col, (size_t)n)); TRY(s.upload(&d_r, row, (size_t)n)); TRY(s.upload(&d_a, alt, (size_t)n));
    TRY(s.alloc(&d_lo, (size_t)n)); TRY(s.alloc(&d_la, (size_t)n));
    hipLaunchKernelGGL(k_rpc_localize, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s.stream, (long long)n, d_tab, d_c, d_r, d_a, d_lo, d_la);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(lon, d_lo, sizeof(double) * n, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipMemcpyAsync(lat, d_la, sizeof(double) * n, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    return 0;
}

int satba_rpc_refit(int32_t n_cam, const double* tables_in, const double* rt, const double* crops, const double* alt_ranges,
                    const double* global_transform, int32_t n_samples, double h, double tol, int32_t max_iter, double* tables_out, double* err,
                    double* margins, double* locs_out, double* target_out, int32_t device) {
    if (n_cam < 0 || !tables_in || !rt || !crops || !alt_ranges || !tables_out || !margins) return fail(SATBA_E_ARG, "null argument");
    if (n_samples < 4 || n_samples > REFIT_MAX_N) return fail(SATBA_E_ARG, "n_samples must be in [4, %d]", REFIT_MAX_N);
    if (n_cam == 0) return 0;
    const int n3 = n_samples * n_samples * n_samples;
    DevRun s;
    TRY(s.begin(device));
    std::vector<RefitCam> cams((size_t)n_cam);
    for (int c = 0; c < n_cam; ++c) {
        RefitCam& q = cams[c];
        memcpy(q.table, tables_in + (size_t)c * 90, sizeof q.table);
        memcpy(q.rt, rt + (size_t)c * 9, sizeof q.rt);
        memcpy(q.crop, crops + (size_t)c * 4, sizeof q.crop);
        q.alt[0] = alt_ranges[2 * c]; q.alt[1] = alt_ranges[2 * c + 1];
        q.margin = 10.0; q.slot = c; q.pad = 0;
    }
    const double zero3[3] = {0.0, 0.0, 0.0};
    RefitCam* d_cams;
    double *d_gt, *d_grid, *d_locs, *d_target, *d_tab, *d_err;
    int* d_cov;
    TRY(s.alloc(&d_cams, (size_t)n_cam)); TRY(s.upload(&d_gt, global_transform ? global_transform : zero3, (size_t)3));
    TRY(s.alloc(&d_grid, (size_t)n_cam * n3 * 3)); TRY(s.alloc(&d_locs, (size_t)n_cam * n3 * 3));
    TRY(s.alloc(&d_target, (size_t)n_cam * n3 * 2)); TRY(s.alloc(&d_tab, (size_t)n_cam * 90));
    TRY(s.alloc(&d_err, (size_t)n_cam * n3)); TRY(s.alloc(&d_cov, (size_t)n_cam));
    std::vector<int> todo((size_t)n_cam), cov((size_t)n_cam);
    for (int c = 0; c < n_cam; ++c) todo[c] = c;
    std::vector<RefitCam> batch;
    while (!todo.empty()) {
        // the cameras of this round, compacted to the front of the device list; slot keeps every camera's place in the output arrays
        // (k_rpc_fit works per slot: it is launched over all slots of the round through an index-free trick -- the round's cameras are
        // fitted in place of their slots by launching one workgroup per camera with the slot's base pointers)
        batch.clear();
        for (int c : todo) batch.push_back(cams[c]);
        HIP_TRY(hipMemcpyAsync(d_cams, batch.data(), sizeof(RefitCam) * batch.size(), hipMemcpyHostToDevice, s.stream));
        const int nb = (int)batch.size();
        hipLaunchKernelGGL(k_refit_grid, dim3((n3 + 255) / 256, nb), dim3(256), 0, s.stream, n_samples, d_cams, d_gt, d_grid, d_locs, d_target);
        for (int b = 0; b < nb; ++b) {  // (slots of a later round are scattered: one launch per run of consecutive slots)
            int e = b;
            while (e + 1 < nb && batch[e + 1].slot == batch[e].slot + 1) ++e;
            const int s0 = batch[b].slot, cnt = e - b + 1;
            hipLaunchKernelGGL(k_rpc_fit, dim3(cnt), dim3(FIT_THREADS), 0, s.stream, n3, d_target + (size_t)s0 * n3 * 2, d_locs + (size_t)s0 * n3 * 3, h, tol,
                               max_iter, d_tab + (size_t)s0 * 90, (double*)nullptr, (int*)nullptr);
            b = e;
        }
        const size_t hull_b = sizeof(double2) * (size_t)n3;  // the re-projected nodes in LDS: 16 KB at the reference's 10 nodes per axis
        if (hull_b > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)k_refit_check, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hull_b));
        hipLaunchKernelGGL(k_refit_check, dim3(nb), dim3(256), hull_b, s.stream, n_samples, d_cams, d_tab, d_grid, d_locs, d_target, d_err, d_cov);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(cov.data(), d_cov, sizeof(int) * n_cam, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipStreamSynchronize(s.stream));
        std::vector<int> nxt;
        for (int c : todo) {
            if (cams[c].margin > 1000.0 || cov[c]) margins[c] = cams[c].margin;  // done (ba_rpcfit.py:263, 341: margin > 1000 gives up)
            else { cams[c].margin *= 2.0; nxt.push_back(c); }
        }
        todo.swap(nxt);
    }
    HIP_TRY(hipMemcpyAsync(tables_out, d_tab, sizeof(double) * 90 * n_cam, hipMemcpyDeviceToHost, s.stream));
    if (err) HIP_TRY(hipMemcpyAsync(err, d_err, sizeof(double) * n_cam * n3, hipMemcpyDeviceToHost, s.stream));
    if (locs_out) HIP_TRY(hipMemcpyAsync(locs_out, d_locs, sizeof(double) * n_cam * n3 * 3, hipMemcpyDeviceToHost, s.stream));
    if (target_out) HIP_TRY(hipMemcpyAsync(target_out, d_target, sizeof(double) * n_cam * n3 * 2, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    for (int i = 0; i < n_cam * 90; ++i)
        if (!std::isfinite(tables_out[i])) return fail(SATBA_E_NONFINITE, "Singular matrix");
    return 0;
}

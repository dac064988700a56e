// satba_outliers (include/satba.h): part of the extern "C" block of satba_capi.hip
int satba_outliers(satba_problem* p, const double* err, double predef_thr, double min_thr, double* cam_thr, uint8_t* remove, int64_t* n_removed) {
    if (!p || !cam_thr || !remove || !n_removed) return fail(SATBA_E_ARG, "null argument");
    // NaN is neither "< 0" (sort the errors) nor ">= 0" (skip the elbow): the elbow kernel would read a buffer nobody sorted
    if (predef_thr != predef_thr || min_thr != min_thr) return fail(SATBA_E_ARG, "predef_thr / min_thr is NaN");
    HIP_TRY(hipSetDevice(p->device));
    const long long K = p->K;
    const Layout& L = p->L;
    const size_t Pz = (size_t)std::max(L.P, 1) + 64, Kz = (size_t)std::max<long long>(K, 1);
    double *d_err = nullptr, *d_cm = nullptr, *d_sorted = nullptr, *d_thr = nullptr, *d_in = nullptr;
    double2* d_f = nullptr;
    unsigned char* d_rm = nullptr;
    unsigned long long* d_cnt = nullptr;
    char* d_cub = nullptr;
    DevAllocs tmp;
    TRY(tmp.alloc(&d_err, Pz)); TRY(tmp.alloc(&d_cm, Kz)); TRY(tmp.alloc(&d_sorted, Kz));
    TRY(tmp.alloc(&d_thr, (size_t)p->M)); TRY(tmp.alloc(&d_rm, Kz)); TRY(tmp.alloc(&d_cnt, 1));
    HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), p->stream));
    HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(double) * Pz, p->stream));
    if (err) {
        TRY(tmp.alloc(&d_in, Kz));
        if (K) HIP_TRY(hipMemcpyAsync(d_in, err, sizeof(double) * K, hipMemcpyHostToDevice, p->stream));
        if (K) hipLaunchKernelGGL(k_out_scatter_ell, dim3(grid_for(K, 256, 4096)), dim3(256), 0, p->stream, K, L.obs_pos, d_in, d_err);
    } else {
        // reprojection errors at the current x: linear-loss residuals, whatever loss the handle is configured for
        TRY(tmp.alloc(&d_f, Pz));
        const int loss = p->loss;
        p->loss = 0;
        int r2 = launch_residual(p, false, d_f, p->d_scal);
        p->loss = loss;
        if (r2) return r2;
        hipLaunchKernelGGL(k_out_err_ell, dim3(grid_for(L.P, 256, 4096)), dim3(256), 0, p->stream, L.P, L.e_cam, d_f, L.e_w, d_err);
    }
    if (K) hipLaunchKernelGGL(k_out_gather_cm, dim3(grid_for(K, 256, 4096)), dim3(256), 0, p->stream, K, L.cm_pos, d_err, d_cm);
    HIP_TRY(hipGetLastError());
    if (predef_thr < 0.0 && K) {  // ascending errors of every camera
        size_t need = 0;
        HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortKeys(nullptr, need, d_cm, d_sorted, (int)K, p->M, L.cam_ofs, L.cam_ofs + 1, 0, 64, p->stream));
        TRY(tmp.alloc(&d_cub, need + 16));
        HIP_TRY(hipcub::DeviceSegmentedRadixSort::SortKeys(d_cub, need, d_cm, d_sorted, (int)K, p->M, L.cam_ofs, L.cam_ofs + 1, 0, 64, p->stream));
    }
    hipLaunchKernelGGL(k_out_elbow, dim3(p->M), dim3(256), 0, p->stream, L.cam_ofs, d_sorted, predef_thr, min_thr, d_thr);
    if (K) hipLaunchKernelGGL(k_out_mask, dim3(grid_for(K, 256, 4096)), dim3(256), 0, p->stream, K, L.obs_pos, L.e_cam, d_err, d_thr, d_rm, d_cnt);
    HIP_TRY(hipGetLastError());
    unsigned long long cnt = 0;
    HIP_TRY(hipMemcpyAsync(cam_thr, d_thr, sizeof(double) * p->M, hipMemcpyDeviceToHost, p->stream));
    if (K) HIP_TRY(hipMemcpyAsync(remove, d_rm, (size_t)K, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipMemcpyAsync(&cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    *n_removed = (int64_t)cnt;
    return 0;
}

// satba_reprojection_errors (include/satba.h): err_k = | |f_k / w_k| |_2 of the linear-loss residual pair at the current x, caller's
// observation order -- ref:bundle_adjust/ba_core.py:335-349 applied to ba_core.fun's output, operation for operation (correctly
// rounded division, squares, addition and square root: k_out_err_ell), without the residual vector crossing the bus (2 K doubles
// down and three numpy passes over them on the host otherwise: 0.07 s per call at 10 M observations).
// The same errors in two steps, so that the download can run beside the solve that follows (the drop-in call returns err_init, which
// nothing on the device needs again): _begin queues the kernels into a buffer of its own and records an event; _fetch, which may be
// called from another host thread while this handle solves, moves the buffer over the copy lanes (copy_big: their streams wait for
// the event; neither p->stream nor the staging buffers are touched).
int satba_reprojection_errors_begin(satba_problem* p) {
    Range range_("satba:reprojection_errors_begin");
    if (!p) return fail(SATBA_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    const Layout& L = p->L;
    if (!p->d_err_keep) TRY(dev_alloc(p, &p->d_err_keep, (size_t)std::max<long long>(p->K, 1)));
    if (!p->ev_err) HIP_TRY(hipEventCreateWithFlags(&p->ev_err, hipEventDisableTiming));
    TRY(copy_lanes_init(p));  // (not in the fetching thread: hipHostMalloc beside a running solve)
    const int loss = p->loss;
    p->loss = 0;
    const int rc = launch_residual(p, false, p->d_ftmp, p->d_scal);
    p->loss = loss;
    if (rc) return rc;
    if (p->K > 0) {
        double* err_ell = reinterpret_cast<double*>(p->d_f);
        p->f_valid = false;
        hipLaunchKernelGGL(k_out_err_ell, dim3(grid_for(L.P, 256, 4096)), dim3(256), 0, p->stream, L.P, L.e_cam, p->d_ftmp, L.e_w, err_ell);
        hipLaunchKernelGGL(k_gather_obs1, dim3(grid_for(p->K, 256, 4096)), dim3(256), 0, p->stream, p->K, L.obs_pos, err_ell, p->d_err_keep);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(p->ev_err, p->stream));
    return 0;
}
int satba_reprojection_errors_fetch(satba_problem* p, double* host_err) {
    Range range_("satba:reprojection_errors_fetch");
    if (!p || !host_err) return fail(SATBA_E_ARG, "null argument");
    if (!p->ev_err || !p->d_err_keep) return fail(SATBA_E_STATE, "satba_reprojection_errors_fetch before _begin");
    HIP_TRY(hipSetDevice(p->device));
    if (p->K <= 0) return 0;
    return copy_big(p, reinterpret_cast<char*>(host_err), reinterpret_cast<char*>(p->d_err_keep), sizeof(double) * (size_t)p->K, true, p->ev_err);
}

int satba_reprojection_errors(satba_problem* p, double* host_err, double* host_cost) {
    Range range_("satba:reprojection_errors");
    if (!p || !host_err) return fail(SATBA_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    const Layout& L = p->L;
    const int loss = p->loss;
    p->loss = 0;  // reprojection errors are those of the plain residuals, whatever loss the handle is configured for
    const int rc = launch_residual(p, false, p->d_ftmp, p->d_scal);
    p->loss = loss;
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(p->h_pin, p->d_scal, sizeof(double), hipMemcpyDeviceToHost, p->stream));
    if (p->K > 0) {
        double* err_ell = reinterpret_cast<double*>(p->d_f);  // (scratch: d_f only holds the residuals of a camera-major linearisation)
        p->f_valid = false;
        hipLaunchKernelGGL(k_out_err_ell, dim3(grid_for(L.P, 256, 4096)), dim3(256), 0, p->stream, L.P, L.e_cam, p->d_ftmp, L.e_w, err_ell);
        hipLaunchKernelGGL(k_gather_obs1, dim3(grid_for(p->K, 256, 4096)), dim3(256), 0, p->stream, p->K, L.obs_pos, err_ell, p->d_stage);
        HIP_TRY(hipGetLastError());
        TRY(copy_to_host(p, host_err, p->d_stage, sizeof(double) * p->K));
    }
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (host_cost) *host_cost = p->h_pin[0];
    return 0;
}

// satba_rpc_affine_approx / satba_rpc_perspective_approx / satba_camera_resection / satba_rpc_mesh (include/satba.h): part of the
// extern "C" block of satba_capi.hip; stand-alone (no handle)
extern "C++" {
namespace {
// results reach the caller only when every one of them is finite: a degenerate camera is an error code, never a NaN matrix
int cam_hand_over(const std::vector<double>& h, size_t n_cam, double* P_out, double* mean_err, double* centers) {
    if (!cam_all_finite(h.data(), h.size())) return fail(SATBA_E_NONFINITE, "Singular matrix: degenerate points, no camera fits them");
    memcpy(P_out, h.data(), sizeof(double) * 12 * n_cam);
    if (mean_err) memcpy(mean_err, h.data() + 12 * n_cam, sizeof(double) * n_cam);
    if (centers) memcpy(centers, h.data() + 13 * n_cam, sizeof(double) * 3 * n_cam);
    return 0;
}
int cam_mesh_check(int32_t n_cam, const double* tables, const double* col_range, const double* row_range, const double* alt_range, int32_t n_col,
                   int32_t n_row, int32_t n_alt) {
    if (n_cam < 0 || !tables || !col_range || !row_range || !alt_range) return fail(SATBA_E_ARG, "null argument or negative count");
    if (n_col < 2 || n_row < 2 || n_alt < 2) return fail(SATBA_E_ARG, "a mesh needs at least 2 samples on every axis");
    if ((long long)n_col * n_row * n_alt > CAM_MAX_PTS) return fail(SATBA_E_ARG, "mesh larger than %d nodes", CAM_MAX_PTS);
    if (!cam_all_finite(tables, (size_t)n_cam * 90)) return fail(SATBA_E_NONFINITE, "non-finite RPC table");
    for (const double* r : {col_range, row_range, alt_range}) {
        if (!cam_all_finite(r, (size_t)n_cam * 2)) return fail(SATBA_E_NONFINITE, "non-finite mesh range");
        for (int c = 0; c < n_cam; ++c)
            if (r[2 * c] == r[2 * c + 1]) return fail(SATBA_E_NONFINITE, "Singular matrix: the mesh of camera %d has no extent on one axis", c);
    }
    return 0;
}
int cam_launch_resect(DevRun& s, CamResectArgs& a, int n_cam, double* P_out, double* mean_err, double* centers) {
    double* d_out;
    TRY(s.alloc(&d_out, (size_t)n_cam * 16));
    a.P = d_out; a.mean_err = d_out + (size_t)n_cam * 12; a.centers = d_out + (size_t)n_cam * 13; a.alts = nullptr;
    const size_t lds_b = a.n_pts <= CAM_LDS_PTS ? sizeof(double) * 5 * (size_t)a.n_pts : 0;
    if (lds_b > 48 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)k_cam_resect<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_b));
    hipLaunchKernelGGL(k_cam_resect<false>, dim3(n_cam), dim3(CAM_THREADS), lds_b, s.stream, a);
    HIP_TRY(hipGetLastError());
    std::vector<double> h((size_t)n_cam * 16);
    HIP_TRY(hipMemcpyAsync(h.data(), d_out, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    if (!centers) h.resize((size_t)n_cam * 13);  // a centre nobody asked for (at infinity for an affine set of points) fails nothing
    return cam_hand_over(h, (size_t)n_cam, P_out, mean_err, centers);
}
}  // namespace
}  // extern "C++"

int satba_rpc_affine_approx(int32_t n_cam, const double* tables, const double* xyz, const double* col0row0, double* P_out, int32_t device) {
    if (n_cam < 0 || !tables || !xyz || !col0row0 || !P_out) return fail(SATBA_E_ARG, "null argument or negative count");
    if (!cam_all_finite(tables, (size_t)n_cam * 90) || !cam_all_finite(xyz, (size_t)n_cam * 3) || !cam_all_finite(col0row0, (size_t)n_cam * 2))
        return fail(SATBA_E_NONFINITE, "non-finite input");
    if (n_cam == 0) return 0;
    DevRun s;
    TRY(s.begin(device));
    double *d_tab, *d_xyz, *d_c0, *d_P;
    TRY(s.upload(&d_tab, tables, (size_t)n_cam * 90)); TRY(s.upload(&d_xyz, xyz, (size_t)n_cam * 3)); TRY(s.upload(&d_c0, col0row0, (size_t)n_cam * 2));
    TRY(s.alloc(&d_P, (size_t)n_cam * 12));
    hipLaunchKernelGGL(k_cam_affine, dim3((n_cam + CAM_THREADS - 1) / CAM_THREADS), dim3(CAM_THREADS), 0, s.stream, n_cam, d_tab, d_xyz, d_c0, d_P);
    HIP_TRY(hipGetLastError());
    std::vector<double> h((size_t)n_cam * 12);
    HIP_TRY(hipMemcpyAsync(h.data(), d_P, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    return cam_hand_over(h, (size_t)n_cam, P_out, nullptr, nullptr);  // (an expansion point on the polar axis has no longitude)
}

int satba_rpc_perspective_approx(int32_t n_cam, const double* tables, const double* col_range, const double* row_range, const double* alt_range,
                                 int32_t n_col, int32_t n_row, int32_t n_alt, const double* crop0, double* P_out, double* mean_err, double* centers,
                                 int32_t device) {
    TRY(cam_mesh_check(n_cam, tables, col_range, row_range, alt_range, n_col, n_row, n_alt));
    if (!P_out) return fail(SATBA_E_ARG, "null argument");
    if (crop0 && !cam_all_finite(crop0, (size_t)n_cam * 2)) return fail(SATBA_E_NONFINITE, "non-finite crop offset");
    if (n_cam == 0) return 0;
    DevRun s;
    TRY(s.begin(device));
    CamResectArgs a{};
    a.n_pts = n_col * n_row * n_alt; a.n_col = n_col; a.n_row = n_row; a.n_alt = n_alt;
    double *d_tab, *d_cr, *d_rr, *d_ar, *d_c0 = nullptr;
    TRY(s.upload(&d_tab, tables, (size_t)n_cam * 90)); TRY(s.upload(&d_cr, col_range, (size_t)n_cam * 2)); TRY(s.upload(&d_rr, row_range, (size_t)n_cam * 2));
    TRY(s.upload(&d_ar, alt_range, (size_t)n_cam * 2));
    if (crop0) TRY(s.upload(&d_c0, crop0, (size_t)n_cam * 2));
    a.tables = d_tab; a.col_range = d_cr; a.row_range = d_rr; a.alt_range = d_ar; a.crop0 = d_c0;
    if (a.n_pts > CAM_LDS_PTS) {  // the mesh does not fit the LDS: a slab per camera
        TRY(s.alloc(&a.X, (size_t)n_cam * a.n_pts * 3)); TRY(s.alloc(&a.x, (size_t)n_cam * a.n_pts * 2));
    }
    return cam_launch_resect(s, a, n_cam, P_out, mean_err, centers);
}

int satba_camera_resection(int32_t n_cam, int32_t n_pts, const double* X, const double* x, double* P_out, double* mean_err, int32_t device) {
    if (n_cam < 0 || n_pts < 0 || !X || !x || !P_out) return fail(SATBA_E_ARG, "null argument or negative count");
    if (n_pts < 6 || n_pts > CAM_MAX_PTS) return fail(SATBA_E_ARG, "a resection needs 6 to %d correspondences", CAM_MAX_PTS);
    if (!cam_all_finite(X, (size_t)n_cam * n_pts * 3) || !cam_all_finite(x, (size_t)n_cam * n_pts * 2)) return fail(SATBA_E_NONFINITE, "non-finite point");
    if (n_cam == 0) return 0;
    DevRun s;
    TRY(s.begin(device));
    CamResectArgs a{};
    a.n_pts = n_pts;
    TRY(s.upload(&a.X, X, (size_t)n_cam * n_pts * 3)); TRY(s.upload(&a.x, x, (size_t)n_cam * n_pts * 2));
    return cam_launch_resect(s, a, n_cam, P_out, mean_err, nullptr);
}

int satba_rpc_mesh(int32_t n_cam, const double* tables, const double* col_range, const double* row_range, const double* alt_range, int32_t n_col,
                   int32_t n_row, int32_t n_alt, double* X_out, double* x_out, double* alt_out, int32_t device) {
    TRY(cam_mesh_check(n_cam, tables, col_range, row_range, alt_range, n_col, n_row, n_alt));
    if (!X_out || !x_out) return fail(SATBA_E_ARG, "null argument");
    if (n_cam == 0) return 0;
    DevRun s;
    TRY(s.begin(device));
    CamResectArgs a{};
    a.n_pts = n_col * n_row * n_alt; a.n_col = n_col; a.n_row = n_row; a.n_alt = n_alt;
    const size_t n = (size_t)n_cam * a.n_pts;
    double *d_tab, *d_cr, *d_rr, *d_ar;
    TRY(s.upload(&d_tab, tables, (size_t)n_cam * 90)); TRY(s.upload(&d_cr, col_range, (size_t)n_cam * 2)); TRY(s.upload(&d_rr, row_range, (size_t)n_cam * 2));
    TRY(s.upload(&d_ar, alt_range, (size_t)n_cam * 2));
    a.tables = d_tab; a.col_range = d_cr; a.row_range = d_rr; a.alt_range = d_ar;
    TRY(s.alloc(&a.X, n * 3)); TRY(s.alloc(&a.x, n * 2)); TRY(s.alloc(&a.alts, n));
    hipLaunchKernelGGL(k_cam_resect<true>, dim3(n_cam), dim3(CAM_THREADS), 0, s.stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(X_out, a.X, sizeof(double) * n * 3, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipMemcpyAsync(x_out, a.x, sizeof(double) * n * 2, hipMemcpyDeviceToHost, s.stream));
    if (alt_out) HIP_TRY(hipMemcpyAsync(alt_out, a.alts, sizeof(double) * n, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    return 0;
}

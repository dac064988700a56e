// satba_rpc_fundamental / satba_rpc_fundamental_kernel_ms (include/satba.h): part of the extern "C" block of satba_capi.hip;
// stand-alone (no handle)
extern "C++" {
namespace {
thread_local double g_fundamental_ms = 0.0;
// the mesh of ref:bundle_adjust/s2p/rpc_utils.py:218-220, 241 in the reference's arithmetic: every operation rounded on its own
void fnd_ranges(const double* roi, const double* tab, int n, double* out) {
#pragma clang fp contract(off)
    const double lo = 1.0 / (2 * n), hi = (2 * n - 1.0) / (2 * n);
    out[0] = roi[0] + lo * roi[2]; out[1] = roi[0] + hi * roi[2];
    out[2] = roi[1] + lo * roi[3]; out[3] = roi[1] + hi * roi[3];
    out[4] = tab[84] - tab[85]; out[5] = tab[84] + tab[85];
}
}  // namespace
}  // extern "C++"

int satba_rpc_fundamental(int32_t n_cam, const double* tables, int32_t n_pairs, const int32_t* pairs, const double* roi, int32_t n, double* F5,
                          double* sv, double* matches, uint8_t* degenerate, int32_t device) {
    if (n_cam < 0 || n_pairs < 0 || !tables || !pairs || !roi || !F5) return fail(SATBA_E_ARG, "null argument or negative count");
    if (n < 2 || n > FND_MAX_N) return fail(SATBA_E_ARG, "the mesh takes 2 to %d samples per axis, got %d", FND_MAX_N, n);
    for (int p = 0; p < 2 * n_pairs; ++p)
        if (pairs[p] < 0 || pairs[p] >= n_cam) return fail(SATBA_E_ARG, "pair %d names image %d outside 0..%d", p / 2, pairs[p], n_cam - 1);
    if (!cam_all_finite(tables, (size_t)n_cam * 90)) return fail(SATBA_E_NONFINITE, "non-finite RPC table");
    if (!cam_all_finite(roi, (size_t)n_pairs * 4)) return fail(SATBA_E_NONFINITE, "non-finite region of interest");
    for (int p = 0; p < n_pairs; ++p)
        if (!(roi[4 * p + 2] > 0.0 && roi[4 * p + 3] > 0.0)) return fail(SATBA_E_ARG, "pair %d: the region of interest needs w > 0 and h > 0", p);
    g_fundamental_ms = 0.0;
    if (n_pairs == 0) return 0;
    const size_t np = (size_t)n_pairs, n3 = (size_t)n * n * n;
    std::vector<double> ranges(np * 6);
    for (size_t p = 0; p < np; ++p) fnd_ranges(roi + 4 * p, tables + (size_t)pairs[2 * p] * 90, n, ranges.data() + 6 * p);
    DevRun s;
    TRY(s.begin(device));
    FundamentalArgs a{};
    a.n = n;
    double *d_tab, *d_rg, *d_out;
    int *d_pairs, *d_status;
    TRY(s.upload(&d_tab, tables, (size_t)n_cam * 90)); TRY(s.upload(&d_rg, ranges.data(), ranges.size())); TRY(s.upload(&d_pairs, pairs, np * 2));
    TRY(s.alloc(&d_out, np * 9)); TRY(s.alloc(&d_status, np));
    if (matches) TRY(s.alloc(&a.matches, np * n3 * 4));
    a.tables = d_tab; a.pairs = d_pairs; a.ranges = d_rg; a.F5 = d_out; a.sv = d_out + np * 5; a.status = d_status;
    HIP_TRY(hipEventRecord(s.e0, s.stream));
    hipLaunchKernelGGL(k_fundamental, dim3(n_pairs), dim3(FND_THREADS), sizeof(double) * 4 * n3, s.stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s.e1, s.stream));
    std::vector<double> h(np * 9);
    std::vector<int> st(np);
    HIP_TRY(hipMemcpyAsync(h.data(), d_out, sizeof(double) * h.size(), hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipMemcpyAsync(st.data(), d_status, sizeof(int) * np, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s.e0, s.e1));
    // results reach the caller only when every pair has a matrix, or when the caller takes the flags: a NaN matrix is never
    // returned as if it were one
    if (!degenerate)
        for (size_t p = 0; p < np; ++p)
            if (st[p]) return fail(SATBA_E_NONFINITE, "Singular matrix: pair %zu (images %d, %d) has no unique affine fundamental matrix", p, pairs[2 * p], pairs[2 * p + 1]);
    if (matches) {
        HIP_TRY(hipMemcpyAsync(matches, a.matches, sizeof(double) * np * n3 * 4, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipStreamSynchronize(s.stream));
    }
    memcpy(F5, h.data(), sizeof(double) * np * 5);
    if (sv) memcpy(sv, h.data() + np * 5, sizeof(double) * np * 4);
    if (degenerate)
        for (size_t p = 0; p < np; ++p) degenerate[p] = st[p] ? 1 : 0;
    g_fundamental_ms = (double)ms;
    return 0;
}

double satba_rpc_fundamental_kernel_ms(void) { return g_fundamental_ms; }

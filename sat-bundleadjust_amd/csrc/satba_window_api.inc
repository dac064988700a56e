// satba_match_window (include/satba.h): part of the extern "C" block of satba_capi.hip, behind satba_match_api.inc, whose front
// (mt_front: uploads, pack, select), tail (mt_emit: scan, emit) and handle it shares.  Kernels: satba_window.h.
extern "C++" {
namespace {
int wn_run(satba_matches* m, int32_t n_cam, const int64_t* n_kp, const float* const* features, const double* const* utm, int32_t n_pairs,
           const int32_t* pairs, const double* boxes, double rx, double ry, float thr, int64_t* counts, int32_t device, float* kernel_ms) {
    const float thr2 = thr * thr;  // float32, as in satba_match_pairs
    DevRun s;
    MtFront f;
    counts[0] = counts[1] = counts[2] = counts[3] = counts[4] = 0;
    TRY(mt_front(s, m, f, n_cam, n_kp, features, utm, n_pairs, pairs, boxes, nullptr, device));
    const long long n_slots = f.n_slots;

    // the second sides' selections behind one another: what is sorted
    std::vector<int> seg((size_t)n_pairs + 1, 0);
    long long n_sort = 0;
    int max_side = 0;
    for (int32_t p = 0; p < n_pairs; ++p) {
        const MatchPair& P = f.hp[(size_t)p];
        counts[1] += P.n[0] + P.n[1];
        if (!P.n[0] || !P.n[1]) ++counts[2];
        seg[(size_t)p] = (int)n_sort;
        n_sort += P.n[1];  // below 2^31: the slots are
        max_side = std::max(max_side, P.n[1]);
    }
    seg[(size_t)n_pairs] = (int)n_sort;
    int pair_bits = 1;
    while (pair_bits < WC_PAIR_BITS && (1ll << pair_bits) < n_pairs) ++pair_bits;

    WcGrid* d_grids; int *d_seg, *d_val, *d_wj, *d_wrow, *d_wnrm; unsigned long long *d_key, *d_keys, *d_cand; double2* d_wutm;
    TRY(s.alloc(&d_grids, (size_t)n_pairs)); TRY(s.upload(&d_seg, seg.data(), seg.size()));
    TRY(s.alloc(&d_key, (size_t)n_sort)); TRY(s.alloc(&d_keys, (size_t)n_sort));
    TRY(s.alloc(&d_val, (size_t)n_sort)); TRY(s.alloc(&d_wj, (size_t)n_sort));
    TRY(s.alloc(&d_wrow, (size_t)n_sort)); TRY(s.alloc(&d_wnrm, (size_t)n_sort));
    TRY(s.alloc(&d_wutm, (size_t)n_sort)); TRY(s.alloc(&d_cand, 1));
    HIP_TRY(hipMemsetAsync(d_cand, 0, sizeof(unsigned long long), s.stream));
    TRY(mt_scan_scratch(s, f));
    size_t tmp_sort = 0;
    char* d_tmp_sort = nullptr;
    const unsigned end_bit = (unsigned)(2 * WC_DIM_BITS + pair_bits);
    if (n_sort) {
        HIP_TRY(rocprim::radix_sort_pairs(nullptr, tmp_sort, d_key, d_keys, d_val, d_wj, (size_t)n_sort, 0u, end_bit, s.stream));
        TRY(s.alloc(&d_tmp_sort, tmp_sort + 16));
        hipLaunchKernelGGL(k_window_grid, dim3((unsigned)n_pairs), dim3(WN_THREADS), 0, s.stream, f.d_pairs, f.d_utm, f.d_sel, rx, ry, d_grids);
        const unsigned gy = (unsigned)std::min(1024, (max_side + WN_THREADS - 1) / WN_THREADS);
        hipLaunchKernelGGL(k_window_keys, dim3((unsigned)n_pairs, gy), dim3(WN_THREADS), 0, s.stream, f.d_pairs, f.d_utm, f.d_sel, d_grids, d_seg, d_key, d_val);
        HIP_TRY(hipGetLastError());
        HIP_TRY(rocprim::radix_sort_pairs(d_tmp_sort, tmp_sort, d_key, d_keys, d_val, d_wj, (size_t)n_sort, 0u, end_bit, s.stream));
        hipLaunchKernelGGL(k_window_gather, dim3((unsigned)((n_sort + WN_THREADS - 1) / WN_THREADS)), dim3(WN_THREADS), 0, s.stream, (int)n_sort, f.d_pairs,
                           d_keys, d_wj, f.d_sel, f.d_utm, f.d_nrm, d_wutm, d_wrow, d_wnrm);
        const dim3 grid((unsigned)((n_slots + WN_THREADS / WN_LANES - 1) / (WN_THREADS / WN_LANES)));
        if (f.float_path)
            hipLaunchKernelGGL((k_window_nearest<WN_LANES, true>), grid, dim3(WN_THREADS), 0, s.stream, n_slots, f.d_pairs, f.d_slot_pair, d_grids, d_seg, f.d_sel,
                               f.d_utm, f.d_nrm_s, d_keys, d_wutm, d_wrow, d_wj, d_wnrm, f.d_rec, f.d_feat, rx, ry, thr2, f.d_hit, f.d_kpj, d_cand);
        else
            hipLaunchKernelGGL((k_window_nearest<WN_LANES, false>), grid, dim3(WN_THREADS), 0, s.stream, n_slots, f.d_pairs, f.d_slot_pair, d_grids, d_seg, f.d_sel,
                               f.d_utm, f.d_nrm_s, d_keys, d_wutm, d_wrow, d_wj, d_wnrm, f.d_rec, f.d_feat, rx, ry, thr2, f.d_hit, f.d_kpj, d_cand);
        HIP_TRY(hipGetLastError());
    }
    unsigned long long n_cand = 0;
    HIP_TRY(hipMemcpyAsync(&n_cand, d_cand, sizeof n_cand, hipMemcpyDeviceToHost, s.stream));
    TRY(mt_emit(s, m, f, counts, kernel_ms));  // synchronises the stream
    counts[4] = (int64_t)n_cand;
    return 0;
}
}  // namespace
}  // extern "C++"

int satba_match_window(int32_t n_cam, const int64_t* n_kp, const float* const* features, const double* const* utm, int32_t n_pairs, const int32_t* pairs,
                       const double* boxes, double rx, double ry, float thr, satba_matches** out, int64_t* counts, int32_t device, float* kernel_ms) {
    if (!out || !counts || !n_kp || !features || !utm || n_cam <= 0 || n_pairs < 0) return fail(SATBA_E_ARG, "null or negative argument");
    *out = nullptr;
    if (n_pairs && (!pairs || !boxes)) return fail(SATBA_E_ARG, "null pairs or boxes");
    if (!(thr > 0.0f)) return fail(SATBA_E_ARG, "thr must be positive, got %g", (double)thr);
    if (!(rx > 0.0) || !(ry > 0.0)) return fail(SATBA_E_ARG, "the window's half-widths must be positive (+inf is fine), got %g x %g", rx, ry);
    if ((long long)n_pairs >= 1ll << WC_PAIR_BITS) return fail(SATBA_E_ARG, "fewer than 2^%d pairs are supported", WC_PAIR_BITS);
    TRY(mt_check_pairs(n_cam, n_kp, features, utm, n_pairs, pairs, boxes));
    satba_matches* m = new (std::nothrow) satba_matches();
    if (!m) return fail(SATBA_E_ARG, "out of host memory");
    const int rc = wn_run(m, n_cam, n_kp, features, utm, n_pairs, pairs, boxes, rx, ry, thr, counts, device, kernel_ms);
    if (rc) {
        mt_free(m);
        return rc;
    }
    *out = m;
    return 0;
}

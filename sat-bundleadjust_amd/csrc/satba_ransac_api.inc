// satba_ransac_fundamental / satba_ransac_models (include/satba.h): part of the extern "C" block of satba_capi.hip; stand-alone
// (no handle).  The host checks the arguments, normalises every pair (satba_ransac_geom.h, sums in the caller's order) and builds
// the item table of k_ransac_score; everything else is the three kernels of satba_ransac.h.
extern "C++" {
namespace {
constexpr long long RSC_MAX_TRIALS_TOTAL = 1ll << 26;  // (pair, trial) lanes of one call: 216 B of models each

int rsc_check_xy(const double* xy, int64_t n) {
    for (int64_t i = 0; i < 4 * n; ++i)
        if (!std::isfinite(xy[i])) return fail(SATBA_E_ARG, "match %lld has a non-finite coordinate", (long long)(i / 4));
    return 0;
}
}  // namespace
}  // extern "C++"

int satba_ransac_fundamental(int32_t n_pairs, const int64_t* pair_ofs, const double* xy, double max_err, int32_t n_trials, uint64_t seed,
                             uint8_t* inlier, double* F, int32_t* best, int32_t device, float* kernel_ms) {
    if (kernel_ms) *kernel_ms = 0.f;
    if (n_pairs < 0) return fail(SATBA_E_ARG, "negative pair count");
    if (!(max_err > 0.0) || !std::isfinite(max_err)) return fail(SATBA_E_ARG, "max_err must be positive and finite");
    if (n_trials < 1 || n_trials > 65536) return fail(SATBA_E_ARG, "n_trials must lie in 1..65536, got %d", n_trials);
    if (n_pairs == 0) return 0;
    if (!pair_ofs) return fail(SATBA_E_ARG, "null pair_ofs");
    if (pair_ofs[0] != 0) return fail(SATBA_E_ARG, "pair_ofs must start at 0");
    for (int p = 0; p < n_pairs; ++p)
        if (pair_ofs[p + 1] < pair_ofs[p]) return fail(SATBA_E_ARG, "pair_ofs decreases at pair %d", p);
    const int64_t n = pair_ofs[n_pairs];
    if (n >= (int64_t)1 << 31) return fail(SATBA_E_ARG, "more than 2^31 matches in one call");
    if (n && (!xy || !inlier)) return fail(SATBA_E_ARG, "null xy or inlier");
    if ((long long)n_pairs * n_trials > RSC_MAX_TRIALS_TOTAL)
        return fail(SATBA_E_ARG, "n_pairs * n_trials = %lld exceeds %lld: split the call", (long long)n_pairs * n_trials, RSC_MAX_TRIALS_TOTAL);
    TRY(rsc_check_xy(xy, n));
    const size_t np = (size_t)n_pairs;
    std::vector<double> T(np * 6, 0.0);
    std::vector<unsigned char> live(np, 0);
    std::vector<int> order;  // live pairs, the largest first: their items take longest
    int max_m = 0;
    for (size_t p = 0; p < np; ++p) {
        const int64_t m = pair_ofs[p + 1] - pair_ofs[p];
        if (m < RSC_MIN_MATCHES || !rsc_normalise(xy + 4 * pair_ofs[p], m, T.data() + 6 * p)) continue;
        live[p] = 1;
        order.push_back((int)p);
        max_m = std::max(max_m, (int)m);
    }
    if (order.empty()) {  // nothing for the device to do: every match is kept
        if (n) memset(inlier, 1, (size_t)n);
        for (size_t p = 0; p < np; ++p) {
            if (F) std::fill(F + 9 * p, F + 9 * p + 9, 0.0);
            if (best) { best[3 * p] = -1; best[3 * p + 1] = (int32_t)(pair_ofs[p + 1] - pair_ofs[p]); best[3 * p + 2] = 0; }
        }
        return 0;
    }
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return pair_ofs[x + 1] - pair_ofs[x] > pair_ofs[y + 1] - pair_ofs[y]; });
    std::vector<int2> items;
    for (int p : order)
        for (int t0 = 0; t0 < n_trials; t0 += RSC_ITEM_TRIALS) items.push_back(make_int2(p, t0));

    DevRun s;
    TRY(s.begin(device));
    RansacArgs a{};
    a.n_pairs = n_pairs; a.n_trials = n_trials; a.seed = seed; a.thr2 = max_err * max_err;
    a.tile = std::min(max_m, RSC_TILE);
    const size_t lanes = np * (size_t)n_trials;
    double *d_xy, *d_T;
    long long* d_ofs;
    unsigned char* d_live;
    int2* d_items;
    static_assert(sizeof(long long) == sizeof(int64_t), "pair_ofs is uploaded as it is");
    TRY(s.upload(&d_xy, xy, (size_t)n * 4)); TRY(s.upload(&d_ofs, (const long long*)pair_ofs, np + 1)); TRY(s.upload(&d_T, T.data(), T.size()));
    TRY(s.upload(&d_live, live.data(), np)); TRY(s.upload(&d_items, items.data(), items.size()));
    TRY(s.alloc(&a.models, lanes * 27)); TRY(s.alloc(&a.nmod, lanes)); TRY(s.alloc(&a.cnt, lanes * 3)); TRY(s.alloc(&a.sum, lanes * 3));
    TRY(s.alloc(&a.inlier, (size_t)n)); TRY(s.alloc(&a.F, np * 9)); TRY(s.alloc(&a.best, np * 3));
    a.xy = d_xy; a.ofs = d_ofs; a.T = d_T; a.live = d_live; a.items = d_items;
    const size_t lds = sizeof(double) * 4 * (size_t)a.tile;
    HIP_TRY(hipFuncSetAttribute((const void*)k_ransac_score, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * 4 * RSC_TILE)));
    HIP_TRY(hipMemsetAsync(a.cnt, 0xff, sizeof(int) * lanes * 3, s.stream));  // -1: the slots of pairs without items
    HIP_TRY(hipEventRecord(s.e0, s.stream));
    hipLaunchKernelGGL(k_ransac_models, dim3((unsigned)((lanes + RSC_MODEL_THREADS - 1) / RSC_MODEL_THREADS)), dim3(RSC_MODEL_THREADS), 0, s.stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_ransac_score, dim3((unsigned)items.size()), dim3(RSC_SCORE_THREADS), lds, s.stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_ransac_pick, dim3(n_pairs), dim3(RSC_PICK_THREADS), 0, s.stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s.e1, s.stream));
    std::vector<double> hF(np * 9);
    std::vector<int32_t> hb(np * 3);
    if (n) HIP_TRY(hipMemcpyAsync(inlier, a.inlier, (size_t)n, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipMemcpyAsync(hF.data(), a.F, sizeof(double) * hF.size(), hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipMemcpyAsync(hb.data(), a.best, sizeof(int32_t) * hb.size(), hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s.e0, s.e1));
    if (F) memcpy(F, hF.data(), sizeof(double) * hF.size());
    if (best) memcpy(best, hb.data(), sizeof(int32_t) * hb.size());
    if (kernel_ms) *kernel_ms = ms;
    return 0;
}

int satba_ransac_models(int64_t m, const double* xy, int32_t n_samples, const int32_t* idx, int32_t* n_models, double* F, int32_t device) {
    if (m < 0 || n_samples < 0) return fail(SATBA_E_ARG, "negative count");
    if (n_samples == 0) return 0;
    if (!xy || !idx || !n_models || !F) return fail(SATBA_E_ARG, "null argument");
    if (m >= (int64_t)1 << 29) return fail(SATBA_E_ARG, "too many matches");
    for (int64_t i = 0; i < 7 * (int64_t)n_samples; ++i)
        if (idx[i] < 0 || idx[i] >= m) return fail(SATBA_E_ARG, "sample %lld names match %d outside 0..%lld", (long long)(i / 7), idx[i], (long long)m - 1);
    TRY(rsc_check_xy(xy, m));
    double T[6];
    std::fill(F, F + (size_t)n_samples * 27, 0.0);
    if (!rsc_normalise(xy, m, T)) {  // no normalisation, no model
        std::fill(n_models, n_models + n_samples, 0);
        return 0;
    }
    DevRun s;
    TRY(s.begin(device));
    double *d_xy, *d_T, *d_models;
    int *d_idx, *d_nmod;
    TRY(s.upload(&d_xy, xy, (size_t)m * 4)); TRY(s.upload(&d_T, (const double*)T, (size_t)6)); TRY(s.upload(&d_idx, idx, (size_t)n_samples * 7));
    TRY(s.alloc(&d_models, (size_t)n_samples * 27)); TRY(s.alloc(&d_nmod, (size_t)n_samples));
    HIP_TRY(hipMemsetAsync(d_models, 0, sizeof(double) * (size_t)n_samples * 27, s.stream));
    hipLaunchKernelGGL(k_ransac_models_idx, dim3((n_samples + RSC_MODEL_THREADS - 1) / RSC_MODEL_THREADS), dim3(RSC_MODEL_THREADS), 0, s.stream,
                       d_xy, d_T, d_idx, n_samples, d_models, d_nmod);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(F, d_models, sizeof(double) * (size_t)n_samples * 27, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipMemcpyAsync(n_models, d_nmod, sizeof(int32_t) * (size_t)n_samples, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    return 0;
}

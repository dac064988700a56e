// satba_sift_detect / satba_sift_fetch / satba_sift_fetch_plane / satba_sift_destroy (include/satba.h): part of the extern "C" block of
// satba_capi.hip.  Stand-alone entry points (no problem handle): detection runs before anything else exists.  Kernels: satba_sift.h.
struct satba_sift {
    int device = 0;
    int64_t n_rows = 0;
    float* rows = nullptr;    // n_rows x 132, on the device
    float* planes = nullptr;  // every Gaussian plane, when keep_planes
    SiftGeom geom;
    std::vector<size_t> oct_ofs;
    DevAllocs mem;  // owns rows and planes
};

extern "C++" {
namespace {
void sf_free(satba_sift* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

int sf_blur(hipStream_t st, const float* in, float* tmp, float* out, int w, int h, float sigma) {
    SiftTaps taps;
    taps.radius = sift_taps(sigma, taps.ker);
    if (taps.radius < 0) return fail(SATBA_E_ARG, "a blur of sigma %g needs more than %d taps", (double)sigma, SIFT_MAX_RADIUS);
    const dim3 gc((unsigned)((h + SIFT_BLUR_TH - 1) / SIFT_BLUR_TH), (unsigned)((w + SIFT_BLUR_TW - 1) / SIFT_BLUR_TW));
    hipLaunchKernelGGL(k_sift_blur_cols, gc, dim3(SIFT_BLUR_TW * SIFT_BLUR_ROWS_PER_PASS), 0, st, in, tmp, w, h, taps);
    const dim3 gr((unsigned)h, (unsigned)((w + SIFT_BLUR_LINE - 1) / SIFT_BLUR_LINE));
    hipLaunchKernelGGL(k_sift_blur_rows, gr, dim3(SIFT_BLUR_LINE), 0, st, (const float*)tmp, out, w, h, taps);
    HIP_TRY(hipGetLastError());
    return 0;
}

int sf_run(satba_sift* S, const float* image, int32_t width, int32_t height, int64_t row_stride, int32_t keep_planes, int64_t* counts, int32_t device,
           float* kernel_ms) {
    const SiftGeom& G = S->geom;
    const int n_oct = G.n_oct, n_planes = G.n_planes;
    S->oct_ofs.assign((size_t)n_oct + 1, 0);
    for (int o = 0; o < n_oct; ++o) S->oct_ofs[(size_t)o + 1] = S->oct_ofs[(size_t)o] + (size_t)n_planes * (size_t)G.w[o] * (size_t)G.h[o];
    const size_t n_plane0 = (size_t)G.w[0] * (size_t)G.h[0];

    DevRun s;
    TRY(s.begin(device));
    S->device = device;
    float *d_img, *d_tmp;
    unsigned* d_cnt;  // [0] max |pixel| bits, [1] candidates, [2] survivors of the interpolation, [3] survivors of the border test
    double* d_scale;
    float* d_planes;  // the handle's when it keeps them, of this run otherwise
    TRY((keep_planes ? S->mem : s).alloc(&d_planes, S->oct_ofs[(size_t)n_oct]));
    if (keep_planes) S->planes = d_planes;
    TRY(s.alloc(&d_img, (size_t)width * (size_t)height));
    HIP_TRY(hipMemcpy2DAsync(d_img, sizeof(float) * (size_t)width, image, sizeof(float) * (size_t)row_stride, sizeof(float) * (size_t)width, (size_t)height,
                             hipMemcpyHostToDevice, s.stream));
    TRY(s.alloc(&d_tmp, n_plane0));
    TRY(s.alloc(&d_cnt, 4));
    TRY(s.alloc(&d_scale, 1));
    HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(unsigned) * 4, s.stream));

    SiftPlanes P;
    memset(&P, 0, sizeof P);
    P.n_oct = n_oct; P.n_planes = n_planes; P.img_w = width; P.img_h = height;
    P.thr = G.thr;
    P.sigma_ratio = G.sigma[0][1] / G.sigma[0][0];
    for (int o = 0; o < n_oct; ++o) {
        P.base[o] = d_planes + S->oct_ofs[(size_t)o];
        P.w[o] = G.w[o]; P.h[o] = G.h[o]; P.delta[o] = G.delta[o];
        for (int k = 0; k < n_planes; ++k) P.sigma[o][k] = G.sigma[o][k];
    }

    HIP_TRY(hipEventRecord(s.e0, s.stream));
    hipLaunchKernelGGL(k_sift_seed, dim3((unsigned)((n_plane0 + 255) / 256)), dim3(256), 0, s.stream, (const float*)d_img, (long long)width, (int)width,
                       (int)height, d_tmp, G.w[0], G.h[0], d_cnt);
    HIP_TRY(hipGetLastError());
    unsigned max_bits = 0;
    HIP_TRY(hipMemcpyAsync(&max_bits, d_cnt, sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    counts[1] = n_oct;
    if (max_bits >= 0x7f800000u) {
        counts[5] = 1;
        return fail(SATBA_E_NONFINITE, "the image holds a non-finite pixel");
    }
    {   // fixed point of the histogram sums: a vote stays below 2^(e + 2) and a histogram has fewer than 2^14 of them
        float a;
        memcpy(&a, &max_bits, sizeof a);
        const int e = a > 0.0f ? std::ilogb(a) + 1 : 0;
        const double scale = std::ldexp(1.0, 46 - e);
        HIP_TRY(hipMemcpyAsync(d_scale, &scale, sizeof scale, hipMemcpyHostToDevice, s.stream));
    }

    // the Gaussian planes: the seed is in d_tmp; a blur reads `in`, writes its column pass to d_col and the result to `out`
    float* d_col;
    TRY(s.alloc(&d_col, n_plane0));
    for (int o = 0; o < n_oct; ++o) {
        const int w = G.w[o], h = G.h[o];
        const size_t plane = (size_t)w * (size_t)h;
        float* base = P.base[o];
        if (o == 0) {
            TRY(sf_blur(s.stream, d_tmp, d_col, base, w, h, G.inc[0][0]));
        } else {
            hipLaunchKernelGGL(k_sift_subsample, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, s.stream,
                               (const float*)(P.base[o - 1] + (size_t)(n_planes - 3) * (size_t)G.w[o - 1] * (size_t)G.h[o - 1]), G.w[o - 1], base, w, h);
            HIP_TRY(hipGetLastError());
        }
        for (int k = 1; k < n_planes; ++k) TRY(sf_blur(s.stream, base + (size_t)(k - 1) * plane, d_col, base + (size_t)k * plane, w, h, G.inc[o][k]));
    }

    // discrete extrema: one pass when the guess holds them, a second with room for all when it does not
    const float thr08 = 0.8f * G.thr;
    size_t cap = n_plane0 / 16 + 4096;
    unsigned n_cand = 0;
    unsigned long long *d_keys = nullptr, *d_sorted = nullptr;
    for (int pass = 0; pass < 2; ++pass) {
        TRY(s.alloc(&d_keys, cap));
        HIP_TRY(hipMemsetAsync(d_cnt + 1, 0, sizeof(unsigned), s.stream));
        for (int o = 0; o < n_oct; ++o) {
            const long long n_in = (long long)(G.w[o] - 2) * (long long)(G.h[o] - 2);
            if (n_in <= 0) continue;
            hipLaunchKernelGGL(k_sift_extrema, dim3((unsigned)((n_in + 255) / 256), (unsigned)(n_planes - 3)), dim3(256), 0, s.stream, (const float*)P.base[o],
                               G.w[o], G.h[o], o, thr08, d_keys, (unsigned)std::min<size_t>(cap, 0xffffffffu), d_cnt + 1);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&n_cand, d_cnt + 1, sizeof(unsigned), hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipStreamSynchronize(s.stream));
        if ((size_t)n_cand <= cap) break;
        if (pass == 1) return fail(SATBA_E_STATE, "the count of discrete extrema changed between two passes");
        cap = n_cand;
    }
    if (n_cand >= 1u << 31) return fail(SATBA_E_ARG, "fewer than 2^31 discrete extrema are supported (%u)", n_cand);
    counts[2] = n_cand;
    const int n = (int)n_cand;
    int total = 0;
    if (n) {
        // the reference's list order: (octave, scale, row, column) is the key itself
        TRY(s.alloc(&d_sorted, (size_t)n));
        size_t tmp_sort = 0, tmp_scan = 0;
        int *d_nori, *d_ofs;
        float* d_theta;
        SiftKey* d_cand;
        char* d_work;
        TRY(s.alloc(&d_nori, (size_t)n + 1)); TRY(s.alloc(&d_ofs, (size_t)n + 1));
        TRY(s.alloc(&d_theta, (size_t)n * SIFT_MAX_ORI)); TRY(s.alloc(&d_cand, (size_t)n));
        HIP_TRY(rocprim::radix_sort_keys(nullptr, tmp_sort, d_keys, d_sorted, (size_t)n, 0, 64, s.stream));
        HIP_TRY(rocprim::exclusive_scan(nullptr, tmp_scan, d_nori, d_ofs, 0, (size_t)n + 1, rocprim::plus<int>(), s.stream));
        TRY(s.alloc(&d_work, std::max(tmp_sort, tmp_scan) + 16));
        HIP_TRY(rocprim::radix_sort_keys(d_work, tmp_sort, d_keys, d_sorted, (size_t)n, 0, 64, s.stream));
        hipLaunchKernelGGL(k_sift_refine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s.stream, P, (const unsigned long long*)d_sorted, n, d_cand, d_cnt + 2);
        HIP_TRY(hipMemsetAsync(d_nori + n, 0, sizeof(int), s.stream));
        hipLaunchKernelGGL(k_sift_orient, dim3((unsigned)n), dim3(64), 0, s.stream, P, (const SiftKey*)d_cand, n, (const double*)d_scale, d_nori, d_theta);
        HIP_TRY(hipGetLastError());
        HIP_TRY(rocprim::exclusive_scan(d_work, tmp_scan, d_nori, d_ofs, 0, (size_t)n + 1, rocprim::plus<int>(), s.stream));
        unsigned stage[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(&total, d_ofs + n, sizeof(int), hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipMemcpyAsync(stage, d_cnt + 2, sizeof stage, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipStreamSynchronize(s.stream));
        counts[3] = stage[0];
        counts[4] = stage[1];
        TRY(S->mem.alloc(&S->rows, SIFT_ROW * (size_t)std::max(total, 1)));
        if (total) {
            hipLaunchKernelGGL(k_sift_describe, dim3((unsigned)n), dim3(64), 0, s.stream, P, (const SiftKey*)d_cand, n, (const double*)d_scale, (const int*)d_nori,
                               (const int*)d_ofs, (const float*)d_theta, S->rows);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipEventRecord(s.e1, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, s.e0, s.e1));
    S->n_rows = total;
    counts[0] = total;
    return 0;
}
}  // namespace
}  // extern "C++"

int satba_sift_detect(const float* image, int32_t width, int32_t height, int64_t row_stride, float thresh_dog, int32_t nb_octaves, int32_t nb_scales,
                      int32_t keep_planes, satba_sift** out, int64_t* counts, int32_t device, float* kernel_ms) {
    if (!out || !counts || !image) return fail(SATBA_E_ARG, "null argument");
    *out = nullptr;
    for (int k = 0; k < 6; ++k) counts[k] = 0;
    if (width < 12 || height < 12) return fail(SATBA_E_ARG, "the image must have at least 12 pixels a side, got %d x %d", width, height);
    if (width >= 1 << 26 || height >= 1 << 26) return fail(SATBA_E_ARG, "sides below 2^26 pixels are supported, got %d x %d", width, height);
    if (row_stride < width) return fail(SATBA_E_ARG, "row_stride %lld is shorter than the width %d", (long long)row_stride, width);
    if (nb_scales < 1 || nb_scales > SIFT_MAX_SCALES) return fail(SATBA_E_ARG, "nb_scales must be in [1, %d], got %d", SIFT_MAX_SCALES, nb_scales);
    if (nb_octaves < 1) return fail(SATBA_E_ARG, "nb_octaves must be positive, got %d", nb_octaves);
    if (!(thresh_dog >= 0.0f)) return fail(SATBA_E_ARG, "thresh_dog must not be negative, got %g", (double)thresh_dog);
    satba_sift* S = new (std::nothrow) satba_sift();
    if (!S) return fail(SATBA_E_ARG, "out of host memory");
    if (sift_geometry(width, height, nb_octaves, nb_scales, thresh_dog, &S->geom)) {
        delete S;
        return fail(SATBA_E_ARG, "no octave fits a %d x %d image", width, height);
    }
    const int rc = sf_run(S, image, width, height, row_stride, keep_planes, counts, device, kernel_ms);
    if (rc) {
        sf_free(S);
        return rc;
    }
    *out = S;
    return 0;
}

int satba_sift_fetch(satba_sift* s, float* keypoints) {
    if (!s) return fail(SATBA_E_ARG, "null handle");
    HIP_TRY(hipSetDevice(s->device));
    if (s->n_rows && !keypoints) return fail(SATBA_E_ARG, "null argument");
    if (s->n_rows) HIP_TRY(hipMemcpy(keypoints, s->rows, sizeof(float) * SIFT_ROW * (size_t)s->n_rows, hipMemcpyDeviceToHost));
    return 0;
}

int satba_sift_fetch_plane(satba_sift* s, int32_t octave, int32_t scale, float* plane, int32_t* w, int32_t* h) {
    if (!s) return fail(SATBA_E_ARG, "null handle");
    if (!s->planes) return fail(SATBA_E_STATE, "the planes were not kept (keep_planes = 0)");
    if (octave < 0 || octave >= s->geom.n_oct || scale < 0 || scale >= s->geom.n_planes)
        return fail(SATBA_E_ARG, "no plane (%d, %d): %d octaves of %d planes", octave, scale, s->geom.n_oct, s->geom.n_planes);
    if (w) *w = s->geom.w[octave];
    if (h) *h = s->geom.h[octave];
    if (plane) {
        HIP_TRY(hipSetDevice(s->device));
        const size_t n = (size_t)s->geom.w[octave] * (size_t)s->geom.h[octave];
        HIP_TRY(hipMemcpy(plane, s->planes + s->oct_ofs[(size_t)octave] + (size_t)scale * n, sizeof(float) * n, hipMemcpyDeviceToHost));
    }
    return 0;
}

void satba_sift_destroy(satba_sift* s) { sf_free(s); }

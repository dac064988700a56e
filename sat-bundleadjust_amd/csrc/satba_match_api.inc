// satba_match_pairs / satba_matches_fetch / satba_matches_destroy (include/satba.h): part of the extern "C" block of satba_capi.hip.
// Stand-alone entry points (no problem handle): matching runs before anything else exists.  Kernels: satba_match.h.
struct satba_matches {
    int device = 0;
    int32_t n_pairs = 0;
    int64_t n_matches = 0;
    std::vector<int64_t> pair_ofs;
    int *kp_i = nullptr, *kp_j = nullptr;
    DevAllocs mem;  // owns the arrays
};

extern "C++" {
namespace {
void mt_free(satba_matches* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    delete m;
}

// the argument checks on images, pairs and boxes that every match entry makes
int mt_check_pairs(int32_t n_cam, const int64_t* n_kp, const float* const* features, const double* const* utm, int32_t n_pairs, const int32_t* pairs,
                   const double* boxes) {
    for (int32_t c = 0; c < n_cam; ++c)
        if (n_kp[c] < 0 || n_kp[c] >= (int64_t)1 << 31) return fail(SATBA_E_ARG, "image %d: keypoint count %lld outside [0, 2^31)", c, (long long)n_kp[c]);
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int32_t i = pairs[2 * p], j = pairs[2 * p + 1];
        if (i < 0 || i >= n_cam || j < 0 || j >= n_cam) return fail(SATBA_E_ARG, "pair %d names an image outside 0..%d", p, n_cam - 1);
        if (i == j) return fail(SATBA_E_ARG, "pair %d matches image %d with itself", p, i);
        for (int k = 0; k < 4; ++k)
            if (boxes[4 * p + k] != boxes[4 * p + k]) return fail(SATBA_E_ARG, "pair %d: the box holds a NaN", p);
        for (int s = 0; s < 2; ++s)
            if (n_kp[pairs[2 * p + s]] && (!features[pairs[2 * p + s]] || !utm[pairs[2 * p + s]]))
                return fail(SATBA_E_ARG, "pair %d: image %d has keypoints but no arrays", p, pairs[2 * p + s]);
    }
    return 0;
}

// rectifying similarities (a, b, q) of the two images from the five coefficients F[0,2], F[1,2], F[2,0], F[2,1], F[2,2] of an affine
// fundamental matrix (Hartley & Zisserman p. 345: c, d, a, b, e), in double, rounded once (ref:3rdparty/sift/simd/linalg.c:108-138)
void mt_similarities(const double* f, float s1[3], float s2[3]) {
    const double c = f[0], d = f[1], a = f[2], b = f[3], e = f[4];
    const double r = std::sqrt(a * a + b * b), s = std::sqrt(c * c + d * d);
    const double z = std::sqrt(r / s), t = 0.5 * e / std::sqrt(r * s), zz = 1 / z;
    s1[0] = (float)(z * b / r); s1[1] = (float)(z * a / r); s1[2] = (float)t;
    s2[0] = (float)(zz * -d / s); s2[1] = (float)(zz * -c / s); s2[2] = (float)-t;
}

// What a match entry holds once its images are uploaded, packed and selected (mt_front), and what the scan-and-emit tail (mt_emit)
// reads.  satba_match_pairs and satba_match_window (satba_window_api.inc) share both; the nearest-neighbour search between them is
// each entry's own and leaves hit / kpj per first-side slot.
struct MtFront {
    std::vector<MatchPair> hp;   // as the device holds them after k_match_select (n[] filled)
    long long n_rows = 0, n_slots = 0;
    bool float_path = false;
    float* d_feat = nullptr; double2* d_utm = nullptr; signed char* d_rec = nullptr;
    int *d_nrm = nullptr, *d_sel = nullptr, *d_nrm_s = nullptr, *d_slot_pair = nullptr, *d_hit = nullptr, *d_pos = nullptr, *d_kpj = nullptr;
    float* d_xx_s = nullptr; MatchPair* d_pairs = nullptr;
    char* d_tmp = nullptr; size_t tmp_scan = 0;  // rocprim's scratch of the scan over the slots
};

// Row space, slot space, uploads, k_match_pack and k_match_select; records s.e0 in front of the pack kernel and returns after the
// read of the selection counts.  F5 may be NULL (no gate: xx_s is zero).
int mt_front(DevRun& s, satba_matches* m, MtFront& f, int32_t n_cam, const int64_t* n_kp, const float* const* features, const double* const* utm,
             int32_t n_pairs, const int32_t* pairs, const double* boxes, const double* F5, int32_t device) {
    const char* env_float = getenv("SATBA_MATCH_FLOAT");  // test switch, read at call time (INTEGRATION.md section 3)
    const bool force_float = env_float && atoi(env_float) != 0;
    const int gate = F5 ? 1 : 0;

    // images named by a pair are uploaded once; rows of all of them in one row space
    std::vector<char> used((size_t)n_cam, 0);
    for (int32_t p = 0; p < n_pairs; ++p) { used[(size_t)pairs[2 * p]] = 1; used[(size_t)pairs[2 * p + 1]] = 1; }
    std::vector<long long> row0((size_t)n_cam + 1, 0);
    for (int32_t c = 0; c < n_cam; ++c) row0[(size_t)c + 1] = row0[(size_t)c] + (used[(size_t)c] ? n_kp[c] : 0);
    const long long n_rows = row0[(size_t)n_cam];
    if (n_rows >= (1ll << 31)) return fail(SATBA_E_ARG, "fewer than 2^31 keypoints over the matched images are supported (%lld)", n_rows);

    // slots: [pair][side], each side rounded up to a tile
    std::vector<MatchPair>& hp = f.hp;
    hp.resize((size_t)n_pairs);
    long long n_slots = 0;
    for (int32_t p = 0; p < n_pairs; ++p) {
        MatchPair& P = hp[(size_t)p];
        memset(&P, 0, sizeof P);
        for (int side = 0; side < 2; ++side) {
            const int32_t im = pairs[2 * p + side];
            P.cnt[side] = (int)n_kp[im];
            P.base[side] = (int)row0[(size_t)im];
            P.cap[side] = (P.cnt[side] + MT_TILE - 1) / MT_TILE * MT_TILE;
            if (n_slots + P.cap[side] >= (1ll << 31)) return fail(SATBA_E_ARG, "the keypoints of all pairs' sides exceed 2^31");
            P.ofs[side] = (int)n_slots;
            n_slots += P.cap[side];
        }
        for (int k = 0; k < 4; ++k) P.box[k] = boxes[4 * p + k];
        if (gate) mt_similarities(F5 + 5 * p, P.s[0], P.s[1]);
    }
    std::vector<int> slot_pair((size_t)(n_slots / MT_TILE) + 1, -1);
    for (int32_t p = 0; p < n_pairs; ++p)
        for (int t = 0; t < hp[(size_t)p].cap[0] / MT_TILE; ++t) slot_pair[(size_t)(hp[(size_t)p].ofs[0] / MT_TILE + t)] = p;
    f.n_rows = n_rows;
    f.n_slots = n_slots;

    TRY(s.begin(device));
    m->device = device;
    m->n_pairs = n_pairs;
    m->pair_ofs.assign((size_t)n_pairs + 1, 0);
    int* d_flag; float2* d_xy;
    TRY(s.alloc(&f.d_feat, (size_t)n_rows * MT_ROW)); TRY(s.alloc(&f.d_utm, (size_t)n_rows));
    for (int32_t c = 0; c < n_cam; ++c) {
        if (!used[(size_t)c] || !n_kp[c]) continue;
        HIP_TRY(hipMemcpyAsync(f.d_feat + row0[(size_t)c] * MT_ROW, features[c], sizeof(float) * MT_ROW * (size_t)n_kp[c], hipMemcpyHostToDevice, s.stream));
        HIP_TRY(hipMemcpyAsync(f.d_utm + row0[(size_t)c], utm[c], sizeof(double2) * (size_t)n_kp[c], hipMemcpyHostToDevice, s.stream));
    }
    TRY(s.alloc(&f.d_rec, (size_t)n_rows * MT_DESC)); TRY(s.alloc(&f.d_nrm, (size_t)n_rows));
    TRY(s.alloc(&d_xy, (size_t)n_rows)); TRY(s.alloc(&d_flag, 1));
    TRY(s.alloc(&f.d_sel, (size_t)n_slots)); TRY(s.alloc(&f.d_nrm_s, (size_t)n_slots));
    TRY(s.alloc(&f.d_xx_s, (size_t)n_slots)); TRY(s.upload(&f.d_pairs, hp.data(), hp.size()));
    TRY(s.upload(&f.d_slot_pair, slot_pair.data(), slot_pair.size()));
    TRY(s.alloc(&f.d_hit, (size_t)n_slots + 1)); TRY(s.alloc(&f.d_pos, (size_t)n_slots + 1));
    TRY(s.alloc(&f.d_kpj, (size_t)n_slots + 1));
    HIP_TRY(hipMemsetAsync(d_flag, 0, sizeof(int), s.stream));
    if (n_slots) {  // slots past a side's selection are read (and masked) by the match kernels
        HIP_TRY(hipMemsetAsync(f.d_sel, 0, sizeof(int) * (size_t)n_slots, s.stream));
        HIP_TRY(hipMemsetAsync(f.d_nrm_s, 0, sizeof(int) * (size_t)n_slots, s.stream));
        HIP_TRY(hipMemsetAsync(f.d_xx_s, 0, sizeof(float) * (size_t)n_slots, s.stream));
    }
    HIP_TRY(hipMemsetAsync(f.d_hit, 0, sizeof(int) * ((size_t)n_slots + 1), s.stream));

    HIP_TRY(hipEventRecord(s.e0, s.stream));
    if (n_rows) hipLaunchKernelGGL(k_match_pack, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, s.stream, n_rows, f.d_feat, f.d_rec, f.d_nrm, d_xy, d_flag);
    if (n_pairs) hipLaunchKernelGGL(k_match_select, dim3(2u * (unsigned)n_pairs), dim3(MT_SEL_THREADS), 0, s.stream, f.d_pairs, f.d_utm, d_xy, f.d_nrm, f.d_sel, f.d_nrm_s, f.d_xx_s, gate);
    HIP_TRY(hipGetLastError());
    int flag = 0;
    HIP_TRY(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, s.stream));
    if (n_pairs) HIP_TRY(hipMemcpyAsync(hp.data(), f.d_pairs, sizeof(MatchPair) * hp.size(), hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    f.float_path = flag != 0 || force_float;
    return 0;
}

// rocprim's scratch for the scan of mt_emit, allocated before the entry's own kernels are queued
int mt_scan_scratch(DevRun& s, MtFront& f) {
    HIP_TRY(rocprim::exclusive_scan(nullptr, f.tmp_scan, f.d_hit, f.d_pos, 0, (size_t)f.n_slots + 1, rocprim::plus<int>(), s.stream));
    TRY(s.alloc(&f.d_tmp, f.tmp_scan + 16));
    return 0;
}

// hit / kpj per first-side slot -> the handle's arrays in slot order, pair_ofs, counts[0] and counts[3]; records s.e1 behind the
// last kernel and reads kernel_ms
int mt_emit(DevRun& s, satba_matches* m, MtFront& f, int64_t* counts, float* kernel_ms) {
    const int32_t n_pairs = m->n_pairs;
    const long long n_slots = f.n_slots;
    int total = 0;
    std::vector<int> h_pos((size_t)n_pairs);
    if (n_slots) {
        const dim3 grid((unsigned)((n_slots + 255) / 256)), blk(256);
        HIP_TRY(rocprim::exclusive_scan(f.d_tmp, f.tmp_scan, f.d_hit, f.d_pos, 0, (size_t)n_slots + 1, rocprim::plus<int>(), s.stream));
        HIP_TRY(hipMemcpyAsync(&total, f.d_pos + n_slots, sizeof(int), hipMemcpyDeviceToHost, s.stream));
        for (int32_t p = 0; p < n_pairs; ++p)
            HIP_TRY(hipMemcpyAsync(&h_pos[(size_t)p], f.d_pos + f.hp[(size_t)p].ofs[0], sizeof(int), hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipStreamSynchronize(s.stream));
        TRY(m->mem.alloc(&m->kp_i, (size_t)std::max(total, 1)));
        TRY(m->mem.alloc(&m->kp_j, (size_t)std::max(total, 1)));
        if (total) {
            hipLaunchKernelGGL(k_match_emit, grid, blk, 0, s.stream, n_slots, f.d_pairs, f.d_slot_pair, f.d_sel, f.d_hit, f.d_pos, f.d_kpj, m->kp_i, m->kp_j);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipEventRecord(s.e1, s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, s.e0, s.e1));
    for (int32_t p = 0; p < n_pairs; ++p) m->pair_ofs[(size_t)p] = h_pos[(size_t)p];
    m->pair_ofs[(size_t)n_pairs] = total;
    m->n_matches = total;
    counts[0] = total;
    counts[3] = f.float_path ? 1 : 0;
    return 0;
}

int mt_run(satba_matches* m, int32_t n_cam, const int64_t* n_kp, const float* const* features, const double* const* utm, int32_t n_pairs,
           const int32_t* pairs, const double* boxes, const double* F5, float thr, float epi_thr, int32_t relative, int64_t* counts, int32_t device,
           float* kernel_ms) {
    const char* env_chunk = getenv("SATBA_MATCH_CHUNK");  // test switch, read at call time (INTEGRATION.md section 3)
    int chunk = 4096;
    if (env_chunk && *env_chunk) {
        chunk = atoi(env_chunk);
        if (chunk <= 0 || chunk % MT_TILE) return fail(SATBA_E_ARG, "SATBA_MATCH_CHUNK must be a positive multiple of %d, got '%s'", MT_TILE, env_chunk);
    }
    const int gate = F5 ? 1 : 0;
    const float thr2 = thr * thr;  // float32, as the reference squares it

    DevRun s;
    MtFront f;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    TRY(mt_front(s, m, f, n_cam, n_kp, features, utm, n_pairs, pairs, boxes, F5, device));
    std::vector<MatchPair>& hp = f.hp;
    const long long n_slots = f.n_slots;

    // work items: (pair, MT_WQ queries, chunk of candidates), in the pairs' order
    std::vector<MatchItem> items;
    long long n_part = 0;
    for (int32_t p = 0; p < n_pairs; ++p) {
        MatchPair& P = hp[(size_t)p];
        counts[1] += P.n[0] + P.n[1];
        P.part_ofs = n_part;
        P.n_chunks = 0;
        if (!P.n[0] || !P.n[1]) { ++counts[2]; continue; }
        P.n_chunks = (P.n[1] + chunk - 1) / chunk;
        n_part += (long long)P.n_chunks * P.cap[0];
        for (int q0 = 0; q0 < P.n[0]; q0 += MT_WQ)
            for (int c = 0; c < P.n_chunks; ++c) items.push_back(MatchItem{p, q0, c * chunk, c});
    }
    if (items.size() >= (size_t)1 << 31) return fail(SATBA_E_ARG, "too many work items: raise SATBA_MATCH_CHUNK");
    const int n_items = (int)items.size();
    MatchItem* d_items; MatchPart* d_part;
    TRY(s.upload(&d_items, items.data(), items.size())); TRY(s.alloc(&d_part, (size_t)n_part));
    if (n_pairs) HIP_TRY(hipMemcpyAsync(f.d_pairs, hp.data(), sizeof(MatchPair) * hp.size(), hipMemcpyHostToDevice, s.stream));
    TRY(mt_scan_scratch(s, f));
    if (n_items) {
        if (f.float_path) {
            if (gate) hipLaunchKernelGGL(k_match_f32<true>, dim3((unsigned)n_items), dim3(MT_WQ), 0, s.stream, n_items, d_items, f.d_pairs, f.d_feat, f.d_sel, f.d_xx_s, chunk, epi_thr, d_part);
            else hipLaunchKernelGGL(k_match_f32<false>, dim3((unsigned)n_items), dim3(MT_WQ), 0, s.stream, n_items, d_items, f.d_pairs, f.d_feat, f.d_sel, f.d_xx_s, chunk, epi_thr, d_part);
        } else {
            const dim3 grid((unsigned)((n_items + MT_WAVES - 1) / MT_WAVES)), blk(64 * MT_WAVES);
            if (gate) hipLaunchKernelGGL(k_match_i8<true>, grid, blk, 0, s.stream, n_items, d_items, f.d_pairs, f.d_rec, f.d_sel, f.d_nrm_s, f.d_xx_s, chunk, epi_thr, d_part);
            else hipLaunchKernelGGL(k_match_i8<false>, grid, blk, 0, s.stream, n_items, d_items, f.d_pairs, f.d_rec, f.d_sel, f.d_nrm_s, f.d_xx_s, chunk, epi_thr, d_part);
        }
        HIP_TRY(hipGetLastError());
    }
    if (n_slots) {
        hipLaunchKernelGGL(k_match_finish, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, s.stream, (int)n_pairs, f.d_pairs, f.d_slot_pair, n_slots, f.d_sel, d_part, thr2, (int)relative, f.d_hit, f.d_kpj);
        HIP_TRY(hipGetLastError());
    }
    return mt_emit(s, m, f, counts, kernel_ms);
}
}  // namespace
}  // extern "C++"

int satba_match_pairs(int32_t n_cam, const int64_t* n_kp, const float* const* features, const double* const* utm, int32_t n_pairs, const int32_t* pairs,
                      const double* boxes, const double* F5, float thr, float epi_thr, int32_t relative, satba_matches** out, int64_t* counts,
                      int32_t device, float* kernel_ms) {
    if (!out || !counts || !n_kp || !features || !utm || n_cam <= 0 || n_pairs < 0) return fail(SATBA_E_ARG, "null or negative argument");
    *out = nullptr;
    if (n_pairs && (!pairs || !boxes)) return fail(SATBA_E_ARG, "null pairs or boxes");
    if (!(thr > 0.0f)) return fail(SATBA_E_ARG, "thr must be positive, got %g", (double)thr);
    if (F5 && !(epi_thr > 0.0f)) return fail(SATBA_E_ARG, "epi_thr must be positive, got %g", (double)epi_thr);
    TRY(mt_check_pairs(n_cam, n_kp, features, utm, n_pairs, pairs, boxes));
    if (F5)
        for (int32_t p = 0; p < n_pairs; ++p)
            for (int k = 0; k < 5; ++k)
                if (!std::isfinite(F5[5 * p + k])) return fail(SATBA_E_ARG, "pair %d: the fundamental matrix is not finite", p);
    satba_matches* m = new (std::nothrow) satba_matches();
    if (!m) return fail(SATBA_E_ARG, "out of host memory");
    const int rc = mt_run(m, n_cam, n_kp, features, utm, n_pairs, pairs, boxes, F5, thr, epi_thr, relative, counts, device, kernel_ms);
    if (rc) {
        mt_free(m);
        return rc;
    }
    *out = m;
    return 0;
}

int satba_matches_fetch(satba_matches* m, int64_t* pair_ofs, int32_t* kp_i, int32_t* kp_j) {
    if (!m) return fail(SATBA_E_ARG, "null handle");
    HIP_TRY(hipSetDevice(m->device));
    if (pair_ofs) std::copy(m->pair_ofs.begin(), m->pair_ofs.end(), pair_ofs);
    const size_t K = (size_t)m->n_matches;
    if (K && kp_i) HIP_TRY(hipMemcpy(kp_i, m->kp_i, sizeof(int) * K, hipMemcpyDeviceToHost));
    if (K && kp_j) HIP_TRY(hipMemcpy(kp_j, m->kp_j, sizeof(int) * K, hipMemcpyDeviceToHost));
    return 0;
}

void satba_matches_destroy(satba_matches* m) { mt_free(m); }

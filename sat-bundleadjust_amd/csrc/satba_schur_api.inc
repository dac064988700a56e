// satba_schur / satba_schur_auto / satba_solve_messages_* (include/satba.h) and the fronts the LM loops queue: part of the extern "C"
// block of satba_capi.hip -- the host side of the Schur phase: the item tables of k_schur_pairs, the route a front takes through the
// kernels of satba_schur.h (decided once: SchurRoute), their launches, and the factorisation beside the pair kernel or the all-reduce.
extern "C++" {
namespace {

// ---------------------------------------------------------------------------------------------------- Schur work items
// One item table of k_schur_pairs (order: satba_schur_items.h) on the device, with its flattened form (k_schur_item_desc).
// dg_weight: weighted table only (ensure_wlayout)
int schur_items_build(satba_problem* p, SchurTable kind, SchurItems* t, long long dg_weight) {
    const bool w = kind == SCHUR_ITEMS_WEIGHTED;
    const std::vector<SchurItemKey> table = schur_item_order(kind, p->M, p->L.C, w ? p->L.dg_spc : 0, dg_weight);
    t->n_blocks = (int)(table.size() / 4);
    TRY(dev_alloc(p, &t->items, table.size()));
    HIP_TRY(hipMemcpy(t->items, table.data(), sizeof(int2) * table.size(), hipMemcpyHostToDevice));
    TRY(dev_alloc(p, &t->desc, table.size()));
    hipLaunchKernelGGL(k_schur_item_desc, dim3((unsigned)((table.size() + 255) / 256)), dim3(256), 0, p->stream, (long long)table.size(), t->items,
                       p->L.pair_ij, p->L.pair_ofs, p->L.C, t->desc, w ? p->L.dg_ofs : (const int*)nullptr, w ? p->L.n_dg : 1);
    HIP_TRY(hipGetLastError());
    return 0;
}
// ... where the pairs alone fill the chip: with few cameras the chunks are what provides the parallelism (50 cameras: 1 225 pairs)
bool schur_merge_enough(const satba_problem* p) {
    const char* mg = getenv("SATBA_SCHUR_MERGE");
    return p->L.n_pairs >= 8192 || (mg && atoi(mg) != 0);
}
// the tables a handle has from its creation on (the weighted one comes with the merged records: ensure_wlayout)
int schur_item_tables(satba_problem* p) {
    TRY(schur_items_build(p, SCHUR_ITEMS_CHUNKED, &p->items_chunked, 0));
    const char* mg = getenv("SATBA_SCHUR_MERGE");  // experiments: 0 keeps the chunked items for every kernel
    if (p->L.C > 1 && schur_merge_enough(p) && !(mg && atoi(mg) == 0)) TRY(schur_items_build(p, SCHUR_ITEMS_MERGED, &p->items_merged, 0));
    return 0;
}

// ---------------------------------------------------------------------------------------------------- the route of a front
// Which kernels a Schur phase launches, on which item table, in which order: decided once per front (schur_route) and read by
// everything that queues or prepares a part of it.
struct SchurRoute {
    bool pairs_run, unit, weighted;  // a pair kernel runs | unit weights + linear loss | on the merged records W
    const SchurItems* items;         // the pair kernel's table
    int n_chunks, red_chunks;        // its chunks per pair (1: one item per pair, straight into S) | partials per pair that somebody adds up
    // diagonal blocks (with J_c^T J_c) and right-hand side: a camera-major pass of its own, k_schur_diag -- or, weighted / robust runs on the
    // merged records, items of the pair kernel in front of every (camera row, chunk) group, whose pair items then find the records in L2
    bool dg_in_pairs, cm_rec;  // cm_rec: k_schur_diag on the merged records -- piece offsets instead of point indices (cam_major)
    int dchunks, diag_xcd;     // partials per camera of either | k_schur_diag: chunks dealt to the XCDs
    bool both;                 // the factorisation BEHIND the Schur kernels (no arrival protocol): diagonal pass and pair kernel in one launch, k_schur_both
    // k_schur_finish -- diagonal blocks, right-hand side, header (and the pairs' chunk partials, finish_red_chunks > 1) in one launch -- runs
    // behind the pair kernel, or in front of it when the factorisation waits beside this stream (finish_dchunks 0: the diagonal blocks come out
    // of the pair kernel, too).  finish_direct: the pair kernel writes (has written) blocks of S itself; finish_scale: S is handed over scaled
    bool finish_first, finish_direct, finish_scale;
    int finish_dchunks, finish_red_chunks, nb_diag;
    bool beside_ok;      // the front: the factorisation may run beside the pair kernel ...
    int wgs, arr_extra;  // ... on that many workgroups (default), C3Args::arr_extra
    // ... and, unit weights, takes the diagonal blocks and the right-hand side of the cameras [c_split, M) from BEHIND the pair kernel
    // (satba_diag_split.h; M: nothing late) -- k_schur_diag and k_schur_finish in front keep the cameras [0, c_split).  In force on fronts
    // with the factorisation waiting (FrontCtx::arrive_epoch) only.  late_tail: the late part as trailing workgroups of the pair launch
    // (k_schur_pairs_diag_late) instead of a launch of its own (k_schur_diag_late)
    int c_split;
    bool late_tail;
};

SchurRoute schur_route(const satba_problem* p, const FrontCtx& f) {
    const bool arrive = f.arrive_epoch != 0;  // the factorisation waits beside this stream
    static const bool one_launch = !(getenv("SATBA_SCHUR_ONE_LAUNCH") && atoi(getenv("SATBA_SCHUR_ONE_LAUNCH")) == 0);
    SchurRoute r;
    r.pairs_run = pairs_run(p); r.unit = unit_run(p); r.weighted = merged_records(p);
    const bool merged = r.pairs_run && r.unit && p->items_merged.desc;
    r.items = merged ? &p->items_merged : (r.weighted ? &p->items_w : &p->items_chunked);
    r.n_chunks = merged ? 1 : p->L.C; r.red_chunks = (r.pairs_run && p->L.C > 1 && !merged) ? p->L.C : 1;
    r.dg_in_pairs = r.weighted && r.pairs_run;
    r.dchunks = r.dg_in_pairs ? p->L.n_dg : (r.weighted ? p->cm_chunks_w : p->cm_chunks);
    r.diag_xcd = (!r.dg_in_pairs && r.dchunks % 8 == 0 && !getenv("SATBA_NO_DIAG_XCD")) ? 1 : 0;
    r.cm_rec = r.weighted && !r.dg_in_pairs;
    r.both = one_launch && !arrive && !r.dg_in_pairs && r.pairs_run;
    r.finish_first = arrive; r.finish_direct = arrive || (r.pairs_run && r.red_chunks == 1);
    r.finish_dchunks = (arrive && r.dg_in_pairs) ? 0 : r.dchunks; r.finish_red_chunks = arrive ? 1 : r.red_chunks;
    r.nb_diag = (int)((std::max<long long>(8ll * p->M * cam_acc_len(p->NP), p->hdr) + 255) / 256);
    r.finish_scale = f.scale_in_finish &&!r.finish_direct && 1 + CH_MAX_STEPS <= r.nb_diag * 256;
    // beside the factorisation (front_schur_solve) -- unit weights: one item per pair (the table exists from 8 192 pairs on, or
    // SATBA_SCHUR_MERGE), no chunk partials; weighted / robust: the chunk items, the last one of a pair adds the partials (SchurArgs::pair_cnt),
    // and the diagonal items (SchurArgs::dg_cnt) -- affine and perspective cameras (the RPC kernel keeps its reduce pass)
    const char* env = getenv("SATBA_CHOL_BESIDE");  // (read at every front: the tests switch it inside one process)
    const bool items_ok = r.unit ? r.red_chunks == 1 : (schur_merge_enough(p) && p->model != RPC);
    r.beside_ok = !(env && atoi(env) == 0) && p->world == 1 && items_ok && r.pairs_run && p->n_c == p->M * p->NP && p->n_c > 128 && p->n_c <= 1024 &&
                  p->N > 0 && !p->beside_off;
    // workgroups (= CUs) lent to the factorisation, a multiple of the eight XCDs.  Measured at 200 cameras x 5 (round 5, LM it/s): beside the
    // unit-weight pair kernel (0.43 ms) 16: 777, 24: 819, 28: 820, 32: 841, 36: 793, 40: 788, 48: 783, 64: 802; beside the weighted one
    // (1.3 ms: the factorisation has three times as long, the pair kernel misses every CU longer) 8: 439, 12: 456, 16: 460, 20: 454,
    // 24: 436, 32: 433 (the sequential front: 433).  Round 6 (faster chain): unit weights -: 865, 24: 846, 32: 865, 40: 809; soft_l1 8: 460, 16: 486, 24: 486
    // the split of the diagonal pass (read at every front: the tests switch it inside one process).  SATBA_DIAG_LATE_COLS: late tile
    // columns (0: the undivided pass); SATBA_DIAG_LATE_FROM: c* directly (tests); SATBA_DIAG_LATE_PLACE: a (own launch) | b (tail of the pair launch)
    const bool split_applies = r.beside_ok && r.unit && !r.dg_in_pairs && r.red_chunks == 1;
    const char *lf = getenv("SATBA_DIAG_LATE_FROM"), *lc = getenv("SATBA_DIAG_LATE_COLS"), *lp = getenv("SATBA_DIAG_LATE_PLACE");
    r.c_split = (lf && *lf) ? diag_split_forced(p->M, atoi(lf), split_applies)
                            : diag_split_camera(p->M, p->NP, (lc && *lc) ? atoi(lc) : diag_late_cols_default(diag_split_tiles(p->M, p->NP)), split_applies);
    r.late_tail = (lp && *lp) ? (*lp == 'b' || *lp == 'B') : DIAG_LATE_TAIL_DEFAULT;
    // (the pair kernel of the weighted / robust runs writes the diagonal blocks and the right-hand side, too; late cameras count themselves in)
    r.wgs = r.weighted ? 16 : 32; r.arr_extra = (r.weighted || r.c_split < p->M) ? 1 : 0;
    return r;
}

SchurArgs schur_args(const satba_problem* p, const FrontCtx& f, const SchurRoute& r, double* rhs) {
    SchurArgs s;
    s.PV = reinterpret_cast<const double2*>(p->d_PV);
    s.pair_ofs = p->L.pair_ofs; s.pair_pts = p->L.pair_pts; s.pair_pi = p->L.pair_pi; s.pair_pj = p->L.pair_pj;
    s.pair_ij = p->L.pair_ij; s.pair_part = p->d_pair_part; s.n_chunks = r.n_chunks; s.items = r.items->items; s.desc = r.items->desc; s.diag_xcd = r.diag_xcd;
    if (r.weighted) {
        s.PV = p->d_W; s.wmode = 1; s.zero_fix = p->L.zero_fix; s.n_dg = p->L.n_dg;
        s.pair_rec = p->L.pair_rec; s.pair_kk = p->L.pair_kk; s.cm_rec = p->L.cm_rec; s.cm_sc = p->L.cm_sc; s.dg_part = p->d_part3;
    }
    if (f.arrive_epoch) {
        s.arrive = p->d_arrive; s.arrive_epoch = f.arrive_epoch; s.pair_cnt = p->d_pair_cnt; s.fail = p->d_fail;
        if (r.dg_in_pairs || r.c_split < p->M) {
            s.dg_cnt = p->d_dg_cnt; s.dg_lam = f.lam; s.dg_lam_dev = f.lam_dev; s.dg_lead = p->lead; s.dg_gc = p->d_gc;
            s.dg_scale_inv = p->d_scale_inv; s.dg_rhs = rhs;
        }
    }
    return s;
}

template <int MODEL, int NP>
int launch_schur(satba_problem* p, const FrontCtx& f, const SchurRoute& r, const ObsArgs& a, double* S, double* rhs) {
    // (schur_route lets the factorisation wait only beside pair items that write S themselves or add their partials up themselves)
    if (f.arrive_epoch && r.unit && r.red_chunks > 1) return fail(SATBA_E_STATE, "factorisation beside a unit-weight pair kernel with chunk partials");
    const CamMajor cm = cam_major(p, r.cm_rec);
    const SchurArgs s = schur_args(p, f, r, rhs);
    // cameras [0, c_split) in front of the pair kernel, [c_split, M) behind it (SchurRoute::c_split)
    const int c_split = f.arrive_epoch ? r.c_split : p->M;
    const bool late = c_split < p->M;
    p->diag_split_last = c_split;
    auto finish = [&]() {
        const long long outs = r.finish_red_chunks > 1 ? p->L.n_pairs * NP * NP : 0;
        hipLaunchKernelGGL(k_schur_finish, dim3((unsigned)(r.nb_diag + (outs + 255) / 256)), dim3(256), 0, p->stream, p->M, NP, p->n_c, r.finish_dchunks, p->d_part3,
                           f.lam, f.lam_dev, p->lead, p->d_gc, p->d_scale_inv, S, rhs, p->d_xb, (int)p->hdr, r.nb_diag, r.finish_red_chunks,
                           p->L.pair_ij, p->d_pair_part, a.gate, r.finish_scale ? p->d_dch : (double*)nullptr, r.finish_scale ? p->d_fail : (int*)nullptr,
                           r.finish_scale ? 1 + CH_MAX_STEPS : 0, late ? c_split : -1, late ? p->d_arrive : (int*)nullptr);
        p->s_scaled = r.finish_scale;
    };
    if (!r.dg_in_pairs && !r.both && c_split > 0)
        hipLaunchKernelGGL((k_schur_diag<MODEL, NP>), dim3(c_split, r.dchunks), dim3(LINC_THREADS), 0, p->stream, a, cm, s, p->d_part3);
    if (r.finish_first) finish();
    if (r.pairs_run) {
        const dim3 igrid((unsigned)r.items->n_blocks);
        if (r.both) {
            const int n_diag = p->M * r.dchunks, n_diag_pad = (n_diag + 7) & ~7;
            const dim3 bgrid(igrid.x + (unsigned)n_diag_pad);
            if (r.unit) hipLaunchKernelGGL((k_schur_both<MODEL, NP, true>), bgrid, dim3(256), 0, p->stream, a, cm, s, p->d_part3, S, n_diag, n_diag_pad, p->M, r.dchunks);
            else hipLaunchKernelGGL((k_schur_both<MODEL, NP, false>), bgrid, dim3(256), 0, p->stream, a, cm, s, p->d_part3, S, n_diag, n_diag_pad, p->M, r.dchunks);
        }
        else if (late && r.late_tail) {
            const int n_pad = ((int)igrid.x + 7) & ~7;
            hipLaunchKernelGGL((k_schur_pairs_diag_late<MODEL, NP>), dim3((unsigned)(n_pad + (p->M - c_split) * r.dchunks)), dim3(256), 0, p->stream, a, cm, s, p->d_part3, S,
                               (int)igrid.x, n_pad, c_split, r.dchunks);
        }
        else if (r.unit) hipLaunchKernelGGL((k_schur_pairs<MODEL, NP, true>), igrid, dim3(256), 0, p->stream, a, s, S);
        else hipLaunchKernelGGL((k_schur_pairs<MODEL, NP, false>), igrid, dim3(256), 0, p->stream, a, s, S);
        HIP_TRY(hipGetLastError());
        if (late && !r.late_tail)
            hipLaunchKernelGGL((k_schur_diag_late<MODEL, NP>), dim3((unsigned)((p->M - c_split) * r.dchunks)), dim3(LINC_THREADS), 0, p->stream, a, cm, s, p->d_part3, S,
                               c_split, r.dchunks);
    }
    if (!r.finish_first) finish();
    HIP_TRY(hipGetLastError());
    return 0;
}

// automatic: the damping comes from the prepare header and the trust radius Delta (satba_schur_auto), which consumes the prepare header
int schur_impl(satba_problem* p, const PhaseCtx& c, FrontCtx f, double lam, bool automatic, double Delta, double lam_floor) {
    Range range_("satba:schur");
    if (!p->linearized || (automatic && !p->prepared)) return fail(SATBA_E_STATE, automatic ? "schur_auto before prepare" : "schur before linearize");
    if (automatic) p->prepared = false;
    const SchurRoute r = schur_route(p, f);
    if (p->N > 0) {
        const bool w = r.weighted;  // the records go into the merged records W, behind the row scales k_linearize left there
        hipLaunchKernelGGL(k_vinv, dim3((p->N + VINV_THREADS - 1) / VINV_THREADS), dim3(VINV_THREADS), 0, p->stream, p->N, lam, automatic ? p->d_xb : nullptr, Delta, lam_floor,
                           p->d_keep, p->d_V, p->d_scale_inv + p->n_c, p->d_lam_used, p->d_x + p->n_c, p->d_g + p->n_c, w ? reinterpret_cast<double*>(p->d_W) : p->d_PV,
                           p->L.perm, p->n_pts_fix, automatic ? c.Delta_dev : nullptr, automatic ? c.lam_force_dev : nullptr, c.gate,
                           w ? p->L.w_fix : (const int*)nullptr);
    } else if (automatic) {
        hipLaunchKernelGGL(k_lambda, dim3(1), dim3(1), 0, p->stream, p->d_xb, Delta, lam_floor, p->d_keep, c.Delta_dev, c.lam_force_dev, c.gate);
    }
    HIP_TRY(hipGetLastError());
    // The header is cleared by k_schur_finish (k_vinv reads it).  S and rhs are only cleared when no pair kernel will run: every block
    // of the lower triangle is otherwise written by the kernels below (k_schur_finish the diagonal blocks and rhs, the pair kernel or
    // k_schur_finish every off-diagonal block).
    if (!r.pairs_run) HIP_TRY(hipMemsetAsync(p->d_xb + p->hdr, 0, sizeof(double) * ((size_t)p->n_c * p->n_c + p->n_c), p->stream));
    f.lam = lam; f.lam_dev = automatic ? p->d_keep + SATBA_KEEP_LAM : nullptr;
    return launch_schur_kernel(p, c.gate, f, r);
}

// header slot SATBA_HDR_CHOL_FAIL of the solve phase = lead x status word of the factorisation: SATBA_CHOL_TIMEOUT = a wait timed out.  Beside the pair kernel that
// means the two kernels did not run at the same time (a profiler collecting counters serialises the launches): the handle goes back
// to one kernel after the other and the caller repeats the front with the same damping.
void beside_disable(satba_problem* p) {
    // (the interval in force is doubled AFTER it has been used: the first one is 64 sequential fronts, as the field says)
    if (p->beside_timeouts > 0) p->beside_retry_after = std::min(p->beside_retry_after * 2, 1 << 20);
    p->beside_off = true; p->beside_clean = 0; ++p->beside_timeouts;
    (void)hipStreamSynchronize(p->chol_stream);
    (void)hipMemsetAsync(p->d_arrive, 0, sizeof(int) * (size_t)(p->M + 2) * SCHUR_ARRIVE_STRIDE, p->stream);
    (void)hipMemsetAsync(p->d_pair_cnt, 0, sizeof(int) * (size_t)std::max<long long>(p->L.n_pairs, 1), p->stream);
    (void)hipMemsetAsync(p->d_dg_cnt, 0, sizeof(int) * (size_t)p->M, p->stream);
}
bool beside_timed_out(satba_problem* p, const double* h) {
    if (!p->beside_last || !(h[SATBA_HDR_CHOL_FAIL] >= SATBA_CHOL_BESIDE_WAIT)) return false;  // (a wait between the two kernels)
    beside_disable(p);
    return true;
}
// ---- the factorisation on a stream of its own, reading every tile of S when its producers have counted in (C3Args::arrive): beside the
// pair kernel on one rank (front_schur_solve), beside the all-reduce of S cut into messages with several (satba_solve_messages_*)
int chol_front_streams(satba_problem* p) {
    if (p->chol_stream) return 0;
    // A priority of its own: streams of one priority share a small pool of hardware queues, and two streams on ONE queue run in
    // submission order -- the factorisation, queued first, would wait for a pair kernel stuck behind it until its waits time out
    // (seen once in a long test process, where the pool had been handed round many times).
    int least = 0, greatest = 0, mine = 0;
    HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIP_TRY(hipStreamGetPriority(p->stream, &mine));
    HIP_TRY(hipStreamCreateWithPriority(&p->chol_stream, hipStreamNonBlocking, mine != greatest ? greatest : least));
    HIP_TRY(hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming));
    TRY(dev_alloc(p, &p->d_arrive, (size_t)(p->M + 2) * SCHUR_ARRIVE_STRIDE));  // (+ k_schur_pairs' start word, + the solve's done word)
    HIP_TRY(hipMemsetAsync(p->d_arrive, 0, sizeof(int) * (size_t)(p->M + 2) * SCHUR_ARRIVE_STRIDE, p->stream));
    TRY(dev_alloc(p, &p->d_pair_cnt, (size_t)std::max<long long>(p->L.n_pairs, 1)));
    HIP_TRY(hipMemsetAsync(p->d_pair_cnt, 0, sizeof(int) * (size_t)std::max<long long>(p->L.n_pairs, 1), p->stream));
    TRY(dev_alloc(p, &p->d_dg_cnt, (size_t)p->M));
    HIP_TRY(hipMemsetAsync(p->d_dg_cnt, 0, sizeof(int) * (size_t)p->M, p->stream));
    return 0;
}
// k_chol_tiles (wgs workgroups) and the backward substitution on the other stream, behind everything queued on p->stream so far; *epoch:
// the launch's epoch (FrontCtx::arrive_epoch, chol_front_finish).  arr_extra: C3Args::arr_extra.
int chol_front_launch(satba_problem* p, const int* gate, int wgs, int arr_extra, long long arr_timeout, int* epoch) {
    Range range_("satba:solve");
    double* S = p->payload();
    double* rhs = S + (size_t)p->n_c * p->n_c;
    const int n = p->n_c;
    HIP_TRY(hipEventRecord(p->ev_fork, p->stream));
    HIP_TRY(hipStreamWaitEvent(p->chol_stream, p->ev_fork, 0));
    HIP_TRY(hipMemsetAsync(p->d_fail, 0, sizeof(int) * (1 + CH_MAX_STEPS), p->chol_stream));
    cholesky_init();
    C3Args g;
    g.A = S; g.n = n; g.b = p->d_dch; g.fail = p->d_fail; g.flags = p->chol.flags; g.epoch = ++p->chol.epoch; g.Linv = p->chol.Linv; g.Cc = p->chol.Cc;
    g.ctr = p->chol.ctr; g.dinv = p->d_dinv; g.ts = nullptr; g.mirror = 1;
#ifdef C3_STAMPS
    if (!p->d_ts) { TRY(dev_alloc(p, &p->d_ts, (size_t)20 * C3_TS)); }
    HIP_TRY(hipMemsetAsync(p->d_ts, 0, sizeof(long long) * 20 * C3_TS, p->chol_stream));
    g.ts = p->d_ts;
#endif
    g.arrive = p->d_arrive; g.arr_M = p->M; g.np = p->NP; g.arr_epoch = g.epoch; g.si = p->d_scale_inv; g.rhs = rhs;
    g.arr_extra = arr_extra; g.arr_timeout = arr_timeout;
    hipLaunchKernelGGL(k_chol_tiles, dim3(std::min(chol_tiles_grid(n, 1), wgs)), dim3(1024), c3_lds_bytes(), p->chol_stream, g, gate);
    hipLaunchKernelGGL(k_trsv_back_mw, dim3((n + CH_SB - 1) / CH_SB), dim3(512), 0, p->chol_stream, S, p->d_dinv, n, p->d_dch,
                       p->d_fail + 1 + CH_TRSV_FLAGS, gate, p->d_arrive + (size_t)SCHUR_ARRIVE_STRIDE * (p->M + 1), g.epoch);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(p->ev_join, p->chol_stream));
    *epoch = g.epoch;
    return 0;
}
// the rest of the solve phase on p->stream: k_unscale waits for the word the backward substitution posts on the other stream (the event
// only orders what follows), then the points' part of the step
int chol_front_finish(satba_problem* p, const int* gate, int epoch) {
    const int nu = std::max(p->n_c, (int)p->hdr);
    hipLaunchKernelGGL(k_unscale, dim3((nu + 255) / 256), dim3(256), 0, p->stream, p->n_c, p->d_scale_inv, p->d_dch, p->d_dc, (int)p->hdr,
                       p->d_xb, p->d_fail, p->lead, p->d_keep, SATBA_HDR_KEEP, SATBA_KEEP_LEN, gate,
                       p->d_arrive + (size_t)SCHUR_ARRIVE_STRIDE * (p->M + 1), epoch);
    HIP_TRY(hipGetLastError());
    TRY(launch_backsub_kernel(p, gate));
    HIP_TRY(hipStreamWaitEvent(p->stream, p->ev_join, 0));
    p->have_step = true;
    return 0;
}

// schur (+ auto damping) and solve of a front
// One rank, more than two tile columns (SchurRoute::beside_ok): the tile factorisation is launched FIRST, on a stream of its own, and works
// beside the pair kernel -- the rows of the pair triangle are finished in ascending order (satba_schur_items.h), i.e. the columns of S
// from the left, and every tile of the factorisation waits for the producers of its columns (C3Args::arrive).  The workgroups of
// the factorisation (SATBA_CHOL_BESIDE_WGS, 1024 threads each: a CU of their own) are resident before the Schur kernels fill the chip.
int front_schur_solve(satba_problem* p, const PhaseCtx& c, bool automatic, double lam, double Delta, double lam_floor) {
    FrontCtx f;
    if (p->beside_off && ++p->beside_clean > p->beside_retry_after) p->beside_off = false;  // (schur_route decides whether it applies at all)
    const SchurRoute r = schur_route(p, f);
    p->beside_last = r.beside_ok;
    if (!p->beside_last) {
        f.scale_in_finish = p->world == 1 && p->n_c > CH_ONE_LAUNCH;  // (the solve follows at once: nobody looks at S in between)
        if (const int rc = schur_impl(p, c, f, lam, automatic, Delta, lam_floor)) { p->s_scaled = false; return rc; }
        return solve_impl(p, c);
    }
    TRY(chol_front_streams(p));
    const char* env_wgs = getenv("SATBA_CHOL_BESIDE_WGS");
    const int wgs = (env_wgs && atoi(env_wgs) > 0) ? atoi(env_wgs) : r.wgs;
    // 5 ms + ~10 x what the kernels in front of a tile's last producer take at HBM speed (hit lists and records: ~100 bytes per hit) -- every
    // kernel of the front is counted, so the sum also covers a tile whose last producer is the late part of the diagonal pass, behind the pair
    // kernel (SchurRoute::c_split: the same K entries, cut in two); a wait's clock starts when the wait does
    const long long timeout = 500000 + (long long)((double)p->L.E * 100.0 / 6e12 * 1e8 * 10.0) + (long long)((double)p->K * 200.0 / 6e12 * 1e8 * 10.0);
    TRY(chol_front_launch(p, c.gate, wgs, r.arr_extra, timeout, &f.arrive_epoch));
    if (const int rc = schur_impl(p, c, f, lam, automatic, Delta, lam_floor)) {
        HIP_TRY(hipStreamWaitEvent(p->stream, p->ev_join, 0));  // (the other stream's work is bounded by its time-out)
        return rc;
    }
    return chol_front_finish(p, c.gate, f.arrive_epoch);
}

// ---- several ranks: the all-reduce of S in messages, the factorisation beside it (round 6, DESIGN.md section 5).  The packed payload
// [header | rhs | columns of the lower triangle] is cut at camera boundaries into messages of about equal size; the caller all-reduces
// message m and tells the handle (satba_solve_messages_arrived), which unpacks its columns and counts their cameras in; k_chol_tiles,
// launched first on the other stream, takes tile column k when the cameras of its 64 columns are in -- the same arrival words, the same
// scale-as-you-read arithmetic and therefore the same bits as beside the pair kernel on one rank and as the sequential front.
// bounds: n_messages + 1 camera indices; the packed range of message m is [pk(bounds[m]), pk(bounds[m + 1])) with
// pk(c) = hdr + n_c + col_ofs(c n_p) for c > 0 and pk(0) = 0 (the first message carries header and right-hand side).
int schur_message_cams(const satba_problem* p, std::vector<int>& cam_bounds) {
    static const int want = getenv("SATBA_PIPELINE_MESSAGES") ? std::max(1, std::min(16, atoi(getenv("SATBA_PIPELINE_MESSAGES")))) : 4;
    const long long n = p->n_c, np = p->NP;
    const long long tri = n * (n + 1) / 2;
    cam_bounds.assign(1, 0);
    for (int m = 1; m < want; ++m) {
        // first camera whose columns start at or behind the fraction m / want of the triangle's entries
        const long long target = tri * m / want;
        int c = cam_bounds.back();
        while (c < p->M && (c * np) * n - (c * np) * ((c * np) - 1) / 2 < target) ++c;
        if (c > cam_bounds.back() && c < p->M) cam_bounds.push_back(c);
    }
    cam_bounds.push_back(p->M);
    return (int)cam_bounds.size() - 1;
}
long long packed_col_ofs(const satba_problem* p, long long col) {  // index of column `col`'s diagonal entry in the packed payload
    return p->hdr + p->n_c + col * p->n_c - col * (col - 1) / 2;
}
bool solve_messages_ok(const satba_problem* p) {  // (the tile kernel with mirror and multi-workgroup substitution: as SchurRoute::beside_ok)
    return p->n_c == p->M * p->NP && p->n_c > 128 && p->n_c <= 1024;
}
// pack S | rhs | header into `packed` and launch the factorisation, which waits for the messages
int solve_messages_begin_impl(satba_problem* p, const int* gate, double* packed, int packed_already) {
    if (!packed) return fail(SATBA_E_ARG, "null argument");
    if (!solve_messages_ok(p)) return fail(SATBA_E_ARG, "the reduced system of this handle is solved in one piece (satba_solve)");
    TRY(chol_front_streams(p));
    if (!packed_already) hipLaunchKernelGGL(k_pack_lower, dim3(p->n_c + 1), dim3(256), 0, p->stream, p->n_c, (int)p->hdr, p->d_xb, packed, 0, 0, p->n_c, gate);
    HIP_TRY(hipGetLastError());
    // a message is a collective of the caller's library between host-side calls: the wait is sized for those, not for a kernel (2 s;
    // SATBA_PIPELINE_TIMEOUT_MS); a time-out is reported like any failed factorisation
    static const long long ms = getenv("SATBA_PIPELINE_TIMEOUT_MS") ? atoll(getenv("SATBA_PIPELINE_TIMEOUT_MS")) : 2000;
    static const int wgs = getenv("SATBA_PIPELINE_WGS") ? std::max(8, atoi(getenv("SATBA_PIPELINE_WGS"))) : 64;
    return chol_front_launch(p, gate, wgs, 0, ms * 100000, &p->msg_epoch);  // (no Schur kernel of this rank is a producer: no FrontCtx)
}
// message m has been all-reduced in `packed`: its columns into S (message 0: header and right-hand side, too), its cameras counted in
int solve_messages_arrived_impl(satba_problem* p, const int* gate, const double* packed, int m) {
    if (!packed) return fail(SATBA_E_ARG, "null argument");
    std::vector<int> cb;
    const int nm = schur_message_cams(p, cb);
    if (m < 0 || m >= nm || !p->msg_epoch) return fail(SATBA_E_STATE, "no such message, or no satba_solve_messages_begin");
    const int c_lo = cb[m] * p->NP, c_hi = cb[m + 1] * p->NP;
    hipLaunchKernelGGL(k_pack_lower, dim3(p->n_c + 1), dim3(256), 0, p->stream, p->n_c, (int)p->hdr, p->d_xb, const_cast<double*>(packed), 1, c_lo, c_hi, gate);
    hipLaunchKernelGGL(k_mark_arrived, dim3((cb[m + 1] - cb[m] + 63) / 64), dim3(64), 0, p->stream, p->d_arrive, cb[m], cb[m + 1], p->M, p->msg_epoch, m == 0 ? 1 : 0,
                       gate);
    HIP_TRY(hipGetLastError());
    return 0;
}
int solve_messages_end_impl(satba_problem* p, const int* gate) {
    if (!p->msg_epoch) return fail(SATBA_E_STATE, "satba_solve_messages_end before _begin");
    const int epoch = p->msg_epoch;
    p->msg_epoch = 0;
    return chol_front_finish(p, gate, epoch);
}

}  // namespace
}  // extern "C++"

int32_t satba_solve_messages(satba_problem* p, int64_t* bounds, int32_t cap) {
    if (!p) return -1;
    if (!solve_messages_ok(p)) return 0;  // the caller all-reduces the whole payload and calls satba_solve
    std::vector<int> cb;
    const int nm = schur_message_cams(p, cb);
    if (bounds) {
        if (cap < nm + 1) return -1;
        for (int m = 0; m <= nm; ++m) bounds[m] = m == 0 ? 0 : (m == nm ? satba_packed_schur_len(p) : packed_col_ofs(p, (long long)cb[m] * p->NP));
    }
    return nm;
}
int satba_solve_messages_begin(satba_problem* p, double* packed, int32_t packed_already) {
    if (!p) return fail(SATBA_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    return solve_messages_begin_impl(p, nullptr, packed, packed_already);
}
int satba_solve_messages_arrived(satba_problem* p, const double* packed, int32_t m) {
    if (!p) return fail(SATBA_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(p->device));
    return solve_messages_arrived_impl(p, nullptr, packed, m);
}
// the packed payload the device-resident loop's parts 10 - 12 work on (satba_lm_part has no pointer argument)
int satba_solve_messages_bind(satba_problem* p, double* packed) {
    if (!p) return fail(SATBA_E_ARG, "null handle");
    p->msg_packed = packed;
    return 0;
}
int satba_solve_messages_end(satba_problem* p) {
    if (!p) return fail(SATBA_E_ARG, "null handle");
    HIP_TRY(hipSetDevice(p->device));
    return solve_messages_end_impl(p, nullptr);
}

int satba_schur(satba_problem* p, double lam) {
    if (!p) return fail(SATBA_E_ARG, "null handle");
    HIP_TRY(hipSetDevice(p->device));
    return schur_impl(p, PhaseCtx{}, FrontCtx{}, lam, false, 0.0, 0.0);
}
int satba_schur_auto(satba_problem* p, double Delta, double lam_floor) {
    if (!p) return fail(SATBA_E_ARG, "null handle");
    HIP_TRY(hipSetDevice(p->device));
    return schur_impl(p, PhaseCtx{}, FrontCtx{}, 0.0, true, Delta, lam_floor);
}

// satba_lm_step / satba_lm_run / satba_lm_begin, _part, _poll, _state / satba_solve_lm (include/satba.h): part of the extern "C" block of
// satba_capi.hip -- the trust-region loop over the phases: the host side of an iteration in C++, the queueing of the device-resident loop.
// The loop of satba/trf.py (scipy's trf_no_bounds with an exact damped step) below the ABI: single rank only -- with several
// ranks the exchange buffer has to be all-reduced between the phases, which is the caller's side of the contract.
// single-rank loops: linearize with the point part of the prepare phase fused into k_linearize (ObsArgs::prep_*)
static PhaseCtx fused_prep_ctx(bool first) { PhaseCtx c; c.fuse_prep = first ? 1 : 0; return c; }

// quadratic model of the cost on the orthonormal basis of span{g_h, gn_h} (satba/trf.py:subspace_model): B (2 x 2, entries Ba Bb Bc),
// gradient (gS0, gS1), and what maps a step (p0, p1) on that basis back to coefficients of (g_h, gn_h).  h: header of the solve
// phase; tmp: scratch header.  Launches the subspace phases only when the Gram matrix is too ill-conditioned to do without.
struct LmModel { double Ba, Bb, Bc, gS0, gS1, sa, alpha, nw; bool one_dim; };
static int lm_subspace_model(satba_problem* p, const double* h, double* tmp, double reg, double jg_sq, LmModel& m) {
    const double ga = h[SATBA_HDR_GRAM_A], gb = h[SATBA_HDR_GRAM_B], gc = h[SATBA_HDR_GRAM_C];
    const double sa = std::sqrt(ga), alpha = gb / ga;
    double ww = gc - gb * alpha, nw = 0.0, b11, b12, b22, ghw = 0.0;
    bool one_dim = false;
    if (ww > 1e-6 * gc) {
        nw = std::sqrt(ww);
        const double m11 = jg_sq, m12 = ga - reg * gb, m22 = gb - reg * gc;
        b11 = m11 / ga;
        b12 = (m12 - alpha * m11) / sa;
        b22 = m22 - 2.0 * alpha * m12 + alpha * alpha * m11;
    } else {
        TRY(subspace_impl(p, PhaseCtx{}, alpha, 1.0 / sa));
        TRY(satba_read_header(p, tmp));
        ww = tmp[SATBA_HDR_WW]; ghw = tmp[SATBA_HDR_GHW];
        if (!(ww > 1e-24 * gc && ww > 0)) {
            one_dim = true;
            b11 = jg_sq / ga; b12 = 0.0; b22 = 1.0; nw = 1.0; ww = 1.0; ghw = 0.0;
        } else {
            nw = std::sqrt(ww);
            TRY(subspace_products_impl(p, PhaseCtx{}));
            TRY(satba_read_header(p, tmp));
            b11 = tmp[SATBA_HDR_B11]; b12 = tmp[SATBA_HDR_B12]; b22 = tmp[SATBA_HDR_B22];
        }
    }
    m.Ba = b11; m.Bb = one_dim ? 0.0 : b12 / nw; m.Bc = one_dim ? 1.0 : b22 / ww;
    m.gS0 = sa; m.gS1 = one_dim ? 0.0 : ghw / nw;
    m.sa = sa; m.alpha = alpha; m.nw = nw; m.one_dim = one_dim;
    return 0;
}

// ---- the three pieces of a host-driven iteration that satba_lm_step and lm_host_loop share (h: header of the solve phase).  The front:
// linearize -> prepare -> damped Gauss-Newton step with the damping from the trust radius (first: scipy's initial radius, Delta is
// ignored), one header read; repeated on the camera-major sums when a term left the fixed-point range
static int lm_front(satba_problem* p, bool first, double Delta, double lam_floor, double* h) {
    for (;;) {
        TRY(linearize_impl(p, fused_prep_ctx(first)));
        TRY(prepare_impl(p, PhaseCtx{}, first ? 1 : 0));
        TRY(front_schur_solve(p, PhaseCtx{}, true, 0.0, first ? -1.0 : Delta, lam_floor));
        TRY(satba_read_header(p, h));
        if (h[SATBA_HDR_FX_BAD] == 0.0 || !p->cam_sums_lds) return 0;
        TRY(satba_camera_sums_fallback(p));
    }
}
// A Cholesky needs a floor where LSMR copes with a numerically singular system: a failed factorisation is repeated with the damping
// x 100 (the same damping after a time-out of the concurrent front: beside_timed_out), at most ten times.  exhausted: all ten were used
static int lm_refactorise(satba_problem* p, double* h, double& reg, bool& exhausted) {
    exhausted = false;
    for (int attempt = 0; attempt < 10; ++attempt) {
        if (h[SATBA_HDR_CHOL_FAIL] == 0 && std::isfinite(h[SATBA_HDR_GRAM_C])) return 0;
        if (!beside_timed_out(p, h)) reg = std::fmax(reg, 1e-16) * 100.0;
        TRY(front_schur_solve(p, PhaseCtx{}, false, reg, 0.0, 0.0));
        TRY(satba_read_header(p, h));
    }
    exhausted = true;
    return 0;
}
// One trial step: the 2-D trust-region subproblem on the model for the radius Delta, the trial point, its header read into t
struct LmTrial { double cost_new, predicted, step_h_norm; bool newton; };
static int lm_trial(satba_problem* p, const LmModel& m, double Delta, double* t, LmTrial& r) {
    double p0, p1;
    r.newton = satba_lm::solve_trust_region_2d(m.Ba, m.Bb, m.Bc, m.gS0, m.gS1, Delta, p0, p1);
    r.predicted = -(0.5 * (p0 * (m.Ba * p0 + m.Bb * p1) + p1 * (m.Bb * p0 + m.Bc * p1)) + m.gS0 * p0 + m.gS1 * p1);
    const double ca = m.one_dim ? p0 / m.sa : p0 / m.sa - p1 * m.alpha / m.nw, cb = m.one_dim ? 0.0 : p1 / m.nw;
    TRY(trial_impl(p, PhaseCtx{}, true, ca, cb));
    TRY(satba_read_header(p, t));
    r.cost_new = t[SATBA_HDR_COST_NEW];
    r.step_h_norm = satba_lm::norm2(p0, p1);
    return 0;
}

// One fixed-work LM iteration of a single-rank handle, the host side in C++ (what bench.py's lm_step does in Python, phase by
// phase): front -> 2-D trust-region subproblem -> trial point -> accept if the cost went down.  first: first iteration (Jacobian
// scaling and trust radius are initialised); Delta: trust radius (ignored when first).  out[8]: cost at x, cost at the trial point,
// new trust radius, accepted (0/1), interior Newton step (0/1), predicted and actual reduction, damping.
int satba_lm_step(satba_problem* p, int32_t first, double Delta, double lam_floor, double* out) {
    if (!p || !out) return fail(SATBA_E_ARG, "null argument");
    if (p->world != 1) return fail(SATBA_E_ARG, "satba_lm_step drives a single-rank handle (world = %d): use the phase entry points", p->world);
    HIP_TRY(hipSetDevice(p->device));
    std::vector<double> hbuf((size_t)p->hdr), tbuf((size_t)p->hdr);
    double* h = hbuf.data();
    const double* keep = h + SATBA_HDR_KEEP;
    TRY(lm_front(p, first != 0, Delta, lam_floor, h));
    double reg = keep[SATBA_KEEP_LAM];
    bool exhausted;
    TRY(lm_refactorise(p, h, reg, exhausted));  // (out of attempts: carries on with what the last one left)
    const double cost = keep[SATBA_KEEP_COST];
    Delta = keep[SATBA_KEEP_DELTA];
    LmModel md;
    TRY(lm_subspace_model(p, h, tbuf.data(), reg, keep[SATBA_KEEP_JG_SQ], md));
    LmTrial t;
    TRY(lm_trial(p, md, Delta, tbuf.data(), t));
    const double actual = std::isfinite(t.cost_new) ? cost - t.cost_new : -1.0;
    double ratio;
    const double Delta_new = satba_lm::update_tr_radius(Delta, actual, t.predicted, t.step_h_norm, t.step_h_norm > 0.95 * Delta, ratio);
    if (actual > 0) TRY(satba_accept(p));
    out[0] = cost; out[1] = t.cost_new; out[2] = Delta_new; out[3] = actual > 0 ? 1.0 : 0.0; out[4] = t.newton ? 1.0 : 0.0;
    out[5] = t.predicted; out[6] = actual; out[7] = reg;
    return 0;
}

// ---- device-resident loop (satba_lmdev.h): reset the state, queue ticks, read the state back
static int lm_reset(satba_problem* p, const satba_lm_opts* o, bool never_stop, bool watch, bool keep_counters = false, long long max_iterations = 0,
                    int cycle_len = 0) {
    LmDev init;
    memset(&init, 0, sizeof init);
    init.run_lin = 1; init.run_solve = 1; init.phase = LM_RUN; init.status = -1; init.first = 1;
    init.never_stop = never_stop ? 1 : 0;
    init.max_nfev = o->max_nfev > 0 ? o->max_nfev : p->n_total * 100;
    init.Delta = -1.0;  // <= 0: scipy's initial radius |x_h| (schur_lambda)
    init.ftol = o->ftol; init.xtol = o->xtol; init.gtol = o->gtol;
    init.max_iterations = max_iterations; init.cycle_len = cycle_len;
    if (watch) {  // the host is going to poll the summary: nothing of an earlier run may still post to it
        HIP_TRY(hipStreamSynchronize(p->stream));
        p->h_lm->word = (unsigned long long)LM_RUN; p->h_lm->sub_requests = 0; p->h_lm->sub_tick = 0; p->h_lm->end_tick = 0;
        __atomic_thread_fence(__ATOMIC_SEQ_CST);
    }
    hipLaunchKernelGGL(k_lm_reset, dim3(1), dim3(1), 0, p->stream, p->d_lm, init, keep_counters ? 1 : 0);
    HIP_TRY(hipGetLastError());
    p->lm_ticks_queued = 0;
    return 0;
}

// one tick (satba_lmdev.h): every launch is gated by the loop's state, nothing waits for the device.  lm_ctx: the context of one part
// of the pattern -- switched by `gate`, the launchers read the loop's scalars from its state in device memory
static PhaseCtx lm_ctx(const satba_problem* p, const int* gate) {
    LmDev* st = p->d_lm;
    PhaseCtx c;
    c.gate = gate; c.Delta_dev = &st->Delta; c.first_dev = &st->first; c.lam_force_dev = &st->lam_force; c.coef_dev = st->coef; c.sub_args_dev = st->sub_args;
    return c;
}

// end of a pattern: the accepted point, or the kept one, into place (the caller checks hipGetLastError)
static void lm_launch_accept(satba_problem* p) {
    const double* x0 = p->d_x0;
    hipLaunchKernelGGL(k_lm_accept, dim3(grid_for(p->n / 2 + 1, 256, 1024)), dim3(256), 0, p->stream, p->d_lm, (long long)p->n, p->d_x, p->d_xnew,
                       p->M * CAMC, p->d_camc, p->d_camc_new, p->d_fxcost, p->d_fxcost_new, x0, x0 ? x0 + p->n + 6 : nullptr, p->d_fxcost0, p->d_bbox);
}
// what the host-side flags say after a queued pattern: the linearisation and the step belong to the point the device ends up at
static void lm_pattern_queued(satba_problem* p) {
    p->linearized = true; p->prepared = false; p->have_step = true;
    p->fxcost_valid = true; p->fxcost_new_valid = false;
    ++p->lm_ticks_queued;
}

// trial evaluation, decision, accepted point (or the kept one) into place; decide1a: k_lm_decide1a rides in the trial's first launch
static int lm_launch_tail(satba_problem* p, bool decide1a) {
    LmDev* st = p->d_lm;
    // the second decision rides in the trial's residual kernel (TrialArgs::lm_st; SATBA_DECIDE2_FUSED=0: the launch of its own)
    static const bool fuse2 = !(getenv("SATBA_DECIDE2_FUSED") && atoi(getenv("SATBA_DECIDE2_FUSED")) == 0);
    PhaseCtx c = lm_ctx(p, &st->run_trial);
    c.decide1a_in_trial = decide1a; c.decide2_in_trial = fuse2;
    TRY(trial_impl(p, c, true, 0.0, 0.0));
    if (!fuse2) hipLaunchKernelGGL(k_lm_decide2, dim3(1), dim3(1), 0, p->stream, st, p->d_xb, p->h_lm_dev);
    const double* x0 = p->d_x0;
    // the scales of the next tick's fixed-point camera sums ride in this launch (k_lm_accept_scales; SATBA_SCALES_IN_ACCEPT=0: k_lin_scales in every tick)
    static const bool fuse_scales = !(getenv("SATBA_SCALES_IN_ACCEPT") && atoi(getenv("SATBA_SCALES_IN_ACCEPT")) == 0);
    if (fuse_scales && p->cam_sums_lds && p->model != RPC) {  // (RPC: eight chains per camera in one workgroup outlast the copy -- C5 1 795 against 1 782 it/s)
        LinScalesArgs q;
        q.M = p->M; q.loss = p->loss; q.n_clear = (int)(p->hdr + (size_t)p->M * p->NP * p->NP + p->n_c);
        q.w_max = p->w_max; q.f_scale = p->f_scale; q.n_max = p->n_max_cam; q.shrink = p->fx_shrink;
        q.rpc = p->d_rpc; q.fx = p->d_fx; q.fxe = p->d_fxe; q.fx_flag = p->d_fxflag; q.clear = p->d_xb;
        SATBA_DISPATCH(p, hipLaunchKernelGGL((k_lm_accept_scales<MODEL, NP>), dim3(grid_for(p->n / 2 + 1, 256, 1024) + 1), dim3(256), 0, p->stream, st, (long long)p->n,
                                             p->d_x, p->d_xnew, p->M * CAMC, p->d_camc, p->d_camc_new, p->d_fxcost, p->d_fxcost_new, x0,
                                             x0 ? x0 + p->n + 6 : nullptr, p->d_fxcost0, p->d_bbox, q));
        p->scales_by_tail = true;
    } else {
        lm_launch_accept(p);
        p->scales_by_tail = false;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

static int lm_launch_tick(satba_problem* p, double lam_floor) {
    LmDev* st = p->d_lm;
    PhaseCtx lin = lm_ctx(p, &st->run_lin);
    lin.fuse_prep = 0;  // (`first` comes from the loop's state)
    lin.skip_lin_scales = p->scales_by_tail && p->cam_sums_lds;
    TRY(linearize_impl(p, lin));
    TRY(prepare_impl(p, lm_ctx(p, &st->run_lin), 0));
    TRY(front_schur_solve(p, lm_ctx(p, &st->run_solve), true, 0.0, -1.0, lam_floor));
    return lm_launch_tail(p, true);
}

// the pattern of the degenerate case (g_h and gn_h parallel to 1e-6): explicit subspace vectors and products, then the tail
static int lm_launch_sub_pattern(satba_problem* p) {
    LmDev* st = p->d_lm;
    TRY(subspace_impl(p, lm_ctx(p, &st->run_sub), 0.0, 0.0));
    hipLaunchKernelGGL(k_lm_decide1b, dim3(1), dim3(1), 0, p->stream, st, p->d_xb);
    TRY(subspace_products_impl(p, lm_ctx(p, &st->run_prod)));
    hipLaunchKernelGGL(k_lm_decide1c, dim3(1), dim3(1), 0, p->stream, st, p->d_xb);
    return lm_launch_tail(p, false);
}

// one tick (direct launches: a captured hipGraph of the pattern was measured in round 3 -- 2 - 9 us between its nodes where back-to-back
// launches leave none, ~30 us in front of every replay, profiles/r3_graph_gaps.txt -- and removed in round 4)
static int lm_queue_tick(satba_problem* p, double lam_floor) {
    TRY(lm_launch_tick(p, lam_floor));
    lm_pattern_queued(p);
    return 0;
}

static int lm_read_state(satba_problem* p, LmDev* host) {
    HIP_TRY(hipMemcpyAsync(host, p->d_lm, sizeof *host, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return 0;
}

// whether this handle can run the device-resident loop: one rank, default dense-solver mode (its kernels carry the gates)
static bool lm_device_loop_ok(const satba_problem* p) {
    const bool off = getenv("SATBA_HOST_LOOP") != nullptr;  // A/B runs and the tests' comparison of the two loops (read per call)
    return !off && p->world == 1 && p->n_c <= 1024;
}
// ... and whether it is the default: everywhere it can run (round 5).  200 x 1 M x 10 M: linear loss 846 it/s on the device against 837
// with the host's two header reads per iteration (the factorisation beside the pair kernel took the dense solve off the critical
// path, and with it the slack that hid the reads); soft_l1 463 / 463 / 463 against 465 / 463 / 464 -- three iterations in ten pause
// there for the degenerate-subspace pattern, which the host has to notice and queue (LM_NEED_SUB: the ticks queued behind the pause
// pass empty); with round 4's Schur phase that cost 411 - 420 against 427 - 438 and the host loop was the default for robust losses
// from 4 M observations on.  Smaller problems: 50 x 100 k x 1 M 2 580 / 2 500, 10 x 5 k x 30 k 6 320 / 5 380 (round 3).
// SATBA_DEVICE_LOOP=0 (or SATBA_HOST_LOOP) selects the host loop.
static bool lm_device_loop_pays(const satba_problem*) {
    if (const char* e = getenv("SATBA_DEVICE_LOOP")) return atoi(e) != 0;
    return true;
}

int satba_lm_state(satba_problem* p, double* out, int32_t n);

// One rank: how many ticks the host queues beyond the device's last report.  Every tick queued behind the end of the loop passes
// empty, but its ~15 launches still cost ~40 us -- with the three of the several-rank protocol (LM_RUN_AHEAD) a fifth of a C2-sized
// solve.  The host queues a tick in ~45 us, so ONE tick of lead keeps the device busy (measured, round 5: C2 8 030 it/s with 1, 8 064
// with 3, 7 625 with 0; C3 3 195 / 3 188 / 3 147; a 4-evaluation C2 solve 0.637 ms against 0.685).  SATBA_RUN_AHEAD overrides.
static int lm_run_ahead_single() {
    static const int v = getenv("SATBA_RUN_AHEAD") ? std::max(0, std::min(8, atoi(getenv("SATBA_RUN_AHEAD")))) : 1;
    return v;
}

// queue ticks until the device reports that the loop has left LM_RUN, lm_run_ahead_single() beyond its last report
static int lm_drive(satba_problem* p, double lam_floor, long long max_ticks) {
    long long sub_served = 0;
    p->scales_by_tail = false;  // the first tick of a run launches k_lin_scales itself
    for (;;) {
        // every evaluation and every repeated factorisation is one pattern: a loop that queues many more has lost track of the device
        if (p->lm_ticks_queued > max_ticks || p->lm_ticks_queued >= LM_MAX_TICKS) return fail(SATBA_E_STATE, "device-resident loop: %lld launch patterns queued without reaching the end", p->lm_ticks_queued);
        TRY(lm_queue_tick(p, lam_floor));
        // watchdog: a tick is milliseconds of device work; a minute without a report means the device is stuck
        auto t_wait = std::chrono::steady_clock::now();
        // (a profiled run -- HIP events around every k_linearize launch -- does not run ahead: no switched-off launch is timed)
        unsigned long long w;
        while (lm_summary_tick(w = __atomic_load_n(&p->h_lm->word, __ATOMIC_ACQUIRE)) + (p->prof_lin ? 0 : lm_run_ahead_single()) < p->lm_ticks_queued) {
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
            if (ms_since(t_wait) > 60000.0) return fail(SATBA_E_HIP, "device-resident loop: no progress report from the device for 60 s");
        }
        const int phase = lm_summary_phase(w);
        const long long req = lm_stamp_value(__atomic_load_n(&p->h_lm->sub_requests, __ATOMIC_ACQUIRE));
        if (req > sub_served) {  // the loop has paused for the degenerate-subspace pattern (the ticks queued behind the pause are switched off)
            sub_served = req;
            TRY(lm_launch_sub_pattern(p));
            ++p->lm_ticks_queued;
            continue;
        }
        if (phase == LM_NEED_HOST) {
            // the factorisation beside the pair kernel timed out (the two kernels did not run at the same time): sequential fronts from
            // here on, and the loop carries on at the front that was lost -- nothing of it was booked (lm_decide1a)
            LmDev st;
            TRY(lm_read_state(p, &st));  // (waits for the stream: every queued tick has passed)
            if (st.host_reason != LM_HOST_BESIDE || !p->beside_last) return 0;
            beside_disable(p);
            hipLaunchKernelGGL(k_lm_resume_front, dim3(1), dim3(1), 0, p->stream, p->d_lm);
            HIP_TRY(hipGetLastError());
            __atomic_store_n(&p->h_lm->word, ((unsigned long long)st.tick << 8) | (unsigned long long)LM_RUN, __ATOMIC_RELEASE);
            p->lm_ticks_queued = st.tick;
            p->scales_by_tail = false;  // (the repeated front's linearisation clears its header itself)
            continue;
        }
        if (phase != LM_RUN && phase != LM_NEED_SUB) return 0;
    }
}

int satba_lm_run(satba_problem* p, int64_t n_iterations, int32_t cycle_len, double lam_floor, double* out, int32_t n_out) {
    if (!p || n_iterations <= 0 || cycle_len < 0 || (out && n_out < 16)) return fail(SATBA_E_ARG, "bad argument");
    if (!lm_device_loop_ok(p)) return fail(SATBA_E_ARG, "satba_lm_run drives a single-rank handle with the default dense solver");
    if (cycle_len > 0 && !p->d_x0) return fail(SATBA_E_STATE, "satba_lm_run with cycles needs a kept point (satba_snapshot_x)");
    HIP_TRY(hipSetDevice(p->device));
    satba_lm_opts o{};
    o.max_nfev = -1;
    TRY(lm_reset(p, &o, true, true, false, n_iterations, cycle_len));
    TRY(lm_drive(p, lam_floor, 24 * n_iterations + 1000));
    if (out) return satba_lm_state(p, out, n_out);
    HIP_TRY(hipStreamSynchronize(p->stream));
    return 0;
}

// ---- the device-resident loop for SEVERAL ranks.  The exchange buffer has to be all-reduced five times inside a tick (DESIGN.md
// section 5) and the collectives are the caller's (torch.distributed on the handle's stream), so the tick comes in parts; the caller
// queues   part 0 | all-reduce(linearize payload) | 1 | all-reduce(header) | 2 | all-reduce(S, rhs) | 3 | all-reduce(header) | 4 |
// all-reduce(header) | 5   without waiting for anything: the decisions between the parts are the same one-thread kernels as for one
// rank, on all-reduced scalars -- every rank decides the same.  The degenerate-subspace pattern: parts 6 | all-reduce(header) | 7 |
// all-reduce(header) | 8 | all-reduce(header) | 9.  A switched-off part leaves the buffer alone; its all-reduce is still issued (the
// ranks' collectives must match) and moves stale numbers nobody reads.  satba_lm_poll: the device's progress report (pinned memory,
// no wait): [0] patterns executed, [1] phase, [2] pauses for the subspace pattern so far, [3] tick of the latest pause, [4] tick at
// which the loop left LM_RUN (0: still running).  The caller must queue exactly out[4] + LM_RUN_AHEAD patterns (satba/trf.py).
int satba_lm_begin(satba_problem* p, const satba_lm_opts* o, int32_t never_stop, int64_t max_iterations, int32_t cycle_len) {
    if (!p || !o || max_iterations < 0 || cycle_len < 0) return fail(SATBA_E_ARG, "bad argument");
    if (p->n_c > 1024) return fail(SATBA_E_ARG, "the device-resident loop needs a reduced system of at most 1024 unknowns");
    if (cycle_len > 0 && !p->d_x0) return fail(SATBA_E_STATE, "cycles need a kept point (satba_snapshot_x)");
    HIP_TRY(hipSetDevice(p->device));
    p->loss = o->loss; p->f_scale = o->f_scale; p->lin_grid = lin_grid_for(p);
    return lm_reset(p, o, never_stop != 0, true, false, max_iterations, cycle_len);
}

int satba_lm_part(satba_problem* p, int32_t part, double lam_floor) {
    if (!p || part < 0 || part > 12) return fail(SATBA_E_ARG, "bad argument");
    HIP_TRY(hipSetDevice(p->device));
    LmDev* st = p->d_lm;
    switch (part) {
        case 0: return linearize_impl(p, lm_ctx(p, &st->run_lin));
        case 1: return prepare_impl(p, lm_ctx(p, &st->run_lin), 0);
        case 2: return schur_impl(p, lm_ctx(p, &st->run_solve), FrontCtx{}, 0.0, true, -1.0, lam_floor);
        case 3: return solve_impl(p, lm_ctx(p, &st->run_solve));
        case 4: {
            PhaseCtx c = lm_ctx(p, &st->run_trial);
            c.decide1a_in_trial = true;  // k_lm_decide1a rides in the trial's first launch (launch_trial)
            return trial_impl(p, c, true, 0.0, 0.0);
        }
        // the solve phase with the all-reduce of S in messages (trf.drive_device_loop): 10 begin, 11 message lam_floor has arrived, 12 end
        case 10: return solve_messages_begin_impl(p, &st->run_solve, p->msg_packed, lam_floor != 0.0 ? 1 : 0);
        case 11: return solve_messages_arrived_impl(p, &st->run_solve, p->msg_packed, (int)lam_floor);
        case 12: return solve_messages_end_impl(p, &st->run_solve);
        case 6: return subspace_impl(p, lm_ctx(p, &st->run_sub), 0.0, 0.0);
        case 7:
            hipLaunchKernelGGL(k_lm_decide1b, dim3(1), dim3(1), 0, p->stream, st, p->d_xb);
            return subspace_products_impl(p, lm_ctx(p, &st->run_prod));
        case 8:
            hipLaunchKernelGGL(k_lm_decide1c, dim3(1), dim3(1), 0, p->stream, st, p->d_xb);
            return trial_impl(p, lm_ctx(p, &st->run_trial), true, 0.0, 0.0);
        default: break;  // 5, 9: decision, accepted point into place
    }
    hipLaunchKernelGGL(k_lm_decide2, dim3(1), dim3(1), 0, p->stream, st, p->d_xb, p->h_lm_dev);
    lm_launch_accept(p);
    HIP_TRY(hipGetLastError());
    lm_pattern_queued(p);
    return 0;
}

int satba_lm_poll(satba_problem* p, int64_t* out, int32_t n) {
    if (!p || !out || n < 5) return fail(SATBA_E_ARG, "bad argument");
    // the four words are stored one by one without a fence (LmSummary): a snapshot is consistent when none of the three stamped
    // words is older than the tick in `word` -- every rank then acts on values at least as new as the tick it acts on
    for (int tries = 0;; ++tries) {
        const unsigned long long w = __atomic_load_n(&p->h_lm->word, __ATOMIC_ACQUIRE);
        const unsigned long long sr = __atomic_load_n(&p->h_lm->sub_requests, __ATOMIC_ACQUIRE);
        const unsigned long long stk = __atomic_load_n(&p->h_lm->sub_tick, __ATOMIC_ACQUIRE);
        const unsigned long long etk = __atomic_load_n(&p->h_lm->end_tick, __ATOMIC_ACQUIRE);
        const long long t = lm_summary_tick(w);
        if (lm_stamp_tick(sr) >= t && lm_stamp_tick(stk) >= t && lm_stamp_tick(etk) >= t) {
            out[0] = t; out[1] = lm_summary_phase(w);
            out[2] = lm_stamp_value(sr); out[3] = lm_stamp_value(stk); out[4] = lm_stamp_value(etk);
            return 0;
        }
        if (tries > 1000000) return fail(SATBA_E_HIP, "device-resident loop: the progress report stays inconsistent");
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
}

int satba_lm_state(satba_problem* p, double* out, int32_t n) {
    if (!p || !out || n < 16) return fail(SATBA_E_ARG, "bad argument");
    HIP_TRY(hipSetDevice(p->device));
    LmDev st;
    TRY(lm_read_state(p, &st));
    for (int i = 0; i < n; ++i) out[i] = 0.0;
    out[0] = st.cost; out[1] = st.cost_new; out[2] = st.Delta; out[3] = st.accepted_total; out[4] = st.interior_total;
    out[5] = st.predicted; out[6] = st.actual; out[7] = st.reg; out[8] = st.phase; out[9] = st.status; out[10] = (double)st.nfev;
    out[11] = (double)st.njev; out[12] = (double)st.iterations; out[13] = (double)st.tick; out[14] = st.host_reason; out[15] = st.g_norm;
    if (n > 16) out[16] = st.initial_cost;
    return 0;
}

// The loop of satba/trf.py on the host (scipy's trf_no_bounds with an exact damped step).  resume: a front has already run on the
// device for the current x (first iteration iff resume->first) and its header is in the exchange buffer, but nothing of it is
// booked -- the device-resident loop stopped there because the fixed-point camera sums overflowed (the host switches the route).
static int lm_host_loop(satba_problem* p, const satba_lm_opts* o, satba_lm_stats* out, const LmDev* resume) {
    const int64_t max_nfev = o->max_nfev > 0 ? o->max_nfev : p->n_total * 100;
    std::vector<double> hbuf((size_t)p->hdr), tbuf((size_t)p->hdr);
    double* h = hbuf.data();
    const double* keep = h + SATBA_HDR_KEEP;
    double cost, g_norm, Delta, initial_cost;
    int64_t nfev = 1, njev = 1, iterations = 0;
    int status = -1;
    double step_norm = 0.0, actual = 0.0;
    bool have_actual = false;
    if (!resume) {
        TRY(lm_front(p, true, 0.0, 0.0, h));
        cost = keep[SATBA_KEEP_COST]; g_norm = keep[SATBA_KEEP_GINF]; Delta = keep[SATBA_KEEP_DELTA];
        initial_cost = cost;
    } else {
        const bool first = resume->first != 0;
        Delta = resume->Delta;
        TRY(satba_read_header(p, h));
        p->linearized = true; p->have_step = true;
        if (h[SATBA_HDR_FX_BAD] != 0.0 && p->cam_sums_lds) {
            TRY(satba_camera_sums_fallback(p));
            TRY(lm_front(p, first, Delta, 0.0, h));
        }
        cost = keep[SATBA_KEEP_COST]; g_norm = keep[SATBA_KEEP_GINF];
        if (first) { Delta = keep[SATBA_KEEP_DELTA]; initial_cost = cost; }
        else {
            initial_cost = resume->initial_cost;
            nfev = resume->nfev; njev = resume->njev + 1; iterations = resume->iterations; status = resume->status;
            step_norm = resume->step_norm; actual = resume->actual; have_actual = resume->have_actual != 0;
        }
    }
    if (!std::isfinite(cost)) return fail(SATBA_E_NONFINITE, "Residuals are not finite in the initial point.");
    if (o->verbose >= 2) printf("%15s%15s%15s%15s%15s%15s\n", "Iteration  ", "Total nfev  ", "Cost     ", "Cost reduction ", "Step norm   ", "Optimality  ");
    for (;;) {
        if (g_norm < o->gtol) status = 1;
        if (o->verbose >= 2) {
            if (have_actual) printf("%10lld     %10lld     %15.4e%15.2e%15.2e%15.2e\n", (long long)iterations, (long long)nfev, cost, actual, step_norm, g_norm);
            else printf("%10lld     %10lld     %15.4e%30s%15.2e\n", (long long)iterations, (long long)nfev, cost, "", g_norm);
        }
        if (status != -1 || nfev == max_nfev) break;
        double reg = keep[SATBA_KEEP_LAM];
        bool exhausted;
        TRY(lm_refactorise(p, h, reg, exhausted));
        if (exhausted) return fail(SATBA_E_STATE, "reduced camera system could not be factorised");
        LmModel md;
        TRY(lm_subspace_model(p, h, tbuf.data(), reg, keep[SATBA_KEEP_JG_SQ], md));

        actual = -1.0;
        while (actual <= 0 && nfev < max_nfev) {
            LmTrial t;
            TRY(lm_trial(p, md, Delta, tbuf.data(), t));
            ++nfev;
            if (!std::isfinite(t.cost_new)) { Delta = 0.25 * t.step_h_norm; continue; }
            actual = cost - t.cost_new;
            double ratio;
            const double Delta_new = satba_lm::update_tr_radius(Delta, actual, t.predicted, t.step_h_norm, t.step_h_norm > 0.95 * Delta, ratio);
            step_norm = std::sqrt(tbuf[SATBA_HDR_STEP_SQ]);
            const int term = satba_lm::check_termination(actual, cost, step_norm, std::sqrt(tbuf[SATBA_HDR_X_SQ]), ratio, o->ftol, o->xtol);
            if (term) { status = term; break; }
            Delta = Delta_new;
        }
        have_actual = true;
        if (actual > 0) {
            TRY(satba_accept(p));
            TRY(lm_front(p, false, Delta, 0.0, h));
            cost = keep[SATBA_KEEP_COST]; g_norm = keep[SATBA_KEEP_GINF];
            ++njev;
        } else {
            step_norm = 0.0; actual = 0.0;
            if (status == -1 && nfev < max_nfev) TRY(lm_front(p, false, Delta, 0.0, h));
        }
        ++iterations;
    }
    if (status == -1) status = 0;
    out->cost = cost; out->initial_cost = initial_cost; out->optimality = g_norm;
    out->nfev = nfev; out->njev = njev; out->iterations = iterations; out->status = status;
    return 0;
}

int satba_solve_lm(satba_problem* p, const satba_lm_opts* o, satba_lm_stats* out) {
    Range range_("satba:solve_lm");
    if (!p || !o || !out) return fail(SATBA_E_ARG, "null argument");
    if (p->world != 1) return fail(SATBA_E_ARG, "satba_solve_lm drives a single-rank handle (world = %d): use the phase entry points", p->world);
    memset(out, 0, sizeof *out);
    HIP_TRY(hipSetDevice(p->device));
    TRY(satba_configure(p, o->loss, o->f_scale));
    bool done = false;
    if (lm_device_loop_ok(p) && lm_device_loop_pays(p) && o->verbose < 2) {
        // the decisions are taken on the device; the host queues ticks LM_RUN_AHEAD beyond the last one the device has reported and
        // watches the summary the device posts into pinned memory
        TRY(lm_reset(p, o, false, true));
        TRY(lm_drive(p, 0.0, 24 * (o->max_nfev > 0 ? o->max_nfev : p->n_total * 100) + 1000));
        LmDev st;
        TRY(lm_read_state(p, &st));
        if (st.phase == LM_DONE) {
            if (!std::isfinite(st.initial_cost)) return fail(SATBA_E_NONFINITE, "Residuals are not finite in the initial point.");
            out->cost = st.cost; out->initial_cost = st.initial_cost; out->optimality = st.g_norm;
            out->nfev = st.nfev; out->njev = st.njev; out->iterations = st.iterations; out->status = st.status == -1 ? 0 : st.status;
            done = true;
        } else if (st.host_reason == LM_HOST_NONFINITE) {
            return fail(SATBA_E_NONFINITE, "Residuals are not finite in the initial point.");
        } else if (st.host_reason == LM_HOST_CHOL) {
            return fail(SATBA_E_STATE, "reduced camera system could not be factorised");
        } else if (st.host_reason == LM_HOST_BESIDE) {
            // lm_drive resumes a handed-back concurrent front itself; it only returns with this reason when the front it handed back was
            // NOT concurrent (p->beside_last false) -- which lm_decide1a no longer raises (SATBA_CHOL_BESIDE_WAIT): an inconsistency, not a route change
            return fail(SATBA_E_STATE, "device-resident loop handed back a front that did not run beside the pair kernel");
        } else {
            TRY(lm_host_loop(p, o, out, &st));  // LM_HOST_FX, fixed-point overflow of the camera sums: the host switches the route and carries on
            done = true;
        }
    }
    if (!done) TRY(lm_host_loop(p, o, out, nullptr));
    if (o->verbose >= 1) {
        static const char* msg[] = {"The maximum number of function evaluations is exceeded.", "`gtol` termination condition is satisfied.",
                                    "`ftol` termination condition is satisfied.", "`xtol` termination condition is satisfied.",
                                    "Both `ftol` and `xtol` termination conditions are satisfied."};
        printf("%s\nFunction evaluations %lld, initial cost %.4e, final cost %.4e, first-order optimality %.2e.\n", msg[out->status], (long long)out->nfev,
               out->initial_cost, out->cost, out->optimality);
    }
    return 0;
}

// satba_lm_scalars (include/satba.h): stand-alone (no handle).  The scalar functions of satba_lm.h as this library carries them, once per
// row: device == 0 the host compilation, device == 1 the device compilation (one thread per row on the default stream of the current device).
extern "C++" {
namespace {
__global__ void k_lm_scalars(long long n, const double* __restrict__ in, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) satba_lm::lm_scalars_row(in + 6 * i, out + 6 * i);
}
}  // namespace
}  // extern "C++"
int satba_lm_scalars(int32_t device, int64_t n, const double* in, double* out) {
    if (device != 0 && device != 1) return fail(SATBA_E_ARG, "device must be 0 (host compilation) or 1 (device compilation)");
    if (n < 0 || n > (1ll << 24)) return fail(SATBA_E_ARG, "between 0 and 2^24 rows");
    if (n == 0) return 0;
    if (!in || !out) return fail(SATBA_E_ARG, "null argument");
    if (device == 0) {
        for (int64_t i = 0; i < n; ++i) satba_lm::lm_scalars_row(in + 6 * i, out + 6 * i);
        return 0;
    }
    const size_t bytes = sizeof(double) * 6 * (size_t)n;
    double *d_in = nullptr, *d_out = nullptr;
    DevAllocs tmp;
    TRY(tmp.alloc(&d_in, 6 * (size_t)n));
    TRY(tmp.alloc(&d_out, 6 * (size_t)n));
    HIP_TRY(hipMemcpy(d_in, in, bytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_lm_scalars, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t) nullptr, (long long)n, d_in, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost));  // (waits for the kernel: the default stream)
    return 0;
}

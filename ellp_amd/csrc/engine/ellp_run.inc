// ellp_run.inc — ellp_engine_run: which loop a slice runs (k_small / k_mid, the exact loop above 1,024 rows, the
// explicit-inverse loop with look-ahead or polled read-backs), the certified hybrid's hand-over to the exact kernels
// (exact_takeover, exact_certify_large), certify-or-redo from the snapshot of the phase's start, and the budget close of the
// two-launch pipeline; with them ensure_inverse, ellp_engine_refresh and ellp_engine_refactor.  Host code only: what it
// launches, and the pieces its re-arms are made of, are in ellp_launch.inc.  Included inside extern "C", behind creation
// (engine_create_impl) and in front of the entry points that call ensure_inverse (read_point, tap, the sharding API) and of
// the phase hand-offs (ellp_phase.inc).

// The explicit-inverse engine is about to be used on an engine that has been running k_small: build
// B^-1 from the current A_B and leave the small path for good.
static ellp_status ensure_inverse(ellp_engine *e, char *errbuf, size_t errlen) {
    if (e->dual_bflip) {  // the caller must be able to tell which rule runs: the explicit-inverse engine has no long-step ratio test
        set_err(errbuf, errlen, "ELLP_FLAG_DUAL_BOUND_FLIPPING: this call needs the explicit-inverse engine, which has no long-step ratio test");
        return ELLP_ERR_ARG;
    }
    launch_flush(e);  // two-launch pipeline: B^-1 is complete only once the open iteration has been booked
    if (e->w_valid) {
        e->small = false;
        return ELLP_OPTIMAL;
    }
    HIPCHK(hipSetDevice(e->device));
    launch_refactor(e);
    HIPCHK(read_state(e));
    prof_collect(e);
    e->w_valid = true;
    e->small = false;
    e->need_dleave = true;
    e->u_valid = false;
    if (e->h_st->status != ST_RUNNING) return status_message(*e->h_st, errbuf, errlen);
    return ELLP_OPTIMAL;
}

// one launch of the LU-per-iteration kernel of ellp_mid.inc for up to `iters` loop bodies (run_small; exact_takeover)
static hipError_t launch_mid(ellp_engine *e, uint64_t iters, int resync) {
    const int64_t per = (int64_t)e->nbs * e->cpb;  // layout of the pricing buffer (Xchg, one segment)
    MidArgs a{};
    a.A_B = e->A_B; a.A_N = e->A_N; a.A_Nt = e->A_Nt; a.c_B = e->c_B; a.c_N = e->c_N; a.x = e->x; a.y = e->y; a.dd = e->dd;
    a.lb = e->lb; a.ub = e->ub; a.kind = e->kindv; a.B_index = e->B_index; a.N_index = e->N_index; a.Nb = e->Nb;
    a.kbuf = e->X + 2 * e->nbs;
    a.rbuf = e->X + 2 * e->nbs + per;
    a.LUa = e->LUa; a.Ut = e->Ut;
    a.st = e->st; a.m = e->m; a.ld = e->ld; a.nN = e->nN; a.ldn = e->ldn;
    a.max_iters = iters;
    a.nch = (int)((e->nN + 63) / 64);
    a.eps = e->eps;
    a.trace = trace_of(e);
    a.stamps = e->small_stamps;
    a.maxviol = e->dual_maxviol;
    a.bflip = e->dual_bflip;
    a.flist = e->bf_list;
    a.resync = resync;
    a.b = e->b_dev;
    // the row-major copy of A_N the pricing pass reads: made afresh at every launch (anything may have
    // touched A_N in between: a hand-off, a sharding call, the other engine)
    hipLaunchKernelGGL(k_mid_transpose, dim3((unsigned)((e->m + 31) / 32), (unsigned)((e->nN + 31) / 32)), dim3(256), 0,
                       e->stream, e->A_N, e->A_Nt, e->m, e->ld, e->nN, e->ldn);
    void *kargs[] = {&a};
    return hipLaunchKernel(mid_kernel(e->kind, e->mid_nt), dim3(1), dim3((unsigned)e->mid_nt), kargs, e->mid_lds, e->stream);
}

// ellp_engine_run for the small path: launches of k_small, each good for up to 16384 iterations
static ellp_status run_small(ellp_engine *e, uint64_t max_iters, char *errbuf, size_t errlen) {
    HIPCHK(read_state(e));
    if (e->h_st->status != ST_RUNNING) return status_message(*e->h_st, errbuf, errlen);
    const uint64_t iters0 = e->h_st->iters;
    uint64_t remaining = max_iters;
    const int64_t per = (int64_t)e->nbs * e->cpb;  // layout of the pricing buffer (Xchg, one segment)
    while (remaining > 0) {
        if (e->mid) {
            HIPCHK(launch_mid(e, remaining < 4096 ? remaining : 4096, 0));
        } else {
            SmallArgs a{};
            a.A_B = e->A_B; a.A_N = e->A_N; a.c_B = e->c_B; a.c_N = e->c_N; a.x = e->x; a.y = e->y; a.dd = e->dd;
            a.lb = e->lb; a.ub = e->ub; a.kind = e->kindv; a.B_index = e->B_index; a.N_index = e->N_index; a.Nb = e->Nb;
            a.kbuf = e->X + 2 * e->nbs;
            a.rbuf = e->X + 2 * e->nbs + per;
            a.st = e->st; a.m = e->m; a.ld = e->ld; a.nN = e->nN;
            a.max_iters = remaining < 16384 ? remaining : 16384;
            a.nch = (int)((e->nN + 63) / 64);
            a.eps = e->eps;
            a.trace = trace_of(e);
            a.stamps = e->small_stamps;
            a.maxviol = e->dual_maxviol;
            a.bflip = e->dual_bflip;
            a.flist = e->bf_list;
            void *kargs[] = {&a};
            HIPCHK(hipLaunchKernel(small_kernel(e->kind, e->small_nt), dim3(1), dim3((unsigned)e->small_nt), kargs,
                                   e->small_lds, e->stream));
        }
        HIPCHK(hipGetLastError());
        HIPCHK(read_state(e));
        e->refactors = e->h_st->iters;  // one LU per loop body, as the reference
        if (e->h_st->status != ST_RUNNING) return status_message(*e->h_st, errbuf, errlen);
        const uint64_t done = e->h_st->iters - iters0;
        remaining = done < max_iters ? max_iters - done : 0;
    }
    return ELLP_MAXITER;
}

double ellp_engine_refresh(ellp_engine *e) {
    if (e) e->hst_fresh = false;  // anything but ellp_engine_run may change the device state behind h_st
    if (!e) return NAN;
    if (hipSetDevice(e->device) != hipSuccess) return NAN;
    if (ensure_inverse(e, nullptr, 0) != ELLP_OPTIMAL) return NAN;
    launch_refresh(e);
    if (read_state(e) != hipSuccess) return NAN;
    prof_collect(e);
    const double res = e->h_st->resid;
    e->last_residual = res;
    if (e->h_st->need_rebuild) {  // an explicit refresh that was refused changes nothing and stops nothing
        const int32_t zero = 0;
        (void)hipMemcpyAsync(&e->st->need_rebuild, &zero, sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
        (void)hipMemcpyAsync(&e->st->tiny, &zero, sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
        (void)hipStreamSynchronize(e->stream);
        e->h_st->need_rebuild = 0;
        e->h_st->tiny = 0;
    }
    return res;
}

ellp_status ellp_engine_refactor(ellp_engine *e, char *errbuf, size_t errlen) {
    if (e) e->hst_fresh = false;  // anything but ellp_engine_run may change the device state behind h_st
    if (!e) return ELLP_ERR_ARG;
    HIPCHK(hipSetDevice(e->device));
    e->w_valid = true;  // about to be
    e->small = false;
    e->need_dleave = true;
    launch_flush(e);
    launch_refactor(e);
    HIPCHK(read_state(e));
    prof_collect(e);
    if (e->h_st->status != ST_RUNNING) return status_message(*e->h_st, errbuf, errlen);
    return ELLP_OPTIMAL;
}

static ellp_status run_colsharded(ellp_engine *e, uint64_t max_iters, ellp_stats *stats, char *errbuf, size_t errlen);

// ---- "certify or redo" (certified hybrid): the start of a phase is kept on the host; a solve that ends Optimal on a point
// that violates an invariant of the reference's loop (see k_invariants) is repeated from that start by the exact kernel
static hipError_t take_snapshot(ellp_engine *e) {
    auto &sn = e->snap;
    const size_t m = (size_t)e->m, nN = (size_t)e->nN, n_c = (size_t)e->n_c;
    sn.x.resize(n_c); sn.B.resize(m); sn.N.resize(nN); sn.Nb.resize(nN); sn.c_B.resize(m); sn.c_N.resize(nN);
    hipError_t rc;
#define SNAP(dst, src, bytes) if ((rc = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, e->stream)) != hipSuccess) return rc
    SNAP(sn.x.data(), e->x, 8 * n_c);
    SNAP(sn.B.data(), e->B_index, 8 * m);
    SNAP(sn.N.data(), e->N_index, 8 * nN);
    SNAP(sn.Nb.data(), e->Nb, nN);
    SNAP(sn.c_B.data(), e->c_B, 8 * m);
    SNAP(sn.c_N.data(), e->c_N, 8 * nN);
    if (e->kind == ELLP_ENGINE_DUAL) {
        sn.y.resize(m); sn.d.resize(n_c);
        SNAP(sn.y.data(), e->y, 8 * m);
        SNAP(sn.d.data(), e->dd, 8 * n_c);
    }
    SNAP(&sn.obj, &e->st->obj, sizeof(double));
#undef SNAP
    if ((rc = hipStreamSynchronize(e->stream)) != hipSuccess) return rc;
    sn.valid = true;
    return hipSuccess;
}

// true if the end point keeps the invariants of the reference's loop to within EPS (or cannot be examined)
static bool end_point_ok(ellp_engine *e, double *detail3) {
    if (!e->inv_out && dmalloc(e, &e->inv_out, 4) != hipSuccess) {
        (void)hipGetLastError();
        return true;
    }
    InvArgs a{e->x, e->lb, e->ub, e->b_dev, e->y, e->dd, e->kindv, e->Nb, e->N_index, e->m, e->n_c, e->nN,
              e->kind == ELLP_ENGINE_DUAL ? 1 : 0, e->inv_out};
    hipLaunchKernelGGL(k_invariants, dim3(1), dim3(1024), 0, e->stream, a);
    double out[3] = {0.0, 0.0, 0.0};
    if (hipMemcpyAsync(out, e->inv_out, sizeof(out), hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
        hipStreamSynchronize(e->stream) != hipSuccess) {
        (void)hipGetLastError();
        return true;
    }
    if (detail3) { detail3[0] = out[0]; detail3[1] = out[1]; detail3[2] = out[2]; }
    if (e->kind == ELLP_ENGINE_PRIMAL) return out[0] <= e->eps;
    if (!(out[1] <= e->eps)) return false;
    // a box problem's dual objective (= minus the original problem's dual infeasibility, the number the caller tests against
    // EPS, dual…:45-50) that lies BELOW -EPS but within what the drift of the carried d can produce: the exact loop decides
    if (e->box_problem && out[2] <= -e->eps && out[2] > -1e-6) return false;
    return true;
}

// back to the start of the phase, and from now on the LU-per-iteration kernel alone (ellp_mid.inc; `large`: run_exact_large)
static ellp_status redo_from_snapshot(ellp_engine *e, bool large, char *errbuf, size_t errlen) {
    const auto &sn = e->snap;
    const int64_t m = e->m, nN = e->nN, ld = e->ld;
    std::vector<int64_t> B((size_t)m), N((size_t)nN), where((size_t)e->n, INT64_MIN), src((size_t)(m + nN));
    HIPCHK(hipMemcpy(B.data(), e->B_index, 8 * (size_t)m, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(N.data(), e->N_index, 8 * (size_t)nN, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < m; ++i) where[(size_t)B[(size_t)i]] = i;
    for (int64_t j = 0; j < nN; ++j) where[(size_t)N[(size_t)j]] = -1 - j;
    for (int64_t i = 0; i < m; ++i) src[(size_t)i] = where[(size_t)sn.B[(size_t)i]];
    for (int64_t j = 0; j < nN; ++j) src[(size_t)(m + j)] = where[(size_t)sn.N[(size_t)j]];
    for (int64_t k = 0; k < m + nN; ++k)
        if (src[(size_t)k] == INT64_MIN) {
            set_err(errbuf, errlen, "redo: the index sets of the snapshot and of the engine differ");
            return ELLP_ERR_PANIC;
        }
    {
        DevTemp<double> A2(e->stream);  // both freed, behind a drained stream, before the rebuild below
        DevTemp<int64_t> src_dev(e->stream);
        HIPCHK(A2.alloc((size_t)(ld * (m + nN))));
        HIPCHK(src_dev.alloc((size_t)(m + nN)));
        HIPCHK(hipMemcpyAsync(src_dev.p, src.data(), 8 * (size_t)(m + nN), hipMemcpyHostToDevice, e->stream));
        hipLaunchKernelGGL(k_restore_cols, dim3((unsigned)(m + nN)), dim3(256), 0, e->stream, e->A_B, e->A_N, src_dev.p, A2.p, ld);
        HIPCHK(hipMemcpyAsync(e->A_B, A2.p, sizeof(double) * (size_t)(ld * m), hipMemcpyDeviceToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->A_N, A2.p + ld * m, sizeof(double) * (size_t)(ld * nN), hipMemcpyDeviceToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->x, sn.x.data(), 8 * (size_t)e->n_c, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->B_index, sn.B.data(), 8 * (size_t)m, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->N_index, sn.N.data(), 8 * (size_t)nN, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->Nb, sn.Nb.data(), (size_t)nN, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->c_B, sn.c_B.data(), 8 * (size_t)m, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->c_N, sn.c_N.data(), 8 * (size_t)nN, hipMemcpyHostToDevice, e->stream));
        if (e->kind == ELLP_ENGINE_DUAL) {
            HIPCHK(hipMemcpyAsync(e->y, sn.y.data(), 8 * (size_t)m, hipMemcpyHostToDevice, e->stream));
            HIPCHK(hipMemcpyAsync(e->dd, sn.d.data(), 8 * (size_t)e->n_c, hipMemcpyHostToDevice, e->stream));
        }
        // the phase's solve_with_initial starts again: every group but the pricing window (a certifying engine has none:
        // the plan certifies with pp_P <= 1 only)
        DevState ns = *e->h_st;
        clear_stop_words(ns);
        clear_relays(ns);
        clear_open_iteration(ns);
        ns.se_valid = 0;
        clear_counts(ns);
        ns.lambda = 0.0;
        ns.obj = sn.obj;
        ns.lr = -1;
        HIPCHK(store_state(e, ns));
        if (e->trace_len > 0) HIPCHK(hipMemsetAsync(e->trace_it, 0, sizeof(unsigned long long) * (size_t)e->trace_len, e->stream));
    }
    if (large) {
        // above 1,024 rows the exact loop is run_exact_large; the explicit inverse follows the restored basis (the exact
        // iterations keep updating it, and the next phase's fast loop starts from it)
        e->exact_large_only = true;
        launch_refactor(e);
        HIPCHK(read_state(e));
        prof_collect(e);
        e->hy_rebuilds += 1;
        if (e->h_st->status != ST_RUNNING) return status_message(*e->h_st, errbuf, errlen);
    } else {
        e->hybrid = false;
        e->small = true;
        e->mid = true;
        e->w_valid = false;
        e->lagged = false;
        e->dual_fused = e->dual_fold = false;
    }
    e->lag_open = e->dual_open = false;
    e->u_valid = false;
    e->need_dleave = true;
    nothing_enqueued(e, 0);  // the same phase again: its snapshot stays, and exact_large_only is this function's to set
    e->since_refactor = e->since_btran = e->since_drift = 0;
    e->hy_redos += 1;
    return ELLP_OPTIMAL;
}

// One iteration with u / rho and B^-1 a_q from a fresh LU of the CURRENT basis (ellp_exact.inc), enqueued; the state is complete
// afterwards.  The workspace must be there (exact_workspace) and the caller has switched the pivot guard off (guard_off).
static void enqueue_exact_iteration(ellp_engine *e) {
    const int64_t m = e->m, ld = e->ld;
    const unsigned gm = (unsigned)((m + 255) / 256), gld = (unsigned)((ld + 255) / 256);
    const size_t lds0 = sizeof(double) * (size_t)m, lds1 = 2 * sizeof(double) * (size_t)m;
    const bool was_lagged = e->lagged, was_fused = e->dual_fused, was_fold = e->dual_fold;
        hipLaunchKernelGGL(k_rows_from_cols, dim3((unsigned)((m + 31) / 32), (unsigned)((m + 31) / 32)), dim3(256), 0, e->stream, e->A_B, e->luw.M, m, ld);
        ellp_lu_rows_factor(&e->luw, e->stream);
        if (e->kind == ELLP_ENGINE_PRIMAL) {
            hipLaunchKernelGGL(k_lu_solve, dim3(1), dim3(1024), lds1, e->stream, e->luw.M, e->luw.piv, m, e->c_B, e->ex_sol, 1, e->ex_fail);
            hipLaunchKernelGGL(k_exact_put_u, dim3(gld), dim3(256), 0, e->stream, e->ex_sol, e->u, m, ld, e->ex_fail);
            e->lagged = false;
            launch_price<0>(e);
            launch_ftran2<0>(e);
            hipLaunchKernelGGL(k_exact_gather_aq, dim3(gm), dim3(256), 0, e->stream, e->A_N, e->st, m, ld, e->ex_rhs);
            hipLaunchKernelGGL(k_lu_solve, dim3(1), dim3(1024), lds0, e->stream, e->luw.M, e->luw.piv, m, e->ex_rhs, e->ex_sol, 0, e->ex_fail);
            ExactLamArgs la{e->ex_sol, e->d, e->lam, e->bidx, e->dpos, e->B_index, e->x, e->lb, e->ub, e->kindv, e->st, m, e->eps, e->ex_fail};
            hipLaunchKernelGGL(k_exact_relam, dim3(gm), dim3(256), 0, e->stream, la);
            launch_update2<0>(e, 1);
            e->lagged = was_lagged;
        } else {
            // x_B = A_B^-1 (b - A_N x_N) from the LU (the kernels of launch_resync form the right-hand side)
            ResyncArgs ra{e->A_N, e->W, e->W2, e->b_dev, e->x, e->xg, e->tvec, e->upart, e->cand, e->maxbits, e->B_index,
                          e->N_index, e->st, e->m, e->ld, e->nN, 0, e->btran_tiles, 1};
            ra.cols_per_tile = (int)((e->nN + e->btran_tiles - 1) / e->btran_tiles);
            const int64_t half = ld >> 1;
            hipLaunchKernelGGL(k_resync_gather, dim3((unsigned)((e->nN + 255) / 256)), dim3(256), 0, e->stream, ra);
            hipLaunchKernelGGL(k_resync_part, dim3((unsigned)((half + 255) / 256), (unsigned)e->btran_tiles), dim3(256), 0, e->stream, ra);
            hipLaunchKernelGGL(k_resync_rhs, dim3(gld), dim3(256), 0, e->stream, ra);
            hipLaunchKernelGGL(k_lu_solve, dim3(1), dim3(1024), lds0, e->stream, e->luw.M, e->luw.piv, m, e->tvec, e->cand, 0, e->ex_fail);
            hipLaunchKernelGGL(k_resync_apply, dim3(gm), dim3(256), 0, e->stream, ra);
            launch_dleave(e);
            hipLaunchKernelGGL(k_exact_unit, dim3(gm), dim3(256), 0, e->stream, e->ex_rhs, m, e->st);
            hipLaunchKernelGGL(k_lu_solve, dim3(1), dim3(1024), lds1, e->stream, e->luw.M, e->luw.piv, m, e->ex_rhs, e->ex_rho, 1, e->ex_fail);
            e->dual_fused = e->dual_fold = false;
            e->price_rho_ovr = e->ex_rho;
            e->dual_seq += 1;
            launch_price<1>(e);
            launch_ftran2<1>(e);
            hipLaunchKernelGGL(k_exact_gather_aq, dim3(gm), dim3(256), 0, e->stream, e->A_N, e->st, m, ld, e->ex_rhs);
            hipLaunchKernelGGL(k_lu_solve, dim3(1), dim3(1024), lds0, e->stream, e->luw.M, e->luw.piv, m, e->ex_rhs, e->ex_sol, 0, e->ex_fail);
            hipLaunchKernelGGL(k_exact_copy, dim3(gm), dim3(256), 0, e->stream, e->ex_sol, e->d, m, e->st, e->ex_fail);
            launch_update2<1>(e, 0);
            e->price_rho_ovr = nullptr;
            e->dual_fused = was_fused;
            e->dual_fold = was_fold;
        }
}

// the LU workspace and the vectors of the exact iteration (allocated at the first use)
static hipError_t exact_workspace(ellp_engine *e) {
    if (e->luw_ready) return hipSuccess;
    const int64_t m = e->m, ld = e->ld;
    hipError_t rc;
    if ((rc = ellp_lu_rows_alloc(&e->luw, m)) != hipSuccess) {
        ellp_lu_rows_free(&e->luw);
        (void)hipGetLastError();
        return rc;
    }
    e->luw_ready = true;
    if ((rc = dmalloc(e, &e->ex_rhs, (size_t)ld)) != hipSuccess) return rc;
    if ((rc = dmalloc(e, &e->ex_sol, (size_t)ld)) != hipSuccess) return rc;
    if ((rc = dmalloc(e, &e->ex_rho, (size_t)ld)) != hipSuccess) return rc;
    if ((rc = dmalloc(e, &e->ex_fail, 4)) != hipSuccess) return rc;
    (void)hipMemsetAsync(e->ex_rho, 0, sizeof(double) * (size_t)ld, e->stream);
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_lu_solve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(16 * m));
    return hipSuccess;
}

// "certify or redo" above 1,024 rows: after a redo every loop body runs on a fresh LU (ellp_engine::exact_large_only) — the
// reference's LU-per-iteration loop on all CUs instead of in one workgroup: a blocked LU (2 ceil(m / 16) launches, ellp_lu.hip) and
// two (primal) / three (dual) solves per iteration; the explicit inverse is still updated along (a later phase goes back to
// the fast loop).  With pipeline 3 (ellp_engine::exact_large_always) this loop is the engine, from the first slice on.
static ellp_status run_exact_large(ellp_engine *e, uint64_t max_iters, char *errbuf, size_t errlen) {
    HIPCHK(exact_workspace(e));
    HIPCHK(read_state(e));
    if (e->h_st->status != ST_RUNNING) return status_message(*e->h_st, errbuf, errlen);
    const uint64_t iters0 = e->h_st->iters;
    e->lag_open = e->dual_open = false;
    e->guard_off = true;
    ellp_status result = ELLP_MAXITER;
    while (e->h_st->iters - iters0 < max_iters) {
        HIPCHK(hipMemsetAsync(e->ex_fail, 0, sizeof(int), e->stream));
        enqueue_exact_iteration(e);
        int failed = 0;
        // not read_state: the LU's failure flag rides along in front of the one synchronisation
        HIPCHK(hipMemcpyAsync(e->h_st, e->st, sizeof(DevState), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipMemcpyAsync(&failed, e->ex_fail, sizeof(int), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipGetLastError());
        prof_collect(e);
        if (failed) {  // a zero on U's diagonal: the reference's unwrap() on None in BTRAN / FTRAN
            set_err(errbuf, errlen, "unwrap() on None: the basis is exactly singular");
            result = ELLP_ERR_PANIC;
            break;
        }
        if (e->h_st->tiny) {  // raised by the update kernel for the explicit inverse's sake: nothing to maintain here
            static const int32_t zero = 0;
            (void)hipMemcpyAsync(&e->st->tiny, &zero, sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
            e->h_st->tiny = 0;
        }
        if (e->h_st->status != ST_RUNNING) {
            result = status_message(*e->h_st, errbuf, errlen);
            break;
        }
    }
    e->guard_off = false;
    e->u_valid = false;
    e->enqueued = 0;
    e->iters_seen = e->h_st->iters;
    e->hy_exact_iters += e->h_st->iters - iters0;
    e->need_dleave = true;
    if (result != ELLP_MAXITER && e->h_st->status != ST_RUNNING) {
        // the solve has ended: the explicit inverse, updated along through pivots no guard has looked at, is rebuilt from
        // the final basis (a phase hand-off and the dual point of read_point read it)
        static const int32_t running = ST_RUNNING;
        static int32_t keep;
        keep = e->h_st->status;
        (void)hipMemcpyAsync(&e->st->status, &running, sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
        launch_refactor(e);
        e->hy_rebuilds += 1;
        DevState after;
        HIPCHK(hipMemcpyAsync(&after, e->st, sizeof(DevState), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        prof_collect(e);
        if (after.status != ST_RUNNING) e->w_valid = false;
        e->h_st->cur = after.cur;
        (void)hipMemcpyAsync(&e->st->status, &keep, sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
        (void)hipMemcpyAsync(&e->st->panic_code, &e->h_st->panic_code, sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
        (void)hipStreamSynchronize(e->stream);
    }
    return result;
}

// The certificate above 1,024 rows (ellp_exact.inc): the explicit-inverse loop has reported a terminal status; one iteration
// is run with u / rho and d = B^-1 a_q from a fresh LU of the basis (dual: x_B recomputed from it first).  Returns as
// exact_takeover does.
static int exact_certify_large(ellp_engine *e, uint64_t remaining, ellp_status *result, char *errbuf, size_t errlen) {
    const int s = e->h_st->status;
    const bool guard = s == ST_NEED_EXACT;  // a refused pivot: nothing of that iteration is committed or counted
    if (!(guard || s == ELLP_OPTIMAL || s == ELLP_INFEASIBLE || s == ELLP_UNBOUNDED)) return 0;
    if (guard && remaining == 0) return 0;  // the slice is used up: the next one starts here
    if (!guard) remaining += 1;  // the loop body that found the status is examined again, not counted twice
    auto fail = [&](hipError_t rc) {
        set_err(errbuf, errlen, "HIP error %s in the certificate of the terminal status", hipGetErrorString(rc));
        *result = ELLP_ERR_DEVICE;
        return 2;
    };
    hipError_t rc;
    if ((rc = exact_workspace(e)) != hipSuccess) {
        e->cert_large = false;  // no memory for the factors: the status goes out uncertified
        e->hy_uncertified += 1;
        return 0;
    }
    // re-arm: the state is complete (a status found by k_ftran_eta comes with that pass's eta update done; one found by a
    // ratio-test fold comes before anything of its iteration is committed); the loop body that found it is not counted twice
    // The counts, lambda and the pricing window go on (the same solve).  se_valid is not cleared here: nothing sets it, the
    // plan certifies without steepest edge only.
    DevState ns = *e->h_st;
    clear_stop_words(ns);
    clear_relays(ns);
    clear_open_iteration(ns);
    ns.usel = ns.usel_next = 0;  // k_exact_put_u writes the first u buffer
    if (!guard && ns.iters > 0) ns.iters -= 1;
    if ((rc = store_state(e, ns)) != hipSuccess) return fail(rc);
    if ((rc = hipMemsetAsync(e->ex_fail, 0, sizeof(int), e->stream)) != hipSuccess) return fail(rc);
    e->guard_off = true;
    e->lag_open = false;
    e->dual_open = false;
    // the first iteration examines the status; if it does NOT confirm it (it pivots), up to exact_K - 1 more follow before the
    // explicit-inverse loop takes over again — the policy of the certified hybrid (oracle/ellp_oracle.c, hybrid_run)
    int failed = 0;
    uint64_t ran = 0;
    int s_first = ST_RUNNING;
    for (int k = 0; k < e->exact_K; ++k) {
        enqueue_exact_iteration(e);
        // not read_state: the LU's failure flag rides along in front of the one synchronisation
        if ((rc = hipMemcpyAsync(e->h_st, e->st, sizeof(DevState), hipMemcpyDeviceToHost, e->stream)) != hipSuccess) return fail(rc);
        if ((rc = hipMemcpyAsync(&failed, e->ex_fail, sizeof(int), hipMemcpyDeviceToHost, e->stream)) != hipSuccess) return fail(rc);
        if ((rc = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(rc);
        if ((rc = hipGetLastError()) != hipSuccess) return fail(rc);
        ran += 1;
        if (k == 0) s_first = e->h_st->status;
        if (e->h_st->status != ST_RUNNING || e->h_st->tiny || failed) break;
        if (ran >= remaining) break;  // the caller's budget
    }
    e->guard_off = false;
    prof_collect(e);
    const int s2 = e->h_st->status;
    e->hy_exact_iters += ran;
    if (failed) e->hy_uncertified += 1;  // an exactly singular basis: the iteration ran on the explicit inverse's numbers
    if (guard) e->hy_guards += 1;
    else {
        e->hy_certs += 1;
        if (s_first != s) e->hy_disagree += 1;
    }
    if (getenv("ELLP_HYBRID_DEBUG"))
        fprintf(stderr, "ellp hybrid: fast status %d at iteration %llu -> exact-LU iteration, status %d%s\n", s,
                (unsigned long long)ns.iters, s2, failed ? " (LU singular: not certified)" : "");
    e->u_valid = false;
    e->since_btran = 0;
    nothing_enqueued(e, e->h_st->iters);
    e->need_dleave = false;
    if (s2 == ST_RUNNING && !e->h_st->tiny) return 1;
    if (s2 == ST_RUNNING) return 1;  // a maintenance request raised by the iteration: the run loop services it
    *result = status_message(*e->h_st, errbuf, errlen);
    return 2;
}

// Certified hybrid (restated in oracle/ellp_oracle.c, hybrid_run): the explicit-inverse loop has stopped — on a guarded
// pivot (ST_NEED_EXACT: nothing of that iteration is committed), on a terminal status, or on an error of its own arithmetic
// (singular rebuild, NaN, an assertion of the reference).  h_st is the drained device state.  The LU-per-iteration kernel
// (k_mid: the reference's arithmetic on a fresh factorisation, primal…:173-189,289-292,404-406; dual…:241-246,281-284)
// runs up to exact_K loop bodies from the same arrays; dual engines recompute x_B = A_B^-1 (b - A_N x_N) from that LU
// first.  The loop body in which a terminal status was found is examined again, not counted twice.
// Returns 0: nothing to do; 1: the loop goes on (status RUNNING, B^-1 rebuilt from the basis k_mid left);
// 2: the solve has ended, *result holds the status k_mid found (certified, or corrected).
static int exact_takeover(ellp_engine *e, uint64_t remaining, ellp_status *result, char *errbuf, size_t errlen) {
    if (e->cert_large && e->world == 1 && !e->colshard) return exact_certify_large(e, remaining, result, errbuf, errlen);
    if (!e->hybrid || e->world != 1 || e->colshard) return 0;
    const int s = e->h_st->status;
    const bool guard = s == ST_NEED_EXACT;
    const bool terminal = s == ELLP_OPTIMAL || s == ELLP_INFEASIBLE || s == ELLP_UNBOUNDED;
    const bool failed = s == ELLP_ERR_SINGULAR || s == ELLP_ERR_NAN || s == ELLP_ERR_PANIC;
    if (!guard && !terminal && !failed) return 0;
    DevState ns = *e->h_st;
    uint64_t budget = remaining;
    if (terminal && ns.iters > 0) {
        ns.iters -= 1;
        budget += 1;
    }
    if (budget == 0) return 0;  // a guarded pivot at the very end of the caller's slice: the next slice starts here
    // The counts, lambda and the pricing window go on (the same solve).  Kept as found, and a question for a later change:
    // open, pe_valid and mv_pending are NOT cleared here, although exact_certify_large clears them at the same
    // moment of its own hand-over.
    clear_stop_words(ns);
    clear_relays(ns);
    auto fail = [&](hipError_t rc) {
        set_err(errbuf, errlen, "HIP error %s in the hand-over to the exact kernel", hipGetErrorString(rc));
        *result = ELLP_ERR_DEVICE;
        return 2;
    };
    hipError_t rc;
    if ((rc = store_state(e, ns)) != hipSuccess) return fail(rc);
    const uint64_t K = budget < (uint64_t)e->exact_K ? budget : (uint64_t)e->exact_K;
    static const int dual_resync = [] {  // diagnostics: ELLP_HYBRID_RESYNC = 1 (default) recomputes x_B only, 2 x_B, y and d
        const char *v = getenv("ELLP_HYBRID_RESYNC");
        return v && v[0] ? atoi(v) : 1;
    }();
    if ((rc = launch_mid(e, K, e->kind == ELLP_ENGINE_DUAL ? dual_resync : 0)) != hipSuccess) return fail(rc);
    if ((rc = read_state(e)) != hipSuccess) return fail(rc);
    const uint64_t did = e->h_st->iters - ns.iters;
    const int s2 = e->h_st->status;
    e->hy_exact_iters += did;
    if (guard) e->hy_guards += 1;
    else {
        e->hy_certs += 1;
        if (!(s2 == s && did <= 1)) e->hy_disagree += 1;
    }
    if (getenv("ELLP_HYBRID_DEBUG"))
        fprintf(stderr, "ellp hybrid: fast status %d at iteration %llu -> exact kernel, %llu iterations, status %d\n", s,
                (unsigned long long)ns.iters, (unsigned long long)did, s2);
    e->u_valid = false;
    e->since_btran = 0;
    nothing_enqueued(e, e->h_st->iters);
    if (e->h_st->pivots != ns.pivots || failed) {
        // the explicit inverse follows the basis (also when the solve has ended: a phase hand-off reads it)
        static const int32_t running = ST_RUNNING;
        if (s2 != ST_RUNNING) (void)hipMemcpyAsync(&e->st->status, &running, sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
        launch_refactor(e);
        e->hy_rebuilds += 1;
        DevState after;
        if ((rc = hipMemcpyAsync(&after, e->st, sizeof(DevState), hipMemcpyDeviceToHost, e->stream)) != hipSuccess) return fail(rc);
        if ((rc = hipStreamSynchronize(e->stream)) != hipSuccess) return fail(rc);
        prof_collect(e);
        if (after.status != ST_RUNNING) {
            if (s2 == ST_RUNNING) {  // the basis the exact kernel left fails the rebuild's guard: that is the loop's next LU
                *e->h_st = after;
                *result = status_message(after, errbuf, errlen);
                return 2;
            }
            e->w_valid = false;
        }
        e->h_st->cur = after.cur;
        if (s2 != ST_RUNNING) {
            static int32_t keep;
            keep = s2;
            (void)hipMemcpyAsync(&e->st->status, &keep, sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
            (void)hipMemcpyAsync(&e->st->panic_code, &e->h_st->panic_code, sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
            (void)hipStreamSynchronize(e->stream);
        }
    }
    if (s2 == ST_RUNNING) {
        if (e->kind == ELLP_ENGINE_DUAL) launch_dleave(e);  // the three-launch loop starts from DevState::lr
        return 1;
    }
    *result = status_message(*e->h_st, errbuf, errlen);
    return 2;
}

// ---- ellp_engine_run and its steps -------------------------------------------------------------------------------------

// n iterations enqueued, the periodic maintenance of B^-1 in front of the one at which it is due
static void enqueue_batch(ellp_engine *e, uint64_t n, int64_t period) {
    for (uint64_t it = 0; it < n; ++it) {
        if (e->since_refactor >= (uint64_t)period) maintain_inverse(e);
        if (e->kind == ELLP_ENGINE_PRIMAL) launch_primal_iteration(e);
        else launch_dual_iteration(e);
    }
}

// what is left of a slice of max_iters that began at iters0, by the iterations that really ran (a stop voids the rest of its batch)
static uint64_t iterations_left(const ellp_engine *e, uint64_t iters0, uint64_t max_iters) {
    const uint64_t done = e->h_st->iters - iters0;
    return done < max_iters ? max_iters - done : 0;
}

// Look-ahead polling (no tiny-pivot maintenance, no profiling, no follow-up refresh due): batch k+1 is enqueued BEFORE the
// host waits for the status of batch k, so the stream never drains while the host looks at a read-back.  A batch enqueued
// after termination — or after a maintenance request of the drift monitor — is a few no-op launches (every kernel returns
// at once when status != RUNNING).  Iterations are counted on the device afterwards.  Enqueues up to `remaining`
// iterations in batches of poll_interval (default 64) and returns with the stream drained and the final state in h_st.
static ellp_status run_look_ahead(ellp_engine *e, uint64_t remaining, int64_t period, char *errbuf, size_t errlen) {
    if (!e->look_ev[0]) {
        HIPCHK(hipEventCreateWithFlags(&e->look_ev[0], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&e->look_ev[1], hipEventDisableTiming));
    }
    const uint64_t lpoll = e->opts.poll_interval > 0 ? (uint64_t)e->opts.poll_interval : 64;
    bool pending[2] = {false, false};
    bool stop = false;
    int slot = 0, last_slot = -1, waited_slot = -1;
    bool last_is_final = false;
    uint64_t to_launch = remaining;
    while (!stop) {
        if (to_launch > 0) {
            const uint64_t batch = to_launch < lpoll ? to_launch : lpoll;
            enqueue_batch(e, batch, period);
            to_launch -= batch;
            launch_dual_close(e);  // a batch ends on a complete state (a fused dual iteration may be open)
            // the objective ellp_stats reports (c . x) rides on the last read-back instead of costing a launch and a
            // synchronisation of its own after the loop (fill_stats)
            if (to_launch == 0 && e->kind == ELLP_ENGINE_PRIMAL) launch_primal_obj(e);
            HIPCHK(hipMemcpyAsync(&e->h_look[slot], e->st, sizeof(DevState), hipMemcpyDeviceToHost, e->stream));
            HIPCHK(hipEventRecord(e->look_ev[slot], e->stream));
            pending[slot] = true;
            last_slot = slot;
            last_is_final = to_launch == 0;
        }
        const int other = slot ^ 1;
        const int wait_on = pending[other] ? other : (to_launch == 0 && pending[slot] ? slot : -1);
        if (wait_on >= 0) {
            HIPCHK(hipEventSynchronize(e->look_ev[wait_on]));
            pending[wait_on] = false;
            waited_slot = wait_on;
            if (e->h_look[wait_on].status != ST_RUNNING || e->h_look[wait_on].tiny || e->h_look[wait_on].fin) stop = true;
        }
        if (to_launch == 0 && !pending[0] && !pending[1]) break;
        slot ^= 1;
    }
    if (last_is_final && waited_slot == last_slot && !pending[0] && !pending[1]) {
        // the read-back just waited for came behind everything that was enqueued: it IS the final state
        *e->h_st = e->h_look[last_slot];
        e->obj_fresh = e->kind == ELLP_ENGINE_PRIMAL;
    } else {
        HIPCHK(read_state(e));
    }
    HIPCHK(hipGetLastError());
    return ELLP_OPTIMAL;
}

// Certify or redo: a hybrid solve that has ended Optimal (certified by the exact kernel) on a point that does not keep the
// invariants of the reference's loop — the explicit-inverse stretch has let x, or the dual's carried d, drift past EPS:
// the caller's next test on that point (the phase-1 objective against EPS, primal…:42-50 / dual…:45-50; the assertions of
// DualPhase2::from, dual_problem.rs:293-310) would fail where the reference's own arithmetic passes — is repeated from the
// start of the phase by the LU-per-iteration kernel alone: from there on the engine IS the reference's loop, bit for bit.
// *result: the status of the solve, Optimal on entry.  Returns ELLP_OPTIMAL, or the error that ends ellp_engine_run at once.
static ellp_status certify_or_redo(ellp_engine *e, ellp_status *result, char *errbuf, size_t errlen) {
    if (!((e->hybrid || (e->cert_large && !e->exact_large_only)) && e->snap.valid && e->world == 1)) return ELLP_OPTIMAL;
    double det[3] = {0.0, 0.0, 0.0};
    bool ok = end_point_ok(e, det);
    if (getenv("ELLP_FORCE_REDO")) ok = false;  // tests: the redo path itself (snapshot, restore, the exact kernel from the start)
    const bool large = !e->hybrid;
    if (!ok && large) {
        // Above 1,024 rows the exact loop costs an LU of 2 m launches and two or three solves of m steps per iteration (about
        // 18 us x m): the redo is taken when the iterations this phase needed, at that price, stay within
        // ELLP_REDO_MAX_SECONDS (default 900 — a 1,850-row phase of 3,000 iterations: 100 s; config 3's 600,000: never);
        // otherwise the point goes out as it is, counted as uncertified (ELLP_TAP_STATE).
        const char *capv = getenv("ELLP_REDO_MAX_SECONDS");  // read when it matters: once per phase end that fails the check
        const double cap = capv && capv[0] ? atof(capv) : 900.0;
        const double est = (double)e->h_st->iters * 18e-6 * (double)e->m;
        if (est > cap) {
            if (getenv("ELLP_HYBRID_DEBUG"))
                fprintf(stderr, "ellp hybrid: end point violates an invariant (x %.3e, d %.3e); a redo would take about %.0f s: not done\n", det[0], det[1], est);
            e->hy_uncertified += 1;
            ok = true;
        }
    }
    if (ok) return ELLP_OPTIMAL;
    if (getenv("ELLP_HYBRID_DEBUG")) {
        if (large)
            fprintf(stderr, "ellp hybrid: end point violates an invariant (x %.3e, d %.3e, objective %.17g): redo on fresh LUs\n", det[0], det[1], det[2]);
        else
            fprintf(stderr, "ellp hybrid: end point violates an invariant (x %.3e, d %.3e, objective %.17g against the carried %.17g): redo\n",
                    det[0], det[1], det[2], e->h_st->obj);
    }
    const ellp_status rs = redo_from_snapshot(e, large, errbuf, errlen);
    if (rs != ELLP_OPTIMAL) return rs;
    *result = large ? run_exact_large(e, e->opts.max_iter, errbuf, errlen) : run_small(e, e->opts.max_iter, errbuf, errlen);
    e->obj_fresh = false;
    return ELLP_OPTIMAL;
}

// The caller's budget (ellp_opts.max_iter) is spent: the reference has run that many FULL loop bodies
// (primal…:162-202), so an unbounded ray, a panic or a NaN found by the ratio test of the last one is its
// result, not MaxIter.  On the two-launch pipeline that ratio test is still open (its fold belongs to the next
// pricing launch, which will not come): close it and take the status from behind the closing kernel.  Slices
// inside the budget stay open — that is what makes slicing free.
static ellp_status close_open_iteration_at_budget(ellp_engine *e, ellp_status *result, char *errbuf, size_t errlen) {
    if (!(e->lag_open && !e->small && e->world == 1 && e->h_st->iters >= e->opts.max_iter)) return ELLP_OPTIMAL;
    launch_flush(e);
    launch_primal_obj(e);
    HIPCHK(read_state(e));
    settle_state(e);
    e->obj_fresh = true;
    if (e->h_st->status != ST_RUNNING && e->h_st->status != ST_NEED_MAINT) *result = status_message(*e->h_st, errbuf, errlen);
    return ELLP_OPTIMAL;
}

ellp_status ellp_engine_run(ellp_engine *e, uint64_t max_iters, ellp_stats *stats, char *errbuf, size_t errlen) {
    if (!e) return ELLP_ERR_ARG;
    if (errbuf && errlen) errbuf[0] = 0;
    HIPCHK(hipSetDevice(e->device));
    e->obj_fresh = false;
    auto t0 = std::chrono::steady_clock::now();
    const uint64_t poll = e->opts.poll_interval > 0 ? (uint64_t)e->opts.poll_interval : (e->m <= 256 ? 64 : 16);
    int64_t period = e->refactor_period;
    if (period <= 0) period = default_period(e->m, e->ld, e->nN);
    ellp_status result = ELLP_MAXITER;
    if ((e->hybrid || e->cert_large) && !e->snap.valid && e->world == 1 && !e->colshard && e->nN > 0 && getenv("ELLP_NO_REDO") == nullptr) {
        launch_flush(e);
        HIPCHK(take_snapshot(e));  // the start of the phase (certify or redo, see end_point_ok)
    }
    if (e->nN == 0) {
        result = ELLP_OPTIMAL;  // primal…:149-151 / dual…:175-177
    } else if (e->small && e->world == 1) {
        result = run_small(e, max_iters, errbuf, errlen);
    } else if (e->exact_large_only && e->world == 1 && !e->colshard) {
        result = run_exact_large(e, max_iters, errbuf, errlen);
    } else {
        uint64_t remaining = max_iters;
        if (e->colshard) return run_colsharded(e, max_iters, stats, errbuf, errlen);
        if (e->world != 1) {
            set_err(errbuf, errlen, "a sharded engine is driven with ellp_engine_step + an all-gather (ellp_amd/dist.py)");
            return ELLP_ERR_ARG;
        }
        if (e->kind == ELLP_ENGINE_DUAL && remaining > 0 && e->need_dleave) {
            launch_dleave(e);
            e->need_dleave = false;
        }
        // a previous slice may already have terminated (h_st is current if the previous call was a run that read it)
        if (!e->hst_fresh) HIPCHK(read_state(e));
        e->hst_fresh = false;
        settle_state(e);
        const uint64_t iters0 = e->h_st->iters;
        if (e->h_st->status == ST_NEED_EXACT && remaining > 0) {  // a guarded pivot closed the previous slice
            const int tk = exact_takeover(e, remaining, &result, errbuf, errlen);
            remaining = tk == 2 ? 0 : iterations_left(e, iters0, max_iters);
        } else if (e->h_st->status == ST_NEED_EXACT) {
            remaining = 0;  // nothing to run: the status stays for the next slice
        } else if (e->h_st->status != ST_RUNNING) {
            result = status_message(*e->h_st, errbuf, errlen);
            remaining = 0;
        }
        const bool can_look_ahead = e->ill_tol <= 0.0 && !e->opts.profile;
        while (remaining > 0 && result == ELLP_MAXITER) {
            // a follow-up refresh is due (maint_chain, set by a serviced request): one polled iteration, then the refresh
            const bool chained = e->maint_chain > 0;
            const bool look_ahead = can_look_ahead && e->maint_chain == 0;
            if (look_ahead) {
                const ellp_status ls = run_look_ahead(e, remaining, period, errbuf, errlen);
                if (ls != ELLP_OPTIMAL) return ls;
            } else {
                enqueue_batch(e, chained ? 1 : (remaining < poll ? remaining : poll), period);
                // this path serves the reactive maintenance of small LPs (and profiling): its follow-up refresh is
                // meant to come AFTER the iteration that follows a tiny pivot, so that iteration is completed here
                if (e->ill_tol > 0.0) launch_flush(e);
                launch_dual_close(e);
                HIPCHK(read_state(e));
                HIPCHK(hipGetLastError());
                prof_collect(e);
            }
            // the tail of both: h_st is the drained state behind everything enqueued
            settle_state(e);
            if (getenv("ELLP_RUN_DEBUG"))
                fprintf(stderr, "ellp run (%s): status %d iters %llu tiny %d fin %d need_rebuild %d lr %lld obj %.17g\n",
                        look_ahead ? "look-ahead" : "polled", e->h_st->status, (unsigned long long)e->h_st->iters, e->h_st->tiny,
                        e->h_st->fin, e->h_st->need_rebuild, (long long)e->h_st->lr, e->h_st->obj);
            remaining = iterations_left(e, iters0, max_iters);
            if (chained) e->maint_chain = 0;
            if (service_maintenance_request(e)) continue;  // refreshed; the follow-up runs polled (maint_chain)
            if (chained && e->h_st->status == ST_RUNNING) maintain_inverse(e, true);  // the follow-up refresh
            if (e->h_st->status != ST_RUNNING) {
                const int tk = exact_takeover(e, remaining, &result, errbuf, errlen);
                if (tk == 1) {
                    remaining = iterations_left(e, iters0, max_iters);
                } else if (tk == 0) {
                    if (e->h_st->status == ST_NEED_EXACT) break;  // the slice is used up: the next one starts with the hand-over
                    result = status_message(*e->h_st, errbuf, errlen);
                }
            }
        }
    }
    if (result == ELLP_OPTIMAL) {
        const ellp_status rs = certify_or_redo(e, &result, errbuf, errlen);
        if (rs != ELLP_OPTIMAL) return rs;
    }
    if (result == ELLP_MAXITER) {
        const ellp_status cs = close_open_iteration_at_budget(e, &result, errbuf, errlen);
        if (cs != ELLP_OPTIMAL) return cs;
    }
    if (stats) {
        fill_stats(e, stats);
        stats->t_loop_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
    // A slice that ends normally has read h_st behind its last iteration; what may have been enqueued after that
    // read (fill_stats' objective kernel, a follow-up refresh) changes neither the status nor the iteration
    // counter, and a request it raises is seen by the next slice's first read-back.  So the next ellp_engine_run
    // need not start with a read-back of its own (15 us of a 20-iteration slice).
    e->hst_fresh = result == ELLP_MAXITER && !e->small && e->world == 1 && !e->colshard && e->nN > 0 &&
                   e->h_st->status == ST_RUNNING;
    return result;
}


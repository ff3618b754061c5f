// ellp_phase.inc — where a phase starts on a resident engine: the phase-1 constructors (ellp_engine_create_primal_phase1,
// ellp_engine_create_dual_phase1), the phase-1 -> phase-2 hand-offs (ellp_engine_rephase, ellp_engine_dual_rephase) and what
// the two dual ones share (dual_point_from_inverse).  Host code only.  The pieces they are made of — the DevState groups and
// store_state, nothing_enqueued / begin_phase, the DevTemp holder — are in ellp_launch.inc, because the re-arms inside
// ellp_engine_run (ellp_run.inc: redo_from_snapshot, exact_certify_large, exact_takeover) are made of them too.  Included
// inside extern "C", behind ellp_run.inc (launch_mid, exact_workspace) and creation (engine_create_impl).

ellp_status ellp_engine_create_primal_phase1(int64_t m, int64_t n, const double *A, const double *b,
                                             const uint8_t *bound_kind, const double *lb, const double *ub,
                                             const double *x, const uint8_t *N_bound, const ellp_opts *opts_in,
                                             ellp_engine **out, char *errbuf, size_t errlen) {
    if (!out) return ELLP_ERR_ARG;
    *out = nullptr;
    if (m <= 0 || n <= 0 || !A || !b || !bound_kind || !lb || !ub || !x || !N_bound) {
        set_err(errbuf, errlen, "null pointer or inconsistent sizes");
        return ELLP_ERR_ARG;
    }
    // the phase-1 problem (primal_problem.rs:137-141, :236-253): costs 0 on the originals and 1 on the m
    // artificials, the artificials Lower(0) and basic, every original variable nonbasic at the bound the
    // caller names
    const int64_t nt = n + m;
    std::vector<double> c((size_t)nt, 0.0), lb2((size_t)nt, 0.0), ub2((size_t)nt, 0.0), x2((size_t)nt, 0.0);
    std::vector<uint8_t> kind2((size_t)nt, (uint8_t)ELLP_BOUND_LOWER), Nb(N_bound, N_bound + n);
    std::vector<int64_t> B((size_t)m), N((size_t)n);
    for (int64_t j = 0; j < n; ++j) {
        kind2[(size_t)j] = bound_kind[j];
        lb2[(size_t)j] = lb[j];
        ub2[(size_t)j] = ub[j];
        x2[(size_t)j] = x[j];
        N[(size_t)j] = j;
    }
    for (int64_t i = 0; i < m; ++i) {
        c[(size_t)(n + i)] = 1.0;
        B[(size_t)i] = n + i;
    }
    return engine_create_impl(ELLP_ENGINE_PRIMAL, m, nt, nt, A, c.data(), b, kind2.data(), lb2.data(), ub2.data(),
                              x2.data(), B.data(), m, N.data(), Nb.data(), n, nullptr, nullptr, opts_in, out, errbuf, errlen,
                              n, true);
}

// The new phase's costs (through the temporary c_dev, which the caller owns: the dual's point is made from it), right-hand
// side (dual: b, at its place in the order; primal: nullptr) and bounds; c_B, c_N and the nonbasic labels follow on the device
static ellp_status upload_phase_data(ellp_engine *e, DevTemp<double> &c_dev, const double *c, const double *b,
                                     const uint8_t *bound_kind, const double *lb, const double *ub, char *errbuf, size_t errlen) {
    const int64_t m = e->m, nN = e->nN, n_c = e->n_c;
    HIPCHK(c_dev.alloc((size_t)n_c));
    HIPCHK(hipMemcpyAsync(c_dev.p, c, sizeof(double) * (size_t)n_c, hipMemcpyHostToDevice, e->stream));
    if (b) HIPCHK(hipMemcpyAsync(e->b_dev, b, sizeof(double) * (size_t)m, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->lb, lb, sizeof(double) * (size_t)n_c, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->ub, ub, sizeof(double) * (size_t)n_c, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->kindv, bound_kind, (size_t)n_c, hipMemcpyHostToDevice, e->stream));
    const int64_t cnt = m > nN ? m : nN;
    hipLaunchKernelGGL(k_rephase, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, e->stream, c_dev.p, e->kindv, e->B_index,
                       e->N_index, e->c_B, e->c_N, e->Nb, m, nN);
    if (e->c_tail) HIPCHK(hipMemcpyAsync(e->c_tail, c_dev.p + e->n, sizeof(double) * (size_t)(n_c - e->n), hipMemcpyDeviceToDevice, e->stream));
    return ELLP_OPTIMAL;
}

ellp_status ellp_engine_rephase(ellp_engine *e, const double *c, const uint8_t *bound_kind, const double *lb,
                                const double *ub, char *errbuf, size_t errlen) {
    if (e) e->hst_fresh = false;  // anything but ellp_engine_run may change the device state behind h_st
    if (!e || !c || !bound_kind || !lb || !ub) return ELLP_ERR_ARG;
    if (errbuf && errlen) errbuf[0] = 0;
    if (e->kind != ELLP_ENGINE_PRIMAL) {
        set_err(errbuf, errlen, "rephase is the primal phase-1 -> phase-2 hand-off");
        return ELLP_ERR_ARG;
    }
    const ellp_status ks = check_bound_kinds(e->n_c, bound_kind, errbuf, errlen);
    if (ks != ELLP_OPTIMAL) return ks;
    HIPCHK(hipSetDevice(e->device));
    launch_flush(e);
    HIPCHK(hipStreamSynchronize(e->stream));
    DevTemp<double> c_dev(e->stream);
    const ellp_status us = upload_phase_data(e, c_dev, c, nullptr, bound_kind, lb, ub, errbuf, errlen);
    if (us != ELLP_OPTIMAL) return us;
    launch_primal_obj(e);  // c.x with the new costs (the objective trace continues from it)
    if (e->trace_len > 0) (void)hipMemsetAsync(e->trace_it, 0, sizeof(unsigned long long) * (size_t)e->trace_len, e->stream);
    // a new solve_with_initial starts here: status, counters and flags afresh; B^-1 and `cur` stay.  Every group is cleared;
    // obj is k_primal_obj's, and lr is left alone (only the dual's kernels write it)
    HIPCHK(read_state(e));
    DevState ns = *e->h_st;
    clear_stop_words(ns);
    clear_relays(ns);
    clear_open_iteration(ns);
    ns.se_valid = 0;  // steepest edge: the last pivot's weight update has been applied by the pricing launch that ended the phase
    restart_pricing_window(ns, e);
    clear_counts(ns);
    ns.lambda = 0.0;
    HIPCHK(store_state(e, ns));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->u_valid = false;  // u = B^-T c_B with the new costs
    begin_phase(e);
    return ELLP_OPTIMAL;
}

// y = B^-T c_B, d = c - A^T y, labels and values of the nonbasic variables, x_B = B^-1 (b - A_N x_N), all from the
// resident B^-1: the common part of DualPhase2::from (dual_problem.rs:278-328; labels :286-323) and of
// DualPhase1::new (:165-214; labels :177-203, `phase1`).  Ends with the loop's own entry assertion
// (dual_simplex_solver.rs:139-151).  c_dev: the costs by variable index, on the device.
static ellp_status dual_point_from_inverse(ellp_engine *e, const double *c_dev, int phase1, const int64_t *N_host,
                                           char *errbuf, size_t errlen) {
    const int64_t m = e->m, nN = e->nN, ld = e->ld, n_c = e->n_c;
    // Certified-hybrid engines take y (and, below, x_B) from a fresh LU of the basis — the LU-per-iteration kernel with zero
    // iterations — as the reference does (dual_problem.rs:162-172, :275-284), not from the explicit inverse: the point is the
    // START of a phase whose carried d the caller will test against EPS at its end, and a d that starts 1e-9 off stays 1e-9 off
    // even when the exact kernel repeats the phase.
    const bool from_lu = e->hybrid && e->LUa != nullptr && e->world == 1;
    if (from_lu) {
        HIPCHK(launch_mid(e, 0, 2));
    } else if (e->exact_large_always) {
        // the exact loop above 1,024 rows: y = B^-T c_B from a fresh LU of the basis as well (x_B follows in every loop body)
        HIPCHK(exact_workspace(e));
        HIPCHK(hipMemsetAsync(e->ex_fail, 0, sizeof(int), e->stream));
        hipLaunchKernelGGL(k_rows_from_cols, dim3((unsigned)((m + 31) / 32), (unsigned)((m + 31) / 32)), dim3(256), 0, e->stream, e->A_B, e->luw.M, m, ld);
        ellp_lu_rows_factor(&e->luw, e->stream);
        hipLaunchKernelGGL(k_lu_solve, dim3(1), dim3(1024), 2 * sizeof(double) * (size_t)m, e->stream, e->luw.M, e->luw.piv, m, e->c_B, e->ex_sol, 1, e->ex_fail);
        int failed = 0;
        HIPCHK(hipMemcpyAsync(&failed, e->ex_fail, sizeof(int), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        if (failed) {
            set_err(errbuf, errlen, "unwrap() on None: the basis is exactly singular");
            return ELLP_ERR_PANIC;
        }
        HIPCHK(hipMemsetAsync(e->y, 0, sizeof(double) * (size_t)ld, e->stream));
        HIPCHK(hipMemcpyAsync(e->y, e->ex_sol, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, e->stream));
    } else {
        launch_btran(e);  // into e->u (a dual engine has no other use for it)
        HIPCHK(hipMemcpyAsync(e->y, e->u, sizeof(double) * (size_t)ld, hipMemcpyDeviceToDevice, e->stream));
    }
    HIPCHK(hipMemsetAsync(e->x, 0, sizeof(double) * (size_t)n_c, e->stream));
    DualRephaseArgs da{e->A_N, e->A_B, e->y, c_dev, e->kindv, e->lb, e->ub, e->N_index, e->B_index, e->dd, e->x, e->Nb,
                       e->st, m, ld, nN, e->eps, phase1};
    hipLaunchKernelGGL(k_dual_rephase, dim3((unsigned)((nN + m + 3) / 4)), dim3(256), 0, e->stream, da);
    launch_resync(e, 1);
    if (from_lu) HIPCHK(launch_mid(e, 0, 1));  // x_B = A_B^-1 (b - A_N x_N) from the LU
    std::vector<double> d((size_t)n_c);
    std::vector<uint8_t> Nb((size_t)(nN > 0 ? nN : 1));
    HIPCHK(hipMemcpyAsync(d.data(), e->dd, sizeof(double) * (size_t)n_c, hipMemcpyDeviceToHost, e->stream));
    if (nN > 0) HIPCHK(hipMemcpyAsync(Nb.data(), e->Nb, (size_t)nN, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(read_state(e));
    HIPCHK(hipGetLastError());
    if (e->h_st->status != ST_RUNNING) return status_message(*e->h_st, errbuf, errlen);
    return dual_start_feasible(nN, N_host, Nb.data(), d.data(), e->eps, errbuf, errlen) ? ELLP_OPTIMAL : ELLP_ERR_PANIC;
}

// the dual objective of the point just made, from y and d as they stand on the device: into DevState::obj on both sides
static ellp_status store_dual_obj(ellp_engine *e, const double *b, const uint8_t *bound_kind, const double *lb, const double *ub,
                                  char *errbuf, size_t errlen) {
    const int64_t m = e->m, n_c = e->n_c;
    std::vector<double> y((size_t)m), d((size_t)n_c);
    HIPCHK(hipMemcpy(y.data(), e->y, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(d.data(), e->dd, sizeof(double) * (size_t)n_c, hipMemcpyDeviceToHost));
    const double obj = host_dual_obj(m, n_c, b, bound_kind, lb, ub, y.data(), d.data());
    HIPCHK(hipMemcpy(&e->st->obj, &obj, sizeof(double), hipMemcpyHostToDevice));
    e->h_st->obj = obj;
    return ELLP_OPTIMAL;
}

ellp_status ellp_engine_dual_rephase(ellp_engine *e, const double *c, const double *b, const uint8_t *bound_kind,
                                     const double *lb, const double *ub, char *errbuf, size_t errlen) {
    if (e) e->hst_fresh = false;  // anything but ellp_engine_run may change the device state behind h_st
    if (!e || !c || !b || !bound_kind || !lb || !ub) return ELLP_ERR_ARG;
    if (errbuf && errlen) errbuf[0] = 0;
    if (e->kind != ELLP_ENGINE_DUAL || e->small || e->colshard || e->world != 1) {
        set_err(errbuf, errlen, "dual_rephase: a resident, unsharded dual engine of the explicit-inverse kind is needed");
        return ELLP_ERR_ARG;
    }
    const ellp_status ks = check_bound_kinds(e->n_c, bound_kind, errbuf, errlen);
    if (ks != ELLP_OPTIMAL) return ks;
    HIPCHK(hipSetDevice(e->device));
    HIPCHK(hipStreamSynchronize(e->stream));
    const int64_t m = e->m, nN = e->nN, ld = e->ld, n_c = e->n_c;
    // ---- N in variable-index order (dual_problem.rs:286-323 enumerates `is_basic`), columns moved along
    std::vector<int64_t> N((size_t)nN), perm((size_t)nN), Nsorted((size_t)nN);
    if (nN > 0) HIPCHK(hipMemcpy(N.data(), e->N_index, sizeof(int64_t) * (size_t)nN, hipMemcpyDeviceToHost));
    for (int64_t j = 0; j < nN; ++j) perm[(size_t)j] = j;
    std::sort(perm.begin(), perm.end(), [&](int64_t a, int64_t b2) { return N[(size_t)a] < N[(size_t)b2]; });
    bool moved = false;
    for (int64_t j = 0; j < nN; ++j) {
        Nsorted[(size_t)j] = N[(size_t)perm[(size_t)j]];
        moved = moved || perm[(size_t)j] != j;
    }
    if (moved && nN > 0) {
        DevTemp<double> A2(e->stream);  // the engine's new A_N, once the columns are in it
        DevTemp<int64_t> perm_dev(e->stream);
        HIPCHK(A2.alloc((size_t)(ld * nN)));
        HIPCHK(perm_dev.alloc((size_t)nN));
        HIPCHK(hipMemcpyAsync(perm_dev.p, perm.data(), sizeof(int64_t) * (size_t)nN, hipMemcpyHostToDevice, e->stream));
        hipLaunchKernelGGL(k_permute_cols, dim3((unsigned)nN), dim3(256), 0, e->stream, e->A_N, A2.p, perm_dev.p, ld);
        HIPCHK(hipMemcpyAsync(e->N_index, Nsorted.data(), sizeof(int64_t) * (size_t)nN, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        replace_alloc(e, e->A_N, A2.p);
        e->A_N = A2.release();
    }
    // ---- new costs, right-hand side, bounds
    DevTemp<double> c_dev(e->stream);
    const ellp_status us = upload_phase_data(e, c_dev, c, b, bound_kind, lb, ub, errbuf, errlen);
    if (us != ELLP_OPTIMAL) return us;
    // a new solve_with_initial: status and counters afresh (the maintenance kernels need a RUNNING engine)
    HIPCHK(read_state(e));
    DevState ns = *e->h_st;
    clear_stop_words(ns);
    // already zero, all five: their writers are k_price2 and k_ftran_eta, launched where EnginePlan::lagged is set, which the plan does for primal engines only
    clear_relays(ns);
    clear_open_iteration(ns);
    clear_counts(ns);
    ns.lr = -1;
    // Kept as found, and a question for a later change: lambda is NOT cleared here (the primal hand-off and the redo clear it),
    // and neither is the host's u_valid below (the primal hand-off clears it).  obj follows from the host (store_dual_obj).
    HIPCHK(store_state(e, ns));
    // y, d and the labels are made from B^-1 and checked against the reference's EPS assertions (dual_problem.rs:275-323);
    // the reference takes a FRESH LU there, so the resident inverse (up to a maintenance period of eta updates old) is
    // rebuilt from A_B first — once per solve
    launch_dual_close(e);
    launch_refactor(e);
    HIPCHK(read_state(e));
    if (e->h_st->status != ST_RUNNING) return status_message(*e->h_st, errbuf, errlen);
    e->since_refactor = 0;
    const ellp_status ps = dual_point_from_inverse(e, c_dev.p, 0, Nsorted.data(), errbuf, errlen);
    if (ps != ELLP_OPTIMAL) return ps;
    const ellp_status os = store_dual_obj(e, b, bound_kind, lb, ub, errbuf, errlen);
    if (os != ELLP_OPTIMAL) return os;
    e->need_dleave = true;
    begin_phase(e);
    e->box_problem = is_box_problem(m, n_c, bound_kind, b);
    if (e->trace_len > 0) HIPCHK(hipMemset(e->trace_it, 0, sizeof(unsigned long long) * (size_t)e->trace_len));
    return ELLP_OPTIMAL;
}

// DualPhase1::new's point (dual_problem.rs:162-214) made on the device: the caller has the box problem's standard
// form and the basis the LU of A^T picked (B_index, and N_index in the order of the permutation, :153-160); the
// engine builds B^-1 and from it y = B^-T c_B, d = c - A^T y, the nonbasic labels and values by the sign of d,
// b~ = b - A x and x_B = B^-1 b~.  No LU of A_B on the host, no solves, no A x product there.
ellp_status ellp_engine_create_dual_phase1(int64_t m, int64_t n, const double *A, const double *c, const double *b,
                                           const uint8_t *bound_kind, const double *lb, const double *ub,
                                           const int64_t *B_index, const int64_t *N_index, const ellp_opts *opts_in,
                                           ellp_engine **out, char *errbuf, size_t errlen) {
    if (errbuf && errlen) errbuf[0] = 0;
    if (!out) return ELLP_ERR_ARG;
    *out = nullptr;
    if (m <= 0 || n <= m || !A || !c || !b || !bound_kind || !lb || !ub || !B_index || !N_index) {
        set_err(errbuf, errlen, "bad arguments (a nonbasic variable is needed: n > m)");
        return ELLP_ERR_ARG;
    }
    const int64_t nN = n - m;
    std::vector<double> zeros((size_t)(n > m ? n : m), 0.0);
    std::vector<uint8_t> Nb((size_t)(nN > 0 ? nN : 1), (uint8_t)ELLP_NB_LOWER);
    ellp_engine *e = nullptr;
    ellp_status s = engine_create_impl(ELLP_ENGINE_DUAL, m, n, n, A, c, b, bound_kind, lb, ub, zeros.data(), B_index, m,
                                       N_index, Nb.data(), nN, zeros.data(), zeros.data(), opts_in, &e, errbuf, errlen, n,
                                       false);
    if (s != ELLP_OPTIMAL) return s;
    std::unique_ptr<ellp_engine, void (*)(ellp_engine *)> own(e, ellp_engine_destroy);  // destroys it on an early return
    if (e->small) {  // k_small keeps no inverse; the point below is made from one all the same
        launch_refactor(e);
        HIPCHK(read_state(e));
        if (e->h_st->status != ST_RUNNING) return status_message(*e->h_st, errbuf, errlen);
    }
    DevTemp<double> c_dev(e->stream);  // behind `own`: it drains the engine's stream before the engine can go
    HIPCHK(c_dev.alloc((size_t)n));
    HIPCHK(hipMemcpyAsync(c_dev.p, c, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, e->stream));
    s = dual_point_from_inverse(e, c_dev.p, 1, N_index, errbuf, errlen);
    if (s != ELLP_OPTIMAL) return s;
    s = store_dual_obj(e, b, bound_kind, lb, ub, errbuf, errlen);
    if (s != ELLP_OPTIMAL) return s;
    e->need_dleave = true;
    e->u_valid = false;
    *out = own.release();
    return ELLP_OPTIMAL;
}

// ellp_launch.inc — the host side of every launch of the explicit-inverse engine: the event brackets (Prof), the argument
// structs filled from ellp_engine, the run-time value -> template instantiation dispatch, one iteration of each loop
// (launch_primal_iteration, launch_dual_iteration), the maintenance of B^-1 (maintain_inverse,
// service_maintenance_request), the state read-back (read_state, settle_state) and the pieces a stopped engine is made ready
// again from (the DevState groups, store_state, nothing_enqueued / begin_phase, DevTemp).  No kernel lives here.  Included inside
// the anonymous namespace behind struct ellp_engine and dmalloc, in front of everything that drives an engine
// (creation, ellp_run.inc, the sharding API, ellp_post.inc).

// ---- small argument expressions, each stated once
inline Xchg xchg_of(const ellp_engine *e) { return Xchg{e->X, e->seg, e->nbs, e->cpb}; }
inline Trace trace_of(const ellp_engine *e) { return Trace{e->trace_obj, e->trace_it, e->trace_len}; }
// the pivot guard of the certifying engines, 0: off (also while the exact iterations run: guard_off).  k_update2 guards the
// hybrid's pivots and those above 1,024 rows (`hybrid_too`); k_price2 and k_dual_fu only run where cert_large certifies
inline double pivot_guard(const ellp_engine *e, bool hybrid_too) {
    return (((hybrid_too && e->hybrid) || e->cert_large) && !e->guard_off) ? e->guard_abs : 0.0;
}

// ---- run-time value -> template argument.  f is called with a std::integral_constant (TV(x): its value); everything is
// inlined, so a launch costs what the switch it replaces cost, and the set of instantiations is the one listed here.
#define TV(x) (decltype(x)::value)
template <int N>
using Int = std::integral_constant<int, N>;
template <typename F>
inline void with_bool(bool v, F &&f) {
    if (v) f(std::true_type{});
    else f(std::false_type{});
}
// EnginePlan::priceT, the double2 per thread for one row of the pricing kernels: {1, 2, 4, 8, 16}
template <typename F>
inline void with_price_tile(int priceT, F &&f) {
    switch (priceT) {
    case 1: f(Int<1>{}); break;
    case 2: f(Int<2>{}); break;
    case 4: f(Int<4>{}); break;
    case 8: f(Int<8>{}); break;
    default: f(Int<16>{}); break;
    }
}
// NR of k_update2 / k_ftran_eta / k_dual_fu, the double2 per thread per row kept in registers: the next of {1, 2, 4, 8};
// beyond 8 the looping instantiation <0> where the kernel has one (LOOPS), else <8> (k_dual_fu: ld <= 4096 by the plan)
template <bool LOOPS, typename F>
inline void with_row_regs(int64_t ld, F &&f) {
    const int64_t nr = ((ld >> 1) + 255) / 256;
    if (nr <= 1) f(Int<1>{});
    else if (nr <= 2) f(Int<2>{});
    else if (nr <= 4) f(Int<4>{});
    else if (!LOOPS || nr <= 8) f(Int<8>{});
    else if constexpr (LOOPS) f(Int<0>{});
}
// NT of k_ftran2, the double2 per lane for one row: the next of {4, 8, 16}, beyond that the looping <0>
template <typename F>
inline void with_ftran_tile(int64_t ld, F &&f) {
    const int64_t nt = ((ld >> 1) + 63) / 64;
    if (nt <= 4) f(Int<4>{});
    else if (nt <= 8) f(Int<8>{});
    else if (nt <= 16) f(Int<16>{});
    else f(Int<0>{});
}

struct Prof {
    ellp_engine *e;
    int id;
    bool on;
    hipEvent_t a{}, b{};
    Prof(ellp_engine *e_, int id_) : e(e_), id(id_), on(e_->opts.profile != 0) {
        if (!on) return;
        if (e->ev_next + 2 > e->ev_pool.size()) {
            for (int k = 0; k < 64; ++k) {
                hipEvent_t ev;
                if (hipEventCreate(&ev) != hipSuccess) { on = false; return; }
                e->ev_pool.push_back(ev);
            }
        }
        a = e->ev_pool[e->ev_next++];
        b = e->ev_pool[e->ev_next++];
        (void)hipEventRecord(a, e->stream);
    }
    ~Prof() {
        if (!on) return;
        (void)hipEventRecord(b, e->stream);
        e->pending.push_back({id, a, b});
    }
};

// What an event bracket adds to the one kernel inside it, relative to rocprofv3's duration of
// that kernel.  Measured on MI355X / ROCm 7.2 with tools/event_cal.hip and with bench.py run
// under rocprofv3: 2.4 us around a 23.6 us kernel, 2.45 us around a null kernel, 2.2-2.5 us
// around k_price / k_ftran2 / k_update2.  It is a property of the event markers, not of the
// kernel, and it cannot be measured live without the profiler: an EMPTY pair reads 4.4 us, and
// differences between one launch and N back-to-back launches include a dispatch gap that varies
// from 0.35 to 2 us with the kernel.  So the constant below is subtracted (2.3 us errs on the
// side of longer kernels); ELLP_EVENT_BRACKET_US overrides it, ELLP_PROF_RAW=1 reports raw
// brackets.  profiles/ holds the rocprofv3 summaries the bench's figures are checked against.
constexpr double EVENT_BRACKET_US = 2.3;

void prof_calibrate(ellp_engine *e) {
    if (e->ev_overhead_ms >= 0.0 || !e->opts.profile) return;
    e->ev_overhead_ms = EVENT_BRACKET_US * 1e-3;
    if (const char *v = getenv("ELLP_PROF_RAW"); v && v[0] == '1') e->ev_overhead_ms = 0.0;
    if (const char *v = getenv("ELLP_EVENT_BRACKET_US"); v && v[0]) {
        const double us = atof(v);
        if (us >= 0.0 && us < 20.0) e->ev_overhead_ms = us * 1e-3;
    }
}

void prof_collect(ellp_engine *e) {
    prof_calibrate(e);
    for (auto &p : e->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            double v = (double)ms - (p.id == ELLP_K_REFACTOR ? 0.0 : e->ev_overhead_ms);
            e->kernel_ms[p.id] += v > 0.0 ? v : 0.0;
            e->kernel_calls[p.id] += 1;
        }
    }
    e->pending.clear();
    e->ev_next = 0;
}

// ---- launches -----------------------------------------------------------------------------
template <int MODE>
void launch_price(ellp_engine *e) {
    PriceArgs a{};
    a.A_N = e->A_N;
    a.W0 = e->W;
    a.W1 = e->W2;
    a.u = e->u;
    a.c_N = e->c_N;
    a.Nb = e->Nb;
    a.N_index = e->N_index;
    a.dd = e->dd;
    a.xc = xchg_of(e);
    a.st = e->st;
    a.ld = e->ld;
    a.nN = e->nN;
    a.cpb = e->cpb;
    a.block0 = e->rank * e->nbs;
    a.eps = e->eps;
    a.pp_on = e->pp_P > 1 ? 1 : 0;
    a.vs_row = !(e->opts.flags & ELLP_FLAG_DENSE_PRICING) ? e->vs_row : nullptr;
    a.vs_val = a.vs_row ? e->vs_val : nullptr;
    a.rho_ovr = MODE == 1 ? e->price_rho_ovr : nullptr;
    if (MODE == 1 && e->dual_fold) {
        a.dp_seq = e->dual_seq;
        a.dp_lrow = e->binfo; a.dp_ldelta = e->bmin; a.dp_lside = e->bmin + e->m; a.dp_d = e->d;
        a.dp_nrb = (int)((e->m + UPD_ROWS - 1) / UPD_ROWS);
        a.dp_maxviol = e->dual_maxviol;
        a.dp_A_N = e->A_N; a.dp_A_B = e->A_B; a.dp_c_B = e->c_B; a.dp_c_N = e->c_N; a.dp_x = e->x; a.dp_dd = e->dd;
        a.dp_B_index = e->B_index; a.dp_N_index = e->N_index; a.dp_Nb = e->Nb;
        a.dp_trace = trace_of(e);
    }
    int mine = e->nblocks - a.block0;
    if (mine > e->nbs) mine = e->nbs;
    if (mine <= 0) mine = 1;  // empty shard (more ranks than pricing blocks): the block only serves DevState::tiny
    dim3 g(mine), b(256);
    if (e->price_wave) {
        hipLaunchKernelGGL((k_price_wave<MODE>), g, b, 0, e->stream, a);
        return;
    }
    with_bool(e->price_nt, [&](auto NT) {
        with_price_tile(e->priceT, [&](auto T) { hipLaunchKernelGGL((k_price<TV(T), MODE, TV(NT)>), g, b, 0, e->stream, a); });
    });
}

template <int MODE>
void launch_ftran2(ellp_engine *e) {
    Ftran2Args a{};
    a.W0 = e->W; a.W1 = e->W2; a.A_N = e->A_N;
    a.xc = xchg_of(e);
    a.N_index = e->N_index; a.B_index = e->B_index; a.Nb = e->Nb; a.kind = e->kindv;
    a.x = e->x; a.lb = e->lb; a.ub = e->ub;
    a.d = e->d; a.lam = e->lam; a.bidx = e->bidx; a.dpos = e->dpos;
    a.st = e->st; a.m = e->m; a.ld = e->ld; a.nN = e->nN; a.nblocks = e->nblocks; a.cpb = e->cpb; a.eps = e->eps;
    a.aq_cur = (MODE == 0 && e->colshard) ? e->aq_cur : nullptr;
    if (MODE == 0 && e->colshard && e->sel_in_ftran) {
        a.sel_packs = e->packs; a.aq_out = e->aq_cur; a.sel_world = e->world; a.mbox_commit = e->sel_commit ? 1 : 0;
    }
    a.pp_on = (MODE == 0 && e->pp_P > 1) ? 1 : 0;
    const dim3 g(e->ftran_blocks), b(256);
    with_ftran_tile(e->ld, [&](auto NT) { hipLaunchKernelGGL((k_ftran2<MODE, TV(NT)>), g, b, e->ftran_lds, e->stream, a); });
}

template <int MODE>
void launch_update2(ellp_engine *e, int update_u) {
    Update2Args a{};
    a.W0 = e->W; a.W1 = e->W2; a.d = e->d; a.lam = e->lam; a.bidx = e->bidx; a.dpos = e->dpos; a.xc = xchg_of(e);
    a.u = e->u; a.u_alt = e->u + e->ld; a.A_N = e->A_N; a.A_B = e->A_B; a.c_B = e->c_B; a.c_N = e->c_N; a.x = e->x; a.y = e->y; a.dd = e->dd;
    a.lb = e->lb; a.ub = e->ub; a.kind = e->kindv; a.B_index = e->B_index; a.N_index = e->N_index; a.Nb = e->Nb;
    a.st = e->st; a.m = e->m; a.ld = e->ld; a.nN = e->nN; a.rows_per_block = e->upd2_rows; a.update_u = update_u;
    a.stage_lds = e->upd_stage; a.eps = e->eps;
    a.ill_tol = e->ill_tol;
    a.guard_abs = pivot_guard(e, true);
    a.aq_cur = (MODE == 0 && e->colshard) ? e->aq_cur : nullptr; a.own0 = e->own0; a.own1 = e->own1;
    a.count_iter = (MODE == 0 && e->lagged) ? 0 : 1;
    a.maxviol = e->dual_maxviol;
    a.se_gamma = (MODE == 0 && e->se) ? e->se_gamma : nullptr;
    a.se_rho = (MODE == 0 && e->se) ? e->se_rho : nullptr;
    a.se_vpart = (MODE == 0 && e->se) ? e->se_vpart : nullptr;
    a.trace = trace_of(e);
    const dim3 g(e->upd2_blocks + (MODE == 0 ? 2 : 3)), b(256);
    const size_t lds = MODE == 0 ? e->upd_lds : 0;
    with_row_regs<true>(e->ld, [&](auto NR) { hipLaunchKernelGGL((k_update2<MODE, TV(NR)>), g, b, lds, e->stream, a); });
}

// out = B^-T v (two buffers of out: DevState::usel; the same one twice where there is no other)
void launch_btran(ellp_engine *e, const double *v, double *out0, double *out1) {
    BtranArgs a{e->W, e->W2, v, e->upart, out0, out1, e->st, e->m, e->ld, e->btran_rows, e->btran_tiles};
    const int64_t half = e->ld >> 1;
    dim3 g((unsigned)((half + 255) / 256), (unsigned)e->btran_tiles);
    hipLaunchKernelGGL(k_btran_part, g, dim3(256), 0, e->stream, a);
    hipLaunchKernelGGL(k_btran_reduce, dim3((unsigned)((e->ld + 255) / 256)), dim3(256), 0, e->stream, a);
}
void launch_btran(ellp_engine *e) { launch_btran(e, e->c_B, e->u, e->u + e->ld); }  // u = B^-T c_B

void launch_refactor_columnwise(ellp_engine *e) {
    Prof p(e, ELLP_K_REFACTOR);
    RefArgs a{e->W, e->W2, e->d, e->A_B, e->used, e->perm, e->st, e->m, e->ld, e->upd_rows,
              e->kind == ELLP_ENGINE_PRIMAL ? e->eps : 0.0};
    e->perm_valid = true;
    hipLaunchKernelGGL(k_ref_begin, dim3(1), dim3(1), 0, e->stream, a);
    hipLaunchKernelGGL(k_ref_init, dim3(1024), dim3(256), 0, e->stream, a);
    for (int64_t k = 0; k < e->m; ++k) {
        hipLaunchKernelGGL(k_ref_ftran, dim3(e->ftran_blocks), dim3(256), 0, e->stream, a);
        hipLaunchKernelGGL(k_ref_pick, dim3(1), dim3(1024), 0, e->stream, a);
        hipLaunchKernelGGL(k_ref_update, dim3(e->upd_blocks), dim3(256), 0, e->stream, a);
    }
    hipLaunchKernelGGL(k_ref_permute, dim3((unsigned)e->m), dim3(256), 0, e->stream, a);
    hipLaunchKernelGGL(k_ref_finish, dim3(1), dim3(1), 0, e->stream, a);
    e->refactors += 1;
    e->since_refactor = 0;
    e->u_valid = false;
}

// the k_bl_factor variant of a rebuild of m rows: workgroup size and sub-panel width (read per rebuild)
struct BlFactorVariant {
    int bl_nt, nbw_max;
};
BlFactorVariant bl_factor_variant(int64_t m) {
    BlFactorVariant v;
    v.bl_nt = (getenv("ELLP_BL_NT") && atoi(getenv("ELLP_BL_NT")) == 1024) ? 1024 : 512;
    v.nbw_max = m <= 2048 ? 16 : (m <= 4096 ? 8 : 4);
    if (const char *s = getenv("ELLP_BL_NBW"); s && s[0]) {  // tests: a narrower sub-panel than the size needs
        const int w = atoi(s);
        if ((w == 8 || w == 4) && w < v.nbw_max) v.nbw_max = w;
    }
    return v;
}

// Blocked rebuild (ellp_rebuild.inc).  One host synchronisation: after the probe for a generalised
// permutation matrix (the artificial / slack bases every phase 1 starts from), to know whether the
// general elimination has to be enqueued at all.  Rebuilds are rare (engine creation, a refused refresh).
void launch_refactor(ellp_engine *e) {
    const bool legacy = e->bl_Cpart == nullptr || (getenv("ELLP_REBUILD") && !strcmp(getenv("ELLP_REBUILD"), "columnwise"));
    if (legacy) {
        launch_refactor_columnwise(e);
        return;
    }
    Prof p(e, ELLP_K_REFACTOR);
    const int64_t m = e->m;
    BlArgs a{};
    a.W0 = e->W; a.W1 = e->W2; a.A_B = e->A_B; a.Cpart = e->bl_Cpart; a.C0 = e->bl_C; a.C1 = e->bl_C + m * BL_NB;
    a.V0 = e->bl_V; a.V1 = e->bl_V + m * BL_NB; a.Vs = e->bl_Vs; a.Wp = e->bl_Wp; a.used = e->used; a.perm = e->perm;
    a.Pm = e->bl_Pm; a.st = e->st; a.m = m; a.ld = e->ld; a.splits = e->bl_splits;
    a.ksplit = (int)round_up((m + e->bl_splits - 1) / e->bl_splits, 16);
    a.eps = e->kind == ELLP_ENGINE_PRIMAL ? e->eps : 0.0;
    e->refactors += 1;
    e->since_refactor = 0;
    e->u_valid = false;
    e->perm_valid = false;
    // ---- shortcut: one nonzero per column, distinct rows
    hipLaunchKernelGGL(k_bl_probe, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, e->stream, a, e->bl_nzval, e->bl_nzrow, e->bl_nzcnt);
    hipLaunchKernelGGL(k_bl_perm_check, dim3(1), dim3(1024), 0, e->stream, a, e->bl_nzval, e->bl_nzrow, e->bl_nzcnt);
    hipLaunchKernelGGL(k_bl_perm_fill, dim3((unsigned)m), dim3(256), 0, e->stream, a, e->bl_nzval, e->bl_nzrow);
    DevState probe;
    if (hipMemcpyAsync(&probe, e->st, sizeof(DevState), hipMemcpyDeviceToHost, e->stream) != hipSuccess ||
        hipStreamSynchronize(e->stream) != hipSuccess)
        return;
    static const int32_t zero = 0;  // static: the copy may still be in flight when this function returns
    (void)hipMemcpyAsync(&e->st->do_update, &zero, sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
    if (probe.status != ST_RUNNING) return;  // singular (or the engine is not running: the kernels did nothing)
    if (probe.do_update) {
        e->rebuild_shortcuts += 1;
        return;
    }
    // ---- general case
    e->perm_valid = true;
    RefArgs ra{e->W, e->W2, e->d, e->A_B, e->used, e->perm, e->st, e->m, e->ld, e->upd_rows, a.eps};
    hipLaunchKernelGGL(k_ref_init, dim3(1024), dim3(256), 0, e->stream, ra);
    const auto [bl_nt, nbw_max] = bl_factor_variant(m);
    for (int64_t k0 = 0; k0 < m; k0 += BL_NB) {
        a.k0 = (int)k0;
        a.nbc = (int)((m - k0) < BL_NB ? (m - k0) : BL_NB);
        a.sel = 0;
        hipLaunchKernelGGL(k_bl_gemm1, dim3((unsigned)((m + 63) / 64), (unsigned)a.splits), dim3(256), 0, e->stream, a);
        hipLaunchKernelGGL(k_bl_sum, dim3(256), dim3(256), 0, e->stream, a);
        for (int j0 = 0; j0 < a.nbc; j0 += nbw_max) {
            a.j0 = j0;
            a.nbw = (a.nbc - j0) < nbw_max ? (a.nbc - j0) : nbw_max;
            a.nacc = j0;
            if (bl_nt == 512) {  // two waves per SIMD, 256 VGPRs each: 4 / 8 / 16 rows per thread
                if (nbw_max == 16) hipLaunchKernelGGL((k_bl_factor<16, 4, 512>), dim3(1), dim3(512), 0, e->stream, a);
                else if (nbw_max == 8) hipLaunchKernelGGL((k_bl_factor<8, 8, 512>), dim3(1), dim3(512), 0, e->stream, a);
                else hipLaunchKernelGGL((k_bl_factor<4, 16, 512>), dim3(1), dim3(512), 0, e->stream, a);
            } else {
                if (nbw_max == 16) hipLaunchKernelGGL((k_bl_factor<16, 2, 1024>), dim3(1), dim3(1024), 0, e->stream, a);
                else if (nbw_max == 8) hipLaunchKernelGGL((k_bl_factor<8, 4, 1024>), dim3(1), dim3(1024), 0, e->stream, a);
                else hipLaunchKernelGGL((k_bl_factor<4, 8, 1024>), dim3(1), dim3(1024), 0, e->stream, a);
            }
            hipLaunchKernelGGL(k_bl_apply, dim3((unsigned)((m + 7) / 8)), dim3(256), 0, e->stream, a);
            a.sel ^= 1;
        }
        hipLaunchKernelGGL(k_bl_gather, dim3((unsigned)a.nbc), dim3(256), 0, e->stream, a);
        hipLaunchKernelGGL(k_bl_gemm2, dim3((unsigned)((e->ld + 127) / 128), (unsigned)((m + 63) / 64)), dim3(256), 0, e->stream, a);
    }
    hipLaunchKernelGGL(k_ref_permute, dim3((unsigned)e->m), dim3(256), 0, e->stream, ra);
    hipLaunchKernelGGL(k_ref_finish, dim3(1), dim3(1), 0, e->stream, ra);
}

// One Newton-Schulz step on the current inverse, enqueued without any host synchronisation: the
// residual max|I - A_B W| of the first GEMM is folded on the device (k_resid_reduce), which also
// decides whether the step is safe; if it is not, the step is skipped, DevState::need_rebuild is set
// and the loop stops with a maintenance request that the host services by rebuilding from A_B.
void launch_refresh(ellp_engine *e) {
    Prof p(e, ELLP_K_REFACTOR);
    GemmArgs a{e->W, e->W2, e->A_B, e->T, e->resid, e->st, e->m, e->ld};
    const unsigned nt = (unsigned)((e->m + 127) / 128);
    static const bool valu = [] {  // measurement: ELLP_GEMM=valu runs round 1's vector-ALU GEMM
        const char *v = getenv("ELLP_GEMM");
        return v && strcmp(v, "valu") == 0;
    }();
    if (valu) hipLaunchKernelGGL(k_gemm128<0>, dim3(nt, nt), dim3(256), 0, e->stream, a);
    else hipLaunchKernelGGL(k_gemm_mfma<0>, dim3(nt, nt), dim3(512), 0, e->stream, a);
    hipLaunchKernelGGL(k_resid_reduce, dim3(1), dim3(256), 0, e->stream, a, (int)(nt * nt));
    if (valu) hipLaunchKernelGGL(k_gemm128<1>, dim3(nt, nt), dim3(256), 0, e->stream, a);
    else hipLaunchKernelGGL(k_gemm_mfma<1>, dim3(nt, nt), dim3(512), 0, e->stream, a);
    hipLaunchKernelGGL(k_copy_to_other, dim3(1024), dim3(256), 0, e->stream, a);
    hipLaunchKernelGGL(k_refresh_finish, dim3(1), dim3(1), 0, e->stream, a);
    e->refreshes += 1;
    e->since_refactor = 0;
    e->u_valid = false;
}

// periodic maintenance of B^-1: Newton-Schulz refresh, full rebuild only if that is not safe
void launch_dleave(ellp_engine *e);
void launch_resync(ellp_engine *e, int force);

// tvec = b - A_N x_N: the front of the resync, and of the primal phase-1 start (its b~)
ResyncArgs launch_resync_rhs(ellp_engine *e, int force) {
    ResyncArgs a{e->A_N, e->W, e->W2, e->b_dev, e->x, e->xg, e->tvec, e->upart, e->cand, e->maxbits, e->B_index,
                 e->N_index, e->st, e->m, e->ld, e->nN, 0, e->btran_tiles, force};
    a.cols_per_tile = (int)((e->nN + e->btran_tiles - 1) / e->btran_tiles);
    const int64_t half = e->ld >> 1;
    hipLaunchKernelGGL(k_resync_gather, dim3((unsigned)((e->nN + 255) / 256)), dim3(256), 0, e->stream, a);
    hipLaunchKernelGGL(k_resync_part, dim3((unsigned)((half + 255) / 256), (unsigned)e->btran_tiles), dim3(256), 0,
                       e->stream, a);
    hipLaunchKernelGGL(k_resync_rhs, dim3((unsigned)((e->ld + 255) / 256)), dim3(256), 0, e->stream, a);
    return a;
}

// x_B from the freshly maintained B^-1 (see k_resync_part)
void launch_resync(ellp_engine *e, int force) {
    if (e->nN <= 0) return;
    if (e->colshard) return;  // b - A_N x_N would need every rank's columns (a reduction over the ranks): not done
    const ResyncArgs a = launch_resync_rhs(e, force);  // k_resync_rhs also zeroes maxbits
    hipLaunchKernelGGL(k_resync_xb, dim3((unsigned)((e->m + 3) / 4)), dim3(256), 0, e->stream, a);
    hipLaunchKernelGGL(k_resync_apply, dim3((unsigned)((e->m + 255) / 256)), dim3(256), 0, e->stream, a);
    if (e->kind == ELLP_ENGINE_DUAL) launch_dleave(e);  // the leaving row is chosen from x (dual…:200-236)
    e->resyncs += 1;
    if (getenv("ELLP_RESYNC_DEBUG")) {  // diagnostics: what the resync found
        unsigned long long hb[2] = {0, 0};
        (void)hipMemcpyAsync(hb, e->maxbits, sizeof(hb), hipMemcpyDeviceToHost, e->stream);
        (void)hipStreamSynchronize(e->stream);
        double dv[2];
        memcpy(dv, hb, sizeof(dv));
        fprintf(stderr, "ellp resync %llu: max|cand - x_B| %.3e, max|x_B| %.3e\n", (unsigned long long)e->resyncs, dv[0], dv[1]);
    }
}

// Maintenance of B^-1: Newton-Schulz refresh, full rebuild if that is not safe, then x_B is checked
// against the fresh inverse (launch_resync).  `reactive` (asked for by the device, or the follow-up of
// such a request) is kept for diagnostics: resynchronising only then was tried and is worse (netlib
// ADLITTLE / BLEND in 60 variable orders, dual: 4 wrong outcomes instead of 1).
void launch_dual_close(ellp_engine *e);
void maintain_inverse(ellp_engine *e, bool reactive = false, bool rebuild = false) {
    // two-launch pipeline: an open iteration (priced, FTRAN done, ratio test not folded) was decided with
    // the inverse that is about to be replaced — drop it; the next k_price2 starts afresh (use_pend = 0) and
    // the iteration is priced again from the maintained inverse.  Its eta-update half is already in B^-1.
    launch_dual_close(e);  // a fused dual iteration is completed, not dropped: its pivot is in B^-1 already
    if (e->lagged) hipLaunchKernelGGL(k_drop_open, dim3(1), dim3(1), 0, e->stream, e->st);
    e->lag_open = false;
    if (rebuild) launch_refactor(e);
    else launch_refresh(e);
    const char *mode = getenv("ELLP_RESYNC");  // diagnostics: "0" never, "1" only on reactive maintenance
    const bool want = mode && mode[0] == '0' ? false : (mode && mode[0] == '1' ? reactive : true);
    if (want) launch_resync(e, 0);
}

// After a read-back with the stream drained: iterations that were enqueued behind a stop (a final
// status or a maintenance request) returned at entry and did not happen, but the host counted them
// when it enqueued them.  Take them back, so that the maintenance schedule follows the iterations
// that really ran (DevState::iters counts every loop body entered).
void reconcile_counters(ellp_engine *e) {
    const uint64_t ran = e->h_st->iters >= e->iters_seen ? e->h_st->iters - e->iters_seen : 0;
    const uint64_t lost = e->enqueued > ran ? e->enqueued - ran : 0;
    if (lost) {
        e->since_refactor = e->since_refactor > lost ? e->since_refactor - lost : 0;
        e->since_btran = e->since_btran > lost ? e->since_btran - lost : 0;
        e->since_drift = e->since_drift > lost ? e->since_drift - lost : 0;
    }
    e->enqueued = 0;
    e->iters_seen = e->h_st->iters;
}

// two-launch pipeline: k_ftran_eta reports the end of the solve in DevState::fin and leaves it to the next
// kernel's leader to make it the status; after a drained read-back the host can do that itself
void adopt_fin(ellp_engine *e) {
    if (e->h_st->status != ST_RUNNING || !e->h_st->fin) return;
    static int32_t fin_status;  // static: asynchronous copy
    fin_status = e->h_st->fin - 1;
    (void)hipMemcpyAsync(&e->st->status, &fin_status, sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
    (void)hipStreamSynchronize(e->stream);
    e->h_st->status = fin_status;
}

// The state read-back: DevState as it stands behind everything enqueued so far, into h_st, with the stream drained.  Every
// caller turns the error into its own return value.  (ellp_engine_run's look-ahead slots and the copies that ride along
// with other copies in front of one synchronisation are not this: they do not drain the stream at once.)
hipError_t read_state(ellp_engine *e) {
    const hipError_t rc = hipMemcpyAsync(e->h_st, e->st, sizeof(DevState), hipMemcpyDeviceToHost, e->stream);
    return rc != hipSuccess ? rc : hipStreamSynchronize(e->stream);
}
// ... and what a loop that enqueues iterations ahead of its read-backs does with it before it looks at the status
void settle_state(ellp_engine *e) {
    reconcile_counters(e);
    adopt_fin(e);
}

// ---- a stopped engine made ready again: the DevState a hand-off (ellp_phase.inc) or a re-arm inside ellp_engine_run
// (ellp_run.inc) uploads is the drained one with some groups of fields cleared.  One function per group; a site calls the
// groups it clears and says which it leaves, and why.
// the words every kernel tests at entry, and the requests and codes that come with a stop
inline void clear_stop_words(DevState &s) {
    s.status = ST_RUNNING;
    s.nan_flag = 0;
    s.tiny = 0;
    s.need_rebuild = 0;
    s.panic_code = 0;
}
// two-launch pipeline: what one launch leaves for the next one's leader (a tiny pivot, the final status)
inline void clear_relays(DevState &s) { s.tiny_p = s.fin = 0; }
// two-launch pipeline: the iteration nobody has folded yet, its pending eta update and column move
inline void clear_open_iteration(DevState &s) { s.open = s.pe_valid = s.mv_pending = 0; }
// a new solve_with_initial counts from zero
inline void clear_counts(DevState &s) { s.iters = s.pivots = s.flips = 0; }
// partial pricing starts over with the first segment
inline void restart_pricing_window(DevState &s, const ellp_engine *e) {
    s.pp_seg = s.pp_empty = s.pp_skip = 0;
    s.pp_lo = 0;
    s.pp_hi = e->pp_P > 1 ? e->pp_S : e->nN;
}
// the state becomes the host's copy and its upload is enqueued
inline hipError_t store_state(ellp_engine *e, const DevState &s) {
    *e->h_st = s;
    return hipMemcpyAsync(e->st, e->h_st, sizeof(DevState), hipMemcpyHostToDevice, e->stream);
}
// ... and the host's side of it: nothing is enqueued, no follow-up refresh is due, DevState::iters stands at `iters`
inline void nothing_enqueued(ellp_engine *e, uint64_t iters) {
    e->maint_chain = 0;
    e->enqueued = 0;
    e->iters_seen = iters;
}
// a new phase starts here: its counters at zero, the old phase's snapshot dropped, and the fast loop again unless the caller
// chose the exact loop (pipeline 3)
inline void begin_phase(ellp_engine *e) {
    nothing_enqueued(e, 0);
    e->snap.valid = false;
    e->exact_large_only = e->exact_large_always;
}

// A device temporary of one host function: hipMalloc on request; on every way out the stream that may still read it is
// drained and the buffer freed.  release(): the engine adopts the buffer (replace_alloc).
template <typename T>
struct DevTemp {
    hipStream_t stream;
    T *p = nullptr;
    explicit DevTemp(hipStream_t s) : stream(s) {}
    DevTemp(DevTemp &&o) noexcept : stream(o.stream), p(o.release()) {}
    DevTemp &operator=(DevTemp &&) = delete;  // move-only: no copy either
    ~DevTemp() {
        if (!p) return;
        (void)hipStreamSynchronize(stream);
        (void)hipFree(p);
    }
    hipError_t alloc(size_t count) { return hipMalloc(reinterpret_cast<void **>(&p), sizeof(T) * (count ? count : 1)); }
    T *release() {
        T *q = p;
        p = nullptr;
        return q;
    }
    operator T *() const { return p; }
};

// DevState::obj = c . x of a primal engine (one small launch; the next read-back brings it)
void launch_primal_obj(ellp_engine *e) {
    hipLaunchKernelGGL(k_primal_obj, dim3(1), dim3(1024), 0, e->stream, e->c_B, e->c_N, e->x, e->B_index, e->N_index, e->m, e->nN,
                       e->st);
}

// After a status read-back: if a kernel asked for maintenance, do it, re-arm the loop and report
// true (the caller keeps going).  The pivot that raised the request is committed (k_update2 raises the
// flag after its bookkeeping); what is void is the rest of the batch behind it.  The device is
// re-armed (status = RUNNING, tiny = 0) BEFORE the maintenance kernels are enqueued: all of them
// (k_gemm128, k_copy_to_other, k_ref_*, k_dleave) return at entry on any other status, so servicing
// the request under ST_NEED_MAINT would refresh nothing and re-select the dual's leaving row from
// nothing.
bool service_maintenance_request(ellp_engine *e) {
    // the request is the status (a later pricing launch of the batch saw the flag) or still the flag
    // (the batch ended with the k_update2 that raised it)
    if (e->h_st->status != ST_NEED_MAINT && !(e->h_st->status == ST_RUNNING && e->h_st->tiny)) return false;
    const int32_t running = ST_RUNNING, zero = 0;
    const bool rebuild = e->h_st->need_rebuild != 0;  // a refresh found B^-1 too far off for Newton-Schulz
    // three words, not store_state: that would upload the whole struct where this copies twelve bytes
    (void)hipMemcpyAsync(&e->st->status, &running, sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
    (void)hipMemcpyAsync(&e->st->tiny, &zero, sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
    (void)hipMemcpyAsync(&e->st->need_rebuild, &zero, sizeof(int32_t), hipMemcpyHostToDevice, e->stream);
    e->h_st->status = ST_RUNNING;
    e->h_st->tiny = 0;
    e->h_st->need_rebuild = 0;
    maintain_inverse(e, true, rebuild);
    e->maint_chain = 1;
    (void)hipStreamSynchronize(e->stream);
    e->maint_requests += 1;
    return true;
}

// between k_ftran2 and k_update2 of an iteration: see k_drift_part
void launch_drift_check(ellp_engine *e) {
    if (e->drift_every <= 0) return;
    if (++e->since_drift < (uint64_t)e->drift_every) return;
    e->since_drift = 0;
    e->drift_checks += 1;
    DriftArgs a{e->A_B, e->A_N, e->d, e->colshard ? e->aq_cur : nullptr, e->upart, e->st, e->m, e->ld, e->btran_rows, e->btran_tiles, e->drift_tol};
    const int64_t half = e->ld >> 1;
    hipLaunchKernelGGL(k_drift_part, dim3((unsigned)((half + 255) / 256), (unsigned)e->btran_tiles), dim3(256), 0,
                       e->stream, a);
    hipLaunchKernelGGL(k_drift_reduce, dim3((unsigned)((e->m + WAVE - 1) / WAVE)), dim3(WAVE), 0, e->stream, a);
}

// ---- two-launch pipeline (ellp_lagged.inc) -------------------------------------------------------
void launch_price2(ellp_engine *e, int use_pend) {
    Price2Args a{};
    a.p.A_N = e->A_N; a.p.W0 = e->W; a.p.W1 = e->W2; a.p.u = nullptr; a.p.c_N = e->c_N; a.p.Nb = e->Nb;
    a.p.N_index = e->N_index; a.p.dd = nullptr; a.p.xc = xchg_of(e); a.p.st = e->st;
    a.p.ld = e->ld; a.p.nN = e->nN; a.p.cpb = e->cpb; a.p.block0 = e->rank * e->nbs; a.p.eps = e->eps;
    a.p.vs_row = e->vs_row; a.p.vs_val = e->vs_val; a.pos_hint = e->pos_hint;
    a.u0 = e->u; a.u1 = e->u + e->ld; a.W0 = e->W; a.W1 = e->W2;
    a.d = e->d; a.lam = e->lam; a.bmin = e->bmin; a.bsec = e->bmin + e->m; a.bidx = e->bidx; a.binfo = e->binfo; a.dpos = e->dpos;
    a.A_N = e->A_N; a.A_B = e->A_B; a.aq_save = e->aq_save; a.c_B = e->c_B; a.c_N = e->c_N; a.x = e->x;
    a.lb = e->lb; a.ub = e->ub; a.kind = e->kindv; a.B_index = e->B_index; a.N_index = e->N_index; a.Nb = e->Nb;
    a.m = e->m; a.rpb = e->upd2_rows; a.use_pend = use_pend; a.ill_tol = e->ill_tol;
    a.guard_abs = pivot_guard(e, false);
    a.aq_cur = e->colshard ? e->aq_cur : nullptr; a.own0 = e->own0; a.own1 = e->own1;
    a.trace = trace_of(e);
    int mine = e->nblocks - a.p.block0;
    if (mine > e->nbs) mine = e->nbs;
    if (mine < 0) mine = 0;
    const dim3 g(mine + P2_BOOK), b(256);
    const size_t lds = e->price2_lds;
    with_bool(e->colshard, [&](auto SH) {  // SH: the sharded instantiations (ellp_lagged.inc)
        if (e->price_wave) {
            hipLaunchKernelGGL((k_price2_wave<TV(SH)>), g, b, lds + sizeof(double) * (size_t)e->ld, e->stream, a);
            return;
        }
        with_bool(e->price_nt, [&](auto NT) {
            with_price_tile(e->priceT, [&](auto T) { hipLaunchKernelGGL((k_price2<TV(T), TV(NT), TV(SH)>), g, b, lds, e->stream, a); });
        });
    });
}

void launch_ftran_eta(ellp_engine *e) {
    FtranEtaArgs a{};
    a.W0 = e->W; a.W1 = e->W2; a.A_N = e->A_N; a.xc = xchg_of(e);
    a.N_index = e->N_index; a.B_index = e->B_index; a.Nb = e->Nb; a.kind = e->kindv;
    a.x = e->x; a.lb = e->lb; a.ub = e->ub; a.d = e->d; a.lam = e->lam; a.bmin = e->bmin; a.bsec = e->bmin + e->m; a.bidx = e->bidx;
    a.binfo = e->binfo; a.dpos = e->dpos;
    a.A_B = e->A_B; a.c_B = e->c_B; a.aq_save = e->aq_save; a.st = e->st; a.m = e->m; a.ld = e->ld; a.nN = e->nN;
    a.nblocks = e->nblocks; a.cpb = e->cpb; a.rows_per_block = e->upd2_rows; a.eps = e->eps;
    if (e->colshard) {
        a.aq_cur = e->aq_cur; a.aq_out = e->aq_cur;
        if (e->sel_in_ftran) {
            a.sel_packs = e->packs; a.sel_world = e->world; a.mbox_commit = e->sel_commit ? 1 : 0;
        }
    }
    const dim3 g(e->upd2_blocks + 1);
    // unsharded, rows in registers up to 2,048 doubles (NR 1, 2, 4): a fifth wave folds and hands the entering column to the
    // four that stream the rows through LDS (+8 ld bytes); the sharded instantiations select in the prologue instead
    const size_t hand_lds = ftran_col_offset(e->nblocks) + sizeof(double) * (size_t)e->ld;
    static_assert(ftran_eta_threads(1, false) == FTRAN_HAND_THREADS && ftran_eta_threads(4, false) == FTRAN_HAND_THREADS &&
                      ftran_eta_threads(8, false) == 256 && ftran_eta_threads(4, true) == 256,
                  "320 threads exactly where hand_lds is used");
    with_bool(e->colshard, [&](auto SH) {
        with_row_regs<true>(e->ld, [&](auto NR) {
            constexpr bool hand = ftran_eta_hands_off(TV(NR), TV(SH));
            hipLaunchKernelGGL((k_ftran_eta<TV(NR), TV(SH)>), g, dim3(ftran_eta_threads(TV(NR), TV(SH))),
                               hand ? hand_lds : e->ftran_lds, e->stream, a);
        });
    });
}

// iteration k of the two-launch pipeline: P_k folds and books iteration k-1 (if one is open), prices k;
// F_k applies the eta of k-1 and forms d_k.  Iteration k itself stays open until the next P or the flush.
void launch_primal_iteration_lagged(ellp_engine *e) {
    const bool full_btran = !e->u_valid || e->since_btran >= (uint64_t)e->btran_refresh;
    if (full_btran) {
        // u = B^-T c_B from the materialised inverse: W and c_B both stand at "all pivots but the open one",
        // exactly the u_{k-1} that P_k advances by the open pivot's rank-1 term
        Prof p(e, ELLP_K_BTRAN);
        launch_btran(e);
        e->since_btran = 0;
        e->u_valid = true;
    }
    {
        Prof p(e, ELLP_K_PRICE);
        launch_price2(e, e->lag_open ? 1 : 0);
    }
    {
        Prof p(e, ELLP_K_FTRAN);
        launch_ftran_eta(e);
    }
    launch_drift_check(e);
    e->lag_open = true;
    e->since_btran += 1;
    e->since_refactor += 1;
    e->enqueued += 1;
}

// closing kernel of a slice: k_update2 folds the open iteration's ratio test, applies its eta update and
// does its bookkeeping (the three-launch path's third kernel, unchanged)
void launch_dual_close(ellp_engine *e);
void launch_flush(ellp_engine *e) {
    launch_dual_close(e);
    if (!e->lag_open) return;
    {
        Prof p(e, ELLP_K_UPDATE);
        launch_update2<0>(e, 1);
    }
    e->lag_open = false;
}

void launch_price_se(ellp_engine *e) {
    SeArgs a{};
    a.A_N = e->A_N; a.u = e->u; a.rho = e->se_rho; a.v = e->se_v; a.c_N = e->c_N; a.Nb = e->Nb; a.N_index = e->N_index;
    a.gamma = e->se_gamma;
    const bool unit_ok = !(e->opts.flags & ELLP_FLAG_DENSE_PRICING);
    a.vs_row = unit_ok ? e->vs_row : nullptr; a.vs_val = unit_ok ? e->vs_val : nullptr;
    a.xc = xchg_of(e); a.st = e->st; a.ld = e->ld; a.nN = e->nN; a.cpb = e->cpb; a.eps = e->eps;
    hipLaunchKernelGGL(k_price_se, dim3((unsigned)e->nblocks), dim3(256), 0, e->stream, a);
}

void launch_primal_iteration(ellp_engine *e) {
    if (e->lagged) {
        launch_primal_iteration_lagged(e);
        return;
    }
    const bool full_btran = (e->opts.btran_mode == 1) || !e->u_valid || e->since_btran >= (uint64_t)e->btran_refresh;
    if (full_btran) {
        Prof p(e, ELLP_K_BTRAN);
        launch_btran(e);
        e->since_btran = 0;
        e->u_valid = true;
    }
    {
        Prof p(e, ELLP_K_PRICE);
        if (e->se) launch_price_se(e);
        else launch_price<0>(e);
    }
    {
        Prof p(e, ELLP_K_FTRAN);
        launch_ftran2<0>(e);
    }
    if (e->se && !e->se_vpart) {  // v = B^-T d from the inverse this iteration's FTRAN used: the weight update of the NEXT pricing launch
        Prof p(e, ELLP_K_BTRAN);
        launch_btran(e, e->d, e->se_v, e->se_v);
    }
    launch_drift_check(e);
    {
        Prof p(e, ELLP_K_UPDATE);
        launch_update2<0>(e, e->opts.btran_mode == 1 ? 0 : 1);
    }
    if (e->se && e->se_vpart) {  // v = the row blocks' partial sums of k_update2, added in block order
        Prof p(e, ELLP_K_BTRAN);
        hipLaunchKernelGGL(k_se_vreduce, dim3((unsigned)((e->ld + 15) / 16)), dim3(256), 0, e->stream, e->se_vpart, e->se_v, e->st, e->ld,
                           e->upd2_blocks);
    }
    e->since_btran += 1;
    e->since_refactor += 1;
    e->enqueued += 1;
}

// the closing block of the fused dual iteration in front (a no-op on the device if that has been closed already)
void launch_dual_close(ellp_engine *e) {
    if (!e->dual_open) return;
    Prof p(e, ELLP_K_DUPDATE);
    DualCloseArgs c{e->d, e->A_N, e->A_B, e->c_B, e->c_N, e->x, e->dd, e->B_index, e->N_index, e->Nb, e->binfo, e->bmin,
                    e->bmin + e->m, (int)((e->m + UPD_ROWS - 1) / UPD_ROWS), e->st, e->m, e->ld, e->ill_tol,
                    trace_of(e), e->dual_maxviol};
    hipLaunchKernelGGL(k_dual_close, dim3(1), dim3(256), 0, e->stream, c);
    e->dual_open = false;
}

// FTRAN + eta update + x_B / d_N / y updates in one pass (ellp_dualfu.inc); the iteration stays open
void launch_dual_fu(ellp_engine *e) {
    Prof p(e, ELLP_K_FTRAN);
    DualFuArgs a{};
    a.W0 = e->W; a.W1 = e->W2; a.A_N = e->A_N; a.xc = xchg_of(e);
    a.N_index = e->N_index; a.B_index = e->B_index; a.x = e->x; a.d = e->d; a.y = e->y; a.dd = e->dd;
    a.lb = e->lb; a.ub = e->ub; a.kind = e->kindv; a.lrow = e->binfo; a.ldelta = e->bmin; a.lside = e->bmin + e->m;
    a.st = e->st; a.m = e->m; a.ld = e->ld; a.nN = e->nN; a.nblocks = e->nblocks; a.eps = e->eps;
    a.seq = e->dual_seq;
    a.maxviol = e->dual_maxviol;
    a.guard_abs = pivot_guard(e, false);
    const dim3 g((unsigned)((e->m + UPD_ROWS - 1) / UPD_ROWS) + DFU_BOOK), b(256);
    with_row_regs<false>(e->ld, [&](auto NR) { hipLaunchKernelGGL((k_dual_fu<TV(NR)>), g, b, 0, e->stream, a); });
    e->dual_open = true;
}

void launch_dual_iteration(ellp_engine *e) {
    e->dual_seq += 1;
    {
        Prof p(e, ELLP_K_DPRICE);
        // closes the fused iteration in front of it if this engine folds the closing work (dual_fold) — unless it
        // returns at entry on a stop, so the host keeps dual_open until a k_dual_close has been enqueued (which does
        // nothing on the device when the iteration is closed already)
        launch_price<1>(e);
    }
    // the drift monitor compares A_B alpha_q with a_q between FTRAN and the update: those iterations keep the
    // three-launch form (both forms leave the same state behind)
    const bool drift_now = e->drift_every > 0 && e->since_drift + 1 >= (uint64_t)e->drift_every;
    if (e->dual_fused && !drift_now) {
        if (e->drift_every > 0) e->since_drift += 1;
        launch_dual_fu(e);
        if (!e->dual_fold) launch_dual_close(e);
        e->since_refactor += 1;
        e->enqueued += 1;
        return;
    }
    {
        Prof p(e, ELLP_K_FTRAN);
        launch_ftran2<1>(e);
    }
    launch_drift_check(e);
    {
        Prof p(e, ELLP_K_DUPDATE);
        launch_update2<1>(e, 0);
    }
    e->since_refactor += 1;
    e->enqueued += 1;
}

void launch_dleave(ellp_engine *e) {
    Prof p(e, ELLP_K_DLEAVE);
    DLeaveArgs a{e->x, e->lb, e->ub, e->kindv, e->B_index, e->st, e->m, e->eps, e->dual_maxviol};
    hipLaunchKernelGGL(k_dleave, dim3(1), dim3(256), 0, e->stream, a);
}

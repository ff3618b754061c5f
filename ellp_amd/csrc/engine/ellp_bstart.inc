// ellp_bstart.inc — ellp_batch_basis_start: the starting points of many small LPs from their bases, one workgroup per LP.
// DESIGN.md §3.11b.
//
// k_start_batch does for its item, without a host decision in between, everything ellp_basis_start (ellp_start.inc) does in
// about 37 launches besides the LU's and one blocking read-back per refinement pass: the basis into LDS, its LU and the
// refined y (bpost_solve_y, k_post_batch's), d_N, the labels and the nonbasic values, t = b - A_N x_N, x_B = B^-1 t with the
// singleton rows snapped, the refinement loop of x_B with the host's stop rule, and r.  k_start_report_batch then runs
// post_report and start_verdict once per item, with the single call's 1,024 threads.  Two launches per chunk, whatever the
// item count; one upload and one read-back per chunk.  The driver (budget, chunks, device, the pinned staging buffer, the
// slab) and the buffer pool are ellp_batch.inc's.
//
// Every output is, bit for bit, what ellp_basis_start returns for the item alone.  The orders of y, d, r and omega are
// those ellp_bpost.inc lists; on top of them
//   t      from (b_i, 0) the nonbasic blocks of the pass merged as (-s_k, -c_k) in block order (k_post_rfold); t_i = s + c;
//   x_B    k_lu_solve mode 0 on small_lu's factors (small_lu_solve: the recorded swaps in order; L by columns,
//          s_r = (-s_i) L[r][i] + s_r, skipped where s_i == 0; U from the last column, coeff = s_i / U_ii first);
//   snap   x_k = t_i / a for a row i of A_B whose only nonzero is a, at position k; after the solve and after every step;
//   res    from (t_i, 0) the basic blocks of the pass over A_B with the current x, in block order;
//   den    |t_i| + (sum over j ascending, from 0.0, of |A_B[i][j]| |x_B[j]|): one chunk of START_XC columns, m <= 128;
//   r      from (b_i, 0) the basic blocks of the LAST pass over A_B, then the nonbasic blocks.  The nonbasic block sums are
//          made before the x loop and needed after it: they are kept in the item's slab region (rkeep, 16 m bytes per
//          block of 64 columns, written once and read once) — reading A_N again would cost 512 ld bytes per block;
//   changed an integer sum.
// x lives in the slab: the pass reads x[var] from there, so every change of x_B is stored and fenced before the next pass.
//
// LDS at 128 rows: bpost_lds_bytes(128) is 151,552 bytes.  Of the about 6.5 KB a start adds, sv (the vector of a solve:
// the residual goes in, the step comes out), sval and srow (the ROW singletons, scanned from A_B in the slab once y is
// final and the column singletons are dead) are reused; t and x_B are the two vectors that are new: 2,048 bytes, 153,600
// in all, the cap.
//
// Included at the end of ellp_engine.hip, after ellp_bpost.inc and ellp_start.inc.

namespace {

constexpr int BSTART_EXTRA = 2;  // t and x_B in LDS besides k_post_batch's vectors

struct StartBatchArgs {
    const double *A_B, *A_N, *c_N;
    double *x, *y, *d, *r, *rho, *omega, *xomega;
    double *rkeep;  // the nonbasic block sums of r: [block][BPOST_ROWS][2]
    uint8_t *Nb;
    int32_t *steps, *xsteps;
    long long *changed;
    int *fail;
    StartVerdict *verdict;
    int64_t ld;
    int by_d;
    double eps;
    PostReportArgs rep;  // the item as the report sees it; rep.x = x, rep.Nb = Nb
};

// x_k = t_i / a on the singleton rows (k_start_snap), then x_B into x (k_start_axpy's store); the stores are visible to the
// workgroup's next pass on return
__device__ __forceinline__ void bstart_snap_store(const int32_t *rs_pos, const double *rs_val, const double *t, double *xb, double *x,
                                                  int64_t var, int m, int tid) {
    __syncthreads();
    if (tid < m && rs_pos[tid] >= 0) xb[rs_pos[tid]] = t[tid] / rs_val[tid];
    __syncthreads();
    if (tid < m) x[var] = xb[tid];
    __threadfence_block();
    __syncthreads();
}

__global__ __launch_bounds__(BPOST_NT) void k_start_batch(const StartBatchArgs *__restrict__ args) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ double s_bc[2];
    __shared__ double s_xomega;
    __shared__ int s_plen, s_ok, s_changed;
    const StartBatchArgs &a = args[blockIdx.x];  // by reference: a pointer is fetched where it is used, not held in a scalar register
    const int tid = threadIdx.x, lane = tid & 63;
    const int m = (int)a.rep.m;
    const int64_t ld = a.ld, nN = a.rep.nN;
    const BpostSh sh = bpost_carve(smem, m, BSTART_EXTRA);
    double *tsh = sh.extra, *xb = sh.extra + m;
    // ---- 1: the LU and y (x is zero: d on the basis is c_B - A_B^T y whatever x holds)
    double omega = 0.0, fs = 0.0, fc = 0.0;
    int32_t steps = 0;
    if (tid == 0) s_changed = 0;
    if (!bpost_solve_y(sh, a.A_B, a.rep, a.x, a.d, m, ld, &s_plen, s_bc, omega, steps, tid)) {
        if (tid == 0) *a.fail = 1;
        return;
    }
    // y is final: rho, den and d on the basis keep their bits in every later pass over A_B; store what the report reads
    if (tid < m) {
        a.y[tid] = sh.ysh[tid];
        a.rho[tid] = sh.rho[tid];
    }
    // ---- 2: LABELS_BY_D needs d_N first (x is still zero)
    if (a.by_d) {
        bpost_pass<false>(a.A_N, a.rep.N_index, a.c_N, a.x, a.d, m, ld, nN, sh.ysh, sh.rho, sh.den, sh.rbas, sh.rsh, nullptr, fs, fc, tid);
        __threadfence_block();
        __syncthreads();
    }
    // ---- 3: labels and nonbasic values, the basic entries of x at +0.0 (k_start_labels)
    {
        int ch = 0;
        for (int64_t j = tid; j < nN; j += BPOST_NT) {
            const int64_t v = a.rep.N_index[j];
            const int old = a.Nb[j];
            int label;
            double val;
            start_label(a.rep.kind, a.rep.lb, a.rep.ub, a.d, a.by_d, v, old, label, val);
            a.x[v] = val;
            a.Nb[j] = (uint8_t)label;
            ch += label != old;
        }
        if (ch) atomicAdd(&s_changed, ch);
    }
    const int64_t var = tid < m ? a.rep.B_index[tid] : 0;
    if (tid < m) a.x[var] = 0.0;
    __threadfence_block();
    __syncthreads();
    // ---- 4: d_N (LABELS_BY_D: the same bits again) and t, the fold of the nonbasic blocks from (b_i, 0)
    if (tid < m) {
        fs = a.rep.b[tid];
        fc = 0.0;
    }
    bpost_pass<false>(a.A_N, a.rep.N_index, a.c_N, a.x, a.d, m, ld, nN, sh.ysh, sh.rho, sh.den, sh.rbas, sh.rsh, a.rkeep, fs, fc, tid);
    // ---- 5, 6: x_B = B^-1 t, the singleton rows of A_B (k_start_rowsing: the columns in ascending order)
    int32_t *rs_pos = sh.srow;  // the column singletons are dead once y is final
    double *rs_val = sh.sval;
    if (tid < m) {
        const double t = fs + fc;
        tsh[tid] = t;
        sh.sv[tid] = t;
        int cnt = 0, pos = -1;
        double val = 0.0;
        for (int j = 0; j < m; ++j) {
            const double v = a.A_B[j * ld + tid];
            if (v != 0.0) {  // a NaN counts
                cnt += 1;
                pos = j;
                val = v;
            }
        }
        rs_pos[tid] = cnt == 1 ? pos : -1;
        rs_val[tid] = cnt == 1 ? val : 0.0;
    }
    __syncthreads();
    small_lu_solve<BPOST_NT>(sh.LU, m, sh.sv, sh.pa, sh.pb, &s_plen, &s_ok, s_bc, tid);
    if (tid < m) xb[tid] = sh.sv[tid];
    bstart_snap_store(rs_pos, rs_val, tsh, xb, a.x, var, m, tid);
    // ---- 7: the refinement loop of x_B, ellp_basis_start's
    const double two_u = 2.220446049250313e-16;  // 2 u, u = 2^-53
    const int nbb = (m + 63) / 64;
    double xomega = 0.0, last = 0.0;
    int32_t xsteps = 0;
    for (;;) {
        bpost_pass<true>(a.A_B, a.rep.B_index, sh.cB, a.x, a.d, m, ld, m, sh.ysh, sh.rho, sh.den, sh.rbas, sh.rsh, nullptr, fs, fc, tid);
        double res = 0.0;
        if (tid < m) {
            double s = tsh[tid], c = 0.0;  // k_post_rfold over the basic blocks, from t
            for (int k = 0; k < nbb; ++k) post_merge(s, c, -sh.rbas[(k * BPOST_ROWS + tid) * 2], -sh.rbas[(k * BPOST_ROWS + tid) * 2 + 1]);
            res = s + c;
            double part = 0.0;  // k_start_xden, one chunk
            for (int j = 0; j < m; ++j) part += fabs(a.A_B[j * ld + tid]) * fabs(xb[j]);
            double den = fabs(tsh[tid]);  // k_start_omega
            den += part;
            sh.sv[tid] = post_ratio(res, den);
        }
        __syncthreads();
        if (tid < 64) {
            PostMax mine{0.0, LLONG_MAX_POST};
            for (int i = lane; i < m; i += 64) mine = post_max(mine, PostMax{sh.sv[i], (long long)i});
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                PostMax o;
                o.v = __shfl_xor(mine.v, off);
                o.i = __shfl_xor(mine.i, off);
                mine = post_max(mine, o);
            }
            if (lane == 0) s_xomega = mine.v;
        }
        __syncthreads();
        xomega = s_xomega;
        if (!(xomega > two_u) || xsteps >= 4 || (xsteps > 0 && !(xomega <= 0.5 * last))) break;
        if (tid < m) sh.sv[tid] = res;
        __syncthreads();
        small_lu_solve<BPOST_NT>(sh.LU, m, sh.sv, sh.pa, sh.pb, &s_plen, &s_ok, s_bc, tid);
        if (tid < m) xb[tid] = xb[tid] + sh.sv[tid];
        bstart_snap_store(rs_pos, rs_val, tsh, xb, a.x, var, m, tid);
        last = xomega;
        xsteps += 1;
    }
    // ---- 8: r from b: the basic blocks of the last pass, then the nonbasic blocks as kept
    if (tid < m) {
        fs = a.rep.b[tid];
        fc = 0.0;
        for (int k = 0; k < nbb; ++k) post_merge(fs, fc, -sh.rbas[(k * BPOST_ROWS + tid) * 2], -sh.rbas[(k * BPOST_ROWS + tid) * 2 + 1]);
        const int64_t nbn = (nN + 63) / 64;
        for (int64_t k = 0; k < nbn; ++k) post_merge(fs, fc, -a.rkeep[(k * BPOST_ROWS + tid) * 2], -a.rkeep[(k * BPOST_ROWS + tid) * 2 + 1]);
        a.r[tid] = fs + fc;
    }
    if (tid == 0) {
        *a.omega = omega;
        *a.steps = steps;
        *a.xomega = xomega;
        *a.xsteps = xsteps;
        *a.changed = (long long)s_changed;
    }
}

__global__ __launch_bounds__(1024) void k_start_report_batch(const StartBatchArgs *args) {
    const StartBatchArgs &a = args[blockIdx.x];
    if (*a.fail) return;  // uniform over the workgroup
    post_report(a.rep, *a.steps);
    StartVerdictArgs va{};
    va.x = a.x; va.lb = a.rep.lb; va.ub = a.rep.ub; va.kind = a.rep.kind; va.B_index = a.rep.B_index; va.kkt = a.rep.out; va.m = a.rep.m;
    va.eps = a.eps;
    va.out = a.verdict;
    start_verdict(va);  // thread 0 wrote the report and is the one that reads it
}

// one item on the batched kernel: its share of the slab (byte offsets in its chunk's slab)
struct BstartPlan {
    int64_t item;
    int64_t ld, nNa, nbn;
    size_t lds;
    size_t o_x, o_y, o_d, o_Nb, o_kkt, o_verdict, o_xomega, o_xsteps, o_changed, o_fail;  // read back
    size_t o_AB, o_AN, o_cB, o_cN, o_b, o_lb, o_ub, o_kind, o_B, o_N;                     // inputs
    size_t o_r, o_rho, o_omega, o_steps, o_rkeep;                                         // device only
    size_t bytes;
};

BpostLayout bstart_layout(const ellp_batch_item *items, BstartPlan *plan, size_t R) {
    BpostLayout L{};
    SlabCursor cur;
    for (size_t k = 0; k < R; ++k) {
        BstartPlan &p = plan[k];
        const ellp_batch_item &it = items[p.item];
        cur.bytes = &p.bytes;
        p.bytes = sizeof(StartBatchArgs);
        p.o_x = cur.take(sizeof(double) * (size_t)it.n);
        p.o_y = cur.take(sizeof(double) * (size_t)it.m);
        p.o_d = cur.take(sizeof(double) * (size_t)it.n);
        p.o_Nb = cur.take((size_t)p.nNa);
        p.o_kkt = cur.take(sizeof(ellp_kkt));
        p.o_verdict = cur.take(sizeof(StartVerdict));
        p.o_xomega = cur.take(sizeof(double));
        p.o_xsteps = cur.take(sizeof(int32_t));
        p.o_changed = cur.take(sizeof(long long));
        p.o_fail = cur.take(sizeof(int));
    }
    L.out_bytes = cur.off;
    for (size_t k = 0; k < R; ++k) {
        BstartPlan &p = plan[k];
        const ellp_batch_item &it = items[p.item];
        cur.bytes = &p.bytes;
        p.o_AB = cur.take(sizeof(double) * (size_t)(p.ld * it.m));
        p.o_AN = cur.take(sizeof(double) * (size_t)(p.ld * p.nNa));
        p.o_cB = cur.take(sizeof(double) * (size_t)it.m);
        p.o_cN = cur.take(sizeof(double) * (size_t)p.nNa);
        p.o_b = cur.take(sizeof(double) * (size_t)it.m);
        p.o_lb = cur.take(sizeof(double) * (size_t)it.n);
        p.o_ub = cur.take(sizeof(double) * (size_t)it.n);
        p.o_kind = cur.take((size_t)it.n);
        p.o_B = cur.take(sizeof(int64_t) * (size_t)it.m);
        p.o_N = cur.take(sizeof(int64_t) * (size_t)p.nNa);
    }
    cur.bytes = nullptr;
    L.o_args = cur.take(sizeof(StartBatchArgs) * R);
    L.stage_bytes = cur.off;
    for (size_t k = 0; k < R; ++k) {
        BstartPlan &p = plan[k];
        cur.bytes = &p.bytes;
        p.o_r = cur.take(sizeof(double) * (size_t)items[p.item].m);
        p.o_rho = cur.take(sizeof(double) * (size_t)items[p.item].m);
        p.o_omega = cur.take(sizeof(double));
        p.o_steps = cur.take(sizeof(int32_t));
        p.o_rkeep = cur.take(sizeof(double) * 2 * BPOST_ROWS * (size_t)(p.nbn > 0 ? p.nbn : 1));
    }
    L.total = cur.off;
    return L;
}

// the calling thread's last ellp_batch_basis_start that passed the checks of the call (ellp_batch_basis_start_info)
thread_local uint64_t g_batch_start_info[4] = {0, 0, 0, 0};

// One chunk: staging, one upload, the two launches, one read-back, the per-item results
ellp_status bstart_run_chunk(ellp_batch_item *items, int mode, double eps, ellp_start_info *infos, BstartPlan *plan, size_t R,
                             BatchCleanup &cl, ellp_status *status_out, char *errbuf, size_t errlen) {
    const BpostLayout L = bstart_layout(items, plan, R);
    hipStream_t stream = cl.hs.stream;
    unsigned char *h = static_cast<unsigned char *>(cl.stage.p);
    unsigned char *dv = static_cast<unsigned char *>(cl.slab.p);
    StartBatchArgs *h_args = slab_at<StartBatchArgs>(h, L.o_args);
    size_t lds = 0;
    for (size_t k = 0; k < R; ++k) {
        const BstartPlan &p = plan[k];
        const ellp_batch_item &it = items[p.item];
        const int64_t m = it.m, n = it.n, nN = it.n_N, ld = p.ld;
        memset(h + p.o_x, 0, sizeof(double) * (size_t)n);  // the pass for d_N reads x before the labels are made
        memset(h + p.o_fail, 0, sizeof(int));
        batch_stage_basis(h, it, ld, p.o_AB, p.o_AN, p.o_cB, p.o_cN);
        memcpy(h + p.o_b, it.b, sizeof(double) * (size_t)m);
        memcpy(h + p.o_lb, it.lb, sizeof(double) * (size_t)n);
        memcpy(h + p.o_ub, it.ub, sizeof(double) * (size_t)n);
        memcpy(h + p.o_kind, it.bound_kind, (size_t)n);
        memcpy(h + p.o_B, it.B_index, sizeof(int64_t) * (size_t)m);
        if (nN > 0) {
            memcpy(h + p.o_N, it.N_index, sizeof(int64_t) * (size_t)nN);
            memcpy(h + p.o_Nb, it.N_bound, (size_t)nN);
        }
        StartBatchArgs a{};
        a.A_B = slab_at<const double>(dv, p.o_AB);
        a.A_N = slab_at<const double>(dv, p.o_AN);
        a.c_N = slab_at<const double>(dv, p.o_cN);
        a.x = slab_at<double>(dv, p.o_x);
        a.y = slab_at<double>(dv, p.o_y);
        a.d = slab_at<double>(dv, p.o_d);
        a.r = slab_at<double>(dv, p.o_r);
        a.rho = slab_at<double>(dv, p.o_rho);
        a.omega = slab_at<double>(dv, p.o_omega);
        a.xomega = slab_at<double>(dv, p.o_xomega);
        a.rkeep = slab_at<double>(dv, p.o_rkeep);
        a.Nb = dv + p.o_Nb;
        a.steps = slab_at<int32_t>(dv, p.o_steps);
        a.xsteps = slab_at<int32_t>(dv, p.o_xsteps);
        a.changed = slab_at<long long>(dv, p.o_changed);
        a.fail = slab_at<int>(dv, p.o_fail);
        a.verdict = slab_at<StartVerdict>(dv, p.o_verdict);
        a.ld = ld;
        a.by_d = mode == ELLP_START_LABELS_BY_D;
        a.eps = eps;
        bpost_report_args(a.rep, dv, p, it);  // rep.x = x, rep.Nb = Nb; c_tail stays NULL: n_c == n
        h_args[k] = a;
        if (p.lds > lds) lds = p.lds;
    }
    // the outputs' region goes up too: x as zeros, the given labels and the fail flags are read before they are written
    HIPCHK(hipMemcpyAsync(dv, h, L.stage_bytes, hipMemcpyHostToDevice, stream));
    const StartBatchArgs *d_args = slab_at<const StartBatchArgs>(dv, L.o_args);
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_start_batch), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // ELLP_POST_PROFILE=1 (tools/batch_start_time.py): one line per chunk, m = the chunk's items, lu_ms = k_start_batch,
    // rest_ms = the reports
    PostProf prof(stream);
    prof.name = "batch_basis_start_profile";
    prof.begin(PostProf::LU);
    hipLaunchKernelGGL(k_start_batch, dim3((unsigned)R), dim3(BPOST_NT), lds, stream, d_args);
    prof.end();
    prof.begin(PostProf::REST);
    hipLaunchKernelGGL(k_start_report_batch, dim3((unsigned)R), dim3(1024), 0, stream, d_args);
    prof.end();
    g_batch_start_info[0] += 2;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, dv, L.out_bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    prof.report((int64_t)R, 0, 0);
    for (size_t k = 0; k < R; ++k) {
        const BstartPlan &p = plan[k];
        ellp_batch_item &it = items[p.item];
        // a singular basis: every output of the item, N_bound too, stays as it was
        if (batch_item_singular(h, p.o_fail, it, &status_out[p.item])) continue;
        memcpy(it.x, h + p.o_x, sizeof(double) * (size_t)it.n);
        if (it.n_N > 0) memcpy(it.N_bound, h + p.o_Nb, (size_t)it.n_N);
        if (it.y) memcpy(it.y, h + p.o_y, sizeof(double) * (size_t)it.m);
        if (it.d) memcpy(it.d, h + p.o_d, sizeof(double) * (size_t)it.n);
        if (infos) {
            ellp_start_info *info = infos + p.item;
            ellp_kkt hk;
            StartVerdict hv;
            long long changed = 0;
            int32_t xsteps = 0;
            memcpy(&hk, h + p.o_kkt, sizeof(hk));
            memcpy(&hv, h + p.o_verdict, sizeof(hv));
            memcpy(&changed, h + p.o_changed, sizeof(changed));
            memcpy(&xsteps, h + p.o_xsteps, sizeof(xsteps));
            memset(info, 0, sizeof(*info));
            info->primal_infeasibility = hv.pinf;
            info->primal_infeasibility_sum = hv.psum;
            info->dual_infeasibility = hk.dual_infeasibility;
            memcpy(&info->x_backward_error, h + p.o_xomega, sizeof(double));
            info->worst_primal_var = hv.worst_primal;
            info->worst_dual_var = hk.worst_dual_var;
            info->labels_changed = (int64_t)changed;
            info->primal_feasible = hv.primal_feasible;
            info->dual_feasible = hv.dual_feasible;
            info->x_refinement_steps = xsteps;
            info->kkt = hk;
        }
        status_out[p.item] = ELLP_OPTIMAL;
    }
    return ELLP_OPTIMAL;
}

}  // namespace

extern "C" ellp_status ellp_batch_basis_start(int64_t count, ellp_batch_item *items, int mode, const ellp_opts *opts_in,
                                              ellp_start_info *infos, ellp_status *status_out, char *errbuf, size_t errlen) {
    if (errbuf && errlen) errbuf[0] = 0;
    if (count < 0 || !items || !status_out) {
        set_err(errbuf, errlen, "count < 0, or items / status_out NULL");
        return ELLP_ERR_ARG;
    }
    if (mode != ELLP_START_KEEP_LABELS && mode != ELLP_START_LABELS_BY_D) {
        set_err(errbuf, errlen, "basis_start: unknown mode %d", mode);
        return ELLP_ERR_ARG;
    }
    // ---- per item: the single call's checks, then who runs it (all before any HIP call)
    std::vector<BstartPlan> plan;
    std::vector<int64_t> single;
    for (int64_t i = 0; i < count; ++i) {
        ellp_batch_item &it = items[i];
        it.err[0] = 0;
        ellp_status s = ELLP_OPTIMAL;
        if (it.n_c != it.n) {
            set_err(it.err, sizeof(it.err), "basis_start: n_c = %lld, a start is made in the standard form (n_c = n = %lld)", (long long)it.n_c,
                    (long long)it.n);
            s = ELLP_ERR_ARG;
        } else {
            s = start_host_checks(it.m, it.n, it.A, it.c, it.b, it.bound_kind, it.lb, it.ub, it.B_index, it.n_B, it.N_index, it.N_bound, it.n_N,
                                  mode, it.x, it.err, sizeof(it.err));
        }
        status_out[i] = s;
        if (s != ELLP_OPTIMAL) continue;
        const size_t lds = bpost_lds_bytes(it.m, BSTART_EXTRA);
        if (lds == 0 || it.n_N > BPOST_MAX_NN) {
            single.push_back(i);
            continue;
        }
        BstartPlan p{};
        p.item = i;
        p.ld = round_up(it.m, 16);
        p.nNa = it.n_N > 0 ? it.n_N : 1;
        p.nbn = (it.n_N + 63) / 64;
        p.lds = lds;
        plan.push_back(p);
    }
    g_batch_start_info[0] = 0;
    g_batch_start_info[1] = plan.size();
    g_batch_start_info[2] = single.size();
    g_batch_start_info[3] = 0;
    if (plan.empty() && single.empty()) return ELLP_OPTIMAL;

    if (!plan.empty()) {
        const double eps = opts_in && opts_in->eps > 0.0 ? opts_in->eps : 1e-10;  // post_host_engine's
        const ellp_status rc = batch_drive(
            plan, single, BPOST_CHUNK_SLACK, opts_in, status_out, &g_batch_start_info[3],
            [&](BstartPlan *pl, size_t R) { return bstart_layout(items, pl, R); },
            [&](BstartPlan *pl, size_t R, BatchCleanup &cl) { return bstart_run_chunk(items, mode, eps, infos, pl, R, cl, status_out, errbuf, errlen); },
            errbuf, errlen);
        if (rc != ELLP_OPTIMAL) return rc;
    }
    // ---- the items the kernel does not take: the single call, inside this one
    for (int64_t i : single) {
        ellp_batch_item &it = items[i];
        status_out[i] = ellp_basis_start(it.m, it.n, it.A, it.c, it.b, it.bound_kind, it.lb, it.ub, it.B_index, it.n_B, it.N_index, it.N_bound,
                                         it.n_N, mode, opts_in, it.x, it.y, it.d, infos ? infos + i : nullptr, it.err, sizeof(it.err));
    }
    return ELLP_OPTIMAL;
}

extern "C" void ellp_batch_basis_start_info(uint64_t *out4) {
    if (!out4) return;
    for (int k = 0; k < 4; ++k) out4[k] = g_batch_start_info[k];
}

// ellp_brange.inc — ellp_batch_ranging: the sensitivity ranging of ellp_range.inc for many small LPs.  DESIGN.md §3.10b.
//
// Five launches per chunk, whatever the item count and whatever the items' shapes:
//   A  k_brange_front     one workgroup per item: k_post_batch's item (bpost_item: the LU in LDS, the refined y, d, r and the
//                         inputs of the report), then the factors by rows (M[r][k], what ellp_lu_rows_factor leaves), the
//                         transposition list as piv[] and the singleton columns into the item's share of the slab;
//   B  k_brange_solve     one workgroup per (item, block of 16 rows), through a table: range_solve_rows<16> on the item's
//                         factors (k_range_solve's body: the per-vector operations of k_lu_solve mode 1 in its order), the
//                         snap of the singleton columns on the rows in LDS, the rows into W;
//   C  k_brange_tab       one workgroup per (item, block of 128 nonbasic columns), through a table: range_tab_tile<0>
//                         (k_range_tab<0>'s body: one accumulator chain of v_mfma_f64_16x16x4_f64 per alpha_ij over k in
//                         ascending blocks of four from +0.0, k zero-filled to the same multiple of 16, rows and columns
//                         beyond the item zero-filled), the records of the epilogue per (column block, row);
//   D  k_brange_fold      one workgroup per item: the fold of the column blocks (range_cfold_row), the nonbasic and
//                         column-less costs (range_cnb_one), the right-hand sides (rng_rhs_cand over the rows of W: min, max
//                         and the first-position tie are exact, so the order is free) and inverse_residual
//                         (range_resid_tile over the item's 64 x 64 tiles: every entry one sum in ascending k, product and
//                         sum rounded separately; the NaN-winning maximum does not depend on the order);
//   E  k_post_report_batch  the KKT report, once per item with the single call's 1,024 threads.
// Every output is, bit for bit, what ellp_ranging returns for the item alone: y, d, r and the report are the batched
// postsolve's (ellp_bpost.inc), everything else runs the single call's own device functions on the single call's numbers.
// An item whose LU meets a zero on U's diagonal sets its flag in A; B to E leave it alone.
//
// The driver (budget, chunks, device, the pinned staging buffer, the slab) and the buffer pool are ellp_batch.inc's; the
// staging of an item is ellp_bpost.inc's.  The outputs an item asks for lie at the front of the slab and come back in one
// read-back; those it does not ask for (W above all) lie behind the inputs and stay on the device.  The fail flags end the
// outputs' region so that one upload from there on zeroes them.
//
// Included at the end of ellp_engine.hip, after ellp_range.inc and ellp_bpost.inc.

namespace {

constexpr int BRANGE_R = 16;       // rows of W per workgroup of launch B: 32 KB of LDS at 128 rows
constexpr int BRANGE_LAUNCHES = 5;

struct BrangeArgs {  // one item as launches A to D see it
    const double *A_B;
    double *M, *sval, *W, *res;
    int64_t *piv;
    int32_t *srow;
    int *fail;
    int64_t m, ld, ldw;
    RngTabArgs tab;
    RngCfoldArgs fold;
    RngCnbArgs cnb;
    RngRhsArgs rhs;
};

__global__ __launch_bounds__(BPOST_NT) void k_brange_front(const PostBatchArgs *pargs, const BrangeArgs *rargs) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ double s_bc[2];
    __shared__ int s_plen;
    const PostBatchArgs a = pargs[blockIdx.x];
    const int tid = threadIdx.x;
    const int m = (int)a.rep.m;
    const BpostSh sh = bpost_carve(smem, m, 0);
    if (!bpost_item(a, sh, &s_plen, s_bc, tid)) return;
    const BrangeArgs &k = rargs[blockIdx.x];
    double *M = k.M;
    for (int e = tid; e < m * m; e += BPOST_NT) {  // by rows: M[r][c] = LU[c * m + r]
        const int r = e / m, c = e - r * m;
        M[e] = sh.LU[c * m + r];
    }
    if (tid < m) {
        int64_t p = tid;  // piv[i]: the row exchanged with row i at step i (small_lu records at most one per step)
        const int plen = s_plen;
        for (int q = 0; q < plen; ++q)
            if (sh.pa[q] == tid) p = sh.pb[q];
        k.piv[tid] = p;
        k.srow[tid] = sh.srow[tid];
        k.sval[tid] = sh.sval[tid];
    }
}

__global__ __launch_bounds__(512) void k_brange_solve(const BrangeArgs *args, const int2 *table) {
    extern __shared__ __align__(16) unsigned char rng_smem[];
    const int2 e = table[blockIdx.x];
    const BrangeArgs &a = args[e.x];
    if (*a.fail) return;  // uniform over the workgroup
    const int64_t m = a.m, i0 = (int64_t)e.y * BRANGE_R;
    const int tid = threadIdx.x;
    double *x = reinterpret_cast<double *>(rng_smem);
    double *acc = x + m * BRANGE_R;
    if (!range_solve_rows<BRANGE_R>(a.M, a.piv, m, i0, x, acc, tid)) {  // launch A has met the same diagonal: not reached
        if (tid == 0) *a.fail = 1;
        return;
    }
    // k_range_snap on the workgroup's rows: column j = v e_k fixes W[j][k] = fl(1 / v) and a zero in every other row
    for (int64_t t = tid; t < m * BRANGE_R; t += 512) {
        const int64_t j = t / BRANGE_R, r = t - j * BRANGE_R;
        const int k = a.srow[j];
        if (k >= 0) x[(int64_t)k * BRANGE_R + r] = (i0 + r == j) ? 1.0 / a.sval[j] : 0.0;
    }
    __syncthreads();
    range_store_rows<BRANGE_R>(x, m, i0, a.W, a.ldw, tid);
}

__global__ __launch_bounds__(512) void k_brange_tab(const BrangeArgs *args, const int2 *table, int64_t count) {
    if ((int64_t)blockIdx.x >= count) return;  // a chunk without a nonbasic column: one idle workgroup
    const int2 e = table[blockIdx.x];
    const BrangeArgs &a = args[e.x];
    if (*a.fail) return;  // uniform over the workgroup
    range_tab_tile<0>(a.tab, e.y, 0);
}

__global__ __launch_bounds__(256) void k_brange_fold(const BrangeArgs *args) {
    __shared__ double s_v[2][128];
    __shared__ int s_p[2][128];
    const BrangeArgs &a = args[blockIdx.x];
    if (*a.fail) return;  // uniform over the workgroup
    const int tid = threadIdx.x;
    const int64_t m = a.m;
    for (int64_t i = tid; i < m; i += 256) range_cfold_row(a.fold, i);
    const int64_t rest = a.cnb.nN + (a.cnb.n_c - a.cnb.n);
    for (int64_t t = tid; t < rest; t += 256) range_cnb_one(a.cnb, t);
    // the right-hand sides: thread (col, part) takes the rows part, part + 2, .. of column col of W; part 1 hands over in LDS
    {
        const RngRhsArgs &r = a.rhs;
        const int col = tid & 127, part = tid >> 7;
        RngRec up{INFINITY, RNG_NOPOS}, dn{-INFINITY, RNG_NOPOS};
        if (col < m)
            for (int64_t i = part; i < m; i += 2) {
                const int64_t var = r.B_index[i];
                double qu, qd;
                rng_rhs_cand(r.W[i * r.ldw + col], r.x[var], r.lb[var], r.ub[var], r.kind[var], r.eps, qu, qd);
                up = rng_pick<1>(up, RngRec{qu, qu == INFINITY ? RNG_NOPOS : (int)i});
                dn = rng_pick<0>(dn, RngRec{qd, qd == -INFINITY ? RNG_NOPOS : (int)i});
            }
        if (part == 1) {
            s_v[0][col] = up.v;
            s_p[0][col] = up.p;
            s_v[1][col] = dn.v;
            s_p[1][col] = dn.p;
        }
        __syncthreads();
        if (part == 0 && col < m) {
            up = rng_pick<1>(up, RngRec{s_v[0][col], s_p[0][col]});
            dn = rng_pick<0>(dn, RngRec{s_v[1][col], s_p[1][col]});
            r.rhs[col] = dn.v;
            r.rhs[m + col] = up.v;
            r.rblk[col] = rng_blocking(dn, r.B_index);
            r.rblk[m + col] = rng_blocking(up, r.B_index);
        }
    }
    // inverse_residual over the item's tiles
    const int64_t t64 = (m + 63) / 64;
    double worst = 0.0;
    for (int64_t ti = 0; ti < t64; ++ti)
        for (int64_t tj = 0; tj < t64; ++tj) worst = nanmax(worst, range_resid_tile(a.A_B, a.W, m, a.ld, a.ldw, ti, tj));
    if (tid == 0) *a.res = worst;
}

// one item on the batched kernels: ellp_batch_postsolve's plan and the ranging's share of the slab
struct BrangePlan : BpostPlan {
    int64_t nblk, nsolve;                            // blocks of 128 nonbasic columns; blocks of BRANGE_R rows
    bool w_y, w_d, w_cost, w_cblk, w_rhs, w_rblk, w_W;  // read back
    size_t o_res, o_cost, o_cblk, o_rhs, o_rblk, o_W;   // read back where wanted, device only else
    size_t o_M, o_piv, o_srow, o_sval, o_pu, o_pd, o_ppu, o_ppd;  // device only
};
struct BrangeLayout {
    size_t out_bytes, up_from, o_pargs, o_rargs, o_tsolve, o_ttab, stage_bytes, total;
    size_t nsolve, ntab;
};

BrangeLayout brange_layout(const ellp_batch_item *items, BrangePlan *plan, size_t R) {
    BrangeLayout L{};
    SlabCursor cur;
    // an array that comes back where it is wanted (pass 0) and stays on the device where it is not (pass 1)
    auto split = [&](int pass, BrangePlan &q) {
        const BrangePlan &p = q;
        const ellp_batch_item &it = items[p.item];
        const size_t m = (size_t)it.m, nc = (size_t)it.n_c;
        if ((pass == 0) == p.w_y) q.o_y = cur.take(sizeof(double) * m);
        if ((pass == 0) == p.w_d) q.o_d = cur.take(sizeof(double) * nc);
        if ((pass == 0) == p.w_cost) q.o_cost = cur.take(sizeof(double) * 2 * nc);
        if ((pass == 0) == p.w_cblk) q.o_cblk = cur.take(sizeof(int64_t) * 2 * nc);
        if ((pass == 0) == p.w_rhs) q.o_rhs = cur.take(sizeof(double) * 2 * m);
        if ((pass == 0) == p.w_rblk) q.o_rblk = cur.take(sizeof(int64_t) * 2 * m);
        if ((pass == 0) == p.w_W) q.o_W = cur.take(sizeof(double) * m * (size_t)p.ld);
    };
    for (size_t k = 0; k < R; ++k) {
        BrangePlan &p = plan[k];
        cur.bytes = &p.bytes;
        p.bytes = sizeof(PostBatchArgs) + sizeof(BrangeArgs) + sizeof(int2) * (size_t)(p.nsolve + p.nblk);
        split(0, p);
        p.o_kkt = cur.take(sizeof(ellp_kkt));
        p.o_res = cur.take(sizeof(double));
    }
    L.up_from = cur.off;
    for (size_t k = 0; k < R; ++k) {
        cur.bytes = &plan[k].bytes;
        plan[k].o_fail = cur.take(sizeof(int));
    }
    L.out_bytes = cur.off;
    L.nsolve = L.ntab = 0;
    for (size_t k = 0; k < R; ++k) {
        BrangePlan &p = plan[k];
        const ellp_batch_item &it = items[p.item];
        cur.bytes = &p.bytes;
        p.o_AB = cur.take(sizeof(double) * (size_t)(p.ld * it.m));
        p.o_AN = cur.take(sizeof(double) * (size_t)(p.ld * p.nNa));
        p.o_cB = cur.take(sizeof(double) * (size_t)it.m);
        p.o_cN = cur.take(sizeof(double) * (size_t)p.nNa);
        p.o_ct = cur.take(sizeof(double) * (size_t)p.ntail);
        p.o_x = cur.take(sizeof(double) * (size_t)it.n_c);
        p.o_b = cur.take(sizeof(double) * (size_t)it.m);
        p.o_lb = cur.take(sizeof(double) * (size_t)it.n_c);
        p.o_ub = cur.take(sizeof(double) * (size_t)it.n_c);
        p.o_kind = cur.take((size_t)it.n_c);
        p.o_B = cur.take(sizeof(int64_t) * (size_t)it.m);
        p.o_N = cur.take(sizeof(int64_t) * (size_t)p.nNa);
        p.o_Nb = cur.take((size_t)p.nNa);
        L.nsolve += (size_t)p.nsolve;
        L.ntab += (size_t)p.nblk;
    }
    cur.bytes = nullptr;
    L.o_pargs = cur.take(sizeof(PostBatchArgs) * R);
    L.o_rargs = cur.take(sizeof(BrangeArgs) * R);
    L.o_tsolve = cur.take(sizeof(int2) * L.nsolve);
    L.o_ttab = cur.take(sizeof(int2) * L.ntab);
    L.stage_bytes = cur.off;
    for (size_t k = 0; k < R; ++k) {
        BrangePlan &p = plan[k];
        const size_t m = (size_t)items[p.item].m, rec = (size_t)p.nblk * m;
        cur.bytes = &p.bytes;
        split(1, p);
        p.o_r = cur.take(sizeof(double) * m);
        p.o_rho = cur.take(sizeof(double) * m);
        p.o_omega = cur.take(sizeof(double));
        p.o_steps = cur.take(sizeof(int32_t));
        p.o_M = cur.take(sizeof(double) * m * m);
        p.o_piv = cur.take(sizeof(int64_t) * m);
        p.o_srow = cur.take(sizeof(int32_t) * m);
        p.o_sval = cur.take(sizeof(double) * m);
        p.o_pu = cur.take(sizeof(double) * rec);
        p.o_pd = cur.take(sizeof(double) * rec);
        p.o_ppu = cur.take(sizeof(int32_t) * rec);
        p.o_ppd = cur.take(sizeof(int32_t) * rec);
    }
    L.total = cur.off;
    return L;
}

// the calling thread's last ellp_batch_ranging that passed the checks of the call (ellp_batch_ranging_info)
thread_local uint64_t g_batch_range_info[4] = {0, 0, 0, 0};

// ELLP_RANGE_PROFILE=1 (tools/batch_ranging_time.py): the five launches of a chunk bracketed with HIP events, one line on
// stderr per chunk
struct BrangeProf {
    enum { NCAT = BRANGE_LAUNCHES };
    bool on;
    hipStream_t stream;
    hipEvent_t ev[NCAT + 1];
    int have;
    BrangeProf(hipStream_t s) : on(getenv("ELLP_RANGE_PROFILE") && getenv("ELLP_RANGE_PROFILE")[0] == '1'), stream(s), have(0) {}
    void mark() {  // before the first launch and after every one
        if (!on || have > NCAT) return;
        if (hipEventCreate(&ev[have]) != hipSuccess) {
            on = false;
            return;
        }
        (void)hipEventRecord(ev[have++], stream);
    }
    void report(size_t items) {  // after the stream has drained
        if (!on || have != NCAT + 1) return;
        float ms[NCAT];
        for (int c = 0; c < NCAT; ++c) {
            ms[c] = 0.f;
            (void)hipEventElapsedTime(&ms[c], ev[c], ev[c + 1]);
        }
        fprintf(stderr, "batch_ranging_profile items=%lld front_ms=%.4f solve_ms=%.4f tableau_ms=%.4f fold_ms=%.4f report_ms=%.4f\n",
                (long long)items, ms[0], ms[1], ms[2], ms[3], ms[4]);
    }
    ~BrangeProf() {
        for (int c = 0; c < have; ++c) (void)hipEventDestroy(ev[c]);
    }
};

// One chunk: staging, one upload, the five launches, one read-back, the per-item results
ellp_status brange_run_chunk(ellp_batch_item *items, const ellp_batch_range_out *outs, double eps, BrangePlan *plan, size_t R,
                             BatchCleanup &cl, ellp_status *status_out, char *errbuf, size_t errlen) {
    const BrangeLayout L = brange_layout(items, plan, R);
    hipStream_t stream = cl.hs.stream;
    unsigned char *h = static_cast<unsigned char *>(cl.stage.p);
    unsigned char *dv = static_cast<unsigned char *>(cl.slab.p);
    PostBatchArgs *h_pargs = slab_at<PostBatchArgs>(h, L.o_pargs);
    BrangeArgs *h_rargs = slab_at<BrangeArgs>(h, L.o_rargs);
    int2 *h_tsolve = slab_at<int2>(h, L.o_tsolve), *h_ttab = slab_at<int2>(h, L.o_ttab);
    size_t lds = 0, lds_solve = 0, ns = 0, nt = 0;
    for (size_t k = 0; k < R; ++k) {
        const BrangePlan &p = plan[k];
        const ellp_batch_item &it = items[p.item];
        const PostBatchArgs pa = bpost_stage_item(h, dv, p, it);
        h_pargs[k] = pa;
        const int64_t m = it.m, n_c = it.n_c;
        BrangeArgs a{};
        a.A_B = pa.A_B;
        a.M = slab_at<double>(dv, p.o_M);
        a.sval = slab_at<double>(dv, p.o_sval);
        a.W = slab_at<double>(dv, p.o_W);
        a.res = slab_at<double>(dv, p.o_res);
        a.piv = slab_at<int64_t>(dv, p.o_piv);
        a.srow = slab_at<int32_t>(dv, p.o_srow);
        a.fail = pa.fail;
        a.m = m; a.ld = p.ld; a.ldw = p.ld;
        double *cost = slab_at<double>(dv, p.o_cost);
        int64_t *cblk = slab_at<int64_t>(dv, p.o_cblk);
        RngTabArgs &t = a.tab;
        t.W = a.W; t.rowmap = nullptr; t.A_N = pa.A_N; t.d = pa.d; t.N_index = pa.rep.N_index; t.Nb = pa.rep.Nb; t.kind = pa.rep.kind;
        t.pu = slab_at<double>(dv, p.o_pu); t.pd = slab_at<double>(dv, p.o_pd);
        t.ppu = slab_at<int32_t>(dv, p.o_ppu); t.ppd = slab_at<int32_t>(dv, p.o_ppd);
        t.out = nullptr; t.m = m; t.ld = p.ld; t.ldw = p.ld; t.nrows = m; t.nN = it.n_N; t.eps = eps;
        RngCfoldArgs &f = a.fold;
        f.pu = t.pu; f.pd = t.pd; f.ppu = t.ppu; f.ppd = t.ppd; f.B_index = pa.rep.B_index; f.N_index = pa.rep.N_index;
        f.cost = cost; f.cblk = cblk; f.m = m; f.n_c = n_c; f.nblk = p.nblk;
        RngCnbArgs &c = a.cnb;
        c.d = pa.d; c.N_index = pa.rep.N_index; c.Nb = pa.rep.Nb; c.kind = pa.rep.kind; c.cost = cost; c.cblk = cblk;
        c.nN = it.n_N; c.n = it.n; c.n_c = n_c;
        RngRhsArgs &r = a.rhs;
        r.W = a.W; r.x = pa.rep.x; r.lb = pa.rep.lb; r.ub = pa.rep.ub; r.kind = pa.rep.kind; r.B_index = pa.rep.B_index;
        r.rhs = slab_at<double>(dv, p.o_rhs); r.rblk = slab_at<int64_t>(dv, p.o_rblk);
        r.m = m; r.ldw = p.ld; r.eps = eps;
        h_rargs[k] = a;
        for (int64_t q = 0; q < p.nsolve; ++q) h_tsolve[ns++] = make_int2((int)k, (int)q);
        for (int64_t q = 0; q < p.nblk; ++q) h_ttab[nt++] = make_int2((int)k, (int)q);
        if (p.lds > lds) lds = p.lds;
        const size_t ls = (size_t)16 * (size_t)m * BRANGE_R;
        if (ls > lds_solve) lds_solve = ls;
    }
    // from the fail flags on: the flags are zeroed, the outputs in front of them are written before they are read
    HIPCHK(hipMemcpyAsync(dv + L.up_from, h + L.up_from, L.stage_bytes - L.up_from, hipMemcpyHostToDevice, stream));
    const PostBatchArgs *d_pargs = slab_at<const PostBatchArgs>(dv, L.o_pargs);
    const BrangeArgs *d_rargs = slab_at<const BrangeArgs>(dv, L.o_rargs);
    const int2 *d_tsolve = slab_at<const int2>(dv, L.o_tsolve), *d_ttab = slab_at<const int2>(dv, L.o_ttab);
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_brange_front), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    BrangeProf prof(stream);
    prof.mark();
    hipLaunchKernelGGL(k_brange_front, dim3((unsigned)R), dim3(BPOST_NT), lds, stream, d_pargs, d_rargs);
    prof.mark();
    hipLaunchKernelGGL(k_brange_solve, dim3((unsigned)L.nsolve), dim3(512), lds_solve, stream, d_rargs, d_tsolve);
    prof.mark();
    // always launched, with one idle workgroup where no item of the chunk has a nonbasic column: the count is a constant
    hipLaunchKernelGGL(k_brange_tab, dim3((unsigned)(L.ntab > 0 ? L.ntab : 1)), dim3(512), 0, stream, d_rargs, d_ttab, (int64_t)L.ntab);
    prof.mark();
    hipLaunchKernelGGL(k_brange_fold, dim3((unsigned)R), dim3(256), 0, stream, d_rargs);
    prof.mark();
    hipLaunchKernelGGL(k_post_report_batch, dim3((unsigned)R), dim3(1024), 0, stream, d_pargs);
    prof.mark();
    g_batch_range_info[0] += BRANGE_LAUNCHES;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, dv, L.out_bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    prof.report(R);
    for (size_t k = 0; k < R; ++k) {
        const BrangePlan &p = plan[k];
        const ellp_batch_item &it = items[p.item];
        const ellp_batch_range_out &bo = outs[p.item];
        const ellp_ranging_out &o = bo.out;
        if (batch_item_singular(h, p.o_fail, items[p.item], &status_out[p.item])) continue;
        const size_t cb = sizeof(double) * (size_t)it.n_c, rb = sizeof(double) * (size_t)it.m;
        if (o.cost_down) memcpy(o.cost_down, h + p.o_cost, cb);
        if (o.cost_up) memcpy(o.cost_up, h + p.o_cost + cb, cb);
        if (o.cost_blocking_down) memcpy(o.cost_blocking_down, h + p.o_cblk, cb);
        if (o.cost_blocking_up) memcpy(o.cost_blocking_up, h + p.o_cblk + cb, cb);
        if (o.rhs_down) memcpy(o.rhs_down, h + p.o_rhs, rb);
        if (o.rhs_up) memcpy(o.rhs_up, h + p.o_rhs + rb, rb);
        if (o.rhs_blocking_down) memcpy(o.rhs_blocking_down, h + p.o_rblk, rb);
        if (o.rhs_blocking_up) memcpy(o.rhs_blocking_up, h + p.o_rblk + rb, rb);
        if (o.d) memcpy(o.d, h + p.o_d, cb);
        if (o.y) memcpy(o.y, h + p.o_y, rb);
        if (o.info) {
            ellp_ranging_info info{};
            memcpy(&info.inverse_residual, h + p.o_res, sizeof(double));
            memcpy(&info.kkt, h + p.o_kkt, sizeof(ellp_kkt));
            *o.info = info;
        }
        if (bo.W)
            for (int64_t i = 0; i < it.m; ++i) memcpy(bo.W + i * it.m, h + p.o_W + sizeof(double) * (size_t)(i * p.ld), rb);
        status_out[p.item] = ELLP_OPTIMAL;
    }
    return ELLP_OPTIMAL;
}

// an item the batched kernels do not take: ellp_ranging's steps, and W from its workspace where that is wanted
ellp_status brange_single(const ellp_batch_item &it, const ellp_opts *opts_in, const ellp_batch_range_out &bo, char *errbuf, size_t errlen) {
    if (errbuf && errlen) errbuf[0] = 0;
    PostOwn own(nullptr, ellp_engine_destroy);
    const ellp_status s = post_host_engine("ranging", it.m, it.n, it.n_c, it.A, it.c, it.b, it.bound_kind, it.lb, it.ub, it.x, it.B_index, it.n_B,
                                           it.N_index, it.N_bound, it.n_N, opts_in, own, errbuf, errlen);
    if (s != ELLP_OPTIMAL) return s;
    ellp_engine *e = own.get();
    ellp_ranging_info scratch{};
    ellp_ranging_out o = bo.out;
    if (!range_wants(&o)) o.info = &scratch;  // W alone
    const ellp_status rs = range_compute(e, &o, errbuf, errlen);
    if (rs != ELLP_OPTIMAL) return rs;
    if (bo.W)
        HIPCHK(hipMemcpy2D(bo.W, sizeof(double) * (size_t)it.m, e->rng_W, sizeof(double) * (size_t)e->ld, sizeof(double) * (size_t)it.m,
                           (size_t)it.m, hipMemcpyDeviceToHost));
    return ELLP_OPTIMAL;
}

}  // namespace

extern "C" ellp_status ellp_batch_ranging(int64_t count, ellp_batch_item *items, const ellp_opts *opts_in,
                                          const ellp_batch_range_out *outs, ellp_status *status_out, char *errbuf, size_t errlen) {
    if (errbuf && errlen) errbuf[0] = 0;
    if (count < 0 || !items || !outs || !status_out) {
        set_err(errbuf, errlen, "count < 0, or items / outs / status_out NULL");
        return ELLP_ERR_ARG;
    }
    // ---- per item: the single call's checks, then who runs it (all before any HIP call)
    std::vector<BrangePlan> plan;
    std::vector<int64_t> single;
    for (int64_t i = 0; i < count; ++i) {
        ellp_batch_item &it = items[i];
        const ellp_batch_range_out &bo = outs[i];
        it.err[0] = 0;
        if (!range_wants(&bo.out) && !bo.W) {
            set_err(it.err, sizeof(it.err), "ranging: nothing is wanted (out is NULL or holds no array)");
            status_out[i] = ELLP_ERR_ARG;
            continue;
        }
        const ellp_status s = post_host_checks("ranging", it.m, it.n, it.n_c, it.A, it.c, it.b, it.bound_kind, it.lb, it.ub, it.x, it.B_index,
                                               it.n_B, it.N_index, it.N_bound, it.n_N, it.err, sizeof(it.err));
        status_out[i] = s;
        if (s != ELLP_OPTIMAL) continue;
        const size_t lds = bpost_lds_bytes(it.m);
        if (lds == 0 || it.n_N > BPOST_MAX_NN) {
            single.push_back(i);
            continue;
        }
        BrangePlan p{};
        p.item = i;
        p.ld = round_up(it.m, 16);
        p.nNa = it.n_N > 0 ? it.n_N : 1;
        p.ntail = it.n_c - it.n;
        p.lds = lds;
        p.nblk = range_blocks(it.n_N);
        p.nsolve = (it.m + BRANGE_R - 1) / BRANGE_R;
        const ellp_ranging_out &o = bo.out;
        p.w_y = o.y != nullptr;
        p.w_d = o.d != nullptr;
        p.w_cost = o.cost_down || o.cost_up;
        p.w_cblk = o.cost_blocking_down || o.cost_blocking_up;
        p.w_rhs = o.rhs_down || o.rhs_up;
        p.w_rblk = o.rhs_blocking_down || o.rhs_blocking_up;
        p.w_W = bo.W != nullptr;
        plan.push_back(p);
    }
    g_batch_range_info[0] = 0;
    g_batch_range_info[1] = plan.size();
    g_batch_range_info[2] = single.size();
    g_batch_range_info[3] = 0;
    if (plan.empty() && single.empty()) return ELLP_OPTIMAL;

    if (!plan.empty()) {
        const double eps = opts_in && opts_in->eps > 0.0 ? opts_in->eps : 1e-10;  // post_host_engine's
        const ellp_status rc = batch_drive(
            plan, single, BPOST_CHUNK_SLACK, opts_in, status_out, &g_batch_range_info[3],
            [&](BrangePlan *pl, size_t R) { return brange_layout(items, pl, R); },
            [&](BrangePlan *pl, size_t R, BatchCleanup &cl) { return brange_run_chunk(items, outs, eps, pl, R, cl, status_out, errbuf, errlen); },
            errbuf, errlen);
        if (rc != ELLP_OPTIMAL) return rc;
    }
    // ---- the items the kernels do not take: the single call's steps, inside this one
    for (int64_t i : single) status_out[i] = brange_single(items[i], opts_in, outs[i], items[i].err, sizeof(items[i].err));
    return ELLP_OPTIMAL;
}

extern "C" void ellp_batch_ranging_info(uint64_t *out4) {
    if (!out4) return;
    for (int k = 0; k < 4; ++k) out4[k] = g_batch_range_info[k];
}

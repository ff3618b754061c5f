// ellp_batch.inc — ellp_batch_solve_with_initial: many small LPs (m <= 128), one workgroup of k_small_batch per LP.
//
// Every item goes through the steps a single call (solve_once on the small path) takes, with the same code where there is
// code to share: check_problem, initial_state and dual_start_feasible of ellp_engine_create, small_threads for the workgroup
// size, the loop of k_small (small_loop) for the iterations, k_primal_obj's sum for the objective.  What is batched is the
// traffic around it: one pinned staging buffer and one device slab hold every item; the host gathers A_B / A_N / c_B / c_N
// (copies, so exact) into the staging buffer, which goes up in one copy; one launch per workgroup size (64 / 128 / 256) runs
// every item of that size; the states and outputs come back in one copy.  An item that the cap of a launch (16,384 loop
// bodies, ELLP_BATCH_LAUNCH_ITERS lowers it) left running is launched again from its device state, as run_small does.
//
// Layout of the slab: [DevState x runnable items][outputs of each item: x, B_index, N_index, Nb (y, d)] | [inputs and
// scratch of each item: A_B, A_N, c_B, c_N, lb, ub, kind, rbuf, kbuf (flist)][SmallArgs of all items][SmallArgs of the
// items of the current launch round].  Everything left of '|' is the one read-back.
//
// Included at the end of ellp_engine.hip (outside its anonymous namespace and extern "C" block).

namespace {

// pinned host buffers and device slabs outlive a call (pinning or allocating 100 MB costs milliseconds)
struct BatchBuf {
    int device = -1;
    bool pinned = false;
    void *p = nullptr;
    size_t cap = 0;
};
struct BatchPool {
    std::mutex mu;
    std::vector<BatchBuf> free_bufs;
};
BatchPool &batch_pool() {
    static BatchPool *p = new BatchPool;  // never destroyed: the HIP runtime may be gone before static destructors run
    return *p;
}
void batch_buf_free(const BatchBuf &b) {
    if (!b.p) return;
    if (b.pinned) (void)hipHostFree(b.p);
    else (void)hipFree(b.p);
}
hipError_t batch_buf_acquire(int device, bool pinned, size_t bytes, BatchBuf *out) {
    {
        BatchPool &bp = batch_pool();
        std::lock_guard<std::mutex> g(bp.mu);
        for (size_t k = 0; k < bp.free_bufs.size(); ++k) {
            const BatchBuf &b = bp.free_bufs[k];
            if (b.device == device && b.pinned == pinned && b.cap >= bytes) {
                *out = b;
                bp.free_bufs.erase(bp.free_bufs.begin() + (long)k);
                return hipSuccess;
            }
        }
    }
    BatchBuf b;
    b.device = device;
    b.pinned = pinned;
    b.cap = bytes;
    const hipError_t rc = pinned ? hipHostMalloc(&b.p, bytes, hipHostMallocDefault) : hipMalloc(&b.p, bytes);
    if (rc != hipSuccess) return rc;
    *out = b;
    return hipSuccess;
}
void batch_buf_release(const BatchBuf &b) {
    if (!b.p) return;
    BatchPool &bp = batch_pool();
    std::lock_guard<std::mutex> g(bp.mu);
    if (bp.free_bufs.size() < 4) {
        bp.free_bufs.push_back(b);
        return;
    }
    batch_buf_free(b);
}

const void *small_batch_kernel(int kind, int nt) {
    if (kind == ELLP_ENGINE_PRIMAL) {
        if (nt == 64) return reinterpret_cast<const void *>(&k_small_batch<0, 64>);
        if (nt == 128) return reinterpret_cast<const void *>(&k_small_batch<0, 128>);
        return reinterpret_cast<const void *>(&k_small_batch<0, 256>);
    }
    if (nt == 64) return reinterpret_cast<const void *>(&k_small_batch<1, 64>);
    if (nt == 128) return reinterpret_cast<const void *>(&k_small_batch<1, 128>);
    return reinterpret_cast<const void *>(&k_small_batch<1, 256>);
}

// byte offsets of one runnable item's arrays in the slab
struct BatchPlan {
    int64_t item;  // index into the caller's items
    int64_t ld, nNa;
    size_t lds;
    int nt;
    size_t o_x, o_B, o_N, o_Nb, o_y, o_d;                                     // outputs
    size_t o_AB, o_AN, o_cB, o_cN, o_lb, o_ub, o_kind, o_rbuf, o_kbuf, o_fl;  // inputs and scratch
    uint64_t done = 0;                                                       // loop bodies run so far
};

struct BatchCleanup {
    HostSet hs;
    BatchBuf stage, slab;
    ~BatchCleanup() {
        if (hs.stream) (void)hipStreamSynchronize(hs.stream);
        batch_buf_release(stage);
        batch_buf_release(slab);
        host_set_release(hs);
    }
};

}  // namespace

extern "C" ellp_status ellp_batch_solve_with_initial(int kind, int64_t count, ellp_batch_item *items, const ellp_opts *opts_in,
                                                     ellp_status *status_out, ellp_stats *stats_out, char *errbuf,
                                                     size_t errlen) {
    if (errbuf && errlen) errbuf[0] = 0;
    if (count < 0 || (count > 0 && (!items || !status_out))) {
        set_err(errbuf, errlen, "count < 0, or items / status_out NULL");
        return ELLP_ERR_ARG;
    }
    if (kind != ELLP_ENGINE_PRIMAL && kind != ELLP_ENGINE_DUAL) {
        set_err(errbuf, errlen, "unknown engine kind %d", kind);
        return ELLP_ERR_ARG;
    }
    ellp_opts opts;
    ellp_default_opts(&opts);
    if (opts_in) opts = *opts_in;
    const bool bflip = kind == ELLP_ENGINE_DUAL && (opts.flags & ELLP_FLAG_DUAL_BOUND_FLIPPING);
    const bool maxviol = kind == ELLP_ENGINE_DUAL && (opts.flags & ELLP_FLAG_DUAL_MAX_VIOLATION);
    if (opts.pipeline != 0 && opts.pipeline != 3) {
        set_err(errbuf, errlen, "batch: pipeline %d; the batch runs the LU-per-iteration kernel (pipeline 0 or 3)", opts.pipeline);
        return ELLP_ERR_ARG;
    }
    if (opts.partial_segments > 1 || (opts.flags & ELLP_FLAG_PRIMAL_STEEPEST_EDGE) || opts.trace_len > 0 || opts.profile) {
        set_err(errbuf, errlen, "batch: partial pricing, steepest edge, traces and profiling are not available in a batch");
        return ELLP_ERR_ARG;
    }
    if (opts.pipeline == 0 && !bflip && (opts.refactor_period > 0 || opts.btran_mode != 0)) {
        set_err(errbuf, errlen, "batch: refactor_period / btran_mode select the explicit-inverse engine, which a batch does not run");
        return ELLP_ERR_ARG;
    }
    const double eps = opts.eps > 0.0 ? opts.eps : 1e-10;
    const uint64_t max_iter = opts.max_iter;

    // ---- per item: the single call's checks, then what the batch cannot take (all before any HIP call)
    std::vector<BatchPlan> plan;
    for (int64_t i = 0; i < count; ++i) {
        ellp_batch_item &it = items[i];
        it.err[0] = 0;
        if (stats_out) memset(&stats_out[i], 0, sizeof(ellp_stats));
        ellp_status s = check_problem(kind, it.m, it.n, it.n_c, it.A, it.c, it.b, it.bound_kind, it.lb, it.ub, it.x, it.B_index,
                                      it.n_B, it.N_index, it.N_bound, it.n_N, it.y, it.d, it.err, sizeof(it.err));
        if (s == ELLP_OPTIMAL && small_lds_bytes(it.m, it.n_N) == 0) {
            set_err(it.err, sizeof(it.err), "batch: the LU-per-iteration kernel of a batch takes up to %d rows within 150 KB of LDS "
                                            "(this LP: m = %lld, |N| = %lld)", SMALL_MAX_M, (long long)it.m, (long long)it.n_N);
            s = ELLP_ERR_ARG;
        }
        if (s == ELLP_OPTIMAL && kind == ELLP_ENGINE_DUAL && !dual_start_feasible(it.n_N, it.N_index, it.N_bound, it.d, eps, it.err, sizeof(it.err)))
            s = ELLP_ERR_PANIC;
        status_out[i] = s;
        if (s != ELLP_OPTIMAL) continue;
        BatchPlan p;
        p.item = i;
        p.ld = round_up(it.m, 16);
        p.nNa = it.n_N > 0 ? it.n_N : 1;
        p.lds = small_lds_bytes(it.m, it.n_N);
        p.nt = small_threads(it.m, it.n_N);
        plan.push_back(p);
    }
    if (plan.empty()) return ELLP_OPTIMAL;

    // ---- layout
    const size_t R = plan.size();
    size_t off = sizeof(DevState) * R;
    auto take = [&](size_t bytes) {
        const size_t o = off;
        off += (bytes + 15) / 16 * 16;
        return o;
    };
    for (BatchPlan &p : plan) {
        const ellp_batch_item &it = items[p.item];
        p.o_x = take(sizeof(double) * (size_t)it.n_c);
        p.o_B = take(sizeof(int64_t) * (size_t)it.m);
        p.o_N = take(sizeof(int64_t) * (size_t)p.nNa);
        p.o_Nb = take((size_t)p.nNa);
        p.o_y = kind == ELLP_ENGINE_DUAL ? take(sizeof(double) * (size_t)p.ld) : 0;
        p.o_d = kind == ELLP_ENGINE_DUAL ? take(sizeof(double) * (size_t)it.n_c) : 0;
    }
    const size_t out_bytes = off;
    for (BatchPlan &p : plan) {
        const ellp_batch_item &it = items[p.item];
        p.o_AB = take(sizeof(double) * (size_t)(p.ld * it.m));
        p.o_AN = take(sizeof(double) * (size_t)(p.ld * p.nNa));
        p.o_cB = take(sizeof(double) * (size_t)it.m);
        p.o_cN = take(sizeof(double) * (size_t)p.nNa);
        p.o_lb = take(sizeof(double) * (size_t)it.n_c);
        p.o_ub = take(sizeof(double) * (size_t)it.n_c);
        p.o_kind = take((size_t)it.n_c);
        p.o_rbuf = take(sizeof(double) * (size_t)p.nNa);
        p.o_kbuf = take(sizeof(double) * (size_t)p.nNa);
        p.o_fl = bflip ? take(sizeof(long long) * (size_t)(p.nNa + 1)) : 0;
    }
    const size_t o_args_all = take(sizeof(SmallArgs) * R);
    const size_t o_args_run = take(sizeof(SmallArgs) * R);
    const size_t total = off;

    // ---- device
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_err(errbuf, errlen, "no HIP device available (this library has no CPU path)");
        return ELLP_ERR_DEVICE;
    }
    int dev = opts.device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
    HIPCHK(hipSetDevice(dev));
    BatchCleanup cl;
    HIPCHK(host_set_acquire(dev, &cl.hs));
    HIPCHK(batch_buf_acquire(dev, true, total, &cl.stage));
    HIPCHK(batch_buf_acquire(dev, false, total, &cl.slab));
    hipStream_t stream = cl.hs.stream;
    unsigned char *h = static_cast<unsigned char *>(cl.stage.p);
    unsigned char *dv = static_cast<unsigned char *>(cl.slab.p);

    // ---- staging: the engine's starting arrays, gathered as ellp_engine_create gathers them on the device
    DevState *h_states = reinterpret_cast<DevState *>(h);
    SmallArgs *h_all = reinterpret_cast<SmallArgs *>(h + o_args_all);
    for (size_t k = 0; k < R; ++k) {
        const BatchPlan &p = plan[k];
        const ellp_batch_item &it = items[p.item];
        const int64_t m = it.m, nN = it.n_N, ld = p.ld;
        h_states[k] = initial_state(kind, m, it.n_c, nN, it.c, it.b, it.bound_kind, it.lb, it.ub, it.x, it.y, it.d);
        memcpy(h + p.o_x, it.x, sizeof(double) * (size_t)it.n_c);
        memcpy(h + p.o_B, it.B_index, sizeof(int64_t) * (size_t)m);
        if (nN > 0) {
            memcpy(h + p.o_N, it.N_index, sizeof(int64_t) * (size_t)nN);
            memcpy(h + p.o_Nb, it.N_bound, (size_t)nN);
        }
        if (kind == ELLP_ENGINE_DUAL) {
            memcpy(h + p.o_y, it.y, sizeof(double) * (size_t)m);
            memcpy(h + p.o_d, it.d, sizeof(double) * (size_t)it.n_c);
        }
        if (kind == ELLP_ENGINE_DUAL) memset(h + p.o_y + sizeof(double) * (size_t)m, 0, sizeof(double) * (size_t)(ld - m));
        double *AB = reinterpret_cast<double *>(h + p.o_AB), *AN = reinterpret_cast<double *>(h + p.o_AN);
        double *cB = reinterpret_cast<double *>(h + p.o_cB), *cN = reinterpret_cast<double *>(h + p.o_cN);
        for (int64_t j = 0; j < m; ++j) {
            memcpy(AB + j * ld, it.A + it.B_index[j] * m, sizeof(double) * (size_t)m);
            memset(AB + j * ld + m, 0, sizeof(double) * (size_t)(ld - m));
            cB[j] = it.c[it.B_index[j]];
        }
        if (nN == 0) memset(AN, 0, sizeof(double) * (size_t)ld);
        for (int64_t j = 0; j < nN; ++j) {
            memcpy(AN + j * ld, it.A + it.N_index[j] * m, sizeof(double) * (size_t)m);
            memset(AN + j * ld + m, 0, sizeof(double) * (size_t)(ld - m));
            cN[j] = it.c[it.N_index[j]];
        }
        memcpy(h + p.o_lb, it.lb, sizeof(double) * (size_t)it.n_c);
        memcpy(h + p.o_ub, it.ub, sizeof(double) * (size_t)it.n_c);
        memcpy(h + p.o_kind, it.bound_kind, (size_t)it.n_c);
        SmallArgs a{};
        a.A_B = reinterpret_cast<double *>(dv + p.o_AB);
        a.A_N = reinterpret_cast<double *>(dv + p.o_AN);
        a.c_B = reinterpret_cast<double *>(dv + p.o_cB);
        a.c_N = reinterpret_cast<double *>(dv + p.o_cN);
        a.x = reinterpret_cast<double *>(dv + p.o_x);
        a.y = kind == ELLP_ENGINE_DUAL ? reinterpret_cast<double *>(dv + p.o_y) : nullptr;
        a.dd = kind == ELLP_ENGINE_DUAL ? reinterpret_cast<double *>(dv + p.o_d) : nullptr;
        a.lb = reinterpret_cast<const double *>(dv + p.o_lb);
        a.ub = reinterpret_cast<const double *>(dv + p.o_ub);
        a.kind = reinterpret_cast<const uint8_t *>(dv + p.o_kind);
        a.B_index = reinterpret_cast<int64_t *>(dv + p.o_B);
        a.N_index = reinterpret_cast<int64_t *>(dv + p.o_N);
        a.Nb = reinterpret_cast<uint8_t *>(dv + p.o_Nb);
        a.rbuf = reinterpret_cast<double *>(dv + p.o_rbuf);
        a.kbuf = reinterpret_cast<double *>(dv + p.o_kbuf);
        a.st = reinterpret_cast<DevState *>(dv) + k;
        a.m = m;
        a.ld = ld;
        a.nN = nN;
        a.max_iters = 0;
        a.nch = (int)((nN + 63) / 64);
        a.eps = eps;
        a.trace = Trace{nullptr, nullptr, 0};
        a.stamps = nullptr;
        a.maxviol = maxviol ? 1 : 0;
        a.bflip = bflip ? 1 : 0;
        a.flist = bflip ? reinterpret_cast<long long *>(dv + p.o_fl) : nullptr;
        h_all[k] = a;
    }
    const size_t up_bytes = o_args_run;  // the round's argument list is written per round
    HIPCHK(hipMemcpyAsync(dv, h, up_bytes, hipMemcpyHostToDevice, stream));

    // ---- launch rounds: every item still running, at most `cap` loop bodies each, grouped by workgroup size
    uint64_t cap = 16384;
    if (const char *v = getenv("ELLP_BATCH_LAUNCH_ITERS"); v && v[0] && atoll(v) > 0 && (uint64_t)atoll(v) < cap) cap = (uint64_t)atoll(v);
    SmallArgs *h_run = reinterpret_cast<SmallArgs *>(h + o_args_run);
    SmallArgs *d_run = reinterpret_cast<SmallArgs *>(dv + o_args_run);
    std::vector<size_t> live;  // plan positions that a launch may still advance
    for (size_t k = 0; k < R; ++k)
        if (items[plan[k].item].n_N > 0 && max_iter > 0) live.push_back(k);
    static const int nts[3] = {64, 128, 256};
    while (!live.empty()) {
        size_t nrun = 0;
        bool more = false;  // some item got less than what its budget still allows
        struct Group { size_t first, cnt, lds; };
        Group grp[3];
        for (int g = 0; g < 3; ++g) {
            grp[g] = Group{nrun, 0, 0};
            for (size_t k : live) {
                const BatchPlan &p = plan[k];
                if (p.nt != nts[g]) continue;
                const uint64_t remaining = max_iter - p.done;
                SmallArgs a = h_all[k];
                a.max_iters = remaining < cap ? remaining : cap;
                more = more || a.max_iters < remaining;
                h_run[nrun++] = a;
                grp[g].cnt += 1;
                if (p.lds > grp[g].lds) grp[g].lds = p.lds;
            }
        }
        HIPCHK(hipMemcpyAsync(d_run, h_run, sizeof(SmallArgs) * nrun, hipMemcpyHostToDevice, stream));
        for (int g = 0; g < 3; ++g) {
            if (grp[g].cnt == 0) continue;
            const void *fn = small_batch_kernel(kind, nts[g]);
            HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)grp[g].lds));
            const SmallArgs *arg = d_run + grp[g].first;
            void *kargs[] = {&arg};
            HIPCHK(hipLaunchKernel(fn, dim3((unsigned)grp[g].cnt), dim3((unsigned)nts[g]), kargs, grp[g].lds, stream));
        }
        HIPCHK(hipGetLastError());
        if (!more) break;  // every item has run to its end or to its budget
        HIPCHK(hipMemcpyAsync(h_states, dv, sizeof(DevState) * R, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        std::vector<size_t> next;
        for (size_t k : live) {
            plan[k].done = h_states[k].iters;
            if (h_states[k].status == ST_RUNNING && plan[k].done < max_iter) next.push_back(k);
        }
        live.swap(next);
    }
    if (kind == ELLP_ENGINE_PRIMAL)
        hipLaunchKernelGGL(k_primal_obj_batch, dim3((unsigned)R), dim3(1024), 0, stream, reinterpret_cast<const SmallArgs *>(dv + o_args_all));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, dv, out_bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));

    // ---- per item: status (run_small), statistics (fill_stats), point (ellp_engine_read_point)
    for (size_t k = 0; k < R; ++k) {
        const BatchPlan &p = plan[k];
        ellp_batch_item &it = items[p.item];
        const DevState &s = h_states[k];
        ellp_status st;
        if (it.n_N == 0) st = ELLP_OPTIMAL;  // primal…:149-151 / dual…:175-177
        else if (s.status != ST_RUNNING) st = status_message(s, it.err, sizeof(it.err));
        else st = ELLP_MAXITER;
        status_out[p.item] = st;
        if (stats_out) {
            ellp_stats &o = stats_out[p.item];
            o.iters = s.iters;
            o.pivots = s.pivots;
            o.bound_flips = s.flips;
            o.refactors = s.iters;  // one LU per loop body, as the reference
            o.obj = s.obj;
        }
        memcpy(it.x, h + p.o_x, sizeof(double) * (size_t)it.n_c);
        memcpy(it.B_index, h + p.o_B, sizeof(int64_t) * (size_t)it.m);
        if (it.n_N > 0) {
            memcpy(it.N_index, h + p.o_N, sizeof(int64_t) * (size_t)it.n_N);
            memcpy(it.N_bound, h + p.o_Nb, (size_t)it.n_N);
        }
        if (kind == ELLP_ENGINE_DUAL) {
            memcpy(it.y, h + p.o_y, sizeof(double) * (size_t)it.m);
            memcpy(it.d, h + p.o_d, sizeof(double) * (size_t)it.n_c);
        }
    }
    return ELLP_OPTIMAL;
}

// ellp_batch.inc — ellp_batch_solve_with_initial: many LPs of up to 1,024 rows, one workgroup per LP: k_small_batch for the
// items a single call runs on k_small (m <= 128), k_mid_batch for those it runs on k_mid for the whole solve.
//
// Every item goes through the steps a single call (solve_once on the small path) takes, with the same code where there is
// code to share: check_problem, exact_loop, initial_state and dual_start_feasible of ellp_engine_create, small_threads /
// mid_threads for the workgroup size, the loops of k_small (small_loop) and k_mid (mid_loop) for the iterations, k_primal_obj's
// sum for the objective.  What is batched is the traffic around it: one pinned staging buffer and one device slab hold every
// item of a chunk; the host gathers A_B / A_N / c_B / c_N (copies, so exact) into the staging buffer, which goes up in one
// copy; one launch per kernel and workgroup size (64 / 128 / 256 small, 256 / 512 / 1024 mid) runs every item of that size;
// the states and outputs come back in one copy.  An item that the cap of a launch (16,384 loop bodies on k_small, 4,096 on
// k_mid, as run_small; ELLP_BATCH_LAUNCH_ITERS lowers both) left running is launched again from its device state.  Before
// every round one k_mid_transpose_batch launch makes the row-major copy A_Nt of every mid item, as launch_mid does.
//
// Chunks: the items are taken in consecutive chunks whose slab stays within a budget (2 GiB; ELLP_BATCH_MAX_BYTES lowers it)
// and at most 65,535 items; a chunk is a batch of its own, so chunking changes no item's bits.  The driver below
// (batch_budget, SlabCursor, batch_cuts, batch_open, batch_drive) states that once for every batched call; DESIGN.md §3.1f.
//
// Layout of the slab: [DevState x runnable items][outputs of each item: x, B_index, N_index, Nb (y, d)] | [inputs and
// scratch of each item: A_B, A_N, c_B, c_N, lb, ub, kind, rbuf, kbuf (flist)][SmallArgs of all items][MidArgs of the mid
// items][SmallArgs, MidArgs of the items of the current launch round] | [device-only factors of each mid item: LUa, Ut,
// A_Nt].  Everything left of the first '|' is the one read-back; everything left of the second is the staging buffer.
//
// ellp_batch_primal_solve runs BOTH phases of a primal solve on the same slab: the item goes up once with the costs and
// bounds of both phases ([BatchPhaseRec x items] after the states; c1, c2, lb2, ub2, kind2 after each item's inputs; one
// BatchPhaseArgs per item next to its SmallArgs), the k_small_batch_primal / k_mid_batch_primal twins hand an item from
// phase 1 to phase 2 inside whichever launch ends its phase 1 (batch_two_phase, ellp_small.inc), a launch round gives every
// item the cap of loop bodies whatever its phase, and between rounds the host reads the records only.
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

const void *small_batch_primal_kernel(int nt) {
    if (nt == 64) return reinterpret_cast<const void *>(&k_small_batch_primal<64>);
    if (nt == 128) return reinterpret_cast<const void *>(&k_small_batch_primal<128>);
    return reinterpret_cast<const void *>(&k_small_batch_primal<256>);
}
const void *mid_batch_primal_kernel(int nt) {
    if (nt == 256) return reinterpret_cast<const void *>(&k_mid_batch_primal<256>);
    if (nt == 512) return reinterpret_cast<const void *>(&k_mid_batch_primal<512>);
    return reinterpret_cast<const void *>(&k_mid_batch_primal<1024>);
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

// one runnable item: its kernel, its share of the slab and the byte offsets of its arrays in its chunk's slab
struct BatchPlan {
    int64_t item;  // index into the caller's items
    int64_t ld, nNa, ldn;
    size_t lds;
    int nt;
    bool mid;                                                                // k_mid_batch (else k_small_batch)
    size_t o_x, o_B, o_N, o_Nb, o_y, o_d;                                     // outputs
    size_t o_AB, o_AN, o_cB, o_cN, o_lb, o_ub, o_kind, o_rbuf, o_kbuf, o_fl;  // inputs and scratch
    size_t o_LUa, o_Ut, o_ANt;                                               // device-only factors (mid)
    size_t o_c1, o_c2, o_lb2, o_ub2, o_kind2;                                // whole primal solves: both phases' inputs
    size_t bytes;                                                            // the item's share of the slab (batch_layout)
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

size_t batch_round16(size_t b) { return (b + 15) / 16 * 16; }

// ---- the driver of every batched call (this file, ellp_bpost.inc, ellp_bstart.inc, ellp_brange.inc): the budget, the slab
// cursor of a layout, the chunk cuts, the device and its buffers, the loop over the chunks.  DESIGN.md §3.1f.

// slab bytes per chunk (the staging buffer is a part of it): 2 GiB; ELLP_BATCH_MAX_BYTES only lowers it
size_t batch_budget() {
    size_t budget = (size_t)2 << 30;
    if (const char *v = getenv("ELLP_BATCH_MAX_BYTES"); v && v[0] && atoll(v) > 0 && (size_t)atoll(v) < budget) budget = (size_t)atoll(v);
    return budget;
}

// the array at byte offset `off` of the staging buffer or the slab
template <class T>
T *slab_at(unsigned char *base, size_t off) {
    return reinterpret_cast<T *>(base + off);
}

// The bump allocator of a layout function: arrays in steps of 16 bytes, in the order they are taken.  What is taken while
// `bytes` points at a plan's share counts towards that share; nullptr: a shared array, counted in the shares up front
struct SlabCursor {
    size_t off = 0;
    size_t *bytes = nullptr;
    size_t take(size_t b) {
        const size_t o = off;
        off += batch_round16(b);
        if (bytes) *bytes += batch_round16(b);
        return o;
    }
};

// chunks: consecutive items within the budget (an item alone over it is a chunk of its own) and at most 65,535 items;
// plan[k].bytes is item k's share, slack what the rounding of a chunk's shared arrays may add
template <class Plan>
std::vector<size_t> batch_cuts(const std::vector<Plan> &plan, size_t budget, size_t slack) {
    std::vector<size_t> cut{0};
    size_t acc = slack;
    for (size_t k = 0; k < plan.size(); ++k) {
        if (k > cut.back() && (acc + plan[k].bytes > budget || k - cut.back() >= 65535)) {
            cut.push_back(k);
            acc = slack;
        }
        acc += plan[k].bytes;
    }
    cut.push_back(plan.size());
    return cut;
}

// the device of the call, its host set, a pinned staging buffer and a slab of the sizes the largest chunk needs
ellp_status batch_open(const ellp_opts *opts_in, size_t max_stage, size_t max_total, BatchCleanup &cl, char *errbuf, size_t errlen) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_err(errbuf, errlen, "no HIP device available (this library has no CPU path)");
        return ELLP_ERR_DEVICE;
    }
    int dev = opts_in ? opts_in->device : -1;  // -1, the default: the current device
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
    HIPCHK(hipSetDevice(dev));
    HIPCHK(host_set_acquire(dev, &cl.hs));
    HIPCHK(batch_buf_acquire(dev, true, max_stage, &cl.stage));
    HIPCHK(batch_buf_acquire(dev, false, max_total, &cl.slab));
    return ELLP_OPTIMAL;
}

// The planned items of a call, chunk by chunk.  layout(plan, R) lays R consecutive plans out (offsets, each share in
// Plan::bytes; its result has stage_bytes and total), run_chunk(plan, R, cl) runs them start to end; *chunks counts the
// chunks that ran.  A chunk that does not return ELLP_OPTIMAL ends the call with that status, which every planned item from
// that chunk on and every item of `single` (the caller's single-path items, not run yet) then carries; the call's other
// results are unspecified (ellp_hip.h).  A failure before the first chunk (no device, no buffer) marks no item.  The host
// set, the stage and the slab are held for the chunks only: they are back in their pools, and the stream has drained, when
// the caller's single-path items run (a single call may take the same host set).
template <class Plan, class Layout, class RunChunk>
ellp_status batch_drive(std::vector<Plan> &plan, const std::vector<int64_t> &single, size_t slack, const ellp_opts *opts_in,
                        ellp_status *status_out, uint64_t *chunks, Layout layout, RunChunk run_chunk, char *errbuf, size_t errlen) {
    (void)layout(plan.data(), plan.size());  // every item's share of a slab
    const std::vector<size_t> cut = batch_cuts(plan, batch_budget(), slack);
    size_t max_stage = 0, max_total = 0;
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
        const auto L = layout(plan.data() + cut[c], cut[c + 1] - cut[c]);
        max_stage = L.stage_bytes > max_stage ? L.stage_bytes : max_stage;
        max_total = L.total > max_total ? L.total : max_total;
    }
    BatchCleanup cl;
    if (const ellp_status s = batch_open(opts_in, max_stage, max_total, cl, errbuf, errlen); s != ELLP_OPTIMAL) return s;
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
        const ellp_status rc = run_chunk(plan.data() + cut[c], cut[c + 1] - cut[c], cl);
        if (rc != ELLP_OPTIMAL) {
            for (size_t k = cut[c]; k < plan.size(); ++k) status_out[plan[k].item] = rc;
            for (int64_t i : single) status_out[i] = rc;
            return rc;
        }
        if (chunks) *chunks += 1;
    }
    return ELLP_OPTIMAL;
}

// A_B, A_N, c_B and c_N of an item gathered into the staging buffer h (copies, so exact): columns of ld >= m doubles, zero
// beyond row m; an item without a nonbasic column gets one zero column
inline void batch_stage_basis(unsigned char *h, const ellp_batch_item &it, int64_t ld, size_t o_AB, size_t o_AN, size_t o_cB, size_t o_cN) {
    const int64_t m = it.m, nN = it.n_N;
    double *AB = slab_at<double>(h, o_AB), *AN = slab_at<double>(h, o_AN), *cB = slab_at<double>(h, o_cB), *cN = slab_at<double>(h, o_cN);
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
}

// the fail flag an item's kernel raised on a zero on U's diagonal, read back: the single call's status and message
inline bool batch_item_singular(const unsigned char *h, size_t o_fail, ellp_batch_item &it, ellp_status *status) {
    int fail = 0;
    memcpy(&fail, h + o_fail, sizeof(int));
    if (!fail) return false;
    set_err(it.err, sizeof(it.err), "invalid B, A_B is not invertible");
    *status = ELLP_ERR_SINGULAR;
    return true;
}

// Per-chunk rounding of the four argument arrays, at most (the chunk budget allows for it)
constexpr size_t BATCH_CHUNK_SLACK = 4 * 16;
// ... and of the records and the two BatchPhaseArgs arrays of a whole primal solve
constexpr size_t BATCH_CHUNK_SLACK_PRIMAL = 7 * 16;

// What ellp_batch_primal_solve adds to a batch: the second phase's inputs and the results, by item index
struct BatchTwo {
    const ellp_batch_primal_item *pitems;
    ellp_batch_primal_result *results;
    uint64_t rounds = 0, upload_last = 0, upload_total = 0, chunks = 0;  // ellp_batch_primal_info
};

// The slab of the items plan[0 .. R): offsets into each BatchPlan, and each item's share of the slab in BatchPlan::bytes
// (its own arrays plus its entries of the shared arrays; a chunk's total is their sum plus at most BATCH_CHUNK_SLACK)
struct BatchLayout {
    size_t out_bytes, o_sargs_all, o_margs_all, o_sargs_run, o_margs_run, stage_bytes, total;
    size_t o_rec, o_pargs_all, o_pargs_run;  // whole primal solves
};
BatchLayout batch_layout(int kind, const ellp_batch_item *items, BatchPlan *plan, size_t R, bool bflip, bool two = false) {
    BatchLayout L{};
    SlabCursor cur;
    cur.off = sizeof(DevState) * R;
    if (two) L.o_rec = cur.take(sizeof(BatchPhaseRec) * R);
    size_t nmid = 0;
    for (size_t k = 0; k < R; ++k) {
        BatchPlan &p = plan[k];
        const ellp_batch_item &it = items[p.item];
        cur.bytes = &p.bytes;
        p.bytes = sizeof(DevState) + 2 * sizeof(SmallArgs) + (p.mid ? 2 * sizeof(MidArgs) : 0);
        if (two) p.bytes += sizeof(BatchPhaseRec) + 2 * sizeof(BatchPhaseArgs);
        p.o_x = cur.take(sizeof(double) * (size_t)it.n_c);
        p.o_B = cur.take(sizeof(int64_t) * (size_t)it.m);
        p.o_N = cur.take(sizeof(int64_t) * (size_t)p.nNa);
        p.o_Nb = cur.take((size_t)p.nNa);
        p.o_y = kind == ELLP_ENGINE_DUAL ? cur.take(sizeof(double) * (size_t)p.ld) : 0;
        p.o_d = kind == ELLP_ENGINE_DUAL ? cur.take(sizeof(double) * (size_t)it.n_c) : 0;
        nmid += p.mid ? 1 : 0;
    }
    L.out_bytes = cur.off;
    for (size_t k = 0; k < R; ++k) {
        BatchPlan &p = plan[k];
        const ellp_batch_item &it = items[p.item];
        cur.bytes = &p.bytes;
        p.o_AB = cur.take(sizeof(double) * (size_t)(p.ld * it.m));
        p.o_AN = cur.take(sizeof(double) * (size_t)(p.ld * p.nNa));
        p.o_cB = cur.take(sizeof(double) * (size_t)it.m);
        p.o_cN = cur.take(sizeof(double) * (size_t)p.nNa);
        p.o_lb = cur.take(sizeof(double) * (size_t)it.n_c);
        p.o_ub = cur.take(sizeof(double) * (size_t)it.n_c);
        p.o_kind = cur.take((size_t)it.n_c);
        // k_mid, like k_small, touches rbuf / kbuf at nonbasic positions j < |N| only, and flist up to |N| entries
        p.o_rbuf = cur.take(sizeof(double) * (size_t)p.nNa);
        p.o_kbuf = cur.take(sizeof(double) * (size_t)p.nNa);
        p.o_fl = bflip ? cur.take(sizeof(long long) * (size_t)(p.nNa + 1)) : 0;
        if (two) {
            p.o_c1 = cur.take(sizeof(double) * (size_t)it.n_c);
            p.o_c2 = cur.take(sizeof(double) * (size_t)it.n_c);
            p.o_lb2 = cur.take(sizeof(double) * (size_t)it.n_c);
            p.o_ub2 = cur.take(sizeof(double) * (size_t)it.n_c);
            p.o_kind2 = cur.take((size_t)it.n_c);
        }
    }
    cur.bytes = nullptr;  // the argument arrays: shared, counted in the items' bytes above
    L.o_sargs_all = cur.take(sizeof(SmallArgs) * R);
    L.o_margs_all = cur.take(sizeof(MidArgs) * nmid);
    if (two) L.o_pargs_all = cur.take(sizeof(BatchPhaseArgs) * R);
    L.o_sargs_run = cur.take(sizeof(SmallArgs) * R);  // the round's argument lists are written per round
    L.o_margs_run = cur.take(sizeof(MidArgs) * nmid);
    if (two) L.o_pargs_run = cur.take(sizeof(BatchPhaseArgs) * R);
    L.stage_bytes = cur.off;
    for (size_t k = 0; k < R; ++k) {
        BatchPlan &p = plan[k];
        if (!p.mid) continue;
        cur.bytes = &p.bytes;
        p.o_LUa = cur.take(sizeof(double) * (size_t)(p.ld * p.ld));
        p.o_Ut = cur.take(sizeof(double) * (size_t)(p.ld * p.ld));
        p.o_ANt = cur.take(sizeof(double) * (size_t)(p.ld * p.ldn));
    }
    L.total = cur.off;
    return L;
}

struct BatchRun {
    int kind;
    bool bflip, maxviol;
    double eps;
    uint64_t max_iter, cap_small, cap_mid;
};

// One chunk of runnable items, start to end: staging, upload, launch rounds, objective, read-back, per-item results
ellp_status batch_run_chunk(const BatchRun &cfg, ellp_batch_item *items, BatchPlan *plan, size_t R, BatchCleanup &cl,
                            ellp_status *status_out, ellp_stats *stats_out, BatchTwo *two, char *errbuf, size_t errlen) {
    const int kind = cfg.kind;
    const BatchLayout L = batch_layout(kind, items, plan, R, cfg.bflip, two != nullptr);
    hipStream_t stream = cl.hs.stream;
    unsigned char *h = static_cast<unsigned char *>(cl.stage.p);
    unsigned char *dv = static_cast<unsigned char *>(cl.slab.p);

    // ---- staging: the engine's starting arrays, gathered as ellp_engine_create gathers them on the device
    DevState *h_states = reinterpret_cast<DevState *>(h);
    SmallArgs *h_all = slab_at<SmallArgs>(h, L.o_sargs_all);
    MidArgs *h_mall = slab_at<MidArgs>(h, L.o_margs_all);
    BatchPhaseRec *h_rec = two ? slab_at<BatchPhaseRec>(h, L.o_rec) : nullptr;
    BatchPhaseArgs *h_pall = two ? slab_at<BatchPhaseArgs>(h, L.o_pargs_all) : nullptr;
    std::vector<size_t> mid_at(R, 0);  // position of a mid item in the MidArgs lists
    size_t nmid = 0;
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
        batch_stage_basis(h, it, ld, p.o_AB, p.o_AN, p.o_cB, p.o_cN);
        memcpy(h + p.o_lb, it.lb, sizeof(double) * (size_t)it.n_c);
        memcpy(h + p.o_ub, it.ub, sizeof(double) * (size_t)it.n_c);
        memcpy(h + p.o_kind, it.bound_kind, (size_t)it.n_c);
        SmallArgs a{};
        a.A_B = slab_at<double>(dv, p.o_AB);
        a.A_N = slab_at<double>(dv, p.o_AN);
        a.c_B = slab_at<double>(dv, p.o_cB);
        a.c_N = slab_at<double>(dv, p.o_cN);
        a.x = slab_at<double>(dv, p.o_x);
        a.y = kind == ELLP_ENGINE_DUAL ? slab_at<double>(dv, p.o_y) : nullptr;
        a.dd = kind == ELLP_ENGINE_DUAL ? slab_at<double>(dv, p.o_d) : nullptr;
        a.lb = slab_at<const double>(dv, p.o_lb);
        a.ub = slab_at<const double>(dv, p.o_ub);
        a.kind = slab_at<const uint8_t>(dv, p.o_kind);
        a.B_index = slab_at<int64_t>(dv, p.o_B);
        a.N_index = slab_at<int64_t>(dv, p.o_N);
        a.Nb = slab_at<uint8_t>(dv, p.o_Nb);
        a.rbuf = slab_at<double>(dv, p.o_rbuf);
        a.kbuf = slab_at<double>(dv, p.o_kbuf);
        a.st = reinterpret_cast<DevState *>(dv) + k;
        a.m = m;
        a.ld = ld;
        a.nN = nN;
        a.max_iters = 0;
        a.nch = (int)((nN + 63) / 64);
        a.eps = cfg.eps;
        a.trace = Trace{nullptr, nullptr, 0};
        a.stamps = nullptr;
        a.maxviol = cfg.maxviol ? 1 : 0;
        a.bflip = cfg.bflip ? 1 : 0;
        a.flist = cfg.bflip ? slab_at<long long>(dv, p.o_fl) : nullptr;
        h_all[k] = a;  // k_primal_obj_batch reads every item's, mid items' included
        if (two) {
            const ellp_batch_primal_item &pi = two->pitems[p.item];
            memcpy(h + p.o_c1, it.c, sizeof(double) * (size_t)it.n_c);
            memcpy(h + p.o_c2, pi.c2, sizeof(double) * (size_t)it.n_c);
            memcpy(h + p.o_lb2, pi.lb2, sizeof(double) * (size_t)it.n_c);
            memcpy(h + p.o_ub2, pi.ub2, sizeof(double) * (size_t)it.n_c);
            memcpy(h + p.o_kind2, pi.bound_kind2, (size_t)it.n_c);
            BatchPhaseRec r{};
            r.phase = 1;
            r.obj1 = std::numeric_limits<double>::quiet_NaN();
            h_rec[k] = r;
            BatchPhaseArgs pa{};
            pa.c1 = slab_at<const double>(dv, p.o_c1);
            pa.c2 = slab_at<const double>(dv, p.o_c2);
            pa.lb2 = slab_at<const double>(dv, p.o_lb2);
            pa.ub2 = slab_at<const double>(dv, p.o_ub2);
            pa.kind2 = slab_at<const uint8_t>(dv, p.o_kind2);
            pa.rec = slab_at<BatchPhaseRec>(dv, L.o_rec) + k;
            pa.n_c = it.n_c;
            pa.max_iter = cfg.max_iter;
            h_pall[k] = pa;
        }
        if (p.mid) {
            // launch_mid's arguments, from the same arrays
            MidArgs ma{};
            ma.A_B = a.A_B; ma.A_N = a.A_N; ma.c_B = a.c_B; ma.c_N = a.c_N; ma.x = a.x; ma.y = a.y; ma.dd = a.dd;
            ma.lb = a.lb; ma.ub = a.ub; ma.kind = a.kind; ma.B_index = a.B_index; ma.N_index = a.N_index; ma.Nb = a.Nb;
            ma.rbuf = a.rbuf;
            ma.kbuf = a.kbuf;
            ma.A_Nt = slab_at<double>(dv, p.o_ANt);
            ma.LUa = slab_at<double>(dv, p.o_LUa);
            ma.Ut = slab_at<double>(dv, p.o_Ut);
            ma.st = a.st; ma.m = m; ma.ld = ld; ma.nN = nN; ma.ldn = p.ldn;
            ma.max_iters = 0;
            ma.nch = a.nch;
            ma.eps = cfg.eps;
            ma.trace = Trace{nullptr, nullptr, 0};
            ma.stamps = nullptr;
            ma.maxviol = a.maxviol;
            ma.resync = 0;
            ma.b = nullptr;
            ma.bflip = a.bflip;
            ma.flist = a.flist;
            mid_at[k] = nmid;
            h_mall[nmid++] = ma;
        }
    }
    HIPCHK(hipMemcpyAsync(dv, h, L.o_sargs_run, hipMemcpyHostToDevice, stream));
    uint64_t uploaded = L.o_sargs_run;

    // ---- launch rounds: every item still running, at most a cap of loop bodies each, grouped by kernel and workgroup size
    SmallArgs *h_run = slab_at<SmallArgs>(h, L.o_sargs_run);
    SmallArgs *d_run = slab_at<SmallArgs>(dv, L.o_sargs_run);
    MidArgs *h_mrun = slab_at<MidArgs>(h, L.o_margs_run);
    MidArgs *d_mrun = slab_at<MidArgs>(dv, L.o_margs_run);
    BatchPhaseArgs *h_prun = two ? slab_at<BatchPhaseArgs>(h, L.o_pargs_run) : nullptr;
    BatchPhaseArgs *d_prun = two ? slab_at<BatchPhaseArgs>(dv, L.o_pargs_run) : nullptr;
    const uint64_t max_iter = cfg.max_iter;
    std::vector<size_t> live;  // plan positions that a launch may still advance
    // (a whole solve also takes the items without nonbasic columns: their checks and hand-off are the workgroup's too)
    for (size_t k = 0; k < R; ++k)
        if (items[plan[k].item].n_N > 0 ? max_iter > 0 : two != nullptr) live.push_back(k);
    static const int nts[6] = {64, 128, 256, 256, 512, 1024};  // k_small_batch x 3, k_mid_batch x 3
    while (!live.empty()) {
        if (two) two->rounds += 1;
        size_t nrun = 0, nmrun = 0, nprun = 0;
        int64_t tiles_i = 0, tiles_j = 0;  // the grid of the round's transposes
        bool more = false;                 // some item got less than what its budget still allows
        struct Group { size_t first, cnt, lds, pfirst; };
        Group grp[6];
        for (int g = 0; g < 6; ++g) {
            const bool gmid = g >= 3;
            grp[g] = Group{gmid ? nmrun : nrun, 0, 0, nprun};
            for (size_t k : live) {
                const BatchPlan &p = plan[k];
                if (p.mid != gmid || p.nt != nts[g]) continue;
                const uint64_t remaining = max_iter - p.done;
                const uint64_t cap = gmid ? cfg.cap_mid : cfg.cap_small;
                // a whole solve: the cap itself, shared by the two phases, each of which may need max_iter loop bodies
                const uint64_t n = two ? cap : (remaining < cap ? remaining : cap);
                more = more || (two ? max_iter > cap / 2 : n < remaining);
                if (two) h_prun[nprun++] = h_pall[k];
                if (gmid) {
                    MidArgs a = h_mall[mid_at[k]];
                    a.max_iters = n;
                    h_mrun[nmrun++] = a;
                    const int64_t ti = (a.m + 31) / 32, tj = (a.nN + 31) / 32;
                    tiles_i = ti > tiles_i ? ti : tiles_i;
                    tiles_j = tj > tiles_j ? tj : tiles_j;
                } else {
                    SmallArgs a = h_all[k];
                    a.max_iters = n;
                    h_run[nrun++] = a;
                }
                grp[g].cnt += 1;
                if (p.lds > grp[g].lds) grp[g].lds = p.lds;
            }
        }
        if (nrun) HIPCHK(hipMemcpyAsync(d_run, h_run, sizeof(SmallArgs) * nrun, hipMemcpyHostToDevice, stream));
        if (nprun) HIPCHK(hipMemcpyAsync(d_prun, h_prun, sizeof(BatchPhaseArgs) * nprun, hipMemcpyHostToDevice, stream));
        uploaded += sizeof(SmallArgs) * nrun + sizeof(MidArgs) * nmrun + sizeof(BatchPhaseArgs) * nprun;
        if (nmrun) {
            HIPCHK(hipMemcpyAsync(d_mrun, h_mrun, sizeof(MidArgs) * nmrun, hipMemcpyHostToDevice, stream));
            // the row-major copy of A_N each k_mid launch reads, made afresh as launch_mid makes it
            hipLaunchKernelGGL(k_mid_transpose_batch, dim3((unsigned)tiles_i, (unsigned)tiles_j, (unsigned)nmrun), dim3(256), 0,
                               stream, static_cast<const MidArgs *>(d_mrun));
        }
        for (int g = 0; g < 6; ++g) {
            if (grp[g].cnt == 0) continue;
            const bool gmid = g >= 3;
            const void *fn = two ? (gmid ? mid_batch_primal_kernel(nts[g]) : small_batch_primal_kernel(nts[g]))
                                 : (gmid ? mid_batch_kernel(kind, nts[g]) : small_batch_kernel(kind, nts[g]));
            HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)grp[g].lds));
            const BatchPhaseArgs *parg = two ? d_prun + grp[g].pfirst : nullptr;
            if (gmid) {
                const MidArgs *arg = d_mrun + grp[g].first;
                void *kargs1[] = {&arg}, *kargs2[] = {&arg, &parg};  // each family gets its own parameter list
                HIPCHK(hipLaunchKernel(fn, dim3((unsigned)grp[g].cnt), dim3((unsigned)nts[g]), two ? kargs2 : kargs1, grp[g].lds, stream));
            } else {
                const SmallArgs *arg = d_run + grp[g].first;
                void *kargs1[] = {&arg}, *kargs2[] = {&arg, &parg};
                HIPCHK(hipLaunchKernel(fn, dim3((unsigned)grp[g].cnt), dim3((unsigned)nts[g]), two ? kargs2 : kargs1, grp[g].lds, stream));
            }
        }
        HIPCHK(hipGetLastError());
        if (!more) break;  // every item has run to its end or to its budget
        if (two) {  // the records say who has ended
            HIPCHK(hipMemcpyAsync(h_rec, dv + L.o_rec, sizeof(BatchPhaseRec) * R, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            std::vector<size_t> next;
            for (size_t k : live)
                if (!h_rec[k].done) next.push_back(k);
            live.swap(next);
            continue;
        }
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
        hipLaunchKernelGGL(k_primal_obj_batch, dim3((unsigned)R), dim3(1024), 0, stream, slab_at<const SmallArgs>(dv, L.o_sargs_all));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, dv, L.out_bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));

    if (two) {
        two->chunks += 1;
        two->upload_last = uploaded;
        two->upload_total += uploaded;
    }

    // ---- per item: status (run_small), statistics (fill_stats), point (ellp_engine_read_point)
    for (size_t k = 0; k < R; ++k) {
        const BatchPlan &p = plan[k];
        ellp_batch_item &it = items[p.item];
        const DevState &s = h_states[k];
        ellp_status st;
        if (two && h_rec[k].verdict == ELLP_ERR_PANIC) {  // the checks of solve() after phase 1 (primal…:42-55)
            set_err(it.err, sizeof(it.err), "assertion failed: obj > -EPS");
            st = ELLP_ERR_PANIC;
        } else if (two && h_rec[k].verdict != 0) st = (ellp_status)h_rec[k].verdict;
        else if (it.n_N == 0) st = ELLP_OPTIMAL;  // primal…:149-151 / dual…:175-177
        else if (s.status != ST_RUNNING) st = status_message(s, it.err, sizeof(it.err));
        else st = ELLP_MAXITER;
        status_out[p.item] = st;
        if (two) {
            const BatchPhaseRec &r = h_rec[k];
            ellp_batch_primal_result &o = two->results[p.item];
            o.status = st;
            o.stage = r.phase;
            o.iters_phase1 = r.phase == 2 ? r.iters1 : s.iters;
            o.iters_phase2 = r.phase == 2 ? s.iters : 0;
            o.obj_phase1 = r.obj1;
            o.obj = s.obj;
        }
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

}  // namespace

// ellp_batch_solve_with_initial, and with `two` ellp_batch_primal_solve (kind ELLP_ENGINE_PRIMAL; items: the phase-1 seams)
static ellp_status batch_solve_impl(int kind, int64_t count, ellp_batch_item *items, const ellp_opts *opts_in,
                                    ellp_status *status_out, ellp_stats *stats_out, BatchTwo *two, char *errbuf, size_t errlen) {
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
    BatchRun cfg{};
    cfg.kind = kind;
    cfg.bflip = bflip;
    cfg.maxviol = maxviol;
    cfg.eps = opts.eps > 0.0 ? opts.eps : 1e-10;
    cfg.max_iter = opts.max_iter;
    cfg.cap_small = 16384;
    cfg.cap_mid = 4096;  // run_small's caps
    if (const char *v = getenv("ELLP_BATCH_LAUNCH_ITERS"); v && v[0] && atoll(v) > 0) {
        const uint64_t c = (uint64_t)atoll(v);
        if (c < cfg.cap_small) cfg.cap_small = c;
        if (c < cfg.cap_mid) cfg.cap_mid = c;
    }
    // ---- per item: the single call's checks, then what the batch cannot take (all before any HIP call)
    std::vector<BatchPlan> plan;
    const int64_t mid_auto = plan_env().mid_auto_max;
    for (int64_t i = 0; i < count; ++i) {
        ellp_batch_item &it = items[i];
        it.err[0] = 0;
        if (stats_out) memset(&stats_out[i], 0, sizeof(ellp_stats));
        ellp_status s = check_problem(kind, it.m, it.n, it.n_c, it.A, it.c, it.b, it.bound_kind, it.lb, it.ub, it.x, it.B_index,
                                      it.n_B, it.N_index, it.N_bound, it.n_N, it.y, it.d, it.err, sizeof(it.err));
        ExactLoop loop = EXACT_NONE;
        size_t slds = 0, mlds = 0;
        if (s == ELLP_OPTIMAL) {
            // the kernel the single call with these options runs for the whole solve; an item it would run on the
            // explicit-inverse engine or the certified hybrid is not run at all
            slds = small_lds_bytes(it.m, it.n_N);
            mlds = mid_lds_bytes(it.m, it.n_N);
            loop = exact_loop(opts, bflip, false, opts.partial_segments, it.m, slds, mlds, mid_auto);
            if (loop == EXACT_NONE) {
                if (it.m > MID_MAX_M)
                    set_err(it.err, sizeof(it.err), "batch: the LU-per-iteration kernels of a batch take up to %d rows (this LP: m = %lld)",
                            MID_MAX_M, (long long)it.m);
                else if (it.m > SMALL_MAX_M && mlds == 0)
                    set_err(it.err, sizeof(it.err), "batch: the LU-per-iteration kernel k_mid takes up to %d rows and %d nonbasic columns "
                                                    "within 150 KB of LDS (this LP: m = %lld, |N| = %lld)",
                            MID_MAX_M, 4096 * 64, (long long)it.m, (long long)it.n_N);
                else if (it.m > SMALL_MAX_M)
                    set_err(it.err, sizeof(it.err), "batch: this LP (m = %lld, |N| = %lld) is over %d rows, where a batch runs only what a "
                                                    "single call runs on k_mid (pipeline 3, dual bound flipping, pipeline 0 with m <= "
                                                    "ELLP_MID_AUTO_MAX); these options select an explicit-inverse engine",
                            (long long)it.m, (long long)it.n_N, SMALL_MAX_M);
                else
                    set_err(it.err, sizeof(it.err), "batch: the LU-per-iteration kernel of a batch takes up to %d rows within 150 KB of LDS "
                                                    "(this LP: m = %lld, |N| = %lld)", SMALL_MAX_M, (long long)it.m, (long long)it.n_N);
                s = ELLP_ERR_ARG;
            }
        }
        if (s == ELLP_OPTIMAL && kind == ELLP_ENGINE_DUAL && !dual_start_feasible(it.n_N, it.N_index, it.N_bound, it.d, cfg.eps, it.err, sizeof(it.err)))
            s = ELLP_ERR_PANIC;
        status_out[i] = s;
        if (s != ELLP_OPTIMAL) continue;
        if (two)
            for (int64_t j = 0; j < it.n_c; ++j)
                if (two->pitems[i].bound_kind2[j] > 4) {
                    set_err(errbuf, errlen, "item %lld: bound_kind2[%lld] out of range", (long long)i, (long long)j);
                    return ELLP_ERR_ARG;
                }
        BatchPlan p;
        p.item = i;
        p.ld = round_up(it.m, 16);
        p.nNa = it.n_N > 0 ? it.n_N : 1;
        p.mid = loop == EXACT_MID;
        p.ldn = p.mid ? (it.n_N + 15) / 16 * 16 : 0;
        p.lds = p.mid ? mlds : slds;
        p.nt = p.mid ? mid_threads(it.m) : small_threads(it.m, it.n_N);
        plan.push_back(p);
    }
    if (plan.empty()) return ELLP_OPTIMAL;

    // ---- the chunks, through the driver (every planned item runs on the batched kernels: no single-path items)
    return batch_drive(
        plan, {}, two ? BATCH_CHUNK_SLACK_PRIMAL : BATCH_CHUNK_SLACK, &opts, status_out, nullptr,
        [&](BatchPlan *pl, size_t R) { return batch_layout(kind, items, pl, R, bflip, two != nullptr); },
        [&](BatchPlan *pl, size_t R, BatchCleanup &cl) { return batch_run_chunk(cfg, items, pl, R, cl, status_out, stats_out, two, errbuf, errlen); },
        errbuf, errlen);
}

// the calling thread's calls of ellp_batch_solve_with_initial (ellp_batch_solve_info): how many so far, the last one's items and kind
static thread_local uint64_t g_batch_solve_info[4] = {0, 0, 0, 0};

extern "C" void ellp_batch_solve_info(uint64_t *out4) {
    if (!out4) return;
    for (int k = 0; k < 4; ++k) out4[k] = g_batch_solve_info[k];
}

extern "C" ellp_status ellp_batch_solve_with_initial(int kind, int64_t count, ellp_batch_item *items, const ellp_opts *opts_in,
                                                     ellp_status *status_out, ellp_stats *stats_out, char *errbuf,
                                                     size_t errlen) {
    g_batch_solve_info[0] += 1;
    g_batch_solve_info[1] = count > 0 ? (uint64_t)count : 0;
    g_batch_solve_info[2] = (uint64_t)kind;
    return batch_solve_impl(kind, count, items, opts_in, status_out, stats_out, nullptr, errbuf, errlen);
}

// the last ellp_batch_primal_solve of the calling thread that passed the checks of the call (ellp_batch_primal_info)
static thread_local uint64_t g_batch_primal_info[4] = {0, 0, 0, 0};

extern "C" ellp_status ellp_batch_primal_solve(int64_t count, ellp_batch_primal_item *items, const ellp_opts *opts_in,
                                               ellp_batch_primal_result *results, char *errbuf, size_t errlen) {
    if (errbuf && errlen) errbuf[0] = 0;
    if (count < 0 || (count > 0 && (!items || !results))) {
        set_err(errbuf, errlen, "count < 0, or items / results NULL");
        return ELLP_ERR_ARG;
    }
    for (int64_t i = 0; i < count; ++i)
        if (!items[i].c2 || !items[i].bound_kind2 || !items[i].lb2 || !items[i].ub2) {
            set_err(errbuf, errlen, "item %lld: c2, bound_kind2, lb2 or ub2 NULL", (long long)i);
            return ELLP_ERR_ARG;
        }
    // the phase-1 seams as a batch of their own; their messages go back into the caller's items
    std::vector<ellp_batch_item> seams((size_t)count);
    std::vector<ellp_status> status((size_t)count);
    std::vector<ellp_stats> stats((size_t)count);
    for (int64_t i = 0; i < count; ++i) {
        seams[(size_t)i] = items[i].p1;
        ellp_batch_primal_result &r = results[i];
        memset(&r, 0, sizeof(r));
        r.stage = 1;
        r.obj_phase1 = std::numeric_limits<double>::quiet_NaN();
    }
    BatchTwo two{};
    two.pitems = items;
    two.results = results;
    const ellp_status rc = batch_solve_impl(ELLP_ENGINE_PRIMAL, count, seams.data(), opts_in, status.data(), stats.data(), &two,
                                            errbuf, errlen);
    for (int64_t i = 0; i < count; ++i) {
        memcpy(items[i].p1.err, seams[(size_t)i].err, sizeof(items[i].p1.err));
        if (rc != ELLP_OPTIMAL || status[(size_t)i] < 0) results[i].status = rc != ELLP_OPTIMAL ? rc : status[(size_t)i];
    }
    if (rc == ELLP_ERR_ARG) return rc;  // refused by the checks of the call: the record keeps the last call that passed them
    g_batch_primal_info[0] = two.rounds;
    g_batch_primal_info[1] = two.upload_last;
    g_batch_primal_info[2] = two.upload_total;
    g_batch_primal_info[3] = two.chunks;
    return rc;
}

extern "C" void ellp_batch_primal_info(uint64_t *out4) {
    if (!out4) return;
    for (int k = 0; k < 4; ++k) out4[k] = g_batch_primal_info[k];
}

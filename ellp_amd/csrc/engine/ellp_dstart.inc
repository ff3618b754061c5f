// ellp_dstart.inc — ellp_batch_dual_phase1_start: the starting point of ellp_engine_create_dual_phase1 for many LPs in the
// launches of one.
//
// For every item, the steps the single call takes on a k_small / k_mid engine, with the same device code: the blocked
// rebuild of B^-1 from A_B (launch_refactor: probe, permutation shortcut, or k_ref_init + macro panels + k_ref_permute),
// y = B^-T c_B (launch_btran), d, labels and nonbasic values (k_dual_rephase, phase-1 labelling), x_B = B^-1 (b - A_N x_N)
// (launch_resync with force = 1), then on the host the loop's entry assertion and the objective (host_dual_obj).  The
// kernel bodies are the device functions the single-engine kernels call (bl_*_body, ref_*_body, btran_*_body,
// resync_*_body, dual_rephase_body).  Each batch kernel reads a per-item record (DStartItem, the argument structs the
// single call would build) with the item in grid dimension z; the grid covers the largest item and blocks beyond an
// item's own grid exit.  Every parameter the single call derives from m (splits, ksplit, btran tiles, the k_bl_factor
// variant and sub-panel width) is derived the same way per item, so each item's arithmetic is the single call's.
//
// Host synchronisations: one after the probe of all items (which items need the general elimination) and one at the
// end (the read-back).  Items whose rebuild failed are stopped by their DevState as in the single call (every later kernel
// checks it; k_dual_rephase, which does not, is skipped for them here).
//
// Slab per chunk: [DevState x items][per item: x, y, d, N_bound] (the one read-back) | [item records, general-case
// map][per item: inputs A_B, A_N, c_B, c, b, lb, ub, kind, B_index, N_index, maxbits] (the one upload, from a pinned
// staging buffer) | [per item scratch: W0, W1, rebuild panels, BTRAN / resync partials].  Chunks follow the budget of
// ellp_batch_solve_with_initial (2 GiB, ELLP_BATCH_MAX_BYTES lowers it; at most 65,535 items); a chunk is a batch of its
// own, so chunking changes no item's bits.
//
// Included at the end of ellp_engine.hip, after ellp_batch.inc (whose pinned / device buffer pool it uses).

namespace {

struct DStartItem {
    BlArgs bl;
    RefArgs ref;
    BtranArgs bt;
    DualRephaseArgs dr;
    ResyncArgs rs;
    double *nzval;
    int64_t *nzrow;
    int32_t *nzcnt;
    int nbw_max;  // the sub-panel width launch_refactor picks for this m
};

__device__ __forceinline__ const DStartItem &ds_item(const DStartItem *items, const int32_t *map) {
    return items[map ? map[blockIdx.z] : blockIdx.z];
}
__device__ __forceinline__ int64_t ds_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- blocked rebuild (launch_refactor)
__global__ __launch_bounds__(256) void k_ds_probe(const DStartItem *items) {
    const DStartItem &it = ds_item(items, nullptr);
    if (blockIdx.x >= ds_cdiv(it.bl.m, 4)) return;
    bl_probe_body(it.bl, it.nzval, it.nzrow, it.nzcnt, blockIdx.x);
}
__global__ __launch_bounds__(1024) void k_ds_perm_check(const DStartItem *items) {
    const DStartItem &it = ds_item(items, nullptr);
    bl_perm_check_body(it.bl, it.nzval, it.nzrow, it.nzcnt);
}
__global__ __launch_bounds__(256) void k_ds_perm_fill(const DStartItem *items) {
    const DStartItem &it = ds_item(items, nullptr);
    if (blockIdx.x >= it.bl.m) return;
    bl_perm_fill_body(it.bl, it.nzval, it.nzrow, blockIdx.x);
}
// launch_refactor's reset of DevState::do_update after the probe, for every item
__global__ __launch_bounds__(256) void k_ds_clear(const DStartItem *items, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) items[i].bl.st->do_update = 0;
}
__global__ __launch_bounds__(256) void k_ds_ref_init(const DStartItem *items, const int32_t *map) {
    ref_init_body(ds_item(items, map).ref, blockIdx.x, gridDim.x);
}
// the macro panel's arguments as launch_refactor has them at (k0, j0); false: the item has no such panel / sub-panel
__device__ __forceinline__ bool ds_panel(const DStartItem &it, int k0, int j0, bool after_sub, BlArgs &a) {
    a = it.bl;
    if (k0 >= a.m) return false;
    a.k0 = k0;
    a.nbc = (int)((a.m - k0) < BL_NB ? (a.m - k0) : BL_NB);
    if (after_sub) {  // k_bl_gather / k_bl_gemm2: sel after all sub-panels of this macro panel
        a.sel = (int)(ds_cdiv(a.nbc, it.nbw_max) & 1);
        return true;
    }
    if (j0 < 0) {  // k_bl_gemm1 / k_bl_sum
        a.sel = 0;
        return true;
    }
    if (j0 >= a.nbc) return false;
    a.j0 = j0;
    a.nbw = (a.nbc - j0) < it.nbw_max ? (a.nbc - j0) : it.nbw_max;
    a.nacc = j0;
    a.sel = (j0 / it.nbw_max) & 1;
    return true;
}
__global__ __launch_bounds__(256) void k_ds_gemm1(const DStartItem *items, const int32_t *map, int k0) {
    const DStartItem &it = ds_item(items, map);
    BlArgs a;
    if (!ds_panel(it, k0, -1, false, a)) return;
    if (blockIdx.x >= ds_cdiv(a.m, 64) || (int)blockIdx.y >= a.splits) return;
    bl_gemm1_body(a, blockIdx.x, blockIdx.y);
}
__global__ __launch_bounds__(256) void k_ds_sum(const DStartItem *items, const int32_t *map, int k0) {
    const DStartItem &it = ds_item(items, map);
    BlArgs a;
    if (!ds_panel(it, k0, -1, false, a)) return;
    bl_sum_body(a, blockIdx.x, gridDim.x);
}
template <int NBW, int RPT, int NT>
__global__ __launch_bounds__(NT) void k_ds_factor(const DStartItem *items, const int32_t *map, int k0, int j0) {
    const DStartItem &it = ds_item(items, map);
    BlArgs a;
    if (!ds_panel(it, k0, j0, false, a)) return;
    bl_factor_body<NBW, RPT, NT>(a);
}
__global__ __launch_bounds__(256) void k_ds_apply(const DStartItem *items, const int32_t *map, int k0, int j0) {
    const DStartItem &it = ds_item(items, map);
    BlArgs a;
    if (!ds_panel(it, k0, j0, false, a)) return;
    if (blockIdx.x >= ds_cdiv(a.m, 8)) return;
    bl_apply_body(a, blockIdx.x);
}
__global__ __launch_bounds__(256) void k_ds_gather(const DStartItem *items, const int32_t *map, int k0) {
    const DStartItem &it = ds_item(items, map);
    BlArgs a;
    if (!ds_panel(it, k0, 0, true, a)) return;
    bl_gather_body(a, blockIdx.x);
}
__global__ __launch_bounds__(256) void k_ds_gemm2(const DStartItem *items, const int32_t *map, int k0) {
    const DStartItem &it = ds_item(items, map);
    BlArgs a;
    if (!ds_panel(it, k0, 0, true, a)) return;
    if (blockIdx.x >= ds_cdiv(a.ld, 128) || blockIdx.y >= ds_cdiv(a.m, 64)) return;
    bl_gemm2_body(a, blockIdx.x, blockIdx.y);
}
__global__ __launch_bounds__(256) void k_ds_ref_permute(const DStartItem *items, const int32_t *map) {
    const DStartItem &it = ds_item(items, map);
    if (blockIdx.x >= it.ref.m) return;
    ref_permute_body(it.ref, blockIdx.x);
}
__global__ void k_ds_ref_finish(const DStartItem *items, const int32_t *map) { ref_finish_body(ds_item(items, map).ref); }

// ---- the point from the inverse (dual_point_from_inverse)
__global__ __launch_bounds__(256) void k_ds_btran_part(const DStartItem *items) {
    const DStartItem &it = ds_item(items, nullptr);
    if (blockIdx.x >= ds_cdiv(it.bt.ld >> 1, 256) || (int)blockIdx.y >= it.bt.ntiles) return;
    btran_part_body(it.bt, blockIdx.x, blockIdx.y);
}
__global__ __launch_bounds__(256) void k_ds_btran_reduce(const DStartItem *items) {
    const DStartItem &it = ds_item(items, nullptr);
    if (blockIdx.x >= ds_cdiv(it.bt.ld, 256)) return;
    btran_reduce_body(it.bt, blockIdx.x);
}
__global__ __launch_bounds__(256) void k_ds_rephase(const DStartItem *items) {
    const DStartItem &it = ds_item(items, nullptr);
    if (it.dr.st->status != ST_RUNNING) return;  // the single call stops before this kernel when the rebuild failed
    if (blockIdx.x >= ds_cdiv(it.dr.nN + it.dr.m, 4)) return;
    dual_rephase_body(it.dr, blockIdx.x);
}
__global__ __launch_bounds__(256) void k_ds_resync_gather(const DStartItem *items) {
    const DStartItem &it = ds_item(items, nullptr);
    if (blockIdx.x >= ds_cdiv(it.rs.nN, 256)) return;
    resync_gather_body(it.rs, blockIdx.x);
}
__global__ __launch_bounds__(256) void k_ds_resync_part(const DStartItem *items) {
    const DStartItem &it = ds_item(items, nullptr);
    if (blockIdx.x >= ds_cdiv(it.rs.ld >> 1, 256) || (int)blockIdx.y >= it.rs.ntiles) return;
    resync_part_body(it.rs, blockIdx.x, blockIdx.y);
}
__global__ __launch_bounds__(256) void k_ds_resync_rhs(const DStartItem *items) {
    const DStartItem &it = ds_item(items, nullptr);
    if (blockIdx.x >= ds_cdiv(it.rs.ld, 256)) return;
    resync_rhs_body(it.rs, blockIdx.x);
}
__global__ __launch_bounds__(256) void k_ds_resync_xb(const DStartItem *items) {
    const DStartItem &it = ds_item(items, nullptr);
    if (blockIdx.x >= ds_cdiv(it.rs.m, 4)) return;
    resync_xb_body(it.rs, blockIdx.x);
}
__global__ __launch_bounds__(256) void k_ds_resync_apply(const DStartItem *items) {
    const DStartItem &it = ds_item(items, nullptr);
    if (blockIdx.x >= ds_cdiv(it.rs.m, 256)) return;
    resync_apply_body(it.rs, blockIdx.x);
}

// per item: its geometry (as engine_create_impl derives it from m) and the byte offsets of its arrays in the chunk's slab
struct DsPlan : RebuildGeometry {
    int64_t item;
    int64_t m, n, nN, ld;
    size_t o_x, o_y, o_d, o_nb;                                                // read-back region
    size_t o_AB, o_AN, o_cB, o_c, o_b, o_lb, o_ub, o_kind, o_B, o_N, o_maxb;   // upload region
    size_t o_W0, o_W1, o_Cp, o_C, o_V, o_Vs, o_Wp, o_Pm, o_nzv, o_nzr, o_nzc, o_used, o_perm, o_up, o_tv, o_cand, o_xg;  // scratch
    size_t out_bytes, in_bytes, scratch_bytes;
};

size_t ds_al(size_t b) { return (b + 255) / 256 * 256; }

void ds_geometry(DsPlan &p) {
    const int64_t m = p.m;
    p.ld = round_up(m, 16);
    static_cast<RebuildGeometry &>(p) = rebuild_geometry(m);
    const int64_t m_ = p.m, n = p.n, nN = p.nN, ld = p.ld, nNa = nN > 0 ? nN : 1;
    size_t o = 0;
    p.o_x = o; o += ds_al(sizeof(double) * (size_t)n);
    p.o_y = o; o += ds_al(sizeof(double) * (size_t)ld);
    p.o_d = o; o += ds_al(sizeof(double) * (size_t)n);
    p.o_nb = o; o += ds_al((size_t)nNa);
    p.out_bytes = o;
    o = 0;
    p.o_AB = o; o += ds_al(sizeof(double) * (size_t)(ld * m_));
    p.o_AN = o; o += ds_al(sizeof(double) * (size_t)(ld * nNa));
    p.o_cB = o; o += ds_al(sizeof(double) * (size_t)m_);
    p.o_c = o; o += ds_al(sizeof(double) * (size_t)n);
    p.o_b = o; o += ds_al(sizeof(double) * (size_t)ld);
    p.o_lb = o; o += ds_al(sizeof(double) * (size_t)n);
    p.o_ub = o; o += ds_al(sizeof(double) * (size_t)n);
    p.o_kind = o; o += ds_al((size_t)n);
    p.o_B = o; o += ds_al(sizeof(int64_t) * (size_t)m_);
    p.o_N = o; o += ds_al(sizeof(int64_t) * (size_t)nNa);
    p.o_maxb = o; o += ds_al(2 * sizeof(unsigned long long));
    p.in_bytes = o;
    o = 0;
    p.o_W0 = o; o += ds_al(sizeof(double) * (size_t)(m_ * ld));
    p.o_W1 = o; o += ds_al(sizeof(double) * (size_t)(m_ * ld));
    p.o_Cp = o; o += ds_al(sizeof(double) * (size_t)(p.bl_splits * m_ * BL_NB));
    p.o_C = o; o += ds_al(sizeof(double) * (size_t)(2 * m_ * BL_NB));
    p.o_V = o; o += ds_al(sizeof(double) * (size_t)(2 * m_ * BL_NB));
    p.o_Vs = o; o += ds_al(sizeof(double) * (size_t)(m_ * 16));
    p.o_Wp = o; o += ds_al(sizeof(double) * (size_t)(BL_NB * ld));
    p.o_Pm = o; o += ds_al(sizeof(int64_t) * (size_t)BL_NB);
    p.o_nzv = o; o += ds_al(sizeof(double) * (size_t)m_);
    p.o_nzr = o; o += ds_al(sizeof(int64_t) * (size_t)m_);
    p.o_nzc = o; o += ds_al(sizeof(int32_t) * (size_t)m_);
    p.o_used = o; o += ds_al(sizeof(int32_t) * (size_t)m_);
    p.o_perm = o; o += ds_al(sizeof(int64_t) * (size_t)m_);
    p.o_up = o; o += ds_al(sizeof(double) * (size_t)(p.btran_tiles * ld));
    p.o_tv = o; o += ds_al(sizeof(double) * (size_t)ld);
    p.o_cand = o; o += ds_al(sizeof(double) * (size_t)ld);
    p.o_xg = o; o += ds_al(sizeof(double) * (size_t)nNa);
    p.scratch_bytes = o;
}

struct DsCleanup {
    BatchBuf stage, slab;
    ~DsCleanup() {
        batch_buf_release(stage);
        batch_buf_release(slab);
    }
};

// One chunk, start to end.  Returns ELLP_OPTIMAL or ELLP_ERR_DEVICE (errbuf set); per-item results in status_out / obj_out.
ellp_status ds_run_chunk(int device, hipStream_t stream, ellp_batch_item *items, DsPlan *plan, size_t R, int nbw_max, int bl_nt,
                         double eps, ellp_status *status_out, double *obj_out, char *errbuf, size_t errlen) {
    // ---- slab layout
    const size_t st_bytes = ds_al(sizeof(DevState) * R);
    size_t out_total = st_bytes;
    std::vector<size_t> out_at(R), in_at(R), sc_at(R);
    for (size_t k = 0; k < R; ++k) {
        out_at[k] = out_total;
        out_total += plan[k].out_bytes;
    }
    const size_t rec_at = out_total;
    size_t in_total = rec_at + ds_al(sizeof(DStartItem) * R);
    const size_t map_at = in_total;
    in_total += ds_al(sizeof(int32_t) * R);
    for (size_t k = 0; k < R; ++k) {
        in_at[k] = in_total;
        in_total += plan[k].in_bytes;
    }
    size_t total = in_total;
    for (size_t k = 0; k < R; ++k) {
        sc_at[k] = total;
        total += plan[k].scratch_bytes;
    }
    DsCleanup cl;
    hipError_t rc = batch_buf_acquire(device, true, in_total, &cl.stage);
    if (rc == hipSuccess) rc = batch_buf_acquire(device, false, total, &cl.slab);
    if (rc != hipSuccess) {
        (void)hipGetLastError();
        set_err(errbuf, errlen, "dual phase-1 start batch: no memory for a chunk of %zu items (%zu bytes)", R, total);
        return ELLP_ERR_DEVICE;
    }
    char *h = static_cast<char *>(cl.stage.p);
    char *dv = static_cast<char *>(cl.slab.p);
    memset(h, 0, in_total);
    int64_t mmax = 0, ldmax = 0, nNmax = 0, tmax = 0;
    std::vector<double> zeros;
    DStartItem *rec = reinterpret_cast<DStartItem *>(h + rec_at);
    for (size_t k = 0; k < R; ++k) {
        const DsPlan &p = plan[k];
        const ellp_batch_item &it = items[p.item];
        const int64_t m = p.m, n = p.n, nN = p.nN, ld = p.ld;
        mmax = m > mmax ? m : mmax;
        ldmax = ld > ldmax ? ld : ldmax;
        nNmax = nN > nNmax ? nN : nNmax;
        tmax = p.btran_tiles > tmax ? p.btran_tiles : tmax;
        // inputs: A_B / A_N / c_B gathered on the host (copies, so exact; zero rows up to ld as k_gather_cols writes them)
        char *in = h + in_at[k];
        double *AB = reinterpret_cast<double *>(in + p.o_AB), *AN = reinterpret_cast<double *>(in + p.o_AN);
        double *cB = reinterpret_cast<double *>(in + p.o_cB);
        for (int64_t j = 0; j < m; ++j) {
            memcpy(AB + j * ld, it.A + it.B_index[j] * m, sizeof(double) * (size_t)m);
            cB[j] = it.c[it.B_index[j]];
        }
        for (int64_t j = 0; j < nN; ++j) memcpy(AN + j * ld, it.A + it.N_index[j] * m, sizeof(double) * (size_t)m);
        memcpy(in + p.o_c, it.c, sizeof(double) * (size_t)n);
        memcpy(in + p.o_b, it.b, sizeof(double) * (size_t)m);
        memcpy(in + p.o_lb, it.lb, sizeof(double) * (size_t)n);
        memcpy(in + p.o_ub, it.ub, sizeof(double) * (size_t)n);
        memcpy(in + p.o_kind, it.bound_kind, (size_t)n);
        memcpy(in + p.o_B, it.B_index, sizeof(int64_t) * (size_t)m);
        if (nN > 0) memcpy(in + p.o_N, it.N_index, sizeof(int64_t) * (size_t)nN);
        // the device state ellp_engine_create_dual_phase1 starts from (x = y = d = 0, every nonbasic label Lower)
        zeros.assign((size_t)(n > m ? n : m), 0.0);
        const DevState init = initial_state(ELLP_ENGINE_DUAL, m, n, nN, it.c, it.b, it.bound_kind, it.lb, it.ub, zeros.data(), zeros.data(),
                                            zeros.data());
        memcpy(h + sizeof(DevState) * k, &init, sizeof(DevState));
        memset(h + out_at[k] + p.o_nb, ELLP_NB_LOWER, (size_t)(nN > 0 ? nN : 1));
        // device pointers of the item
        char *o = dv + out_at[k], *di = dv + in_at[k], *s = dv + sc_at[k];
        DevState *st = reinterpret_cast<DevState *>(dv) + k;
        double *W0 = reinterpret_cast<double *>(s + p.o_W0), *W1 = reinterpret_cast<double *>(s + p.o_W1);
        const double *dAB = reinterpret_cast<const double *>(di + p.o_AB), *dAN = reinterpret_cast<const double *>(di + p.o_AN);
        int64_t *dB = reinterpret_cast<int64_t *>(di + p.o_B), *dN = reinterpret_cast<int64_t *>(di + p.o_N);
        double *x = reinterpret_cast<double *>(o + p.o_x), *y = reinterpret_cast<double *>(o + p.o_y);
        double *dd = reinterpret_cast<double *>(o + p.o_d);
        uint8_t *Nb = reinterpret_cast<uint8_t *>(o + p.o_nb);
        int32_t *used = reinterpret_cast<int32_t *>(s + p.o_used);
        int64_t *perm = reinterpret_cast<int64_t *>(s + p.o_perm);
        double *upart = reinterpret_cast<double *>(s + p.o_up);
        DStartItem r;
        memset(&r, 0, sizeof(r));
        BlArgs &a = r.bl;
        a.W0 = W0; a.W1 = W1; a.A_B = dAB; a.Cpart = reinterpret_cast<double *>(s + p.o_Cp);
        a.C0 = reinterpret_cast<double *>(s + p.o_C); a.C1 = a.C0 + m * BL_NB;
        a.V0 = reinterpret_cast<double *>(s + p.o_V); a.V1 = a.V0 + m * BL_NB;
        a.Vs = reinterpret_cast<double *>(s + p.o_Vs); a.Wp = reinterpret_cast<double *>(s + p.o_Wp);
        a.used = used; a.perm = perm; a.Pm = reinterpret_cast<int64_t *>(s + p.o_Pm); a.st = st; a.m = m; a.ld = ld;
        a.splits = p.bl_splits;
        a.ksplit = (int)round_up((m + p.bl_splits - 1) / p.bl_splits, 16);
        a.eps = 0.0;  // a dual engine's rebuild guard (launch_refactor)
        r.ref = RefArgs{W0, W1, nullptr, dAB, used, perm, st, m, ld, p.upd_rows, 0.0};
        // BTRAN straight into y: the single call writes u (DevState::usel = 0 there) and copies all ld entries into y
        r.bt = BtranArgs{W0, W1, reinterpret_cast<const double *>(di + p.o_cB), upart, y, y + ld, st, m, ld, p.btran_rows,
                         p.btran_tiles};
        r.dr = DualRephaseArgs{dAN, dAB, y, reinterpret_cast<const double *>(di + p.o_c), reinterpret_cast<const uint8_t *>(di + p.o_kind),
                               reinterpret_cast<const double *>(di + p.o_lb), reinterpret_cast<const double *>(di + p.o_ub), dN, dB,
                               dd, x, Nb, st, m, ld, nN, eps, 1};
        r.rs = ResyncArgs{dAN, W0, W1, reinterpret_cast<const double *>(di + p.o_b), x, reinterpret_cast<double *>(s + p.o_xg),
                          reinterpret_cast<double *>(s + p.o_tv), upart, reinterpret_cast<double *>(s + p.o_cand),
                          reinterpret_cast<unsigned long long *>(di + p.o_maxb), dB, dN, st, m, ld, nN, 0, p.btran_tiles, 1};
        r.rs.cols_per_tile = (int)((nN + p.btran_tiles - 1) / p.btran_tiles);
        r.nzval = reinterpret_cast<double *>(s + p.o_nzv);
        r.nzrow = reinterpret_cast<int64_t *>(s + p.o_nzr);
        r.nzcnt = reinterpret_cast<int32_t *>(s + p.o_nzc);
        r.nbw_max = nbw_max;
        rec[k] = r;
    }
#define DSCHK(expr)                                                                                                     \
    do {                                                                                                                \
        hipError_t _e = (expr);                                                                                         \
        if (_e != hipSuccess) {                                                                                         \
            (void)hipStreamSynchronize(stream);                                                                         \
            set_err(errbuf, errlen, "HIP error %s in ellp_batch_dual_phase1_start (%s)", hipGetErrorString(_e), #expr); \
            return ELLP_ERR_DEVICE;                                                                                     \
        }                                                                                                               \
    } while (0)
    DSCHK(hipMemcpyAsync(dv, h, in_total, hipMemcpyHostToDevice, stream));
    const DStartItem *drec = reinterpret_cast<const DStartItem *>(dv + rec_at);
    int32_t *dmap = reinterpret_cast<int32_t *>(dv + map_at);
    const unsigned Z = (unsigned)R;
    // ---- rebuild: the permutation probe of every item, then one synchronisation
    hipLaunchKernelGGL(k_ds_probe, dim3((unsigned)((mmax + 3) / 4), 1, Z), dim3(256), 0, stream, drec);
    hipLaunchKernelGGL(k_ds_perm_check, dim3(1, 1, Z), dim3(1024), 0, stream, drec);
    hipLaunchKernelGGL(k_ds_perm_fill, dim3((unsigned)mmax, 1, Z), dim3(256), 0, stream, drec);
    std::vector<DevState> sts(R);
    DSCHK(hipMemcpyAsync(sts.data(), dv, sizeof(DevState) * R, hipMemcpyDeviceToHost, stream));
    DSCHK(hipStreamSynchronize(stream));
    hipLaunchKernelGGL(k_ds_clear, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, stream, drec, (int64_t)R);
    std::vector<int32_t> gen;
    int64_t gmax = 0, gldmax = 0;
    for (size_t k = 0; k < R; ++k)
        if (sts[k].status == ST_RUNNING && !sts[k].do_update) {
            gen.push_back((int32_t)k);
            gmax = plan[k].m > gmax ? plan[k].m : gmax;
            gldmax = plan[k].ld > gldmax ? plan[k].ld : gldmax;
        }
    if (!gen.empty()) {  // ---- general case, for the items that are not a generalised permutation
        DSCHK(hipMemcpyAsync(dmap, gen.data(), sizeof(int32_t) * gen.size(), hipMemcpyHostToDevice, stream));
        const unsigned G = (unsigned)gen.size();
        hipLaunchKernelGGL(k_ds_ref_init, dim3(1024, 1, G), dim3(256), 0, stream, drec, dmap);
        for (int k0 = 0; k0 < gmax; k0 += BL_NB) {
            hipLaunchKernelGGL(k_ds_gemm1, dim3((unsigned)((gmax + 63) / 64), 8, G), dim3(256), 0, stream, drec, dmap, k0);
            hipLaunchKernelGGL(k_ds_sum, dim3(256, 1, G), dim3(256), 0, stream, drec, dmap, k0);
            for (int j0 = 0; j0 < BL_NB; j0 += nbw_max) {
                if (bl_nt == 512) {
                    if (nbw_max == 16) hipLaunchKernelGGL((k_ds_factor<16, 4, 512>), dim3(1, 1, G), dim3(512), 0, stream, drec, dmap, k0, j0);
                    else if (nbw_max == 8) hipLaunchKernelGGL((k_ds_factor<8, 8, 512>), dim3(1, 1, G), dim3(512), 0, stream, drec, dmap, k0, j0);
                    else hipLaunchKernelGGL((k_ds_factor<4, 16, 512>), dim3(1, 1, G), dim3(512), 0, stream, drec, dmap, k0, j0);
                } else {
                    if (nbw_max == 16) hipLaunchKernelGGL((k_ds_factor<16, 2, 1024>), dim3(1, 1, G), dim3(1024), 0, stream, drec, dmap, k0, j0);
                    else if (nbw_max == 8) hipLaunchKernelGGL((k_ds_factor<8, 4, 1024>), dim3(1, 1, G), dim3(1024), 0, stream, drec, dmap, k0, j0);
                    else hipLaunchKernelGGL((k_ds_factor<4, 8, 1024>), dim3(1, 1, G), dim3(1024), 0, stream, drec, dmap, k0, j0);
                }
                hipLaunchKernelGGL(k_ds_apply, dim3((unsigned)((gmax + 7) / 8), 1, G), dim3(256), 0, stream, drec, dmap, k0, j0);
            }
            hipLaunchKernelGGL(k_ds_gather, dim3(BL_NB, 1, G), dim3(256), 0, stream, drec, dmap, k0);
            hipLaunchKernelGGL(k_ds_gemm2, dim3((unsigned)((gldmax + 127) / 128), (unsigned)((gmax + 63) / 64), G), dim3(256), 0, stream,
                               drec, dmap, k0);
        }
        hipLaunchKernelGGL(k_ds_ref_permute, dim3((unsigned)gmax, 1, G), dim3(256), 0, stream, drec, dmap);
        hipLaunchKernelGGL(k_ds_ref_finish, dim3(1, 1, G), dim3(1), 0, stream, drec, dmap);
    }
    // ---- y, d, labels and values, x_B (every kernel but k_dual_rephase skips an item whose rebuild failed)
    const int64_t halfmax = ldmax >> 1;
    hipLaunchKernelGGL(k_ds_btran_part, dim3((unsigned)((halfmax + 255) / 256), (unsigned)tmax, Z), dim3(256), 0, stream, drec);
    hipLaunchKernelGGL(k_ds_btran_reduce, dim3((unsigned)((ldmax + 255) / 256), 1, Z), dim3(256), 0, stream, drec);
    hipLaunchKernelGGL(k_ds_rephase, dim3((unsigned)((nNmax + mmax + 3) / 4), 1, Z), dim3(256), 0, stream, drec);
    if (nNmax > 0) {
        hipLaunchKernelGGL(k_ds_resync_gather, dim3((unsigned)((nNmax + 255) / 256), 1, Z), dim3(256), 0, stream, drec);
        hipLaunchKernelGGL(k_ds_resync_part, dim3((unsigned)((halfmax + 255) / 256), (unsigned)tmax, Z), dim3(256), 0, stream, drec);
        hipLaunchKernelGGL(k_ds_resync_rhs, dim3((unsigned)((ldmax + 255) / 256), 1, Z), dim3(256), 0, stream, drec);
        hipLaunchKernelGGL(k_ds_resync_xb, dim3((unsigned)((mmax + 3) / 4), 1, Z), dim3(256), 0, stream, drec);
        hipLaunchKernelGGL(k_ds_resync_apply, dim3((unsigned)((mmax + 255) / 256), 1, Z), dim3(256), 0, stream, drec);
    }
    DSCHK(hipGetLastError());
    // ---- one read-back: states and outputs
    DSCHK(hipMemcpyAsync(h, dv, out_total, hipMemcpyDeviceToHost, stream));
    DSCHK(hipStreamSynchronize(stream));
#undef DSCHK
    for (size_t k = 0; k < R; ++k) {
        const DsPlan &p = plan[k];
        ellp_batch_item &it = items[p.item];
        DevState st;
        memcpy(&st, h + sizeof(DevState) * k, sizeof(DevState));
        const char *o = h + out_at[k];
        const double *x = reinterpret_cast<const double *>(o + p.o_x), *y = reinterpret_cast<const double *>(o + p.o_y);
        const double *d = reinterpret_cast<const double *>(o + p.o_d);
        const uint8_t *Nb = reinterpret_cast<const uint8_t *>(o + p.o_nb);
        ellp_status s = ELLP_OPTIMAL;
        if (st.status != ST_RUNNING) s = status_message(st, it.err, sizeof(it.err));
        else if (!dual_start_feasible(p.nN, it.N_index, Nb, d, eps, it.err, sizeof(it.err))) s = ELLP_ERR_PANIC;
        status_out[p.item] = s;
        if (s != ELLP_OPTIMAL) continue;
        memcpy(it.x, x, sizeof(double) * (size_t)p.n);
        if (p.nN > 0) memcpy(it.N_bound, Nb, (size_t)p.nN);
        memcpy(it.y, y, sizeof(double) * (size_t)p.m);
        memcpy(it.d, d, sizeof(double) * (size_t)p.n);
        if (obj_out) obj_out[p.item] = host_dual_obj(p.m, p.n, it.b, it.bound_kind, it.lb, it.ub, y, d);
    }
    return ELLP_OPTIMAL;
}

}  // namespace

extern "C" ellp_status ellp_batch_dual_phase1_start(int64_t count, ellp_batch_item *items, const ellp_opts *opts_in,
                                                    ellp_status *status_out, double *obj_out, char *errbuf, size_t errlen) {
    if (errbuf && errlen) errbuf[0] = 0;
    if (count < 0 || (count > 0 && (!items || !status_out))) {
        set_err(errbuf, errlen, "count < 0, or items / status_out NULL");
        return ELLP_ERR_ARG;
    }
    ellp_opts opts;
    ellp_default_opts(&opts);
    if (opts_in) opts = *opts_in;
    const bool bflip = (opts.flags & ELLP_FLAG_DUAL_BOUND_FLIPPING) != 0;
    if (refuse_bflip_pipeline(opts, bflip, opts.partial_segments, errbuf, errlen)) return ELLP_ERR_ARG;
    if (const char *v = getenv("ELLP_REBUILD"); v && !strcmp(v, "columnwise")) {
        set_err(errbuf, errlen, "dual phase-1 start batch: ELLP_REBUILD=columnwise selects the column-by-column rebuild, which a batch does not run");
        return ELLP_ERR_ARG;
    }
    const double eps = opts.eps > 0.0 ? opts.eps : 1e-10;
    const int64_t mid_auto = plan_env().mid_auto_max;
    // ---- per item: the single call's checks, then what the batch cannot take (all before any HIP call)
    std::vector<DsPlan> plan;
    for (int64_t i = 0; i < count; ++i) {
        ellp_batch_item &it = items[i];
        it.err[0] = 0;
        if (obj_out) obj_out[i] = 0.0;
        ellp_status s = ELLP_OPTIMAL;
        if (it.m <= 0 || it.n <= it.m || !it.A || !it.c || !it.b || !it.bound_kind || !it.lb || !it.ub || !it.B_index ||
            !it.N_index || !it.x || !it.N_bound || !it.y || !it.d) {
            set_err(it.err, sizeof(it.err), "bad arguments (a nonbasic variable is needed: n > m; A, c, b, bounds, B_index, "
                                            "N_index, x, N_bound, y and d are needed)");
            s = ELLP_ERR_ARG;
        } else if (it.m > MID_MAX_M) {
            set_err(it.err, sizeof(it.err), "dual phase-1 start batch: m = %lld; the batch takes up to %d rows", (long long)it.m, MID_MAX_M);
            s = ELLP_ERR_ARG;
        } else {
            const int64_t nN = it.n - it.m;
            std::vector<double> zeros((size_t)it.n, 0.0);
            std::vector<uint8_t> Nb((size_t)nN, (uint8_t)ELLP_NB_LOWER);
            s = check_problem(ELLP_ENGINE_DUAL, it.m, it.n, it.n, it.A, it.c, it.b, it.bound_kind, it.lb, it.ub, zeros.data(),
                              it.B_index, it.m, it.N_index, Nb.data(), nN, zeros.data(), zeros.data(), it.err, sizeof(it.err));
            if (s == ELLP_OPTIMAL &&
                exact_loop(opts, bflip, false, opts.partial_segments, it.m, small_lds_bytes(it.m, nN), mid_lds_bytes(it.m, nN), mid_auto) == EXACT_NONE) {
                set_err(it.err, sizeof(it.err), "dual phase-1 start batch: these options run m = %lld on the explicit-inverse engine "
                                                "(its start comes from another factorisation); pipeline 3, bound flipping or "
                                                "ELLP_MID_AUTO_MAX select the LU-per-iteration kernels", (long long)it.m);
                s = ELLP_ERR_ARG;
            }
        }
        status_out[i] = s;
        if (s != ELLP_OPTIMAL) continue;
        DsPlan p{};
        p.item = i;
        p.m = it.m;
        p.n = it.n;
        p.nN = it.n - it.m;
        ds_geometry(p);
        plan.push_back(p);
    }
    if (plan.empty()) return ELLP_OPTIMAL;
    // the sub-panel width and k_bl_factor variant launch_refactor picks (every item has m <= 1,024, so the same for all)
    const auto [bl_nt, nbw_max] = bl_factor_variant(MID_MAX_M);
    const size_t budget = batch_budget();
    int dev = opts.device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_err(errbuf, errlen, "no HIP device available (this library has no CPU path)");
        return ELLP_ERR_DEVICE;
    }
    if (hipSetDevice(dev) != hipSuccess) {
        set_err(errbuf, errlen, "hipSetDevice(%d) failed", dev);
        return ELLP_ERR_DEVICE;
    }
    HostSet hs;
    if (host_set_acquire(dev, &hs) != hipSuccess) {
        set_err(errbuf, errlen, "no stream for the batch");
        return ELLP_ERR_DEVICE;
    }
    size_t k = 0;
    ellp_status rc = ELLP_OPTIMAL;
    while (k < plan.size() && rc == ELLP_OPTIMAL) {
        size_t e = k, acc = 0;
        while (e < plan.size()) {
            const size_t b = sizeof(DevState) + sizeof(DStartItem) + sizeof(int32_t) + 768 + plan[e].out_bytes + plan[e].in_bytes +
                             plan[e].scratch_bytes;
            if (e > k && (acc + b > budget || e - k >= 65535)) break;
            acc += b;
            ++e;
        }
        rc = ds_run_chunk(dev, hs.stream, items, plan.data() + k, e - k, nbw_max, bl_nt, eps, status_out, obj_out, errbuf, errlen);
        k = e;
    }
    host_set_release(hs);
    return rc;
}

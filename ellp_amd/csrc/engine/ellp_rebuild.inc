// ellp_rebuild.inc — B^-1 from A_B in blocks (SURVEY.md §8 f1; replaces the m x 3 launches of the
// product-form rebuild, 45 ms at m = 2000 and 250 ms at m = 4000).
//
// Same elimination as before — Gauss-Jordan on W (starting from I) with partial pivoting: the basic
// columns come in one at a time, alpha = W a_k, pivot row p = first maximum of |alpha_i| over the rows
// not used yet, eta update with row p — so the pivots are still partial-pivot LU's U_kk and the
// reference's singularity guard (any |U_ii| < EPS is Err("A_B is not invertible"), primal…:175-179)
// applies to them unchanged.  What changes is the order of the arithmetic:
//
//   macro panel of NB = 64 columns K:
//     C = W A_B[:, K]                          one GEMM (m x m x 64), split over K for parallelism
//     sub-panels of 16 / 8 / 4 columns:        ONE workgroup holds the m x nb sub-panel in registers and
//       k_bl_factor                            does its nb pivot steps there (two barriers per step): the
//                                              result is V_s = T_s[:, P_s] - I[:, P_s], T_s = E_nb ... E_1
//       k_bl_apply                             the rest of C and the accumulated V of the macro panel get
//                                              T_s applied:  M <- M + V_s M[P_s, :]  (2 MB, L2-resident)
//     W <- W + V_acc W[P, :]                   one rank-64 update of the whole inverse (read + write once)
//
// so B^-1 is read and written once per 64 columns instead of once per column.  Rows are permuted at the
// end as before (row k belongs to basic position k).
//
// Shortcut: a basis whose columns have one nonzero each in distinct rows — the artificial basis of
// primal phase 1, the slack basis a dual start uses — is inverted by inspection (k_bl_probe / k_bl_perm);
// its LU pivots are those nonzeros.

constexpr int BL_NB = 64;

#ifdef ELLP_BL_STAMPS
// dev builds (-DELLP_BL_STAMPS): 100 MHz ticks of k_bl_factor's phases, summed over launches [load, search, publish, update, store, launches]
__device__ unsigned long long g_bl_stamps[8];
#define BL_STAMP(slot)                                        \
    if (tid == 0) {                                           \
        const unsigned long long _t = wall_clock64();         \
        atomicAdd(&g_bl_stamps[slot], _t - t_prev);           \
        t_prev = _t;                                          \
    }
#else
#define BL_STAMP(slot)
#endif

struct BlArgs {
    double *W0, *W1;
    const double *A_B;
    double *Cpart;      // [splits][m][BL_NB] partial products of the macro panel
    double *C0, *C1;    // m x BL_NB, ping-pong: the macro panel under elimination
    double *V0, *V1;    // m x BL_NB, ping-pong: accumulated V of the macro panel
    double *Vs;         // m x 16: the sub-panel's V_s
    double *Wp;         // BL_NB x ld: the pivot rows of the macro panel
    int32_t *used;
    int64_t *perm;      // perm[k] = pivot row of basic column k
    int64_t *Pm;        // pivot rows of the current macro panel (BL_NB)
    DevState *st;
    int64_t m, ld;
    int k0;             // first column of the macro panel
    int nbc;            // columns in the macro panel (<= BL_NB)
    int j0, nbw;        // sub-panel: columns [j0, j0 + nbw) of the macro panel
    int nacc;           // columns of V accumulated so far in this macro panel (= j0)
    int splits, ksplit; // G1: K-range per split
    int sel;            // ping-pong selector of (C, V): input = sel, output = sel ^ 1
    double eps;
};

// ---- shortcut: generalised permutation matrix
__device__ __forceinline__ void bl_probe_body(BlArgs a, double *nzval, int64_t *nzrow, int32_t *nzcnt, unsigned bx) {
    // one wave per basic column: count its nonzeros, remember the (last) one
    const int lane = threadIdx.x & 63;
    const int64_t k = (int64_t)bx * 4 + (threadIdx.x >> 6);
    if (k >= a.m) return;
    const double *col = a.A_B + k * a.ld;
    int cnt = 0;
    long long row = -1;
    double val = 0.0;
    for (int64_t i = lane; i < a.m; i += WAVE) {
        const double v = col[i];
        if (v != 0.0) {  // NaN counts as a nonzero
            cnt += 1;
            row = i;
            val = v;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int oc = __shfl_xor(cnt, o);
        const long long orow = __shfl_xor(row, o);
        const double ov = __shfl_xor(val, o);
        if (orow > row) {
            row = orow;
            val = ov;
        }
        cnt += oc;
    }
    if (lane == 0) {
        nzcnt[k] = cnt;
        nzrow[k] = row;
        nzval[k] = val;
    }
}
__global__ __launch_bounds__(256) void k_bl_probe(BlArgs a, double *nzval, int64_t *nzrow, int32_t *nzcnt) { bl_probe_body(a, nzval, nzrow, nzcnt, blockIdx.x); }
// one block: is it a generalised permutation?  (every column one nonzero, all rows distinct).  Writes
// st->do_update = 1 if so (and applies the singularity guard to the pivots), 0 otherwise.
// twin of k_bl_perm_check's body (kept in step by hand; tests/test_gpu_batch_dual_start.py compares them bit for bit)
__device__ __forceinline__ void bl_perm_check_body(BlArgs a, const double *nzval, const int64_t *nzrow,
                                                         const int32_t *nzcnt) {
    DevState *st = a.st;
    if (st->status != ST_RUNNING) return;
    int bad = 0, sing = 0;
    for (int64_t k = threadIdx.x; k < a.m; k += 1024) a.used[k] = 0;
    __syncthreads();
    for (int64_t k = threadIdx.x; k < a.m; k += 1024) {
        if (nzcnt[k] != 1) {
            bad = 1;
        } else {
            if (atomicAdd(&a.used[nzrow[k]], 1) != 0) bad = 1;
            const double v = fabs(nzval[k]);
            if (v != v || v == INFINITY || v == 0.0 || v < a.eps) sing = 1;  // 1 / Inf would be a finite, singular W
        }
    }
    bad = __syncthreads_or(bad);
    sing = __syncthreads_or(sing);
    if (threadIdx.x == 0) {
        st->do_update = bad ? 0 : 1;
        if (!bad && sing) st->status = ELLP_ERR_SINGULAR;
    }
}
// the single-engine kernel keeps its own copy of the body, twin of bl_perm_check_body: calling that costs it 2 VGPRs (DESIGN.md §3.1g)
__global__ __launch_bounds__(1024) void k_bl_perm_check(BlArgs a, const double *nzval, const int64_t *nzrow,
                                                         const int32_t *nzcnt) {
    DevState *st = a.st;
    if (st->status != ST_RUNNING) return;
    int bad = 0, sing = 0;
    for (int64_t k = threadIdx.x; k < a.m; k += 1024) a.used[k] = 0;
    __syncthreads();
    for (int64_t k = threadIdx.x; k < a.m; k += 1024) {
        if (nzcnt[k] != 1) {
            bad = 1;
        } else {
            if (atomicAdd(&a.used[nzrow[k]], 1) != 0) bad = 1;
            const double v = fabs(nzval[k]);
            if (v != v || v == INFINITY || v == 0.0 || v < a.eps) sing = 1;  // 1 / Inf would be a finite, singular W
        }
    }
    bad = __syncthreads_or(bad);
    sing = __syncthreads_or(sing);
    if (threadIdx.x == 0) {
        st->do_update = bad ? 0 : 1;
        if (!bad && sing) st->status = ELLP_ERR_SINGULAR;
    }
}
// W[cur] = inverse of the generalised permutation: row k has 1 / v_k at column nzrow[k]
__device__ __forceinline__ void bl_perm_fill_body(BlArgs a, const double *nzval, const int64_t *nzrow, unsigned bx) {
    const DevState *st = a.st;
    if (st->status != ST_RUNNING || !st->do_update) return;
    double *W = st->cur ? a.W1 : a.W0;
    const int64_t k = bx;
    double2 *row = reinterpret_cast<double2 *>(W + k * a.ld);
    for (int64_t t = threadIdx.x; t < (a.ld >> 1); t += 256) row[t] = make_double2(0.0, 0.0);
    __syncthreads();
    if (threadIdx.x == 0) W[k * a.ld + nzrow[k]] = 1.0 / nzval[k];
}
__global__ __launch_bounds__(256) void k_bl_perm_fill(BlArgs a, const double *nzval, const int64_t *nzrow) { bl_perm_fill_body(a, nzval, nzrow, blockIdx.x); }

// ---- G1: Cpart[s][i][j] = sum over t in split s of W[i][t] * A_B[(k0 + j) ld + t]
// block = 64 rows x 64 columns, 256 threads, 4 x 4 outputs each, K tiles of 16 through LDS
__device__ __forceinline__ void bl_gemm1_body(BlArgs a, unsigned bx, unsigned by) {
    __shared__ double sA[16][64 + 1];
    __shared__ double sB[16][64 + 1];
    const DevState *st = a.st;
    if (st->status != ST_RUNNING) return;
    const double *W = st->cur ? a.W1 : a.W0;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t i0 = (int64_t)bx * 64;
    const int s = by;
    const int64_t t_lo = (int64_t)s * a.ksplit, t_hi = (t_lo + a.ksplit < a.m) ? t_lo + a.ksplit : a.m;
    double acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
    const int lr = tid >> 2, lk = (tid & 3) * 4;  // staging: row / column lr, 4 consecutive k
    for (int64_t t0 = t_lo; t0 < t_hi; t0 += 16) {
        {
            const int64_t i = i0 + lr;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t t = t0 + lk + c;
                sA[lk + c][lr] = (i < a.m && t < t_hi) ? W[i * a.ld + t] : 0.0;
            }
            const int j = lr;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t t = t0 + lk + c;
                sB[lk + c][j] = (j < a.nbc && t < t_hi) ? a.A_B[(int64_t)(a.k0 + j) * a.ld + t] : 0.0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            double av[4], bv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) av[r] = sA[kk][ty * 4 + r];
#pragma unroll
            for (int c = 0; c < 4; ++c) bv[c] = sB[kk][tx * 4 + c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] = fma(av[r], bv[c], acc[r][c]);
        }
        __syncthreads();
    }
    double *out = a.Cpart + (int64_t)s * a.m * BL_NB;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t i = i0 + ty * 4 + r;
        if (i >= a.m) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) out[i * BL_NB + tx * 4 + c] = acc[r][c];
    }
}
__global__ __launch_bounds__(256) void k_bl_gemm1(BlArgs a) { bl_gemm1_body(a, blockIdx.x, blockIdx.y); }
// C[sel] = sum of the splits in a fixed order; V[sel] = 0
__device__ __forceinline__ void bl_sum_body(BlArgs a, unsigned bx, unsigned gx) {
    if (a.st->status != ST_RUNNING) return;
    double *C = a.sel ? a.C1 : a.C0;
    double *V = a.sel ? a.V1 : a.V0;
    const int64_t total = a.m * BL_NB;
    for (int64_t e = (int64_t)bx * 256 + threadIdx.x; e < total; e += (int64_t)gx * 256) {
        double s = 0.0;
        for (int k = 0; k < a.splits; ++k) s += a.Cpart[(int64_t)k * total + e];
        C[e] = s;
        V[e] = 0.0;
    }
}
__global__ __launch_bounds__(256) void k_bl_sum(BlArgs a) { bl_sum_body(a, blockIdx.x, gridDim.x); }

// ---- sub-panel: NBW pivot steps in the registers of one workgroup (1024 threads, RPT rows each)
// NT threads (a power of two, 256 or 1024), RPT rows per thread (NT * RPT >= m), NBW columns
// twin of k_bl_factor's body (kept in step by hand; tests/test_gpu_batch_dual_start.py compares them bit for bit)
template <int NBW, int RPT, int NT>
__device__ __forceinline__ void bl_factor_body(BlArgs a) {
    __shared__ double s_v[2][16];
    __shared__ long long s_i[2][16];
    __shared__ double s_prow[2][16];
    __shared__ long long s_pm[16];
    DevState *st = a.st;
    if (st->status != ST_RUNNING) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#ifdef ELLP_BL_STAMPS
    unsigned long long t_prev = wall_clock64();
    if (tid == 0) atomicAdd(&g_bl_stamps[5], 1ull);
#endif
    const double *C = a.sel ? a.C1 : a.C0;
    double r[RPT][NBW];
    bool used[RPT];
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr) {
        const int64_t i = tid + NT * rr;
        used[rr] = i < a.m ? (a.used[i] != 0) : true;
        // 16-byte loads (a row of the macro panel is BL_NB doubles and j0 is even, so a pair never leaves the row);
        // the tile's 256 KB go through ONE CU: the load and the store below were a third of the kernel as 8-byte accesses
        const double2 *row2 = reinterpret_cast<const double2 *>(C + (i < a.m ? i : 0) * BL_NB + a.j0);
#pragma unroll
        for (int c = 0; c < NBW; c += 2) {
            const double2 v = row2[c >> 1];
            r[rr][c] = (i < a.m && c < a.nbw) ? v.x : 0.0;
            r[rr][c + 1] = (i < a.m && c + 1 < a.nbw) ? v.y : 0.0;
        }
    }
    // The step loop is unrolled (every register index is a constant) and synchronises through LDS only
    // (lds_barrier: lgkmcnt, not vmcnt): a DPP search inside each wave, one barrier, every thread folds the
    // NT/64 wave candidates itself, the owner publishes the pivot row, a second barrier, the update.  In-kernel
    // stamps (tools/bl_stamps.py): every phase is bound by the vector instructions the waves of ONE CU issue, not
    // by the barriers.  LDS scratch is double-buffered by the parity of the step.
    bool dead = false;  // a singular pivot was met (uniform)
    BL_STAMP(0)
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
        if (j < a.nbw && !dead) {
        const int par = j & 1;
        // ---- pivot: first maximum of |alpha_i| over the rows not used yet
        double bv = -1.0;
        long long bi = -1;
#pragma unroll
        for (int rr = 0; rr < RPT; ++rr) {
            const double v = fabs(r[rr][j]);
            if (!used[rr] && v > bv) {  // rows of a thread come in increasing order: strict keeps the first
                bv = v;
                bi = tid + NT * rr;
            }
        }
        {
            // the wave's first maximum: DPP maximum of |alpha|, then DPP minimum of the row among the lanes that hold it
            // (the ds_bpermute butterfly this replaces was six dependent steps through the LDS crossbar)
            const double nv = bv != bv ? INFINITY : bv;  // a NaN must surface as the pivot and fail the test below
            const double wm = wave_allmax_dpp(nv);
            const int wi = wave_allmin_dpp((nv == wm && bi >= 0) ? (int)bi : 0x7fffffff);
            bv = wi == 0x7fffffff ? -1.0 : (wm == INFINITY ? NAN : wm);
            bi = wi == 0x7fffffff ? -1 : wi;
        }
        if (lane == 0) {
            s_v[par][wave] = bv;
            s_i[par][wave] = bi;
        }
        lds_barrier();
        BL_STAMP(1)
        // every thread folds the NT/64 wave candidates itself (a broadcast read each): no second search by wave 0, no
        // second barrier
        bv = s_v[par][0];
        bi = s_i[par][0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) {
            const double ov = s_v[par][w];
            const long long oi = s_i[par][w];
            if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) {
                bv = ov;
                bi = oi;
            }
        }
        // primal: any |U_ii| < EPS is Err("A_B is not invertible") (primal…:175-179); dual: only a zero pivot
        const bool bad = bi < 0 || bv != bv || bv == 0.0 || bv < a.eps;
        if (bad && tid == 0) {
            st->refk = a.k0 + a.j0 + j;  // diagnostics: which column, which pivot
            st->r = bi;
            st->d_r = bv;
            st->status = ELLP_ERR_SINGULAR;
        }
        const long long p = bad ? -1 : bi;
        if (p < 0) {
            dead = true;  // uniform
        } else {
        // ---- the owner publishes the pivot row of the tile
        if ((p & (NT - 1)) == tid) {
#pragma unroll
            for (int rr = 0; rr < RPT; ++rr)
                if (rr == (int)(p / NT)) {
#pragma unroll
                    for (int c = 0; c < NBW; ++c) s_prow[par][c] = r[rr][c];
                    used[rr] = true;
                }
            s_pm[j] = p;
        }
        lds_barrier();
        double prow[NBW];
#pragma unroll
        for (int c = 0; c < NBW; ++c) prow[c] = s_prow[par][c];
        BL_STAMP(2)
        const double inv = 1.0 / prow[j];
        // ---- eta with row p on the whole tile; column j keeps the eta column itself.  The step is bound by the
        // number of vector instructions (m x NBW updates on ONE CU), so the pivot's own row is not singled out by
        // a select per element: its registers are multiplied by 0 (every other row's by 1, exact) and it takes
        // f = 1/pivot, which makes fma(f, prow[c], 0) = prow[c] / pivot exactly the value the select form stored
#pragma unroll
        for (int rr = 0; rr < RPT; ++rr) {
            const bool is_p = tid + NT * rr == p;
            const double keep = is_p ? 0.0 : 1.0;
            const double f = is_p ? inv : -(r[rr][j] * inv);
#pragma unroll
            for (int c = 0; c < NBW; ++c) {
                if (c == j) r[rr][c] = f;
                else r[rr][c] = fma(f, prow[c], r[rr][c] * keep);
            }
        }
        BL_STAMP(3)
        }  // p >= 0
        }  // j < nbw
    }
    if (dead) return;
    // ---- bookkeeping of the pivots, V_s = T_s[:, P_s] - I[:, P_s]
    lds_barrier();
    if (tid < a.nbw) {
        const long long p = s_pm[tid];
        a.used[p] = 1;
        a.perm[a.k0 + a.j0 + tid] = p;
        a.Pm[a.j0 + tid] = p;
    }
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr) {
        const int64_t i = tid + NT * rr;
        if (i >= a.m) continue;
        double2 *vrow = reinterpret_cast<double2 *>(a.Vs + i * 16);
#pragma unroll
        for (int c = 0; c < NBW; c += 2) {
            double v0 = r[rr][c], v1 = r[rr][c + 1];
            if (c < a.nbw && s_pm[c] == i) v0 -= 1.0;
            if (c + 1 < a.nbw && s_pm[c + 1] == i) v1 -= 1.0;
            if (c + 1 < a.nbw) vrow[c >> 1] = make_double2(v0, v1);
            else if (c < a.nbw) a.Vs[i * 16 + c] = v0;
        }
    }
    BL_STAMP(4)
}
// the single-engine kernel keeps its own copy of the body, twin of bl_factor_body: calling that costs k_bl_factor<16, *, *> 12 VGPRs and
// k_bl_factor<16, 2, 1024> 4 more scalar spills (DESIGN.md §3.1g)
template <int NBW, int RPT, int NT>
__global__ __launch_bounds__(NT) void k_bl_factor(BlArgs a) {
    __shared__ double s_v[2][16];
    __shared__ long long s_i[2][16];
    __shared__ double s_prow[2][16];
    __shared__ long long s_pm[16];
    DevState *st = a.st;
    if (st->status != ST_RUNNING) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#ifdef ELLP_BL_STAMPS
    unsigned long long t_prev = wall_clock64();
    if (tid == 0) atomicAdd(&g_bl_stamps[5], 1ull);
#endif
    const double *C = a.sel ? a.C1 : a.C0;
    double r[RPT][NBW];
    bool used[RPT];
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr) {
        const int64_t i = tid + NT * rr;
        used[rr] = i < a.m ? (a.used[i] != 0) : true;
        // 16-byte loads (a row of the macro panel is BL_NB doubles and j0 is even, so a pair never leaves the row);
        // the tile's 256 KB go through ONE CU: the load and the store below were a third of the kernel as 8-byte accesses
        const double2 *row2 = reinterpret_cast<const double2 *>(C + (i < a.m ? i : 0) * BL_NB + a.j0);
#pragma unroll
        for (int c = 0; c < NBW; c += 2) {
            const double2 v = row2[c >> 1];
            r[rr][c] = (i < a.m && c < a.nbw) ? v.x : 0.0;
            r[rr][c + 1] = (i < a.m && c + 1 < a.nbw) ? v.y : 0.0;
        }
    }
    // The step loop is unrolled (every register index is a constant) and synchronises through LDS only
    // (lds_barrier: lgkmcnt, not vmcnt): a DPP search inside each wave, one barrier, every thread folds the
    // NT/64 wave candidates itself, the owner publishes the pivot row, a second barrier, the update.  In-kernel
    // stamps (tools/bl_stamps.py): every phase is bound by the vector instructions the waves of ONE CU issue, not
    // by the barriers.  LDS scratch is double-buffered by the parity of the step.
    bool dead = false;  // a singular pivot was met (uniform)
    BL_STAMP(0)
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
        if (j < a.nbw && !dead) {
        const int par = j & 1;
        // ---- pivot: first maximum of |alpha_i| over the rows not used yet
        double bv = -1.0;
        long long bi = -1;
#pragma unroll
        for (int rr = 0; rr < RPT; ++rr) {
            const double v = fabs(r[rr][j]);
            if (!used[rr] && v > bv) {  // rows of a thread come in increasing order: strict keeps the first
                bv = v;
                bi = tid + NT * rr;
            }
        }
        {
            // the wave's first maximum: DPP maximum of |alpha|, then DPP minimum of the row among the lanes that hold it
            // (the ds_bpermute butterfly this replaces was six dependent steps through the LDS crossbar)
            const double nv = bv != bv ? INFINITY : bv;  // a NaN must surface as the pivot and fail the test below
            const double wm = wave_allmax_dpp(nv);
            const int wi = wave_allmin_dpp((nv == wm && bi >= 0) ? (int)bi : 0x7fffffff);
            bv = wi == 0x7fffffff ? -1.0 : (wm == INFINITY ? NAN : wm);
            bi = wi == 0x7fffffff ? -1 : wi;
        }
        if (lane == 0) {
            s_v[par][wave] = bv;
            s_i[par][wave] = bi;
        }
        lds_barrier();
        BL_STAMP(1)
        // every thread folds the NT/64 wave candidates itself (a broadcast read each): no second search by wave 0, no
        // second barrier
        bv = s_v[par][0];
        bi = s_i[par][0];
#pragma unroll
        for (int w = 1; w < NT / 64; ++w) {
            const double ov = s_v[par][w];
            const long long oi = s_i[par][w];
            if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) {
                bv = ov;
                bi = oi;
            }
        }
        // primal: any |U_ii| < EPS is Err("A_B is not invertible") (primal…:175-179); dual: only a zero pivot
        const bool bad = bi < 0 || bv != bv || bv == 0.0 || bv < a.eps;
        if (bad && tid == 0) {
            st->refk = a.k0 + a.j0 + j;  // diagnostics: which column, which pivot
            st->r = bi;
            st->d_r = bv;
            st->status = ELLP_ERR_SINGULAR;
        }
        const long long p = bad ? -1 : bi;
        if (p < 0) {
            dead = true;  // uniform
        } else {
        // ---- the owner publishes the pivot row of the tile
        if ((p & (NT - 1)) == tid) {
#pragma unroll
            for (int rr = 0; rr < RPT; ++rr)
                if (rr == (int)(p / NT)) {
#pragma unroll
                    for (int c = 0; c < NBW; ++c) s_prow[par][c] = r[rr][c];
                    used[rr] = true;
                }
            s_pm[j] = p;
        }
        lds_barrier();
        double prow[NBW];
#pragma unroll
        for (int c = 0; c < NBW; ++c) prow[c] = s_prow[par][c];
        BL_STAMP(2)
        const double inv = 1.0 / prow[j];
        // ---- eta with row p on the whole tile; column j keeps the eta column itself.  The step is bound by the
        // number of vector instructions (m x NBW updates on ONE CU), so the pivot's own row is not singled out by
        // a select per element: its registers are multiplied by 0 (every other row's by 1, exact) and it takes
        // f = 1/pivot, which makes fma(f, prow[c], 0) = prow[c] / pivot exactly the value the select form stored
#pragma unroll
        for (int rr = 0; rr < RPT; ++rr) {
            const bool is_p = tid + NT * rr == p;
            const double keep = is_p ? 0.0 : 1.0;
            const double f = is_p ? inv : -(r[rr][j] * inv);
#pragma unroll
            for (int c = 0; c < NBW; ++c) {
                if (c == j) r[rr][c] = f;
                else r[rr][c] = fma(f, prow[c], r[rr][c] * keep);
            }
        }
        BL_STAMP(3)
        }  // p >= 0
        }  // j < nbw
    }
    if (dead) return;
    // ---- bookkeeping of the pivots, V_s = T_s[:, P_s] - I[:, P_s]
    lds_barrier();
    if (tid < a.nbw) {
        const long long p = s_pm[tid];
        a.used[p] = 1;
        a.perm[a.k0 + a.j0 + tid] = p;
        a.Pm[a.j0 + tid] = p;
    }
#pragma unroll
    for (int rr = 0; rr < RPT; ++rr) {
        const int64_t i = tid + NT * rr;
        if (i >= a.m) continue;
        double2 *vrow = reinterpret_cast<double2 *>(a.Vs + i * 16);
#pragma unroll
        for (int c = 0; c < NBW; c += 2) {
            double v0 = r[rr][c], v1 = r[rr][c + 1];
            if (c < a.nbw && s_pm[c] == i) v0 -= 1.0;
            if (c + 1 < a.nbw && s_pm[c + 1] == i) v1 -= 1.0;
            if (c + 1 < a.nbw) vrow[c >> 1] = make_double2(v0, v1);
            else if (c < a.nbw) a.Vs[i * 16 + c] = v0;
        }
    }
    BL_STAMP(4)
}

// ---- M <- M + V_s M[P_s, :] for M = [C[:, j0+nbw .. nbc) | V[:, 0 .. nacc)], out of place; the new
// columns V[:, nacc .. nacc+nbw) = V_s.  One thread per (row, 4 columns).
__device__ __forceinline__ void bl_apply_body(BlArgs a, unsigned bx) {
    __shared__ double s_mp[16][2 * BL_NB];
    if (a.st->status != ST_RUNNING) return;
    const double *Cin = a.sel ? a.C1 : a.C0, *Vin = a.sel ? a.V1 : a.V0;
    double *Cout = a.sel ? a.C0 : a.C1, *Vout = a.sel ? a.V0 : a.V1;
    const int tid = threadIdx.x;
    // rows P_s of M: columns 0..63 = C, 64..127 = V.  Rows nbw..15 of the scratch are ZEROED: they are
    // multiplied by zero coefficients below, and 0 * (whatever a previous kernel left in LDS, NaN included)
    // is not 0
    for (int e = tid; e < 16 * 2 * BL_NB; e += 256) {
        const int k = e / (2 * BL_NB), c = e % (2 * BL_NB);
        double v = 0.0;
        if (k < a.nbw) {
            const long long p = a.Pm[a.j0 + k];
            v = c < BL_NB ? Cin[p * BL_NB + c] : Vin[p * BL_NB + (c - BL_NB)];
        }
        s_mp[k][c] = v;
    }
    __syncthreads();
    const int c_lo = a.j0 + a.nbw;  // C columns still to be eliminated
    const int64_t rows_per_block = 256 / 32;
    const int64_t i = (int64_t)bx * rows_per_block + tid / 32;
    const int cg = (tid % 32) * 4;  // 4 columns of the 128
    if (i >= a.m) return;
    double vs[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) vs[k] = k < a.nbw ? a.Vs[i * 16 + k] : 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = cg + u;
        if (c < BL_NB) {
            if (c >= c_lo && c < a.nbc) {
                double v = Cin[i * BL_NB + c];
#pragma unroll
                for (int k = 0; k < 16; ++k) v = fma(vs[k], s_mp[k][c], v);
                Cout[i * BL_NB + c] = v;
            }
        } else {
            const int cv = c - BL_NB;
            if (cv < a.nacc) {
                double v = Vin[i * BL_NB + cv];
#pragma unroll
                for (int k = 0; k < 16; ++k) v = fma(vs[k], s_mp[k][c], v);
                Vout[i * BL_NB + cv] = v;
            } else if (cv < a.nacc + a.nbw) {
                Vout[i * BL_NB + cv] = vs[cv - a.nacc];
            }
        }
    }
}
__global__ __launch_bounds__(256) void k_bl_apply(BlArgs a) { bl_apply_body(a, blockIdx.x); }

// ---- Wp = W[Pm, :]
__device__ __forceinline__ void bl_gather_body(BlArgs a, unsigned bx) {
    const DevState *st = a.st;
    if (st->status != ST_RUNNING) return;
    const double *W = st->cur ? a.W1 : a.W0;
    const int k = bx;
    if (k >= a.nbc) return;
    const double2 *src = reinterpret_cast<const double2 *>(W + a.Pm[k] * a.ld);
    double2 *dst = reinterpret_cast<double2 *>(a.Wp + (int64_t)k * a.ld);
    for (int64_t t = threadIdx.x; t < (a.ld >> 1); t += 256) dst[t] = src[t];
}
__global__ __launch_bounds__(256) void k_bl_gather(BlArgs a) { bl_gather_body(a, blockIdx.x); }
// ---- G2: W[i, :] += V[i, 0..nbc) . Wp      block = 64 rows x 128 columns, thread = 4 rows x 8 columns
__device__ __forceinline__ void bl_gemm2_body(BlArgs a, unsigned bx, unsigned by) {
    __shared__ double sV[64][BL_NB + 1];
    __shared__ double sW[16][128];
    const DevState *st = a.st;
    if (st->status != ST_RUNNING) return;
    double *W = st->cur ? a.W1 : a.W0;
    const double *V = a.sel ? a.V1 : a.V0;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t i0 = (int64_t)by * 64, c0 = (int64_t)bx * 128;
    for (int e = tid; e < 64 * BL_NB; e += 256) {
        const int rr = e / BL_NB, k = e % BL_NB;
        const int64_t i = i0 + rr;
        sV[rr][k] = (i < a.m && k < a.nbc) ? V[i * BL_NB + k] : 0.0;
    }
    double acc[4][8];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[r][c] = 0.0;
    for (int k0 = 0; k0 < a.nbc; k0 += 16) {
        __syncthreads();
        for (int e = tid; e < 16 * 128; e += 256) {
            const int k = e / 128, c = e % 128;
            sW[k][c] = (k0 + k < a.nbc && c0 + c < a.ld) ? a.Wp[(int64_t)(k0 + k) * a.ld + c0 + c] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            double av[4], bv[8];
#pragma unroll
            for (int r = 0; r < 4; ++r) av[r] = sV[ty * 4 + r][k0 + kk];
#pragma unroll
            for (int c = 0; c < 8; ++c) bv[c] = sW[kk][tx * 8 + c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[r][c] = fma(av[r], bv[c], acc[r][c]);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t i = i0 + ty * 4 + r;
        if (i >= a.m) continue;
#pragma unroll
        for (int c = 0; c < 8; c += 2) {
            const int64_t col = c0 + tx * 8 + c;
            if (col >= a.ld) continue;
            double2 *w = reinterpret_cast<double2 *>(W + i * a.ld + col);
            double2 v = *w;
            v.x += acc[r][c];
            v.y += acc[r][c + 1];
            *w = v;
        }
    }
}
__global__ __launch_bounds__(256) void k_bl_gemm2(BlArgs a) { bl_gemm2_body(a, blockIdx.x, blockIdx.y); }

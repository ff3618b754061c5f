// ellp_bpost.inc — ellp_batch_postsolve: the postsolve of ellp_post.inc for many small LPs, one workgroup per LP.
// DESIGN.md §3.9b.
//
// k_post_batch does for its item, without a host decision in between, what post_compute does in about 2 ceil(m / 16) + 12
// launches and three synchronisations: the basis into LDS, its LU (small_lu: the numbers of ellp_lu_rows_factor, stored by
// columns), y = B^-T c_B by the operations of k_lu_solve mode 1, the singleton columns, the compensated pass over the basic
// columns (rho, the denominators, omega), the refinement loop with the host's stop rule, the pass over the nonbasic columns
// (d) and the fold of r.  k_post_report_batch then runs post_report once per item.  Two launches per chunk, whatever the
// item count.
//
// Every output is, bit for bit, what ellp_postsolve returns for the item alone: the build has -ffp-contract=off, so equal
// operations in equal order give equal bits, and the orders are the ones ellp_post.inc fixes by its launch geometry —
//   y    U^T: x_i = (b_i - acc_i) / U_ii, then acc_k = acc_k + U[i][k] x_i for the later k (thread k keeps acc_k);  L^T:
//        descending steps k, s_i = s_i - L[k][i] x_k for the earlier i, skipped where x_k == 0;  the transpositions in reverse;
//   d    one row tile (m <= 128 < POST_TR): lane l owns rows 2l and 2l + 1, two post_dot2 (the six of the tile's other
//        row pairs add +0 to sums that are never -0, and are left out), the 6-step butterfly 32 .. 1, k_post_dfold's merge
//        from (0, 0), d_v = t + (e - c) from TwoSum(c_v, -s), den = |c_v| + ab;
//   r    blocks of 64 columns, wave w takes the block's columns w, w + 4, ..., the four waves merged in wave order, then
//        from s = b_i the blocks merged as (-s_k, -c_k) in block order, the basic blocks first; r_i = s + c;
//   omega  the NaN-winning maximum of post_max: the value does not depend on the order.
// The workgroup always has four waves, so the four-wave order of r needs no emulation.
//
// The columns are read from the gathered, padded copies A_B / A_N in the chunk's slab (ld a multiple of 16: the double2
// loads are aligned), which the host stages as ellp_batch.inc stages them (batch_stage_basis).  The driver (budget, chunks,
// device, the pinned staging buffer, the slab) and the buffer pool are ellp_batch.inc's.  An item the kernel does not take
// (m > 128, |N| > 65,536) goes through ellp_postsolve inside the call.
//
// Included at the end of ellp_engine.hip, after ellp_batch.inc and ellp_post.inc.

namespace {

constexpr int BPOST_NT = 256;
constexpr int64_t BPOST_MAX_NN = 65536;  // post_cpb is 64 up to here: the block order of r is the single call's
constexpr int BPOST_ROWS = 128;          // the rows a wave's lanes own (2 each)

struct PostBatchArgs {
    const double *A_B, *A_N, *c_N;
    double *y, *d, *r, *rho, *omega;
    int32_t *steps;
    int *fail;
    int64_t ld;
    PostReportArgs rep;  // the item as the report sees it (m, n, n_c, nN, c_B, c_tail, x, b, the index sets)
};

// bytes of dynamic LDS k_post_batch needs (0: does not fit); the cap is small_lds_bytes'.  extra: vectors of m doubles a
// kernel built on it keeps besides (k_start_batch, ellp_bstart.inc)
inline size_t bpost_lds_bytes(int64_t m, int extra = 0) {
    if (m > SMALL_MAX_M || m < 1) return 0;
    size_t b = sizeof(double) * (size_t)(m * m)             // LU
               + sizeof(double) * (size_t)(extra * m)
               + sizeof(double) * BPOST_ROWS                // y, zero beyond m
               + sizeof(double) * (size_t)(5 * m)           // c_B, rho, den, the vector of a solve, singleton values
               + sizeof(double) * 2 * BPOST_ROWS * 2        // r: the two basic blocks
               + sizeof(double) * 4 * BPOST_ROWS * 2        // r: the four waves of a block
               + sizeof(int32_t) * (size_t)(4 * m);         // singleton rows, swap list a, swap list b, position -> row
    b = (b + 15) / 16 * 16;
    return b <= 150 * 1024 ? b : 0;
}

// v = B^-T v with the operations of k_lu_solve mode 1 on small_lu's factors (LU[k * m + r] is its M[r * m + k]).  Thread t
// keeps entry t and its accumulator in registers; every step broadcasts one entry.
__device__ __forceinline__ void bpost_btran(const double *LU, int m, double *v, const int32_t *pa, const int32_t *pb, int plen,
                                            double *slot2, int tid) {
    const double *col = LU + (tid < m ? tid : 0) * m;
    const double diag = col[tid < m ? tid : 0];
    double mine = tid < m ? v[tid] : 0.0, acc = 0.0;
    int stp = 0;
    for (int i = 0; i < m; ++i) {
        if (tid == i) {
            double xi = mine - acc;
            xi = xi / diag;
            mine = xi;
        }
        const double xi = small_bcast<BPOST_NT>(mine, i, slot2, stp++, tid);
        if (tid > i && tid < m) acc = acc + col[i] * xi;
    }
    for (int k = m - 1; k > 0; --k) {
        const double xk = small_bcast<BPOST_NT>(mine, k, slot2, stp++, tid);
        if (xk != 0.0 && tid < k) mine = mine - col[k] * xk;
    }
    if (tid < m) v[tid] = mine;
    __syncthreads();
    if (tid == 0)
        for (int k = plen - 1; k >= 0; --k) {
            const double t = v[pa[k]];
            v[pa[k]] = v[pb[k]];
            v[pb[k]] = t;
        }
    __syncthreads();
}

// k_post_pass + k_post_dfold over the stored columns C (one row tile), and the block sums of r: BASIC keeps them per block
// in rbas (the last pass over A_B counts), else they are merged into the fold (fs, fc) of thread i = row i at once, and
// kept per block in rkeep (global memory, as rbas is laid out) where that is given
template <bool BASIC>
__device__ __forceinline__ void bpost_pass(const double *C, const int64_t *index, const double *cpos, const double *x, double *d, int m,
                                           int64_t ld, int64_t ncols, const double *ysh, double *rho, double *den, double *rbas,
                                           double *rsh, double *rkeep, double &fs, double &fc, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    const bool ok0 = 2 * lane < m, ok1 = 2 * lane + 1 < m;
    const double yv0 = ysh[2 * lane], yv1 = ysh[2 * lane + 1];
    const int64_t nblocks = (ncols + 63) / 64;
    for (int64_t blk = 0; blk < nblocks; ++blk) {
        double rs0 = 0.0, rc0 = 0.0, rs1 = 0.0, rc1 = 0.0;
        const int64_t c0 = blk * 64;
        const int64_t c1 = (c0 + 64 < ncols) ? c0 + 64 : ncols;
        for (int64_t j = c0 + wave; j < c1; j += 4) {
            const int64_t var = index[j];
            const double xv = x[var];
            double2 v = ok0 ? *reinterpret_cast<const double2 *>(C + j * ld + 2 * lane) : make_double2(0.0, 0.0);
            if (!ok1) v.y = 0.0;  // the padding row of an odd m
            double s = 0.0, c = 0.0, ab = 0.0;
            post_dot2(s, c, v.x, yv0);
            post_dot2(s, c, v.y, yv1);
            ab += fabs(v.x) * fabs(yv0);
            ab += fabs(v.y) * fabs(yv1);
            post_dot2(rs0, rc0, xv, v.x);
            post_dot2(rs1, rc1, xv, v.y);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double s2 = __shfl_xor(s, off), c2 = __shfl_xor(c, off), ab2 = __shfl_xor(ab, off);
                post_merge(s, c, s2, c2);
                ab = ab + ab2;
            }
            if (lane == 0) {  // k_post_dfold over the one tile
                double fs2 = 0.0, fc2 = 0.0, fab = 0.0;
                post_merge(fs2, fc2, s, c);
                fab += ab;
                const double cv = cpos[j];
                double t, e;
                post_two_sum(cv, -fs2, t, e);
                const double dv = t + (e - fc2);
                d[var] = dv;
                if (BASIC) {
                    rho[j] = dv;
                    den[j] = fabs(cv) + fab;
                }
            }
        }
        double *mine = rsh + (size_t)wave * BPOST_ROWS * 2;
        mine[4 * lane] = rs0;
        mine[4 * lane + 1] = rc0;
        mine[4 * lane + 2] = rs1;
        mine[4 * lane + 3] = rc1;
        __syncthreads();
        if (tid < m) {
            double s = rsh[2 * tid], c = rsh[2 * tid + 1];
#pragma unroll
            for (int w = 1; w < 4; ++w) post_merge(s, c, rsh[(w * BPOST_ROWS + tid) * 2], rsh[(w * BPOST_ROWS + tid) * 2 + 1]);
            if (BASIC) {
                rbas[(blk * BPOST_ROWS + tid) * 2] = s;
                rbas[(blk * BPOST_ROWS + tid) * 2 + 1] = c;
            } else {
                post_merge(fs, fc, -s, -c);
                if (rkeep) {
                    rkeep[(blk * BPOST_ROWS + tid) * 2] = s;
                    rkeep[(blk * BPOST_ROWS + tid) * 2 + 1] = c;
                }
            }
        }
        __syncthreads();
    }
}

// the carve of the dynamic LDS: bpost_lds_bytes(m, extra), the extra vectors between rsh and the integers
struct BpostSh {
    double *LU, *ysh, *cB, *rho, *den, *sv, *sval, *rbas, *rsh, *extra;
    int32_t *srow, *pa, *pb, *lop;
};
__device__ __forceinline__ BpostSh bpost_carve(unsigned char *smem, int m, int extra) {
    BpostSh s;
    s.LU = reinterpret_cast<double *>(smem);
    s.ysh = s.LU + m * m;
    s.cB = s.ysh + BPOST_ROWS;
    s.rho = s.cB + m;
    s.den = s.rho + m;
    s.sv = s.den + m;
    s.sval = s.sv + m;
    s.rbas = s.sval + m;
    s.rsh = s.rbas + 2 * BPOST_ROWS * 2;
    s.extra = s.rsh + 4 * BPOST_ROWS * 2;
    s.srow = reinterpret_cast<int32_t *>(s.extra + extra * m);
    s.pa = s.srow + m;
    s.pb = s.pa + m;
    s.lop = s.pb + m;
    return s;
}

// Steps 1 and 2 of an item, shared by k_post_batch and k_start_batch: the basis into LDS, its singleton columns, its LU,
// y = B^-T c_B and the refinement loop of y (post_solve_y's).  false: a zero on U's diagonal, nothing was written.  On
// return sh.ysh holds y; sh.rho, sh.den, sh.rbas and d on the basis are those of the last pass over A_B (with the x given);
// *plen the length of the swap list; omega and steps of y
__device__ __forceinline__ bool bpost_solve_y(const BpostSh &sh, const double *A_B, const PostReportArgs &rep, const double *x, double *d,
                                              int m, int64_t ld, int *plen, double *s_bc, double &omega, int32_t &steps, int tid) {
    __shared__ double s_wv[8], s_wd[8];
    __shared__ int s_wi[8], s_wp[8];
    __shared__ double s_omega;
    const int lane = tid & 63;
    double *LU = sh.LU, *ysh = sh.ysh, *cB = sh.cB, *rho = sh.rho, *den = sh.den, *sv = sh.sv, *sval = sh.sval;
    int32_t *srow = sh.srow;
    // ---- A_B into LDS by columns (ld = m), c_B, y = 0
    for (int e = tid; e < m * m; e += BPOST_NT) {
        const int j = e / m, i = e - j * m;
        LU[e] = A_B[j * ld + i];
    }
    for (int i = tid; i < BPOST_ROWS; i += BPOST_NT) ysh[i] = 0.0;
    if (tid < m) cB[tid] = rep.c_B[tid];
    __syncthreads();
    // ---- the columns with a single nonzero (k_post_singletons): thread j scans column j, from row j on (LDS banks)
    if (tid < m) {
        int cnt = 0, row = -1, i = tid;
        double val = 0.0;
        for (int t = 0; t < m; ++t) {
            const double v = LU[tid * m + i];
            if (v != 0.0) {  // a NaN counts
                cnt += 1;
                row = i;
                val = v;
            }
            if (++i == m) i = 0;
        }
        srow[tid] = cnt == 1 ? row : -1;
        sval[tid] = cnt == 1 ? val : 0.0;
    }
    __syncthreads();
    small_lu<BPOST_NT>(LU, m, sh.pa, sh.pb, plen, sh.lop, s_wv, s_wd, s_wi, s_wp, tid);
    // a zero on U's diagonal: the item's flag (set by the caller), and nothing else of the item is written
    if (__syncthreads_or(tid < m && LU[tid * m + tid] == 0.0)) return false;
    const int pl = *plen;
    // ---- y = B^-T c_B, the singletons imposed
    if (tid < m) sv[tid] = cB[tid];
    __syncthreads();
    bpost_btran(LU, m, sv, sh.pa, sh.pb, pl, s_bc, tid);
    if (tid < m) ysh[tid] = sv[tid];
    __syncthreads();
    if (tid < m && srow[tid] >= 0) ysh[srow[tid]] = cB[tid] / sval[tid];
    __syncthreads();
    // ---- the pass over the basic columns and the refinement loop, post_solve_y's
    const double two_u = 2.220446049250313e-16;  // 2 u, u = 2^-53
    double last = 0.0, fs = 0.0, fc = 0.0;
    steps = 0;
    for (;;) {
        bpost_pass<true>(A_B, rep.B_index, cB, x, d, m, ld, m, ysh, rho, den, sh.rbas, sh.rsh, nullptr, fs, fc, tid);
        if (tid < 64) {  // k_post_omega
            PostMax mine{0.0, LLONG_MAX_POST};
            for (int i = lane; i < m; i += 64) mine = post_max(mine, PostMax{post_ratio(rho[i], den[i]), (long long)i});
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                PostMax o;
                o.v = __shfl_xor(mine.v, off);
                o.i = __shfl_xor(mine.i, off);
                mine = post_max(mine, o);
            }
            if (lane == 0) s_omega = mine.v;
        }
        __syncthreads();
        omega = s_omega;
        if (!(omega > two_u) || steps >= 4 || (steps > 0 && !(omega <= 0.5 * last))) break;
        if (tid < m) sv[tid] = rho[tid];
        __syncthreads();
        bpost_btran(LU, m, sv, sh.pa, sh.pb, pl, s_bc, tid);
        if (tid < m) ysh[tid] = ysh[tid] + sv[tid];
        __syncthreads();
        if (tid < m && srow[tid] >= 0) ysh[srow[tid]] = cB[tid] / sval[tid];
        __syncthreads();
        last = omega;
        steps += 1;
    }
    return true;
}

// The whole item of k_post_batch on the carve sh: false, with the item's flag set and nothing else written, on a zero on
// U's diagonal.  On return the factors are in sh.LU, the swap list in (sh.pa, sh.pb, *s_plen) and the singleton columns in
// (sh.srow, sh.sval), which k_brange_front (ellp_brange.inc) keeps for the ranging
__device__ __forceinline__ bool bpost_item(const PostBatchArgs &a, const BpostSh &sh, int *s_plen, double *s_bc, int tid) {
    const int m = (int)a.rep.m;
    const int64_t ld = a.ld, nN = a.rep.nN;
    double omega = 0.0, fs = 0.0, fc = 0.0;
    int32_t steps = 0;
    if (!bpost_solve_y(sh, a.A_B, a.rep, a.rep.x, a.d, m, ld, s_plen, s_bc, omega, steps, tid)) {
        if (tid == 0) *a.fail = 1;
        return false;
    }
    // ---- r from b, the basic blocks first, then the nonbasic ones as their pass delivers them; d on the way
    if (tid < m) {
        fs = a.rep.b[tid];
        fc = 0.0;
        const int nbb = (m + 63) / 64;
        for (int k = 0; k < nbb; ++k) post_merge(fs, fc, -sh.rbas[(k * BPOST_ROWS + tid) * 2], -sh.rbas[(k * BPOST_ROWS + tid) * 2 + 1]);
    }
    bpost_pass<false>(a.A_N, a.rep.N_index, a.c_N, a.rep.x, a.d, m, ld, nN, sh.ysh, sh.rho, sh.den, sh.rbas, sh.rsh, nullptr, fs, fc, tid);
    for (int64_t v = a.rep.n + tid; v < a.rep.n_c; v += BPOST_NT) a.d[v] = a.rep.c_tail[v - a.rep.n];
    if (tid < m) {
        a.r[tid] = fs + fc;
        a.y[tid] = sh.ysh[tid];
        a.rho[tid] = sh.rho[tid];
    }
    if (tid == 0) {
        *a.omega = omega;
        *a.steps = steps;
    }
    return true;
}

__global__ __launch_bounds__(BPOST_NT) void k_post_batch(const PostBatchArgs *args) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ double s_bc[2];
    __shared__ int s_plen;
    const PostBatchArgs a = args[blockIdx.x];
    (void)bpost_item(a, bpost_carve(smem, (int)a.rep.m, 0), &s_plen, s_bc, threadIdx.x);
}

__global__ __launch_bounds__(1024) void k_post_report_batch(const PostBatchArgs *args) {
    const PostBatchArgs &a = args[blockIdx.x];
    if (*a.fail) return;  // uniform over the workgroup
    post_report(a.rep, *a.steps);
}

// one item on the batched kernel: its share of the slab (byte offsets in its chunk's slab)
struct BpostPlan {
    int64_t item;
    int64_t ld, nNa, ntail;
    size_t lds;
    size_t o_y, o_d, o_r, o_kkt, o_fail;                                                            // read back
    size_t o_AB, o_AN, o_cB, o_cN, o_ct, o_x, o_b, o_lb, o_ub, o_kind, o_B, o_N, o_Nb;              // inputs
    size_t o_rho, o_omega, o_steps;                                                                 // device only
    size_t bytes;
};
struct BpostLayout {
    size_t out_bytes, o_args, stage_bytes, total;
};
constexpr size_t BPOST_CHUNK_SLACK = 16;  // the rounding of the argument array

BpostLayout bpost_layout(const ellp_batch_item *items, BpostPlan *plan, size_t R) {
    BpostLayout L{};
    SlabCursor cur;
    for (size_t k = 0; k < R; ++k) {
        BpostPlan &p = plan[k];
        const ellp_batch_item &it = items[p.item];
        cur.bytes = &p.bytes;
        p.bytes = sizeof(PostBatchArgs);
        p.o_y = cur.take(sizeof(double) * (size_t)it.m);
        p.o_d = cur.take(sizeof(double) * (size_t)it.n_c);
        p.o_r = cur.take(sizeof(double) * (size_t)it.m);
        p.o_kkt = cur.take(sizeof(ellp_kkt));
        p.o_fail = cur.take(sizeof(int));
    }
    L.out_bytes = cur.off;
    for (size_t k = 0; k < R; ++k) {
        BpostPlan &p = plan[k];
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
    }
    cur.bytes = nullptr;
    L.o_args = cur.take(sizeof(PostBatchArgs) * R);
    L.stage_bytes = cur.off;
    for (size_t k = 0; k < R; ++k) {
        BpostPlan &p = plan[k];
        cur.bytes = &p.bytes;
        p.o_rho = cur.take(sizeof(double) * (size_t)items[p.item].m);
        p.o_omega = cur.take(sizeof(double));
        p.o_steps = cur.take(sizeof(int32_t));
    }
    L.total = cur.off;
    return L;
}

// the calling thread's last ellp_batch_postsolve that passed the checks of the call (ellp_batch_postsolve_info)
thread_local uint64_t g_batch_post_info[4] = {0, 0, 0, 0};

// The item as the report sees it, from its plan's offsets in the slab dv (BpostPlan and BstartPlan name them alike); c_tail
// is the caller's.  ra.steps stays 0: the batch reads the item's steps on the device
template <class Plan>
void bpost_report_args(PostReportArgs &ra, unsigned char *dv, const Plan &p, const ellp_batch_item &it) {
    ra.r = slab_at<double>(dv, p.o_r);
    ra.d = slab_at<double>(dv, p.o_d);
    ra.rho = slab_at<double>(dv, p.o_rho);
    ra.y = slab_at<double>(dv, p.o_y);
    ra.omega = slab_at<double>(dv, p.o_omega);
    ra.b = slab_at<double>(dv, p.o_b);
    ra.x = slab_at<double>(dv, p.o_x);
    ra.lb = slab_at<double>(dv, p.o_lb);
    ra.ub = slab_at<double>(dv, p.o_ub);
    ra.c_B = slab_at<double>(dv, p.o_cB);
    ra.c_N = slab_at<double>(dv, p.o_cN);
    ra.kind = slab_at<uint8_t>(dv, p.o_kind);
    ra.Nb = slab_at<uint8_t>(dv, p.o_Nb);
    ra.B_index = slab_at<int64_t>(dv, p.o_B);
    ra.N_index = slab_at<int64_t>(dv, p.o_N);
    ra.m = it.m; ra.n = it.n; ra.n_c = it.n_c; ra.nN = it.n_N;
    ra.out = slab_at<ellp_kkt>(dv, p.o_kkt);
}

// One item into the staging buffer h, as its plan lays it out, and its arguments in the slab dv.  Shared by
// ellp_batch_postsolve and ellp_batch_ranging (ellp_brange.inc), whose plan extends this one
PostBatchArgs bpost_stage_item(unsigned char *h, unsigned char *dv, const BpostPlan &p, const ellp_batch_item &it) {
    const int64_t m = it.m, nN = it.n_N;
    memset(h + p.o_fail, 0, sizeof(int));
    batch_stage_basis(h, it, p.ld, p.o_AB, p.o_AN, p.o_cB, p.o_cN);
    if (p.ntail > 0) memcpy(h + p.o_ct, it.c + it.n, sizeof(double) * (size_t)p.ntail);
    memcpy(h + p.o_x, it.x, sizeof(double) * (size_t)it.n_c);
    memcpy(h + p.o_b, it.b, sizeof(double) * (size_t)m);
    memcpy(h + p.o_lb, it.lb, sizeof(double) * (size_t)it.n_c);
    memcpy(h + p.o_ub, it.ub, sizeof(double) * (size_t)it.n_c);
    memcpy(h + p.o_kind, it.bound_kind, (size_t)it.n_c);
    memcpy(h + p.o_B, it.B_index, sizeof(int64_t) * (size_t)m);
    if (nN > 0) {
        memcpy(h + p.o_N, it.N_index, sizeof(int64_t) * (size_t)nN);
        memcpy(h + p.o_Nb, it.N_bound, (size_t)nN);
    }
    PostBatchArgs a{};
    a.A_B = slab_at<double>(dv, p.o_AB);
    a.A_N = slab_at<double>(dv, p.o_AN);
    a.c_N = slab_at<double>(dv, p.o_cN);
    a.y = slab_at<double>(dv, p.o_y);
    a.d = slab_at<double>(dv, p.o_d);
    a.r = slab_at<double>(dv, p.o_r);
    a.rho = slab_at<double>(dv, p.o_rho);
    a.omega = slab_at<double>(dv, p.o_omega);
    a.steps = slab_at<int32_t>(dv, p.o_steps);
    a.fail = slab_at<int>(dv, p.o_fail);
    a.ld = p.ld;
    bpost_report_args(a.rep, dv, p, it);
    a.rep.c_tail = slab_at<double>(dv, p.o_ct);
    return a;
}

// One chunk: staging, one upload, the two launches, one read-back, the per-item results
ellp_status bpost_run_chunk(ellp_batch_item *items, const ellp_batch_post_out *outs, BpostPlan *plan, size_t R, BatchCleanup &cl,
                            ellp_status *status_out, char *errbuf, size_t errlen) {
    const BpostLayout L = bpost_layout(items, plan, R);
    hipStream_t stream = cl.hs.stream;
    unsigned char *h = static_cast<unsigned char *>(cl.stage.p);
    unsigned char *dv = static_cast<unsigned char *>(cl.slab.p);
    PostBatchArgs *h_args = slab_at<PostBatchArgs>(h, L.o_args);
    size_t lds = 0;
    for (size_t k = 0; k < R; ++k) {
        const BpostPlan &p = plan[k];
        h_args[k] = bpost_stage_item(h, dv, p, items[p.item]);
        if (p.lds > lds) lds = p.lds;
    }
    // the outputs' region goes up too (the fail flags are its only part that is read before it is written)
    HIPCHK(hipMemcpyAsync(dv, h, L.stage_bytes, hipMemcpyHostToDevice, stream));
    const PostBatchArgs *d_args = slab_at<const PostBatchArgs>(dv, L.o_args);
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_post_batch), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    // ELLP_POST_PROFILE=1 (tools/batch_postsolve_time.py): one line per chunk in the single call's format, with m = the
    // chunk's items, lu_ms = k_post_batch (everything up to r) and rest_ms = the reports
    PostProf prof(stream);
    prof.name = "batch_postsolve_profile";
    prof.begin(PostProf::LU);
    hipLaunchKernelGGL(k_post_batch, dim3((unsigned)R), dim3(BPOST_NT), lds, stream, d_args);
    prof.end();
    prof.begin(PostProf::REST);
    hipLaunchKernelGGL(k_post_report_batch, dim3((unsigned)R), dim3(1024), 0, stream, d_args);
    prof.end();
    g_batch_post_info[0] += 2;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h, dv, L.out_bytes, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    prof.report((int64_t)R, 0, 0);
    for (size_t k = 0; k < R; ++k) {
        const BpostPlan &p = plan[k];
        const ellp_batch_item &it = items[p.item];
        const ellp_batch_post_out &o = outs[p.item];
        if (batch_item_singular(h, p.o_fail, items[p.item], &status_out[p.item])) continue;
        if (o.y) memcpy(o.y, h + p.o_y, sizeof(double) * (size_t)it.m);
        if (o.d) memcpy(o.d, h + p.o_d, sizeof(double) * (size_t)it.n_c);
        if (o.r) memcpy(o.r, h + p.o_r, sizeof(double) * (size_t)it.m);
        if (o.kkt) memcpy(o.kkt, h + p.o_kkt, sizeof(ellp_kkt));
        status_out[p.item] = ELLP_OPTIMAL;
    }
    return ELLP_OPTIMAL;
}

}  // namespace

extern "C" ellp_status ellp_batch_postsolve(int64_t count, ellp_batch_item *items, const ellp_opts *opts_in,
                                            const ellp_batch_post_out *outs, ellp_status *status_out, char *errbuf, size_t errlen) {
    if (errbuf && errlen) errbuf[0] = 0;
    if (count < 0 || !items || !outs || !status_out) {
        set_err(errbuf, errlen, "count < 0, or items / outs / status_out NULL");
        return ELLP_ERR_ARG;
    }
    // ---- per item: the single call's checks, then who runs it (all before any HIP call)
    std::vector<BpostPlan> plan;
    std::vector<int64_t> single;
    for (int64_t i = 0; i < count; ++i) {
        ellp_batch_item &it = items[i];
        const ellp_batch_post_out &o = outs[i];
        it.err[0] = 0;
        if (!o.y && !o.d && !o.r && !o.kkt) {
            set_err(it.err, sizeof(it.err), "postsolve: none of y, d, r, kkt is wanted");
            status_out[i] = ELLP_ERR_ARG;
            continue;
        }
        const ellp_status s = post_host_checks("postsolve", it.m, it.n, it.n_c, it.A, it.c, it.b, it.bound_kind, it.lb, it.ub, it.x,
                                               it.B_index, it.n_B, it.N_index, it.N_bound, it.n_N, it.err, sizeof(it.err));
        status_out[i] = s;
        if (s != ELLP_OPTIMAL) continue;
        const size_t lds = bpost_lds_bytes(it.m);
        if (lds == 0 || it.n_N > BPOST_MAX_NN) {
            single.push_back(i);
            continue;
        }
        BpostPlan p{};
        p.item = i;
        p.ld = round_up(it.m, 16);
        p.nNa = it.n_N > 0 ? it.n_N : 1;
        p.ntail = it.n_c - it.n;
        p.lds = lds;
        plan.push_back(p);
    }
    g_batch_post_info[0] = 0;
    g_batch_post_info[1] = plan.size();
    g_batch_post_info[2] = single.size();
    g_batch_post_info[3] = 0;
    if (plan.empty() && single.empty()) return ELLP_OPTIMAL;

    if (!plan.empty()) {
        const ellp_status rc = batch_drive(
            plan, single, BPOST_CHUNK_SLACK, opts_in, status_out, &g_batch_post_info[3],
            [&](BpostPlan *pl, size_t R) { return bpost_layout(items, pl, R); },
            [&](BpostPlan *pl, size_t R, BatchCleanup &cl) { return bpost_run_chunk(items, outs, pl, R, cl, status_out, errbuf, errlen); },
            errbuf, errlen);
        if (rc != ELLP_OPTIMAL) return rc;
    }
    // ---- the items the kernel does not take: the single call, inside this one
    for (int64_t i : single) {
        ellp_batch_item &it = items[i];
        const ellp_batch_post_out &o = outs[i];
        status_out[i] = ellp_postsolve(it.m, it.n, it.n_c, it.A, it.c, it.b, it.bound_kind, it.lb, it.ub, it.x, it.B_index, it.n_B, it.N_index,
                                       it.N_bound, it.n_N, opts_in, o.y, o.d, o.r, o.kkt, it.err, sizeof(it.err));
    }
    return ELLP_OPTIMAL;
}

extern "C" void ellp_batch_postsolve_info(uint64_t *out4) {
    if (!out4) return;
    for (int k = 0; k < 4; ++k) out4[k] = g_batch_post_info[k];
}

// ellp_dualfu.inc — the dual iteration in two bandwidth passes (+ one small closing block) instead of three.
//
// In the dual loop the pivot row is fixed BEFORE the entering column is known (dual…:200-236 picks the
// leaving row first), so the eta update of an iteration does not have to wait for anything the FTRAN of the
// same iteration produces except the column alpha_q = B^-1 a_q itself — and row i of the update needs only
// alpha_i (its own dot product), alpha_r = rho . a_q (which every block can form itself from the pivot row it
// fetches anyway) and rho.  So FTRAN (dual…:294) and the eta update become ONE pass over B^-1:
//
//   k_price<.,1>   P   alpha_j = rho . a_j, ratios, per-block first argmin                      8 ld |N| bytes
//   k_dual_fu      FU  prologue: dual ratio argmin (dual…:279-289) and alpha_r; per row (held in registers):
//                      alpha_i = row . a_q, row' = row - (alpha_i/alpha_r) rho (row r: rho/alpha_r), x_B update
//                      (dual…:311); block 0: d_N update (dual…:296-300), block 1: y (dual…:302)  16 m ld bytes
//   closing work       the column / index / cost swap (dual…:322-333), the scalars, the next leaving row
//                      (dual…:200-236) from per-row-block records FU left, the tiny-pivot test.  It cannot be in FU:
//                      the swap overwrites A_N[:, q], which late-starting blocks of FU still read, and B_index[r] /
//                      DevState::cur change hands there ("a kernel never reads a state field one of its own blocks
//                      writes").  Engines without tiny-pivot maintenance (m > 512) fold it into the NEXT pricing
//                      launch's prologue (dual_price_prologue in ellp_engine.hip); the others, and every point where
//                      a complete state is needed (end of a batch, maintenance, read-back), use k_dual_close (L).
//
// against P + k_ftran2<1> (8 m ld) + k_update2<1> (16 m ld): one third of the traffic over B^-1 less and one
// dependent bandwidth kernel less.  Iterations on which the drift monitor looks at A_B alpha_q - a_q run in the
// three-launch form (all forms leave identical state).
// The arithmetic of every quantity is the three-launch path's; the FTRAN dot products are summed in another
// order (a block per row group instead of a wave per row).
//
// Included inside the anonymous namespace of ellp_engine.hip.

struct DualFuArgs {
    double *W0, *W1;
    const double *A_N;
    Xchg xc;
    const int64_t *N_index, *B_index;
    double *x, *d, *y, *dd;
    const double *lb, *ub;
    const uint8_t *kind;
    // per row block, for the closing block's choice of the next leaving row: the first of the block's rows whose
    // variable violates a bound after this iteration's update (-1: none), its delta and side
    int32_t *lrow;
    double *ldelta, *lside;
    DevState *st;
    int64_t m, ld, nN;
    int nblocks;
    double eps;
    unsigned long long seq;  // number of this fused iteration (>= 1): what it leaves to be closed is DevState::dp_seq = seq
    int maxviol;
    double guard_abs;  // > 0: a pivot with |alpha_r| < guard_abs is refused (ST_NEED_EXACT)             // ELLP_FLAG_DUAL_MAX_VIOLATION: a block's record is its row of largest violation
};

constexpr int DFU_BOOK = 2;  // block 0: reduced costs of the nonbasic variables, block 1: y

template <int NR>  // double2 per thread per row: ceil(ld / 512), 1 / 2 / 4 / 8
__global__ __launch_bounds__(256) void k_dual_fu(DualFuArgs a) {
    __shared__ double s_wk[4];
    __shared__ long long s_wp[4];
    __shared__ double s_dot[4][UPD_ROWS + 1];
    DevState *st = a.st;
    if (st->status != ST_RUNNING) return;
    const int64_t r = st->lr;
    if (r < 0) return;  // k_price<.,1> has reported Optimal
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nan_flag = st->nan_flag;
    const int cur = st->cur;
    const double delta = st->ldelta;
    const double *src = cur ? a.W1 : a.W0;
    double *dst = cur ? a.W0 : a.W1;
    const int64_t half = a.ld >> 1, m = a.m;
    const bool row_block = blockIdx.x >= DFU_BOOK;
    const int64_t row0 = ((int64_t)blockIdx.x - DFU_BOOK) * UPD_ROWS;

    // ---- loads that do not depend on the decision: the block argmins first, then the pivot row and the block's rows
    double bk = INFINITY;
    long long bp = -1;
    {
        double kv[4];
        double pv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int b = tid + 256 * u;
            const int bc = b < a.nblocks ? b : 0;
            kv[u] = a.xc.bk(bc);
            pv[u] = a.xc.bp(bc);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int b = tid + 256 * u;
            const long long p = b < a.nblocks ? (long long)pv[u] : -1;
            if (p >= 0 && (bp < 0 || kv[u] < bk || (kv[u] == bk && p < bp))) {
                bk = kv[u];
                bp = p;
            }
        }
    }
    const int64_t myrow = row0 + tid;
    const bool own = row_block && tid < UPD_ROWS && myrow < m;
    const int64_t bi0 = a.B_index[own ? myrow : 0];
    double2 pr[NR], wreg[UPD_ROWS][NR];
    {
        const double2 *rho2 = reinterpret_cast<const double2 *>(src + r * a.ld);
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            const int64_t t = tid + 256 * u;
            const double2 v = rho2[t < half ? t : 0];
            pr[u] = t < half ? v : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int k = 0; k < UPD_ROWS; ++k) {
            const int64_t i = row0 + k;
            const bool ok = row_block && i < m;
            const double2 *srow = reinterpret_cast<const double2 *>(src + (ok ? i : 0) * a.ld);
#pragma unroll
            for (int u = 0; u < NR; ++u) {
                const int64_t t = tid + 256 * u;
                const double2 wv = srow[t < half ? t : 0];
                wreg[k][u] = (ok && t < half) ? wv : make_double2(0.0, 0.0);
            }
        }
    }
    const double xi0 = a.x[bi0], lbi0 = a.lb[bi0], ubi0 = a.ub[bi0];
    const int k0 = a.kind[bi0];
    for (int b = tid + 4 * 256; b < a.nblocks; b += 256) {  // more than 1024 pricing blocks: the rest of the argmins
        const long long p = (long long)a.xc.bp(b);
        if (p < 0) continue;
        const double k = a.xc.bk(b);
        if (bp < 0 || k < bk || (k == bk && p < bp)) {
            bk = k;
            bp = p;
        }
    }
    // ---- dual ratio test: FIRST minimum (dual…:279), same reduction as k_ftran2<1>
    // lexicographic (ratio, position) minimum over the wave: DPP butterfly inside the rows of 16 lanes, the four rows
    // through readlane (the minimum of a set does not depend on the order it is formed in)
    {
        int bpi = (int)bp;  // positions are below 2^31
#define DFU_STEP(CTRL)                                                               \
        {                                                                            \
            const double ok = dpp_f64<CTRL>(bk);                                     \
            const int op = dpp_i32<CTRL>(bpi);                                       \
            if (op >= 0 && (bpi < 0 || ok < bk || (ok == bk && op < bpi))) {         \
                bk = ok;                                                             \
                bpi = op;                                                            \
            }                                                                        \
        }
        DFU_STEP(0xB1)
        DFU_STEP(0x4E)
        DFU_STEP(0x141)
        DFU_STEP(0x140)
#undef DFU_STEP
        double rk = readlane_f64(bk, 0);
        int rp = __builtin_amdgcn_readlane(bpi, 0);
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            const double ok = readlane_f64(bk, 16 * k);
            const int op = __builtin_amdgcn_readlane(bpi, 16 * k);
            if (op >= 0 && (rp < 0 || ok < rk || (ok == rk && op < rp))) {
                rk = ok;
                rp = op;
            }
        }
        bk = rk;
        bp = rp;
    }
    if (lane == 0) {
        s_wk[wave] = bk;
        s_wp[wave] = bp;
    }
    lds_barrier();
    bk = s_wk[0];
    bp = s_wp[0];
    for (int w = 1; w < 4; ++w)
        if (s_wp[w] >= 0 && (bp < 0 || s_wk[w] < bk || (s_wk[w] == bk && s_wp[w] < bp))) {
            bk = s_wk[w];
            bp = s_wp[w];
        }
    const long long q = bp;
    const double theta_d = (delta < 0.0) ? -bk : bk;  // dual…:286-289
    if (nan_flag) {
        if (blockIdx.x == 0 && tid == 0) st->status = ELLP_ERR_NAN;
        return;
    }
    if (q < 0) {
        if (blockIdx.x == 0 && tid == 0) {
            st->iters += 1;
            st->status = ELLP_INFEASIBLE;  // dual unbounded, dual…:281-284
        }
        return;
    }
    // ---- alpha_q = B^-1 a_q (dual…:294) for the pivot row and the block's rows, from the registers
    const double2 *col = reinterpret_cast<const double2 *>(a.A_N + q * a.ld);
    double2 cq[NR];
#pragma unroll
    for (int u = 0; u < NR; ++u) {
        const int64_t t = tid + 256 * u;
        const double2 cv = col[t < half ? t : 0];
        cq[u] = t < half ? cv : make_double2(0.0, 0.0);
    }
    {
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            a0 = fma(pr[u].x, cq[u].x, a0);
            a1 = fma(pr[u].y, cq[u].y, a1);
        }
        const double s = wave_sum(a0 + a1);
        if (lane == 0) s_dot[wave][UPD_ROWS] = s;
    }
#pragma unroll
    for (int k = 0; k < UPD_ROWS; ++k) {
        double a0 = 0.0, a1 = 0.0;
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            a0 = fma(wreg[k][u].x, cq[u].x, a0);
            a1 = fma(wreg[k][u].y, cq[u].y, a1);
        }
        const double s = wave_sum(a0 + a1);
        if (lane == 0) s_dot[wave][k] = s;
    }
    lds_barrier();
    // every block forms alpha_r from the same slices in the same order as the block that owns row r forms alpha_r
    // as one of ITS rows: the value is the same bit pattern everywhere
    const double alpha_r = ((s_dot[0][UPD_ROWS] + s_dot[1][UPD_ROWS]) + s_dot[2][UPD_ROWS]) + s_dot[3][UPD_ROWS];
    if (a.guard_abs > 0.0 && fabs(alpha_r) < a.guard_abs) {  // see ST_NEED_EXACT (ellp_engine.hip): every block returns before its first store
        if (blockIdx.x == 0 && tid == 0) st->status = ST_NEED_EXACT;
        return;
    }
    const double theta_p = delta / alpha_r;  // dual…:305-309

    if (row_block) {
        // ---- eta update of the block's rows: W' = E W with the pivot row r and the column alpha_q
#pragma unroll
        for (int k = 0; k < UPD_ROWS; ++k) {
            const int64_t i = row0 + k;
            if (i >= m) continue;
            const double al = ((s_dot[0][k] + s_dot[1][k]) + s_dot[2][k]) + s_dot[3][k];
            const double f = (i != r) ? -(al / alpha_r) : 0.0;
            double2 *drow = reinterpret_cast<double2 *>(dst + i * a.ld);
#pragma unroll
            for (int u = 0; u < NR; ++u) {
                const int64_t t = tid + 256 * u;
                if (t >= half) continue;
                double2 o;
                if (i == r) {
                    o = make_double2(pr[u].x / alpha_r, pr[u].y / alpha_r);
                } else {
                    o.x = fma(f, pr[u].x, wreg[k][u].x);
                    o.y = fma(f, pr[u].y, wreg[k][u].y);
                }
                store_row2<true>(drow + t, o);
            }
        }
        // alpha_q itself, the basic part of the point (dual…:311; position r: the leaving variable reaches its bound), and
        // whether the position's variable violates a bound afterwards — for position r that is the ENTERING variable
        // with the value the closing block gives it (dual…:313)
        if (wave == 0) {
            bool viol = false;
            double vdelta = 0.0;
            int vside = 0;
            if (own) {
                const int k = tid;
                const double al = ((s_dot[0][k] + s_dot[1][k]) + s_dot[2][k]) + s_dot[3][k];
                a.d[myrow] = al;
                const double xn = xi0 - theta_p * al;
                a.x[bi0] = xn;
                if (myrow == r) {
                    const int64_t jq = a.N_index[q];
                    viol = dual_violation_v(a.x[jq] + theta_p, a.kind[jq], a.lb[jq], a.ub[jq], a.eps, &vdelta, &vside);
                } else {
                    viol = dual_violation_v(xn, k0, lbi0, ubi0, a.eps, &vdelta, &vside);
                }
            }
            unsigned long long bal = __ballot(viol);
            if (a.maxviol && bal) {  // the block's rows sit on lanes 0..7: the largest |delta|, first of equals
                double ad = viol ? fabs(vdelta) : -1.0;
                if (ad != ad) ad = INFINITY;
                double mx = ad;
                mx = fmax(mx, __shfl_xor(mx, 1));
                mx = fmax(mx, __shfl_xor(mx, 2));
                mx = fmax(mx, __shfl_xor(mx, 4));
                bal = __ballot(viol && ad == mx) & 0xffull;
            }
            const int first = bal ? __ffsll((long long)bal) - 1 : -1;
            if (lane == (first < 0 ? 0 : first)) {
                const int64_t rb = (int64_t)blockIdx.x - DFU_BOOK;
                a.lrow[rb] = first < 0 ? -1 : (int32_t)(row0 + first);
                a.ldelta[rb] = vdelta;
                a.lside[rb] = (double)vside;
            }
        }
        return;
    }
    if (blockIdx.x == 0) {
        // ---- block 0: d[N_j] -= theta_d * alpha_j for every nonbasic j != q (dual…:296-300), and the commit
        for (int64_t j0 = tid; j0 < a.nN; j0 += 4 * 256) {
            int64_t v[4];
            double al[4], dv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t j = j0 + 256 * k;
                const bool ok = j < a.nN && j != q;
                v[k] = ok ? a.N_index[j] : -1;
                al[k] = ok ? a.xc.r(j) : 0.0;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) dv[k] = v[k] >= 0 ? a.dd[v[k]] : 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (v[k] >= 0) a.dd[v[k]] = dv[k] - theta_d * al[k];
        }
        if (tid == 0) {  // the decision, for k_dual_close
            ELLP_CHECK(st, q >= 0 && q < a.nN, 9121);
            ELLP_CHECK(st, r >= 0 && r < m, 9122);
            st->s_cur = cur;
            st->s_q = q;
            st->s_at_lower = 0;
            st->s_jq = a.N_index[q];
            st->s_r = r;
            st->s_lv = a.B_index[r];
            st->s_delta = delta;
            st->s_side = st->lside;
            st->s_theta_d = theta_d;
            st->dp_seq = a.seq;  // open until the next pricing launch (dual_price_prologue) or k_dual_close has closed it
        }
        return;
    }
    // ---- block 1: y += theta_d * rho (dual…:302)
    {
        const double *rho = src + r * a.ld;
        for (int64_t i = tid; i < m; i += 256) a.y[i] = a.y[i] + theta_d * rho[i];
    }
}

// The closing block of a fused dual iteration: everything k_update2<1>'s bookkeeping blocks do besides the d_N, y and
// x_B loops (those ran in k_dual_fu).  Engines without tiny-pivot maintenance let the NEXT pricing launch do this work
// in its prologue (dual_price_prologue: the block that owns position q swaps the columns before it prices them, block
// 0 books the scalars) and launch this kernel only where a complete state is needed — the end of a batch, before
// maintenance; it does nothing if the iteration in front of it has been closed already.
struct DualCloseArgs {
    const double *d;
    double *A_N, *A_B, *c_B, *c_N, *x, *dd;
    int64_t *B_index, *N_index;
    uint8_t *Nb;
    const int32_t *lrow;
    const double *ldelta, *lside;
    int nrb;  // row blocks of k_dual_fu
    DevState *st;
    int64_t m, ld;
    double ill_tol;
    Trace trace;
    int maxviol;
};
__global__ __launch_bounds__(256) void k_dual_close(DualCloseArgs a) {
    __shared__ long long s_tmp[4];
    __shared__ double s_amax[4];
    DevState *st = a.st;
    if (st->status != ST_RUNNING) return;
    if (st->dp_seq == ~0ull || st->dp_applied == st->dp_seq) return;  // nothing open
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = a.m;
    bool tiny_pivot = false;
    if (a.ill_tol > 0.0) {  // see k_update2
        const double d_r = a.d[st->s_r];
        double amax = 0.0;
        for (int64_t i = tid; i < m; i += 256) amax = fmax(amax, fabs(a.d[i]));
        amax = wave_allmax_dpp(amax != amax ? INFINITY : amax);
        if (lane == 0) s_amax[wave] = amax;
        __syncthreads();
        amax = fmax(fmax(s_amax[0], s_amax[1]), fmax(s_amax[2], s_amax[3]));
        tiny_pivot = fabs(d_r) < a.ill_tol * amax;
    }
    const DualLeave lv = dual_first_violation(a.lrow, a.ldelta, a.lside, a.nrb, tid, s_tmp, a.maxviol);
    dual_close_swap(a.A_N, a.A_B, a.c_B, a.c_N, a.dd, a.N_index, a.Nb, st, a.ld, tid);
    if (tid == 128) {
        dual_close_scalars(st, a.d, a.x, a.B_index, a.trace, lv.lr, lv.delta, lv.side);
        st->dp_seq = ~0ull;
        if (tiny_pivot && st->status == ST_RUNNING) st->tiny = 1;
    }
}

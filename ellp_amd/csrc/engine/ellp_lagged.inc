// ellp_lagged.inc — the primal iteration in TWO launches instead of three (ellp_opts.pipeline = 2,
// the default from m = 1024).
//
// Three-launch iteration k:   price(k) | ftran(k): entering fold, d_k = W_k a_q | update(k): ratio fold,
//                             W_{k+1} = E_k W_k, bookkeeping            — B^-1 is read twice and written once.
// Two-launch iteration k:     P_k = k_price2   [ratio fold + bookkeeping of iteration k-1] + pricing of k
//                             F_k = k_ftran_eta [entering fold of k] + ONE pass over B^-1 that applies the
//                                   eta update of pivot k-1 (W_k = E_{k-1} W_{k-1}, written to the other
//                                   buffer) and, from the freshly updated rows still in registers, forms
//                                   d_k = +-W_k a_q and lambda_i                — B^-1 read once, written once.
// Per pivot 8 m ld bytes less traffic (176 MB instead of 208 MB at config 3) and one dependent kernel
// boundary less.  What makes it possible: pricing does not need W_k, only u_k = u_{k-1} + (r_q/alpha_r) rho
// with rho = row r of W_{k-1}, which every pricing block forms in registers / LDS once the ratio fold
// (recomputed in every block's prologue from per-row-block minima of lambda, a few hundred doubles) has
// named r.  The position q that the leaving column moves into is priced from A_B[:, r] directly, while a
// bookkeeping block moves the columns (the entering column is parked in aq_save and reaches A_B[:, r] in
// F_k, so that no block of P_k reads a column another block of P_k writes).
//
// Who writes what (rule of the file: a kernel never reads a state field one of its own blocks writes):
//   P_k leader:  pe_valid / pe_r / pe_d_r / pe_alpha_r / f_src (the eta F_k has to apply), usel_next,
//                the counters, the point, B_index[r]; block 1: u[usel ^ 1], the column move, N_index[q],
//                Nb[q], c_N[q], mv_*.
//   F_k block 0: A_B[:, mv_r] <- aq_save, c_B[mv_r]; at its end the snapshot s_* of iteration k, cur, usel,
//                and — if no candidate is left — fin (the status itself is written by the NEXT kernel's
//                leader: all of F_k's blocks must still apply the eta update, see ST_NEED_MAINT).
// An iteration is COUNTED when F_k commits its entering variable (the reference counts loop bodies entered)
// and COMPLETE when the following P has folded its ratio test — or k_update2 as the closing kernel, which the
// host enqueues only when something needs the completed state (read-back, phase hand-off, maintenance of a
// stopped engine): run() slices leave the last iteration open, so slicing costs nothing.
// Host side: launch_primal_iteration_lagged / launch_flush.
//
// The arithmetic of every quantity is the three-launch path's (same fma's on the same operands); only the
// summation order of the FTRAN dot products differs (a block of 256 threads per row instead of a wave).

struct Price2Args {
    PriceArgs p;              // A_N, c_N, Nb, N_index, xc, st, ld, nN, cpb, block0, eps (u, W0/W1 as below)
    double *u0, *u1;          // DevState::usel names the current one; the bookkeeping block writes the other
    double *W0, *W1;          // rho = row r of the buffer DevState::cur names
    const double *d, *lam, *bmin, *bsec;   // bmin / bsec: smallest and second smallest lambda of each row block
    const int32_t *bidx, *binfo;          // binfo: 2 * (row of the smallest) + (d_i > 0)
    const uint8_t *dpos;
    double *A_N, *A_B, *aq_save, *c_B, *c_N, *x;
    const double *lb, *ub;
    const uint8_t *kind;
    int64_t *B_index, *N_index;
    uint8_t *Nb;
    int64_t m;
    int rpb;        // rows per block of k_ftran_eta (1, 2, 4 or 8): bmin[b] = min lambda over rows b*rpb..
    int use_pend;   // 0: nothing to fold (first iteration of a slice, or the open decision was dropped)
    uint8_t *pos_hint;  // k_price2_wave: per nonbasic position, 1 = a unit column sat here at the previous launch
    // column-sharded engines (ellp_shard.inc): this rank holds the nonbasic positions [own0, own1) only; the entering
    // column of the open iteration is in aq_cur on every rank (k_ftran_eta's block 0 left it there from the winner's pack)
    const double *aq_cur;   // null: not sharded
    int64_t own0, own1;
    double ill_tol;
    double guard_abs;  // > 0: a pivot with |alpha_r| < guard_abs is NOT taken — every block returns before the bookkeeping and the
                       // pricing, the leader drops the open iteration and writes ST_NEED_EXACT (certified engines, ellp_engine.hip)
    Trace trace;
};

// what k_price2 needs of the state, fetched as ONE batch of 16-byte loads at entry (every separate
// `st->field` test in front of a branch is a round trip of its own, and the prologue is a chain of them)
struct PHead {
    int status, nan_flag, cur, s_at_lower, tiny, fin, usel, s_nbq;
    long long s_q;
    double s_rq, s_lambda0;
};
__device__ __forceinline__ PHead load_phead(const DevState *st) {
    static_assert(offsetof(DevState, s_cur) == 16 && offsetof(DevState, s_q) == 32 && offsetof(DevState, s_rq) == 64 &&
                      offsetof(DevState, fin) == 80 && offsetof(DevState, tiny) == 28 && offsetof(DevState, s_nbq) == 88,
                  "DevState head layout");
    const int4 *h = reinterpret_cast<const int4 *>(st);
    const int4 g0 = h[0], g1 = h[1], g5 = h[5];
    const longlong2 g2 = reinterpret_cast<const longlong2 *>(st)[2];
    const double2 g4 = reinterpret_cast<const double2 *>(st)[4];
    PHead o;
    o.status = g0.x; o.nan_flag = g0.y; o.cur = g0.w;
    o.s_at_lower = g1.y; o.tiny = g1.w;
    o.s_q = g2.x;
    o.s_rq = g4.x; o.s_lambda0 = g4.y;
    o.fin = g5.x; o.usel = g5.y; o.s_nbq = g5.z;
    return o;
}

struct PendInfo {
    int has;        // 1: a decision was folded; r, lambda, side are valid
    long long r;    // leaving row, -1: bound flip
    double lambda;
    int side;
    long long q;    // nonbasic position the decision refers to
    double cf;      // r_q / alpha_r
    double d_r, alpha_r;
    int newlabel;   // Nb[q] after the bookkeeping (side, or the flipped label)
};

constexpr int P2_BOOK = 2;  // bookkeeping blocks in front of the pricing blocks

// entry checks of k_price2 on the fetched head; returns false if the block has to return
__device__ __forceinline__ bool price2_entry(DevState *st, const PHead &h) {
    if (h.status != ST_RUNNING) return false;
    if (h.tiny) {  // a maintenance request (tiny pivot, drift monitor, refused refresh): stop the batch here
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            st->status = ST_NEED_MAINT;
            __threadfence();
            st->tiny = 0;
        }
        return false;
    }
    if (h.fin) {  // k_ftran_eta found no entering candidate: now it may become the status
        if (blockIdx.x == 0 && threadIdx.x == 0) st->status = h.fin - 1;
        return false;
    }
    return true;
}

// (smallest, its row info, second smallest) of a set of lambda's; combine() keeps the pair exact: the
// second smallest of a union is the smaller of the two seconds and the larger of the two firsts
struct Min2 {
    double m1, m2;
    int info;
};
__device__ __forceinline__ Min2 min2_combine(const Min2 &x, const Min2 &y) {
    Min2 o;
    if (x.m1 <= y.m1) {
        o.m1 = x.m1;
        o.info = x.info;
        o.m2 = fmin(x.m2, y.m1);
    } else {
        o.m1 = y.m1;
        o.info = y.info;
        o.m2 = fmin(y.m2, x.m1);
    }
    return o;
}

// First half of the ratio-test prologue; its loads are issued with the head's.  Row-block minima ->
// chunk minima in LDS (for the exact fold) and, per wave, the (smallest, second smallest) pair over all
// row blocks (for the shortcut of price2_fold).  chunkmin: >= ceil(m/64) doubles; s_m2: 4 entries.
__device__ __forceinline__ void price2_stage_minima(const Price2Args &a, double *chunkmin, Min2 *s_m2) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nrb = (int)((a.m + a.rpb - 1) / a.rpb);
    const int per = 64 / a.rpb;  // row blocks per 64-row chunk
    Min2 acc{INFINITY, INFINITY, -1};
    for (int b0 = 0; b0 < nrb; b0 += 256) {
        const int b = b0 + tid;
        const int bc = b < nrb ? b : 0;
        const double t = a.bmin[bc], t2 = a.bsec[bc];
        const int inf = a.binfo[bc];
        double v = b < nrb ? t : INFINITY;
        if (b < nrb) acc = min2_combine(acc, Min2{t, t2, inf});
        for (int o = 1; o < per; o <<= 1) v = fmin(v, __shfl_xor(v, o));
        if ((lane % per) == 0 && b < nrb) chunkmin[b / per] = v;
    }
    // wave-wide combine without the LDS crossbar (__shfl_xor is ds_bpermute here, ~100 cycles a step on the critical
    // path of every pricing launch): four DPP butterfly steps inside each row of 16 lanes, then the four rows through
    // readlane.  min2_combine is symmetric in its arguments up to the choice among equal firsts, which the margin
    // test below rejects anyway, so the order of the combination does not matter.
#define MIN2_DPP_STEP(CTRL)                                   \
    {                                                         \
        Min2 y;                                               \
        y.m1 = dpp_f64<CTRL>(acc.m1);                         \
        y.m2 = dpp_f64<CTRL>(acc.m2);                         \
        y.info = dpp_i32<CTRL>(acc.info);                     \
        acc = min2_combine(acc, y);                           \
    }
    MIN2_DPP_STEP(0xB1)   // quad_perm [1,0,3,2]
    MIN2_DPP_STEP(0x4E)   // quad_perm [2,3,0,1]
    MIN2_DPP_STEP(0x141)  // row_half_mirror
    MIN2_DPP_STEP(0x140)  // row_mirror
#undef MIN2_DPP_STEP
    {
        Min2 rw[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            rw[k].m1 = readlane_f64(acc.m1, 16 * k);
            rw[k].m2 = readlane_f64(acc.m2, 16 * k);
            rw[k].info = __builtin_amdgcn_readlane(acc.info, 16 * k);
        }
        acc = min2_combine(min2_combine(rw[0], rw[1]), min2_combine(rw[2], rw[3]));
    }
    if (lane == 0) s_m2[wave] = acc;
}

// Second half: wave 0 folds (primal…:379-400, exactly: ratio_fold), everybody gets (r, lambda, side); the
// values that hang off r (d_r, hence alpha_r and r_q/alpha_r) are loaded by every thread itself, together
// with its slice of rho — one round trip instead of two.  Returns false if the kernel has to stop.
__device__ __forceinline__ bool price2_fold(const Price2Args &a, const PHead &h, const double *chunkmin, const Min2 *s_m2,
                                            PendInfo *s_pi, PendInfo &pi, bool leader) {
    DevState *st = a.p.st;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    pi.has = 0;
    pi.r = -1;
    pi.q = -1;
    pi.lambda = 0.0;
    pi.side = 0;
    pi.cf = pi.d_r = pi.alpha_r = 0.0;
    pi.newlabel = 0;
    if (!a.use_pend) return true;
    lds_barrier();  // chunkmin and the per-wave pairs are complete
    // Shortcut.  Let L be the smallest of all lambda_i and of lambda_0 (the entering variable's own span).
    // If everything else is at least 2 EPS above L, the reference's sequential scan (primal…:379-400) ends at
    // L's owner whatever the order: when its turn comes the running minimum is >= L + 2 EPS, so it wins by the
    // strict branch, and afterwards nothing is below L - EPS or within EPS of it.  Then the answer is in the
    // row-block records already fetched and no lambda has to be read at all.  Otherwise: the exact fold.
    Min2 g = min2_combine(min2_combine(s_m2[0], s_m2[1]), min2_combine(s_m2[2], s_m2[3]));
    const double l0 = h.s_lambda0;
    bool fast = false;
    if (g.m1 >= 0.0 && g.m1 - 0.0 == g.m1) {  // not NaN, not negative (the panic of primal…:402 goes through the exact fold)
        if (l0 - g.m1 >= 2.0 * a.p.eps && g.m2 - g.m1 >= 2.0 * a.p.eps && g.info >= 0 && !isinf(g.m1)) {
            fast = true;
            pi.lambda = g.m1;
            pi.r = g.info >> 1;
            pi.side = (g.info & 1) ? ELLP_NB_UPPER : ELLP_NB_LOWER;
        } else if (g.m1 - l0 >= 2.0 * a.p.eps && l0 >= 0.0) {  // the bound flip of primal…:223-231
            fast = true;
            pi.lambda = l0;
            pi.r = -1;
            pi.side = ELLP_NB_LOWER;
        }
    }
    if (!fast) {
        if (wave == 0) {
            const RatioResult rr = ratio_fold(chunkmin, (int)((a.m + 63) >> 6), a.m, a.lam, a.bidx, a.dpos, h.s_lambda0, a.p.eps, lane);
            if (lane == 0) {
                s_pi->lambda = rr.lambda;
                s_pi->r = rr.nb;
                s_pi->side = rr.side;
            }
        }
        lds_barrier();
        pi.lambda = s_pi->lambda;
        pi.r = s_pi->r;
        pi.side = s_pi->side;
    }
    pi.has = 1;
    pi.q = h.s_q;
    const double lambda = pi.lambda;
    if (h.nan_flag) {
        if (leader) st->status = ELLP_ERR_NAN;
        return false;
    }
    if (!(lambda >= 0.0)) {  // primal…:402
        if (leader) {
            st->panic_code = 402;
            st->status = ELLP_ERR_PANIC;
        }
        return false;
    }
    if (isinf(lambda)) {  // primal…:404-406 (the loop body was counted when k_ftran_eta entered it)
        if (leader) st->status = ELLP_UNBOUNDED;
        return false;
    }
    if (pi.r >= 0) {
        pi.newlabel = pi.side;
    } else {
        const int nbq = h.s_nbq;
        pi.newlabel = nbq == ELLP_NB_LOWER ? ELLP_NB_UPPER : (nbq == ELLP_NB_UPPER ? ELLP_NB_LOWER : nbq);
    }
    return true;
}
// d_r, alpha_r, r_q/alpha_r once d[r] has been loaded
__device__ __forceinline__ void price2_pivot_scalars(PendInfo &pi, const PHead &h, double d_r) {
    pi.d_r = d_r;
    pi.alpha_r = h.s_at_lower ? -d_r : d_r;
    pi.cf = h.s_rq / pi.alpha_r;
}

// the two bookkeeping blocks of k_price2 (what k_update2<0>'s bookkeeping blocks do, primal…:408-417, :205-232)
// SH: the engine is column-sharded (a compile-time switch: the unsharded kernels must not carry its branches — measured:
// 0.6-0.8 us per launch of either kernel at config 3 when they did)
template <bool SH>
__device__ __forceinline__ void price2_bookkeeping(const Price2Args &a, const PHead &h, const PendInfo &pi) {
    DevState *st = a.p.st;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t m = a.m, ld = a.p.ld;
    const int cur = h.cur, usel = h.usel;
    if (blockIdx.x == 0) {
        // block 0: the point, the basic side of the swap, the counters, and the eta k_ftran_eta applies
        if (!pi.has) {
            if (tid == 0) {
                st->pe_valid = 0;
                st->f_src = cur;
                st->usel_next = usel;
            }
            return;
        }
        const long long r = pi.r;
        const double lambda = pi.lambda;
        const int64_t jq = st->s_jq;
        const int at_lower = h.s_at_lower;
        bool tiny_pivot = false;
        if (a.ill_tol > 0.0 && r >= 0) {
            __shared__ double s_amax[4];
            double amax = 0.0;
            for (int64_t i = tid; i < m; i += 256) amax = fmax(amax, fabs(a.d[i]));
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) amax = fmax(amax, __shfl_xor(amax, o));
            if (lane == 0) s_amax[wave] = amax;
            __syncthreads();
            amax = fmax(fmax(s_amax[0], s_amax[1]), fmax(s_amax[2], s_amax[3]));
            tiny_pivot = fabs(pi.d_r) < a.ill_tol * amax;
        }
        if (lambda > 0.0) {  // primal…:408-417
            for (int64_t i0 = tid; i0 < m; i0 += 4 * 256) {
                int64_t bi[4];
                double xv[4], dv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int64_t i = i0 + 256 * k;
                    bi[k] = i < m ? a.B_index[i] : -1;
                    dv[k] = i < m ? a.d[i] : 0.0;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) xv[k] = bi[k] >= 0 ? a.x[bi[k]] : 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (bi[k] >= 0) a.x[bi[k]] = xv[k] + lambda * dv[k];
            }
            if (tid == 0) {
                if (at_lower) a.x[jq] = a.x[jq] + lambda;
                else a.x[jq] = a.x[jq] - lambda;
            }
        }
        __syncthreads();  // B_index reads above vs the write below
        if (tid == 0) {
            st->lambda = lambda;
            st->open = 0;
            if (lambda > 0.0) st->obj = st->obj + (at_lower ? lambda * h.s_rq : -(lambda * h.s_rq));
            trace_put(a.trace, st->iters, st->obj);
            st->f_src = cur;
            if (r >= 0) {
                a.B_index[r] = jq;
                st->pivots += 1;
                st->pe_valid = 1;
                st->pe_r = r;
                st->pe_d_r = pi.d_r;
                st->pe_alpha_r = pi.alpha_r;
                st->usel_next = usel ^ 1;
                if (tiny_pivot) st->tiny_p = 1;  // relayed by k_ftran_eta: this launch's own blocks test `tiny` at entry
            } else {  // primal…:223-231
                st->flips += 1;
                st->pe_valid = 0;
                st->usel_next = usel;
                if (h.s_nbq != ELLP_NB_LOWER && h.s_nbq != ELLP_NB_UPPER) {  // a Free label cannot be flipped
                    st->panic_code = 229;  // "pivot should have been unbounded"
                    st->status = ELLP_ERR_PANIC;
                }
            }
        }
        return;
    }
    // block 1: u for the next iteration, the column move and everything indexed by the nonbasic position q
    if (!pi.has) return;
    const long long q = pi.q, r = pi.r;
    if (r < 0) {
        if (tid == 0) a.Nb[q] = (uint8_t)pi.newlabel;
        return;
    }
    const double *W = cur ? a.W1 : a.W0;
    const double2 *rho2 = reinterpret_cast<const double2 *>(W + r * ld);
    const double2 *us = reinterpret_cast<const double2 *>(usel ? a.u1 : a.u0);
    double2 *ud = reinterpret_cast<double2 *>(usel ? a.u0 : a.u1);
    double2 *cn = reinterpret_cast<double2 *>(a.A_N + q * ld);
    const double2 *cb = reinterpret_cast<const double2 *>(a.A_B + r * ld);
    double2 *sv = reinterpret_cast<double2 *>(a.aq_save);
    const bool own_q = !SH || (q >= a.own0 && q < a.own1);  // sharded: only the owner of position q holds (and rewrites) it
    const double2 *aqc = SH ? reinterpret_cast<const double2 *>(a.aq_cur) : cn;
    for (int64_t t = tid; t < (ld >> 1); t += 256) {
        const double2 p = rho2[t];
        double2 w = us[t];
        w.x = fma(pi.cf, p.x, w.x);
        w.y = fma(pi.cf, p.y, w.y);
        ud[t] = w;
        const double2 aq = aqc[t];
        if (own_q) cn[t] = cb[t];  // the leaving column becomes nonbasic column q ...
        sv[t] = aq;     // ... the entering one reaches A_B[:, r] in k_ftran_eta (a pricing block reads A_B[:, r] now)
    }
    if (tid == 0) {
        st->cq_save = a.c_N[q];
        a.c_N[q] = a.c_B[r];
        a.N_index[q] = a.bidx[r];
        a.Nb[q] = (uint8_t)pi.side;
        st->mv_r = r;
        st->mv_pending = 1;
    }
}

// ------------------------------------------------------------------ P: block-per-column-group shape
template <int T, bool NT, bool SH = false>
__global__ __launch_bounds__(256) void k_price2(Price2Args a) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ PendInfo s_pi;
    __shared__ Min2 s_m2[4];
    __shared__ double s_part[2][4][4];
    DevState *st = a.p.st;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t ld = a.p.ld, half = ld >> 1;
    double *chunkmin = reinterpret_cast<double *>(smem);
    // ---- round trip 1: the state head and (if a decision is open) the row-block minima
    const PHead h = load_phead(st);
    if (a.use_pend) price2_stage_minima(a, chunkmin, s_m2);
    if (!price2_entry(st, h)) return;
    // ---- round trip 2 (inside the fold): the lambda's of the chunk(s) that can hold the minimum
    PendInfo pi;
    if (!price2_fold(a, h, chunkmin, s_m2, &s_pi, pi, blockIdx.x == 0 && tid == 0)) return;
    const bool pivoted = pi.has && pi.r >= 0;
    // ---- round trip 3: d[r], this thread's slices of u_{k-1} and of rho
    const double2 *u2 = reinterpret_cast<const double2 *>(h.usel ? a.u1 : a.u0);
    const double2 *rho2 = reinterpret_cast<const double2 *>((h.cur ? a.W1 : a.W0) + (pivoted ? pi.r : 0) * ld);
    const double d_r = a.d[pivoted ? pi.r : 0];
    double2 ur[T], pr[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const int64_t idx = tid + 256 * t;
        const int64_t ic = idx < half ? idx : 0;
        const double2 uv = u2[ic];
        const double2 pv = rho2[ic];
        ur[t] = idx < half ? uv : make_double2(0.0, 0.0);
        pr[t] = (pivoted && idx < half) ? pv : make_double2(0.0, 0.0);
    }
    // (behind the loads above: d_r arrives with u and rho, one round trip)
    if (a.guard_abs > 0.0 && pivoted && fabs(d_r) < a.guard_abs) {  // see ST_NEED_EXACT: nothing of the iteration is committed
        if (blockIdx.x == 0 && tid == 0) {
            st->open = 0;
            st->iters -= 1;  // k_ftran_eta counted it when it entered it
            st->status = ST_NEED_EXACT;
        }
        return;
    }
    if (pivoted) {
        price2_pivot_scalars(pi, h, d_r);
#pragma unroll
        for (int t = 0; t < T; ++t) {  // u_k = u_{k-1} + (r_q / alpha_r) rho (the bookkeeping block writes the same values)
            ur[t].x = fma(pi.cf, pr[t].x, ur[t].x);
            ur[t].y = fma(pi.cf, pr[t].y, ur[t].y);
        }
    }
    if (blockIdx.x < P2_BOOK) {
        price2_bookkeeping<SH>(a, h, pi);
        return;
    }
    const int gb = a.p.block0 + (int)blockIdx.x - P2_BOOK;  // global pricing block
    const int64_t j0 = (int64_t)gb * a.p.cpb;
    const int64_t j1 = (j0 + a.p.cpb < a.p.nN) ? j0 + a.p.cpb : a.p.nN;
    if (j0 >= a.p.nN) return;
    const long long qpos = pi.has ? pi.q : -1;
    double best = -INFINITY;
    int buf = 0;
    // unit columns (PriceArgs::vs_row): every wave fetches the flags of the block's columns itself (lane l: column
    // j0 + l); the position that changes hands in this launch is priced from A_B like any general column
    const bool use_vs = a.p.vs_row != nullptr;
    int sgl = -1;
    double svl = 0.0;
    if (use_vs && j0 + lane < j1 && j0 + lane != qpos) {
        const int64_t v = a.p.N_index[j0 + lane];
        sgl = a.p.vs_row[v];
        svl = a.p.vs_val[v];
    }
    const double *u_prev = reinterpret_cast<const double *>(u2), *rho_g = reinterpret_cast<const double *>(rho2);
    for (int64_t j = j0; j < j1; j += 4, buf ^= 1) {
        const int ncol = (int)((j1 - j) < 4 ? (j1 - j) : 4);
        int nb_pre = 0;
        double cd_pre = 0.0;
        {
            const int64_t jo = j + (tid < ncol ? tid : 0);
            nb_pre = a.p.Nb[jo];
            cd_pre = a.p.c_N[jo];
            if (jo == qpos) {  // this position changes hands in this very launch: take the new owner's data
                nb_pre = pi.newlabel;
                if (pivoted) cd_pre = a.c_B[pi.r];
            }
        }
        int sg[4] = {-1, -1, -1, -1};
        bool all_unit = use_vs;
        int dense0 = -1;  // a general column of the group: unit columns are pointed at it (no traffic of their own)
        if (use_vs) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < ncol) {
                    sg[k] = __builtin_amdgcn_readlane(sgl, (int)(j - j0) + k);
                    if (sg[k] < 0) {
                        all_unit = false;
                        if (dense0 < 0) dense0 = k;
                    }
                }
            }
        }
        // the column-owner threads (tid < ncol, all in wave 0): their own column's flag, value and entry of u_k
        // (the same fma the staging above and the bookkeeping block perform)
        // (the shuffles run on all lanes: a lane that sits out cannot be read from)
        const int sg_sh = __shfl(sgl, ((int)(j - j0) + (tid & 3)) & 63);
        const double my_sv = __shfl(svl, ((int)(j - j0) + (tid & 3)) & 63);
        const int my_sg = (use_vs && tid < ncol) ? sg_sh : -1;
        double u_unit = 0.0;
        if (my_sg >= 0) {
            u_unit = u_prev[my_sg];
            if (pivoted) u_unit = fma(pi.cf, rho_g[my_sg], u_unit);
        }
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        if (!all_unit) {
            const double2 *col[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int64_t jj = (j + k < j1) ? j + k : j1 - 1;
                if (use_vs && k < ncol && sg[k] >= 0) jj = j + dense0;
                col[k] = reinterpret_cast<const double2 *>((pivoted && jj == qpos) ? a.A_B + pi.r * ld : a.p.A_N + jj * ld);
            }
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const int64_t idx = tid + 256 * t;
                if (idx < half) {
                    double2 v[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) v[k] = load_col2<NT>(col[k] + idx);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        acc[k] = fma(v[k].x, ur[t].x, acc[k]);
                        acc[k] = fma(v[k].y, ur[t].y, acc[k]);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = wave_sum(acc[k]);
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) s_part[buf][wave][k] = acc[k];
        }
        __syncthreads();
        if (tid < ncol) {
            const int k = tid;
            double dot = ((s_part[buf][0][k] + s_part[buf][1][k]) + s_part[buf][2][k]) + s_part[buf][3][k];
            if (my_sg >= 0) dot = my_sv * u_unit;
            const int64_t jj = j + k;
            const int nb = nb_pre;
            const double rj = cd_pre - dot;
            double key = -INFINITY;
            if (rj != rj) st->nan_flag = 1;
            else key = primal_key(rj, nb, a.p.eps);
            a.p.xc.r(jj) = rj;
            a.p.xc.key(jj) = key;
            best = fmax(best, key);
        }
    }
    if (wave == 0) {
        double v = (lane < 4) ? best : -INFINITY;
        v = fmax(v, __shfl_xor(v, 1));
        v = fmax(v, __shfl_xor(v, 2));
        if (lane == 0) a.p.xc.bk(gb) = v;
    }
}

// ------------------------------------------------------------------ P: wave-per-column-pair shape
// (cache-resident A_N, as k_price_wave).  u_k is staged once per block in LDS (8 ld bytes) instead of
// being re-read from L1/L2 per column pair: it does not exist in memory while this kernel runs.  The
// first 4 KiB of each wave's first column pair are fetched into registers BEFORE the prologue, so that
// the column stream is already running when the fold and the u_k staging finish.
template <bool SH = false>
__global__ __launch_bounds__(256, 4) void k_price2_wave(Price2Args a) {  // 4 waves per SIMD: all ~1026 blocks resident at once (127 VGPRs)
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ PendInfo s_pi;
    __shared__ Min2 s_m2[4];
    __shared__ double s_k[4];
    DevState *st = a.p.st;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t ld = a.p.ld, half = ld >> 1;
    double2 *s_u = reinterpret_cast<double2 *>(smem);                // ld doubles
    double *chunkmin = reinterpret_cast<double *>(smem) + ld;        // ceil(m/64) doubles
    // ---- round trip 1: the state head, the row-block minima, the head of this wave's first column pair
    const PHead h = load_phead(st);
    if (a.use_pend) price2_stage_minima(a, chunkmin, s_m2);
    const bool pricing = blockIdx.x >= P2_BOOK;
    const int gb = a.p.block0 + (int)blockIdx.x - P2_BOOK;
    const int64_t j0 = pricing ? (int64_t)gb * a.p.cpb : 0;
    const int64_t j1 = pricing ? ((j0 + a.p.cpb < a.p.nN) ? j0 + a.p.cpb : a.p.nN) : 0;
    const int64_t jf = j0 + 2 * wave;  // this wave's first pair
    const bool havef = pricing && jf < j1;
    double2 pf0[4], pf1[4];
    // unit columns (PriceArgs::vs_row): lane l holds the flag of column j0 + l (two dependent loads, used only after
    // the fold).  Whether the first pair is worth prefetching is taken from a HINT: the flags the previous launch
    // saw at these positions (pos_hint; right for every position but the one that changed hands since — a hint only
    // decides about the prefetch, never about a dot product).  It arrives with the state head, which the entry check
    // below waits for anyway, so the prefetch is issued one round trip into the three of the prologue.
    const bool use_vs = a.p.vs_row != nullptr;
    int sgl = -1;
    double svl = 0.0;
    int hint = 0;
    if (use_vs && pricing && j0 + lane < j1) {
        hint = a.pos_hint[j0 + lane];
        const int64_t v = a.p.N_index[j0 + lane];
        sgl = a.p.vs_row[v];
        svl = a.p.vs_val[v];
    }
    bool skip_pf = false;
    if (use_vs && havef) {
        const int h0 = __builtin_amdgcn_readlane(hint, (int)(jf - j0));
        const int h1 = __builtin_amdgcn_readlane(hint, (int)((jf + 1 < j1 ? jf + 1 : jf) - j0));
        skip_pf = h0 && h1;
    }
    {
        __builtin_amdgcn_sched_barrier(0);
        const int64_t jclamp = SH ? a.own0 : 0;  // a column this rank holds (column-sharded: position 0 may be a peer's)
        const int64_t ja = havef ? jf : jclamp, jb = (havef && jf + 1 < j1) ? jf + 1 : ja;
        const double2 *c0 = reinterpret_cast<const double2 *>(a.p.A_N + ja * ld);
        const double2 *c1 = reinterpret_cast<const double2 *>(a.p.A_N + jb * ld);
        if (!skip_pf) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t t = lane + WAVE * k;
                const int64_t tc = t < half ? t : 0;
                pf0[k] = c0[tc];
                pf1[k] = c1[tc];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) pf0[k] = pf1[k] = make_double2(0.0, 0.0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (!price2_entry(st, h)) return;
    // ---- round trip 2 (inside the fold): the lambda's of the chunk(s) that can hold the minimum
    PendInfo pi;
    if (!price2_fold(a, h, chunkmin, s_m2, &s_pi, pi, blockIdx.x == 0 && tid == 0)) return;
    const bool pivoted = pi.has && pi.r >= 0;
    // ---- round trip 3: d[r], u_{k-1} and rho slices -> u_k in LDS
    {
        const double2 *u2 = reinterpret_cast<const double2 *>(h.usel ? a.u1 : a.u0);
        const double2 *rho2 = reinterpret_cast<const double2 *>((h.cur ? a.W1 : a.W0) + (pivoted ? pi.r : 0) * ld);
        const double d_r = a.d[pivoted ? pi.r : 0];
        double2 ur[8], pr[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int64_t idx = tid + 256 * t;
            const int64_t ic = idx < half ? idx : 0;
            ur[t] = u2[ic];
            pr[t] = rho2[ic];
        }
        // (behind the loads above: d_r arrives with u and rho, one round trip)
        if (a.guard_abs > 0.0 && pivoted && fabs(d_r) < a.guard_abs) {  // see ST_NEED_EXACT: nothing of the iteration is committed
            if (blockIdx.x == 0 && tid == 0) {
                st->open = 0;
                st->iters -= 1;  // k_ftran_eta counted it when it entered it
                st->status = ST_NEED_EXACT;
            }
            return;
        }
        if (pivoted) price2_pivot_scalars(pi, h, d_r);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int64_t idx = tid + 256 * t;
            if (idx < half) {
                double2 w = ur[t];
                if (pivoted) {
                    w.x = fma(pi.cf, pr[t].x, w.x);
                    w.y = fma(pi.cf, pr[t].y, w.y);
                }
                s_u[idx] = w;
            }
        }
    }
    if (!pricing) {
        price2_bookkeeping<SH>(a, h, pi);
        return;
    }
    lds_barrier();
    if (j0 >= a.p.nN) return;
    const long long qpos = pi.has ? pi.q : -1;
    double best = -INFINITY;  // lanes 0 and 1 own the pair's two columns
    for (int64_t j = jf; j < j1; j += 8) {
        const int ncol = (j1 - j) < 2 ? 1 : 2;
        int nb_pre = 0;
        double cd_pre = 0.0;
        {
            const int64_t jo = j + (lane < ncol ? lane : 0);
            nb_pre = a.p.Nb[jo];
            cd_pre = a.p.c_N[jo];
            if (jo == qpos) {
                nb_pre = pi.newlabel;
                if (pivoted) cd_pre = a.c_B[pi.r];
            }
        }
        const int64_t ja = j, jb = (j + 1 < j1 ? j + 1 : j);
        const bool sub0 = pivoted && ja == qpos, sub1 = pivoted && jb == qpos;
        // unit columns: not streamed (the position that changes hands — its variable is not N_index's yet — is priced
        // from A_B like a general column); next to a general column they are pointed at it: no traffic of their own
        const int s0 = (use_vs && ja != qpos) ? __builtin_amdgcn_readlane(sgl, (int)(ja - j0)) : -1;
        const int s1 = (use_vs && jb != qpos) ? __builtin_amdgcn_readlane(sgl, (int)(jb - j0)) : -1;
        const bool stream = !(s0 >= 0 && s1 >= 0);
        const double2 *c0r = reinterpret_cast<const double2 *>(sub0 ? a.A_B + pi.r * ld : a.p.A_N + ja * ld);
        const double2 *c1r = reinterpret_cast<const double2 *>(sub1 ? a.A_B + pi.r * ld : a.p.A_N + jb * ld);
        const double2 *c0 = s0 >= 0 ? c1r : c0r, *c1 = s1 >= 0 ? c0r : c1r;
        double acc0 = 0.0, acc1 = 0.0;
        int64_t tstart = lane;
        if (j == jf && !sub0 && !sub1 && stream && !skip_pf) {  // the prefetched head of the first pair (unless it is the position that changes hands)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t t = lane + WAVE * k;
                const double2 uv = s_u[t < half ? t : 0];
                const double2 uu = t < half ? uv : make_double2(0.0, 0.0);
                acc0 = fma(pf0[k].x, uu.x, acc0);
                acc0 = fma(pf0[k].y, uu.y, acc0);
                acc1 = fma(pf1[k].x, uu.x, acc1);
                acc1 = fma(pf1[k].y, uu.y, acc1);
            }
            tstart = lane + 4 * WAVE;
        }
        for (int64_t t0 = tstart; stream && t0 < half; t0 += 4 * WAVE) {
            double2 uu[4], v0[4], v1[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t t = t0 + WAVE * k;
                const int64_t tc = t < half ? t : 0;
                const double2 uv = s_u[tc];
                uu[k] = t < half ? uv : make_double2(0.0, 0.0);
                v0[k] = c0[tc];
                v1[k] = c1[tc];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc0 = fma(v0[k].x, uu[k].x, acc0);
                acc0 = fma(v0[k].y, uu[k].y, acc0);
                acc1 = fma(v1[k].x, uu[k].x, acc1);
                acc1 = fma(v1[k].y, uu[k].y, acc1);
            }
        }
        if (stream) {
            acc0 = wave_sum(acc0);
            acc1 = wave_sum(acc1);
        }
        if (s0 >= 0) acc0 = readlane_f64(svl, (int)(ja - j0)) * reinterpret_cast<const double *>(s_u)[s0];
        if (s1 >= 0) acc1 = readlane_f64(svl, (int)(jb - j0)) * reinterpret_cast<const double *>(s_u)[s1];
        if (lane < ncol) {
            const double dot = lane == 0 ? acc0 : acc1;
            const int64_t jj = j + lane;
            const int nb = nb_pre;
            const double rj = cd_pre - dot;
            double key = -INFINITY;
            if (rj != rj) st->nan_flag = 1;
            else key = primal_key(rj, nb, a.p.eps);
            a.p.xc.r(jj) = rj;
            a.p.xc.key(jj) = key;
            best = fmax(best, key);
        }
    }
    if (use_vs && wave == 0 && j0 + lane < j1) a.pos_hint[j0 + lane] = sgl >= 0 ? 1 : 0;  // for the next launch's prefetch
    double v = (lane < 2) ? best : -INFINITY;
    v = fmax(v, __shfl_xor(v, 1));
    if (lane == 0) s_k[wave] = v;
    __syncthreads();
    if (tid == 0) a.p.xc.bk(gb) = fmax(fmax(s_k[0], s_k[1]), fmax(s_k[2], s_k[3]));
}

// Maintenance replaces the inverse an open iteration was decided with: the iteration is dropped (its
// eta-update half is already in B^-1, its pricing is simply redone) and, having been counted when
// k_ftran_eta entered it, un-counted.
__global__ void k_drop_open(DevState *st) {
    if (st->status != ST_RUNNING && st->status != ST_NEED_MAINT) return;
    if (st->open) {
        st->open = 0;
        st->iters -= 1;
    }
}

// ------------------------------------------------------------------ F: entering fold + eta update + FTRAN
struct FtranEtaArgs {
    double *W0, *W1;
    const double *A_N;
    Xchg xc;
    const int64_t *N_index, *B_index;
    const uint8_t *Nb, *kind;
    const double *x, *lb, *ub;
    double *d, *lam, *bmin, *bsec;
    int32_t *bidx, *binfo;
    uint8_t *dpos;
    double *A_B, *c_B;
    const double *aq_save;
    // column-sharded engines: the entering column comes from the gathered packs — chosen HERE, in every block's prologue
    // (sel_packs; shard_select_wave instead of the entering fold), or by k_sh_select after a full exchange (sel_packs null,
    // aq_cur set: position in st->sh_q, column in aq_cur).  Block 0 leaves the column in aq_out for the next k_price2.
    const double *sel_packs, *aq_cur;
    double *aq_out;
    int sel_world, mbox_commit;
    DevState *st;
    int64_t m, ld, nN;
    int nblocks, cpb, rows_per_block;
    double eps;
};

// rows [row0, row0 + nrows) (nrows <= 4), streamed: dst = E src (if `apply`), acc[k] += new row . a_q
__device__ __forceinline__ void eta_ftran_rows_stream(const double *src, double *dst, const double2 *col, bool have_col,
                                                      int64_t m, int64_t ld, bool apply, int64_t r, const double dv[UPD_ROWS],
                                                      double d_r, double alpha_r, int64_t row0, int nrows, int tid,
                                                      double acc0[UPD_ROWS], double acc1[UPD_ROWS]) {
    const int64_t half = ld >> 1;
    const double2 *rho2 = reinterpret_cast<const double2 *>(src + (apply ? r : 0) * ld);
    double f[UPD_ROWS];
    int64_t ii[UPD_ROWS];
#pragma unroll
    for (int k = 0; k < UPD_ROWS; ++k) {
        const int64_t i = row0 + k;
        const bool ok = i < m && k < nrows;
        ii[k] = ok ? i : -1;
        f[k] = (ok && apply && i != r) ? -(dv[k] / d_r) : 0.0;
    }
    for (int64_t t = tid; t < half; t += 256) {
        const double2 p = apply ? rho2[t] : make_double2(0.0, 0.0);
        const double2 c = have_col ? col[t] : make_double2(0.0, 0.0);
        double2 w[UPD_ROWS];
#pragma unroll
        for (int k = 0; k < UPD_ROWS; ++k)
            if (ii[k] >= 0) w[k] = reinterpret_cast<const double2 *>(src + ii[k] * ld)[t];
#pragma unroll
        for (int k = 0; k < UPD_ROWS; ++k) {
            if (ii[k] < 0) continue;
            double2 o = w[k];
            if (apply) {
                if (ii[k] == r) {
                    o = make_double2(p.x / alpha_r, p.y / alpha_r);
                } else {
                    o.x = fma(f[k], p.x, w[k].x);
                    o.y = fma(f[k], p.y, w[k].y);
                }
                store_row2<true>(reinterpret_cast<double2 *>(dst + ii[k] * ld) + t, o);
            }
            acc0[k] = fma(o.x, c.x, acc0[k]);
            acc1[k] = fma(o.y, c.y, acc1[k]);
        }
    }
}

// NR = double2 per thread per row held in registers for the block's first UPD_ROWS rows (ceil(ld/512));
// NR == 0: all rows are streamed after the fold.
// Every wave folds, stores and reduces in the same order: the body of the sharded instantiations, of NR == 0 and of NR == 8
// (the unsharded NR = 1, 2, 4 run ftran_eta_handoff below).
template <int NR, bool SH>
__device__ __forceinline__ void ftran_eta_whole(const FtranEtaArgs &a) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ long long s_q;
    __shared__ double s_wk[4];
    __shared__ int s_nh, s_band;
    __shared__ int s_hblk[FC_SLOTS];
    __shared__ double s_hkey[FC_SLOTS * 64];
    __shared__ int32_t s_hidx[FC_SLOTS * 64];
    __shared__ double s_dot[4][2 * UPD_ROWS];
    __shared__ double s_lam[2 * UPD_ROWS];
    __shared__ int s_dp[2 * UPD_ROWS];
    DevState *st = a.st;
    if (st->status != ST_RUNNING) return;
    STAMP(1, 0);  // -DELLP_DBG_STAMPS builds (tools/stamps.py): 0 entry, 5 block maxima staged, 6 candidates chosen, 7 their keys here,
                  // 1 q known, 2 eta stores issued, 3 dot products reduced, 4 end
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nan_flag = st->nan_flag;
    const int src_sel = st->f_src;
    const int apply = st->pe_valid;
    const int64_t r = st->pe_r;
    const double d_r = st->pe_d_r, alpha_r = st->pe_alpha_r;
    const double *src = src_sel ? a.W1 : a.W0;
    double *dst = src_sel ? a.W0 : a.W1;
    const int64_t half = a.ld >> 1, m = a.m;
    constexpr int NBK = 1;
    const bool row_block = blockIdx.x >= NBK;
    const int R = a.rows_per_block;
    const int64_t row0 = ((int64_t)blockIdx.x - NBK) * R;

    // ---- staging loads of the entering fold first, then everything that does not depend on q
    double *s_bk = reinterpret_cast<double *>(smem);
    double tmax = -INFINITY;
    double v0[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int b = tid + 256 * u;
        const double t = a.xc.bk(b < a.nblocks ? b : 0);
        v0[u] = b < a.nblocks ? t : -INFINITY;
    }
    // threads 0..R-1 own the lambda_i of the block's rows: their gathers hang off B_index
    const int64_t myrow = row0 + tid;
    const bool own = row_block && tid < R && myrow < m;
    const int64_t bi0 = a.B_index[own ? myrow : 0];
    __builtin_amdgcn_sched_barrier(0);
    double dv[UPD_ROWS], dv2[UPD_ROWS];
#pragma unroll
    for (int k = 0; k < UPD_ROWS; ++k) {
        dv[k] = (row_block && k < R && row0 + k < m) ? a.d[row0 + k] : 0.0;
        dv2[k] = (row_block && UPD_ROWS + k < R && row0 + UPD_ROWS + k < m) ? a.d[row0 + UPD_ROWS + k] : 0.0;
    }
    constexpr int NRR = NR > 0 ? NR : 1;
    double2 wreg[UPD_ROWS][NRR];
    if (NR > 0) {
#pragma unroll
        for (int k = 0; k < UPD_ROWS; ++k) {
            const int64_t i = row0 + k;
            const bool ok = row_block && k < R && i < m;
            const double2 *srow = reinterpret_cast<const double2 *>(src + (ok ? i : 0) * a.ld);
#pragma unroll
            for (int u = 0; u < NR; ++u) {
                const int64_t t = tid + 256 * u;
                const double2 wv = srow[t < half ? t : 0];
                wreg[k][u] = (ok && t < half) ? wv : make_double2(0.0, 0.0);
            }
        }
    }
    // the pivot row of the eta update is known from the state (it does NOT hang off the entering fold):
    // fetch it with the rows, so that the updated rows can be stored as soon as the fold lets go of the
    // block, before the entering column has even been requested
    // (measured: config 5, NR = 8: 60 -> 51 us; config 3, NR = 4: 15.7 -> 16.9 us, so only from NR = 8)
    constexpr bool EARLY = NR >= 8;
    double2 pr[NRR];
    if (EARLY) {
        const double2 *rho2 = reinterpret_cast<const double2 *>(src + (apply ? r : 0) * a.ld);
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            const int64_t t = tid + 256 * u;
            const double2 pv = rho2[t < half ? t : 0];
            pr[u] = (apply && t < half) ? pv : make_double2(0.0, 0.0);
        }
    }
    const double xi0 = a.x[bi0], lbi0 = a.lb[bi0], ubi0 = a.ub[bi0];
    const int k0 = a.kind[bi0];
    const double *sel_packs = SH ? a.sel_packs : nullptr, *aq_in = SH ? a.aq_cur : nullptr;
    if (SH) {
        if (sel_packs) {
            if (wave == 0) {
                const WaveSelect ws = shard_select_wave(sel_packs, a.sel_world, a.ld, a.eps, lane);
                if (lane == 0) {
                    s_q = ws.verdict ? -2 : ws.q;
                    s_nh = ws.src_rank;
                    s_band = ws.src_c;
                }
            }
            lds_barrier();
            if (blockIdx.x == 0 && tid == 0) {
                if (a.mbox_commit) st->mbox_gen += 1;  // the packs have been consumed (also when they were not conclusive)
                if (s_q == -2) st->status = ST_NEED_FULL;
            }
            if (s_q == -2) return;  // nothing of this launch has been stored: it is enqueued again behind the full exchange
        } else {
            if (tid == 0) s_q = st->sh_q;
            lds_barrier();
        }
    } else {
    // ---- entering fold (same code path as k_ftran2<0>)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (tid + 256 * u < a.nblocks) s_bk[tid + 256 * u] = v0[u];
        tmax = fmax(tmax, v0[u]);
    }
    for (int b0 = tid + 4 * 256; b0 < a.nblocks; b0 += 4 * 256) {
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int b = b0 + 256 * u;
            const double t = a.xc.bk(b < a.nblocks ? b : 0);
            v[u] = b < a.nblocks ? t : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (b0 + 256 * u < a.nblocks) s_bk[b0 + 256 * u] = v[u];
            tmax = fmax(tmax, v[u]);
        }
    }
    if (tid == 0) {
        s_nh = 0;
        s_band = 0;
    }
    tmax = wave_allmax_dpp(tmax);  // DPP butterfly + readlane (no NaN here: keys are never NaN)
    if (lane == 0) s_wk[wave] = tmax;
    lds_barrier();
    STAMP(1, 5);
    const double M = fmax(fmax(s_wk[0], s_wk[1]), fmax(s_wk[2], s_wk[3]));
    for (int b = tid; b < a.nblocks; b += 256) {
        const double v = s_bk[b];
        if (M - v < 4.0 * a.eps) {
            const int slot = atomicAdd(&s_nh, 1);
            if (slot < FC_SLOTS) s_hblk[slot] = b;
        } else if (M - v < 6.0 * a.eps) {
            s_band = 1;
        }
    }
    lds_barrier();
    STAMP(1, 6);
    const int nh = s_nh;
    const bool fast = M > -INFINITY && nh <= FC_SLOTS && !s_band;
    if (fast) {
        if (tid == 0) {
            for (int i = 1; i < nh; ++i) {
                const int v = s_hblk[i];
                int j = i - 1;
                while (j >= 0 && s_hblk[j] > v) {
                    s_hblk[j + 1] = s_hblk[j];
                    --j;
                }
                s_hblk[j + 1] = v;
            }
        }
        lds_barrier();
        for (int sl = wave; sl < nh; sl += 4) {
            const int64_t j = (int64_t)s_hblk[sl] * a.cpb + lane;
            const bool ok = lane < a.cpb && j < a.nN;
            const int64_t jc = ok ? j : 0;
            const double kl = a.xc.key(jc);
            const int64_t il = a.N_index[jc];
            const double kv = ok ? kl : -INFINITY;
            s_hkey[sl * 64 + lane] = kv;
            s_hidx[sl * 64 + lane] = ok ? (int32_t)il : 0;
            if (M - kv < 6.0 * a.eps && !(M - kv < 4.0 * a.eps)) s_band = 1;
        }
        lds_barrier();
        STAMP(1, 7);
    }
    if (wave == 0) {
        long long q = -1;
        bool done = false;
        if (fast && !s_band) {
            FoldState f{false, 0.0, 0, -1};
            for (int sl = 0; sl < nh; ++sl)
                fold_elements(f, s_hkey[sl * 64 + lane], s_hidx[sl * 64 + lane], (int64_t)s_hblk[sl] * a.cpb, a.eps, lane);
            q = f.qacc;
            done = true;
        }
        if (!done && M > -INFINITY) q = entering_fold_full(s_bk, a.nblocks, a.cpb, a.nN, a.xc, a.N_index, a.eps, lane);
        if (lane == 0) s_q = q;
    }
    lds_barrier();
    }
    const long long q = s_q;
    STAMP(1, 1);
    if (nan_flag) {  // fatal: nothing of this engine is used afterwards
        if (blockIdx.x == 0 && tid == 0) st->status = ELLP_ERR_NAN;
        return;
    }
    const bool have_col = q >= 0;
    const int at_lower = have_col ? (a.Nb[q] == ELLP_NB_LOWER ? 1 : 0) : 0;
    const double sgn = at_lower ? -1.0 : 1.0;
    const double *sel_rec = (SH && sel_packs && have_col)
                                ? sel_packs + (int64_t)s_nh * pack_doubles(a.ld) + SH_HDR + (int64_t)s_band * (SH_REC + a.ld)
                                : nullptr;  // the winner's record: key, N.index, position, r_q, then its column
    const double2 *col = reinterpret_cast<const double2 *>(sel_rec ? sel_rec + SH_REC : (aq_in ? aq_in : a.A_N + (have_col ? q : 0) * a.ld));

    if (row_block) {
        double acc0[2 * UPD_ROWS], acc1[2 * UPD_ROWS];
#pragma unroll
        for (int k = 0; k < 2 * UPD_ROWS; ++k) acc0[k] = acc1[k] = 0.0;
        if (NR > 0) {
            double2 cq[NRR];
            if (!EARLY) {  // pivot row and entering column in one round trip
                const double2 *rho2 = reinterpret_cast<const double2 *>(src + (apply ? r : 0) * a.ld);
#pragma unroll
                for (int u = 0; u < NR; ++u) {
                    const int64_t t = tid + 256 * u;
                    const int64_t tc = t < half ? t : 0;
                    const double2 pv = rho2[tc];
                    const double2 cv = col[tc];
                    pr[u] = (apply && t < half) ? pv : make_double2(0.0, 0.0);
                    cq[u] = (have_col && t < half) ? cv : make_double2(0.0, 0.0);
                }
            }
            // eta update of the register-held rows: store them now, keep the new values for the dot products
            if (apply) {
#pragma unroll
                for (int k = 0; k < UPD_ROWS; ++k) {
                    const int64_t i = row0 + k;
                    if (!(k < R && i < m)) continue;
                    const double f = (i != r) ? -(dv[k] / d_r) : 0.0;
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
                        wreg[k][u] = o;
                    }
                }
            }
            STAMP(1, 2);
            if (EARLY) {
#pragma unroll
                for (int u = 0; u < NR; ++u) {
                    const int64_t t = tid + 256 * u;
                    const double2 cv = col[t < half ? t : 0];
                    cq[u] = (have_col && t < half) ? cv : make_double2(0.0, 0.0);
                }
            }
#pragma unroll
            for (int k = 0; k < UPD_ROWS; ++k) {
                const int64_t i = row0 + k;
                if (!(k < R && i < m)) continue;
#pragma unroll
                for (int u = 0; u < NR; ++u) {
                    acc0[k] = fma(wreg[k][u].x, cq[u].x, acc0[k]);
                    acc1[k] = fma(wreg[k][u].y, cq[u].y, acc1[k]);
                }
            }
        } else {
            eta_ftran_rows_stream(src, dst, col, have_col, m, a.ld, apply != 0, r, dv, d_r, alpha_r, row0, R < UPD_ROWS ? R : UPD_ROWS,
                                  tid, acc0, acc1);
        }
        if (R > UPD_ROWS)
            eta_ftran_rows_stream(src, dst, col, have_col, m, a.ld, apply != 0, r, dv2, d_r, alpha_r, row0 + UPD_ROWS, R - UPD_ROWS, tid,
                                  acc0 + UPD_ROWS, acc1 + UPD_ROWS);
        if (have_col) {
            // ---- d_i = +-(row . a_q): wave sums, then the four waves in a fixed order
#pragma unroll
            for (int k = 0; k < 2 * UPD_ROWS; ++k) {
                const double s = wave_sum(acc0[k] + acc1[k]);
                if (lane == 0) s_dot[wave][k] = s;
            }
            __syncthreads();
            STAMP(1, 3);
            double li = INFINITY;
            if (own) {
                const int k = tid;
                const double di = sgn * (((s_dot[0][k] + s_dot[1][k]) + s_dot[2][k]) + s_dot[3][k]);
                const double xi = xi0, lbi = lbi0, ubi = ubi0;
                a.d[myrow] = di;
                li = primal_lambda(di, xi, lbi, ubi, k0, a.eps);  // primal…:320-367
                if (li != li) st->nan_flag = 1;
                a.lam[myrow] = li;
                a.bidx[myrow] = (int32_t)bi0;
                a.dpos[myrow] = di > 0.0 ? 1 : 0;
            }
            if (tid < 2 * UPD_ROWS) {
                s_lam[tid] = li;
                s_dp[tid] = own ? (a.dpos[myrow] ? 1 : 0) : 0;
            }
            __syncthreads();
            if (tid == 0) {  // smallest and second smallest lambda of the block, and whose the smallest is
                double m1 = INFINITY, m2 = INFINITY;
                int info = -1;
                for (int k = 0; k < R; ++k) {
                    const double v = s_lam[k];
                    if (v < m1) {
                        m2 = m1;
                        m1 = v;
                        info = (int)(2 * (row0 + k)) + s_dp[k];
                    } else if (v < m2) {
                        m2 = v;
                    }
                }
                a.bmin[blockIdx.x - NBK] = m1;
                a.bsec[blockIdx.x - NBK] = m2;
                a.binfo[blockIdx.x - NBK] = info;
            }
            STAMP(1, 4);
        }
        return;
    }
    // ---------------- block 0: the deferred half of the column move, then the commit of this iteration
    if (SH && sel_rec) {  // column-sharded: the next k_price2 (and a closing k_update2) take the entering column from aq_cur
        double2 *dstc = reinterpret_cast<double2 *>(a.aq_out);
        for (int64_t t = tid; t < half; t += 256) dstc[t] = col[t];
    }
    if (st->mv_pending) {
        const int64_t mr = st->mv_r;
        double2 *cb = reinterpret_cast<double2 *>(a.A_B + mr * a.ld);
        const double2 *sv = reinterpret_cast<const double2 *>(a.aq_save);
        for (int64_t t = tid; t < half; t += 256) cb[t] = sv[t];
        if (tid == 0) a.c_B[mr] = st->cq_save;
    }
    if (tid == 0) {
        const int new_cur = apply ? (src_sel ^ 1) : src_sel;
        if (st->tiny_p) {  // raised by k_price2's bookkeeping (a tiny pivot): now it may stop the next launch
            st->tiny_p = 0;
            st->tiny = 1;
        }
        st->mv_pending = 0;
        st->cur = new_cur;
        st->usel = st->usel_next;
        st->s_cur = new_cur;
        st->iters += 1;  // a loop body is entered (primal…:163-168); its ratio test is folded by the next kernel
        st->open = q < 0 ? 0 : 1;
        if (q < 0) {  // primal…:289-292; the status itself is written by the next kernel's leader
            st->fin = ELLP_OPTIMAL + 1;
        } else {
            const int64_t jq = a.N_index[q];
            ELLP_CHECK(st, q < a.nN, 9111);
            st->s_q = q;
            st->s_at_lower = at_lower;
            st->s_nbq = a.Nb[q];
            st->s_jq = jq;
            st->s_rq = sel_rec ? sel_rec[3] : (aq_in ? st->sh_rq : a.xc.r(q));
            const int kk = a.kind[jq];  // primal…:305-311
            st->s_lambda0 = (kk == ELLP_BOUND_TWOSIDED) ? a.ub[jq] - a.lb[jq] : (kk == ELLP_BOUND_FIXED ? 0.0 : INFINITY);
        }
    }
}

// ------------------------------------------------------------------ F, unsharded, rows in registers: one wave decides, four stream
// A wave has ONE outstanding-memory counter for loads and stores.  A wave that has row stores in flight and then consumes a
// global load therefore waits for its own store burst to be acknowledged.  So the work of a row block is divided among the
// five waves of a 320-thread block:
//   wave 0      owns no row and stores none: it folds alone (same functions, same values), reads Nb[q], fetches the entering
//               column and leaves column, q and the sign in LDS; after the last barrier it writes the block's tail;
//   waves 1..4  load a quarter of the rows and of the pivot row each, store the updated rows as soon as those are there, and
//               take q and the column from LDS at the hand-off barrier.
// Rule for every wave: between its first row store and the end of the kernel it consumes no global load.
// The arithmetic is that of ftran_eta_whole: the same fmas on the same operands in the same order, thread 64 + s owns the
// columns thread s owns there, every row keeps its butterfly order and the four streaming waves their order
// ((s0 + s1) + s2) + s3.
constexpr int FTRAN_HAND_THREADS = 320;

// the lanes of one wave run in lockstep: what one lane wrote to LDS is there for the others once the wave's LDS traffic retired
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// a use the compiler cannot move: the wait for the load behind `v` stands HERE and not at a later first use
template <class T>
__device__ __forceinline__ void retire_here(T &v) { asm volatile("" : "+v"(v)); }
// byte offset of the entering column behind the staged block maxima in the dynamic LDS of k_ftran_eta
__host__ __device__ constexpr size_t ftran_col_offset(int nblocks) { return (sizeof(double) * (size_t)nblocks + 16 + 15) & ~(size_t)15; }

// K rows reduced together: every step issues all K exchanges before it waits for one; each row's order is wave_sum's
template <int K>
__device__ __forceinline__ void wave_sum_rows(double s[UPD_ROWS]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        double t[K];
#pragma unroll
        for (int k = 0; k < K; ++k) t[k] = __shfl_xor(s[k], o);
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] += t[k];
    }
}

template <int NR>
__device__ __forceinline__ void ftran_eta_handoff(const FtranEtaArgs &a) {
    static_assert(NR >= 1 && NR <= 4, "rows of at most 2,048 doubles: at most UPD_ROWS rows per block");
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ long long s_q;
    __shared__ int s_leave, s_atl, s_nh, s_band;
    __shared__ int s_hblk[FC_SLOTS];
    __shared__ double s_hkey[FC_SLOTS * 64];
    __shared__ int32_t s_hidx[FC_SLOTS * 64];
    __shared__ double s_dot[4][UPD_ROWS];
    __shared__ double s_lam[UPD_ROWS];
    __shared__ int s_dp[UPD_ROWS];
    DevState *st = a.st;
    STAMP(1, 0);  // -DELLP_DBG_STAMPS builds (tools/stamps.py): 0 entry, 5 block maxima staged, 6 candidates chosen, 1 q known,
                  // 7 column published (all wave 0), 2 stores of the first streaming wave issued (thread 64), 3 dot products
                  // reduced, 4 end (wave 0)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int sid = tid - 64;  // streaming waves: thread 64 + s owns double2 columns s + 256 u of the block's rows
    // the ways out that do not depend on q, decided ONCE per block (another block of this launch may raise nan_flag meanwhile)
    if (tid == 0) s_leave = st->status != ST_RUNNING ? 1 : (st->nan_flag ? 2 : 0);
    const int src_sel = st->f_src;
    const int apply = st->pe_valid;
    const int64_t r = st->pe_r;
    const double d_r = st->pe_d_r, alpha_r = st->pe_alpha_r;
    const double *src = src_sel ? a.W1 : a.W0;
    double *dst = src_sel ? a.W0 : a.W1;
    const int64_t half = a.ld >> 1, m = a.m;
    constexpr int NBK = 1;
    const bool row_block = blockIdx.x >= NBK;
    const int R = a.rows_per_block;  // <= UPD_ROWS: eight rows per block start at m = 3,072, NR <= 4 ends at ld = 2,048
    const int64_t row0 = ((int64_t)blockIdx.x - NBK) * R;
    double *s_bk = reinterpret_cast<double *>(smem);
    double2 *s_col = reinterpret_cast<double2 *>(smem + ftran_col_offset(a.nblocks));

    // ---- every global value a wave will ever need, requested at entry.  Wave 0: the block maxima of the fold first
    constexpr int FB = 16;  // block maxima per lane held in registers across the row loads (1,024 pricing blocks)
    double v0[FB];  // as loaded: every select on a loaded value waits where its branch is taken up again, not here
    // threads 0..R-1 (in wave 0) own the lambda_i of the block's rows: their gathers hang off B_index
    const int64_t myrow = row0 + tid;
    const bool own = row_block && tid < R && myrow < m;
    int64_t bi0 = 0;
    double xi0 = 0.0, lbi0 = 0.0, ubi0 = 0.0;
    int k0 = 0;
    // streaming waves: the previous d, rows and pivot row as loaded (clamped addresses): what lies outside the block's rows
    // or beyond the row's end is never stored, and reaches the dot products as zero
    double dv[UPD_ROWS];
    double2 wreg[UPD_ROWS][NR], pr[NR];

    // eta update of this thread's columns of the block's rows: store them, keep the new values for the dot products
    auto eta_store = [&]() {
        if (!apply) return;
#pragma unroll
        for (int k = 0; k < UPD_ROWS; ++k) {
            const int64_t i = row0 + k;
            if (!(k < R && i < m)) continue;
            const double f = (i != r) ? -(dv[k] / d_r) : 0.0;
            double2 *drow = reinterpret_cast<double2 *>(dst + i * a.ld);
#pragma unroll
            for (int u = 0; u < NR; ++u) {
                const int64_t t = sid + 256 * u;
                if (t >= half) continue;
                double2 o;
                if (i == r) {
                    o = make_double2(pr[u].x / alpha_r, pr[u].y / alpha_r);
                } else {
                    o.x = fma(f, pr[u].x, wreg[k][u].x);
                    o.y = fma(f, pr[u].y, wreg[k][u].y);
                }
                store_row2<true>(drow + t, o);
                wreg[k][u] = o;
            }
        }
    };

    // the wait for rows and pivot row stands in front of a wave's first store, whole: a counted wait for a load between
    // two stores waits for the older store as well
    auto rows_retired = [&]() {
#pragma unroll
        for (int k = 0; k < UPD_ROWS; ++k) {
            retire_here(dv[k]);
#pragma unroll
            for (int u = 0; u < NR; ++u) {
                retire_here(wreg[k][u].x);
                retire_here(wreg[k][u].y);
            }
        }
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            retire_here(pr[u].x);
            retire_here(pr[u].y);
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), as an instruction the compiler's own wait insertion accounts for
    };

    // block 0 behind the hand-off, all five waves: the deferred half of the column move
    auto block0_move = [&]() {
        if (!st->mv_pending) return;
        const int64_t mr = st->mv_r;
        double2 *cb = reinterpret_cast<double2 *>(a.A_B + mr * a.ld);
        const double2 *sv = reinterpret_cast<const double2 *>(a.aq_save);
        for (int64_t t = tid; t < half; t += FTRAN_HAND_THREADS) cb[t] = sv[t];
        if (tid == 0) a.c_B[mr] = st->cq_save;
    };

    // The two roles are two branches from entry to the kernel's end, each with the block's three barriers in it, so that
    // neither carries the other's registers (the rows are not live across the fold, the fold's staging not across the row
    // loads) and neither inherits a wait for what the other has in flight.
    if (wave == 0) {
        const double *pb[FB];
#pragma unroll
        for (int u = 0; u < FB; ++u) {
            const int b = lane + 64 * u;
            pb[u] = &a.xc.bk(b < a.nblocks ? b : 0);
        }
        __builtin_amdgcn_sched_barrier(0);  // all addresses, then all loads: one round trip
#pragma unroll
        for (int u = 0; u < FB; ++u) v0[u] = *pb[u];
        bi0 = a.B_index[own ? myrow : 0];
        lds_barrier();  // the entry barrier: every wave of the block arrives at its own, nothing above leaves the kernel
        const int leave = s_leave;
        if (leave) {  // block-uniform (LDS): the streaming waves leave at theirs.  Nothing of this launch has been stored
            if (leave == 2 && blockIdx.x == 0 && tid == 0) st->status = ELLP_ERR_NAN;  // fatal: nothing of this engine is used afterwards
            return;
        }
        // the gathers of the lambda owners (threads 0..R-1 are this wave's): issued here, in no other wave's path
        xi0 = a.x[bi0];
        lbi0 = a.lb[bi0];
        ubi0 = a.ub[bi0];
        k0 = a.kind[bi0];
        // ---- the entering fold, by this wave alone: lockstep lanes and wave_lds_sync() stand where the block's barriers stood
        double tmax = -INFINITY;
#pragma unroll
        for (int u = 0; u < FB; ++u) {
            const bool in = lane + 64 * u < a.nblocks;
            if (in) s_bk[lane + 64 * u] = v0[u];
            tmax = fmax(tmax, in ? v0[u] : -INFINITY);
        }
        for (int b0 = lane + 64 * FB; b0 < a.nblocks; b0 += 64 * FB) {
            double v[FB];
#pragma unroll
            for (int u = 0; u < FB; ++u) {
                const int b = b0 + 64 * u;
                const double t = a.xc.bk(b < a.nblocks ? b : 0);
                v[u] = b < a.nblocks ? t : -INFINITY;
            }
#pragma unroll
            for (int u = 0; u < FB; ++u) {
                if (b0 + 64 * u < a.nblocks) s_bk[b0 + 64 * u] = v[u];
                tmax = fmax(tmax, v[u]);
            }
        }
        if (lane == 0) {
            s_nh = 0;
            s_band = 0;
        }
        const double M = wave_allmax_dpp(tmax);  // DPP butterfly + readlane (no NaN here: keys are never NaN)
        wave_lds_sync();
        STAMP(1, 5);
        for (int b = lane; b < a.nblocks; b += 64) {
            const double v = s_bk[b];
            if (M - v < 4.0 * a.eps) {
                const int slot = atomicAdd(&s_nh, 1);
                if (slot < FC_SLOTS) s_hblk[slot] = b;
            } else if (M - v < 6.0 * a.eps) {
                s_band = 1;
            }
        }
        wave_lds_sync();
        STAMP(1, 6);
        const int nh = s_nh;
        const bool fast = M > -INFINITY && nh <= FC_SLOTS && !s_band;
        if (fast) {
            if (lane == 0) {
                for (int i = 1; i < nh; ++i) {
                    const int v = s_hblk[i];
                    int j = i - 1;
                    while (j >= 0 && s_hblk[j] > v) {
                        s_hblk[j + 1] = s_hblk[j];
                        --j;
                    }
                    s_hblk[j + 1] = v;
                }
            }
            wave_lds_sync();
            for (int sl = 0; sl < nh; ++sl) {
                const int64_t j = (int64_t)s_hblk[sl] * a.cpb + lane;
                const bool ok = lane < a.cpb && j < a.nN;
                const int64_t jc = ok ? j : 0;
                const double kl = a.xc.key(jc);
                const int64_t il = a.N_index[jc];
                const double kv = ok ? kl : -INFINITY;
                s_hkey[sl * 64 + lane] = kv;
                s_hidx[sl * 64 + lane] = ok ? (int32_t)il : 0;
                if (M - kv < 6.0 * a.eps && !(M - kv < 4.0 * a.eps)) s_band = 1;
            }
            wave_lds_sync();
        }
        long long q = -1;
        bool done = false;
        if (fast && !s_band) {
            FoldState f{false, 0.0, 0, -1};
            for (int sl = 0; sl < nh; ++sl)
                fold_elements(f, s_hkey[sl * 64 + lane], s_hidx[sl * 64 + lane], (int64_t)s_hblk[sl] * a.cpb, a.eps, lane);
            q = f.qacc;
            done = true;
        }
        if (!done && M > -INFINITY) q = entering_fold_full(s_bk, a.nblocks, a.cpb, a.nN, a.xc, a.N_index, a.eps, lane);
        STAMP(1, 1);
        // ---- Nb[q] and the column in one round trip; the column goes to LDS for all four waves
        const bool hc = q >= 0;
        int nbq = a.Nb[hc ? q : 0];
        if (row_block && hc) {
            const double2 *col = reinterpret_cast<const double2 *>(a.A_N + q * a.ld);
            double2 cv[4 * NR];
#pragma unroll
            for (int u = 0; u < 4 * NR; ++u) {
                const int64_t t = lane + 64 * u;
                cv[u] = col[t < half ? t : 0];
            }
            __builtin_amdgcn_sched_barrier(0);  // all loads, one wait, then the LDS writes: not a round trip per element
#pragma unroll
            for (int u = 0; u < 4 * NR; ++u) {
                retire_here(cv[u].x);
                retire_here(cv[u].y);
            }
#pragma unroll
            for (int u = 0; u < 4 * NR; ++u) {
                const int64_t t = lane + 64 * u;
                if (t < half) s_col[t] = cv[u];
            }
        }
        // every load of this wave is retired here, ahead of the barrier and of its stores
        retire_here(nbq);
        retire_here(xi0);
        retire_here(lbi0);
        retire_here(ubi0);
        retire_here(k0);
        if (lane == 0) {
            s_q = q;
            s_atl = hc ? (nbq == ELLP_NB_LOWER ? 1 : 0) : 0;
        }
        STAMP(1, 7);
    } else {
        // ---- streaming waves: every global value they will ever need, requested at entry
#pragma unroll
        for (int k = 0; k < UPD_ROWS; ++k) dv[k] = (row_block && k < R && row0 + k < m) ? a.d[row0 + k] : 0.0;
#pragma unroll
        for (int k = 0; k < UPD_ROWS; ++k) {
            const int64_t i = row0 + k;
            const bool ok = row_block && k < R && i < m;
            const double2 *srow = reinterpret_cast<const double2 *>(src + (ok ? i : 0) * a.ld);
#pragma unroll
            for (int u = 0; u < NR; ++u) {
                const int64_t t = sid + 256 * u;
                wreg[k][u] = srow[t < half ? t : 0];
            }
        }
        {  // the pivot row of the eta update is known from the state: it comes with the rows
            const double2 *rho2 = reinterpret_cast<const double2 *>(src + (apply ? r : 0) * a.ld);
#pragma unroll
            for (int u = 0; u < NR; ++u) {
                const int64_t t = sid + 256 * u;
                pr[u] = rho2[t < half ? t : 0];
            }
        }
        lds_barrier();  // the entry barrier
        if (s_leave) return;  // block-uniform (LDS): wave 0 leaves at its own
        // the update needs rows, rho and the previous d only, nothing the fold produces: retire them once, store at once
        rows_retired();
        if (row_block) {
            eta_store();
            STAMP_AT(1, 2, 64);
        }
        lds_barrier();  // the hand-off (below): LDS traffic only, the stores stay in flight across it
        if (!row_block) {
            block0_move();
            return;
        }
        if (s_q < 0) return;  // block-uniform: LDS
        // ---- d_i = +-(row . a_q), a_q from LDS: wave sums, then the four streaming waves in a fixed order
        double acc0[UPD_ROWS], acc1[UPD_ROWS];
#pragma unroll
        for (int k = 0; k < UPD_ROWS; ++k) acc0[k] = acc1[k] = 0.0;
        double2 cq[NR];
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            const int64_t t = sid + 256 * u;
            const double2 cv = s_col[t < half ? t : 0];
            cq[u] = t < half ? cv : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int k = 0; k < UPD_ROWS; ++k) {
            const int64_t i = row0 + k;
            if (!(k < R && i < m)) continue;
#pragma unroll
            for (int u = 0; u < NR; ++u) {
                const bool in = sid + 256 * u < half;
                acc0[k] = fma(in ? wreg[k][u].x : 0.0, cq[u].x, acc0[k]);
                acc1[k] = fma(in ? wreg[k][u].y : 0.0, cq[u].y, acc1[k]);
            }
        }
        double s[UPD_ROWS];
#pragma unroll
        for (int k = 0; k < UPD_ROWS; ++k) s[k] = acc0[k] + acc1[k];
        // only the R rows the block has (1, 2 or 4), step by step together
        if (R >= 3) wave_sum_rows<4>(s);
        else if (R == 2) wave_sum_rows<2>(s);
        else wave_sum_rows<1>(s);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < UPD_ROWS; ++k) s_dot[wave - 1][k] = s[k];
        }
        lds_barrier();  // the last barrier (below); nothing follows it here: the rest is wave 0's own
        return;
    }
    // ---- wave 0 from here on; each barrier below is the one the streaming waves meet at the same point of their branch.
    // The hand-off.  Every wave that passed its entry barrier reaches it: the only way out in between is `leave`, read from
    // LDS after that barrier and therefore the same in all five waves, and nothing above returns, whatever the fold found
    // (q < 0 included: the optimal end still applies the eta update in the streaming waves).
    lds_barrier();
    const long long q = s_q;
    const bool have_col = q >= 0;  // block-uniform: LDS
    const int at_lower = s_atl;

    if (!row_block) {
        // ---------------- block 0: the deferred half of the column move, then the commit of this iteration
        block0_move();
        if (tid == 0) {
            const int new_cur = apply ? (src_sel ^ 1) : src_sel;
            if (st->tiny_p) {  // raised by k_price2's bookkeeping (a tiny pivot): now it may stop the next launch
                st->tiny_p = 0;
                st->tiny = 1;
            }
            st->mv_pending = 0;
            st->cur = new_cur;
            st->usel = st->usel_next;
            st->s_cur = new_cur;
            st->iters += 1;  // a loop body is entered (primal…:163-168); its ratio test is folded by the next kernel
            st->open = q < 0 ? 0 : 1;
            if (q < 0) {  // primal…:289-292; the status itself is written by the next kernel's leader
                st->fin = ELLP_OPTIMAL + 1;
            } else {
                const int64_t jq = a.N_index[q];
                ELLP_CHECK(st, q < a.nN, 9111);
                st->s_q = q;
                st->s_at_lower = at_lower;
                st->s_nbq = a.Nb[q];
                st->s_jq = jq;
                st->s_rq = a.xc.r(q);
                const int kk = a.kind[jq];  // primal…:305-311
                st->s_lambda0 = (kk == ELLP_BOUND_TWOSIDED) ? a.ub[jq] - a.lb[jq] : (kk == ELLP_BOUND_FIXED ? 0.0 : INFINITY);
            }
        }
        return;
    }
    if (!have_col) return;  // all five waves together
    lds_barrier();          // the dot products of the four streaming waves are in s_dot: reached by all five waves or by none
    STAMP(1, 3);
    const double sgn = at_lower ? -1.0 : 1.0;
    double li = INFINITY;
    int dp = 0;
    if (own) {
        const int k = tid;
        const double di = sgn * (((s_dot[0][k] + s_dot[1][k]) + s_dot[2][k]) + s_dot[3][k]);
        a.d[myrow] = di;
        li = primal_lambda(di, xi0, lbi0, ubi0, k0, a.eps);  // primal…:320-367
        if (li != li) st->nan_flag = 1;
        dp = di > 0.0 ? 1 : 0;
        a.lam[myrow] = li;
        a.bidx[myrow] = (int32_t)bi0;
        a.dpos[myrow] = (uint8_t)dp;
    }
    if (tid < UPD_ROWS) {
        s_lam[tid] = li;
        s_dp[tid] = dp;
    }
    wave_lds_sync();
    if (tid == 0) {  // smallest and second smallest lambda of the block, and whose the smallest is
        double m1 = INFINITY, m2 = INFINITY;
        int info = -1;
        for (int k = 0; k < R; ++k) {
            const double v = s_lam[k];
            if (v < m1) {
                m2 = m1;
                m1 = v;
                info = (int)(2 * (row0 + k)) + s_dp[k];
            } else if (v < m2) {
                m2 = v;
            }
        }
        a.bmin[blockIdx.x - NBK] = m1;
        a.bsec[blockIdx.x - NBK] = m2;
        a.binfo[blockIdx.x - NBK] = info;
    }
    STAMP(1, 4);
}

constexpr bool ftran_eta_hands_off(int NR, bool SH) { return !SH && NR >= 1 && NR <= 4; }
// threads per block: the deciding wave comes on top of the four that own the rows' columns
constexpr int ftran_eta_threads(int NR, bool SH) { return ftran_eta_hands_off(NR, SH) ? FTRAN_HAND_THREADS : 256; }

template <int NR, bool SH = false>
__global__ __launch_bounds__(ftran_eta_threads(NR, SH)) void k_ftran_eta(FtranEtaArgs a) {
    if constexpr (ftran_eta_hands_off(NR, SH)) ftran_eta_handoff<NR>(a);
    else ftran_eta_whole<NR, SH>(a);
}

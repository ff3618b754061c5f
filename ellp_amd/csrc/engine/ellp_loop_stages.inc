// ellp_loop_stages.inc — the stages that small_loop (ellp_small.inc) and mid_loop (ellp_mid.inc) run with the same text.
// The two loops differ in where the factors live and how the factorisation and the solves are called; what they do with
// the solutions — classification of a priced column, the first-minimum butterfly, the entering fold, the bookkeeping around
// the bound flips, the commit of a pivot or flip — is the reference's rule once, here.
//
// Three stages are still written out in both loops, because moving them here costs a kernel registers (the tables are in
// profiles/rules_refactor_regs.txt): the dual leaving-row search (SGPR spills in k_small<1, 128> and k_small_batch<1, .>),
// wave 0's part of the primal ratio test (SGPR spills in k_small_batch_primal<128> and <256>) with its per-row pass, and
// the chunk maximum of the primal keys (a DPP maximum in small_loop costs k_small_batch_primal<64> a wave of occupancy).
// They call the scalar rules of ellp_rules.inc like everything else.
//
// A stage is a function of the loop's arguments (`Args`: SmallArgs or MidArgs, which name every field used here alike) and
// of the values and LDS arrays the loop hands it.  It returns values and never leaves the kernel; the loops keep the `for`,
// every barrier and fence, the stamps, the factorisation and solve calls and every early return with its status store.
// KIND: 0 primal, 1 dual.  NT: threads of the workgroup.
//
// Included inside the anonymous namespace of ellp_engine.hip ahead of ellp_small.inc (uses the rules of ellp_rules.inc,
// FoldState / fold_elements, trace_put).

// The first-minimum butterfly of the dual ratio test (chunk fold and entering fold): every lane gets the wave's
// lexicographic minimum of (k, p) over the lanes with p >= 0
__device__ __forceinline__ void wave_first_min(double *k, long long *p) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ok = __shfl_xor(*k, o);
        const long long op = __shfl_xor(*p, o);
        if (op >= 0 && (*p < 0 || ok < *k || (ok == *k && op < *p))) {
            *k = ok;
            *p = op;
        }
    }
}

// ---------------- pricing, after the dot product of nonbasic position j < nN with u (primal) / rho (dual): the reduced
// cost and its key (primal…:189, :253-270) or alpha_j and its ratio (dual…:255-278) go to rbuf / kbuf; *key / *pos (which
// the caller has set to -inf / +inf and -1) take what the chunk fold compares.
template <int KIND, class Args>
__device__ __forceinline__ void classify_column(const Args &a, int64_t j, double dot, double delta, double eps, int *s_nan, double *key,
                                                long long *pos) {
    const int nb = a.Nb[j];
    if (KIND == 0) {
        const double rj = a.c_N[j] - dot;
        if (rj != rj) *s_nan = 1;
        else *key = primal_key(rj, nb, eps);
        a.rbuf[j] = rj;
        a.kbuf[j] = *key;
    } else {
        const double al = (delta < 0.0) ? -dot : dot;
        a.rbuf[j] = dot;  // alpha as dual…:286-288 leaves it (the negation undone)
        const bool keep = dual_keep(al, nb, eps);
        if (keep) {
            const double ratio = a.dd[a.N_index[j]] / al;
            if (ratio != ratio) *s_nan = 1;
            *key = ratio;
            *pos = j;
        }
        if (a.bflip) a.kbuf[j] = keep ? *key : __longlong_as_double(0x7ff8000000000000ll);
    }
}

// ---------------- entering variable, by wave 0 from the chunk records: the reference's sequential max_by fold
// (primal…:271-287), exactly, or the first minimum (min_by, dual…:279) with theta_d's sign restored (dual…:286-289)
template <int KIND, class Args>
__device__ __forceinline__ void enter_fold(const Args &a, int nch, int64_t nN, double delta, double eps, int lane, const double *cmx,
                                           const long long *cps, long long *s_q, double *s_theta) {
    if (KIND == 0) {
        FoldState f{false, 0.0, 0, -1};
        for (int g0 = 0; g0 < nch; g0 += WAVE) {
            const double bm = (g0 + lane < nch) ? cmx[g0 + lane] : -INFINITY;
            int from = 0;
            for (;;) {
                const bool pred = lane >= from && bm > -INFINITY && (!f.have || f.racc - bm < eps);
                const unsigned long long mask = __ballot(pred);
                if (!mask) break;
                const int bl = __ffsll((long long)mask) - 1;
                const int64_t jb = (int64_t)(g0 + bl) * 64;
                const int64_t j = jb + lane;
                const bool valid = j < nN;
                const double k = valid ? a.kbuf[j] : -INFINITY;
                const long long idx = valid ? a.N_index[j] : 0;
                fold_elements(f, k, idx, jb, eps, lane);
                from = bl + 1;
            }
        }
        if (lane == 0) *s_q = f.qacc;
    } else {
        double bk = INFINITY;
        long long bp = -1;
        for (int c = lane; c < nch; c += WAVE) {
            const long long p = cps[c];
            if (p < 0) continue;
            const double k = cmx[c];
            if (bp < 0 || k < bk || (k == bk && p < bp)) {
                bk = k;
                bp = p;
            }
        }
        wave_first_min(&bk, &bp);
        if (lane == 0) {
            *s_q = bp;
            *s_theta = (delta < 0.0) ? -bk : bk;
        }
    }
}

// ---------------- bound flipping (extension; oracle: g_dual_rule & 1), around bf_walk and the solve the loop does:
// row i of sum a_j dx_j over the nflip positions of flist, in flist order (x_N moves, x_B follows by B^-1 of this)
template <class Args>
__device__ __forceinline__ double flip_row_rhs(const Args &a, int nflip, int64_t ld, int i) {
    double acc = 0.0;
    for (int k = 0; k < nflip; ++k) {
        const long long pj = a.flist[k];
        const int64_t vj = a.N_index[pj];
        const double dx = (a.Nb[pj] == ELLP_NB_LOWER) ? (a.ub[vj] - a.lb[vj]) : (a.lb[vj] - a.ub[vj]);
        acc += a.A_N[pj * ld + i] * dx;
    }
    return acc;
}
// the flipped variables go to their other bound and take its label (after every thread has read the old labels)
template <int NT, class Args>
__device__ __forceinline__ void flip_relabel(const Args &a, int nflip, int tid) {
    for (int k = tid; k < nflip; k += NT) {
        const long long pj = a.flist[k];
        const int64_t vj = a.N_index[pj];
        const bool lower = a.Nb[pj] == ELLP_NB_LOWER;
        a.x[vj] = lower ? a.ub[vj] : a.lb[vj];
        a.Nb[pj] = lower ? ELLP_NB_UPPER : ELLP_NB_LOWER;
    }
}
// the leaving row's violation after the flips have moved x_B
template <class Args>
__device__ __forceinline__ double flip_delta(const Args &a, long long lr, int side) {
    const int64_t bi = a.B_index[lr];
    return (side == ELLP_NB_UPPER) ? a.x[bi] - a.ub[bi] : a.x[bi] - a.lb[bi];
}

// ---------------- commit, thread 0 alone (the loops swap the columns and update the vectors themselves)
// the objective's step along the entering column, shared by a primal pivot and a primal flip
template <class Args>
__device__ __forceinline__ void commit_primal_step(const Args &a, long long q, double lambda, int at_lower) {
    DevState *st = a.st;
    st->lambda = lambda;
    if (lambda > 0.0) st->obj = st->obj + (at_lower ? lambda * a.rbuf[q] : -(lambda * a.rbuf[q]));
    trace_put(a.trace, st->iters, st->obj);
}
// primal pivot (primal…:205-221): position q and row r exchange variable, cost and label
template <class Args>
__device__ __forceinline__ void commit_primal_pivot(const Args &a, long long q, long long r, int64_t jq, int side, double lambda,
                                                    int at_lower) {
    const int64_t t = a.B_index[r];
    a.B_index[r] = jq;
    a.N_index[q] = t;
    const double tc = a.c_N[q];
    a.c_N[q] = a.c_B[r];
    a.c_B[r] = tc;
    a.Nb[q] = (uint8_t)side;
    a.st->pivots += 1;
    commit_primal_step(a, q, lambda, at_lower);
}
// primal bound flip (primal…:223-231); *s_stop: the label was neither bound (panic 229)
template <class Args>
__device__ __forceinline__ void commit_primal_flip(const Args &a, long long q, double lambda, int at_lower, int *s_stop) {
    const int nbq = a.Nb[q];
    a.st->flips += 1;
    commit_primal_step(a, q, lambda, at_lower);
    if (nbq == ELLP_NB_LOWER) a.Nb[q] = ELLP_NB_UPPER;
    else if (nbq == ELLP_NB_UPPER) a.Nb[q] = ELLP_NB_LOWER;
    else {
        a.st->panic_code = 229;
        a.st->status = ELLP_ERR_PANIC;
        *s_stop = 1;
    }
}
// dual pivot (dual…:296-316, :322-333): lv is the variable that leaves row r; *s_stop: theta_p is NaN
template <class Args>
__device__ __forceinline__ void commit_dual_pivot(const Args &a, long long q, long long r, int64_t jq, int64_t lv, int side,
                                                  double theta_d, double theta_p, double delta_upd, int *s_stop) {
    DevState *st = a.st;
    a.dd[lv] = -theta_d;
    a.dd[jq] = 0.0;
    a.x[jq] = a.x[jq] + theta_p;
    st->obj = st->obj + theta_d * delta_upd;
    trace_put(a.trace, st->iters, st->obj);
    a.B_index[r] = jq;
    a.N_index[q] = lv;
    a.Nb[q] = (uint8_t)side;
    const double tc = a.c_N[q];  // the dual loop does not use costs; kept consistent for a later hand-off
    a.c_N[q] = a.c_B[r];
    a.c_B[r] = tc;
    st->pivots += 1;
    if (theta_p != theta_p) {
        st->status = ELLP_ERR_NAN;
        *s_stop = 1;
    }
}

// ellp_small.inc — the reference's loop, literally, for small LPs (m <= 128): ONE persistent workgroup
// runs whole iterations of
//   primal  src/solvers/primal/primal_simplex_solver.rs:160-235 (+ pivot() :238-435)
//   dual    src/solvers/dual/dual_simplex_solver.rs:188-334
// back to back inside one launch, with the LU of A_B re-done EVERY iteration in LDS exactly as the
// reference does (primal…:173, dual…:241), instead of an explicit B^-1 carried by eta updates.
//
// Why a second path.  (1) Launch-bound regime: at m = 27 (netlib AFIRO) the three-launch iteration is
// pure dispatch latency; here an iteration is a few hundred workgroup barriers and no launch at all.
// (2) Exactness: small real LPs run through bases of condition 1e7-1e9 (netlib ADLITTLE in most
// variable orders).  An explicit inverse is then only good to cond * 1e-16 ~ 1e-7 however often it is
// refreshed, a structurally zero alpha_j comes out as 1e-9 > EPS, is taken as pivot and the basis turns
// singular; the reference's sparse-in-effect LU keeps such entries at 0 or 1e-17.  Every floating-point
// operation below is the one the CPU oracle (oracle/ellp_oracle.c: lu_factor_inplace, lu_btran, lu_solve,
// the sequential dot products and updates) performs, in the same order with the same roundings (no
// contraction: the library is built with -ffp-contract=off), so on this path the engine's pivots, point
// and duals are the oracle's bit for bit — including the dual ratio test's exact-minimum ties.
//
// Parallelism inside the workgroup (256 threads): the LU's trailing update and row swaps over the
// matrix elements, the triangular solves as column sweeps (or, for the dot-product forms nalgebra's
// tr_solve uses, pipelined over rows so that every sum is still accumulated in index order), pricing one
// column per lane with a sequential dot product, the decision folds by the same exact wave emulations
// the large engine uses.  State lives in the same HBM arrays as the large engine's (A_B, A_N, c_B, c_N,
// x, B_index, N_index, Nb, y, d), so phase hand-off and read-back are shared; only B^-1 is not kept.
//
// What the loop does with the solutions — classification of a priced column, the first-minimum and entering folds, the
// bookkeeping around the bound flips, the commit of a pivot or flip — is not written here but in ellp_loop_stages.inc,
// which mid_loop (ellp_mid.inc) calls as well; the scalar pivot rules are ellp_rules.inc.  This file keeps the loop's
// skeleton (barriers, stamps, early returns), the LU and the solves in LDS, and the three stages that file names as left
// in place (leaving row, primal ratio test, chunk maximum).
//
// Included inside the anonymous namespace of ellp_engine.hip after ellp_loop_stages.inc (uses DevState, ratio_fold and the stages).

struct SmallArgs {
    double *A_B, *A_N, *c_B, *c_N, *x, *y, *dd;
    const double *lb, *ub;
    const uint8_t *kind;
    int64_t *B_index, *N_index;
    uint8_t *Nb;
    double *rbuf, *kbuf;  // per nonbasic position: r_j / alpha_j, Dantzig key / dual ratio
    DevState *st;
    int64_t m, ld, nN;
    unsigned long long max_iters;
    int nch;  // chunks of 64 nonbasic positions
    double eps;
    Trace trace;
    unsigned long long *stamps;  // measurement (ELLP_SMALL_STAMPS): 100 MHz ticks per phase of the iteration, or null
    int maxviol;  // dual, an extension (ELLP_FLAG_DUAL_MAX_VIOLATION): the leaving row of largest violation, first of equals
    // dual, an extension (ELLP_FLAG_DUAL_BOUND_FLIPPING; oracle eo_set_dual_rule bit 0): the long-step ratio test; flist
    // (nN entries) takes the positions whose variable changes bound in this iteration
    int bflip;
    long long *flist;
};

// ---- bound-flipping ratio test (extension; oracle/ellp_oracle.c, g_dual_rule & 1), shared by k_small and k_mid ----
// The next breakpoint after (ck, cp) in (ratio, position) order among the eligible positions (kbuf[j] is the ratio, NaN where
// position j is not eligible).  The whole workgroup calls it; every thread returns the same pair (position -1: none left).
// s_k / s_p: NT / 64 entries of scratch.
template <int NT>
__device__ __forceinline__ void bf_next(const double *kbuf, int64_t nN, double ck, long long cp, int tid, double *s_k, long long *s_p,
                                        double *out_k, long long *out_p) {
    constexpr int NWV = NT / 64;
    double bk = INFINITY;
    long long bp = -1;
    for (int64_t j = tid; j < nN; j += NT) {
        const double k = kbuf[j];
        if (k != k) continue;
        if (!(k > ck || (k == ck && j > cp))) continue;
        if (bp < 0 || k < bk || (k == bk && j < bp)) {
            bk = k;
            bp = j;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ok = __shfl_xor(bk, o);
        const long long op = __shfl_xor(bp, o);
        if (op >= 0 && (bp < 0 || ok < bk || (ok == bk && op < bp))) {
            bk = ok;
            bp = op;
        }
    }
    __syncthreads();  // the scratch may still be read from a previous call
    if ((tid & 63) == 0) {
        s_k[tid >> 6] = bk;
        s_p[tid >> 6] = bp;
    }
    __syncthreads();
    bk = s_k[0];
    bp = s_p[0];
    for (int w = 1; w < NWV; ++w) {
        const double ok = s_k[w];
        const long long op = s_p[w];
        if (op >= 0 && (bp < 0 || ok < bk || (ok == bk && op < bp))) {
            bk = ok;
            bp = op;
        }
    }
    *out_k = bk;
    *out_p = bp;
}

// The walk over the breakpoints: from the first minimum (ck, cp) on, a BOXED variable whose stretch leaves the slope positive
// (slope - |alpha_j| (ub_j - lb_j) > 0) and that is not the last breakpoint is passed — its position goes to flist — and
// the next one is examined; the one that is not passed enters.  Returns the number of passed positions; *q_out / *k_out: the
// entering position and its ratio.  Uniform over the workgroup.
template <int NT>
__device__ __forceinline__ int bf_walk(const double *kbuf, const double *rbuf, const int64_t *N_index, const uint8_t *kind, const double *lb,
                                       const double *ub, long long *flist, int64_t nN, double delta, double ck, long long cp, int tid,
                                       double *s_k, long long *s_p, long long *q_out, double *k_out) {
    double slope = fabs(delta);
    int taken = 0;
    for (;;) {
        const int64_t vj = N_index[cp];
        const bool boxed = kind[vj] == ELLP_BOUND_TWOSIDED;
        const double drop = boxed ? fabs(rbuf[cp]) * (ub[vj] - lb[vj]) : INFINITY;
        if (!boxed || !(slope - drop > 0.0)) break;
        double nk;
        long long np;
        bf_next<NT>(kbuf, nN, ck, cp, tid, s_k, s_p, &nk, &np);
        if (np < 0) break;  // the last breakpoint enters whatever its kind
        if (tid == 0) flist[taken] = cp;
        slope -= drop;
        taken += 1;
        ck = nk;
        cp = np;
    }
    *q_out = cp;
    *k_out = ck;
    return taken;
}

constexpr int SMALL_MAX_M = 128;
constexpr int SMALL_THREADS = 256;  // the largest workgroup; k_small<KIND, NT> runs with NT = 64, 128 or 256 (small_threads)

// bytes of dynamic LDS k_small needs (0: does not fit)
inline size_t small_lds_bytes(int64_t m, int64_t nN) {
    if (m > SMALL_MAX_M || m < 1) return 0;
    const size_t nch = (size_t)((nN + 63) / 64);
    size_t b = sizeof(double) * (size_t)(m * m)      // LU
               + sizeof(double) * (size_t)(3 * m)    // v1 (u / rho), v2 (d / alpha_q), lam
               + sizeof(double) * nch                // chunk maxima / minima
               + sizeof(long long) * nch             // dual: chunk argmin positions
               + sizeof(int32_t) * (size_t)(3 * m)   // bidx, swap list a, swap list b
               + (size_t)m + 64;                     // dpos + slack
    b = (b + 15) / 16 * 16;
    return b <= 150 * 1024 ? b : 0;
}

// LU of the m x m matrix in LDS (column-major, ld = m), nalgebra's LU::new as restated by the oracle's
// lu_factor_inplace: pivot = FIRST entry of maximal modulus in the column, a zero pivot column is
// skipped, multipliers a * (1/diag), trailing update c[r] = (-c_k[i]) * l[r] + c[r].
// The transposition list goes to (pa, pb), its length to *plen.
//
// Thread t owns ROW t of the matrix (NT >= m) for the whole factorisation.  Rows are NOT moved while
// factorising: each thread carries the position its row currently has (`pos`), a pivot exchanges two
// positions, and one gather at the end puts the rows where the reference's swaps would have put them
// (lop: position -> row).  A step is: my entry of column i (one LDS read), the first maximum by
// position (DPP max, ballot, DPP min over the tied positions), the multiplier, the entries of the pivot
// row to the right (one read per column, lane j takes column i+1+j) and the trailing update of my row
// for the columns whose pivot-row entry is not zero — the skip the oracle makes (`a == 0`), taken for
// whole columns at once from a ballot, which on the sparse bases of real LPs leaves little to do.
// One workgroup barrier per step when the workgroup has several waves, none with one wave.
template <int NT>
__device__ __forceinline__ void small_lu(double *LU, int m, int32_t *pa, int32_t *pb, int *plen, int32_t *lop,
                                         double *s_wv, double *s_wd, int *s_wi, int *s_wp, int tid) {
    constexpr int NW = NT / 64;
    const int lane = tid & 63, wave = tid >> 6;
    if (tid == 0) *plen = 0;
    int pos = tid < m ? tid : 0x7fffffff;  // rows beyond m never take part
    for (int i = 0; i < m; ++i) {
        double *ci = LU + i * m;
        // ---- pivot search over the rows at positions i..m-1
        const bool cand = tid < m && pos >= i;
        const double cur = tid < m ? ci[tid] : 0.0;
        double v = -1.0;
        if (cand) {
            v = fabs(cur);
            if (v != v) v = (pos == i) ? INFINITY : -1.0;  // `v > best` is false for a NaN: only position i itself can carry one
        }
        const double M = wave_allmax_dpp(v);
        const bool tied = cand && v == M;
        int pmin = 0x7fffffff, P = 0;  // the pivot's position and row
        double diag = 0.0;
        {
            unsigned long long bl = __ballot(tied);
            if (__popcll(bl) > 1) {  // several entries of that modulus (the +-1 of slack columns): the first by position
                pmin = wave_allmin_dpp(tied ? pos : 0x7fffffff);
                bl = __ballot(tied && pos == pmin);
            }
            const int L = bl ? __ffsll((long long)bl) - 1 : 0;
            diag = readlane_f64(cur, L);
            pmin = bl ? __builtin_amdgcn_readlane(pos, L) : 0x7fffffff;
            P = wave * 64 + L;
        }
        if (NW > 1) {
            const int par = (i & 1) * 4;  // double-buffered by the parity of the step: one barrier per step is enough
            if (lane == 0) {
                s_wv[par + wave] = M;
                s_wd[par + wave] = diag;
                s_wi[par + wave] = P;
                s_wp[par + wave] = pmin;
            }
            __syncthreads();  // also: every row's trailing update of step i-1 is in LDS
            double best = s_wv[par];
            diag = s_wd[par];
            P = s_wi[par];
            pmin = s_wp[par];
#pragma unroll
            for (int w = 1; w < NW; ++w) {
                const double wv = s_wv[par + w];
                const int wp = s_wp[par + w];
                if (wv > best || (wv == best && wp < pmin)) {
                    best = wv;
                    diag = s_wd[par + w];
                    P = s_wi[par + w];
                    pmin = wp;
                }
            }
        }
        if (diag == 0.0) continue;
        const double inv_diag = 1.0 / diag;
        // ---- the pivot's row takes position i, the row that had it takes the pivot's
        if (pmin != i) {
            if (pos == i) pos = pmin;
            else if (tid == P) pos = i;
            if (tid == 0) {
                pa[*plen] = i;
                pb[*plen] = pmin;
                *plen = *plen + 1;
            }
        }
        // ---- multiplier of my row, trailing update of my row
        const bool below = tid < m && pos > i;
        double l = 0.0;
        if (below) {
            l = cur * inv_diag;
            ci[tid] = l;
        }
        const int w = m - i - 1;
#pragma unroll 1
        for (int base = 0; base < w; base += 64) {
            const int kc = i + 1 + base + lane;
            const double ak = (base + lane < w) ? LU[kc * m + P] : 0.0;
            unsigned long long mask = __ballot(ak != 0.0);  // NaN != 0: such a column is updated, as in the oracle
            while (mask) {
                int kk[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (mask) {
                        kk[u] = i + 1 + base + __ffsll((long long)mask) - 1;
                        mask &= mask - 1;
                    } else kk[u] = -1;
                }
                double av[4], cv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (kk[u] >= 0) {
                        av[u] = -LU[kk[u] * m + P];
                        cv[u] = below ? LU[kk[u] * m + tid] : 0.0;
                    }
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (kk[u] >= 0 && below) LU[kk[u] * m + tid] = av[u] * l + cv[u];
            }
        }
    }
    // ---- rows into position order: what the reference's row swaps (of whole rows, L part included) leave
    if (tid < m) lop[pos] = tid;
    __syncthreads();
    const int src = tid < m ? lop[tid] : 0;
#pragma unroll 1
    for (int c0 = 0; c0 < m; c0 += 8) {
        double t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (tid < m && c0 + u < m) t[u] = LU[(c0 + u) * m + src];
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (tid < m && c0 + u < m) LU[(c0 + u) * m + tid] = t[u];
    }
    __syncthreads();
}

// the value `mine` of thread src to every thread.  One wave: a readlane.  Several waves: through LDS, the slot
// double-buffered by the parity of the caller's step counter so that one barrier per step is enough.
template <int NT>
__device__ __forceinline__ double small_bcast(double mine, int src, double *slot2, int step, int tid) {
    if (NT == 64) return readlane_f64(mine, src);
    double *sl = slot2 + (step & 1);
    if (tid == src) *sl = mine;
    __syncthreads();
    return *sl;
}

// U^T x = b (nalgebra tr_solve_upper_triangular, oracle lu_tr_solve_upper): x_i = (b_i - sum_{k<i} U[k,i] x_k) / U_ii
// with the sum accumulated for k = 0, 1, ... in that order.  Thread i keeps b_i and its sum in registers and
// adds term k as soon as x_k is broadcast, so the order of every sum is the sequential one; its column of U is
// fetched eight entries ahead.  Returns 0 (in *ok) on a zero diagonal.
template <int NT>
__device__ __forceinline__ void small_tr_solve_upper(const double *LU, int m, double *b, int *ok, double *slot2, int tid) {
    const double *ci = LU + (tid < m ? tid : 0) * m;
    double mine = tid < m ? b[tid] : 0.0, dot = 0.0;
    const double diag = tid < m ? ci[tid] : 1.0;
    const int zero = __syncthreads_or(tid < m && diag == 0.0);
    if (tid == 0) *ok = zero ? 0 : 1;
    __syncthreads();
    if (zero) return;
#pragma unroll 1
    for (int k0 = 0; k0 < m; k0 += 8) {
        double cc[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) cc[u] = (k0 + u < m) ? ci[k0 + u] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int k = k0 + u;
            if (k < m) {
                if (tid == k) {
                    double v = mine;
                    v -= dot;
                    v /= diag;
                    mine = v;
                }
                const double xk = small_bcast<NT>(mine, k, slot2, k, tid);
                if (tid > k && tid < m) dot += cc[u] * xk;
            }
        }
    }
    if (tid < m) b[tid] = mine;
    __syncthreads();
}

// L^T x = b, unit diagonal (oracle lu_tr_solve_lower_unit): x_i = b_i - sum_{k>i} L[k,i] x_k with the sum
// accumulated for k = i+1, i+2, ... — the FIRST term is the one that becomes known last, so nothing
// can be accumulated ahead of time: a dependent chain of m^2/2 additions, done by one lane (8 k
// additions at m = 128).  The products do not depend on the chain and pipeline behind it.
__device__ __forceinline__ void small_tr_solve_lower_unit(const double *LU, int m, double *b, double *P, int tid) {
    // wave 0: lane j forms the product of term i+1+j (all products of a row at once) and parks it in LDS; the
    // additions are then made one after the other in term order — per term one addition and half a 16-byte
    // LDS read, nothing else (a single wave issues one instruction every few cycles whatever its lane count)
    if (tid < 64) {
        for (int i = m - 2; i >= 0; --i) {
            const double *ci = LU + i * m;
            const int cnt = m - i - 1;
            for (int j = tid; j < cnt; j += 64) P[j] = ci[i + 1 + j] * b[i + 1 + j];
            double dot = 0.0;
            int j = 0;
            for (; j + 8 <= cnt; j += 8) {
                double q[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) q[u] = P[j + u];
#pragma unroll
                for (int u = 0; u < 8; ++u) dot += q[u];
            }
            for (; j < cnt; ++j) dot += P[j];
            if (tid == 0) b[i] -= dot;
        }
    }
    __syncthreads();
}

// u = A_B^-T v (primal…:184-187, dual…:248-253; oracle lu_btran): U^T, L^T, then the inverse permutation
template <int NT>
__device__ __forceinline__ void small_btran(const double *LU, int m, double *v, const int32_t *pa, const int32_t *pb,
                                            const int *plen, int *ok, double *slot2, double *scratch, int tid) {
    small_tr_solve_upper<NT>(LU, m, v, ok, slot2, tid);
    if (!*ok) return;
    small_tr_solve_lower_unit(LU, m, v, scratch, tid);
    if (tid == 0) {
        for (int k = *plen - 1; k >= 0; --k) {
            const double t = v[pa[k]];
            v[pa[k]] = v[pb[k]];
            v[pb[k]] = t;
        }
    }
    __syncthreads();
}

// LU::solve (primal…:295, dual…:294; oracle lu_solve): x = P b; L y = x and U z = y as column sweeps.  Thread t
// keeps entry t of the vector in a register; each step broadcasts one entry (small_bcast) and the column of
// L / U it multiplies is fetched eight steps ahead.
template <int NT>
__device__ __forceinline__ void small_lu_solve(const double *LU, int m, double *b, const int32_t *pa, const int32_t *pb,
                                               const int *plen, int *ok, double *slot2, int tid) {
    if (tid == 0) {
        for (int k = 0; k < *plen; ++k) {
            const double t = b[pa[k]];
            b[pa[k]] = b[pb[k]];
            b[pb[k]] = t;
        }
    }
    const double diag = tid < m ? LU[tid * m + tid] : 1.0;
    const int zero = __syncthreads_or(tid < m && diag == 0.0);  // also: the permuted b is visible
    if (tid == 0) *ok = zero ? 0 : 1;
    double mine = tid < m ? b[tid] : 0.0;
    __syncthreads();
    if (zero) return;
    int stp = 0;
#pragma unroll 1
    for (int i0 = 0; i0 + 1 < m; i0 += 8) {
        double cl[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) cl[u] = (i0 + u + 1 < m && tid < m) ? LU[(i0 + u) * m + tid] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + u;
            if (i + 1 < m) {
                const double coeff = small_bcast<NT>(mine, i, slot2, stp++, tid);
                if (coeff != 0.0 && tid > i && tid < m) mine = (-coeff) * cl[u] + mine;
            }
        }
    }
#pragma unroll 1
    for (int i0 = m - 1; i0 >= 0; i0 -= 8) {
        double cu[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) cu[u] = (i0 - u >= 0 && tid < m) ? LU[(i0 - u) * m + tid] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 - u;
            if (i >= 0) {
                if (tid == i) mine = mine / diag;
                const double coeff = small_bcast<NT>(mine, i, slot2, stp++, tid);
                if (coeff != 0.0 && tid < i) mine = (-coeff) * cu[u] + mine;
            }
        }
    }
    if (tid < m) b[tid] = mine;
    __syncthreads();
}

// workgroup size: every row needs a thread (LU, solves); more threads only help pricing and the copies, and
// with one wave (m <= 64) no step of the LU or of the solves needs a workgroup barrier
inline int small_threads(int64_t m, int64_t nN) {
    if (nN > 2048) return 256;
    return m <= 64 ? 64 : (m <= 128 ? 128 : 256);
}

#define SMALL_STAMP(slot)                                   \
    if (a.stamps && tid == 0) {                             \
        const unsigned long long _t = wall_clock64();       \
        a.stamps[slot] += _t - t_prev;                      \
        t_prev = _t;                                        \
    }

// The loop of k_small for the LP of `a`, run by the whole workgroup.  A function of its arguments alone (no blockIdx), so
// that k_small_batch can run one LP per workgroup with the same code.
template <int KIND, int NT>
__device__ __forceinline__ void small_loop(const SmallArgs &a) {
    unsigned long long t_prev = a.stamps ? wall_clock64() : 0ull;
    unsigned long long c_prev = a.stamps ? clock64() : 0ull;
    constexpr int NW = NT / 64;
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ double s_wv[8], s_wd[8];
    __shared__ int s_wi[8], s_wp[8];
    __shared__ double s_bc[2];
    __shared__ long long s_tmp[4];
    __shared__ int s_plen, s_ok, s_stop, s_side, s_nan;
    __shared__ long long s_q, s_r;
    __shared__ double s_lambda, s_theta, s_delta;
    DevState *st = a.st;
    if (st->status != ST_RUNNING) return;
    const int m = (int)a.m;
    const int64_t ld = a.ld, nN = a.nN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nch = a.nch;
    double *LU = reinterpret_cast<double *>(smem);
    double *v1 = LU + (size_t)m * m;  // u (primal) / rho (dual)
    double *v2 = v1 + m;              // d (primal) / alpha_q (dual)
    double *lam = v2 + m;
    double *cmx = lam + m;
    long long *cps = reinterpret_cast<long long *>(cmx + nch);
    int32_t *bidx = reinterpret_cast<int32_t *>(cps + nch);
    int32_t *pa = bidx + m;
    int32_t *pb = pa + m;
    uint8_t *dpos = reinterpret_cast<uint8_t *>(pb + m);
    const double eps = a.eps;

    for (unsigned long long it = 0; it < a.max_iters; ++it) {
        if (tid == 0) {
            st->iters += 1;  // a loop body is entered (primal…:163-168, dual…:191-196)
            s_stop = 0;
            s_nan = 0;
        }
        // ---------------- dual: leaving row first (dual…:200-236), the LU is done regardless (quirk Q4)
        long long lr = -1;
        if (KIND == 1) {
            long long best = INT64_MAX;
            double bad = -1.0;
            double dl;
            int sd;
            for (int i = tid; i < m; i += NT)
                if (dual_violation(a.B_index, a.x, a.kind, a.lb, a.ub, eps, i, &dl, &sd)) {
                    if (!a.maxviol) {
                        best = i;
                        break;
                    }
                    double ad = fabs(dl);
                    if (ad != ad) ad = INFINITY;
                    if (ad > bad) {
                        bad = ad;
                        best = i;
                    }
                }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const long long ob = __shfl_xor(best, o);
                const double oa = __shfl_xor(bad, o);
                if (a.maxviol ? (oa > bad || (oa == bad && ob < best)) : (ob < best)) {
                    best = ob;
                    bad = oa;
                }
            }
            if (lane == 0) {
                s_tmp[wave] = best;
                s_wv[wave] = bad;
            }
            __syncthreads();
            best = s_tmp[0];
            bad = s_wv[0];
            for (int w = 1; w < NW; ++w)
                if (a.maxviol ? (s_wv[w] > bad || (s_wv[w] == bad && s_tmp[w] < best)) : (s_tmp[w] < best)) {
                    best = s_tmp[w];
                    bad = s_wv[w];
                }
            __syncthreads();  // s_wv is the LU's scratch next
            lr = best == INT64_MAX ? -1 : best;
            if (tid == 0 && lr >= 0) {
                double delta = 0.0;
                int side = 0;
                dual_violation(a.B_index, a.x, a.kind, a.lb, a.ub, eps, lr, &delta, &side);
                s_delta = delta;
                s_side = side;
            }
        }
        SMALL_STAMP(0)
        // ---------------- lu = A_B.clone().lu()
        {
            int k = tid / m, r = tid - k * m;
            const int dk = NT / m, dr = NT - dk * m;
#pragma unroll 4
            for (int e = tid; e < m * m; e += NT) {
                LU[e] = a.A_B[(int64_t)k * ld + r];
                k += dk;
                r += dr;
                if (r >= m) {
                    r -= m;
                    ++k;
                }
            }
        }
        __syncthreads();
        SMALL_STAMP(1)
        small_lu<NT>(LU, m, pa, pb, &s_plen, bidx, s_wv, s_wd, s_wi, s_wp, tid);
        SMALL_STAMP(2)
        if (KIND == 0) {  // primal…:175-179
            int small = 0;
            for (int i = tid; i < m; i += NT)
                if (fabs(LU[i * m + i]) < eps) small = 1;
            if (__syncthreads_or(small)) {
                if (tid == 0) st->status = ELLP_ERR_SINGULAR;
                return;
            }
        } else if (lr < 0) {  // dual…:243-246
            if (tid == 0) st->status = ELLP_OPTIMAL;
            return;
        }
        // ---------------- BTRAN: u = B^-T c_B (primal…:184-187) / rho = row r of B^-1 (dual…:248-253)
        for (int i = tid; i < m; i += NT) v1[i] = (KIND == 0) ? a.c_B[i] : (i == lr ? 1.0 : 0.0);
        __syncthreads();
        small_btran<NT>(LU, m, v1, pa, pb, &s_plen, &s_ok, s_bc, lam, tid);
        if (!s_ok) {
            if (tid == 0) {
                st->panic_code = KIND == 0 ? 187 : 249;
                st->status = ELLP_ERR_PANIC;
            }
            return;
        }
        SMALL_STAMP(3)
        // ---------------- pricing (primal…:189 + keys :253-270 / dual…:255-278), one column per lane,
        // the dot product accumulated in row order
        const double delta = (KIND == 1) ? s_delta : 0.0;
        for (int c = wave; c < nch; c += NW) {
            const int64_t j = (int64_t)c * 64 + lane;
            double key = (KIND == 0) ? -INFINITY : INFINITY;
            long long pos = -1;
            if (j < nN) {
                const double *cj = a.A_N + j * ld;
                double dot = 0.0;
                int i = 0;
                for (; i + 8 <= m; i += 8) {  // eight loads in flight; the sum is still accumulated in row order
                    double pr[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) pr[u] = cj[i + u] * v1[i + u];
#pragma unroll
                    for (int u = 0; u < 8; ++u) dot += pr[u];
                }
                for (; i < m; ++i) dot += cj[i] * v1[i];
                classify_column<KIND>(a, j, dot, delta, eps, &s_nan, &key, &pos);
            }
            if (KIND == 0) {
                double v = key;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
                if (lane == 0) cmx[c] = v;
            } else {
                wave_first_min(&key, &pos);  // lexicographic (ratio, position)
                if (lane == 0) {
                    cmx[c] = key;
                    cps[c] = pos;
                }
            }
        }
        __syncthreads();
        if (s_nan) {
            if (tid == 0) st->status = ELLP_ERR_NAN;
            return;
        }
        SMALL_STAMP(4)
        // ---------------- entering variable
        if (wave == 0) enter_fold<KIND>(a, nch, nN, delta, eps, lane, cmx, cps, &s_q, &s_theta);
        __syncthreads();
        long long q = s_q;
        if (q < 0) {
            if (tid == 0) st->status = (KIND == 0) ? ELLP_OPTIMAL : ELLP_INFEASIBLE;  // primal…:289-292 / dual…:281-284
            return;
        }
        SMALL_STAMP(5)
        if (tid == 0) ELLP_CHECK(st, q < nN, 9131);
        double theta_sel = (KIND == 1) ? s_theta : 0.0;
        double delta_upd = delta;  // the leaving row's violation the updates use (after the bound flips, if any)
        if (KIND == 1 && a.bflip) {
            // extension: the long-step ratio test (oracle: g_dual_rule & 1)
            double ck;
            const int nflip = bf_walk<NT>(a.kbuf, a.rbuf, a.N_index, a.kind, a.lb, a.ub, a.flist, nN, delta, (delta < 0.0) ? -theta_sel : theta_sel, q,
                                          tid, s_wv, s_tmp, &q, &ck);
            theta_sel = (delta < 0.0) ? -ck : ck;
            if (nflip > 0) {
                __syncthreads();  // flist is complete
                // x_N moves, x_B follows: B^-1 (sum of a_j dx_j) with this iteration's LU
                for (int i = tid; i < m; i += NT) v2[i] = flip_row_rhs(a, nflip, ld, i);
                __syncthreads();  // every thread has read the labels before they change
                flip_relabel<NT>(a, nflip, tid);
                small_lu_solve<NT>(LU, m, v2, pa, pb, &s_plen, &s_ok, s_bc, tid);
                if (!s_ok) {
                    if (tid == 0) {
                        st->panic_code = 2940;
                        st->status = ELLP_ERR_PANIC;
                    }
                    return;
                }
                for (int i = tid; i < m; i += NT) {
                    const int64_t bi = a.B_index[i];
                    a.x[bi] = a.x[bi] - v2[i];
                }
                __syncthreads();
                delta_upd = flip_delta(a, lr, s_side);
                __syncthreads();  // v2 is the FTRAN's next
            }
        }
        // ---------------- FTRAN: d = +-B^-1 a_q (primal…:295-300) / alpha_q (dual…:294)
        const int64_t jq = a.N_index[q];
        for (int i = tid; i < m; i += NT) v2[i] = a.A_N[q * ld + i];
        __syncthreads();
        small_lu_solve<NT>(LU, m, v2, pa, pb, &s_plen, &s_ok, s_bc, tid);
        SMALL_STAMP(6)
        if (!s_ok) {
            if (tid == 0) {
                st->panic_code = KIND == 0 ? 295 : 294;
                st->status = ELLP_ERR_PANIC;
            }
            return;
        }
        if (KIND == 0) {
            const int at_lower = a.Nb[q] == ELLP_NB_LOWER ? 1 : 0;
            // ---- ratio test (primal…:305-400): lambda_i per basic row, then the sequential fold
            if (tid < m) {
                const int i = tid;
                double di = v2[i];
                if (at_lower) di = -di;
                v2[i] = di;
                const int64_t bi = a.B_index[i];
                const double xi = a.x[bi], lbi = a.lb[bi], ubi = a.ub[bi];
                const double li = primal_lambda(di, xi, lbi, ubi, a.kind[bi], eps);  // primal…:320-367
                if (li != li) s_nan = 1;
                lam[i] = li;
                bidx[i] = (int32_t)bi;
                dpos[i] = di > 0.0 ? 1 : 0;
            }
            __syncthreads();
            if (wave == 0) {
                const int nck = (m + 63) >> 6;
                // chunk minima into cmx[0..nck): cmx is free again (the entering fold is done)
                for (int c = 0; c < nck; ++c) {
                    const int i = c * 64 + lane;
                    const double cm = wave_min(i < m ? lam[i] : INFINITY);
                    if (lane == 0) cmx[c] = cm;
                }
                const int kq = a.kind[jq];  // primal…:305-311
                const double lambda0 = (kq == ELLP_BOUND_TWOSIDED) ? a.ub[jq] - a.lb[jq] : (kq == ELLP_BOUND_FIXED ? 0.0 : INFINITY);
                const RatioResult rr = ratio_fold(cmx, nck, m, lam, bidx, dpos, lambda0, eps, lane);
                if (lane == 0) {
                    s_lambda = rr.lambda;
                    s_r = rr.nb;
                    s_side = rr.side;
                }
            }
            __syncthreads();
            const double lambda = s_lambda;
            const long long r = s_r;
            if (s_nan) {
                if (tid == 0) st->status = ELLP_ERR_NAN;
                return;
            }
            if (!(lambda >= 0.0)) {  // primal…:402
                if (tid == 0) {
                    st->panic_code = 402;
                    st->status = ELLP_ERR_PANIC;
                }
                return;
            }
            if (isinf(lambda)) {  // primal…:404-406
                if (tid == 0) st->status = ELLP_UNBOUNDED;
                return;
            }
            if (lambda > 0.0) {  // primal…:408-417
                if (tid < m) {
                    const int64_t bi = a.B_index[tid];
                    a.x[bi] = a.x[bi] + lambda * v2[tid];
                }
                if (tid == 0) {
                    if (at_lower) a.x[jq] = a.x[jq] + lambda;
                    else a.x[jq] = a.x[jq] - lambda;
                }
            }
            __syncthreads();
            if (r >= 0) {  // primal…:205-221
                for (int i = tid; i < m; i += NT) {
                    const double t = a.A_N[q * ld + i];
                    a.A_N[q * ld + i] = a.A_B[r * ld + i];
                    a.A_B[r * ld + i] = t;
                }
                if (tid == 0) commit_primal_pivot(a, q, r, jq, s_side, lambda, at_lower);
            } else if (tid == 0) {
                commit_primal_flip(a, q, lambda, at_lower, &s_stop);
            }
        } else {
            // ---------------- dual updates (dual…:296-316) and swap (:322-333)
            const double theta_d = theta_sel;
            const long long r = lr;
            const int64_t lv = a.B_index[r];
            __syncthreads();  // B_index[r] is read by everybody before thread 0 rewrites it
            for (int64_t j = tid; j < nN; j += NT) {
                const int64_t vj = a.N_index[j];
                a.dd[vj] = a.dd[vj] - theta_d * a.rbuf[j];
            }
            for (int i = tid; i < m; i += NT) a.y[i] = a.y[i] + theta_d * v1[i];
            const double theta_p = delta_upd / v2[r];
            if (tid < m) {
                const int64_t bi = a.B_index[tid];
                a.x[bi] = a.x[bi] - theta_p * v2[tid];
            }
            __syncthreads();
            for (int i = tid; i < m; i += NT) {
                const double t = a.A_B[r * ld + i];
                a.A_B[r * ld + i] = a.A_N[q * ld + i];
                a.A_N[q * ld + i] = t;
            }
            if (tid == 0) commit_dual_pivot(a, q, r, jq, lv, s_side, theta_d, theta_p, delta_upd, &s_stop);
        }
        __syncthreads();
        SMALL_STAMP(7)
        if (a.stamps && tid == 0) {
            a.stamps[8] += 1;
            const unsigned long long c_now = clock64();
            a.stamps[9] += c_now - c_prev;  // shader-clock cycles of the iteration (s_memtime)
            c_prev = c_now;
        }
        const int stop = s_stop;
        __syncthreads();  // thread 0 clears the flag at the top of the next iteration
        if (stop) return;
    }
}

template <int KIND, int NT>
__global__ __launch_bounds__(NT) void k_small(SmallArgs a) {
    small_loop<KIND, NT>(a);
}

// Batched solves (ellp_batch_solve_with_initial): workgroup b runs the LP of items[b] — its own arrays, DevState, rbuf / kbuf /
// flist and its own dynamic LDS — exactly as k_small runs it alone.  An item that ends (or has ended in an earlier launch)
// retires its workgroup only.  The address of the item is uniform and the items are never written during the launch, so
// the copy below comes in with scalar loads, once, ahead of the loop.
template <int KIND, int NT>
__global__ __launch_bounds__(NT) void k_small_batch(const SmallArgs *__restrict__ items) {
    const SmallArgs a = items[blockIdx.x];
    small_loop<KIND, NT>(a);
}

// c . x of every LP of a batch (k_primal_obj's sum, one workgroup per item): the objective a primal single call reports
__global__ __launch_bounds__(1024) void k_primal_obj_batch(const SmallArgs *__restrict__ items) {
    const SmallArgs a = items[blockIdx.x];
    primal_obj(a.c_B, a.c_N, a.x, a.B_index, a.N_index, a.m, a.nN, a.st);
}

// ---- both phases of a primal solve inside the batch's launches (ellp_batch_primal_solve) ----
// The LU-per-iteration loops carry no inverse: a phase starts from x, B_index, N_index, Nb, the costs and the bounds.  So the
// workgroup that ends an item's phase 1 makes the checks of solve() (primal_simplex_solver.rs:42-55), the hand-off of
// PrimalPhase2::from_phase1 (k_rephase's re-gather and relabel, the reset of ellp_engine_rephase) and goes on into phase 2
// itself, while its neighbours are wherever they are.  DevState and the loops' arguments stay as they are; what the two
// phases need beyond them is here.
struct BatchPhaseRec {  // per item, in the slab: read by the host between launch rounds and with the results
    int32_t phase;    // 1 / 2: the phase the item's DevState belongs to
    int32_t done;     // the solve has ended: no further launch takes the item
    int32_t verdict;  // 0, or the status the checks after phase 1 ended the solve with (ELLP_ERR_PANIC, ELLP_INFEASIBLE)
    int32_t pad;
    unsigned long long iters1;  // loop bodies of phase 1, once it has been handed off
    double obj1;                // c1 . x after phase 1 (NaN until phase 1 has ended Optimal)
};
struct BatchPhaseArgs {
    const double *c1;  // phase 1's costs by variable (the loop has them gathered only)
    const double *c2, *lb2, *ub2;
    const uint8_t *kind2;
    BatchPhaseRec *rec;
    int64_t n_c;
    unsigned long long max_iter;  // loop bodies each phase may run (opts.max_iter)
};

// k_primal_obj's sum by a workgroup of NT threads: thread t stands in for the threads t, t + NT, ... of its 1,024, wave by
// wave, so every partial sum and their order are that kernel's.  It gives phase 2 the starting objective of a fresh seam
// call; the objective a solve reports does not depend on it (k_primal_obj_batch forms it anew for every item at the end
// of the chunk), so this sum is the first thing to drop should the twins' registers need it.
template <int NT>
__device__ __forceinline__ void primal_obj_wg(const double *c_B, const double *c_N, const double *x, const int64_t *B_index,
                                              const int64_t *N_index, int64_t m, int64_t nN, DevState *st, double *s_p) {
    for (int v0 = 0; v0 < 1024; v0 += NT) {
        const int v = v0 + (int)threadIdx.x;
        double acc = 0.0;
        for (int64_t i = v; i < m; i += 1024) acc = fma(c_B[i], x[B_index[i]], acc);
        for (int64_t j = v; j < nN; j += 1024) {
            const double cj = c_N[j];
            if (cj != 0.0) acc = fma(cj, x[N_index[j]], acc);
        }
        acc = wave_sum(acc);
        if ((v & 63) == 0) s_p[v >> 6] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += s_p[w];
        st->obj = t;
    }
}

// One launch's share of an item's solve: at most item.max_iters loop bodies, of phase 1, of phase 2, or of both with the
// hand-off in between.  Loop::run is the item's loop (small_loop / mid_loop), called from ONE place: the second trip runs
// phase 2 on the same arrays, LDS scratch included (every thread is past the barrier below before the loop starts again).
template <int NT, class Loop, class Args>
__device__ __forceinline__ void batch_two_phase(const Args &item, const BatchPhaseArgs &pb) {
    __shared__ double s_po[16];
    BatchPhaseRec *rec = pb.rec;
    if (rec->done) return;
    DevState *st = item.st;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t m = item.m, nN = item.nN;
    int phase = rec->phase;
    unsigned long long left = item.max_iters;  // the launch's cap, for both phases together
#pragma unroll 1
    for (int trip = 0; trip < 2; ++trip) {
        Args a = item;
        if (phase == 2) {
            a.lb = pb.lb2;
            a.ub = pb.ub2;
            a.kind = pb.kind2;
        }
        const unsigned long long it0 = st->iters, rem = pb.max_iter - it0;
        a.max_iters = left < rem ? left : rem;
        // The loop's thread 0 counts its first body before the loop's first barrier: no wave may enter it before every
        // wave has read the count above, or a late wave would see it + 1, run one body fewer and unpair the barriers.
        __syncthreads();
        if (nN > 0) Loop::run(a);  // without nonbasic columns the seam is Optimal as it stands (primal…:149-151)
        __threadfence_block();
        __syncthreads();
        const unsigned long long it1 = st->iters;
        const int status = nN > 0 ? st->status : (int)ELLP_OPTIMAL;
        left -= it1 - it0;
        if (phase == 2 || status != ELLP_OPTIMAL) {
            if (tid == 0 && (status != ST_RUNNING || it1 >= pb.max_iter)) rec->done = 1;
            return;
        }
        // ---- the checks of solve() on c1 . x, summed in index order as StandardForm::obj sums it; every wave forms the
        // whole sum (64 products at a time, added one after the other), so no broadcast is needed
        double obj = 0.0;
        for (int64_t i0 = 0; i0 < pb.n_c; i0 += 64) {
            const int64_t i = i0 + lane;
            const double p = i < pb.n_c ? pb.c1[i] * item.x[i] : 0.0;
            const int cnt = pb.n_c - i0 < 64 ? (int)(pb.n_c - i0) : 64;
            for (int u = 0; u < cnt; ++u) obj += readlane_f64(p, u);
        }
        const int verdict = !(obj > -item.eps) ? (int)ELLP_ERR_PANIC : (!(obj < item.eps) ? (int)ELLP_INFEASIBLE : 0);
        if (tid == 0) {
            rec->obj1 = obj;
            if (verdict) {
                rec->verdict = verdict;
                rec->done = 1;
            }
        }
        if (verdict) return;
        __syncthreads();  // every thread has read phase 1's status and count
        // ---- PrimalPhase2::from_phase1: costs by the current index sets, Free labels (k_rephase); a fresh seam's state
        for (int64_t k = tid; k < m; k += NT) item.c_B[k] = pb.c2[item.B_index[k]];
        for (int64_t k = tid; k < nN; k += NT) {
            const int64_t j = item.N_index[k];
            item.c_N[k] = pb.c2[j];
            if (pb.kind2[j] == ELLP_BOUND_FREE) item.Nb[k] = ELLP_NB_FREE;
        }
        if (tid == 0) {
            rec->iters1 = it1;
            rec->phase = 2;
            st->status = ST_RUNNING;
            st->panic_code = 0;
            st->iters = 0;
            st->pivots = 0;
            st->flips = 0;
            st->lambda = 0.0;
        }
        __threadfence_block();
        __syncthreads();
        primal_obj_wg<NT>(item.c_B, item.c_N, item.x, item.B_index, item.N_index, m, nN, st, s_po);
        __threadfence_block();
        __syncthreads();
        phase = 2;
    }
}

template <int NT>
struct SmallPrimalLoop {
    static __device__ __forceinline__ void run(const SmallArgs &a) { small_loop<0, NT>(a); }
};

// k_small_batch<0, NT> for a whole primal solve: workgroup b runs the LP of items[b] through both phases (phases[b])
template <int NT>
__global__ __launch_bounds__(NT) void k_small_batch_primal(const SmallArgs *__restrict__ items,
                                                           const BatchPhaseArgs *__restrict__ phases) {
    const SmallArgs a = items[blockIdx.x];
    const BatchPhaseArgs pb = phases[blockIdx.x];
    batch_two_phase<NT, SmallPrimalLoop<NT>>(a, pb);
}

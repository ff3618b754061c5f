// ellp_mid.inc — the reference's loop, literally, for LPs whose basis no longer fits LDS (128 < m <= 1024):
// ONE persistent workgroup runs whole iterations of
//   primal  src/solvers/primal/primal_simplex_solver.rs:160-235 (+ pivot() :238-435)
//   dual    src/solvers/dual/dual_simplex_solver.rs:188-334
// with the LU of A_B re-done EVERY iteration (primal…:173, dual…:241), as ellp_small.inc does for m <= 128 — the
// same arithmetic as the CPU oracle (oracle/ellp_oracle.c: lu_factor_inplace, lu_btran, lu_solve), operation for
// operation, so pivots, point and duals are the oracle's bit for bit.  Why it exists: an explicit inverse carried
// by eta updates is only good to cond * 1e-16; on block-diagonal replications of the netlib LPs (m = 148 … 336)
// the explicit-inverse loop ends wrongly on 10-40 % of the variable orders (tests/campaign/blockdiag_cpu.py), the
// LU-per-iteration loop does not.
//
// What differs from ellp_small.inc is where the factors live and how the m sequential steps are organised:
//   * the matrix is in global memory (L2-resident: 0.9 MB at m = 336), column-major with PHYSICAL rows — rows are
//     never moved; thread t owns row t for the whole iteration and carries the position `pos` the reference's
//     row swaps would have given it (lop: position -> row lives in LDS);
//   * the LU is blocked by panels of 16 columns: a panel is factored in REGISTERS (thread t holds its row's 16
//     entries; a step is one DPP pivot search, one LDS record per wave, one barrier), then the columns to the
//     right get the panel's 16 eliminations at once — per element the same operations in the same order as the
//     reference's right-looking loop (a <- (-u_kj) * l_rk + a for k ascending), so the bits are the same; the
//     pivot rows of a column are finished by one lane per column (a 16 x 16 unit-lower solve), columns whose
//     pivot-row entries are all zero are not touched at all (the oracle's own `a == 0` skip — on the sparse
//     bases of real LPs that is most of them);
//   * U is written a second time, row-major by position (Ut), as its entries become final: the transposed
//     solve of BTRAN walks rows of U;
//   * the triangular solves are blocked by 16 positions: one wave finishes a diagonal block with readlane
//     broadcasts (no barrier inside), everybody else applies the block's 16 updates in order from registers
//     they prefetched — m/16 barrier pairs instead of m;
//   * L^T w = u~ is the dependent chain it is in the oracle (the first term of every sum is the one that
//     becomes known last): all threads stage the next row's products in LDS while one wave adds the current
//     row's, skipping zero products (exact: the accumulator starts at +0 and can never become -0);
//   * pricing reads a row-major copy of A_N (A_Nt, rebuilt at every launch, one column rewritten per pivot):
//     lane j accumulates column j's dot product in row order with coalesced loads.
//
// What does NOT differ is not written twice: the stages between the solves (column classification, the first-minimum and
// entering folds, bound-flip bookkeeping, commit) are the functions of ellp_loop_stages.inc that small_loop calls, on the
// scalar rules of ellp_rules.inc.  This file keeps the loop's skeleton (barriers, fences, stamps, early returns), the
// factorisation and the solves, and the three stages that file names as left in place (leaving row, primal ratio test,
// chunk maximum).
//
// Included inside the anonymous namespace of ellp_engine.hip after ellp_small.inc.

struct MidArgs {
    double *A_B, *A_N, *A_Nt, *c_B, *c_N, *x, *y, *dd;
    const double *lb, *ub;
    const uint8_t *kind;
    int64_t *B_index, *N_index;
    uint8_t *Nb;
    double *rbuf, *kbuf;  // per nonbasic position: r_j / alpha_j, Dantzig key / dual ratio
    double *LUa, *Ut;     // ld x m column-major (physical rows): L multipliers + U; m x ld row-major by position: U
    DevState *st;
    int64_t m, ld, nN, ldn;
    unsigned long long max_iters;
    int nch;  // chunks of 64 nonbasic positions
    double eps;
    Trace trace;
    unsigned long long *stamps;  // measurement (ELLP_SMALL_STAMPS): 100 MHz ticks per phase of the iteration, or null
    int maxviol;  // dual, an extension (ELLP_FLAG_DUAL_MAX_VIOLATION): the leaving row of largest violation, first of equals
    // certified hybrid, dual hand-over (oracle/ellp_oracle.c: hybrid_resync): before the first iteration of this launch
    // x_B = A_B^-1 (b - A_N x_N), y = A_B^-T c_B, d = c - A^T y from a fresh LU of the basis — the explicit-inverse loop
    // that ran before has carried them with the errors of its alpha, and the leaving-row test compares x_B with its
    // bounds to within EPS
    int resync;  // 1: x_B; 2: x_B, y and d
    const double *b;
    int bflip;  // dual, an extension (ELLP_FLAG_DUAL_BOUND_FLIPPING): see SmallArgs
    long long *flist;
};

constexpr int MID_MAX_M = 1024;
constexpr int MID_NB = 16;   // panel width = block size of the solves
// columns per tile of the trailing update
__host__ __device__ constexpr int mid_jt(int nt) { return nt >= 512 ? 512 : 256; }

inline int mid_threads(int64_t m) { return m <= 256 ? 256 : (m <= 512 ? 512 : 1024); }

// The four big phases (LU, the two transposed solves, FTRAN) are functions of their own (`__noinline__`: inlined into the
// kernel they push it to 256 VGPRs and hundreds of spilled SGPRs).  Across a call the compiler no longer knows which
// address space a pointer is in and would fall back to FLAT loads and stores for everything — LDS included, every
// access waiting on both counters (measured: 5 us per pivot step instead of 0.5).  So the functions get ONE pointer,
// the base of the dynamic LDS with its address space in the type; the kernel's arguments are parked at that base and
// every pointer a function uses is re-typed (global: address_space(1), LDS: address_space(3)) where it is fetched.
#define MID_AS1 __attribute__((address_space(1)))
#define MID_AS3 __attribute__((address_space(3)))
typedef MID_AS1 double gf64;
typedef MID_AS1 unsigned long long gu64;
typedef MID_AS3 double lf64;
typedef MID_AS3 int32_t li32;
typedef MID_AS3 long long li64;
typedef MID_AS3 unsigned char lu8;
typedef MID_AS3 const MidArgs largs;

constexpr int MID_ARGS_BYTES = (int)((sizeof(MidArgs) + 255) / 256 * 256);

// byte offsets of the arrays in the dynamic LDS (shared by the host, which needs the total, and the device)
struct MidOff {
    int v1, v2, lam, ws, ud;     // m doubles each: u / rho; d / alpha_q; lambda_i; work vector by position; diagonal of U
    int cmx, cps;                // nch doubles / long longs
    int nUt;                     // mid_jt x 16 doubles (negated pivot-row entries of a tile); also the L^T product rows (2 x m)
    int recM, recD, recR;        // per parity and wave: candidate modulus, value, rest of its row (16)
    int L11;                     // 2 x 16 x 16
    int xb;                      // 2 x 16
    int recI;                    // per parity and wave: position, row
    int bidx, lop;               // m int32 each
    int prow, nzm, list, cnt;    // 16, mid_jt, mid_jt, 8 int32
    int dpos;                    // m bytes
    int bytes;
};
__host__ __device__ inline MidOff mid_offsets(int64_t m, int nch, int nt) {
    MidOff o;
    const int nw = nt / 64;
    int64_t d = MID_ARGS_BYTES;
    auto take = [&](int64_t n) { const int64_t at = d; d += n; return (int)at; };
    o.v1 = take(8 * m);
    o.v2 = take(8 * m);
    o.lam = take(8 * m);
    o.ws = take(8 * m);
    o.ud = take(8 * m);
    o.cmx = take(8 * (int64_t)nch);
    o.cps = take(8 * (int64_t)nch);
    const int jt = mid_jt(nt);
    const int64_t tile = (int64_t)MID_NB * jt > 2 * m ? (int64_t)MID_NB * jt : 2 * m;
    o.nUt = take(8 * tile);
    o.recM = take(8 * 2 * nw);
    o.recD = take(8 * 2 * nw);
    o.recR = take(8 * 2 * nw * 16);
    o.L11 = take(8 * 512);
    o.xb = take(8 * 32);
    o.recI = take(4 * 8 * nw);
    o.bidx = take(4 * m);
    o.lop = take(4 * m);
    o.prow = take(4 * 16);
    o.nzm = take(4 * jt);
    o.list = take(4 * jt);
    o.cnt = take(4 * 8);
    o.dpos = take(m + 64);
    o.bytes = (int)((d + 15) / 16 * 16);
    return o;
}
// bytes of dynamic LDS k_mid needs (0: does not fit / not this path's size)
inline size_t mid_lds_bytes(int64_t m, int64_t nN) {
    if (m > MID_MAX_M || m <= SMALL_MAX_M) return 0;
    const int64_t nch = (nN + 63) / 64;
    if (nch > 4096) return 0;
    const MidOff o = mid_offsets(m, (int)nch, mid_threads(m));
    return o.bytes <= 150 * 1024 ? (size_t)o.bytes : 0;
}

// A_Nt[i * ldn + j] = A_N[j * ld + i], the 32 x 32 tile at rows 32 bx, columns 32 by
__device__ __forceinline__ void mid_transpose_tile(double (*tile)[33], const double *A_N, double *A_Nt, int64_t m, int64_t ld,
                                                   int64_t nN, int64_t ldn, unsigned bx, unsigned by) {
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const int64_t i0 = (int64_t)bx * 32, j0 = (int64_t)by * 32;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t j = j0 + ty + 8 * k, i = i0 + tx;
        tile[ty + 8 * k][tx] = (j < nN && i < m) ? A_N[j * ld + i] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = i0 + ty + 8 * k, j = j0 + tx;
        if (i < m && j < nN) A_Nt[i * ldn + j] = tile[tx][ty + 8 * k];
    }
}
__global__ __launch_bounds__(256) void k_mid_transpose(const double *A_N, double *A_Nt, int64_t m, int64_t ld, int64_t nN, int64_t ldn) {
    __shared__ double tile[32][33];
    mid_transpose_tile(tile, A_N, A_Nt, m, ld, nN, ldn, blockIdx.x, blockIdx.y);
}
// the same for every item of a batch launch (k_mid_batch): item blockIdx.z; the grid covers the largest item, the tiles
// beyond an item's own m x nN leave
__global__ __launch_bounds__(256) void k_mid_transpose_batch(const MidArgs *__restrict__ items) {
    __shared__ double tile[32][33];
    const MidArgs &a = items[blockIdx.z];
    if ((int64_t)blockIdx.x * 32 >= a.m || (int64_t)blockIdx.y * 32 >= a.nN) return;
    mid_transpose_tile(tile, a.A_N, a.A_Nt, a.m, a.ld, a.nN, a.ldn, blockIdx.x, blockIdx.y);
}

#define MID_STAMP(slot)                                     \
    if (stamps && tid == 0) {                               \
        const unsigned long long _t = wall_clock64();       \
        stamps[slot] += _t - t_prev;                        \
        t_prev = _t;                                        \
    }

// ---------------------------------------------------------------------------------------------------------
// LU of A_B (nalgebra's LU::new as restated by the oracle's lu_factor_inplace): pivot = FIRST entry of maximal
// modulus in the column, a zero pivot column is skipped, multipliers a * (1/diag), trailing update
// c[r] = (-c_k[i]) * l[r] + c[r].  On return: LUa holds L (multipliers, physical rows) and U (physical rows),
// Ut the rows of U by position, `pos` this thread's row position, L.lop the inverse map, `udiag` (thread i) and
// L.ud[i] the diagonal entry U_ii.
struct MidRow {
    int pos;
    double udiag;
};
// max / min over the first 16 lanes (one DPP row); v must not be NaN
__device__ __forceinline__ double row16_max(double v) {
    v = fmax(v, dpp_f64<0xB1>(v));
    v = fmax(v, dpp_f64<0x4E>(v));
    v = fmax(v, dpp_f64<0x141>(v));
    v = fmax(v, dpp_f64<0x140>(v));
    return readlane_f64(v, 0);
}
__device__ __forceinline__ int row16_min(int v) {
    v = min(v, dpp_i32<0xB1>(v));
    v = min(v, dpp_i32<0x4E>(v));
    v = min(v, dpp_i32<0x141>(v));
    v = min(v, dpp_i32<0x140>(v));
    return __builtin_amdgcn_readlane(v, 0);
}
template <int NT>
__device__ __noinline__ MidRow mid_lu(lu8 *base, int tid) {
    largs *pa = reinterpret_cast<largs *>(base);
    const int m = (int)pa->m;
    const int64_t ld = pa->ld;
    const MidOff o = mid_offsets(m, pa->nch, NT);
    gu64 *stamps = (gu64 *)pa->stamps;
    gf64 *LUa = (gf64 *)pa->LUa;
    gf64 *Ut = (gf64 *)pa->Ut;
    const gf64 *A_B = (const gf64 *)pa->A_B;
    lf64 *recM = reinterpret_cast<lf64 *>(base + o.recM);
    lf64 *recD = reinterpret_cast<lf64 *>(base + o.recD);
    lf64 *recR = reinterpret_cast<lf64 *>(base + o.recR);
    li32 *recI = reinterpret_cast<li32 *>(base + o.recI);
    lf64 *L11 = reinterpret_cast<lf64 *>(base + o.L11);
    li32 *prow = reinterpret_cast<li32 *>(base + o.prow);
    lf64 *nUt = reinterpret_cast<lf64 *>(base + o.nUt);
    li32 *nzm = reinterpret_cast<li32 *>(base + o.nzm);
    li32 *list = reinterpret_cast<li32 *>(base + o.list);
    li32 *cnt = reinterpret_cast<li32 *>(base + o.cnt);
    li32 *lop = reinterpret_cast<li32 *>(base + o.lop);
    lf64 *ud = reinterpret_cast<lf64 *>(base + o.ud);
    constexpr int NW = NT / 64;
    constexpr int JT = mid_jt(NT);
    const int lane = tid & 63, wave = tid >> 6;
    int pos = tid < m ? tid : 0x7fffffff;  // rows beyond m never take part
    double udiag = 0.0;
    unsigned long long t_prev = stamps ? wall_clock64() : 0ull;
    for (int kp = 0; kp < m; kp += MID_NB) {
        const gf64 *src = kp == 0 ? A_B : (const gf64 *)LUa;  // the first panel's pass over the matrix is also the copy A_B -> LUa
        double p[MID_NB];
#pragma unroll
        for (int c = 0; c < MID_NB; ++c) p[c] = (tid < m && kp + c < m) ? src[(int64_t)(kp + c) * ld + tid] : 0.0;
        if (stamps) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
        MID_STAMP(10)
#pragma unroll
        for (int c = 0; c < MID_NB; ++c) {
            const int i = kp + c;
            if (i < m) {
                // ---- pivot search over the rows at positions i..m-1: this wave's candidate
                const double cur = p[c];
                const bool cand = tid < m && pos >= i;
                double v = -1.0;
                if (cand) {
                    v = fabs(cur);
                    if (v != v) v = (pos == i) ? INFINITY : -1.0;  // `v > best` is false for a NaN: only position i itself can carry one
                }
                const double M = wave_allmax_dpp(v);
                const bool tied = cand && v == M;
                unsigned long long bl = __ballot(tied);
                if (__popcll(bl) > 1) {  // several entries of that modulus (the +-1 of slack columns): the first by position
                    const int pm = wave_allmin_dpp(tied ? pos : 0x7fffffff);
                    bl = __ballot(tied && pos == pm);
                }
                const int par = i & 1;
                const int lw = bl ? __ffsll((long long)bl) - 1 : 0;
                if (lane == lw) {  // the record: modulus, position | value, row, which of the row's later entries are not zero | they
                    const int slot = par * NW + wave;
                    int nz = 0;
#pragma unroll
                    for (int c2 = c + 1; c2 < MID_NB; ++c2) {
                        recR[slot * 16 + c2] = p[c2];
                        if (p[c2] != 0.0) nz |= 1 << c2;  // NaN != 0: such a column is updated, as in the oracle
                    }
                    recM[slot] = bl ? M : -2.0;
                    recD[slot] = cur;
                    recI[4 * slot] = pos;
                    recI[4 * slot + 1] = tid;
                    recI[4 * slot + 2] = nz;
                }
                lds_barrier();  // one barrier per step: the records are double-buffered by the parity of the step
                // ---- the winner among the waves' candidates: lane w looks at wave w's record
                int bw;
                {
                    const bool has = lane < NW;
                    const double wm = has ? recM[par * NW + lane] : -3.0;
                    const int wp = has ? recI[4 * (par * NW + lane)] : 0x7fffffff;
                    const double best = row16_max(wm);
                    const int pm = row16_min((has && wm == best) ? wp : 0x7fffffff);
                    const unsigned long long wb = __ballot(has && wm == best && wp == pm);
                    bw = __ffsll((long long)wb) - 1;
                }
                const int slot = par * NW + bw;
                const double diag = recD[slot];
                const int pmin = recI[4 * slot], P = recI[4 * slot + 1];
                const int nz = __builtin_amdgcn_readfirstlane(recI[4 * slot + 2]);
                double ak[MID_NB];
#pragma unroll
                for (int c2 = c + 1; c2 < MID_NB; ++c2) ak[c2] = recR[slot * 16 + c2];
                if (tid == i) udiag = diag;
                if (diag != 0.0) {
                    const double inv_diag = 1.0 / diag;
                    // ---- the pivot's row takes position i, the row that had it takes the pivot's
                    if (pmin != i) {
                        if (pos == i) pos = pmin;
                        else if (tid == P) pos = i;
                    }
                    // ---- multiplier of my row, elimination of my row within the panel
                    const bool below = tid < m && pos > i;
                    double l = 0.0;
                    if (below) {
                        l = cur * inv_diag;
                        p[c] = l;
                    }
#pragma unroll
                    for (int c2 = c + 1; c2 < MID_NB; ++c2) {
                        if ((nz >> c2) & 1) {  // uniform
                            if (below) p[c2] = (-ak[c2]) * l + p[c2];
                        }
                    }
                }
            }
        }
        MID_STAMP(11)
        // ---- the panel goes back: multipliers and U entries by physical row; U also by position; the 16 pivot rows
        // publish their multipliers (L11) and their row numbers for the columns to the right
        if (tid < m && pos >= kp) {
#pragma unroll
            for (int c = 0; c < MID_NB; ++c)
                if (kp + c < m) LUa[(int64_t)(kp + c) * ld + tid] = p[c];
            if (pos < kp + MID_NB) {
                const int ar = pos - kp;
                prow[ar] = tid;
#pragma unroll
                for (int c = 0; c < MID_NB; ++c) {
                    if (c < ar) L11[ar * 16 + c] = p[c];
                    else if (kp + c < m) Ut[(int64_t)pos * ld + kp + c] = p[c];
                }
            }
        }
        if (kp + MID_NB >= m) break;
        __syncthreads();
        MID_STAMP(12)
        const bool below16 = tid < m && pos >= kp + MID_NB;
        for (int j0 = kp + MID_NB; j0 < m; j0 += JT) {
            // ---- one lane per column: the column's 16 pivot-row entries through the unit-lower solve with L11
            if (tid < JT) {
                const int j = j0 + tid;
                int msk = 0;
                if (j < m) {
                    double e[MID_NB];
#pragma unroll
                    for (int ar = 0; ar < MID_NB; ++ar) e[ar] = src[(int64_t)j * ld + prow[ar]];
                    // per entry the eliminations c = 0, 1, ... in that order; column-of-L by column so that the 15 - c
                    // updates of a step are independent of each other
#pragma unroll
                    for (int c = 0; c < MID_NB - 1; ++c) {
                        const double ec = e[c];
                        const bool nzc = ec != 0.0;  // the oracle skips a zero pivot-row entry (keeps the sign of a zero)
#pragma unroll
                        for (int ar = c + 1; ar < MID_NB; ++ar) {
                            const double t = (-ec) * L11[ar * 16 + c] + e[ar];
                            e[ar] = nzc ? t : e[ar];
                        }
                    }
#pragma unroll
                    for (int ar = 0; ar < MID_NB; ++ar) {
                        LUa[(int64_t)j * ld + prow[ar]] = e[ar];
                        Ut[(int64_t)(kp + ar) * ld + j] = e[ar];
                        nUt[tid * 16 + ar] = -e[ar];
                        if (e[ar] != 0.0) msk |= 1 << ar;
                    }
                    if (kp == 0) msk |= 1 << 16;  // the first pass copies every column
                }
                const bool act = msk != 0;
                const unsigned long long bal = __ballot(act);
                if (act) {
                    const int k = __popcll(bal & ((1ull << lane) - 1ull));
                    list[wave * 64 + k] = tid;
                    nzm[tid] = msk;
                }
                if (lane == 0) cnt[wave] = __popcll(bal);
            }
            __syncthreads();
            MID_STAMP(13)
            // ---- every row below the panel: the 16 eliminations of its entry in each active column, in order
            if (below16) {
#pragma unroll 1
                for (int w = 0; w < JT / 64; ++w) {
                    const int n = cnt[w];
#pragma unroll 1
                    for (int k0 = 0; k0 < n; k0 += 8) {
                        int uu[8], mk[8];
                        double vv[8];
#pragma unroll
                        for (int q = 0; q < 8; ++q) {
                            uu[q] = list[w * 64 + (k0 + q < n ? k0 + q : k0)];
                            mk[q] = __builtin_amdgcn_readfirstlane(nzm[uu[q]]);
                            vv[q] = src[(int64_t)(j0 + uu[q]) * ld + tid];
                        }
#pragma unroll
                        for (int q = 0; q < 8; ++q) {
                            if (k0 + q < n) {
                                double val = vv[q];
                                const lf64 *nu = nUt + uu[q] * 16;
                                if ((mk[q] & 0xffff) == 0xffff) {  // a dense column: all 16, no tests
                                    double nv[MID_NB];
#pragma unroll
                                    for (int ar = 0; ar < MID_NB; ++ar) nv[ar] = nu[ar];
#pragma unroll
                                    for (int ar = 0; ar < MID_NB; ++ar) val = nv[ar] * p[ar] + val;
                                } else {
#pragma unroll
                                    for (int ar = 0; ar < MID_NB; ++ar)
                                        if ((mk[q] >> ar) & 1) val = nu[ar] * p[ar] + val;
                                }
                                LUa[(int64_t)(j0 + uu[q]) * ld + tid] = val;
                            }
                        }
                    }
                }
            }
            __syncthreads();
            MID_STAMP(14)
        }
    }
    __syncthreads();
    if (tid < m) {
        lop[pos] = tid;
        ud[tid] = udiag;
    }
    __syncthreads();
    return MidRow{pos, udiag};
}

// U^T x = b (nalgebra tr_solve_upper_triangular, oracle lu_tr_solve_upper): x_i = (b_i - sum_{k<i} U[k,i] x_k) / U_ii
// with the sum accumulated for k = 0, 1, ... in that order.  Thread i keeps b_i and its sum; blocks of 16: the wave
// that holds the block's 16 threads finishes them one after the other (readlane broadcasts), every later thread
// then adds the block's 16 terms in order.  Result to ws (by index).  Returns false on a zero diagonal.
template <int NT>
__device__ __noinline__ bool mid_tr_solve_upper(lu8 *base, int tid, double bi, double udiag) {
    largs *pa = reinterpret_cast<largs *>(base);
    const int m = (int)pa->m;
    const int64_t ld = pa->ld;
    const MidOff o = mid_offsets(m, pa->nch, NT);
    gu64 *stamps = (gu64 *)pa->stamps;
    gf64 *LUa = (gf64 *)pa->LUa;
    gf64 *Ut = (gf64 *)pa->Ut;
    (void)stamps; (void)LUa; (void)Ut; (void)ld;
    lf64 *xb = reinterpret_cast<lf64 *>(base + o.xb);
    lf64 *ws = reinterpret_cast<lf64 *>(base + o.ws);

    const int lane = tid & 63, wave = tid >> 6;
    if (__syncthreads_or(tid < m && udiag == 0.0)) return false;
    double dot = 0.0, xi = 0.0;
    // two sets of prefetched entries, used alternately (a register copy of a load still in flight would wait for it)
    double ua[MID_NB], ub[MID_NB];
    const int ti = tid < m ? tid : 0;
    auto fetch = [&](double (&u)[MID_NB], int kb0) {
#pragma unroll
        for (int ar = 0; ar < MID_NB; ++ar) u[ar] = Ut[(int64_t)(kb0 + ar < m ? kb0 + ar : m - 1) * ld + ti];  // unconditional (see ld_l); unused where tid <= kb0 + ar
    };
    auto block = [&](const double (&ut)[MID_NB], int kb) {
        const int nb = kb + MID_NB;
        const int par = (kb >> 4) & 1;
        if (wave == (kb >> 6)) {
            const int l0 = kb & 63;
#pragma unroll
            for (int ar = 0; ar < MID_NB; ++ar) {
                const int k = kb + ar;
                if (k < m) {
                    if (tid == k) {
                        double v = bi;
                        v -= dot;
                        v /= udiag;
                        xi = v;
                    }
                    const double xk = readlane_f64(xi, l0 + ar);
                    if (tid > k && tid < nb && tid < m) dot += ut[ar] * xk;
                }
            }
            if (lane >= l0 && lane < l0 + MID_NB) xb[par * 16 + lane - l0] = xi;
        }
        lds_barrier();
        if (tid >= nb && tid < m) {
            double xc[MID_NB];
#pragma unroll
            for (int ar = 0; ar < MID_NB; ++ar) xc[ar] = xb[par * 16 + ar];
#pragma unroll
            for (int ar = 0; ar < MID_NB; ++ar)
                if (kb + ar < m) dot += ut[ar] * xc[ar];
        }
    };
    fetch(ua, 0);
    for (int kb = 0; kb < m; kb += 2 * MID_NB) {
        fetch(ub, kb + MID_NB);
        block(ua, kb);
        if (kb + MID_NB >= m) break;
        fetch(ua, kb + 2 * MID_NB);
        block(ub, kb + MID_NB);
    }
    if (tid < m) ws[tid] = xi;
    __syncthreads();
    return true;
}

// L^T x = b, unit diagonal (oracle lu_tr_solve_lower_unit): x_i = b_i - sum_{k>i} L[k,i] x_k with the sum accumulated
// for k = i+1, i+2, ... — the FIRST term is the one that becomes known last, so the m^2/2 additions are one dependent
// chain.  In place on ws (by position).  Step i: every thread k stages the product L[k,i-1] x_k of the NEXT row
// (k >= i+1; x_k is final) and the raw L[i, i-1] in LDS — the loads were issued four rows earlier — while wave 0
// adds row i's products in order.  Zero products are skipped: the accumulator starts at +0, a sum of doubles is -0
// only if every term is, so it is never -0 and adding +-0 changes nothing.
template <int NT>
__device__ __noinline__ void mid_tr_solve_lower_unit(lu8 *base, int tid, int pos) {
    largs *pa = reinterpret_cast<largs *>(base);
    const int m = (int)pa->m;
    const int64_t ld = pa->ld;
    const MidOff o = mid_offsets(m, pa->nch, NT);
    gu64 *stamps = (gu64 *)pa->stamps;
    gf64 *LUa = (gf64 *)pa->LUa;
    gf64 *Ut = (gf64 *)pa->Ut;
    (void)stamps; (void)LUa; (void)Ut; (void)ld;
    lf64 *nUt = reinterpret_cast<lf64 *>(base + o.nUt);
    lf64 *ws = reinterpret_cast<lf64 *>(base + o.ws);
    const int lane = tid & 63, wave = tid >> 6;
    lf64 *P = nUt;  // two rows of m
    // thread `tid` owns physical row tid, which sits at position k = pos: it stages that position's terms (its loads
    // run down its own row of L: coalesced across the threads)
    const int k = tid < m ? pos : 0x7fffffff;
    // four loads in flight: lvA..lvD = L[k, r] for the next four rows to stage; the loop body is written out four times
    // with the roles rotated, so that no register copy ever touches a load still in flight
    double lvA = 0.0, lvB = 0.0, lvC = 0.0, lvD = 0.0;
    // unconditional, from a clamped address (a load under a branch makes the compiler drain ALL loads at the first use;
    // what a thread fetches for a row it has no term in is never used)
    auto ld_l = [&](int r) -> double { return LUa[(int64_t)(r > 0 ? r : 0) * ld + tid]; };
    // stage row m-2: one term, k = m-1, raw (its x is b_{m-1}, final already)
    if (k == m - 1) P[((m - 2) & 1) * m + k] = ld_l(m - 2);
    lvA = ld_l(m - 3);
    lvB = ld_l(m - 4);
    lvC = ld_l(m - 5);
    lvD = ld_l(m - 6);
    __syncthreads();
    double wnext = ws[m - 1];
    int i = m - 2;
#define MID_CHAIN_STEP(LV)                                                                                        \
    {                                                                                                             \
        /* everybody: stage row i-1 (terms k >= i; the one at k = i stays raw: x_i is being computed right now) */ \
        if (i >= 1 && k >= i && k < m) {                                                                          \
            const double xk = (k > i) ? ws[k] : 1.0;                                                              \
            P[((i - 1) & 1) * m + k] = LV * xk;                                                                   \
        }                                                                                                         \
        LV = ld_l(i - 5);                                                                                         \
        chain_row();                                                                                              \
        lds_barrier();                                                                                            \
        --i;                                                                                                      \
    }
    auto chain_row = [&]() {
        // ---- wave 0: x_i.  All of the row's products are fetched at once (lane l takes term i+1+l of every stretch
        // of 64), so that the stretches cost one LDS round trip together, not one each.
        if (wave == 0) {
            lf64 *Pi = P + (i & 1) * m;
            constexpr int NCH = NT / 64;
            const double bi = ws[i];
            double pr[NCH];
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                const int kk = i + 1 + 64 * ch + lane;
                pr[ch] = kk < m ? Pi[kk] : 0.0;
            }
            if (lane == 0) pr[0] = pr[0] * wnext;
            double dot = 0.0;
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                if (i + 1 + 64 * ch < m) {  // uniform
                    unsigned long long mask = __ballot(pr[ch] != 0.0);  // a NaN product is added, as in the oracle
                    if (mask) {
                        if (__popcll(mask) <= 10) {
                            while (mask) {
                                const int l = __ffsll((long long)mask) - 1;
                                dot += readlane_f64(pr[ch], l);
                                mask &= mask - 1;
                            }
                        } else {
                            // a dense stretch: every lane adds its 64 terms itself, in order, from LDS (two per 16-byte
                            // read); the stretch's first term may be the one that was still raw
                            if (ch == 0 && lane == 0) Pi[i + 1] = pr[0];
                            const lf64 *q = Pi + i + 1 + 64 * ch;
                            const int cntk = m - (i + 1 + 64 * ch) < 64 ? m - (i + 1 + 64 * ch) : 64;
                            int l = 0;
                            for (; l + 8 <= cntk; l += 8) {
                                double t[8];
#pragma unroll
                                for (int u = 0; u < 8; ++u) t[u] = q[l + u];
#pragma unroll
                                for (int u = 0; u < 8; ++u) dot += t[u];
                            }
                            for (; l < cntk; ++l) dot += q[l];
                        }
                    }
                }
            }
            wnext = bi - dot;
            if (lane == 0) ws[i] = wnext;
        }
    };
    while (i >= 0) {
        MID_CHAIN_STEP(lvA)
        if (i < 0) break;
        MID_CHAIN_STEP(lvB)
        if (i < 0) break;
        MID_CHAIN_STEP(lvC)
        if (i < 0) break;
        MID_CHAIN_STEP(lvD)
    }
#undef MID_CHAIN_STEP
}

// LU::solve (primal…:295, dual…:294; oracle lu_solve): x = P b; L y = x and U z = y as column sweeps, blocked by 16
// positions.  `mine` = entry of b on this thread's physical row = entry of P b at position pos.  Result: v2 by index.
// Wave 0 finishes the diagonal blocks; wave 1 stages the 16 x 16 diagonal blocks of L / U in LDS one block ahead (its
// loads are issued two blocks ahead); every thread prefetches the 16 entries of its row the next block multiplies.
template <int NT>
__device__ __noinline__ bool mid_lu_solve(lu8 *base, int tid, int pos, double mine) {
    largs *pa = reinterpret_cast<largs *>(base);
    const int m = (int)pa->m;
    const int64_t ld = pa->ld;
    const MidOff o = mid_offsets(m, pa->nch, NT);
    gu64 *stamps = (gu64 *)pa->stamps;
    gf64 *LUa = (gf64 *)pa->LUa;
    gf64 *Ut = (gf64 *)pa->Ut;
    (void)stamps; (void)LUa; (void)Ut; (void)ld;
    lf64 *ud = reinterpret_cast<lf64 *>(base + o.ud);
    lf64 *ws = reinterpret_cast<lf64 *>(base + o.ws);
    lf64 *L11 = reinterpret_cast<lf64 *>(base + o.L11);
    lf64 *xb = reinterpret_cast<lf64 *>(base + o.xb);
    li32 *lop = reinterpret_cast<li32 *>(base + o.lop);
    lf64 *v2 = reinterpret_cast<lf64 *>(base + o.v2);

    const int lane = tid & 63, wave = tid >> 6;
    if (__syncthreads_or(tid < m && ud[tid] == 0.0)) return false;
    lf64 *xs = ws;
    if (tid < m) xs[pos] = mine;
    double g[4] = {0.0, 0.0, 0.0, 0.0};
    // entry s of this lane of the diagonal block at kb0: (row ar, column c) = ((lane + 64 s) / 16, (lane + 64 s) % 16);
    // L: L[kb0 + ar, kb0 + c] for c < ar (by physical row); U: U[kb0 + ar, kb0 + c] for c > ar (by position)
    auto diag_L = [&](int kb0) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int ar = (lane + 64 * s) >> 4, c = (lane + 64 * s) & 15;
            const int pr_ = kb0 + ar < 0 ? 0 : (kb0 + ar < m ? kb0 + ar : m - 1), pc_ = kb0 + c < 0 ? 0 : (kb0 + c < m ? kb0 + c : m - 1);
            g[s] = LUa[(int64_t)pc_ * ld + lop[pr_]];  // unconditional, clamped; only c < ar of valid positions is used
        }
    };
    auto diag_U = [&](int kb0) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int ar = (lane + 64 * s) >> 4, c = (lane + 64 * s) & 15;
            const int pr_ = kb0 + ar < 0 ? 0 : (kb0 + ar < m ? kb0 + ar : m - 1), pc_ = kb0 + c < 0 ? 0 : (kb0 + c < m ? kb0 + c : m - 1);
            g[s] = Ut[(int64_t)pr_ * ld + pc_];  // unconditional, clamped; only c > ar of valid positions is used
        }
    };
    auto diag_put = [&](int buf) {
#pragma unroll
        for (int s = 0; s < 4; ++s) L11[buf * 256 + lane + 64 * s] = g[s];
    };
    // two sets of prefetched row entries, used alternately (a register copy of a load still in flight would wait for it)
    double la[MID_NB], lb[MID_NB];
    auto fetch = [&](double (&l)[MID_NB], int kb0) {
#pragma unroll
        for (int c = 0; c < MID_NB; ++c) {  // unconditional, clamped (see mid_tr_solve_lower_unit); used only where valid
            const int col = kb0 + c < 0 ? 0 : (kb0 + c < m ? kb0 + c : m - 1);
            l[c] = LUa[(int64_t)col * ld + tid];
        }
    };
    // ---- L y = x (unit diagonal): for i ascending, b[r] = (-b[i]) * L[r,i] + b[r] for r > i, skipped when b[i] == 0
    auto blockL = [&](const double (&lc)[MID_NB], int kb) {
        const int nb = kb + MID_NB;
        const int par = (kb >> 4) & 1;
        if (wave == 1) {
            diag_put(par ^ 1);
            diag_L(nb + MID_NB);
        } else if (wave == 0) {
            double xa = (lane < MID_NB && kb + lane < m) ? xs[kb + lane] : 0.0;
            double l11[MID_NB];
#pragma unroll
            for (int c = 0; c < MID_NB; ++c) l11[c] = L11[par * 256 + (lane & 15) * 16 + c];
#pragma unroll
            for (int c = 0; c < MID_NB - 1; ++c) {
                const double coeff = readlane_f64(xa, c);
                if (coeff != 0.0 && kb + c + 1 < m) {
                    if (lane > c && lane < MID_NB) xa = (-coeff) * l11[c] + xa;
                }
            }
            if (lane < MID_NB) xb[par * 16 + lane] = xa;
        }
        lds_barrier();
        if (tid < m) {
            if (pos >= nb) {
#pragma unroll
                for (int h = 0; h < MID_NB; h += 8) {  // eight coefficients per LDS round trip
                    double xc[8];
#pragma unroll
                    for (int c = 0; c < 8; ++c) xc[c] = xb[par * 16 + h + c];
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        const double coeff = xc[c];
                        if (coeff != 0.0 && kb + h + c < m) mine = (-coeff) * lc[h + c] + mine;
                    }
                }
                if (pos < nb + MID_NB) xs[pos] = mine;
            } else if (pos >= kb) {
                mine = xb[par * 16 + pos - kb];
            }
        }
        lds_barrier();
    };
    fetch(la, 0);
    if (wave == 1) {
        diag_L(0);
        diag_put(0);
        diag_L(MID_NB);
    }
    __syncthreads();
    for (int kb = 0; kb < m; kb += 2 * MID_NB) {
        fetch(lb, kb + MID_NB);
        blockL(la, kb);
        if (kb + MID_NB >= m) break;
        fetch(la, kb + 2 * MID_NB);
        blockL(lb, kb + MID_NB);
    }
    // ---- U z = y: for i descending, b[i] /= U_ii; b[r] = (-b[i]) * U[r,i] + b[r] for r < i, skipped when b[i] == 0
    auto blockU = [&](const double (&lc)[MID_NB], int kb) {
        const int pb = kb - MID_NB;  // the block below (next to be done)
        const int par = (kb >> 4) & 1;
        if (wave == 1) {
            diag_put(par ^ 1);
            diag_U(pb - MID_NB);
        } else if (wave == 0) {
            double ya = (lane < MID_NB && kb + lane < m) ? xs[kb + lane] : 0.0;
            const double dg = (lane < MID_NB && kb + lane < m) ? ud[kb + lane] : 1.0;
            double u11[MID_NB];
#pragma unroll
            for (int c = 0; c < MID_NB; ++c) u11[c] = L11[par * 256 + (lane & 15) * 16 + c];
#pragma unroll
            for (int c = MID_NB - 1; c >= 0; --c) {
                if (kb + c < m) {
                    if (lane == c) ya = ya / dg;
                    const double coeff = readlane_f64(ya, c);
                    if (coeff != 0.0) {
                        if (lane < c) ya = (-coeff) * u11[c] + ya;
                    }
                }
            }
            if (lane < MID_NB) xb[par * 16 + lane] = ya;
        }
        lds_barrier();
        if (tid < m) {
            if (pos < kb) {
#pragma unroll
                for (int h = 8; h >= 0; h -= 8) {  // eight coefficients per LDS round trip
                    double xc[8];
#pragma unroll
                    for (int c = 0; c < 8; ++c) xc[c] = xb[par * 16 + h + c];
#pragma unroll
                    for (int c = 7; c >= 0; --c) {
                        const double coeff = xc[c];
                        if (coeff != 0.0 && kb + h + c < m) mine = (-coeff) * lc[h + c] + mine;
                    }
                }
                if (pos >= pb) xs[pos] = mine;
            } else if (pos < kb + MID_NB) {
                mine = xb[par * 16 + pos - kb];
            }
        }
        lds_barrier();
    };
    const int kb_last = ((m - 1) / MID_NB) * MID_NB;
    if (tid < m && pos >= kb_last) xs[pos] = mine;
    fetch(la, kb_last);
    if (wave == 1) {
        diag_U(kb_last);
        diag_put((kb_last >> 4) & 1);
        diag_U(kb_last - MID_NB);
    }
    __syncthreads();
    for (int kb = kb_last; kb >= 0; kb -= 2 * MID_NB) {
        fetch(lb, kb - MID_NB);
        blockU(la, kb);
        if (kb - MID_NB < 0) break;
        fetch(la, kb - 2 * MID_NB);
        blockU(lb, kb - MID_NB);
    }
    if (tid < m) v2[pos] = mine;
    __syncthreads();
    return true;
}

// Pricing's dot product of one column of the row-major copy of A_N (cj: its first entry, stride ldn) with v1, accumulated in
// row order with eight loads in flight.  The caller clamps the address of a lane past the last column and loads
// unconditionally (DESIGN.md §3.1b).
__device__ __forceinline__ double mid_dot(const double *cj, int64_t ldn, int m, const double *v1) {
    double dot = 0.0;
    int i = 0;
    for (; i + 8 <= m; i += 8) {
        double pr[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) pr[u] = cj[(int64_t)(i + u) * ldn] * v1[i + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) dot += pr[u];
    }
    for (; i < m; ++i) dot += cj[(int64_t)i * ldn] * v1[i];
    return dot;
}

// The loop of k_mid for the LP of `a`, run by the whole workgroup.  A function of its arguments alone (no blockIdx), so
// that k_mid_batch can run one LP per workgroup with the same code (as small_loop is for k_small / k_small_batch).
template <int KIND, int NT>
__device__ __forceinline__ void mid_loop(const MidArgs a) {
    unsigned long long t_prev = a.stamps ? wall_clock64() : 0ull;
    unsigned long long c_prev = a.stamps ? clock64() : 0ull;
    constexpr int NW = NT / 64;
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ long long s_tmp[16];
    __shared__ double s_bad[16];
    __shared__ int s_stop, s_side, s_nan;
    __shared__ long long s_q, s_r;
    __shared__ double s_lambda, s_theta, s_delta;
    DevState *st = a.st;
    if (st->status != ST_RUNNING) return;
    const int m = (int)a.m;
    const int64_t ld = a.ld, nN = a.nN, ldn = a.ldn;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nch = a.nch;
    const MidOff o = mid_offsets(m, nch, NT);
    if (tid == 0) *reinterpret_cast<MidArgs *>(smem) = a;  // the phase functions fetch what they need from here
    lu8 *base = (lu8 *)smem;
    double *v1 = reinterpret_cast<double *>(smem + o.v1), *v2 = reinterpret_cast<double *>(smem + o.v2);
    double *lam = reinterpret_cast<double *>(smem + o.lam), *cmx = reinterpret_cast<double *>(smem + o.cmx);
    double *ws = reinterpret_cast<double *>(smem + o.ws), *ckm = reinterpret_cast<double *>(smem + o.nUt);
    long long *cps = reinterpret_cast<long long *>(smem + o.cps);
    int32_t *bidx = reinterpret_cast<int32_t *>(smem + o.bidx);
    uint8_t *dpos = reinterpret_cast<uint8_t *>(smem + o.dpos);
    unsigned long long *stamps = a.stamps;
    __syncthreads();
    const double eps = a.eps;

    if (KIND == 1 && a.resync) {
        // t = b - A_N x_N, column by column in position order (the oracle's order); x_N staged in rbuf first
        for (int64_t j = tid; j < nN; j += NT) a.rbuf[j] = a.x[a.N_index[j]];
        __threadfence_block();
        __syncthreads();
        const MidRow mr0 = mid_lu<NT>(base, tid);
        double t = 0.0;
        if (tid < m) {
            t = a.b[tid];
            const double *col = a.A_N + tid;
            int64_t j = 0;
            for (; j + 8 <= nN; j += 8) {  // eight loads in flight; the subtraction order is still j ascending
                double xv[8], av[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    xv[u] = a.rbuf[j + u];
                    av[u] = col[(j + u) * ld];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (xv[u] != 0.0) t = t - av[u] * xv[u];
            }
            for (; j < nN; ++j) {
                const double xj = a.rbuf[j];
                if (xj != 0.0) t = t - col[j * ld] * xj;
            }
        }
        if (mid_lu_solve<NT>(base, tid, mr0.pos, t)) {  // a singular basis keeps the carried x_B: the loop below reports it
            if (tid < m) a.x[a.B_index[tid]] = v2[tid];
            // y = B^-T c_B and d = c - A^T y from the same LU (dual_problem.rs:162-172 at this basis): the carried d has taken
            // theta_d * alpha_j with the explicit inverse's alpha_j at every pivot, and the phase objective the caller
            // tests against EPS (dual_simplex_solver.rs:45-50) is a sum over its entries
            const double cb = tid < m ? a.c_B[tid] : 0.0;
            if (a.resync >= 2 && mid_tr_solve_upper<NT>(base, tid, cb, mr0.udiag)) {
                mid_tr_solve_lower_unit<NT>(base, tid, mr0.pos);
                if (tid < m) v1[tid] = ws[mr0.pos];
                __syncthreads();
                if (tid < m) {
                    a.y[tid] = v1[tid];
                    a.dd[a.B_index[tid]] = 0.0;
                }
                for (int c = wave; c < nch; c += NW) {
                    const int64_t j = (int64_t)c * 64 + lane;
                    const double dot = mid_dot(a.A_Nt + (j < nN ? j : 0), ldn, m, v1);
                    if (j < nN) a.dd[a.N_index[j]] = a.c_N[j] - dot;
                }
            }
        }
        __threadfence_block();
        __syncthreads();
    }

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
            if (tid < m && dual_violation(a.B_index, a.x, a.kind, a.lb, a.ub, eps, tid, &dl, &sd)) {
                best = tid;
                bad = fabs(dl);
                if (bad != bad) bad = INFINITY;
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
                s_bad[wave] = bad;
            }
            __syncthreads();
            best = s_tmp[0];
            bad = s_bad[0];
            for (int w = 1; w < NW; ++w)
                if (a.maxviol ? (s_bad[w] > bad || (s_bad[w] == bad && s_tmp[w] < best)) : (s_tmp[w] < best)) {
                    best = s_tmp[w];
                    bad = s_bad[w];
                }
            lr = best == INT64_MAX ? -1 : best;
            if (tid == 0 && lr >= 0) {
                double delta = 0.0;
                int side = 0;
                dual_violation(a.B_index, a.x, a.kind, a.lb, a.ub, eps, lr, &delta, &side);
                s_delta = delta;
                s_side = side;
            }
        }
        MID_STAMP(0)
        // ---------------- lu = A_B.clone().lu()
        const MidRow mr = mid_lu<NT>(base, tid);
        const int pos = mr.pos;
        const double udiag = mr.udiag;
        MID_STAMP(1)
        if (KIND == 0) {  // primal…:175-179
            if (__syncthreads_or(tid < m && fabs(udiag) < eps)) {
                if (tid == 0) st->status = ELLP_ERR_SINGULAR;
                return;
            }
        } else if (lr < 0) {  // dual…:243-246
            if (tid == 0) st->status = ELLP_OPTIMAL;
            return;
        }
        // ---------------- BTRAN: u = B^-T c_B (primal…:184-187) / rho = row r of B^-1 (dual…:248-253)
        {
            const double bi = tid < m ? ((KIND == 0) ? a.c_B[tid] : (tid == lr ? 1.0 : 0.0)) : 0.0;
            if (!mid_tr_solve_upper<NT>(base, tid, bi, udiag)) {
                if (tid == 0) {
                    st->panic_code = KIND == 0 ? 187 : 249;
                    st->status = ELLP_ERR_PANIC;
                }
                return;
            }
            MID_STAMP(2)
            mid_tr_solve_lower_unit<NT>(base, tid, pos);
            if (tid < m) v1[tid] = ws[pos];  // u = P^-1 w
            __syncthreads();
        }
        MID_STAMP(3)
        // ---------------- pricing (primal…:189 + keys :253-270 / dual…:255-278), one column per lane, the dot
        // product accumulated in row order from the row-major copy of A_N
        const double delta = (KIND == 1) ? s_delta : 0.0;
        for (int c = wave; c < nch; c += NW) {
            const int64_t j = (int64_t)c * 64 + lane;
            double key = (KIND == 0) ? -INFINITY : INFINITY;
            long long ppos = -1;
            const double dot = mid_dot(a.A_Nt + (j < nN ? j : 0), ldn, m, v1);
            if (j < nN) classify_column<KIND>(a, j, dot, delta, eps, &s_nan, &key, &ppos);
            if (KIND == 0) {
                const double v = wave_allmax_dpp(key);  // keys are never NaN
                if (lane == 0) cmx[c] = v;
            } else {
                wave_first_min(&key, &ppos);  // lexicographic (ratio, position)
                if (lane == 0) {
                    cmx[c] = key;
                    cps[c] = ppos;
                }
            }
        }
        __syncthreads();
        if (s_nan) {
            if (tid == 0) st->status = ELLP_ERR_NAN;
            return;
        }
        MID_STAMP(4)
        // ---------------- entering variable
        if (wave == 0) enter_fold<KIND>(a, nch, nN, delta, eps, lane, cmx, cps, &s_q, &s_theta);
        __syncthreads();
        long long q = s_q;
        if (q < 0) {
            if (tid == 0) st->status = (KIND == 0) ? ELLP_OPTIMAL : ELLP_INFEASIBLE;  // primal…:289-292 / dual…:281-284
            return;
        }
        if (tid == 0) ELLP_CHECK(st, q < nN, 9141);
        double theta_sel = (KIND == 1) ? s_theta : 0.0;
        double delta_upd = delta;  // the leaving row's violation the updates use (after the bound flips, if any)
        if (KIND == 1 && a.bflip) {
            // extension: the long-step ratio test (oracle: g_dual_rule & 1; ellp_small.inc: bf_walk)
            double ck;
            const int nflip = bf_walk<NT>(a.kbuf, a.rbuf, a.N_index, a.kind, a.lb, a.ub, a.flist, nN, delta, (delta < 0.0) ? -theta_sel : theta_sel, q,
                                          tid, s_bad, s_tmp, &q, &ck);
            theta_sel = (delta < 0.0) ? -ck : ck;
            if (nflip > 0) {
                __syncthreads();  // flist is complete
                const double acc = tid < m ? flip_row_rhs(a, nflip, ld, tid) : 0.0;
                __syncthreads();  // every thread has read the labels before they change
                flip_relabel<NT>(a, nflip, tid);
                if (!mid_lu_solve<NT>(base, tid, pos, acc)) {
                    if (tid == 0) {
                        st->panic_code = 2940;
                        st->status = ELLP_ERR_PANIC;
                    }
                    return;
                }
                if (tid < m) {
                    const int64_t bi = a.B_index[tid];
                    a.x[bi] = a.x[bi] - v2[tid];
                }
                __threadfence_block();
                __syncthreads();
                delta_upd = flip_delta(a, lr, s_side);
                __syncthreads();  // v2 is the FTRAN's next
            }
        }
        // ---------------- FTRAN: d = +-B^-1 a_q (primal…:295-300) / alpha_q (dual…:294)
        const int64_t jq = a.N_index[q];
        {
            const double mine = tid < m ? a.A_N[q * ld + tid] : 0.0;
            if (!mid_lu_solve<NT>(base, tid, pos, mine)) {
                if (tid == 0) {
                    st->panic_code = KIND == 0 ? 295 : 294;
                    st->status = ELLP_ERR_PANIC;
                }
                return;
            }
        }
        MID_STAMP(5)
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
                // chunk minima: to the head of the tile buffer (free outside the LU)
                for (int c = 0; c < nck; ++c) {
                    const int i = c * 64 + lane;
                    const double cm = wave_min(i < m ? lam[i] : INFINITY);
                    if (lane == 0) ckm[c] = cm;
                }
                const int kq = a.kind[jq];  // primal…:305-311
                const double lambda0 = (kq == ELLP_BOUND_TWOSIDED) ? a.ub[jq] - a.lb[jq] : (kq == ELLP_BOUND_FIXED ? 0.0 : INFINITY);
                const RatioResult rr = ratio_fold(ckm, nck, m, lam, bidx, dpos, lambda0, eps, lane);
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
                if (tid < m) {
                    const double t = a.A_N[q * ld + tid];
                    const double tb = a.A_B[r * ld + tid];
                    a.A_N[q * ld + tid] = tb;
                    a.A_Nt[(int64_t)tid * ldn + q] = tb;
                    a.A_B[r * ld + tid] = t;
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
            if (tid < m) a.y[tid] = a.y[tid] + theta_d * v1[tid];
            const double theta_p = delta_upd / v2[r];
            if (tid < m) {
                const int64_t bi = a.B_index[tid];
                a.x[bi] = a.x[bi] - theta_p * v2[tid];
            }
            __syncthreads();
            if (tid < m) {
                const double t = a.A_B[r * ld + tid];
                const double tn = a.A_N[q * ld + tid];
                a.A_B[r * ld + tid] = tn;
                a.A_N[q * ld + tid] = t;
                a.A_Nt[(int64_t)tid * ldn + q] = t;
            }
            if (tid == 0) commit_dual_pivot(a, q, r, jq, lv, s_side, theta_d, theta_p, delta_upd, &s_stop);
        }
        __threadfence_block();
        __syncthreads();
        MID_STAMP(6)
        if (stamps && tid == 0) {
            stamps[8] += 1;
            const unsigned long long c_now = clock64();
            stamps[9] += c_now - c_prev;  // shader-clock cycles of the iteration (s_memtime)
            c_prev = c_now;
        }
        const int stop = s_stop;
        __syncthreads();  // thread 0 clears the flag at the top of the next iteration
        if (stop) return;
    }
}

template <int KIND, int NT>
__global__ __launch_bounds__(NT) void k_mid(MidArgs a) {
    mid_loop<KIND, NT>(a);
}

// Batched solves (ellp_batch_solve_with_initial): workgroup b runs the LP of items[b] — its own arrays, factors, DevState,
// rbuf / kbuf / flist and its own dynamic LDS — exactly as k_mid runs it alone; mid_loop parks the item in LDS where k_mid
// parks its argument.  The item's address is uniform and the items are never written during the launch (scalar loads).
template <int KIND, int NT>
__global__ __launch_bounds__(NT) void k_mid_batch(const MidArgs *__restrict__ items) {
    const MidArgs a = items[blockIdx.x];
    mid_loop<KIND, NT>(a);
}

template <int NT>
struct MidPrimalLoop {
    static __device__ __forceinline__ void run(const MidArgs &a) { mid_loop<0, NT>(a); }
};

// k_mid_batch<0, NT> for a whole primal solve (batch_two_phase, ellp_small.inc).  A_Nt is the copy of A_N the round's
// transpose made; the hand-off changes no column, so phase 2 goes on with it.
template <int NT>
__global__ __launch_bounds__(NT) void k_mid_batch_primal(const MidArgs *__restrict__ items,
                                                         const BatchPhaseArgs *__restrict__ phases) {
    const MidArgs a = items[blockIdx.x];
    const BatchPhaseArgs pb = phases[blockIdx.x];
    batch_two_phase<NT, MidPrimalLoop<NT>>(a, pb);
}

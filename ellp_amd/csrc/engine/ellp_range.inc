// ellp_range.inc — sensitivity ranging: the cost and right-hand-side ranges of the basis and point an engine stands on
// (ellp_engine_ranging), or of a point in host memory (ellp_ranging), and chosen rows of the tableau
// (ellp_engine_tableau_rows).  DESIGN.md §3.10; the definitions are in include/ellp_hip.h.
//
//   the postsolve       post_compute's steps first: the fresh LU of A_B stays in post_luw, d in post_d;
//   W = B^-1            row i solves A_B^T rho = e_i with that LU: k_range_solve<R>, R right-hand sides per workgroup, the
//                       grid over blocks of R rows.  Every workgroup walks the factors once (U^T forward, L^T backward, the
//                       transpositions in reverse), its R vectors in LDS as [k][r]; per vector the operations of k_lu_solve
//                       mode 1 in its order, so a row of W has the bits that kernel would give for e_i; then the entries a
//                       basic column with a single nonzero fixes on its own are imposed (k_range_snap, as k_post_snap on y);
//   inverse_residual    max |I - A_B W|, k_range_resid: every entry one sum in ascending k, product and sum rounded separately
//                       (what tests/ranging_model.py forms from the returned W, bit for bit); nanmax over tiles;
//   the tableau pass    k_range_tab<0>: W (row-major) x A_N (stored columns) on the matrix cores in k_gemm_mfma's shape (128 x 128
//                       tiles, BK = 16, two LDS buffers, register prefetch, ragged edges zero-filled on the way into LDS).
//                       Both operands are contiguous along k: four lanes take the 16 k of one row or column (one 128-byte
//                       line), transposed into LDS.  The epilogue forms the up and down candidates of every accumulator
//                       element from d, the label and the kind of its column, reduces them over the 16 lanes that share a
//                       row, the wave's two column tiles and the four waves of a row (LDS), and writes one record
//                       (up, up_pos, down, down_pos) per (row, column block); k_range_cfold folds the blocks.  T is never
//                       stored.  k_range_tab<1> is the same kernel with a storing epilogue and a row map (tableau_rows):
//                       one accumulator chain over k in ascending blocks of 4 in both, so alpha_ij has the same bits;
//   the rhs pass        k_range_rhs: one read of W, a thread per column k (coalesced along the row), four waves share the
//                       rows; x, kind, lb, ub through B_index.
// No floating-point atomics; min, max and the first-position tie-break are exact, so no result depends on a reduction order.
// Nothing the engine reads later is written (the workspace is the ranging's own, released by ellp_engine_destroy).
//
// Included at the end of ellp_engine.hip, after ellp_post.inc.

namespace {

constexpr int RNG_NOPOS = 0x7fffffff;  // "no position" of a limit

struct RngRec {
    double v;
    int p;
};
// the better of two candidates for the upper (UP = 1: the smaller) or the lower limit (the larger): NaN wins, of NaNs and
// of equals the smaller position.  Symmetric in its operands, so both sides of a butterfly hold the same record.
template <int UP>
__device__ __forceinline__ RngRec rng_pick(RngRec a, RngRec b) {
    const bool an = a.v != a.v, bn = b.v != b.v;
    if (an || bn) {
        if (an && bn) return a.p < b.p ? a : b;
        return an ? a : b;
    }
    if (UP ? (b.v < a.v) : (b.v > a.v)) return b;
    if (b.v == a.v) return a.p < b.p ? a : b;
    return a;
}
__device__ __forceinline__ double rng_pos(double v) { return (v != v) ? v : (v > 0.0 ? v : 0.0); }  // max(v, 0), keeps NaN, +0.0
__device__ __forceinline__ double rng_neg(double v) { return (v != v) ? v : (v < 0.0 ? v : 0.0); }  // min(v, 0)

// The candidates one tableau entry alpha gives the cost range of its row.  code: the label of the column (ELLP_NB_LOWER /
// UPPER / FREE) or 3 (kind Fixed, or no column: not read).  qu = +Inf / qd = -Inf: no candidate.  "+ 0.0" makes every zero
// +0.0.  A NaN alpha, or a NaN quotient on a side that is a candidate, makes both NaN.
__device__ __forceinline__ void rng_cost_cand(double al, double dv, int code, double eps, double &qu, double &qd) {
    qu = INFINITY;
    qd = -INFINITY;
    if (code == 3) return;
    if (al != al) {
        qu = qd = al;
        return;
    }
    const bool ps = al > eps, ns = al < -eps;
    if (!ps && !ns) return;
    double nu, nd;
    bool cu, cd;
    if (code == ELLP_NB_LOWER) {
        nu = nd = rng_pos(dv);
        cu = ps;
        cd = ns;
    } else if (code == ELLP_NB_UPPER) {
        nu = nd = rng_neg(dv);
        cu = ns;
        cd = ps;
    } else {
        nu = ps ? rng_pos(dv) : rng_neg(dv);
        nd = ps ? rng_neg(dv) : rng_pos(dv);
        cu = cd = true;
    }
    const double u = nu / al + 0.0, d = nd / al + 0.0;
    if ((cu && u != u) || (cd && d != d)) {
        qu = qd = NAN;
        return;
    }
    if (cu) qu = u;
    if (cd) qd = d;
}

// The candidates the basic variable of one row (x, its kind and bounds) gives the range of right-hand side k through w = W[i][k]
__device__ __forceinline__ void rng_rhs_cand(double w, double x, double lb, double ub, int kind, double eps, double &qu, double &qd) {
    qu = INFINITY;
    qd = -INFINITY;
    if (w != w) {
        qu = qd = w;
        return;
    }
    const bool ps = w > eps, ns = w < -eps;
    if (!ps && !ns) return;
    const bool has_u = kind == ELLP_BOUND_UPPER || kind == ELLP_BOUND_TWOSIDED || kind == ELLP_BOUND_FIXED;
    const bool has_l = kind == ELLP_BOUND_LOWER || kind == ELLP_BOUND_TWOSIDED || kind == ELLP_BOUND_FIXED;
    const bool cu = ps ? has_u : has_l, cd = ps ? has_l : has_u;
    const double to_u = has_u ? rng_pos(ub - x) : 0.0, to_l = has_l ? rng_pos(x - lb) : 0.0;
    const double u = (ps ? to_u / w : to_l / -w) + 0.0;
    const double d = (ps ? to_l / -w : to_u / w) + 0.0;
    if ((cu && u != u) || (cd && d != d)) {
        qu = qd = NAN;
        return;
    }
    if (cu) qu = u;
    if (cd) qd = d;
}

// ---- W = B^-1 by rows: R right-hand sides e_{i0}, .., e_{i0 + R - 1} per workgroup (512 threads: thread = (k slot, r)).
// range_solve_rows: on return x ([m][R], LDS; acc: as much again) holds the rows as [k][r], visible to every thread.  false: a
// zero on U's diagonal (the same for every thread), x is then not to be read.  Shared by k_range_solve and k_brange_solve
// (ellp_brange.inc)
template <int R>
__device__ __forceinline__ bool range_solve_rows(const double *M, const int64_t *piv, int64_t m, int64_t i0, double *x, double *acc, int tid) {
    constexpr int KS = 512 / R;
    const int r = tid % R, ks = tid / R;
    for (int64_t t = tid; t < m * R; t += 512) {
        x[t] = 0.0;
        acc[t] = 0.0;
    }
    __syncthreads();
    // U^T: x_i = (b_i - acc_i) / U_ii, then acc_k += U[i][k] x_i for every later k (k_lu_solve mode 1; b = e_{i0 + r})
    for (int64_t i = 0; i < m; ++i) {
        const double diag = M[i * m + i];
        if (diag == 0.0) return false;
        double xi = ((i == i0 + r) ? 1.0 : 0.0) - acc[i * R + r];
        xi = xi / diag;
        if (ks == 0) x[i * R + r] = xi;
        const double *urow = M + i * m;
        for (int64_t k = i + 1 + ks; k < m; k += KS) acc[k * R + r] = acc[k * R + r] + urow[k] * xi;
        __syncthreads();
    }
    // L^T: step k (descending) subtracts L[k][i] x_k from every earlier x_i, skipped for a zero x_k
    for (int64_t k = m - 1; k > 0; --k) {
        const double xk = x[k * R + r];
        if (xk != 0.0) {
            const double *lrow = M + k * m;
            for (int64_t i = ks; i < k; i += KS) x[i * R + r] = x[i * R + r] - lrow[i] * xk;
        }
        __syncthreads();
    }
    if (tid < R)
        for (int64_t i = m - 1; i >= 0; --i) {
            const int64_t p = piv[i];
            if (p != i) {
                const double t = x[i * R + tid];
                x[i * R + tid] = x[p * R + tid];
                x[p * R + tid] = t;
            }
        }
    __syncthreads();
    return true;
}
// the rows of range_solve_rows from LDS to W
template <int R>
__device__ __forceinline__ void range_store_rows(const double *x, int64_t m, int64_t i0, double *W, int64_t ldw, int tid) {
    for (int64_t t = tid; t < m * R; t += 512) {
        const int64_t rr = t / m, k = t - rr * m;
        if (i0 + rr < m) W[(i0 + rr) * ldw + k] = x[k * R + rr];
    }
}
template <int R>
__global__ __launch_bounds__(512) void k_range_solve(const double *M, const int64_t *piv, int64_t m, double *W, int64_t ldw, int *fail) {
    extern __shared__ __align__(16) unsigned char rng_smem[];
    double *x = reinterpret_cast<double *>(rng_smem);  // [m][R]: the solution
    double *acc = x + m * R;                           // [m][R]: sum_{k < i} U[k][i] x_k
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * R;
    if (!range_solve_rows<R>(M, piv, m, i0, x, acc, tid)) {
        if (tid == 0) *fail = 1;
        return;
    }
    range_store_rows<R>(x, m, i0, W, ldw, tid);
}

// A basic column with a single nonzero, column j = a e_k, states a W[i][k] = delta_ij on its own: W[j][k] = fl(1 / a) and an
// exact zero in every other row, as k_post_snap imposes on y (the elimination leaves 1e-17 there when row k was a pivot row
// before column j's turn: a componentwise backward error of 1).  One workgroup per column; sing_row, sing_val: k_post_singletons.
__global__ __launch_bounds__(256) void k_range_snap(double *W, const int64_t *sing_row, const double *sing_val, int64_t m, int64_t ldw) {
    const int64_t j = blockIdx.x, k = sing_row[j];
    if (k < 0) return;
    const double inv = 1.0 / sing_val[j];
    for (int64_t i = threadIdx.x; i < m; i += 256) W[i * ldw + k] = (i == j) ? inv : 0.0;
}

// ---- max |I - A_B W|: 64 x 64 tiles, a thread 4 x 4 entries, every entry one sum over k = 0 .. m-1 in ascending order
// the maximum of tile (ti, tj) by one workgroup of 256 threads; the value is thread 0's.  Shared by k_range_resid and
// k_brange_fold (ellp_brange.inc): a caller that takes several tiles needs no barrier between them (every tile has one
// between thread 0's read of s_red and the next write of it)
__device__ __forceinline__ double range_resid_tile(const double *A_B, const double *W, int64_t m, int64_t ld, int64_t ldw, int64_t ti, int64_t tj) {
    __shared__ double sa[16][64], sb[16][64], s_red[4];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int64_t i0 = ti * 64, j0 = tj * 64;
    double s[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) s[r][c] = 0.0;
    for (int64_t k0 = 0; k0 < m; k0 += 16) {
        const int64_t k = k0 + ty;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = i0 + tx * 4 + q, j = j0 + tx * 4 + q;
            sa[ty][tx * 4 + q] = (k < m && i < m) ? A_B[k * ld + i] : 0.0;
            sb[ty][tx * 4 + q] = (k < m && j < m) ? W[k * ldw + j] : 0.0;
        }
        __syncthreads();
        const int kn = (m - k0 < 16) ? (int)(m - k0) : 16;
        for (int kk = 0; kk < kn; ++kk) {
            double av[4], bv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                av[q] = sa[kk][ty * 4 + q];
                bv[q] = sb[kk][tx * 4 + q];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) s[r][c] = __dadd_rn(s[r][c], __dmul_rn(av[r], bv[c]));
        }
        __syncthreads();
    }
    double worst = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int64_t i = i0 + ty * 4 + r, j = j0 + tx * 4 + c;
            if (i < m && j < m) worst = nanmax(worst, fabs((i == j ? 1.0 : 0.0) - s[r][c]));
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) worst = nanmax(worst, __shfl_xor(worst, o));
    if ((tid & 63) == 0) s_red[tid >> 6] = worst;
    __syncthreads();
    return tid == 0 ? nanmax(nanmax(s_red[0], s_red[1]), nanmax(s_red[2], s_red[3])) : 0.0;
}
__global__ __launch_bounds__(256) void k_range_resid(const double *A_B, const double *W, int64_t m, int64_t ld, int64_t ldw, double *tilemax) {
    const double t = range_resid_tile(A_B, W, m, ld, ldw, blockIdx.y, blockIdx.x);
    if (threadIdx.x == 0) tilemax[blockIdx.y * gridDim.x + blockIdx.x] = t;
}
__global__ __launch_bounds__(256) void k_range_resmax(const double *tilemax, int64_t ntiles, double *out) {
    __shared__ double s_red[4];
    double worst = 0.0;
    for (int64_t t = threadIdx.x; t < ntiles; t += 256) worst = nanmax(worst, tilemax[t]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) worst = nanmax(worst, __shfl_xor(worst, o));
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = worst;
    __syncthreads();
    if (threadIdx.x == 0) *out = nanmax(nanmax(s_red[0], s_red[1]), nanmax(s_red[2], s_red[3]));
}

// ---- the tableau pass
struct RngTabArgs {
    const double *W;        // row-major, leading dimension ldw
    const int64_t *rowmap;  // the rows of W taken (null: 0 .. nrows - 1)
    const double *A_N;      // the stored columns, leading dimension ld
    const double *d;        // by variable
    const int64_t *N_index;
    const uint8_t *Nb, *kind;
    double *pu, *pd;        // STORE 0: the records, [column block][row]
    int32_t *ppu, *ppd;
    double *out;            // STORE 1: nrows x nN
    int64_t m, ld, ldw, nrows, nN;
    double eps;
    // STORE 2, 3 (ellp_cert.inc): the point, the bounds and the basis the ray's row test reads; the flag bytes
    const double *cx, *clb, *cub;
    const int64_t *cB;
    uint8_t *cbits;
};
// the epilogues of the certificate's searches (ellp_cert.inc): STORE 2 the Farkas row flags, STORE 3 the ray's column flags
template <int STORE>
__device__ __forceinline__ void cert_tab_epilogue(const RngTabArgs &a, const mfma_d4 (&acc)[4][2], int *scratch, int64_t bx, int64_t by);

// tile (row block by, column block bx) by one workgroup of 512 threads.  Shared by k_range_tab and k_brange_tab
// (ellp_brange.inc), which takes a and bx per workgroup from a table
template <int STORE>
__device__ __forceinline__ void range_tab_tile(const RngTabArgs &a, int64_t bx, int64_t by) {
    constexpr int BM = 128, BN = 128, BK = 16;
    __shared__ __align__(16) double sA[2][BK][BM];
    __shared__ __align__(16) double sB[2][BK][BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 2, wc = wave & 3;  // the wave's 64 x 32 piece
    const int64_t m = a.m;
    const int64_t i0 = by * BM, j0 = bx * BN;

    mfma_d4 acc[4][2];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[r][c] = mfma_d4{0.0, 0.0, 0.0, 0.0};

    // global -> register staging of one stage: thread t takes tile row (of W) and tile column (of A_N) t >> 2 and the 4
    // consecutive k = (t & 3) * 4 .. + 3 of each.  Loads are unconditional from clamped addresses; the zero fill of the ragged
    // edges is applied when the registers go to LDS, after the stage's MFMAs (k_gemm_mfma).
    const int tq = tid >> 2, tk = (tid & 3) * 4;
    const bool ia_ok = i0 + tq < a.nrows, jb_ok = j0 + tq < a.nN;
    int64_t ia = ia_ok ? i0 + tq : a.nrows - 1;
    if (a.rowmap) ia = a.rowmap[ia];
    const double *pa = a.W + ia * a.ldw;
    const double *pb = a.A_N + (jb_ok ? j0 + tq : a.nN - 1) * a.ld;
    const int64_t mlast = (m - 1) & ~(int64_t)1;  // a double2 from the last even index stays inside the row (ld, ldw are even)
    double2 ra[2], rb[2];
    auto load_stage = [&](int64_t k0) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int64_t k = k0 + tk + 2 * p < mlast ? k0 + tk + 2 * p : mlast;
            ra[p] = *reinterpret_cast<const double2 *>(pa + k);
            rb[p] = *reinterpret_cast<const double2 *>(pb + k);
        }
    };
    auto store_stage = [&](int buf, int64_t k0) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int64_t k = k0 + tk + 2 * p;
            sA[buf][tk + 2 * p][tq] = (ia_ok && k < m) ? ra[p].x : 0.0;
            sA[buf][tk + 2 * p + 1][tq] = (ia_ok && k + 1 < m) ? ra[p].y : 0.0;
            sB[buf][tk + 2 * p][tq] = (jb_ok && k < m) ? rb[p].x : 0.0;
            sB[buf][tk + 2 * p + 1][tq] = (jb_ok && k + 1 < m) ? rb[p].y : 0.0;
        }
    };

    const int fr = lane & 15, fk = lane >> 4;  // fragment coordinates of this lane
    load_stage(0);
    store_stage(0, 0);
    __syncthreads();
    int buf = 0;
    for (int64_t k0 = 0; k0 < m; k0 += BK) {
        const bool more = k0 + BK < m;
        if (more) load_stage(k0 + BK);  // in flight during the MFMAs below
#pragma unroll
        for (int k4 = 0; k4 < BK / 4; ++k4) {
            double af[4], bf[2];
#pragma unroll
            for (int r = 0; r < 4; ++r) af[r] = sA[buf][k4 * 4 + fk][wr * 64 + r * 16 + fr];
#pragma unroll
            for (int c = 0; c < 2; ++c) bf[c] = sB[buf][k4 * 4 + fk][wc * 32 + c * 16 + fr];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 2; ++c) acc[r][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[r], bf[c], acc[r][c], 0, 0, 0);
        }
        if (more) store_stage(buf ^ 1, k0 + BK);
        __syncthreads();
        buf ^= 1;
    }

    // ---- epilogue: element v of acc[r][c] is row i0 + wr * 64 + r * 16 + fk + 4 v, column j0 + wc * 32 + c * 16 + fr
    if constexpr (STORE >= 2) {  // sA is free: the last stage's readers are past the loop's final barrier
        cert_tab_epilogue<STORE>(a, acc, reinterpret_cast<int *>(&sA[0][0][0]), bx, by);
        return;
    }
    if (STORE) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int64_t i = i0 + wr * 64 + r * 16 + fk + 4 * v, j = j0 + wc * 32 + c * 16 + fr;
                    if (i < a.nrows && j < a.nN) a.out[i * a.nN + j] = acc[r][c][v];
                }
        return;
    }
    double dv[2];
    int code[2], jj[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int64_t j = j0 + wc * 32 + c * 16 + fr;
        jj[c] = (int)j;
        dv[c] = 0.0;
        code[c] = 3;
        if (j < a.nN) {
            const int64_t var = a.N_index[j];
            dv[c] = a.d[var];
            code[c] = a.kind[var] == ELLP_BOUND_FIXED ? 3 : (int)a.Nb[j];
        }
    }
    double *s_v = &sA[0][0][0];                            // [side][wc][row of the tile]: free, the last stage's readers are
    int *s_p = reinterpret_cast<int *>(&sB[0][0][0]);      // past the loop's final barrier
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            RngRec up{INFINITY, RNG_NOPOS}, dn{-INFINITY, RNG_NOPOS};
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                double qu, qd;
                rng_cost_cand(acc[r][c][v], dv[c], code[c], a.eps, qu, qd);
                up = rng_pick<1>(up, RngRec{qu, qu == INFINITY ? RNG_NOPOS : jj[c]});
                dn = rng_pick<0>(dn, RngRec{qd, qd == -INFINITY ? RNG_NOPOS : jj[c]});
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {  // the 16 lanes with this fk hold the 16 columns of the row
                up = rng_pick<1>(up, RngRec{__shfl_xor(up.v, o), __shfl_xor(up.p, o)});
                dn = rng_pick<0>(dn, RngRec{__shfl_xor(dn.v, o), __shfl_xor(dn.p, o)});
            }
            if (fr == 0) {
                const int row = wr * 64 + r * 16 + fk + 4 * v;
                s_v[(0 * 4 + wc) * BM + row] = up.v;
                s_p[(0 * 4 + wc) * BM + row] = up.p;
                s_v[(1 * 4 + wc) * BM + row] = dn.v;
                s_p[(1 * 4 + wc) * BM + row] = dn.p;
            }
        }
    __syncthreads();
    if (tid < BM && i0 + tid < a.nrows) {
        RngRec up{s_v[tid], s_p[tid]}, dn{s_v[4 * BM + tid], s_p[4 * BM + tid]};
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            up = rng_pick<1>(up, RngRec{s_v[w * BM + tid], s_p[w * BM + tid]});
            dn = rng_pick<0>(dn, RngRec{s_v[(4 + w) * BM + tid], s_p[(4 + w) * BM + tid]});
        }
        const int64_t o = bx * a.nrows + i0 + tid;
        a.pu[o] = up.v;
        a.ppu[o] = up.p;
        a.pd[o] = dn.v;
        a.ppd[o] = dn.p;
    }
}
template <int STORE>
__global__ __launch_bounds__(512) void k_range_tab(RngTabArgs a) {
    range_tab_tile<STORE>(a, blockIdx.x, blockIdx.y);
}

// the blocking variable of a limit: -1 when it is infinite
__device__ __forceinline__ int64_t rng_blocking(RngRec r, const int64_t *index) {
    if (r.p == RNG_NOPOS || r.v == INFINITY || r.v == -INFINITY) return -1;
    return index[r.p];
}

// the records of a basic row folded over the column blocks, written by variable (cost: [down | up], n_c each)
struct RngCfoldArgs {
    const double *pu, *pd;
    const int32_t *ppu, *ppd;
    const int64_t *B_index, *N_index;
    double *cost;
    int64_t *cblk;
    int64_t m, n_c, nblk;
};
__device__ __forceinline__ void range_cfold_row(const RngCfoldArgs &a, int64_t i) {
    RngRec up{INFINITY, RNG_NOPOS}, dn{-INFINITY, RNG_NOPOS};
    for (int64_t k = 0; k < a.nblk; ++k) {
        up = rng_pick<1>(up, RngRec{a.pu[k * a.m + i], a.ppu[k * a.m + i]});
        dn = rng_pick<0>(dn, RngRec{a.pd[k * a.m + i], a.ppd[k * a.m + i]});
    }
    const int64_t var = a.B_index[i];
    a.cost[var] = dn.v;
    a.cost[a.n_c + var] = up.v;
    a.cblk[var] = rng_blocking(dn, a.N_index);
    a.cblk[a.n_c + var] = rng_blocking(up, a.N_index);
}
__global__ __launch_bounds__(256) void k_range_cfold(RngCfoldArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < a.m) range_cfold_row(a, i);
}

// the nonbasic variables (by position) and the costs without a column
struct RngCnbArgs {
    const double *d;
    const int64_t *N_index;
    const uint8_t *Nb, *kind;
    double *cost;
    int64_t *cblk;
    int64_t nN, n, n_c;
};
__device__ __forceinline__ void range_cnb_one(const RngCnbArgs &a, int64_t t) {
    int64_t var;
    double up = INFINITY, dn = -INFINITY;
    if (t < a.nN) {
        var = a.N_index[t];
        const double dv = a.d[var];
        if (a.kind[var] != ELLP_BOUND_FIXED) {
            if (a.Nb[t] == ELLP_NB_LOWER) dn = 0.0 - rng_pos(dv);
            else if (a.Nb[t] == ELLP_NB_UPPER) up = 0.0 - rng_neg(dv);
            else {
                up = rng_pos(-dv);
                dn = rng_neg(-dv);
            }
            if (dv != dv) up = dn = dv;
        }
    } else {
        var = a.n + (t - a.nN);
    }
    a.cost[var] = dn;
    a.cost[a.n_c + var] = up;
    a.cblk[var] = (dn == -INFINITY) ? -1 : var;
    a.cblk[a.n_c + var] = (up == INFINITY) ? -1 : var;
}
__global__ __launch_bounds__(256) void k_range_cnb(RngCnbArgs a) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < a.nN + (a.n_c - a.n)) range_cnb_one(a, t);
}

// ---- the right-hand sides: 64 columns of W per workgroup, wave w takes the rows w, w + 4, ..
struct RngRhsArgs {
    const double *W, *x, *lb, *ub;
    const uint8_t *kind;
    const int64_t *B_index;
    double *rhs;     // [down | up], m each
    int64_t *rblk;
    int64_t m, ldw;
    double eps;
};
__global__ __launch_bounds__(256) void k_range_rhs(RngRhsArgs a) {
    __shared__ double s_v[2][4][64];
    __shared__ int s_p[2][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t k = (int64_t)blockIdx.x * 64 + lane;
    RngRec up{INFINITY, RNG_NOPOS}, dn{-INFINITY, RNG_NOPOS};
    if (k < a.m)
        for (int64_t i = wave; i < a.m; i += 4) {
            const int64_t var = a.B_index[i];
            double qu, qd;
            rng_rhs_cand(a.W[i * a.ldw + k], a.x[var], a.lb[var], a.ub[var], a.kind[var], a.eps, qu, qd);
            up = rng_pick<1>(up, RngRec{qu, qu == INFINITY ? RNG_NOPOS : (int)i});
            dn = rng_pick<0>(dn, RngRec{qd, qd == -INFINITY ? RNG_NOPOS : (int)i});
        }
    s_v[0][wave][lane] = up.v;
    s_p[0][wave][lane] = up.p;
    s_v[1][wave][lane] = dn.v;
    s_p[1][wave][lane] = dn.p;
    __syncthreads();
    if (wave == 0 && k < a.m) {
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            up = rng_pick<1>(up, RngRec{s_v[0][w][lane], s_p[0][w][lane]});
            dn = rng_pick<0>(dn, RngRec{s_v[1][w][lane], s_p[1][w][lane]});
        }
        a.rhs[k] = dn.v;
        a.rhs[a.m + k] = up.v;
        a.rblk[k] = rng_blocking(dn, a.B_index);
        a.rblk[a.m + k] = rng_blocking(up, a.B_index);
    }
}

// dst[p][0 .. m) = W[positions[p]][0 .. m)
__global__ __launch_bounds__(256) void k_range_gather(const double *W, const int64_t *positions, double *dst, int64_t m, int64_t ldw) {
    const double *src = W + positions[blockIdx.x] * ldw;
    for (int64_t k = threadIdx.x; k < m; k += 256) dst[(int64_t)blockIdx.x * m + k] = src[k];
}

int64_t range_blocks(int64_t nN) { return (nN + 127) / 128; }
int range_rhs_per_block(int64_t m) {  // the vectors of a workgroup take 16 m R bytes of LDS, at most 128 KB
    int R = 16;
    while (R > 1 && 16 * m * R > (128 << 10)) R >>= 1;
    return R;
}

hipError_t range_workspace(ellp_engine *e) {
    if (e->rng_ready) return hipSuccess;
    const int64_t m = e->m, ld = e->ld, nN = e->nN, n_c = e->n_c;
    const int64_t nblk = range_blocks(nN) > 0 ? range_blocks(nN) : 1, t64 = (m + 63) / 64;
    hipError_t rc;
    if ((rc = post_alloc(e, &e->rng_W, (size_t)(m * ld))) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->rng_pu, (size_t)(nblk * m))) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->rng_pd, (size_t)(nblk * m))) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->rng_ppu, (size_t)(nblk * m))) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->rng_ppd, (size_t)(nblk * m))) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->rng_cost, (size_t)(2 * n_c))) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->rng_cblk, (size_t)(2 * n_c))) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->rng_rhs, (size_t)(2 * m))) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->rng_rblk, (size_t)(2 * m))) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->rng_res, (size_t)(t64 * t64 + 1))) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->rng_fail, (size_t)4)) != hipSuccess) return rc;
    e->rng_ready = true;
    return hipSuccess;
}

template <int R>
hipError_t range_launch_solve(ellp_engine *e) {
    const int64_t m = e->m;
    const size_t lds = (size_t)16 * (size_t)m * R;
    if (lds > 65536) {
        const hipError_t rc = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_range_solve<R>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (rc != hipSuccess) return rc;
    }
    hipLaunchKernelGGL(k_range_solve<R>, dim3((unsigned)((m + R - 1) / R)), dim3(512), lds, e->stream, e->post_luw.M, e->post_luw.piv, m, e->rng_W,
                       e->ld, e->rng_fail);
    return hipSuccess;
}

// ELLP_RANGE_PROFILE=1 (measurements, tools/ranging_time.py): the stages bracketed with HIP events, one line on stderr per call
struct RangeProf {
    enum { SOLVE = 0, RESID = 1, TAB = 2, RHS = 3, NCAT = 4 };
    bool on;
    hipStream_t stream;
    hipEvent_t ev[NCAT][2];
    bool have[NCAT];
    RangeProf(hipStream_t s) : on(getenv("ELLP_RANGE_PROFILE") && getenv("ELLP_RANGE_PROFILE")[0] == '1'), stream(s) {
        for (int c = 0; c < NCAT; ++c) have[c] = false;
    }
    void begin(int c) {
        if (!on) return;
        if (hipEventCreate(&ev[c][0]) != hipSuccess) return;
        if (hipEventCreate(&ev[c][1]) != hipSuccess) {
            (void)hipEventDestroy(ev[c][0]);
            return;
        }
        have[c] = true;
        (void)hipEventRecord(ev[c][0], stream);
    }
    void end(int c) {
        if (on && have[c]) (void)hipEventRecord(ev[c][1], stream);
    }
    void report(int64_t m, int64_t nN) {  // after the stream has drained
        if (!on) return;
        float ms[NCAT] = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < NCAT; ++c)
            if (have[c]) (void)hipEventElapsedTime(&ms[c], ev[c][0], ev[c][1]);
        fprintf(stderr, "ranging_profile m=%lld nN=%lld solve_ms=%.4f resid_ms=%.4f tableau_ms=%.4f rhs_ms=%.4f\n", (long long)m, (long long)nN,
                ms[SOLVE], ms[RESID], ms[TAB], ms[RHS]);
    }
    ~RangeProf() {
        for (int c = 0; c < NCAT; ++c)
            if (have[c]) {
                (void)hipEventDestroy(ev[c][0]);
                (void)hipEventDestroy(ev[c][1]);
            }
    }
};

// the postsolve, then W; on return the stream has drained and post_luw, post_d, rng_W describe the completed point
ellp_status range_inverse(ellp_engine *e, ellp_kkt *kkt, RangeProf &prof, char *errbuf, size_t errlen) {
    const ellp_status s = post_compute(e, nullptr, nullptr, nullptr, kkt, errbuf, errlen);
    if (s != ELLP_OPTIMAL) return s;
    HIPCHK(range_workspace(e));
    HIPCHK(hipMemsetAsync(e->rng_fail, 0, sizeof(int), e->stream));
    prof.begin(RangeProf::SOLVE);
    switch (range_rhs_per_block(e->m)) {
    case 16: HIPCHK(range_launch_solve<16>(e)); break;
    case 8: HIPCHK(range_launch_solve<8>(e)); break;
    case 4: HIPCHK(range_launch_solve<4>(e)); break;
    case 2: HIPCHK(range_launch_solve<2>(e)); break;
    default: HIPCHK(range_launch_solve<1>(e)); break;
    }
    hipLaunchKernelGGL(k_range_snap, dim3((unsigned)e->m), dim3(256), 0, e->stream, e->rng_W, e->post_srow, e->post_sval, e->m, e->ld);
    prof.end(RangeProf::SOLVE);
    int fail = 0;
    HIPCHK(hipMemcpyAsync(&fail, e->rng_fail, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipGetLastError());
    if (fail) {  // post_compute's own solve has met the same diagonal: not reached
        set_err(errbuf, errlen, "invalid B, A_B is not invertible");
        return ELLP_ERR_SINGULAR;
    }
    return ELLP_OPTIMAL;
}

void range_launch_tab(ellp_engine *e, const int64_t *rowmap, int64_t nrows, double *out) {
    if (e->nN <= 0 || nrows <= 0) return;
    RngTabArgs a{};
    a.W = e->rng_W; a.rowmap = rowmap; a.A_N = e->A_N; a.d = e->post_d; a.N_index = e->N_index; a.Nb = e->Nb; a.kind = e->kindv;
    a.pu = e->rng_pu; a.pd = e->rng_pd; a.ppu = e->rng_ppu; a.ppd = e->rng_ppd; a.out = out;
    a.m = e->m; a.ld = e->ld; a.ldw = e->ld; a.nrows = nrows; a.nN = e->nN; a.eps = e->eps;
    const dim3 grid((unsigned)range_blocks(e->nN), (unsigned)((nrows + 127) / 128));
    if (out) hipLaunchKernelGGL(k_range_tab<1>, grid, dim3(512), 0, e->stream, a);
    else hipLaunchKernelGGL(k_range_tab<0>, grid, dim3(512), 0, e->stream, a);
}

bool range_wants(const ellp_ranging_out *o) {
    return o && (o->cost_down || o->cost_up || o->cost_blocking_down || o->cost_blocking_up || o->rhs_down || o->rhs_up ||
                 o->rhs_blocking_down || o->rhs_blocking_up || o->d || o->y || o->info);
}

// everything after the refusals, on a complete state; the outputs are written only when everything succeeded
ellp_status range_compute(ellp_engine *e, const ellp_ranging_out *out, char *errbuf, size_t errlen) {
    const int64_t m = e->m, nN = e->nN, n = e->n, n_c = e->n_c, ld = e->ld;
    RangeProf prof(e->stream);
    ellp_ranging_info info{};
    const ellp_status s = range_inverse(e, &info.kkt, prof, errbuf, errlen);
    if (s != ELLP_OPTIMAL) return s;
    const unsigned t64 = (unsigned)((m + 63) / 64);
    prof.begin(RangeProf::RESID);
    hipLaunchKernelGGL(k_range_resid, dim3(t64, t64), dim3(256), 0, e->stream, e->A_B, e->rng_W, m, ld, ld, e->rng_res + 1);
    hipLaunchKernelGGL(k_range_resmax, dim3(1), dim3(256), 0, e->stream, e->rng_res + 1, (int64_t)t64 * t64, e->rng_res);
    prof.end(RangeProf::RESID);
    prof.begin(RangeProf::TAB);
    range_launch_tab(e, nullptr, m, nullptr);
    RngCfoldArgs f{};
    f.pu = e->rng_pu; f.pd = e->rng_pd; f.ppu = e->rng_ppu; f.ppd = e->rng_ppd; f.B_index = e->B_index; f.N_index = e->N_index;
    f.cost = e->rng_cost; f.cblk = e->rng_cblk; f.m = m; f.n_c = n_c; f.nblk = range_blocks(nN);
    hipLaunchKernelGGL(k_range_cfold, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, e->stream, f);
    prof.end(RangeProf::TAB);
    const int64_t rest = nN + (n_c - n);
    if (rest > 0) {
        RngCnbArgs c{};
        c.d = e->post_d; c.N_index = e->N_index; c.Nb = e->Nb; c.kind = e->kindv; c.cost = e->rng_cost; c.cblk = e->rng_cblk;
        c.nN = nN; c.n = n; c.n_c = n_c;
        hipLaunchKernelGGL(k_range_cnb, dim3((unsigned)((rest + 255) / 256)), dim3(256), 0, e->stream, c);
    }
    prof.begin(RangeProf::RHS);
    RngRhsArgs r{};
    r.W = e->rng_W; r.x = e->x; r.lb = e->lb; r.ub = e->ub; r.kind = e->kindv; r.B_index = e->B_index; r.rhs = e->rng_rhs;
    r.rblk = e->rng_rblk; r.m = m; r.ldw = ld; r.eps = e->eps;
    hipLaunchKernelGGL(k_range_rhs, dim3((unsigned)((m + 63) / 64)), dim3(256), 0, e->stream, r);
    prof.end(RangeProf::RHS);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&info.inverse_residual, e->rng_res, sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    prof.report(m, nN);
    const size_t cb = sizeof(double) * (size_t)n_c, rb = sizeof(double) * (size_t)m;
    if (out->cost_down) HIPCHK(hipMemcpy(out->cost_down, e->rng_cost, cb, hipMemcpyDeviceToHost));
    if (out->cost_up) HIPCHK(hipMemcpy(out->cost_up, e->rng_cost + n_c, cb, hipMemcpyDeviceToHost));
    if (out->cost_blocking_down) HIPCHK(hipMemcpy(out->cost_blocking_down, e->rng_cblk, cb, hipMemcpyDeviceToHost));
    if (out->cost_blocking_up) HIPCHK(hipMemcpy(out->cost_blocking_up, e->rng_cblk + n_c, cb, hipMemcpyDeviceToHost));
    if (out->rhs_down) HIPCHK(hipMemcpy(out->rhs_down, e->rng_rhs, rb, hipMemcpyDeviceToHost));
    if (out->rhs_up) HIPCHK(hipMemcpy(out->rhs_up, e->rng_rhs + m, rb, hipMemcpyDeviceToHost));
    if (out->rhs_blocking_down) HIPCHK(hipMemcpy(out->rhs_blocking_down, e->rng_rblk, rb, hipMemcpyDeviceToHost));
    if (out->rhs_blocking_up) HIPCHK(hipMemcpy(out->rhs_blocking_up, e->rng_rblk + m, rb, hipMemcpyDeviceToHost));
    if (out->d) HIPCHK(hipMemcpy(out->d, e->post_d, cb, hipMemcpyDeviceToHost));
    if (out->y) HIPCHK(hipMemcpy(out->y, e->post_y, rb, hipMemcpyDeviceToHost));
    if (out->info) *out->info = info;
    return ELLP_OPTIMAL;
}

// the refusals of the engine forms, answered before any HIP call
bool range_refused(ellp_engine *e, const char *who, char *errbuf, size_t errlen) {
    if (!e) {
        set_err(errbuf, errlen, "%s: no engine", who);
        return true;
    }
    if (e->world > 1 || e->colshard) {
        set_err(errbuf, errlen, "%s: not on a sharded engine (every rank holds a part of the columns or of the pricing)", who);
        return true;
    }
    if (e->h_st && e->h_st->status < 0) {
        set_err(errbuf, errlen, "%s: the engine ended with an error (status %d): there is no point to examine", who, (int)e->h_st->status);
        return true;
    }
    return false;
}

}  // namespace

extern "C" {

ellp_status ellp_engine_ranging(ellp_engine *e, const ellp_ranging_out *out, char *errbuf, size_t errlen) {
    if (errbuf && errlen) errbuf[0] = 0;
    if (range_refused(e, "ranging", errbuf, errlen)) return ELLP_ERR_ARG;
    if (!range_wants(out)) {
        set_err(errbuf, errlen, "ranging: nothing is wanted (out is NULL or holds no array)");
        return ELLP_ERR_ARG;
    }
    ellp_status closing = ELLP_OPTIMAL;
    const ellp_status cs = post_complete_open(e, &closing, errbuf, errlen);
    if (cs != ELLP_OPTIMAL) return cs;
    char err2[256];
    const ellp_status s = range_compute(e, out, closing == ELLP_OPTIMAL ? errbuf : err2, closing == ELLP_OPTIMAL ? errlen : sizeof(err2));
    if (s != ELLP_OPTIMAL) {
        if (closing != ELLP_OPTIMAL) set_err(errbuf, errlen, "%s", err2);
        return s;
    }
    return closing;
}

ellp_status ellp_ranging(int64_t m, int64_t n, int64_t n_c, const double *A, const double *c, const double *b, const uint8_t *bound_kind,
                         const double *lb, const double *ub, const double *x, const int64_t *B_index, int64_t n_B, const int64_t *N_index,
                         const uint8_t *N_bound, int64_t n_N, const ellp_opts *opts_in, const ellp_ranging_out *out, char *errbuf,
                         size_t errlen) {
    if (errbuf && errlen) errbuf[0] = 0;
    if (!range_wants(out)) {
        set_err(errbuf, errlen, "ranging: nothing is wanted (out is NULL or holds no array)");
        return ELLP_ERR_ARG;
    }
    PostOwn own(nullptr, ellp_engine_destroy);
    const ellp_status s = post_host_engine("ranging", m, n, n_c, A, c, b, bound_kind, lb, ub, x, B_index, n_B, N_index, N_bound, n_N, opts_in, own,
                                           errbuf, errlen);
    if (s != ELLP_OPTIMAL) return s;
    return range_compute(own.get(), out, errbuf, errlen);
}

ellp_status ellp_engine_tableau_rows(ellp_engine *e, const int64_t *positions, int64_t k, double *alpha, double *rho, char *errbuf,
                                     size_t errlen) {
    if (errbuf && errlen) errbuf[0] = 0;
    if (range_refused(e, "tableau_rows", errbuf, errlen)) return ELLP_ERR_ARG;
    if (!positions || !alpha || k < 1) {
        set_err(errbuf, errlen, "tableau_rows: positions or alpha is NULL, or k < 1");
        return ELLP_ERR_ARG;
    }
    for (int64_t p = 0; p < k; ++p)
        if (positions[p] < 0 || positions[p] >= e->m) {
            set_err(errbuf, errlen, "tableau_rows: positions[%lld] = %lld is outside [0, %lld)", (long long)p, (long long)positions[p], (long long)e->m);
            return ELLP_ERR_ARG;
        }
    ellp_status closing = ELLP_OPTIMAL;
    const ellp_status cs = post_complete_open(e, &closing, errbuf, errlen);
    if (cs != ELLP_OPTIMAL) return cs;
    char err2[256];
    char *eb = closing == ELLP_OPTIMAL ? errbuf : err2;
    const size_t el = closing == ELLP_OPTIMAL ? errlen : sizeof(err2);
    RangeProf prof(e->stream);
    ellp_status s = range_inverse(e, nullptr, prof, eb, el);
    if (s == ELLP_OPTIMAL) {
        // the call's own buffers: the positions, k rows of the tableau, k rows of W
        const int64_t m = e->m, nN = e->nN;
        DevTemp<int64_t> pos(e->stream);
        DevTemp<double> al(e->stream), rh(e->stream);
        auto body = [&](char *errbuf, size_t errlen) -> ellp_status {
            HIPCHK(pos.alloc((size_t)k));
            HIPCHK(al.alloc((size_t)(k * (nN > 0 ? nN : 1))));
            if (rho) HIPCHK(rh.alloc((size_t)(k * m)));
            HIPCHK(hipMemcpyAsync(pos.p, positions, sizeof(int64_t) * (size_t)k, hipMemcpyHostToDevice, e->stream));
            range_launch_tab(e, pos.p, k, al.p);
            if (rho) hipLaunchKernelGGL(k_range_gather, dim3((unsigned)k), dim3(256), 0, e->stream, e->rng_W, pos.p, rh.p, m, e->ld);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(e->stream));
            if (nN > 0) HIPCHK(hipMemcpy(alpha, al.p, sizeof(double) * (size_t)(k * nN), hipMemcpyDeviceToHost));
            if (rho) HIPCHK(hipMemcpy(rho, rh.p, sizeof(double) * (size_t)(k * m), hipMemcpyDeviceToHost));
            return ELLP_OPTIMAL;
        };
        s = body(eb, el);
    }
    if (s != ELLP_OPTIMAL) {
        if (closing != ELLP_OPTIMAL) set_err(errbuf, errlen, "%s", err2);
        return s;
    }
    return closing;
}

}  // extern "C"

// ellp_cert.inc — certificates: a Farkas vector or a ray for the basis and point an engine stands on
// (ellp_engine_certificate), or for a point in host memory (ellp_certificate), each with a report of how good a proof it is.
// DESIGN.md §3.12; the definitions are in include/ellp_hip.h.
//
// A pure function of (the arrays, the basis, the labels): every source starts from the postsolve's fresh LU (post_solve_y);
// nothing is read from a loop's carried u, rho, alpha, s_q or s_r.
//   FARKAS_COSTS   the postsolve's refined y, unchanged;
//   FARKAS_ROW     x_B as ellp_basis_start(KEEP_LABELS) makes it (into cert_x: the engine's x is not written); W = B^-1
//                  (range_inverse); k_cert_tab<2>: the ranging's tableau pass with the Farkas epilogue — per accumulator
//                  element "this column passes dual_keep" for either side of the row, ORed over the 16 lanes of a row, the
//                  wave's two column tiles and the four waves (LDS), one flag byte per (column block, row); k_cert_ffold ORs
//                  the blocks, applies dual_violation to the row's variable and takes the smallest qualifying position;
//                  y = -+B^-T e_r by post_solve_y on the right-hand side -+e_r (the LU is kept);
//   RAY_COLUMN     d from the postsolve; k_cert_tab<3>: per element "row i bounds the step of column j" (primal_lambda of the
//                  signed alpha at the engine's x is not +inf), ORed over the thread's 16 rows, the lane groups (__shfl_xor
//                  16, 32) and the two wave rows (LDS), one byte per (row block, column); k_cert_rfold ORs the blocks,
//                  applies primal_key and the column's own kind, takes the smallest; r_B = -+B^-1 a_q by cert_solve_x, the
//                  warm start's solve, singleton-row snap, refinement loop and stop rule.
// A NaN alpha, x or d raises bit 4 of the same bytes: ELLP_ERR_NAN.  Boolean OR and integer minimum only: no result depends on
// a reduction order.
//   the report     z = A^T y is minus the d of k_post_pass on zero costs; A r is minus its r on a zero right-hand side with r in
//                  x's place; k_cert_farkas / k_cert_ray: one workgroup of 1,024 threads, compensated sums in the order of
//                  k_post_report's (thread k takes k, k + 1024, ..; then post_block_sum's tree), post_max maxima.
//
// Included at the end of ellp_engine.hip, after ellp_range.inc.

namespace {

struct CertVerify {
    double gap, yb, sup, dirv, residual, c_r, bdv, norm;
    long long wdir, wrow, wbv;
};

// calls: of the two entry points; launches: g_post_launches over the last call (every kernel is counted where it is launched:
// here by CERT_LAUNCH, in post_launch_pass, start_fold and start_solve_x by themselves); steps: its refinement steps
struct CertCalls {
    uint64_t calls = 0, launches = 0, steps = 0;
};
CertCalls g_cert_calls;
#define CERT_LAUNCH(...)                 \
    do {                                 \
        hipLaunchKernelGGL(__VA_ARGS__); \
        g_post_launches += 1;            \
    } while (0)

// ---- the epilogues of the tableau pass (range_tab_tile<2>, <3>).  Element v of acc[r][c] is row i0 + wr * 64 + r * 16 + fk +
// 4 v, column j0 + wc * 32 + c * 16 + fr.  scratch: 32 KB of LDS no thread reads any more.
template <int STORE>
__device__ __forceinline__ void cert_tab_epilogue(const RngTabArgs &a, const mfma_d4 (&acc)[4][2], int *scratch, int64_t bx, int64_t by) {
    constexpr int BM = 128, BN = 128;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 2, wc = wave & 3, fr = lane & 15, fk = lane >> 4;
    const int64_t i0 = by * BM, j0 = bx * BN;
    bool ok[2];
    int nb[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int64_t j = j0 + wc * 32 + c * 16 + fr;
        ok[c] = j < a.nN;
        nb[c] = ok[c] ? (int)a.Nb[j] : 0;
    }
    if (STORE == 2) {
        // bit 1: a column passes dual_keep for a row that violates its lower bound (al = -alpha); bit 2: its upper bound
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                int bits = 0;
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    if (!ok[c]) continue;
                    const double al = acc[r][c][v];
                    if (al != al) bits |= 4;
                    else {
                        if (dual_keep(-al, nb[c], a.eps)) bits |= 1;
                        if (dual_keep(al, nb[c], a.eps)) bits |= 2;
                    }
                }
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) bits |= __shfl_xor(bits, o);  // the 16 lanes with this fk hold the row's columns
                if (fr == 0) scratch[wc * BM + wr * 64 + r * 16 + fk + 4 * v] = bits;
            }
        __syncthreads();
        if (tid < BM && i0 + tid < a.nrows)
            a.cbits[bx * a.nrows + i0 + tid] = (uint8_t)(scratch[tid] | scratch[BM + tid] | scratch[2 * BM + tid] | scratch[3 * BM + tid]);
    } else {
        // bit 1: a row bounds the step of this column
        bool up[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            up[c] = false;
            if (ok[c]) up[c] = nb[c] == ELLP_NB_LOWER || (nb[c] == ELLP_NB_FREE && a.d[a.N_index[j0 + wc * 32 + c * 16 + fr]] < 0.0);
        }
        int blk[2] = {0, 0};
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int64_t i = i0 + wr * 64 + r * 16 + fk + 4 * v;
                if (i >= a.nrows) continue;
                const int64_t bi = a.cB[i];
                const double xi = a.cx[bi], lbi = a.clb[bi], ubi = a.cub[bi];
                const int k = a.kind[bi];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    if (!ok[c]) continue;
                    const double al = acc[r][c][v];
                    if (al != al || xi != xi) {
                        blk[c] |= 4;
                        continue;
                    }
                    const double li = primal_lambda(up[c] ? -al : al, xi, lbi, ubi, k, a.eps);
                    if (li != li) blk[c] |= 4;
                    else if (li != INFINITY) blk[c] |= 1;
                }
            }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            blk[c] |= __shfl_xor(blk[c], 16);  // the four lane groups fk hold the rows of a column
            blk[c] |= __shfl_xor(blk[c], 32);
            if (fk == 0) scratch[wr * BN + wc * 32 + c * 16 + fr] = blk[c];
        }
        __syncthreads();
        if (tid < BN && j0 + tid < a.nN) a.cbits[by * a.nN + j0 + tid] = (uint8_t)(scratch[tid] | scratch[BN + tid]);
    }
}
template <int STORE>
__global__ __launch_bounds__(512) void k_cert_tab(RngTabArgs a) {
    range_tab_tile<STORE>(a, blockIdx.x, blockIdx.y);
}

// the smallest qualifying position, the count and the NaN flag of one workgroup of 1,024 threads: pick[0 .. 2]
__device__ __forceinline__ long long cert_block_pick(long long first, int cnt, int nan, int64_t *pick) {
    __shared__ long long s_f[1024];
    __shared__ int s_c[1024], s_n[1024];
    const int tid = threadIdx.x;
    s_f[tid] = first;
    s_c[tid] = cnt;
    s_n[tid] = nan;
    __syncthreads();
    for (int h = 512; h >= 1; h >>= 1) {
        if (tid < h) {
            s_f[tid] = s_f[tid + h] < s_f[tid] ? s_f[tid + h] : s_f[tid];
            s_c[tid] += s_c[tid + h];
            s_n[tid] |= s_n[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        pick[0] = s_f[0] == INT64_MAX ? -1 : s_f[0];
        pick[1] = s_c[0];
        pick[2] = s_n[0];
    }
    return s_f[0];
}

struct CertFoldArgs {
    const uint8_t *bits;
    const int64_t *B_index, *N_index;
    const uint8_t *Nb, *kind;
    const double *x, *lb, *ub, *d;
    int64_t m, nN, nblk;
    double eps;
    int64_t *pick;
};
// Farkas: row i qualifies when dual_violation finds its variable outside a bound and no column kept that side
__global__ __launch_bounds__(1024) void k_cert_ffold(CertFoldArgs a) {
    long long first = INT64_MAX;
    int cnt = 0, nan = 0;
    for (int64_t i = threadIdx.x; i < a.m; i += 1024) {
        int bits = 0;
        for (int64_t k = 0; k < a.nblk; ++k) bits |= a.bits[k * a.m + i];
        const double xi = a.x[a.B_index[i]];
        if ((bits & 4) || xi != xi) nan = 1;
        double delta;
        int side;
        if (dual_violation(a.B_index, a.x, a.kind, a.lb, a.ub, a.eps, i, &delta, &side) && !(bits & (side == ELLP_NB_LOWER ? 1 : 2))) {
            if (i < first) first = i;
            cnt += 1;
        }
    }
    const long long f = cert_block_pick(first, cnt, nan, a.pick);
    if (threadIdx.x == 0) {
        double delta = 0.0;
        int side = 0;
        if (f != INT64_MAX) dual_violation(a.B_index, a.x, a.kind, a.lb, a.ub, a.eps, f, &delta, &side);
        a.pick[3] = side;
    }
}
// ray: position j qualifies when it is an entering candidate, its own kind leaves the step unbounded and no row bounds it
__global__ __launch_bounds__(1024) void k_cert_rfold(CertFoldArgs a) {
    long long first = INT64_MAX;
    int cnt = 0, nan = 0;
    for (int64_t j = threadIdx.x; j < a.nN; j += 1024) {
        int bits = 0;
        for (int64_t k = 0; k < a.nblk; ++k) bits |= a.bits[k * a.nN + j];
        const int64_t var = a.N_index[j];
        const double dv = a.d[var];
        if ((bits & 4) || dv != dv) nan = 1;
        const int kd = a.kind[var];
        const bool open = kd == ELLP_BOUND_FREE || kd == ELLP_BOUND_LOWER || kd == ELLP_BOUND_UPPER;
        if (primal_key(dv, a.Nb[j], a.eps) > -INFINITY && open && !(bits & 1)) {
            if (j < first) first = j;
            cnt += 1;
        }
    }
    const long long f = cert_block_pick(first, cnt, nan, a.pick);
    if (threadIdx.x == 0) {
        int up = 0;
        if (f != INT64_MAX) up = a.Nb[f] == ELLP_NB_LOWER || (a.Nb[f] == ELLP_NB_FREE && a.d[a.N_index[f]] < 0.0);
        a.pick[3] = up;
    }
}

// x_N by label and kind as k_start_labels sets it (the labels are kept and not written); the basic positions at +0.0
__global__ __launch_bounds__(256) void k_cert_xn(const int64_t *B_index, const int64_t *N_index, const uint8_t *Nb, const uint8_t *kind,
                                                 const double *lb, const double *ub, double *x, int64_t m, int64_t nN) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < nN) {
        const int64_t v = N_index[j];
        int label;
        double val;
        start_label(kind, lb, ub, nullptr, 0, v, Nb[j], label, val);
        x[v] = val;
    }
    if (j < m) x[B_index[j]] = 0.0;
}
// rhs = sign e_r, the sign from the side the row violates (pick[3]): Lower -1, Upper +1
__global__ __launch_bounds__(256) void k_cert_unit(double *rhs, int64_t m, const int64_t *pick) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) rhs[i] = (i == pick[0]) ? (pick[3] == ELLP_NB_LOWER ? -1.0 : 1.0) : 0.0;
}
// t = column pick[0] of A_N
__global__ __launch_bounds__(256) void k_cert_col(const double *A_N, int64_t ld, double *t, int64_t m, const int64_t *pick) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) t[i] = A_N[pick[0] * ld + i];
}
// the ray by variable on the columns below n_check (vec is zero before): r_q = +-1, r_B = -+xb
__global__ __launch_bounds__(256) void k_cert_rvec(double *vec, const double *xb, const int64_t *B_index, const int64_t *N_index, int64_t m,
                                                   int64_t n_check, const int64_t *pick) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool up = pick[3] != 0;
    if (i < m && B_index[i] < n_check) vec[B_index[i]] = up ? -xb[i] : xb[i];
    if (i == 0 && N_index[pick[0]] < n_check) vec[N_index[pick[0]]] = up ? 1.0 : -1.0;
}

struct CertVerArgs {
    const double *vec, *b, *d, *res, *c_B, *c_N, *lb, *ub;
    const uint8_t *kind;
    const int64_t *B_index, *N_index;
    int64_t m, nN, n_check;
    CertVerify *out;
};
__device__ __forceinline__ bool cert_has_ub(int k) { return k == ELLP_BOUND_UPPER || k == ELLP_BOUND_TWOSIDED || k == ELLP_BOUND_FIXED; }
__device__ __forceinline__ bool cert_has_lb(int k) { return k == ELLP_BOUND_LOWER || k == ELLP_BOUND_TWOSIDED || k == ELLP_BOUND_FIXED; }
// the report of a Farkas vector y (vec): z_v = -d_v of the pass on zero costs
__global__ __launch_bounds__(1024) void k_cert_farkas(CertVerArgs a) {
    __shared__ PostMax sh[1024];
    __shared__ double shs[1024], shc[1024];
    const int tid = threadIdx.x;
    PostMax dirv{0.0, LLONG_MAX_POST}, nrm{0.0, LLONG_MAX_POST};
    double gs = 0.0, gc = 0.0, ys = 0.0, yc = 0.0, ss = 0.0, sc = 0.0;
    for (int64_t k = tid; k < a.m + a.n_check; k += 1024) {
        if (k < a.m) {
            post_dot2(gs, gc, a.vec[k], a.b[k]);
            post_dot2(ys, yc, a.vec[k], a.b[k]);
            nrm = post_max(nrm, PostMax{fabs(a.vec[k]), (long long)k});
        } else {
            const int64_t v = k - a.m;
            const double z = -a.d[v];
            const int kd = a.kind[v];
            if (z != z) dirv = post_max(dirv, PostMax{z, (long long)v});
            else if (z > 0.0) {
                if (cert_has_ub(kd)) {
                    const double ubv = kd == ELLP_BOUND_FIXED ? a.lb[v] : a.ub[v];  // Fixed: x = lb, as k_post_report reads it
                    post_dot2(gs, gc, -z, ubv);
                    post_dot2(ss, sc, z, ubv);
                } else dirv = post_max(dirv, PostMax{z, (long long)v});
            } else if (z < 0.0) {
                if (cert_has_lb(kd)) {
                    post_dot2(gs, gc, -z, a.lb[v]);
                    post_dot2(ss, sc, z, a.lb[v]);
                } else dirv = post_max(dirv, PostMax{-z, (long long)v});
            }
        }
    }
    const PostMax dm = post_block_max(dirv, sh);
    const PostMax nm = post_block_max(nrm, sh);
    const double gap = post_block_sum(gs, gc, shs, shc);
    const double yb = post_block_sum(ys, yc, shs, shc);
    const double sup = post_block_sum(ss, sc, shs, shc);
    if (tid == 0) {
        CertVerify o{};
        o.gap = gap;
        o.yb = yb;
        o.sup = sup;
        o.dirv = dm.v;
        o.wdir = (dm.v == 0.0) ? -1 : dm.i;
        o.norm = nm.v;
        o.wrow = o.wbv = -1;
        *a.out = o;
    }
}
// the report of a ray r (vec, by variable, zero from n_check on): res = -(A r) from the pass on a zero right-hand side
__global__ __launch_bounds__(1024) void k_cert_ray(CertVerArgs a) {
    __shared__ PostMax sh[1024];
    __shared__ double shs[1024], shc[1024];
    const int tid = threadIdx.x;
    PostMax rm{0.0, LLONG_MAX_POST}, bd{0.0, LLONG_MAX_POST}, nrm{0.0, LLONG_MAX_POST};
    for (int64_t i = tid; i < a.m; i += 1024) rm = post_max(rm, PostMax{fabs(a.res[i]), (long long)i});
    for (int64_t v = tid; v < a.n_check; v += 1024) {
        const double rv = a.vec[v];
        const int kd = a.kind[v];
        nrm = post_max(nrm, PostMax{fabs(rv), (long long)v});
        if (rv != rv || (rv > 0.0 && cert_has_ub(kd)) || (rv < 0.0 && cert_has_lb(kd))) bd = post_max(bd, PostMax{fabs(rv), (long long)v});
    }
    double s = 0.0, c = 0.0;
    for (int64_t k = tid; k < a.m + a.nN; k += 1024) {
        if (k < a.m) post_dot2(s, c, a.c_B[k], a.vec[a.B_index[k]]);
        else post_dot2(s, c, a.c_N[k - a.m], a.vec[a.N_index[k - a.m]]);
    }
    const PostMax rmx = post_block_max(rm, sh);
    const PostMax bdx = post_block_max(bd, sh);
    const PostMax nm = post_block_max(nrm, sh);
    const double cr = post_block_sum(s, c, shs, shc);
    if (tid == 0) {
        CertVerify o{};
        o.residual = rmx.v;
        o.wrow = (rmx.v == 0.0) ? -1 : rmx.i;
        o.bdv = bdx.v;
        o.wbv = (bdx.v == 0.0) ? -1 : bdx.i;
        o.c_r = cr;
        o.norm = nm.v;
        o.wdir = -1;
        *a.out = o;
    }
}

int64_t cert_bits_count(int64_t m, int64_t nN) {
    const int64_t f = range_blocks(nN) * m, r = ((m + 127) / 128) * nN;
    return (f > r ? f : r) > 0 ? (f > r ? f : r) : 1;
}

hipError_t cert_workspace(ellp_engine *e) {
    if (e->cert_ready) return hipSuccess;
    const int64_t m = e->m, ld = e->ld, nN = e->nN, n_c = e->n_c, n = e->n;
    const int64_t nchunks = (m + START_XC - 1) / START_XC, wide = (ld > nN ? ld : nN) > n_c ? (ld > nN ? ld : nN) : n_c;
    hipError_t rc;
    if ((rc = post_alloc(e, &e->cert_x, (size_t)n_c)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->cert_xb, (size_t)ld)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->cert_t, (size_t)ld)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->cert_res, (size_t)ld)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->cert_dx, (size_t)ld)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->cert_xpart, (size_t)(nchunks * m))) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->cert_omega, (size_t)1)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->cert_rspos, (size_t)m)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->cert_rsval, (size_t)m)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->cert_vec, (size_t)wide)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->cert_rhs, (size_t)ld)) != hipSuccess) return rc;
    if (!e->cert_zero) {
        if ((rc = post_alloc(e, &e->cert_zero, (size_t)wide)) != hipSuccess) return rc;
        if ((rc = hipMemsetAsync(e->cert_zero, 0, sizeof(double) * (size_t)wide, e->stream)) != hipSuccess) return rc;
    }
    if ((rc = post_alloc(e, &e->cert_bits, (size_t)cert_bits_count(m, nN))) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->cert_ckind, (size_t)n)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->cert_clb, (size_t)n)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->cert_cub, (size_t)n)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->cert_pick, (size_t)4)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->cert_ver, (size_t)((sizeof(CertVerify) + 7) / 8))) != hipSuccess) return rc;
    e->cert_ready = true;
    return hipSuccess;
}

// cert_xb = B^-1 cert_t with the LU in post_luw, and cert_x at B_index: step 5 of ellp_basis_start itself (start_solve_x) on
// the certificate's own point
ellp_status cert_solve_x(ellp_engine *e, PostProf &prof, int32_t *steps_out, char *errbuf, size_t errlen) {
    const PostOver ov{e->c_B, e->c_N, e->post_y, e->cert_x, false};
    const StartXWork w{e->cert_t, e->cert_xb, e->cert_res, e->cert_dx, e->cert_xpart, e->cert_omega, e->cert_x, e->cert_rspos, e->cert_rsval};
    double omega = 0.0;
    return start_solve_x(e, w, &ov, prof, &omega, steps_out, errbuf, errlen);
}

void cert_launch_tab(ellp_engine *e, int source, const double *x) {
    const int64_t m = e->m, nN = e->nN;
    if (nN <= 0) return;
    RngTabArgs a{};
    a.W = e->rng_W; a.A_N = e->A_N; a.d = e->post_d; a.N_index = e->N_index; a.Nb = e->Nb; a.kind = e->kindv;
    a.m = m; a.ld = e->ld; a.ldw = e->ld; a.nrows = m; a.nN = nN; a.eps = e->eps;
    a.cx = x; a.clb = e->lb; a.cub = e->ub; a.cB = e->B_index; a.cbits = e->cert_bits;
    const dim3 grid((unsigned)range_blocks(nN), (unsigned)((m + 127) / 128));
    if (source == ELLP_CERT_FARKAS_ROW) CERT_LAUNCH(k_cert_tab<2>, grid, dim3(512), 0, e->stream, a);
    else CERT_LAUNCH(k_cert_tab<3>, grid, dim3(512), 0, e->stream, a);
}

// ELLP_CERT_PROFILE=1 (measurements, tools/certificate_time.py): device time of the stages, one line on stderr per call
struct CertProf {
    enum { BASE = 0, POINT = 1, TAB = 2, VECTOR = 3, VERIFY = 4, NCAT = 5 };
    bool on;
    hipStream_t stream;
    hipEvent_t ev[NCAT][2];
    bool have[NCAT];
    CertProf(hipStream_t s) : on(getenv("ELLP_CERT_PROFILE") && getenv("ELLP_CERT_PROFILE")[0] == '1'), stream(s) {
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
    void report(int source, int64_t m, int64_t nN) {  // after the stream has drained
        if (!on) return;
        float ms[NCAT] = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < NCAT; ++c)
            if (have[c]) (void)hipEventElapsedTime(&ms[c], ev[c][0], ev[c][1]);
        fprintf(stderr, "certificate_profile source=%d m=%lld nN=%lld base_ms=%.4f point_ms=%.4f tableau_ms=%.4f vector_ms=%.4f verify_ms=%.4f\n",
                source, (long long)m, (long long)nN, ms[BASE], ms[POINT], ms[TAB], ms[VECTOR], ms[VERIFY]);
    }
    ~CertProf() {
        for (int c = 0; c < NCAT; ++c)
            if (have[c]) {
                (void)hipEventDestroy(ev[c][0]);
                (void)hipEventDestroy(ev[c][1]);
            }
    }
};

// everything after the refusals, on a complete state; vec and info are written only when everything succeeded
ellp_status cert_compute(ellp_engine *e, int source, int64_t n_check, const uint8_t *chk_kind, const double *chk_lb, const double *chk_ub,
                         double *vec, ellp_cert_info *info, char *errbuf, size_t errlen) {
    const int64_t m = e->m, nN = e->nN, n_c = e->n_c, ld = e->ld;
    const unsigned mb = (unsigned)((m + 255) / 256);
    const int64_t bB = post_blocks(m), bN = post_blocks(nN);
    const uint64_t launches0 = g_post_launches;
    g_cert_calls.launches = 0;
    g_cert_calls.steps = 0;
    HIPCHK(post_workspace(e));
    if (source != ELLP_CERT_FARKAS_COSTS) HIPCHK(range_workspace(e));
    HIPCHK(cert_workspace(e));
    const uint8_t *vkind = e->kindv;
    const double *vlb = e->lb, *vub = e->ub;
    if (chk_kind) {
        HIPCHK(hipMemcpyAsync(e->cert_ckind, chk_kind, (size_t)n_check, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->cert_clb, chk_lb, sizeof(double) * (size_t)n_check, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->cert_cub, chk_ub, sizeof(double) * (size_t)n_check, hipMemcpyHostToDevice, e->stream));
        vkind = e->cert_ckind;
        vlb = e->cert_clb;
        vub = e->cert_cub;
    }
    CertProf prof(e->stream);
    PostProf pprof(e->stream);
    RangeProf rprof(e->stream);
    const bool farkas = source != ELLP_CERT_RAY_COLUMN;
    int32_t steps = 0;
    int64_t pick[4] = {-1, 0, 0, 0};
    bool found = false;
    prof.begin(CertProf::BASE);
    if (source == ELLP_CERT_FARKAS_COSTS) {
        const ellp_status s = post_solve_y(e, pprof, &steps, errbuf, errlen);
        if (s != ELLP_OPTIMAL) return s;
        HIPCHK(hipMemcpyAsync(e->cert_vec, e->post_y, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, e->stream));
        prof.end(CertProf::BASE);
        found = true;
    } else {
        const ellp_status s = range_inverse(e, nullptr, rprof, errbuf, errlen);  // the LU, y, d; W = B^-1
        if (s != ELLP_OPTIMAL) return s;
        prof.end(CertProf::BASE);
        CertFoldArgs f{};
        f.bits = e->cert_bits; f.B_index = e->B_index; f.N_index = e->N_index; f.Nb = e->Nb; f.kind = e->kindv; f.lb = e->lb; f.ub = e->ub;
        f.d = e->post_d; f.m = m; f.nN = nN; f.eps = e->eps; f.pick = e->cert_pick;
        if (source == ELLP_CERT_FARKAS_ROW) {
            prof.begin(CertProf::POINT);
            const int64_t wide = m > nN ? m : nN;
            HIPCHK(hipMemsetAsync(e->cert_x, 0, sizeof(double) * (size_t)n_c, e->stream));
            CERT_LAUNCH(k_cert_xn, dim3((unsigned)((wide + 255) / 256)), dim3(256), 0, e->stream, e->B_index, e->N_index, e->Nb, e->kindv, e->lb,
                        e->ub, e->cert_x, m, nN);
            const PostOver ov{e->c_B, e->c_N, e->post_y, e->cert_x, false};
            post_launch_pass(e, false, &ov);  // the partial sums of A_N x_N (d_N again, the same bits)
            start_fold(e, bB, bN, e->b_dev, e->cert_t);
            int32_t xsteps = 0;
            const ellp_status xs = cert_solve_x(e, pprof, &xsteps, errbuf, errlen);
            if (xs != ELLP_OPTIMAL) return xs;
            prof.end(CertProf::POINT);
            prof.begin(CertProf::TAB);
            cert_launch_tab(e, source, e->cert_x);
            f.x = e->cert_x;
            f.nblk = range_blocks(nN);
            CERT_LAUNCH(k_cert_ffold, dim3(1), dim3(1024), 0, e->stream, f);
            prof.end(CertProf::TAB);
        } else {
            prof.begin(CertProf::TAB);
            cert_launch_tab(e, source, e->x);
            f.x = e->x;
            f.nblk = (m + 127) / 128;
            CERT_LAUNCH(k_cert_rfold, dim3(1), dim3(1024), 0, e->stream, f);
            prof.end(CertProf::TAB);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(pick, e->cert_pick, sizeof(pick), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        if (pick[2]) {
            set_err(errbuf, errlen, "certificate: NaN in the tableau, the point or the reduced costs");
            return ELLP_ERR_NAN;
        }
        found = pick[0] >= 0;
        if (found && source == ELLP_CERT_FARKAS_ROW) {
            prof.begin(CertProf::VECTOR);
            CERT_LAUNCH(k_cert_unit, dim3(mb), dim3(256), 0, e->stream, e->cert_rhs, m, e->cert_pick);
            const PostOver ov{e->cert_rhs, e->cert_zero, e->cert_vec, e->x, false};
            const ellp_status s2 = post_solve_y(e, pprof, &steps, errbuf, errlen, &ov);
            if (s2 != ELLP_OPTIMAL) return s2;
            prof.end(CertProf::VECTOR);
        } else if (found) {
            prof.begin(CertProf::VECTOR);
            CERT_LAUNCH(k_cert_col, dim3(mb), dim3(256), 0, e->stream, e->A_N, ld, e->cert_t, m, e->cert_pick);
            HIPCHK(hipMemsetAsync(e->cert_x, 0, sizeof(double) * (size_t)n_c, e->stream));
            const ellp_status s2 = cert_solve_x(e, pprof, &steps, errbuf, errlen);
            if (s2 != ELLP_OPTIMAL) return s2;
            HIPCHK(hipMemsetAsync(e->cert_vec, 0, sizeof(double) * (size_t)n_c, e->stream));
            CERT_LAUNCH(k_cert_rvec, dim3(mb), dim3(256), 0, e->stream, e->cert_vec, e->cert_xb, e->B_index, e->N_index, m, n_check, e->cert_pick);
            prof.end(CertProf::VECTOR);
        }
    }
    CertVerify hv{};
    if (found) {
        prof.begin(CertProf::VERIFY);
        CertVerArgs va{};
        va.vec = e->cert_vec; va.b = e->b_dev; va.d = e->post_d; va.res = e->cert_res; va.c_B = e->c_B; va.c_N = e->c_N; va.lb = vlb; va.ub = vub;
        va.kind = vkind; va.B_index = e->B_index; va.N_index = e->N_index; va.m = m; va.nN = nN; va.n_check = n_check;
        va.out = reinterpret_cast<CertVerify *>(e->cert_ver);
        if (farkas) {
            const PostOver ov{e->cert_zero, e->cert_zero, e->cert_vec, e->x, false};
            post_launch_pass(e, true, &ov);  // post_d = -A^T y
            post_launch_pass(e, false, &ov);
            CERT_LAUNCH(k_cert_farkas, dim3(1), dim3(1024), 0, e->stream, va);
        } else {
            const PostOver ov{e->c_B, e->c_N, e->post_y, e->cert_vec, false};
            post_launch_pass(e, true, &ov);  // the partial sums of A r
            post_launch_pass(e, false, &ov);
            start_fold(e, 0, bB + bN, e->cert_zero, e->cert_res);
            CERT_LAUNCH(k_cert_ray, dim3(1), dim3(1024), 0, e->stream, va);
        }
        prof.end(CertProf::VERIFY);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&hv, e->cert_ver, sizeof(CertVerify), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipMemcpy(vec, e->cert_vec, sizeof(double) * (size_t)(farkas ? m : n_check), hipMemcpyDeviceToHost));
    }
    prof.report(source, m, nN);
    g_cert_calls.steps = (uint64_t)steps;
    g_cert_calls.launches = g_post_launches - launches0;
    memset(info, 0, sizeof(*info));
    info->kind = farkas ? ELLP_CERT_KIND_FARKAS : ELLP_CERT_KIND_RAY;
    info->found = found ? 1 : 0;
    info->source = source == ELLP_CERT_FARKAS_COSTS ? -1 : pick[0];
    info->qualifying = pick[1];
    info->worst_dir_var = info->worst_row = info->worst_bound_var = -1;
    if (found) {
        info->gap = hv.gap; info->y_b = hv.yb; info->sup = hv.sup; info->dir_violation = hv.dirv; info->residual = hv.residual;
        info->c_r = hv.c_r; info->bound_dir_violation = hv.bdv; info->norm = hv.norm; info->worst_dir_var = hv.wdir;
        info->worst_row = hv.wrow; info->worst_bound_var = hv.wbv;
    }
    info->refine_steps = steps;
    return ELLP_OPTIMAL;
}

// the refusals both forms share, host only; n: the columns of the standard form
bool cert_refused(int source, int64_t n_check, int64_t n, const uint8_t *chk_kind, const double *chk_lb, const double *chk_ub, const double *vec,
                  const ellp_cert_info *info, char *errbuf, size_t errlen) {
    if (source != ELLP_CERT_FARKAS_COSTS && source != ELLP_CERT_FARKAS_ROW && source != ELLP_CERT_RAY_COLUMN) {
        set_err(errbuf, errlen, "certificate: unknown source %d", source);
        return true;
    }
    if (n_check < 1 || n_check > n) {
        set_err(errbuf, errlen, "certificate: n_check = %lld is outside [1, %lld]", (long long)n_check, (long long)n);
        return true;
    }
    if (!vec || !info) {
        set_err(errbuf, errlen, "certificate: vec or info is NULL");
        return true;
    }
    const int given = (chk_kind != nullptr) + (chk_lb != nullptr) + (chk_ub != nullptr);
    if (given != 0 && given != 3) {
        set_err(errbuf, errlen, "certificate: chk_kind, chk_lb and chk_ub are given together or not at all");
        return true;
    }
    if (chk_kind)
        for (int64_t v = 0; v < n_check; ++v)
            if (chk_kind[v] > ELLP_BOUND_FIXED) {
                set_err(errbuf, errlen, "certificate: chk_kind[%lld] out of range", (long long)v);
                return true;
            }
    return false;
}

}  // namespace

extern "C" {

ellp_status ellp_engine_certificate(ellp_engine *e, int source, int64_t n_check, const uint8_t *chk_kind, const double *chk_lb,
                                    const double *chk_ub, double *vec, ellp_cert_info *info, char *errbuf, size_t errlen) {
    if (errbuf && errlen) errbuf[0] = 0;
    g_cert_calls.calls += 1;
    if (range_refused(e, "certificate", errbuf, errlen)) return ELLP_ERR_ARG;
    if (cert_refused(source, n_check, e->n, chk_kind, chk_lb, chk_ub, vec, info, errbuf, errlen)) return ELLP_ERR_ARG;
    ellp_status closing = ELLP_OPTIMAL;
    char err2[256];
    const ellp_status cs = post_complete_open(e, &closing, err2, sizeof(err2));  // the status that closes an open iteration is the run's
    if (cs != ELLP_OPTIMAL) {
        set_err(errbuf, errlen, "%s", err2);
        return cs;
    }
    return cert_compute(e, source, n_check, chk_kind, chk_lb, chk_ub, vec, info, errbuf, errlen);
}

ellp_status ellp_certificate(int64_t m, int64_t n, int64_t n_c, const double *A, const double *c, const double *b, const uint8_t *bound_kind,
                             const double *lb, const double *ub, const double *x, const int64_t *B_index, int64_t n_B, const int64_t *N_index,
                             const uint8_t *N_bound, int64_t n_N, const ellp_opts *opts_in, int source, int64_t n_check, const uint8_t *chk_kind,
                             const double *chk_lb, const double *chk_ub, double *vec, ellp_cert_info *info, char *errbuf, size_t errlen) {
    if (errbuf && errlen) errbuf[0] = 0;
    g_cert_calls.calls += 1;
    if (cert_refused(source, n_check, n, chk_kind, chk_lb, chk_ub, vec, info, errbuf, errlen)) return ELLP_ERR_ARG;
    PostOwn own(nullptr, ellp_engine_destroy);
    const ellp_status s = post_host_engine("certificate", m, n, n_c, A, c, b, bound_kind, lb, ub, x, B_index, n_B, N_index, N_bound, n_N, opts_in,
                                           own, errbuf, errlen);
    if (s != ELLP_OPTIMAL) return s;
    return cert_compute(own.get(), source, n_check, chk_kind, chk_lb, chk_ub, vec, info, errbuf, errlen);
}

void ellp_certificate_info(uint64_t *out4) {
    if (!out4) return;
    out4[0] = g_cert_calls.calls;
    out4[1] = g_cert_calls.launches;
    out4[2] = g_cert_calls.steps;
    out4[3] = 0;
}

}  // extern "C"

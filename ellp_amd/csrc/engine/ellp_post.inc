// ellp_post.inc — postsolve: duals, reduced costs, the row residual and a KKT report for the basis and point an engine
// stands on (ellp_engine_postsolve), or for a point in host memory (ellp_postsolve).  DESIGN.md §3.9.
//
//   y = B^-T c_B        from a FRESH LU of the current A_B (k_rows_from_cols, ellp_lu_rows_factor, k_lu_solve mode 1), never
//                       from the loop's carried u / y / explicit inverse;
//   d_v = c_v - a_v . y and r = b - sum_v x_v a_v   from ONE read of every stored column (k_post_pass), in compensated
//                       arithmetic: TwoProduct by fma, TwoSum, the Dot2 bound of Ogita, Rump and Oishi, each result rounded once;
//   singleton columns   a basic column a e_k fixes y_k = fl(c / a) on its own: imposed after the solve and after every step;
//   refinement of y     while omega = max_i |rho_i| / (|c_B| + |A_B|^T |y|)_i > 2u (rho = d on the basic variables, both out
//                       of the same pass): delta = B^-T rho, y += delta, the pass again over the basic columns;
//   the report          one block, NaN-propagating maxima (nanmax of k_drift_part's fold), compensated objectives.
//
// Nothing the engine reads later is written: the workspace (an m x m copy of A_B by rows with its LU work, vectors of m and
// n_c doubles, the partial sums of the pass) is the postsolve's own, made at the first call and released by
// ellp_engine_destroy; W, u, x, y, dd, DevState, the pipeline's buffers, the engine's mode and w_valid stay as they are.
// ensure_inverse is not called (it would change the mode for good).
//
// Geometry of the pass (it fixes the order of every sum: no floating-point atomics, two calls on one state give the same
// bits).  grid = (column blocks, row tiles), 256 threads = 4 waves.  A row tile is POST_TR = 512 rows: lane l of every wave
// owns rows 128 k + 2 l and 128 k + 2 l + 1 of the tile, k = 0..3 (one double2 load each, along the column, as the pricing
// kernels read).  A column block is cpb columns (post_cpb: 64, doubled until a pass has at most 1,024 blocks); wave w takes
// the block's columns w, w + 4, ...  The tile of y is staged in LDS once per workgroup and held in registers from there.
//   a_v . y   8 compensated products per lane, a 6-step butterfly over the wave, lane 0 writes (sum, correction, sum of
//             |a||y|) per (row tile, column); k_post_dfold folds the row tiles in tile order and rounds c_v - (s + c) once.
//   r         each lane carries (sum, correction) of x_v a_iv for its 8 rows over the wave's columns, in registers; the 4
//             waves are folded in wave order through LDS, the block's pairs written per (column block, row); k_post_rfold
//             folds b_i and the blocks in block order — the basic blocks first, then the nonbasic — and rounds once.
// Longest chain of compensated operations (the K of the bound in tests/postsolve_model.py):
//   d: 8 + 6 + ceil(m / 512) + 1;    r: cpb / 4 + 3 + (blocks of A_B + blocks of A_N) + 1.
//
// Included at the end of ellp_engine.hip.

namespace {

constexpr int POST_TR = 512;  // rows per tile
constexpr long long LLONG_MAX_POST = 0x7fffffffffffffffLL;  // "no index yet" of a maximum
// kernels enqueued so far by post_launch_pass, start_fold, start_solve_x and the certificates' own stages, each counted where
// it is launched (ellp_certificate_info reports the difference over a call; diagnostics, not thread safe)
uint64_t g_post_launches = 0;

// s + e = a + b exactly (Knuth)
__device__ __forceinline__ void post_two_sum(double a, double b, double &s, double &e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
// (s, c) += a * b, the product split by fma
__device__ __forceinline__ void post_dot2(double &s, double &c, double a, double b) {
    const double p = a * b;
    const double pe = fma(a, b, -p);
    double t, se;
    post_two_sum(s, p, t, se);
    s = t;
    c += se + pe;
}
// (s, c) += (s2, c2); symmetric in its operands, so both sides of a butterfly hold the same pair
__device__ __forceinline__ void post_merge(double &s, double &c, double s2, double c2) {
    double t, e;
    post_two_sum(s, s2, t, e);
    s = t;
    c = (c + c2) + e;
}

struct PostPassArgs {
    const double *C;        // the stored columns (A_B or A_N), leading dimension ld
    const int64_t *index;   // the variable of each column
    const double *y, *x;
    double *dpart;          // [row tile][column][3]: sum, correction, sum |a||y|
    double *rpart;          // [column block][row][2]
    int64_t m, ld, ncols, dstride, rblock0;
    int cpb;
};

__global__ __launch_bounds__(256) void k_post_pass(PostPassArgs a) {
    __shared__ double ys[POST_TR];
    __shared__ double rsh[4][POST_TR][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.y * POST_TR;
    for (int i = tid; i < POST_TR; i += 256) ys[i] = (r0 + i < a.m) ? a.y[r0 + i] : 0.0;
    __syncthreads();
    double yv[8], rs[8], rc[8];
    bool ok0[4], ok1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int li = 128 * k + 2 * lane;
        yv[2 * k] = ys[li];
        yv[2 * k + 1] = ys[li + 1];
        ok0[k] = r0 + li < a.m;
        ok1[k] = r0 + li + 1 < a.m;
        rs[2 * k] = rs[2 * k + 1] = rc[2 * k] = rc[2 * k + 1] = 0.0;
    }
    const int64_t c0 = (int64_t)blockIdx.x * a.cpb;
    const int64_t c1 = (c0 + a.cpb < a.ncols) ? c0 + a.cpb : a.ncols;
    for (int64_t j = c0 + wave; j < c1; j += 4) {
        const double xv = a.x[a.index[j]];
        const double *col = a.C + j * a.ld + r0 + 2 * lane;
        double2 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // ld is a multiple of 16 >= m: a row pair that starts below m lies inside the column
            v[k] = ok0[k] ? *reinterpret_cast<const double2 *>(col + 128 * k) : make_double2(0.0, 0.0);
            if (!ok1[k]) v[k].y = 0.0;  // the padding row of an odd m
        }
        double s = 0.0, c = 0.0, ab = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            post_dot2(s, c, v[k].x, yv[2 * k]);
            post_dot2(s, c, v[k].y, yv[2 * k + 1]);
            ab += fabs(v[k].x) * fabs(yv[2 * k]);
            ab += fabs(v[k].y) * fabs(yv[2 * k + 1]);
            post_dot2(rs[2 * k], rc[2 * k], xv, v[k].x);
            post_dot2(rs[2 * k + 1], rc[2 * k + 1], xv, v[k].y);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double s2 = __shfl_xor(s, off), c2 = __shfl_xor(c, off), ab2 = __shfl_xor(ab, off);
            post_merge(s, c, s2, c2);
            ab = ab + ab2;
        }
        if (lane == 0) {
            double *o = a.dpart + ((int64_t)blockIdx.y * a.dstride + j) * 3;
            o[0] = s;
            o[1] = c;
            o[2] = ab;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int li = 128 * k + 2 * lane;
        rsh[wave][li][0] = rs[2 * k];
        rsh[wave][li][1] = rc[2 * k];
        rsh[wave][li + 1][0] = rs[2 * k + 1];
        rsh[wave][li + 1][1] = rc[2 * k + 1];
    }
    __syncthreads();
    for (int i = tid; i < POST_TR; i += 256) {
        if (r0 + i >= a.m) continue;
        double s = rsh[0][i][0], c = rsh[0][i][1];
#pragma unroll
        for (int w = 1; w < 4; ++w) post_merge(s, c, rsh[w][i][0], rsh[w][i][1]);
        double *o = a.rpart + ((a.rblock0 + blockIdx.x) * a.m + r0 + i) * 2;
        o[0] = s;
        o[1] = c;
    }
}

// d_v = c_v - a_v . y per column, the row tiles folded in tile order; for the basic columns also rho by position and the
// denominator of omega
struct PostDfoldArgs {
    const double *dpart, *cpos;
    const int64_t *index;
    double *d, *rho, *den;  // rho, den: basic pass only (else null)
    int64_t ncols, dstride;
    int ntiles;
};
__global__ __launch_bounds__(256) void k_post_dfold(PostDfoldArgs a) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.ncols) return;
    double s = 0.0, c = 0.0, ab = 0.0;
    for (int t = 0; t < a.ntiles; ++t) {
        const double *p = a.dpart + ((int64_t)t * a.dstride + j) * 3;
        post_merge(s, c, p[0], p[1]);
        ab += p[2];
    }
    const double cv = a.cpos[j];
    double t, e;
    post_two_sum(cv, -s, t, e);
    const double dv = t + (e - c);
    a.d[a.index[j]] = dv;
    if (a.rho) {
        a.rho[j] = dv;
        a.den[j] = fabs(cv) + ab;
    }
}

// r_i = b_i - sum over the column blocks, in block order
__global__ __launch_bounds__(256) void k_post_rfold(const double *rpart, const double *b, double *r, int64_t m, int64_t nblocks) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    double s = b[i], c = 0.0;
    for (int64_t k = 0; k < nblocks; ++k) {
        const double *p = rpart + (k * m + i) * 2;
        post_merge(s, c, -p[0], -p[1]);
    }
    r[i] = s + c;
}

__global__ __launch_bounds__(256) void k_post_tail(const double *c_tail, double *d, int64_t n, int64_t n_c) {
    const int64_t v = n + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v < n_c) d[v] = c_tail[v - n];
}

__global__ __launch_bounds__(256) void k_post_axpy(double *y, const double *dy, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) y[i] = y[i] + dy[i];
}

// The basic columns with a single nonzero (slacks, artificials): column j = a e_k states a y_k = c_B[j] on its own, so
// y_k = fl(c_B[j] / a) is that component correctly rounded.  The LU does not deliver it when row k was taken as a pivot row
// before column j's turn: y_k then comes out of the general elimination, and where the true value is 0 a computed 1e-17
// is a componentwise backward error of 1 that no refinement step removes (each multiplies it by u, none makes it 0).
// One wave per column; sing_row[j] = k, sing_val[j] = a, or sing_row[j] = -1.
__global__ __launch_bounds__(256) void k_post_singletons(const double *A_B, int64_t m, int64_t ld, int64_t *sing_row, double *sing_val) {
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= m) return;
    const double *col = A_B + j * ld;
    int cnt = 0;
    long long row = -1;
    double val = 0.0;
    for (int64_t i = lane; i < m; i += 64) {
        const double v = col[i];
        if (v != 0.0) {  // a NaN counts
            cnt += 1;
            row = i;
            val = v;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int c2 = __shfl_xor(cnt, off);
        const long long r2 = __shfl_xor(row, off);
        const double v2 = __shfl_xor(val, off);
        if (r2 > row) {
            row = r2;
            val = v2;
        }
        cnt += c2;
    }
    if (lane == 0) {
        sing_row[j] = cnt == 1 ? row : -1;
        sing_val[j] = cnt == 1 ? val : 0.0;
    }
}
__global__ __launch_bounds__(256) void k_post_snap(double *y, const double *c_B, const int64_t *sing_row, const double *sing_val, int64_t m) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j < m && sing_row[j] >= 0) y[sing_row[j]] = c_B[j] / sing_val[j];  // two such columns in one row: a singular basis, refused before
}

// a maximum with its place: NaN wins (the smallest index that holds one), then the larger value, of equals the smaller index
struct PostMax {
    double v;
    long long i;
};
__device__ __forceinline__ PostMax post_max(PostMax a, PostMax b) {
    const bool an = a.v != a.v, bn = b.v != b.v;
    if (an || bn) {
        if (an && bn) return a.i < b.i ? a : b;
        return an ? a : b;
    }
    if (b.v > a.v) return b;
    if (b.v == a.v) return a.i < b.i ? a : b;
    return a;
}
__device__ PostMax post_block_max(PostMax mine, PostMax *sh) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = mine;
    __syncthreads();
    for (int s = 512; s >= 1; s >>= 1) {
        if (tid < s) sh[tid] = post_max(sh[tid], sh[tid + s]);
        __syncthreads();
    }
    return sh[0];
}
__device__ double post_block_sum(double s, double c, double *shs, double *shc) {
    const int tid = threadIdx.x;
    __syncthreads();
    shs[tid] = s;
    shc[tid] = c;
    __syncthreads();
    for (int h = 512; h >= 1; h >>= 1) {
        if (tid < h) {
            double s1 = shs[tid], c1 = shc[tid];
            post_merge(s1, c1, shs[tid + h], shc[tid + h]);
            shs[tid] = s1;
            shc[tid] = c1;
        }
        __syncthreads();
    }
    return shs[0] + shc[0];
}
// max(v, 0) that keeps a NaN and never returns -0.0
__device__ __forceinline__ double post_pos(double v) { return (v != v) ? v : (v > 0.0 ? v : 0.0); }
__device__ __forceinline__ double post_ratio(double rho, double den) {
    const double num = fabs(rho);
    if (num == 0.0) return 0.0;  // 0 / 0: a column and a cost of zeros has no backward error
    return num / den;
}

// omega of the current y (one block)
__global__ __launch_bounds__(1024) void k_post_omega(const double *rho, const double *den, int64_t m, double *omega) {
    __shared__ PostMax sh[1024];
    PostMax mine{0.0, LLONG_MAX_POST};
    for (int64_t i = threadIdx.x; i < m; i += 1024) mine = post_max(mine, PostMax{post_ratio(rho[i], den[i]), (long long)i});
    const PostMax w = post_block_max(mine, sh);
    if (threadIdx.x == 0) *omega = w.v;
}

struct PostReportArgs {
    const double *r, *d, *rho, *y, *b, *x, *lb, *ub, *c_B, *c_N, *c_tail;
    const uint8_t *kind, *Nb;
    const int64_t *B_index, *N_index;
    const double *omega;
    int64_t m, n, n_c, nN;
    int32_t steps;
    ellp_kkt *out;
};
// The report of one LP, by one workgroup of 1,024 threads (the strided sums and the trees fix the order of the objectives);
// k_post_report runs it for an engine, k_post_report_batch (ellp_bpost.inc) once per item of a batch
__device__ __forceinline__ void post_report(const PostReportArgs &a, int32_t steps) {
    __shared__ PostMax sh[1024];
    __shared__ double shs[1024], shc[1024];
    const int tid = threadIdx.x;
    // max_i |r_i|
    PostMax mine{0.0, LLONG_MAX_POST};
    for (int64_t i = tid; i < a.m; i += 1024) mine = post_max(mine, PostMax{fabs(a.r[i]), (long long)i});
    const PostMax pr = post_block_max(mine, sh);
    // bound violations by kind
    mine = PostMax{0.0, LLONG_MAX_POST};
    for (int64_t v = tid; v < a.n_c; v += 1024) {
        const double xv = a.x[v], l = a.lb[v], u = a.ub[v];
        double viol = 0.0;
        switch (a.kind[v]) {
        case ELLP_BOUND_LOWER: viol = post_pos(l - xv); break;
        case ELLP_BOUND_UPPER: viol = post_pos(xv - u); break;
        case ELLP_BOUND_TWOSIDED: viol = post_pos(nanmax(l - xv, xv - u)); break;
        case ELLP_BOUND_FIXED: viol = fabs(xv - l); break;
        default: viol = (xv != xv) ? xv : 0.0; break;  // Free: none, but a NaN is never hidden
        }
        mine = post_max(mine, PostMax{viol, (long long)v});
    }
    const PostMax bv = post_block_max(mine, sh);
    // dual infeasibility over the nonbasic positions
    mine = PostMax{0.0, LLONG_MAX_POST};
    for (int64_t j = tid; j < a.nN; j += 1024) {
        const int64_t v = a.N_index[j];
        const double dv = a.d[v];
        double inf;
        if (a.kind[v] == ELLP_BOUND_FIXED) inf = (dv != dv) ? dv : 0.0;
        else if (a.Nb[j] == ELLP_NB_LOWER) inf = post_pos(-dv);
        else if (a.Nb[j] == ELLP_NB_UPPER) inf = post_pos(dv);
        else inf = fabs(dv);
        mine = post_max(mine, PostMax{inf, (long long)v});
    }
    const PostMax di = post_block_max(mine, sh);
    // max |d| on the basis
    mine = PostMax{0.0, LLONG_MAX_POST};
    for (int64_t i = tid; i < a.m; i += 1024) mine = post_max(mine, PostMax{fabs(a.rho[i]), (long long)i});
    const PostMax br = post_block_max(mine, sh);
    // c . x: the basic positions, the nonbasic positions, the costs without a column
    double s = 0.0, c = 0.0;
    const int64_t total = a.m + a.nN + (a.n_c - a.n);
    for (int64_t k = tid; k < total; k += 1024) {
        double cv, xv;
        if (k < a.m) {
            cv = a.c_B[k];
            xv = a.x[a.B_index[k]];
        } else if (k < a.m + a.nN) {
            cv = a.c_N[k - a.m];
            xv = a.x[a.N_index[k - a.m]];
        } else {
            cv = a.c_tail[k - a.m - a.nN];
            xv = a.x[a.n + (k - a.m - a.nN)];
        }
        post_dot2(s, c, cv, xv);
    }
    const double pobj = post_block_sum(s, c, shs, shc);
    // b . y + the bound terms of StandardForm::dual_obj (standard_form.rs:52-68)
    s = 0.0;
    c = 0.0;
    for (int64_t k = tid; k < a.m + a.n_c; k += 1024) {
        if (k < a.m) {
            post_dot2(s, c, a.b[k], a.y[k]);
        } else {
            const int64_t v = k - a.m;
            const double dv = a.d[v];
            switch (a.kind[v]) {
            case ELLP_BOUND_LOWER: post_dot2(s, c, a.lb[v], dv); break;
            case ELLP_BOUND_UPPER: post_dot2(s, c, a.ub[v], dv); break;
            case ELLP_BOUND_TWOSIDED: post_dot2(s, c, (dv > 0.0) ? a.lb[v] : a.ub[v], dv); break;
            case ELLP_BOUND_FIXED: post_dot2(s, c, a.lb[v], dv); break;
            default: break;
            }
        }
    }
    const double dobj = post_block_sum(s, c, shs, shc);
    if (tid == 0) {
        ellp_kkt k;
        k.primal_residual = pr.v;
        k.bound_violation = bv.v;
        k.dual_infeasibility = di.v;
        k.basic_reduced_cost = br.v;
        k.y_backward_error = *a.omega;
        k.primal_obj = pobj;
        k.dual_obj = dobj;
        k.worst_row = (pr.v == 0.0) ? -1 : pr.i;
        k.worst_bound_var = (bv.v == 0.0) ? -1 : bv.i;
        k.worst_dual_var = (di.v == 0.0) ? -1 : di.i;
        k.refinement_steps = steps;
        k.reserved = 0;
        *a.out = k;
    }
}
__global__ __launch_bounds__(1024) void k_post_report(PostReportArgs a) { post_report(a, a.steps); }

int post_cpb(int64_t ncols) {
    int cpb = 64;
    while ((ncols + cpb - 1) / cpb > 1024) cpb *= 2;
    return cpb;
}
int64_t post_blocks(int64_t ncols) { return ncols > 0 ? (ncols + post_cpb(ncols) - 1) / post_cpb(ncols) : 0; }

// the workspace of the postsolve (allocated at the first use; the vectors through dmalloc, the LU work on its own).
// post_ready is set last: a call whose allocation failed half way leaves it false, and the next call allocates what is
// still missing instead of launching on null pointers; post_luw_ready tells ellp_engine_destroy that the LU work exists
template <typename T>
hipError_t post_alloc(ellp_engine *e, T **p, size_t count) { return *p ? hipSuccess : dmalloc(e, p, count); }

hipError_t post_workspace(ellp_engine *e) {
    if (e->post_ready) return hipSuccess;
    const int64_t m = e->m, ld = e->ld, nN = e->nN, n_c = e->n_c;
    const int64_t ntiles = (m + POST_TR - 1) / POST_TR, wide = m > nN ? m : nN;
    hipError_t rc;
    if (!e->post_luw_ready) {
        if ((rc = ellp_lu_rows_alloc(&e->post_luw, m)) != hipSuccess) {
            ellp_lu_rows_free(&e->post_luw);
            (void)hipGetLastError();
            return rc;
        }
        e->post_luw_ready = true;
    }
    if ((rc = post_alloc(e, &e->post_y, (size_t)ld)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->post_dy, (size_t)ld)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->post_rho, (size_t)ld)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->post_den, (size_t)ld)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->post_r, (size_t)ld)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->post_d, (size_t)n_c)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->post_dpart, (size_t)(ntiles * wide * 3))) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->post_rpart, (size_t)((post_blocks(m) + post_blocks(nN)) * m * 2))) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->post_omega, (size_t)2)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->post_kkt, (size_t)1)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->post_fail, (size_t)4)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->post_srow, (size_t)m)) != hipSuccess) return rc;
    if ((rc = post_alloc(e, &e->post_sval, (size_t)m)) != hipSuccess) return rc;
    if (16 * m > 65536)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_lu_solve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(16 * m));
    e->post_ready = true;
    return hipSuccess;
}

// what a pass or a solve takes in place of the engine's own vectors (ellp_cert.inc): the costs by position, the vector in
// y's place, the point; refactor false: post_luw already holds the LU of A_B
struct PostOver {
    const double *cB, *cN;
    double *y;
    const double *x;
    bool refactor;
};

void post_launch_pass(ellp_engine *e, bool basic, const PostOver *ov = nullptr) {
    const int64_t m = e->m, nN = e->nN;
    const int64_t ncols = basic ? m : nN;
    if (ncols <= 0) return;
    const int ntiles = (int)((m + POST_TR - 1) / POST_TR);
    PostPassArgs a{};
    a.C = basic ? e->A_B : e->A_N;
    a.index = basic ? e->B_index : e->N_index;
    a.y = ov ? ov->y : e->post_y;
    a.x = ov ? ov->x : e->x;
    a.dpart = e->post_dpart;
    a.rpart = e->post_rpart;
    a.m = m;
    a.ld = e->ld;
    a.ncols = ncols;
    a.dstride = m > nN ? m : nN;
    a.rblock0 = basic ? 0 : post_blocks(m);
    a.cpb = post_cpb(ncols);
    hipLaunchKernelGGL(k_post_pass, dim3((unsigned)post_blocks(ncols), (unsigned)ntiles), dim3(256), 0, e->stream, a);
    PostDfoldArgs f{};
    f.dpart = e->post_dpart;
    f.cpos = basic ? (ov ? ov->cB : e->c_B) : (ov ? ov->cN : e->c_N);
    f.index = a.index;
    f.d = e->post_d;
    f.rho = basic ? e->post_rho : nullptr;
    f.den = basic ? e->post_den : nullptr;
    f.ncols = ncols;
    f.dstride = a.dstride;
    f.ntiles = ntiles;
    hipLaunchKernelGGL(k_post_dfold, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, e->stream, f);
    g_post_launches += 2;
}

// ELLP_POST_PROFILE=1 (measurements, tools/postsolve_time.py): the stages of a postsolve bracketed with HIP events; one line on
// stderr per call, milliseconds of device time: the LU (with the copy of A_B by rows), the triangular solves, the pass
// (k_post_pass + k_post_dfold, basic and nonbasic), everything else (singletons, omega, the folds of r, the report)
struct PostProf {
    enum { LU = 0, SOLVE = 1, PASS = 2, REST = 3, NCAT = 4 };
    bool on;
    hipStream_t stream;
    const char *name = "postsolve_profile";  // the first word of the line (ellp_basis_start brackets its stages with the same struct)
    struct Span { int cat; hipEvent_t a, b; };
    std::vector<Span> spans;
    PostProf(hipStream_t s) : on(getenv("ELLP_POST_PROFILE") && getenv("ELLP_POST_PROFILE")[0] == '1'), stream(s) {}
    void begin(int cat) {
        if (!on) return;
        Span sp{cat, nullptr, nullptr};
        if (hipEventCreate(&sp.a) != hipSuccess || hipEventCreate(&sp.b) != hipSuccess) return;
        (void)hipEventRecord(sp.a, stream);
        spans.push_back(sp);
    }
    void end() {
        if (on && !spans.empty()) (void)hipEventRecord(spans.back().b, stream);
    }
    void report(int64_t m, int64_t nN, int steps) {  // after the stream has drained
        if (!on) return;
        double ms[NCAT] = {0};
        int passes = 0;
        for (Span &sp : spans) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, sp.a, sp.b) == hipSuccess) ms[sp.cat] += t;
            passes += sp.cat == PASS;
        }
        fprintf(stderr, "%s m=%lld nN=%lld steps=%d passes=%d lu_ms=%.4f solve_ms=%.4f pass_ms=%.4f rest_ms=%.4f\n", name, (long long)m,
                (long long)nN, steps, passes, ms[LU], ms[SOLVE], ms[PASS], ms[REST]);
    }
    ~PostProf() {
        for (Span &sp : spans) {
            if (sp.a) (void)hipEventDestroy(sp.a);
            if (sp.b) (void)hipEventDestroy(sp.b);
        }
    }
};

// the fresh LU of A_B and the refined y (post_y; rho, den and omega of it; the basic part of d and of the partial sums of r
// from the last pass over A_B); *steps: the refinement steps taken.  Shared by the postsolve and ellp_basis_start
ellp_status post_solve_y(ellp_engine *e, PostProf &prof, int32_t *steps_out, char *errbuf, size_t errlen, const PostOver *ov = nullptr) {
    const int64_t m = e->m, ld = e->ld;
    const double *cB = ov ? ov->cB : e->c_B;
    double *yv = ov ? ov->y : e->post_y;
    const size_t lds = 2 * sizeof(double) * (size_t)m;
    const unsigned mb = (unsigned)((m + 255) / 256);
    HIPCHK(hipMemsetAsync(e->post_fail, 0, sizeof(int), e->stream));
    if (!ov || ov->refactor) {
        prof.begin(PostProf::LU);
        hipLaunchKernelGGL(k_rows_from_cols, dim3((unsigned)((m + 31) / 32), (unsigned)((m + 31) / 32)), dim3(256), 0, e->stream, e->A_B,
                           e->post_luw.M, m, ld);
        ellp_lu_rows_factor(&e->post_luw, e->stream);
        prof.end();
    }
    prof.begin(PostProf::SOLVE);
    hipLaunchKernelGGL(k_lu_solve, dim3(1), dim3(1024), lds, e->stream, e->post_luw.M, e->post_luw.piv, m, cB, yv, 1, e->post_fail);
    prof.end();
    int fail = 0;
    HIPCHK(hipMemcpyAsync(&fail, e->post_fail, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipGetLastError());
    if (fail) {
        set_err(errbuf, errlen, "invalid B, A_B is not invertible");
        return ELLP_ERR_SINGULAR;
    }
    prof.begin(PostProf::REST);
    hipLaunchKernelGGL(k_post_singletons, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, e->stream, e->A_B, m, ld, e->post_srow, e->post_sval);
    hipLaunchKernelGGL(k_post_snap, dim3(mb), dim3(256), 0, e->stream, yv, cB, e->post_srow, e->post_sval, m);
    prof.end();
    const double two_u = 2.220446049250313e-16;  // 2 u, u = 2^-53
    double omega = 0.0, last = 0.0;
    int32_t steps = 0;
    for (;;) {
        prof.begin(PostProf::PASS);
        post_launch_pass(e, true, ov);
        prof.end();
        hipLaunchKernelGGL(k_post_omega, dim3(1), dim3(1024), 0, e->stream, e->post_rho, e->post_den, m, e->post_omega);
        HIPCHK(hipMemcpyAsync(&omega, e->post_omega, sizeof(double), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        // refine while omega > 2u, fewer than 4 steps were taken and the last step at least halved omega (a NaN ends it)
        if (!(omega > two_u) || steps >= 4 || (steps > 0 && !(omega <= 0.5 * last))) break;
        prof.begin(PostProf::SOLVE);
        hipLaunchKernelGGL(k_lu_solve, dim3(1), dim3(1024), lds, e->stream, e->post_luw.M, e->post_luw.piv, m, e->post_rho,
                           e->post_dy, 1, e->post_fail);
        prof.end();
        hipLaunchKernelGGL(k_post_axpy, dim3(mb), dim3(256), 0, e->stream, yv, e->post_dy, m);
        hipLaunchKernelGGL(k_post_snap, dim3(mb), dim3(256), 0, e->stream, yv, cB, e->post_srow, e->post_sval, m);
        last = omega;
        steps += 1;
    }
    *steps_out = steps;
    return ELLP_OPTIMAL;
}

// steps 2 to 5 on a complete state; the outputs are written only when everything succeeded
ellp_status post_compute(ellp_engine *e, double *y, double *d, double *r, ellp_kkt *kkt, char *errbuf, size_t errlen) {
    const int64_t m = e->m, nN = e->nN, n = e->n, n_c = e->n_c;
    HIPCHK(post_workspace(e));
    const unsigned mb = (unsigned)((m + 255) / 256);
    PostProf prof(e->stream);
    int32_t steps = 0;
    const ellp_status ys = post_solve_y(e, prof, &steps, errbuf, errlen);
    if (ys != ELLP_OPTIMAL) return ys;
    prof.begin(PostProf::PASS);
    post_launch_pass(e, false);
    prof.end();
    prof.begin(PostProf::REST);
    if (n_c > n) hipLaunchKernelGGL(k_post_tail, dim3((unsigned)((n_c - n + 255) / 256)), dim3(256), 0, e->stream, e->c_tail, e->post_d, n, n_c);
    hipLaunchKernelGGL(k_post_rfold, dim3(mb), dim3(256), 0, e->stream, e->post_rpart, e->b_dev, e->post_r, m,
                       post_blocks(m) + post_blocks(nN));
    PostReportArgs ra{};
    ra.r = e->post_r; ra.d = e->post_d; ra.rho = e->post_rho; ra.y = e->post_y; ra.b = e->b_dev; ra.x = e->x; ra.lb = e->lb; ra.ub = e->ub;
    ra.c_B = e->c_B; ra.c_N = e->c_N; ra.c_tail = e->c_tail; ra.kind = e->kindv; ra.Nb = e->Nb; ra.B_index = e->B_index;
    ra.N_index = e->N_index; ra.omega = e->post_omega; ra.m = m; ra.n = n; ra.n_c = n_c; ra.nN = nN; ra.steps = steps;
    ra.out = e->post_kkt;
    hipLaunchKernelGGL(k_post_report, dim3(1), dim3(1024), 0, e->stream, ra);
    prof.end();
    HIPCHK(hipGetLastError());
    ellp_kkt hk;
    HIPCHK(hipMemcpyAsync(&hk, e->post_kkt, sizeof(ellp_kkt), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    prof.report(m, nN, steps);
    if (y) HIPCHK(hipMemcpy(y, e->post_y, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost));
    if (d) HIPCHK(hipMemcpy(d, e->post_d, sizeof(double) * (size_t)n_c, hipMemcpyDeviceToHost));
    if (r) HIPCHK(hipMemcpy(r, e->post_r, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost));
    if (kkt) *kkt = hk;
    return ELLP_OPTIMAL;
}

// The host-memory forms (ellp_postsolve, ellp_ranging): the checks answered before any HIP call, then a minimal engine that
// holds the point in the engine's layout.  who: the caller's name in the messages.
typedef std::unique_ptr<ellp_engine, void (*)(ellp_engine *)> PostOwn;
// the checks (ellp_batch_postsolve makes them per item)
ellp_status post_host_checks(const char *who, int64_t m, int64_t n, int64_t n_c, const double *A, const double *c, const double *b,
                             const uint8_t *bound_kind, const double *lb, const double *ub, const double *x, const int64_t *B_index,
                             int64_t n_B, const int64_t *N_index, const uint8_t *N_bound, int64_t n_N, char *errbuf, size_t errlen) {
    if (m < 1) {
        set_err(errbuf, errlen, "%s: m < 1 (without rows y is empty and d = c: answered on the host)", who);
        return ELLP_ERR_ARG;
    }
    if (m > PLAN_MAX_M) {  // the engines' own limit (plan_engine); k_lu_solve keeps 16 m bytes in LDS
        set_err(errbuf, errlen, "%s: m = %lld rows, at most %lld (the limit of ellp_engine_create)", who, (long long)m, (long long)PLAN_MAX_M);
        return ELLP_ERR_ARG;
    }
    if (n < 0 || n_c < n || !A || !c || !b || !bound_kind || !lb || !ub || !x || !B_index || (n_N > 0 && (!N_index || !N_bound))) {
        set_err(errbuf, errlen, "%s: null pointer or inconsistent sizes", who);
        return ELLP_ERR_ARG;
    }
    if (n_B != m || n_N < 0 || n_B + n_N != n) {
        set_err(errbuf, errlen, "%s: invalid B/N, %lld + %lld elements for %lld rows and %lld columns", who, (long long)n_B,
                (long long)n_N, (long long)m, (long long)n);
        return ELLP_ERR_ARG;
    }
    const ellp_status cs = check_problem(ELLP_ENGINE_PRIMAL, m, n, n_c, A, c, b, bound_kind, lb, ub, x, B_index, n_B, N_index, N_bound,
                                         n_N, nullptr, nullptr, errbuf, errlen);
    if (cs != ELLP_OPTIMAL) return ELLP_ERR_ARG;  // an index, a label or a kind out of range
    return ELLP_OPTIMAL;
}
ellp_status post_host_engine(const char *who, int64_t m, int64_t n, int64_t n_c, const double *A, const double *c, const double *b,
                             const uint8_t *bound_kind, const double *lb, const double *ub, const double *x, const int64_t *B_index,
                             int64_t n_B, const int64_t *N_index, const uint8_t *N_bound, int64_t n_N, const ellp_opts *opts_in,
                             PostOwn &own, char *errbuf, size_t errlen) {
    const ellp_status chk = post_host_checks(who, m, n, n_c, A, c, b, bound_kind, lb, ub, x, B_index, n_B, N_index, N_bound, n_N, errbuf, errlen);
    if (chk != ELLP_OPTIMAL) return chk;
    ellp_opts opts;
    ellp_default_opts(&opts);
    if (opts_in) opts = *opts_in;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_err(errbuf, errlen, "no HIP device available (this library has no CPU path)");
        return ELLP_ERR_DEVICE;
    }
    // a minimal upload into the engine's layout: the stored columns, the costs by position, the point, the bounds and b —
    // no inverse, no pricing buffers, no loop; then the steps of ellp_engine_postsolve on the same kernels
    own.reset(new ellp_engine());
    ellp_engine *e = own.get();
    e->opts = opts;
    e->opts.profile = 0;
    e->eps = opts.eps > 0.0 ? opts.eps : 1e-10;
    e->kind = ELLP_ENGINE_PRIMAL;
    e->m = m;
    e->n = n;
    e->n_c = n_c;
    e->nN = n_N;
    e->ld = (m + 15) / 16 * 16;  // plan_engine's leading dimension
    ellp_status s = create_host_set(e, errbuf, errlen);
    if (s != ELLP_OPTIMAL) return s;
    const int64_t ld = e->ld, nNa = n_N > 0 ? n_N : 1;
    HIPCHK(dmalloc(e, &e->A_B, (size_t)(ld * m)));
    HIPCHK(dmalloc(e, &e->A_N, (size_t)(ld * nNa)));
    HIPCHK(dmalloc(e, &e->c_B, (size_t)m));
    HIPCHK(dmalloc(e, &e->c_N, (size_t)nNa));
    HIPCHK(dmalloc(e, &e->x, (size_t)n_c));
    HIPCHK(dmalloc(e, &e->lb, (size_t)n_c));
    HIPCHK(dmalloc(e, &e->ub, (size_t)n_c));
    HIPCHK(dmalloc(e, &e->kindv, (size_t)n_c));
    HIPCHK(dmalloc(e, &e->b_dev, (size_t)ld));
    HIPCHK(dmalloc(e, &e->B_index, (size_t)m));
    HIPCHK(dmalloc(e, &e->N_index, (size_t)nNa));
    HIPCHK(dmalloc(e, &e->Nb, (size_t)nNa));
    HIPCHK(dmalloc(e, &e->st, 1));
    HIPCHK(hipMemsetAsync(e->b_dev, 0, sizeof(double) * (size_t)ld, e->stream));
    return create_upload(e, A, c, b, bound_kind, lb, ub, x, B_index, N_index, N_bound, nullptr, nullptr, n, errbuf, errlen);
}

// An iteration the two-launch pipeline has left open is completed first, exactly as ellp_engine_read_point does; *closing: the
// status that produced (ELLP_OPTIMAL: none)
ellp_status post_complete_open(ellp_engine *e, ellp_status *closing, char *errbuf, size_t errlen) {
    e->hst_fresh = false;  // anything but ellp_engine_run may change the device state behind h_st
    HIPCHK(hipSetDevice(e->device));
    const bool was_open = e->lag_open;
    launch_flush(e);
    *closing = ELLP_OPTIMAL;
    if (was_open) {
        HIPCHK(read_state(e));
        adopt_fin(e);
        const int32_t stt = e->h_st->status;
        if (stt != ST_RUNNING && stt != ST_NEED_MAINT && stt != ELLP_OPTIMAL) *closing = status_message(*e->h_st, errbuf, errlen);
    }
    return ELLP_OPTIMAL;
}

}  // namespace

extern "C" {

ellp_status ellp_engine_postsolve(ellp_engine *e, double *y, double *d, double *r, ellp_kkt *kkt, char *errbuf, size_t errlen) {
    if (errbuf && errlen) errbuf[0] = 0;
    if (!e) {
        set_err(errbuf, errlen, "postsolve: no engine");
        return ELLP_ERR_ARG;
    }
    if (!y && !d && !r && !kkt) {
        set_err(errbuf, errlen, "postsolve: none of y, d, r, kkt is wanted");
        return ELLP_ERR_ARG;
    }
    if (e->world > 1 || e->colshard) {
        set_err(errbuf, errlen, "postsolve: not on a sharded engine (every rank holds a part of the columns or of the pricing)");
        return ELLP_ERR_ARG;
    }
    if (e->h_st && e->h_st->status < 0) {
        set_err(errbuf, errlen, "postsolve: the engine ended with an error (status %d): there is no point to examine", (int)e->h_st->status);
        return ELLP_ERR_ARG;
    }
    ellp_status closing = ELLP_OPTIMAL;
    const ellp_status cs = post_complete_open(e, &closing, errbuf, errlen);
    if (cs != ELLP_OPTIMAL) return cs;
    char err2[256];
    const ellp_status s = post_compute(e, y, d, r, kkt, closing == ELLP_OPTIMAL ? errbuf : err2, closing == ELLP_OPTIMAL ? errlen : sizeof(err2));
    if (s != ELLP_OPTIMAL) {
        if (closing != ELLP_OPTIMAL) set_err(errbuf, errlen, "%s", err2);
        return s;
    }
    return closing;
}

ellp_status ellp_postsolve(int64_t m, int64_t n, int64_t n_c, const double *A, const double *c, const double *b,
                           const uint8_t *bound_kind, const double *lb, const double *ub, const double *x, const int64_t *B_index,
                           int64_t n_B, const int64_t *N_index, const uint8_t *N_bound, int64_t n_N, const ellp_opts *opts_in,
                           double *y, double *d, double *r, ellp_kkt *kkt, char *errbuf, size_t errlen) {
    if (errbuf && errlen) errbuf[0] = 0;
    if (!y && !d && !r && !kkt) {
        set_err(errbuf, errlen, "postsolve: none of y, d, r, kkt is wanted");
        return ELLP_ERR_ARG;
    }
    PostOwn own(nullptr, ellp_engine_destroy);
    const ellp_status s = post_host_engine("postsolve", m, n, n_c, A, c, b, bound_kind, lb, ub, x, B_index, n_B, N_index, N_bound, n_N, opts_in,
                                           own, errbuf, errlen);
    if (s != ELLP_OPTIMAL) return s;
    return post_compute(own.get(), y, d, r, kkt, errbuf, errlen);
}

}  // extern "C"

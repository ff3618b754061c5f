// ellp_start.inc — a starting POINT from a BASIS (ellp_basis_start): what a warm-started solve hands to
// ellp_engine_create.  DESIGN.md §3.11.  Built on the postsolve's minimal engine and workspace (ellp_post.inc):
//
//   1  LU of A_B, y = B^-T c_B refined to omega <= 2u          post_solve_y, the postsolve's bits
//   2  d = c - A^T y                                            k_post_pass / k_post_dfold, the postsolve's bits
//   3  labels and nonbasic values, basic entries of x at +0.0   k_start_labels (new)
//   4  t = b - A_N x_N                                          the same pass: its partial sums of r over the nonbasic blocks
//   5  x_B = B^-1 t, refined as y is                            k_lu_solve mode 0; residual t - A_B x_B from the pass over the
//                                                               basic columns; k_start_xden, k_start_omega, k_start_axpy (new)
//   6  the KKT report of the point, the basic-only measures     k_post_report; k_start_verdict (new)
//
// Reads of A_N: KEEP_LABELS knows x_N before any d, so steps 2 and 4 are ONE pass over A_N.  LABELS_BY_D needs d_N for the
// labels, so A_N is read twice: once for d (x_N still zero), once for t.  A_B is read once per refinement pass of y, once
// per refinement pass of x_B, and once per pass by k_start_xden (|A_B| |x_B| is a sum over a ROW, which the pass, that sums
// |a||y| over columns, does not deliver).
//
// Orders (no floating-point atomics; two calls return the same bits): the sums of the pass as in ellp_post.inc;
// |A_B||x_B|_i in chunks of 256 columns, ascending inside a chunk, the chunks folded in ascending order; the maxima are
// exact (post_max); the sum of the basic violations: thread k of 1,024 takes positions k, k + 1024, ... in ascending
// order, compensated, then the tree of post_block_sum.  The count of changed labels is an integer sum.
//
// Singleton ROWS of A_B are snapped as the postsolve snaps y on singleton columns: a row i whose only nonzero is a, at position
// k, states a x_k = t_i on its own, so x_k = fl(t_i / a) is imposed after the solve and after every step (k_start_rowsing,
// k_start_snap).  Without it a degenerate basis keeps omega_x = 1 for good: where t_i = 0 the true x_k is 0, the solve returns
// 1e-17, and a refinement step multiplies that by u but never makes it 0 (afiro's optimal basis has such a row).
//
// Included at the end of ellp_engine.hip, after ellp_post.inc.

namespace {

constexpr int START_XC = 256;  // columns per chunk of |A_B||x_B|

struct StartLabelArgs {
    const int64_t *B_index, *N_index;
    uint8_t *Nb;
    const uint8_t *kind;
    const double *lb, *ub, *d;
    double *x;
    int64_t m, nN;
    int by_d;
    unsigned long long *changed;
};
// the label and the value of the nonbasic variable v by its kind (TwoSided: the given label, or the sign of d); shared
// with k_start_batch (ellp_bstart.inc)
__device__ __forceinline__ void start_label(const uint8_t *kind, const double *lb, const double *ub, const double *d, int by_d, int64_t v,
                                            int old, int &label, double &val) {
    label = ELLP_NB_LOWER;
    val = 0.0;
    switch (kind[v]) {
    case ELLP_BOUND_FREE: label = ELLP_NB_FREE; val = 0.0; break;
    case ELLP_BOUND_LOWER: label = ELLP_NB_LOWER; val = lb[v]; break;
    case ELLP_BOUND_UPPER: label = ELLP_NB_UPPER; val = ub[v]; break;
    case ELLP_BOUND_TWOSIDED:
        if (by_d) label = (d[v] < 0.0) ? ELLP_NB_UPPER : ELLP_NB_LOWER;  // d >= 0 or NaN: Lower
        else label = (old == ELLP_NB_UPPER) ? ELLP_NB_UPPER : ELLP_NB_LOWER;  // a given Free: Lower
        val = (label == ELLP_NB_UPPER) ? ub[v] : lb[v];
        break;
    default: label = ELLP_NB_LOWER; val = lb[v]; break;  // Fixed
    }
}
// position j of N: label and value by kind; position i of B: x = +0.0
__global__ __launch_bounds__(256) void k_start_labels(StartLabelArgs a) {
    __shared__ int cnt[256];
    const int tid = threadIdx.x;
    const int64_t j = (int64_t)blockIdx.x * 256 + tid;
    int ch = 0;
    if (j < a.nN) {
        const int64_t v = a.N_index[j];
        const int old = a.Nb[j];
        int label;
        double val;
        start_label(a.kind, a.lb, a.ub, a.d, a.by_d, v, old, label, val);
        a.x[v] = val;
        a.Nb[j] = (uint8_t)label;
        ch = label != old;
    }
    if (j < a.m) a.x[a.B_index[j]] = 0.0;
    cnt[tid] = ch;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) cnt[tid] += cnt[tid + s];
        __syncthreads();
    }
    if (tid == 0 && cnt[0]) atomicAdd(a.changed, (unsigned long long)cnt[0]);
}

// part[chunk][i] = sum over the chunk's columns j, ascending, of |A_B[i][j]| |xb[j]|
__global__ __launch_bounds__(256) void k_start_xden(const double *A_B, const double *xb, double *part, int64_t m, int64_t ld) {
    __shared__ double xs[START_XC];
    const int64_t j0 = (int64_t)blockIdx.y * START_XC;
    const int64_t j1 = (j0 + START_XC < m) ? j0 + START_XC : m;
    if (j0 + threadIdx.x < m) xs[threadIdx.x] = fabs(xb[j0 + threadIdx.x]);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    double s = 0.0;
    for (int64_t j = j0; j < j1; ++j) s += fabs(A_B[j * ld + i]) * xs[j - j0];
    part[(int64_t)blockIdx.y * m + i] = s;
}

// omega of x_B: max_i |res_i| / (|t_i| + sum of the chunks), one block
__global__ __launch_bounds__(1024) void k_start_omega(const double *res, const double *t, const double *part, int64_t m, int nchunks,
                                                      double *omega) {
    __shared__ PostMax sh[1024];
    PostMax mine{0.0, LLONG_MAX_POST};
    for (int64_t i = threadIdx.x; i < m; i += 1024) {
        double den = fabs(t[i]);
        for (int c = 0; c < nchunks; ++c) den += part[(int64_t)c * m + i];
        mine = post_max(mine, PostMax{post_ratio(res[i], den), (long long)i});
    }
    const PostMax w = post_block_max(mine, sh);
    if (threadIdx.x == 0) *omega = w.v;
}

// xb += dx (dx null: xb as it is), and x_B into x at B_index
__global__ __launch_bounds__(256) void k_start_axpy(double *xb, const double *dx, double *x, const int64_t *B_index, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    double v = xb[i];
    if (dx) {
        v = v + dx[i];
        xb[i] = v;
    }
    x[B_index[i]] = v;
}

// the rows of A_B with a single nonzero: its position (or -1) and value.  One thread per row, the columns in ascending order
// (neighbouring threads read neighbouring rows of a column)
__global__ __launch_bounds__(256) void k_start_rowsing(const double *A_B, int64_t m, int64_t ld, int64_t *sing_pos, double *sing_val) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    int cnt = 0;
    int64_t pos = -1;
    double val = 0.0;
    for (int64_t j = 0; j < m; ++j) {
        const double v = A_B[j * ld + i];
        if (v != 0.0) {  // a NaN counts
            cnt += 1;
            pos = j;
            val = v;
        }
    }
    sing_pos[i] = cnt == 1 ? pos : -1;
    sing_val[i] = cnt == 1 ? val : 0.0;
}
__global__ __launch_bounds__(256) void k_start_snap(double *xb, double *x, const double *t, const int64_t *B_index, const int64_t *sing_pos,
                                                    const double *sing_val, int64_t m) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m || sing_pos[i] < 0) return;  // two such rows with one position: a singular basis, refused before
    const double v = t[i] / sing_val[i];
    xb[sing_pos[i]] = v;
    x[B_index[sing_pos[i]]] = v;
}

struct StartVerdict {
    double pinf, psum;
    long long worst_primal;
    int32_t primal_feasible, dual_feasible;
};
struct StartVerdictArgs {
    const double *x, *lb, *ub;
    const uint8_t *kind;
    const int64_t *B_index;
    const ellp_kkt *kkt;
    int64_t m;
    double eps;
    StartVerdict *out;
};
// the bound violations of the BASIC positions (the nonbasic ones sit on their bounds by construction), and the two flags.
// One workgroup of 1,024 threads: k_start_verdict runs it for the single call, k_start_report_batch (ellp_bstart.inc) once
// per item of a batch
__device__ __forceinline__ void start_verdict(const StartVerdictArgs &a) {
    __shared__ PostMax sh[1024];
    __shared__ double shs[1024], shc[1024];
    const int tid = threadIdx.x;
    PostMax mine{0.0, LLONG_MAX_POST};
    double s = 0.0, c = 0.0;
    for (int64_t i = tid; i < a.m; i += 1024) {
        const int64_t v = a.B_index[i];
        const double xv = a.x[v], l = a.lb[v], u = a.ub[v];
        double viol = 0.0;
        switch (a.kind[v]) {  // as k_post_report
        case ELLP_BOUND_LOWER: viol = post_pos(l - xv); break;
        case ELLP_BOUND_UPPER: viol = post_pos(xv - u); break;
        case ELLP_BOUND_TWOSIDED: viol = post_pos(nanmax(l - xv, xv - u)); break;
        case ELLP_BOUND_FIXED: viol = fabs(xv - l); break;
        default: viol = (xv != xv) ? xv : 0.0; break;
        }
        mine = post_max(mine, PostMax{viol, (long long)v});
        double t, e;
        post_two_sum(s, viol, t, e);
        s = t;
        c += e;
    }
    const PostMax pv = post_block_max(mine, sh);
    const double psum = post_block_sum(s, c, shs, shc);
    if (tid == 0) {
        StartVerdict o;
        o.pinf = pv.v;
        o.psum = psum;
        o.worst_primal = (pv.v == 0.0) ? -1 : pv.i;
        const double di = a.kkt->dual_infeasibility, br = a.kkt->basic_reduced_cost;
        o.primal_feasible = (pv.v < a.eps) ? 1 : 0;           // a NaN compares false
        o.dual_feasible = (di < a.eps && br == br) ? 1 : 0;   // br: a NaN in c_B or y shows there even without nonbasic columns
        *a.out = o;
    }
}
__global__ __launch_bounds__(1024) void k_start_verdict(StartVerdictArgs a) { start_verdict(a); }

// t or a residual from the partial sums of the pass: base - (the blocks first .. first + count), in block order
void start_fold(ellp_engine *e, int64_t first, int64_t count, const double *base, double *out) {
    const int64_t m = e->m;
    hipLaunchKernelGGL(k_post_rfold, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, e->stream, e->post_rpart + first * m * 2, base, out, m,
                       count);
    g_post_launches += 1;
}

// Step 5, stated once: xb = B^-1 t with the LU in post_luw, written into x at B_index — the solve, the singleton-row snap, and
// refinement while omega_x > 2u, fewer than 4 steps were taken and the last step at least halved omega (the rule of y's
// refinement).  ov: whose point the residual pass reads (null: the engine's own x, which must then be w.x).  Shared by
// ellp_basis_start and the certificates (ellp_cert.inc)
struct StartXWork {
    double *t, *xb, *res, *dx, *xpart, *xomega, *x;
    int64_t *rs_pos;
    double *rs_val;
};
ellp_status start_solve_x(ellp_engine *e, const StartXWork &w, const PostOver *ov, PostProf &prof, double *omega_out, int32_t *steps_out,
                          char *errbuf, size_t errlen) {
    const int64_t m = e->m, ld = e->ld;
    const size_t lds = 2 * sizeof(double) * (size_t)m;
    const unsigned mb = (unsigned)((m + 255) / 256);
    const int nchunks = (int)((m + START_XC - 1) / START_XC);
    const int64_t bB = post_blocks(m);
    prof.begin(PostProf::SOLVE);
    hipLaunchKernelGGL(k_lu_solve, dim3(1), dim3(1024), lds, e->stream, e->post_luw.M, e->post_luw.piv, m, w.t, w.xb, 0, e->post_fail);
    prof.end();
    hipLaunchKernelGGL(k_start_axpy, dim3(mb), dim3(256), 0, e->stream, w.xb, (const double *)nullptr, w.x, e->B_index, m);
    hipLaunchKernelGGL(k_start_rowsing, dim3(mb), dim3(256), 0, e->stream, e->A_B, m, ld, w.rs_pos, w.rs_val);
    hipLaunchKernelGGL(k_start_snap, dim3(mb), dim3(256), 0, e->stream, w.xb, w.x, w.t, e->B_index, w.rs_pos, w.rs_val, m);
    g_post_launches += 4;
    const double two_u = 2.220446049250313e-16;
    double omega = 0.0, last = 0.0;
    int32_t xsteps = 0;
    for (;;) {
        prof.begin(PostProf::PASS);
        post_launch_pass(e, true, ov);  // the partial sums of A_B x_B (y is unchanged: rho, den and d on the basis keep their bits)
        prof.end();
        prof.begin(PostProf::REST);
        start_fold(e, 0, bB, w.t, w.res);
        hipLaunchKernelGGL(k_start_xden, dim3(mb, (unsigned)nchunks), dim3(256), 0, e->stream, e->A_B, w.xb, w.xpart, m, ld);
        hipLaunchKernelGGL(k_start_omega, dim3(1), dim3(1024), 0, e->stream, w.res, w.t, w.xpart, m, nchunks, w.xomega);
        g_post_launches += 2;
        prof.end();
        HIPCHK(hipMemcpyAsync(&omega, w.xomega, sizeof(double), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        if (!(omega > two_u) || xsteps >= 4 || (xsteps > 0 && !(omega <= 0.5 * last))) break;
        prof.begin(PostProf::SOLVE);
        hipLaunchKernelGGL(k_lu_solve, dim3(1), dim3(1024), lds, e->stream, e->post_luw.M, e->post_luw.piv, m, w.res, w.dx, 0, e->post_fail);
        prof.end();
        hipLaunchKernelGGL(k_start_axpy, dim3(mb), dim3(256), 0, e->stream, w.xb, (const double *)w.dx, w.x, e->B_index, m);
        hipLaunchKernelGGL(k_start_snap, dim3(mb), dim3(256), 0, e->stream, w.xb, w.x, w.t, e->B_index, w.rs_pos, w.rs_val, m);
        g_post_launches += 3;
        last = omega;
        xsteps += 1;
    }
    *omega_out = omega;
    *steps_out = xsteps;
    return ELLP_OPTIMAL;
}

// the refusals of ellp_basis_start, host only (ellp_batch_basis_start makes them per item)
ellp_status start_host_checks(int64_t m, int64_t n, const double *A, const double *c, const double *b, const uint8_t *bound_kind,
                              const double *lb, const double *ub, const int64_t *B_index, int64_t n_B, const int64_t *N_index,
                              const uint8_t *N_bound, int64_t n_N, int mode, const double *x, char *errbuf, size_t errlen) {
    if (mode != ELLP_START_KEEP_LABELS && mode != ELLP_START_LABELS_BY_D) {
        set_err(errbuf, errlen, "basis_start: unknown mode %d", mode);
        return ELLP_ERR_ARG;
    }
    if (m < 1 || m > PLAN_MAX_M) {
        set_err(errbuf, errlen, "basis_start: m = %lld rows, 1 to %lld are taken", (long long)m, (long long)PLAN_MAX_M);
        return ELLP_ERR_ARG;
    }
    if (!A || !c || !b || !bound_kind || !lb || !ub || !B_index || !x || (n_N > 0 && (!N_index || !N_bound))) {
        set_err(errbuf, errlen, "basis_start: null pointer");
        return ELLP_ERR_ARG;
    }
    if (n_B != m || n_N < 0 || n_B + n_N != n) {
        set_err(errbuf, errlen, "basis_start: invalid B/N, %lld + %lld elements for %lld rows and %lld columns", (long long)n_B,
                (long long)n_N, (long long)m, (long long)n);
        return ELLP_ERR_ARG;
    }
    {
        std::vector<uint8_t> seen((size_t)n, 0);
        for (int64_t k = 0; k < n; ++k) {
            const int64_t v = k < m ? B_index[k] : N_index[k - m];
            if (v < 0 || v >= n) {
                set_err(errbuf, errlen, "basis_start: %s_index[%lld] = %lld out of range", k < m ? "B" : "N", (long long)(k < m ? k : k - m),
                        (long long)v);
                return ELLP_ERR_ARG;
            }
            if (seen[(size_t)v]) {
                set_err(errbuf, errlen, "basis_start: variable %lld is listed twice in B and N", (long long)v);
                return ELLP_ERR_ARG;
            }
            seen[(size_t)v] = 1;
        }
    }
    for (int64_t j = 0; j < n_N; ++j)
        if (N_bound[j] > ELLP_NB_FREE) {
            set_err(errbuf, errlen, "basis_start: N_bound[%lld] out of range", (long long)j);
            return ELLP_ERR_ARG;
        }
    for (int64_t v = 0; v < n; ++v)
        if (bound_kind[v] > ELLP_BOUND_FIXED) {
            set_err(errbuf, errlen, "basis_start: bound_kind[%lld] out of range", (long long)v);
            return ELLP_ERR_ARG;
        }
    return post_host_checks("basis_start", m, n, n, A, c, b, bound_kind, lb, ub, x, B_index, n_B, N_index, N_bound, n_N, errbuf, errlen);
}

}  // namespace

extern "C" {

ellp_status ellp_basis_start(int64_t m, int64_t n, const double *A, const double *c, const double *b, const uint8_t *bound_kind,
                             const double *lb, const double *ub, const int64_t *B_index, int64_t n_B, const int64_t *N_index,
                             uint8_t *N_bound, int64_t n_N, int mode, const ellp_opts *opts_in, double *x, double *y, double *d,
                             ellp_start_info *info, char *errbuf, size_t errlen) {
    if (errbuf && errlen) errbuf[0] = 0;
    // every refusal is answered before any HIP call
    ellp_status s = start_host_checks(m, n, A, c, b, bound_kind, lb, ub, B_index, n_B, N_index, N_bound, n_N, mode, x, errbuf, errlen);
    if (s != ELLP_OPTIMAL) return s;
    const std::vector<double> zeros((size_t)n, 0.0);
    PostOwn own(nullptr, ellp_engine_destroy);
    s = post_host_engine("basis_start", m, n, n, A, c, b, bound_kind, lb, ub, zeros.data(), B_index, n_B, N_index, N_bound, n_N,
                                     opts_in, own, errbuf, errlen);
    if (s != ELLP_OPTIMAL) return s;
    ellp_engine *e = own.get();
    const int64_t ld = e->ld;
    HIPCHK(post_workspace(e));
    const int nchunks = (int)((m + START_XC - 1) / START_XC);
    double *t = nullptr, *xb = nullptr, *res = nullptr, *dx = nullptr, *xpart = nullptr, *xomega = nullptr;
    unsigned long long *changed = nullptr;
    StartVerdict *verdict = nullptr;
    int64_t *rs_pos = nullptr;
    double *rs_val = nullptr;
    HIPCHK(dmalloc(e, &rs_pos, (size_t)m));
    HIPCHK(dmalloc(e, &rs_val, (size_t)m));
    HIPCHK(dmalloc(e, &t, (size_t)ld));
    HIPCHK(dmalloc(e, &xb, (size_t)ld));
    HIPCHK(dmalloc(e, &res, (size_t)ld));
    HIPCHK(dmalloc(e, &dx, (size_t)ld));
    HIPCHK(dmalloc(e, &xpart, (size_t)((int64_t)nchunks * m)));
    HIPCHK(dmalloc(e, &xomega, (size_t)1));
    HIPCHK(dmalloc(e, &changed, (size_t)1));
    HIPCHK(dmalloc(e, &verdict, (size_t)1));
    HIPCHK(hipMemsetAsync(changed, 0, sizeof(unsigned long long), e->stream));
    PostProf prof(e->stream);
    prof.name = "basis_start_profile";
    // 1: LU and y
    int32_t ysteps = 0;
    s = post_solve_y(e, prof, &ysteps, errbuf, errlen);
    if (s != ELLP_OPTIMAL) return s;  // ELLP_ERR_SINGULAR: nothing was written
    const int64_t wide = m > n_N ? m : n_N;
    const int64_t bB = post_blocks(m), bN = post_blocks(n_N);
    StartLabelArgs la{};
    la.B_index = e->B_index; la.N_index = e->N_index; la.Nb = e->Nb; la.kind = e->kindv; la.lb = e->lb; la.ub = e->ub; la.d = e->post_d;
    la.x = e->x; la.m = m; la.nN = n_N; la.by_d = mode == ELLP_START_LABELS_BY_D; la.changed = changed;
    // 2 - 4: d, the labels and x_N, t
    if (mode == ELLP_START_LABELS_BY_D) {
        prof.begin(PostProf::PASS);
        post_launch_pass(e, false);  // d_N (x is zero)
        prof.end();
    }
    prof.begin(PostProf::REST);
    hipLaunchKernelGGL(k_start_labels, dim3((unsigned)((wide + 255) / 256)), dim3(256), 0, e->stream, la);
    prof.end();
    prof.begin(PostProf::PASS);
    post_launch_pass(e, false);  // d_N (the same bits again in LABELS_BY_D) and the partial sums of A_N x_N
    prof.end();
    prof.begin(PostProf::REST);
    start_fold(e, bB, bN, e->b_dev, t);
    prof.end();
    // 5: x_B and its refinement
    double omega = 0.0;
    int32_t xsteps = 0;
    const StartXWork xw{t, xb, res, dx, xpart, xomega, e->x, rs_pos, rs_val};
    s = start_solve_x(e, xw, nullptr, prof, &omega, &xsteps, errbuf, errlen);
    if (s != ELLP_OPTIMAL) return s;
    // 6: the report of the finished point and the verdict
    prof.begin(PostProf::REST);
    start_fold(e, 0, bB + bN, e->b_dev, e->post_r);
    PostReportArgs ra{};
    ra.r = e->post_r; ra.d = e->post_d; ra.rho = e->post_rho; ra.y = e->post_y; ra.b = e->b_dev; ra.x = e->x; ra.lb = e->lb; ra.ub = e->ub;
    ra.c_B = e->c_B; ra.c_N = e->c_N; ra.c_tail = e->c_tail; ra.kind = e->kindv; ra.Nb = e->Nb; ra.B_index = e->B_index;
    ra.N_index = e->N_index; ra.omega = e->post_omega; ra.m = m; ra.n = n; ra.n_c = n; ra.nN = n_N; ra.steps = ysteps;
    ra.out = e->post_kkt;
    hipLaunchKernelGGL(k_post_report, dim3(1), dim3(1024), 0, e->stream, ra);
    StartVerdictArgs va{};
    va.x = e->x; va.lb = e->lb; va.ub = e->ub; va.kind = e->kindv; va.B_index = e->B_index; va.kkt = e->post_kkt; va.m = m; va.eps = e->eps;
    va.out = verdict;
    hipLaunchKernelGGL(k_start_verdict, dim3(1), dim3(1024), 0, e->stream, va);
    prof.end();
    HIPCHK(hipGetLastError());
    ellp_kkt hk;
    StartVerdict hv;
    unsigned long long hchanged = 0;
    HIPCHK(hipMemcpyAsync(&hk, e->post_kkt, sizeof(ellp_kkt), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(&hv, verdict, sizeof(StartVerdict), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(&hchanged, changed, sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    prof.report(m, n_N, ysteps + xsteps);
    HIPCHK(hipMemcpy(x, e->x, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    if (n_N > 0) HIPCHK(hipMemcpy(N_bound, e->Nb, (size_t)n_N, hipMemcpyDeviceToHost));
    if (y) HIPCHK(hipMemcpy(y, e->post_y, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost));
    if (d) HIPCHK(hipMemcpy(d, e->post_d, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    if (info) {
        memset(info, 0, sizeof(*info));
        info->primal_infeasibility = hv.pinf;
        info->primal_infeasibility_sum = hv.psum;
        info->dual_infeasibility = hk.dual_infeasibility;
        info->x_backward_error = omega;
        info->worst_primal_var = hv.worst_primal;
        info->worst_dual_var = hk.worst_dual_var;
        info->labels_changed = (int64_t)hchanged;
        info->primal_feasible = hv.primal_feasible;
        info->dual_feasible = hv.dual_feasible;
        info->x_refinement_steps = xsteps;
        info->kkt = hk;
    }
    return ELLP_OPTIMAL;
}

}  // extern "C"

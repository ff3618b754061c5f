// ellp_exact.inc — the certificate of the certified hybrid ABOVE 1,024 rows (DESIGN.md §3.1c), where the persistent
// LU-per-iteration kernel of ellp_mid.inc (a thread per row) no longer fits: one iteration of the loop with everything that
// decides it taken from a FRESH LU factorisation of the basis, as the reference takes it every iteration
// (primal_simplex_solver.rs:173-189,289-300,404-406; dual_simplex_solver.rs:241-253,281-284,294) —
//   * the LU: partial pivoting, first maximum, multipliers a (1/diag), the oracle's lu_factor_inplace number for number
//     (ellp_lu.hip's blocked right-looking kernels on a copy of A_B stored by rows; two launches per 16-column panel);
//   * the solves with it: one workgroup each, the vector in LDS, one barrier pair per step (k_lu_solve);
//   * everything else — pricing, the entering fold, the ratio test, the updates — by the engine's own bandwidth kernels,
//     fed the EXACT u (or rho) and the EXACT d = B^-1 a_q instead of the explicit inverse's.
// A structural zero of B^-1 a_q is an exact zero again (the elimination never touches it), which is what the explicit
// inverse cannot deliver on ill-conditioned bases.  Used when the explicit-inverse loop reports a terminal status: if this
// iteration ends the same way, the status is certified; if it pivots, the pivot is made (with the exact d) and the loop
// goes on.  Cost: the LU (5.5 ms at m = 1100, 12 ms at m = 1850) + two (primal) or three (dual) solves of m steps — paid once
// per phase by the certificate, per iteration by a repeated phase and by an engine made with pipeline = 3 above 1,024 rows
// (run_exact_large, DESIGN.md §3.1d).
//
// Included inside the anonymous namespace of ellp_engine.hip.

// M[r * m + k] = A_B[k * ld + r]  (the basis by rows, for ellp_lu_rows_factor)
__global__ __launch_bounds__(256) void k_rows_from_cols(const double *A_B, double *M, int64_t m, int64_t ld) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const int64_t r0 = (int64_t)blockIdx.x * 32, k0 = (int64_t)blockIdx.y * 32;
    for (int s = ty; s < 32; s += 8) {
        const int64_t k = k0 + s, r = r0 + tx;
        tile[s][tx] = (k < m && r < m) ? A_B[k * ld + r] : 0.0;
    }
    __syncthreads();
    for (int s = ty; s < 32; s += 8) {
        const int64_t r = r0 + s, k = k0 + tx;
        if (r < m && k < m) M[r * m + k] = tile[tx][s];
    }
}

// One workgroup, the vector in LDS.  M: the factors by rows (row = position), piv: the transposition list.
//   mode 0  x = U^-1 L^-1 P b   (oracle lu_solve: P as the recorded swaps in order; L column by column with the zero skip;
//                                U column by column from the last, x_i = b_i / U_ii first)
//   mode 1  x = P^-1 L^-T U^-T b (oracle lu_btran).  U^T: x_i = (b_i - sum_{k<i} U[k,i] x_k) / U_ii, the sum accumulated in
//           ascending k as the oracle's dot product is (step k adds U[k,i] x_k to every later i's accumulator);  L^T: step k
//           (descending) subtracts L[k,i] x_k from every earlier b_i — the oracle sums the same terms in ascending k and
//           subtracts the sum: equal up to the rounding of a sum of at most m terms, the one place this certificate is not
//           the oracle's arithmetic bit for bit (the persistent kernels are).
// *fail = 1: a zero on U's diagonal (the reference's unwrap() on None).
__global__ __launch_bounds__(1024) void k_lu_solve(const double *M, const int64_t *piv, int64_t m, const double *in, double *out, int mode, int *fail) {
    extern __shared__ __align__(16) unsigned char lu_smem[];
    double *s = reinterpret_cast<double *>(lu_smem);
    double *acc = s + m;  // mode 1 only
    __shared__ int s_fail;
    const int tid = threadIdx.x;
    if (tid == 0) s_fail = 0;
    for (int64_t i = tid; i < m; i += 1024) {
        s[i] = in[i];
        if (mode == 1) acc[i] = 0.0;
    }
    __syncthreads();
    if (mode == 0) {
        if (tid == 0)
            for (int64_t i = 0; i < m; ++i) {
                const int64_t p = piv[i];
                if (p != i) {
                    const double t = s[i];
                    s[i] = s[p];
                    s[p] = t;
                }
            }
        __syncthreads();
        for (int64_t i = 0; i + 1 < m; ++i) {
            const double coeff = s[i];
            if (coeff != 0.0) {
                const double a = -coeff;
                for (int64_t r = i + 1 + tid; r < m; r += 1024) s[r] = a * M[r * m + i] + s[r];
            }
            __syncthreads();
        }
        for (int64_t i = m - 1; i >= 0; --i) {
            const double diag = M[i * m + i];
            if (diag == 0.0) {
                if (tid == 0) s_fail = 1;
                __syncthreads();
                break;
            }
            const double coeff = s[i] / diag;
            __syncthreads();
            if (tid == 0) s[i] = coeff;
            if (coeff != 0.0) {
                const double a = -coeff;
                for (int64_t r = tid; r < i; r += 1024) s[r] = a * M[r * m + i] + s[r];
            }
            __syncthreads();
        }
    } else {
        for (int64_t i = 0; i < m; ++i) {
            const double diag = M[i * m + i];
            if (diag == 0.0) {
                if (tid == 0) s_fail = 1;
                __syncthreads();
                break;
            }
            double xi = s[i] - acc[i];
            xi = xi / diag;
            __syncthreads();
            if (tid == 0) s[i] = xi;
            const double *urow = M + i * m;
            for (int64_t k = i + 1 + tid; k < m; k += 1024) acc[k] = acc[k] + urow[k] * xi;
            __syncthreads();
        }
        if (!s_fail) {
            for (int64_t k = m - 1; k > 0; --k) {
                const double xk = s[k];
                if (xk != 0.0) {
                    const double *lrow = M + k * m;
                    for (int64_t i = tid; i < k; i += 1024) s[i] = s[i] - lrow[i] * xk;
                }
                __syncthreads();
            }
            if (tid == 0)
                for (int64_t i = m - 1; i >= 0; --i) {
                    const int64_t p = piv[i];
                    if (p != i) {
                        const double t = s[i];
                        s[i] = s[p];
                        s[p] = t;
                    }
                }
            __syncthreads();
        }
    }
    if (s_fail) {
        if (tid == 0) *fail = 1;
        return;
    }
    for (int64_t i = tid; i < m; i += 1024) out[i] = s[i];
}

// the entering column the fold of k_ftran2 chose, as the right-hand side of the exact FTRAN
__global__ __launch_bounds__(256) void k_exact_gather_aq(const double *A_N, const DevState *st, int64_t m, int64_t ld, double *rhs) {
    if (st->status != ST_RUNNING) return;
    const int64_t q = st->s_q;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) rhs[i] = A_N[q * ld + i];
}

// primal: d = +-(exact B^-1 a_q) and, per basic row, lambda_i / the variable / the sign of d_i — what k_ftran2's epilogue
// leaves for the ratio-test fold of k_update2 (primal…:295-300, :320-367), from the exact solve
struct ExactLamArgs {
    const double *sol;
    double *d, *lam;
    int32_t *bidx;
    uint8_t *dpos;
    const int64_t *B_index;
    const double *x, *lb, *ub;
    const uint8_t *kind;
    DevState *st;
    int64_t m;
    double eps;
    const int *fail;
};
__global__ __launch_bounds__(256) void k_exact_relam(ExactLamArgs a) {
    if (a.st->status != ST_RUNNING || *a.fail) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.m) return;
    const double di = a.st->s_at_lower ? -a.sol[i] : a.sol[i];
    a.d[i] = di;
    const int64_t bi = a.B_index[i];
    const double xi = a.x[bi], lbi = a.lb[bi], ubi = a.ub[bi];
    const int k = a.kind[bi];
    const double li = primal_lambda(di, xi, lbi, ubi, k, a.eps);  // primal…:320-367
    if (li != li) a.st->nan_flag = 1;
    a.lam[i] = li;
    a.bidx[i] = (int32_t)bi;
    a.dpos[i] = di > 0.0 ? 1 : 0;
}
// dual: alpha_q = the exact B^-1 a_q (dual…:294)
__global__ __launch_bounds__(256) void k_exact_copy(const double *src, double *dst, int64_t m, const DevState *st, const int *fail) {
    if (st->status != ST_RUNNING || *fail) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) dst[i] = src[i];
}
// u (both buffers of the two-launch pipeline) = the exact B^-T c_B
__global__ __launch_bounds__(256) void k_exact_put_u(const double *src, double *u, int64_t m, int64_t ld, const int *fail) {
    if (*fail) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < ld) {
        const double v = i < m ? src[i] : 0.0;
        u[i] = v;
        u[ld + i] = v;
    }
}
// dual: e_r as the right-hand side of the BTRAN that gives rho = row r of B^-1 (dual…:248-253)
__global__ __launch_bounds__(256) void k_exact_unit(double *rhs, int64_t m, const DevState *st) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) rhs[i] = (i == st->lr) ? 1.0 : 0.0;
}

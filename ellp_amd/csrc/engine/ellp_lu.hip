// ellp_lu.hip — LU with partial pivoting of A^T on the device (the basis of dual phase 1).
//
// The reference picks the starting basis of dual phase 1 from `std_form.A.transpose().lu()`
// (src/solvers/dual/dual_problem.rs:139-160): all it consumes is the row permutation (which columns of A become
// basic) and the diagonal of U (`< EPS` -> panic).  That is n·m² flop on one host core — 56 GFLOP and about a
// minute at config 3's shape, a quarter of an hour at config 5's — in front of a simplex loop that takes seconds.
//
// Same algorithm as ellp_amd/csrc/host/dense.h LU / oracle lu_factor_inplace (pivot = FIRST entry of maximal
// modulus in the column; a zero pivot column is skipped; multipliers a·(1/diag); trailing update
// c_k[r] = (-c_k[i])·c_i[r] + c_k[r], skipped for a zero c_k[i]), and every stored number is BITWISE the host
// loop's: an entry M[r,k] receives its updates in the order of the steps whatever thread makes them, each one
// a separately rounded multiply and add (compiled with -ffp-contract=off).
//
// M = A^T (nv x m) is walked through A's own column-major storage: row r of M is column r of A, m contiguous
// doubles — so a row swap moves two contiguous rows, the trailing update of a row is a contiguous stream, and
// the matrix needs no transposition.  Two launches per elimination step: in k_lut_step each wave updates one
// row (its multiplier from the pivot row parked in a scratch buffer) and reports |M[r, i+1]| for the next pivot
// search; the one-block k_lut_fold folds the per-block candidates (first maximum by row), parks the next pivot
// row and the row it displaces, and records the pivot — rows are swapped lazily: the displaced row is read
// from its parked copy by the wave that owns the pivot's old position.  (Folding in the block that finishes
// last, one launch per step, was measured first: every block then needs an agent-scope release fence, which on
// this part writes back its XCD's L2 — the per-XCD L2s are not coherent with each other — and a launch never
// took less than 110 us however little there was to eliminate.  A kernel boundary does that write-back once.)
// Right-looking and unblocked: the whole trailing matrix is read and written once per step (about
// 16·nv·m²/2 bytes in all: 0.3 TB at config 3's shape); a blocked variant would divide that by the panel width.
//
// The SQUARE device-resident matrix by rows (ellp_lu_rows_factor, below the rectangular kernels) has that blocked variant:
// panels of LUP_W = 16 columns, two launches per panel instead of two per column, the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "ellp_hip.h"
#include "ellp_lu_dev.h"

namespace {

struct LuState {
    long long piv;     // pivot row of the step the next k_lut_step eliminates
    double diag;       // its entry in the pivot column
    int32_t skip;      // diag == 0: the column is skipped (dense.h: `continue`)
    int32_t pad;
};
struct LuCand {
    double v;
    long long r;
};

constexpr int LU_RPB = 4;  // rows (= waves) per block

__device__ __forceinline__ bool lu_better(double ov, long long orr, double bv, long long br) {
    return orr >= 0 && (br < 0 || ov > bv || (ov == bv && orr < br));
}

// Launch `i` (i = -1: nothing to eliminate, only the candidates of column 0):
//   block 0            writes the pivot row of step i to position i (the other half of the lazy swap)
//   block 1 + b, wave w eliminates row r = i + 1 + 4 b + w with the pivot of step i and reports |M[r, i+1]|
__global__ __launch_bounds__(256) void k_lut_step(double *M, int64_t m, int64_t nv, int64_t i, const double *prow,
                                                  const double *irow, LuCand *cands, const LuState *st) {
    __shared__ double s_v[LU_RPB];
    __shared__ long long s_r[LU_RPB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long piv = st->piv;
    const bool skip = i < 0 || st->skip != 0;
    const int64_t nxt = i + 1;  // the column searched for the next step
    double cv = -1.0;
    long long cr = -1;
    if (blockIdx.x == 0) {
        if (!skip && piv != i)
            for (int64_t k = tid; k < m; k += 256) M[i * m + k] = prow[k];
    } else {
        const int64_t r = nxt + (int64_t)(blockIdx.x - 1) * LU_RPB + wave;
        if (r < nv) {
            double *dst = M + r * m;
            double first = 0.0;  // M[r, i+1] after this step
            if (!skip) {
                const bool moved = r == piv;  // this position receives the row the pivot displaced
                const double *src = moved ? irow : dst;
                const double inv_diag = 1.0 / st->diag;
                const double l = __dmul_rn(src[i], inv_diag);
                if (moved)
                    for (int64_t k = lane; k < i; k += 64) dst[k] = src[k];
                if (lane == 0) dst[i] = l;
                // four 64-entry chunks in flight per wave: the loop is a chain of dependent round trips otherwise
                for (int64_t k0 = nxt + lane; k0 < m; k0 += 256) {
                    double pv[4], sv[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int64_t k = k0 + 64 * u;
                        const int64_t kc = k < m ? k : m - 1;
                        pv[u] = prow[kc];
                        sv[u] = src[kc];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int64_t k = k0 + 64 * u;
                        if (k < m) {
                            const double f = -pv[u];
                            double val = sv[u];
                            if (f != 0.0) val = __dadd_rn(__dmul_rn(f, l), val);
                            if (f != 0.0 || moved) dst[k] = val;
                            if (u == 0 && k == nxt) first = val;
                        }
                    }
                }
            } else if (nxt < m && lane == 0) {
                first = dst[nxt];
            }
            if (nxt < m) {
                first = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(first)),
                                         __builtin_amdgcn_readfirstlane(__double2loint(first)));
                double v = fabs(first);
                if (v != v) v = (r == nxt) ? INFINITY : -1.0;  // `v > best` is false for a NaN: only the diagonal can carry one
                cv = v;
                cr = r;
            }
        }
    }
    if (nxt >= m) return;  // the last elimination: nothing to search
    if (lane == 0) {
        s_v[wave] = cv;
        s_r[wave] = cr;
    }
    __syncthreads();
    if (tid == 0) {
        double bv = s_v[0];
        long long br = s_r[0];
        for (int w = 1; w < LU_RPB; ++w)
            if (lu_better(s_v[w], s_r[w], bv, br)) {
                bv = s_v[w];
                br = s_r[w];
            }
        cands[blockIdx.x] = LuCand{bv, br};
    }
}

// one block of 1024 threads: the pivot of column nxt from the ncand per-block candidates, rows piv and nxt parked
__global__ __launch_bounds__(1024) void k_lut_fold(const double *M, int64_t m, int64_t nxt, const LuCand *cands,
                                                   unsigned ncand, double *prow, double *irow, LuState *st,
                                                   int64_t *pivot_out, double *udiag_out) {
    __shared__ double s_v[16];
    __shared__ long long s_r[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double bv = -1.0;
    long long br = -1;
    for (unsigned b = tid; b < ncand; b += 1024) {
        const LuCand c = cands[b];
        if (lu_better(c.v, c.r, bv, br)) {
            bv = c.v;
            br = c.r;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o);
        const long long orr = __shfl_xor(br, o);
        if (lu_better(ov, orr, bv, br)) {
            bv = ov;
            br = orr;
        }
    }
    if (lane == 0) {
        s_v[wave] = bv;
        s_r[wave] = br;
    }
    __syncthreads();
    bv = s_v[0];
    br = s_r[0];
    for (int w = 1; w < 16; ++w)
        if (lu_better(s_v[w], s_r[w], bv, br)) {
            bv = s_v[w];
            br = s_r[w];
        }
    // br >= 0: row nxt itself is always a candidate (nv >= m)
    const double diag = M[br * m + nxt];
    for (int64_t k = tid; k < m; k += 1024) {
        prow[k] = M[br * m + k];
        irow[k] = M[nxt * m + k];
    }
    if (tid == 0) {
        st->piv = br;
        st->diag = diag;
        st->skip = diag == 0.0 ? 1 : 0;
        pivot_out[nxt] = diag == 0.0 ? nxt : br;  // a skipped column appends no transposition (dense.h)
        udiag_out[nxt] = diag;
    }
}

// ---- blocked form for a square matrix by rows: panels of LUP_W columns.  An entry (r, k) still receives the updates of the
// steps i = 0 .. min(r, k) - 1 in ascending i, each a separately rounded multiply and add, skipped for a zero -M[i,k] and for
// a skipped (zero pivot) step — so every stored number is the unblocked form's.
//   panel kernel   ONE workgroup: columns j0 .. j0+w-1 of the rows j0 .. m-1; per column the pivot search (first maximum,
//                  k_lut_step's NaN rule), the exchange inside the panel, the scaling and the update of the panel's later
//                  columns; piv / udiag recorded.  No synchronisation across workgroups (see the header).  A thread keeps its
//                  rows' 16 entries in registers up to 2 rows per thread (k_lup_panel_reg<1>, <2>: up to 1,024 / 2,048 rows
//                  left); above that the rows stay in global memory, which is this CU's L1/L2 (k_lup_panel_mem).
//   update kernel  one workgroup per strip of 16 columns outside the panel, all rows: the panel's exchanges in step order
//                  (staged in LDS — everything a column needs lies in that column, so strips never wait for each other),
//                  right of the panel the panel's 16 rows finished (a chain of up to 15 steps per entry) and the trailing
//                  rows updated, each entry in a register through its 16 multiply-adds.
constexpr int LUP_W = 16;
constexpr int LUP_NT = 1024;

struct LupBest {
    double v;
    int r;
};
// workgroup-wide first maximum of (v, r); every thread returns it.  s_v / s_r: 16 entries each
__device__ __forceinline__ LupBest lup_reduce(double bv, int br, double *s_v, int *s_r) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o);
        const int orr = __shfl_xor(br, o);
        if (lu_better(ov, orr, bv, br)) {
            bv = ov;
            br = orr;
        }
    }
    if (lane == 0) {
        s_v[wave] = bv;
        s_r[wave] = br;
    }
    __syncthreads();
    bv = s_v[0];
    br = s_r[0];
#pragma unroll
    for (int w = 1; w < LUP_NT / 64; ++w)
        if (lu_better(s_v[w], s_r[w], bv, br)) {
            bv = s_v[w];
            br = s_r[w];
        }
    return LupBest{bv, br};
}
__device__ __forceinline__ double lup_key(double x, bool diagonal) {
    double v = fabs(x);
    if (v != v) v = diagonal ? INFINITY : -1.0;  // k_lut_step's rule: `v > best` is false for a NaN, only the diagonal can carry one
    return v;
}

// one row of a thread of k_lup_panel_reg: its 16 panel entries in registers (every index is a constant once the loops are
// unrolled: nothing may reach scratch memory)
struct LupRow {
    double a[LUP_W];
    int row;  // -1: none
    __device__ __forceinline__ void load(const double *M, int64_t m, int64_t j0, int w, int64_t r) {
        row = r < m ? (int)r : -1;
#pragma unroll
        for (int c = 0; c < LUP_W; ++c) a[c] = (r < m && c < w) ? M[r * m + j0 + c] : 0.0;
    }
    __device__ __forceinline__ void store(double *M, int64_t m, int64_t j0, int w) const {
        if (row < 0) return;
#pragma unroll
        for (int c = 0; c < LUP_W; ++c)
            if (c < w) M[(int64_t)row * m + j0 + c] = a[c];
    }
    __device__ __forceinline__ void candidate(int c, int i, double &bv, int &br) const {
        if (row >= i) {
            const double v = lup_key(a[c], row == i);
            if (br < 0 || v > bv) {
                bv = v;
                br = row;
            }
        }
    }
    __device__ __forceinline__ void publish(int p, int i, double *s_prow, double *s_irow) const {
        if (row == p) {
#pragma unroll
            for (int q = 0; q < LUP_W; ++q) s_prow[q] = a[q];
        }
        if (row == i) {
#pragma unroll
            for (int q = 0; q < LUP_W; ++q) s_irow[q] = a[q];
        }
    }
    __device__ __forceinline__ void eliminate(int c, int p, int i, double inv_diag, const double *s_prow, const double *s_irow) {
        if (p != i && row == p) {
#pragma unroll
            for (int q = 0; q < LUP_W; ++q) a[q] = s_irow[q];
        } else if (p != i && row == i) {
#pragma unroll
            for (int q = 0; q < LUP_W; ++q) a[q] = s_prow[q];
        }
        if (row > i) {
            const double l = __dmul_rn(a[c], inv_diag);
            a[c] = l;
#pragma unroll
            for (int q = 0; q < LUP_W; ++q)
                if (q > c) {
                    const double f = -s_prow[q];
                    if (f != 0.0) a[q] = __dadd_rn(__dmul_rn(f, l), a[q]);
                }
        }
    }
};

// rows j0 .. m-1 (at most RPT * 1024 of them, RPT = 1 or 2), thread t keeps rows j0 + t and j0 + t + 1024 in registers
template <int RPT>
__global__ __launch_bounds__(LUP_NT) void k_lup_panel_reg(double *M, int64_t m, int64_t j0, int64_t *piv, double *udiag) {
    __shared__ double s_v[LUP_NT / 64];
    __shared__ int s_r[LUP_NT / 64];
    __shared__ double s_prow[LUP_W], s_irow[LUP_W];
    const int tid = threadIdx.x;
    const int w = (int)(m - j0 < LUP_W ? m - j0 : LUP_W);
    LupRow r0, r1;
    r0.load(M, m, j0, w, j0 + tid);
    if (RPT > 1) r1.load(M, m, j0, w, j0 + tid + LUP_NT);
#pragma unroll
    for (int c = 0; c < LUP_W; ++c) {
        if (c < w) {
            const int i = (int)j0 + c;
            double bv = -1.0;
            int br = -1;
            r0.candidate(c, i, bv, br);
            if (RPT > 1) r1.candidate(c, i, bv, br);
            const int p = lup_reduce(bv, br, s_v, s_r).r;  // >= i: row i itself is always a candidate
            r0.publish(p, i, s_prow, s_irow);
            if (RPT > 1) r1.publish(p, i, s_prow, s_irow);
            __syncthreads();
            const double diag = s_prow[c];
            if (tid == 0) {
                piv[i] = diag == 0.0 ? i : p;  // a skipped column appends no transposition (dense.h)
                udiag[i] = diag;
            }
            if (diag != 0.0) {
                const double inv_diag = 1.0 / diag;
                r0.eliminate(c, p, i, inv_diag, s_prow, s_irow);
                if (RPT > 1) r1.eliminate(c, p, i, inv_diag, s_prow, s_irow);
            }
        }
    }
    r0.store(M, m, j0, w);
    if (RPT > 1) r1.store(M, m, j0, w);
}

// any number of rows: thread t owns rows j0 + t + 1024 k, which stay in memory
__global__ __launch_bounds__(LUP_NT) void k_lup_panel_mem(double *M, int64_t m, int64_t j0, int64_t *piv, double *udiag) {
    __shared__ double s_v[LUP_NT / 64];
    __shared__ int s_r[LUP_NT / 64];
    __shared__ double s_prow[LUP_W], s_irow[LUP_W];
    const int tid = threadIdx.x;
    const int w = (int)(m - j0 < LUP_W ? m - j0 : LUP_W);
    for (int c = 0; c < w; ++c) {
        const int64_t i = j0 + c;
        double bv = -1.0;
        int br = -1;
        for (int64_t r = j0 + tid; r < m; r += LUP_NT)
            if (r >= i) {
                const double v = lup_key(M[r * m + i], r == i);
                if (br < 0 || v > bv) {
                    bv = v;
                    br = (int)r;
                }
            }
        const int64_t p = lup_reduce(bv, br, s_v, s_r).r;
        if (tid < LUP_W) {
            s_prow[tid] = tid < w ? M[p * m + j0 + tid] : 0.0;
            s_irow[tid] = tid < w ? M[i * m + j0 + tid] : 0.0;
        }
        __syncthreads();
        const double diag = s_prow[c];
        if (tid == 0) {
            piv[i] = diag == 0.0 ? i : p;
            udiag[i] = diag;
        }
        if (diag != 0.0) {
            const double inv_diag = 1.0 / diag;
            if (p != i && tid < w) M[i * m + j0 + tid] = s_prow[tid];  // position i is read by nobody in this step
            for (int64_t r = j0 + tid; r < m; r += LUP_NT)
                if (r > i) {
                    double *dst = M + r * m + j0;
                    const bool moved = r == p;  // this position receives the row the pivot displaced (its old copy: s_irow)
                    const double *src = moved ? s_irow : dst;
                    const double l = __dmul_rn(src[c], inv_diag);
                    if (moved)
                        for (int q = 0; q < c; ++q) dst[q] = s_irow[q];
                    dst[c] = l;
                    for (int q = c + 1; q < w; ++q) {
                        const double f = -s_prow[q];
                        double val = src[q];
                        if (f != 0.0) val = __dadd_rn(__dmul_rn(f, l), val);
                        if (f != 0.0 || moved) dst[q] = val;
                    }
                }
        }
        // the next column's search reads what this step wrote: rows keep their threads; s_prow / s_irow are loaded from rows
        // other threads wrote only behind the barrier inside lup_reduce
    }
}

// strip s = columns 16 s .. 16 s + 15, all rows; the strip of the panel itself has nothing to do
__global__ __launch_bounds__(LUP_NT) void k_lup_update(double *M, int64_t m, int64_t j0, const int64_t *piv, const double *udiag) {
    __shared__ double s_val[2 * LUP_W][LUP_W];  // slot c: position j0 + c; slot 16 + c: the position step c exchanged with, if below the panel
    __shared__ double s_L[LUP_W][LUP_W];        // the panel's multipliers among its own 16 rows
    __shared__ int64_t s_pos[2 * LUP_W];        // -1: slot unused
    __shared__ int s_slot[LUP_W];               // the slot step c exchanges slot c with (c: no exchange)
    __shared__ int s_skip[LUP_W];
    const int tid = threadIdx.x;
    const int64_t k0 = (int64_t)blockIdx.x * LUP_W;
    if (k0 == j0) return;
    const bool right = k0 > j0;  // then the panel is a full one
    const int w = (int)(m - j0 < LUP_W ? m - j0 : LUP_W);
    if (tid == 0) {
        for (int c = 0; c < 2 * LUP_W; ++c) s_pos[c] = c < w ? j0 + c : -1;
        for (int c = 0; c < LUP_W; ++c) {
            int slot = c;
            if (c < w) {
                const int64_t p = piv[j0 + c];
                if (p < j0 + w) slot = (int)(p - j0);
                else {
                    slot = LUP_W + c;
                    for (int c2 = 0; c2 < c; ++c2)
                        if (s_pos[LUP_W + c2] == p) slot = LUP_W + c2;
                    s_pos[slot] = p;
                }
            }
            s_slot[c] = slot;
            s_skip[c] = c < w ? (udiag[j0 + c] == 0.0) : 1;
        }
    } else if (right && tid >= 256 && tid < 256 + LUP_W * LUP_W) {
        const int c = (tid - 256) >> 4, i = (tid - 256) & 15;
        s_L[c][i] = i < c ? M[(j0 + c) * m + j0 + i] : 0.0;
    }
    __syncthreads();
    const int sl = tid >> 4, cl = tid & 15;
    const int64_t k = k0 + cl;
    const int64_t pos = tid < 2 * LUP_W * LUP_W ? s_pos[sl] : -1;
    if (pos >= 0 && k < m) s_val[sl][cl] = M[pos * m + k];
    __syncthreads();
    if (tid < LUP_W && k < m) {
        for (int c = 0; c < w; ++c) {
            const int s = s_slot[c];
            if (s != c) {
                const double t = s_val[c][cl];
                s_val[c][cl] = s_val[s][cl];
                s_val[s][cl] = t;
            }
        }
        if (right)
            for (int c = 1; c < LUP_W; ++c) {
                double val = s_val[c][cl];
                for (int i = 0; i < c; ++i) {
                    const double f = s_skip[i] ? 0.0 : -s_val[i][cl];
                    if (f != 0.0) val = __dadd_rn(__dmul_rn(f, s_L[c][i]), val);
                }
                s_val[c][cl] = val;
            }
    }
    __syncthreads();
    if (pos >= 0 && k < m) M[pos * m + k] = s_val[sl][cl];
    if (!right) return;
    __syncthreads();  // the trailing rows an exchange has moved are read below by other threads
    if (k >= m) return;
    double f[LUP_W];
#pragma unroll
    for (int i = 0; i < LUP_W; ++i) f[i] = s_skip[i] ? 0.0 : -s_val[i][cl];
    for (int64_t r = j0 + LUP_W + sl; r < m; r += 2 * (LUP_NT / LUP_W)) {
        const int64_t r2 = r + LUP_NT / LUP_W;
        const bool two = r2 < m;
        const int64_t rb = two ? r2 : r;
        const double *la = M + r * m + j0, *lb = M + rb * m + j0;
        double va = M[r * m + k], vb = M[rb * m + k];
        double l1[LUP_W], l2[LUP_W];
#pragma unroll
        for (int i = 0; i < LUP_W; ++i) {
            l1[i] = la[i];
            l2[i] = lb[i];
        }
#pragma unroll
        for (int i = 0; i < LUP_W; ++i)
            if (f[i] != 0.0) {
                va = __dadd_rn(__dmul_rn(f[i], l1[i]), va);
                vb = __dadd_rn(__dmul_rn(f[i], l2[i]), vb);
            }
        M[r * m + k] = va;
        if (two) M[r2 * m + k] = vb;
    }
}

void set_err(char *errbuf, size_t len, const char *msg, hipError_t e) {
    if (errbuf && len) snprintf(errbuf, len, "%s: %s", msg, hipGetErrorString(e));
}

}  // namespace

// ---- the same factorisation of a DEVICE-RESIDENT square matrix stored by rows (ellp_lu_dev.h): the certificate of the
// certified hybrid above 1,024 rows (ellp_exact.inc) factors the basis with it.  M (m x m, row r at M + r m) is overwritten
// by the factors exactly as the oracle's lu_factor_inplace leaves them (L's multipliers below the diagonal, U on and above;
// rows in pivoted order), piv[i] = the row exchanged with row i at step i, udiag[i] = U_ii.
hipError_t ellp_lu_rows_alloc(EllpLuWork *w, int64_t m) {
    memset(w, 0, sizeof(*w));
    w->m = m;
    hipError_t rc;
    const unsigned max_blocks = (unsigned)((m + LU_RPB - 1) / LU_RPB) + 1;
    if ((rc = hipMalloc(reinterpret_cast<void **>(&w->M), sizeof(double) * (size_t)(m * m))) != hipSuccess) return rc;
    if ((rc = hipMalloc(reinterpret_cast<void **>(&w->prow), sizeof(double) * (size_t)m)) != hipSuccess) return rc;
    if ((rc = hipMalloc(reinterpret_cast<void **>(&w->irow), sizeof(double) * (size_t)m)) != hipSuccess) return rc;
    if ((rc = hipMalloc(reinterpret_cast<void **>(&w->udiag), sizeof(double) * (size_t)m)) != hipSuccess) return rc;
    if ((rc = hipMalloc(reinterpret_cast<void **>(&w->piv), sizeof(int64_t) * (size_t)m)) != hipSuccess) return rc;
    if ((rc = hipMalloc(&w->cands, sizeof(LuCand) * (size_t)max_blocks)) != hipSuccess) return rc;
    if ((rc = hipMalloc(&w->st, sizeof(LuState))) != hipSuccess) return rc;
    return hipSuccess;
}
void ellp_lu_rows_free(EllpLuWork *w) {
    (void)hipFree(w->M); (void)hipFree(w->prow); (void)hipFree(w->irow); (void)hipFree(w->udiag); (void)hipFree(w->piv);
    (void)hipFree(w->cands); (void)hipFree(w->st);
    memset(w, 0, sizeof(*w));
}
void ellp_lu_rows_factor(EllpLuWork *w, hipStream_t stream) {
    const int64_t m = w->m;
    const unsigned strips = (unsigned)((m + LUP_W - 1) / LUP_W);
    for (int64_t j0 = 0; j0 < m; j0 += LUP_W) {
        const int64_t rows = m - j0;
        if (rows <= LUP_NT) hipLaunchKernelGGL(k_lup_panel_reg<1>, dim3(1), dim3(LUP_NT), 0, stream, w->M, m, j0, w->piv, w->udiag);
        else if (rows <= 2 * LUP_NT) hipLaunchKernelGGL(k_lup_panel_reg<2>, dim3(1), dim3(LUP_NT), 0, stream, w->M, m, j0, w->piv, w->udiag);
        else hipLaunchKernelGGL(k_lup_panel_mem, dim3(1), dim3(LUP_NT), 0, stream, w->M, m, j0, w->piv, w->udiag);
        if (strips > 1) hipLaunchKernelGGL(k_lup_update, dim3(strips), dim3(LUP_NT), 0, stream, w->M, m, j0, w->piv, w->udiag);
    }
}
void ellp_lu_rows_factor_unblocked(EllpLuWork *w, hipStream_t stream) {
    const int64_t m = w->m;
    (void)hipMemsetAsync(w->st, 0, sizeof(LuState), stream);
    for (int64_t i = -1; i < m; ++i) {
        const int64_t rows = m - i - 1;
        const unsigned grid = (unsigned)((rows + LU_RPB - 1) / LU_RPB) + 1;
        hipLaunchKernelGGL(k_lut_step, dim3(grid), dim3(256), 0, stream, w->M, m, m, i, w->prow, w->irow, static_cast<LuCand *>(w->cands),
                           static_cast<LuState *>(w->st));
        if (i + 1 < m)
            hipLaunchKernelGGL(k_lut_fold, dim3(1), dim3(1024), 0, stream, w->M, m, i + 1, static_cast<const LuCand *>(w->cands), grid, w->prow,
                               w->irow, static_cast<LuState *>(w->st), w->piv, w->udiag);
    }
}

static double g_lu_rows_last_ms = 0.0;
extern "C" double ellp_hip_lu_rows_last_ms(void) { return g_lu_rows_last_ms; }

extern "C" ellp_status ellp_hip_lu_rows(int64_t m, const double *M_in, int variant, double *factors_out, int64_t *pivot_out,
                                        double *udiag_out, int device, char *errbuf, size_t errlen) {
    if (errbuf && errlen) errbuf[0] = 0;
    if (m <= 0) {
        if (errbuf && errlen) snprintf(errbuf, errlen, "ellp_hip_lu_rows: m = %lld, a square matrix of at least one row is needed", (long long)m);
        return ELLP_ERR_ARG;
    }
    if (!M_in || !factors_out || !pivot_out || !udiag_out) {
        if (errbuf && errlen) snprintf(errbuf, errlen, "ellp_hip_lu_rows: NULL pointer (M_in, factors_out, pivot_out and udiag_out are all needed)");
        return ELLP_ERR_ARG;
    }
    if (variant != 0 && variant != 1) {
        if (errbuf && errlen) snprintf(errbuf, errlen, "ellp_hip_lu_rows: unknown variant %d (0 = unblocked, 1 = blocked)", variant);
        return ELLP_ERR_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        if (errbuf && errlen) snprintf(errbuf, errlen, "no HIP device available");
        return ELLP_ERR_DEVICE;
    }
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return ELLP_ERR_DEVICE;
    EllpLuWork w;
    memset(&w, 0, sizeof(w));
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipError_t rc = hipSuccess;
    auto cleanup = [&] {
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        ellp_lu_rows_free(&w);
    };
#define LCHK(expr)                                      \
    do {                                                \
        rc = (expr);                                    \
        if (rc != hipSuccess) {                         \
            set_err(errbuf, errlen, #expr, rc);         \
            cleanup();                                  \
            return ELLP_ERR_DEVICE;                     \
        }                                               \
    } while (0)
    const size_t bytes = sizeof(double) * (size_t)(m * m);
    LCHK(ellp_lu_rows_alloc(&w, m));
    LCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    LCHK(hipEventCreate(&ev0));
    LCHK(hipEventCreate(&ev1));
    LCHK(hipMemcpyAsync(w.M, M_in, bytes, hipMemcpyHostToDevice, stream));
    LCHK(hipEventRecord(ev0, stream));
    if (variant == 1) ellp_lu_rows_factor(&w, stream);
    else ellp_lu_rows_factor_unblocked(&w, stream);
    LCHK(hipEventRecord(ev1, stream));
    LCHK(hipGetLastError());
    LCHK(hipMemcpyAsync(factors_out, w.M, bytes, hipMemcpyDeviceToHost, stream));
    LCHK(hipMemcpyAsync(pivot_out, w.piv, sizeof(int64_t) * (size_t)m, hipMemcpyDeviceToHost, stream));
    LCHK(hipMemcpyAsync(udiag_out, w.udiag, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, stream));
    LCHK(hipStreamSynchronize(stream));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) g_lu_rows_last_ms = (double)ms;
#undef LCHK
    cleanup();
    return ELLP_OPTIMAL;
}

extern "C" ellp_status ellp_hip_lu_transposed(int64_t m, int64_t nv, const double *A, int64_t *pivot_out,
                                              double *udiag_out, int device, char *errbuf, size_t errlen) {
    if (errbuf && errlen) errbuf[0] = 0;
    if (m < 0 || nv < 0 || (m > 0 && nv > 0 && (!A || !pivot_out || !udiag_out))) return ELLP_ERR_ARG;
    if (nv < m) {
        if (errbuf && errlen) snprintf(errbuf, errlen, "ellp_hip_lu_transposed needs nv >= m (every column of A^T gets a pivot row)");
        return ELLP_ERR_ARG;
    }
    if (m == 0) return ELLP_OPTIMAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        if (errbuf && errlen) snprintf(errbuf, errlen, "no HIP device available");
        return ELLP_ERR_DEVICE;
    }
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return ELLP_ERR_DEVICE;
    double *dM = nullptr, *prow = nullptr, *irow = nullptr, *udiag = nullptr;
    int64_t *piv = nullptr;
    LuCand *cands = nullptr;
    LuState *st = nullptr;
    hipStream_t stream = nullptr;
    hipError_t rc = hipSuccess;
    auto cleanup = [&] {
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); }
        (void)hipFree(dM); (void)hipFree(prow); (void)hipFree(irow); (void)hipFree(udiag); (void)hipFree(piv); (void)hipFree(cands); (void)hipFree(st);
    };
#define LCHK(expr)                                      \
    do {                                                \
        rc = (expr);                                    \
        if (rc != hipSuccess) {                         \
            set_err(errbuf, errlen, #expr, rc);         \
            cleanup();                                  \
            return ELLP_ERR_DEVICE;                     \
        }                                               \
    } while (0)
    const unsigned max_blocks = (unsigned)((nv + LU_RPB - 1) / LU_RPB) + 1;
    LCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    LCHK(hipMalloc(reinterpret_cast<void **>(&dM), sizeof(double) * (size_t)(m * nv)));
    LCHK(hipMalloc(reinterpret_cast<void **>(&prow), sizeof(double) * (size_t)m));
    LCHK(hipMalloc(reinterpret_cast<void **>(&irow), sizeof(double) * (size_t)m));
    LCHK(hipMalloc(reinterpret_cast<void **>(&udiag), sizeof(double) * (size_t)m));
    LCHK(hipMalloc(reinterpret_cast<void **>(&piv), sizeof(int64_t) * (size_t)m));
    LCHK(hipMalloc(reinterpret_cast<void **>(&cands), sizeof(LuCand) * (size_t)max_blocks));
    LCHK(hipMalloc(reinterpret_cast<void **>(&st), sizeof(LuState)));
    LCHK(hipMemcpyAsync(dM, A, sizeof(double) * (size_t)(m * nv), hipMemcpyHostToDevice, stream));
    LCHK(hipMemsetAsync(st, 0, sizeof(LuState), stream));
    for (int64_t i = -1; i < m; ++i) {
        const int64_t rows = nv - i - 1;
        const unsigned grid = (unsigned)((rows + LU_RPB - 1) / LU_RPB) + 1;
        hipLaunchKernelGGL(k_lut_step, dim3(grid), dim3(256), 0, stream, dM, m, nv, i, prow, irow, cands, st);
        if (i + 1 < m)
            hipLaunchKernelGGL(k_lut_fold, dim3(1), dim3(1024), 0, stream, dM, m, i + 1, cands, grid, prow, irow, st, piv, udiag);
    }
    LCHK(hipGetLastError());
    LCHK(hipMemcpyAsync(pivot_out, piv, sizeof(int64_t) * (size_t)m, hipMemcpyDeviceToHost, stream));
    LCHK(hipMemcpyAsync(udiag_out, udiag, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, stream));
    LCHK(hipStreamSynchronize(stream));
#undef LCHK
    cleanup();
    return ELLP_OPTIMAL;
}

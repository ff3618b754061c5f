// ellp_gemm.inc — the two m x m x m f64 GEMMs of the Newton-Schulz refresh on the matrix cores
// (v_mfma_f64_16x16x4_f64; lane layout checked by tools/mfma_f64_check.hip and stated in
// /opt/skills/guides/cdna_hip_programming.md: A[i][k] in lane i + 16 k, B[k][j] in lane j + 16 k,
// D[i][j] with j = lane & 15, i = (lane >> 4) + 4 v for the four results v of a lane).
//
//   STEP 0:  E = I - A_B W[cur]      -> W[cur^1]     (A_B column-major, W row-major)
//   STEP 1:  T = W[cur] + W[cur] E   -> T            (everything row-major)
//
// One 512-thread workgroup (eight waves, two per SIMD, so that one wave's LDS reads and barrier waits are
// covered by the other's MFMAs) makes a 128 x 128 tile of the result; each wave owns a 64 x 32 piece =
// 4 x 2 MFMA tiles = 8 accumulators of 4 f64 per lane (64 AGPRs).  K advances
// 16 per stage: the 128 x 16 slab of A and the 16 x 128 slab of B go through LDS stored k-major with the
// tile dimension contiguous, so every fragment read is one ds_read_b64 whose 16-lane groups each cover
// 128 contiguous bytes (no bank conflict); the row-major A of STEP 1 is transposed on its way into LDS.
// Two LDS buffers and a register prefetch of the next stage's global loads: one barrier per stage, the
// loads of stage s+1 are in flight while the 32 MFMAs per wave of stage s issue.  Per stage and wave:
// 24 ds_read_b64 against 32 MFMAs — the matrix pipe, not LDS or the vector ALU, is what is busy.
//
// Included inside the anonymous namespace of ellp_engine.hip (uses GemmArgs, DevState, ST_RUNNING).

typedef double mfma_d4 __attribute__((ext_vector_type(4)));

template <int STEP>
__global__ __launch_bounds__(512) void k_gemm_mfma(GemmArgs a) {
    constexpr int BM = 128, BN = 128, BK = 16;
    __shared__ __align__(16) double sA[2][BK][BM];
    __shared__ __align__(16) double sB[2][BK][BN];
    if (a.st->status != ST_RUNNING) return;
    if (STEP == 1 && a.st->need_rebuild) return;  // k_resid_reduce: not a small perturbation any more
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 2, wc = wave & 3;  // the wave's 64 x 32 piece
    const int64_t m = a.m, ld = a.ld;
    const double *Wc = a.st->cur ? a.W1 : a.W0;
    double *Wo = a.st->cur ? a.W0 : a.W1;
    const double *A = STEP == 0 ? a.A_B : Wc;
    const double *B = STEP == 0 ? Wc : Wo;
    double *C = STEP == 0 ? Wo : a.T;
    const int64_t i0 = (int64_t)blockIdx.y * BM, j0 = (int64_t)blockIdx.x * BN;

    mfma_d4 acc[4][2];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[r][c] = mfma_d4{0.0, 0.0, 0.0, 0.0};

    // ---- global -> register staging of one stage: 4 doubles of A and 4 of B per thread
    // k-major operands (A of STEP 0, B always): thread t takes row k = t >> 5 of the slab and the 4
    // consecutive tile entries (t & 31) * 4 .. + 3.
    // row-major A (STEP 1): thread t takes tile row i = t & 127 and the 4 consecutive k = (t >> 7) * 4 .. + 3.
    // Loads are unconditional from clamped addresses and the zero fill of the ragged edges (m is not a multiple of
    // 128 or 16) is applied when the registers go to LDS, AFTER the stage's MFMAs: a select on a loaded value right
    // behind the load would make the compiler wait for the load (vmcnt(0)) before the MFMAs it is meant to overlap.
    double2 ra[2], rb[2];
    const int kq = tid >> 5, x8 = (tid & 31) * 4;
    const int ai = tid & 127, ak8 = (tid >> 7) * 4;
    const int64_t mlast = (m - 1) & ~(int64_t)1;  // the last even index: a double2 from there stays inside the row (ld is even)
    auto clampi = [&](int64_t v) { return v < mlast ? v : mlast; };
    auto load_stage = [&](int64_t k0) {
        if (STEP == 0) {
            const int64_t k = k0 + kq < m ? k0 + kq : m - 1;
#pragma unroll
            for (int p = 0; p < 2; ++p) ra[p] = *reinterpret_cast<const double2 *>(A + k * ld + clampi(i0 + x8 + 2 * p));
        } else {
            const int64_t i = i0 + ai < m ? i0 + ai : m - 1;
#pragma unroll
            for (int p = 0; p < 2; ++p) ra[p] = *reinterpret_cast<const double2 *>(A + i * ld + clampi(k0 + ak8 + 2 * p));
        }
        const int64_t k = k0 + kq < m ? k0 + kq : m - 1;
#pragma unroll
        for (int p = 0; p < 2; ++p) rb[p] = *reinterpret_cast<const double2 *>(B + k * ld + clampi(j0 + x8 + 2 * p));
    };
    auto masked = [&](double2 v, bool row_ok, int64_t x) {  // x: index of v.x along the contiguous dimension
        double2 o;
        o.x = (row_ok && x < m) ? v.x : 0.0;
        o.y = (row_ok && x + 1 < m) ? v.y : 0.0;
        return o;
    };
    auto store_stage = [&](int buf, int64_t k0) {
        if (STEP == 0) {
            const bool ok = k0 + kq < m;
#pragma unroll
            for (int p = 0; p < 2; ++p)
                *reinterpret_cast<double2 *>(&sA[buf][kq][x8 + 2 * p]) = masked(ra[p], ok, i0 + x8 + 2 * p);
        } else {
            const bool ok = i0 + ai < m;
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const double2 v = masked(ra[p], ok, k0 + ak8 + 2 * p);
                sA[buf][ak8 + 2 * p][ai] = v.x;
                sA[buf][ak8 + 2 * p + 1][ai] = v.y;
            }
        }
        const bool ok = k0 + kq < m;
#pragma unroll
        for (int p = 0; p < 2; ++p)
            *reinterpret_cast<double2 *>(&sB[buf][kq][x8 + 2 * p]) = masked(rb[p], ok, j0 + x8 + 2 * p);
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
        if (more) store_stage(buf ^ 1, k0 + BK);  // nobody reads buf^1 any more: its last readers passed the previous barrier
        __syncthreads();
        buf ^= 1;
    }

    // ---- epilogue
    double worst = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int64_t i = i0 + wr * 64 + r * 16 + fk + 4 * v;
                const int64_t j = j0 + wc * 32 + c * 16 + fr;
                if (i < m && j < m) {
                    double o;
                    if (STEP == 0) o = (i == j ? 1.0 : 0.0) - acc[r][c][v];
                    else o = Wc[i * ld + j] + acc[r][c][v];
                    C[i * ld + j] = o;
                    worst = nanmax(worst, fabs(o));
                }
            }
    if (STEP == 0) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) worst = nanmax(worst, __shfl_xor(worst, o));
        double *s_red = &sA[0][0][0];  // free: the last stage's readers are past the loop's final barrier
        if (lane == 0) s_red[wave] = worst;
        __syncthreads();
        if (tid == 0)
            a.tilemax[blockIdx.y * gridDim.x + blockIdx.x] = nanmax(nanmax(nanmax(s_red[0], s_red[1]), nanmax(s_red[2], s_red[3])), nanmax(nanmax(s_red[4], s_red[5]), nanmax(s_red[6], s_red[7])));
    }
}

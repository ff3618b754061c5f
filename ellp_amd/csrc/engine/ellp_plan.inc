// ellp_plan.inc — which engine an LP gets: everything ellp_engine_create decides from (kind, m, |N|, opts, environment)
// alone, in one pure function (no HIP call; plan_env() alone reads the environment).  ellp_engine derives from EnginePlan,
// so e->small, e->cpb, ... are the plan; redo_from_snapshot, set_shard, step, shard_columns and enqueue_exact_iteration change
// the engine's copy on purpose.  ellp_engine_plan (ellp_hip.h) shows the plan to tests without a device.  Included after
// ellp_mid.inc: the LDS sizes and workgroup sizes stay with the kernels whose layout they describe.

// what the rebuild of B^-1 and the BTRAN / resync partial sums derive from m alone; the batched dual start
// (ellp_dstart.inc) derives them here too, so each item's arithmetic is the single call's
struct RebuildGeometry {
    int bl_splits = 1, upd_rows = 4, btran_rows = 1, btran_tiles = 1;  // splits of the rebuild's first GEMM; rows per block (<= UPD_ROWS)
};
inline RebuildGeometry rebuild_geometry(int64_t m) {
    RebuildGeometry g;
    const int64_t nrb64 = (m + 63) / 64;
    const int sp = (int)((256 + nrb64 - 1) / nrb64);
    g.bl_splits = sp < 1 ? 1 : (sp > 8 ? 8 : sp);
    g.upd_rows = m >= 1024 ? 4 : (m >= 256 ? 2 : 1);
    g.btran_rows = (int)((m + 63) / 64);
    if (g.btran_rows < 8) g.btran_rows = 8;
    g.btran_tiles = (int)((m + g.btran_rows - 1) / g.btran_rows);
    return g;
}

struct EnginePlan : RebuildGeometry {
    // launch geometry
    int64_t ld = 0;
    int cpb = 1, nblocks = 1, priceT = 1;
    bool price_nt = false;
    bool price_wave = false;  // wave-per-column pricing (cache-resident A_N, rows long enough to fill a wave)
    int upd_blocks = 1;
    int upd2_rows = 4, upd2_blocks = 1;  // k_update2 (<= 2*UPD_ROWS)
    int ftran_blocks = 1;
    int upd_stage = 1;
    size_t upd_lds = 0, ftran_lds = 0, price2_lds = 0;
    int nbs = 1;        // pricing blocks of this rank's shard (world = 1: all of them)
    int64_t seg = 0;
    // maintenance
    int refactor_period = 0;
    double ill_tol = 0.0;  // reactive maintenance threshold (small LPs and steepest edge)
    int drift_every = 0;   // iterations between two drift checks of B^-1 (0: off)
    double drift_tol = 0.0;
    // mode
    int pp_P = 0;            // partial pricing: number of segments (<= 1: off)
    int64_t pp_S = 0;        // positions per segment
    bool se = false;         // ELLP_FLAG_PRIMAL_STEEPEST_EDGE (ellp_se.inc): three launches + one transposed GEMV per iteration
    bool want_se_vpart = false;  // ... v = B^-T d from k_update2's row blocks instead of that GEMV
    int dual_maxviol = 0;  // ELLP_FLAG_DUAL_MAX_VIOLATION
    int dual_bflip = 0;    // ELLP_FLAG_DUAL_BOUND_FLIPPING: the long-step ratio test (LU-per-iteration kernels only)
    bool small = false;    // run() uses k_small or, with `mid`, k_mid: no explicit inverse is kept
    bool mid = false;      // 128 < m <= 1024: that loop with its factors in global memory (ellp_mid.inc)
    size_t small_lds = 0, mid_lds = 0;
    int small_nt = SMALL_THREADS;  // workgroup size of k_small for this LP (small_threads)
    int mid_nt = 0;
    int64_t ldn = 0;
    bool hybrid = false;      // certified hybrid (DESIGN.md §3.1c): explicit inverse with a pivot guard, k_mid certifies
    bool cert_large = false;  // above 1,024 rows (ellp_exact.inc): terminal statuses certified by an exact-LU iteration
    double guard_abs = 0.0;
    int exact_K = 8;
    bool exact_large_always = false;  // pipeline 3 above 1,024 rows: the LU-per-iteration loop over all CUs, for good
    bool lagged = false;      // two launches per primal iteration (ellp_lagged.inc)
    bool dual_fused = false;  // dual: FTRAN and eta update in one pass over B^-1 (ellp_dualfu.inc)
    bool dual_fold = false;   // ... and its closing work done by the next pricing launch (no tiny-pivot maintenance)
    bool want_unit_table = false;  // the unit-column table (PriceArgs::vs_row) is made at creation
    bool want_stamps = false;      // ELLP_SMALL_STAMPS: per-phase tick sums of k_small
};

// what creation reads from the environment, each with the parsing it has always had
struct PlanEnv {
    int64_t mid_auto_max = SMALL_MAX_M;  // ELLP_MID_AUTO_MAX, set (even empty): up to how many rows the exact loop alone is the default
    std::optional<double> ill_tol, drift_tol, guard_abs;  // ELLP_ILL_TOL (set), ELLP_DRIFT_TOL, ELLP_GUARD_ABS (not empty): diagnostics
    std::optional<int> drift_every;                       // ELLP_DRIFT_EVERY (not empty): diagnostics
    int small_nt = 0;      // ELLP_SMALL_NT: measurement, a workgroup size that still has a thread per row
    int exact_K = 0;       // ELLP_EXACT_K (> 0): diagnostics
    bool no_unit_columns = false, small_stamps = false, no_hybrid = false, dual_fold_off = false, se_btran = false;  // set at all
};

inline PlanEnv plan_env() {
    PlanEnv v;
    if (const char *s = getenv("ELLP_MID_AUTO_MAX")) v.mid_auto_max = atoll(s);
    if (const char *s = getenv("ELLP_ILL_TOL")) v.ill_tol = atof(s);
    if (const char *s = getenv("ELLP_DRIFT_EVERY"); s && s[0]) v.drift_every = atoi(s);
    if (const char *s = getenv("ELLP_DRIFT_TOL"); s && s[0]) v.drift_tol = atof(s);
    if (const char *s = getenv("ELLP_GUARD_ABS"); s && s[0]) v.guard_abs = atof(s);
    if (const char *s = getenv("ELLP_SMALL_NT")) v.small_nt = atoi(s);
    if (const char *s = getenv("ELLP_EXACT_K"); s && s[0] && atoi(s) > 0) v.exact_K = atoi(s);
    v.no_unit_columns = getenv("ELLP_NO_UNIT_COLUMNS") != nullptr;
    v.small_stamps = getenv("ELLP_SMALL_STAMPS") != nullptr;
    v.no_hybrid = getenv("ELLP_NO_HYBRID") != nullptr;
    v.dual_fold_off = getenv("ELLP_DUAL_FOLD_OFF") != nullptr;
    v.se_btran = getenv("ELLP_SE_BTRAN") != nullptr;
    return v;
}

// plan_engine's `avail`, what creation may fail to obtain: the LDS attribute of the chosen k_small; k_mid's attribute, LUa, Ut, A_Nt
enum { PLAN_AVAIL_SMALL = 1, PLAN_AVAIL_MID = 2, PLAN_AVAIL_ALL = 3 };
constexpr int64_t PLAN_MAX_M = 8192;  // the widest pricing tile (16 double2 per thread and row), the blocked rebuild

// Default maintenance period, from a cost model: a refresh costs T_r ~ 2*(2 m^3)/25 TFLOP/s + 60 us
// (two GEMM launches, a residual read-back with a host sync), an iteration T_i ~ (8 ld |N| + 24 m ld)
// / 5 TB/s + 15 us, and the period is the smallest one whose refreshes stay within a BUDGET of the
// loop time: 30 % up to m = 1024, falling linearly to 3 % at m = 2000 and beyond (config 3: 1000
// iterations, as measured), never below 16.  Why so generous on small and mid-size LPs: the reference
// factorises afresh every iteration, and the error of B^-1 a_q is cond(A_B) times that of B^-1 — a
// tall 500 x 100 LP of the benign synthetic family left the oracle's path after 166 pivots with B^-1
// untouched and after 162 with a period of 62 (x off by 2e-9 against EPS = 1e-10; the error grew
// 25-fold within 9 pivots at cond 6e4), and stays on it for 1200 pivots with a period of 16.  Beyond
// the model, the drift monitor (k_drift_part) asks for a refresh when the LP needs one (DESIGN.md §5).
inline int64_t default_period(int64_t m_, int64_t ld_, int64_t nN_) {
    const double m = (double)m_, ld = (double)ld_, nN = (double)(nN_ > 0 ? nN_ : 1);
    const double t_refresh = 4.0 * m * m * m / 25e12 + 60e-6;
    const double t_iter = (8.0 * ld * nN + 24.0 * m * ld) / 5e12 + 15e-6;
    double budget = 0.30;
    if (m > 1024.0) budget = m >= 2000.0 ? 0.03 : 0.30 - 0.27 * (m - 1024.0) / 976.0;
    int64_t p = (int64_t)std::ceil(t_refresh / (budget * t_iter));
    if (p < 16) p = 16;
    if (p > 1000) p = 1000;
    return p;
}

// Which LU-per-iteration loop a single call runs for the whole solve: EXACT_SMALL (k_small), EXACT_MID (k_mid) or
// EXACT_NONE (the explicit-inverse engine, alone or as the certified hybrid).  The exact loop ALONE is the default up to
// m <= 128 (k_small, factors in LDS, 1-5 x slower per iteration than the explicit-inverse engine).  Above that the default
// is the certified hybrid; pipeline = 3, the dual's bound flipping or ELLP_MID_AUTO_MAX (`mid_auto`) still select k_mid for
// whole solves up to 1024 rows (15-40 x slower).  plan_engine and the two batch entries ask this alone.
enum ExactLoop { EXACT_NONE = 0, EXACT_SMALL = 1, EXACT_MID = 2 };
inline ExactLoop exact_loop(const ellp_opts &o, bool dual_bflip, bool se, int pp_P, int64_t m, size_t small_lds, size_t mid_lds,
                            int64_t mid_auto) {
    const int pl = o.pipeline;
    const bool fits = small_lds > 0 || mid_lds > 0;
    const bool wanted = pp_P <= 1 && !se && (pl == 3 || dual_bflip || (pl == 0 && o.refactor_period <= 0 && o.btran_mode == 0 &&
                                                                          o.profile == 0 && (m <= SMALL_MAX_M || m <= mid_auto)));
    if (!wanted || !fits) return EXACT_NONE;
    return small_lds > 0 ? EXACT_SMALL : EXACT_MID;
}

// refusal 3 (the batched dual start answers it for a whole batch, with partial_segments as pp_P)
inline bool refuse_bflip_pipeline(const ellp_opts &o, bool dual_bflip, int pp_P, char *errbuf, size_t errlen) {
    if (!dual_bflip || !(o.pipeline == 1 || o.pipeline == 2 || pp_P > 1)) return false;
    set_err(errbuf, errlen, "ELLP_FLAG_DUAL_BOUND_FLIPPING runs on the LU-per-iteration kernels (pipeline 0 or 3, up to 1,024 rows), "
                            "not on the explicit-inverse pipelines 1 / 2");
    return true;
}

// The plan of an engine of `kind` for m rows and n_N nonbasic columns (m >= 1, n_N >= 0), every decision once and in the
// order of its dependencies (DESIGN.md §3.0).  `avail`: PLAN_AVAIL_* bits of the resources creation can obtain — it plans
// with all, acquires what the plan asks for, and plans again without the one that failed.  Returns ELLP_OPTIMAL, or a
// refusal with its text: ELLP_ERR_ARG in the order (1) pricing tile, (3) bound flipping with pipeline 1 / 2, (4) steepest
// edge with partial pricing / pipeline 2, 3 / btran_mode 1, (5) bound flipping above 1,024 rows — creation puts (2), the
// dual's initial feasibility, behind (1) — and ELLP_ERR_DEVICE where a loop the caller insisted on has lost k_mid.
inline ellp_status plan_engine(int kind, int64_t m, int64_t n_N, const ellp_opts &o, const PlanEnv &env, int avail, EnginePlan *out,
                               char *errbuf, size_t errlen) {
    EnginePlan p;
    const bool primal = kind == ELLP_ENGINE_PRIMAL, dual = kind == ELLP_ENGINE_DUAL;
    const int pl = o.pipeline;
    const int64_t nNa = n_N > 0 ? n_N : 1;
    const int64_t ld = p.ld = round_up(m, 16);

    // ---- the sizes alone: launch geometry
    if (m > PLAN_MAX_M) {
        set_err(errbuf, errlen, "m = %lld exceeds this build's pricing tile (m <= 8192)", (long long)m);
        return ELLP_ERR_ARG;
    }
    // A_N far beyond the Infinity Cache -> stream it with nt loads from ~2048 blocks; otherwise
    // ~1024 blocks (the entering fold stages one maximum per block).  tools/price_bench.hip
    p.price_nt = 8.0 * (double)ld * (double)nNa > 160e6;
    int64_t cpb = p.price_nt ? (n_N + 2047) / 2048 : (n_N + 1023) / 1024;
    cpb = cpb < 1 ? 1 : (cpb > 64 ? 64 : cpb);
    p.cpb = (int)cpb;
    p.nblocks = (int)((nNa + cpb - 1) / cpb);
    p.nbs = p.nblocks;
    p.seg = 2 * (int64_t)p.nbs + 2 * (int64_t)p.nbs * p.cpb;
    const int64_t need = ((ld >> 1) + 255) / 256;  // double2 per thread for one row: <= 16 by the refusal above
    p.priceT = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : need <= 8 ? 8 : 16;
    static_cast<RebuildGeometry &>(p) = rebuild_geometry(m);
    p.upd_blocks = (int)((m + p.upd_rows - 1) / p.upd_rows);
    const int64_t fw = m < 2048 ? m : 2048;
    p.ftran_blocks = (int)((fw + 3) / 4);
    const int nchunks = (int)((m + 63) >> 6);
    const size_t staged = sizeof(double) * (size_t)nchunks + (size_t)m * (8 + 4 + 1) + 16;
    p.upd_stage = staged <= 40 * 1024 ? 1 : 0;  // keep >= 4 update blocks per CU resident
    p.upd_lds = p.upd_stage ? staged : sizeof(double) * (size_t)nchunks + 16;
    p.ftran_lds = sizeof(double) * (size_t)p.nblocks + 16;
    p.price2_lds = sizeof(double) * (size_t)nchunks + 16;

    // ---- the options: pricing rules, and what they refuse
    if (primal && o.partial_segments > 1 && n_N > 0) {
        // partial pricing (f4): segments of ceil(|N| / P) positions, never more segments than positions
        int P = o.partial_segments;
        if ((int64_t)P > n_N) P = (int)n_N;
        const int64_t S = (n_N + P - 1) / P;
        P = (int)((n_N + S - 1) / S);
        if (P > 1) {
            p.pp_P = P;
            p.pp_S = S;
        }
    }
    p.dual_maxviol = (dual && (o.flags & ELLP_FLAG_DUAL_MAX_VIOLATION)) ? 1 : 0;
    p.dual_bflip = (dual && (o.flags & ELLP_FLAG_DUAL_BOUND_FLIPPING)) ? 1 : 0;
    if (refuse_bflip_pipeline(o, p.dual_bflip, p.pp_P, errbuf, errlen)) return ELLP_ERR_ARG;
    const bool se_asked = primal && (o.flags & ELLP_FLAG_PRIMAL_STEEPEST_EDGE);
    if (se_asked && (p.pp_P > 1 || pl == 2 || pl == 3 || o.btran_mode == 1)) {
        // the caller must be able to tell which rule ran: steepest edge exists on the three-launch explicit-inverse engine only
        set_err(errbuf, errlen, "ELLP_FLAG_PRIMAL_STEEPEST_EDGE runs on the three-launch pipeline (pipeline 0 or 1) with full "
                                "pricing and the incremental BTRAN: not with partial_segments > 1, pipeline 2 / 3 or btran_mode 1");
        return ELLP_ERR_ARG;
    }
    p.se = se_asked && n_N > 0;
    // unit columns of the matrix (slacks, artificials, any other column with a single nonzero): the table the pricing kernels
    // of both loops consult; steepest edge needs it for its permutation test.  ELLP_FLAG_DENSE_PRICING or ELLP_NO_UNIT_COLUMNS: off
    p.want_unit_table = n_N > 0 && (p.se || (!(o.flags & ELLP_FLAG_DENSE_PRICING) && !env.no_unit_columns));
    // v = B^-T d accumulated by k_update2's row blocks (their rows of the old inverse are in registers there) where every
    // row of a block goes through the register path: <= UPD_ROWS rows per block and NR > 0 (ld <= 4096); otherwise the GEMV
    p.want_se_vpart = p.se && ld <= 4096 && !env.se_btran;
    // k_update2: 8 rows per block once m is large — half as many blocks re-stage the fold inputs (13 m bytes each) and
    // re-read the pivot row; measured -9 us of 58 at m=4000, +0.4 us at m=2000 (upd_rows is UPD_ROWS from 1,024 rows)
    p.upd2_rows = (m >= 3072 && !p.want_se_vpart) ? 8 : p.upd_rows;
    p.upd2_blocks = (int)((m + p.upd2_rows - 1) / p.upd2_rows);

    // ---- maintenance
    p.refactor_period = o.refactor_period > 0 ? o.refactor_period : 0;
    // reactive maintenance after a tiny pivot (|alpha_r| < ill_tol * max|alpha|): small LPs, and steepest edge at any
    // size — its longer steps meet such pivots often enough that at config 5 a variable once left the basis 0.03
    // off its bound between two looks of the drift monitor (DESIGN.md §5); costs the look-ahead of the run loop
    p.ill_tol = env.ill_tol.value_or((m <= 512 || se_asked) ? 1e-3 : 0.0);
    // drift monitor: only where refreshes are rare (period > 64), four checks per period; one GEMV
    // over A_B + a one-block fold, ~70 us at config 3 (0.7 % of the loop)
    const int64_t period = p.refactor_period > 0 ? p.refactor_period : default_period(m, ld, n_N);
    p.drift_every = env.drift_every.value_or(period > 64 ? (int)(period / 4 > 64 ? period / 4 : 64) : 0);
    p.drift_tol = env.drift_tol.value_or(1e-10);  // a backstop: config 3 drifts to 1.4e-11 in 3000 updates without any refresh

    // ---- the loop.  Small LPs: the reference's own loop in one persistent workgroup (ellp_small.inc, ellp_mid.inc) unless
    // the caller asked for the explicit-inverse engine (a maintenance period, a launch structure, profiling)
    p.small_lds = small_lds_bytes(m, n_N);
    p.mid_lds = mid_lds_bytes(m, n_N);
    const ExactLoop loop = exact_loop(o, p.dual_bflip, p.se, p.pp_P, m, p.small_lds, p.mid_lds, env.mid_auto_max);
    p.want_stamps = loop != EXACT_NONE && env.small_stamps;
    const bool mid_lost = loop == EXACT_MID && !(avail & PLAN_AVAIL_MID);
    if (mid_lost && (pl == 3 || p.dual_bflip)) {
        set_err(errbuf, errlen, "pipeline 3: no device memory for the factors of the persistent-workgroup loop");
        return ELLP_ERR_DEVICE;
    }
    p.mid = loop == EXACT_MID && !mid_lost;
    p.small = p.mid || (loop == EXACT_SMALL && (avail & PLAN_AVAIL_SMALL));
    if (p.small && !p.mid) {
        p.small_nt = small_threads(m, n_N);
        if ((env.small_nt == 64 || env.small_nt == 128 || env.small_nt == 256) && env.small_nt >= m) p.small_nt = env.small_nt;
    }
    // the long-step ratio test exists in k_small / k_mid only (a selection walk and one more solve with the iteration's LU)
    if (p.dual_bflip && !p.small && n_N > 0) {
        set_err(errbuf, errlen, "ELLP_FLAG_DUAL_BOUND_FLIPPING: the LU-per-iteration kernels take up to 1,024 rows (this LP: %lld)", (long long)m);
        return ELLP_ERR_ARG;
    }
    // Certificates of the explicit-inverse loop, the default with pipeline 0.  Up to 1,024 rows the certified hybrid
    // (DESIGN.md §3.1c; restated in oracle/ellp_oracle.c: hybrid_run): the three-launch pipeline (its ratio-test fold sits
    // in front of every store of the iteration, so a guarded pivot can be refused by all blocks alike) with the pivot guard
    // on; every terminal status and every guarded iteration is re-examined by k_mid from the same arrays (exact_takeover).
    // Above (the persistent kernel's limit): terminal statuses certified by an exact-LU iteration (ellp_exact.inc).  Off
    // with an explicit pipeline, ELLP_FLAG_NO_CERTIFY, partial pricing, steepest edge, btran_mode 1 and on sharded engines.
    const bool certify = !p.small && pl == 0 && !(o.flags & ELLP_FLAG_NO_CERTIFY) && n_N > 0 && p.pp_P <= 1 && !p.se && o.btran_mode == 0 &&
                         !env.no_hybrid;
    p.hybrid = certify && p.mid_lds > 0 && (avail & PLAN_AVAIL_MID);  // without k_mid: the plain explicit-inverse engine
    p.cert_large = certify && m > MID_MAX_M;
    if (p.mid || p.hybrid) {
        p.mid_nt = mid_threads(m);
        p.ldn = (n_N + 15) / 16 * 16;
    }
    if (p.hybrid || p.cert_large) {
        p.guard_abs = env.guard_abs.value_or(1e-7);
        if (env.exact_K > 0) p.exact_K = env.exact_K;
    }
    // pipeline 3 above 1,024 rows, under the condition exact_loop() sets below them: the LU-per-iteration loop over all CUs
    // (run_exact_large) is the engine — no hybrid, certificate, guard or snapshot: the loop is its own certificate.  The
    // explicit inverse is built, updated along and rebuilt at the end of a solve, so the phase hand-offs and read_point work.
    p.exact_large_always = !p.small && pl == 3 && m > MID_MAX_M && n_N > 0 && p.pp_P <= 1 && !p.se;
    // two launches per iteration from m = 384 (ellp_lagged.inc, ellp_dualfu.inc; tools/pipeline_threshold.py for the size), or
    // on request; partial pricing and steepest edge run on the three-launch pipeline
    const bool two_launch = !p.small && !p.hybrid && n_N > 0 && (pl == 2 || (pl == 0 && m >= 384));
    p.lagged = two_launch && primal && !p.se && o.btran_mode == 0 && p.pp_P <= 1;
    p.dual_fused = two_launch && dual && ld <= 4096;
    p.dual_fold = p.dual_fused && p.ill_tol <= 0.0 && !env.dual_fold_off;
    // wave-per-column pricing: cache-resident A_N, rows that fill a wave, and >= 5 columns per
    // block so that all four waves of a block have a column pair (measured at C3/C4: 18.9 -> 18.0
    // and 15.8 -> 14.3 us; the number of columns per block between 5 and 16 makes no difference);
    // k_price2_wave of the two-launch pipeline keeps u in 8 double2 per thread
    p.price_wave = !p.price_nt && ld >= 512 && cpb >= 5 && !(p.lagged && ld > 4096);
    *out = p;
    return ELLP_OPTIMAL;
}

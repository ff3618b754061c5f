/*
 * ellp_hip.h — C ABI of the MI355X-native revised-simplex pivot engine.
 *
 * Drop-in boundary for kehlert/ellp 0.2.0's hot path.  The reference has no FFI; the seam
 * this ABI replaces is the generic method
 *
 *   PrimalSimplexSolver::solve_with_initial   src/solvers/primal/primal_simplex_solver.rs:95
 *   DualSimplexSolver::solve_with_initial     src/solvers/dual/dual_simplex_solver.rs:110
 *
 * i.e. everything between `prob.unpack()` and the returned SolutionStatus: the per-iteration
 * BTRAN, pricing, entering selection, FTRAN, ratio test, point update and basis swap
 * (primal…:160-235 + pivot() :238-435; dual…:188-334).  Problem / StandardForm / phase
 * construction / the m == 0 trivial solver stay on the host (INTEGRATION.md shows the Rust
 * binding a maintainer would add).
 *
 * Conventions (mirroring what solve_with_initial has in hand, standard_form.rs:21-34):
 *   - A is m x n, column-major, leading dimension m (nalgebra DMatrix storage), read-only.
 *   - c, x, bound_kind/lb/ub have length n_c >= n (n_c > n only in primal phase 1 with free
 *     variables, primal_problem.rs:141,223,250-253).  b has length m.
 *   - Bound (problem.rs:191-197) is flattened to kind + lb + ub:
 *       0 Free, 1 Lower(lb), 2 Upper(ub), 3 TwoSided(lb, ub), 4 Fixed(lb)
 *   - Point{x, N, B} (standard_form.rs:21-25) is flattened to x, B_index[n_B],
 *     N_index[n_N], N_bound[n_N] (0 Lower, 1 Upper, 2 Free; standard_form.rs:206-210) and is
 *     updated IN PLACE, so the warm-start contract (phase 1 -> phase 2) survives.
 *   - No unwinding across the boundary: Err(EllPError) and panics of the reference come back
 *     as negative status codes with a message in errbuf.
 *   - Re-entrant: no global mutable state; every call/engine owns its HIP stream.
 *   - There is NO CPU fallback: if no HIP device is usable the call returns ELLP_ERR_DEVICE.
 */
#ifndef ELLP_HIP_H
#define ELLP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ELLP_HIP_ABI_VERSION 1

/* SolutionStatus (src/solver.rs:28-33) + error codes */
typedef enum ellp_status {
    ELLP_OPTIMAL = 0,
    ELLP_INFEASIBLE = 1,
    ELLP_UNBOUNDED = 2,
    ELLP_MAXITER = 3,
    ELLP_ERR_BAD_DIMS = -1, /* Err("invalid B/N, has .. elements but .. expected") primal…:124-140 */
    ELLP_ERR_SINGULAR = -2, /* Err("invalid B, A_B is not invertible")              primal…:175-179 */
    ELLP_ERR_NAN = -3,      /* NaN met in pricing / ratio keys                      primal…:282    */
    ELLP_ERR_DEVICE = -4,   /* HIP runtime error / no device / extension missing                   */
    ELLP_ERR_ARG = -5,      /* NULL pointer, index out of range, m == 0 (host handles that case)   */
    ELLP_ERR_PANIC = -6     /* an assert!/panic!/unwrap() of the reference would have fired        */
} ellp_status;

enum { ELLP_BOUND_FREE = 0, ELLP_BOUND_LOWER = 1, ELLP_BOUND_UPPER = 2, ELLP_BOUND_TWOSIDED = 3,
       ELLP_BOUND_FIXED = 4 };
enum { ELLP_NB_LOWER = 0, ELLP_NB_UPPER = 1, ELLP_NB_FREE = 2 };

#define ELLP_MAX_ITER_NONE UINT64_MAX /* PrimalSimplexSolver::new(None), primal…:26-30 */
#define ELLP_FLAG_DENSE_PRICING 1      /* ellp_opts.flags */
#define ELLP_FLAG_DUAL_MAX_VIOLATION 2 /* ellp_opts.flags */
#define ELLP_FLAG_PRIMAL_STEEPEST_EDGE 4 /* ellp_opts.flags */
#define ELLP_FLAG_NO_CERTIFY 8 /* ellp_opts.flags: the plain explicit-inverse engine where the default is the certified hybrid */
#define ELLP_FLAG_DUAL_BOUND_FLIPPING 16 /* ellp_opts.flags */

typedef struct ellp_opts {
    uint64_t max_iter;       /* self.max_iter (primal…:16, dual…:17); default 1000 (:21) */
    double eps;              /* EPS, src/util.rs:1; <= 0 selects 1e-10 */
    int32_t device;          /* HIP device ordinal; < 0 = current device */
    int32_t refactor_period; /* iterations between refactorisations of B^-1; <= 0 = default */
    int32_t btran_mode;      /* 0 default (incremental u, periodic refresh); 1 = u = B^-T c_B every iteration */
    int32_t poll_interval;   /* iterations enqueued between host polls of the status word; <= 0 = default */
    int32_t profile;         /* != 0: bracket every launch with HIP events (ellp_stats.kernel_ms) */
    int32_t use_graph;       /* reserved, must be 0 (hipGraph replay of the launch sequence is not implemented:
                                on gfx950 the per-iteration cost is GPU-side dispatch, not host launches) */
    int32_t pipeline;        /* launch structure of an iteration: 0 = engine default by size — m <= 128: 3; 128 < m <= 1024: the
                                CERTIFIED HYBRID: 1 with a pivot guard, every terminal status and every guarded iteration
                                re-examined by the LU-per-iteration kernel of 3 from the same arrays (DESIGN.md §3.1c;
                                ELLP_FLAG_NO_CERTIFY: plain 1 / 2 by size); m > 1024: 2 with the same guard in its kernels'
                                prologues, refused iterations and terminal statuses run on a fresh LU of the basis (§3.1d) —,
                                1 = three launches (pricing | FTRAN | eta update), 2 = two bandwidth
                                passes (primal: pricing | eta update of the previous pivot fused with this iteration's
                                FTRAN; dual: pricing | FTRAN fused with this iteration's eta update, + a closing block),
                                3 = the reference's loop with an LU of the basis per iteration, the oracle's pivots: up to 1,024
                                rows the whole loop in one persistent workgroup (factors in LDS up to 128 rows, in global
                                memory above; bit for bit the oracle); from 1,025 to 8,192 rows, with full pricing
                                (partial_segments <= 1), every loop body over all CUs — a blocked LU of the basis, the
                                triangular solves, the bandwidth kernels fed the exact vectors (the oracle's
                                status, iteration count and basis, values to 1e-11) — with no hybrid, certificate or redo: the
                                loop is its own certificate.  Such an engine keeps a resident inverse for the phase hand-offs
                                and refuses ellp_engine_step and sharding (ELLP_ERR_ARG) */
    int32_t trace_len;       /* > 0: keep the objective after each of the last `trace_len` iterations in a ring buffer on
                                the device (ellp_engine_read_trace) — what the reference's `debug!("{iter} | {obj}")` line
                                (primal…:161, dual…:189) prints; off by default, as the reference's logging is */
    int32_t partial_segments; /* > 1: partial pricing (an extension the reference's README lists as future work, not its
                                 behaviour): the nonbasic positions are cut into this many segments of
                                 ceil(|N| / segments) positions; an iteration prices one segment with the reference's
                                 entering rule; a pass that finds no candidate moves to the next segment (and counts
                                 as an iteration), `segments` such passes in a row are the optimality test.  Primal
                                 engines on one GPU, three-launch pipeline.  0 or 1: every column every iteration */
    int32_t flags;           /* bit 0 (ELLP_FLAG_DENSE_PRICING): stream every nonbasic column in the primal pricing pass,
                                also the unit columns (slacks, artificials), whose dot product the kernels otherwise
                                form from their single entry — same numbers, measured both ways by bench.py
                                bit 1 (ELLP_FLAG_DUAL_MAX_VIOLATION), an EXTENSION, dual engines: the leaving
                                row is the basic position with the LARGEST bound violation (first of equals) instead of the
                                first violated one (dual_simplex_solver.rs:200-236).  Not the reference's rule — restated in
                                the oracle (eo_set_dual_rule(2)) and checked against it; 24 x fewer iterations on the 200 x 500
                                LP of SURVEY.md §8d, and what makes a dual solve at config 4's size finish at all
                                bit 2 (ELLP_FLAG_PRIMAL_STEEPEST_EDGE), an EXTENSION, primal engines: steepest-edge pricing
                                (exact Goldfarb-Reid weights, ellp_se.inc) instead of the reference's Dantzig rule
                                (primal_simplex_solver.rs:253-287); restated in the oracle (eo_set_primal_rule(1)); runs on the
                                three-launch explicit-inverse engine at every size, with the reactive tiny-pivot maintenance
                                on.  Meant for RESIDENT solves (both phases on one engine, ellp_engine_rephase): a second
                                engine created with this flag at phase 1's end basis broke down at config 5's size (4000 x
                                40000) — the ratio test has no pivot-size safeguard, as the reference's has none
                                bit 3 (ELLP_FLAG_NO_CERTIFY): with pipeline 0, the plain explicit-inverse engine above 128 rows — no
                                pivot guard, no certificate behind a terminal status, no repeated solve (measurements, and the
                                replay side of a sharded run's self-check: sharded engines run without them)
                                bit 4 (ELLP_FLAG_DUAL_BOUND_FLIPPING), an EXTENSION (ellp's README.md:114-116),
                                dual engines: the long-step ("bound flipping") ratio test — the dual step goes past the
                                breakpoints of BOXED nonbasic variables, each moved to its other bound instead of entering, for as
                                long as the leaving row's infeasibility |delta| minus the sum of |alpha_j| (ub_j - lb_j) over the
                                passed breakpoints stays positive; breakpoints in (ratio, position) order; x_B follows the flips
                                by one more solve with the iteration's LU.  Restated in the oracle first (eo_set_dual_rule bit
                                0) and reproduced bit for bit.  Runs on the LU-per-iteration kernels only (pipeline 0 or 3, up
                                to 1,024 rows; with this flag pipeline 0 selects them at every such size): more rows, pipeline
                                1 / 2, partial pricing, or a call that needs the explicit-inverse engine (ellp_engine_step,
                                ellp_engine_refactor, sharding) return ELLP_ERR_ARG.  Combines with bit 1.  Ignored by primal
                                engines. */
} ellp_opts;

/* kernel ids for ellp_stats.kernel_ms / kernel_calls */
enum {
    ELLP_K_PRICE = 0,   /* r = c_N - A_N^T u (+ keys)          primal…:189, :253-270 */
    ELLP_K_SELECT = 1,  /* entering fold                        primal…:271-287       */
    ELLP_K_FTRAN = 2,   /* d = +-B^-1 a_q                       primal…:295-300, dual…:294 */
    ELLP_K_RATIO = 3,   /* ratio test + x update + swap         primal…:305-417, :205-232 */
    ELLP_K_UPDATE = 4,  /* rank-1 (eta) update of B^-1          (replaces primal…:173 / dual…:241) */
    ELLP_K_BTRAN = 5,   /* u = B^-T c_B                         primal…:184-187 */
    ELLP_K_REFACTOR = 6,/* B^-1 from A_B (all launches of one refactorisation) */
    ELLP_K_DLEAVE = 7,  /* dual leaving scan + rho               dual…:200-253 */
    ELLP_K_DPRICE = 8,  /* alpha = A_N^T rho (+ ratios)          dual…:255-278 */
    ELLP_K_DSELECT = 9, /* dual ratio argmin                     dual…:279-289 */
    ELLP_K_DUPDATE = 10,/* d, y, x updates + swap                dual…:296-333 */
    ELLP_K_EVENT_COST = 11, /* not a kernel: kernel_ms[11] = the event-bracket cost subtracted per launch */
    ELLP_K_COUNT = 12
};

typedef struct ellp_stats {
    uint64_t iters;       /* loop bodies entered (the reference's `iter` bookkeeping) */
    uint64_t pivots;      /* basis changes */
    uint64_t bound_flips; /* entering variable moved bound-to-bound (primal…:223-231) */
    uint64_t refactors;
    double obj;           /* c.x (primal) / dual objective (dual) at return */
    double t_loop_s;      /* wall time of the device loop */
    double t_setup_s;     /* upload + initial factorisation */
    double kernel_ms[ELLP_K_COUNT];      /* profile != 0 only: summed HIP-event time */
    uint64_t kernel_calls[ELLP_K_COUNT]; /* profile != 0 only */
} ellp_stats;

/* Fills *o with the defaults that reproduce reference behaviour (max_iter 1000, eps 1e-10). */
void ellp_default_opts(ellp_opts *o);

/* Number of usable HIP devices (0 if none / runtime unavailable). Never throws. */
int ellp_hip_device_count(void);
int ellp_hip_abi_version(void);

/*
 * PrimalSimplexSolver::solve_with_initial (primal_simplex_solver.rs:95-236).
 * Synchronous: uploads, runs the device loop, writes x / B_index / N_index / N_bound back.
 */
ellp_status ellp_primal_solve_with_initial(
    int64_t m, int64_t n, int64_t n_c,
    const double *A, const double *c, const double *b,
    const uint8_t *bound_kind, const double *lb, const double *ub,
    double *x,
    int64_t *B_index, int64_t n_B,
    int64_t *N_index, uint8_t *N_bound, int64_t n_N,
    const ellp_opts *opts, ellp_stats *stats, char *errbuf, size_t errbuf_len);

/*
 * DualSimplexSolver::solve_with_initial (dual_simplex_solver.rs:110-335).
 * y (m) and d (n_c) are the DualFeasiblePoint's vectors (dual_problem.rs:12-16), in/out.
 */
ellp_status ellp_dual_solve_with_initial(
    int64_t m, int64_t n, int64_t n_c,
    const double *A, const double *c, const double *b,
    const uint8_t *bound_kind, const double *lb, const double *ub,
    double *x,
    int64_t *B_index, int64_t n_B,
    int64_t *N_index, uint8_t *N_bound, int64_t n_N,
    double *y, double *d,
    const ellp_opts *opts, ellp_stats *stats, char *errbuf, size_t errbuf_len);

/*
 * Batched solve_with_initial of many LPs of up to 1,024 rows (kind: ELLP_ENGINE_PRIMAL or ELLP_ENGINE_DUAL), one workgroup
 * per LP, in launches of the LU-per-iteration kernels: ellp_small.inc's up to 128 rows, ellp_mid.inc's for 129 - 1,024 rows
 * where the single call with the same opts runs that kernel for the whole solve (pipeline 3, ELLP_FLAG_DUAL_BOUND_FLIPPING,
 * or pipeline 0 with m <= ELLP_MID_AUTO_MAX).  Every item ends exactly as the single call
 * (ellp_primal_solve_with_initial / ellp_dual_solve_with_initial with the same opts) ends it: status, iteration counts,
 * index sets and the bits of x (y and d for the dual).  An item's arrays are the single call's arguments; x, B_index,
 * N_index, N_bound (y, d) are updated in place.
 *
 * Returns the status of the call as a whole: ELLP_ERR_ARG (count < 0, items or status_out NULL, an unknown kind, options the
 * batch refuses: pipeline other than 0 / 3, partial_segments > 1, ELLP_FLAG_PRIMAL_STEEPEST_EDGE, trace_len > 0, profile,
 * and the options that make a single call take the explicit-inverse engine instead: refactor_period > 0 or btran_mode != 0
 * on pipeline 0 without ELLP_FLAG_DUAL_BOUND_FLIPPING), ELLP_ERR_DEVICE, or ELLP_OPTIMAL.  These checks and the
 * per-item ones run before any HIP call.  Per item: status_out[i], stats_out[i] (iters, pivots, bound_flips, refactors,
 * obj; may be NULL) and items[i].err.  An item the kernels cannot take (m == 0, m > 1,024, LDS, or one the single call
 * would run on an explicit-inverse engine, e.g. m > 128 with default opts) gets ELLP_ERR_ARG.  Large batches run in
 * consecutive chunks whose device memory stays within a fixed budget; chunking changes no item's result.  When the call as
 * a whole fails (any return value but ELLP_OPTIMAL), status_out, stats_out and the items' arrays are unspecified: items of
 * chunks that ran before the failure may have been updated, the others not.
 * Of opts.flags only ELLP_FLAG_DUAL_MAX_VIOLATION and ELLP_FLAG_DUAL_BOUND_FLIPPING take effect; opts.max_iter holds per item.
 */
typedef struct ellp_batch_item {
    int64_t m, n, n_c;
    const double *A, *c, *b;
    const uint8_t *bound_kind;
    const double *lb, *ub;
    double *x;
    int64_t *B_index;
    int64_t n_B;
    int64_t *N_index;
    uint8_t *N_bound;
    int64_t n_N;
    double *y, *d;  /* dual only */
    char err[256];  /* out: the item's message */
} ellp_batch_item;

ellp_status ellp_batch_solve_with_initial(int kind, int64_t count, ellp_batch_item *items, const ellp_opts *opts,
                                          ellp_status *status_out, ellp_stats *stats_out, char *errbuf,
                                          size_t errbuf_len);

/* Diagnostics of the calling thread's calls of ellp_batch_solve_with_initial: out4[0] how many it has made so far, [1] the
 * items and [2] the kind of the last one, [3] 0.  Counted at entry, whatever the call then returns. */
void ellp_batch_solve_info(uint64_t *out4);

/*
 * Both phases of many primal solves in one batched call: what PrimalSimplexSolver::solve does between building phase 1 and
 * reading the result (primal_simplex_solver.rs:32-93), per item, on the kernels and with the workgroup sizes of
 * ellp_batch_solve_with_initial(ELLP_ENGINE_PRIMAL, ...):
 *   1. phase 1 on p1, opts.max_iter loop bodies at most;
 *   2. the checks of solve() (:42-55): a phase-1 status other than Optimal ends the item at stage 1 with that status;
 *      otherwise obj = c1 . x (summed in index order, as StandardForm::obj): !(obj > -eps) is ELLP_ERR_PANIC ("assertion
 *      failed: obj > -EPS"), !(obj < eps) is ELLP_INFEASIBLE, both at stage 1;
 *   3. the hand-off of PrimalPhase2::from_phase1 (primal_problem.rs:263-291): the costs re-gathered from c2 by the current
 *      index sets, kinds and bounds replaced by bound_kind2 / lb2 / ub2 (n_c entries each), a nonbasic variable whose new
 *      kind is Free labelled ELLP_NB_FREE, status and counters afresh;
 *   4. phase 2 with opts.max_iter loop bodies of its own: its status, stage 2.
 * The workgroup that ends an item's phase 1 does steps 2 to 4 itself, in the same launch: no item waits for another one's
 * phase 1, and an item goes to the device once.  Every item ends as the two ellp_batch_solve_with_initial calls with the
 * host's checks and hand-off in between end it, bit for bit.  x, B_index, N_index and N_bound of p1 hold the point of the
 * phase that ended the solve (at stage 2 with the Free labels).  Options, refusals and chunking are those of
 * ellp_batch_solve_with_initial (per-item errors in results[i].status and p1.err; every check runs before any HIP call);
 * the call also returns ELLP_ERR_ARG when results is NULL, when c2, bound_kind2, lb2 or ub2 of an item is NULL, or when a
 * bound_kind2 entry of an item that passed its own checks is above 4.  A launch gives every running item at most
 * 16,384 (up to 128 rows) / 4,096 loop bodies, phase 1 and phase 2 together (ELLP_BATCH_LAUNCH_ITERS lowers both); an
 * item still running is launched again from its device state in whichever phase it is, with the same bits.
 */
typedef struct ellp_batch_primal_item {
    ellp_batch_item p1;         /* the phase-1 seam arrays, as for ellp_batch_solve_with_initial; updated in place */
    const double *c2;           /* phase 2: n_c costs */
    const uint8_t *bound_kind2; /*          n_c kinds */
    const double *lb2, *ub2;    /*          n_c bounds */
} ellp_batch_primal_item;

typedef struct ellp_batch_primal_result {
    ellp_status status; /* of the phase that ended the solve, or an error */
    int32_t stage;      /* 1: ended in or after phase 1; 2: ended in phase 2 */
    uint64_t iters_phase1, iters_phase2;
    double obj_phase1;  /* c1.x after phase 1 (NaN if phase 1 did not end Optimal) */
    double obj;         /* c.x of the phase that ended the solve, as ellp_stats.obj */
} ellp_batch_primal_result;

ellp_status ellp_batch_primal_solve(int64_t count, ellp_batch_primal_item *items, const ellp_opts *opts,
                                    ellp_batch_primal_result *results, char *errbuf, size_t errbuf_len);

/* Diagnostics of the calling thread's last ellp_batch_primal_solve that passed the checks of the call: out4[0] launch rounds
 * (summed over the chunks), [1] bytes uploaded by the last chunk (the items, then the argument lists of every round),
 * [2] bytes uploaded by all chunks, [3] chunks. */
void ellp_batch_primal_info(uint64_t *out4);

/*
 * Resident form of the same path: the tableau stays in HBM between calls, so a caller
 * (bench.py, a phase-1 -> phase-2 hand-off, a windowed parity test) can run the loop in
 * slices without re-uploading.  create = unpack + gather (primal…:99-155); run = the loop for
 * at most `max_iters` further iterations (returns ELLP_MAXITER when the slice is used up,
 * exactly as the loop does when iter > max_iter); read = copy the point back.
 */
typedef struct ellp_engine ellp_engine;
enum { ELLP_ENGINE_PRIMAL = 0, ELLP_ENGINE_DUAL = 1 };

ellp_status ellp_engine_create(
    int kind,
    int64_t m, int64_t n, int64_t n_c,
    const double *A, const double *c, const double *b,
    const uint8_t *bound_kind, const double *lb, const double *ub,
    const double *x,
    const int64_t *B_index, int64_t n_B,
    const int64_t *N_index, const uint8_t *N_bound, int64_t n_N,
    const double *y, const double *d, /* dual only, else NULL */
    const ellp_opts *opts, ellp_engine **out, char *errbuf, size_t errbuf_len);

/*
 * Primal phase 1 built ON THE DEVICE (primal_problem.rs:236-246, the branch without free
 * variables): the caller passes the standard form (A m x n, b, bounds) and the nonbasic start it has chosen
 * for the n original variables (x[j] = the bound value, N_bound[j] = its label, primal_problem.rs:95-135);
 * the engine appends the m artificial columns itself — b~ = b - A x (one pass over A in HBM), column n+i =
 * signum(b~_i) e_i, value |b~_i|, cost 1, Lower(0), basic — so neither the m x m block nor b~ is computed or
 * uploaded by the host.  The resulting engine has n + m columns (read_point sizes) and is what
 * ellp_engine_create would have built from the phase-1 arrays of the reference.
 */
ellp_status ellp_engine_create_primal_phase1(
    int64_t m, int64_t n,
    const double *A, const double *b,
    const uint8_t *bound_kind, const double *lb, const double *ub,
    const double *x, const uint8_t *N_bound,
    const ellp_opts *opts, ellp_engine **out, char *errbuf, size_t errbuf_len);

ellp_status ellp_engine_run(ellp_engine *e, uint64_t max_iters, ellp_stats *stats,
                            char *errbuf, size_t errbuf_len);

/* Certified endings (pipeline 0, m > 128): a status Optimal / Infeasible / Unbounded that ellp_engine_run
 * (and the one-shot solve_with_initial entry points) return has been decided by the reference's arithmetic on a fresh LU of the
 * final basis.  Between 129 and 1,024 rows a solve that ends Optimal on a point violating an invariant of the reference's loop by
 * more than EPS is repeated from the arrays the phase started with by the LU-per-iteration kernel alone; ellp_stats.iters is then
 * the repeated solve's count, and the engine keeps running on that kernel (no resident inverse: ellp_engine_dual_rephase returns
 * ELLP_ERR_ARG, as on any engine of that kind).  Above 1,024 rows (up to 8,192) the same repetition runs every loop body on a
 * fresh LU of the basis over all CUs (about 18 us x m per iteration), and is taken only when the iterations the phase needed,
 * at that price, stay within ELLP_REDO_MAX_SECONDS (environment, default 900); otherwise the point is returned as it stands
 * and counted (ELLP_TAP_STATE, "not certified").  The resident inverse follows that loop: the next phase runs fast again.
 *
 * ellp_engine_run(e, K) runs up to K loop bodies.  On the two-launch primal pipeline (m >= 384) a slice leaves the
 * ratio test of its last iteration to the next slice's first kernel; when the slice spends the caller's whole budget
 * (ellp_opts.max_iter loop bodies since the engine was made or re-phased) that iteration is completed before the
 * status is taken, so that — as in the reference, which runs max_iter FULL loop bodies (primal…:162-202) — an
 * unbounded ray found in the last permitted iteration is reported as ELLP_UNBOUNDED, not ELLP_MAXITER.
 * ellp_engine_read_point completes an open iteration too; it returns ELLP_OPTIMAL when the point was delivered and the
 * loop can go on (or had ended), otherwise the status that completing the open iteration produced (ELLP_UNBOUNDED,
 * ELLP_ERR_PANIC, ELLP_ERR_NAN): the arrays are filled in either case. */
ellp_status ellp_engine_read_point(ellp_engine *e, double *x, int64_t *B_index,
                                   int64_t *N_index, uint8_t *N_bound, double *y, double *d,
                                   char *errbuf, size_t errbuf_len);

/*
 * Column-block sharding of the pricing pass over several GPUs (one process per GPU).
 * The nonbasic positions are split into `world` contiguous blocks; rank k prices block k and
 * writes (per-block maxima / argmins, keys, reduced costs) into segment k of one exchange
 * buffer of world*seg doubles.  Between ellp_engine_step(e, 0) [pricing] and
 * ellp_engine_step(e, 1) [FTRAN + ratio test + eta update] the caller all-gathers that buffer
 * (RCCL over xGMI via torch.distributed, see ellp_amd/dist.py); everything else is replicated on
 * every rank and deterministic, so all ranks take the same pivots.
 *   segment_doubles: doubles per rank segment for a given world size
 *   set_shard   : choose (rank, world) before the first step; exchange_buffer = caller-owned
 *                 device memory of world*segment_doubles doubles (e.g. a torch tensor's data_ptr,
 *                 so the collective library sees its own allocation), or NULL to let the engine
 *                 allocate it
 *   exchange_info: device pointer of the buffer, doubles per segment, rank, world
 *   set_stream  : run the engine's launches on a caller-owned HIP stream (NULL = its own)
 *   step        : enqueue one half-iteration (never blocks): 0 = pricing, 1 = the rest,
 *                 2 = the rest of this iteration followed by the next iteration's pricing
 *   poll        : copy the status word back; ELLP_MAXITER = still running
 */
int64_t ellp_engine_segment_doubles(ellp_engine *e, int world);
ellp_status ellp_engine_set_shard(ellp_engine *e, int rank, int world, void *exchange_buffer, char *errbuf,
                                  size_t errbuf_len);
ellp_status ellp_engine_exchange_info(ellp_engine *e, void **base, int64_t *seg_doubles, int *rank, int *world);
ellp_status ellp_engine_set_stream(ellp_engine *e, void *hip_stream);
ellp_status ellp_engine_step(ellp_engine *e, int phase, char *errbuf, size_t errbuf_len);
ellp_status ellp_engine_poll(ellp_engine *e, ellp_stats *stats, char *errbuf, size_t errbuf_len);

/*
 * Phase-1 -> phase-2 hand-off of the primal method without leaving HBM (SURVEY.md §8 f2;
 * primal_problem.rs:263-291): the matrix, the basis, the point and B^-1 stay where they are; the
 * costs and bounds (n_c entries each) are replaced, and a nonbasic variable whose new bound is Free
 * gets the label Free (:285-289).  Status and counters start afresh, as for a new
 * solve_with_initial call.  Primal engines only.
 */
ellp_status ellp_engine_rephase(ellp_engine *e, const double *c, const uint8_t *bound_kind, const double *lb,
                                const double *ub, char *errbuf, size_t errbuf_len);

/* DualPhase1::new's starting point made on the device (src/solvers/dual/dual_problem.rs:162-214).
 * In: the box problem's standard form (A m x n column-major, c, b, bounds: TwoSided or Fixed only) and the basis
 * the LU of A^T picked (dual_problem.rs:139-160): B_index[m] and N_index[n-m] in the order of the permutation.
 * The engine builds B^-1 and from it y = B^-T c_B, d = c - A^T y, each nonbasic variable's label and value by
 * the sign of d_i (:177-203), b~ = b - A x and x_B = B^-1 b~ (:206-213); read them back with
 * ellp_engine_read_point.  The result is a dual engine ready for ellp_engine_run (phase 1) and, after it,
 * ellp_engine_dual_rephase (phase 2).  A bound of another kind is the reference's panic (ELLP_ERR_PANIC). */
ellp_status ellp_engine_create_dual_phase1(int64_t m, int64_t n, const double *A, const double *c, const double *b,
                                           const uint8_t *bound_kind, const double *lb, const double *ub,
                                           const int64_t *B_index, const int64_t *N_index, const ellp_opts *opts,
                                           ellp_engine **out, char *errbuf, size_t errlen);

/*
 * The same starting point for many LPs at once, without an engine per LP: for every item, B^-1 from A_B (the blocked
 * rebuild), y, d, the nonbasic labels and values, x_B, the loop's entry assertion and the starting objective, each bit
 * for bit what ellp_engine_create_dual_phase1 followed by ellp_engine_read_point gives for that item alone with these
 * options.  All items' kernels run in the same launches (one workgroup grid per item in grid dimension z), with one host
 * synchronisation after the permutation probe and one read-back.  Per item (ellp_batch_item, n = n_c, n_B = m,
 * n_N = n - m): inputs A, c, b, bound_kind, lb, ub, B_index, N_index (in the order the caller's phase-1 basis has them);
 * outputs x (n), N_bound (n - m), y (m), d (n), err and status_out[i] (ELLP_OPTIMAL, ELLP_ERR_SINGULAR, ELLP_ERR_PANIC,
 * ELLP_ERR_ARG); obj_out[i] (may be NULL) the starting objective.  Items the single call would not start on the
 * LU-per-iteration kernels (m > 1,024, or options that give it the explicit-inverse engine) are refused with
 * ELLP_ERR_ARG.  Chunks within the batch's device budget (ELLP_BATCH_MAX_BYTES) change no item's bits.  Returns
 * ELLP_ERR_ARG for bad arguments of the call, ELLP_ERR_DEVICE on a HIP failure, otherwise ELLP_OPTIMAL. */
ellp_status ellp_batch_dual_phase1_start(int64_t count, ellp_batch_item *items, const ellp_opts *opts,
                                         ellp_status *status_out, double *obj_out, char *errbuf, size_t errlen);

/*
 * The dual method's phase-1 -> phase-2 hand-off without leaving HBM (SURVEY.md §8 f2;
 * DualPhase2::from(phase_1), dual_problem.rs:258-404) for the common case that the box problem of phase 1
 * has the same matrix as the original standard form (no TwoSided / Fixed variable was dropped,
 * dual_problem.rs:96-112 — the caller checks that).  With the basis phase 1 ended on and the resident
 * B^-1: y = B^-T c_B, d = c - A^T y, every nonbasic variable to the bound its kind and the sign of d_i
 * name (with the reference's assertions), N re-listed in variable order (columns moved along on the
 * device), x_B = B^-1 (b - A_N x_N), the dual objective, status and counters afresh.  c, kind, lb, ub:
 * n_c entries of the ORIGINAL standard form; b: m entries.  Engines of the explicit-inverse kind only
 * (m > 128): the persistent small-LP kernel carries no inverse — re-create the engine there.
 */
ellp_status ellp_engine_dual_rephase(ellp_engine *e, const double *c, const double *b, const uint8_t *bound_kind,
                                     const double *lb, const double *ub, char *errbuf, size_t errbuf_len);

/*
 * The same sharded loop driven from inside the library, with the exchange done by RCCL directly
 * on the engine's stream (ncclAllGather, in place, seg doubles per rank) — no host language in the
 * per-iteration path.  RCCL is bound at run time (dlopen; `rccl_path` may name the library the
 * process already uses, e.g. torch's copy; NULL = "librccl.so.1"), so a single-GPU user of this
 * library needs no RCCL.  Rank 0 calls ellp_comm_unique_id(), the 128 bytes travel to the other
 * ranks by any means (torch.distributed broadcast in ellp_amd/dist.py), every rank calls
 * ellp_engine_comm_init() (collective), then ellp_engine_run_sharded() (collective: every rank
 * must pass the same max_iters; the ranks take identical decisions, so they issue identical
 * sequences of collectives).  Returns like ellp_engine_run.
 */
#define ELLP_COMM_ID_BYTES 128
ellp_status ellp_comm_unique_id(const char *rccl_path, void *id_out, char *errbuf, size_t errbuf_len);
ellp_status ellp_engine_comm_init(ellp_engine *e, const char *rccl_path, const void *id, int rank, int world,
                                  char *errbuf, size_t errbuf_len);
ellp_status ellp_engine_run_sharded(ellp_engine *e, uint64_t max_iters, ellp_stats *stats, char *errbuf,
                                    size_t errbuf_len);

/*
 * Column-block sharding with SHARDED STORAGE (primal engines): after
 * ellp_engine_shard_columns(e, rank, world) the engine keeps only the nonbasic columns of its own block
 * (the rest of A_N is released) and ellp_engine_run_sharded() exchanges, once per iteration, one small
 * "pack" per rank — its maximal Dantzig key and the at most two candidates within 6 EPS of it, each with
 * its column (64 KB at m = 4000) — instead of the whole pricing output; when ties reach further the loop
 * falls back, for that iteration, to gathering the complete pricing output (exact in every case, see
 * ellp_amd/csrc/engine/ellp_shard.inc).  Transports for the exchange, chosen by what has been set up:
 *   ellp_engine_comm_init          RCCL all-gather on the engine's stream
 *   ellp_engine_mailbox_*          peer-to-peer mailbox: every rank stores its pack directly into every
 *                                  peer's memory (hipIpc-mapped, over xGMI) and raises a flag there; export
 *                                  gives this rank's two IPC handles (2 x 64 bytes: slots, flags), connect
 *                                  takes those of all ranks in rank order (world x 128 bytes)
 *   ellp_engine_set_exchange_callback   the library stages the segments through host memory and calls
 *                                  fn(user, host_buffer, segment_bytes, world) to all-gather them in place
 *                                  (own segment at rank * segment_bytes); for tests and gloo
 * All of them are collective in the usual sense: every rank makes the same calls in the same order.
 */
typedef int (*ellp_exchange_fn)(void *user, void *host_buffer, int64_t segment_bytes, int world);
ellp_status ellp_engine_shard_columns(ellp_engine *e, int rank, int world, char *errbuf, size_t errbuf_len);
ellp_status ellp_engine_set_exchange_callback(ellp_engine *e, ellp_exchange_fn fn, void *user);
#define ELLP_IPC_HANDLE_BYTES 64
ellp_status ellp_engine_mailbox_export(ellp_engine *e, void *handles_out /* 2 x 64 bytes */, char *errbuf, size_t errbuf_len);
ellp_status ellp_engine_mailbox_connect(ellp_engine *e, const void *all_handles /* world x 128 bytes */, char *errbuf,
                                        size_t errbuf_len);
/* one exchange of a test pattern through the mailbox, every word checked; ELLP_OPTIMAL if it arrived intact */
ellp_status ellp_engine_mailbox_selftest(ellp_engine *e, int rounds, char *errbuf, size_t errbuf_len);
/* counters of the sharded loop: [0] iterations that needed the full exchange, [1] column requests,
 * [2] transport (1 RCCL, 2 mailbox, 3 callback), [3] doubles per pack, [4] first own position, [5] one past the last */
ellp_status ellp_engine_shard_info(ellp_engine *e, double *out6);
/* The selection the ranks run on the gathered packs, as a host function (the same source the kernel
 * k_sh_select compiles; no device needed): packs = world * ellp_shard_pack_doubles(ld) doubles, each pack
 * [M_s, count, overflow, 0, then `count` records of (key, N.index, position, r_j, column[ld])].
 * Returns 1 if the packs are not conclusive (the full exchange is needed), 0 with *q = entering position
 * (-1: none) and the (rank, slot) of the pack that holds its column, -1 on bad arguments. */
int ellp_shard_select_compact(const double *packs, int world, int64_t ld, double eps, int64_t *q, int *src_rank,
                              int *src_slot);
int64_t ellp_shard_pack_doubles(int64_t ld);

/*
 * The optional per-iteration objective trace (ellp_opts.trace_len > 0): the last entries of
 * the ring, oldest first: iters_out[k] = the loop body just completed, obj_out[k] = the objective after it
 * (primal: c.x carried by obj += +-lambda r_q per pivot from c.x at engine creation / hand-off; dual: the dual
 * objective as the loop itself carries it, dual…:316).  Returns the number of entries written (<= cap).
 */
int64_t ellp_engine_read_trace(ellp_engine *e, uint64_t *iters_out, double *obj_out, int64_t cap);

/* The engine ellp_engine_create would make for (kind, m rows, n_N nonbasic columns, opts; NULL: the defaults) — its launch
 * geometry, maintenance settings and mode, decided as creation decides them (the same function, the same environment
 * variables) but without any HIP call: for tests, and for asking "who runs what" on a machine without a device.
 * avail_mask: which of the resources creation may fail to obtain it got: bit 0 the LDS attribute of k_small, bit 1 k_mid's
 * attribute and factor arrays; 3 = all, what creation assumes first.  Writes ELLP_PLAN_FIELDS doubles to out, in this order:
 *   0 ld, 1 cpb, 2 nblocks, 3 priceT, 4 price_nt, 5 price_wave, 6 upd_rows, 7 upd_blocks, 8 upd2_rows, 9 upd2_blocks,
 *   10 ftran_blocks, 11 btran_rows, 12 btran_tiles, 13 upd_stage, 14 upd_lds, 15 ftran_lds, 16 price2_lds, 17 bl_splits,
 *   18 nbs, 19 seg, 20 refactor_period, 21 ill_tol, 22 drift_every, 23 drift_tol, 24 pp_P, 25 pp_S, 26 se, 27 se_vpart wanted,
 *   28 dual_maxviol, 29 dual_bflip, 30 small, 31 mid, 32 small_lds, 33 mid_lds, 34 small_nt, 35 mid_nt, 36 ldn, 37 hybrid,
 *   38 cert_large, 39 guard_abs, 40 exact_K, 41 exact_large_always, 42 lagged, 43 dual_fused, 44 dual_fold,
 *   45 unit-column table wanted, 46 stamps wanted.
 * Returns ELLP_OPTIMAL, or the refusal ellp_engine_create would answer for these options with its text: ELLP_ERR_ARG (in the
 * order: m > 8192; bound flipping with pipeline 1 / 2; steepest edge with partial pricing, pipeline 2 / 3 or btran_mode 1;
 * bound flipping above 1,024 rows), ELLP_ERR_DEVICE where avail_mask takes k_mid from pipeline 3 or bound flipping; and
 * ELLP_ERR_ARG for an unknown kind, m < 1, n_N < 0, out NULL or cap < ELLP_PLAN_FIELDS. */
#define ELLP_PLAN_FIELDS 47
ellp_status ellp_engine_plan(int kind, int64_t m, int64_t n_N, const ellp_opts *opts, int avail_mask, double *out, int64_t cap,
                             char *errbuf, size_t errbuf_len);

/* Debug/parity taps: copy an internal device vector to host. what: see ELLP_TAP_*. Returns
 * the number of doubles written (<= cap) or a negative ellp_status. */
enum { ELLP_TAP_U = 0, ELLP_TAP_R = 1, ELLP_TAP_D = 2, ELLP_TAP_BINV = 3, ELLP_TAP_KEY = 4,
       ELLP_TAP_ALPHA = 5, ELLP_TAP_STATE = 6 /* 12 doubles: status,cur,s_q,s_r,theta_d,delta,lr,ldelta,iters,pivots,lambda,rq;
                                                  cap >= 14: + drift, drift checks; cap >= 20: + maintenance requests
                                                  serviced, Newton-Schulz refreshes, rebuilds, x_B resyncs, last
                                                  refresh residual, launches per primal iteration;
                                                  cap >= 22: + rebuilds settled by the permutation shortcut, setup seconds;
                                                  cap >= 28 (29, 30): + certified hybrid: on?, guarded pivots handed to the exact kernel,
                                                  terminal statuses examined, of those not confirmed, loop bodies run by the
                                                  exact kernel, rebuilds of B^-1 after a hand-over (, solves repeated by the exact
                                                  kernel)(, end points returned NOT certified: a repetition above 1,024 rows that
                                                  ELLP_REDO_MAX_SECONDS ruled out, a singular LU in the certificate) */,
       ELLP_TAP_SE_GAMMA = 7 /* the steepest-edge weights gamma_j = 1 + |B^-1 a_j|^2 (ELLP_FLAG_PRIMAL_STEEPEST_EDGE), n_N doubles
                                by nonbasic position.  The update a pivot asks for is applied by the NEXT pricing launch, so the
                                weights are those of the basis and the position order that the LAST PRICING LAUNCH priced: after
                                ellp_engine_run(e, k) they belong to the point ellp_engine_read_point returned after run(k - 1)
                                (at creation and after ellp_engine_rephase: to the point the engine stands on).  ELLP_ERR_ARG on
                                an engine without the flag. */,
       ELLP_TAP_RESYNC_T = 8 /* t = b - A_N x_N as the last x_B resync (or the primal phase-1 start) formed it, m doubles */,
       ELLP_TAP_RESYNC_CAND = 9 /* cand = B^-1 t of the last x_B resync, adopted or not, m doubles */,
       ELLP_TAP_REBUILD_PERM = 10 /* test hook: the pivot rows of the last rebuild of B^-1, m doubles (cap >= m): entry k is the
                                     row the elimination pivoted on for basic column k, blocked or column by column.  After a
                                     rebuild that ended in ELLP_ERR_SINGULAR the entries from the refused column on are not
                                     those of that rebuild.  ELLP_ERR_ARG when the last rebuild took the permutation shortcut
                                     (which does not eliminate) and when no rebuild has run. */ };
int64_t ellp_engine_tap(ellp_engine *e, int what, double *dst, int64_t cap);

/* One Newton-Schulz step W <- W + W (I - A_B W) on the resident inverse (two f64 GEMMs); this
 * is what the engine does every `refactor_period` iterations.  Returns max|I - A_B W| measured
 * before the step (NaN on error); if that is >= 1e-4 nothing is changed (rebuild instead).  A NaN or
 * Inf in W makes the returned maximum NaN or Inf (the maximum propagates NaN), which refuses the step too. */
double ellp_engine_refresh(ellp_engine *e);

/* Forces a full rebuild of B^-1 from A_B now (used by tests and when a refresh is not safe). */
ellp_status ellp_engine_refactor(ellp_engine *e, char *errbuf, size_t errbuf_len);

/* Test / diagnostic hook: raises the maintenance request a kernel raises after a tiny pivot or a
 * drift-monitor hit (DevState::tiny), as if the last iteration had asked for it.  The next run()/poll()
 * services it: B^-1 is refreshed (and x_B re-checked) before any further iteration. */
ellp_status ellp_engine_request_maintenance(ellp_engine *e);

/* Test hook: multiplies the resident B^-1 by `factor` (a damaged inverse, to exercise the path on
 * which a refresh is refused and the host rebuilds from A_B). */
ellp_status ellp_engine_debug_scale_inverse(ellp_engine *e, double factor);

/* Test hook: replaces the resident B^-1 by W, m x m row-major without padding in host memory: the
 * mirror of ELLP_TAP_BINV (what is set is what that tap reads back, bit for bit).  Nothing else of the
 * engine's state follows: x_B stays as it is until the next maintenance. */
ellp_status ellp_engine_debug_set_inverse(ellp_engine *e, const double *W);

/* Test hook: replaces the engine's point by x, n_c doubles by variable index in host memory: the mirror
 * of the x that ellp_engine_read_point returns (what is set is what it reads back, bit for bit).  Nothing
 * else of the engine's state follows (the carried objective, the dual's leaving row): it is there to put
 * a chosen x_B in front of the next maintenance.  An iteration the two-launch pipeline has left open is
 * completed first, as ellp_engine_read_point does. */
ellp_status ellp_engine_debug_set_x(ellp_engine *e, const double *x);

/* max_ij |(B^-1 A_B - I)_ij| computed on device (drift monitor; tests); NaN if any
 * entry is NaN: never a finite number for an inverse that holds a NaN or an Inf. */
double ellp_engine_inverse_residual(ellp_engine *e);

void ellp_engine_destroy(ellp_engine *e);

/*
 * Postsolve: duals, reduced costs, the row residual and a KKT report for the basis and the point an engine stands on
 * (DESIGN.md §3.9).  The problem is a minimisation; y = B^-T c_B, d = c - A^T y, r = b - A x, so y_i is the derivative
 * of the optimal objective with respect to b_i.  y comes from a fresh LU of the current A_B (never from the loop's carried
 * vectors or explicit inverse) and is refined until its componentwise backward error omega = max_i |rho_i| /
 * (|c_B| + |A_B|^T |y|)_i, rho = c_B - A_B^T y, is at most 2u (u = 2^-53; at most 4 steps, given up when a step does not
 * halve omega; a component a basic column with a single nonzero a e_k fixes on its own is set to y_k = fl(c / a)); d and r are formed from one read of every stored column in compensated arithmetic (error per entry at most
 * u |exact| + gamma_K^2 * sum of the absolute values of the terms) with a reduction order fixed by the launch geometry:
 * two calls on the same state return the same bits.  The engine's state is not touched (a workspace of its own, made at
 * the first call): running on afterwards gives the bits it would have given without the call.
 *   y: m doubles; d: n_c doubles by variable (d_v = c_v for v >= n); r: m doubles; any of y, d, r, kkt may be NULL (not
 *   wanted); all four NULL: ELLP_ERR_ARG.
 * Works for primal and dual engines of every mode, between any two slices and after the run has ended.  An iteration the
 * two-launch pipeline has left open is completed first, as ellp_engine_read_point does; if that produces a status it is
 * returned, with the outputs of the completed point.  A singular basis: ELLP_ERR_SINGULAR, outputs untouched.  Refused
 * with ELLP_ERR_ARG before any HIP call: e NULL, a sharded or column-sharded engine, an engine whose status is an error.
 */
typedef struct ellp_kkt {
    double primal_residual;     /* max_i |r_i|, r = b - A x */
    double bound_violation;     /* max_v violation of x_v's bound by kind (Fixed: |x_v - lb_v|; Free: 0) */
    double dual_infeasibility;  /* max over nonbasic positions j, v = N_index[j]: kind Fixed: 0; label Lower: max(-d_v, 0);
                                   Upper: max(d_v, 0); Free: |d_v| */
    double basic_reduced_cost;  /* max over basic i of |d_{B[i]}| */
    double y_backward_error;    /* omega of the returned y */
    double primal_obj;          /* c.x, compensated */
    double dual_obj;            /* b.y + the bound terms of StandardForm::dual_obj (standard_form.rs:52-68), compensated */
    int64_t worst_row, worst_bound_var, worst_dual_var; /* where the three maxima sit (the smallest such index; of NaNs the
                                   first); -1: the maximum is 0 */
    int32_t refinement_steps;
    int32_t reserved;
} ellp_kkt;

ellp_status ellp_engine_postsolve(ellp_engine *e, double *y /* m */, double *d /* n_c */, double *r /* m */,
                                  ellp_kkt *kkt, char *errbuf, size_t errbuf_len);

/* The same for a point in host memory (the arguments of ellp_primal_solve_with_initial after it returned): a minimal
 * upload into the engine's layout, the same kernels, the same bits.  ELLP_ERR_ARG before any HIP call: a NULL input,
 * m < 1, m > 8192 (the limit of ellp_engine_create), n_B != m, n_B + n_N != n, an index, label or kind out of range, or none
 * of y, d, r, kkt wanted. */
ellp_status ellp_postsolve(int64_t m, int64_t n, int64_t n_c, const double *A, const double *c, const double *b,
                           const uint8_t *bound_kind, const double *lb, const double *ub, const double *x,
                           const int64_t *B_index, int64_t n_B, const int64_t *N_index, const uint8_t *N_bound, int64_t n_N,
                           const ellp_opts *opts, double *y, double *d, double *r, ellp_kkt *kkt,
                           char *errbuf, size_t errbuf_len);

/*
 * The postsolve of many small LPs in one call: the items are those of ellp_batch_solve_with_initial
 * after it returned (x, B_index, N_index and N_bound are read; an item's y and d are ignored), outs[i] says where item i's
 * results go.  Every output of every item is, bit for bit, what ellp_postsolve returns for that item alone, whatever batch
 * it sits in, at whatever position and however the batch is chunked.  An item of up to 128 rows and 65,536 nonbasic
 * columns is done by one workgroup (k_post_batch: the basis and its LU in LDS, the refinement loop and its stop rule on
 * the device), two launches per chunk whatever the item count; any other valid item is run inside the call through
 * ellp_postsolve.  Per item: status_out[i] and items[i].err, the checks, messages and statuses of ellp_postsolve
 * (ELLP_ERR_ARG before any HIP call; ELLP_ERR_SINGULAR with the item's outputs untouched); a failing item changes nothing
 * for the others.  The call as a whole: ELLP_ERR_ARG (count < 0; items, outs or status_out NULL), ELLP_ERR_DEVICE, or
 * ELLP_OPTIMAL; every check runs before any HIP call.  Chunks (budget ELLP_BATCH_MAX_BYTES, at most 65,535 items), the
 * pinned staging buffer, the slab and the buffer pool are those of ellp_batch_solve_with_initial: one upload and one
 * read-back per chunk.  Of opts only device is read by the batched kernel.
 */
typedef struct ellp_batch_post_out {
    double *y, *d, *r; /* m, n_c, m doubles */
    ellp_kkt *kkt;
} ellp_batch_post_out; /* any may be NULL; all NULL: the item's ELLP_ERR_ARG */

ellp_status ellp_batch_postsolve(int64_t count, ellp_batch_item *items, const ellp_opts *opts,
                                 const ellp_batch_post_out *outs, ellp_status *status_out,
                                 char *errbuf, size_t errbuf_len);

/* Diagnostics of the calling thread's last ellp_batch_postsolve that passed the checks of the call: out4[0] kernel launches
 * of the batched path, [1] items on the batched kernel, [2] items on the single path, [3] chunks. */
void ellp_batch_postsolve_info(uint64_t *out4);

/*
 * A starting point from a basis: what a warm-started solve hands to ellp_engine_create.  Standard form,
 * minimisation, n_c = n; the arguments are those of ellp_postsolve without x.  In this order, on the postsolve's kernels
 * and workspace: the fresh LU of A_B and y = B^-T c_B refined to omega <= 2u; d = c - A^T y; the labels and the nonbasic
 * values (by kind: Free -> label Free, 0; Lower -> Lower, lb; Upper -> Upper, ub; Fixed -> Lower, lb; TwoSided with
 * ELLP_START_KEEP_LABELS: the given label, a given Free becomes Lower; TwoSided with ELLP_START_LABELS_BY_D: d_v >= 0 or NaN ->
 * Lower, else Upper — the rule of DualPhase2::from); t = b - A_N x_N; x_B = B^-1 t, refined as y is until
 * omega_x = max_i |t - A_B x_B|_i / (|t| + |A_B||x_B|)_i <= 2u (at most 4 steps, given up when a step does not halve it);
 * the KKT report of that point and the measures a solver needs to decide whether it may start there.  d, t and the residuals
 * come from the postsolve's compensated pass (KEEP_LABELS: one read of A_N; LABELS_BY_D: two, the labels need d first).
 * Reduction orders are fixed by the launch geometry: two calls on the same arguments return the same bits.
 *   N_bound: in/out, the repaired labels are written back; x: n, y: m, d: n doubles; y, d and info may be NULL.
 * ELLP_ERR_SINGULAR: a zero pivot, every output (N_bound too) untouched.  ELLP_ERR_ARG with a message before any HIP call: a
 * NULL input or x, m < 1, m > 8192, n_B != m, n_B + n_N != n, an index out of range or listed twice across B and N, a label
 * or a kind above its range, an unknown mode.
 */
enum { ELLP_START_KEEP_LABELS = 0, ELLP_START_LABELS_BY_D = 1 };

typedef struct ellp_start_info {
    double primal_infeasibility;     /* max over BASIC positions of the bound violation of x (by kind, as ellp_kkt.bound_violation) */
    double primal_infeasibility_sum; /* the sum of those violations, compensated, basic positions in ascending order */
    double dual_infeasibility;       /* as ellp_kkt.dual_infeasibility for the labels returned */
    double x_backward_error;         /* omega of x_B: max_i |t - A_B x_B|_i / (|t| + |A_B| |x_B|)_i, t = b - A_N x_N */
    int64_t worst_primal_var, worst_dual_var; /* smallest index holding the maximum; of NaNs the first; -1: the maximum is 0 */
    int64_t labels_changed;          /* nonbasic positions whose returned label differs from the one passed in */
    int32_t primal_feasible, dual_feasible; /* measure < eps (the eps option); 0 for a NaN; dual_feasible is also 0 when
                                        kkt.basic_reduced_cost is a NaN (a NaN in c_B shows there even without nonbasic columns) */
    int32_t x_refinement_steps, reserved;
    ellp_kkt kkt;                    /* the full report of the point made (its y_backward_error and refinement_steps are y's) */
} ellp_start_info;

ellp_status ellp_basis_start(int64_t m, int64_t n, const double *A, const double *c, const double *b,
                             const uint8_t *bound_kind, const double *lb, const double *ub,
                             const int64_t *B_index, int64_t n_B, const int64_t *N_index, uint8_t *N_bound /* in/out */, int64_t n_N,
                             int mode, const ellp_opts *opts,
                             double *x /* out, n */, double *y /* out, m */, double *d /* out, n */,
                             ellp_start_info *info, char *errbuf, size_t errbuf_len);

/*
 * The starting points of many small LPs in one call.  Items are ellp_batch_item with n_c = n; per item
 * x (n doubles) is out, y (m) and d (n) are out and may be NULL, N_bound is in/out, infos[i] (infos may be NULL) is the
 * item's ellp_start_info.  Every output of every item is, bit for bit, what ellp_basis_start returns for that item alone,
 * whatever batch it sits in, at whatever position and however the batch is chunked.  An item of up to 128 rows and 65,536
 * nonbasic columns is done by one workgroup (k_start_batch: the basis and its LU in LDS, both refinement loops and their
 * stop rules on the device) and reported by one more (k_start_report_batch): two launches, one upload and one read-back
 * per chunk whatever the item count; any other valid item is run inside the call through ellp_basis_start.  Per item:
 * status_out[i] and items[i].err, with the checks, messages, order and statuses of ellp_basis_start (ELLP_ERR_ARG before any
 * HIP call, also for n_c != n; ELLP_ERR_SINGULAR with every output of the item, N_bound included, untouched); a failing
 * item changes nothing for the others.  The call as a whole: ELLP_ERR_ARG (count < 0; items or status_out NULL; an unknown
 * mode), ELLP_ERR_DEVICE, or ELLP_OPTIMAL; every check runs before any HIP call.  Chunks (budget ELLP_BATCH_MAX_BYTES, at
 * most 65,535 items), the pinned staging buffer, the slab and the buffer pool are those of ellp_batch_solve_with_initial.
 * Of opts the batched kernels read device and eps.
 */
ellp_status ellp_batch_basis_start(int64_t count, ellp_batch_item *items, int mode, const ellp_opts *opts,
                                   ellp_start_info *infos /* may be NULL */, ellp_status *status_out,
                                   char *errbuf, size_t errbuf_len);

/* Diagnostics of the calling thread's last ellp_batch_basis_start that passed the checks of the call: out4[0] kernel launches
 * of the batched path, [1] items on the batched kernel, [2] items on the single path, [3] chunks. */
void ellp_batch_basis_start_info(uint64_t *out4);

/*
 * Sensitivity ranging: over what change of one cost coefficient the basis stays optimal, and over what change of one
 * right-hand side it stays feasible.  Standard form, minimisation, at the basis and point the engine stands
 * on.  The call runs the postsolve above (with the completion of an open iteration, the fresh LU and the refined y) and uses
 * its factors and its d; then W = B^-1 row by row from that LU (A_B^T rho_i = e_i, many right-hand sides per workgroup, the
 * arithmetic of the postsolve's own transposed solve), every row of the tableau alpha = W A_N on the matrix cores with the
 * ratio test in the epilogue (the tableau is never stored), and one pass over W for the right-hand sides.
 *
 * All results are CHANGES delta with down <= 0 <= up; -+Inf: unlimited, the blocking variable is then -1.  eps is the
 * engine's eps option.  Zeros are +0.0.
 *   cost of a nonbasic v (label Lower / Upper / Free; kind Fixed: unlimited both ways):
 *       Lower (up, down) = (+Inf, -max(d_v, 0));  Upper (-min(d_v, 0), -Inf);  Free (max(-d_v, 0), min(-d_v, 0)); blocking v.
 *   cost of the basic variable at position i: over the non-Fixed nonbasic positions j, v = N_index[j], alpha = alpha_ij:
 *       Lower: alpha > eps limits up, alpha < -eps limits down, by fl(max(d_v, 0) / alpha);
 *       Upper: alpha < -eps limits up, alpha > eps limits down, by fl(min(d_v, 0) / alpha);
 *       Free:  |alpha| > eps limits both, d_v clamped so that up >= 0 >= down;
 *       up = the smallest, down = the largest such quotient; blocking = N_index of the first extremal position.
 *   a cost without a column (v >= n): (-Inf, +Inf, -1).
 *   right-hand side of row k: over the basic positions i with w = W[i][k], |w| > eps, x = x_{B[i]} and its bounds:
 *       up:   w > 0 and an upper bound (kind Upper, TwoSided, Fixed): fl(max(ub - x, 0) / w);
 *             w < 0 and a lower bound (kind Lower, TwoSided, Fixed): fl(max(x - lb, 0) / -w);
 *       down: w > 0 and a lower bound: fl(max(x - lb, 0) / -w);  w < 0 and an upper bound: fl(max(ub - x, 0) / w);
 *       up = the smallest, down = the largest; blocking = B_index of the first extremal position.
 *   NaN: a NaN alpha_ij (j not Fixed) or w_ik, or a NaN d_v or x in a quotient the definition forms, makes BOTH limits of that
 *   row NaN (blocking: the first position that holds one); a NaN never yields a finite limit.
 * min and max are exact and ties go to the smallest position, so no result depends on the order of the reduction: two calls
 * on one state return the same bits.  The engine's state is not touched (a workspace of its own, m x ld doubles for W and
 * four words per row and block of 128 columns, made at the first call).
 *
 * Every pointer of ellp_ranging_out may be NULL (not wanted); all NULL: ELLP_ERR_ARG.  Status and refusals as for
 * ellp_engine_postsolve (a status produced by completing an open iteration is returned with the outputs; ELLP_ERR_SINGULAR
 * leaves them untouched; ELLP_ERR_ARG before any HIP call: e NULL, out NULL or empty, a sharded engine, an engine in error).
 */
typedef struct ellp_ranging_info {
    double inverse_residual; /* max_ij |(I - A_B W)_ij| of the computed W, each entry summed in ascending k without fma; NaN
                                if any entry is.  Reported, never used to refuse a result */
    int64_t reserved;
    ellp_kkt kkt;            /* the report of the underlying postsolve */
} ellp_ranging_info;

typedef struct ellp_ranging_out {
    double *cost_down, *cost_up;                     /* n_c, by variable */
    int64_t *cost_blocking_down, *cost_blocking_up;  /* n_c */
    double *rhs_down, *rhs_up;                       /* m, by row */
    int64_t *rhs_blocking_down, *rhs_blocking_up;    /* m */
    double *d;                                       /* n_c: the postsolve's reduced costs the ratios were formed from */
    double *y;                                       /* m: the postsolve's duals (with d and info->kkt: one call gives both) */
    ellp_ranging_info *info;
} ellp_ranging_out;

ellp_status ellp_engine_ranging(ellp_engine *e, const ellp_ranging_out *out, char *errbuf, size_t errbuf_len);

/* The same for a point in host memory, with the argument list and the refusals of ellp_postsolve: the same kernels, the
 * same bits. */
ellp_status ellp_ranging(int64_t m, int64_t n, int64_t n_c, const double *A, const double *c, const double *b,
                         const uint8_t *bound_kind, const double *lb, const double *ub, const double *x,
                         const int64_t *B_index, int64_t n_B, const int64_t *N_index, const uint8_t *N_bound, int64_t n_N,
                         const ellp_opts *opts, const ellp_ranging_out *out, char *errbuf, size_t errbuf_len);

/*
 * The ranging of many small LPs in one call: the items are those of ellp_batch_postsolve (the arrays a
 * solve_with_initial call left; x, B_index, N_index and N_bound are read), outs[i] says where item i's results go.  Every
 * output of every item — the eight range arrays, d, y, info->inverse_residual and info->kkt — is, bit for bit, what
 * ellp_ranging returns for that item alone (any NaN equals any NaN), whatever batch it sits in, at whatever position and
 * however the batch is chunked.  An item of up to 128 rows and 65,536 nonbasic columns goes through the batched kernels,
 * FIVE launches per chunk whatever the item count and the items' shapes: k_brange_front (one workgroup per item: the
 * batched postsolve's item, its factors kept), k_brange_solve (W = B^-1, 16 rows per workgroup, the singleton columns
 * snapped), k_brange_tab (the tableau pass on the matrix cores, one workgroup per item and block of 128 columns),
 * k_brange_fold (one workgroup per item: the fold of the blocks, the nonbasic costs, the right-hand sides,
 * inverse_residual) and k_post_report_batch (the KKT report).  Any other valid item is run inside the call by the steps of
 * ellp_ranging.  W (optional, m x m row-major): B^-1 as the ranging formed it, row i what ellp_engine_tableau_rows returns as
 * rho for position i.  Per item: status_out[i] and items[i].err, the checks, messages and statuses of ellp_ranging
 * (ELLP_ERR_ARG before any HIP call, also where nothing is wanted: every pointer of out NULL and W NULL; ELLP_ERR_SINGULAR
 * with the item's outputs untouched); a failing item changes nothing for the others.  The call as a whole: ELLP_ERR_ARG
 * (count < 0; items, outs or status_out NULL), ELLP_ERR_DEVICE, or ELLP_OPTIMAL; every check runs before any HIP call.
 * Chunks (budget ELLP_BATCH_MAX_BYTES, at most 65,535 items), the pinned staging buffer, the slab and the buffer pool are
 * those of ellp_batch_solve_with_initial: one upload and one read-back per chunk; what an item does not ask for is not
 * read back (the two halves of a down / up pair come back together; W only where it is asked for).  Of opts the batched
 * kernels read device and eps.
 */
typedef struct ellp_batch_range_out {
    ellp_ranging_out out;   /* every pointer may be NULL; all NULL and W NULL: the item's ELLP_ERR_ARG */
    double *W;              /* optional, m x m row-major */
} ellp_batch_range_out;

ellp_status ellp_batch_ranging(int64_t count, ellp_batch_item *items, const ellp_opts *opts,
                               const ellp_batch_range_out *outs, ellp_status *status_out,
                               char *errbuf, size_t errbuf_len);

/* Diagnostics of the calling thread's last ellp_batch_ranging that passed the checks of the call: out4[0] kernel launches
 * of the batched path (5 per chunk), [1] items on the batched kernels, [2] items on the single path, [3] chunks. */
void ellp_batch_ranging_info(uint64_t *out4);

/* Chosen rows of the tableau and of W behind them, as the ranging forms them (the same kernel with a storing epilogue: the
 * same bits): alpha[p * n_N + j] = rho_i . a_{N[j]} and rho[p * m + k] = W[i][k] for i = positions[p], p < k.  rho may be
 * NULL.  Refusals as above, and a position outside [0, m), k < 1 or positions / alpha NULL: ELLP_ERR_ARG before any HIP call.
 * Every call pays the whole postsolve and the whole of W again (the state may have moved between two calls), whatever k
 * is: 30 ms at 2000 rows, 160 ms at 4000; ask for all the rows wanted in one call. */
ellp_status ellp_engine_tableau_rows(ellp_engine *e, const int64_t *positions, int64_t k, double *alpha /* k x n_N */,
                                     double *rho /* k x m */, char *errbuf, size_t errbuf_len);

/*
 * Certificates: a Farkas vector for an infeasible LP, a ray for an unbounded one, each with a report of
 * how good a proof it is.  Standard form: A x = b (m x n), bounds (kind, lb, ub) per variable, minimise c . x.
 *
 * Farkas vector y in R^m, z = A^T y.  For variable j: sup_j = z_j ub_j if z_j > 0, z_j lb_j if z_j < 0, 0 if z_j == 0; where
 * the bound needed is infinite (kind Free, Lower with z_j > 0, Upper with z_j < 0) j contributes 0 to the sum and |z_j| to
 * dir_violation (a NaN-propagating maximum, worst_dir_var its first index).  gap = y . b - sum_j sup_j.  Every feasible x
 * has y . b = sum z_j x_j <= sum sup_j, so gap > 0 with dir_violation == 0 proves infeasibility; a positive dir_violation
 * says how far the proof leans on a tolerance.
 *
 * Ray r in R^n: residual = max_i |(A r)_i|, c_r = c . r, bound_dir_violation = max |r_j| over the j with r_j > 0 and a finite
 * upper bound or r_j < 0 and a finite lower bound (Fixed counts on both sides).  c_r < 0 with the other two zero proves
 * unboundedness from any feasible point.
 *
 * The certificate is a function of (the arrays, the basis, the labels) only: every source starts from the postsolve's fresh
 * LU of A_B in a workspace of its own, nothing is read from what a loop carried.
 *   ELLP_CERT_FARKAS_COSTS  y = B^-T c_B of the engine's costs, the postsolve's refined y unchanged (the proof a primal
 *                           phase-1 optimum with a positive objective carries: its costs are zero on the problem's columns).
 *   ELLP_CERT_FARKAS_ROW    x_B is recomputed as ellp_basis_start(ELLP_START_KEEP_LABELS) makes it; basic position r
 *                           qualifies when the dual loop's leaving rule finds its variable outside a bound by more than eps
 *                           and no nonbasic column passes the dual ratio test's filter for that side (the condition under
 *                           which the dual simplex answers Infeasible); the smallest such r; y = -+B^-T e_r, refined as the
 *                           postsolve refines y, the sign such that gap is the violation.
 *   ELLP_CERT_RAY_COLUMN    d from the postsolve; nonbasic position q qualifies when it is a primal entering candidate
 *                           (|d| >= eps with the sign its label asks for), its own kind is Free, Lower or Upper, and no basic
 *                           row bounds the step (the primal ratio test gives +inf in every row, at the point the engine
 *                           stands on); the smallest such q; r_q = +-1 (up from a Lower label, down from an Upper one, a Free
 *                           one against the sign of d), r_B = -+B^-1 a_q refined to a componentwise backward error <= 2u.
 * The searches read the whole tableau B^-1 A_N once on the matrix cores (the ranging's pass with another epilogue; alpha_ij has
 * the bits ellp_engine_tableau_rows returns); every decision is a boolean OR or an integer minimum, so no result depends on a
 * reduction order.  The report comes from the postsolve's compensated pass (z = A^T y, A r) and compensated sums in a fixed
 * order: two calls give the same bits.
 *
 * n_check in [1, n]: only columns 0 .. n_check - 1 take part in the report (a ray is returned on these, other entries
 * dropped); chk_kind / chk_lb / chk_ub (n_check each, or all three NULL: the engine's own bounds) are the bounds the report is
 * made against.  vec: m doubles for a Farkas source, n_check for the ray.
 * ELLP_OPTIMAL: info is filled; found == 0 leaves vec untouched.  ELLP_ERR_SINGULAR, ELLP_ERR_NAN (a NaN in the tableau, in d
 * or in x where a decision reads it): vec and info untouched.  ELLP_ERR_ARG before any HIP call: the refusals of
 * ellp_engine_postsolve / ellp_postsolve, an unknown source, n_check outside [1, n], vec or info NULL, some but not all of
 * chk_* NULL, a chk_kind out of range.  The engine's state is not touched (an open iteration of the two-launch pipeline is
 * completed first, as the postsolve does); the workspace is released by ellp_engine_destroy.
 */
enum { ELLP_CERT_FARKAS_COSTS = 0, ELLP_CERT_FARKAS_ROW = 1, ELLP_CERT_RAY_COLUMN = 2 };
enum { ELLP_CERT_KIND_NONE = 0, ELLP_CERT_KIND_FARKAS = 1, ELLP_CERT_KIND_RAY = 2 };
typedef struct ellp_cert_info {
    int32_t kind;               /* ELLP_CERT_KIND_*: what the source makes (FARKAS or RAY, also when found == 0) */
    int32_t found;
    int64_t source;             /* the row position r or the nonbasic position q the vector came from; -1: none, or the
                                   cost-based Farkas vector */
    int64_t qualifying;         /* how many rows or columns qualified (0 for ELLP_CERT_FARKAS_COSTS) */
    double gap, y_b, sup;       /* Farkas: y . b - sum sup_j, and its two parts; each a compensated sum rounded once */
    double dir_violation;       /* Farkas */
    double residual, c_r;       /* ray */
    double bound_dir_violation; /* ray */
    double norm;                /* max |entry| of the vector */
    int64_t worst_dir_var, worst_row, worst_bound_var; /* where the three maxima sit; -1: the maximum is 0 */
    int32_t refine_steps;       /* refinement steps of the vector's own solve */
    int32_t reserved;
} ellp_cert_info;

ellp_status ellp_engine_certificate(ellp_engine *e, int source, int64_t n_check, const uint8_t *chk_kind, const double *chk_lb,
                                    const double *chk_ub, double *vec, ellp_cert_info *info, char *errbuf, size_t errbuf_len);
/* The same for a point in host memory, with the argument list of ellp_postsolve: the checks before any HIP call, a minimal
 * engine, the same kernels and the same bits. */
ellp_status ellp_certificate(int64_t m, int64_t n, int64_t n_c, const double *A, const double *c, const double *b,
                             const uint8_t *bound_kind, const double *lb, const double *ub, const double *x,
                             const int64_t *B_index, int64_t n_B, const int64_t *N_index, const uint8_t *N_bound, int64_t n_N,
                             const ellp_opts *opts, int source, int64_t n_check, const uint8_t *chk_kind, const double *chk_lb,
                             const double *chk_ub, double *vec, ellp_cert_info *info, char *errbuf, size_t errbuf_len);
/* The process's certificate calls: out4[0] calls of the two entry points so far (refused ones included), out4[1] kernels
 * the last call enqueued — its own stages, every compensated pass and fold and the solves of x_B, each counted where it is
 * launched; the LU, the triangular solves of y and B^-1 are not counted; independent of n, of m only through the refinement
 * steps — out4[2] the refinement steps of its vector, out4[3] 0.  Not thread safe. */
void ellp_certificate_info(uint64_t *out4);

/*
 * SURVEY.md §8 f3 — the rank check of the standard form on the device: column-pivoted Householder
 * QR of A^T (src/standard_form.rs:142 `A.transpose().col_piv_qr()`), reduced to what :143-181
 * consume.  A: m x nv column-major (ld = m) in HOST memory, not modified.  pivot_out[i] = the
 * column of A^T (row of A) swapped into position i at step i (the transposition list),
 * rdiag_out[i] = |R_ii|, both of length min(m, nv).  Default: the host loop's steps with norms and dot products reduced in
 * parallel (fast mode; |R_ii| to rounding, reproducible from run to run) — and, if at any step the two best pivot candidates
 * were different but closer than those reductions can tell apart (1e-12 relative), the factorisation is done again in
 * the exact mode, in which every floating-point result is bitwise what the host loop of ellp_amd/csrc/host/dense.h
 * (ColPivQR) produces (4x slower): the pivot order is the host loop's in every case.  ELLP_QR_EXACT=1 in the environment:
 * exact from the start; ELLP_QR_EXACT=0: fast without the fall-back (measurements).  device < 0: current device.
 */
ellp_status ellp_hip_qr_transposed(int64_t m, int64_t nv, const double *A, int64_t *pivot_out, double *rdiag_out,
                                   int device, char *errbuf, size_t errbuf_len);

/* LU with partial pivoting of A^T on the device: `std_form.A.transpose().lu()` of DualPhase1::new
 * (src/solvers/dual/dual_problem.rs:139-160) reduced to what :141-160 consume.  A: m x nv column-major (the box
 * problem's standard-form matrix), nv >= m.  pivot_out[i] = the row of A^T (= column of A) exchanged with row i at
 * step i (i itself: no exchange; also for a skipped zero column), udiag_out[i] = U_ii, both of length m.  Every
 * floating-point result is bitwise what the host loop of ellp_amd/csrc/host/dense.h (LU) produces.
 * device < 0: current device. */
ellp_status ellp_hip_lu_transposed(int64_t m, int64_t nv, const double *A, int64_t *pivot_out, double *udiag_out,
                                   int device, char *errbuf, size_t errbuf_len);

/*
 * The same factorisation of a SQUARE matrix stored by rows (row r at M_in + r * m, host memory), as the LU-per-iteration loop
 * above 1,024 rows takes it of the basis every iteration: uploaded, factored, read back.  variant 0: the
 * unblocked form, two launches per column; variant 1: the blocked form the engine uses, panels of 16 columns, two launches
 * per panel.  factors_out (m x m by rows): L's multipliers below the diagonal, U on and above, rows in pivoted order;
 * pivot_out[i] = the row exchanged with row i at step i (i itself: none, also for a skipped zero column); udiag_out[i] = U_ii.
 * Both variants leave byte for byte what the host loop of ellp_amd/csrc/host/dense.h (LU) leaves.  m <= 0, a NULL pointer or
 * an unknown variant: ELLP_ERR_ARG with a message, before any HIP call.  device < 0: current device.
 * ellp_hip_lu_rows_last_ms: device time of the factorisation alone in the last successful call (measurements; not thread safe).
 */
ellp_status ellp_hip_lu_rows(int64_t m, const double *M_in, int variant, double *factors_out, int64_t *pivot_out,
                             double *udiag_out, int device, char *errbuf, size_t errbuf_len);
double ellp_hip_lu_rows_last_ms(void);

#ifdef __cplusplus
}
#endif
#endif

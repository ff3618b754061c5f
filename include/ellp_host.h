/*
 * ellp_host.h — C view of the C++ host mirror (ellp_amd/csrc/host/ellp.h) so that Python
 * (ctypes) and C callers can drive the same Problem -> solve() flow the reference exposes
 * (src/lib.rs:109-129).  The simplex loops behind solve() run on the GPU via ellp_hip.h.
 */
#ifndef ELLP_HOST_H
#define ELLP_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "ellp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ellp_problem ellp_problem;

/* ConstraintOp (problem.rs:299-303) */
enum { ELLP_OP_LTE = 0, ELLP_OP_EQ = 1, ELLP_OP_GTE = 2 };
enum { ELLP_SOLVER_PRIMAL = 0, ELLP_SOLVER_DUAL = 1 };

ellp_problem *ellp_problem_new(void);                      /* Problem::new         problem.rs:20 */
ellp_problem *ellp_problem_clone(const ellp_problem *p);
void ellp_problem_free(ellp_problem *p);
/* Problem::add_var (problem.rs:24): returns the id or -1 (message in errbuf). name may be NULL. */
int64_t ellp_problem_add_var(ellp_problem *p, double obj_coeff, int bound_kind, double lb, double ub,
                             const char *name, char *errbuf, size_t errbuf_len);
int64_t ellp_problem_add_var_with_id(ellp_problem *p, double obj_coeff, int bound_kind, double lb, double ub,
                                     int64_t id, const char *name, char *errbuf, size_t errbuf_len);
/* Problem::add_constraint (problem.rs:85): 0 ok, -1 error. */
int ellp_problem_add_constraint(ellp_problem *p, int64_t n, const int64_t *var_ids, const double *coeffs,
                                int op, double rhs, char *errbuf, size_t errbuf_len);
int64_t ellp_problem_num_vars(const ellp_problem *p);
int64_t ellp_problem_num_constraints(const ellp_problem *p);
/* Problem::is_feasible (problem.rs:108) */
int ellp_problem_is_feasible(const ellp_problem *p, const double *x, int64_t n);
/* parse_mps (parse_mps.rs:23): NULL on error (message in errbuf). */
ellp_problem *ellp_parse_mps(const char *text, char *errbuf, size_t errbuf_len);

/* SolverResult (solver.rs:6-12) flattened. */
typedef struct ellp_result {
    int status;        /* ellp_status: OPTIMAL / INFEASIBLE / UNBOUNDED / MAXITER or an error */
    double obj;        /* Optimal: sol.obj(); MaxIter: the `obj` field */
    int64_t nx;        /* prob.variables.len() */
    double *x;         /* Optimal: sol.x(), owned by the result (ellp_result_free) */
    uint64_t iters_phase1, iters_phase2;
    char err[512];
} ellp_result;

/* PrimalSimplexSolver / DualSimplexSolver ::solve (primal…:32, dual…:33).
 * max_iter: ELLP_MAX_ITER_NONE = ::new(None); 1000 = ::default().  opts may be NULL; only its
 * engine fields (device, refactor_period, btran_mode, poll_interval) are used. */
int ellp_solve(const ellp_problem *p, int solver, uint64_t max_iter, const ellp_opts *opts, ellp_result *out);
void ellp_result_free(ellp_result *r);

/* ellp_solve with the opt-in postsolve (ellp_engine_postsolve / ellp_postsolve, ellp_hip.h): with postsolve != 0 an Optimal
 * result also carries the duals (one per constraint of the problem, in order: the derivative of the optimal objective with
 * respect to that constraint's right-hand side — the problem is a minimisation, so <= 0 for a binding `<=` row, >= 0 for a
 * binding `>=` row — and 0.0 for a row the rank check dropped as redundant), the reduced costs d = c - A^T y of the
 * problem's variables, and the KKT report of the final point in standard form.  postsolve == 0: exactly ellp_solve, not one
 * extra device call, has_postsolve = 0.  ellp_solve, ellp_result and ellp_solve_batch are unchanged. */
typedef struct ellp_result_ex {
    ellp_result result;
    int has_postsolve;
    int64_t n_duals;           /* the problem's constraints */
    double *duals;             /* owned by the result (ellp_result_ex_free) */
    int64_t n_reduced_costs;   /* the problem's variables */
    double *reduced_costs;
    ellp_kkt kkt;
} ellp_result_ex;
int ellp_solve_ex(const ellp_problem *p, int solver, uint64_t max_iter, const ellp_opts *opts, int postsolve, ellp_result_ex *out);
void ellp_result_ex_free(ellp_result_ex *r);

/* ellp_solve with a flags word: ELLP_SOLVE_POSTSOLVE as ellp_solve_ex's postsolve, ELLP_SOLVE_RANGING (implies the postsolve)
 * adds the sensitivity ranging of an Optimal result (ellp_engine_ranging / ellp_ranging, ellp_hip.h has the definitions): for
 * every variable of the problem the change of its cost over which the final basis stays optimal, for every constraint the
 * change of its right-hand side over which the basis stays feasible (down <= 0 <= up, -+Inf: unlimited; a row the rank check
 * dropped: 0, 0, -1).  Blocking entries are indices of the standard form: below the problem's variable count that variable,
 * above a slack or phase-1 column, -1 for an unlimited side.  The final basis is reported in the same indices: B_index
 * (one per row of the standard form), N_index / N_bound (ELLP_NB_*), x_std (the point by standard-form index) and
 * row_origin (the constraint each row of the standard form came from).  flags == 0: exactly ellp_solve, not one extra device
 * call.  ellp_solve_ex and ellp_result_ex are unchanged. */
#define ELLP_SOLVE_POSTSOLVE 1u
#define ELLP_SOLVE_RANGING 2u
typedef struct ellp_result_rng {
    ellp_result_ex ex;
    int has_ranging;
    int64_t n_cost;            /* the problem's variables */
    double *cost_down, *cost_up;
    int64_t *cost_blocking_down, *cost_blocking_up;
    int64_t n_rhs;             /* the problem's constraints */
    double *rhs_down, *rhs_up;
    int64_t *rhs_blocking_down, *rhs_blocking_up;
    double inverse_residual;
    int64_t n_B, n_N, n_x_std; /* the final basis in standard form */
    int64_t *B_index, *N_index, *row_origin;
    uint8_t *N_bound;
    double *x_std;
} ellp_result_rng;
int ellp_solve_flags(const ellp_problem *p, int solver, uint64_t max_iter, const ellp_opts *opts, unsigned flags, ellp_result_rng *out);
void ellp_result_rng_free(ellp_result_rng *r);

/* A warm start: solve from a given basis.  Indices are those of the standard form of the problem — its
 * variables, then the slacks — which is what B_index / N_index of an ellp_result_rng hold after a dual solve; after a primal
 * solve the phase-1 columns follow at indices >= the standard form's columns: such an entry of N is dropped, one in B makes
 * the start unusable.  N_index NULL: N is the complement of B in ascending order, every label Lower; N_bound NULL: every
 * label Lower (ellp_basis_start repairs the labels by kind, and for the dual solver by the sign of d).
 * The point of the basis is made on the device (ellp_basis_start: ELLP_START_KEEP_LABELS for the primal solver, which needs
 * primal_feasible; ELLP_START_LABELS_BY_D for the dual solver, which needs dual_feasible).  Each solver runs its own method
 * only: after a changed right-hand side call the dual solver, after a changed cost the primal solver.  A usable start runs
 * phase 2 directly on the standard form (iters_phase1 = 0, report->used = 1).  An unusable start is never an error: the call
 * then does exactly what ellp_solve_flags does, with used = 0 and reason
 *   1  B has not one entry per row, or N (after the drop) not one per remaining column;
 *   2  an index out of range (a phase-1 column in B is one) or listed twice;
 *   3  A_B is singular;   4  the point is not feasible for this solver's method;   5  the problem has no rows.
 * On Optimal the basis fields of ellp_result_rng (B_index, N_index, N_bound, x_std, row_origin) are always filled, so that
 * solves chain; has_postsolve / has_ranging follow flags as in ellp_solve_flags.  ELLP_ERR_ARG: p, start or out NULL, an
 * unknown solver or flag.  report may be NULL.  Free with ellp_result_rng_free. */
typedef struct ellp_start { int64_t n_B; const int64_t *B_index; int64_t n_N; const int64_t *N_index; const uint8_t *N_bound; } ellp_start;
typedef struct ellp_start_report { int used; int reason; ellp_start_info info; } ellp_start_report;
int ellp_solve_start(const ellp_problem *p, int solver, uint64_t max_iter, const ellp_opts *opts, unsigned flags,
                     const ellp_start *start, ellp_result_rng *out, ellp_start_report *report);
/* Certificates: ellp_solve_flags / ellp_solve_start (start may be NULL: no warm start) with one more flag,
 * ELLP_SOLVE_CERTIFICATE, which only this entry point accepts.  With the flag an Infeasible result of primal phase 1 (an
 * optimum with a positive objective) or of dual phase 2 carries a Farkas vector — vec: one entry per constraint of the
 * problem, with the sign convention of the duals (<= 0 on a `<=` row, >= 0 on a `>=` row, 0.0 on a row the rank check
 * dropped) — and an Unbounded result of primal phase 2 a ray — vec: one entry per variable of the problem; info is the
 * device's report (ellp_cert_info, include/ellp_hip.h) on the standard form the vector was made on.  Every other ending has
 * kind ELLP_CERT_KIND_NONE and a reason: infeasibility decided by the set-up, no rows, a loop status of primal phase 1,
 * MaxIter, Optimal, search found none, or a certificate call that met a NaN or a singular basis.  Without the flag the call
 * is exactly ellp_solve_flags / ellp_solve_start (not one extra device call) and *cert is zeroed.  ELLP_ERR_ARG: p, out or
 * cert NULL, an unknown solver or flag.  report may be NULL.  Free out with ellp_result_rng_free, cert with
 * ellp_result_cert_free. */
#define ELLP_SOLVE_CERTIFICATE 4u
typedef struct ellp_result_cert { int kind; char reason[128]; int64_t n; double *vec; ellp_cert_info info; } ellp_result_cert;
int ellp_solve_cert(const ellp_problem *p, int solver, uint64_t max_iter, const ellp_opts *opts, unsigned flags,
                    const ellp_start *start, ellp_result_rng *out, ellp_start_report *report, ellp_result_cert *cert);
void ellp_result_cert_free(ellp_result_cert *c);
/* Test/diagnostic tap, host only: the start as ellp_solve_start maps it into the standard form.  *rows, *cols: the standard
 * form's; B_out (rows), N_out / Nb_out (cols - rows) when the return is 0; capacity: what the arrays hold, at least *cols.
 * Returns 0, a reason (1, 2, 5) or a negative ellp_status. */
int ellp_debug_map_start(const ellp_problem *p, const ellp_start *start, int64_t *rows, int64_t *cols, int64_t *B_out,
                         int64_t *N_out, uint8_t *Nb_out, int64_t capacity);

/* solve() of many problems by one solver in lock step: every phase's device loops of the problems the small kernel
 * takes (1 to 128 rows, with nonbasic columns), and of the 129 to 1,024-row problems the single call runs on the exact
 * mid-size kernel (pipeline 3, ELLP_MID_AUTO_MAX, the dual's bound flipping), run in one batched
 * ellp_batch_solve_with_initial; the dual's phase-1 starts of the latter come from one ellp_batch_dual_phase1_start.  The
 * rest go through ellp_solve.  out[k] is exactly what ellp_solve(probs[k], ...) fills in (ellp_result_free each).  Returns ELLP_ERR_ARG
 * (count < 0, a NULL pointer, an unknown solver), ELLP_ERR_DEVICE (host memory; every out[k] says so) or 0. */
int ellp_solve_batch(const ellp_problem *const *probs, int64_t count, int solver, uint64_t max_iter, const ellp_opts *opts,
                     ellp_result *out);

/* ellp_solve_batch with the postsolve of ellp_solve_ex: postsolve != 0 adds, to every Optimal out[k], the duals, reduced costs
 * and KKT report that ellp_solve_ex(probs[k], ..., 1, ...) returns, bit for bit, from ONE ellp_batch_postsolve call for the
 * whole batch (ellp_hip.h; a problem without rows is answered on the host).  A refusal or a singular basis of one problem is
 * that out[k]'s status and message, as ellp_solve_ex reports it.  postsolve == 0: exactly ellp_solve_batch, not one extra
 * device call, has_postsolve = 0.  Free each out[k] with ellp_result_ex_free.  ellp_solve_batch is unchanged. */
int ellp_solve_batch_ex(const ellp_problem *const *probs, int64_t count, int solver, uint64_t max_iter, const ellp_opts *opts,
                        int postsolve, ellp_result_ex *out);

/* ellp_solve_batch_ex with warm starts: starts[k] is problem k's start as ellp_solve_start takes it, or NULL
 * for none.  Per problem the standard form is built and the start mapped as ellp_solve_start maps it, with its reasons
 * unchanged; the points of ALL mapped starts are made in ONE ellp_batch_basis_start call (ELLP_START_KEEP_LABELS for the
 * primal solver, ELLP_START_LABELS_BY_D for the dual), and phase 2 of the usable starts the batch takes runs in ONE
 * ellp_batch_solve_with_initial call of their own (iters_phase1 = 0).  A usable start the batch does not take runs phase 2
 * alone, from the point already made; the problems whose start is not usable, and those without one, are solved by the
 * cold batch of ellp_solve_batch.  out[k] is what ellp_solve_start(probs[k], ..., starts[k], ...) fills in, reports[k] its
 * report (zeros for a problem without a start), and on Optimal the basis fields of EVERY out[k] are filled, started or not,
 * so that batches chain.  flags: 0 or ELLP_SOLVE_POSTSOLVE (one ellp_batch_postsolve call for the whole batch).
 * ELLP_ERR_ARG: count < 0, probs, starts, out or reports NULL, a NULL problem, an unknown solver, an unknown flag or
 * ELLP_SOLVE_RANGING (the batched ranging is ellp_solve_batch_flags'); ELLP_ERR_DEVICE (host memory; every out[k] says so) or 0.  Free each
 * out[k] with ellp_result_rng_free.  ellp_solve_batch and ellp_solve_batch_ex are unchanged. */
int ellp_solve_batch_start(const ellp_problem *const *probs, int64_t count, int solver, uint64_t max_iter, const ellp_opts *opts,
                           unsigned flags, const ellp_start *const *starts, ellp_result_rng *out, ellp_start_report *reports);

/* ellp_solve_batch_start with the flags of ellp_solve_flags, and with starts optional.  starts NULL: no
 * problem has a start (reports may then be NULL and is not written); otherwise starts[k] may be NULL as above and reports is
 * needed.  flags: ELLP_SOLVE_POSTSOLVE and ELLP_SOLVE_RANGING (implies the postsolve).  Without ELLP_SOLVE_RANGING the call is
 * exactly ellp_solve_batch_start where starts is given, and exactly ellp_solve_batch_ex with the basis fields of every
 * Optimal out[k] filled where it is NULL.  With it every Optimal out[k] is, bit for bit, what
 * ellp_solve_flags(probs[k], ..., ELLP_SOLVE_POSTSOLVE | ELLP_SOLVE_RANGING, ...) fills in — with starts, what
 * ellp_solve_start(probs[k], ..., starts[k], ...) fills in — and the whole batch makes ONE ellp_batch_ranging call
 * (ellp_hip.h) and no ellp_batch_postsolve call: the ranging's own y, d and report are the postsolve.  A problem without
 * rows is answered on the host; a row the rank check dropped has (0, 0, -1).  Where the single call fails (a singular
 * basis, a refusal) out[k] carries that status and message.  ELLP_ERR_ARG before any device work: count < 0, probs or out
 * NULL, starts given without reports, a NULL problem, an unknown solver or an unknown flag bit; ELLP_ERR_DEVICE (host
 * memory; every out[k] says so) or 0.  Free each out[k] with ellp_result_rng_free. */
int ellp_solve_batch_flags(const ellp_problem *const *probs, int64_t count, int solver, uint64_t max_iter, const ellp_opts *opts,
                           unsigned flags, const ellp_start *const *starts /* may be NULL: no starts */, ellp_result_rng *out,
                           ellp_start_report *reports /* may be NULL when starts is */);

/* Test/diagnostic tap: the flattened phase-1 problem (exactly the arrays that solve() hands to
 * ellp_*_solve_with_initial) so the host setup can be checked without a GPU.  All arrays are
 * owned by the struct (ellp_flat_phase_free).  Returns 0, 1 if the setup already proves
 * infeasibility (None), or a negative ellp_status. */
typedef struct ellp_flat_phase {
    int64_t m, n, n_c, n_B, n_N;
    double *A, *c, *b, *lb, *ub, *x, *y, *d;
    uint8_t *bound_kind, *N_bound;
    int64_t *B_index, *N_index;
} ellp_flat_phase;
int ellp_debug_phase1(const ellp_problem *p, int solver, ellp_flat_phase *out, char *errbuf, size_t errbuf_len);
void ellp_flat_phase_free(ellp_flat_phase *f);

#ifdef __cplusplus
}
#endif
#endif

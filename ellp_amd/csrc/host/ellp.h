// ellp.h — C++ host mirror of kehlert/ellp's public API (src/lib.rs:109-129) for the one path
// this repository accelerates.  Names, argument meaning and error behaviour follow the
// reference so that tests read like tests/integration_tests.rs; the per-iteration simplex loops
// (solve_with_initial) are NOT here — they run on the MI355X through include/ellp_hip.h.
//
//   Problem / Bound / Constraint / ConstraintOp / Variable / VariableId   src/problem.rs
//   StandardForm / Point / Basic / Nonbasic / NonbasicBound               src/standard_form.rs
//   PrimalPhase1/2, DualPhase1/2                                          src/solvers/*/..._problem.rs
//   PrimalSimplexSolver / DualSimplexSolver / SolverResult / Solution     src/solvers, src/solver.rs
//   parse_mps                                                             src/parse_mps.rs
#pragma once

#include <cstdint>
#include <exception>
#include <limits>
#include <optional>
#include <stdexcept>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

#include "dense.h"
#include "ellp_hip.h"

namespace ellp {

constexpr double EPS = 1e-10;  // src/util.rs:1

// src/error.rs:3-11
struct EllPError : std::runtime_error {
    explicit EllPError(const std::string &msg) : std::runtime_error(msg) {}
};
// a panic!/assert! of the reference (never crosses the C boundary as an exception)
struct EllPPanic : std::logic_error {
    explicit EllPPanic(const std::string &msg) : std::logic_error(msg) {}
};

// src/problem.rs:190-197
struct Bound {
    enum Kind : std::uint8_t { Free = 0, Lower = 1, Upper = 2, TwoSided = 3, Fixed = 4 };
    Kind kind = Free;
    double lb = 0.0, ub = 0.0;
    static Bound free() { return {Free, 0.0, 0.0}; }
    static Bound lower(double l) { return {Lower, l, 0.0}; }
    static Bound upper(double u) { return {Upper, 0.0, u}; }
    static Bound two_sided(double l, double u) { return {TwoSided, l, u}; }
    static Bound fixed(double v) { return {Fixed, v, v}; }
};

using VariableId = std::size_t;  // src/problem.rs:277-278

enum class ConstraintOp { Lte, Eq, Gte };  // src/problem.rs:298-303

struct Variable {  // src/problem.rs:156-162
    VariableId id;
    double obj_coeff;
    Bound bound;
    std::optional<std::string> name;
};

struct Constraint {  // src/problem.rs:225-230
    std::vector<std::pair<VariableId, double>> coeffs;
    ConstraintOp op;
    double rhs;
};

class Problem {  // src/problem.rs:11-154
public:
    std::vector<Variable> variables;
    std::vector<Constraint> constraints;

    VariableId add_var(double obj_coeff, Bound bound, std::optional<std::string> name = std::nullopt);
    VariableId add_var_with_id(double obj_coeff, Bound bound, VariableId id,
                               std::optional<std::string> name = std::nullopt);
    void add_constraint(std::vector<std::pair<VariableId, double>> coeffs, ConstraintOp op, double rhs);
    bool is_feasible(const std::vector<double> &x) const;

private:
    std::unordered_set<std::string> var_names_;
    std::unordered_set<VariableId> var_ids_;
};

// src/standard_form.rs:205-221
enum class NonbasicBound : std::uint8_t { Lower = 0, Upper = 1, Free = 2 };
struct Nonbasic {
    std::size_t index;
    NonbasicBound bound;
};
struct Basic {
    std::size_t index;
};
struct Point {  // src/standard_form.rs:20-25
    std::vector<double> x;
    std::vector<Nonbasic> N;
    std::vector<Basic> B;
};

struct StandardForm {  // src/standard_form.rs:27-75
    std::vector<double> c;
    dense::Matrix A;
    std::vector<double> b;
    std::vector<Bound> bounds;
    Problem prob;
    // extension: row k of A came from prob.constraints[row_origin[k]] (the rows the rank check kept, standard_form.rs:142-181);
    // what maps the duals of a postsolve back to the user's constraints
    std::vector<std::size_t> row_origin;

    std::size_t rows() const { return static_cast<std::size_t>(A.rows); }
    std::size_t cols() const { return static_cast<std::size_t>(A.cols); }
    double obj(const std::vector<double> &x) const;
    double dual_obj(const std::vector<double> &y, const std::vector<double> &d) const;
    std::vector<double> extract_solution(const Point &point) const;

    // impl From<Problem> for Option<StandardForm>  (standard_form.rs:78-191)
    static std::optional<StandardForm> from_problem(Problem prob);
};

struct DualFeasiblePoint {  // src/solvers/dual/dual_problem.rs:11-16
    std::vector<double> y, d;
    Point point;
};

struct PrimalPhase2;
struct PrimalPhase1 {  // src/solvers/primal/primal_problem.rs:38-43
    StandardForm std_form;
    Point point;
    std::vector<std::size_t> phase_1_vars;
    double obj() const { return std_form.obj(point.x); }
    static std::optional<PrimalPhase1> from_problem(Problem prob);  // :80-261
};
struct PrimalPhase2 {  // :59-63
    StandardForm std_form;
    Point point;
    double obj() const { return std_form.obj(point.x); }
    static PrimalPhase2 from_phase1(PrimalPhase1 phase_1);  // :263-291
};

struct DualPhase1 {  // src/solvers/dual/dual_problem.rs:41-46
    StandardForm std_form;
    DualFeasiblePoint point;
    StandardForm orig_std_form;
    // true: B and N are set (the LU of A^T picked them, :139-160) but y, d, x and the nonbasic labels are still
    // zero / Lower — ellp_engine_create_dual_phase1 makes them on the device (:162-214)
    bool point_deferred = false;
    double obj() const { return std_form.dual_obj(point.y, point.d); }
    // defer_point: leave :162-214 (LU of A_B, three solves, A x) to the device when the engine is of the
    // explicit-inverse kind (rows > 128) and there is a nonbasic variable
    static std::optional<DualPhase1> from_problem(Problem prob, bool defer_point = false);  // :89-256
};
struct DualPhase2 {  // :69-73
    StandardForm std_form;
    DualFeasiblePoint point;
    double obj() const { return std_form.dual_obj(point.y, point.d); }
    static DualPhase2 from_phase1(DualPhase1 phase_1);  // :258-404
    // the same without its linear algebra: original standard form, B mapped through the variable ids, N listed
    // in variable order with placeholder labels, x / y / d zero — for the device hand-off
    // (ellp_engine_dual_rephase), which fills them in
    static DualPhase2 shell_from_phase1(DualPhase1 phase_1);
    // the linear algebra of from_phase1 on a shell (dual_problem.rs:275-350: LU of A_B, y, d, labels, x): what the host
    // falls back to when the device hand-off is not available (an engine of the LU-per-iteration kind keeps no
    // inverse) or trips one of the reference's EPS assertions on its inexact inverse
    void point_on_host();
};

enum class SolutionStatus { Optimal, Infeasible, Unbounded, MaxIter };  // src/solver.rs:27-33

// extension (with_postsolve(true)): the duals, reduced costs and KKT report of an Optimal solution (ellp_engine_postsolve /
// ellp_postsolve, include/ellp_hip.h).  The problem is a minimisation, d = c - A^T y, and duals[i] is the derivative of the
// optimal objective with respect to the right-hand side of constraint i of the user's Problem: <= 0 for a binding `<=` row,
// >= 0 for a binding `>=` row, 0.0 for a row the rank check dropped as redundant.
struct Postsolve {
    std::vector<double> duals;          // one per constraint of the Problem, in order
    std::vector<double> reduced_costs;  // one per variable of the Problem, in order
    ellp_kkt kkt{};
};

// extension (with_ranging(true)): over what change of one cost coefficient the final basis stays optimal and over what change
// of one right-hand side it stays feasible (ellp_engine_ranging / ellp_ranging, include/ellp_hip.h has the definitions).  All
// limits are changes, down <= 0 <= up, -+infinity: unlimited.  A blocking entry is an index of the standard form (below the
// number of the Problem's variables: that variable; above: a slack or phase-1 column) or -1 for an unlimited side.
struct Ranging {
    std::vector<double> cost_down, cost_up;                          // one per variable of the Problem, in order
    std::vector<std::int64_t> cost_blocking_down, cost_blocking_up;
    std::vector<double> rhs_down, rhs_up;                            // one per constraint of the Problem, in order; a row the rank
    std::vector<std::int64_t> rhs_blocking_down, rhs_blocking_up;    // check dropped: (0.0, 0.0, -1)
    double inverse_residual = 0.0;                                   // max |I - A_B W| of the computed inverse (0 without rows)
};

struct Solution {  // src/solver.rs:35-54
    StandardForm std_form;
    Point point;
    std::optional<Postsolve> post;  // set by a solver made with_postsolve(true)
    std::optional<Ranging> rng;     // set by a solver made with_ranging(true)
    const Ranging &ranging() const {
        if (!rng) throw EllPError("solve(..., ranging=True) was not asked for");
        return *rng;
    }
    double obj() const { return std_form.obj(point.x); }
    std::vector<double> x() const { return std_form.extract_solution(point); }
    const Postsolve &postsolve() const {
        if (!post) throw EllPError("solve(..., postsolve=True) was not asked for");
        return *post;
    }
    const std::vector<double> &duals() const { return postsolve().duals; }
    const std::vector<double> &reduced_costs() const { return postsolve().reduced_costs; }
    const ellp_kkt &kkt() const { return postsolve().kkt; }
};

// extension (with_certificate(true)): the proof an Infeasible or Unbounded result carries (ellp_engine_certificate /
// ellp_certificate, include/ellp_hip.h has the definitions).  Farkas: vec has one entry per constraint of the Problem, with the
// sign convention of duals() (0.0 for a row the rank check dropped); Ray: one per variable of the Problem.  info is the device's
// report on the standard form the vector was made on.  kind None: there is no certificate, and reason says which case it is
struct Certificate {
    enum Kind { None = 0, Farkas = 1, Ray = 2 } kind = None;
    std::string reason;
    std::vector<double> vec;
    ellp_cert_info info{};
};

struct SolverResult {  // src/solver.rs:6-12
    enum Kind { Optimal, Infeasible, Unbounded, MaxIter } kind = Infeasible;
    std::optional<Solution> solution;  // Optimal
    double max_iter_obj = 0.0;         // MaxIter { obj }
    std::uint64_t iters_phase1 = 0, iters_phase2 = 0;  // extension: iteration counts of the device loops
    std::optional<Certificate> cert;   // set by a solver made with_certificate(true), whatever the result
};

// solvers/trivial/solve_trivial_problem.rs:5-96
SolutionStatus solve_trivial_problem(const StandardForm &std_form, std::vector<double> &x,
                                     std::vector<Nonbasic> &N, bool minimize);

// Engine knobs that have no counterpart in the reference (0 = engine default).
struct EngineOptions {
    int device = -1;
    int refactor_period = 0;
    int btran_mode = 0;
    int poll_interval = 0;
    int partial_segments = 0;  // ellp_opts.partial_segments (> 1: partial pricing, an opt-in extension)
    int pipeline = 0;  // ellp_opts.pipeline: 0 = chosen by size, 1 / 2 = launches per iteration, 3 = persistent small kernel
    int flags = 0;     // ellp_opts.flags (include/ellp_hip.h): ELLP_FLAG_DENSE_PRICING, and the opt-in extensions ELLP_FLAG_DUAL_MAX_VIOLATION,
                       // ELLP_FLAG_PRIMAL_STEEPEST_EDGE, ELLP_FLAG_DUAL_BOUND_FLIPPING; ELLP_FLAG_NO_CERTIFY
};

// extension (solve_from): a basis to start from, in the indices of StandardForm::from_problem(prob) — the Problem's variables,
// then the slacks; what Solution's basis reports after a dual solve, and after a primal solve with the phase-1 columns
// appended at indices >= cols() (such an entry of N is dropped, one in B makes the start unusable).  has_N false: N is the
// complement of B in ascending order, every label Lower before the repair of ellp_basis_start.
struct StartBasis {
    std::vector<std::int64_t> B, N;
    std::vector<std::uint8_t> Nb;
    bool has_N = false;
};
// why a start was not used (an unusable start is never an error: solve_from then returns exactly what solve returns)
enum StartReason {
    START_USED = 0,
    START_BAD_SIZE = 1,     // B has not rows() entries, or N (after the drop) not cols() - rows()
    START_BAD_INDEX = 2,    // an index out of range (a phase-1 column in B is one), or listed twice
    START_SINGULAR = 3,     // A_B is not invertible
    START_NOT_FEASIBLE = 4, // the point is not primal feasible (primal solver) / not dual feasible (dual solver)
    START_NO_ROWS = 5,      // a problem without rows has no basis: the start is ignored
};
struct StartReport {
    bool used = false;
    int reason = START_USED;
    ellp_start_info info{};  // the measures of ellp_basis_start (zero where it was not reached)
};
// the start mapped into the standard form and checked (sizes, then indices and duplicates): START_USED and B, N, Nb of the
// call to ellp_basis_start, or the reason.  Host only
int map_start(const StandardForm &sf, const StartBasis &start, std::vector<std::int64_t> &B, std::vector<std::int64_t> &N,
              std::vector<std::uint8_t> &Nb);

class PrimalSimplexSolver {  // src/solvers/primal/primal_simplex_solver.rs:15-93
public:
    PrimalSimplexSolver() : max_iter_(1000) {}  // Default, :19-23
    explicit PrimalSimplexSolver(std::optional<std::uint64_t> max_iter)  // new(), :26-30
        : max_iter_(max_iter.value_or(std::numeric_limits<std::uint64_t>::max())) {}
    PrimalSimplexSolver &with_engine(const EngineOptions &o) { engine_ = o; return *this; }
    // extension, off by default (off: not one extra device call): an Optimal Solution carries duals(), reduced_costs(), kkt()
    // (from the resident engine that ran phase 2 where there is one and it takes the call, else from phase 2's arrays)
    PrimalSimplexSolver &with_postsolve(bool on) { postsolve_ = on; return *this; }
    // extension, off by default (off: not one extra device call): an Optimal Solution carries ranging(); implies the postsolve, which
    // comes out of the same device call (one LU, not two)
    PrimalSimplexSolver &with_ranging(bool on) { ranging_ = on; if (on) postsolve_ = true; return *this; }
    // extension, off by default (off: not one extra device call): the result carries a Certificate — a Farkas vector where phase 1
    // ends Optimal with a positive objective, a ray where phase 2 ends Unbounded, else kind None with the reason
    PrimalSimplexSolver &with_certificate(bool on) { certificate_ = on; return *this; }

    SolverResult solve(Problem prob) const;  // :32-93
    // extension: phase 2 directly from the point of `start` where that point is primal feasible (ellp_basis_start, KEEP_LABELS),
    // iters_phase1 = 0; else exactly solve(prob).  This solver runs the primal method only: a start that is dual but not
    // primal feasible (a changed right-hand side) is one for DualSimplexSolver::solve_from
    SolverResult solve_from(Problem prob, const StartBasis &start, StartReport *report = nullptr) const;
    // :95-236 — the loop itself runs on the GPU (ellp_primal_solve_with_initial)
    SolutionStatus solve_with_initial(const StandardForm &std_form, Point &pt, std::uint64_t *iters = nullptr) const;

private:
    std::uint64_t max_iter_;
    EngineOptions engine_;
    bool postsolve_ = false;
    bool ranging_ = false;
    bool certificate_ = false;
};

class DualSimplexSolver {  // src/solvers/dual/dual_simplex_solver.rs:16-108
public:
    DualSimplexSolver() : max_iter_(1000) {}
    explicit DualSimplexSolver(std::optional<std::uint64_t> max_iter)
        : max_iter_(max_iter.value_or(std::numeric_limits<std::uint64_t>::max())) {}
    DualSimplexSolver &with_engine(const EngineOptions &o) { engine_ = o; return *this; }
    DualSimplexSolver &with_postsolve(bool on) { postsolve_ = on; return *this; }
    DualSimplexSolver &with_ranging(bool on) { ranging_ = on; if (on) postsolve_ = true; return *this; }
    // extension, off by default: a Farkas vector where phase 2 ends Infeasible; the fall-back into the primal solver passes the
    // option on and returns that result's certificate
    DualSimplexSolver &with_certificate(bool on) { certificate_ = on; return *this; }

    SolverResult solve(Problem prob) const;
    // extension: phase 2 directly from the point of `start` where it is dual feasible (ellp_basis_start, LABELS_BY_D); else
    // exactly solve(prob).  The dual method only: after a changed cost call PrimalSimplexSolver::solve_from
    SolverResult solve_from(Problem prob, const StartBasis &start, StartReport *report = nullptr) const;
    SolutionStatus solve_with_initial(const StandardForm &std_form, DualFeasiblePoint &pt,
                                      std::uint64_t *iters = nullptr) const;

private:
    std::uint64_t max_iter_;
    EngineOptions engine_;
    bool postsolve_ = false;
    bool ranging_ = false;
    bool certificate_ = false;
};

// Many problems solved by one solver (solver: ELLP_SOLVER_PRIMAL / ELLP_SOLVER_DUAL) in lock step, the device loops of a
// phase in one batched call (ellp_batch_solve_with_initial).  Outcome k is what solve(probs[k]) returns, or the
// exception it throws (error set).
struct BatchOutcome {
    SolverResult result;
    std::exception_ptr error;
};
// postsolve: every Optimal outcome's Solution carries duals(), reduced_costs() and kkt(), from ONE ellp_batch_postsolve call for
// the whole batch, with the bits of solve() with_postsolve(true); false: not one extra device call
// starts (one entry per problem, null: none): the warm start of solve_from for a batch.  The points of all
// mapped starts come from ONE ellp_batch_basis_start call, phase 2 of the usable ones the batch takes runs in ONE
// ellp_batch_solve_with_initial call of their own (iters_phase1 = 0), a usable one it does not take runs phase 2 alone from
// the point already made, and the problems without a usable start join the cold batch.  Outcome k is solve_from's (the
// postsolve by the one batched call); (*reports)[k] its StartReport (untouched defaults for a problem without a start).
// starts null: the cold batch alone, not one extra device call.  Throws std::invalid_argument on a length mismatch
// ranging (implies the postsolve): every Optimal outcome's Solution also carries its Ranging, with the bits of solve()
// with_ranging(true) (of solve_from where starts are given), from ONE ellp_batch_ranging call for the whole batch and no
// ellp_batch_postsolve call; false: not one extra device call
std::vector<BatchOutcome> solve_batch(int solver, std::vector<Problem> probs, std::uint64_t max_iter, const EngineOptions &eng,
                                      bool postsolve = false, const std::vector<const StartBasis *> *starts = nullptr,
                                      std::vector<StartReport> *reports = nullptr, bool ranging = false);

// src/parse_mps.rs:11-66.  Variables/rows are taken in file order (the reference iterates
// HashMaps, so its order is unspecified).
struct MpsParsingError : std::runtime_error {
    explicit MpsParsingError(const std::string &msg) : std::runtime_error("MPS parsing error. " + msg) {}
};
Problem parse_mps(const std::string &mps);

}  // namespace ellp

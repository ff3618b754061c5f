// capi.cpp — extern "C" surface of the host mirror (include/ellp_host.h).  Exceptions never
// cross this boundary: EllPError / panics of the reference become status codes + messages.
#include <cstdio>
#include <cstring>

#include <type_traits>

#include "ellp.h"
#include "ellp_host.h"

struct ellp_problem {
    ellp::Problem prob;
};

namespace {
void put(char *buf, size_t len, const std::string &msg) {
    if (buf && len) std::snprintf(buf, len, "%s", msg.c_str());
}
ellp::Bound make_bound(int kind, double lb, double ub) {
    switch (kind) {
    case ELLP_BOUND_FREE: return ellp::Bound::free();
    case ELLP_BOUND_LOWER: return ellp::Bound::lower(lb);
    case ELLP_BOUND_UPPER: return ellp::Bound::upper(ub);
    case ELLP_BOUND_TWOSIDED: return ellp::Bound::two_sided(lb, ub);
    case ELLP_BOUND_FIXED: return ellp::Bound::fixed(lb);
    default: throw ellp::EllPError("invalid bound kind");
    }
}
}  // namespace

extern "C" {

ellp_problem *ellp_problem_new(void) { return new ellp_problem(); }
ellp_problem *ellp_problem_clone(const ellp_problem *p) { return p ? new ellp_problem(*p) : nullptr; }
void ellp_problem_free(ellp_problem *p) { delete p; }

int64_t ellp_problem_add_var_with_id(ellp_problem *p, double obj_coeff, int bound_kind, double lb, double ub,
                                     int64_t id, const char *name, char *errbuf, size_t errlen) {
    try {
        std::optional<std::string> nm;
        if (name) nm = std::string(name);
        if (id < 0) throw ellp::EllPError("negative variable id");
        return static_cast<int64_t>(p->prob.add_var_with_id(obj_coeff, make_bound(bound_kind, lb, ub),
                                                            static_cast<ellp::VariableId>(id), std::move(nm)));
    } catch (const std::exception &e) {
        put(errbuf, errlen, e.what());
        return -1;
    }
}
int64_t ellp_problem_add_var(ellp_problem *p, double obj_coeff, int bound_kind, double lb, double ub,
                             const char *name, char *errbuf, size_t errlen) {
    return ellp_problem_add_var_with_id(p, obj_coeff, bound_kind, lb, ub,
                                        static_cast<int64_t>(p->prob.variables.size()), name, errbuf, errlen);
}
int ellp_problem_add_constraint(ellp_problem *p, int64_t n, const int64_t *ids, const double *coeffs, int op,
                                double rhs, char *errbuf, size_t errlen) {
    try {
        std::vector<std::pair<ellp::VariableId, double>> cf;
        cf.reserve(static_cast<size_t>(n));
        for (int64_t k = 0; k < n; ++k) {
            if (ids[k] < 0) throw ellp::EllPError("negative variable id");
            cf.emplace_back(static_cast<ellp::VariableId>(ids[k]), coeffs[k]);
        }
        const ellp::ConstraintOp o = op == ELLP_OP_LTE ? ellp::ConstraintOp::Lte
                                     : op == ELLP_OP_GTE ? ellp::ConstraintOp::Gte
                                                         : ellp::ConstraintOp::Eq;
        p->prob.add_constraint(std::move(cf), o, rhs);
        return 0;
    } catch (const std::exception &e) {
        put(errbuf, errlen, e.what());
        return -1;
    }
}
int64_t ellp_problem_num_vars(const ellp_problem *p) { return static_cast<int64_t>(p->prob.variables.size()); }
int64_t ellp_problem_num_constraints(const ellp_problem *p) { return static_cast<int64_t>(p->prob.constraints.size()); }
int ellp_problem_is_feasible(const ellp_problem *p, const double *x, int64_t n) {
    return p->prob.is_feasible(std::vector<double>(x, x + n)) ? 1 : 0;
}
ellp_problem *ellp_parse_mps(const char *text, char *errbuf, size_t errlen) {
    try {
        auto *p = new ellp_problem();
        p->prob = ellp::parse_mps(text ? text : "");
        return p;
    } catch (const std::exception &e) {
        put(errbuf, errlen, e.what());
        return nullptr;
    }
}

}  // extern "C"

namespace {
ellp::EngineOptions engine_options(const ellp_opts *opts) {
    ellp::EngineOptions eo;
    if (opts) {
        eo.device = opts->device;
        eo.refactor_period = opts->refactor_period;
        eo.btran_mode = opts->btran_mode;
        eo.poll_interval = opts->poll_interval;
        eo.pipeline = opts->pipeline;
        eo.partial_segments = opts->partial_segments;
        eo.flags = opts->flags;
    }
    return eo;
}
// *out from what `run` returns or throws
template <class F>
int fill_result(ellp_result *out, F &&run, ellp_result_ex *ex = nullptr, ellp_result_rng *rng = nullptr, bool basis_always = false,
                ellp_result_cert *cert = nullptr) {
    std::memset(out, 0, sizeof(*out));
    try {
        ellp::SolverResult r = run();
        out->iters_phase1 = r.iters_phase1;
        out->iters_phase2 = r.iters_phase2;
        if (cert && r.cert) {
            cert->kind = static_cast<int>(r.cert->kind);
            put(cert->reason, sizeof(cert->reason), r.cert->reason.c_str());
            cert->n = static_cast<int64_t>(r.cert->vec.size());
            cert->vec = new double[r.cert->vec.size() ? r.cert->vec.size() : 1];
            std::memcpy(cert->vec, r.cert->vec.data(), sizeof(double) * r.cert->vec.size());
            cert->info = r.cert->info;
        }
        switch (r.kind) {
        case ellp::SolverResult::Optimal: {
            out->status = ELLP_OPTIMAL;
            out->obj = r.solution->obj();
            const std::vector<double> x = r.solution->x();
            out->nx = static_cast<int64_t>(x.size());
            out->x = new double[x.size() ? x.size() : 1];
            std::memcpy(out->x, x.data(), sizeof(double) * x.size());
            if (ex && r.solution->post) {
                const ellp::Postsolve &ps = *r.solution->post;
                auto dup = [](const std::vector<double> &v) {
                    double *q = new double[v.size() ? v.size() : 1];
                    std::memcpy(q, v.data(), sizeof(double) * v.size());
                    return q;
                };
                ex->has_postsolve = 1;
                ex->n_duals = static_cast<int64_t>(ps.duals.size());
                ex->duals = dup(ps.duals);
                ex->n_reduced_costs = static_cast<int64_t>(ps.reduced_costs.size());
                ex->reduced_costs = dup(ps.reduced_costs);
                ex->kkt = ps.kkt;
            }
            auto dup = [](const auto &v) {
                using T = typename std::decay_t<decltype(v)>::value_type;
                T *q = new T[v.size() ? v.size() : 1];
                std::memcpy(q, v.data(), sizeof(T) * v.size());
                return q;
            };
            if (rng && r.solution->rng) {
                const ellp::Ranging &rg = *r.solution->rng;
                rng->has_ranging = 1;
                rng->n_cost = static_cast<int64_t>(rg.cost_down.size());
                rng->cost_down = dup(rg.cost_down); rng->cost_up = dup(rg.cost_up);
                rng->cost_blocking_down = dup(rg.cost_blocking_down); rng->cost_blocking_up = dup(rg.cost_blocking_up);
                rng->n_rhs = static_cast<int64_t>(rg.rhs_down.size());
                rng->rhs_down = dup(rg.rhs_down); rng->rhs_up = dup(rg.rhs_up);
                rng->rhs_blocking_down = dup(rg.rhs_blocking_down); rng->rhs_blocking_up = dup(rg.rhs_blocking_up);
                rng->inverse_residual = rg.inverse_residual;
            }
            if (rng && (r.solution->rng || basis_always)) {  // the final basis: with the ranging, and always after ellp_solve_start
                const ellp::Point &pt = r.solution->point;
                std::vector<int64_t> B, N, ro;
                std::vector<uint8_t> Nb;
                for (const auto &bv : pt.B) B.push_back(static_cast<int64_t>(bv.index));
                for (const auto &nb : pt.N) {
                    N.push_back(static_cast<int64_t>(nb.index));
                    Nb.push_back(static_cast<uint8_t>(nb.bound));
                }
                for (size_t o : r.solution->std_form.row_origin) ro.push_back(static_cast<int64_t>(o));
                rng->n_B = static_cast<int64_t>(B.size()); rng->n_N = static_cast<int64_t>(N.size());
                rng->n_x_std = static_cast<int64_t>(pt.x.size());
                rng->B_index = dup(B); rng->N_index = dup(N); rng->N_bound = dup(Nb); rng->row_origin = dup(ro); rng->x_std = dup(pt.x);
            }
            break;
        }
        case ellp::SolverResult::Infeasible: out->status = ELLP_INFEASIBLE; break;
        case ellp::SolverResult::Unbounded: out->status = ELLP_UNBOUNDED; break;
        case ellp::SolverResult::MaxIter:
            out->status = ELLP_MAXITER;
            out->obj = r.max_iter_obj;
            break;
        }
    } catch (const ellp::EllPError &e) {
        out->status = std::strstr(e.what(), "not invertible") ? ELLP_ERR_SINGULAR : ELLP_ERR_BAD_DIMS;
        put(out->err, sizeof(out->err), e.what());
    } catch (const ellp::EllPPanic &e) {
        out->status = ELLP_ERR_PANIC;
        put(out->err, sizeof(out->err), e.what());
    } catch (const std::exception &e) {
        out->status = ELLP_ERR_DEVICE;
        put(out->err, sizeof(out->err), e.what());
    }
    return out->status;
}
// the C view of a start as the C++ one; a negative count or a missing array gives sizes no standard form has (reason 1)
ellp::StartBasis start_basis(const ellp_start *st) {
    ellp::StartBasis sb;
    if (st->n_B > 0 && st->B_index) sb.B.assign(st->B_index, st->B_index + st->n_B);
    if (st->N_index) {
        sb.has_N = true;
        if (st->n_N > 0) sb.N.assign(st->N_index, st->N_index + st->n_N);
        if (st->N_bound) sb.Nb.assign(st->N_bound, st->N_bound + sb.N.size());
        else sb.Nb.assign(sb.N.size(), 0);  // without labels: every one Lower before the repair
    }
    return sb;
}
}  // namespace

extern "C" {

int ellp_solve(const ellp_problem *p, int solver, uint64_t max_iter, const ellp_opts *opts, ellp_result *out) {
    const ellp::EngineOptions eo = engine_options(opts);
    const std::optional<std::uint64_t> mi =
        max_iter == ELLP_MAX_ITER_NONE ? std::nullopt : std::optional<std::uint64_t>(max_iter);
    return fill_result(out, [&] {
        return solver == ELLP_SOLVER_PRIMAL ? ellp::PrimalSimplexSolver(mi).with_engine(eo).solve(p->prob)
                                            : ellp::DualSimplexSolver(mi).with_engine(eo).solve(p->prob);
    });
}

int ellp_solve_ex(const ellp_problem *p, int solver, uint64_t max_iter, const ellp_opts *opts, int postsolve, ellp_result_ex *out) {
    if (!out) return ELLP_ERR_ARG;
    std::memset(out, 0, sizeof(*out));
    if (!p || (solver != ELLP_SOLVER_PRIMAL && solver != ELLP_SOLVER_DUAL)) {
        out->result.status = ELLP_ERR_ARG;
        put(out->result.err, sizeof(out->result.err), "ellp_solve_ex: no problem, or an unknown solver");
        return ELLP_ERR_ARG;
    }
    const ellp::EngineOptions eo = engine_options(opts);
    const std::optional<std::uint64_t> mi =
        max_iter == ELLP_MAX_ITER_NONE ? std::nullopt : std::optional<std::uint64_t>(max_iter);
    ellp_result base;
    const int s = fill_result(&base, [&] {
        return solver == ELLP_SOLVER_PRIMAL ? ellp::PrimalSimplexSolver(mi).with_engine(eo).with_postsolve(postsolve != 0).solve(p->prob)
                                            : ellp::DualSimplexSolver(mi).with_engine(eo).with_postsolve(postsolve != 0).solve(p->prob);
    }, out);
    out->result = base;
    return s;
}

int ellp_solve_flags(const ellp_problem *p, int solver, uint64_t max_iter, const ellp_opts *opts, unsigned flags, ellp_result_rng *out) {
    if (!out) return ELLP_ERR_ARG;
    std::memset(out, 0, sizeof(*out));
    if (!p || (solver != ELLP_SOLVER_PRIMAL && solver != ELLP_SOLVER_DUAL) || (flags & ~(ELLP_SOLVE_POSTSOLVE | ELLP_SOLVE_RANGING))) {
        out->ex.result.status = ELLP_ERR_ARG;
        put(out->ex.result.err, sizeof(out->ex.result.err), "ellp_solve_flags: no problem, an unknown solver or an unknown flag");
        return ELLP_ERR_ARG;
    }
    const ellp::EngineOptions eo = engine_options(opts);
    const std::optional<std::uint64_t> mi =
        max_iter == ELLP_MAX_ITER_NONE ? std::nullopt : std::optional<std::uint64_t>(max_iter);
    const bool post = (flags & ELLP_SOLVE_POSTSOLVE) != 0, rng = (flags & ELLP_SOLVE_RANGING) != 0;
    ellp_result base;
    const int s = fill_result(&base, [&] {
        return solver == ELLP_SOLVER_PRIMAL ? ellp::PrimalSimplexSolver(mi).with_engine(eo).with_postsolve(post).with_ranging(rng).solve(p->prob)
                                            : ellp::DualSimplexSolver(mi).with_engine(eo).with_postsolve(post).with_ranging(rng).solve(p->prob);
    }, &out->ex, out);
    out->ex.result = base;
    return s;
}

int ellp_solve_start(const ellp_problem *p, int solver, uint64_t max_iter, const ellp_opts *opts, unsigned flags, const ellp_start *start,
                     ellp_result_rng *out, ellp_start_report *report) {
    if (report) std::memset(report, 0, sizeof(*report));
    if (!out) return ELLP_ERR_ARG;
    std::memset(out, 0, sizeof(*out));
    if (!p || !start || (solver != ELLP_SOLVER_PRIMAL && solver != ELLP_SOLVER_DUAL) || (flags & ~(ELLP_SOLVE_POSTSOLVE | ELLP_SOLVE_RANGING))) {
        out->ex.result.status = ELLP_ERR_ARG;
        put(out->ex.result.err, sizeof(out->ex.result.err), "ellp_solve_start: no problem, no start, an unknown solver or an unknown flag");
        return ELLP_ERR_ARG;
    }
    const ellp::StartBasis sb = start_basis(start);
    const ellp::EngineOptions eo = engine_options(opts);
    const std::optional<std::uint64_t> mi =
        max_iter == ELLP_MAX_ITER_NONE ? std::nullopt : std::optional<std::uint64_t>(max_iter);
    const bool post = (flags & ELLP_SOLVE_POSTSOLVE) != 0, rng = (flags & ELLP_SOLVE_RANGING) != 0;
    ellp::StartReport rep;
    ellp_result base;
    const int s = fill_result(&base, [&] {
        return solver == ELLP_SOLVER_PRIMAL
                   ? ellp::PrimalSimplexSolver(mi).with_engine(eo).with_postsolve(post).with_ranging(rng).solve_from(p->prob, sb, &rep)
                   : ellp::DualSimplexSolver(mi).with_engine(eo).with_postsolve(post).with_ranging(rng).solve_from(p->prob, sb, &rep);
    }, &out->ex, out, /*basis_always=*/true);
    out->ex.result = base;
    if (report) {
        report->used = rep.used ? 1 : 0;
        report->reason = rep.reason;
        report->info = rep.info;
    }
    return s;
}

int ellp_solve_cert(const ellp_problem *p, int solver, uint64_t max_iter, const ellp_opts *opts, unsigned flags, const ellp_start *start,
                    ellp_result_rng *out, ellp_start_report *report, ellp_result_cert *cert) {
    if (report) std::memset(report, 0, sizeof(*report));
    if (cert) std::memset(cert, 0, sizeof(*cert));
    if (!out) return ELLP_ERR_ARG;
    std::memset(out, 0, sizeof(*out));
    if (!p || !cert || (solver != ELLP_SOLVER_PRIMAL && solver != ELLP_SOLVER_DUAL) ||
        (flags & ~(ELLP_SOLVE_POSTSOLVE | ELLP_SOLVE_RANGING | ELLP_SOLVE_CERTIFICATE))) {
        out->ex.result.status = ELLP_ERR_ARG;
        put(out->ex.result.err, sizeof(out->ex.result.err), "ellp_solve_cert: no problem, no cert, an unknown solver or an unknown flag");
        return ELLP_ERR_ARG;
    }
    const unsigned rest = flags & ~ELLP_SOLVE_CERTIFICATE;
    if (!(flags & ELLP_SOLVE_CERTIFICATE))  // exactly the existing entry points
        return start ? ellp_solve_start(p, solver, max_iter, opts, rest, start, out, report) : ellp_solve_flags(p, solver, max_iter, opts, rest, out);
    const ellp::EngineOptions eo = engine_options(opts);
    const std::optional<std::uint64_t> mi =
        max_iter == ELLP_MAX_ITER_NONE ? std::nullopt : std::optional<std::uint64_t>(max_iter);
    const bool post = (flags & ELLP_SOLVE_POSTSOLVE) != 0, rng = (flags & ELLP_SOLVE_RANGING) != 0;
    ellp::StartReport rep;
    ellp::StartBasis sb;
    if (start) sb = start_basis(start);
    ellp_result base;
    const int s = fill_result(&base, [&] {
        ellp::PrimalSimplexSolver ps(mi);
        ellp::DualSimplexSolver ds(mi);
        ps.with_engine(eo).with_postsolve(post).with_ranging(rng).with_certificate(true);
        ds.with_engine(eo).with_postsolve(post).with_ranging(rng).with_certificate(true);
        if (start) return solver == ELLP_SOLVER_PRIMAL ? ps.solve_from(p->prob, sb, &rep) : ds.solve_from(p->prob, sb, &rep);
        return solver == ELLP_SOLVER_PRIMAL ? ps.solve(p->prob) : ds.solve(p->prob);
    }, &out->ex, out, /*basis_always=*/start != nullptr, cert);
    out->ex.result = base;
    if (report && start) {
        report->used = rep.used ? 1 : 0;
        report->reason = rep.reason;
        report->info = rep.info;
    }
    return s;
}

void ellp_result_cert_free(ellp_result_cert *c) {
    if (!c) return;
    delete[] c->vec;
    c->vec = nullptr;
    c->n = 0;
}

int ellp_debug_map_start(const ellp_problem *p, const ellp_start *start, int64_t *rows, int64_t *cols, int64_t *B_out, int64_t *N_out,
                         uint8_t *Nb_out, int64_t capacity) {
    if (!p || !start || !rows || !cols) return ELLP_ERR_ARG;
    try {
        auto sf = ellp::StandardForm::from_problem(p->prob);
        if (!sf) return ELLP_ERR_ARG;
        *rows = static_cast<int64_t>(sf->rows());
        *cols = static_cast<int64_t>(sf->cols());
        if (sf->rows() == 0) return ellp::START_NO_ROWS;
        std::vector<int64_t> B, N;
        std::vector<uint8_t> Nb;
        const int reason = ellp::map_start(*sf, start_basis(start), B, N, Nb);
        if (reason != ellp::START_USED) return reason;
        if (capacity < *cols) return ELLP_ERR_ARG;
        if (B_out) std::memcpy(B_out, B.data(), sizeof(int64_t) * B.size());
        if (N_out) std::memcpy(N_out, N.data(), sizeof(int64_t) * N.size());
        if (Nb_out) std::memcpy(Nb_out, Nb.data(), Nb.size());
        return 0;
    } catch (const std::exception &) {
        return ELLP_ERR_PANIC;
    }
}

void ellp_result_rng_free(ellp_result_rng *r) {
    if (!r) return;
    ellp_result_ex_free(&r->ex);
    delete[] r->cost_down; delete[] r->cost_up; delete[] r->cost_blocking_down; delete[] r->cost_blocking_up;
    delete[] r->rhs_down; delete[] r->rhs_up; delete[] r->rhs_blocking_down; delete[] r->rhs_blocking_up;
    delete[] r->B_index; delete[] r->N_index; delete[] r->row_origin; delete[] r->N_bound; delete[] r->x_std;
    r->cost_down = r->cost_up = r->rhs_down = r->rhs_up = r->x_std = nullptr;
    r->cost_blocking_down = r->cost_blocking_up = r->rhs_blocking_down = r->rhs_blocking_up = r->B_index = r->N_index = r->row_origin = nullptr;
    r->N_bound = nullptr;
}

void ellp_result_ex_free(ellp_result_ex *r) {
    if (!r) return;
    ellp_result_free(&r->result);
    delete[] r->duals;
    delete[] r->reduced_costs;
    r->duals = r->reduced_costs = nullptr;
}

int ellp_solve_batch(const ellp_problem *const *probs, int64_t count, int solver, uint64_t max_iter, const ellp_opts *opts,
                     ellp_result *out) {
    if (count < 0 || (count > 0 && (!probs || !out)) || (solver != ELLP_SOLVER_PRIMAL && solver != ELLP_SOLVER_DUAL))
        return ELLP_ERR_ARG;
    for (int64_t k = 0; k < count; ++k)
        if (!probs[k]) return ELLP_ERR_ARG;
    std::vector<ellp::Problem> ps;
    ps.reserve(static_cast<size_t>(count));
    for (int64_t k = 0; k < count; ++k) ps.push_back(probs[k]->prob);
    std::vector<ellp::BatchOutcome> res;
    try {
        res = ellp::solve_batch(solver, std::move(ps), max_iter, engine_options(opts));
    } catch (const std::exception &e) {  // host memory: the batch as a whole
        for (int64_t k = 0; k < count; ++k) {
            std::memset(&out[k], 0, sizeof(out[k]));
            out[k].status = ELLP_ERR_DEVICE;
            put(out[k].err, sizeof(out[k].err), e.what());
        }
        return ELLP_ERR_DEVICE;
    }
    for (int64_t k = 0; k < count; ++k)
        fill_result(&out[k], [&] {
            if (res[k].error) std::rethrow_exception(res[k].error);
            return std::move(res[k].result);
        });
    return ELLP_OPTIMAL;
}

int ellp_solve_batch_ex(const ellp_problem *const *probs, int64_t count, int solver, uint64_t max_iter, const ellp_opts *opts,
                        int postsolve, ellp_result_ex *out) {
    if (count < 0 || (count > 0 && (!probs || !out)) || (solver != ELLP_SOLVER_PRIMAL && solver != ELLP_SOLVER_DUAL))
        return ELLP_ERR_ARG;
    for (int64_t k = 0; k < count; ++k)
        if (!probs[k]) return ELLP_ERR_ARG;
    std::vector<ellp::Problem> ps;
    ps.reserve(static_cast<size_t>(count));
    for (int64_t k = 0; k < count; ++k) ps.push_back(probs[k]->prob);
    std::vector<ellp::BatchOutcome> res;
    for (int64_t k = 0; k < count; ++k) std::memset(&out[k], 0, sizeof(out[k]));
    try {
        res = ellp::solve_batch(solver, std::move(ps), max_iter, engine_options(opts), postsolve != 0);
    } catch (const std::exception &e) {  // host memory: the batch as a whole
        for (int64_t k = 0; k < count; ++k) {
            out[k].result.status = ELLP_ERR_DEVICE;
            put(out[k].result.err, sizeof(out[k].result.err), e.what());
        }
        return ELLP_ERR_DEVICE;
    }
    for (int64_t k = 0; k < count; ++k) {
        ellp_result base;
        fill_result(&base, [&] {
            if (res[k].error) std::rethrow_exception(res[k].error);
            return std::move(res[k].result);
        }, &out[k]);
        out[k].result = base;
    }
    return ELLP_OPTIMAL;
}

// ellp_solve_batch_start and ellp_solve_batch_flags after their checks: starts and reports may be NULL (no starts)
static int solve_batch_rng(const ellp_problem *const *probs, int64_t count, int solver, uint64_t max_iter, const ellp_opts *opts,
                           unsigned flags, const ellp_start *const *starts, ellp_result_rng *out, ellp_start_report *reports) {
    for (int64_t k = 0; k < count; ++k) {
        std::memset(&out[k], 0, sizeof(out[k]));
        if (reports) std::memset(&reports[k], 0, sizeof(reports[k]));
    }
    std::vector<ellp::Problem> ps;
    ps.reserve(static_cast<size_t>(count));
    std::vector<ellp::StartBasis> sb(static_cast<size_t>(count));
    std::vector<const ellp::StartBasis *> sp(static_cast<size_t>(count), nullptr);
    std::vector<ellp::StartReport> rep;
    std::vector<ellp::BatchOutcome> res;
    try {
        for (int64_t k = 0; k < count; ++k) {
            ps.push_back(probs[k]->prob);
            if (starts && starts[k]) {
                sb[static_cast<size_t>(k)] = start_basis(starts[k]);
                sp[static_cast<size_t>(k)] = &sb[static_cast<size_t>(k)];
            }
        }
        res = ellp::solve_batch(solver, std::move(ps), max_iter, engine_options(opts), (flags & ELLP_SOLVE_POSTSOLVE) != 0,
                                starts ? &sp : nullptr, starts ? &rep : nullptr, (flags & ELLP_SOLVE_RANGING) != 0);
    } catch (const std::exception &e) {  // host memory: the batch as a whole
        for (int64_t k = 0; k < count; ++k) {
            out[k].ex.result.status = ELLP_ERR_DEVICE;
            put(out[k].ex.result.err, sizeof(out[k].ex.result.err), e.what());
        }
        return ELLP_ERR_DEVICE;
    }
    for (int64_t k = 0; k < count; ++k) {
        ellp_result base;
        fill_result(&base, [&] {
            if (res[k].error) std::rethrow_exception(res[k].error);
            return std::move(res[k].result);
        }, &out[k].ex, &out[k], /*basis_always=*/true);
        out[k].ex.result = base;
        if (reports && starts) {
            reports[k].used = rep[static_cast<size_t>(k)].used ? 1 : 0;
            reports[k].reason = rep[static_cast<size_t>(k)].reason;
            reports[k].info = rep[static_cast<size_t>(k)].info;
        }
    }
    return ELLP_OPTIMAL;
}

int ellp_solve_batch_start(const ellp_problem *const *probs, int64_t count, int solver, uint64_t max_iter, const ellp_opts *opts,
                           unsigned flags, const ellp_start *const *starts, ellp_result_rng *out, ellp_start_report *reports) {
    if (count < 0 || !probs || !starts || !out || !reports || (solver != ELLP_SOLVER_PRIMAL && solver != ELLP_SOLVER_DUAL) ||
        (flags & ~ELLP_SOLVE_POSTSOLVE))  // ELLP_SOLVE_RANGING too: that is ellp_solve_batch_flags
        return ELLP_ERR_ARG;
    for (int64_t k = 0; k < count; ++k)
        if (!probs[k]) return ELLP_ERR_ARG;
    return solve_batch_rng(probs, count, solver, max_iter, opts, flags, starts, out, reports);
}

int ellp_solve_batch_flags(const ellp_problem *const *probs, int64_t count, int solver, uint64_t max_iter, const ellp_opts *opts,
                           unsigned flags, const ellp_start *const *starts, ellp_result_rng *out, ellp_start_report *reports) {
    if (count < 0 || !probs || !out || (starts && !reports) || (solver != ELLP_SOLVER_PRIMAL && solver != ELLP_SOLVER_DUAL) ||
        (flags & ~(ELLP_SOLVE_POSTSOLVE | ELLP_SOLVE_RANGING)))
        return ELLP_ERR_ARG;
    for (int64_t k = 0; k < count; ++k)
        if (!probs[k]) return ELLP_ERR_ARG;
    return solve_batch_rng(probs, count, solver, max_iter, opts, flags, starts, out, reports);
}

static void fill_flat(ellp_flat_phase *o, const ellp::StandardForm &sf, const ellp::Point &pt,
                      const std::vector<double> *y, const std::vector<double> *d) {
    auto dupd = [](const std::vector<double> &v) {
        double *p = new double[v.size() ? v.size() : 1];
        std::memcpy(p, v.data(), sizeof(double) * v.size());
        return p;
    };
    o->m = static_cast<int64_t>(sf.rows());
    o->n = static_cast<int64_t>(sf.cols());
    o->n_c = static_cast<int64_t>(sf.bounds.size());
    o->n_B = static_cast<int64_t>(pt.B.size());
    o->n_N = static_cast<int64_t>(pt.N.size());
    o->A = dupd(sf.A.a);
    o->c = dupd(sf.c);
    o->b = dupd(sf.b);
    o->x = dupd(pt.x);
    std::vector<double> lb, ub;
    o->bound_kind = new uint8_t[sf.bounds.size() ? sf.bounds.size() : 1];
    for (size_t i = 0; i < sf.bounds.size(); ++i) {
        o->bound_kind[i] = static_cast<uint8_t>(sf.bounds[i].kind);
        lb.push_back(sf.bounds[i].lb);
        ub.push_back(sf.bounds[i].kind == ellp::Bound::Fixed ? sf.bounds[i].lb : sf.bounds[i].ub);
    }
    o->lb = dupd(lb);
    o->ub = dupd(ub);
    o->B_index = new int64_t[pt.B.size() ? pt.B.size() : 1];
    for (size_t i = 0; i < pt.B.size(); ++i) o->B_index[i] = static_cast<int64_t>(pt.B[i].index);
    o->N_index = new int64_t[pt.N.size() ? pt.N.size() : 1];
    o->N_bound = new uint8_t[pt.N.size() ? pt.N.size() : 1];
    for (size_t j = 0; j < pt.N.size(); ++j) {
        o->N_index[j] = static_cast<int64_t>(pt.N[j].index);
        o->N_bound[j] = static_cast<uint8_t>(pt.N[j].bound);
    }
    o->y = y ? dupd(*y) : nullptr;
    o->d = d ? dupd(*d) : nullptr;
}

int ellp_debug_phase1(const ellp_problem *p, int solver, ellp_flat_phase *out, char *errbuf, size_t errlen) {
    std::memset(out, 0, sizeof(*out));
    try {
        if (solver == ELLP_SOLVER_PRIMAL) {
            auto ph = ellp::PrimalPhase1::from_problem(p->prob);
            if (!ph) return 1;
            fill_flat(out, ph->std_form, ph->point, nullptr, nullptr);
        } else {
            auto ph = ellp::DualPhase1::from_problem(p->prob);
            if (!ph) return 1;
            fill_flat(out, ph->std_form, ph->point.point, &ph->point.y, &ph->point.d);
        }
        return 0;
    } catch (const std::exception &e) {
        put(errbuf, errlen, e.what());
        return ELLP_ERR_PANIC;
    }
}

void ellp_flat_phase_free(ellp_flat_phase *f) {
    if (!f) return;
    delete[] f->A; delete[] f->c; delete[] f->b; delete[] f->lb; delete[] f->ub; delete[] f->x;
    delete[] f->y; delete[] f->d; delete[] f->bound_kind; delete[] f->N_bound;
    delete[] f->B_index; delete[] f->N_index;
    std::memset(f, 0, sizeof(*f));
}

void ellp_result_free(ellp_result *r) {
    if (r && r->x) {
        delete[] r->x;
        r->x = nullptr;
    }
}

}  // extern "C"

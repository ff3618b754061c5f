// solvers.cpp — PrimalSimplexSolver / DualSimplexSolver drivers.
//   solve():                primal_simplex_solver.rs:32-93, dual_simplex_solver.rs:33-108 (host)
//   solve_with_initial():   the seam.  Checks that stay on the host are the ones the reference
//                           does before its loop (m == 0 -> trivial solver); everything else is
//                           one call through the C ABI into the HIP engine.  No CPU loop exists
//                           here: if the engine cannot run, the error is raised.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <exception>
#include <limits>
#include <stdexcept>
#include <type_traits>

#include "ellp.h"

#include <cstdlib>

namespace ellp {

namespace {

struct Flat {
    std::vector<std::uint8_t> kind;
    std::vector<double> lb, ub;
    std::vector<std::int64_t> B, N;
    std::vector<std::uint8_t> Nb;
};

Flat flatten(const StandardForm &sf, const Point &pt) {
    Flat f;
    const size_t nc = sf.bounds.size();
    f.kind.resize(nc);
    f.lb.resize(nc);
    f.ub.resize(nc);
    for (size_t i = 0; i < nc; ++i) {
        f.kind[i] = static_cast<std::uint8_t>(sf.bounds[i].kind);
        f.lb[i] = sf.bounds[i].lb;
        f.ub[i] = (sf.bounds[i].kind == Bound::Fixed) ? sf.bounds[i].lb : sf.bounds[i].ub;
    }
    for (const auto &b : pt.B) f.B.push_back(static_cast<std::int64_t>(b.index));
    for (const auto &n : pt.N) {
        f.N.push_back(static_cast<std::int64_t>(n.index));
        f.Nb.push_back(static_cast<std::uint8_t>(n.bound));
    }
    return f;
}

void unflatten(const Flat &f, Point &pt) {
    for (size_t i = 0; i < pt.B.size(); ++i) pt.B[i].index = static_cast<size_t>(f.B[i]);
    for (size_t j = 0; j < pt.N.size(); ++j) {
        pt.N[j].index = static_cast<size_t>(f.N[j]);
        pt.N[j].bound = static_cast<NonbasicBound>(f.Nb[j]);
    }
}

// the item of a batched call: the standard form, its flattened bounds and index sets, the point x (and y, d where the call
// reads or writes them)
ellp_batch_item batch_item_of(const StandardForm &sf, Flat &f, std::vector<double> &x, std::vector<double> *y = nullptr,
                              std::vector<double> *d = nullptr) {
    ellp_batch_item it;
    std::memset(&it, 0, sizeof(it));
    it.m = static_cast<std::int64_t>(sf.rows());
    it.n = static_cast<std::int64_t>(sf.cols());
    it.n_c = static_cast<std::int64_t>(sf.bounds.size());
    it.A = sf.A.a.data();
    it.c = sf.c.data();
    it.b = sf.b.data();
    it.bound_kind = f.kind.data();
    it.lb = f.lb.data();
    it.ub = f.ub.data();
    it.x = x.data();
    it.B_index = f.B.data();
    it.n_B = static_cast<std::int64_t>(f.B.size());
    it.N_index = f.N.data();
    it.N_bound = f.Nb.data();
    it.n_N = static_cast<std::int64_t>(f.N.size());
    if (y) it.y = y->data();
    if (d) it.d = d->data();
    return it;
}

ellp_opts make_opts(std::uint64_t max_iter, const EngineOptions &e) {
    ellp_opts o;
    ellp_default_opts(&o);
    o.max_iter = max_iter;
    o.eps = EPS;
    o.device = e.device;
    o.refactor_period = e.refactor_period;
    o.btran_mode = e.btran_mode;
    o.poll_interval = e.poll_interval;
    o.pipeline = e.pipeline;
    o.partial_segments = e.partial_segments;
    o.flags = e.flags;
    return o;
}

SolutionStatus to_status(ellp_status s, const char *err) {
    switch (s) {
    case ELLP_OPTIMAL: return SolutionStatus::Optimal;
    case ELLP_INFEASIBLE: return SolutionStatus::Infeasible;
    case ELLP_UNBOUNDED: return SolutionStatus::Unbounded;
    case ELLP_MAXITER: return SolutionStatus::MaxIter;
    case ELLP_ERR_BAD_DIMS:
    case ELLP_ERR_SINGULAR: throw EllPError(err);  // Err(EllPError), primal…:124-140, :175-179
    case ELLP_ERR_DEVICE: throw std::runtime_error(std::string("HIP engine unavailable: ") + err);
    default: throw EllPPanic(err);
    }
}

}  // namespace

// primal_simplex_solver.rs:95-236
SolutionStatus PrimalSimplexSolver::solve_with_initial(const StandardForm &sf, Point &pt, std::uint64_t *iters) const {
    if (iters) *iters = 0;
    if (sf.rows() == 0) {  // :118-122
        if (!pt.B.empty()) throw EllPPanic("assertion failed: B.is_empty()");
        return solve_trivial_problem(sf, pt.x, pt.N, true);
    }
    Flat f = flatten(sf, pt);
    const ellp_opts o = make_opts(max_iter_, engine_);
    ellp_stats st{};
    char err[512] = {0};
    const ellp_status s = ellp_primal_solve_with_initial(
        static_cast<std::int64_t>(sf.rows()), static_cast<std::int64_t>(sf.cols()),
        static_cast<std::int64_t>(sf.bounds.size()), sf.A.a.data(), sf.c.data(), sf.b.data(), f.kind.data(),
        f.lb.data(), f.ub.data(), pt.x.data(), f.B.data(), static_cast<std::int64_t>(f.B.size()), f.N.data(),
        f.Nb.data(), static_cast<std::int64_t>(f.N.size()), &o, &st, err, sizeof(err));
    if (iters) *iters = st.iters;
    const SolutionStatus out = to_status(s, err);
    unflatten(f, pt);
    return out;
}

namespace {

// owns a resident engine for the two phases of one primal solve
struct EngineHandle {
    ellp_engine *e = nullptr;
    ~EngineHandle() { if (e) ellp_engine_destroy(e); }
};

// one phase on a resident engine: run, then bring the point back (x, B, N as at the seam)
SolutionStatus run_resident(ellp_engine *e, std::uint64_t max_iter, Flat &f, Point &pt, std::uint64_t *iters) {
    ellp_stats st{};
    char err[512] = {0};
    const ellp_status s = ellp_engine_run(e, max_iter, &st, err, sizeof(err));
    if (iters) *iters = st.iters;
    SolutionStatus out = to_status(s, err);
    const ellp_status rs = ellp_engine_read_point(e, pt.x.data(), f.B.data(), f.N.data(), f.Nb.data(), nullptr,
                                                  nullptr, err, sizeof(err));
    if (rs != ELLP_OPTIMAL) out = to_status(rs, err);  // an error, or the status the still open last iteration ended in
    unflatten(f, pt);
    return out;
}

// with_postsolve(true): duals, reduced costs and the KKT report of an Optimal solution.  `e`: the resident engine that ran
// phase 2 (examined where it stands, ellp_engine_postsolve); null, or an engine that call refuses (a sharded one): the
// phase-2 arrays go up once more (ellp_postsolve).
// Without rows it is answered here: y is empty and d = c.
//
// In two steps: y, d and the report of the standard form (here, or for many solutions at once by solve_batch's one
// ellp_batch_postsolve call), then map_postsolve: y to the Problem's constraints, d to its variables.
void map_postsolve(Solution &sol, const std::vector<double> &y, const std::vector<double> &d, const ellp_kkt &kkt) {
    const StandardForm &sf = sol.std_form;
    const size_t m = sf.rows(), nv = sf.prob.variables.size();
    if (sf.row_origin.size() != m) throw EllPPanic("assertion failed: std_form.row_origin.len() == std_form.rows()");
    Postsolve ps;
    ps.kkt = kkt;
    ps.duals.assign(sf.prob.constraints.size(), 0.0);
    for (size_t k = 0; k < m; ++k) ps.duals[sf.row_origin[k]] = y[k];
    ps.reduced_costs.assign(d.begin(), d.begin() + static_cast<std::ptrdiff_t>(nv));
    sol.post = std::move(ps);
}

void attach_postsolve(Solution &sol, ellp_engine *e, const EngineOptions &eng) {
    const StandardForm &sf = sol.std_form;
    const size_t m = sf.rows(), nc = sf.bounds.size();
    Postsolve ps;
    std::vector<double> y(m, 0.0), d(nc, 0.0);
    if (m == 0) {
        d = sf.c;
        ellp_kkt &k = ps.kkt;
        k.worst_row = k.worst_bound_var = k.worst_dual_var = -1;
        k.primal_obj = sf.obj(sol.point.x);
        k.dual_obj = sf.dual_obj(y, d);
        for (size_t v = 0; v < nc; ++v) {
            const Bound &bd = sf.bounds[v];
            const double xv = sol.point.x[v];
            double viol = 0.0;
            switch (bd.kind) {
            case Bound::Free: break;
            case Bound::Lower: viol = bd.lb - xv; break;
            case Bound::Upper: viol = xv - bd.ub; break;
            case Bound::TwoSided: viol = std::max(bd.lb - xv, xv - bd.ub); break;
            case Bound::Fixed: viol = std::fabs(xv - bd.lb); break;
            }
            if (viol > k.bound_violation) {
                k.bound_violation = viol;
                k.worst_bound_var = static_cast<std::int64_t>(v);
            }
        }
        for (const Nonbasic &nb : sol.point.N) {
            const double dv = d[nb.index];
            double inf;
            if (sf.bounds[nb.index].kind == Bound::Fixed) inf = 0.0;
            else if (nb.bound == NonbasicBound::Lower) inf = -dv;
            else if (nb.bound == NonbasicBound::Upper) inf = dv;
            else inf = std::fabs(dv);
            if (inf > k.dual_infeasibility) {
                k.dual_infeasibility = inf;
                k.worst_dual_var = static_cast<std::int64_t>(nb.index);
            }
        }
    } else {
        char err[512] = {0};
        ellp_status s = ELLP_ERR_ARG;
        if (e) s = ellp_engine_postsolve(e, y.data(), d.data(), nullptr, &ps.kkt, err, sizeof(err));
        if (s == ELLP_ERR_ARG) {
            // no resident engine, or one the postsolve refuses (a sharded engine): the phase-2 arrays go up once more
            Flat f = flatten(sf, sol.point);
            const ellp_opts o = make_opts(0, eng);
            s = ellp_postsolve(static_cast<std::int64_t>(m), static_cast<std::int64_t>(sf.cols()), static_cast<std::int64_t>(nc),
                               sf.A.a.data(), sf.c.data(), sf.b.data(), f.kind.data(), f.lb.data(), f.ub.data(), sol.point.x.data(),
                               f.B.data(), static_cast<std::int64_t>(f.B.size()), f.N.data(), f.Nb.data(),
                               static_cast<std::int64_t>(f.N.size()), &o, y.data(), d.data(), nullptr, &ps.kkt, err, sizeof(err));
        }
        if (s != ELLP_OPTIMAL) to_status(s, err);  // throws: a singular basis is an EllPError, a refusal of the arrays a panic
    }
    map_postsolve(sol, y, d, ps.kkt);
}

// The arrays of one ranging of a standard form, as ellp_ranging_out names them: filled by a ranging call (attach_ranging, or
// for many solutions at once by solve_batch's one ellp_batch_ranging call), then mapped to the Problem by map_ranging
struct RangeArrays {
    std::vector<double> cd, cu, rd, ru, y, d;
    std::vector<std::int64_t> cbd, cbu, rbd, rbu;
    ellp_ranging_info info{};
    RangeArrays(size_t m, size_t nc)
        : cd(nc, -std::numeric_limits<double>::infinity()), cu(nc, std::numeric_limits<double>::infinity()), rd(m, 0.0), ru(m, 0.0),
          y(m, 0.0), d(nc, 0.0), cbd(nc, -1), cbu(nc, -1), rbd(m, -1), rbu(m, -1) {}
    ellp_ranging_out out() {
        ellp_ranging_out o{};
        o.cost_down = cd.data(); o.cost_up = cu.data(); o.cost_blocking_down = cbd.data(); o.cost_blocking_up = cbu.data();
        o.rhs_down = rd.data(); o.rhs_up = ru.data(); o.rhs_blocking_down = rbd.data(); o.rhs_blocking_up = rbu.data();
        o.info = &info;
        o.y = y.data(); o.d = d.data();
        return o;
    }
};

// ra to the Problem's variables and constraints: the costs of the first nv columns, the rows by row_origin, a dropped row
// (0.0, 0.0, -1).  With rows the ranging's own y, d and report become the Solution's postsolve (no second LU)
void map_ranging(Solution &sol, const RangeArrays &ra) {
    const StandardForm &sf = sol.std_form;
    const size_t m = sf.rows(), nv = sf.prob.variables.size();
    Ranging rg;
    if (m > 0) {
        rg.inverse_residual = ra.info.inverse_residual;
        map_postsolve(sol, ra.y, ra.d, ra.info.kkt);
    }
    if (sf.row_origin.size() != m) throw EllPPanic("assertion failed: std_form.row_origin.len() == std_form.rows()");
    const auto head = [nv](const auto &v) { return std::decay_t<decltype(v)>(v.begin(), v.begin() + static_cast<std::ptrdiff_t>(nv)); };
    rg.cost_down = head(ra.cd); rg.cost_up = head(ra.cu); rg.cost_blocking_down = head(ra.cbd); rg.cost_blocking_up = head(ra.cbu);
    const size_t ncon = sf.prob.constraints.size();
    rg.rhs_down.assign(ncon, 0.0); rg.rhs_up.assign(ncon, 0.0); rg.rhs_blocking_down.assign(ncon, -1); rg.rhs_blocking_up.assign(ncon, -1);
    for (size_t k = 0; k < m; ++k) {
        const size_t o = sf.row_origin[k];
        rg.rhs_down[o] = ra.rd[k]; rg.rhs_up[o] = ra.ru[k]; rg.rhs_blocking_down[o] = ra.rbd[k]; rg.rhs_blocking_up[o] = ra.rbu[k];
    }
    sol.rng = std::move(rg);
}

// with_ranging(true): the cost and right-hand-side ranges of an Optimal solution, from the engine that ran phase 2 where there
// is one and it takes the call (ellp_engine_ranging), else from phase 2's arrays (ellp_ranging).  The ranging runs the
// postsolve itself, so its y, d and report are taken from the same call and become the Solution's postsolve (no second LU).
// Without rows both are answered here: every variable is nonbasic with d = c, and there is no right-hand side.
void attach_ranging(Solution &sol, ellp_engine *e, const EngineOptions &eng) {
    const StandardForm &sf = sol.std_form;
    const size_t m = sf.rows(), nc = sf.bounds.size();
    const double inf = std::numeric_limits<double>::infinity();
    RangeArrays ra(m, nc);
    if (m == 0) {
        attach_postsolve(sol, e, eng);
        for (const Nonbasic &nb : sol.point.N) {
            const size_t v = nb.index;
            const double dv = sf.c[v];
            if (sf.bounds[v].kind == Bound::Fixed) continue;
            if (nb.bound == NonbasicBound::Lower) ra.cd[v] = 0.0 - std::max(dv, 0.0);
            else if (nb.bound == NonbasicBound::Upper) ra.cu[v] = 0.0 - std::min(dv, 0.0);
            else {
                ra.cu[v] = std::max(-dv, 0.0) + 0.0;
                ra.cd[v] = std::min(-dv, 0.0) + 0.0;
            }
            if (ra.cd[v] != -inf) ra.cbd[v] = static_cast<std::int64_t>(v);
            if (ra.cu[v] != inf) ra.cbu[v] = static_cast<std::int64_t>(v);
        }
    } else {
        char err[512] = {0};
        ellp_ranging_out out = ra.out();
        ellp_status s = ELLP_ERR_ARG;
        if (e) s = ellp_engine_ranging(e, &out, err, sizeof(err));
        if (s == ELLP_ERR_ARG) {
            Flat f = flatten(sf, sol.point);
            const ellp_opts o = make_opts(0, eng);
            s = ellp_ranging(static_cast<std::int64_t>(m), static_cast<std::int64_t>(sf.cols()), static_cast<std::int64_t>(nc), sf.A.a.data(),
                             sf.c.data(), sf.b.data(), f.kind.data(), f.lb.data(), f.ub.data(), sol.point.x.data(), f.B.data(),
                             static_cast<std::int64_t>(f.B.size()), f.N.data(), f.Nb.data(), static_cast<std::int64_t>(f.N.size()), &o, &out,
                             err, sizeof(err));
        }
        if (s != ELLP_OPTIMAL) to_status(s, err);  // throws, as attach_postsolve
    }
    map_ranging(sol, ra);
}

// with_certificate(true): no certificate, and why (reason: one of the cases of DESIGN.md §3.12)
void no_certificate(SolverResult &res, const char *reason) {
    Certificate c;
    c.reason = reason;
    res.cert = std::move(c);
}

// with_certificate(true): the Farkas vector or the ray of the basis, labels and point (sf, pt) an Infeasible / Unbounded ending
// stands on, from the resident engine where there is one and it takes the call, else from the arrays (as attach_postsolve).
// n_check leading columns are verified against chk (null: sf's own bounds).  The vector goes to the Problem: a Farkas y to the
// constraints by row_origin (a dropped row: 0.0), a ray to the variables.  A basis the device calls singular, or a NaN, gives
// no certificate and says so in reason; the result itself stays what it was.
void attach_certificate(SolverResult &res, const StandardForm &sf, const Point &pt, ellp_engine *e, const EngineOptions &eng, int source,
                        size_t n_check, const std::vector<Bound> *chk, const char *reason) {
    const size_t m = sf.rows(), nc = sf.bounds.size();
    if (m == 0) return no_certificate(res, "no rows: decided by the trivial solver");
    Certificate c;
    std::vector<double> vec(source == ELLP_CERT_RAY_COLUMN ? n_check : m, 0.0), clb, cub;
    std::vector<std::uint8_t> ckind;
    if (chk) {
        for (size_t i = 0; i < n_check; ++i) {
            const Bound &bd = (*chk)[i];
            ckind.push_back(static_cast<std::uint8_t>(bd.kind));
            clb.push_back(bd.lb);
            cub.push_back(bd.kind == Bound::Fixed ? bd.lb : bd.ub);
        }
    }
    char err[512] = {0};
    ellp_status s = ELLP_ERR_ARG;
    const std::int64_t nchk = static_cast<std::int64_t>(n_check);
    if (e) s = ellp_engine_certificate(e, source, nchk, chk ? ckind.data() : nullptr, chk ? clb.data() : nullptr, chk ? cub.data() : nullptr,
                                       vec.data(), &c.info, err, sizeof(err));
    if (s == ELLP_ERR_ARG) {  // no resident engine, or one the call refuses: the arrays go up once more
        Flat f = flatten(sf, pt);
        const ellp_opts o = make_opts(0, eng);
        s = ellp_certificate(static_cast<std::int64_t>(m), static_cast<std::int64_t>(sf.cols()), static_cast<std::int64_t>(nc), sf.A.a.data(),
                             sf.c.data(), sf.b.data(), f.kind.data(), f.lb.data(), f.ub.data(), pt.x.data(), f.B.data(),
                             static_cast<std::int64_t>(f.B.size()), f.N.data(), f.Nb.data(), static_cast<std::int64_t>(f.N.size()), &o, source, nchk,
                             chk ? ckind.data() : nullptr, chk ? clb.data() : nullptr, chk ? cub.data() : nullptr, vec.data(), &c.info, err,
                             sizeof(err));
    }
    if (s == ELLP_ERR_SINGULAR || s == ELLP_ERR_NAN) return no_certificate(res, s == ELLP_ERR_NAN ? "the certificate call met a NaN" : "the certificate call found the basis singular");
    if (s != ELLP_OPTIMAL) to_status(s, err);  // throws: no device, or arrays the call refuses
    if (!c.info.found) return no_certificate(res, "search found none");
    c.reason = reason;
    if (source == ELLP_CERT_RAY_COLUMN) {
        c.kind = Certificate::Ray;
        const size_t nv = sf.prob.variables.size();
        c.vec.assign(nv, 0.0);
        for (size_t v = 0; v < nv && v < n_check; ++v) c.vec[v] = vec[v];
    } else {
        c.kind = Certificate::Farkas;
        if (sf.row_origin.size() != m) throw EllPPanic("assertion failed: std_form.row_origin.len() == std_form.rows()");
        c.vec.assign(sf.prob.constraints.size(), 0.0);
        for (size_t k = 0; k < m; ++k) c.vec[sf.row_origin[k]] = vec[k];
    }
    res.cert = std::move(c);
}

// the bounds of StandardForm::from_problem behind a primal phase-1 form: the Problem's own on its variables (phase 1 fixes
// dependent free ones at 0), the form's on the slacks
std::vector<Bound> original_bounds(const StandardForm &sf, size_t n_orig) {
    std::vector<Bound> out(sf.bounds.begin(), sf.bounds.begin() + static_cast<std::ptrdiff_t>(n_orig));
    for (size_t i = 0; i < sf.prob.variables.size() && i < n_orig; ++i) out[i] = sf.prob.variables[i].bound;
    return out;
}

}  // namespace

// primal_simplex_solver.rs:32-93.  The two solve_with_initial calls of the reference become two
// slices of ONE resident engine: after phase 1 only the costs and bounds are replaced on the
// device (ellp_engine_rephase, primal_problem.rs:263-291) — the matrix, the basis and B^-1 stay in
// HBM.  Problems the seam never sends to the device (m == 0, no nonbasic column) take the plain path.
SolverResult PrimalSimplexSolver::solve(Problem prob) const {
    SolverResult res;
    auto p1 = PrimalPhase1::from_problem(std::move(prob));
    if (!p1) {
        res.kind = SolverResult::Infeasible;
        if (certificate_) no_certificate(res, "infeasibility decided by the set-up");
        return res;
    }
    PrimalPhase1 phase_1 = std::move(*p1);
    const bool resident = phase_1.std_form.rows() > 0 && !phase_1.point.N.empty();
    // the columns of StandardForm::from_problem: the phase-1 columns stand behind them
    const size_t n_orig = phase_1.phase_1_vars.empty() ? phase_1.std_form.bounds.size() : phase_1.phase_1_vars.front();
    EngineHandle eng;
    Flat f1;
    SolutionStatus s1;
    if (resident) {
        f1 = flatten(phase_1.std_form, phase_1.point);
        const StandardForm &sf = phase_1.std_form;
        const ellp_opts o = make_opts(max_iter_, engine_);
        char err[512] = {0};
        const ellp_status cs = ellp_engine_create(
            ELLP_ENGINE_PRIMAL, static_cast<std::int64_t>(sf.rows()), static_cast<std::int64_t>(sf.cols()),
            static_cast<std::int64_t>(sf.bounds.size()), sf.A.a.data(), sf.c.data(), sf.b.data(), f1.kind.data(),
            f1.lb.data(), f1.ub.data(), phase_1.point.x.data(), f1.B.data(), static_cast<std::int64_t>(f1.B.size()),
            f1.N.data(), f1.Nb.data(), static_cast<std::int64_t>(f1.N.size()), nullptr, nullptr, &o, &eng.e, err,
            sizeof(err));
        if (cs != ELLP_OPTIMAL) to_status(cs, err);  // throws: Err(EllPError) / panic / device
        s1 = run_resident(eng.e, max_iter_, f1, phase_1.point, &res.iters_phase1);
    } else {
        s1 = solve_with_initial(phase_1.std_form, phase_1.point, &res.iters_phase1);
    }
    switch (s1) {
    case SolutionStatus::Optimal: {
        const double obj = phase_1.obj();
        if (!(obj > -EPS)) throw EllPPanic("assertion failed: obj > -EPS");
        if (!(obj < EPS)) {
            res.kind = SolverResult::Infeasible;
            if (certificate_) {  // phase-1 costs are zero on the problem's columns: y = B^-T c_B is the proof
                const std::vector<Bound> chk = original_bounds(phase_1.std_form, n_orig);
                attach_certificate(res, phase_1.std_form, phase_1.point, resident ? eng.e : nullptr, engine_, ELLP_CERT_FARKAS_COSTS, n_orig, &chk,
                                   "primal phase 1 optimal with a positive objective");
            }
            return res;
        }
        break;
    }
    case SolutionStatus::Infeasible:
        res.kind = SolverResult::Infeasible;
        if (certificate_) no_certificate(res, "primal phase 1 ended with a loop status");
        return res;
    case SolutionStatus::Unbounded: throw EllPPanic("primal phase 1 should never be unbounded");
    case SolutionStatus::MaxIter:
        res.kind = SolverResult::MaxIter;
        res.max_iter_obj = std::numeric_limits<double>::infinity();
        if (certificate_) no_certificate(res, "MaxIter");
        return res;
    }
    PrimalPhase2 phase_2 = PrimalPhase2::from_phase1(std::move(phase_1));
    SolutionStatus s2;
    if (resident) {
        Flat f2 = flatten(phase_2.std_form, phase_2.point);
        char err[512] = {0};
        const ellp_status rs = ellp_engine_rephase(eng.e, phase_2.std_form.c.data(), f2.kind.data(), f2.lb.data(),
                                                   f2.ub.data(), err, sizeof(err));
        if (rs != ELLP_OPTIMAL) to_status(rs, err);
        s2 = run_resident(eng.e, max_iter_, f2, phase_2.point, &res.iters_phase2);
    } else {
        s2 = solve_with_initial(phase_2.std_form, phase_2.point, &res.iters_phase2);
    }
    switch (s2) {
    case SolutionStatus::Optimal:
        res.kind = SolverResult::Optimal;
        res.solution = Solution{std::move(phase_2.std_form), std::move(phase_2.point), std::nullopt, std::nullopt};
        if (ranging_) attach_ranging(*res.solution, resident ? eng.e : nullptr, engine_);  // the engine that ran phase 2, before it goes
        else if (postsolve_) attach_postsolve(*res.solution, resident ? eng.e : nullptr, engine_);
        if (certificate_) no_certificate(res, "Optimal");
        return res;
    case SolutionStatus::Infeasible: throw EllPPanic("primal phase 2 should never be infeasible");
    case SolutionStatus::Unbounded:
        res.kind = SolverResult::Unbounded;
        if (certificate_)
            attach_certificate(res, phase_2.std_form, phase_2.point, resident ? eng.e : nullptr, engine_, ELLP_CERT_RAY_COLUMN, n_orig, nullptr,
                               "primal phase 2 unbounded");
        return res;
    case SolutionStatus::MaxIter:
        res.kind = SolverResult::MaxIter;
        res.max_iter_obj = phase_2.obj();
        if (certificate_) no_certificate(res, "MaxIter");
        return res;
    }
    return res;
}

// dual_simplex_solver.rs:110-335
SolutionStatus DualSimplexSolver::solve_with_initial(const StandardForm &sf, DualFeasiblePoint &dp,
                                                     std::uint64_t *iters) const {
    if (iters) *iters = 0;
    Point &pt = dp.point;
    if (sf.rows() == 0) {  // :132-136
        if (!pt.B.empty()) throw EllPPanic("assertion failed: B.is_empty()");
        return solve_trivial_problem(sf, pt.x, pt.N, true);
    }
    Flat f = flatten(sf, pt);
    const ellp_opts o = make_opts(max_iter_, engine_);
    ellp_stats st{};
    char err[512] = {0};
    const ellp_status s = ellp_dual_solve_with_initial(
        static_cast<std::int64_t>(sf.rows()), static_cast<std::int64_t>(sf.cols()),
        static_cast<std::int64_t>(sf.bounds.size()), sf.A.a.data(), sf.c.data(), sf.b.data(), f.kind.data(),
        f.lb.data(), f.ub.data(), pt.x.data(), f.B.data(), static_cast<std::int64_t>(f.B.size()), f.N.data(),
        f.Nb.data(), static_cast<std::int64_t>(f.N.size()), dp.y.data(), dp.d.data(), &o, &st, err, sizeof(err));
    if (iters) *iters = st.iters;
    const SolutionStatus out = to_status(s, err);
    unflatten(f, pt);
    return out;
}

namespace {
// one phase of the dual method on a resident engine: run, bring the point and the duals back
SolutionStatus run_resident_dual(ellp_engine *e, std::uint64_t max_iter, Flat &f, DualFeasiblePoint &dp, std::uint64_t *iters) {
    ellp_stats st{};
    char err[512] = {0};
    const ellp_status s = ellp_engine_run(e, max_iter, &st, err, sizeof(err));
    if (iters) *iters = st.iters;
    SolutionStatus out = to_status(s, err);
    const ellp_status rs = ellp_engine_read_point(e, dp.point.x.data(), f.B.data(), f.N.data(), f.Nb.data(), dp.y.data(),
                                                  dp.d.data(), err, sizeof(err));
    if (rs != ELLP_OPTIMAL) out = to_status(rs, err);
    unflatten(f, dp.point);
    return out;
}
}  // namespace

// dual_simplex_solver.rs:33-108.  Where the engine is of the explicit-inverse kind (m > 128) and the box
// problem of phase 1 has the original standard form's matrix (no TwoSided / Fixed variable was dropped,
// dual_problem.rs:96-112), the two solve_with_initial calls are two slices of ONE resident engine:
// DualPhase2::from(phase_1) (dual_problem.rs:258-404) is done on the device from the resident B^-1
// (ellp_engine_dual_rephase) — the matrix is uploaded once and no LU is computed on the host.
SolverResult DualSimplexSolver::solve(Problem prob) const {
    SolverResult res;
    Problem orig_for_fallback = prob;  // phase_1.into_orig_prob()
    // ELLP_HOST_DUAL_POINT=1 (diagnostics): the starting point of phase 1 is made on the host, as the reference makes it
    const char *hostpt = std::getenv("ELLP_HOST_DUAL_POINT");
    auto p1 = DualPhase1::from_problem(std::move(prob), /*defer_point=*/!(hostpt && hostpt[0] == '1'));
    if (!p1) {
        res.kind = SolverResult::Infeasible;
        if (certificate_) no_certificate(res, "infeasibility decided by the set-up");
        return res;
    }
    DualPhase1 phase_1 = std::move(*p1);
    const StandardForm &sf1 = phase_1.std_form;
    const bool deferred = phase_1.point_deferred;  // rows > 128, N not empty: the device makes y, d, x (:162-214)
    const bool resident = sf1.rows() > 128 && !phase_1.point.point.N.empty() &&
                          sf1.rows() == phase_1.orig_std_form.rows() && sf1.cols() == phase_1.orig_std_form.cols() &&
                          sf1.bounds.size() == phase_1.orig_std_form.bounds.size() && sf1.A.a == phase_1.orig_std_form.A.a;
    EngineHandle eng;
    SolutionStatus s1;
    if (deferred) {
        Flat f1 = flatten(sf1, phase_1.point.point);
        const ellp_opts o = make_opts(max_iter_, engine_);
        char err[512] = {0};
        const ellp_status cs = ellp_engine_create_dual_phase1(
            static_cast<std::int64_t>(sf1.rows()), static_cast<std::int64_t>(sf1.cols()), sf1.A.a.data(), sf1.c.data(),
            sf1.b.data(), f1.kind.data(), f1.lb.data(), f1.ub.data(), f1.B.data(), f1.N.data(), &o, &eng.e, err,
            sizeof(err));
        if (cs != ELLP_OPTIMAL) to_status(cs, err);
        s1 = run_resident_dual(eng.e, max_iter_, f1, phase_1.point, &res.iters_phase1);
    } else if (resident) {
        Flat f1 = flatten(sf1, phase_1.point.point);
        const ellp_opts o = make_opts(max_iter_, engine_);
        char err[512] = {0};
        const ellp_status cs = ellp_engine_create(
            ELLP_ENGINE_DUAL, static_cast<std::int64_t>(sf1.rows()), static_cast<std::int64_t>(sf1.cols()),
            static_cast<std::int64_t>(sf1.bounds.size()), sf1.A.a.data(), sf1.c.data(), sf1.b.data(), f1.kind.data(),
            f1.lb.data(), f1.ub.data(), phase_1.point.point.x.data(), f1.B.data(), static_cast<std::int64_t>(f1.B.size()),
            f1.N.data(), f1.Nb.data(), static_cast<std::int64_t>(f1.N.size()), phase_1.point.y.data(),
            phase_1.point.d.data(), &o, &eng.e, err, sizeof(err));
        if (cs != ELLP_OPTIMAL) to_status(cs, err);
        s1 = run_resident_dual(eng.e, max_iter_, f1, phase_1.point, &res.iters_phase1);
    } else {
        s1 = solve_with_initial(phase_1.std_form, phase_1.point, &res.iters_phase1);
    }
    switch (s1) {
    case SolutionStatus::Optimal: {
        const double obj = phase_1.obj();
        if (!(obj < EPS)) throw EllPPanic("assertion failed: obj < EPS");
        if (!(obj > -EPS)) {
            // dual infeasible: classify with the primal solver, default max_iter (dual…:51-66)
            SolverResult r = PrimalSimplexSolver().with_engine(engine_).with_certificate(certificate_).solve(std::move(orig_for_fallback));
            if (r.kind == SolverResult::Optimal)
                throw EllPPanic("assertion failed: matches!(result, Infeasible | Unbounded | MaxIter)");
            return r;
        }
        break;
    }
    case SolutionStatus::Infeasible: throw EllPPanic("dual phase 1 should never be infeasible");
    case SolutionStatus::Unbounded: throw EllPPanic("dual phase 1 should never be unbounded");
    case SolutionStatus::MaxIter:
        res.kind = SolverResult::MaxIter;
        res.max_iter_obj = std::numeric_limits<double>::infinity();
        if (certificate_) no_certificate(res, "MaxIter");
        return res;
    }
    DualPhase2 phase_2;
    SolutionStatus s2;
    if (resident) {
        phase_2 = DualPhase2::shell_from_phase1(std::move(phase_1));
        Flat f2 = flatten(phase_2.std_form, phase_2.point.point);
        char err[512] = {0};
        // an engine that runs whole iterations inside one persistent launch (m <= 128, pipeline 3, or a certified-hybrid engine
        // that has repeated its phase with the exact kernel) keeps no inverse: no hand-off on the device there — asked of
        // the engine itself (ELLP_TAP_STATE [19] = launches per iteration, 0 for that kind), not inferred from an error code
        double tapv[20] = {0};
        const bool has_inverse = ellp_engine_tap(eng.e, ELLP_TAP_STATE, tapv, 20) >= 20 && tapv[19] != 0.0;
        const ellp_status rs = has_inverse ? ellp_engine_dual_rephase(eng.e, phase_2.std_form.c.data(), phase_2.std_form.b.data(),
                                                                      f2.kind.data(), f2.lb.data(), f2.ub.data(), err, sizeof(err))
                                           : ELLP_ERR_ARG;
        if (rs == ELLP_OPTIMAL) {
            s2 = run_resident_dual(eng.e, max_iter_, f2, phase_2.point, &res.iters_phase2);
        } else if (!has_inverse || rs == ELLP_ERR_PANIC) {
            // no hand-off on this engine, or one of the reference's EPS
            // assertions on the sign of d tripped on the device's inverse, which is not the fresh LU the reference
            // takes (dual_problem.rs:275-284): do the hand-off as the reference does, on the host — if the assertion
            // is the reference's own it fires again there, as the panic it is.  Any other error of the hand-off (a device
            // error, bad arguments) is reported, not retried
            ellp_engine_destroy(eng.e);
            eng.e = nullptr;
            phase_2.point_on_host();
            s2 = solve_with_initial(phase_2.std_form, phase_2.point, &res.iters_phase2);
        } else {
            to_status(rs, err);
            return res;
        }
    } else {
        if (eng.e) {  // phase 1 ran on a resident engine whose matrix is not phase 2's
            ellp_engine_destroy(eng.e);
            eng.e = nullptr;
        }
        phase_2 = DualPhase2::from_phase1(std::move(phase_1));
        s2 = solve_with_initial(phase_2.std_form, phase_2.point, &res.iters_phase2);
    }
    switch (s2) {
    case SolutionStatus::Optimal:
        res.kind = SolverResult::Optimal;
        res.solution = Solution{std::move(phase_2.std_form), std::move(phase_2.point.point), std::nullopt, std::nullopt};
        if (ranging_) attach_ranging(*res.solution, eng.e, engine_);  // eng.e: set only where it ran phase 2
        else if (postsolve_) attach_postsolve(*res.solution, eng.e, engine_);
        if (certificate_) no_certificate(res, "Optimal");
        return res;
    case SolutionStatus::Infeasible:
        res.kind = SolverResult::Infeasible;
        if (certificate_)
            attach_certificate(res, phase_2.std_form, phase_2.point.point, eng.e, engine_, ELLP_CERT_FARKAS_ROW, phase_2.std_form.cols(), nullptr,
                               "dual phase 2 infeasible");
        return res;
    case SolutionStatus::Unbounded: throw EllPPanic("dual phase 2 should never return unbounded");
    case SolutionStatus::MaxIter:
        res.kind = SolverResult::MaxIter;
        res.max_iter_obj = phase_2.obj();
        if (certificate_) no_certificate(res, "MaxIter");
        return res;
    }
    return res;
}

// ---- solve_from: a warm start

int map_start(const StandardForm &sf, const StartBasis &start, std::vector<std::int64_t> &B, std::vector<std::int64_t> &N,
              std::vector<std::uint8_t> &Nb) {
    const std::int64_t m = static_cast<std::int64_t>(sf.rows()), n = static_cast<std::int64_t>(sf.cols());
    if (static_cast<std::int64_t>(start.B.size()) != m) return START_BAD_SIZE;
    for (std::int64_t v : start.B)
        if (v < 0 || v >= n) return START_BAD_INDEX;  // v >= n: a phase-1 column of a primal solve's basis
    B = start.B;
    N.clear();
    Nb.clear();
    std::vector<std::uint8_t> seen(static_cast<size_t>(n), 0);
    if (start.has_N) {
        if (start.Nb.size() != start.N.size()) return START_BAD_SIZE;
        for (size_t j = 0; j < start.N.size(); ++j) {
            if (start.N[j] >= n) continue;  // a phase-1 column that ended nonbasic: it does not exist here
            N.push_back(start.N[j]);
            Nb.push_back(start.Nb[j]);
        }
        if (static_cast<std::int64_t>(N.size()) != n - m) return START_BAD_SIZE;
        for (size_t j = 0; j < N.size(); ++j)
            if (N[j] < 0 || Nb[j] > 2) return START_BAD_INDEX;
    }
    for (std::int64_t v : B) {
        if (seen[static_cast<size_t>(v)]) return START_BAD_INDEX;
        seen[static_cast<size_t>(v)] = 1;
    }
    if (start.has_N) {
        for (std::int64_t v : N) {
            if (seen[static_cast<size_t>(v)]) return START_BAD_INDEX;
            seen[static_cast<size_t>(v)] = 1;
        }
    } else {
        for (std::int64_t v = 0; v < n; ++v)
            if (!seen[static_cast<size_t>(v)]) {
                N.push_back(v);
                Nb.push_back(static_cast<std::uint8_t>(NonbasicBound::Lower));
            }
    }
    return START_USED;
}

namespace {

// the point of the start in standard form, or the reason it cannot be used; on START_USED pt (and y, d) hold what
// ellp_basis_start made
int start_point(const StandardForm &sf, const StartBasis &start, int mode, const EngineOptions &eng, DualFeasiblePoint &dp,
                ellp_start_info &info) {
    if (sf.rows() == 0) return START_NO_ROWS;
    std::vector<std::int64_t> B, N;
    std::vector<std::uint8_t> Nb;
    const int mapped = map_start(sf, start, B, N, Nb);
    if (mapped != START_USED) return mapped;
    if (sf.bounds.size() != sf.cols()) return START_BAD_SIZE;  // the standard form of a Problem has no cost without a column
    Point shape;
    shape.B.resize(B.size());
    shape.N.resize(N.size());
    Flat f = flatten(sf, shape);
    const size_t m = sf.rows(), n = sf.cols();
    dp.point.x.assign(n, 0.0);
    dp.y.assign(m, 0.0);
    dp.d.assign(n, 0.0);
    const ellp_opts o = make_opts(0, eng);
    char err[512] = {0};
    const ellp_status s = ellp_basis_start(static_cast<std::int64_t>(m), static_cast<std::int64_t>(n), sf.A.a.data(), sf.c.data(), sf.b.data(),
                                           f.kind.data(), f.lb.data(), f.ub.data(), B.data(), static_cast<std::int64_t>(B.size()), N.data(),
                                           Nb.data(), static_cast<std::int64_t>(N.size()), mode, &o, dp.point.x.data(), dp.y.data(),
                                           dp.d.data(), &info, err, sizeof(err));
    if (s == ELLP_ERR_SINGULAR) return START_SINGULAR;
    if (s == ELLP_ERR_ARG) return START_BAD_INDEX;  // more rows than an engine takes, or what map_start should have caught
    if (s != ELLP_OPTIMAL) to_status(s, err);       // throws: no device
    if (!(mode == ELLP_START_KEEP_LABELS ? info.primal_feasible : info.dual_feasible)) return START_NOT_FEASIBLE;
    dp.point.B.resize(B.size());
    dp.point.N.resize(N.size());
    f.B = B;
    f.N = N;
    f.Nb = Nb;
    unflatten(f, dp.point);
    return START_USED;
}

// what a warm start makes of phase 2's status, the phase-2 switch of solve(): shared by run_from_start and by solve_batch's
// batched phase 2 of the started problems
void end_from_start(int kind, SolutionStatus s2, StandardForm &sf, DualFeasiblePoint &dp, SolverResult &res) {
    if (kind == ELLP_ENGINE_PRIMAL) {
        if (s2 == SolutionStatus::Infeasible) throw EllPPanic("primal phase 2 should never be infeasible");
        if (s2 == SolutionStatus::Unbounded) { res.kind = SolverResult::Unbounded; return; }
    } else {
        if (s2 == SolutionStatus::Unbounded) throw EllPPanic("dual phase 2 should never return unbounded");
        if (s2 == SolutionStatus::Infeasible) { res.kind = SolverResult::Infeasible; return; }
    }
    if (s2 == SolutionStatus::MaxIter) {
        res.kind = SolverResult::MaxIter;
        res.max_iter_obj = kind == ELLP_ENGINE_DUAL ? sf.dual_obj(dp.y, dp.d) : sf.obj(dp.point.x);
        return;
    }
    res.kind = SolverResult::Optimal;
    res.solution = Solution{std::move(sf), std::move(dp.point), std::nullopt, std::nullopt};
}

// phase 2 from the point of a usable start, on a resident engine where the seam sends the problem to the device
// (plain: the seam's call for a problem without nonbasic columns, as in solve())
template <class Plain>
SolverResult run_from_start(int kind, StandardForm sf, DualFeasiblePoint dp, std::uint64_t max_iter, const EngineOptions &engine,
                            bool postsolve, bool ranging, bool certificate, Plain &&plain) {
    SolverResult res;
    EngineHandle eng;
    SolutionStatus s2;
    if (!dp.point.N.empty()) {
        Flat f = flatten(sf, dp.point);
        const ellp_opts o = make_opts(max_iter, engine);
        char err[512] = {0};
        const bool is_dual = kind == ELLP_ENGINE_DUAL;
        const ellp_status cs = ellp_engine_create(
            kind, static_cast<std::int64_t>(sf.rows()), static_cast<std::int64_t>(sf.cols()), static_cast<std::int64_t>(sf.bounds.size()),
            sf.A.a.data(), sf.c.data(), sf.b.data(), f.kind.data(), f.lb.data(), f.ub.data(), dp.point.x.data(), f.B.data(),
            static_cast<std::int64_t>(f.B.size()), f.N.data(), f.Nb.data(), static_cast<std::int64_t>(f.N.size()),
            is_dual ? dp.y.data() : nullptr, is_dual ? dp.d.data() : nullptr, &o, &eng.e, err, sizeof(err));
        if (cs != ELLP_OPTIMAL) to_status(cs, err);
        s2 = is_dual ? run_resident_dual(eng.e, max_iter, f, dp, &res.iters_phase2) : run_resident(eng.e, max_iter, f, dp.point, &res.iters_phase2);
    } else {
        s2 = plain(sf, dp, &res.iters_phase2);
    }
    const bool ending = (kind == ELLP_ENGINE_PRIMAL && s2 == SolutionStatus::Unbounded) || (kind == ELLP_ENGINE_DUAL && s2 == SolutionStatus::Infeasible);
    if (certificate && ending) {  // before end_from_start: sf and the point are still here
        res.kind = kind == ELLP_ENGINE_PRIMAL ? SolverResult::Unbounded : SolverResult::Infeasible;
        attach_certificate(res, sf, dp.point, eng.e, engine, kind == ELLP_ENGINE_PRIMAL ? ELLP_CERT_RAY_COLUMN : ELLP_CERT_FARKAS_ROW, sf.cols(), nullptr,
                           kind == ELLP_ENGINE_PRIMAL ? "primal phase 2 unbounded" : "dual phase 2 infeasible");
        return res;
    }
    end_from_start(kind, s2, sf, dp, res);
    if (certificate) no_certificate(res, res.kind == SolverResult::Optimal ? "Optimal" : "MaxIter");
    if (res.kind != SolverResult::Optimal || !res.solution) return res;
    if (ranging) attach_ranging(*res.solution, eng.e, engine);
    else if (postsolve) attach_postsolve(*res.solution, eng.e, engine);
    return res;
}

SolverResult primal_from_point(const PrimalSimplexSolver &single, StandardForm sf, DualFeasiblePoint dp, std::uint64_t max_iter,
                               const EngineOptions &engine, bool postsolve, bool ranging, bool certificate = false) {
    return run_from_start(ELLP_ENGINE_PRIMAL, std::move(sf), std::move(dp), max_iter, engine, postsolve, ranging, certificate,
                          [&single](const StandardForm &f, DualFeasiblePoint &p, std::uint64_t *it) { return single.solve_with_initial(f, p.point, it); });
}
SolverResult dual_from_point(const DualSimplexSolver &single, StandardForm sf, DualFeasiblePoint dp, std::uint64_t max_iter,
                             const EngineOptions &engine, bool postsolve, bool ranging, bool certificate = false) {
    return run_from_start(ELLP_ENGINE_DUAL, std::move(sf), std::move(dp), max_iter, engine, postsolve, ranging, certificate,
                          [&single](const StandardForm &f, DualFeasiblePoint &p, std::uint64_t *it) { return single.solve_with_initial(f, p, it); });
}

}  // namespace

SolverResult PrimalSimplexSolver::solve_from(Problem prob, const StartBasis &start, StartReport *report) const {
    StartReport local;
    StartReport &rep = report ? *report : local;
    rep = StartReport{};
    auto sfo = StandardForm::from_problem(prob);
    if (!sfo) {  // as solve()
        SolverResult res;
        res.kind = SolverResult::Infeasible;
        if (certificate_) no_certificate(res, "infeasibility decided by the set-up");
        return res;
    }
    DualFeasiblePoint dp;
    rep.reason = start_point(*sfo, start, ELLP_START_KEEP_LABELS, engine_, dp, rep.info);
    if (rep.reason != START_USED) return solve(std::move(prob));
    rep.used = true;
    return primal_from_point(*this, std::move(*sfo), std::move(dp), max_iter_, engine_, postsolve_, ranging_, certificate_);
}

SolverResult DualSimplexSolver::solve_from(Problem prob, const StartBasis &start, StartReport *report) const {
    StartReport local;
    StartReport &rep = report ? *report : local;
    rep = StartReport{};
    auto sfo = StandardForm::from_problem(prob);
    if (!sfo) {
        SolverResult res;
        res.kind = SolverResult::Infeasible;
        if (certificate_) no_certificate(res, "infeasibility decided by the set-up");
        return res;
    }
    DualFeasiblePoint dp;
    rep.reason = start_point(*sfo, start, ELLP_START_LABELS_BY_D, engine_, dp, rep.info);
    if (rep.reason != START_USED) return solve(std::move(prob));
    rep.used = true;
    return dual_from_point(*this, std::move(*sfo), std::move(dp), max_iter_, engine_, postsolve_, ranging_, certificate_);
}

}  // namespace ellp

// ---- solve_batch: solve() of many problems, the device loops in batched calls for the problems the LU-per-iteration kernels
// take: the primal's two phases in one call per batch (ellp_batch_primal_solve), the dual's phase by phase in lock step
// (ellp_batch_solve_with_initial).  Each problem takes the steps solve() takes
// for it — the host set-up, the checks between the phases, the hand-off — and the device loops compute what the single
// calls compute, so every outcome is solve()'s.  Problems the batch does not take run through solve() itself.
namespace ellp {

namespace {

// one solve_with_initial of a batch: the arrays of the single call and its outcome
struct Seam {
    const StandardForm *sf = nullptr;
    Point *pt = nullptr;
    DualFeasiblePoint *dp = nullptr;  // dual
    Flat f;
    ellp_status status = ELLP_ERR_ARG;
    ellp_stats stats{};
    std::string err;
};

// false: the call as a whole was refused (options, device) — the caller runs those problems on the single path
bool run_seams(int kind, std::vector<Seam *> &seams, std::uint64_t max_iter, const EngineOptions &eng) {
    if (seams.empty()) return true;
    std::vector<ellp_batch_item> items(seams.size());
    for (size_t k = 0; k < seams.size(); ++k) {
        Seam &s = *seams[k];
        s.f = flatten(*s.sf, *s.pt);
        items[k] = batch_item_of(*s.sf, s.f, s.pt->x, s.dp ? &s.dp->y : nullptr, s.dp ? &s.dp->d : nullptr);
    }
    const ellp_opts o = make_opts(max_iter, eng);
    std::vector<ellp_status> st(seams.size());
    std::vector<ellp_stats> stats(seams.size());
    char err[512] = {0};
    if (ellp_batch_solve_with_initial(kind, static_cast<std::int64_t>(items.size()), items.data(), &o, st.data(), stats.data(), err,
                                      sizeof(err)) != ELLP_OPTIMAL)
        return false;
    for (size_t k = 0; k < seams.size(); ++k) {
        Seam &s = *seams[k];
        s.status = st[k];
        s.stats = stats[k];
        s.err = items[k].err;
        unflatten(s.f, *s.pt);
    }
    return true;
}

// the slots of a batch that have not ended yet
struct Slot {
    size_t out;  // index into the outcomes
    bool done = false;
};

template <class F>
void settle(BatchOutcome &o, Slot &slot, F &&f) {
    try {
        f();
    } catch (...) {
        o.error = std::current_exception();
        slot.done = true;
    }
}

bool batchable(const StandardForm &sf, size_t n_N) { return sf.rows() > 0 && sf.rows() <= 128 && n_N > 0; }

// the primal also batches 129 - 1,024 rows where solve() with these options runs k_mid for the whole solve (the engine's
// exact_loop: pipeline 3, or pipeline 0 with m <= ELLP_MID_AUTO_MAX); an item the batch still refuses (too wide for the
// kernel's LDS) comes back as ELLP_ERR_ARG and goes through solve()
bool primal_batchable(const StandardForm &sf, size_t n_N, const EngineOptions &eng) {
    if (batchable(sf, n_N)) return true;
    const std::int64_t m = static_cast<std::int64_t>(sf.rows());
    if (m <= 128 || m > 1024 || n_N == 0) return false;
    if (eng.pipeline == 3) return true;
    const char *ev = std::getenv("ELLP_MID_AUTO_MAX");
    return eng.pipeline == 0 && ev && m <= std::atoll(ev);
}

// the dual batches 129 - 1,024 rows where solve() with these options runs k_mid (the same rule, plus bound flipping); their
// phase-1 start, which solve() makes on the device (point_deferred), comes from ellp_batch_dual_phase1_start
bool dual_mid_batchable(const StandardForm &sf, size_t n_N, const EngineOptions &eng) {
    const std::int64_t m = static_cast<std::int64_t>(sf.rows());
    if (m <= 128 || m > 1024 || n_N == 0) return false;
    if (eng.flags & ELLP_FLAG_DUAL_BOUND_FLIPPING) return true;
    return primal_batchable(sf, n_N, eng);
}

// the costs and bounds PrimalPhase2::from_phase1 (primal_problem.rs:263-291) gives phase 2, derived without consuming phase 1:
// the whole solve goes to the device in one call (ellp_batch_primal_solve), which needs both phases' inputs up front
struct Phase2Inputs {
    std::vector<double> c;
    std::vector<std::uint8_t> kind;
    std::vector<double> lb, ub;
};

Phase2Inputs phase2_inputs(const PrimalPhase1 &p1) {
    const StandardForm &sf = p1.std_form;
    Phase2Inputs in;
    in.c = sf.c;
    std::vector<Bound> bounds = sf.bounds;
    for (size_t i : p1.phase_1_vars) {
        in.c[i] = 0.0;
        bounds[i] = Bound::fixed(0.0);
    }
    for (size_t i = 0; i < sf.prob.variables.size(); ++i) {
        in.c[i] = sf.prob.variables[i].obj_coeff;
        bounds[i] = sf.prob.variables[i].bound;
    }
    const size_t nc = bounds.size();
    in.kind.resize(nc);
    in.lb.resize(nc);
    in.ub.resize(nc);
    for (size_t i = 0; i < nc; ++i) {  // as flatten
        in.kind[i] = static_cast<std::uint8_t>(bounds[i].kind);
        in.lb[i] = bounds[i].lb;
        in.ub[i] = (bounds[i].kind == Bound::Fixed) ? bounds[i].lb : bounds[i].ub;
    }
    return in;
}

// solve() of every problem of `which`, both phases in ONE batched call: phase 1 is built on the host as solve() builds it,
// the device makes the checks after phase 1 and the hand-off per item (no problem waits for another one's phase 1, and a
// problem's matrix goes up once), and what comes back maps to SolverResult as the two switch blocks of solve() map it
void primal_batch(std::vector<Problem> &probs, const std::vector<size_t> &which, std::uint64_t max_iter, const EngineOptions &eng,
                  std::vector<BatchOutcome> &out) {
    const PrimalSimplexSolver single = PrimalSimplexSolver(max_iter).with_engine(eng);
    struct Item {
        Slot slot;
        std::optional<PrimalPhase1> p1;
        Flat f;
        Phase2Inputs in2;
    };
    std::vector<Item> items(which.size());
    auto fallback = [&](Item &it) {
        settle(out[it.slot.out], it.slot, [&] { out[it.slot.out].result = single.solve(probs[it.slot.out]); });
        it.slot.done = true;
    };
    // phase 1 on the host
    std::vector<Item *> run;
    for (size_t k = 0; k < which.size(); ++k) {
        Item &it = items[k];
        it.slot.out = which[k];
        settle(out[it.slot.out], it.slot, [&] {
            auto p1 = PrimalPhase1::from_problem(probs[which[k]]);
            if (!p1) {
                out[it.slot.out].result.kind = SolverResult::Infeasible;
                it.slot.done = true;
                return;
            }
            it.p1 = std::move(*p1);
        });
        if (it.slot.done) continue;
        if (!primal_batchable(it.p1->std_form, it.p1->point.N.size(), eng)) {
            fallback(it);
            continue;
        }
        run.push_back(&it);
    }
    if (run.empty()) return;
    std::vector<ellp_batch_primal_item> bi(run.size());
    for (size_t k = 0; k < run.size(); ++k) {
        Item &it = *run[k];
        const StandardForm &sf = it.p1->std_form;
        it.f = flatten(sf, it.p1->point);
        it.in2 = phase2_inputs(*it.p1);
        ellp_batch_primal_item &b = bi[k];
        std::memset(&b, 0, sizeof(b));
        b.p1 = batch_item_of(sf, it.f, it.p1->point.x);
        b.c2 = it.in2.c.data();
        b.bound_kind2 = it.in2.kind.data();
        b.lb2 = it.in2.lb.data();
        b.ub2 = it.in2.ub.data();
    }
    const ellp_opts o = make_opts(max_iter, eng);
    std::vector<ellp_batch_primal_result> br(run.size());
    char err[512] = {0};
    if (ellp_batch_primal_solve(static_cast<std::int64_t>(bi.size()), bi.data(), &o, br.data(), err, sizeof(err)) != ELLP_OPTIMAL) {
        for (Item *it : run) fallback(*it);  // the call as a whole was refused (options, device)
        return;
    }
    for (size_t k = 0; k < run.size(); ++k) {
        Item &it = *run[k];
        const ellp_batch_primal_result &r = br[k];
        if (r.status == ELLP_ERR_ARG) {  // not taken by the batch kernel (LDS)
            fallback(it);
            continue;
        }
        SolverResult &res = out[it.slot.out].result;
        settle(out[it.slot.out], it.slot, [&] {
            const SolutionStatus s = to_status(r.status, bi[k].p1.err);  // throws what the phase that ended the solve raised
            unflatten(it.f, it.p1->point);
            res.iters_phase1 = r.iters_phase1;
            if (r.stage == 1) {  // the checks after phase 1 (solve(), primal…:42-55), made on the device
                switch (s) {
                case SolutionStatus::Optimal: throw EllPPanic("batch: phase 1 ended Optimal without a verdict");
                case SolutionStatus::Infeasible: res.kind = SolverResult::Infeasible; return;  // by status or by objective
                case SolutionStatus::Unbounded: throw EllPPanic("primal phase 1 should never be unbounded");
                case SolutionStatus::MaxIter:
                    res.kind = SolverResult::MaxIter;
                    res.max_iter_obj = std::numeric_limits<double>::infinity();
                    return;
                }
                return;
            }
            res.iters_phase2 = r.iters_phase2;
            PrimalPhase2 p2 = PrimalPhase2::from_phase1(std::move(*it.p1));
            it.p1.reset();
            switch (s) {
            case SolutionStatus::Optimal:
                res.kind = SolverResult::Optimal;
                res.solution = Solution{std::move(p2.std_form), std::move(p2.point), std::nullopt, std::nullopt};
                break;
            case SolutionStatus::Infeasible: throw EllPPanic("primal phase 2 should never be infeasible");
            case SolutionStatus::Unbounded: res.kind = SolverResult::Unbounded; break;
            case SolutionStatus::MaxIter:
                res.kind = SolverResult::MaxIter;
                res.max_iter_obj = p2.obj();
                break;
            }
        });
        it.slot.done = true;
    }
}

void dual_batch(std::vector<Problem> &probs, const std::vector<size_t> &which, std::uint64_t max_iter, const EngineOptions &eng,
                std::vector<BatchOutcome> &out) {
    const DualSimplexSolver single = DualSimplexSolver(max_iter).with_engine(eng);
    const char *hostpt = std::getenv("ELLP_HOST_DUAL_POINT");
    const bool defer = !(hostpt && hostpt[0] == '1');
    struct Item {
        Slot slot;
        std::optional<DualPhase1> p1;
        std::optional<DualPhase2> p2;
        Seam seam;
    };
    std::vector<Item> items(which.size());
    auto fallback = [&](Item &it) {
        settle(out[it.slot.out], it.slot, [&] { out[it.slot.out].result = single.solve(probs[it.slot.out]); });
        it.slot.done = true;
    };
    std::vector<Seam *> seams;
    std::vector<Item *> deferred;  // phase-1 start made on the device, in one batched call
    for (size_t w = 0; w < which.size(); ++w) {
        Item &it = items[w];
        const size_t k = which[w];
        it.slot.out = k;
        settle(out[k], it.slot, [&] {
            auto p1 = DualPhase1::from_problem(probs[k], defer);
            if (!p1) {
                out[k].result.kind = SolverResult::Infeasible;
                it.slot.done = true;
                return;
            }
            it.p1 = std::move(*p1);
        });
        if (it.slot.done) continue;
        if (it.p1->point_deferred) {
            if (dual_mid_batchable(it.p1->std_form, it.p1->point.point.N.size(), eng)) deferred.push_back(&it);
            else fallback(it);
            continue;
        }
        if (!batchable(it.p1->std_form, it.p1->point.point.N.size())) {
            fallback(it);
            continue;
        }
        it.seam.sf = &it.p1->std_form;
        it.seam.pt = &it.p1->point.point;
        it.seam.dp = &it.p1->point;
        seams.push_back(&it.seam);
    }
    if (!deferred.empty()) {
        // the starting points solve() makes with ellp_engine_create_dual_phase1, all in one call and bit for bit the same
        // (x, labels, y, d; the seam's starting objective is host_dual_obj of these, as the resident engine's is, and a
        // k_mid engine's loop finds its own leaving row).  An item whose start fails (a singular basis, a panic) or that the
        // call refuses goes through solve(), which meets the same failure
        std::vector<Flat> fl(deferred.size());
        std::vector<ellp_batch_item> bi(deferred.size());
        for (size_t k = 0; k < deferred.size(); ++k) {
            const StandardForm &sf = deferred[k]->p1->std_form;
            DualFeasiblePoint &dp = deferred[k]->p1->point;
            fl[k] = flatten(sf, dp.point);
            bi[k] = batch_item_of(sf, fl[k], dp.point.x, &dp.y, &dp.d);
        }
        const ellp_opts o = make_opts(max_iter, eng);
        std::vector<ellp_status> st(deferred.size(), ELLP_ERR_ARG);
        char err[512] = {0};
        const ellp_status rc = ellp_batch_dual_phase1_start(static_cast<std::int64_t>(bi.size()), bi.data(), &o, st.data(), nullptr,
                                                            err, sizeof(err));
        for (size_t k = 0; k < deferred.size(); ++k) {
            Item &it = *deferred[k];
            if (rc != ELLP_OPTIMAL || st[k] != ELLP_OPTIMAL) {
                fallback(it);
                continue;
            }
            unflatten(fl[k], it.p1->point.point);
            it.p1->point_deferred = false;
            it.seam.sf = &it.p1->std_form;
            it.seam.pt = &it.p1->point.point;
            it.seam.dp = &it.p1->point;
            seams.push_back(&it.seam);
        }
    }
    if (!run_seams(ELLP_ENGINE_DUAL, seams, max_iter, eng)) {
        for (Item &it : items)
            if (!it.slot.done) fallback(it);
        return;
    }
    // the checks after phase 1 (dual…:44-77); the dual-infeasible ones are classified by the primal solver, in one batch
    std::vector<size_t> classify;
    seams.clear();
    for (Item &it : items) {
        if (it.slot.done) continue;
        if (it.seam.status == ELLP_ERR_ARG) {
            fallback(it);
            continue;
        }
        SolverResult &res = out[it.slot.out].result;
        settle(out[it.slot.out], it.slot, [&] {
            const SolutionStatus s1 = to_status(it.seam.status, it.seam.err.c_str());
            res.iters_phase1 = it.seam.stats.iters;
            switch (s1) {
            case SolutionStatus::Optimal: {
                const double obj = it.p1->obj();
                if (!(obj < EPS)) throw EllPPanic("assertion failed: obj < EPS");
                if (!(obj > -EPS)) {
                    classify.push_back(it.slot.out);
                    it.slot.done = true;
                    return;
                }
                break;
            }
            case SolutionStatus::Infeasible: throw EllPPanic("dual phase 1 should never be infeasible");
            case SolutionStatus::Unbounded: throw EllPPanic("dual phase 1 should never be unbounded");
            case SolutionStatus::MaxIter:
                res.kind = SolverResult::MaxIter;
                res.max_iter_obj = std::numeric_limits<double>::infinity();
                it.slot.done = true;
                return;
            }
            it.p2 = DualPhase2::from_phase1(std::move(*it.p1));
            it.p1.reset();
        });
        if (it.slot.done) continue;
        it.seam = Seam{};
        it.seam.sf = &it.p2->std_form;
        it.seam.pt = &it.p2->point.point;
        it.seam.dp = &it.p2->point;
        seams.push_back(&it.seam);
    }
    if (!classify.empty()) {
        // PrimalSimplexSolver::default() (max_iter 1000) with the same engine options, as solve() does; its result replaces
        // the dual's
        for (size_t k : classify) out[k].result = SolverResult{};
        primal_batch(probs, classify, 1000, eng, out);
        for (size_t k : classify)
            if (!out[k].error && out[k].result.kind == SolverResult::Optimal) {
                out[k].result = SolverResult{};
                try {
                    throw EllPPanic("assertion failed: matches!(result, Infeasible | Unbounded | MaxIter)");
                } catch (...) {
                    out[k].error = std::current_exception();
                }
            }
    }
    const bool ran = run_seams(ELLP_ENGINE_DUAL, seams, max_iter, eng);
    for (Item &it : items) {
        if (it.slot.done) continue;
        SolverResult &res = out[it.slot.out].result;
        settle(out[it.slot.out], it.slot, [&] {
            SolutionStatus s2;
            if (!ran || it.seam.status == ELLP_ERR_ARG) {
                s2 = single.solve_with_initial(it.p2->std_form, it.p2->point, &res.iters_phase2);  // what solve() calls here
            } else {
                s2 = to_status(it.seam.status, it.seam.err.c_str());
                res.iters_phase2 = it.seam.stats.iters;
            }
            switch (s2) {
            case SolutionStatus::Optimal:
                res.kind = SolverResult::Optimal;
                res.solution = Solution{std::move(it.p2->std_form), std::move(it.p2->point.point), std::nullopt, std::nullopt};
                break;
            case SolutionStatus::Infeasible: res.kind = SolverResult::Infeasible; break;
            case SolutionStatus::Unbounded: throw EllPPanic("dual phase 2 should never return unbounded");
            case SolutionStatus::MaxIter:
                res.kind = SolverResult::MaxIter;
                res.max_iter_obj = it.p2->obj();
                break;
            }
        });
        it.slot.done = true;
    }
}

// What batch_postsolve and batch_ranging share.  Every Optimal outcome gets its results from ONE batched call for all of them
// (the items over 128 rows take the single call's path inside it); without rows it is answered on the host (`host`, what the
// attach_ function of solve() does there).  An item's refusal or singular basis becomes that outcome's exception, the one
// solve() with the same request throws.  No Optimal outcome with rows: not one device call.  Payload: the output arrays of
// one job, the struct that hands them to the call (out) and their way into the Solution (map)
template <class Payload, class Host, class Call>
void batch_attach(std::vector<BatchOutcome> &out, const EngineOptions &eng, Host host, Call call) {
    struct Job {
        size_t k;
        Flat f;
        Payload p;
    };
    auto fail = [&](size_t k) {
        out[k].error = std::current_exception();
        out[k].result = SolverResult{};
    };
    std::vector<Job> jobs;
    for (size_t k = 0; k < out.size(); ++k) {
        if (out[k].error || out[k].result.kind != SolverResult::Optimal || !out[k].result.solution) continue;
        Solution &sol = *out[k].result.solution;
        if (sol.std_form.rows() == 0) {
            try {
                host(sol, nullptr, eng);
            } catch (...) {
                fail(k);
            }
            continue;
        }
        jobs.push_back(Job{k, flatten(sol.std_form, sol.point), Payload(sol.std_form)});
    }
    if (jobs.empty()) return;
    std::vector<ellp_batch_item> items(jobs.size());
    std::vector<decltype(jobs[0].p.out())> outs(jobs.size());
    for (size_t q = 0; q < jobs.size(); ++q) {
        Solution &sol = *out[jobs[q].k].result.solution;
        items[q] = batch_item_of(sol.std_form, jobs[q].f, sol.point.x);
        outs[q] = jobs[q].p.out();
    }
    const ellp_opts o = make_opts(0, eng);
    std::vector<ellp_status> st(jobs.size(), ELLP_ERR_DEVICE);
    char err[512] = {0};
    const ellp_status rc = call(static_cast<std::int64_t>(items.size()), items.data(), &o, outs.data(), st.data(), err, sizeof(err));
    for (size_t q = 0; q < jobs.size(); ++q) {
        Job &j = jobs[q];
        try {
            if (rc != ELLP_OPTIMAL) to_status(rc, err);  // throws, as the attach_ function
            else if (st[q] != ELLP_OPTIMAL) to_status(st[q], items[q].err);
            j.p.map(*out[j.k].result.solution);
        } catch (...) {
            fail(j.k);
        }
    }
}

// solve_batch(..., postsolve): duals, reduced costs and the report, from ellp_batch_postsolve
void batch_postsolve(std::vector<BatchOutcome> &out, const EngineOptions &eng) {
    struct Payload {
        std::vector<double> y, d;
        ellp_kkt kkt;
        explicit Payload(const StandardForm &sf) : y(sf.rows(), 0.0), d(sf.bounds.size(), 0.0) { std::memset(&kkt, 0, sizeof(kkt)); }
        ellp_batch_post_out out() { return ellp_batch_post_out{y.data(), d.data(), nullptr, &kkt}; }
        void map(Solution &sol) const { map_postsolve(sol, y, d, kkt); }
    };
    batch_attach<Payload>(out, eng, attach_postsolve, ellp_batch_postsolve);
}

// solve_batch(..., ranging): the ranges, and with them the duals, reduced costs and report, from ellp_batch_ranging (and no
// ellp_batch_postsolve call)
void batch_ranging(std::vector<BatchOutcome> &out, const EngineOptions &eng) {
    struct Payload {
        RangeArrays ra;
        explicit Payload(const StandardForm &sf) : ra(sf.rows(), sf.bounds.size()) {}
        ellp_batch_range_out out() { return ellp_batch_range_out{ra.out(), nullptr}; }
        void map(Solution &sol) const { map_ranging(sol, ra); }
    };
    batch_attach<Payload>(out, eng, attach_ranging, ellp_batch_ranging);
}

// solve_batch(..., starts): the problems that come with a start.  Per problem the steps of solve_from:
// the standard form, map_start and the reasons of §3.11; then the points of ALL mapped starts from ONE
// ellp_batch_basis_start call (KEEP_LABELS for the primal solver, LABELS_BY_D for the dual; the verdict is start_point's),
// and phase 2 of the usable ones the batch takes in ONE ellp_batch_solve_with_initial call of their own.  A usable start
// the batch does not take runs phase 2 alone, from the point already made.  The problems whose start is not usable are
// returned in `cold`: they join the cold batch, untouched
void start_batch(int solver, std::vector<Problem> &probs, const std::vector<const StartBasis *> &starts, std::uint64_t max_iter,
                 const EngineOptions &eng, std::vector<BatchOutcome> &out, std::vector<StartReport> &reports, std::vector<size_t> &cold) {
    const int kind = solver == ELLP_ENGINE_PRIMAL ? ELLP_ENGINE_PRIMAL : ELLP_ENGINE_DUAL;
    const int mode = kind == ELLP_ENGINE_PRIMAL ? ELLP_START_KEEP_LABELS : ELLP_START_LABELS_BY_D;
    const std::optional<std::uint64_t> mi = max_iter;
    const PrimalSimplexSolver psingle = PrimalSimplexSolver(mi).with_engine(eng);
    const DualSimplexSolver dsingle = DualSimplexSolver(mi).with_engine(eng);
    struct Job {
        Slot slot;
        std::optional<StandardForm> sf;
        std::vector<std::int64_t> B, N;
        std::vector<std::uint8_t> Nb;
        Flat f;
        DualFeasiblePoint dp;
        Seam seam;
    };
    std::vector<Job> jobs;
    jobs.reserve(probs.size());
    // ---- the standard form and the mapping, on the host
    for (size_t k = 0; k < probs.size(); ++k) {
        if (!starts[k]) {
            cold.push_back(k);
            continue;
        }
        Job j;
        j.slot.out = k;
        int reason = START_USED;
        settle(out[k], j.slot, [&] {
            auto sfo = StandardForm::from_problem(probs[k]);
            if (!sfo) {  // as solve_from
                out[k].result.kind = SolverResult::Infeasible;
                j.slot.done = true;
                return;
            }
            j.sf = std::move(*sfo);
            if (j.sf->rows() == 0) reason = START_NO_ROWS;
            else if ((reason = map_start(*j.sf, *starts[k], j.B, j.N, j.Nb)) == START_USED && j.sf->bounds.size() != j.sf->cols())
                reason = START_BAD_SIZE;
        });
        if (j.slot.done) continue;
        if (reason != START_USED) {
            reports[k].reason = reason;
            cold.push_back(k);
            continue;
        }
        jobs.push_back(std::move(j));
    }
    if (jobs.empty()) return;
    // ---- every point in one call
    std::vector<ellp_batch_item> items(jobs.size());
    std::vector<ellp_start_info> infos(jobs.size());
    for (size_t q = 0; q < jobs.size(); ++q) {
        Job &j = jobs[q];
        const StandardForm &sf = *j.sf;
        Point shape;
        shape.B.resize(j.B.size());
        shape.N.resize(j.N.size());
        j.f = flatten(sf, shape);
        j.dp.point.x.assign(sf.cols(), 0.0);
        j.dp.y.assign(sf.rows(), 0.0);
        j.dp.d.assign(sf.cols(), 0.0);
        std::memset(&infos[q], 0, sizeof(infos[q]));
        ellp_batch_item &it = items[q];
        it = batch_item_of(sf, j.f, j.dp.point.x, &j.dp.y, &j.dp.d);  // n_c == n here (START_BAD_SIZE)
        it.B_index = j.B.data();  // the mapped start, not the shape's placeholders, which the resizes above gave its counts
        it.N_index = j.N.data();
        it.N_bound = j.Nb.data();
    }
    const ellp_opts o0 = make_opts(0, eng);
    std::vector<ellp_status> st(jobs.size(), ELLP_ERR_DEVICE);
    char err[512] = {0};
    const ellp_status rc = ellp_batch_basis_start(static_cast<std::int64_t>(items.size()), items.data(), mode, &o0, infos.data(), st.data(),
                                                  err, sizeof(err));
    std::vector<Seam *> seams;
    std::vector<Job *> seamed;
    auto alone = [&](Job &j) {  // phase 2 alone, from the point already made
        const size_t k = j.slot.out;
        settle(out[k], j.slot, [&] {
            out[k].result = kind == ELLP_ENGINE_PRIMAL ? primal_from_point(psingle, std::move(*j.sf), std::move(j.dp), max_iter, eng, false, false)
                                                       : dual_from_point(dsingle, std::move(*j.sf), std::move(j.dp), max_iter, eng, false, false);
        });
        j.slot.done = true;
    };
    for (size_t q = 0; q < jobs.size(); ++q) {
        Job &j = jobs[q];
        const size_t k = j.slot.out;
        StartReport &rep = reports[k];
        int reason = START_USED;
        settle(out[k], j.slot, [&] {  // start_point's verdict
            if (rc != ELLP_OPTIMAL) to_status(rc, err);  // throws: no device
            rep.info = infos[q];
            if (st[q] == ELLP_ERR_SINGULAR) reason = START_SINGULAR;
            else if (st[q] == ELLP_ERR_ARG) reason = START_BAD_INDEX;
            else if (st[q] != ELLP_OPTIMAL) to_status(st[q], items[q].err);
            else if (!(mode == ELLP_START_KEEP_LABELS ? infos[q].primal_feasible : infos[q].dual_feasible)) reason = START_NOT_FEASIBLE;
        });
        if (j.slot.done) continue;
        if (reason != START_USED) {
            rep.reason = reason;
            cold.push_back(k);
            continue;
        }
        rep.used = true;
        j.dp.point.B.resize(j.B.size());
        j.dp.point.N.resize(j.N.size());
        j.f.B = j.B;
        j.f.N = j.N;
        j.f.Nb = j.Nb;
        unflatten(j.f, j.dp.point);
        const size_t nN = j.dp.point.N.size();
        const bool takes = kind == ELLP_ENGINE_PRIMAL ? primal_batchable(*j.sf, nN, eng) : (batchable(*j.sf, nN) || dual_mid_batchable(*j.sf, nN, eng));
        if (!takes) {
            alone(j);
            continue;
        }
        j.seam.sf = &*j.sf;
        j.seam.pt = &j.dp.point;
        j.seam.dp = kind == ELLP_ENGINE_DUAL ? &j.dp : nullptr;
        seams.push_back(&j.seam);
        seamed.push_back(&j);
    }
    std::sort(cold.begin(), cold.end());
    // ---- phase 2 of the usable starts the batch takes, in one call of their own
    const bool ran = run_seams(kind, seams, max_iter, eng);
    for (Job *jp : seamed) {
        Job &j = *jp;
        if (!ran || j.seam.status == ELLP_ERR_ARG) {  // refused as a whole (options, device) or not taken (LDS): the single path
            alone(j);
            continue;
        }
        SolverResult &res = out[j.slot.out].result;
        settle(out[j.slot.out], j.slot, [&] {
            const SolutionStatus s2 = to_status(j.seam.status, j.seam.err.c_str());
            res.iters_phase2 = j.seam.stats.iters;
            end_from_start(kind, s2, *j.sf, j.dp, res);
        });
        j.slot.done = true;
    }
}

}  // namespace

std::vector<BatchOutcome> solve_batch(int solver, std::vector<Problem> probs, std::uint64_t max_iter, const EngineOptions &eng,
                                      bool postsolve, const std::vector<const StartBasis *> *starts, std::vector<StartReport> *reports,
                                      bool ranging) {
    std::vector<BatchOutcome> out(probs.size());
    std::vector<size_t> cold;
    if (starts) {
        if (starts->size() != probs.size()) throw std::invalid_argument("solve_batch: one start (or none) per problem");
        std::vector<StartReport> local;
        std::vector<StartReport> &rep = reports ? *reports : local;
        rep.assign(probs.size(), StartReport{});
        start_batch(solver, probs, *starts, max_iter, eng, out, rep, cold);
    } else {
        cold.resize(probs.size());
        for (size_t k = 0; k < cold.size(); ++k) cold[k] = k;
    }
    if (!cold.empty()) {
        if (solver == ELLP_ENGINE_PRIMAL) primal_batch(probs, cold, max_iter, eng, out);
        else dual_batch(probs, cold, max_iter, eng, out);
    }
    if (ranging) batch_ranging(out, eng);  // its y, d and report are the postsolve
    else if (postsolve) batch_postsolve(out, eng);
    return out;
}

}  // namespace ellp

"""solve(prob, postsolve=True) through the user API: duals(), reduced_costs() and kkt() of both solvers.

Sign convention (ellp_amd.Solution): a minimisation, d = c - A^T y, duals()[i] = d obj / d rhs_i: <= 0 for a binding `<=` row,
>= 0 for a binding `>=` row, exactly 0.0 for a row the rank check dropped.

The fixtures: reduced_costs() against d_j = c_j - sum_i a_ij y_i recomputed in rational arithmetic from the user's Problem
and the returned duals(), within the bound of tests/postsolve_model.py (a dropped row has y_i = 0 and adds nothing).  The
rows, from the Problem and the returned x: an `=` row's |rhs - a.x|, a `<=` row's a.x - rhs and a `>=` row's rhs - a.x are at
most kkt.primal_residual + kkt.bound_violation (the slack is a variable with the bound Lower(0)) + the entry bound of that
row — for the rows the standard form kept: all of them where no row was dropped, else those with a nonzero dual.
"""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import postsolve_model as PM  # noqa: E402
from helpers import GOLDEN, known_answers, read_mps  # noqa: E402

from ellp_amd import Bound, DualSimplexSolver, EllPError, PrimalSimplexSolver, Problem  # noqa: E402

pytestmark = pytest.mark.gpu
KA = known_answers()
SOLVERS = {"primal": PrimalSimplexSolver, "dual": DualSimplexSolver}
EPS = 1e-10
SEEN = {"dual_infeasibility": 0.0}


def _small(extra=()):
    p = Problem()
    p.add_var(-1.0, Bound.Lower(0.0))
    p.add_var(-1.0, Bound.Lower(0.0))
    p.add_constraint([(0, 1.0), (1, 2.0)], "Lte", 4.0)
    p.add_constraint([(0, 3.0), (1, 1.0)], "Lte", 6.0)
    for con in extra:
        p.add_constraint(*con)
    return p


@pytest.mark.parametrize("solver", ["primal", "dual"])
def test_two_row_lp(solver):
    """min -x1 - x2, x1 + 2 x2 <= 4, 3 x1 + x2 <= 6, x >= 0: two rows, cond < 10, so 1e-12 absolute"""
    res = SOLVERS[solver].default().solve(_small(), postsolve=True)
    assert res.kind == "optimal"
    sol = res.solution
    np.testing.assert_allclose(sol.x(), [1.6, 1.2], rtol=0, atol=1e-12)
    np.testing.assert_allclose(sol.duals(), [-0.4, -0.2], rtol=0, atol=1e-12)
    np.testing.assert_allclose(sol.reduced_costs(), [0.0, 0.0], rtol=0, atol=1e-12)
    k = sol.kkt()
    assert abs(k["primal_obj"] + 2.8) <= 1e-12 and abs(k["dual_obj"] + 2.8) <= 1e-12
    assert k["primal_residual"] <= 1e-12 and k["dual_infeasibility"] <= 1e-12 and k["y_backward_error"] <= 2 * PM.U


@pytest.mark.parametrize("solver", ["primal", "dual"])
def test_equality_added_twice(solver):
    """The same LP with the equality x1 + x2 = 2.5 added twice: the rank check drops one of the two, its dual is exactly 0.0
    and the duals still give the objective.  The reference's rank check (standard_form.rs:142-181) only drops rows of a
    problem with more rows than columns whose matrix has full column rank — anything else with a dependent row it answers
    with None, "infeasible" — so x1 - x2 = 0.5 is there as well: five rows, four columns (two slacks), x = (1.5, 1)."""
    eq = ([(0, 1.0), (1, 1.0)], "Eq", 2.5)
    res = SOLVERS[solver].default().solve(_small([([(0, 1.0), (1, -1.0)], "Eq", 0.5), eq, eq]), postsolve=True)
    assert res.kind == "optimal"
    sol = res.solution
    y = sol.duals()
    assert len(y) == 5
    np.testing.assert_allclose(sol.x(), [1.5, 1.0], rtol=0, atol=1e-12)
    assert (y[3] == 0.0) != (y[4] == 0.0), y
    assert abs(y[3] + y[4] + 1.0) <= 1e-12 and abs(y[2]) <= 1e-12, y
    assert abs(sol.obj() + 2.5) <= 1e-12
    assert abs(float(np.dot(y, [4.0, 6.0, 0.5, 2.5, 2.5])) - sol.obj()) <= 1e-12  # x >= 0: no bound terms
    np.testing.assert_allclose(sol.reduced_costs(), [0.0, 0.0], rtol=0, atol=1e-12)


def _optimal_fixtures():
    out = [(p["name"], p) for p in KA["problems"] if p["check"] in ("optimal", "optimal_obj")]
    out += [(p["name"], p) for p in KA["netlib"]]
    return out


def _fixture_of(fx):
    return read_mps(os.path.join(GOLDEN, fx["file"])) if "file" in fx else fx


@pytest.mark.parametrize("solver", ["primal", "dual"])
@pytest.mark.parametrize("fx", [f for _, f in _optimal_fixtures()], ids=[n for n, _ in _optimal_fixtures()])
def test_known_answers(fx, solver):
    """every Optimal fixture (the README example is one of them) and the netlib LPs"""
    _check_fixture(_fixture_of(fx), solver, fx["name"])


@pytest.mark.parametrize("solver", ["primal", "dual"])
def test_above_128_rows_on_the_resident_engines(solver):
    """Six copies of AFIRO as one LP (162 rows, every variable Lower(0)): above 128 rows the dual solver keeps ONE resident
    engine for both phases (the hand-off is ellp_engine_dual_rephase) and the postsolve examines that engine after phase 2;
    the fixtures above all have at most 128 rows and take the dual's one-shot path"""
    from helpers import blockdiag
    ka = next(p for p in KA["netlib"] if p["name"] == "afiro")
    fxd = blockdiag(read_mps(os.path.join(GOLDEN, ka["file"])), 6)
    assert len(fxd["constraints"]) > 128
    sol = _check_fixture(fxd, solver, "afiro x 6")
    assert abs(sol.obj() / (6 * ka["obj"]) - 1.0) <= 1e-9


def _check_fixture(fxd, solver, name):
    fx = {"name": name}
    prob = Problem.from_fixture(fxd)
    flat = prob._debug_phase1("primal")
    res = SOLVERS[solver].default().solve(prob, postsolve=True)
    assert res.kind == "optimal", res
    sol = res.solution
    x, y, d, k = sol.x(), sol.duals(), sol.reduced_costs(), sol.kkt()
    nv, nc = len(fxd["vars"]), len(fxd["constraints"])
    assert len(y) == nc and len(d) == nv
    if flat is None or flat["m"] == 0:  # no row reaches the device: answered on the host, y = 0 and d = c
        assert not np.any(y) and list(d) == [float(obj) for obj, _ in fxd["vars"]]
        return sol
    kept_all = flat["m"] == nc
    kd, kr = PM.chain_lengths(nc, max(flat["n"] - flat["m"], 1))
    # reduced costs
    col = [[] for _ in range(nv)]
    for i, (coeffs, op, rhs) in enumerate(fxd["constraints"]):
        for j, a in coeffs:
            col[j].append((i, a))
    for j in range(nv):
        rows = [i for i, _ in col[j]]
        av = [a for _, a in col[j]]
        cj = Fraction(float(fxd["vars"][j][0]))
        ex = cj - PM.exact_dot(av, y[rows])
        S = abs(cj) + PM.exact_dot(av, y[rows], absolute=True)
        assert abs(Fraction(float(d[j])) - ex) <= PM.entry_bound(ex, S, kd), (fx["name"], "d", j, d[j], float(ex))
    # rows
    slackness = Fraction(k["primal_residual"]) + Fraction(k["bound_violation"])
    for i, (coeffs, op, rhs) in enumerate(fxd["constraints"]):
        if not (kept_all or y[i] != 0.0):
            continue
        idx = [j for j, _ in coeffs]
        av = [a for _, a in coeffs]
        ax = PM.exact_dot(av, x[idx])
        S = abs(Fraction(float(rhs))) + PM.exact_dot(av, x[idx], absolute=True)
        viol = ax - Fraction(float(rhs)) if op == "Lte" else (Fraction(float(rhs)) - ax if op == "Gte" else abs(ax - Fraction(float(rhs))))
        bound = (Fraction(k["primal_residual"]) if op == "Eq" else slackness) + PM.entry_bound(viol, S, kr)
        assert viol <= bound, (fx["name"], "row", i, float(viol), float(bound))
    obj = sol.obj()
    print(f"{fx['name']} {solver}: obj {obj!r}, primal_obj - dual_obj {k['primal_obj'] - k['dual_obj']:.3e}, dual_infeasibility "
          f"{k['dual_infeasibility']:.3e}, primal_residual {k['primal_residual']:.3e}, omega {k['y_backward_error'] / PM.U:.3f} u")
    assert abs(k["primal_obj"] - k["dual_obj"]) <= 1e-9 * (1.0 + abs(obj)), (k["primal_obj"], k["dual_obj"])
    SEEN["dual_infeasibility"] = max(SEEN["dual_infeasibility"], k["dual_infeasibility"])
    print(f"largest dual_infeasibility so far: {SEEN['dual_infeasibility']:.3e}")
    assert k["dual_infeasibility"] <= 2 * EPS, k["dual_infeasibility"]
    return sol


@pytest.mark.parametrize("solver", ["primal", "dual"])
def test_without_the_flag_nothing_changes(solver):
    fx = next(p for p in KA["problems"] if p["name"] == KA["readme"]["problem"])
    plain = SOLVERS[solver].default().solve(Problem.from_fixture(fx))
    post = SOLVERS[solver].default().solve(Problem.from_fixture(fx), postsolve=True)
    assert plain.kind == post.kind == "optimal" and plain.iters == post.iters
    assert plain.solution.obj() == post.solution.obj() and (plain.solution.x() == post.solution.x()).all()
    assert abs(plain.solution.obj() - KA["readme"]["obj"]) < 1e-12
    for f in (plain.solution.duals, plain.solution.reduced_costs, plain.solution.kkt):
        with pytest.raises(EllPError, match="postsolve=True"):
            f()

"""solve(prob, ranging=True) through the user API: cost_ranging(), rhs_ranging() and basis() of both solvers, on the Optimal
fixtures of tests/golden/known_answers.json and on AFIRO.

The standard form is rebuilt here from the user's Problem as StandardForm::from_problem lays it out (the variables in order,
one slack per inequality row handed out from the last column backwards, +1 for `<=` and -1 for `>=`, the rows the rank check
kept through row_origin; the primal solver's phase-1 variables, Fixed at 0 in phase 2, behind them), and the ranges are judged in
rational arithmetic with the exact inverse at the end basis the solve reports (tests/ranging_model.py, check_cost_limit /
check_rhs_limit): inside a finite limit every sign and bound holds, outside the blocking one is lost.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ranging_model as RM  # noqa: E402
from helpers import GOLDEN, known_answers, read_mps  # noqa: E402

from ellp_amd import Bound, DualSimplexSolver, EllPError, PrimalSimplexSolver, Problem  # noqa: E402

pytestmark = pytest.mark.gpu
KA = known_answers()
SOLVERS = {"primal": PrimalSimplexSolver, "dual": DualSimplexSolver}
EPS = 1e-10


def _fixtures():
    out = [(p["name"], p) for p in KA["problems"] if p["check"] in ("optimal", "optimal_obj")]
    out += [(p["name"], p) for p in KA["netlib"] if p["name"] == "afiro"]
    return out


def _standard_form(fxd, flat, n_sf, row_origin):
    """(A, b, c, kind, lb, ub) of the phase-2 standard form with n_sf columns"""
    nv, ncon = len(fxd["vars"]), len(fxd["constraints"])
    ns = sum(1 for _, op, _ in fxd["constraints"] if op != "Eq")
    A = np.zeros((ncon, nv + ns))
    b = np.zeros(ncon)
    slack = nv + ns - 1
    for i, (coeffs, op, rhs) in enumerate(fxd["constraints"]):
        b[i] = rhs
        for j, a in coeffs:
            A[i, j] = a
        if op != "Eq":
            A[i, slack] = 1.0 if op == "Lte" else -1.0
            slack -= 1
    A, b = A[row_origin], b[row_origin]
    m = len(row_origin)
    flatA = flat["A"].reshape(flat["n"], flat["m"]).T
    assert flat["m"] == m and (flatA[:, :nv + ns] == A).all() and (flat["b"] == b).all()  # the layout assumed here is the library's
    # the dual solver ends on the standard form itself; the primal's phase 2 keeps the phase-1 variables (Fixed at 0), of which
    # those behind flat["n"] have a cost entry and no column
    assert n_sf == nv + ns or n_sf == flat["n_c"], (n_sf, nv + ns, flat["n"], flat["n_c"])
    A = flatA[:, :min(flat["n"], n_sf)]
    c, kind, lb, ub = np.zeros(n_sf), np.full(n_sf, 1, dtype=np.uint8), np.zeros(n_sf), np.zeros(n_sf)
    for v, (obj, bound) in enumerate(fxd["vars"]):
        bd = Bound.from_fixture(bound)
        c[v], kind[v], lb[v], ub[v] = obj, bd.kind, bd.lb, bd.ub
    kind[nv + ns:] = 4  # the phase-1 columns: Fixed(0) in phase 2
    return A, b, c, kind, lb, ub


@pytest.mark.parametrize("solver", ["primal", "dual"])
@pytest.mark.parametrize("fx", [f for _, f in _fixtures()], ids=[n for n, _ in _fixtures()])
def test_ranges_mean_what_they_say(fx, solver):
    fxd = read_mps(os.path.join(GOLDEN, fx["file"])) if "file" in fx else fx
    prob = Problem.from_fixture(fxd)
    flat = prob._debug_phase1("primal")
    res = SOLVERS[solver].default().solve(prob, ranging=True)
    assert res.kind == "optimal", res
    sol = res.solution
    nv, ncon = len(fxd["vars"]), len(fxd["constraints"])
    cd, cu, cb = sol.cost_ranging()
    rd, ru, rb = sol.rhs_ranging()
    assert len(cd) == len(cu) == nv and cb.shape == (nv, 2) and len(rd) == len(ru) == ncon and rb.shape == (ncon, 2)
    assert (cd <= 0).all() and (cu >= 0).all() and (rd <= 0).all() and (ru >= 0).all()
    assert len(sol.duals()) == ncon  # ranging implies the postsolve
    bs = sol.basis()
    if flat is None or flat["m"] == 0:  # no row reaches the device: every variable nonbasic, d = c, answered on the host
        assert len(bs["B"]) == 0 and not np.any(rd) and not np.any(ru) and (rb == -1).all()
        for v, (obj, bound) in enumerate(fxd["vars"]):
            assert cd[v] in (-np.inf, -max(obj, 0.0), min(-obj, 0.0)) and cu[v] in (np.inf, -min(obj, 0.0), max(-obj, 0.0))
        return
    B, N, Nb, x, ro = bs["B"], bs["N"], bs["Nb"], bs["x"], bs["row_origin"]
    m = len(B)
    A, b, c, kind, lb, ub = _standard_form(fxd, flat, len(x), ro)
    ex = RM.ExactRanging(m, A.shape[1], len(x), A, c, b, kind, lb, ub, x, B, N, Nb, EPS)
    two = 2 * ex.eps
    tiny_a = sum(1 for i in range(m) for a in ex.alpha(i) if 0 < abs(a) <= two)
    tiny_w = sum(1 for row in ex.W for w in row if 0 < abs(w) <= two)
    assert 100 * tiny_a <= m * len(N) and 100 * tiny_w <= m * m, (tiny_a, tiny_w)
    posB = {int(v): i for i, v in enumerate(B)}
    posN = {int(v): j for j, v in enumerate(N)}
    checked = 0
    for v in range(nv):
        if v in posB:
            for up, L, blk in ((True, cu[v], cb[v, 1]), (False, cd[v], cb[v, 0])):
                if np.isfinite(L):
                    ex.check_cost_limit(posB[v], L, blk, up)
                    checked += 1
                else:
                    assert blk == -1
        else:
            dn, up, bd, bu = ex.cost_nonbasic(posN[v])
            for got, want in ((cd[v], dn), (cu[v], up)):
                want = float(want)
                assert got == want if np.isinf(want) else abs(got - want) <= 1e-9 * (1.0 + abs(want)), (v, got, want)
            assert (cb[v, 0], cb[v, 1]) == (bd, bu), (v, cb[v], bd, bu)
    dropped = set(range(ncon)) - set(int(o) for o in ro)
    for o in dropped:
        assert (rd[o], ru[o], rb[o, 0], rb[o, 1]) == (0.0, 0.0, -1, -1)
    for k, o in enumerate(ro):
        for up, L, blk in ((True, ru[o], rb[o, 1]), (False, rd[o], rb[o, 0])):
            if np.isfinite(L):
                ex.check_rhs_limit(k, L, blk, up)
                checked += 1
            else:
                assert blk == -1
    print(f"{fx['name']} {solver}: {m} rows, {checked} finite limits hold in exact arithmetic; inverse_residual {bs['inverse_residual']:.3e}")


@pytest.mark.parametrize("solver", ["primal", "dual"])
def test_without_the_flag_nothing_changes(solver):
    fx = next(p for p in KA["problems"] if p["name"] == KA["readme"]["problem"])
    plain = SOLVERS[solver].default().solve(Problem.from_fixture(fx))
    rng = SOLVERS[solver].default().solve(Problem.from_fixture(fx), ranging=True)
    assert plain.kind == rng.kind == "optimal" and plain.iters == rng.iters
    assert plain.solution.obj() == rng.solution.obj() and (plain.solution.x() == rng.solution.x()).all()
    for f in (plain.solution.cost_ranging, plain.solution.rhs_ranging, plain.solution.basis):
        with pytest.raises(EllPError, match="ranging=True"):
            f()
    post = SOLVERS[solver].default().solve(Problem.from_fixture(fx), postsolve=True)
    with pytest.raises(EllPError, match="ranging=True"):
        post.solution.cost_ranging()
    assert (post.solution.duals() == rng.solution.duals()).all()

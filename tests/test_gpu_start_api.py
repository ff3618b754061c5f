"""solve(prob, start=...) on the device: restarts at the optimum, re-solves after a change of the right-hand sides or of the
costs, the agreement with the ranging, unusable starts, the larger engines, and that solve(prob) without a start is untouched.

Perturbation k of constraint or variable k (0-based, file order of helpers.read_mps) multiplies the value by
1 + s sin(k + 1) (tests/start_cases.py).  Objectives are compared to relative 1e-9, the project's stated tolerance.

The netlib LPs here have at most 128 rows, where the device loop is bit for bit the oracle's: the arrays _engine.basis_start
returns are handed to the oracle's primal / dual solve_with_initial as a Phase-shaped view, and the warm solve's iteration
count, final index sets and x must equal the oracle's exactly.  The 162-row and 400-row engines are compared on results only.

A singular start is made of two columns proportional by a power of two (an exact zero pivot, see tests/test_gpu_start.py).
adlittle has no slack basis (41 slacks, 56 rows): the primal-infeasible start is its slack columns completed by structural ones.

Checked on the CPU before any device run: the oracle solves blockdiag(afiro, 6) to Optimal under rhs s = 0.05 (dual) and cost
s = 0.05 (primal).  The 400 x 900 LP of the benchmark's family (min c.x, A x <= b, x >= 0 with every a_ij in [0.1, 1.1], b > 0)
is Optimal under any rhs s < 1 by its shape: x = 0 stays feasible and the feasible set stays bounded (the oracle's LU-per-
iteration dual loop does not finish its 9e5 phase-1 iterations in a quarter of an hour on the CPU).  No other s was needed.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402
import start_cases as SC  # noqa: E402
import start_model as SM  # noqa: E402

pytestmark = pytest.mark.gpu
REL = 1e-9


def _A():
    import ellp_amd
    return ellp_amd


def _solver(which, **kw):
    A = _A()
    return (A.PrimalSimplexSolver if which == "primal" else A.DualSimplexSolver)(max_iter=100000, **kw)


def _close(a, b):
    return abs(a - b) <= REL * max(1.0, abs(b))


_CACHE = {}


def _cold(name, fx, which):
    """the cold solve of a fixture with its ranging, once per (name, solver)"""
    key = (name, which)
    if key not in _CACHE:
        _CACHE[key] = _solver(which).solve(_A().Problem.from_fixture(fx), ranging=True)
    return _CACHE[key]


def _optimal_fixtures():
    out = [(f["name"], f) for f in helpers.known_answers()["problems"] if f["check"] in ("optimal", "optimal_obj")]
    out += [(n, SC.netlib(n)) for n in ("afiro", "adlittle", "blend")]
    keep = []
    for name, fx in out:
        rc, rows, cols, *_ = _A()._debug_map_start(_A().Problem.from_fixture(fx), dict(B=[]))
        if rows > 0 and cols > rows:
            keep.append((name, fx))
    return keep


FIXTURES = _optimal_fixtures()
_SKIPPED = []


def test_the_fixtures_with_rows_and_nonbasic_columns():
    """17 optimal fixtures; 2 have no variable, 2 a variable but no row (the start is ignored there, reason 5) and the 2 linear
    systems no nonbasic column: 11 have rows and nonbasic columns, and every one of them is restarted below"""
    assert [n for n, _ in FIXTURES] == ["small_prob_%d" % k for k in range(1, 8)] + ["beale_cycle", "afiro", "adlittle", "blend"]
    A = _A()
    for name in ("one_variable_no_constraints", "linear_system_2d"):
        fx = next(f for f in helpers.known_answers()["problems"] if f["name"] == name)
        ref = _solver("dual").solve(A.Problem.from_fixture(fx))
        got = _solver("dual").solve(A.Problem.from_fixture(fx), start=dict(B=list(range(len(fx["constraints"])))))
        assert got.kind == ref.kind == "optimal" and got.solution.obj() == ref.solution.obj()
        assert got.start["reason"] == (5 if not fx["constraints"] else 0), (name, got.start)


@pytest.mark.parametrize("which", ["primal", "dual"])
@pytest.mark.parametrize("name", [n for n, _ in FIXTURES])
def test_restart_at_the_optimum(name, which):
    fx = dict(FIXTURES)[name]
    cold = _cold(name, fx, which)
    assert cold.kind == "optimal"
    basis = cold.solution.basis()
    rc, rows, cols, *_ = _A()._debug_map_start(_A().Problem.from_fixture(fx), dict(B=basis["B"]))
    if (basis["B"] >= cols).any():  # the cold basis holds a phase-1 column: the only reason to leave a fixture out
        _SKIPPED.append((name, which))
        assert len(_SKIPPED) <= 2, _SKIPPED
        pytest.skip("the cold basis holds a phase-1 column in B")
    warm = _solver(which).solve(_A().Problem.from_fixture(fx), start=cold.solution)
    print(name, which, "cold iters", cold.iters, "warm", warm.iters, warm.start["used"], warm.start["reason"],
          warm.start["primal_infeasibility"], warm.start["dual_infeasibility"])
    assert warm.start["used"] and warm.start["reason"] == 0, warm.start
    assert warm.kind == "optimal" and tuple(warm.iters) == (0, 1), warm.iters
    assert _close(warm.solution.obj(), cold.solution.obj())
    assert sorted(warm.solution.basis()["B"].tolist()) == sorted(b for b in basis["B"].tolist())


def _oracle_from_start(fx_new, basis, which):
    """the oracle's loop from the point ellp_basis_start makes of `basis` on the perturbed LP: (iters, view after the solve)"""
    from ellp_amd import _engine as E
    from oracle import ellp_oracle as eo
    v = SC.oracle_optimum(fx_new)  # the standard form of the perturbed LP (its point is overwritten below)
    rc, rows, cols, B, N, Nb = _A()._debug_map_start(_A().Problem.from_fixture(fx_new), basis)
    assert rc == 0 and (rows, cols) == (v.m, v.n)
    mode = E.START_KEEP_LABELS if which == "primal" else E.START_LABELS_BY_D
    s, x, y, d, Nb2, info = E.basis_start(SC.flat_of(v, B, N, Nb), mode)
    assert s == E.OPTIMAL
    v.x[:v.n], v.B[:] = x, B
    v.N[:len(N)], v.Nb[:len(N)], v.nN = N, Nb2, len(N)
    v.y, v.d = y.copy(), np.concatenate([d, v.c[v.n:]])
    st, it, msg = (eo.primal_solve_with_initial(v, 100000) if which == "primal" else eo.dual_solve_with_initial(v, 100000))
    assert st == 0, (st, msg)
    return it, v, info


PERTURBED = [("adlittle", "rhs", 0.05, "dual"), ("adlittle", "rhs", 0.3, "dual"), ("adlittle", "cost", 0.05, "primal"),
             ("adlittle", "cost", 0.3, "primal"), ("blend", "rhs", 0.05, "dual"), ("blend", "rhs", 0.3, "dual"),
             ("blend", "cost", 0.05, "primal")]


@pytest.mark.parametrize("name,what,s,which", PERTURBED)
def test_resolve_after_a_perturbation(name, what, s, which):
    fx = SC.netlib(name)
    cold0 = _cold(name, fx, "dual")  # a dual solve's basis lives in the standard form's own indices
    fx_new = SC.perturbed(fx, what, s)
    cold = _solver(which).solve(_A().Problem.from_fixture(fx_new))
    warm = _solver(which).solve(_A().Problem.from_fixture(fx_new), start=cold0.solution)
    print(name, what, s, which, "cold", cold.iters, "warm", warm.iters, warm.start["labels_changed"])
    assert cold.kind == "optimal" and warm.kind == "optimal"
    assert warm.start["used"] and warm.iters[0] == 0, warm.start
    assert _close(warm.solution.obj(), cold.solution.obj()), (warm.solution.obj(), cold.solution.obj())
    it, v, info = _oracle_from_start(fx_new, cold0.solution.basis(), which)
    wb = warm.solution.basis()
    assert warm.iters[1] == it, (warm.iters, it)
    assert wb["B"].tolist() == v.B.tolist() and wb["N"].tolist() == v.N[:v.nN].tolist() and wb["Nb"].tolist() == v.Nb[:v.nN].tolist()
    assert (wb["x"].view(np.uint64) == v.x[:v.n].view(np.uint64)).all()
    assert warm.start["labels_changed"] == info["labels_changed"]


def test_ranging_and_warm_start_agree_on_a_cost():
    fx = SC.netlib("adlittle")
    cold = _cold("adlittle", fx, "dual")
    down, up, _ = cold.solution.cost_ranging()
    finite = [k for k in range(len(up)) if np.isfinite(up[k]) and up[k] > 1e-6 * max(1.0, abs(fx["vars"][k][0]))]
    assert finite
    k = finite[0]
    for factor, stays in ((0.5, True), (2.0, False)):
        fx_new = SC.perturbed(fx, "cost", 0.0)
        fx_new["vars"][k][0] = fx["vars"][k][0] + factor * float(up[k])
        warm = _solver("primal").solve(_A().Problem.from_fixture(fx_new), start=cold.solution)
        ref = _solver("primal").solve(_A().Problem.from_fixture(fx_new))
        print("cost", k, factor, warm.iters, ref.iters)
        assert warm.start["used"] and warm.kind == "optimal" and _close(warm.solution.obj(), ref.solution.obj())
        if stays:
            assert tuple(warm.iters) == (0, 1) and warm.solution.basis()["B"].tolist() == cold.solution.basis()["B"].tolist()
        else:
            assert warm.iters[0] == 0 and warm.iters[1] >= 2  # at least one pivot before the pass that finds no candidate


def test_ranging_and_warm_start_agree_on_a_right_hand_side():
    fx = SC.netlib("adlittle")
    cold = _cold("adlittle", fx, "dual")
    down, up, _ = cold.solution.rhs_ranging()
    finite = [k for k in range(len(up)) if np.isfinite(up[k]) and up[k] > 1e-6 * max(1.0, abs(fx["constraints"][k][2]))]
    assert finite
    k = finite[0]
    for factor, stays in ((0.5, True), (2.0, False)):
        fx_new = SC.perturbed(fx, "rhs", 0.0)
        fx_new["constraints"][k][2] = fx["constraints"][k][2] + factor * float(up[k])
        warm = _solver("dual").solve(_A().Problem.from_fixture(fx_new), start=cold.solution)
        ref = _solver("dual").solve(_A().Problem.from_fixture(fx_new))
        print("rhs", k, factor, warm.iters, ref.iters)
        assert warm.start["used"] and warm.kind == "optimal" and _close(warm.solution.obj(), ref.solution.obj())
        if stays:
            assert tuple(warm.iters) == (0, 1) and warm.solution.basis()["B"].tolist() == cold.solution.basis()["B"].tolist()
        else:
            assert warm.iters[0] == 0 and warm.iters[1] >= 2


def _same_as_cold(fx, which, start, reason):
    ref = _solver(which).solve(_A().Problem.from_fixture(fx))
    got = _solver(which).solve(_A().Problem.from_fixture(fx), start=start)
    assert not got.start["used"] and got.start["reason"] == reason, got.start
    assert got.kind == ref.kind and tuple(got.iters) == tuple(ref.iters)
    assert (got.solution.x().view(np.uint64) == ref.solution.x().view(np.uint64)).all()
    return got


def test_unusable_starts_solve_cold():
    fx = SC.netlib("adlittle")
    basis = _cold("adlittle", fx, "dual").solution.basis()
    B = basis["B"]
    v = SC.oracle_optimum(fx)
    for which in ("primal", "dual"):
        _same_as_cold(fx, which, dict(B=B[:-1]), 1)                                    # B one short
        _same_as_cold(fx, which, dict(B=np.concatenate([B[:-1], B[:1]])), 2)           # a duplicated index
        _same_as_cold(fx, which, dict(B=np.concatenate([B[:-1], [v.n]])), 2)           # a phase-1 index in B
    # two proportional columns: adlittle with one more variable whose column is twice variable 0's (at a cost that never pays,
    # so the LP keeps its optimum); both basic.  The new variable takes index nv, the slacks move up by one
    nv = len(fx["vars"])
    fx2 = SC.perturbed(fx, "cost", 0.0)
    fx2["vars"].append([2.0 * abs(fx["vars"][0][0]) + 1.0, ["Lower", 0.0, 0.0]])
    for con in fx2["constraints"]:
        con[0] += [[nv, 2.0 * a] for j, a in con[0] if j == 0]
    B_cold2 = _solver("dual").solve(_A().Problem.from_fixture(fx2), ranging=True).solution.basis()["B"].tolist()
    B2 = [0, nv] + [b for b in B_cold2 if b not in (0, nv)][:len(B) - 2]
    assert len(B2) == len(B)
    _same_as_cold(fx2, "dual", dict(B=B2), 3)
    _same_as_cold(fx2, "primal", dict(B=B2), 3)
    # a slack basis for the primal solver.  adlittle has 41 slacks for 56 rows (15 equality rows), so the slack columns are
    # completed by the first structural columns, in index order, that keep the columns independent: primal infeasible by
    # 5.0e5 in the model
    m, n = v.m, v.n
    A = v.A_matrix()
    sb = list(range(nv, n))
    for j in range(nv):
        if len(sb) < m and np.linalg.matrix_rank(A[:, sb + [j]]) == len(sb) + 1:
            sb.append(j)
    assert len(sb) == m
    rest = [j for j in range(n) if j not in sb]
    mod = SM.Start(A, v.c[:n], v.b, v.kind[:n], v.lb[:n], v.ub[:n], sb, rest, np.zeros(n - m, dtype=np.uint8), SM.KEEP_LABELS)
    assert mod.primal_infeasibility > 1000 * SM.F(1e-10)
    got = _same_as_cold(fx, "primal", dict(B=sb), 4)
    assert abs(got.start["primal_infeasibility"] - float(mod.primal_infeasibility)) <= 1e-9 * float(mod.primal_infeasibility)
    assert got.start["worst_primal_var"] == mod.worst_primal_var and got.start["primal_feasible"] == 0
    # the optimal basis after the cost change s = 0.3 for the DUAL solver: dual infeasible
    got = _same_as_cold(SC.perturbed(fx, "cost", 0.3), "dual", basis, 4)
    print("dual infeasibility of the old basis after the cost change:", got.start["dual_infeasibility"])
    assert got.start["dual_infeasibility"] > 1.0 and got.start["dual_feasible"] == 0


def _dense(seed, m, n):
    """the benchmark's family (synth.dense_lp) as a fixture: min c.x, A x <= b, x >= 0"""
    from ellp_amd import synth
    A, b, c = synth.dense_lp(seed, m, n)
    return {"vars": [[float(c[j]), ["Lower", 0.0, 0.0]] for j in range(n)],
            "constraints": [[[[j, float(A[i, j])] for j in range(n)], "Lte", float(b[i])] for i in range(m)]}


@pytest.mark.parametrize("name,what,which", [("blockdiag-afiro-6", "rhs", "dual"), ("blockdiag-afiro-6", "cost", "primal"),
                                              ("dense-400x900", "rhs", "dual")])
def test_larger_engines(name, what, which):
    fx = helpers.blockdiag(SC.netlib("afiro"), 6) if name.startswith("blockdiag") else _dense(20260301, 400, 900)
    # the cold solves of the 400-row LP are the primal solver's: its cold dual solve needs 9.1e5 loop bodies of phase 1 (30 s),
    # the primal 1.9e4 (0.7 s), and the optimal objective does not depend on the method
    coldwith = "primal" if name.startswith("dense") else "dual"
    cold0 = _cold(name, fx, coldwith)
    assert cold0.kind == "optimal"
    fx_new = SC.perturbed(fx, what, 0.05)
    cold = _solver(which if coldwith == "dual" else coldwith).solve(_A().Problem.from_fixture(fx_new))
    warm = _solver(which).solve(_A().Problem.from_fixture(fx_new), start=cold0.solution)
    print(name, what, which, "cold", cold.iters, "warm", warm.iters)
    assert cold.kind == "optimal" and warm.kind == "optimal"
    assert warm.start["used"] and warm.iters[0] == 0, warm.start
    assert _close(warm.solution.obj(), cold.solution.obj()), (warm.solution.obj(), cold.solution.obj())


def test_solve_without_a_start_is_untouched():
    import ctypes as C
    A = _A()
    for name in ("small_prob_1", "afiro", "adlittle"):
        fx = dict(FIXTURES)[name]
        for which, kind in (("primal", 0), ("dual", 1)):
            res = _solver(which).solve(A.Problem.from_fixture(fx))
            assert not hasattr(res, "start")
            r = A._Result()
            p = A.Problem.from_fixture(fx)
            A.host_lib().ellp_solve(p._h, kind, 100000, None, C.byref(r))
            try:
                x = np.ctypeslib.as_array(r.x, shape=(r.nx,)).copy()
                assert (r.iters_phase1, r.iters_phase2) == tuple(res.iters)
                assert (x.view(np.uint64) == res.solution.x().view(np.uint64)).all()
            finally:
                A.host_lib().ellp_result_free(C.byref(r))


def test_chained_resolves_need_no_ranging():
    """an Optimal result of solve(start=...) carries its basis: the next solve starts from it"""
    fx = SC.netlib("afiro")
    res = _cold("afiro", fx, "dual")
    for s in (0.05, 0.1):
        fx_new = SC.perturbed(fx, "rhs", s)
        res = _solver("dual").solve(_A().Problem.from_fixture(fx_new), start=res.solution)
        assert res.kind == "optimal" and res.start["used"] and res.iters[0] == 0
        ref = _solver("dual").solve(_A().Problem.from_fixture(fx_new))
        assert _close(res.solution.obj(), ref.solution.obj())
        assert set(res.solution.basis()) == {"B", "N", "Nb", "x", "row_origin"}

"""solve_batch(problems, starts=...) on the device: entry i is solve(problems[i], start=starts[i]) to the bit — kind, iters, obj,
x, .start and basis() — for both solvers, on the known-answer fixtures that have rows and nonbasic columns and on afiro,
adlittle and blend (27, 56 and 74 rows: all on the batched kernels).

The starts are the basis() of a first (dual) solve, whose indices are the standard form's own; the problems are then perturbed
as tests/start_cases.py perturbs them: the right-hand sides by 1 + s sin(k + 1) for the dual solver, the costs likewise for the
primal solver, s = 0.05.  One batch mixes used starts, a start of every reason 1 to 5 and None; the info counters show that
all mapped starts went into one ellp_batch_basis_start call and all used ones into one ellp_batch_solve_with_initial call.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import start_cases as SC  # noqa: E402
from test_gpu_start_api import FIXTURES  # noqa: E402

pytestmark = pytest.mark.gpu
S = 0.05
WHAT = {"primal": "cost", "dual": "rhs"}


def _A():
    import ellp_amd
    return ellp_amd


def _E():
    from ellp_amd import _engine as E
    return E


def _solver(which, **kw):
    A = _A()
    return (A.PrimalSimplexSolver if which == "primal" else A.DualSimplexSolver)(max_iter=100000, **kw)


_FIRST = {}


def first():
    """[(name, fixture, basis of the first solve)], once"""
    if not _FIRST:
        A = _A()
        out = []
        for name, fx in FIXTURES:
            res = _solver("dual").solve(A.Problem.from_fixture(fx), ranging=True)
            assert res.kind == "optimal", name
            out.append((name, fx, res.solution.basis()))
        _FIRST["all"] = out
    return _FIRST["all"]


def perturbed_problems(which):
    A = _A()
    return [A.Problem.from_fixture(SC.perturbed(fx, WHAT[which], S)) for _, fx, _ in first()]


def _same_value(tag, a, b):
    if isinstance(b, dict):
        assert isinstance(a, dict) and set(a) == set(b), (tag, a, b)
        for k in b:
            _same_value((tag, k), a[k], b[k])
    elif isinstance(b, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (tag, a, b)
    elif isinstance(b, float):
        assert np.float64(a).tobytes() == np.float64(b).tobytes(), (tag, a, b)
    else:
        assert a == b, (tag, a, b)


def _same(tag, got, ref, postsolve=False):
    """an entry of solve_batch(..., starts=...) against solve(p, start=s), or against the exception it raises"""
    if isinstance(ref, Exception):
        assert type(got) is type(ref) and str(got) == str(ref), (tag, got, ref)
        return
    assert not isinstance(got, Exception), (tag, got)
    assert (got.kind, tuple(got.iters)) == (ref.kind, tuple(ref.iters)), (tag, got.kind, ref.kind, got.iters, ref.iters)
    assert hasattr(got, "start") == hasattr(ref, "start"), tag
    if hasattr(ref, "start"):
        _same_value((tag, "start"), got.start, ref.start)
    if ref.kind == "optimal":
        _same_value((tag, "obj"), got.solution.obj(), ref.solution.obj())
        _same_value((tag, "x"), got.solution.x(), ref.solution.x())
        if hasattr(ref, "start"):
            _same_value((tag, "basis"), got.solution.basis(), ref.solution.basis())
        else:  # solve(p) without a start reports no basis; the batch with starts given always does
            assert set(got.solution.basis()) == {"B", "N", "Nb", "x", "row_origin"}, tag
        if postsolve:
            _same_value((tag, "duals"), got.solution.duals(), ref.solution.duals())
            _same_value((tag, "reduced_costs"), got.solution.reduced_costs(), ref.solution.reduced_costs())
            _same_value((tag, "kkt"), got.solution.kkt(), ref.solution.kkt())
    elif ref.kind == "maxiter":
        _same_value((tag, "obj"), got.obj, ref.obj)


def _single(solver, p, s, **kw):
    try:
        return solver.solve(p, start=s, **kw) if s is not None else solver.solve(p, **kw)
    except Exception as e:  # noqa: BLE001 — compared with what solve_batch hands back
        return e


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_every_entry_is_the_single_warm_solve(which):
    E = _E()
    ps = perturbed_problems(which)
    ss = [basis for _, _, basis in first()]
    solver = _solver(which)
    before = E.batch_solve_info()["calls"]
    got = solver.solve_batch(ps, starts=ss)
    info, after = E.batch_basis_start_info(), E.batch_solve_info()
    assert len(got) == len(ps)
    used = 0
    for (name, _, _), p, s, g in zip(first(), ps, ss, got):
        ref = _single(solver, p, s)
        _same((which, name), g, ref)
        print(which, name, "warm iters", tuple(g.iters), "used", g.start["used"], "reason", g.start["reason"])
        assert not g.start["used"] or g.iters[0] == 0, (name, g.iters, g.start)
        used += g.start["used"]
    assert used >= len(ps) - 2, used  # a small change keeps nearly every old basis feasible for the solver's method
    # every start was mapped (reason 0 or 3, 4): ONE call made all the points, two launches per chunk
    assert info == {"launches": 2, "batched": len(ps), "single": 0, "chunks": 1}
    # every used start has rows and nonbasic columns and at most 128 rows: ONE batched phase-2 call took them all; the cold batch
    # of the unused ones (if any) makes its own calls only for the dual solver
    kind = E.ENGINE_PRIMAL if which == "primal" else E.ENGINE_DUAL
    if used == len(ps):
        assert (after["calls"] - before, after["items"], after["kind"]) == (1, used, kind)
    else:
        assert after["calls"] - before >= 1


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_one_batch_mixes_used_starts_every_reason_and_none(which):
    A = _A()
    by_name = {name: (fx, basis) for name, fx, basis in first()}
    fx, basis = by_name["adlittle"]
    B = basis["B"]
    cols = len(basis["B"]) + len(basis["N"])
    what = WHAT[which]
    good = SC.perturbed(fx, what, S)
    # reason 3: adlittle with one more variable whose column is twice variable 0's, both basic (tests/test_gpu_start_api.py)
    nv = len(fx["vars"])
    fx2 = SC.perturbed(fx, "cost", 0.0)
    fx2["vars"].append([2.0 * abs(fx["vars"][0][0]) + 1.0, ["Lower", 0.0, 0.0]])
    for con in fx2["constraints"]:
        con[0] += [[nv, 2.0 * a] for j, a in con[0] if j == 0]
    B_cold2 = _solver("dual").solve(A.Problem.from_fixture(fx2), ranging=True).solution.basis()["B"].tolist()
    B2 = [0, nv] + [b for b in B_cold2 if b not in (0, nv)][:len(B) - 2]
    # reason 4: the old basis after the change the OTHER solver is made for (s = 0.3)
    other = SC.perturbed(fx, "rhs" if which == "primal" else "cost", 0.3)
    norows = {"vars": [[1.0, ["Lower", 0.5, 0.0]], [-1.0, ["TwoSided", 0.0, 2.0]]], "constraints": []}
    afx, abasis = by_name["afiro"]
    cases = [("used-adlittle", good, basis, 0),
             ("none", good, None, None),
             ("reason-1", good, dict(B=B[:-1]), 1),
             ("reason-2", good, dict(B=np.concatenate([B[:-1], [cols]])), 2),
             ("used-afiro", SC.perturbed(afx, what, S), abasis, 0),
             ("reason-3", fx2, dict(B=B2), 3),
             ("reason-4", other, basis, 4),
             ("reason-5", norows, dict(B=[]), 5),
             ("none-afiro", afx, None, None),
             ("used-blend", SC.perturbed(by_name["blend"][0], what, S), by_name["blend"][1], 0)]
    ps = [A.Problem.from_fixture(c[1]) for c in cases]
    ss = [c[2] for c in cases]
    solver = _solver(which)
    got = solver.solve_batch(ps, starts=ss)
    info = _E().batch_basis_start_info()
    for (label, _, s, reason), p, g in zip(cases, ps, got):
        ref = _single(solver, p, s)
        _same((which, label), g, ref)
        if reason is None:
            assert not hasattr(g, "start"), label
        else:
            assert g.start["reason"] == reason and g.start["used"] == (reason == 0), (label, g.start)
            if reason != 5:  # adlittle, afiro and blend need phase-1 iterations when solved cold: 0 exactly where the start was used
                assert (g.iters[0] == 0) == (reason == 0), (label, g.iters)
        if g.kind == "optimal":
            assert set(g.solution.basis()) == {"B", "N", "Nb", "x", "row_origin"}, label  # started or not
    # the mapped starts (used, reason 3, reason 4) were one call's items
    assert info == {"launches": 2, "batched": 5, "single": 0, "chunks": 1}


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_postsolve_matches_the_single_warm_solve(which):
    ps = perturbed_problems(which)
    ss = [basis for _, _, basis in first()]
    ss[1] = None
    solver = _solver(which)
    got = solver.solve_batch(ps, starts=ss, postsolve=True)
    for (name, _, _), p, s, g in zip(first(), ps, ss, got):
        _same((which, name), g, _single(solver, p, s, postsolve=True), postsolve=True)


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_a_two_round_chain(which):
    A = _A()
    fxs = [fx for _, fx, _ in first()]
    ps = [A.Problem.from_fixture(fx) for fx in fxs]
    solver = _solver(which)
    r1 = solver.solve_batch(ps, starts=[None] * len(ps))
    for (name, _, _), p, g in zip(first(), ps, r1):  # without a start: what solve(p) returns, and a basis on top
        ref = solver.solve(p)
        assert not hasattr(g, "start") and g.kind == ref.kind == "optimal", name
        assert tuple(g.iters) == tuple(ref.iters) and g.solution.x().tobytes() == ref.solution.x().tobytes(), name
        assert set(g.solution.basis()) == {"B", "N", "Nb", "x", "row_origin"}, name
    # round 2 from round 1's bases (a primal solve's basis may hold a phase-1 column: that start is reason 2, its solve cold)
    ps2 = [A.Problem.from_fixture(SC.perturbed(fx, WHAT[which], S)) for fx in fxs]
    ss = [r.solution if r.kind == "optimal" else None for r in r1]
    r2 = solver.solve_batch(ps2, starts=ss)
    used = 0
    for (name, _, _), p, s, g in zip(first(), ps2, ss, r2):
        _same((which, name, "round 2"), g, _single(solver, p, s.basis()))
        print(which, name, "round 2:", g.kind, tuple(g.iters), g.start["used"], g.start["reason"])
        if which == "dual" and name in ("afiro", "adlittle", "blend"):  # a dual solve's basis lives in the standard form's indices
            assert g.kind == "optimal" and g.start["used"] and g.iters[0] == 0, (name, g.kind, g.start)
        used += g.start["used"]
    assert used >= len(ps2) // 2, used


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_without_starts_nothing_changed(which):
    """starts=None: what solve(p) returns, as tests/test_gpu_batch.py compares it, and not one call of the start's"""
    A, E = _A(), _E()
    E.batch_basis_start([], 0)  # resets the counters of this thread
    ps = [A.Problem.from_fixture(fx) for _, fx, _ in first()]
    solver = _solver(which)
    got = solver.solve_batch(ps)
    assert E.batch_basis_start_info() == {"launches": 0, "batched": 0, "single": 0, "chunks": 0}
    for (name, _, _), p, g in zip(first(), ps, got):
        ref = _single(solver, p, None)
        assert not hasattr(g, "start")
        assert (g.kind, tuple(g.iters)) == (ref.kind, tuple(ref.iters)), name
        assert np.float64(g.solution.obj()).tobytes() == np.float64(ref.solution.obj()).tobytes(), name
        assert g.solution.x().tobytes() == ref.solution.x().tobytes(), name
        with pytest.raises(A.EllPError):
            g.solution.basis()

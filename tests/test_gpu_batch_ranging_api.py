"""solve_batch(problems, ranging=True) through the user API: every entry is what solve(p, ranging=True) returns — kind,
iteration counts, x, obj, cost_ranging(), rhs_ranging(), basis(), duals(), reduced_costs() and every kkt() entry as bytes, an
exception the same exception — from one ellp_batch_ranging call for the whole batch and no ellp_batch_postsolve call; the
same with starts from a first batch; without the flag solve_batch makes no such call."""
import numpy as np
import pytest

from helpers import known_answers
from test_gpu_batch import random_lp

pytestmark = pytest.mark.gpu
KA = known_answers()
_PS = []


def problems():
    """the fixtures of known_answers.json, an infeasible and an unbounded problem, the m == 0 problem, a problem with a
    redundant row (the rank check drops it) and 24 random LPs of up to 128 rows"""
    if not _PS:
        from ellp_amd import Problem
        fxs = [fx for fx in KA["problems"]]
        fxs.append({"vars": [[1.0, ["Lower", 0.0, 0.0]]], "constraints": [[[[0, 1.0]], "Lte", -1.0]]})           # infeasible
        fxs.append({"vars": [[-1.0, ["Lower", 0.0, 0.0]]], "constraints": [[[[0, 1.0]], "Gte", 1.0]]})            # unbounded
        fxs.append({"vars": [[1.0, ["Lower", 0.5, 0.0]], [-1.0, ["TwoSided", 0.0, 2.0]]], "constraints": []})    # m == 0
        # more equality rows than columns: the rank check keeps two and drops one (standard_form.rs:142-181)
        fxs.append({"vars": [[2.0, ["Lower", 0.0, 0.0]], [-1.0, ["Lower", 0.0, 0.0]]],
                    "constraints": [[[[0, -2.0], [1, -2.0]], "Eq", -8.0], [[[0, 2.0], [1, 1.0]], "Eq", 6.0], [[[0, 2.0]], "Eq", 4.0]]})
        sizes = [1, 2, 5, 16, 17, 33, 64, 65, 100, 127, 128, 40, 3, 8, 12, 20, 24, 30, 48, 56, 72, 80, 96, 112]
        fxs += [random_lp(np.random.default_rng(81000 + s), m) for s, m in enumerate(sizes)]
        _PS.extend(Problem.from_fixture(fx) for fx in fxs)
    return _PS


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).tobytes()


def _single(solver, p, **kw):
    try:
        return solver.solve(p, **kw)
    except Exception as e:  # noqa: BLE001 — compared with what solve_batch hands back
        return e


def _same(tag, got, ref):
    import ellp_amd
    if isinstance(ref, Exception):
        assert type(got) is type(ref) and str(got) == str(ref), (tag, got, ref)
        return
    assert not isinstance(got, Exception), (tag, got)
    assert (got.kind, got.iters) == (ref.kind, ref.iters), (tag, got.kind, ref.kind, got.iters, ref.iters)
    if ref.kind == ellp_amd.SolverResult.Optimal:
        g, r = got.solution, ref.solution
        assert _bits(g.obj()) == _bits(r.obj()), tag
        assert g.x().tobytes() == r.x().tobytes(), tag
        for what in ("cost_ranging", "rhs_ranging"):
            for a, b in zip(getattr(g, what)(), getattr(r, what)()):
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (tag, what)
        ba, bb = g.basis(), r.basis()
        assert set(ba) == set(bb) >= {"B", "N", "Nb", "x", "row_origin", "inverse_residual"}
        for key in bb:
            assert (_bits(ba[key]) == _bits(bb[key])) if key == "inverse_residual" else (ba[key].tobytes() == bb[key].tobytes()), (tag, key)
        assert g.duals().tobytes() == r.duals().tobytes(), tag
        assert g.reduced_costs().tobytes() == r.reduced_costs().tobytes(), tag
        k, k2 = g.kkt(), r.kkt()
        assert set(k) == set(k2)
        for key in k2:
            assert (_bits(k[key]) == _bits(k2[key])) if isinstance(k2[key], float) else (k[key] == k2[key]), (tag, key, k[key], k2[key])
    elif ref.kind == ellp_amd.SolverResult.MaxIter:
        assert _bits(got.obj) == _bits(ref.obj), tag


def _solver(which):
    import ellp_amd
    return (ellp_amd.PrimalSimplexSolver if which == "primal" else ellp_amd.DualSimplexSolver)()


def _zero_records():
    """an empty call of each: the records read 0 items, 0 launches, 0 chunks"""
    from ellp_amd import _engine as E
    E.batch_postsolve([])
    E.batch_ranging([])
    zero = {"launches": 0, "batched": 0, "single": 0, "chunks": 0}
    assert E.batch_postsolve_info() == zero and E.batch_ranging_info() == zero
    return zero


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_equal_to_solve_with_one_call(which):
    import ellp_amd
    from ellp_amd import _engine as E
    ps, solver = problems(), _solver(which)
    zero = _zero_records()
    got = solver.solve_batch(ps, ranging=True)
    info = E.batch_ranging_info()  # the calling thread's last ellp_batch_ranging: the one of this batch
    assert E.batch_postsolve_info() == zero  # and no ellp_batch_postsolve call
    assert len(got) == len(ps)
    refs = [_single(solver, p, ranging=True) for p in ps]
    kinds = [r.kind if not isinstance(r, Exception) else "error" for r in refs]
    assert "infeasible" in kinds and "unbounded" in kinds
    optimal_with_rows = 0
    for k, (g, ref) in enumerate(zip(got, refs)):
        _same((which, k), g, ref)
        if not isinstance(ref, Exception) and ref.kind == ellp_amd.SolverResult.Optimal and len(ref.solution.basis()["B"]) > 0:
            optimal_with_rows += 1
    assert optimal_with_rows >= 5  # the comparison is not empty
    # one call's worth: every Optimal problem with rows in its standard form is an item of it
    assert info["batched"] + info["single"] == optimal_with_rows and info["single"] == 0
    assert info["chunks"] == 1 and 1 <= info["launches"] <= 8
    # a row the rank check dropped: (0.0, 0.0, -1)
    red = got[len(KA["problems"]) + 3]
    assert red.kind == ellp_amd.SolverResult.Optimal and len(red.solution.basis()["B"]) == 2
    down, up, blk = red.solution.rhs_ranging()
    dropped = [i for i in range(3) if i not in set(red.solution.basis()["row_origin"])]
    assert len(dropped) == 1 and (down[dropped[0]], up[dropped[0]], tuple(blk[dropped[0]])) == (0.0, 0.0, (-1, -1))


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_equal_to_solve_with_starts_from_a_first_batch(which):
    import ellp_amd
    from ellp_amd import _engine as E
    ps, solver = problems(), _solver(which)
    first = solver.solve_batch(ps, ranging=True)
    starts = [r.solution if not isinstance(r, Exception) and r.kind == ellp_amd.SolverResult.Optimal else None for r in first]
    assert sum(s is not None for s in starts) >= 5
    zero = _zero_records()
    got = solver.solve_batch(ps, starts=starts, ranging=True)
    info = E.batch_ranging_info()
    assert E.batch_postsolve_info() == zero
    assert info["chunks"] == 1 and 1 <= info["launches"] <= 8
    used = 0
    for k, (p, g, s) in enumerate(zip(ps, got, starts)):
        ref = _single(solver, p, start=s, ranging=True) if s is not None else _single(solver, p, ranging=True)
        _same((which, "started", k), g, ref)
        if s is not None:
            assert g.start == ref.start, (which, k)
            used += bool(g.start["used"])
    assert used >= 1


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_unchanged_without_the_flag(which):
    from ellp_amd import _engine as E
    ps, solver = problems(), _solver(which)
    zero = _zero_records()
    plain = solver.solve_batch(ps)
    assert E.batch_ranging_info() == zero and E.batch_postsolve_info() == zero
    post = solver.solve_batch(ps, postsolve=True)
    assert E.batch_ranging_info() == zero and E.batch_postsolve_info() != zero
    import ellp_amd
    for g in plain + post:
        if not isinstance(g, Exception) and g.kind == ellp_amd.SolverResult.Optimal:
            with pytest.raises(ellp_amd.EllPError):
                g.solution.cost_ranging()

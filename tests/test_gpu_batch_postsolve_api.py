"""solve_batch(problems, postsolve=True) through the user API: every entry is what solve(p, postsolve=True) returns — kind,
iteration counts, x, obj, duals(), reduced_costs() and every kkt() entry as bytes, an exception the same exception — from
one ellp_batch_postsolve call for the whole batch; without the flag solve_batch is what it was, and makes no such call."""
import os

import numpy as np
import pytest

from helpers import GOLDEN, blockdiag, known_answers, read_mps
from test_gpu_batch import random_lp

pytestmark = pytest.mark.gpu
KA = known_answers()
_PS = []


def problems():
    """the fixtures of known_answers.json, the three netlib LPs, the m == 0 problem, blockdiag(adlittle, 3) (168 rows: the
    single path inside the call) and 12 random LPs"""
    if not _PS:
        from ellp_amd import Problem
        fxs = [fx for fx in KA["problems"]] + [read_mps(os.path.join(GOLDEN, f["file"])) for f in KA["netlib"]]
        fxs.append({"vars": [[1.0, ["Lower", 0.5, 0.0]], [-1.0, ["TwoSided", 0.0, 2.0]]], "constraints": []})  # m == 0
        fxs.append(blockdiag(read_mps(os.path.join(GOLDEN, "netlib", "adlittle.mps")), 3))
        fxs += [random_lp(np.random.default_rng(71000 + s), int(np.random.default_rng(72000 + s).integers(1, 40))) for s in range(12)]
        _PS.extend(Problem.from_fixture(fx) for fx in fxs)
    return _PS


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).tobytes()


def _single(solver, p, **kw):
    try:
        return solver.solve(p, **kw)
    except Exception as e:  # noqa: BLE001 — compared with what solve_batch hands back
        return e


def _same(tag, got, ref, post):
    import ellp_amd
    if isinstance(ref, Exception):
        assert type(got) is type(ref) and str(got) == str(ref), (tag, got, ref)
        return
    assert not isinstance(got, Exception), (tag, got)
    assert (got.kind, got.iters) == (ref.kind, ref.iters), (tag, got.kind, ref.kind, got.iters, ref.iters)
    if ref.kind == ellp_amd.SolverResult.Optimal:
        assert _bits(got.solution.obj()) == _bits(ref.solution.obj()), tag
        assert got.solution.x().tobytes() == ref.solution.x().tobytes(), tag
        if post:
            assert got.solution.duals().tobytes() == ref.solution.duals().tobytes(), tag
            assert got.solution.reduced_costs().tobytes() == ref.solution.reduced_costs().tobytes(), tag
            k, k2 = got.solution.kkt(), ref.solution.kkt()
            assert set(k) == set(k2)
            for key in k2:
                assert (_bits(k[key]) == _bits(k2[key])) if isinstance(k2[key], float) else (k[key] == k2[key]), (tag, key, k[key], k2[key])
        else:
            with pytest.raises(ellp_amd.EllPError):
                got.solution.duals()
    elif ref.kind == ellp_amd.SolverResult.MaxIter:
        assert _bits(got.obj) == _bits(ref.obj), tag


def _solver(which):
    import ellp_amd
    return (ellp_amd.PrimalSimplexSolver if which == "primal" else ellp_amd.DualSimplexSolver)()


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_equal_to_solve_with_one_call(which):
    import ellp_amd
    from ellp_amd import _engine as E
    ps, solver = problems(), _solver(which)
    got = solver.solve_batch(ps, postsolve=True)
    info = E.batch_postsolve_info()  # the calling thread's last ellp_batch_postsolve: the one of this batch
    assert len(got) == len(ps)
    refs = [_single(solver, p, postsolve=True) for p in ps]
    optimal_with_rows = 0
    for k, (p, g, ref) in enumerate(zip(ps, got, refs)):
        _same((which, k), g, ref, True)
        if not isinstance(ref, Exception) and ref.kind == ellp_amd.SolverResult.Optimal and len(ref.solution.duals()) > 0:
            optimal_with_rows += 1
    assert optimal_with_rows > 10
    # one call's worth: every Optimal problem with rows is an item of it, the 168-row one on the single path inside it
    # (a problem whose constraints all drop out of the standard form has m == 0 and is answered on the host)
    assert optimal_with_rows - 2 <= info["batched"] + info["single"] <= optimal_with_rows
    assert info["chunks"] == 1 and 1 <= info["launches"] <= 4
    big = got[len(KA["problems"]) + len(KA["netlib"]) + 1]
    if not isinstance(big, Exception) and big.kind == ellp_amd.SolverResult.Optimal:
        assert info["single"] == 1


def test_c_entry_without_the_flag_is_ellp_solve_batch():
    """ellp_solve_batch_ex(..., postsolve = 0): the results of ellp_solve_batch, has_postsolve = 0, no ellp_batch_postsolve call"""
    import ctypes as C

    import ellp_amd
    from ellp_amd import _engine as E
    ps = problems()[:len(KA["problems"])]
    n = len(ps)
    L = ellp_amd.host_lib()
    handles = (C.c_void_p * n)(*[p._h for p in ps])
    E.batch_postsolve([])
    before = E.batch_postsolve_info()
    rxs, rs = (ellp_amd._ResultEx * n)(), (ellp_amd._Result * n)()
    try:
        assert L.ellp_solve_batch_ex(handles, n, ellp_amd.PrimalSimplexSolver._KIND, 1000, None, 0, rxs) == E.OPTIMAL
        assert L.ellp_solve_batch(handles, n, ellp_amd.PrimalSimplexSolver._KIND, 1000, None, rs) == E.OPTIMAL
        assert E.batch_postsolve_info() == before
        for rx, r in zip(rxs, rs):
            assert rx.has_postsolve == 0 and not rx.duals and not rx.reduced_costs
            a, b = rx.result, r
            assert (a.status, a.iters_phase1, a.iters_phase2, a.nx, a.err) == (b.status, b.iters_phase1, b.iters_phase2, b.nx, b.err)
            assert _bits(a.obj) == _bits(b.obj)
            if a.nx:
                assert np.ctypeslib.as_array(a.x, shape=(a.nx,)).tobytes() == np.ctypeslib.as_array(b.x, shape=(b.nx,)).tobytes()
    finally:
        for rx in rxs:
            L.ellp_result_ex_free(C.byref(rx))
        for r in rs:
            L.ellp_result_free(C.byref(r))


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_unchanged_without_the_flag(which):
    from ellp_amd import _engine as E
    ps, solver = problems(), _solver(which)
    E.batch_postsolve([])  # an empty call: the record reads 0 items, 0 launches, 0 chunks
    before = E.batch_postsolve_info()
    assert before == {"launches": 0, "batched": 0, "single": 0, "chunks": 0}
    got = solver.solve_batch(ps)
    assert E.batch_postsolve_info() == before  # not one ellp_batch_postsolve call
    for k, (p, g) in enumerate(zip(ps, got)):
        _same((which, "plain", k), g, _single(solver, p), False)

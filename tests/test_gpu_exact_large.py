"""pipeline = 3 from 1,025 to 8,192 rows: the LU-per-iteration loop over all CUs (run_exact_large: the blocked LU of ellp_lu.hip,
k_lu_solve, the engine's bandwidth kernels fed the exact u / rho and B^-1 a_q) as an engine of its own, selected by the caller —
from the first slice on, through both phase hand-offs, with no hybrid, certificate or redo.  Status, iteration count and basis
are the oracle's; x (y, d) to 1e-11 (1 + max|.|), the tolerance tests/test_gpu_hybrid.py sets for the same loop as a redo (the
L^T solve sums in another order, ellp_exact.inc).  All cases at m = 1,100; the oracle's runs are computed once and shared."""
import functools

import numpy as np
import pytest

from oracle import ellp_oracle as eo
from test_gpu_hybrid import _quick_primal_start

pytestmark = pytest.mark.gpu
M_ROWS = 1100
PHASE2_BODIES = 200  # the primal phase 2 of this start needs 2,093 loop bodies: both sides run the first 200 of them


def _E():
    from ellp_amd import _engine as E
    return E


class _V:
    pass


def _view(f):
    ov = _V()
    for k, val in f.items():
        setattr(ov, k, val.copy() if hasattr(val, "copy") else val)
    ov.nB, ov.nN = len(f["B"]), len(f["N"])
    return ov


def _start(which):
    from ellp_amd import synth
    return _quick_primal_start(9, M_ROWS, 40, 5) if which == "primal" else synth.dual_start_flat(9, M_ROWS, 40)


@functools.lru_cache(maxsize=None)
def _oracle(which):
    """(end point, status, loop bodies) of the oracle on the start of `which`; never modified by the tests"""
    ov = _view(_start(which))
    st, it, _ = (eo.primal_solve_with_initial if which == "primal" else eo.dual_solve_with_initial)(ov, 100000)
    assert st == eo.OPTIMAL and 100 < it < 1000, (st, it)
    return ov, st, it


def _flat(f):
    E = _E()
    return E.FlatProblem(f["m"], f["n"], f["n_c"], f["A"], f["c"], f["b"], f["kind"], f["lb"], f["ub"], f["x"], f["B"], f["N"], f["Nb"],
                         f.get("y"), f.get("d"))


def _engine(which, f, **opts):
    E = _E()
    fp = _flat(f)
    return fp, E.Engine(E.ENGINE_PRIMAL if which == "primal" else E.ENGINE_DUAL, fp, E.default_opts(pipeline=3, **opts))


def _same_point(which, fp, ov):
    np.testing.assert_array_equal(fp.B, ov.B)
    np.testing.assert_array_equal(np.sort(fp.N[:fp.nN]), np.sort(ov.N[:ov.nN]))
    np.testing.assert_allclose(fp.x, ov.x, rtol=0, atol=1e-11 * (1.0 + np.abs(ov.x).max()))
    if which == "dual":
        np.testing.assert_allclose(fp.y, ov.y, rtol=0, atol=1e-11 * (1.0 + np.abs(ov.y).max()))
        np.testing.assert_allclose(fp.d, ov.d, rtol=0, atol=1e-11 * (1.0 + np.abs(ov.d).max()))


def _exact_loop_alone(c, bodies):
    assert c["hybrid_exact_iters"] == bodies and c["hybrid_redos"] == 0, c
    assert not c["hybrid"] and not c["certified_by_exact_lu_iteration"], c


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_pipeline_3_above_1024_rows_is_the_exact_loop(which):
    """fails on an engine that falls through to the plain explicit-inverse loop: that one counts no exact loop bodies"""
    ov, st_o, it_o = _oracle(which)
    fp, eng = _engine(which, _start(which), max_iter=100000)
    try:
        st, stats, msg = eng.run(100000)
        eng.read_point()
        c = eng.counters()
    finally:
        eng.close()
    assert st == st_o and int(stats.iters) == it_o, (st, stats.iters, it_o, msg)
    _same_point(which, fp, ov)
    _exact_loop_alone(c, int(stats.iters))


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_slices_compose(which):
    ov, st_o, it_o = _oracle(which)
    fp, eng = _engine(which, _start(which), max_iter=100000)
    try:
        s1, t1, _ = eng.run(1)
        s2, t2, _ = eng.run(2)
        assert (s1, s2) == (_E().MAXITER, _E().MAXITER) and (int(t1.iters), int(t2.iters)) == (1, 3)
        st, stats, msg = eng.run(100000)
        eng.read_point()
        c = eng.counters()
    finally:
        eng.close()
    assert st == st_o and int(stats.iters) == it_o, (st, stats.iters, it_o, msg)
    _same_point(which, fp, ov)
    _exact_loop_alone(c, it_o)


def test_the_budget_ends_the_loop_one_body_short():
    E = _E()
    _, _, it_o = _oracle("dual")
    fp, eng = _engine("dual", _start("dual"), max_iter=it_o - 1)
    try:
        st, stats, msg = eng.run(it_o - 1)
        c = eng.counters()
    finally:
        eng.close()
    assert st == E.MAXITER and int(stats.iters) == it_o - 1, (st, stats.iters, msg)
    _exact_loop_alone(c, it_o - 1)


@pytest.mark.parametrize("n,budget", [(40, PHASE2_BODIES), (20, 100000)], ids=["first-200-bodies-of-phase-2", "both-phases-to-the-end"])
def test_primal_rephase_keeps_the_exact_loop(n, budget):
    """phase 1, then the phase-2 costs and bounds (primal_problem.rs:263-291) on the resident engine: the oracle's two calls, the
    second from the oracle's own phase-1 end point.  From the start every other case uses (40 structural columns) phase 2 needs
    2,093 loop bodies: both sides run PHASE2_BODIES of them (a budget is part of the loop's contract: MaxIter after exactly that
    many bodies, same basis).  From the same start with 20 structural columns the oracle needs 53 + 113 bodies: both phases run
    to Optimal, which also covers the rebuild of the inverse at the end of a solve after a re-phasing."""
    from ellp_amd import synth
    E = _E()
    if n == 40:
        f = _start("primal")
        ov, st_o, it_o = _oracle("primal")
    else:
        f = _quick_primal_start(9, M_ROWS, n, 5)
        ov = _view(f)
        st_o, it_o, _ = eo.primal_solve_with_initial(ov, 100000)
        assert st_o == eo.OPTIMAL and it_o < 400, (st_o, it_o)
    f2 = synth.primal_phase2_from(f, ov.x, ov.B, ov.N[:ov.nN], ov.Nb[:ov.nN])
    ov2 = _view(f2)
    st_o2, it_o2, _ = eo.primal_solve_with_initial(ov2, budget)
    if n == 40:
        assert st_o2 == eo.MAXITER and it_o2 == PHASE2_BODIES, (st_o2, it_o2)
    else:
        assert st_o2 == eo.OPTIMAL and 0 < it_o2 < 400, (st_o2, it_o2)
    fp, eng = _engine("primal", f, max_iter=100000)
    try:
        st, stats, msg = eng.run(100000)
        eng.read_point()
        assert st == st_o and int(stats.iters) == it_o, (st, stats.iters, msg)
        _same_point("primal", fp, ov)
        eng.rephase(f2["c"], f2["kind"], f2["lb"], f2["ub"])
        st2, stats2, msg2 = eng.run(budget)
        eng.read_point()
        c = eng.counters()
    finally:
        eng.close()
    assert st2 == st_o2 and int(stats2.iters) == it_o2, (st2, stats2.iters, it_o2, msg2)
    _same_point("primal", fp, ov2)
    _exact_loop_alone(c, it_o + it_o2)


def test_dual_rephase_keeps_the_exact_loop():
    """tests/test_gpu_dual_rephase.py's case on the family at 1,100 x 20 (the oracle needs 325 + 391 loop bodies): phase 1 on
    the engine, its end point handed to the oracle's own DualPhase2::from, then phase 2 from both"""
    E = _E()
    d1, err = eo.dual_phase1(eo.synth_problem(9, M_ROWS, 20))
    assert d1 is not None and not err
    v1 = d1.view()
    ov1 = v1.copy()
    st_o1, it_o1, _ = eo.dual_solve_with_initial(ov1, 100000)
    assert st_o1 == eo.OPTIMAL and it_o1 < 400, (st_o1, it_o1)
    fp = E.FlatProblem(v1.m, v1.n, v1.n_c, v1.A, v1.c, v1.b, v1.kind, v1.lb, v1.ub, v1.x, v1.B, v1.N[:v1.nN], v1.Nb[:v1.nN], v1.y, v1.d)
    eng = E.Engine(E.ENGINE_DUAL, fp, E.default_opts(max_iter=100000, pipeline=3))
    try:
        st1, stats1, msg1 = eng.run(100000)
        eng.read_point()
        assert st1 == st_o1 and int(stats1.iters) == it_o1, (st1, stats1.iters, it_o1, msg1)
        _same_point("dual", fp, ov1)
        d1.store_point(ov1)
        d2, err2 = eo.dual_phase2(d1)
        assert d2 is not None and not err2
        v2 = d2.view()
        ov2 = v2.copy()
        st_o2, it_o2, _ = eo.dual_solve_with_initial(ov2, 100000)
        assert st_o2 == eo.OPTIMAL and it_o2 < 400, (st_o2, it_o2)
        eng.dual_rephase(v2.c, v2.b, v2.kind, v2.lb, v2.ub)
        eng.read_point()
        np.testing.assert_array_equal(fp.N, v2.N[:v2.nN])  # variable order
        st2, stats2, msg2 = eng.run(100000)
        eng.read_point()
        c = eng.counters()
    finally:
        eng.close()
    assert st2 == st_o2 and int(stats2.iters) == it_o2, (st2, stats2.iters, it_o2, msg2)
    _same_point("dual", fp, ov2)
    _exact_loop_alone(c, it_o1 + it_o2)


def _all_kinds_start(seed, m=1030, n=60):
    """A primal feasible start with every bound kind among the basic and the nonbasic variables: n sparse structural columns
    (nonbasic on a bound, Free ones at 0) and an identity of m basic columns whose values lie inside their bounds, except a few
    that sit exactly on one (degenerate rows).  TwoSided and Fixed basics are kept few: a TwoSided basic with d_i < 0 bounds
    the step by 0 wherever it stands (quirk Q1), so with many of them no body would move x."""
    rng = np.random.default_rng(seed)
    ncols = n + m
    A = np.zeros((m, ncols), order="F")
    A[:, :n] = np.where(rng.random((m, n)) < 0.05, rng.normal(size=(m, n)), 0.0)
    A[np.arange(m), n + np.arange(m)] = 1.0
    kind = np.empty(ncols, dtype=np.uint8)
    kind[:n] = np.arange(n) % 5
    kind[n:] = rng.choice([0, 1, 2, 3, 4], size=m, p=[0.05, 0.55, 0.38, 0.015, 0.005])
    lb, ub, x = np.zeros(ncols), np.zeros(ncols), np.zeros(ncols)
    w = 0.5 + rng.random(ncols)           # distance to the one bound / half width of a box
    t = rng.random(ncols)                 # where a basic variable stands inside
    t[rng.random(ncols) < 0.004] = 0.0    # a few exactly on a bound
    t[rng.random(ncols) < 0.004] = 1.0
    two = n + np.where(kind[n:] == 3)[0]  # the few TwoSided basics: at lb, at ub, inside, in turn
    t[two[0::3]], t[two[1::3]] = 0.0, 1.0
    Nb = np.zeros(n, dtype=np.uint8)
    for j in range(ncols):
        k, basic = kind[j], j >= n
        if k == 0:
            x[j] = (t[j] - 0.5) if basic else 0.0
        elif k == 1:
            lb[j] = -w[j]
            x[j] = lb[j] + (t[j] * w[j] if basic else 0.0)
        elif k == 2:
            ub[j] = w[j]
            x[j] = ub[j] - (t[j] * w[j] if basic else 0.0)
        elif k == 3:
            lb[j], ub[j] = -w[j], w[j]
            x[j] = lb[j] + (t[j] if basic else float(j % 2)) * 2 * w[j]
        else:
            lb[j] = ub[j] = x[j] = t[j] - 0.5
        if not basic:
            Nb[j] = 2 if k == 0 else (1 if (k == 2 or (k == 3 and j % 2)) else 0)
    b = np.zeros(m)
    for j in range(ncols):
        if x[j] != 0.0:
            b += A[:, j] * x[j]
    c = np.zeros(ncols)
    c[:n] = rng.normal(size=n)
    return dict(m=m, n=ncols, n_c=ncols, A=A.reshape(-1, order="F"), c=c, b=b, kind=kind, lb=lb, ub=ub, x=x,
                B=np.arange(n, ncols, dtype=np.int64), N=np.arange(n, dtype=np.int64), Nb=Nb)


def test_every_bound_kind_reaches_the_exact_ratio_test():
    """The starts above are all-Lower (with Fixed artificials in phase 2), so of the bounded ratio lambda_i (primal…:320-367,
    primal_lambda in ellp_rules.inc) k_exact_relam only ever took the Lower and Fixed branches.  Here: m = 1,030 (the smallest
    size class above k_mid), 60 structural columns, all five bound kinds basic and nonbasic, the first 30 loop bodies; status,
    body count and basis are the oracle's, x to this file's tolerance.

    Seed 2, chosen on the CPU from the oracle's run: it neither ends nor panics within the 30 bodies, 11 of them move x, and
    over the 30 x 1,030 rows the branches are taken |d_i| < EPS 25,166 times; Free 369; Lower: d_i > 0 1,474, x_i > lb 1,504,
    else 0 twice; Upper: d_i > 0 and x_i < ub 1,102, d_i > 0 else 0 twice, d_i <= 0 1,217; TwoSided: d_i > 0 and x_i < ub 39,
    d_i > 0 else 0 four times, d_i <= 0 else 0 19 times; Fixed twice.  The division of quirk Q1 (TwoSided, d_i <= 0,
    x_i < lb) is not reachable from a feasible point: its lambda_i is negative and ends the loop by the panic of primal…:402."""
    E = _E()
    f = _all_kinds_start(2)
    assert sorted(set(f["kind"][f["B"]])) == sorted(set(f["kind"][f["N"]])) == [0, 1, 2, 3, 4]
    ov = _view(f)
    st_o, it_o, _ = eo.primal_solve_with_initial(ov, 30)
    assert st_o == eo.MAXITER and it_o == 30, (st_o, it_o)
    fp, eng = _engine("primal", f, max_iter=30)
    try:
        st, stats, msg = eng.run(30)
        eng.read_point()
        c = eng.counters()
    finally:
        eng.close()
    assert st == E.MAXITER and int(stats.iters) == 30, (st, stats.iters, msg)
    _same_point("primal", fp, ov)
    _exact_loop_alone(c, 30)


def test_sharding_and_stepping_are_refused():
    E = _E()
    fp, eng = _engine("dual", _start("dual"), max_iter=100000)
    try:
        with pytest.raises(E.EllpHipError) as ex:
            eng.set_shard(0, 2)
        assert ex.value.status == E.ERR_ARG and "pipeline 3" in ex.value.msg
        with pytest.raises(E.EllpHipError) as ex:
            eng.step(0)
        assert ex.value.status == E.ERR_ARG and "pipeline 3" in ex.value.msg
    finally:
        eng.close()


def test_bound_flipping_above_1024_rows_is_still_refused():
    E = _E()
    with pytest.raises(E.EllpHipError) as ex:
        E.Engine(E.ENGINE_DUAL, _flat(_start("dual")), E.default_opts(max_iter=100000, pipeline=3, flags=E.FLAG_DUAL_BOUND_FLIPPING))
    assert ex.value.status == E.ERR_ARG and "1,024 rows" in ex.value.msg

"""Batched solves of mid-size LPs (129 to 1,024 rows, k_mid_batch): every item must end exactly as the single seam call
with the same options ends it, and as the oracle — status, iteration counts, B, N, Nb and the bits of x (y, d) — for both
kinds and phases, at every mid workgroup size, next to small and refused items, across relaunches and chunks, with the
dual's extensions, and through the user API against solve()."""
import os

import numpy as np
import pytest

from helpers import GOLDEN, blockdiag, known_answers, permuted_fixture, read_mps
from oracle import ellp_oracle as eo
from test_gpu_small import assert_identical, flat

pytestmark = pytest.mark.gpu
MI = 100000
BUDGET = 25  # loop bodies for the dense synthetic LPs: they end at MAXITER


def _E():
    from ellp_amd import _engine as E
    return E


def _netlib(name, copies, seed):
    ka = next(p for p in known_answers()["netlib"] if p["name"] == name)
    return permuted_fixture(blockdiag(read_mps(os.path.join(GOLDEN, ka["file"])), copies), np.random.default_rng(seed))


NETLIB = [("blend", 2, 11), ("blend", 2, 12), ("adlittle", 3, 13), ("adlittle", 3, 14), ("adlittle", 6, 15)]
DENSE = [(300, 700), (650, 1300)]

_CASES = {}


class Case:
    """one phase of one LP at the seam: its view, and the oracle's end of it under max_iter"""

    def __init__(self, tag, view, max_iter):
        fn = eo.primal_solve_with_initial if tag[0] == "primal" else eo.dual_solve_with_initial
        self.tag, self.v, self.max_iter = tag, view, max_iter
        self.o = view.copy()
        self.r = fn(self.o, max_iter)


def cases(which):
    """phase 1 and phase 2 of the netlib replications (to the end), phase 1 of the dense LPs (under BUDGET)"""
    if which in _CASES:
        return _CASES[which]
    out = []
    for name, copies, seed in NETLIB:
        prob = eo.Problem.from_fixture(_netlib(name, copies, seed))
        p1, err = eo.primal_phase1(prob) if which == "primal" else eo.dual_phase1(prob)
        assert p1 is not None and not err
        c1 = Case((which, name, copies, seed, 1), p1.view(), MI)
        assert 128 < c1.v.m <= 1024
        out.append(c1)
        assert c1.r[0] == eo.OPTIMAL
        p1.store_point(c1.o)
        if which == "primal":
            v2 = eo.primal_phase2(p1).view()
        else:
            p2, err2 = eo.dual_phase2(p1)
            assert p2 is not None and not err2
            v2 = p2.view()
        out.append(Case((which, name, copies, seed, 2), v2, MI))
    for m, n in DENSE:
        synth = eo.synth_problem(20260301 + m, m, n)
        p1, err = eo.primal_phase1(synth) if which == "primal" else eo.dual_phase1(synth)
        out.append(Case((which, "dense", m, n, 1), p1.view(), BUDGET))
    _CASES[which] = out
    return out


def kind_of(which):
    E = _E()
    return E.ENGINE_PRIMAL if which == "primal" else E.ENGINE_DUAL


def single(which, fp, opts):
    E = _E()
    return (E.primal_solve_with_initial if which == "primal" else E.dual_solve_with_initial)(fp, opts)


def same_as_single(tag, which, fp, res, view, opts):
    """the batch's item equals the single seam call with the same options, to the bit"""
    one = flat(view)
    st1, stats1, msg1 = single(which, one, opts)
    st, stats, msg = res
    assert (st, stats.iters, stats.pivots, msg) == (st1, stats1.iters, stats1.pivots, msg1), (tag, st, st1, msg, msg1)
    if st1 < 0:
        return
    for a in ("x", "B", "N", "Nb") + (("y", "d") if which == "dual" else ()):
        assert getattr(fp, a).tobytes() == getattr(one, a).tobytes(), (tag, a)
    assert np.float64(stats.obj).tobytes() == np.float64(stats1.obj).tobytes(), tag


def run_batch(which, cs, opts_of, check_single=False):
    """one batch call per max_iter over the cases; every item against the oracle (and the single call)"""
    E = _E()
    for mi in sorted({c.max_iter for c in cs}):
        sub = [c for c in cs if c.max_iter == mi]
        fps = [flat(c.v) for c in sub]
        res = E.batch_solve_with_initial(kind_of(which), fps, opts_of(mi))
        for c, fp, (st, stats, msg) in zip(sub, fps, res):
            assert_identical(c.tag, c.o, *c.r, fp, st, stats, msg, which)
            if check_single:
                same_as_single(c.tag, which, fp, (st, stats, msg), c.v, opts_of(mi))


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_mid_batch_bit_for_bit(which):
    E = _E()
    cs = cases(which)
    assert {256, 512, 1024} == {256 if c.v.m <= 256 else (512 if c.v.m <= 512 else 1024) for c in cs}
    assert sum(c.r[0] == eo.MAXITER for c in cs) >= 2
    run_batch(which, cs, lambda mi: E.default_opts(max_iter=mi, pipeline=3), check_single=True)


def _small_views(which):
    """AFIRO's and a small random LP's phase 1: items of k_small_batch"""
    afiro = read_mps(os.path.join(GOLDEN, "netlib", "afiro.mps"))
    out = []
    for fx in (afiro, blockdiag(afiro, 2)):
        prob = eo.Problem.from_fixture(fx)
        p1, _ = eo.primal_phase1(prob) if which == "primal" else eo.dual_phase1(prob)
        out.append(Case((which, "small", p1.view().m), p1.view(), MI))
    return out


def _item_1025(which):
    from test_batch_cpu import _item
    fp = _item(1025, 3)
    if which == "dual":
        fp.y, fp.d = np.zeros(fp.m), np.zeros(fp.n_c)
    return fp


def _bad_items(which, v):
    """copies of a mid view the single call refuses: a basis of the wrong size; for the dual a start that is not dual
    feasible (a nonbasic at its lower bound with d < 0)"""
    dims = flat(v)
    dims.nB = dims.m - 1  # ELLP_ERR_BAD_DIMS
    out = [dims]
    if which == "dual":
        nf = flat(v)
        j = next(k for k in range(nf.nN) if nf.Nb[k] == 0)
        nf.d[nf.N[j]] = -1.0
        out.append(nf)
    return out


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_mixed_small_mid_and_refused(which):
    E = _E()
    opts = E.default_opts(max_iter=MI, pipeline=3)
    good = _small_views(which) + [c for c in cases(which) if c.max_iter == MI][:4]
    fps = [flat(c.v) for c in good]
    tall = _item_1025(which)
    bad = _bad_items(which, good[-1].v)
    mixed = fps[:1] + [tall] + fps[1:3] + bad + fps[3:]
    res = E.batch_solve_with_initial(kind_of(which), mixed, opts)
    at = {id(fp): r for fp, r in zip(mixed, res)}
    assert at[id(tall)][0] == E.ERR_ARG and "1024 rows" in at[id(tall)][2]
    for b, b1 in zip(bad, _bad_items(which, good[-1].v)):
        st1, stats1, msg1 = single(which, b1, opts)
        assert st1 < 0 and (at[id(b)][0], at[id(b)][2]) == (st1, msg1)
    for c, fp in zip(good, fps):
        assert_identical(c.tag, c.o, *c.r, fp, *at[id(fp)], which)


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_relaunches_and_chunks(which, monkeypatch):
    E = _E()
    cs = _small_views(which) + cases(which)
    monkeypatch.setenv("ELLP_BATCH_LAUNCH_ITERS", "7")
    run_batch(which, cs, lambda mi: E.default_opts(max_iter=mi, pipeline=3))
    monkeypatch.delenv("ELLP_BATCH_LAUNCH_ITERS")
    monkeypatch.setenv("ELLP_BATCH_MAX_BYTES", str(4 << 20))  # a few items per chunk
    run_batch(which, cs, lambda mi: E.default_opts(max_iter=mi, pipeline=3))


@pytest.mark.parametrize("flags", ["maxviol", "bflip", "both"])
def test_dual_extensions_match_the_single_call(flags):
    E = _E()
    f = {"maxviol": E.FLAG_DUAL_MAX_VIOLATION, "bflip": E.FLAG_DUAL_BOUND_FLIPPING,
         "both": E.FLAG_DUAL_MAX_VIOLATION | E.FLAG_DUAL_BOUND_FLIPPING}[flags]
    pipeline = 3 if flags == "maxviol" else 0  # bound flipping selects k_mid at pipeline 0
    cs = cases("dual")
    for mi in (MI, BUDGET):
        sub = [c for c in cs if c.max_iter == mi]
        fps = [flat(c.v) for c in sub]
        opts = E.default_opts(max_iter=mi, flags=f, pipeline=pipeline)
        res = E.batch_solve_with_initial(E.ENGINE_DUAL, fps, opts)
        for c, fp, r in zip(sub, fps, res):
            assert r[0] != E.ERR_ARG, (c.tag, r[2])
            same_as_single((flags,) + c.tag, "dual", fp, r, c.v, opts)


def test_mid_auto_max(monkeypatch):
    E = _E()
    monkeypatch.setenv("ELLP_MID_AUTO_MAX", "200")
    cs = [c for c in cases("primal") if c.tag[1] == "adlittle" and c.tag[4] == 1]
    c168 = next(c for c in cs if c.v.m == 168)
    c336 = next(c for c in cs if c.v.m == 336)
    fps = [flat(c168.v), flat(c336.v)]
    opts = E.default_opts(max_iter=MI)
    res = E.batch_solve_with_initial(E.ENGINE_PRIMAL, fps, opts)
    assert_identical(c168.tag, c168.o, *c168.r, fps[0], *res[0], "primal")
    same_as_single(c168.tag, "primal", fps[0], res[0], c168.v, opts)
    assert res[1][0] == E.ERR_ARG and "336" in res[1][2]


def _same(tag, got, ref):
    import ellp_amd
    if isinstance(ref, Exception):
        assert type(got) is type(ref) and str(got) == str(ref), (tag, got, ref)
        return
    assert not isinstance(got, Exception), (tag, got)
    assert (got.kind, got.iters) == (ref.kind, ref.iters), (tag, got.kind, ref.kind, got.iters, ref.iters)
    if ref.kind == ellp_amd.SolverResult.Optimal:
        assert np.float64(got.solution.obj()).tobytes() == np.float64(ref.solution.obj()).tobytes(), tag
        assert got.solution.x().tobytes() == ref.solution.x().tobytes(), tag
    elif ref.kind == ellp_amd.SolverResult.MaxIter:
        assert np.float64(got.obj).tobytes() == np.float64(ref.obj).tobytes(), tag


def _single_solve(solver, p):
    try:
        return solver.solve(p)
    except Exception as e:  # noqa: BLE001 — compared with what solve_batch hands back
        return e


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_user_api_equals_solve(which):
    import ellp_amd
    from ellp_amd import Problem
    KA = known_answers()
    fxs = [_netlib("blend", 2, 21), _netlib("adlittle", 3, 22), _netlib("adlittle", 6, 23)]
    fxs += [read_mps(os.path.join(GOLDEN, "netlib", "afiro.mps"))] + list(KA["problems"][:4])
    infeasible = {"vars": [[1.0, ["Lower", 0.0, 0.0]]], "constraints": [[[[0, 1.0]], "Gte", 2.0], [[[0, 1.0]], "Lte", 1.0]]}
    fxs.append(blockdiag(infeasible, 70))  # 140 rows, infeasible
    ps = [Problem.from_fixture(fx) for fx in fxs]
    cls = ellp_amd.PrimalSimplexSolver if which == "primal" else ellp_amd.DualSimplexSolver
    kinds = set()
    for solver in (cls.new(MI, pipeline=3), cls.new(40, pipeline=3)):
        got = solver.solve_batch(ps)
        assert len(got) == len(ps)
        for k, (p, g) in enumerate(zip(ps, got)):
            ref = _single_solve(solver, p)
            _same((which, solver.max_iter, k), g, ref)
            kinds.add(type(ref).__name__ if isinstance(ref, Exception) else ref.kind)
    assert {"optimal", "infeasible", "maxiter"} <= kinds

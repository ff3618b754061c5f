"""Batched solves of many small LPs (ellp_batch_solve_with_initial; PrimalSimplexSolver / DualSimplexSolver.solve_batch):
every LP of a batch must end exactly as it ends alone — status, iteration counts, index sets and the bits of x (y, d) —
at the seam against the oracle, next to items that fail, across launch slices, with the dual's extensions, and through
the user API against solve()."""
import os

import numpy as np
import pytest

from helpers import GOLDEN, blockdiag, known_answers, read_mps
from oracle import ellp_oracle as eo
from test_gpu_small import assert_identical, flat

pytestmark = pytest.mark.gpu
KA = known_answers()
MI = 5000


def _E():
    from ellp_amd import _engine as E
    return E


def random_lp(rng, m):
    """an LP of m constraints with every bound kind and every constraint kind (integer data half of the time: ties)"""
    n = int(rng.integers(1, m + 40))
    dens = float(rng.choice([0.1, 0.3, 0.6])) if m > 20 else float(rng.choice([0.3, 0.6, 1.0]))
    integer = rng.random() < 0.5
    vars_ = []
    for _ in range(n):
        c = float(rng.integers(-4, 5)) if integer else float(rng.normal())
        k = rng.choice(["Lower", "Lower", "Upper", "TwoSided", "Free", "Fixed"], p=[0.35, 0.15, 0.15, 0.2, 0.1, 0.05])
        lo = float(rng.integers(-3, 3)) if integer else float(rng.normal())
        hi = lo + (float(rng.integers(1, 5)) if integer else float(abs(rng.normal()) + 0.1))
        vars_.append([c, {"Lower": ["Lower", lo, 0.0], "Upper": ["Upper", 0.0, hi], "TwoSided": ["TwoSided", lo, hi],
                          "Free": ["Free", 0.0, 0.0], "Fixed": ["Fixed", lo, lo]}[k]])
    cons = []
    for _ in range(m):
        coeffs = []
        for j in range(n):
            if rng.random() < dens:
                a = float(rng.integers(-3, 4)) if integer else float(rng.normal())
                if a != 0.0:
                    coeffs.append([j, a])
        op = str(rng.choice(["Lte", "Gte", "Eq"], p=[0.45, 0.35, 0.2]))
        cons.append([coeffs, op, float(rng.integers(-5, 8)) if integer else float(rng.normal() * 2)])
    return {"vars": vars_, "constraints": cons}


def fixtures():
    from test_gpu_random import wide_fixture
    fxs = [fx for fx in KA["problems"]] + [read_mps(os.path.join(GOLDEN, f["file"])) for f in KA["netlib"]]
    fxs += [random_lp(np.random.default_rng(31000 + s), int(np.random.default_rng(41000 + s).integers(1, 129))) for s in range(200)]
    fxs.append(wide_fixture(np.random.default_rng(300)))  # > 2,048 nonbasic columns: the 256-thread group
    return fxs


def nt_group(v):
    return 256 if v.nN > 2048 else (64 if v.m <= 64 else 128)


class Case:
    """one LP at the seam: its phase-1 view, the oracle's end of phase 1, and phase 2's view from there (or None)"""

    def __init__(self, p1, v1, which):
        fn = eo.primal_solve_with_initial if which == "primal" else eo.dual_solve_with_initial
        self.v1 = v1
        self.o1 = v1.copy()
        self.r1 = fn(self.o1, MI)
        self.v2 = self.o2 = self.r2 = None
        if self.r1[0] != eo.OPTIMAL:
            return
        p1.store_point(self.o1)
        if which == "primal":
            if not abs(self.o1.obj()) < 1e-10:
                return
            v2 = eo.primal_phase2(p1).view()
        else:
            if not p1.dual_obj() > -1e-10:
                return
            p2, err2 = eo.dual_phase2(p1)
            if p2 is None or err2:
                return
            v2 = p2.view()
        if v2.m == 0:
            return
        self.v2 = v2
        self.o2 = v2.copy()
        self.r2 = fn(self.o2, MI)


_CASES = {}


def cases(which):
    if which not in _CASES:
        out = []
        for fx in fixtures():
            prob = eo.Problem.from_fixture(fx)
            p1, err = eo.primal_phase1(prob) if which == "primal" else eo.dual_phase1(prob)
            if p1 is None or err:
                continue
            v1 = p1.view()
            if v1.m == 0 or v1.m > 128 or v1.nN == 0:
                continue
            out.append(Case(p1, v1, which))
        _CASES[which] = out
    return _CASES[which]


def kind_of(which):
    E = _E()
    return E.ENGINE_PRIMAL if which == "primal" else E.ENGINE_DUAL


def check_against_oracle(which, phase, opts=None):
    E = _E()
    cs = [c for c in cases(which) if (c.v1 if phase == 1 else c.v2) is not None]
    views = [c.v1 if phase == 1 else c.v2 for c in cs]
    fps = [flat(v) for v in views]
    res = E.batch_solve_with_initial(kind_of(which), fps, opts or E.default_opts(max_iter=MI))
    for k, (c, fp, (st, stats, msg)) in enumerate(zip(cs, fps, res)):
        ov, (st_o, it_o, err_o) = (c.o1, c.r1) if phase == 1 else (c.o2, c.r2)
        assert_identical((which, phase, k), ov, st_o, it_o, err_o, fp, st, stats, msg, which)
    return views


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_seam_batch_bit_for_bit_with_the_oracle(which):
    v1 = check_against_oracle(which, 1)
    assert len(v1) > 150
    # the wide LP keeps > 2,048 nonbasic columns in the primal's phase 1 only (the dual's box problem drops columns)
    assert {nt_group(v) for v in v1} == ({64, 128, 256} if which == "primal" else {64, 128})
    assert len(check_against_oracle(which, 2)) > 40


def _bad_items(which):
    """a singular starting basis, a basis of the wrong size, a NaN cost: copies of AFIRO's phase-1 view"""
    E = _E()
    afiro = read_mps(os.path.join(GOLDEN, "netlib", "afiro.mps"))
    prob = eo.Problem.from_fixture(afiro)
    p1, _ = eo.primal_phase1(prob) if which == "primal" else eo.dual_phase1(prob)
    v = p1.view()
    singular, dims, nan = flat(v), flat(v), flat(v)
    singular.B[1] = singular.B[0]
    dims.nB = v.m - 1
    nan.c = nan.c.copy()
    nan.c[int(nan.N[0])] = np.nan
    nan.c[int(nan.B[0])] = np.nan
    return [singular, dims, nan]


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_failing_items_are_isolated(which):
    E = _E()
    single = E.primal_solve_with_initial if which == "primal" else E.dual_solve_with_initial
    cs = cases(which)
    fps = [flat(c.v1) for c in cs]
    bad = _bad_items(which)
    alone = []
    for b in _bad_items(which):
        st, stats, msg = single(b, E.default_opts(max_iter=MI))
        alone.append((st, stats.iters, msg))
    assert any(a[0] < 0 for a in alone)
    mixed = fps[:3] + [bad[0]] + fps[3:90] + [bad[1]] + fps[90:] + [bad[2]]
    res = E.batch_solve_with_initial(kind_of(which), mixed, E.default_opts(max_iter=MI))
    got = [res[3], res[91], res[-1]]
    for (st, stats, msg), (st_a, it_a, msg_a) in zip(got, alone):
        assert (st, stats.iters, msg) == (st_a, it_a, msg_a)
    rest = res[:3] + res[4:91] + res[92:-1]
    for k, (c, fp, (st, stats, msg)) in enumerate(zip(cs, fps, rest)):
        assert_identical((which, "mixed", k), c.o1, *c.r1, fp, st, stats, msg, which)


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_budget_slices_and_relaunches(which, monkeypatch):
    E = _E()
    fn = eo.primal_solve_with_initial if which == "primal" else eo.dual_solve_with_initial
    cs = cases(which)
    for mi in (1, 6):
        fps = [flat(c.v1) for c in cs]
        res = E.batch_solve_with_initial(kind_of(which), fps, E.default_opts(max_iter=mi))
        hit = 0
        for k, (c, fp, (st, stats, msg)) in enumerate(zip(cs, fps, res)):
            ov = c.v1.copy()
            st_o, it_o, err_o = fn(ov, mi)
            hit += st_o == eo.MAXITER
            assert_identical((which, "max_iter", mi, k), ov, st_o, it_o, err_o, fp, st, stats, msg, which)
        assert hit > 20
    monkeypatch.setenv("ELLP_BATCH_LAUNCH_ITERS", "7")
    check_against_oracle(which, 1)
    check_against_oracle(which, 2)


@pytest.mark.parametrize("flags", ["maxviol", "bflip", "both"])
def test_dual_extensions_match_the_single_call(flags):
    E = _E()
    f = {"maxviol": E.FLAG_DUAL_MAX_VIOLATION, "bflip": E.FLAG_DUAL_BOUND_FLIPPING,
         "both": E.FLAG_DUAL_MAX_VIOLATION | E.FLAG_DUAL_BOUND_FLIPPING}[flags]
    cs = cases("dual")[:80]
    views = [c.v1 for c in cs] + [c.v2 for c in cs if c.v2 is not None]
    fps = [flat(v) for v in views]
    res = E.batch_solve_with_initial(E.ENGINE_DUAL, fps, E.default_opts(max_iter=MI, flags=f))
    for k, (v, fp, (st, stats, msg)) in enumerate(zip(views, fps, res)):
        one = flat(v)
        st1, stats1, msg1 = E.dual_solve_with_initial(one, E.default_opts(max_iter=MI, flags=f, pipeline=3))
        assert (st, stats.iters, stats.pivots, msg) == (st1, stats1.iters, stats1.pivots, msg1), (flags, k)
        if st1 < 0:
            continue
        for a in ("x", "B", "N", "Nb", "y", "d"):
            assert getattr(fp, a).tobytes() == getattr(one, a).tobytes(), (flags, k, a)
        assert np.float64(stats.obj).tobytes() == np.float64(stats1.obj).tobytes()
    # the rule took effect: some phase-1 runs take another path than the plain dual loop (the oracle's counts)
    assert sum(r[1].iters != c.r1[1] for c, r in zip(cs, res)) > 0


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


def _single(solver, p):
    try:
        return solver.solve(p)
    except Exception as e:  # noqa: BLE001 — compared with what solve_batch hands back
        return e


@pytest.mark.parametrize("which", ["primal", "dual"])
def test_user_api_equals_solve(which):
    import ellp_amd
    from ellp_amd import Problem
    fxs = [fx for fx in KA["problems"]] + [read_mps(os.path.join(GOLDEN, f["file"])) for f in KA["netlib"]]
    fxs.append({"vars": [[1.0, ["Lower", 0.5, 0.0]], [-1.0, ["TwoSided", 0.0, 2.0]]], "constraints": []})  # m == 0
    adl = read_mps(os.path.join(GOLDEN, "netlib", "adlittle.mps"))
    fxs.append(blockdiag(adl, 3))  # 168 rows: the single path
    fxs += [random_lp(np.random.default_rng(51000 + s), int(np.random.default_rng(52000 + s).integers(1, 40))) for s in range(12)]
    ps = [Problem.from_fixture(fx) for fx in fxs]
    ps.append(ps[len(KA["problems"]) + 1])  # ADLITTLE a second time
    cls = ellp_amd.PrimalSimplexSolver if which == "primal" else ellp_amd.DualSimplexSolver
    kinds = set()
    for solver in (cls(), cls(max_iter=4)):
        got = solver.solve_batch(ps)
        assert len(got) == len(ps)
        for k, (p, g) in enumerate(zip(ps, got)):
            ref = _single(solver, p)
            _same((which, solver.max_iter, k), g, ref)
            kinds.add(type(ref).__name__ if isinstance(ref, Exception) else ref.kind)
    assert {"optimal", "infeasible", "maxiter"} <= kinds

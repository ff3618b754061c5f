"""Both phases of a batch of primal solves in one call (ellp_batch_primal_solve; PrimalSimplexSolver.solve_batch runs on it):
every item must end exactly as the two-call path ends it — ellp_batch_solve_with_initial on phase 1, the host's checks, the
oracle's phase-2 construction, ellp_batch_solve_with_initial on phase 2 — in status, stage, both iteration counts, index
sets, labels and the bits of x and of the phase-1 objective; whatever max_iter, launch cap or chunk size cuts the solve;
without waiting for its neighbours' phase 1 (launch rounds); and through the user API against solve()."""
import math
import os

import numpy as np
import pytest

from helpers import GOLDEN, blockdiag, known_answers, permuted_fixture, read_mps
from oracle import ellp_oracle as eo
from test_gpu_batch import random_lp
from test_gpu_random import feasible_fixture, random_fixture
from test_gpu_small import flat

pytestmark = pytest.mark.gpu
KA = known_answers()
MI = 5000
EPS = 1e-10


def _E():
    from ellp_amd import _engine as E
    return E


def fixtures():
    """the known answers, ~60 random LPs of 1 to 40 rows (all bound and constraint kinds; feasible and bounded ones)"""
    fxs = [("ka", fx["name"], fx) for fx in KA["problems"]]
    fxs += [("random", s, random_fixture(np.random.default_rng(7100 + s))) for s in range(25)]
    fxs += [("feasible", s, feasible_fixture(np.random.default_rng(7200 + s))) for s in range(25)]
    fxs += [("random_lp", s, random_lp(np.random.default_rng(7300 + s), 14 + 2 * s)) for s in range(12)]
    return fxs


class Item:
    """one LP that reaches the seam: its fixture, phase 1's view and the inputs of phase 2 (known before phase 1 runs)"""

    def __init__(self, tag, fx, max_m=128):
        self.tag, self.fx = tag, fx
        p1 = self.phase1()
        self.ok = p1 is not None
        if not self.ok:
            return
        self.v1 = p1.view()
        self.ok = 0 < self.v1.m <= max_m  # without nonbasic columns too (the linear systems): Optimal as they stand
        if not self.ok:
            return
        v2 = eo.primal_phase2(p1).view()  # PrimalPhase2::from_phase1 sets costs and bounds whatever the point is
        self.in2 = (v2.c, v2.kind, v2.lb, v2.ub)

    def phase1(self):
        p1, err = eo.primal_phase1(eo.Problem.from_fixture(self.fx))
        return None if (p1 is None or err) else p1

    def arg(self):
        fp = flat(self.v1)
        return fp, (fp,) + self.in2


def host_obj(c, x):
    """StandardForm::obj: the products added in index order"""
    s = 0.0
    for ci, xi in zip(c.tolist(), x.tolist()):
        s += ci * xi
    return s


def two_calls(items, opts):
    """the path solve_batch took before: phase 1 of every item in one batch, the checks of solve() on the host, phase 2 of
    the items that pass them in a second batch.  Returns (status, stage, iters1, iters2, obj1, obj, msg, fp) per item."""
    E = _E()
    fps1 = [flat(it.v1) for it in items]
    res1 = E.batch_solve_with_initial(E.ENGINE_PRIMAL, fps1, opts)
    out = [None] * len(items)
    second = []
    for k, (it, fp, (st, stats, msg)) in enumerate(zip(items, fps1, res1)):
        if st != E.OPTIMAL:
            out[k] = (st, 1, stats.iters, 0, math.nan, stats.obj, msg, fp)
            continue
        obj1 = host_obj(fp.c, fp.x)
        if not obj1 > -opts.eps:
            out[k] = (E.ERR_PANIC, 1, stats.iters, 0, obj1, stats.obj, "assertion failed: obj > -EPS", fp)
            continue
        if not obj1 < opts.eps:
            out[k] = (E.INFEASIBLE, 1, stats.iters, 0, obj1, stats.obj, msg, fp)
            continue
        p1 = it.phase1()
        ov = it.v1.copy()
        ov.x[:], ov.B[:], ov.N[:fp.nN], ov.Nb[:fp.nN] = fp.x, fp.B, fp.N, fp.Nb
        p1.store_point(ov)
        v2 = eo.primal_phase2(p1).view()
        for a, b in zip((v2.c, v2.kind, v2.lb, v2.ub), it.in2):
            assert a.tobytes() == b.tobytes(), it.tag  # phase 2's inputs do not depend on phase 1's end
        second.append((k, flat(v2), stats.iters, obj1))
    res2 = E.batch_solve_with_initial(E.ENGINE_PRIMAL, [s[1] for s in second], opts)
    for (k, fp2, it1, obj1), (st, stats, msg) in zip(second, res2):
        out[k] = (st, 2, it1, stats.iters, obj1, stats.obj, msg, fp2)
    return out


def one_call(items, opts):
    E = _E()
    args = [it.arg() for it in items]
    res = E.batch_primal_solve([a[1] for a in args], opts)
    return [r + (a[0],) for r, a in zip(res, args)]


def bits(v):
    return np.float64(v).tobytes()


def assert_same(tag, got, ref):
    assert got[:4] == ref[:4], (tag, got[:7], ref[:7])  # status, stage, both iteration counts
    assert got[6] == ref[6], (tag, got[6], ref[6])
    assert (math.isnan(got[4]) and math.isnan(ref[4])) or bits(got[4]) == bits(ref[4]), (tag, got[4], ref[4])
    if ref[0] < 0:
        return
    assert bits(got[5]) == bits(ref[5]), (tag, got[5], ref[5])
    g, r = got[7], ref[7]
    for a in ("B", "N", "Nb", "x"):
        assert getattr(g, a).tobytes() == getattr(r, a).tobytes(), (tag, a)


_POP = {}


def population():
    """the items, and what the two-call path makes of them under MI"""
    if not _POP:
        E = _E()
        items = [it for it in (Item((kind, s), fx) for kind, s, fx in fixtures()) if it.ok]
        _POP["items"] = items
        _POP["ref"] = two_calls(items, E.default_opts(max_iter=MI))
    return _POP["items"], _POP["ref"]


def mixed12():
    """12 items of every ending, the longest solves among them"""
    items, ref = population()
    order = sorted(range(len(items)), key=lambda k: -(ref[k][2] + ref[k][3]))
    pick = order[:6]
    for want in ((E_INFEASIBLE, 1), (E_UNBOUNDED, 2), (E_OPTIMAL, 2)):
        pick += [k for k in order if (ref[k][0], ref[k][1]) == want and k not in pick][:2]
    return [items[k] for k in pick[:12]], [ref[k] for k in pick[:12]]


E_OPTIMAL, E_INFEASIBLE, E_UNBOUNDED, E_MAXITER = 0, 1, 2, 3


def test_seam_bit_for_bit_with_the_two_call_path():
    E = _E()
    items, ref = population()
    assert len(items) >= 60
    got = one_call(items, E.default_opts(max_iter=MI))
    for it, g, r in zip(items, got, ref):
        assert_same(it.tag, g, r)
    endings = {(r[0], r[1]) for r in ref}
    assert {(E_INFEASIBLE, 1), (E_OPTIMAL, 2), (E_UNBOUNDED, 2)} <= endings, endings
    # infeasible BY OBJECTIVE: phase 1 itself ended Optimal
    assert any(r[0] == E_INFEASIBLE and r[1] == 1 and not math.isnan(r[4]) for r in ref)
    info = E.batch_primal_info()
    assert info["rounds"] == 1 and info["chunks"] == 1  # MI loop bodies per phase fit the cap of one launch


def test_max_iter_boundaries():
    """each phase has its own budget of max_iter loop bodies: MaxIter at stage 1 and at stage 2"""
    E = _E()
    items, ref = population()
    k = next(k for k, r in enumerate(ref) if r[1] == 2 and r[0] == E_OPTIMAL and r[2] >= 3 and r[3] >= r[2] + 2)
    i1, i2 = ref[k][2], ref[k][3]
    seen = set()
    for mi in sorted({i1 - 1, i1, i1 + 1, i2 - 1, i2, max(i1, i2) + 1}):
        opts = E.default_opts(max_iter=mi)
        (g,), (r,) = one_call([items[k]], opts), two_calls([items[k]], opts)
        assert_same((items[k].tag, mi), g, r)
        seen.add((r[0], r[1]))
    assert {(E_MAXITER, 1), (E_MAXITER, 2), (E_OPTIMAL, 2)} <= seen, (i1, i2, seen)


@pytest.mark.parametrize("cap", [1, 7])
def test_a_launch_cut_anywhere_changes_nothing(cap, monkeypatch):
    E = _E()
    items, ref = mixed12()
    assert len(items) == 12 and max(r[2] + r[3] for r in ref) > 7
    monkeypatch.setenv("ELLP_BATCH_LAUNCH_ITERS", str(cap))
    got = one_call(items, E.default_opts(max_iter=MI))
    for it, g, r in zip(items, got, ref):
        assert_same((it.tag, cap), g, r)
    rounds = E.batch_primal_info()["rounds"]
    assert rounds == math.ceil(max(r[2] + r[3] for r in ref) / cap), rounds


def test_chunks_change_nothing(monkeypatch):
    E = _E()
    items, ref = mixed12()
    one_call(items, E.default_opts(max_iter=MI))
    whole = E.batch_primal_info()
    assert whole["chunks"] == 1
    monkeypatch.setenv("ELLP_BATCH_MAX_BYTES", str(whole["upload_bytes"] // 3))
    got = one_call(items, E.default_opts(max_iter=MI))
    assert E.batch_primal_info()["chunks"] >= 3
    for it, g, r in zip(items, got, ref):
        assert_same(it.tag, g, r)


def test_a_refused_call_leaves_the_diagnostics():
    """ellp_batch_primal_info speaks of the last call that passed the checks of the call"""
    E = _E()
    items, _ = mixed12()
    one_call(items[:2], E.default_opts(max_iter=MI))
    before = E.batch_primal_info()
    assert before["rounds"] >= 1 and before["chunks"] == 1 and before["upload_bytes"] > 0
    with pytest.raises(E.EllpHipError):
        one_call(items[:2], E.default_opts(max_iter=MI, pipeline=1))
    assert E.batch_primal_info() == before


def test_no_lock_step(monkeypatch):
    """P's phase 1 is long, Q's is short and its phase 2 long: the rounds follow the longest SOLVE, not the longest phase 1
    plus the longest phase 2"""
    E = _E()
    items, ref = population()
    two = [k for k, r in enumerate(ref) if r[1] == 2]
    p = max(two, key=lambda k: ref[k][2] - ref[k][3])
    q = max(two, key=lambda k: ref[k][3] - ref[k][2])
    i1, i2 = [ref[p][2], ref[q][2]], [ref[p][3], ref[q][3]]
    cap = next(c for c in (3, 2, 1)
               if math.ceil(max(i1) / c) + math.ceil(max(i2) / c) - (math.ceil(max(a + b for a, b in zip(i1, i2)) / c) + 1) >= 2)
    monkeypatch.setenv("ELLP_BATCH_LAUNCH_ITERS", str(cap))
    got = one_call([items[p], items[q]], E.default_opts(max_iter=MI))
    assert_same(items[p].tag, got[0], ref[p])
    assert_same(items[q].tag, got[1], ref[q])
    rounds = E.batch_primal_info()["rounds"]
    print(f"no lock step: (i1, i2) = {list(zip(i1, i2))}, cap {cap}, rounds {rounds}")
    assert rounds <= math.ceil(max(a + b for a, b in zip(i1, i2)) / cap) + 1
    assert rounds < math.ceil(max(i1) / cap) + math.ceil(max(i2) / cap)


def test_failing_items_are_isolated():
    """a singular starting basis and an index out of range get their error; the other items' bits do not change"""
    E = _E()
    items, ref = mixed12()
    args = [it.arg() for it in items]
    sing_fp, sing = items[0].arg()
    sing_fp.B[1] = sing_fp.B[0]  # the same column twice in the basis
    st_s, stats_s, msg_s = E.primal_solve_with_initial(flat_copy(sing_fp), E.default_opts(max_iter=MI, pipeline=3))
    range_fp, rng_item = items[1].arg()
    range_fp.N[0] = range_fp.n_c + 5
    st_r, _, msg_r = E.primal_solve_with_initial(flat_copy(range_fp), E.default_opts(max_iter=MI, pipeline=3))
    assert st_s < 0 and st_r == E.ERR_ARG, (st_s, st_r)
    mixed = [a[1] for a in args[:4]] + [sing] + [a[1] for a in args[4:9]] + [rng_item] + [a[1] for a in args[9:]]
    res = E.batch_primal_solve(mixed, E.default_opts(max_iter=MI))
    assert (res[4][0], res[4][1], res[4][6]) == (st_s, 1, msg_s) and res[4][2] == stats_s.iters
    assert (res[10][0], res[10][1], res[10][6]) == (st_r, 1, msg_r)
    rest = res[:4] + res[5:10] + res[11:]
    for it, a, g, r in zip(items, args, rest, ref):
        assert_same(it.tag, g + (a[0],), r)


def flat_copy(fp):
    E = _E()
    out = E.FlatProblem(fp.m, fp.n, fp.n_c, fp.A, fp.c, fp.b, fp.kind, fp.lb, fp.ub, fp.x, fp.B, fp.N, fp.Nb)
    return out


def _same(tag, got, ref):
    import ellp_amd
    if isinstance(ref, Exception):
        assert type(got) is type(ref) and str(got) == str(ref), (tag, got, ref)
        return
    assert not isinstance(got, Exception), (tag, got)
    assert (got.kind, got.iters) == (ref.kind, ref.iters), (tag, got.kind, ref.kind, got.iters, ref.iters)
    if ref.kind == ellp_amd.SolverResult.Optimal:
        assert bits(got.solution.obj()) == bits(ref.solution.obj()), tag
        assert got.solution.x().tobytes() == ref.solution.x().tobytes(), tag
    elif ref.kind == ellp_amd.SolverResult.MaxIter:
        assert bits(got.obj) == bits(ref.obj), tag


def _single(solver, p):
    try:
        return solver.solve(p)
    except Exception as e:  # noqa: BLE001 — compared with what solve_batch hands back
        return e


def test_mid_and_small_items_in_one_call():
    """ADLITTLE x 3 in three variable orders (168 rows: k_mid_batch_primal) next to two items of k_small_batch_primal"""
    import ellp_amd
    adl = read_mps(os.path.join(GOLDEN, "netlib", "adlittle.mps"))
    fxs = [permuted_fixture(blockdiag(adl, 3), np.random.default_rng(s)) for s in (61, 62, 63)]
    fxs += [read_mps(os.path.join(GOLDEN, "netlib", "afiro.mps")), feasible_fixture(np.random.default_rng(7201))]
    ps = [ellp_amd.Problem.from_fixture(fx) for fx in fxs]
    # at the seam first: the call itself must take the 168-row items (solve_batch would quietly solve refused ones singly)
    E = _E()
    seam = [Item(("mid", k), fx, max_m=1024) for k, fx in enumerate(fxs)]
    assert all(it.ok for it in seam) and [it.v1.m > 128 for it in seam] == [True, True, True, False, False]
    res = one_call(seam, E.default_opts(max_iter=MI, pipeline=3))
    for it, r in zip(seam, res):
        assert (r[0], r[1]) == (E_OPTIMAL, 2) and r[3] > 0, (it.tag, r[:7])
    assert E.batch_primal_info()["chunks"] == 1
    solver = ellp_amd.PrimalSimplexSolver.new(None, pipeline=3)
    got = solver.solve_batch(ps)
    assert E.batch_primal_info()["chunks"] == 1  # one call, both kernels
    for k, (p, g) in enumerate(zip(ps, got)):
        ref = _single(solver, p)
        _same(("mid", k), g, ref)
        assert ref.kind == ellp_amd.SolverResult.Optimal and ref.iters[1] > 0, (k, ref.kind, ref.iters)


NO_ROWS = {"vars": [[1.0, ["Lower", 0.5, 0.0]], [-1.0, ["TwoSided", 0.0, 2.0]]], "constraints": []}


def test_user_api_equals_solve_and_uploads_once():
    import ellp_amd
    E = _E()
    fxs = [fx for _, _, fx in fixtures()[len(KA["problems"]):]][:35]
    fxs += [read_mps(os.path.join(GOLDEN, f["file"])) for f in KA["netlib"]][:4]
    fxs += [NO_ROWS, next(fx for fx in KA["problems"] if fx["name"] == "linear_system_2d")]  # the latter: no nonbasic column
    assert len(fxs) == 40
    shapes = set()
    free = 0
    a_bytes = 0
    for fx in fxs:  # what a seam call stages of the matrix per item: A_B and A_N, columns padded to 16 rows
        p1, err = eo.primal_phase1(eo.Problem.from_fixture(fx))
        if p1 is None or err:
            continue
        v = p1.view()
        free += v.n_c > v.n
        shapes.add("no rows" if v.m == 0 else ("no nonbasic column" if v.nN == 0 else "seam"))
        if 0 < v.m <= 128 and v.nN > 0:
            a_bytes += 8 * ((v.m + 15) // 16 * 16) * (v.m + v.nN)
    assert free >= 1 and shapes == {"no rows", "no nonbasic column", "seam"}
    ps = [ellp_amd.Problem.from_fixture(fx) for fx in fxs]
    solver = ellp_amd.PrimalSimplexSolver(max_iter=MI)
    got = solver.solve_batch(ps)
    info = E.batch_primal_info()
    kinds = set()
    for k, (p, g) in enumerate(zip(ps, got)):
        ref = _single(solver, p)
        _same(("api", k), g, ref)
        kinds.add(type(ref).__name__ if isinstance(ref, Exception) else ref.kind)
    assert {"optimal", "infeasible", "unbounded"} <= kinds, kinds
    # the matrices went up once: all the rest of the staging buffer (states, points, costs and bounds of both phases,
    # argument lists) is less than a second copy of them, which is what a second seam call would stage at the least
    print(f"upload {info['upload_bytes']} bytes, matrices {a_bytes} bytes")
    assert info["chunks"] == 1 and a_bytes < info["upload_bytes"] < 2 * a_bytes, (info, a_bytes)

"""Batched dual phase-1 starts (ellp_batch_dual_phase1_start): every item's x, N_bound, y, d, starting objective and status
must be, bit for bit, what ellp_engine_create_dual_phase1 followed by ellp_engine_read_point gives for that item alone
with the same options — on netlib replications, dense synthetic LPs, a permutation-shortcut basis, failing items mixed
in, small chunks and a narrower sub-panel of the blocked rebuild."""
import os

import numpy as np
import pytest

from helpers import GOLDEN, blockdiag, known_answers, permuted_fixture, read_mps
from oracle import ellp_oracle as eo

pytestmark = pytest.mark.gpu


def _E():
    from ellp_amd import _engine as E
    return E


def _netlib(name, copies, seed):
    ka = next(p for p in known_answers()["netlib"] if p["name"] == name)
    return permuted_fixture(blockdiag(read_mps(os.path.join(GOLDEN, ka["file"])), copies), np.random.default_rng(seed))


_VIEWS = {}


def _phase1_args(key):
    """(m, n, A, c, b, kind, lb, ub, B, N) of DualPhase1's box problem and basis, as the oracle builds them"""
    if key not in _VIEWS:
        if key[0] == "netlib":
            prob = eo.Problem.from_fixture(_netlib(*key[1:]))
        else:
            prob = eo.synth_problem(*key[1:])
        d1, err = eo.dual_phase1(prob)
        assert d1 is not None and not err, err
        v = d1.view()
        assert v.n_c == v.n and v.nN > 0
        _VIEWS[key] = (v.m, v.n, v.A.copy(), v.c.copy(), v.b.copy(), v.kind.copy(), v.lb.copy(), v.ub.copy(), v.B.copy(),
                       v.N[:v.nN].copy())
    return _VIEWS[key]


NETLIB = [("netlib", "blend", 2, 11), ("netlib", "adlittle", 3, 13), ("netlib", "adlittle", 6, 15)]
DENSE = [("synth", 20260411, 300, 700), ("synth", 20260412, 650, 1300)]


def _box(m, nN, seed, perm_basis=True, singular=False, bad_kind=False):
    """a box problem of m rows: nN dense random columns, then m basis columns — a scaled, permuted identity (the rebuild's
    permutation shortcut) or dense random ones; `singular` zeroes a basis column, `bad_kind` gives one nonbasic variable
    a bound that is not two-sided or fixed (the reference's panic)"""
    rng = np.random.default_rng(seed)
    n = m + nN
    A = np.zeros((m, n))
    A[:, :nN] = rng.standard_normal((m, nN))
    if perm_basis:
        A[rng.permutation(m), nN + np.arange(m)] = rng.uniform(0.5, 2.0, m) * rng.choice([-1.0, 1.0], m)
    else:
        A[:, nN:] = rng.standard_normal((m, m)) + 4.0 * np.eye(m)
    if singular:
        A[:, nN + 1] = 0.0
    kind = np.full(n, 3, np.uint8)
    kind[rng.integers(0, nN, nN // 5)] = 4  # some fixed
    if bad_kind:
        kind[0] = 1
    lb = -rng.uniform(0.5, 2.0, n)
    ub = rng.uniform(0.5, 2.0, n)
    ub[kind == 4] = lb[kind == 4]
    B = nN + rng.permutation(m)
    return (m, n, A.ravel(order="F").copy(), rng.standard_normal(n), rng.standard_normal(m), kind, lb, ub, B,
            np.arange(nN))


def _host_dual_obj(m, n, b, kind, lb, ub, y, d):
    """the engine's starting objective (host_dual_obj): the same sums in the same order"""
    obj = 0.0
    for i in range(m):
        obj += float(b[i]) * float(y[i])
    for i in range(n):
        k = int(kind[i])
        if k == 1 or k == 4:
            obj += float(lb[i]) * float(d[i])
        elif k == 2:
            obj += float(ub[i]) * float(d[i])
        elif k == 3:
            obj += float(lb[i]) * float(d[i]) if d[i] > 0.0 else float(ub[i]) * float(d[i])
    return obj


def _single(args, opts):
    E = _E()
    m, n, A, c, b, kind, lb, ub, B, N = args
    try:
        eng = E.Engine.dual_phase1(m, n, A, c, b, kind, lb, ub, B, N, opts)
    except E.EllpHipError as e:
        return e.status, None, e.msg
    try:
        fp = eng.read_point()
        assert eng.closing_status == E.OPTIMAL
        return E.OPTIMAL, (fp.x.copy(), fp.Nb.copy(), fp.y.copy(), fp.d.copy()), _host_dual_obj(m, n, b, kind, lb, ub, fp.y, fp.d)
    finally:
        eng.close()


def _check(problems, opts):
    E = _E()
    res = E.batch_dual_phase1_start(problems, opts)
    statuses = []
    for args, (s, obj, msg, fp) in zip(problems, res):
        s1, pt, o1 = _single(args, opts)
        assert s == s1, (args[0], s, s1, msg, o1)
        statuses.append(s)
        if s != E.OPTIMAL:
            assert msg == o1, (msg, o1)  # the same message
            continue
        x, Nb, y, d = pt
        assert fp.x.tobytes() == x.tobytes()
        assert fp.Nb.tobytes() == Nb.tobytes()
        assert fp.y.tobytes() == y.tobytes()
        assert fp.d.tobytes() == d.tobytes()
        assert np.float64(obj).tobytes() == np.float64(o1).tobytes(), (obj, o1)
    return statuses


@pytest.mark.parametrize("flags,pipeline", [(16, 0), (16 | 2, 0), (0, 3)])
def test_netlib_and_dense_starts_bit_for_bit(flags, pipeline):
    E = _E()
    probs = [_phase1_args(k) for k in NETLIB + DENSE]
    assert all(128 < p[0] <= 1024 for p in probs)
    st = _check(probs, E.default_opts(flags=flags, pipeline=pipeline))
    assert st == [E.OPTIMAL] * len(probs)


def test_shortcut_general_small_and_failing_items_in_one_call():
    E = _E()
    probs = [_box(300, 200, 1), _box(300, 200, 2, perm_basis=False), _box(200, 100, 3, perm_basis=False, singular=True),
             _box(160, 90, 4, bad_kind=True), _box(60, 40, 5, perm_basis=False), _phase1_args(NETLIB[1]),
             _box(100, 50, 6, singular=True, perm_basis=True)]
    st = _check(probs, E.default_opts(pipeline=3))
    assert st[0] == st[1] == st[4] == st[5] == E.OPTIMAL
    assert st[2] == st[6] == E.ERR_SINGULAR and st[3] == E.ERR_PANIC, st


def test_chunks_and_narrow_subpanel(monkeypatch):
    E = _E()
    probs = [_phase1_args(k) for k in NETLIB] + [_box(300, 200, 7, perm_basis=False), _box(130, 60, 8)]
    opts = E.default_opts(flags=16)
    base = E.batch_dual_phase1_start(probs, opts)
    monkeypatch.setenv("ELLP_BATCH_MAX_BYTES", str(4 << 20))
    chunked = E.batch_dual_phase1_start(probs, opts)
    for (s0, o0, _, f0), (s1, o1, _, f1) in zip(base, chunked):
        assert s0 == s1 == E.OPTIMAL
        assert np.float64(o0).tobytes() == np.float64(o1).tobytes()
        for a in ("x", "Nb", "y", "d"):
            assert getattr(f0, a).tobytes() == getattr(f1, a).tobytes(), a
    monkeypatch.delenv("ELLP_BATCH_MAX_BYTES")
    monkeypatch.setenv("ELLP_BL_NBW", "8")
    st = _check(probs, opts)
    assert st == [E.OPTIMAL] * len(probs)


# ---- the user API: DualSimplexSolver.solve_batch takes the 129 - 1,024-row problems whose options run k_mid, their
# phase-1 starts made by the batched call; every entry must be solve(p)'s to the bit
_INFEASIBLE = {"vars": [[1.0, ["Lower", 0.0, 0.0]]], "constraints": [[[[0, 1.0]], "Gte", 2.0], [[[0, 1.0]], "Lte", 1.0]]}
# min -x0 with x0 <= 1 + x1, x1 free to grow: unbounded, so the dual is infeasible and the primal classifies it
_UNBOUNDED = {"vars": [[-1.0, ["Lower", 0.0, 0.0]], [0.0, ["Lower", 0.0, 0.0]]],
              "constraints": [[[[0, 1.0], [1, -1.0]], "Lte", 1.0], [[[0, 1.0], [1, 1.0]], "Gte", 0.0]]}


def _single_solve(solver, p):
    try:
        return solver.solve(p)
    except Exception as e:  # noqa: BLE001 — compared with what solve_batch hands back
        return e


def test_user_api_equals_solve():
    import ellp_amd
    from ellp_amd import Problem
    from test_gpu_batch_mid import _same
    KA = known_answers()
    fxs = [_netlib("blend", 2, 31), _netlib("adlittle", 3, 32), _netlib("adlittle", 6, 33),
           read_mps(os.path.join(GOLDEN, "netlib", "afiro.mps"))] + list(KA["problems"][:3])
    fxs += [blockdiag(_INFEASIBLE, 70), blockdiag(_UNBOUNDED, 70)]  # 140 rows each
    ps = [Problem.from_fixture(fx) for fx in fxs]
    tall = Problem.from_fixture(blockdiag(_INFEASIBLE, 520))  # 1,040 rows: above the batch, through solve()
    BF, MV = 16, 2
    kinds = set()
    for mi, opts, extra in [(None, dict(flags=BF), [tall]), (None, dict(flags=BF | MV), [tall]), (None, dict(pipeline=3), []),
                            (40, dict(flags=BF), []), (40, dict(pipeline=3), [])]:
        solver = ellp_amd.DualSimplexSolver.new(mi, **opts)
        probs = ps + extra
        got = solver.solve_batch(probs)
        assert len(got) == len(probs)
        for k, (p, g) in enumerate(zip(probs, got)):
            ref = _single_solve(solver, p)
            _same((mi, tuple(opts.items()), k), g, ref)
            kinds.add(type(ref).__name__ if isinstance(ref, Exception) else ref.kind)
    assert {"optimal", "infeasible", "unbounded", "maxiter"} <= kinds, kinds

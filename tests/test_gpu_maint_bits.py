"""The periodic maintenance passes of an explicit-inverse engine, bit for bit against tests/maint_bits_model.py: the full
BTRAN (k_btran_part / _reduce), the drift monitor (k_drift_part / _reduce) and the x_B resync (k_resync_part / _rhs / _xb /
_apply).  tests/test_gpu_maint.py holds the same kernels inside the rounding bound of ANY evaluation order; this file holds
them to the one order they have, so that their loads, their spread over workgroups and their launches can be rearranged and
the values shown to be the same.  The engines are driven as tests/test_gpu_maint.py drives them (its helpers are imported).

Sizes (engine_plan must agree with maint_model.geometry): 129 = ld - 15, 8 rows a tile, 17 tiles, the last of one row;
144 = ld; 513: 9 rows a tile, 57 tiles, a second, ragged block of columns; 1025: more rows than 1,024 threads, 17 rows a tile.
Patterns of c_B and x_N: all zero (everything skipped), one nonzero per tile, dense.  The drift monitor has no skip: plain, a
NaN and an Inf planted in B^-1.  The Newton-Schulz refresh is not compared here: its two GEMMs and its copy into the other
buffer are what they were (tests/test_gpu_refresh.py)."""
import numpy as np
import pytest

import maint_bits_model as bm
import maint_model as mm
from test_gpu_maint import _E, _binv, _bits, _check_plan, _drift_run, _flatA, _opts

pytestmark = pytest.mark.gpu

SIZES = (129, 144, 513, 1025)
PATTERNS = ("zero", "one-per-tile", "dense")


def _same_bits(label, dev, model):
    dev, model = np.asarray(dev, dtype=np.float64).reshape(-1), np.asarray(model, dtype=np.float64).reshape(-1)
    bad = np.flatnonzero(_bits(dev) != _bits(model))
    print(f"{label}: {bad.size} of {dev.size} entries differ in bits" + (f" (first at {bad[0]}: device {dev[bad[0]]!r}, model {model[bad[0]]!r})" if bad.size else ""))
    assert bad.size == 0, label


def _pattern(pattern, count, per_tile, rng):
    v = rng.uniform(0.25, 1.25, size=count) * rng.choice([-1.0, 1.0], size=count)
    if pattern == "zero":
        v[:] = 0.0
    elif pattern == "one-per-tile":
        v[np.arange(count) % per_tile != per_tile - 1] = 0.0  # the last row of every full tile: a ragged last tile stays empty
    return v


# ------------------------------------------------------------------------------------------------ BTRAN
@pytest.mark.parametrize("m", SIZES)
def test_btran_bits(m):
    E = _E()
    base = mm.btran_case(m, "dense")
    _, rows, tiles = mm.geometry(m)
    opts = _opts(btran_mode=1)
    _check_plan(E.ENGINE_PRIMAL, m, base.n - m, opts)
    for pattern in PATTERNS:
        c_B = _pattern(pattern, m, rows, np.random.default_rng(8100 + m))
        if pattern == "one-per-tile":
            assert np.count_nonzero(c_B) == m // rows
        c = np.concatenate([c_B, base.c[m:]])
        fp = E.FlatProblem(base.m, base.n, base.n, _flatA(base.A), c, base.b, base.kind, base.lb, base.ub, base.x, base.B, base.N, base.Nb)
        eng = E.Engine(E.ENGINE_PRIMAL, fp, opts)
        try:
            eng.debug_set_inverse(base.W_random)
            W = _binv(eng, m)
            assert np.array_equal(_bits(W), _bits(base.W_random))
            eng.step(0)
            assert int(eng.tap(E.TAP_STATE, 12)[0]) == 100
            u = eng.tap(E.TAP_U, m)
        finally:
            eng.close()
        _same_bits(f"btran m={m} c_B={pattern}", u, bm.btran(W, c_B))


# ------------------------------------------------------------------------------------------------ the drift monitor
@pytest.mark.parametrize("damage", [None, np.nan, np.inf], ids=["plain", "nan", "inf"])
@pytest.mark.parametrize("m", SIZES)
def test_drift_bits(m, damage, monkeypatch):
    """DevState::drift of one check.  The planted NaN / Inf sits in a row of B^-1 that is not the pivot row, in a column where
    a_q is nonzero (all are), so d carries it and with it every row of A_B d."""
    E = _E()
    monkeypatch.setenv("ELLP_DRIFT_EVERY", "1")
    dual = True  # a primal engine's ratio test meets the NaN as well (tests/test_gpu_maint.py); the monitor is the same kernel
    hit = None
    if damage is not None:
        eng, _, _, _, r = _drift_run(m, dual)
        eng.close()
        hit = ((r + 1) % m, m // 2, damage)
    eng, cnt, checks, _, _ = _drift_run(m, dual, damage=hit)
    try:
        d = eng.tap(E.TAP_D, m)
        q = int(eng.tap(E.TAP_STATE, 12)[2])
    finally:
        eng.close()
    c = mm.pivot_case(m, dual)
    B, N = c.B, c.N  # the basis the monitor saw: the engine's first (step(1) has gone on to the update)
    assert checks == 1
    if damage is not None:
        assert not np.isfinite(d).all()
    want = bm.drift(c.A[:, B], d, c.A[:, N[q]], 1.0)
    print(f"drift m={m} {damage}: device {cnt['drift']!r}, model {want!r}")
    assert np.isnan(want) if damage is np.nan else (np.isposinf(want) if damage is np.inf else 0.5e-6 < want < 2e-6)
    _same_bits(f"drift m={m} {damage}", [cnt["drift"]], [want])


# ------------------------------------------------------------------------------------------------ the resync of x_B
def _resync_case(m, nN):
    """maint_model.pivot_case's primal LP (every nonbasic column a positive combination of the basic ones, cost -1 on them)
    with nN nonbasic columns instead of 24, so that a tile of the resync's front has ten columns"""
    from types import SimpleNamespace
    rng = np.random.default_rng(8300 + m)
    Bm = mm.conditioned_basis(m, 7200 + m)
    A = np.concatenate([Bm, Bm @ rng.uniform(0.1, 1.0, size=(m, nN))], axis=1)
    n = m + nN
    return SimpleNamespace(m=m, n=n, A=A, c=np.concatenate([np.zeros(m), -np.ones(nN)]), x=np.concatenate([rng.uniform(0.5, 1.5, size=m), np.zeros(nN)]),
                           B=np.arange(m, dtype=np.int64), N=np.arange(m, n, dtype=np.int64))


@pytest.mark.parametrize("m", SIZES)
def test_resync_bits(m):
    """one pivot, the carried x_B pushed past the adoption threshold (dense, one-per-tile) or left alone (zero: nothing is
    adopted), then the maintenance of the next step: t, cand and x as the resync left them"""
    E = _E()
    tiles = mm.geometry(m)[2]
    base = _resync_case(m, 9 * tiles + 5)
    nN = base.n - m
    cols = (nN + tiles - 1) // tiles
    assert cols == 10 and nN % cols != 0 and (nN + cols - 1) // cols < tiles  # a batch of 8 and a rest; a ragged tile; empty tiles
    opts = _opts(refactor_period=1)
    _check_plan(E.ENGINE_PRIMAL, m, nN, opts)
    for pattern in PATTERNS:
        x_N = np.abs(_pattern(pattern, nN, cols, np.random.default_rng(8200 + m)))
        lb = np.concatenate([np.zeros(m), x_N])
        x = np.concatenate([base.x[:m], x_N])
        b = base.A @ x
        kind = np.full(base.n, mm.LOWER, dtype=np.uint8)
        fp0 = E.FlatProblem(m, base.n, base.n, _flatA(base.A), base.c, b, kind, lb, np.zeros(base.n), x, base.B, base.N,
                            np.zeros(nN, dtype=np.uint8))
        eng = E.Engine(E.ENGINE_PRIMAL, fp0, opts)
        try:
            eng.step(0)
            eng.step(1)
            fp = eng.read_point()
            x0, B, N = fp.x.copy(), fp.B.copy(), fp.N.copy()
            assert sorted(B) != sorted(base.B)
            x_set = x0.copy()
            if pattern != "zero":
                x_set[B[m // 3]] += 2e-11 * (1.0 + np.abs(x0[B]).max())
            eng.debug_set_x(x_set)
            before = eng.counters()
            eng.step(0)
            after = eng.counters()
            W = _binv(eng, m)
            t = eng.tap(E.TAP_RESYNC_T, m)
            cand = eng.tap(E.TAP_RESYNC_CAND, m)
            x1 = eng.read_point().x.copy()
        finally:
            eng.close()
        assert after["resyncs"] == before["resyncs"] + 1 and after["refreshes"] == before["refreshes"] + 1
        t_m = bm.rhs(base.A[:, N], x_set[N], b)
        cand_m, maxdiff, maxx, adopt, xB_m = bm.resync(W, t_m, x_set[B])
        print(f"resync m={m} x_N={pattern}: max|cand - x_B| {maxdiff:.3e}, max|x_B| {maxx:.3e}, adopted {adopt}")
        assert adopt == (pattern != "zero")
        _same_bits(f"resync m={m} x_N={pattern} t", t, t_m)
        _same_bits(f"resync m={m} x_N={pattern} cand", cand, cand_m)
        _same_bits(f"resync m={m} x_N={pattern} x_B", x1[B], xB_m)
        _same_bits(f"resync m={m} x_N={pattern} x_N", x1[N], x_set[N])

"""The kernels that keep an explicit-inverse engine right between two rebuilds of B^-1 (ellp_engine.hip), each against the
extended-precision model of tests/maint_model.py, entry by entry, within the rounding bound of an f64 evaluation in any
order: no factor on it.

    BTRAN                 k_btran_part / _reduce          u = B^-T c_B after step(0) of a primal engine with btran_mode 1
    drift monitor         k_drift_part / _reduce          its value, its threshold from both sides, NaN and Inf in B^-1
    resync of x_B         k_resync_gather / _part / _rhs / _xb / _apply     the threshold 1e-11 (1 + max|x_B|) from both
                          sides (Engine.debug_set_x puts the carried x_B where it is wanted), a refused refresh, a NaN
    dual start            launch_btran + k_dual_rephase + the forced resync, through Engine.dual_phase1 and dual_rephase
    primal phase-1 start  the front of the resync (b~ = b - A x) + k_phase1_art, through Engine.primal_phase1

All engines are pipeline 1: explicit inverse, three launches per iteration, no certifying hybrid.  The sizes are named after
the tile geometry they meet (maint_model.SIZES; engine_plan must agree): 1 tile, fewer than 8, exactly 8, 8k + 1 (9, 17, 33,
57), 64; a ragged last tile; m = ld and m = ld - 15.  tests/test_maint_model_cpu.py shows that the bounds let a correct
evaluation through and stop a dropped or doubled tile, a skipped row, a flipped sign, a lost last element, b + s and a
transposed W, and that no input here leaves a label or an adoption undecided.

Not covered: the aq_cur branch of the monitor (column-sharded engines), pp_skip (partial pricing), the usel = 1 buffer of
the two-launch pipeline.  ELLP_TAP_U delivers m entries whatever the count asked for, so the ld - m padding entries of u are
not looked at.  The maintenance request after a NaN or an Inf in B^-1 is followed on a dual engine: a primal engine's ratio test
meets the NaN too (k_ftran2 raises nan_flag), the monitor still reports NaN, and k_update2 ends the solve with ERR_NAN.

Largest |device - model| / bound met on an MI355X (records, not limits: the limit is 1):
    BTRAN u (the four W / c_B cases of a size)   m=1 0.600, 2 0.582, 16 0.077, 17 0.100, 64 0.016, 65 0.021, 129 0.008, 257 0.006,
                                                 512 0.003, 513 0.004, 520 0.003, 1030 0.001
    drift (primal / dual)                        m=17 0.045 / 0.035, 129 0.001 / 0.001, 520 0.001 / 0.001
    resync x_B                                   primal m=17 0.033, 129 0.018, 520 0.008; dual m=129 0.010
    dual_phase1 y / d / basic d / x_B            m=17 0.049 / 0.011 / 0.012 / 0.012, 64 0.009 / 0.001 / 0.002 / 0.001,
                                                 65 0.008 / 0.001 / 0.001 / 0.001, 257 0.001 / 0.000 / 0.000 / 0.000
    dual_rephase y / d / basic d / x_B           m=140 0.011 / 0.005 / 0.007 / 0.006
    primal_phase1 artificial values              m=17 0.031, 129 0.016, 520 0.065
"""
import numpy as np
import pytest

import maint_model as mm

pytestmark = pytest.mark.gpu
L = np.longdouble
ST_RUNNING = 100


def _E():
    from ellp_amd import _engine as E
    return E


def _opts(**kw):
    kw.setdefault("refactor_period", 1 << 30)
    return _E().default_opts(max_iter=None, pipeline=1, **kw)


def _flatA(A):
    return np.asarray(A).reshape(-1, order="F")


def _fp(c, dual=False):
    E = _E()
    return E.FlatProblem(c.m, c.n, c.n, _flatA(c.A), c.c, c.b, c.kind, c.lb, c.ub, c.x, c.B, c.N, c.Nb,
                         y=c.y if dual else None, d=c.d if dual else None)


def _binv(eng, m):
    return eng.tap(_E().TAP_BINV, m * m).reshape(m, m).copy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _inside(label, dev, model, bound):
    r = mm.worst(dev, model, bound)
    print(f"{label}: max |device - model| / bound = {r:.3f}")
    assert r <= 1.0, (label, r)
    return r


def _check_plan(kind, m, nN, opts):
    E = _E()
    s, plan, msg = E.engine_plan(kind, m, nN, opts)
    assert s == E.OPTIMAL, msg
    assert (int(plan["ld"]), int(plan["btran_rows"]), int(plan["btran_tiles"])) == mm.geometry(m), plan
    assert not plan["small"] and not plan["mid"] and not plan["hybrid"] and not plan["lagged"]


# ------------------------------------------------------------------------------------------------ BTRAN
@pytest.mark.parametrize("pattern", mm.C_PATTERNS)
@pytest.mark.parametrize("m", list(mm.SIZES), ids=mm.size_id)
def test_btran_against_the_model(m, pattern):
    """u = B^-T c_B from the engine's own rebuilt inverse and from a dense random matrix in its place (BTRAN does not care
    that it is an inverse), with c_B mostly zeros (the skip branch) and all nonzero"""
    E = _E()
    c = mm.btran_case(m, pattern)
    opts = _opts(btran_mode=1)
    _check_plan(E.ENGINE_PRIMAL, m, c.n - m, opts)
    eng = E.Engine(E.ENGINE_PRIMAL, _fp(c), opts)
    try:
        for which in ("own", "random"):
            if which == "random":
                eng.debug_set_inverse(c.W_random)
            W = _binv(eng, m)
            eng.step(0)
            assert int(eng.tap(E.TAP_STATE, 12)[0]) == ST_RUNNING
            u = eng.tap(E.TAP_U, m)
            mdl = mm.btran(W, c.c_B)
            _inside(f"btran m={m} c_B={pattern} W={which}", u, mdl.u, mdl.du)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ the drift monitor
def _drift_run(m, dual, damage=None):
    """a fresh engine, its inverse scaled by 1 + 1e-6 (and damaged), one iteration in two steps with the monitor in between.
    Returns what the monitor saw and what the model makes of the same d, the engine still open."""
    E = _E()
    kind = E.ENGINE_DUAL if dual else E.ENGINE_PRIMAL
    c = mm.pivot_case(m, dual)
    opts = _opts()
    _check_plan(kind, m, c.n - m, opts)
    eng = E.Engine(kind, _fp(c, dual), opts)
    try:
        assert eng.counters()["launches_per_iteration"] == 3
        W = _binv(eng, m) * mm.DRIFT_SCALE
        if damage is not None:
            W[damage[0], damage[1]] = damage[2]
        eng.debug_set_inverse(W)
        fp = eng.read_point()
        B, N, Nb = fp.B.copy(), fp.N.copy(), fp.Nb.copy()
        checks0 = eng.counters()["drift_checks"]
        eng.step(0)
        eng.step(1)
        d = eng.tap(E.TAP_D, m)
        st = eng.tap(E.TAP_STATE, 12)
        q, r = int(st[2]), int(st[3])
        cnt = eng.counters()
        sgn = 1.0 if dual or Nb[q] != mm.NB_LOWER else -1.0
        mdl = mm.drift(c.A[:, B], d, c.A[:, N[q]], sgn) if np.isfinite(d).all() else None
        return eng, cnt, cnt["drift_checks"] - checks0, mdl, r
    except Exception:
        eng.close()
        raise


@pytest.mark.parametrize("dual", [False, True], ids=["primal", "dual"])
@pytest.mark.parametrize("m", mm.DRIFT_SIZES, ids=mm.size_id)
def test_drift_value_against_the_model(m, dual, monkeypatch):
    monkeypatch.setenv("ELLP_DRIFT_EVERY", "1")
    eng, cnt, checks, mdl, _ = _drift_run(m, dual)
    eng.close()
    err = abs(L(cnt["drift"]) - mdl.rel)
    print(f"drift m={m} {'dual' if dual else 'primal'}: device {cnt['drift']!r}, model {float(mdl.rel)!r}, "
          f"|difference| / bound = {float(err / mdl.drel):.3f}")
    assert checks == 1
    assert 0.5e-6 < float(mdl.rel) < 2e-6
    assert err <= mdl.drel, (cnt["drift"], float(mdl.rel), float(mdl.drel))


@pytest.mark.parametrize("dual", [False, True], ids=["primal", "dual"])
def test_drift_threshold_from_both_sides(dual, monkeypatch):
    """drift_tol a thousandth below the drift: a maintenance request; a thousandth above: none.  The request of THIS check is
    read with poll(), which services it without running anything; the run(1) that follows makes an iteration and with it a
    check of its own, on the inverse as it is by then (refreshed after a request; still scaled, and one eta update on, after
    none: the dual engine's second drift is 1.08e-6, above the tolerance, the primal's is not).  So after run(1) the count
    has grown by one more exactly if the drift that run reports exceeds the tolerance."""
    m = 129
    monkeypatch.setenv("ELLP_DRIFT_EVERY", "1")
    eng, cnt0, _, mdl, _ = _drift_run(m, dual)
    eng.close()
    rel = float(mdl.rel)
    assert float(mdl.drel) < 1e-3 * (1e-3 * rel)  # the bound is orders below the gap
    for factor, requests in ((1.0 - 1e-3, 1), (1.0 + 1e-3, 0)):
        tol = rel * factor
        monkeypatch.setenv("ELLP_DRIFT_TOL", repr(tol))
        eng, cnt, checks, mdl2, _ = _drift_run(m, dual)
        try:
            assert checks == 1 and _bits(cnt["drift"]) == _bits(cnt0["drift"])  # the same run
            st_p, _, msg_p = eng.poll()
            polled = eng.counters()
            st, _, msg = eng.run(1)
            after = eng.counters()
        finally:
            eng.close()
        print(f"drift_tol = drift * {factor}: maintenance requests {cnt['maint_requests']} -> {polled['maint_requests']} (poll: status "
              f"{st_p} {msg_p!r}) -> {after['maint_requests']} (run(1): status {st} {msg!r}, its own check saw {after['drift']!r})")
        assert polled["maint_requests"] == cnt["maint_requests"] + requests, (factor, cnt, polled)
        assert polled["refreshes"] == cnt["refreshes"] + requests
        assert after["drift_checks"] == 2 and st == _E().MAXITER
        assert after["maint_requests"] == polled["maint_requests"] + (1 if after["drift"] > tol else 0), (factor, polled, after)
        if requests:
            assert after["drift"] < 1e-3 * tol  # the refresh that serviced the request has repaired the inverse


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_drift_monitor_sees_nan_and_inf(bad, monkeypatch):
    """One NaN in a row of B^-1 that is not the pivot row: d holds a NaN, the monitor's residual is NaN, it reports NaN and
    raises the maintenance request, which the next run services.  (With fmax folds the NaN dropped out: a small finite
    drift and no request.)  One +Inf: the residual is +Inf in every row, the drift +Inf, the request is raised (fmax or
    not)."""
    m = 129
    monkeypatch.setenv("ELLP_DRIFT_EVERY", "1")
    eng, _, _, _, r = _drift_run(m, True)
    eng.close()
    row = (r + 1) % m
    eng, cnt, checks, _, r2 = _drift_run(m, True, damage=(row, m // 2, bad))
    try:
        assert r2 == r and checks == 1
        st, _, msg = eng.run(1)
        after = eng.counters()
    finally:
        eng.close()
    print(f"{bad} in row {row} of B^-1 (pivot row {r}): drift {cnt['drift']!r}; next run: status {st} {msg!r}, "
          f"maintenance requests {cnt['maint_requests']} -> {after['maint_requests']}, rebuilds {cnt['rebuilds']} -> {after['rebuilds']}")
    assert np.isnan(cnt["drift"]) if np.isnan(bad) else np.isposinf(cnt["drift"]), cnt["drift"]
    assert after["maint_requests"] >= cnt["maint_requests"] + 1, (cnt, after)
    assert after["rebuilds"] >= cnt["rebuilds"] + 1, (cnt, after)  # a refresh cannot repair such an inverse: it is rebuilt from A_B


def test_drift_monitor_reports_nan_on_a_primal_engine_before_the_solve_ends(monkeypatch):
    """The same NaN on a primal engine: the monitor, which runs between the FTRAN and the update, reports NaN; the ratio
    test has met the NaN as well (k_ftran2 raises nan_flag for a basic variable off its bound), so k_update2 ends the solve
    with ERR_NAN and there is nothing left to maintain"""
    m = 129
    monkeypatch.setenv("ELLP_DRIFT_EVERY", "1")
    eng, _, _, _, r = _drift_run(m, False)
    eng.close()
    row = (r + 1) % m
    eng, cnt, checks, _, _ = _drift_run(m, False, damage=(row, m // 2, np.nan))
    try:
        st, _, msg = eng.run(1)
    finally:
        eng.close()
    print(f"primal, NaN in row {row} of B^-1 (pivot row {r}): drift {cnt['drift']!r}; next run: status {st} {msg!r}")
    assert checks == 1 and np.isnan(cnt["drift"]), cnt["drift"]
    assert st == _E().ERR_NAN, (st, msg)


# ------------------------------------------------------------------------------------------------ the resync of x_B
def _resync_run(m, dual, delta=None, nan=False, scale_inverse=None):
    """one pivot, then x_B[k] is moved by delta * (1 + max|x_B|) (or made NaN) and the maintenance that the next step(0)
    starts with (refactor_period 1) refreshes B^-1 and checks x_B against it.  Returns the case, what was set, what is there
    afterwards, the indices, the inverse the resync used and the counters before and after."""
    E = _E()
    kind = E.ENGINE_DUAL if dual else E.ENGINE_PRIMAL
    c = mm.pivot_case(m, dual)
    opts = _opts(refactor_period=1)
    _check_plan(kind, m, c.n - m, opts)
    eng = E.Engine(kind, _fp(c, dual), opts)
    try:
        eng.step(0)
        eng.step(1)
        fp = eng.read_point()
        x0, B, N = fp.x.copy(), fp.B.copy(), fp.N.copy()
        assert sorted(B) != sorted(c.B)  # a pivot has happened
        k = B[m // 3]
        x_set = x0.copy()
        if nan:
            x_set[k] = np.nan
        elif delta:
            x_set[k] += delta * (1.0 + np.abs(x0[B]).max())
        if scale_inverse:
            eng.debug_scale_inverse(scale_inverse)
        eng.debug_set_x(x_set)
        assert np.array_equal(_bits(eng.read_point().x), _bits(x_set))  # the hook is the mirror of read_point
        before = eng.counters()
        eng.step(0)
        after = eng.counters()
        W = _binv(eng, m)
        x1 = eng.read_point().x.copy()
        assert np.array_equal(eng.fp.B, B) and np.array_equal(eng.fp.N, N)
    finally:
        eng.close()
    assert after["resyncs"] == before["resyncs"] + 1 and after["refreshes"] == before["refreshes"] + 1
    return c, x0, x_set, x1, B, N, W, after


@pytest.mark.parametrize("m,dual", [(m, False) for m in mm.RESYNC_SIZES] + [(129, True)],
                         ids=[f"primal-{mm.size_id(m)}" for m in mm.RESYNC_SIZES] + [f"dual-{mm.size_id(129)}"])
def test_resync_threshold_from_both_sides(m, dual):
    """half the threshold away: x stays bit for bit what it was; twice the threshold: every x_B is the model's candidate
    within its bound and x_N is untouched.  Nonbasic variables sit at 0 (skipped), at a nonzero lower bound and (primal) at
    an upper bound, so b - A_N x_N has content."""
    c, x0, x_set, x1, B, N, W, _ = _resync_run(m, dual, delta=0.5e-11)
    A_N = c.A[:, N]
    clean = mm.resync(W, A_N, x0[N], c.b, x0[B])
    print(f"resync m={m}: carried x_B is {float(clean.maxdiff / clean.thr):.4f} of the threshold away from the candidate")
    assert clean.maxdiff <= 0.1 * clean.thr  # precondition: without a push the carried x_B is as good as the candidate
    assert (x0[N] == 0).any() and (x0[N] != 0).any()
    below = mm.resync(W, A_N, x_set[N], c.b, x_set[B])
    assert below.adopt is False
    assert np.array_equal(_bits(x1), _bits(x_set))
    c, x0, x_set, x1, B, N, W2, _ = _resync_run(m, dual, delta=2e-11)
    assert np.array_equal(_bits(W2), _bits(W))
    above = mm.resync(W, A_N, x_set[N], c.b, x_set[B])
    assert above.adopt is True
    _inside(f"resync m={m} {'dual' if dual else 'primal'} x_B", x1[B], above.cand, above.dcand)
    assert np.array_equal(_bits(x1[N]), _bits(x_set[N]))
    assert x1[B[m // 3]] != x_set[B[m // 3]]


def test_resync_after_a_refused_refresh_changes_nothing():
    """B^-1 scaled by 1.5: the refresh is refused (need_rebuild), and k_resync_apply leaves x alone although x_B is 1e-3 off:
    the inverse is rebuilt first, then x_B is checked again"""
    m = 129
    c, x0, x_set, x1, B, N, W, after = _resync_run(m, False, delta=1e-3, scale_inverse=1.5)
    assert after["last_refresh_residual"] >= 1e-4
    assert np.array_equal(_bits(x1), _bits(x_set))


def test_resync_with_a_nan_in_x_adopts_nothing():
    """a NaN in the carried x_B: |cand - x_B| is NaN, k_resync_xb records it as +Inf, and the isinf test of k_resync_apply
    keeps everything as it is: that is what the code does today, pinned here"""
    m = 129
    c, x0, x_set, x1, B, N, W, _ = _resync_run(m, False, nan=True)
    assert np.isnan(x_set).sum() == 1
    assert np.array_equal(_bits(x1), _bits(x_set))


# ------------------------------------------------------------------------------------------------ the dual start from the inverse
def _check_dual_point(label, c, fp, W, phase1):
    dp = mm.dual_point(W, c.A, c.c, c.b, c.kind, c.lb, c.ub, c.B, c.N, phase1)
    assert not dp.undecided.any() and not dp.panics.any()
    assert np.array_equal(fp.B, c.B) and np.array_equal(fp.N, c.N)
    _inside(f"{label} y", fp.y, dp.y, dp.dy)
    _inside(f"{label} d", fp.d, dp.d, dp.dd)
    _inside(f"{label} d of the basic variables against 0", fp.d[c.B], np.zeros(c.m), dp.dd[c.B] + np.abs(dp.d[c.B]))
    np.testing.assert_array_equal(fp.Nb, dp.labels)
    assert np.array_equal(_bits(fp.x[c.N]), _bits(dp.x_N))
    _inside(f"{label} x_B", fp.x[c.B], dp.x_B, dp.dx_B)
    return dp


@pytest.mark.parametrize("m", mm.BOX_SIZES)
def test_dual_phase1_point_against_the_model(m):
    """DualPhase1::new's point on a box LP (TwoSided and Fixed): BTRAN, k_dual_rephase with the phase-1 labelling and the
    forced resync together"""
    E = _E()
    c = mm.box_case(m)
    eng = E.Engine.dual_phase1(c.m, c.n, _flatA(c.A), c.c, c.b, c.kind, c.lb, c.ub, c.B, c.N, _opts())
    try:
        W = _binv(eng, m)
        fp = eng.read_point()
    finally:
        eng.close()
    dp = _check_dual_point(f"dual_phase1 m={m}", c, fp, W, True)
    assert set(np.unique(dp.labels)) == {mm.NB_LOWER, mm.NB_UPPER}


def test_dual_rephase_point_against_the_model():
    """DualPhase2::from's point on the mixed Lower / Upper / Free / TwoSided LP (140 rows): the engine is created on the box
    problem of the same matrix, then handed the phase-2 costs, right-hand side and bounds"""
    E = _E()
    c = mm.mixed_case()
    m, n = c.m, c.n
    z = np.zeros(n)
    box = E.FlatProblem(m, n, n, _flatA(c.A), z, np.zeros(m), np.full(n, mm.TWOSIDED, dtype=np.uint8), -np.ones(n), np.ones(n), z,
                        c.B, c.N, np.zeros(n - m, dtype=np.uint8), y=np.zeros(m), d=z)
    eng = E.Engine(E.ENGINE_DUAL, box, _opts())
    try:
        eng.dual_rephase(c.c, c.b, c.kind, c.lb, c.ub)
        W = _binv(eng, m)
        fp = eng.read_point()
    finally:
        eng.close()
    dp = _check_dual_point(f"dual_rephase m={m}", c, fp, W, False)
    assert set(np.unique(dp.labels)) == {mm.NB_LOWER, mm.NB_UPPER, mm.NB_FREE}


# ------------------------------------------------------------------------------------------------ the device-made primal phase 1
@pytest.mark.parametrize("m,n", mm.PHASE1_SIZES)
def test_primal_phase1_start_against_the_model(m, n):
    """b~ = b - A x: the artificial values are |b~| within its bound, the artificial columns signum(b~) e_i (seen as the
    diagonal of B^-1, which is the basis itself), with b~_0 = +0.0 and b~_1 = -0.0 exactly: +1 and -1"""
    E = _E()
    c = mm.phase1_case(m, n)
    mdl = mm.phase1_rhs(c.A, c.x, c.b)
    eng = E.Engine.primal_phase1(m, n, _flatA(c.A), c.b, c.kind, c.lb, c.ub, c.x, c.Nb, _opts())
    try:
        W = _binv(eng, m)
        fp = eng.read_point()
    finally:
        eng.close()
    assert np.array_equal(_bits(fp.x[:n]), _bits(c.x))
    _inside(f"primal_phase1 m={m} artificial values", fp.x[n:], np.abs(mdl.t), mdl.dt)
    t64 = np.asarray(mdl.t, dtype=np.float64)
    assert (np.abs(mdl.t[2:]) > mdl.dt[2:]).all()
    want = np.where(np.signbit(t64), -1.0, 1.0)
    want[0], want[1] = 1.0, -1.0  # b~ = +0.0 and -0.0: nothing is rounded there
    assert np.array_equal(_bits(fp.x[n:n + 2]), _bits(np.zeros(2)))
    np.testing.assert_array_equal(W, np.diag(want))

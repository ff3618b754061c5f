"""tests/se_model.py checked on the CPU (no GPU needed): the model is the definition's recurrence; a plain f64 numpy
evaluation of the creation formulas and of every step of both phases stays inside the derived bounds dG on every LP shape
tests/test_gpu_se_weights.py uses; each of five mistakes lands outside them at the first step that exercises it; the LPs
that test names do what it relies on.  Pivots are the oracle's under the restated rule (eo.set_primal_rule(1)), one loop
body per call."""
import functools

import numpy as np
import pytest

import refresh_model as rm
import se_model as sm
from oracle import ellp_oracle as eo

L = np.longdouble
BLOCK_EDGE_STEPS = 120  # the GPU test looks at steps 1-12 and 113-120 of phase 1 there


def _phase1(rows):
    seed, m, n = {**sm.SOLVES, **sm.BLOCK_EDGES}[rows]
    p1, err = eo.primal_phase1(eo.Problem.from_fixture(sm.boxed_lp(seed, m, n)))
    assert p1 is not None and not err
    assert p1.view().m == rows
    return p1


def _walk(v, limit):
    """one oracle loop body per call on the view v (in place).  Returns the end status and one record per loop body:
    (B, N before it, q, r) with r = -1 for a bound flip."""
    steps = []
    status = eo.MAXITER
    while len(steps) < limit:
        B0, N0, Nb0 = v.B.copy(), v.N[:v.nN].copy(), v.Nb[:v.nN].copy()
        status, _, msg = eo.primal_solve_with_initial(v, 1)
        if status != eo.MAXITER:
            break
        rr = np.flatnonzero(B0 != v.B)
        if rr.size:
            qq = np.flatnonzero(N0 != v.N[:v.nN])
            assert rr.size == 1 and qq.size == 1
            steps.append((B0, N0, int(qq[0]), int(rr[0])))
        else:
            qq = np.flatnonzero(Nb0 != v.Nb[:v.nN])
            assert qq.size == 1
            steps.append((B0, N0, int(qq[0]), -1))
    return status, steps


@functools.lru_cache(maxsize=None)
def _solve(rows):
    """(A, [(phase, status, steps)]) under the restated steepest-edge rule, made once per shape"""
    eo.set_primal_rule(1)
    try:
        p1 = _phase1(rows)
        v = p1.view()
        A = np.ascontiguousarray(v.A_matrix())
        if rows in sm.BLOCK_EDGES:
            st, steps = _walk(v, BLOCK_EDGE_STEPS)
            return A, [(1, st, steps)], None
        st1, steps1 = _walk(v, 1000)
        obj1 = v.obj()
        p1.store_point(v)
        v2 = eo.primal_phase2(p1).view()
        np.testing.assert_array_equal(v2.A, v.A)
        st2, steps2 = _walk(v2, 1000)
        return A, [(1, st1, steps1), (2, st2, steps2)], obj1
    finally:
        eo.set_primal_rule(0)


def _is_signed_perm(Bm):
    nz = Bm != 0.0
    return (nz.sum(axis=0) == 1).all() and (nz.sum(axis=1) == 1).all() and (np.abs(Bm[nz]) == 1.0).all()


def _replay(rows, mistake=None):
    """the f64 evaluation along the oracle's pivots, every step against the model built from the evaluation's OWN previous
    weights (as the GPU test builds it from the device's).  Yields (phase, k, record, model, G_f64, G_mutated)."""
    A, phases, _ = _solve(rows)
    G = None
    last = None
    for phase, _, steps in phases:
        for k, (B0, N0, q, r) in enumerate(steps):
            A_N = np.ascontiguousarray(A[:, N0])
            if G is None:
                if _is_signed_perm(A[:, B0]):
                    start, G = sm.start_perm(A_N), sm.start_perm_f64(A_N)
                else:  # the free variables are basic at the phase-1 start: a general basis
                    W0 = np.linalg.inv(A[:, B0])
                    start, G = sm.start_general(W0, A_N), sm.start_general_f64(W0, A_N)
                yield phase, -1, None, start, G, None
            if r < 0:
                Gm = None
                if mistake == "again_after_flip" and last is not None:
                    Gm = sm.step_f64(G, last[0], A_N, last[1], last[2], last[3])
                yield phase, k, (B0, N0, q, r), None, G, Gm
                continue
            W = np.linalg.inv(A[:, B0])
            d = W @ A_N[:, q]
            if k % 2:
                d = -d  # the device hands over +-alpha_q
            mdl = sm.step(G, W, A_N, q, r, d)
            Gn = sm.step_f64(G, W, A_N, q, r, d)
            Gm = sm.step_f64(G, W, A_N, q, r, d, mistake) if mistake and mistake != "again_after_flip" else None
            yield phase, k, (B0, N0, q, r), mdl, Gn, Gm
            G, last = Gn, (W, q, r, d)


ALL_ROWS = sorted(sm.SOLVES) + sorted(sm.BLOCK_EDGES)


@pytest.mark.parametrize("rows", ALL_ROWS)
def test_f64_evaluation_stays_inside_the_bounds(rows):
    worst = 0.0
    for phase, k, rec, mdl, G, _ in _replay(rows):
        if mdl is None:
            continue
        ratio = np.abs(G.astype(L) - mdl.G) / mdl.dG
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1).all(), (rows, phase, k, int(np.argmax(ratio)), float(ratio.max()))
    print(f"rows {rows}: max |G_f64 - G_model| / dG = {worst:.3f}")
    assert worst > 0.0


@pytest.mark.parametrize("rows", sorted(sm.SOLVES))
def test_f64_general_start_stays_inside_its_bound(rows):
    """the start at phase 1's end basis (a general basis), as a fresh engine makes it"""
    A, phases, _ = _solve(rows)
    B0, N0, _, _ = phases[1][2][0]
    assert not _is_signed_perm(A[:, B0])
    W = np.linalg.inv(A[:, B0])
    A_N = np.ascontiguousarray(A[:, N0])
    mdl = sm.start_general(W, A_N)
    ratio = np.abs(sm.start_general_f64(W, A_N).astype(L) - mdl.G) / mdl.dG
    assert (ratio <= 1).all(), float(ratio.max())
    # and the formula is the definition's, up to the f64 inverse it starts from
    ref = sm.definition(A, B0, N0)
    tol = np.linalg.cond(A[:, B0]) * A.shape[0] * 2.0 ** -52
    assert (np.abs(mdl.G - ref) <= tol * ref).all(), (float((np.abs(mdl.G - ref) / ref).max()), tol)


@pytest.mark.parametrize("rows", [17, 39])
def test_model_step_is_the_definitions_recurrence(rows):
    """from the definition's weights, one model step with an accurate inverse gives the definition's weights of the next
    basis: the Goldfarb-Reid identity, to what the f64 inverse allows"""
    A, phases, _ = _solve(rows)
    for phase, _, steps in phases:
        piv = [s for s in steps if s[3] >= 0]
        for B0, N0, q, r in piv[:3] + piv[-3:]:
            W = np.linalg.inv(A[:, B0])
            A_N = np.ascontiguousarray(A[:, N0])
            G0 = np.asarray(sm.definition(A, B0, N0), dtype=np.float64)
            mdl = sm.step(G0, W, A_N, q, r, W @ A_N[:, q])
            B1, N1 = B0.copy(), N0.copy()
            B1[r], N1[q] = N0[q], B0[r]
            ref = sm.definition(A, B1, N1)
            err = float((np.abs(mdl.G - ref) / ref).max())
            tol = (np.linalg.cond(A[:, B0]) + np.linalg.cond(A[:, B1])) * A.shape[0] * 2.0 ** -52  # of the f64 inverse
            assert err < tol, (rows, phase, q, r, err, tol)


def _exercised(mistake, rec, mdl, G_before, had_pivot):
    """does this loop body exercise the mistake?  sign / dropped: a pivot; q_kept: a pivot; stored_gq: a pivot at which the
    stored weight is no f64 evaluation of 1 + |alpha|^2 (further from it than that sum's own bound); again_after_flip: a
    flip that follows a pivot"""
    q, r = rec[2], rec[3]
    if mistake == "again_after_flip":
        return r < 0 and had_pivot
    if r < 0:
        return False
    if mistake == "stored_gq":
        return abs(L(G_before[q]) - mdl.gq) > mdl.dgq
    return True


@pytest.mark.parametrize("rows", [17, 39, 70])
@pytest.mark.parametrize("mistake", sm.MISTAKES)
def test_each_mistake_lands_outside_the_bounds(mistake, rows):
    """At the first loop body that exercises the mistake, no fewer than half the positions it touches (those where the
    mutated f64 evaluation differs from the right one at all) are outside dG.  "stored_gq" is the exception, and it is
    stated, not hidden: the stored weight starts as an f64 evaluation of the same sum and drifts away from it pivot by
    pivot, so at the first pivot where it is further from 1 + |alpha|^2 than that sum's own bound (phase 1, step 10 / 8 /
    8 at 17 / 39 / 70 rows) only 3 of 30 / 1 of 74 / 1 of 137 touched positions are outside yet; asserted for it: at that
    step at least one position is outside, and no fewer than half are within the next 10 pivots."""
    G_before, had_pivot, phase_now, first = None, False, 0, None
    pivots_since = 0
    for phase, k, rec, mdl, G, Gm in _replay(rows, mistake):
        if rec is None:
            G_before = G
            continue
        if phase != phase_now:
            phase_now, had_pivot = phase, False  # the hand-off drops the pending update
        hit = _exercised(mistake, rec, mdl, G_before, had_pivot)
        had_pivot = had_pivot or rec[3] >= 0
        if not hit:
            G_before = G
            continue
        touched = Gm != G
        outside = touched if mdl is None else np.abs(Gm.astype(L) - mdl.G) > mdl.dG  # a flip: the weights must not move at all
        n_t, n_o = int(touched.sum()), int((outside & touched).sum())
        print(f"{mistake}, rows {rows}: phase {phase} step {k}: {n_t} positions touched, {n_o} outside dG")
        assert n_t >= 1
        if mistake != "stored_gq":
            assert 2 * n_o >= n_t, (mistake, rows, phase, k)
            return
        if first is None:
            first = (phase, k)
            assert n_o >= 1, (mistake, rows, phase, k)
        if 2 * n_o >= n_t:
            return
        pivots_since += 1
        assert pivots_since <= 10, (mistake, rows, first, phase, k)
        G_before = G
    raise AssertionError(f"{mistake}: never exercised on rows {rows}")


@pytest.mark.parametrize("rows", sorted(sm.SOLVES))
def test_the_lps_do_what_the_gpu_test_relies_on(rows):
    A, phases, obj1 = _solve(rows)
    (_, st1, steps1), (_, st2, steps2) = phases
    assert st1 == eo.OPTIMAL and st2 == eo.OPTIMAL
    assert abs(obj1) < 1e-10  # phase 1 found a feasible point
    flips1 = sum(1 for s in steps1 if s[3] < 0)
    flips2 = sum(1 for s in steps2 if s[3] < 0)
    print(f"rows {rows}: phase 1 {len(steps1)} steps, {flips1} flips; phase 2 {len(steps2)} steps, {flips2} flips")
    assert flips2 >= 1 and len(steps1) < 300 and len(steps2) < 300  # the GPU test checks every step of both phases


@pytest.mark.parametrize("rows", sorted(sm.BLOCK_EDGES))
def test_the_block_edge_lps_run_long_enough(rows):
    _, phases, _ = _solve(rows)
    assert phases[0][1] == eo.MAXITER and len(phases[0][2]) == BLOCK_EDGE_STEPS


@pytest.mark.skipif(not rm.LONGDOUBLE_IS_WIDE, reason="np.longdouble is not the 80-bit format here: only double-double exists")
@pytest.mark.parametrize("rows", [16, 39])
def test_definition_in_both_arithmetics(rows):
    """np.longdouble against pure double-double.  The 80-bit residual stops the refinement at cond(B) 2^-63, so that run is
    asked for 2^-40 only and the two must agree to 2^-38"""
    A, phases, _ = _solve(rows)
    for B0, N0, _, _ in (phases[0][2][0], phases[1][2][0], phases[1][2][-1]):
        a = sm.definition(A, B0, N0, arith=sm._Wide, tol=2.0 ** -40)
        b = sm.definition(A, B0, N0, arith=sm._DD)
        assert (np.abs(a - b) <= 2.0 ** -38 * a).all(), float((np.abs(a - b) / a).max())
    # and one step, one general start
    B0, N0, q, r = next(s for s in phases[1][2] if s[3] >= 0)
    W, A_N = np.linalg.inv(A[:, B0]), np.ascontiguousarray(A[:, N0])
    G0 = sm.start_general_f64(W, A_N)
    sa, sb = sm.step(G0, W, A_N, q, r, W @ A_N[:, q], arith=sm._Wide), sm.step(G0, W, A_N, q, r, W @ A_N[:, q], arith=sm._DD)
    assert (np.abs(sa.G - sb.G) <= 2.0 ** -8 * sa.dG).all()
    ga, gb = sm.start_general(W, A_N, arith=sm._Wide), sm.start_general(W, A_N, arith=sm._DD)
    assert (np.abs(ga.G - gb.G) <= 2.0 ** -8 * ga.dG).all()


def test_definition_against_exact_rational_arithmetic():
    """a 4 x 4 basis and 5 columns in Fractions (Gauss-Jordan, exact): the double-double definition must agree to 2^-58,
    the 2^-60 of its refinement carried through the sum of squares"""
    from fractions import Fraction
    rng = np.random.default_rng(11)
    m, nN = 4, 5
    A = np.hstack([rng.uniform(-1.0, 1.0, size=(m, m)) + np.diag([1.5, -2.0, 1.0, 3.0]), rng.uniform(-1.0, 1.0, size=(m, nN))])
    M = [[Fraction(float(A[i, j])) for j in range(m + nN)] for i in range(m)]
    for k in range(m):
        p = max(range(k, m), key=lambda i: abs(M[i][k]))
        M[k], M[p] = M[p], M[k]
        M[k] = [x / M[k][k] for x in M[k]]
        for i in range(m):
            if i != k:
                M[i] = [x - M[i][k] * y for x, y in zip(M[i], M[k])]
    exact = [1 + sum(M[i][m + j] ** 2 for i in range(m)) for j in range(nN)]
    got = sm.definition(A, np.arange(m), np.arange(m, m + nN))
    if rm.LONGDOUBLE_IS_WIDE:
        for j in range(nN):
            hi = float(got[j])
            lo = float(got[j] - L(hi))
            err = abs(Fraction(hi) + Fraction(lo) - exact[j]) / exact[j]
            assert err <= Fraction(1, 2 ** 58), (j, float(err))
    else:  # np.longdouble holds no more than f64 here: the returned value is the rounded one
        for j in range(nN):
            assert abs(Fraction(float(got[j])) - exact[j]) / exact[j] <= Fraction(1, 2 ** 52)

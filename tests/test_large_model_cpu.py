"""tests/large_model.py without a device: the model takes the oracle's pivots where the oracle is affordable, and the
committed cases decide nothing by rounding — the condition under which tests/test_gpu_large_pivots.py may demand the
model's pivots of the engine with no allowance for ties."""
import functools

import numpy as np
import pytest

import large_model as lm
from oracle import ellp_oracle as eo


# ------------------------------------------------------------------------------------------------- the model against the oracle
@pytest.mark.parametrize("m", [130, 300])
@pytest.mark.parametrize("kind_of,quirks", [(lm.PRIMAL, False), (lm.PRIMAL, True), (lm.DUAL, False)])
def test_model_takes_the_oracles_pivots(kind_of, quirks, m):
    """60 loop bodies of the explicit-inverse CPU loop from a dense start basis with the eight unit columns and mixed bounds:
    the same index sets and labels, the same x (y, d) to rounding, in long double and in f64.  quirks: with fixed and
    two-sided basic variables, whose exact-zero ties the committed cases avoid."""
    W = 60
    cs = lm.make_case(kind_of, m, 272, 7, 60 if kind_of == lm.PRIMAL else 40, quirks=quirks)
    assert set(np.unique(cs.kind[cs.B])) | set(np.unique(cs.kind[cs.N])) == {0, 1, 2, 3, 4}
    assert (np.count_nonzero(cs.A[:, cs.N], axis=0) == 1).sum() == 8
    ov = cs.view()
    solve = eo.primal_binv_solve_with_initial if kind_of == lm.PRIMAL else eo.dual_binv_solve_with_initial
    st, it, msg, _ = solve(ov, W)
    assert st == eo.MAXITER and it == W, msg
    for dtype in (lm.L, np.float64):
        mo = lm.Model(cs, dtype=dtype)
        assert mo.run(W) == lm.MAXITER and mo.iters == W
        np.testing.assert_array_equal(mo.B, ov.B)
        np.testing.assert_array_equal(mo.N, ov.N)
        np.testing.assert_array_equal(mo.Nb, ov.Nb)
        names = ("x", "y", "d") if kind_of == lm.DUAL else ("x",)
        for name in names:
            want = getattr(ov, name)
            assert np.abs(getattr(mo, name).astype(np.float64) - want).max() <= 1e-10 * (1 + np.abs(want).max()), name
    if kind_of == lm.PRIMAL and not quirks:
        flips = sum(1 for _, _, r in mo.pivots if r < 0)
        assert 0 < flips < W  # bound flips and pivots both occur
    if quirks:
        assert any(what == "leave" and sep == 0.0 for _, what, sep in mo.decisions)  # a tie at exactly 0, settled by the index


@pytest.mark.parametrize("m", [130, 300])
def test_model_runs_to_the_oracles_end(m):
    """a primal and a dual case solved to the end: the oracle's status, iteration count and point"""
    for kind_of, count, scale in ((lm.PRIMAL, 12, 8.0), (lm.DUAL, 10, 0.02)):
        cs = lm.make_case(kind_of, m, 272, 11, count, scale)
        ov = cs.view()
        solve = eo.primal_binv_solve_with_initial if kind_of == lm.PRIMAL else eo.dual_binv_solve_with_initial
        st, it, msg, _ = solve(ov, 400)
        mo = lm.Model(cs)
        assert mo.run(400) == st == lm.OPTIMAL and mo.iters == it, msg
        np.testing.assert_array_equal(mo.B, ov.B)
        np.testing.assert_array_equal(mo.Nb, ov.Nb)
        assert np.abs(mo.x.astype(np.float64) - ov.x).max() <= 1e-10 * (1 + np.abs(ov.x).max())


@pytest.mark.parametrize("m", [130, 300])
def test_rows_and_weights_against_a_dense_inverse(m):
    """rows of the product-form B^-1, one by one and in a batch, and gamma_j = 1 + |B^-1 a_j|^2 after 30 pivots, against
    numpy's inverse of the basis the model stands on"""
    cs = lm.make_case(lm.PRIMAL, m, 272, 5, 60)
    mo = lm.Model(cs)
    mo.run(30)
    assert len(mo.etas) > 15
    W = np.linalg.inv(cs.A[:, mo.B])
    tol = 1e-12 * (1 + np.abs(W).max())
    assert np.abs(mo.rows(np.arange(m)).astype(np.float64) - W).max() <= tol
    for i in (0, int(mo.etas[0][0]), int(mo.etas[-1][0]), m - 1):
        assert np.abs(mo.row(i).astype(np.float64) - W[i]).max() <= tol
    part = len(mo.etas) // 2
    Wp = np.linalg.inv(cs.A[:, mo.B_after[part]])
    assert np.abs(mo.rows(np.arange(m), upto=part).astype(np.float64) - Wp).max() <= tol
    G = 1 + ((W @ cs.A[:, mo.N]) ** 2).sum(axis=0)
    assert np.abs(mo.gamma_now().astype(np.float64) - G).max() <= 1e-12 * G.max()


def test_steepest_edge_model_takes_the_oracles_pivots():
    """|r_j| / sqrt(gamma_j) with the weights from their definition against the oracle's steepest-edge rule (exact start,
    Goldfarb-Reid updates) in its LU-per-iteration loop"""
    cs = lm.make_case(lm.PRIMAL, 130, 272, 7, 60)
    ov = cs.view()
    eo.set_primal_rule(1)
    try:
        st, it, msg = eo.primal_solve_with_initial(ov, 30)
    finally:
        eo.set_primal_rule(0)
    mo = lm.Model(cs, steepest_edge=True)
    assert mo.run(30) == st == lm.MAXITER and it == 30, msg
    np.testing.assert_array_equal(mo.B, ov.B)
    np.testing.assert_array_equal(mo.Nb, ov.Nb)
    assert np.abs(mo.x.astype(np.float64) - ov.x).max() <= 1e-10 * (1 + np.abs(ov.x).max())


# --------------------------------------------------------------------------------------- the committed cases decide nothing by rounding
RUNS = [(name, False, lm.CASES[name][6]) for name in lm.CASES] + [("p4097", True, 16)]


@functools.lru_cache(maxsize=None)
def _pair(name, se, window):
    cs = lm.case(name)
    out = []
    for dtype in (lm.L, np.float64):
        mo = lm.Model(cs, dtype=dtype, steepest_edge=se)
        mo.run(window)
        mo.AN = mo.A = None  # only the logs and the point are looked at
        out.append(mo)
    return out


@pytest.mark.parametrize("name,se,window", RUNS, ids=["%s%s" % (r[0], "-se" if r[1] else "") for r in RUNS])
def test_committed_cases_are_separated(name, se, window):
    """over the whole window, in both precisions: every entering and leaving decision at least SEP_MIN (relative) from its
    runner-up, no compared quantity in [NEAR_LO, NEAR_HI], and the f64 run takes the long-double run's pivots"""
    hi, lo = _pair(name, se, window)
    for mo in (hi, lo):
        assert mo.decisions
        worst = min(mo.decisions, key=lambda d: d[2])
        assert worst[2] >= lm.SEP_MIN, worst
        assert not mo.near and mo.compared_min_outside > 0, mo.near
    assert hi.pivots == lo.pivots and hi.status == lo.status and hi.iters == lo.iters
    assert lm.SEP_MIN == 1e-6 and (lm.NEAR_LO, lm.NEAR_HI) == (1e-13, 1e-7) and lm.MARGIN <= 1024


@pytest.mark.parametrize("name", ["p4097end", "d4096end"])
def test_terminating_cases_end_optimal_within_their_window(name):
    """... and at a vertex within its bounds: the reference's rules can end elsewhere (quirk Q1 leaves a two-sided variable
    nonbasic off its bound, the dual rule never looks at a fixed basic variable), and the GPU test's KKT check needs a
    true optimum"""
    hi, _ = _pair(name, False, lm.CASES[name][6])
    assert hi.status == lm.OPTIMAL and 20 < hi.iters <= 80
    cs, x = hi.cs, hi.x.astype(np.float64)
    N, Nb, B = hi.N, hi.Nb, hi.B
    at = np.where(Nb == lm.NB_LOWER, cs.lb[N], np.where(Nb == lm.NB_UPPER, cs.ub[N], x[N]))
    assert np.abs(x[N] - at).max() <= 1e-12 * (1 + np.abs(x).max())
    k = cs.kind[B]
    assert (np.where((k == lm.LOWER) | (k == lm.TWOSIDED) | (k == lm.FIXED), cs.lb[B] - x[B], -1.0) <= lm.EPS).all()
    assert (np.where((k == lm.UPPER) | (k == lm.TWOSIDED) | (k == lm.FIXED), x[B] - cs.ub[B], -1.0) <= lm.EPS).all()


def test_window_cases_do_not_end():
    for name, se, window in RUNS:
        if not name.endswith("end"):
            hi, _ = _pair(name, se, window)
            assert hi.status == lm.MAXITER and hi.iters == window, name

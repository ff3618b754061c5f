"""The two models of tests/ranging_model.py against a hand-worked LP and against each other, the special cases of the
definitions (include/ellp_hip.h) one by one, and the refusals of the C ABI that need no device."""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ranging_model as RM  # noqa: E402

INF = RM.INF
EPS = 1e-10


def _hand():
    """min c.x, A x = b.  Basis {0, 1}; nonbasic 2, 3 at Lower, 4 (TwoSided [0, 1]) at Upper, 5 Fixed at 0; variable 6 has a
    cost and no column.  A_B = [[1, 1], [1, 3]], B^-1 = [[1.5, -0.5], [-0.5, 0.5]], x_B = (3, 1), y = (-1.5, -0.5),
    d_N = (1.5, 0.5, -1.5, 0.25); tableau rows (1.5, -0.5, 1.5, 1) and (-0.5, 0.5, -0.5, 0).  Variable 1 is TwoSided [0, 4]."""
    A = np.array([[1.0, 1.0, 1.0, 0.0, 1.0, 1.0],
                  [1.0, 3.0, 0.0, 1.0, 0.0, 1.0]])
    c = np.array([-2.0, -3.0, 0.0, 0.0, -3.0, -1.75, 1.0])
    kind = np.array([1, 3, 1, 1, 3, 4, 1], dtype=np.uint8)
    lb = np.zeros(7)
    ub = np.array([0.0, 4.0, 0.0, 0.0, 1.0, 0.0, 0.0])
    x = np.array([3.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0])
    b = A @ x[:6]
    B, N, Nb = np.array([0, 1]), np.array([2, 3, 4, 5]), np.array([0, 0, 1, 0], dtype=np.uint8)
    return dict(m=2, n=6, n_c=7, A=A, c=c, b=b, kind=kind, lb=lb, ub=ub, x=x, B=B, N=N, Nb=Nb)


# what the definitions give, worked by hand
HAND_COST = {  # variable: (down, up, blocking_down, blocking_up)
    0: (-1.0, 1.0, 3, 2),      # down: 0.5 / -0.5 at position 1 and -1.5 / 1.5 at position 2 tie: the first, variable 3
    1: (-3.0, 1.0, 2, 3),      # up: 0.5 / 0.5 = 1 (variable 3) before -1.5 / -0.5 = 3 (variable 4)
    2: (-1.5, INF, 2, -1),
    3: (-0.5, INF, 3, -1),
    4: (-INF, 1.5, -1, 4),
    5: (-INF, INF, -1, -1),    # Fixed; as a Lower variable it would have limited variable 0's up at 0.25
    6: (-INF, INF, -1, -1),    # no column
}
HAND_RHS = {  # row: (down, up, blocking_down, blocking_up)
    0: (-2.0, 2.0, 0, 1),      # down: 3 / -1.5 (variable 0) against (4 - 1) / -0.5 = -6; up: 1 / 0.5
    1: (-2.0, 6.0, 1, 0),      # up: 3 / 0.5 (variable 0) and (4 - 1) / 0.5 (variable 1) tie: the first
}


def _f64_ranges(p):
    A_B, A_N = p["A"][:, p["B"]], p["A"][:, p["N"]]
    W = np.linalg.inv(A_B)
    y = W.T @ p["c"][p["B"]]
    d = p["c"].copy()
    d[:p["n"]] = p["c"][:p["n"]] - p["A"].T @ y
    cost = RM.cost_ranging_f64(W @ A_N, d, p["B"], p["N"], p["Nb"], p["kind"], p["n"], p["n_c"], EPS)
    rhs = RM.rhs_ranging_f64(W, p["x"], p["B"], p["kind"], p["lb"], p["ub"], EPS)
    return cost, rhs


def test_hand_worked_lp_f64_model():
    cost, rhs = _f64_ranges(_hand())
    for v, want in HAND_COST.items():
        assert tuple(float(a[v]) if k < 2 else int(a[v]) for k, a in enumerate(cost)) == want, (v, [a[v] for a in cost])
    for k, want in HAND_RHS.items():
        assert tuple(float(a[k]) if q < 2 else int(a[k]) for q, a in enumerate(rhs)) == want, (k, [a[k] for a in rhs])
    assert not np.signbit(np.concatenate([cost[0], cost[1], rhs[0], rhs[1]])[np.concatenate([cost[0], cost[1], rhs[0], rhs[1]]) == 0.0]).any()


def test_hand_worked_lp_exact_model():
    p = _hand()
    ex = RM.ExactRanging(**p)
    assert [[float(v) for v in row] for row in ex.W] == [[1.5, -0.5], [-0.5, 0.5]]
    assert [float(v) for v in ex.dN] == [1.5, 0.5, -1.5, 0.25]
    for i, v in enumerate(p["B"]):
        assert ex.cost_basic(i) == HAND_COST[int(v)]
    for j, v in enumerate(p["N"]):
        assert ex.cost_nonbasic(j) == HAND_COST[int(v)]
    for k in range(2):
        assert ex.rhs(k) == HAND_RHS[k]
    # what the limits mean
    for i, v in enumerate(p["B"]):
        dn, up, bd, bu = HAND_COST[int(v)]
        ex.check_cost_limit(i, up, bu, True)
        ex.check_cost_limit(i, dn, bd, False)
    for k in range(2):
        dn, up, bd, bu = HAND_RHS[k]
        ex.check_rhs_limit(k, up, bu, True)
        ex.check_rhs_limit(k, dn, bd, False)


def test_the_meaning_check_refuses_a_wrong_limit():
    ex = RM.ExactRanging(**_hand())
    for bad in (0.5, 2.0):  # too small: the blocker keeps its sign outside; too large: a sign is lost inside
        try:
            ex.check_cost_limit(0, bad, 2, True)
        except AssertionError:
            continue
        raise AssertionError(f"a wrong limit {bad} passed the meaning check")


def _seeded(seed=20260301, m=6, n=10):
    rng = np.random.default_rng(seed)
    A = np.round(rng.normal(size=(m, n)) * 8) / 8
    perm = rng.permutation(n)
    B, N = np.sort(perm[:m]), np.sort(perm[m:])
    kind = rng.choice([1, 2, 3], size=n).astype(np.uint8)
    lb, ub = np.where(kind != 2, -1.0, 0.0), np.where(kind != 1, 2.0, 0.0)
    Nb = np.array([0 if kind[v] == 1 else (1 if kind[v] == 2 else rng.integers(0, 2)) for v in N], dtype=np.uint8)
    x = np.zeros(n)
    x[N] = np.where(Nb == 0, lb[N], ub[N])
    x[B] = rng.uniform(-0.5, 1.5, size=m)
    # costs that make the basis optimal: d_N with the sign the label demands
    y = rng.normal(size=m)
    dN = np.where(Nb == 0, 1.0, -1.0) * rng.uniform(0.1, 2.0, size=n - m)
    c = A.T @ y
    c[N] += dN
    return dict(m=m, n=n, n_c=n, A=A, c=c, b=A @ x, kind=kind, lb=lb, ub=ub, x=x, B=B, N=N, Nb=Nb)


def test_models_agree_on_a_seeded_case():
    p = _seeded()
    cost, rhs = _f64_ranges(p)
    ex = RM.ExactRanging(**p)
    pos = {int(v): j for j, v in enumerate(p["N"])}

    def close(got, want):
        want = float(want)
        return got == want if np.isinf(want) or want == 0 else abs(got - want) <= 1e-9 * abs(want)

    for i, v in enumerate(p["B"]):
        dn, up, bd, bu = ex.cost_basic(i)
        assert close(cost[0][v], dn) and close(cost[1][v], up) and (cost[2][v], cost[3][v]) == (bd, bu), (i, v)
        if np.isfinite(cost[1][v]):
            ex.check_cost_limit(i, cost[1][v], cost[3][v], True)
        if np.isfinite(cost[0][v]):
            ex.check_cost_limit(i, cost[0][v], cost[2][v], False)
    for v, j in pos.items():
        dn, up, bd, bu = ex.cost_nonbasic(j)
        assert close(cost[0][v], dn) and close(cost[1][v], up) and (cost[2][v], cost[3][v]) == (bd, bu), v
    for k in range(p["m"]):
        dn, up, bd, bu = ex.rhs(k)
        assert close(rhs[0][k], dn) and close(rhs[1][k], up) and (rhs[2][k], rhs[3][k]) == (bd, bu), k
        if np.isfinite(rhs[1][k]):
            ex.check_rhs_limit(k, rhs[1][k], rhs[3][k], True)
        if np.isfinite(rhs[0][k]):
            ex.check_rhs_limit(k, rhs[0][k], rhs[2][k], False)


def _one_row(alpha, d, Nb, kind=None):
    """the cost range of ONE basic variable (variable 0) against nonbasic variables 1 .. k"""
    k = len(alpha)
    kind = np.array([1] + ([1] * k if kind is None else list(kind)), dtype=np.uint8)
    out = RM.cost_ranging_f64(np.array([alpha], dtype=np.float64), np.concatenate([[0.0], d]), [0], np.arange(1, k + 1), Nb, kind, k + 1, k + 1, EPS)
    return tuple(a[0] for a in out)


def test_infinities_and_eps():
    # nothing eligible: entries within eps, or of the sign that never blocks
    assert _one_row([1e-11, -1e-11], [1.0, 1.0], [0, 0]) == (-INF, INF, -1, -1)
    assert _one_row([2.0], [1.0], [0]) == (-INF, 0.5, -1, 1)     # Lower, alpha > 0: only up
    assert _one_row([-2.0], [1.0], [0]) == (-0.5, INF, 1, -1)
    assert _one_row([2.0], [-1.0], [1]) == (-0.5, INF, 1, -1)    # Upper, alpha > 0: only down
    assert _one_row([-2.0], [-1.0], [1]) == (-INF, 0.5, -1, 1)


def test_fixed_kind_is_not_read():
    assert _one_row([2.0, 4.0], [1.0, 1.0], [0, 0], kind=[4, 1]) == (-INF, 0.25, -1, 2)
    assert _one_row([np.nan, 4.0], [np.nan, 1.0], [0, 0], kind=[4, 1]) == (-INF, 0.25, -1, 2)  # not even its NaN


def test_free_label_limits_both_sides():
    dn, up, bd, bu = _one_row([2.0, 8.0], [1.0, 8.0], [2, 0])
    assert (dn, up, bd, bu) == (0.0, 0.5, 1, 1) and not np.signbit(dn)  # up 1 / 2, down min(1, 0) / 2 = 0
    assert _one_row([-2.0], [1.0], [2]) == (-0.5, 0.0, 1, 1)
    assert _one_row([2.0], [0.0], [2]) == (0.0, 0.0, 1, 1)
    # as a nonbasic variable of its own
    out = RM.cost_ranging_f64(np.zeros((1, 2)), np.array([0.0, 0.25, -0.25]), [0], [1, 2], [2, 2], np.array([1, 0, 0]), 3, 3, EPS)
    assert (out[0][1], out[1][1], out[0][2], out[1][2]) == (-0.25, 0.0, 0.0, 0.25)


def test_a_wrong_signed_d_is_clamped():
    assert _one_row([2.0], [-1e-12], [0]) == (-INF, 0.0, -1, 1)  # Lower with d < 0: the limit is 0, never negative
    assert _one_row([2.0], [1e-12], [1]) == (0.0, INF, 1, -1)
    out = RM.cost_ranging_f64(np.zeros((1, 1)), np.array([0.0, -1e-12]), [0], [1], [0], np.array([1, 1]), 2, 2, EPS)
    assert out[0][1] == 0.0 and not np.signbit(out[0][1]) and out[1][1] == INF


def test_nan_rule():
    # a NaN alpha: both limits, whatever else the row holds; blocking: the first position with a NaN
    dn, up, bd, bu = _one_row([4.0, np.nan, -4.0], [1.0, 1.0, 1.0], [0, 0, 0])
    assert np.isnan(dn) and np.isnan(up) and (bd, bu) == (2, 2)
    # a NaN d: in the rows where its column is a candidate
    dn, up, bd, bu = _one_row([4.0, 2.0], [1.0, np.nan], [0, 0])
    assert np.isnan(dn) and np.isnan(up)
    assert _one_row([4.0, 1e-12], [1.0, np.nan], [0, 0]) == (-INF, 0.25, -1, 1)  # |alpha| <= eps: d is not read
    # the right-hand sides: a NaN x is read where |w| > eps
    W = np.array([[1.0, 0.0], [0.5, 1.0]])
    out = RM.rhs_ranging_f64(W, np.array([np.nan, 1.0]), [0, 1], np.array([1, 1]), np.zeros(2), np.zeros(2), EPS)
    assert np.isnan(out[0][0]) and np.isnan(out[1][0]) and (out[0][1], out[1][1]) == (-1.0, INF)
    out = RM.rhs_ranging_f64(np.array([[np.nan, 1.0], [0.0, 1.0]]), np.array([1.0, 1.0]), [0, 1], np.array([0, 0]), np.zeros(2), np.zeros(2), EPS)
    assert np.isnan(out[0][0]) and np.isnan(out[1][0]) and (out[0][1], out[1][1]) == (-INF, INF)  # Free basic variables: no limit
    assert np.isnan(RM.inverse_residual_f64(np.eye(2), np.array([[1.0, np.nan], [0.0, 1.0]])))
    assert RM.inverse_residual_f64(np.array([[2.0, 0.0], [0.0, 4.0]]), np.array([[0.5, 0.125], [0.0, 0.25]])) == 0.25


def test_exact_inverse():
    rng = np.random.default_rng(5)
    M = rng.normal(size=(7, 7))
    W = RM.exact_inverse(M)
    for i in range(7):
        for j in range(7):
            assert sum(Fraction(float(M[i, k])) * W[k][j] for k in range(7)) == (1 if i == j else 0)


def test_refusals_need_no_device():
    from ellp_amd import _engine as E
    L = E.lib()
    err = C.create_string_buffer(512)
    rg = E.Ranging(2, 7)
    assert L.ellp_engine_ranging(None, C.byref(rg._out()), err, 512) == E.ERR_ARG and b"no engine" in err.value
    pos, al = np.zeros(1, dtype=np.int64), np.zeros(4)
    assert L.ellp_engine_tableau_rows(None, E._p(pos), 1, E._p(al), None, err, 512) == E.ERR_ARG
    p = _hand()
    fp = E.FlatProblem(p["m"], p["n"], p["n_c"], p["A"].T.reshape(-1), p["c"], p["b"], p["kind"], p["lb"], p["ub"], p["x"], p["B"], p["N"], p["Nb"])
    o = E.default_opts()
    # nothing wanted
    assert L.ellp_ranging(*fp._args(), C.byref(o), None, err, 512) == E.ERR_ARG
    assert L.ellp_ranging(*fp._args(), C.byref(o), C.byref(E.RangingOut()), err, 512) == E.ERR_ARG and b"nothing is wanted" in err.value
    # bad arrays: a basis of the wrong size, a null matrix, an index out of range, no rows
    args = fp._args()
    bad = list(args)
    bad[11] = 1
    assert L.ellp_ranging(*bad, C.byref(o), C.byref(rg._out()), err, 512) == E.ERR_ARG and b"invalid B/N" in err.value
    bad = list(args)
    bad[3] = None
    assert L.ellp_ranging(*bad, C.byref(o), C.byref(rg._out()), err, 512) == E.ERR_ARG
    fp2 = E.FlatProblem(p["m"], p["n"], p["n_c"], p["A"].T.reshape(-1), p["c"], p["b"], p["kind"], p["lb"], p["ub"], p["x"], [0, 9], p["N"], p["Nb"])
    assert L.ellp_ranging(*fp2._args(), C.byref(o), C.byref(rg._out()), err, 512) == E.ERR_ARG
    bad = list(args)
    bad[0] = 0
    assert L.ellp_ranging(*bad, C.byref(o), C.byref(rg._out()), err, 512) == E.ERR_ARG and b"m < 1" in err.value

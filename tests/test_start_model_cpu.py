"""The exact model of ellp_basis_start (tests/start_model.py) checked on the host: the label rule, the point of a hand-worked
basis, the verdicts with their NaN handling, the structured solver against the dense one, and the whole model against the
numpy construction at afiro's optimal basis (the optimum of the reference's own loops)."""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import start_cases as SC  # noqa: E402
import start_model as SM  # noqa: E402

NAN = float("nan")


def test_label_rule():
    for mode in (SM.KEEP_LABELS, SM.LABELS_BY_D):
        for given in (0, 1, 2):
            assert SM.label_rule(SM.FREE, given, mode, Fraction(-1)) == (SM.NB_FREE, None)
            assert SM.label_rule(SM.LOWER, given, mode, Fraction(-1)) == (SM.NB_LOWER, "lb")
            assert SM.label_rule(SM.UPPER, given, mode, Fraction(1)) == (SM.NB_UPPER, "ub")
            assert SM.label_rule(SM.FIXED, given, mode, Fraction(1)) == (SM.NB_LOWER, "lb")
    assert SM.label_rule(SM.TWOSIDED, 0, SM.KEEP_LABELS, Fraction(-1)) == (SM.NB_LOWER, "lb")
    assert SM.label_rule(SM.TWOSIDED, 1, SM.KEEP_LABELS, Fraction(1)) == (SM.NB_UPPER, "ub")
    assert SM.label_rule(SM.TWOSIDED, 2, SM.KEEP_LABELS, Fraction(1)) == (SM.NB_LOWER, "lb")  # a given Free becomes Lower
    assert SM.label_rule(SM.TWOSIDED, 1, SM.LABELS_BY_D, Fraction(0)) == (SM.NB_LOWER, "lb")  # d >= 0
    assert SM.label_rule(SM.TWOSIDED, 0, SM.LABELS_BY_D, Fraction(-1, 8)) == (SM.NB_UPPER, "ub")


def _hand():
    """2 rows, 4 columns: x0 + x1 + s0 = 4, x0 - x1 + s1 = 1; basis (x0, x1); x2 in [0, 2] boxed, s1 >= 0"""
    A = np.array([[1.0, 1.0, 1.0, 0.0], [1.0, -1.0, 0.0, 1.0]])
    c = np.array([1.0, 2.0, -3.0, 0.0])
    b = np.array([4.0, 1.0])
    kind = np.array([1, 1, 3, 1], dtype=np.uint8)
    lb, ub = np.zeros(4), np.array([np.inf, np.inf, 2.0, np.inf])
    return A, c, b, kind, lb, ub


def test_hand_worked_basis():
    A, c, b, kind, lb, ub = _hand()
    # y: y0 + y1 = 1, y0 - y1 = 2 -> (3/2, -1/2); d2 = -3 - 3/2 = -9/2, d3 = 0 - (-1/2) = 1/2
    s = SM.Start(A, c, b, kind, lb, ub, [0, 1], [2, 3], [0, 0], SM.KEEP_LABELS)
    assert s.y == [Fraction(3, 2), Fraction(-1, 2)]
    assert s.d == [0, 0, Fraction(-9, 2), Fraction(1, 2)]
    assert s.labels == [0, 0] and s.labels_changed == 0
    assert s.t == [4, 1] and s.x == [Fraction(5, 2), Fraction(3, 2), 0, 0]
    assert (s.primal_infeasibility, s.worst_primal_var, s.primal_infeasibility_sum) == (0, -1, 0)
    assert (s.dual_infeasibility, s.worst_dual_var) == (Fraction(9, 2), 2)  # Lower with d < 0
    assert s.flags(1e-10) == (1, 0) and s.far_from(1e-10) == (True, True)
    # by d the boxed variable goes to its upper bound 2: t = (2, 1), x_B = (3/2, 1/2), and the point is dual feasible
    s = SM.Start(A, c, b, kind, lb, ub, [0, 1], [2, 3], [0, 0], SM.LABELS_BY_D)
    assert s.labels == [1, 0] and s.labels_changed == 1
    assert s.t == [2, 1] and s.x == [Fraction(3, 2), Fraction(1, 2), 2, 0]
    assert s.dual_infeasibility == 0 and s.flags(1e-10) == (1, 1)
    assert s.min_twosided_d == Fraction(9, 2)
    # a right-hand side that pushes x1 below its bound: b = (1, 4) -> x_B = (5/2, -3/2) with x2 at 0
    s = SM.Start(A, c, np.array([1.0, 4.0]), kind, lb, ub, [0, 1], [2, 3], [0, 0], SM.KEEP_LABELS)
    assert (s.primal_infeasibility, s.worst_primal_var, s.primal_infeasibility_sum) == (Fraction(3, 2), 1, Fraction(3, 2))
    assert s.flags(1e-10)[0] == 0
    assert s.omega_x([2.5, -1.5, 0.0, 0.0]) == 0


def test_verdicts_in_floats_with_nan():
    assert SM.verdict(0.0, 0.0, 0.0, 1e-10) == (1, 1)
    assert SM.verdict(1e-10, 9e-11, 0.0, 1e-10) == (0, 1)          # strict: measure < eps
    assert SM.verdict(NAN, 0.0, 0.0, 1e-10) == (0, 1)              # a NaN in b, or in a basic variable's bound
    assert SM.verdict(0.0, NAN, 0.0, 1e-10) == (1, 0)              # a NaN in c
    assert SM.verdict(0.0, 0.0, NAN, 1e-10) == (1, 0)              # a NaN in c_B without any nonbasic column
    assert SM.nanmax_first([1.0, NAN, 3.0, NAN], [7, 5, 2, 3])[1] == 3 and SM.nanmax_first([0.0, 0.0], [1, 2]) == (0.0, -1)
    assert SM.nanmax_first([2.0, 2.0, 1.0], [9, 4, 1]) == (2.0, 4)
    for kind in (SM.LOWER, SM.UPPER, SM.TWOSIDED, SM.FIXED, SM.FREE):
        v = SM.violation_f64(kind, 0.0, 1.0, NAN)
        assert v != v, kind                                        # a NaN x is never hidden, not even on a Free variable
    assert SM.violation_f64(SM.TWOSIDED, NAN, 1.0, 0.5) != SM.violation_f64(SM.TWOSIDED, NAN, 1.0, 0.5)
    z = SM.violation_f64(SM.LOWER, 0.0, 1.0, 0.0)
    assert z == 0.0 and not np.signbit(z)
    assert SM.violation_f64(SM.FIXED, 2.0, 2.0, 1.5) == 0.5 and SM.violation_f64(SM.FREE, 0.0, 0.0, -9.0) == 0.0


def test_bidiagonal_solver_is_the_dense_one():
    rng = np.random.default_rng(3)
    m = 9
    perm = [int(p) for p in rng.permutation(m)]
    sub = rng.choice([1.0, 0.5, -0.5, 2.0], size=m)
    A_B, solve, solve_t = SM.bidiagonal(perm, sub)
    rhs = [Fraction(int(v), 4) for v in rng.integers(-9, 10, size=m)]
    rows = [[SM.F(A_B[i, k]) for k in range(m)] for i in range(m)]
    cols = [[SM.F(A_B[i, k]) for i in range(m)] for k in range(m)]
    assert solve(rhs) == SM.solve_dense(rows, rhs)
    assert solve_t(rhs) == SM.solve_dense(cols, rhs)


def test_against_numpy_on_afiro():
    """at the optimum of the reference's loops the exact start is that optimum: feasible both ways, x and d those of numpy to
    rounding, no label changed — and the float model of step 5 reaches omega_x <= 2u only with the singleton rows snapped"""
    v = SC.oracle_optimum(SC.netlib("afiro"))
    A = v.A_matrix()
    N, Nb = v.N[:v.nN], v.Nb[:v.nN]
    for mode in (SM.KEEP_LABELS, SM.LABELS_BY_D):
        s = SM.Start(A, v.c, v.b, v.kind, v.lb, v.ub, v.B, N, Nb, mode)
        assert s.labels == [int(k) for k in Nb] and s.labels_changed == 0
        assert s.flags(1e-10) == (1, 1) and s.far_from(1e-10) == (True, True)
        A_B = A[:, v.B]
        y = np.linalg.solve(A_B.T, v.c[v.B])
        d = v.c[:v.n] - A.T @ y
        xN = v.x[:v.n].copy()
        xN[v.B] = 0.0
        x = xN.copy()
        x[v.B] = np.linalg.solve(A_B, v.b - A @ xN)
        assert np.abs(np.array([float(q) for q in s.y]) - y).max() <= 1e-12 * max(1.0, np.abs(y).max())
        assert np.abs(np.array([float(q) for q in s.d]) - d).max() <= 1e-12 * max(1.0, np.abs(d).max())
        assert np.abs(np.array([float(q) for q in s.x]) - x).max() <= 1e-12 * max(1.0, np.abs(x).max())
        assert np.abs(np.array([float(q) for q in s.x]) - v.x[:v.n]).max() <= 1e-9 * max(1.0, np.abs(x).max())
        assert s.omega_x([float(q) for q in s.x]) <= 2 * SM.U      # the exact x rounded entry by entry
    xb, w, steps = SM.float_model_x(A[:, v.B], [float(q) for q in s.t])
    assert w <= 2 * SM.U and steps <= 4, (w / SM.U, steps)
    assert s.omega_x(x) > 0.5                                       # plain LAPACK, no snap: a backward error of one

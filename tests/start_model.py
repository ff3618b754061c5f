"""Exact model of ellp_basis_start (ellp_amd/csrc/engine/ellp_start.inc) for the tests.

Everything is rational arithmetic (fractions.Fraction) on the f64 inputs, by the definitions of include/ellp_hip.h:

    y = B^-T c_B,  d = c - A^T y                         exactly
    labels and nonbasic values                            the rule by kind; TwoSided: the given label (KEEP_LABELS, a given
                                                          Free becomes Lower) or the sign of the exact d (LABELS_BY_D: d >= 0
                                                          Lower, else Upper)
    t = b - A_N x_N,  x_B = B^-1 t                        exactly
    primal infeasibility                                  max and sum over the BASIC positions of the bound violation by kind
    dual infeasibility                                    max over the nonbasic positions by label (kind Fixed: 0)
    labels_changed                                        positions whose label differs from the one passed in

The linear solves are Gaussian elimination in Fractions (O(m^3): fine to some tens of rows) or, for a basis the caller
knows the structure of, two callables solve(rhs) -> A_B^-1 rhs and solve_t(rhs) -> A_B^-T rhs (bidiagonal() below: O(m)).

LABELS_BY_D on the device uses the sign of the COMPUTED d; it equals the model's label wherever the exact d of a TwoSided
nonbasic variable is not within rounding of zero — a condition on the test's inputs (Start.min_twosided_d).

NaN.  A Fraction cannot hold one, so the verdicts are stated apart, in floats (verdict()): a flag is `measure < eps`, which a
NaN measure fails; dual_feasible is also 0 when max |d_B| is a NaN (a NaN cost of a basic variable reaches no nonbasic
d only where there is no nonbasic column).  nanmax_first() is the maximum the kernels form: a NaN wins, at its first index.
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
FREE, LOWER, UPPER, TWOSIDED, FIXED = 0, 1, 2, 3, 4  # bound kinds
NB_LOWER, NB_UPPER, NB_FREE = 0, 1, 2                # nonbasic labels
KEEP_LABELS, LABELS_BY_D = 0, 1


def F(v):
    return Fraction(float(v))


def solve_dense(M, rhs):
    """M x = rhs in Fractions; M: list of rows of Fractions (copied).  Raises ZeroDivisionError on a singular M."""
    m = len(M)
    a = [list(row) + [rhs[i]] for i, row in enumerate(M)]
    for k in range(m):
        p = next((i for i in range(k, m) if a[i][k] != 0), None)
        if p is None:
            raise ZeroDivisionError("singular")
        a[k], a[p] = a[p], a[k]
        piv = a[k][k]
        for i in range(k + 1, m):
            if a[i][k] != 0:
                f = a[i][k] / piv
                ri, rk = a[i], a[k]
                for j in range(k, m + 1):
                    if rk[j] != 0:
                        ri[j] -= f * rk[j]
    x = [Fraction(0)] * m
    for k in range(m - 1, -1, -1):
        s = a[k][m]
        for j in range(k + 1, m):
            if a[k][j] != 0:
                s -= a[k][j] * x[j]
        x[k] = s / a[k][k]
    return x


def bidiagonal(perm, sub):
    """Solvers of A_B = P L: L unit lower bidiagonal with L[i][i-1] = sub[i] (sub[0] unused), row perm[i] of A_B = row i of L.
    Returns (A_B as an (m, m) f64 array, solve, solve_t), both solves O(m) in Fractions."""
    m = len(perm)
    L = np.eye(m)
    for i in range(1, m):
        L[i, i - 1] = sub[i]
    A_B = np.zeros((m, m))
    A_B[np.asarray(perm), :] = L
    fs = [F(s) for s in sub]

    def solve(rhs):  # P L x = rhs: (L x)_i = rhs[perm[i]]
        x = [Fraction(0)] * m
        for i in range(m):
            x[i] = rhs[perm[i]] - (fs[i] * x[i - 1] if i > 0 else 0)
        return x

    def solve_t(rhs):  # L^T (P^T y) = rhs; z = P^T y, z_i = y[perm[i]]
        z = [Fraction(0)] * m
        for i in range(m - 1, -1, -1):
            z[i] = rhs[i] - (fs[i + 1] * z[i + 1] if i + 1 < m else 0)
        y = [Fraction(0)] * m
        for i in range(m):
            y[perm[i]] = z[i]
        return y

    return A_B, solve, solve_t


def violation(kind, lb, ub, x):
    """bound violation of one variable by kind, exactly (x a Fraction; lb, ub f64)"""
    z = Fraction(0)
    if kind == LOWER:
        return max(F(lb) - x, z)
    if kind == UPPER:
        return max(x - F(ub), z)
    if kind == TWOSIDED:
        return max(F(lb) - x, x - F(ub), z)
    if kind == FIXED:
        return abs(x - F(lb))
    return z


def label_rule(kind, given, mode, d):
    """(label, which bound holds the value: 'lb', 'ub' or None for 0) of one nonbasic position"""
    if kind == FREE:
        return NB_FREE, None
    if kind == LOWER:
        return NB_LOWER, "lb"
    if kind == UPPER:
        return NB_UPPER, "ub"
    if kind == FIXED:
        return NB_LOWER, "lb"
    if mode == LABELS_BY_D:
        lab = NB_LOWER if d >= 0 else NB_UPPER
    else:
        lab = NB_UPPER if given == NB_UPPER else NB_LOWER
    return lab, "ub" if lab == NB_UPPER else "lb"


def _max_first(values, indices):
    """(max, smallest index holding it); (0, -1) when the maximum is 0"""
    best, where = Fraction(0), -1
    for v, i in sorted(zip(values, indices), key=lambda p: p[1]):
        if v > best:
            best, where = v, i
    return best, where


class Start:
    """The exact start of one basis.  A: (m, n) f64 array; c, kind, lb, ub: n entries; b: m; B, N, Nb: the index sets and the
    labels passed in; solve / solve_t: optional exact solvers of A_B (default: dense elimination)."""

    def __init__(self, A, c, b, kind, lb, ub, B, N, Nb, mode, solve=None, solve_t=None):
        self.A = A = np.asarray(A, dtype=np.float64)
        self.m, self.n = A.shape
        m = self.m
        B, N = [int(v) for v in B], [int(v) for v in N]
        self.B, self.N = B, N
        if solve is None:
            rows = [[F(A[i, v]) for v in B] for i in range(m)]
            cols = [[F(A[i, v]) for i in range(m)] for v in B]
            solve = lambda rhs: solve_dense(rows, rhs)
            solve_t = lambda rhs: solve_dense(cols, rhs)
        self.y = solve_t([F(c[v]) for v in B])
        nz = [np.nonzero(A[:, v])[0] for v in range(self.n)]
        self.d = [F(c[v]) - sum((F(A[i, v]) * self.y[i] for i in nz[v]), Fraction(0)) for v in range(self.n)]
        self.labels, self.x = [], [Fraction(0)] * self.n
        for j, v in enumerate(N):
            lab, which = label_rule(int(kind[v]), int(Nb[j]), mode, self.d[v])
            self.labels.append(lab)
            self.x[v] = F(lb[v]) if which == "lb" else (F(ub[v]) if which == "ub" else Fraction(0))
        self.labels_changed = sum(1 for j in range(len(N)) if self.labels[j] != int(Nb[j]))
        self.t = [F(b[i]) - sum((F(A[i, v]) * self.x[v] for v in N if A[i, v] != 0.0), Fraction(0)) for i in range(m)]
        xB = solve(self.t)
        for i, v in enumerate(B):
            self.x[v] = xB[i]
        viol = [violation(int(kind[v]), lb[v], ub[v], self.x[v]) for v in B]
        self.primal_infeasibility, self.worst_primal_var = _max_first(viol, B)
        self.primal_infeasibility_sum = sum(viol, Fraction(0))
        inf = []
        for j, v in enumerate(N):
            dv = self.d[v]
            if int(kind[v]) == FIXED:
                inf.append(Fraction(0))
            elif self.labels[j] == NB_LOWER:
                inf.append(max(-dv, Fraction(0)))
            elif self.labels[j] == NB_UPPER:
                inf.append(max(dv, Fraction(0)))
            else:
                inf.append(abs(dv))
        self.dual_infeasibility, self.worst_dual_var = _max_first(inf, N)
        two = [abs(self.d[v]) for v in N if int(kind[v]) == TWOSIDED]
        self.min_twosided_d = min(two) if two else None

    def omega_x(self, x, t=None):
        """omega of a given f64 x_B (by variable) for the exact t (or a given one): max_i |t - A_B x_B|_i / (|t| + |A_B||x_B|)_i"""
        t = self.t if t is None else t
        w = Fraction(0)
        for i in range(self.m):
            s = sum((F(self.A[i, v]) * F(x[v]) for v in self.B if self.A[i, v] != 0.0), Fraction(0))
            den = abs(t[i]) + sum((abs(F(self.A[i, v]) * F(x[v])) for v in self.B if self.A[i, v] != 0.0), Fraction(0))
            if t[i] - s != 0:
                w = max(w, abs(t[i] - s) / den)
        return w

    def far_from(self, eps, factor=1000):
        """(primal, dual): whether each exact measure lies at least `factor` on either side of eps — the condition under
        which the device's flag must equal the model's"""
        def far(v):
            return v * factor <= F(eps) or v >= F(eps) * factor
        return far(self.primal_infeasibility), far(self.dual_infeasibility)

    def flags(self, eps):
        return int(self.primal_infeasibility < F(eps)), int(self.dual_infeasibility < F(eps))


def nanmax_first(values, indices):
    """the kernels' maximum in floats: a NaN wins (its smallest index), else the largest value at its smallest index; (0.0, -1)
    when the maximum is 0"""
    best, where = 0.0, -1
    for v, i in sorted(zip((float(v) for v in values), (int(i) for i in indices)), key=lambda p: p[1]):
        if v != v:
            return v, i
        if v > best:
            best, where = v, i
    return best, where


def violation_f64(kind, lb, ub, x):
    """k_start_verdict's violation of one variable in f64 (max(v, 0) keeps a NaN and never gives -0.0)"""
    def pos(v):
        return v if v != v else (v if v > 0.0 else 0.0)
    if kind == LOWER:
        return pos(lb - x)
    if kind == UPPER:
        return pos(x - ub)
    if kind == TWOSIDED:
        a, b = lb - x, x - ub
        return pos(a if a != a else (b if (b > a or b != b) else a))
    if kind == FIXED:
        return abs(x - lb)
    return x if x != x else 0.0


def verdict(primal_infeasibility, dual_infeasibility, basic_reduced_cost, eps):
    """(primal_feasible, dual_feasible) from f64 measures, NaN included: a NaN is never feasible"""
    pf = 1 if primal_infeasibility < eps else 0
    df = 1 if (dual_infeasibility < eps and basic_reduced_cost == basic_reduced_cost) else 0
    return pf, df


def float_model_x(A_B, t):
    """Step 5 in f64 with exact residuals rounded once, as postsolve_model.float_model does for y: x_B = A_B^-1 t by numpy's
    LU, rows of A_B with a single nonzero a at position k snapped to x_k = fl(t_i / a) after the solve and after every step,
    refinement while omega_x > 2u, fewer than 4 steps were taken and the last step at least halved it.  Returns
    (x_B, omega_x as a float, steps): what the algorithm reaches when the residual is as good as the compensated pass makes it."""
    A_B = np.asarray(A_B, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    m = A_B.shape[0]

    def residual(x):
        res, w = np.zeros(m), Fraction(0)
        for i in range(m):
            nz = np.nonzero(A_B[i, :])[0]
            s = sum((F(A_B[i, k]) * F(x[k]) for k in nz), Fraction(0))
            den = abs(F(t[i])) + sum((abs(F(A_B[i, k]) * F(x[k])) for k in nz), Fraction(0))
            res[i] = float(F(t[i]) - s)
            if F(t[i]) - s != 0:
                w = max(w, abs(F(t[i]) - s) / den)
        return res, float(w)

    def snap(x):
        for i in range(m):
            nz = np.nonzero(A_B[i, :])[0]
            if len(nz) == 1:
                x[nz[0]] = t[i] / A_B[i, nz[0]]
        return x

    x = snap(np.linalg.solve(A_B, t))
    steps, last = 0, 0.0
    while True:
        res, w = residual(x)
        if not (w > 2 * U) or steps >= 4 or (steps > 0 and not (w <= 0.5 * last)):
            return x, w, steps
        x = snap(x + np.linalg.solve(A_B, res))
        last = w
        steps += 1

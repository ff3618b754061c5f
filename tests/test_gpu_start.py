"""ellp_basis_start on the device against the exact model of tests/start_model.py.

Shapes, the smallest at which each piece can go wrong: m = 1 (n = 2); m = 3 (small_prob_1 at its optimal and at its slack
basis); m = 17 with 3 nonbasic columns (ld = 32 padding, fewer columns than one block); m = 27 (afiro, both modes); m = 513
with 40 nonbasic columns (two row tiles of the pass, three chunks of |A_B||x_B|; A_B a row-permuted unit lower bidiagonal
matrix, so that the exact solves are O(m) in Fractions).

What is asserted, and with which tolerance (u = 2^-53; no factor on any bound):
  labels, labels_changed     equal to the model's (for TwoSided variables in LABELS_BY_D the test first asserts, from the model,
                             that their exact |d| is above 1e-6: the sign of the computed d is then the exact one)
  d                          every entry within  u |exact| + gamma_K^2 S  of the exact d of the RETURNED y (postsolve_model's
                             bound and chain length K_d)
  t                          is not an output.  It is checked through what is made of it: kkt.primal_residual against the exact
                             max_i |b - A x|_i of the returned x within the bound of r (chain K_r), and omega_x below
  omega_y                    reported <= 2u, and within  omega (3u + 2 gamma_{K_d+1}) + 2 gamma_{K_d}^2  of the exact omega of
                             the returned y (tests/test_gpu_postsolve.py's tolerance)
  omega_x                    reported <= 2u, and within  omega (3u + 2 gamma_{m+1}) + 2 gamma_{K_r}^2 + u  of the exact omega_x of
                             the returned x for the EXACT t: the numerator carries the entry bound of the pass, the denominator
                             is a plain sum of at most m + 1 rounded non-negative terms, the quotient one rounding, and the
                             device's t is the exact t rounded once (a change of the residual by at most u |t_i|, of omega by u)
  measures, worst indices    bit for bit the definitions of include/ellp_hip.h applied in f64 to the returned x and d (max, abs
                             and one subtraction are exact or correctly rounded on both sides); the sum within
                             u |sum| + gamma_K^2 |sum|, K = ceil(m / 1024) + 10 + 1
  measures against the model |x_dev - x_exact| <= |A_B^-1| |t - A_B x_dev| <= |A_B^-1| omega_x (|t| + |A_B||x_dev|) holds exactly, so
                             with omega_x <= 4u (above) the basic values, and with them the 1-Lipschitz violations, lie within
                             tol_x = 2 max_i (|A_B^-1| 4u (|t| + |A_B||x_exact|))_i of the model's (|A_B^-1| from numpy, the
                             factor 2 covers its rounding and x_dev in place of x_exact); the same with A_B^T, c_B, y for the
                             duals, and tol_d = max_v |a_v| . tol_y + the entry bound for the reduced costs
  flags                      equal to the model's wherever the model's exact measure lies a factor 1000 on either side of eps
                             (asserted from the model, on the CPU, for every case)
  two calls                  the same bits in every output

Met on an MI355X (records, not limits): omega_y 0 to 0.48 u with 0 or 1 steps; omega_x 0 to 1.83 u (afiro, 0 steps after the
snap of its singleton row; 0.27 u after 1 step at 17 rows); d: largest |got - exact| / bound 0.75; every measure equal to
the model's to all printed digits.
"""
import ctypes as C
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402
import postsolve_model as PM  # noqa: E402
import start_cases as SC  # noqa: E402
import start_model as SM  # noqa: E402

pytestmark = pytest.mark.gpu
U = SM.U
EPS = 1e-10


def _E():
    from ellp_amd import _engine as E
    return E


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _fp(c):
    E = _E()
    return E.FlatProblem(c["m"], c["n"], c["n"], np.asarray(c["A"]).reshape(-1, order="F"), c["c"], c["b"], c["kind"], c["lb"], c["ub"],
                         np.zeros(c["n"]), c["B"], c["N"], c["Nb"])


def _case_of_view(v, B=None, N=None, Nb=None):
    return dict(m=v.m, n=v.n, A=v.A_matrix(), c=v.c[:v.n], b=v.b, kind=v.kind[:v.n], lb=v.lb[:v.n], ub=v.ub[:v.n],
                B=v.B if B is None else np.asarray(B, dtype=np.int64), N=v.N[:v.nN] if N is None else np.asarray(N, dtype=np.int64),
                Nb=v.Nb[:v.nN] if Nb is None else np.asarray(Nb, dtype=np.uint8))


def _known(name):
    return next(f for f in helpers.known_answers()["problems"] if f["name"] == name)


def _one_row():
    return dict(m=1, n=2, A=np.array([[2.0, 1.0]]), c=np.array([1.0, 3.0]), b=np.array([3.0]), kind=np.array([1, 3], dtype=np.uint8),
                lb=np.array([0.0, 0.5]), ub=np.array([np.inf, 1.0]), B=np.array([0]), N=np.array([1]), Nb=np.array([1], dtype=np.uint8))


def _small_optimal():
    return _case_of_view(SC.oracle_optimum(_known("small_prob_1")))


def _small_slack():
    v = SC.oracle_optimum(_known("small_prob_1"))
    nv = v.n - v.m  # the slacks are the last m columns
    return _case_of_view(v, B=np.arange(nv, v.n), N=np.arange(nv), Nb=np.zeros(nv, dtype=np.uint8))


def _seventeen():
    rng = np.random.default_rng(20260517)
    m, nN = 17, 3
    n = m + nN
    A = np.round(rng.normal(size=(m, n)) * 8) / 8
    A[rng.random(size=(m, n)) < 0.4] = 0.0
    A[np.arange(m), nN + np.arange(m)] += 4.0
    kind = np.array([3, 0, 2] + [1, 3, 0, 2, 4] * 3 + [1, 1], dtype=np.uint8)
    lb = -np.round(rng.uniform(0, 2, size=n) * 8) / 8
    ub = np.where(kind == 4, lb, lb + 1.0 + np.round(rng.uniform(0, 2, size=n) * 8) / 8)
    return dict(m=m, n=n, A=A, c=np.round(rng.normal(size=n) * 16) / 16, b=np.round(rng.normal(size=m) * 16) / 16, kind=kind, lb=lb, ub=ub,
                B=np.arange(nN, n), N=np.arange(nN), Nb=np.array([2, 1, 0], dtype=np.uint8))


def _afiro():
    return _case_of_view(SC.oracle_optimum(SC.netlib("afiro")))


_BIDIAG = {}


def _bidiag():
    if not _BIDIAG:
        _BIDIAG["case"], _BIDIAG["perm"], _BIDIAG["sub"] = SC.bidiagonal_case()
    return _BIDIAG["case"]


CASES = {
    "1x2-keep": (_one_row, 0), "1x2-by-d": (_one_row, 1),
    "small_prob_1-optimal-keep": (_small_optimal, 0), "small_prob_1-optimal-by-d": (_small_optimal, 1),
    "small_prob_1-slack-keep": (_small_slack, 0), "small_prob_1-slack-by-d": (_small_slack, 1),
    "17x20-keep": (_seventeen, 0), "17x20-by-d": (_seventeen, 1),
    "afiro-keep": (_afiro, 0), "afiro-by-d": (_afiro, 1),
    "513x553-keep": (_bidiag, 0), "513x553-by-d": (_bidiag, 1),
}


def _model(name, c, mode):
    if name.startswith("513"):
        _, solve, solve_t = SM.bidiagonal(_BIDIAG["perm"], _BIDIAG["sub"])
        return SM.Start(c["A"], c["c"], c["b"], c["kind"], c["lb"], c["ub"], c["B"], c["N"], c["Nb"], mode, solve=solve, solve_t=solve_t)
    return SM.Start(c["A"], c["c"], c["b"], c["kind"], c["lb"], c["ub"], c["B"], c["N"], c["Nb"], mode)


@pytest.mark.parametrize("name", list(CASES))
def test_against_exact_model(name):
    E = _E()
    make, mode = CASES[name]
    c = make()
    m, n = c["m"], c["n"]
    A, B, N = c["A"], [int(v) for v in c["B"]], [int(v) for v in c["N"]]
    fp = _fp(c)
    mod = _model(name, c, mode)
    # conditions on the inputs, from the model alone
    if mode == 1 and mod.min_twosided_d is not None:
        assert mod.min_twosided_d > Fraction(1, 10 ** 6), (name, float(mod.min_twosided_d))
    far_p, far_d = mod.far_from(EPS)
    assert far_p and far_d, (name, float(mod.primal_infeasibility), float(mod.dual_infeasibility))
    s, x, y, d, Nb, info = E.basis_start(fp, mode)
    assert s == E.OPTIMAL, info
    s2, x2, y2, d2, Nb2, info2 = E.basis_start(fp, mode)
    assert s2 == E.OPTIMAL
    for a, b in ((x, x2), (y, y2), (d, d2)):
        assert (_bits(a) == _bits(b)).all(), name
    assert (Nb == Nb2).all()
    for k, v in info.items():
        if k == "kkt":
            for kk, vv in v.items():
                assert _bits([vv])[0] == _bits([info2["kkt"][kk]])[0] if isinstance(vv, float) else vv == info2["kkt"][kk], (name, kk)
        elif isinstance(v, float):
            assert _bits([v])[0] == _bits([info2[k]])[0], (name, k)
        else:
            assert v == info2[k], (name, k)
    kkt = info["kkt"]
    # labels
    assert [int(k) for k in Nb] == mod.labels, name
    assert info["labels_changed"] == mod.labels_changed, name
    for j, v in enumerate(N):
        assert x[v] == float(mod.x[v]), (name, "x_N", v)  # a bound, or 0
    # omega as reported
    assert kkt["y_backward_error"] <= 2 * U and info["x_backward_error"] <= 2 * U, (name, kkt["y_backward_error"] / U, info["x_backward_error"] / U)
    assert 0 <= kkt["refinement_steps"] <= 4 and 0 <= info["x_refinement_steps"] <= 4
    # d and r of the returned point within the postsolve's bound
    fp.x, fp.Nb = x.copy(), Nb.copy()
    ex = PM.Exact.of(fp, y)
    kd, kr = PM.chain_lengths(m, len(N))
    big_d, big_r, worst = Fraction(0), Fraction(0), 0.0
    d_exact = []
    for v in range(n):
        e, S = ex.d(v)
        bound = PM.entry_bound(e, S, kd)
        big_d = max(big_d, bound)
        d_exact.append(e)
        err = abs(Fraction(float(d[v])) - e)
        assert err <= bound, (name, "d", v, float(err), float(bound))
        worst = max(worst, float(err / bound)) if bound else worst
    r_max = Fraction(0)
    for i in range(m):
        e, S = ex.r(i)
        big_r = max(big_r, PM.entry_bound(e, S, kr))
        r_max = max(r_max, abs(e))
    assert abs(Fraction(kkt["primal_residual"]) - r_max) <= big_r, (name, kkt["primal_residual"], float(r_max))
    # omega_y and omega_x recomputed
    w = ex.omega()
    g1, g0 = Fraction(PM.gamma(kd + 1)), Fraction(PM.gamma(kd))
    assert abs(Fraction(kkt["y_backward_error"]) - w) <= w * (3 * Fraction(U) + 2 * g1) + 2 * g0 * g0, (name, kkt["y_backward_error"], float(w))
    wx = mod.omega_x(x)
    gm, gr = Fraction(PM.gamma(m + 1)), Fraction(PM.gamma(kr))
    tol_w = wx * (3 * Fraction(U) + 2 * gm) + 2 * gr * gr + Fraction(U)
    print(f"{name}: omega_y {kkt['y_backward_error'] / U:.3f} u ({kkt['refinement_steps']} steps), omega_x {info['x_backward_error'] / U:.3f} u "
          f"({info['x_refinement_steps']} steps; exact {float(wx) / U:.3f} u), d: max err / bound {worst:.3f}, primal infeasibility "
          f"{info['primal_infeasibility']:.3e} (model {float(mod.primal_infeasibility):.3e}), dual {info['dual_infeasibility']:.3e} "
          f"(model {float(mod.dual_infeasibility):.3e}), labels changed {info['labels_changed']}")
    assert abs(Fraction(info["x_backward_error"]) - wx) <= tol_w, (name, info["x_backward_error"] / U, float(wx) / U)
    # the measures: the definitions on the returned arrays, bit for bit
    viol = [SM.violation_f64(int(c["kind"][v]), float(c["lb"][v]), float(c["ub"][v]), float(x[v])) for v in B]
    pinf, wp = SM.nanmax_first(viol, B)
    assert _bits([info["primal_infeasibility"]])[0] == _bits([pinf])[0] and info["worst_primal_var"] == wp, (name, info, pinf, wp)
    rep = PM.report_from(fp, d, np.zeros(m))
    assert _bits([info["dual_infeasibility"]])[0] == _bits([rep["dual_infeasibility"]])[0], name
    assert info["worst_dual_var"] == rep["worst_dual_var"] == kkt["worst_dual_var"], name
    assert _bits([kkt["bound_violation"]])[0] == _bits([rep["bound_violation"]])[0], name
    psum = sum((Fraction(v) for v in viol), Fraction(0))
    gs = Fraction(PM.gamma((m + 1023) // 1024 + 11))
    assert abs(Fraction(info["primal_infeasibility_sum"]) - psum) <= (Fraction(U) + gs * gs) * psum, (name, info["primal_infeasibility_sum"])
    # ... and against the model's
    A_B = A[:, B]
    inv = np.abs(np.linalg.inv(A_B))
    t_abs = np.array([float(abs(q)) for q in mod.t])
    xB_abs = np.array([float(abs(mod.x[v])) for v in B])
    tol_x = 2.0 * float((inv @ (4 * U * (t_abs + np.abs(A_B) @ xB_abs))).max())
    assert abs(info["primal_infeasibility"] - float(mod.primal_infeasibility)) <= tol_x + U * float(mod.primal_infeasibility), (name, tol_x)
    assert abs(info["primal_infeasibility_sum"] - float(mod.primal_infeasibility_sum)) <= m * tol_x + 2 * U * float(mod.primal_infeasibility_sum), name
    y_abs = np.array([float(abs(q)) for q in mod.y])
    tol_y = 2.0 * (inv.T @ (4 * U * (np.abs(c["c"][B]) + np.abs(A_B).T @ y_abs)))
    tol_d = float((np.abs(A).T @ tol_y).max()) + float(big_d)
    assert abs(info["dual_infeasibility"] - float(mod.dual_infeasibility)) <= tol_d + U * float(mod.dual_infeasibility), (name, tol_d)
    assert (info["primal_feasible"], info["dual_feasible"]) == mod.flags(EPS), (name, info, mod.flags(EPS))


def _raw(c, mode, sentinel=-7.0):
    """the C call with sentinel-filled outputs"""
    E = _E()
    fp = _fp(c)
    x, y, d = np.full(c["n"], sentinel), np.full(c["m"], sentinel), np.full(c["n"], sentinel)
    Nb = np.ascontiguousarray(c["Nb"], dtype=np.uint8).copy()
    info = E.StartInfo()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    err = C.create_string_buffer(512)
    s = E.lib().ellp_basis_start(fp.m, fp.n, p(fp.A), p(fp.c), p(fp.b), p(fp.kind), p(fp.lb), p(fp.ub), p(fp.B), fp.nB, p(fp.N), p(Nb), fp.nN,
                                 mode, None, p(x), p(y), p(d), C.byref(info), err, 512)
    return s, x, y, d, Nb, info, err.value.decode()


@pytest.mark.parametrize("mode", [0, 1])
def test_singular_basis_leaves_the_outputs_untouched(mode):
    E = _E()
    c = _seventeen()
    # two proportional columns.  The factor is a power of two: scaling by it commutes with every rounding, so the elimination
    # meets an exact zero pivot, which is what ELLP_ERR_SINGULAR reports (a factor like 2.5 leaves a pivot of rounding size,
    # a basis that is numerically singular but not refused)
    c["A"][:, c["B"][5]] = 2.0 * c["A"][:, c["B"][2]]
    c["Nb"] = np.array([2, 2, 2], dtype=np.uint8)        # labels the repair would change
    s, x, y, d, Nb, info, msg = _raw(c, mode)
    assert s == E.ERR_SINGULAR and msg
    assert (x == -7.0).all() and (y == -7.0).all() and (d == -7.0).all() and Nb.tolist() == [2, 2, 2]
    assert info.labels_changed == 0 and info.primal_feasible == 0 and info.dual_feasible == 0


def test_nan_is_never_feasible():
    E = _E()
    base = _small_optimal()
    s, *_, info = E.basis_start(_fp(base), 0)
    assert s == E.OPTIMAL and (info["primal_feasible"], info["dual_feasible"]) == (1, 1)
    for mode in (0, 1):
        c = dict(base, b=base["b"].copy())
        c["b"][1] = np.nan
        s, x, y, d, Nb, info = E.basis_start(_fp(c), mode)
        assert s == E.OPTIMAL and info["primal_feasible"] == 0 and info["primal_infeasibility"] != info["primal_infeasibility"], info
        for v in (int(base["B"][0]), int(base["N"][0])):  # a basic and a nonbasic cost
            c = dict(base, c=base["c"].copy())
            c["c"][v] = np.nan
            s, x, y, d, Nb, info = E.basis_start(_fp(c), mode)
            assert s == E.OPTIMAL and info["dual_feasible"] == 0, (mode, v, info)
        # the bound of a basic variable
        v = int(base["B"][0])
        c = dict(base, lb=base["lb"].copy(), ub=base["ub"].copy())
        c["lb"][v] = c["ub"][v] = np.nan
        s, x, y, d, Nb, info = E.basis_start(_fp(c), mode)
        assert s == E.OPTIMAL and (info["primal_feasible"] == 0 or int(base["kind"][v]) == 0), (mode, info)


def test_labels_by_d_moves_a_boxed_variable_to_its_upper_bound():
    """the hand-worked basis of tests/test_start_model_cpu.py: x2 in [0, 2] nonbasic with d = -9/2"""
    E = _E()
    c = dict(m=2, n=4, A=np.array([[1.0, 1.0, 1.0, 0.0], [1.0, -1.0, 0.0, 1.0]]), c=np.array([1.0, 2.0, -3.0, 0.0]), b=np.array([4.0, 1.0]),
             kind=np.array([1, 1, 3, 1], dtype=np.uint8), lb=np.zeros(4), ub=np.array([np.inf, np.inf, 2.0, np.inf]), B=np.array([0, 1]),
             N=np.array([2, 3]), Nb=np.array([0, 0], dtype=np.uint8))
    s, x, y, d, Nb, info = E.basis_start(_fp(c), E.START_KEEP_LABELS)
    assert s == E.OPTIMAL and Nb.tolist() == [0, 0] and x.tolist() == [2.5, 1.5, 0.0, 0.0] and info["labels_changed"] == 0
    assert d[2] == -4.5 and info["dual_infeasibility"] == 4.5 and info["worst_dual_var"] == 2 and info["dual_feasible"] == 0
    s, x, y, d, Nb, info = E.basis_start(_fp(c), E.START_LABELS_BY_D)
    assert s == E.OPTIMAL and Nb.tolist() == [1, 0] and x.tolist() == [1.5, 0.5, 2.0, 0.0] and info["labels_changed"] == 1
    assert y.tolist() == [1.5, -0.5] and d.tolist() == [0.0, 0.0, -4.5, 0.5]
    assert (info["dual_infeasibility"], info["worst_dual_var"], info["dual_feasible"], info["primal_feasible"]) == (0.0, -1, 1, 1)

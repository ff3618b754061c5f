"""ellp_engine_ranging / ellp_ranging / ellp_engine_tableau_rows on the device against tests/ranging_model.py.

BY DEFINITION, bit for bit: every limit and blocking index equals the f64 model applied to the returned d, all tableau rows
from tableau_rows, the returned rows of W and the point read afterwards; two calls on one state return the same bits;
inverse_residual equals, bit for bit, the NaN-propagating maximum of |I - A_B W| as the model forms it from the returned W
(the device sums every entry in ascending k with separately rounded products, k_range_resid: the bit-for-bit form of the
check, not the any-order bound).

THE GEMM: |alpha_ij - rho_i . a_j| <= gamma_m sum_k |rho_ik| |a_kj| with the exact dot product of the RETURNED rho_i and the
stored column, gamma_m = m u / (1 - m u), no slack factor; every entry up to 200 rows, above that 16 rows x 64 columns drawn
with a seed, the last row and the last column always among them.

W: for the same rows the exact residual e_i - A_B^T rho_i and its componentwise backward error
max_k |res_k| / (|e_i| + |A_B|^T |rho_i|)_k, against 4 x the worst such error of numpy.linalg.solve (LAPACK) on the same
systems (the pivot orders of the two LUs differ).  LAPACK's raw rows are no yardstick here: where a basic column has a single
nonzero, a e_k, its equation reads a rho_k = delta_ij, and a computed 1e-17 where rho_k is exactly 0 is an error of 1 — which
LAPACK shows at six of the seven shapes, and against which any W, W = 0 included, would pass.  So the reference rows get the
entries those columns fix (what k_range_snap does on the device) before they are measured, and their figure is in units of
u.  test_the_backward_error_measure_can_fail holds the measure itself to that: W = 0 and a W wrong by 1e-3 in one entry fail.

MEANING, at 17 x 30 and 50 x 120 at the optimum, in exact arithmetic with the exact inverse (ranging_model.ExactRanging):
inside a finite limit L (delta = L (1 - 2^-20)) every non-Fixed nonbasic reduced cost keeps the sign its label demands and
every basic variable its bounds; outside (delta = L (1 + 2^-20)) the blocking one has lost it; L = 0 asserts the blocker's
side only.  Left out: entries with 0 < |alpha| or |w| <= 2 eps, asserted to be at most 1 % of the entries.  Entries that are
exactly zero are not left out — check_cost_limit and check_rhs_limit evaluate them like any other (they move nothing, so they
hold trivially), and a blocker on one fails the check: at 17 x 30 the end basis keeps slack
columns, 80 of 799 tableau entries are exact zeros, none is a nonzero below 2 eps (the same at 50 x 120: 0 of 8,500).

Ranging is called straight after run(40), before any read_point: on the pipeline = 2 engines the slice leaves its last
iteration open and the call must complete it.

Met on an MI355X (records, not limits): largest |alpha - exact| / bound 0.112 (dual 20 x 50), 0.035 (50 x 120), 0.013
(200 x 500), 0.0035 / 0.0027 / 0.0032 (the sampled shapes).  Componentwise backward error, rows of W / reference
(numpy.linalg.solve with the singleton entries imposed): 2.84 / 2.63 u (17 x 30), 2.61 / 3.72 u (50 x 120), 4.93 / 9.33 u
(200 x 500), 6.13 / 8.27 u (600 x 1500), 4.91 / 5.42 u (1040 x 1300), 1.93 / 0.82 u (dual 20 x 50), 4.88 / 2.58 u (dual 600),
4.99 / 6.51 u (2050 x 2100, R = 2).  Without the imposed entries numpy.linalg.solve's figure is 1 (= 2^53 u) on every shape
but the 20 x 50 dual, and so was the device's before k_range_snap.  inverse_residual 1.2e-15 to 7.2e-15.
"""
import os
import sys
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ranging_model as RM  # noqa: E402
from test_gpu_postsolve import CASES, _E, _bits, _engine, _primal_fp  # noqa: E402  (the engines are made as there)

pytestmark = pytest.mark.gpu
U = 2.0 ** -53

ARR = ("cost_down", "cost_up", "cost_blocking_down", "cost_blocking_up", "rhs_down", "rhs_up", "rhs_blocking_down", "rhs_blocking_up", "d")


def _same(a, b):
    """bit for bit, any NaN equal to any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return bool((a == b).all())
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (_bits(np.where(na, 0.0, a)) == _bits(np.where(nb, 0.0, b))).all())


def _same_ranging(a, b):
    return all(_same(getattr(a, k), getattr(b, k)) for k in ARR) and _same([a.inverse_residual], [b.inverse_residual])


def _mat(fp):
    return fp.A.reshape(fp.n, fp.m).T


@lru_cache(maxsize=None)
def _case(name, to_optimal=False):
    """one engine per case: run, ranging (before any read_point), the point, ranging again, all tableau rows and W"""
    E = _E()
    eng, fp = _engine(name)
    try:
        s, st, msg = eng.run(100000 if to_optimal else 40)
        if to_optimal:
            assert s == E.OPTIMAL, (s, msg)
        rg = eng.ranging()
        assert eng.closing_status == E.OPTIMAL
        eng.read_point()
        assert eng.closing_status == E.OPTIMAL
        rg2 = eng.ranging()
        alpha, W = eng.tableau_rows(np.arange(fp.m))
        eps = E.default_opts().eps
    finally:
        eng.close()
    return fp, rg, rg2, alpha, W, eps


def _check_definition(fp, rg, alpha, W, eps, label):
    N, Nb = fp.N[:fp.nN], fp.Nb[:fp.nN]
    cost = RM.cost_ranging_f64(alpha, rg.d, fp.B, N, Nb, fp.kind, fp.n, fp.n_c, eps)
    rhs = RM.rhs_ranging_f64(W, fp.x, fp.B, fp.kind, fp.lb, fp.ub, eps)
    for got, want, what in zip((rg.cost_down, rg.cost_up, rg.cost_blocking_down, rg.cost_blocking_up), cost, ARR[:4]):
        bad = [v for v in range(fp.n_c) if not _same(got[v:v + 1], want[v:v + 1])]
        assert not bad, (label, what, bad[:5], got[bad[:5]], want[bad[:5]])
    for got, want, what in zip((rg.rhs_down, rg.rhs_up, rg.rhs_blocking_down, rg.rhs_blocking_up), rhs, ARR[4:8]):
        bad = [k for k in range(fp.m) if not _same(got[k:k + 1], want[k:k + 1])]
        assert not bad, (label, what, bad[:5], got[bad[:5]], want[bad[:5]])
    assert (rg.cost_down <= 0).all() and (rg.cost_up >= 0).all() and (rg.rhs_down <= 0).all() and (rg.rhs_up >= 0).all()
    fin = np.isfinite(rg.cost_up[fp.B])
    print(f"{label}: {int(fin.sum())} of {fp.m} basic costs limited above, {int(np.isfinite(rg.rhs_up).sum())} of {fp.m} rhs limited above; "
          f"inverse_residual {rg.inverse_residual:.3e}")


@pytest.mark.parametrize("name", list(CASES))
def test_by_definition(name):
    fp, rg, rg2, alpha, W, eps = _case(name)
    assert _same_ranging(rg, rg2), name  # completing an iteration twice completes it once: the same bits
    _check_definition(fp, rg, alpha, W, eps, name)
    want = RM.inverse_residual_f64(_mat(fp)[:, fp.B], W)
    assert _same([rg.inverse_residual], [want]), (name, rg.inverse_residual, want)
    assert rg.kkt["y_backward_error"] <= 2 * U


@pytest.mark.parametrize("name", ["primal-17x30-small", "primal-50x120"])
def test_by_definition_at_the_optimum(name):
    fp, rg, rg2, alpha, W, eps = _case(name, True)
    assert _same_ranging(rg, rg2), name
    _check_definition(fp, rg, alpha, W, eps, name + "-optimal")


def _sample(fp, name):
    """(rows, columns) the exact checks look at"""
    if fp.m <= 200:
        return np.arange(fp.m), np.arange(fp.nN)
    rng = np.random.default_rng(7)
    rows = np.sort(np.unique(np.concatenate([rng.choice(fp.m - 1, 15, replace=False), [fp.m - 1]])))
    cols = np.sort(np.unique(np.concatenate([rng.choice(fp.nN - 1, 63, replace=False), [fp.nN - 1]])))
    return rows, cols


@pytest.mark.parametrize("name", list(CASES))
def test_tableau_entries_within_the_any_order_bound(name):
    fp, rg, rg2, alpha, W, eps = _case(name)
    rows, cols = _sample(fp, name)
    A_N = _mat(fp)[:, fp.N[:fp.nN]][:, cols]
    Wz, we = RM.int_matrix(W[rows])
    Az, ae = RM.int_matrix(A_N)
    exact = Wz.dot(Az)                      # integers over 2^-(we + ae)
    S = np.abs(Wz).dot(np.abs(Az))
    scale = Fraction(2) ** (we + ae)
    g = Fraction(fp.m * U) / (1 - Fraction(fp.m * U))
    worst = 0.0
    for a, i in enumerate(rows):
        for b, j in enumerate(cols):
            err = abs(Fraction(float(alpha[i, j])) - exact[a, b] * scale)
            bound = g * S[a, b] * scale
            assert err <= bound, (name, int(i), int(j), float(err), float(bound))
            if bound:
                worst = max(worst, float(err / bound))
    print(f"{name}: {len(rows)} x {len(cols)} tableau entries, largest |alpha - exact| / bound = {worst:.4f}")


def _backward_errors(A_B, rhos, rows):
    """the componentwise backward error of every rho (a solution of A_B^T rho = e_i, i in rows), exactly"""
    Az, ae = RM.int_matrix(A_B)
    Rz, re_ = RM.int_matrix(rhos)
    prod = Rz.dot(Az)                       # row a: (A_B^T rho_a)^T over 2^-(ae + re_)
    den = np.abs(Rz).dot(np.abs(Az))
    scale = Fraction(2) ** (ae + re_)
    out = []
    for a, i in enumerate(rows):
        w = Fraction(0)
        for k in range(A_B.shape[0]):
            res = (1 if k == i else 0) - prod[a, k] * scale
            if res != 0:
                w = max(w, abs(res) / ((1 if k == i else 0) + den[a, k] * scale))
        out.append(w)
    return out


def _worst_place(A_B, rhos, rows):
    """where the largest backward error sits: (row of W, component, nonzeros of that column of A_B) — for the log"""
    errs = _backward_errors(A_B, rhos, rows)
    a = max(range(len(rows)), key=lambda t: errs[t])
    res = np.abs((np.arange(A_B.shape[0]) == rows[a]) - rhos[a] @ A_B)
    k = int(np.argmax(res / ((np.arange(A_B.shape[0]) == rows[a]) + np.abs(rhos[a]) @ np.abs(A_B) + 1e-300)))
    return int(rows[a]), k, int(np.count_nonzero(A_B[:, k]))


def _lapack_rows(A_B, rows):
    """the rows of the inverse by numpy.linalg.solve, with the entries imposed that a basic column with a single nonzero fixes
    on its own (column j = a e_k: rho_i[k] = 1 / a for i = j, exactly 0 otherwise), as k_range_snap imposes them on the device"""
    m = A_B.shape[0]
    rhs = np.zeros((m, len(rows)))
    rhs[rows, np.arange(len(rows))] = 1.0
    R = np.linalg.solve(A_B.T, rhs).T
    snapped = 0
    for j in range(m):
        nz = np.nonzero(A_B[:, j])[0]
        if len(nz) == 1:
            k = nz[0]
            R[:, k] = np.where(rows == j, 1.0 / A_B[k, j], 0.0)
            snapped += 1
    return R, snapped


@pytest.mark.parametrize("name", list(CASES))
def test_rows_of_the_inverse_against_lapack(name):
    fp, rg, rg2, alpha, W, eps = _case(name)
    rows, _ = _sample(fp, name)
    A_B = _mat(fp)[:, fp.B]
    ours = max(_backward_errors(A_B, W[rows], rows))
    R, snapped = _lapack_rows(A_B, rows)
    ref = max(_backward_errors(A_B, R, rows))
    print(f"{name}: {snapped} singleton basic columns imposed on the reference rows")
    assert ref <= 64 * U, (name, "the reference is no yardstick", float(ref) / U)  # in units of u, or 4 x it binds nothing
    print(f"{name}: backward error of the rows of W {float(ours) / U:.3f} u, of numpy.linalg.solve {float(ref) / U:.3f} u ({len(rows)} rows); "
          f"worst (row, component, nonzeros of its column): {_worst_place(A_B, W[rows], rows)}")
    assert ours <= 4 * ref, (name, float(ours) / U, float(ref) / U)


@pytest.mark.parametrize("name", ["primal-200x500-hybrid", "primal-1040x1300"])
def test_the_backward_error_measure_can_fail(name):
    """what the check above would let through: nothing of this size.  W = 0, and the returned W with one entry of a sampled row
    off by 1e-3 of the row's largest, both miss 4 x the reference by orders of magnitude."""
    fp, rg, rg2, alpha, W, eps = _case(name)
    rows, _ = _sample(fp, name)
    A_B = _mat(fp)[:, fp.B]
    R, _ = _lapack_rows(A_B, rows)
    ref = max(_backward_errors(A_B, R, rows))
    assert max(_backward_errors(A_B, np.zeros_like(W[rows]), rows)) > 4 * ref
    bad = W[rows].copy()
    bad[-1, int(np.argmax(np.abs(A_B).sum(axis=1)))] += 1e-3 * np.abs(bad[-1]).max()  # the entry most columns of A_B read
    assert max(_backward_errors(A_B, bad, rows)) > 4 * ref


def test_two_right_hand_sides_per_workgroup():
    """2,050 rows: the 16 m R bytes of LDS of k_range_solve allow R = 2 vectors per workgroup (R = 4 ends at 2,048 rows; R = 16,
    8 and 4 run at the shapes above, the last two with more than 64 KB of dynamic LDS).  Limits by definition, bit for bit, on
    every row; 8 rows of W — both rows of the first workgroup, the last row — against the reference.  R = 1 (above 4,096 rows)
    is the same template and is not run by any test."""
    E = _E()
    fp = _primal_fp(2050, 2100)
    eng = E.Engine(E.ENGINE_PRIMAL, fp, E.default_opts(max_iter=None))
    try:
        eng.run(40)
        rg = eng.ranging()
        eng.read_point()
        alpha, W = eng.tableau_rows(np.arange(fp.m))
    finally:
        eng.close()
    _check_definition(fp, rg, alpha, W, E.default_opts().eps, "primal-2050x2100")
    rows = np.sort(np.unique(np.concatenate([[0, 1, fp.m - 1], np.random.default_rng(7).choice(fp.m - 1, 5, replace=False)])))
    A_B = _mat(fp)[:, fp.B]
    ours = max(_backward_errors(A_B, W[rows], rows))
    R, snapped = _lapack_rows(A_B, rows)
    ref = max(_backward_errors(A_B, R, rows))
    print(f"primal-2050x2100: backward error of the rows of W {float(ours) / U:.3f} u, of the reference {float(ref) / U:.3f} u ({len(rows)} rows)")
    assert ref <= 64 * U and ours <= 4 * ref, (float(ours) / U, float(ref) / U)


@pytest.mark.parametrize("name", ["primal-17x30-small", "primal-50x120"])
def test_meaning_at_the_optimum(name):
    fp, rg, rg2, alpha, W, eps = _case(name, True)
    ex = RM.ExactRanging.of(fp, eps)
    two = 2 * ex.eps
    tiny_a = sum(1 for i in range(fp.m) for a in ex.alpha(i) if 0 < abs(a) <= two)
    tiny_w = sum(1 for row in ex.W for w in row if 0 < abs(w) <= two)
    assert 100 * tiny_a <= fp.m * fp.nN and 100 * tiny_w <= fp.m * fp.m, (name, tiny_a, tiny_w)
    checked = 0
    for i, v in enumerate(fp.B):
        for up, L, blk in ((True, rg.cost_up[v], rg.cost_blocking_up[v]), (False, rg.cost_down[v], rg.cost_blocking_down[v])):
            if np.isfinite(L):
                ex.check_cost_limit(i, L, blk, up)
                checked += 1
            else:
                assert blk == -1
    for k in range(fp.m):
        for up, L, blk in ((True, rg.rhs_up[k], rg.rhs_blocking_up[k]), (False, rg.rhs_down[k], rg.rhs_blocking_down[k])):
            if np.isfinite(L):
                ex.check_rhs_limit(k, L, blk, up)
                checked += 1
            else:
                assert blk == -1
    print(f"{name}: {checked} finite limits checked in exact arithmetic; {tiny_a} tableau entries and {tiny_w} entries of the inverse left out")
    assert checked > fp.m


@pytest.mark.parametrize("name", ["primal-17x30-small", "primal-200x500-hybrid", "primal-600x1500-two-launch", "dual-600-two-launch"])
def test_state_neutrality(name):
    """run, ranging, run gives the bits of run, run"""
    out = []
    for with_ranging in (True, False):
        eng, fp = _engine(name)
        try:
            s1, st1, _ = eng.run(40)
            if with_ranging:
                eng.ranging()
                eng.tableau_rows([0, fp.m - 1])
            s2, st2, _ = eng.run(40)
            eng.read_point()
        finally:
            eng.close()
        out.append((fp, s1, s2, st1.iters, st2.iters))
    (fa, a1, a2, ia1, ia2), (fb, b1, b2, ib1, ib2) = out
    assert (a1, a2, ia1, ia2) == (b1, b2, ib1, ib2)
    assert (_bits(fa.x) == _bits(fb.x)).all()
    assert (fa.B == fb.B).all() and (fa.N == fb.N).all() and (fa.Nb == fb.Nb).all()
    if fa.y is not None:
        assert (_bits(fa.y) == _bits(fb.y)).all() and (_bits(fa.d) == _bits(fb.d)).all()


def test_host_form_gives_the_engine_forms_bits():
    E = _E()
    fp = _primal_fp(50, 120)
    s, st, msg = E.primal_solve_with_initial(fp, E.default_opts(max_iter=1000))
    assert s == E.OPTIMAL, (s, msg)
    host = E.ranging(fp)
    eng = E.Engine(E.ENGINE_PRIMAL, fp, E.default_opts(max_iter=None))
    try:
        dev = eng.ranging()
    finally:
        eng.close()
    assert _same_ranging(host, dev)
    for key in host.kkt:
        assert _same([host.kkt[key]], [dev.kkt[key]]) if isinstance(host.kkt[key], float) else host.kkt[key] == dev.kkt[key], key


def test_partial_outputs_and_refusals():
    E = _E()
    import ctypes as C
    eng, fp = _engine("primal-17x30-small")
    try:
        eng.run(40)
        full = eng.ranging()
        only = E.RangingOut()
        up = np.zeros(fp.m)
        only.rhs_up = up.ctypes.data
        err = C.create_string_buffer(512)
        assert E.lib().ellp_engine_ranging(eng._h, C.byref(only), err, 512) == E.OPTIMAL
        assert _same(up, full.rhs_up)
        assert E.lib().ellp_engine_ranging(eng._h, C.byref(E.RangingOut()), err, 512) == E.ERR_ARG
        for bad in ([fp.m], [-1], []):
            with pytest.raises(E.EllpHipError) as ei:
                eng.tableau_rows(bad)
            assert ei.value.status == E.ERR_ARG
        # a chosen subset, repeated and out of order: the rows of the full call
        al_all, W_all = eng.tableau_rows(np.arange(fp.m))
        al, W = eng.tableau_rows([fp.m - 1, 0, fp.m - 1])
        assert _same(al, al_all[[fp.m - 1, 0, fp.m - 1]]) and _same(W, W_all[[fp.m - 1, 0, fp.m - 1]])
    finally:
        eng.close()
    fp2 = _primal_fp(200, 500)
    eng = E.Engine(E.ENGINE_PRIMAL, fp2, E.default_opts(max_iter=None, pipeline=1))
    try:
        eng.shard_columns(0, 1)
        with pytest.raises(E.EllpHipError) as ei:
            eng.ranging()
        assert ei.value.status == E.ERR_ARG
    finally:
        eng.close()


def test_nan_in_a_basic_entry():
    """one basic entry of x set to NaN: the rhs limits of every row k that reads it (|W[i][k]| > eps) are NaN, no limit
    derived from it is finite, the others are those of the clean point; nothing faults"""
    E = _E()
    eng, fp = _engine("primal-50x120")
    try:
        eng.run(40)
        eng.read_point()
        clean = eng.ranging()
        _, W = eng.tableau_rows(np.arange(fp.m))
        i = int(np.argmax((np.abs(W) > 1e-10).sum(axis=1)))  # the basic position most rows read
        v = int(fp.B[i])
        assert int(fp.kind[v]) != 0
        x2 = fp.x.copy()
        x2[v] = np.nan
        eng.debug_set_x(x2)
        rg = eng.ranging()
    finally:
        eng.close()
    reads = np.abs(W[i]) > E.default_opts().eps
    assert reads.any()
    assert np.isnan(rg.rhs_up[reads]).all() and np.isnan(rg.rhs_down[reads]).all()
    assert (rg.rhs_blocking_up[reads] == v).all() and (rg.rhs_blocking_down[reads] == v).all()  # the position that holds the NaN
    assert _same(rg.rhs_up[~reads], clean.rhs_up[~reads]) and _same(rg.rhs_down[~reads], clean.rhs_down[~reads])
    fp3 = E.FlatProblem(fp.m, fp.n, fp.n_c, fp.A, fp.c, fp.b, fp.kind, fp.lb, fp.ub, x2, fp.B, fp.N, fp.Nb)
    want = RM.rhs_ranging_f64(W, fp3.x, fp.B, fp.kind, fp.lb, fp.ub, E.default_opts().eps)
    for got, w in zip((rg.rhs_down, rg.rhs_up, rg.rhs_blocking_down, rg.rhs_blocking_up), want):
        assert _same(got, w)
    # the costs do not read x
    assert _same(rg.cost_up, clean.cost_up) and _same(rg.cost_down, clean.cost_down)

"""The models of tests/postsolve_model.py checked on the host, and the refusals of ellp_engine_postsolve / ellp_postsolve
that are answered before any HIP call (no device needed, as tests/test_plan_cpu.py does for creation)."""
import ctypes as C
import os
import sys
import types
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import postsolve_model as PM  # noqa: E402

from ellp_amd import _engine as E  # noqa: E402
from ellp_amd import synth  # noqa: E402


def _oracle_basis(seed, m, n, iters=40):
    """the synthetic phase-1 LP and the point 40 oracle iterations lead to"""
    from oracle import ellp_oracle as eo
    f = synth.primal_phase1_flat(seed, m, n)
    ph = types.SimpleNamespace(m=f["m"], n=f["n"], n_c=f["n_c"], A=f["A"], c=f["c"], b=f["b"], kind=f["kind"], lb=f["lb"],
                               ub=f["ub"], x=f["x"].copy(), B=f["B"].copy(), N=f["N"].copy(), Nb=f["Nb"].copy(),
                               nB=len(f["B"]), nN=len(f["N"]))
    st, it, err = eo.primal_solve_with_initial(ph, iters)
    assert it <= iters and not err and st in (E.OPTIMAL, E.MAXITER), (st, it, err)  # the 17-row phase 1 ends after 23
    return f, ph


def test_exact_dot_is_fraction_arithmetic():
    rng = np.random.default_rng(5)
    a = rng.normal(size=40) * 10.0 ** rng.integers(-30, 30, size=40)
    b = rng.normal(size=40) * 10.0 ** rng.integers(-30, 30, size=40)
    a[3] = 0.0
    ref = sum((Fraction(float(p)) * Fraction(float(q)) for p, q in zip(a, b)), Fraction(0))
    assert PM.exact_dot(a, b) == ref
    assert PM.exact_dot(a, b, absolute=True) == sum((abs(Fraction(float(p)) * Fraction(float(q))) for p, q in zip(a, b)), Fraction(0))


def test_geometry_and_bound():
    assert PM.post_cpb(17) == 64 and PM.post_blocks(17) == 1 and PM.post_blocks(0) == 0
    assert PM.post_cpb(36000) == 64 and PM.post_blocks(36000) == 563
    assert PM.post_cpb(70000) == 128 and PM.post_blocks(70000) == 547
    kd, kr = PM.chain_lengths(1040, 1300)
    assert kd == 8 + 6 + 3 + 1 and kr == 16 + 3 + 17 + 21 + 1
    # the bound is u |exact| + gamma_K^2 S, nothing more
    assert PM.entry_bound(Fraction(1), Fraction(2), 10) == Fraction(PM.U) + Fraction(PM.gamma(10)) ** 2 * 2


@pytest.mark.parametrize("m,n", [(17, 30), (50, 120), (200, 500), (600, 1500), (1040, 1300)])
def test_float_model_meets_two_u(m, n):
    """one refinement step with exact residuals reaches omega <= 2u on the bases the GPU tests stand on: the index sets
    after 40 iterations of the synthetic phase-1 LPs"""
    f, ph = _oracle_basis(20260301, m, n)
    A = f["A"].reshape(f["n"], m).T
    y, w, steps = PM.float_model(A[:, ph.B], f["c"][ph.B])
    print(f"m={m}: omega = {w / PM.U:.3f} u after {steps} refinement steps")
    assert w <= 2 * PM.U
    # the exact model's omega of that y is the one the float model reported
    ex = PM.Exact(m, f["n"], f["n_c"], A, f["c"], f["b"], f["kind"], f["lb"], f["ub"], ph.x, ph.B, ph.N, ph.Nb, y)
    assert float(ex.omega()) == w


def test_report_definitions():
    """report_from on a hand-made point: every kind, every label, ties and the -1 of a zero maximum"""
    fp = types.SimpleNamespace(m=2, n=6, n_c=7, nN=4, x=np.array([0.5, 3.0, -1.0, 2.0, 9.0, 0.0, 4.0]),
                               kind=np.array([0, 1, 2, 3, 4, 1, 4], dtype=np.uint8), lb=np.array([0, 1.0, 0, 0.0, 9.0, 0, 4.5]),
                               ub=np.array([0, 0, -2.0, 1.0, 0, 0, 0]), B=np.array([1, 3]), N=np.array([5, 0, 2, 4]),
                               Nb=np.array([0, 2, 1, 0], dtype=np.uint8))
    d = np.array([-0.25, 1e-17, 0.125, 0.0, -7.0, -0.25, 0.0])
    r = np.array([0.0, 0.0])
    k = PM.report_from(fp, d, r)
    assert (k["primal_residual"], k["worst_row"]) == (0.0, -1)
    assert (k["bound_violation"], k["worst_bound_var"]) == (1.0, 2)   # x_2 = -1 above its upper bound -2; x_3 = 2 over ub 1 ties: the smaller index
    assert (k["dual_infeasibility"], k["worst_dual_var"]) == (0.25, 0)  # Free |d_0| ties Lower -d_5: the smaller variable; Fixed x_4: 0
    assert k["basic_reduced_cost"] == 1e-17
    r[1] = np.nan
    assert np.isnan(PM.report_from(fp, d, r)["primal_residual"]) and PM.report_from(fp, d, r)["worst_row"] == 1


# ---- refusals answered without a device

def _flat(m=3, nN=4):
    n = m + nN
    A = np.zeros((m, n), order="F")
    A[:, :nN] = 1.0
    A[np.arange(m), nN + np.arange(m)] = 1.0
    z = np.zeros(n)
    return E.FlatProblem(m, n, n, A.reshape(-1, order="F"), z, np.ones(m), np.full(n, 1, dtype=np.uint8), z, z, z,
                         nN + np.arange(m, dtype=np.int64), np.arange(nN, dtype=np.int64), np.zeros(nN, dtype=np.uint8))


def _call(fp, args=None, outs=(True, True, True, True)):
    y, d, r, k = np.zeros(max(fp.m, 1)), np.zeros(fp.n_c), np.zeros(max(fp.m, 1)), E.Kkt()
    err = C.create_string_buffer(512)
    o = E.default_opts()
    a = fp._args() if args is None else args
    s = E.lib().ellp_postsolve(*a, C.byref(o), E._p(y) if outs[0] else None, E._p(d) if outs[1] else None,
                               E._p(r) if outs[2] else None, C.byref(k) if outs[3] else None, err, 512)
    return s, err.value.decode()


def test_engine_postsolve_refuses_null_engine():
    err = C.create_string_buffer(512)
    y = np.zeros(4)
    s = E.lib().ellp_engine_postsolve(None, E._p(y), None, None, None, err, 512)
    assert s == E.ERR_ARG and err.value


def test_postsolve_refuses_nothing_wanted():
    s, msg = _call(_flat(), outs=(False, False, False, False))
    assert s == E.ERR_ARG and "none of" in msg


@pytest.mark.parametrize("what", ["m0", "m_too_large", "nB", "sum", "B_range", "N_range", "Nb_range", "kind_range", "null_A", "null_x", "null_B"])
def test_postsolve_refuses_bad_arguments(what):
    fp = _flat()
    a = fp._args()  # m, n, n_c, A, c, b, kind, lb, ub, x, B, nB, N, Nb, nN
    if what == "m0":
        a[0] = 0
    elif what == "m_too_large":  # above the engines' own limit of 8,192 rows: refused, not a failed launch
        a[0] = a[11] = 8193
        a[1] = a[2] = 8193 + fp.nN
    elif what == "nB":
        a[11] = fp.m - 1
    elif what == "sum":
        a[14] = fp.nN - 1
    elif what == "B_range":
        fp.B[1] = fp.n
    elif what == "N_range":
        fp.N[0] = -1
    elif what == "Nb_range":
        fp.Nb[2] = 3
    elif what == "kind_range":
        fp.kind[0] = 5
    elif what == "null_A":
        a[3] = None
    elif what == "null_x":
        a[9] = None
    elif what == "null_B":
        a[10] = None
    s, msg = _call(fp, a)
    assert s == E.ERR_ARG and msg, (what, s, msg)

"""Inputs shared by the warm-start tests (tests/test_start_model_cpu.py, tests/test_gpu_start.py, tests/test_gpu_start_api.py):
standard forms with an optimal basis from the reference's own loops (the oracle, on the CPU), the perturbations of the
issue's table, and the structured 513-row basis."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import helpers  # noqa: E402


def netlib(name):
    return helpers.read_mps(os.path.join(helpers.GOLDEN, "netlib", name + ".mps"))


def perturbed(fx, what, s):
    """perturbation k of constraint (what == 'rhs') or variable ('cost') k, 0-based in file order: value * (1 + s sin(k + 1))"""
    out = {"vars": [[obj, list(bound)] for obj, bound in fx["vars"]],
           "constraints": [[[list(c) for c in coeffs], op, rhs] for coeffs, op, rhs in fx["constraints"]]}
    if what == "rhs":
        for k, con in enumerate(out["constraints"]):
            con[2] = con[2] * (1.0 + s * math.sin(k + 1))
    else:
        for k, var in enumerate(out["vars"]):
            var[0] = var[0] * (1.0 + s * math.sin(k + 1))
    return out


def oracle_optimum(fx):
    """the original standard form of a fixture with the optimal point of the oracle's dual solve: a Phase view (A, c, b, kind,
    lb, ub, x, B, N, Nb, y, d) in the indices of StandardForm::from_problem — variables, then slacks"""
    from oracle import ellp_oracle as eo
    p1, err = eo.dual_phase1(eo.Problem.from_fixture(fx))
    assert p1 and err == 0, err
    v1 = p1.view()
    st, _, msg = eo.dual_solve_with_initial(v1)
    assert st == 0, (st, msg)
    p1.store_point(v1)
    p2, err = eo.dual_phase2(p1)
    assert p2 and err == 0, err
    v = p2.view()
    st, _, msg = eo.dual_solve_with_initial(v)
    assert st == 0, (st, msg)
    return v


def flat_of(v, B=None, N=None, Nb=None):
    """an _engine.FlatProblem of a standard form (a Phase view) with a basis (default: the view's)"""
    from ellp_amd import _engine as E
    B = v.B if B is None else B
    N = v.N[:v.nN] if N is None else N
    Nb = v.Nb[:v.nN] if Nb is None else Nb
    return E.FlatProblem(v.m, v.n, v.n, v.A, v.c[:v.n], v.b, v.kind[:v.n], v.lb[:v.n], v.ub[:v.n], np.zeros(v.n), B, N, Nb)


def bidiagonal_case(m=513, nN=40, seed=20260513):
    """m rows, A_B a row-permuted unit lower bidiagonal matrix with sub-diagonal entries from {1, 1/2, -1/2, 2} (an exact
    solve is O(m) in Fractions), nN nonbasic columns of small dyadic entries, mixed kinds.  Returns a dict of arrays and the
    (perm, sub) of start_model.bidiagonal."""
    rng = np.random.default_rng(seed)
    perm = [int(p) for p in rng.permutation(m)]
    sub = rng.choice([1.0, 0.5, -0.5, 2.0], size=m)
    sub[::7] = 0.0  # break the chain: x stays of moderate size
    n = m + nN
    A = np.zeros((m, n))
    L = np.eye(m)
    for i in range(1, m):
        L[i, i - 1] = sub[i]
    B = np.arange(nN, n, dtype=np.int64)
    A[np.asarray(perm), nN:] = L
    for j in range(nN):
        rows = rng.choice(m, size=5, replace=False)
        A[rows, j] = rng.integers(-8, 9, size=5) / 4.0
    c = np.round(rng.normal(size=n) * 16) / 16
    b = np.round(rng.normal(size=m) * 16) / 16
    kind = np.ones(n, dtype=np.uint8)
    kind[:nN] = rng.choice([0, 1, 2, 3, 4], size=nN)
    kind[nN::5] = 0
    kind[nN + 1::5] = 3
    lb = np.where(kind == 0, 0.0, -np.round(rng.uniform(0, 2, size=n) * 8) / 8)
    ub = np.where(kind == 0, 0.0, lb + 1.0 + np.round(rng.uniform(0, 2, size=n) * 8) / 8)
    ub = np.where(kind == 4, lb, ub)
    Nb = rng.choice([0, 1, 2], size=nN).astype(np.uint8)
    return dict(m=m, n=n, A=A, c=c, b=b, kind=kind, lb=lb, ub=ub, B=B, N=np.arange(nN, dtype=np.int64), Nb=Nb), perm, sub

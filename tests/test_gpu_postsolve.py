"""ellp_engine_postsolve / ellp_postsolve on the device against the exact model of tests/postsolve_model.py.

Inputs of the model are the engine's own read_point output (x, B, N, Nb) and the y the postsolve returned; every entry of d
and r must lie within  u |exact| + gamma_K^2 S  of its exact value (K from the kernel's geometry, postsolve_model's
docstring; no factor on the bound), the report's maxima must be, bit for bit, the definitions of include/ellp_hip.h applied
to the returned d, r and the point, and must agree with the exact maxima within the largest entry bound.

omega: y_backward_error <= 2u, and against the exact omega of the returned y within
    omega (3u + 2 gamma_{K_d + 1}) + 2 gamma_{K_d}^2
— the numerator |rho_i| carries the entry bound u |rho| + gamma_{K_d}^2 S, the denominator is a plain f64 sum of K_d + 1
rounded non-negative products (relative error gamma_{K_d + 1}), the quotient one more rounding.

The objectives: compensated sums of (m + n_c) terms, a chain of ceil(terms / 1024) + 10 + 1 operations (a thread's stride,
the block's tree), same bound.

At the two largest shapes (600 x 1500 and 1040 x 1300) the exact d is checked on a seeded sample of 64 columns; everywhere
else on every column, and r, omega and the objectives on every row and column at every shape.

test_against_exact_model calls postsolve() straight after run(40), before any read_point: on the two pipeline = 2 engines
the slice leaves its last iteration open, and the postsolve must complete it before it looks at the point.  The model's
inputs are read afterwards; a postsolve that skipped the completion would describe another basis and another x.

Met on an MI355X (records, not limits): largest |got - exact| / bound 0.944 (50 x 120), 0.941 (200 x 500), 0.887 (600 x 1500),
0.925 (1040 x 1300), 0.769 / 0.789 (the duals), 0.69 - 0.93 (the wide LPs); omega 0 to 1.81 u with 0 or 1 refinement steps.
"""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import postsolve_model as PM  # noqa: E402

pytestmark = pytest.mark.gpu
U = PM.U


def _E():
    from ellp_amd import _engine as E
    return E


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _primal_fp(m, n, seed=20260301):
    from ellp_amd import synth
    E = _E()
    f = synth.primal_phase1_flat(seed, m, n)
    return E.FlatProblem(f["m"], f["n"], f["n_c"], f["A"], f["c"], f["b"], f["kind"], f["lb"], f["ub"], f["x"], f["B"], f["N"], f["Nb"])


def _dual_fp_synth(m, n, seed=20260301):
    from ellp_amd import synth
    E = _E()
    f = synth.dual_start_flat(seed, m, n)
    return E.FlatProblem(f["m"], f["n"], f["n_c"], f["A"], f["c"], f["b"], f["kind"], f["lb"], f["ub"], f["x"], f["B"], f["N"], f["Nb"],
                         y=f["y"], d=f["d"])


def _dual_fp_oracle():
    """the dual phase-1 arrays of tests/test_gpu_dist.py::_dual_flat (20 x 50), rebuilt here"""
    from oracle import ellp_oracle as eo
    E = _E()
    p1, err = eo.dual_phase1(eo.synth_problem(20260301, 20, 50))
    v = p1.view()
    return E.FlatProblem(v.m, v.n, v.n_c, v.A, v.c, v.b, v.kind, v.lb, v.ub, v.x, v.B, v.N[:v.nN], v.Nb[:v.nN], v.y, v.d)


CASES = {
    "primal-17x30-small": (lambda: _primal_fp(17, 30), 0, dict()),
    "primal-50x120": (lambda: _primal_fp(50, 120), 0, dict()),
    "primal-200x500-hybrid": (lambda: _primal_fp(200, 500), 0, dict()),
    "primal-600x1500-two-launch": (lambda: _primal_fp(600, 1500), 0, dict(pipeline=2)),
    "primal-1040x1300": (lambda: _primal_fp(1040, 1300), 0, dict()),
    "dual-20x50": (_dual_fp_oracle, 1, dict()),
    "dual-600-two-launch": (lambda: _dual_fp_synth(600, 400), 1, dict(pipeline=2)),
}
SAMPLED = ("primal-600x1500-two-launch", "primal-1040x1300")  # the two largest shapes


def _engine(name):
    E = _E()
    make, kind, kw = CASES[name]
    fp = make()
    return E.Engine(kind, fp, E.default_opts(max_iter=None, **kw)), fp


def _check_against_exact(fp, y, d, r, k, sample_cols=None, label=""):
    """the whole comparison of one postsolve with the exact model; returns the largest |got - exact| / bound met"""
    ex = PM.Exact.of(fp, y)
    kd, kr = PM.chain_lengths(fp.m, fp.nN)
    worst = 0.0
    big_r = Fraction(0)
    r_exact = []
    for i in range(fp.m):
        e, S = ex.r(i)
        bound = PM.entry_bound(e, S, kr)
        big_r = max(big_r, bound)
        r_exact.append(e)
        err = abs(Fraction(float(r[i])) - e)
        assert err <= bound, (label, "r", i, float(err), float(bound))
        if bound:
            worst = max(worst, float(err / bound))
    cols = range(fp.n_c) if sample_cols is None else sample_cols
    big_d = Fraction(0)
    d_exact = {}
    for v in cols:
        e, S = ex.d(int(v))
        bound = PM.entry_bound(e, S, kd)
        big_d = max(big_d, bound)
        d_exact[int(v)] = e
        err = abs(Fraction(float(d[v])) - e)
        assert err <= bound, (label, "d", v, float(err), float(bound))
        if bound:
            worst = max(worst, float(err / bound))
    # omega
    w = ex.omega()
    g1, g0 = Fraction(PM.gamma(kd + 1)), Fraction(PM.gamma(kd))
    tol = w * (3 * Fraction(U) + 2 * g1) + 2 * g0 * g0
    print(f"{label}: omega = {k['y_backward_error'] / U:.3f} u after {k['refinement_steps']} steps (exact {float(w) / U:.3f} u); "
          f"max |got - exact| / bound = {worst:.3f}; primal_residual {k['primal_residual']:.3e}, dual_infeasibility "
          f"{k['dual_infeasibility']:.3e}, basic_reduced_cost {k['basic_reduced_cost']:.3e}")
    assert abs(Fraction(k["y_backward_error"]) - w) <= tol, (label, k["y_backward_error"], float(w))
    assert k["y_backward_error"] <= 2 * U, (label, k["y_backward_error"] / U)
    assert 0 <= k["refinement_steps"] <= 4
    # the maxima: the definitions on the returned arrays, bit for bit
    rep = PM.report_from(fp, d, r)
    for key, val in rep.items():
        if isinstance(val, float):
            assert _bits([k[key]])[0] == _bits([val])[0], (label, key, k[key], val)
        else:
            assert k[key] == val, (label, key, k[key], val)
    # ... and the exact maxima within the largest entry bound
    assert abs(Fraction(k["primal_residual"]) - max(abs(e) for e in r_exact)) <= big_r, (label, "primal_residual")
    if sample_cols is None:
        N, Nb = fp.N[:fp.nN], fp.Nb[:fp.nN]
        inf = Fraction(0)
        for j in range(fp.nN):
            e = d_exact[int(N[j])]
            if int(fp.kind[N[j]]) == 4:
                continue
            inf = max(inf, -e if Nb[j] == 0 else (e if Nb[j] == 1 else abs(e)))
        assert abs(Fraction(k["dual_infeasibility"]) - inf) <= big_d, (label, "dual_infeasibility")
        assert abs(Fraction(k["basic_reduced_cost"]) - max(abs(d_exact[int(v)]) for v in fp.B)) <= big_d, (label, "basic_reduced_cost")
    # the objectives
    terms = fp.m + fp.n_c
    g = Fraction(PM.gamma((terms + 1023) // 1024 + 11))
    po = ex.primal_obj()
    assert abs(Fraction(k["primal_obj"]) - po) <= Fraction(U) * abs(po) + g * g * PM.exact_dot(fp.c, fp.x, absolute=True), (label, "primal_obj")
    do = ex.dual_obj(d)
    coef = np.where(np.isin(fp.kind, (1, 3, 4)), np.abs(fp.lb), 0.0) + np.where(np.isin(fp.kind, (2, 3)), np.abs(fp.ub), 0.0)
    S = PM.exact_dot(fp.b, y, absolute=True) + PM.exact_dot(coef, d, absolute=True)
    assert abs(Fraction(k["dual_obj"]) - do) <= Fraction(U) * abs(do) + g * g * S, (label, "dual_obj")
    return worst


@pytest.mark.parametrize("name", list(CASES))
def test_against_exact_model(name):
    E = _E()
    eng, fp = _engine(name)
    try:
        eng.run(40)
        # straight after the slice: on the two-launch pipeline the last iteration is still open, and the postsolve has to
        # complete it itself (its outputs belong to the completed point, the one read_point delivers afterwards)
        y, d, r, k = eng.postsolve()
        assert eng.closing_status == E.OPTIMAL
        eng.read_point()
        assert eng.closing_status == E.OPTIMAL
        y2, d2, r2, k2 = eng.postsolve()  # the same state (completing an iteration twice completes it once): the same bits
    finally:
        eng.close()
    assert (_bits(y) == _bits(y2)).all() and (_bits(d) == _bits(d2)).all() and (_bits(r) == _bits(r2)).all()
    assert all(_bits([k[key]])[0] == _bits([k2[key]])[0] if isinstance(k[key], float) else k[key] == k2[key] for key in k)
    sample = None
    if name in SAMPLED:
        sample = np.sort(np.random.default_rng(7).choice(fp.n_c, 64, replace=False))
    _check_against_exact(fp, y, d, r, k, sample, name)


def _wide_fp(seed, which):
    from oracle import ellp_oracle as eo
    from test_gpu_random import wide_fixture
    E = _E()
    prob = eo.Problem.from_fixture(wide_fixture(np.random.default_rng(seed)))
    p1, err = (eo.primal_phase1 if which == "primal" else eo.dual_phase1)(prob)
    assert p1 is not None and not err
    v = p1.view()
    return E.FlatProblem(v.m, v.n, v.n_c, v.A, v.c, v.b, v.kind, v.lb, v.ub, v.x, v.B, v.N[:v.nN], v.Nb[:v.nN], v.y, v.d)


@pytest.mark.parametrize("which", ["primal", "dual"])
@pytest.mark.parametrize("seed", [300, 305, 311])
def test_every_bound_kind(seed, which):
    """random wide LPs with Lower, Upper, TwoSided and Fixed variables, primal and dual phase 1"""
    E = _E()
    fp = _wide_fp(seed, which)
    eng = E.Engine(E.ENGINE_PRIMAL if which == "primal" else E.ENGINE_DUAL, fp, E.default_opts(max_iter=None))
    try:
        eng.run(40)
        eng.read_point()
        y, d, r, k = eng.postsolve()
    finally:
        eng.close()
    kinds = set(int(t) for t in fp.kind)
    print(f"seed {seed} {which}: {fp.m} x {fp.n}, kinds {sorted(kinds)}, labels {sorted(set(int(t) for t in fp.Nb[:fp.nN]))}")
    assert which == "dual" or 4 in kinds  # the dual's phase 1 is the box problem: every variable TwoSided
    _check_against_exact(fp, y, d, r, k, None, f"wide-{seed}-{which}")


def test_free_labels_and_fixed_variables():
    """the wide LPs have no Free variable: the 17-row point with some nonbasic variables made Free (label Free) and some
    Fixed, through ellp_postsolve; Free counts |d_v|, Fixed nothing"""
    E = _E()
    eng, fp = _engine("primal-17x30-small")
    try:
        eng.run(10)
        eng.read_point()
    finally:
        eng.close()
    for j in range(0, fp.nN, 3):
        fp.kind[fp.N[j]] = 0
        fp.Nb[j] = 2
    for j in range(1, fp.nN, 3):
        fp.kind[fp.N[j]] = 4
    y, d, r, k = E.postsolve(fp)
    rep = PM.report_from(fp, d, r)
    free = [int(fp.N[j]) for j in range(0, fp.nN, 3)]
    assert k["dual_infeasibility"] >= max(abs(d[v]) for v in free) > 0.0
    assert k["worst_dual_var"] == rep["worst_dual_var"] and int(fp.kind[k["worst_dual_var"]]) != 4
    _check_against_exact(fp, y, d, r, k, None, "free-and-fixed")


@pytest.mark.parametrize("name", ["primal-17x30-small", "primal-200x500-hybrid", "primal-600x1500-two-launch", "dual-600-two-launch"])
def test_state_neutrality(name):
    """run, postsolve, run gives the bits of run, run"""
    E = _E()
    out = []
    for with_post in (True, False):
        eng, fp = _engine(name)
        try:
            s1, st1, _ = eng.run(40)
            if with_post:
                eng.postsolve()
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


def test_sees_a_moved_basic_entry_and_nan():
    """what k_invariants cannot: a basic entry moved by 1e-6 inside its bounds shows in primal_residual (about
    1e-6 max_i |a_iv|) and nowhere in bound_violation; a NaN entry gives NaN, not a fault and not a finite number"""
    E = _E()
    eng, fp = _engine("primal-50x120")
    try:
        eng.run(40)
        eng.read_point()
        y0, d0, r0, k0 = eng.postsolve()
        dense = [int(v) for v in fp.B if v < 120]  # a structural (dense) basic column
        v = dense[0]
        x2 = fp.x.copy()
        x2[v] += 1e-6
        eng.debug_set_x(x2)
        y, d, r, k = eng.postsolve()
        fp2 = E.FlatProblem(fp.m, fp.n, fp.n_c, fp.A, fp.c, fp.b, fp.kind, fp.lb, fp.ub, x2, fp.B, fp.N, fp.Nb)
        ex = PM.Exact.of(fp2, y)
        kd, kr = PM.chain_lengths(fp.m, fp.nN)
        exact = [ex.r(i) for i in range(fp.m)]
        top = max(range(fp.m), key=lambda i: (abs(exact[i][0]), -i))
        assert abs(Fraction(k["primal_residual"]) - abs(exact[top][0])) <= PM.entry_bound(*exact[top], kr)
        assert k["worst_row"] == top
        col = fp.A.reshape(fp.n, fp.m)[v]
        assert 0.5e-6 * np.abs(col).max() <= k["primal_residual"] <= 2e-6 * np.abs(col).max()
        assert k["bound_violation"] == k0["bound_violation"]
        x2[v] = np.nan
        eng.debug_set_x(x2)
        y, d, r, k = eng.postsolve()
        assert np.isnan(k["primal_residual"]) and not np.isfinite(k["primal_obj"])
    finally:
        eng.close()


def test_host_form_gives_the_engine_forms_bits():
    E = _E()
    fp = _primal_fp(50, 120)
    s, st, msg = E.primal_solve_with_initial(fp, E.default_opts(max_iter=1000))
    assert s == E.OPTIMAL, (s, msg)
    y, d, r, k = E.postsolve(fp)
    eng = E.Engine(E.ENGINE_PRIMAL, fp, E.default_opts(max_iter=None))
    try:
        y2, d2, r2, k2 = eng.postsolve()
    finally:
        eng.close()
    assert (_bits(y) == _bits(y2)).all() and (_bits(d) == _bits(d2)).all() and (_bits(r) == _bits(r2)).all()
    for key in k:
        assert (_bits([k[key]])[0] == _bits([k2[key]])[0]) if isinstance(k[key], float) else (k[key] == k2[key]), key
    _check_against_exact(fp, y, d, r, k, None, "host-form-50x120")


def test_refused_on_a_column_sharded_engine():
    E = _E()
    fp = _primal_fp(200, 500)
    eng = E.Engine(E.ENGINE_PRIMAL, fp, E.default_opts(max_iter=None, pipeline=1))
    try:
        eng.shard_columns(0, 1)
        with pytest.raises(E.EllpHipError) as ei:
            eng.postsolve()
        assert ei.value.status == E.ERR_ARG
    finally:
        eng.close()

"""ellp_batch_postsolve on the device: every output of every item is, as bytes, what ellp_postsolve returns for the item
alone — at the edge shapes of k_post_batch (rows 1, 2, 17, 63, 64, 65, 127, 128; nonbasic columns 1, 63, 64, 65, 129), on
points of both engine kinds, with n_c > n, Free labels and Fixed kinds, reversed, chunked, next to failing items and next
to a NaN — and lies within the bound of the exact model of tests/postsolve_model.py (the geometry is the single call's, so
chain_lengths holds unchanged).

Met on an MI355X (records, not limits): largest |got - exact| / bound 0.953 (64 x 129), 0.700 (127 rows), 0.553 / 0.440
(128 rows), under 0.01 at the other edge shapes; omega 0 to 1.48 u, one refinement step at 127 rows; the hand-made 24 x 24
basis of test_refinement_runs_on_the_device: one step, omega 0.282 u afterwards.
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

# (rows, nonbasic columns): every row count and every column count of the issue's table at least once
EDGES = [(1, 1), (2, 63), (17, 64), (63, 65), (64, 129), (65, 1), (127, 64), (128, 63), (128, 129), (17, 129), (64, 64), (127, 1)]


def _E():
    from ellp_amd import _engine as E
    return E


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _copy(fp):
    E = _E()
    out = E.FlatProblem(fp.m, fp.n, fp.n_c, fp.A, fp.c, fp.b, fp.kind, fp.lb, fp.ub, fp.x, fp.B, fp.N, fp.Nb, nN=fp.nN)
    out.nB = fp.nB
    return out


def _restrict(fp, keep):
    """the point of fp on its basic columns and its first `keep` nonbasic columns (n_c == n), renumbered in place order"""
    E = _E()
    assert fp.n_c == fp.n and keep <= fp.nN
    cols = np.sort(np.r_[fp.B, fp.N[:keep]])
    new = {int(v): k for k, v in enumerate(cols)}
    A = fp.A.reshape(fp.n, fp.m)[cols].reshape(-1)
    return E.FlatProblem(fp.m, len(cols), len(cols), A, fp.c[cols], fp.b, fp.kind[cols], fp.lb[cols], fp.ub[cols], fp.x[cols],
                         [new[int(v)] for v in fp.B], [new[int(v)] for v in fp.N[:keep]], fp.Nb[:keep])


def _synth(m, n, seed=20260301):
    from ellp_amd import synth
    E = _E()
    f = synth.primal_phase1_flat(seed, m, n)
    return E.FlatProblem(f["m"], f["n"], f["n_c"], f["A"], f["c"], f["b"], f["kind"], f["lb"], f["ub"], f["x"], f["B"], f["N"], f["Nb"])


_ITEMS = {}


def items():
    """[(label, FlatProblem)] and, once, the single call's result of each: (y, d, r, kkt)"""
    if _ITEMS:
        return _ITEMS["fps"], _ITEMS["ref"]
    from oracle import ellp_oracle as eo
    from test_gpu_batch import random_lp
    from test_gpu_random import wide_fixture
    from test_gpu_small import flat
    E = _E()
    primal, dual = [], []  # (label, fp), advanced by a batched solve of their kind below
    for m, nN in EDGES:
        primal.append((f"edge-{m}x{nN}", _synth(m, max(nN - m, 8), seed=20260301 + m)))
    primal.append(("free-and-fixed", _synth(17, 30)))
    fxs = [(f"random-{s}", random_lp(np.random.default_rng(61000 + s), int(np.random.default_rng(62000 + s).integers(1, 129))))
           for s in range(60)]
    fxs.append(("wide", wide_fixture(np.random.default_rng(300))))
    for label, fx in fxs:
        prob = eo.Problem.from_fixture(fx)
        for which, phase1, out in (("primal", eo.primal_phase1, primal), ("dual", eo.dual_phase1, dual)):
            p1, err = phase1(prob)
            if p1 is None or err:
                continue
            v = p1.view()
            if v.m == 0 or v.m > 128 or v.nN == 0:
                continue
            out.append((f"{label}-{which}", flat(v)))
    # a few iterations (to the end for most): the bases are not the starting ones
    for kind, group in ((E.ENGINE_PRIMAL, primal), (E.ENGINE_DUAL, dual)):
        res = E.batch_solve_with_initial(kind, [fp for _, fp in group], E.default_opts(max_iter=60))
        assert all(st >= 0 for st, _, _ in res), [(lab, st, msg) for (lab, _), (st, _, msg) in zip(group, res) if st < 0]
    fps = []
    for (label, fp), (m, nN) in zip(primal, EDGES):
        fps.append((label, _restrict(fp, nN)))
    label, fp = primal[len(EDGES)]
    fp = _copy(fp)
    for j in range(0, fp.nN, 3):  # as test_gpu_postsolve.test_free_labels_and_fixed_variables
        fp.kind[fp.N[j]] = 0
        fp.Nb[j] = 2
    for j in range(1, fp.nN, 3):
        fp.kind[fp.N[j]] = 4
    fps.append((label, fp))
    fps += [(lab, _copy(fp)) for lab, fp in primal[len(EDGES) + 1:]] + [(lab, _copy(fp)) for lab, fp in dual]
    assert any(fp.n_c > fp.n for _, fp in fps), "no item with n_c > n"
    assert len(primal) > len(EDGES) + 20 and len(dual) > 20
    assert any(fp.nN > 2048 for _, fp in fps)
    ref = [E.postsolve(_copy(fp)) for _, fp in fps]
    _ITEMS["fps"], _ITEMS["ref"] = fps, ref
    return fps, ref


def _same_bits(tag, got, ref):
    """(y, d, r, kkt) against (y, d, r, kkt), as bytes"""
    for name, a, b in zip("ydr", got[:3], ref[:3]):
        assert a.shape == b.shape and (_bits(a) == _bits(b)).all(), (tag, name, np.flatnonzero(_bits(a) != _bits(b))[:8])
    k, k2 = got[3], ref[3]
    assert set(k) == set(k2)
    for key in k2:
        if isinstance(k2[key], float):
            assert _bits([k[key]])[0] == _bits([k2[key]])[0], (tag, key, k[key], k2[key])
        else:
            assert k[key] == k2[key], (tag, key, k[key], k2[key])


def _batch(fps, **kw):
    E = _E()
    res = E.batch_postsolve([_copy(fp) for fp in fps], **kw)
    return res, E.batch_postsolve_info()


def test_bits_equal_the_single_call(monkeypatch):
    E = _E()
    fps, ref = items()
    only = [fp for _, fp in fps]
    res, info = _batch(only)
    assert info["batched"] == len(only) and info["single"] == 0 and info["chunks"] == 1
    per_chunk = info["launches"] // info["chunks"]
    assert info["launches"] == per_chunk * info["chunks"] and 1 <= per_chunk <= 4
    for (label, _), (st, y, d, r, k, msg), rf in zip(fps, res, ref):
        assert st == E.OPTIMAL and msg == "", (label, st, msg)
        _same_bits(label, (y, d, r, k), rf)
    # three items: the same launches per chunk
    res3, info3 = _batch(only[:3])
    assert (info3["launches"], info3["batched"], info3["chunks"]) == (per_chunk, 3, 1)
    # reversed
    resr, _ = _batch(only[::-1])
    for (label, _), (st, y, d, r, k, msg), rf in zip(fps[::-1], resr, ref[::-1]):
        assert st == E.OPTIMAL, (label, st, msg)
        _same_bits(("reversed", label), (y, d, r, k), rf)
    # chunked by the budget
    monkeypatch.setenv("ELLP_BATCH_MAX_BYTES", str(1 << 20))
    resc, infoc = _batch(only)
    assert infoc["chunks"] >= 3 and infoc["launches"] == per_chunk * infoc["chunks"] and infoc["batched"] == len(only)
    for (label, _), (st, y, d, r, k, msg), rf in zip(fps, resc, ref):
        assert st == E.OPTIMAL, (label, st, msg)
        _same_bits(("chunked", label), (y, d, r, k), rf)


def _check_against_exact(fp, y, d, r, k, sample_cols=None, label=""):
    """the whole comparison of one postsolve with the exact model (test_gpu_postsolve._check_against_exact, copied); returns
    the largest |got - exact| / bound met"""
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


def test_against_exact_model():
    """the batch's own outputs against the exact model: the edge shapes (the 128-row ones on a seeded sample of 48 columns)
    and the item with Free labels and Fixed kinds"""
    E = _E()
    fps, _ = items()
    chosen = [(lab, fp) for lab, fp in fps if lab.startswith("edge-") or lab == "free-and-fixed"]
    chosen = [c for c in chosen if c[0] not in ("edge-64x64",)]
    assert len(chosen) == 12
    res, _ = _batch([fp for _, fp in chosen])
    for (label, fp), (st, y, d, r, k, msg) in zip(chosen, res):
        assert st == E.OPTIMAL, (label, st, msg)
        sample = None
        if fp.m >= 127 and fp.n_c > 48:
            sample = np.sort(np.random.default_rng(7).choice(fp.n_c, 48, replace=False))
        _check_against_exact(fp, y, d, r, k, sample, label)


def ill_conditioned(m=24, nN=7, seed=5, gap=1e-10, row_decades=6.0):
    """a hand-made point: a dense m x m basis whose second column is the first plus `gap` times noise (condition number
    about 1 / gap), its rows scaled over 2 * row_decades decades, so that the first solve's componentwise backward error
    stays above 2u; no solve is needed, the postsolve takes any basis"""
    E = _E()
    rng = np.random.default_rng(seed)
    B = rng.normal(size=(m, m))
    B[:, 1] = B[:, 0] + gap * rng.normal(size=m)
    scale = 10.0 ** rng.uniform(-row_decades, row_decades, size=m)
    n = m + nN
    A = np.empty((m, n))
    A[:, :nN] = rng.normal(size=(m, nN))
    A[:, nN:] = B
    A *= scale[:, None]
    x = rng.normal(size=n)
    return E.FlatProblem(m, n, n, A.T.reshape(-1), rng.normal(size=n), rng.normal(size=m), np.ones(n, np.uint8), np.zeros(n), np.zeros(n),
                         x, np.arange(nN, n), np.arange(nN), np.zeros(nN, np.uint8))


def test_refinement_runs_on_the_device():
    E = _E()
    fp = ill_conditioned()
    ref = E.postsolve(_copy(fp))
    print(f"ill-conditioned 24 x 24: the single call took {ref[3]['refinement_steps']} steps, omega = {ref[3]['y_backward_error'] / U:.3f} u")
    assert ref[3]["refinement_steps"] >= 1  # the condition of this test: the loop runs
    fps, refs = items()
    res, _ = _batch([fps[0][1], fp, fps[1][1]])
    assert [st for st, *_ in res] == [E.OPTIMAL] * 3
    assert res[1][4]["refinement_steps"] == ref[3]["refinement_steps"]
    _same_bits("ill-conditioned", res[1][1:5], ref)
    _same_bits("before", res[0][1:5], refs[0])
    _same_bits("after", res[2][1:5], refs[1])


def _single(fp):
    E = _E()
    try:
        return (E.OPTIMAL, "") + E.postsolve(_copy(fp))
    except E.EllpHipError as e:
        return (e.status, e.msg, None, None, None, None)


def test_failing_items_are_isolated():
    E = _E()
    fps, ref = items()
    good = [fp for _, fp in fps[:9]]
    singular, index, dims = _copy(good[3]), _copy(good[4]), _copy(good[5])
    singular.B[1] = singular.B[0]  # a repeated column
    index.N[0] = index.n + 3
    dims.nB = dims.m - 1
    bad = [singular, index, dims]
    alone = [_single(b) for b in bad]
    assert [a[0] for a in alone] == [E.ERR_SINGULAR, E.ERR_ARG, E.ERR_ARG] and all(a[1] for a in alone)
    mixed = good[:2] + [bad[0]] + good[2:5] + [bad[1], bad[2]] + good[5:]
    at = (2, 6, 7)
    res, info = _batch(mixed, fill=-7.5)
    assert info["batched"] == len(good) + 1  # the singular one reaches the kernel
    for pos, a in zip(at, alone):
        st, y, d, r, k, msg = res[pos]
        assert (st, msg) == a[:2]
        assert k is None and all((v == -7.5).all() for v in (y, d, r))  # untouched
    rest = [res[k] for k in range(len(mixed)) if k not in at]
    for k, ((st, y, d, r, kk, msg), rf) in enumerate(zip(rest, ref[:9])):
        assert st == E.OPTIMAL and msg == ""
        _same_bits(("mixed", k), (y, d, r, kk), rf)


def test_nan_in_x():
    E = _E()
    fps, ref = items()
    nan = _copy(fps[2][1])
    nan.x[int(nan.B[0])] = np.nan
    alone = E.postsolve(_copy(nan))
    assert np.isnan(alone[3]["primal_residual"]) and not np.isfinite(alone[3]["primal_obj"])
    res, _ = _batch([fps[0][1], nan, fps[1][1]])
    assert [st for st, *_ in res] == [E.OPTIMAL] * 3
    k = res[1][4]
    assert np.isnan(k["primal_residual"]) and not np.isfinite(k["primal_obj"])
    _same_bits("nan", res[1][1:5], alone)
    _same_bits("before", res[0][1:5], ref[0])
    _same_bits("after", res[2][1:5], ref[1])


def test_large_items_take_the_single_path():
    E = _E()
    fps, ref = items()
    big = _synth(200, 300)  # 200 rows, 500 nonbasic columns
    s, _, msg = E.primal_solve_with_initial(big, E.default_opts(max_iter=40))
    assert s >= 0, (s, msg)
    assert (big.m, big.nN) == (200, 500)
    alone = E.postsolve(_copy(big))
    res, info = _batch([fps[0][1], big, fps[1][1]])
    assert (info["batched"], info["single"]) == (2, 1)
    assert [st for st, *_ in res] == [E.OPTIMAL] * 3
    _same_bits("big", res[1][1:5], alone)
    _same_bits("before", res[0][1:5], ref[0])
    _same_bits("after", res[2][1:5], ref[1])


def test_refusal_chunks_and_single_path_in_one_call(monkeypatch):
    """a refused item, two batched items, one on the single path and one more batched item, cut into chunks by the budget"""
    from batch_driver_case import DRIVER_BUDGET, driver_items
    E = _E()
    f3, f17, f129, f128 = driver_items()
    refused = _copy(f17)
    refused.N[0] = refused.n + 3
    run = [f3, f17, f129, f128]
    alone = [_single(fp) for fp in [refused] + run]
    assert alone[0][0] == E.ERR_ARG and alone[0][1] and [a[0] for a in alone[1:]] == [E.OPTIMAL] * 4
    _, one = _batch([f3])
    assert one["chunks"] == 1
    per_chunk = one["launches"]
    monkeypatch.setenv("ELLP_BATCH_MAX_BYTES", str(DRIVER_BUDGET))
    res, info = _batch([refused] + run, fill=-7.5)
    assert info["chunks"] >= 2
    assert info == {"launches": per_chunk * info["chunks"], "batched": 3, "single": 1, "chunks": info["chunks"]}
    st, y, d, r, k, msg = res[0]
    assert (st, msg) == alone[0][:2] and k is None and all((v == -7.5).all() for v in (y, d, r))  # untouched
    for pos, ((st, y, d, r, k, msg), a) in enumerate(zip(res[1:], alone[1:]), 1):
        assert st == E.OPTIMAL and msg == "", (pos, st, msg)
        _same_bits(("driver", pos), (y, d, r, k), a[2:])

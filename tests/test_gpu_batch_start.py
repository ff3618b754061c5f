"""ellp_batch_basis_start on the device: every output of every item is, as bytes, what ellp_basis_start returns for the item
alone — x, y, d, the labels and every field of ellp_start_info with its kkt, in both modes — at the edge shapes of
k_start_batch (rows 1, 2, 17, 63, 64, 65, 127, 128; nonbasic columns 1, 63, 64, 65, 129; one item with more than 2,048
nonbasic columns), with TwoSided variables under given Upper and Free labels, Free and Fixed kinds, afiro's optimal basis
(the singleton-row snap) and a basis on which x_B is refined; reversed, chunked, next to a singular item, next to a NaN and
next to an item of 129 rows that takes the single path inside the call.  The cases of tests/test_gpu_start.py that fit the
kernel are also held against the exact model of tests/start_model.py, with that file's tolerances: the geometry is the single
call's, so its chain lengths hold unchanged.

The items are built as tests/test_gpu_batch_postsolve.py builds its own (EDGES, _restrict), on bases advanced by a short
batched solve.
"""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import postsolve_model as PM  # noqa: E402
import start_cases as SC  # noqa: E402
import start_model as SM  # noqa: E402
from test_gpu_batch_postsolve import EDGES, _copy, _restrict, _synth  # noqa: E402

pytestmark = pytest.mark.gpu
U = SM.U
EPS = 1e-10
MODES = [0, 1]


def _E():
    from ellp_amd import _engine as E
    return E


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def refined_case():
    """a basis of tests/start_cases.py on which the single call refines x_B: adlittle's optimal basis (56 rows; one step, met on
    an MI355X in both modes — the tests that use it assert that first)"""
    return SC.flat_of(SC.oracle_optimum(SC.netlib("adlittle")))


_ITEMS = {}


def items():
    """[(label, FlatProblem)], n_c == n everywhere; the x of an item is never read"""
    if _ITEMS:
        return _ITEMS["fps"]
    E = _E()
    edge = [(f"edge-{m}x{nN}", _synth(m, max(nN - m, 8), seed=20260301 + m)) for m, nN in EDGES]
    more = [("wide-17x2117", _synth(17, 2100)), ("kinds-17", _synth(17, 30)), ("boxed-33", _synth(33, 40))]
    res = E.batch_solve_with_initial(E.ENGINE_PRIMAL, [fp for _, fp in edge + more], E.default_opts(max_iter=60))
    assert all(st >= 0 for st, _, _ in res), [(lab, st, msg) for (lab, _), (st, _, msg) in zip(edge + more, res) if st < 0]
    fps = [(label, _restrict(fp, nN)) for (label, fp), (m, nN) in zip(edge, EDGES)]
    label, fp = more[0]
    assert fp.nN > 2048 and fp.n_c == fp.n
    fps.append((label, _copy(fp)))
    # Free kinds under a Free label and Fixed kinds (as test_gpu_postsolve.test_free_labels_and_fixed_variables)
    label, fp = more[1]
    fp = _copy(fp)
    for j in range(0, fp.nN, 3):
        fp.kind[fp.N[j]] = 0
        fp.Nb[j] = 2
    for j in range(1, fp.nN, 3):
        fp.kind[fp.N[j]] = 4
    fps.append((label, fp))
    # TwoSided nonbasic variables: a given Upper, a given Free (becomes Lower), a given Lower, in turn; one basic too
    label, fp = more[2]
    fp = _copy(fp)
    for j in range(fp.nN):
        v = fp.N[j]
        fp.kind[v], fp.lb[v], fp.ub[v] = 3, -0.25 * (1 + j % 3), 0.5 + 0.125 * (j % 5)
        fp.Nb[j] = (1, 2, 0)[j % 3]
    v = fp.B[0]
    fp.kind[v], fp.lb[v], fp.ub[v] = 3, -1.0, 1.0
    fps.append((label, fp))
    fps.append(("afiro-optimal", SC.flat_of(SC.oracle_optimum(SC.netlib("afiro")))))
    fps.append(("refined-adlittle", refined_case()))
    assert all(fp.n_c == fp.n for _, fp in fps)
    _ITEMS["fps"] = fps
    return fps


_REF = {}


def ref(mode):
    """the single call's result of every item, once per mode"""
    if mode not in _REF:
        E = _E()
        _REF[mode] = [E.basis_start(_copy(fp), mode) for _, fp in items()]
        assert all(r[0] == E.OPTIMAL for r in _REF[mode])
    return _REF[mode]


def _same_info(tag, a, b):
    assert set(a) == set(b), (tag, set(a) ^ set(b))
    for key, vb in b.items():
        if isinstance(vb, dict):
            _same_info((tag, key), a[key], vb)
        elif isinstance(vb, float):
            assert _bits([a[key]])[0] == _bits([vb])[0], (tag, key, a[key], vb)
        else:
            assert a[key] == vb, (tag, key, a[key], vb)


def _same_bits(tag, got, want):
    """(status, x, y, d, Nb, info) against the same of the single call, as bytes"""
    assert got[0] == want[0], (tag, got[0], want[0], got[5].get("message"))
    for name, a, b in zip("xyd", got[1:4], want[1:4]):
        assert a.shape == b.shape and (_bits(a) == _bits(b)).all(), (tag, name, np.flatnonzero(_bits(a) != _bits(b))[:8])
    assert got[4].dtype == np.uint8 and (got[4] == want[4]).all(), (tag, "Nb")
    _same_info(tag, got[5], want[5])


def _batch(fps, mode, **kw):
    E = _E()
    res = E.batch_basis_start([_copy(fp) for fp in fps], mode, **kw)
    return res, E.batch_basis_start_info()


@pytest.mark.parametrize("mode", MODES)
def test_bits_equal_the_single_call(mode, monkeypatch):
    fps, want = items(), ref(mode)
    only = [fp for _, fp in fps]
    res, info = _batch(only, mode)
    assert info == {"launches": 2, "batched": len(only), "single": 0, "chunks": 1}
    for (label, _), got, w in zip(fps, res, want):
        _same_bits(label, got, w)
    print("x refinement steps:", {lab: w[5]["x_refinement_steps"] for (lab, _), w in zip(fps, want) if w[5]["x_refinement_steps"]},
          "labels changed:", sum(w[5]["labels_changed"] for w in want))
    # three items: the same two launches
    res3, info3 = _batch(only[:3], mode)
    assert info3 == {"launches": 2, "batched": 3, "single": 0, "chunks": 1}
    # reversed
    resr, _ = _batch(only[::-1], mode)
    for (label, _), got, w in zip(fps[::-1], resr, want[::-1]):
        _same_bits(("reversed", label), got, w)
    # chunked by the budget
    monkeypatch.setenv("ELLP_BATCH_MAX_BYTES", str(1 << 20))
    resc, infoc = _batch(only, mode)
    assert infoc["chunks"] >= 3 and infoc["launches"] == 2 * infoc["chunks"] and infoc["batched"] == len(only) and infoc["single"] == 0
    for (label, _), got, w in zip(fps, resc, want):
        _same_bits(("chunked", label), got, w)


def test_the_content_cases_are_what_they_claim():
    """the labels the repair changes, the snap and the refinement are really met (conditions of this file's cases)"""
    fps = dict(items())
    want = dict(zip((lab for lab, _ in items()), ref(0)))
    boxed = fps["boxed-33"]
    assert sorted(set(boxed.Nb.tolist())) == [0, 1, 2]
    got = want["boxed-33"]
    assert got[4].tolist() == [(1, 0, 0)[j % 3] for j in range(boxed.nN)]           # Upper kept, Free -> Lower
    assert got[5]["labels_changed"] == sum(1 for j in range(boxed.nN) if j % 3 == 1)
    assert all(got[1][boxed.N[j]] == (boxed.ub if j % 3 == 0 else boxed.lb)[boxed.N[j]] for j in range(boxed.nN))
    kinds = fps["kinds-17"]
    assert {0, 4} <= set(kinds.kind[kinds.N].tolist())
    afiro = fps["afiro-optimal"]
    A_B = afiro.A.reshape(afiro.n, afiro.m)[afiro.B].T
    assert ((A_B != 0).sum(axis=1) == 1).any()                                      # a singleton row: the snap acts
    assert want["refined-adlittle"][5]["x_refinement_steps"] >= 1                        # the x loop runs on the single call
    assert dict(zip((lab for lab, _ in items()), ref(1)))["refined-adlittle"][5]["x_refinement_steps"] >= 1


@pytest.mark.parametrize("mode", MODES)
def test_x_refinement_runs_on_the_device(mode):
    E = _E()
    fps, want = items(), ref(mode)
    k = [lab for lab, _ in fps].index("refined-adlittle")
    assert want[k][5]["x_refinement_steps"] >= 1  # the condition of this test, on the single call first
    res, _ = _batch([fps[0][1], fps[k][1], fps[1][1]], mode)
    assert [r[0] for r in res] == [E.OPTIMAL] * 3
    assert res[1][5]["x_refinement_steps"] == want[k][5]["x_refinement_steps"]
    _same_bits("refined", res[1], want[k])
    _same_bits("before", res[0], want[0])
    _same_bits("after", res[2], want[1])


@pytest.mark.parametrize("mode", MODES)
def test_a_singular_item_is_isolated(mode):
    E = _E()
    fps, want = items(), ref(mode)
    import test_gpu_start as TS
    good = [fp for _, fp in fps[:6]]
    # the singular basis of tests/test_gpu_start.py: two columns proportional by a power of two in dyadic data, so that the
    # elimination meets an exact zero pivot; labels the repair would change
    c = TS._seventeen()
    c["A"][:, c["B"][5]] = 2.0 * c["A"][:, c["B"][2]]
    c["Nb"] = np.array([2, 2, 2], dtype=np.uint8)
    singular = TS._fp(c)
    alone = E.basis_start(_copy(singular), mode)
    assert alone[0] == E.ERR_SINGULAR and alone[5]["message"]
    mixed = good[:3] + [singular] + good[3:]
    res, info = _batch(mixed, mode, fill=-7.5)
    assert info["batched"] == len(mixed) and info["launches"] == 2  # the singular one reaches the kernel
    st, x, y, d, Nb, inf = res[3]
    assert st == E.ERR_SINGULAR and inf == {"message": alone[5]["message"]}
    assert all((v == -7.5).all() for v in (x, y, d)) and (Nb == singular.Nb).all()  # untouched
    for k, (got, w) in enumerate(zip(res[:3] + res[4:], want[:6])):
        _same_bits(("mixed", k), got, w)


@pytest.mark.parametrize("mode", MODES)
def test_a_nan_in_b_changes_no_other_item(mode):
    E = _E()
    fps, want = items(), ref(mode)
    nan = _copy(fps[2][1])
    nan.b[1] = np.nan
    alone = E.basis_start(_copy(nan), mode)
    assert alone[0] == E.OPTIMAL and alone[5]["primal_feasible"] == 0 and np.isnan(alone[5]["primal_infeasibility"])
    res, _ = _batch([fps[0][1], nan, fps[1][1]], mode)
    _same_bits("nan", res[1], alone)
    _same_bits("before", res[0], want[0])
    _same_bits("after", res[2], want[1])


@pytest.mark.parametrize("mode", MODES)
def test_an_item_of_129_rows_takes_the_single_path(mode):
    E = _E()
    fps, want = items(), ref(mode)
    big = _synth(129, 40)
    s, _, msg = E.primal_solve_with_initial(big, E.default_opts(max_iter=40))
    assert s >= 0, (s, msg)
    assert big.m == 129 and big.n_c == big.n
    alone = E.basis_start(_copy(big), mode)
    assert alone[0] == E.OPTIMAL
    res, info = _batch([fps[0][1], big, fps[1][1]], mode)
    assert info == {"launches": 2, "batched": 2, "single": 1, "chunks": 1}
    _same_bits("129 rows", res[1], alone)
    _same_bits("before", res[0], want[0])
    _same_bits("after", res[2], want[1])


def test_against_exact_model():
    """the batch's own outputs against the exact model, for the cases of tests/test_gpu_start.py of at most 128 rows, with
    that file's tolerances"""
    import test_gpu_start as TS
    E = _E()
    names = [n for n in TS.CASES if not n.startswith("513")]
    cases = {n: TS.CASES[n][0]() for n in names}
    got = {}
    for mode in MODES:
        sel = [n for n in names if TS.CASES[n][1] == mode]
        res, info = _batch([TS._fp(cases[n]) for n in sel], mode)
        assert info["batched"] == len(sel) and info["single"] == 0
        got.update(zip(sel, res))
    for name in names:
        c, mode = cases[name], TS.CASES[name][1]
        m, n = c["m"], c["n"]
        A, B, N = c["A"], [int(v) for v in c["B"]], [int(v) for v in c["N"]]
        mod = SM.Start(c["A"], c["c"], c["b"], c["kind"], c["lb"], c["ub"], c["B"], c["N"], c["Nb"], mode)
        if mode == 1 and mod.min_twosided_d is not None:
            assert mod.min_twosided_d > Fraction(1, 10 ** 6), (name, float(mod.min_twosided_d))
        assert all(mod.far_from(EPS)), name
        s, x, y, d, Nb, info = got[name]
        assert s == E.OPTIMAL, (name, info)
        kkt = info["kkt"]
        assert [int(k) for k in Nb] == mod.labels and info["labels_changed"] == mod.labels_changed, name
        for v in N:
            assert x[v] == float(mod.x[v]), (name, "x_N", v)
        assert kkt["y_backward_error"] <= 2 * U and info["x_backward_error"] <= 2 * U, name
        assert 0 <= kkt["refinement_steps"] <= 4 and 0 <= info["x_refinement_steps"] <= 4
        # omega_x of the returned x, exactly
        kd, kr = PM.chain_lengths(m, len(N))
        wx = mod.omega_x(x)
        gm, gr = Fraction(PM.gamma(m + 1)), Fraction(PM.gamma(kr))
        tol_w = wx * (3 * Fraction(U) + 2 * gm) + 2 * gr * gr + Fraction(U)
        assert abs(Fraction(info["x_backward_error"]) - wx) <= tol_w, (name, info["x_backward_error"] / U, float(wx) / U)
        # d of the returned y within the postsolve's entry bound
        fp = TS._fp(c)
        fp.x, fp.Nb = x.copy(), Nb.copy()
        ex = PM.Exact.of(fp, y)
        big_d = Fraction(0)
        for v in range(n):
            e, S = ex.d(v)
            bound = PM.entry_bound(e, S, kd)
            big_d = max(big_d, bound)
            assert abs(Fraction(float(d[v])) - e) <= bound, (name, "d", v)
        # the measures: the definitions on the returned arrays, bit for bit, and the model's within tol_x / tol_d
        viol = [SM.violation_f64(int(c["kind"][v]), float(c["lb"][v]), float(c["ub"][v]), float(x[v])) for v in B]
        pinf, wp = SM.nanmax_first(viol, B)
        assert _bits([info["primal_infeasibility"]])[0] == _bits([pinf])[0] and info["worst_primal_var"] == wp, name
        A_B = A[:, B]
        inv = np.abs(np.linalg.inv(A_B))
        t_abs = np.array([float(abs(q)) for q in mod.t])
        xB_abs = np.array([float(abs(mod.x[v])) for v in B])
        tol_x = 2.0 * float((inv @ (4 * U * (t_abs + np.abs(A_B) @ xB_abs))).max())
        for i, v in enumerate(B):
            assert abs(x[v] - float(mod.x[v])) <= tol_x + U * abs(float(mod.x[v])), (name, "x_B", i)
        assert abs(info["primal_infeasibility"] - float(mod.primal_infeasibility)) <= tol_x + U * float(mod.primal_infeasibility), name
        assert abs(info["primal_infeasibility_sum"] - float(mod.primal_infeasibility_sum)) <= m * tol_x + 2 * U * float(mod.primal_infeasibility_sum), name
        y_abs = np.array([float(abs(q)) for q in mod.y])
        tol_y = 2.0 * (inv.T @ (4 * U * (np.abs(c["c"][B]) + np.abs(A_B).T @ y_abs)))
        tol_d = float((np.abs(A).T @ tol_y).max()) + float(big_d)
        assert abs(info["dual_infeasibility"] - float(mod.dual_infeasibility)) <= tol_d + U * float(mod.dual_infeasibility), name
        assert (info["primal_feasible"], info["dual_feasible"]) == mod.flags(EPS), (name, info, mod.flags(EPS))


def test_refusal_chunks_and_single_path_in_one_call(monkeypatch):
    """a refused item, two batched items (3 and 17 rows), one of 129 rows on the single path and one more batched item of
    128 rows, cut into chunks by the budget: every branch of the batched calls' shared chunk driver in one call (LABELS_BY_D)"""
    from batch_driver_case import DRIVER_BUDGET, driver_items
    E = _E()
    mode = 1
    f3, f17, f129, f128 = driver_items()
    refused = _copy(f17)
    refused.N[0] = refused.n + 3
    run = [f3, f17, f129, f128]
    alone = [E.basis_start(_copy(fp), mode) for fp in [refused] + run]
    assert alone[0][0] == E.ERR_ARG and alone[0][5]["message"] and [a[0] for a in alone[1:]] == [E.OPTIMAL] * 4
    monkeypatch.setenv("ELLP_BATCH_MAX_BYTES", str(DRIVER_BUDGET))
    res, info = _batch([refused] + run, mode, fill=-7.5)
    assert info["chunks"] >= 2
    assert info == {"launches": 2 * info["chunks"], "batched": 3, "single": 1, "chunks": info["chunks"]}
    st, x, y, d, Nb, inf = res[0]
    assert st == E.ERR_ARG and inf == {"message": alone[0][5]["message"]}
    assert all((v == -7.5).all() for v in (x, y, d)) and (Nb == refused.Nb).all()  # untouched
    for pos, (got, a) in enumerate(zip(res[1:], alone[1:]), 1):
        assert got[5]["message"] == "", (pos, got[5])
        _same_bits(("driver", pos), got, a)

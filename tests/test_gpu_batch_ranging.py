"""ellp_batch_ranging on the device: every output of every item is, bit for bit (any NaN equal to any NaN), what ellp_ranging
returns for the item alone — on the items of tests/test_gpu_batch_postsolve.py and at the edge shapes of the ranging's own
kernels (rows 1, 2, 15, 16, 17, 63, 64, 65, 127, 128: odd m for the double2 clamp of the tableau pass, m no multiple of 4 or
of 16 for its k fill, the 16-row blocks of k_brange_solve and the 64-row tiles of inverse_residual; nonbasic columns 1, 15, 16,
17, 127, 128, 129, 257: the fragment and column-block edges, and three blocks to fold), on points of both engine kinds, with
n_c > n, Free labels, Fixed kinds and slack-heavy bases (singleton basic columns: the snap runs), reversed, chunked, next to
failing items and next to a NaN.  From the returned W the right-hand-side limits and inverse_residual equal the definitions
of tests/ranging_model.py bit for bit, and at the two optima of test_gpu_ranging.py's meaning test every finite limit holds in
exact arithmetic.

What is independent of what: the single call and the batch run the same device functions (range_solve_rows, range_tab_tile,
range_resid_tile, ...), so the bit-equality tests show that the batch's plumbing — tables, slab, geometry, snap, fold —
changes nothing, not that those functions are right.  That rests on tests/ranging_model.py: on test_gpu_ranging.py for the
single call, and here on the definition tests from the returned W and on the exact-arithmetic meaning test."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ranging_model as RM  # noqa: E402
from test_gpu_batch_postsolve import _E, _copy, _restrict, _synth, items as post_items  # noqa: E402
from test_gpu_postsolve import _primal_fp  # noqa: E402
from test_gpu_ranging import ARR, _mat, _same  # noqa: E402

pytestmark = pytest.mark.gpu

# (rows, nonbasic columns) besides those of test_gpu_batch_postsolve.EDGES: with them every row count and every column
# count of the docstring at least once
MORE = [(15, 15), (16, 16), (1, 17), (16, 127), (2, 128), (15, 257), (63, 257), (128, 257), (127, 128), (128, 16), (64, 15),
        (65, 17), (17, 1)]
_ITEMS = {}


def items():
    """[(label, FlatProblem)] and, once, the single call's Ranging of each"""
    if _ITEMS:
        return _ITEMS["fps"], _ITEMS["ref"]
    E = _E()
    fps = list(post_items()[0])
    more = [(f"more-{m}x{nN}", _synth(m, max(nN, 8), seed=20260401 + 131 * m + nN)) for m, nN in MORE]
    res = E.batch_solve_with_initial(E.ENGINE_PRIMAL, [fp for _, fp in more], E.default_opts(max_iter=60))
    assert all(st >= 0 for st, _, _ in res)
    fps += [(label, _restrict(fp, nN)) for (label, fp), (m, nN) in zip(more, MORE)]
    # slack-heavy bases: a starting basis (every basic column has a single nonzero) and bases a few pivots away from one
    fps.append(("start-17", _synth(17, 30)))
    few = [(f"few-{m}-{it}", _synth(m, n, seed=20260501 + m), it) for m, n, it in ((17, 30, 3), (64, 64, 10), (65, 129, 20), (128, 100, 30))]
    for label, fp, it in few:
        st = E.batch_solve_with_initial(E.ENGINE_PRIMAL, [fp], E.default_opts(max_iter=it))[0][0]
        assert st >= 0
        fps.append((label, fp))
    mixed = 0
    for _, fp in fps[-5:]:
        nz = (_mat(fp)[:, fp.B] != 0).sum(axis=0)
        mixed += bool((nz == 1).any() and (nz > 1).any())
    assert mixed >= 2, "no basis with both singleton and other basic columns"
    assert {fp.m for _, fp in fps} >= {1, 2, 15, 16, 17, 63, 64, 65, 127, 128}
    assert {fp.nN for _, fp in fps} >= {1, 15, 16, 17, 127, 128, 129, 257}
    assert any(fp.n_c > fp.n for _, fp in fps) and any((fp.Nb[:fp.nN] == 2).any() for _, fp in fps)
    assert any((fp.kind[fp.N[:fp.nN]] == 4).any() for _, fp in fps)
    ref = [E.ranging(_copy(fp)) for _, fp in fps]
    _ITEMS["fps"], _ITEMS["ref"] = fps, ref
    return fps, ref


def _same_rg(tag, got, ref):
    """every array of ARR, y, inverse_residual and every KKT field"""
    for name in ARR + ("y",):
        a, b = getattr(got, name), getattr(ref, name)
        assert a.shape == b.shape and _same(a, b), (tag, name)
    assert _same([got.inverse_residual], [ref.inverse_residual]), (tag, got.inverse_residual, ref.inverse_residual)
    assert set(got.kkt) == set(ref.kkt)
    for key, val in ref.kkt.items():
        assert _same([got.kkt[key]], [val]) if isinstance(val, float) else got.kkt[key] == val, (tag, key, got.kkt[key], val)


def _batch(fps, **kw):
    E = _E()
    res = E._batch_ranging_raw([_copy(fp) for fp in fps], **kw)
    return res, E.batch_ranging_info()


def test_bits_equal_the_single_call(monkeypatch):
    E = _E()
    fps, ref = items()
    only = [fp for _, fp in fps]
    res, info = _batch(only)
    assert info["batched"] == len(only) and info["single"] == 0 and info["chunks"] == 1
    per_chunk = info["launches"] // info["chunks"]
    assert info["launches"] == per_chunk * info["chunks"] and 1 <= per_chunk <= 8
    for (label, _), (st, rg, W, msg), rf in zip(fps, res, ref):
        assert st == E.OPTIMAL and msg == "" and W is None, (label, st, msg)
        _same_rg(label, rg, rf)
    # three items: the same launches per chunk
    res3, info3 = _batch(only[:3])
    assert (info3["launches"], info3["batched"], info3["chunks"]) == (per_chunk, 3, 1)
    # reversed
    resr, _ = _batch(only[::-1])
    for (label, _), (st, rg, W, msg), rf in zip(fps[::-1], resr, ref[::-1]):
        assert st == E.OPTIMAL, (label, st, msg)
        _same_rg(("reversed", label), rg, rf)
    # chunked by the budget
    monkeypatch.setenv("ELLP_BATCH_MAX_BYTES", str(1 << 20))
    resc, infoc = _batch(only)
    assert infoc["chunks"] >= 3 and infoc["launches"] == per_chunk * infoc["chunks"] and infoc["batched"] == len(only)
    for (label, _), (st, rg, W, msg), rf in zip(fps, resc, ref):
        assert st == E.OPTIMAL, (label, st, msg)
        _same_rg(("chunked", label), rg, rf)


def test_by_definition_from_the_returned_inverse():
    E = _E()
    fps, ref = items()
    chosen = [(lab, fp) for lab, fp in fps if lab.startswith(("edge-", "more-", "start-", "few-")) or lab == "free-and-fixed"]
    assert len(chosen) >= 25
    eps = E.default_opts().eps
    res, _ = _batch([fp for _, fp in chosen], want_W=True)
    for (label, fp), (st, rg, W, msg) in zip(chosen, res):
        assert st == E.OPTIMAL and W.shape == (fp.m, fp.m), (label, st, msg)
        want = RM.rhs_ranging_f64(W, fp.x, fp.B, fp.kind, fp.lb, fp.ub, eps)
        for got, w, what in zip((rg.rhs_down, rg.rhs_up, rg.rhs_blocking_down, rg.rhs_blocking_up), want, ARR[4:8]):
            assert _same(got, w), (label, what)
        res_want = RM.inverse_residual_f64(_mat(fp)[:, fp.B], W)
        assert _same([rg.inverse_residual], [res_want]), (label, rg.inverse_residual, res_want)
        assert (rg.cost_down <= 0).all() and (rg.cost_up >= 0).all() and (rg.rhs_down <= 0).all() and (rg.rhs_up >= 0).all()
    # one case built both ways: W's rows are the single engine path's rho, and the costs follow from its tableau rows
    for want_label in ("more-63x257", "few-64-10"):
        k = [lab for lab, _ in chosen].index(want_label)
        fp, (st, rg, W, msg) = chosen[k][1], res[k]
        eng = E.Engine(E.ENGINE_PRIMAL, _copy(fp), E.default_opts(max_iter=None))
        try:
            alpha, rho = eng.tableau_rows(np.arange(fp.m))
        finally:
            eng.close()
        assert _same(W, rho), want_label
        N, Nb = fp.N[:fp.nN], fp.Nb[:fp.nN]
        cost = RM.cost_ranging_f64(alpha, rg.d, fp.B, N, Nb, fp.kind, fp.n, fp.n_c, eps)
        for got, w, what in zip((rg.cost_down, rg.cost_up, rg.cost_blocking_down, rg.cost_blocking_up), cost, ARR[:4]):
            assert _same(got, w), (want_label, what)


def test_meaning_at_the_optimum():
    E = _E()
    fps = [_primal_fp(17, 30), _primal_fp(50, 120)]
    res = E.batch_solve_with_initial(E.ENGINE_PRIMAL, fps, E.default_opts(max_iter=100000))
    assert [st for st, _, _ in res] == [E.OPTIMAL] * 2, res
    eps = E.default_opts().eps
    out, _ = _batch(fps)
    for fp, (st, rg, W, msg) in zip(fps, out):
        assert st == E.OPTIMAL, (st, msg)
        name = f"{fp.m}x{fp.nN}"
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


def _single(fp):
    E = _E()
    try:
        return E.OPTIMAL, "", E.ranging(_copy(fp))
    except E.EllpHipError as e:
        return e.status, e.msg, None


def _untouched(rg, W, fill):
    return all((getattr(rg, name) == (int(fill) if getattr(rg, name).dtype == np.int64 else fill)).all() for name in rg.ARRAYS) and \
        (W is None or (W == fill).all())


def test_failing_items_are_isolated():
    E = _E()
    fps, ref = items()
    good = [fp for _, fp in fps[:9]]
    singular, index, nothing = _copy(good[3]), _copy(good[4]), _copy(good[5])
    singular.B[1] = singular.B[0]  # a repeated column
    index.N[0] = index.n + 3
    alone = [_single(singular), _single(index)]
    assert [a[0] for a in alone] == [E.ERR_SINGULAR, E.ERR_ARG] and all(a[1] for a in alone)
    mixed = good[:2] + [singular] + good[2:5] + [index, nothing] + good[5:]
    at = (2, 6, 7)
    wanted = [None] * len(mixed)
    wanted[7] = []
    E = _E()
    res = E._batch_ranging_raw([_copy(fp) for fp in mixed], want_W=False, fill=-7.5, wanted=wanted)
    info = E.batch_ranging_info()
    assert info["batched"] == len(good) + 1  # the singular one reaches the kernels
    for pos, a in zip(at[:2], alone):
        st, rg, W, msg = res[pos]
        assert (st, msg) == a[:2]
        assert _untouched(rg, W, -7.5)
    st, rg, W, msg = res[7]
    assert st == E.ERR_ARG and "nothing is wanted" in msg and _untouched(rg, W, -7.5)
    rest = [res[k] for k in range(len(mixed)) if k not in at]
    for k, ((st, rg, W, msg), rf) in enumerate(zip(rest, ref[:9])):
        assert st == E.OPTIMAL and msg == ""
        _same_rg(("mixed", k), rg, rf)
    # the singular item with W asked for: W stays as it was too
    res2, _ = _batch([good[0], singular, good[1]], want_W=True, fill=-7.5)
    assert res2[1][0] == E.ERR_SINGULAR and _untouched(res2[1][1], res2[1][2], -7.5)
    _same_rg("before", res2[0][1], ref[0])
    _same_rg("after", res2[2][1], ref[1])


def test_nan_in_a_basic_entry():
    E = _E()
    fps, ref = items()
    k = [lab for lab, _ in fps].index("more-63x257")
    clean, nan = fps[k][1], _copy(fps[k][1])
    eps = E.default_opts().eps
    (_, _, W, _), = _batch([clean], want_W=True)[0]
    i = int(np.argmax((np.abs(W) > eps).sum(axis=1)))  # the basic position most rows read
    v = int(nan.B[i])
    assert int(nan.kind[v]) != 0
    nan.x[v] = np.nan
    alone = E.ranging(_copy(nan))
    res, _ = _batch([fps[0][1], nan, fps[1][1]])
    assert [st for st, *_ in res] == [E.OPTIMAL] * 3
    rg = res[1][1]
    reads = np.abs(W[i]) > eps
    assert reads.any()
    assert np.isnan(rg.rhs_up[reads]).all() and np.isnan(rg.rhs_down[reads]).all()
    assert (rg.rhs_blocking_up[reads] == v).all() and (rg.rhs_blocking_down[reads] == v).all()
    want = RM.rhs_ranging_f64(W, nan.x, nan.B, nan.kind, nan.lb, nan.ub, eps)
    for got, w in zip((rg.rhs_down, rg.rhs_up, rg.rhs_blocking_down, rg.rhs_blocking_up), want):
        assert _same(got, w)
    _same_rg("nan", rg, alone)
    _same_rg("before", res[0][1], ref[0])
    _same_rg("after", res[2][1], ref[1])


def test_large_items_take_the_single_path():
    E = _E()
    fps, ref = items()
    big = _synth(129, 140)
    s, _, msg = E.primal_solve_with_initial(big, E.default_opts(max_iter=40))
    assert s >= 0 and big.m == 129, (s, msg)
    alone = E.ranging(_copy(big))
    res, info = _batch([fps[0][1], big, fps[1][1]], want_W=True)
    assert (info["batched"], info["single"]) == (2, 1)
    assert [st for st, *_ in res] == [E.OPTIMAL] * 3
    _same_rg("big", res[1][1], alone)
    assert _same([RM.inverse_residual_f64(_mat(big)[:, big.B], res[1][2])], [alone.inverse_residual])  # W is the single path's
    _same_rg("before", res[0][1], ref[0])
    _same_rg("after", res[2][1], ref[1])


def test_same_bits_twice():
    fps, _ = items()
    only = [fp for _, fp in fps[::4]]
    a, _ = _batch(only, want_W=True)
    b, _ = _batch(only, want_W=True)
    for (sa, ra, Wa, _), (sb, rb, Wb, _) in zip(a, b):
        assert sa == sb
        for name in ra.ARRAYS:
            assert getattr(ra, name).tobytes() == getattr(rb, name).tobytes(), name
        assert Wa.tobytes() == Wb.tobytes()
        assert np.float64(ra.inverse_residual).tobytes() == np.float64(rb.inverse_residual).tobytes()


def test_refusal_chunks_and_single_path_in_one_call(monkeypatch):
    """a refused item, two batched items (3 and 17 rows), one of 129 rows on the single path and one more batched item of
    128 rows, cut into chunks by the budget: every branch of the batched calls' shared chunk driver in one call"""
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
    st, rg, W, msg = res[0]
    assert (st, msg) == alone[0][:2] and _untouched(rg, W, -7.5)
    for pos, ((st, rg, W, msg), a) in enumerate(zip(res[1:], alone[1:]), 1):
        assert st == E.OPTIMAL and msg == "", (pos, st, msg)
        _same_rg(("driver", pos), rg, a[2])

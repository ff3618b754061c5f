"""CPU-side checks of the batch's mid-size items (129 to 1,024 rows, k_mid_batch): which items pass the per-item checks
and which are refused, with their own status and a message naming the limit.  These checks run before any HIP call, so on
a machine without a device a call whose items passed them fails as a whole with ELLP_ERR_DEVICE; on an MI355X it solves."""
import ctypes as C

import numpy as np

from ellp_amd import _engine as E
from test_batch_cpu import _item


def _wide_item(m, nN):
    """a primal LP of m rows and nN all-zero nonbasic columns (identity basis on the last m columns), built without touching
    the zero pages of its matrix"""
    n = m + nN
    A = np.zeros(m * n)  # column-major; only the basis columns are written
    A[nN * m + np.arange(m) * (m + 1)] = 1.0
    return E.FlatProblem(m, n, n, A, np.ones(n), np.ones(m), np.zeros(n, np.uint8), np.zeros(n), np.full(n, np.inf),
                         np.r_[np.zeros(nN), np.ones(m)], np.arange(nN, n), np.arange(nN), np.zeros(nN, np.uint8))


def _raw(kind, fps, opts):
    """the C call itself: the status of the call and every item's status and message, also where the call fails"""
    n = len(fps)
    items = (E.BatchItem * n)()
    for it, fp in zip(items, fps):
        it.m, it.n, it.n_c = fp.m, fp.n, fp.n_c
        it.A, it.c, it.b, it.bound_kind = E._p(fp.A), E._p(fp.c), E._p(fp.b), E._p(fp.kind)
        it.lb, it.ub, it.x = E._p(fp.lb), E._p(fp.ub), E._p(fp.x)
        it.B_index, it.n_B = E._p(fp.B), fp.nB
        it.N_index, it.N_bound, it.n_N = E._p(fp.N), E._p(fp.Nb), fp.nN
        it.y, it.d = E._p(fp.y), E._p(fp.d)
    status = (C.c_int * n)()
    stats = (E.Stats * n)()
    err = C.create_string_buffer(512)
    s = E.lib().ellp_batch_solve_with_initial(kind, n, items, C.byref(opts), status, stats, err, 512)
    return s, [(status[k], items[k].err.decode()) for k in range(n)]


def test_pipeline3_mid_item_passes_the_item_checks():
    try:
        r = E.batch_solve_with_initial(E.ENGINE_PRIMAL, [_item(129, 4)], E.default_opts(pipeline=3, max_iter=50))
    except E.EllpHipError as e:
        assert e.status == E.ERR_DEVICE, (e.status, e.msg)  # no device: the call got past the item's checks
    else:
        assert r[0][0] != E.ERR_ARG, r[0]  # solved on k_mid_batch
        assert r[0][1].iters > 0


def test_mid_items_refused_with_their_limit():
    small, tall, wide, mid = _item(3, 2), _item(1025, 4), _wide_item(129, 4096 * 64 + 1), _item(160, 3)
    x_tall, x_wide = tall.x.copy(), wide.x.copy()
    s, res = _raw(E.ENGINE_PRIMAL, [small, tall, mid, wide], E.default_opts(pipeline=3, max_iter=50))
    assert s in (E.OPTIMAL, E.ERR_DEVICE)
    (s_small, m_small), (s_tall, m_tall), (s_mid, m_mid), (s_wide, m_wide) = res
    assert s_tall == E.ERR_ARG and "1024 rows" in m_tall and "1025" in m_tall, m_tall
    assert s_wide == E.ERR_ARG and "150 KB" in m_wide and "262145" in m_wide, m_wide
    # the neighbours passed their checks (and, with a device, solved)
    assert s_small != E.ERR_ARG and s_mid != E.ERR_ARG, (m_small, m_mid)
    assert tall.x.tobytes() == x_tall.tobytes() and wide.x.tobytes() == x_wide.tobytes()  # untouched


def test_mid_item_under_default_options_is_refused():
    # a single call runs 129 rows on the certified hybrid by default: the batch does not take it
    r = E.batch_solve_with_initial(E.ENGINE_PRIMAL, [_item(129, 4)])
    assert r[0][0] == E.ERR_ARG and "129" in r[0][2] and "ELLP_MID_AUTO_MAX" in r[0][2]


def test_mid_auto_max_selects_the_batch(monkeypatch):
    monkeypatch.setenv("ELLP_MID_AUTO_MAX", "200")
    s, res = _raw(E.ENGINE_PRIMAL, [_item(168, 4), _item(336, 4)], E.default_opts(max_iter=50))
    assert s in (E.OPTIMAL, E.ERR_DEVICE)
    assert res[0][0] != E.ERR_ARG, res[0]
    assert res[1][0] == E.ERR_ARG and "336" in res[1][1], res[1]


def test_dual_mid_item_needs_y_and_d():
    for kw in (dict(pipeline=3), dict(flags=E.FLAG_DUAL_BOUND_FLIPPING)):
        r = E.batch_solve_with_initial(E.ENGINE_DUAL, [_item(200, 4)], E.default_opts(**kw))
        assert r[0][0] == E.ERR_ARG and "y and d" in r[0][2], kw

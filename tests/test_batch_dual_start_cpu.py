"""CPU-side checks of ellp_batch_dual_phase1_start (the dual's phase-1 starting points of many LPs in one call): the header
declares it, the call's own argument checks, and the per-item checks that run before any HIP call (so on a machine without
a device a call whose items all fail them returns ELLP_OPTIMAL with every item's status and message)."""
import ctypes as C
import os
import re

import numpy as np

from ellp_amd import _engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _box(m, n):
    """a box problem (every variable two-sided) with an identity basis on the last m columns (only the basis columns of A
    are nonzero)"""
    A = np.zeros(m * n)
    A[(n - m) * m + np.arange(m) * (m + 1)] = 1.0
    return (m, n, A, np.ones(n), np.zeros(m), np.full(n, 3, np.uint8), np.zeros(n), np.ones(n),
            np.arange(n - m, n), np.arange(n - m))


def _raw(problems, opts, count=None, items_null=False, status_null=False):
    n = len(problems)
    items = (E.BatchItem * max(n, 1))()
    keep = []
    for it, (m, nn, A, c, b, kind, lb, ub, B, N) in zip(items, problems):
        arrs = [np.ascontiguousarray(a) for a in (A, c, b, kind, lb, ub)] + [np.ascontiguousarray(B, np.int64),
                                                                             np.ascontiguousarray(N, np.int64)]
        outs = [np.zeros(max(nn, 1)), np.zeros(max(nn - m, 1), np.uint8), np.zeros(max(m, 1)), np.zeros(max(nn, 1))]
        keep += arrs + outs
        it.m, it.n, it.n_c = m, nn, nn
        it.A, it.c, it.b, it.bound_kind, it.lb, it.ub = (E._p(a) for a in arrs[:6])
        it.B_index, it.n_B, it.N_index, it.n_N = E._p(arrs[6]), m, E._p(arrs[7]), nn - m
        it.x, it.N_bound, it.y, it.d = (E._p(a) for a in outs)
    status = (C.c_int * max(n, 1))()
    obj = (C.c_double * max(n, 1))()
    err = C.create_string_buffer(512)
    s = E.lib().ellp_batch_dual_phase1_start(n if count is None else count, None if items_null else items, C.byref(opts),
                                             None if status_null else status, obj, err, 512)
    return s, [(status[k], items[k].err.decode()) for k in range(n)], err.value.decode()


def test_header_declares_the_batched_start():
    hdr = open(os.path.join(ROOT, "include", "ellp_hip.h")).read()
    assert re.search(r"ellp_status\s+ellp_batch_dual_phase1_start\(\s*int64_t count,\s*ellp_batch_item \*items,\s*"
                     r"const ellp_opts \*opts,\s*ellp_status \*status_out,\s*double \*obj_out,\s*char \*errbuf,\s*size_t errlen\)",
                     hdr)
    assert "#define ELLP_HIP_ABI_VERSION 1" in hdr


def test_call_arguments_checked():
    o = E.default_opts(pipeline=3)
    s, _, msg = _raw([_box(3, 5)], o, count=-1)
    assert s == E.ERR_ARG and "count < 0" in msg
    s, _, msg = _raw([_box(3, 5)], o, items_null=True)
    assert s == E.ERR_ARG and "NULL" in msg
    s, _, msg = _raw([_box(3, 5)], o, status_null=True)
    assert s == E.ERR_ARG and "NULL" in msg
    s, _, msg = _raw([], o)
    assert s == E.OPTIMAL and msg == ""  # nothing to do: no HIP call


def test_items_refused_with_their_own_status():
    o = E.default_opts(pipeline=3)
    tall, square, no_nonbasic = _box(1025, 1030), _box(4, 4), _box(5, 3)
    s, res, _ = _raw([tall, square, no_nonbasic], o)
    assert s == E.OPTIMAL  # every item failed its checks before any HIP call
    (s_tall, m_tall), (s_sq, m_sq), (s_nn, m_nn) = res
    assert s_tall == E.ERR_ARG and "1025" in m_tall and "1024 rows" in m_tall, m_tall
    assert s_sq == E.ERR_ARG and "n > m" in m_sq, m_sq
    assert s_nn == E.ERR_ARG and "n > m" in m_nn, m_nn


def test_item_with_null_array_refused():
    o = E.default_opts(pipeline=3)
    m, n, A, c, b, kind, lb, ub, B, N = _box(3, 6)
    items = (E.BatchItem * 1)()
    it = items[0]
    it.m, it.n, it.n_c = m, n, n
    it.A, it.c, it.b, it.bound_kind, it.lb, it.ub = E._p(A), None, E._p(b), E._p(kind), E._p(lb), E._p(ub)
    B, N = np.ascontiguousarray(B, np.int64), np.ascontiguousarray(N, np.int64)
    it.B_index, it.n_B, it.N_index, it.n_N = E._p(B), m, E._p(N), n - m
    st = (C.c_int * 1)()
    s = E.lib().ellp_batch_dual_phase1_start(1, items, C.byref(o), st, None, None, 0)
    assert s == E.OPTIMAL and st[0] == E.ERR_ARG and "bad arguments" in items[0].err.decode()


def test_default_options_above_128_rows_refused():
    """the single call starts these on the certified hybrid, from an LU: not the batch's arithmetic"""
    s, res, _ = _raw([_box(200, 260)], E.default_opts())
    assert s == E.OPTIMAL
    assert res[0][0] == E.ERR_ARG and "explicit-inverse" in res[0][1], res[0]


def test_bound_flipping_with_an_explicit_inverse_pipeline_refused():
    s, _, msg = _raw([_box(3, 5)], E.default_opts(pipeline=1, flags=E.FLAG_DUAL_BOUND_FLIPPING))
    assert s == E.ERR_ARG and "BOUND_FLIPPING" in msg

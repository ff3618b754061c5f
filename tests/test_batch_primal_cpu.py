"""CPU-side checks of the whole-solve batched primal call (ellp_batch_primal_solve): the symbol is exported, and the
argument checks answer before any HIP call — on a machine without a device, a call that reached one would return
ELLP_ERR_DEVICE instead."""
import ctypes as C

import numpy as np

from ellp_amd import _engine as E
from test_batch_cpu import _item


def _phase2(fp, kind_value=0):
    return (fp, np.ones(fp.n_c), np.full(fp.n_c, kind_value, np.uint8), np.zeros(fp.n_c), np.full(fp.n_c, np.inf))


def _raw(count, items, results, opts=None):
    err = C.create_string_buffer(512)
    o = opts or E.default_opts()
    s = E.lib().ellp_batch_primal_solve(count, items, C.byref(o), results, err, 512)
    return s, err.value.decode()


def _refused(items, **kw):
    try:
        E.batch_primal_solve(items, E.default_opts(**kw))
    except E.EllpHipError as e:
        return e.status, e.msg
    raise AssertionError(f"not refused: {kw}")


def test_symbol_exported():
    assert hasattr(E.lib(), "ellp_batch_primal_solve")
    assert hasattr(E.lib(), "ellp_batch_primal_info")
    assert callable(E.batch_primal_solve)
    assert E.lib().ellp_hip_abi_version() == 1


def test_negative_count():
    items = (E.BatchPrimalItem * 1)()
    res = (E.BatchPrimalResult * 1)()
    s, msg = _raw(-1, items, res)
    assert s == E.ERR_ARG and msg


def test_null_items_or_results():
    items = (E.BatchPrimalItem * 1)()
    res = (E.BatchPrimalResult * 1)()
    s, msg = _raw(1, None, res)
    assert s == E.ERR_ARG and msg
    s, msg = _raw(1, items, None)
    assert s == E.ERR_ARG and msg


def test_null_c2_and_bad_kind2():
    fp = _item(3, 2)
    items = (E.BatchPrimalItem * 1)()  # every phase-2 pointer NULL
    res = (E.BatchPrimalResult * 1)()
    s, msg = _raw(1, items, res)
    assert s == E.ERR_ARG and "c2" in msg
    s, msg = _refused([_phase2(fp, kind_value=5)])
    assert s == E.ERR_ARG and "bound_kind2" in msg


def test_refused_options():
    fp = _item(3, 2)
    for kw in (dict(pipeline=1), dict(partial_segments=2), dict(trace_len=16), dict(flags=E.FLAG_PRIMAL_STEEPEST_EDGE)):
        s, msg = _refused([_phase2(fp)], **kw)
        assert s == E.ERR_ARG and msg, kw


def test_items_the_batch_cannot_take_have_their_own_status():
    big, bad = _item(129, 4), _item(3, 2)
    bad.nB = 2  # B of 2 elements for 3 rows: the single call's ELLP_ERR_BAD_DIMS
    x0 = big.x.copy()
    r = E.batch_primal_solve([_phase2(big), _phase2(bad)])
    assert [(x[0], x[1]) for x in r] == [(E.ERR_ARG, 1), (E.ERR_BAD_DIMS, 1)]
    assert "129" in r[0][6] and "invalid B" in r[1][6]
    assert np.isnan(r[0][4]) and big.x.tobytes() == x0.tobytes()  # no phase-1 objective, untouched
    assert E.batch_primal_solve([]) == []

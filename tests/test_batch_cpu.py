"""CPU-side checks of the batched solve (ellp_batch_solve_with_initial, ellp_solve_batch, solve_batch): the symbols are
exported, and the argument checks answer before any HIP call — on a machine without a device, a call that reached one
would return ELLP_ERR_DEVICE instead."""
import ctypes as C

import numpy as np

import ellp_amd
from ellp_amd import _engine as E


def _item(m, nN):
    """a well-formed primal LP of m rows (identity basis on the last m columns) and nN nonbasic columns"""
    n = m + nN
    A = np.zeros((m, n))
    A[:, :nN] = 1.0
    A[:, nN:] = np.eye(m)
    return E.FlatProblem(m, n, n, A.T.reshape(-1), np.ones(n), np.ones(m), np.zeros(n, np.uint8), np.zeros(n),
                         np.full(n, np.inf), np.r_[np.zeros(nN), np.ones(m)], np.arange(nN, n), np.arange(nN),
                         np.zeros(nN, np.uint8))


def _raw(kind, count, items, opts):
    status = (C.c_int * max(count, 1))()
    stats = (E.Stats * max(count, 1))()
    err = C.create_string_buffer(512)
    s = E.lib().ellp_batch_solve_with_initial(kind, count, items, C.byref(opts), status, stats, err, 512)
    return s, err.value.decode()


def test_symbols_exported():
    assert hasattr(E.lib(), "ellp_batch_solve_with_initial")
    assert hasattr(ellp_amd.host_lib(), "ellp_solve_batch")
    assert callable(E.batch_solve_with_initial)
    assert callable(ellp_amd.PrimalSimplexSolver.solve_batch)
    assert callable(ellp_amd.DualSimplexSolver.solve_batch)
    assert E.lib().ellp_hip_abi_version() == 1


def test_negative_count_and_null_items():
    s, msg = _raw(E.ENGINE_PRIMAL, -1, None, E.default_opts())
    assert s == E.ERR_ARG and msg
    s, msg = _raw(E.ENGINE_PRIMAL, 1, None, E.default_opts())
    assert s == E.ERR_ARG and msg
    s, msg = _raw(7, 0, None, E.default_opts())
    assert s == E.ERR_ARG and "kind" in msg


def test_refused_options():
    fp = _item(3, 2)
    refused = [dict(pipeline=1), dict(pipeline=2), dict(partial_segments=2), dict(flags=E.FLAG_PRIMAL_STEEPEST_EDGE),
               dict(trace_len=16), dict(profile=1), dict(refactor_period=8), dict(btran_mode=1)]
    for kw in refused:
        try:
            E.batch_solve_with_initial(E.ENGINE_PRIMAL, [fp], E.default_opts(**kw))
        except E.EllpHipError as e:
            assert e.status == E.ERR_ARG and e.msg, kw
        else:
            raise AssertionError(f"{kw} was not refused")
    # the dual's long-step ratio test runs on k_small whatever refactor_period says, as in a single call
    for kw in (dict(refactor_period=8, flags=E.FLAG_DUAL_BOUND_FLIPPING), dict(pipeline=3, refactor_period=8)):
        r = E.batch_solve_with_initial(E.ENGINE_DUAL, [_item(129, 1)], E.default_opts(**kw))
        assert r[0][0] == E.ERR_ARG  # the item (no y, d), not the call


def test_items_the_batch_cannot_take_have_their_own_status():
    big, empty, bad = _item(129, 4), _item(1, 1), _item(3, 2)
    empty.m = 0
    bad.nB = 2  # B of 2 elements for 3 rows: the single call's ELLP_ERR_BAD_DIMS
    x0 = big.x.copy()
    r = E.batch_solve_with_initial(E.ENGINE_PRIMAL, [big, empty, bad])
    assert [s for s, _, _ in r] == [E.ERR_ARG, E.ERR_ARG, E.ERR_BAD_DIMS]
    assert "129" in r[0][2] and "m == 0" in r[1][2] and "invalid B" in r[2][2]
    assert big.x.tobytes() == x0.tobytes()  # untouched


def test_dual_item_needs_y_and_d():
    r = E.batch_solve_with_initial(E.ENGINE_DUAL, [_item(3, 2)])
    assert r[0][0] == E.ERR_ARG and "y and d" in r[0][2]


def test_empty_batches():
    assert E.batch_solve_with_initial(E.ENGINE_PRIMAL, []) == []
    assert ellp_amd.PrimalSimplexSolver().solve_batch([]) == []
    assert ellp_amd.DualSimplexSolver().solve_batch([]) == []

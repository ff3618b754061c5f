"""CPU-side checks of the batched ranging (ellp_batch_ranging, ellp_solve_batch_flags): the symbols are exported with the
documented signatures, the call-level and the per-item refusals answer before any HIP call with the messages of
ellp_ranging — on a machine without a device, a call that reached one would return ELLP_ERR_DEVICE instead — and the ctypes
mirror of ellp_batch_range_out has the size of the header's."""
import ctypes as C
import inspect
import os
import subprocess
import tempfile

import numpy as np

import ellp_amd
from ellp_amd import _engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _item(m, nN):
    """a well-formed point of m rows (identity basis on the last m columns) and nN nonbasic columns"""
    n = m + nN
    A = np.zeros((m, n))
    A[:, :nN] = 1.0
    A[:, nN:] = np.eye(m)
    return E.FlatProblem(m, n, n, A.T.reshape(-1), np.ones(n), np.ones(m), np.zeros(n, np.uint8), np.zeros(n),
                         np.full(n, np.inf), np.r_[np.zeros(nN), np.ones(m)], np.arange(nN, n), np.arange(nN),
                         np.zeros(nN, np.uint8))


def _raw(count, items, outs, status):
    err = C.create_string_buffer(512)
    s = E.lib().ellp_batch_ranging(count, items, C.byref(E.default_opts()), outs, status, err, 512)
    return s, err.value.decode()


def _single_message(fp, want=True):
    """status and message of ellp_ranging for the same arrays (refused before any HIP call)"""
    out = E.RangingOut()
    up = np.zeros(max(fp.m, 1))
    if want:
        out.rhs_up = up.ctypes.data
    err = C.create_string_buffer(512)
    s = E.lib().ellp_ranging(*fp._args(), C.byref(E.default_opts()), C.byref(out), err, 512)
    return s, err.value.decode()


def test_symbols_and_signatures():
    assert hasattr(E.lib(), "ellp_batch_ranging") and hasattr(E.lib(), "ellp_batch_ranging_info")
    assert hasattr(ellp_amd.host_lib(), "ellp_solve_batch_flags")
    assert list(inspect.signature(E.batch_ranging).parameters)[:3] == ["flat_problems", "opts", "want_W"]
    assert inspect.signature(E.batch_ranging).parameters["want_W"].default is False
    assert set(E.batch_ranging_info()) == {"launches", "batched", "single", "chunks"}
    sig = inspect.signature(ellp_amd.PrimalSimplexSolver.solve_batch)
    assert list(sig.parameters) == ["self", "problems", "starts", "postsolve", "ranging"]
    assert sig.parameters["ranging"].default is False and sig.parameters["postsolve"].default is False
    assert "ranging=True" in ellp_amd.PrimalSimplexSolver.solve_batch.__doc__
    assert "5 per" in E.batch_ranging_info.__doc__  # the launch count per chunk is stated


def test_call_level_refusals():
    items, outs, status = (E.BatchItem * 1)(), (E.BatchRangeOut * 1)(), (C.c_int * 1)()
    for args in ((-1, items, outs, status), (1, None, outs, status), (1, items, None, status), (1, items, outs, None),
                 (0, None, outs, status)):
        s, msg = _raw(*args)
        assert s == E.ERR_ARG and msg, args[0]


def test_count_zero_is_fine():
    items, outs, status = (E.BatchItem * 1)(), (E.BatchRangeOut * 1)(), (C.c_int * 1)()
    s, msg = _raw(0, items, outs, status)
    assert s == E.OPTIMAL and msg == ""
    assert E.batch_ranging([]) == []
    assert E.batch_ranging_info() == {"launches": 0, "batched": 0, "single": 0, "chunks": 0}


def test_per_item_refusals_are_the_single_calls():
    no_rows, short_b, bad_index, bad_label, bad_kind, too_big, sizes = (_item(3, 2) for _ in range(7))
    no_rows.m = 0
    short_b.nB = 2
    bad_index.B[1] = 99
    bad_label.Nb[0] = 7
    bad_kind.kind[2] = 9
    too_big.m = 1 << 20
    sizes.n_c = sizes.n - 1
    bad = [no_rows, short_b, bad_index, bad_label, bad_kind, too_big, sizes]
    res = E._batch_ranging_raw(bad, fill=-7.0)
    for fp, (s, rg, W, msg) in zip(bad, res):
        ss, smsg = _single_message(fp)
        assert ss == E.ERR_ARG and smsg
        assert (s, msg) == (ss, smsg)
        assert all((getattr(rg, name) == -7).all() for name in rg.ARRAYS)  # untouched
    assert "m < 1" in res[0][3] and "invalid B/N" in res[1][3] and "B_index[1]" in res[2][3]
    assert all(r[1] is None and r[2] is None for r in E.batch_ranging(bad))


def test_item_that_wants_nothing():
    fp = _item(3, 2)
    (s, rg, W, msg), = E._batch_ranging_raw([fp], wanted=[[]])  # every pointer of out NULL and W NULL
    assert (s, msg) == _single_message(fp, want=False)
    assert s == E.ERR_ARG and "nothing is wanted" in msg


def _flags(probs, n, solver, flags, with_out=True):
    L = ellp_amd.host_lib()
    rrs = (ellp_amd._ResultRng * max(n, 1))()
    handles = (C.c_void_p * max(n, 1))(*[None if p is None else p._h for p in probs])
    return L.ellp_solve_batch_flags(handles, n, solver, 1000, None, flags, None, rrs if with_out else None, None)


def test_solve_batch_flags_refusals():
    p = ellp_amd.Problem()
    p.add_var(1.0, ellp_amd.Bound.Lower(0.0))
    assert _flags([p], 1, 0, 4) == E.ERR_ARG        # an unknown flag bit
    assert _flags([p], 1, 0, 3 | 8) == E.ERR_ARG
    assert _flags([None], 1, 0, 3) == E.ERR_ARG     # a NULL problem
    assert _flags([p], 1, 7, 3) == E.ERR_ARG        # an unknown solver
    assert _flags([p], -1, 0, 3) == E.ERR_ARG
    assert _flags([p], 1, 0, 3, with_out=False) == E.ERR_ARG
    # starts without reports
    L = ellp_amd.host_lib()
    rrs = (ellp_amd._ResultRng * 1)()
    sptr = (C.POINTER(ellp_amd._Start) * 1)()
    assert L.ellp_solve_batch_flags((C.c_void_p * 1)(p._h), 1, 0, 1000, None, 3, sptr, rrs, None) == E.ERR_ARG
    # ellp_solve_batch_start goes on refusing the ranging flag
    reps = (ellp_amd._StartReport * 1)()
    assert L.ellp_solve_batch_start((C.c_void_p * 1)(p._h), 1, 0, 1000, None, 2, sptr, rrs, reps) == E.ERR_ARG


def test_empty_batch():
    for cls in (ellp_amd.PrimalSimplexSolver, ellp_amd.DualSimplexSolver):
        assert cls().solve_batch([], ranging=True) == []
        assert cls().solve_batch([], starts=[], ranging=True) == []


def test_struct_sizes_match_the_header():
    src = ('#include <stdio.h>\n#include "ellp_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(ellp_batch_range_out), '
           'sizeof(ellp_ranging_out), sizeof(ellp_ranging_info)); return 0; }\n')
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "sizes.c"), os.path.join(td, "sizes")
        with open(c, "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), c, "-o", exe])
        sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    assert sizes == [C.sizeof(E.BatchRangeOut), C.sizeof(E.RangingOut), C.sizeof(E.RangingInfo)]
    assert C.sizeof(E.BatchRangeOut) == 12 * C.sizeof(C.c_void_p)

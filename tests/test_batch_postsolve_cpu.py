"""CPU-side checks of the batched postsolve (ellp_batch_postsolve): the symbols are exported, the call-level and the
per-item refusals answer before any HIP call with the messages of ellp_postsolve — on a machine without a device, a call
that reached one would return ELLP_ERR_DEVICE instead — and the ctypes structs have the sizes of the header's."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

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
    s = E.lib().ellp_batch_postsolve(count, items, C.byref(E.default_opts()), outs, status, err, 512)
    return s, err.value.decode()


def _single_message(fp, want=True):
    """status and message of ellp_postsolve for the same arrays (refused before any HIP call)"""
    y = np.zeros(max(fp.m, 1))
    err = C.create_string_buffer(512)
    s = E.lib().ellp_postsolve(*fp._args(), C.byref(E.default_opts()), E._p(y) if want else None, None, None, None, err, 512)
    return s, err.value.decode()


def test_symbols_exported():
    assert hasattr(E.lib(), "ellp_batch_postsolve")
    assert hasattr(E.lib(), "ellp_batch_postsolve_info")
    assert callable(E.batch_postsolve) and callable(E.batch_postsolve_info)
    assert set(E.batch_postsolve_info()) == {"launches", "batched", "single", "chunks"}


def test_call_level_refusals():
    items, outs, status = (E.BatchItem * 1)(), (E.BatchPostOut * 1)(), (C.c_int * 1)()
    for args in ((-1, items, outs, status), (1, None, outs, status), (1, items, None, status), (1, items, outs, None),
                 (0, None, outs, status)):
        s, msg = _raw(*args)
        assert s == E.ERR_ARG and msg, args[0]


def test_count_zero_is_fine():
    items, outs, status = (E.BatchItem * 1)(), (E.BatchPostOut * 1)(), (C.c_int * 1)()
    s, msg = _raw(0, items, outs, status)
    assert s == E.OPTIMAL and msg == ""
    assert E.batch_postsolve([]) == []


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
    res = E.batch_postsolve(bad, fill=-7.0)
    for fp, (s, y, d, r, kkt, msg) in zip(bad, res):
        ss, smsg = _single_message(fp)
        assert ss == E.ERR_ARG and smsg
        assert (s, msg) == (ss, smsg)
        assert kkt is None
        assert all((a == -7.0).all() for a in (y, d, r))  # untouched
    assert "m < 1" in res[0][5] and "invalid B/N" in res[1][5] and "B_index[1]" in res[2][5]


def test_item_that_wants_nothing():
    fp = _item(3, 2)
    items, outs, status = (E.BatchItem * 1)(), (E.BatchPostOut * 1)(), (C.c_int * 1)()
    it = items[0]
    it.m, it.n, it.n_c = fp.m, fp.n, fp.n_c
    it.A, it.c, it.b, it.bound_kind = E._p(fp.A), E._p(fp.c), E._p(fp.b), E._p(fp.kind)
    it.lb, it.ub, it.x = E._p(fp.lb), E._p(fp.ub), E._p(fp.x)
    it.B_index, it.n_B, it.N_index, it.N_bound, it.n_N = E._p(fp.B), fp.nB, E._p(fp.N), E._p(fp.Nb), fp.nN
    s, msg = _raw(1, items, outs, status)
    assert s == E.OPTIMAL and msg == ""  # the item's refusal, not the call's
    assert (status[0], items[0].err.decode()) == _single_message(fp, want=False)
    assert status[0] == E.ERR_ARG and "none of y, d, r, kkt" in items[0].err.decode()


def test_struct_sizes_match_the_header():
    src = ('#include <stdio.h>\n#include "ellp_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(ellp_batch_post_out), '
           'sizeof(ellp_kkt), sizeof(ellp_batch_item)); return 0; }\n')
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "sizes.c"), os.path.join(td, "sizes")
        with open(c, "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), c, "-o", exe])
        sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    assert sizes == [C.sizeof(E.BatchPostOut), C.sizeof(E.Kkt), C.sizeof(E.BatchItem)]
    assert C.sizeof(E.BatchPostOut) == 4 * C.sizeof(C.c_void_p)

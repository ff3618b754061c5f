"""CPU-side checks of the batched warm start: ellp_batch_basis_start answers every whole-call and every per-item refusal
before any HIP call, with the message ellp_basis_start gives for the same item — on a machine without a device a call that
reached one would return ELLP_ERR_DEVICE instead; the ctypes structs have the sizes of the header's; solve_batch refuses a
list of starts of the wrong length; ellp_solve_batch_start refuses the ranging flag."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import ellp_amd
from ellp_amd import _engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _good(m=2, nN=3):
    """a well-formed item as tests/test_start_abi_cpu.py makes it: A = [A_N | I], the identity basic"""
    n = m + nN
    A = np.zeros((m, n), order="F")
    A[:, :nN] = 1.0
    A[np.arange(m), nN + np.arange(m)] = 1.0
    return dict(m=m, n=n, n_c=n, A=A.reshape(-1, order="F"), c=np.ones(n), b=np.ones(m), kind=np.ones(n, dtype=np.uint8), lb=np.zeros(n),
                ub=np.full(n, np.inf), B=nN + np.arange(m, dtype=np.int64), nB=m, N=np.arange(nN, dtype=np.int64),
                Nb=np.zeros(nN, dtype=np.uint8), nN=nN, x=np.full(n, -7.0), y=np.full(m, -7.0), d=np.full(n, -7.0))


# the refusals of tests/test_start_abi_cpu.py that are the item's (the mode is the call's)
REFUSALS = {
    "null-A": dict(A=None), "null-c": dict(c=None), "null-b": dict(b=None), "null-kind": dict(kind=None), "null-lb": dict(lb=None),
    "null-ub": dict(ub=None), "null-B": dict(B=None), "null-N": dict(N=None), "null-Nb": dict(Nb=None), "null-x": dict(x=None),
    "m-zero": dict(m=0, nB=0, n=3, n_c=3), "m-negative": dict(m=-1), "m-above-8192": dict(m=8193, nB=8193, n=8196, n_c=8196),
    "nB-not-m": dict(nB=1), "nB-plus-nN-not-n": dict(n=6, n_c=6), "nN-negative": dict(nN=-1, n=1, n_c=1),
    "B-out-of-range": dict(B=np.array([3, 5], dtype=np.int64)), "B-negative": dict(B=np.array([-1, 4], dtype=np.int64)),
    "N-out-of-range": dict(N=np.array([0, 1, 9], dtype=np.int64)),
    "twice-in-B": dict(B=np.array([3, 3], dtype=np.int64)), "twice-in-N": dict(N=np.array([0, 1, 1], dtype=np.int64)),
    "twice-across-B-and-N": dict(N=np.array([0, 1, 4], dtype=np.int64)),
    "label-above-range": dict(Nb=np.array([0, 3, 0], dtype=np.uint8)), "kind-above-range": dict(kind=np.array([1, 1, 5, 1, 1], dtype=np.uint8)),
}


def _p(v):
    return None if v is None else v.ctypes.data_as(C.c_void_p)


def _fill(it, a):
    it.m, it.n, it.n_c = a["m"], a["n"], a["n_c"]
    it.A, it.c, it.b, it.bound_kind = _p(a["A"]), _p(a["c"]), _p(a["b"]), _p(a["kind"])
    it.lb, it.ub, it.x = _p(a["lb"]), _p(a["ub"]), _p(a["x"])
    it.B_index, it.n_B, it.N_index, it.N_bound, it.n_N = _p(a["B"]), a["nB"], _p(a["N"]), _p(a["Nb"]), a["nN"]
    it.y, it.d = _p(a["y"]), _p(a["d"])


def _single(a, mode=0):
    err = C.create_string_buffer(512)
    s = E.lib().ellp_basis_start(a["m"], a["n"], _p(a["A"]), _p(a["c"]), _p(a["b"]), _p(a["kind"]), _p(a["lb"]), _p(a["ub"]), _p(a["B"]), a["nB"],
                                 _p(a["N"]), _p(a["Nb"]), a["nN"], mode, None, _p(a["x"]), _p(a["y"]), _p(a["d"]), None, err, 512)
    return s, err.value.decode()


def _raw(count, items, mode, infos, status):
    err = C.create_string_buffer(512)
    s = E.lib().ellp_batch_basis_start(count, items, mode, None, infos, status, err, 512)
    return s, err.value.decode()


def test_symbols_exported():
    assert hasattr(E.lib(), "ellp_batch_basis_start") and hasattr(E.lib(), "ellp_batch_basis_start_info")
    assert callable(E.batch_basis_start) and callable(E.batch_basis_start_info)
    assert set(E.batch_basis_start_info()) == {"launches", "batched", "single", "chunks"}
    assert hasattr(ellp_amd.host_lib(), "ellp_solve_batch_start")


def test_call_level_refusals():
    items, infos, status = (E.BatchItem * 1)(), (E.StartInfo * 1)(), (C.c_int * 1)()
    _fill(items[0], _good())
    for args in ((-1, items, 0, infos, status), (1, None, 0, infos, status), (1, items, 0, infos, None), (0, None, 0, infos, status),
                 (1, items, 2, infos, status), (1, items, -1, infos, status)):
        status[0] = 77
        s, msg = _raw(*args)
        assert s == E.ERR_ARG and msg, args[0]
        assert status[0] == 77
    assert _raw(1, items, 2, infos, status)[1] == _single(_good(), mode=2)[1]  # the unknown mode: the single call's words


def test_count_zero_is_fine():
    items, status = (E.BatchItem * 1)(), (C.c_int * 1)()
    assert _raw(0, items, 0, None, status) == (E.OPTIMAL, "")
    assert E.batch_basis_start([], 0) == []
    assert E.batch_basis_start_info() == {"launches": 0, "batched": 0, "single": 0, "chunks": 0}


@pytest.mark.parametrize("mode", [0, 1])
def test_per_item_refusals_are_the_single_calls(mode):
    """all the refusals in ONE call: every item is answered on the host, so the call never looks for a device"""
    names = sorted(REFUSALS)
    cases = [dict(_good(), **REFUSALS[n]) for n in names]
    items, infos, status = (E.BatchItem * len(cases))(), (E.StartInfo * len(cases))(), (C.c_int * len(cases))()
    for it, a in zip(items, cases):
        _fill(it, a)
    assert _raw(len(cases), items, mode, infos, status) == (E.OPTIMAL, "")
    for k, (name, a) in enumerate(zip(names, cases)):
        ss, smsg = _single(a, mode)
        assert ss == E.ERR_ARG and smsg, name
        assert (status[k], items[k].err.decode()) == (ss, smsg), name
        for key in ("x", "y", "d"):  # nothing was written
            assert a[key] is None or (a[key] == -7.0).all(), (name, key)
        assert infos[k].labels_changed == 0 and infos[k].kkt.refinement_steps == 0
    assert E.batch_basis_start_info() == {"launches": 0, "batched": 0, "single": 0, "chunks": 0}


def test_an_item_with_costs_beyond_its_columns_is_refused():
    a = dict(_good(), n_c=6)
    items, status = (E.BatchItem * 1)(), (C.c_int * 1)()
    _fill(items[0], a)
    assert _raw(1, items, 0, None, status) == (E.OPTIMAL, "")
    assert status[0] == E.ERR_ARG and "n_c" in items[0].err.decode()


def test_the_wrapper_returns_the_message_and_leaves_the_arrays():
    fp = E.FlatProblem(2, 5, 5, _good()["A"], np.ones(5), np.ones(2), np.ones(5, np.uint8), np.zeros(5), np.full(5, np.inf), np.zeros(5),
                       [3, 3], [0, 1, 2], [0, 0, 0])
    (s, x, y, d, Nb, info), = E.batch_basis_start([fp], 0, fill=-7.0)
    assert s == E.ERR_ARG and info == {"message": "basis_start: variable 3 is listed twice in B and N"}
    assert all((v == -7.0).all() for v in (x, y, d)) and Nb.tolist() == [0, 0, 0]


def test_struct_sizes_match_the_header():
    src = ('#include <stdio.h>\n#include "ellp_hip.h"\n#include "ellp_host.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
           'sizeof(ellp_batch_item), sizeof(ellp_start_info), sizeof(ellp_kkt), sizeof(ellp_start), sizeof(ellp_start_report), '
           'sizeof(ellp_result_rng)); return 0; }\n')
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "sizes.c"), os.path.join(td, "sizes")
        with open(c, "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), c, "-o", exe])
        sizes = [int(v) for v in subprocess.check_output([exe]).split()]
    assert sizes == [C.sizeof(E.BatchItem), C.sizeof(E.StartInfo), C.sizeof(E.Kkt), C.sizeof(ellp_amd._Start), C.sizeof(ellp_amd._StartReport),
                     C.sizeof(ellp_amd._ResultRng)]
    assert C.sizeof(E.StartInfo) == 7 * 8 + 4 * 4 + C.sizeof(E.Kkt)


def _prob():
    """min -x0 - 2 x1, x0 + x1 <= 4, x0 - x1 <= 1, x >= 0"""
    p = ellp_amd.Problem()
    p.add_var(-1.0, ellp_amd.Bound.Lower(0.0))
    p.add_var(-2.0, ellp_amd.Bound.Lower(0.0))
    p.add_constraint([(0, 1.0), (1, 1.0)], "Lte", 4.0)
    p.add_constraint([(0, 1.0), (1, -1.0)], "Lte", 1.0)
    return p


def test_solve_batch_refuses_starts_of_the_wrong_length():
    ps = [_prob(), _prob()]
    for which in (ellp_amd.PrimalSimplexSolver, ellp_amd.DualSimplexSolver):
        for starts in ([], [None], [None, None, None], [dict(B=[0, 1])]):
            with pytest.raises(ValueError):
                which().solve_batch(ps, starts=starts)
    with pytest.raises((ValueError, TypeError)):
        ellp_amd.DualSimplexSolver().solve_batch(ps, starts=[None, 3.5])  # neither None, a dict nor a Solution


def test_solve_batch_start_refuses_the_ranging_flag_and_bad_arguments():
    L = ellp_amd.host_lib()
    ps = [_prob(), _prob()]
    handles = (C.c_void_p * 2)(*[p._h for p in ps])
    B = np.array([0, 1], dtype=np.int64)
    st = ellp_amd._Start(2, B.ctypes.data, 0, None, None)
    starts = (C.POINTER(ellp_amd._Start) * 2)(C.pointer(st), None)
    out, rep = (ellp_amd._ResultRng * 2)(), (ellp_amd._StartReport * 2)()
    call = lambda *a: L.ellp_solve_batch_start(*a)
    assert call(handles, 2, 1, 1000, None, 2, starts, out, rep) == E.ERR_ARG   # ELLP_SOLVE_RANGING: there is no batched ranging
    assert call(handles, 2, 1, 1000, None, 1 | 2, starts, out, rep) == E.ERR_ARG
    assert call(handles, 2, 1, 1000, None, 4, starts, out, rep) == E.ERR_ARG                                # an unknown flag
    assert call(handles, 2, 2, 1000, None, 0, starts, out, rep) == E.ERR_ARG                                # an unknown solver
    assert call(handles, -1, 1, 1000, None, 0, starts, out, rep) == E.ERR_ARG
    assert call(None, 2, 1, 1000, None, 0, starts, out, rep) == E.ERR_ARG
    assert call(handles, 2, 1, 1000, None, 0, None, out, rep) == E.ERR_ARG
    assert call(handles, 2, 1, 1000, None, 0, starts, None, rep) == E.ERR_ARG
    assert call(handles, 2, 1, 1000, None, 0, starts, out, None) == E.ERR_ARG
    assert all(o.ex.result.x is None or not o.ex.result.x for o in out)  # nothing was allocated

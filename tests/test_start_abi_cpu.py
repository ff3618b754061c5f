"""The refusals of ellp_basis_start and ellp_solve_start, answered with ELLP_ERR_ARG and a message before any HIP call (no
device is needed: on a machine without one a call that reached the device would answer ELLP_ERR_DEVICE), and the mapping of a
start into the standard form (ellp_debug_map_start, host only): the complement for a missing N, the phase-1 indices of a
primal solve's basis dropped from N and refused in B, sizes before indices."""
import ctypes as C

import numpy as np
import pytest

import ellp_amd
from ellp_amd import _engine as E


def _good(m=2, nN=3):
    """a well-formed call: A = [A_N | I], the identity basic"""
    n = m + nN
    A = np.zeros((m, n), order="F")
    A[:, :nN] = 1.0
    A[np.arange(m), nN + np.arange(m)] = 1.0
    return dict(m=m, n=n, A=A.reshape(-1, order="F"), c=np.ones(n), b=np.ones(m), kind=np.ones(n, dtype=np.uint8), lb=np.zeros(n),
                ub=np.full(n, np.inf), B=nN + np.arange(m, dtype=np.int64), nB=m, N=np.arange(nN, dtype=np.int64),
                Nb=np.zeros(nN, dtype=np.uint8), nN=nN, mode=0, x=np.full(n, -7.0), y=np.full(m, -7.0), d=np.full(n, -7.0))


def _call(a, info=True):
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    err = C.create_string_buffer(512)
    inf = E.StartInfo()
    s = E.lib().ellp_basis_start(a["m"], a["n"], p(a["A"]), p(a["c"]), p(a["b"]), p(a["kind"]), p(a["lb"]), p(a["ub"]), p(a["B"]), a["nB"],
                                 p(a["N"]), p(a["Nb"]), a["nN"], a["mode"], None, p(a["x"]), p(a["y"]), p(a["d"]),
                                 C.byref(inf) if info else None, err, 512)
    return s, err.value.decode()


def _with(**kw):
    a = _good()
    a.update(kw)
    return a


REFUSALS = {
    "null-A": dict(A=None), "null-c": dict(c=None), "null-b": dict(b=None), "null-kind": dict(kind=None), "null-lb": dict(lb=None),
    "null-ub": dict(ub=None), "null-B": dict(B=None), "null-N": dict(N=None), "null-Nb": dict(Nb=None), "null-x": dict(x=None),
    "m-zero": dict(m=0, nB=0, n=3), "m-negative": dict(m=-1), "m-above-8192": dict(m=8193, nB=8193, n=8196),
    "nB-not-m": dict(nB=1), "nB-plus-nN-not-n": dict(n=6), "nN-negative": dict(nN=-1, n=1),
    "B-out-of-range": dict(B=np.array([3, 5], dtype=np.int64)), "B-negative": dict(B=np.array([-1, 4], dtype=np.int64)),
    "N-out-of-range": dict(N=np.array([0, 1, 9], dtype=np.int64)),
    "twice-in-B": dict(B=np.array([3, 3], dtype=np.int64)), "twice-in-N": dict(N=np.array([0, 1, 1], dtype=np.int64)),
    "twice-across-B-and-N": dict(N=np.array([0, 1, 4], dtype=np.int64)),
    "label-above-range": dict(Nb=np.array([0, 3, 0], dtype=np.uint8)), "kind-above-range": dict(kind=np.array([1, 1, 5, 1, 1], dtype=np.uint8)),
    "unknown-mode": dict(mode=2), "negative-mode": dict(mode=-1),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_basis_start_refuses(name):
    a = _with(**REFUSALS[name])
    s, msg = _call(a)
    assert s == E.ERR_ARG and msg, (name, s, msg)
    for k in ("x", "y", "d"):  # nothing was written
        assert a[k] is None or (a[k] == -7.0).all(), (name, k)


def test_basis_start_takes_null_y_d_info():
    """y, d and info are optional: such a call passes every check and goes on to the device (ELLP_ERR_DEVICE without one)"""
    s, msg = _call(_with(y=None, d=None), info=False)
    assert s in (E.OPTIMAL, E.ERR_DEVICE), (s, msg)


def _prob():
    """min -x0 - 2 x1, x0 + x1 <= 4, x0 - x1 <= 1, x >= 0: 2 rows, 4 columns (2 variables, 2 slacks)"""
    p = ellp_amd.Problem()
    p.add_var(-1.0, ellp_amd.Bound.Lower(0.0))
    p.add_var(-2.0, ellp_amd.Bound.Lower(0.0))
    p.add_constraint([(0, 1.0), (1, 1.0)], "Lte", 4.0)
    p.add_constraint([(0, 1.0), (1, -1.0)], "Lte", 1.0)
    return p


def test_solve_start_refuses():
    L = ellp_amd.host_lib()
    B = np.array([0, 1], dtype=np.int64)
    st = ellp_amd._Start(2, B.ctypes.data, 0, None, None)
    p = _prob()
    rr, rep = ellp_amd._ResultRng(), ellp_amd._StartReport()
    assert L.ellp_solve_start(p._h, 0, 1000, None, 0, C.byref(st), None, C.byref(rep)) == E.ERR_ARG  # no out
    for args in ((None, 0, 1000, None, 0, C.byref(st)), (p._h, 0, 1000, None, 0, None), (p._h, 2, 1000, None, 0, C.byref(st)),
                 (p._h, -1, 1000, None, 0, C.byref(st)), (p._h, 0, 1000, None, 4, C.byref(st))):
        rr = ellp_amd._ResultRng()
        assert L.ellp_solve_start(*args, C.byref(rr), C.byref(rep)) == E.ERR_ARG, args
        assert rr.ex.result.status == E.ERR_ARG and rr.ex.result.err, args
        assert rep.used == 0
        L.ellp_result_rng_free(C.byref(rr))


def test_start_is_mapped_into_the_standard_form():
    p = _prob()
    m = ellp_amd._debug_map_start
    # B alone: N is the complement in ascending order, every label Lower
    rc, rows, cols, B, N, Nb = m(p, dict(B=[1, 2]))
    assert (rc, rows, cols) == (0, 2, 4) and B.tolist() == [1, 2] and N.tolist() == [0, 3] and Nb.tolist() == [0, 0]
    # B, N, Nb as a dual solve reports them
    rc, _, _, B, N, Nb = m(p, dict(B=[3, 0], N=[2, 1], Nb=[1, 0]))
    assert rc == 0 and B.tolist() == [3, 0] and N.tolist() == [2, 1] and Nb.tolist() == [1, 0]
    # as a primal solve reports them: the two phase-1 columns 4, 5 ended nonbasic and are dropped
    rc, _, _, B, N, Nb = m(p, dict(B=[0, 1], N=[4, 2, 5, 3], Nb=[0, 1, 0, 0]))
    assert rc == 0 and N.tolist() == [2, 3] and Nb.tolist() == [1, 0]
    # a phase-1 column in B: reason 2, whatever N holds
    assert m(p, dict(B=[0, 4]))[0] == 2
    assert m(p, dict(B=[0, 4], N=[1, 2, 5, 3], Nb=[0, 0, 0, 0]))[0] == 2
    # sizes (reason 1) come before indices and duplicates (reason 2)
    assert m(p, dict(B=[0]))[0] == 1 and m(p, dict(B=[0, 1, 2]))[0] == 1
    assert m(p, dict(B=[0, 1], N=[2]))[0] == 1 and m(p, dict(B=[0, 1], N=[2, 3, 0], Nb=[0, 0, 0]))[0] == 1
    assert m(p, dict(B=[0, 0]))[0] == 2 and m(p, dict(B=[0, -1]))[0] == 2
    assert m(p, dict(B=[0, 1], N=[2, 2], Nb=[0, 0]))[0] == 2 and m(p, dict(B=[0, 1], N=[1, 2], Nb=[0, 0]))[0] == 2
    assert m(p, dict(B=[0, 1], N=[2, -3], Nb=[0, 0]))[0] == 2 and m(p, dict(B=[0, 1], N=[2, 3], Nb=[0, 3]))[0] == 2
    # without rows there is no basis to start from: reason 5
    q = ellp_amd.Problem()
    q.add_var(1.0, ellp_amd.Bound.Lower(0.0))
    assert m(q, dict(B=[]))[0] == 5

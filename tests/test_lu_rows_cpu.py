"""ellp_hip_lu_rows (the LU of a square matrix by rows the exact loop above 1,024 rows factors the basis with): the symbol is
there, and its argument refusals come with their messages before any HIP call — no device is touched."""
import ctypes as C

import numpy as np

from ellp_amd import _engine as E


def _call(m, M, variant, fac, piv, ud):
    err = C.create_string_buffer(512)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    s = E.lib().ellp_hip_lu_rows(m, p(M), variant, p(fac), p(piv), p(ud), -1, err, 512)
    return s, err.value.decode()


def _arrays(m=3):
    return np.eye(m), np.zeros((m, m)), np.zeros(m, dtype=np.int64), np.zeros(m)


def test_the_symbol_exists():
    assert hasattr(E.lib(), "ellp_hip_lu_rows")
    assert callable(E.lu_rows)


def test_no_rows_is_refused():
    M, fac, piv, ud = _arrays()
    for m in (0, -4):
        s, msg = _call(m, M, 1, fac, piv, ud)
        assert s == E.ERR_ARG and "at least one row" in msg, (s, msg)


def test_a_null_pointer_is_refused():
    M, fac, piv, ud = _arrays()
    for args in ((None, fac, piv, ud), (M, None, piv, ud), (M, fac, None, ud), (M, fac, piv, None)):
        s, msg = _call(3, args[0], 0, *args[1:])
        assert s == E.ERR_ARG and "NULL pointer" in msg, (s, msg)


def test_an_unknown_variant_is_refused():
    M, fac, piv, ud = _arrays()
    for variant in (2, -1):
        s, msg = _call(3, M, variant, fac, piv, ud)
        assert s == E.ERR_ARG and "unknown variant %d" % variant in msg, (s, msg)
    assert fac.tobytes() == np.zeros((3, 3)).tobytes()  # nothing was written

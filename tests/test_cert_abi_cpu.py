"""The certificate entry points refuse bad arguments with ELLP_ERR_ARG and a message before any HIP call (so also on a machine
without a device); the ABI version is still 1; the declarations stand in the public header."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ellp_amd import _engine as E  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flat(m=4, nN=6):
    n = m + nN
    A = np.zeros((m, n), order="F")
    A[:, :nN] = 1.0
    A[np.arange(m), nN + np.arange(m)] = 1.0
    z = np.zeros(n)
    return E.FlatProblem(m, n, n, A.reshape(-1, order="F"), z, np.ones(m), np.full(n, 1, dtype=np.uint8), z, z, z,
                         nN + np.arange(m, dtype=np.int64), np.arange(nN, dtype=np.int64), np.zeros(nN, dtype=np.uint8))


def _call(fp, args=None, source=E.CERT_FARKAS_ROW, n_check=None, chk=(None, None, None), vec=True, info=True):
    v, i = np.full(fp.n, 7.0), E.CertInfo()
    err = C.create_string_buffer(512)
    o = E.default_opts()
    a = fp._args() if args is None else args
    s = E.lib().ellp_certificate(*a, C.byref(o), source, fp.n if n_check is None else n_check, E._p(chk[0]), E._p(chk[1]), E._p(chk[2]),
                                 E._p(v) if vec else None, C.byref(i) if info else None, err, 512)
    assert (v == 7.0).all() and i.found == 0 and i.kind == 0  # a refusal writes nothing
    return s, err.value.decode()


def test_abi_version_is_still_1():
    assert E.lib().ellp_hip_abi_version() == 1
    assert re.search(r"#define ELLP_HIP_ABI_VERSION 1\b", open(os.path.join(ROOT, "include", "ellp_hip.h")).read())


def test_the_declarations_are_in_the_header():
    h = open(os.path.join(ROOT, "include", "ellp_hip.h")).read()
    for name in ("ellp_engine_certificate", "ellp_certificate", "ellp_certificate_info", "ellp_cert_info", "ELLP_CERT_FARKAS_COSTS",
                 "ELLP_CERT_FARKAS_ROW", "ELLP_CERT_RAY_COLUMN"):
        assert re.search(r"\b%s\b" % name, h), name
        if name.startswith("ellp_") and name != "ellp_cert_info":
            assert hasattr(E.lib(), name), name
    assert C.sizeof(E.CertInfo) == 8 + 16 + 8 * 8 + 24 + 8  # the layout of ellp_cert_info


def _small_problem():
    import ellp_amd as L
    p = L.Problem()
    p.add_var(-1.0, L.Bound.Lower(0.0))
    p.add_constraint([(0, 1.0)], "Lte", 4.0)
    return p


def test_solve_cert_is_declared_and_refuses_bad_arguments():
    import ellp_amd as L
    h = open(os.path.join(ROOT, "include", "ellp_host.h")).read()
    for name in ("ellp_solve_cert", "ellp_result_cert_free", "ellp_result_cert", "ELLP_SOLVE_CERTIFICATE"):
        assert re.search(r"\b%s\b" % name, h), name
    assert re.search(r"#define ELLP_SOLVE_CERTIFICATE 4u", h)
    H = L.host_lib()
    p = _small_problem()
    before = E.certificate_info()["calls"]

    def call(prob, solver, flags, out=True, cert=True):
        rr, rc = L._ResultRng(), L._ResultCert()
        s = H.ellp_solve_cert(prob, solver, 1000, None, flags, None, C.byref(rr) if out else None, None, C.byref(rc) if cert else None)
        assert rc.kind == 0 and rc.n == 0 and not rc.vec
        return s

    assert call(None, 0, 4) == E.ERR_ARG
    assert call(p._h, 2, 4) == E.ERR_ARG          # an unknown solver
    assert call(p._h, 0, 8) == E.ERR_ARG          # an unknown flag
    assert call(p._h, 0, 4 | 16) == E.ERR_ARG
    assert call(p._h, 0, 4, out=False) == E.ERR_ARG
    assert call(p._h, 0, 4, cert=False) == E.ERR_ARG
    assert E.certificate_info()["calls"] == before  # refused before anything is asked of the device


def test_the_existing_entry_points_still_refuse_the_flag():
    import ellp_amd as L
    H = L.host_lib()
    p = _small_problem()
    rr = L._ResultRng()
    assert H.ellp_solve_flags(p._h, 0, 1000, None, 4, C.byref(rr)) == E.ERR_ARG
    assert H.ellp_solve_flags(p._h, 0, 1000, None, 1 | 4, C.byref(rr)) == E.ERR_ARG
    st, keep = L._start_struct({"B": [1]})
    rep = L._StartReport()
    assert H.ellp_solve_start(p._h, 0, 1000, None, 4, C.byref(st), C.byref(rr), C.byref(rep)) == E.ERR_ARG


def test_endings_the_set_up_decides_carry_a_reason_and_make_no_device_call():
    """infeasibility found while the standard form is built, and problems without rows (the trivial solver): no certificate,
    the documented reason, and not one certificate call"""
    import ellp_amd as L
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import known_answers
    want = {"two_variables_infeasible_free": "infeasibility decided by the set-up",
            "infeasible_constraint_without_coeffs": "infeasibility decided by the set-up",
            "infeasible_constraint_without_coeffs_and_no_vars": "infeasibility decided by the set-up",
            "linear_system_3d_infeasible": "infeasibility decided by the set-up",
            "one_variable_unbounded_upper": "no rows: decided by the trivial solver",
            "one_variable_unbounded_free": "no rows: decided by the trivial solver",
            "two_variables_unbounded": "no rows: decided by the trivial solver"}
    fx = {p["name"]: p for p in known_answers()["problems"]}
    before = E.certificate_info()["calls"]
    for name, reason in want.items():
        for S in (L.PrimalSimplexSolver, L.DualSimplexSolver):
            plain = S.default().solve(L.Problem.from_fixture(fx[name]))
            res = S.default().solve(L.Problem.from_fixture(fx[name]), certificate=True)
            assert res.kind == plain.kind == fx[name]["check"] and res.iters == plain.iters, name
            assert res.certificate is None and res.certificate_reason == reason, (name, res.certificate_reason)
            assert plain.certificate is None and plain.certificate_reason is None
    assert E.certificate_info()["calls"] == before


def test_engine_certificate_refuses_a_null_engine():
    v, i = np.zeros(4), E.CertInfo()
    err = C.create_string_buffer(512)
    before = E.certificate_info()["calls"]
    s = E.lib().ellp_engine_certificate(None, E.CERT_FARKAS_ROW, 1, None, None, None, E._p(v), C.byref(i), err, 512)
    assert s == E.ERR_ARG and b"no engine" in err.value
    assert E.certificate_info()["calls"] == before + 1  # a refused call counts: the counter shows who called


@pytest.mark.parametrize("what", ["source", "source_neg", "n_check_0", "n_check_big", "vec", "info", "chk_one", "chk_two", "chk_kind"])
def test_certificate_refuses_its_own_arguments(what):
    fp = _flat()
    kw = {}
    k3 = (np.full(fp.n, 1, dtype=np.uint8), np.zeros(fp.n), np.zeros(fp.n))
    if what == "source":
        kw["source"] = 3
    elif what == "source_neg":
        kw["source"] = -1
    elif what == "n_check_0":
        kw["n_check"] = 0
    elif what == "n_check_big":
        kw["n_check"] = fp.n + 1
    elif what == "vec":
        kw["vec"] = False
    elif what == "info":
        kw["info"] = False
    elif what == "chk_one":
        kw["chk"] = (k3[0], None, None)
    elif what == "chk_two":
        kw["chk"] = (k3[0], k3[1], None)
    elif what == "chk_kind":
        k3[0][fp.n - 1] = 5
        kw["chk"] = k3
    s, msg = _call(fp, **kw)
    assert s == E.ERR_ARG and msg.startswith("certificate:"), (what, s, msg)


@pytest.mark.parametrize("what", ["m0", "m_too_large", "nB", "sum", "B_range", "N_range", "Nb_range", "kind_range", "null_A", "null_x", "null_B"])
def test_certificate_makes_the_refusals_of_the_postsolve(what):
    fp = _flat()
    a = fp._args()  # m, n, n_c, A, c, b, kind, lb, ub, x, B, nB, N, Nb, nN
    n_check = 1
    if what == "m0":
        a[0] = 0
    elif what == "m_too_large":
        a[0] = a[11] = 8193
        a[1] = a[2] = 8193 + fp.nN
    elif what == "nB":
        a[11] = fp.m - 1
    elif what == "sum":
        a[14] = fp.nN - 1
    elif what == "B_range":
        fp.B[1] = fp.n
    elif what == "N_range":
        fp.N[0] = -1
    elif what == "Nb_range":
        fp.Nb[2] = 3
    elif what == "kind_range":
        fp.kind[0] = 5
    elif what == "null_A":
        a[3] = None
    elif what == "null_x":
        a[9] = None
    elif what == "null_B":
        a[10] = None
    for source in (E.CERT_FARKAS_COSTS, E.CERT_FARKAS_ROW, E.CERT_RAY_COLUMN):
        s, msg = _call(fp, a, source=source, n_check=n_check)
        assert s == E.ERR_ARG and msg, (what, source, s, msg)

"""ellp_amd — MI355X-native revised-simplex pivot engine behind kehlert/ellp's solver API.

The names exported here mirror the reference crate's public API (src/lib.rs:109-129):

    Problem, Bound, ConstraintOp, PrimalSimplexSolver, DualSimplexSolver, SolverResult,
    EllPError, parse_mps

`Problem` / `StandardForm` / phase construction live in the C++ host mirror
(ellp_amd/csrc/host, libellp_host.so); the per-iteration simplex loops
(`solve_with_initial`) run on the GPU through the C ABI of include/ellp_hip.h
(libellp_hip.so, hand-written HIP for gfx950).  There is no CPU implementation of the loops in
this package: without the built libraries / a HIP device, solving raises.
"""
import ctypes as C
import os

import numpy as np

from . import _engine
from ._engine import MAX_ITER_NONE, Opts

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.path.join(_HERE, "libellp_host.so")

__all__ = ["Problem", "Bound", "ConstraintOp", "PrimalSimplexSolver", "DualSimplexSolver", "SolverResult",
           "EllPError", "MpsParsingError", "parse_mps"]


class EllPError(Exception):
    """src/error.rs:3-11"""


class MpsParsingError(Exception):
    """src/parse_mps.rs:11-15"""


class Bound:
    """src/problem.rs:190-197. Bound.Free / Lower(lb) / Upper(ub) / TwoSided(lb, ub) / Fixed(v)."""
    KINDS = ("Free", "Lower", "Upper", "TwoSided", "Fixed")

    def __init__(self, kind, lb=0.0, ub=0.0):
        self.kind, self.lb, self.ub = kind, float(lb), float(ub)

    Free = None  # set below

    @staticmethod
    def Lower(lb):
        return Bound(1, lb, 0.0)

    @staticmethod
    def Upper(ub):
        return Bound(2, 0.0, ub)

    @staticmethod
    def TwoSided(lb, ub):
        return Bound(3, lb, ub)

    @staticmethod
    def Fixed(v):
        return Bound(4, v, v)

    @staticmethod
    def from_fixture(b):
        kind, lb, ub = b
        k = Bound.KINDS.index(kind)
        return Bound(k, lb, lb if k == 4 else ub)

    def __repr__(self):
        return f"Bound.{self.KINDS[self.kind]}({self.lb}, {self.ub})"


Bound.Free = Bound(0)


class ConstraintOp:
    """src/problem.rs:298-303"""
    Lte, Eq, Gte = 0, 1, 2
    _BY_NAME = {"Lte": 0, "Eq": 1, "Gte": 2}


class _Result(C.Structure):
    _fields_ = [("status", C.c_int), ("obj", C.c_double), ("nx", C.c_int64), ("x", C.POINTER(C.c_double)),
                ("iters_phase1", C.c_uint64), ("iters_phase2", C.c_uint64), ("err", C.c_char * 512)]


class _ResultEx(C.Structure):
    """ellp_result_ex (include/ellp_host.h)"""
    _fields_ = [("result", _Result), ("has_postsolve", C.c_int), ("n_duals", C.c_int64), ("duals", C.POINTER(C.c_double)),
                ("n_reduced_costs", C.c_int64), ("reduced_costs", C.POINTER(C.c_double)), ("kkt", _engine.Kkt)]


class _ResultRng(C.Structure):
    """ellp_result_rng (include/ellp_host.h)"""
    _PD, _PI = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    _fields_ = [("ex", _ResultEx), ("has_ranging", C.c_int), ("n_cost", C.c_int64), ("cost_down", _PD), ("cost_up", _PD),
                ("cost_blocking_down", _PI), ("cost_blocking_up", _PI), ("n_rhs", C.c_int64), ("rhs_down", _PD), ("rhs_up", _PD),
                ("rhs_blocking_down", _PI), ("rhs_blocking_up", _PI), ("inverse_residual", C.c_double), ("n_B", C.c_int64),
                ("n_N", C.c_int64), ("n_x_std", C.c_int64), ("B_index", _PI), ("N_index", _PI), ("row_origin", _PI),
                ("N_bound", C.POINTER(C.c_uint8)), ("x_std", _PD)]


class _Start(C.Structure):
    """ellp_start (include/ellp_host.h)"""
    _fields_ = [("n_B", C.c_int64), ("B_index", C.c_void_p), ("n_N", C.c_int64), ("N_index", C.c_void_p), ("N_bound", C.c_void_p)]


class _StartReport(C.Structure):
    """ellp_start_report (include/ellp_host.h)"""
    _fields_ = [("used", C.c_int), ("reason", C.c_int), ("info", _engine.StartInfo)]


class _ResultCert(C.Structure):
    """ellp_result_cert (include/ellp_host.h)"""
    _fields_ = [("kind", C.c_int), ("reason", C.c_char * 128), ("n", C.c_int64), ("vec", C.POINTER(C.c_double)),
                ("info", _engine.CertInfo)]


class _FlatPhase(C.Structure):
    _fields_ = ([(k, C.c_int64) for k in ("m", "n", "n_c", "n_B", "n_N")] +
                [(k, C.POINTER(C.c_double)) for k in ("A", "c", "b", "lb", "ub", "x", "y", "d")] +
                [("bound_kind", C.POINTER(C.c_uint8)), ("N_bound", C.POINTER(C.c_uint8)),
                 ("B_index", C.POINTER(C.c_int64)), ("N_index", C.POINTER(C.c_int64))])


_host = None


def host_lib():
    """Loads libellp_host.so (which links libellp_hip.so). Raises if either is missing."""
    global _host
    if _host is not None:
        return _host
    _engine.lib()  # the engine must load first; raises with build instructions if missing
    if not os.path.exists(HOST_LIB_PATH):
        raise ImportError(f"{HOST_LIB_PATH} is missing: build it with `python -m ellp_amd.build`")
    L = C.CDLL(HOST_LIB_PATH)
    L.ellp_problem_new.restype = C.c_void_p
    L.ellp_problem_clone.restype = C.c_void_p
    L.ellp_problem_clone.argtypes = [C.c_void_p]
    L.ellp_problem_free.argtypes = [C.c_void_p]
    L.ellp_problem_add_var.restype = C.c_int64
    L.ellp_problem_add_var.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_double, C.c_double, C.c_char_p,
                                       C.c_char_p, C.c_size_t]
    L.ellp_problem_add_var_with_id.restype = C.c_int64
    L.ellp_problem_add_var_with_id.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int64,
                                               C.c_char_p, C.c_char_p, C.c_size_t]
    L.ellp_problem_add_constraint.restype = C.c_int
    L.ellp_problem_add_constraint.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_double,
                                              C.c_char_p, C.c_size_t]
    L.ellp_problem_num_vars.restype = C.c_int64
    L.ellp_problem_num_vars.argtypes = [C.c_void_p]
    L.ellp_problem_num_constraints.restype = C.c_int64
    L.ellp_problem_num_constraints.argtypes = [C.c_void_p]
    L.ellp_problem_is_feasible.restype = C.c_int
    L.ellp_problem_is_feasible.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.ellp_parse_mps.restype = C.c_void_p
    L.ellp_parse_mps.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.ellp_solve.restype = C.c_int
    L.ellp_solve.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(Opts), C.POINTER(_Result)]
    L.ellp_result_free.argtypes = [C.POINTER(_Result)]
    L.ellp_solve_ex.restype = C.c_int
    L.ellp_solve_ex.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(Opts), C.c_int, C.POINTER(_ResultEx)]
    L.ellp_result_ex_free.argtypes = [C.POINTER(_ResultEx)]
    L.ellp_solve_flags.restype = C.c_int
    L.ellp_solve_flags.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(Opts), C.c_uint, C.POINTER(_ResultRng)]
    L.ellp_result_rng_free.argtypes = [C.POINTER(_ResultRng)]
    L.ellp_solve_start.restype = C.c_int
    L.ellp_solve_start.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(Opts), C.c_uint, C.POINTER(_Start),
                                   C.POINTER(_ResultRng), C.POINTER(_StartReport)]
    L.ellp_solve_cert.restype = C.c_int
    L.ellp_solve_cert.argtypes = [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(Opts), C.c_uint, C.POINTER(_Start),
                                  C.POINTER(_ResultRng), C.POINTER(_StartReport), C.POINTER(_ResultCert)]
    L.ellp_result_cert_free.argtypes = [C.POINTER(_ResultCert)]
    L.ellp_debug_map_start.restype = C.c_int
    L.ellp_debug_map_start.argtypes = [C.c_void_p, C.POINTER(_Start), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int64]
    L.ellp_solve_batch_ex.restype = C.c_int
    L.ellp_solve_batch_ex.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_uint64, C.POINTER(Opts), C.c_int, C.c_void_p]
    L.ellp_solve_batch_start.restype = C.c_int
    L.ellp_solve_batch_start.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_uint64, C.POINTER(Opts), C.c_uint, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
    L.ellp_solve_batch_flags.restype = C.c_int
    L.ellp_solve_batch_flags.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_uint64, C.POINTER(Opts), C.c_uint, C.c_void_p, C.c_void_p,
                                         C.c_void_p]
    L.ellp_solve_batch.restype = C.c_int
    L.ellp_solve_batch.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_uint64, C.POINTER(Opts), C.c_void_p]
    L.ellp_debug_phase1.restype = C.c_int
    L.ellp_debug_phase1.argtypes = [C.c_void_p, C.c_int, C.POINTER(_FlatPhase), C.c_char_p, C.c_size_t]
    L.ellp_flat_phase_free.argtypes = [C.POINTER(_FlatPhase)]
    _host = L
    return L


class Problem:
    """src/problem.rs:11-154"""

    def __init__(self, _handle=None):
        self._h = _handle if _handle is not None else host_lib().ellp_problem_new()

    def __del__(self):
        try:
            if self._h:
                host_lib().ellp_problem_free(self._h)
                self._h = None
        except Exception:
            pass

    def clone(self):
        return Problem(host_lib().ellp_problem_clone(self._h))

    def add_var(self, obj_coeff, bound, name=None):
        err = C.create_string_buffer(512)
        vid = host_lib().ellp_problem_add_var(self._h, float(obj_coeff), bound.kind, bound.lb, bound.ub,
                                              None if name is None else name.encode(), err, 512)
        if vid < 0:
            raise EllPError(err.value.decode())
        return vid

    def add_var_with_id(self, obj_coeff, bound, var_id, name=None):
        err = C.create_string_buffer(512)
        vid = host_lib().ellp_problem_add_var_with_id(self._h, float(obj_coeff), bound.kind, bound.lb, bound.ub,
                                                      int(var_id), None if name is None else name.encode(), err, 512)
        if vid < 0:
            raise EllPError(err.value.decode())
        return vid

    def add_constraint(self, coeffs, op, rhs):
        ids = np.asarray([c[0] for c in coeffs], dtype=np.int64)
        cf = np.asarray([c[1] for c in coeffs], dtype=np.float64)
        if isinstance(op, str):
            op = ConstraintOp._BY_NAME[op]
        err = C.create_string_buffer(512)
        rc = host_lib().ellp_problem_add_constraint(self._h, len(ids), ids.ctypes.data_as(C.c_void_p),
                                                    cf.ctypes.data_as(C.c_void_p), int(op), float(rhs), err, 512)
        if rc != 0:
            raise EllPError(err.value.decode())

    def is_feasible(self, x):
        xv = np.ascontiguousarray(x, dtype=np.float64)
        return bool(host_lib().ellp_problem_is_feasible(self._h, xv.ctypes.data_as(C.c_void_p), xv.size))

    @property
    def num_vars(self):
        return host_lib().ellp_problem_num_vars(self._h)

    @property
    def num_constraints(self):
        return host_lib().ellp_problem_num_constraints(self._h)

    @staticmethod
    def from_fixture(fx):
        p = Problem()
        for k, (obj, bound) in enumerate(fx["vars"]):
            p.add_var(obj, Bound.from_fixture(bound), f"x{k + 1}")
        for coeffs, op, rhs in fx["constraints"]:
            p.add_constraint(coeffs, op, rhs)
        return p

    def _debug_phase1(self, solver):
        """Flattened phase-1 arrays (what solve() passes to the engine); None if infeasible by setup."""
        f = _FlatPhase()
        err = C.create_string_buffer(512)
        rc = host_lib().ellp_debug_phase1(self._h, 0 if solver == "primal" else 1, C.byref(f), err, 512)
        if rc == 1:
            return None
        if rc < 0:
            raise EllPError(err.value.decode())

        def arr(p, n, dt):
            return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True) if (p and n) else np.zeros(0, dtype=dt)
        out = dict(m=f.m, n=f.n, n_c=f.n_c, A=arr(f.A, f.m * f.n, np.float64), c=arr(f.c, f.n_c, np.float64),
                   b=arr(f.b, f.m, np.float64), kind=arr(f.bound_kind, f.n_c, np.uint8),
                   lb=arr(f.lb, f.n_c, np.float64), ub=arr(f.ub, f.n_c, np.float64), x=arr(f.x, f.n_c, np.float64),
                   B=arr(f.B_index, f.n_B, np.int64), N=arr(f.N_index, f.n_N, np.int64),
                   Nb=arr(f.N_bound, f.n_N, np.uint8),
                   y=arr(f.y, f.m, np.float64) if f.y else None, d=arr(f.d, f.n_c, np.float64) if f.d else None)
        host_lib().ellp_flat_phase_free(C.byref(f))
        return out


class Solution:
    """src/solver.rs:35-54; with solve(prob, postsolve=True) also duals(), reduced_costs() and kkt().

    Sign convention: the problem is a minimisation, d = c - A^T y, and duals()[i] is the derivative of the optimal objective
    with respect to the right-hand side of constraint i: <= 0 for a binding `<=` row, >= 0 for a binding `>=` row, and 0.0
    for a row the rank check dropped as redundant."""

    def __init__(self, obj, x, post=None, rng=None):
        self._obj, self._x, self._post, self._rng = obj, x, post, rng

    def obj(self):
        return self._obj

    def x(self):
        return self._x

    def _postsolve(self):
        if self._post is None:
            raise EllPError("solve(..., postsolve=True) was not asked for")
        return self._post

    def duals(self):
        """one per constraint of the Problem, in order"""
        return self._postsolve()[0]

    def reduced_costs(self):
        """one per variable of the Problem, in order"""
        return self._postsolve()[1]

    def kkt(self):
        """the report of ellp_kkt (include/ellp_hip.h) as a dict, for the final point in standard form"""
        return self._postsolve()[2]

    def _ranging(self):
        if getattr(self, "_rng", None) is None:
            raise EllPError("solve(..., ranging=True) was not asked for")
        return self._rng

    def cost_ranging(self):
        """(down, up, blocking): for every variable of the Problem, in order, the change of its cost coefficient over which the
        final basis stays optimal: down <= 0 <= up, -+inf unlimited.  blocking: (n, 2) indices of the standard form (below
        the number of variables: that variable, above: a slack), the variable whose reduced cost changes sign first below /
        above, -1 for an unlimited side.  Definitions: include/ellp_hip.h."""
        r = self._ranging()
        return r["cost_down"], r["cost_up"], np.stack([r["cost_blocking_down"], r["cost_blocking_up"]], axis=1)

    def rhs_ranging(self):
        """(down, up, blocking): for every constraint of the Problem, in order, the change of its right-hand side over which the
        final basis stays feasible; a row the rank check dropped: (0.0, 0.0, -1).  blocking as for cost_ranging: the basic
        variable that reaches a bound first."""
        r = self._ranging()
        return r["rhs_down"], r["rhs_up"], np.stack([r["rhs_blocking_down"], r["rhs_blocking_up"]], axis=1)

    def basis(self):
        """the final basis in standard form, as the ranging saw it: dict(B, N, Nb, x, row_origin, inverse_residual); after
        solve(prob, start=...) also without the ranging (then without inverse_residual).  It can be handed back as `start`."""
        if getattr(self, "_rng", None) is None and getattr(self, "_basis", None) is not None:
            return dict(self._basis)
        r = self._ranging()
        return {k: r[k] for k in ("B", "N", "Nb", "x", "row_origin", "inverse_residual")}


class SolverResult:
    """src/solver.rs:6-12: Optimal(Solution) | Infeasible | Unbounded | MaxIter{obj}"""
    Optimal, Infeasible, Unbounded, MaxIter = "optimal", "infeasible", "unbounded", "maxiter"

    def __init__(self, kind, solution=None, obj=None, iters=(0, 0)):
        self.kind, self.solution, self.obj, self.iters = kind, solution, obj, iters
        # solve(..., certificate=True): a dict with kind ("farkas" / "ray"), y (one per constraint, the signs of duals()) or ray
        # (one per variable), reason and the device's report (ellp_cert_info); None where there is none, certificate_reason
        # then says which case it is
        self.certificate, self.certificate_reason = None, None

    def __repr__(self):
        if self.kind == self.Optimal:
            return f"found optimal point with objective {self.solution.obj()}"
        if self.kind == self.MaxIter:
            return f"reached max iterations, current objective = {self.obj}"
        return f"problem is {self.kind}"


class _Solver:
    _KIND = 0

    def __init__(self, max_iter=1000, **engine_opts):
        """Default-constructed solvers have max_iter 1000 (primal…:19-23); `new(None)` is max_iter=None."""
        self.max_iter = MAX_ITER_NONE if max_iter is None else int(max_iter)
        self._opts = _engine.default_opts(**engine_opts) if engine_opts else None

    @classmethod
    def new(cls, max_iter=None, **engine_opts):
        return cls(max_iter, **engine_opts)

    @classmethod
    def default(cls):
        return cls()

    def _solve_cert(self, prob, start, flags):
        st, keep = _start_struct(start) if start is not None else (None, None)
        rr, rep, rc = _ResultRng(), _StartReport(), _ResultCert()
        host_lib().ellp_solve_cert(prob._h, self._KIND, self.max_iter, C.byref(self._opts) if self._opts is not None else None,
                                   flags | 4, C.byref(st) if st is not None else None, C.byref(rr), C.byref(rep), C.byref(rc))
        del keep
        try:
            res = _started_result(rr, rep if start is not None else None, basis=start is not None)
            res.certificate_reason = rc.reason.decode()
            if rc.kind:
                vec = np.ctypeslib.as_array(rc.vec, shape=(rc.n,)).copy() if rc.n else np.zeros(0)
                res.certificate = dict(rc.info.as_dict(), reason=res.certificate_reason, **{"y" if rc.kind == 1 else "ray": vec})
            return res
        finally:
            host_lib().ellp_result_cert_free(C.byref(rc))
            host_lib().ellp_result_rng_free(C.byref(rr))

    def solve(self, prob, start=None, postsolve=False, ranging=False, certificate=False):
        """certificate=True: an Infeasible or Unbounded result carries its proof in .certificate (a Farkas vector or a ray with the
        device's report on it; None with .certificate_reason where the ending is one that has none).  Off by default, and off
        means not one extra device call.

        postsolve=True: an Optimal result's Solution also has duals(), reduced_costs() and kkt() (one more pass on the
        device after the solve; off by default, and off means not one extra device call).  ranging=True (implies the
        postsolve): also cost_ranging(), rhs_ranging() and basis().

        start: a basis to start from — a dict with B and optionally N, Nb (what Solution.basis() returns), or a Solution that
        has a basis.  The point of that basis is made on the device; where it is feasible for this solver's method (primal
        feasible for the primal solver, dual feasible for the dual solver) phase 2 starts there and iters[0] is 0, otherwise
        the solve is exactly the cold one.  Each solver runs its own method only: after a changed right-hand side use the
        dual solver, after a changed cost the primal solver.  The result has .start = dict(used, reason, ...) (reasons:
        include/ellp_host.h), and an Optimal Solution's basis() works without ranging=True, so re-solves chain."""
        if certificate:
            return self._solve_cert(prob, start, (3 if ranging else 0) | (1 if postsolve else 0))
        if start is not None:
            return self._solve_start(prob, start, (3 if ranging else 0) | (1 if postsolve else 0))
        if ranging:
            rr = _ResultRng()
            host_lib().ellp_solve_flags(prob._h, self._KIND, self.max_iter,
                                        C.byref(self._opts) if self._opts is not None else None, 3, C.byref(rr))
            try:
                res = _to_result(rr.ex.result)
                if res.kind == SolverResult.Optimal:
                    rx = rr.ex
                    arr = lambda p, n: np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, dtype=p._type_)
                    if rx.has_postsolve:
                        res.solution._post = (arr(rx.duals, rx.n_duals), arr(rx.reduced_costs, rx.n_reduced_costs), rx.kkt.as_dict())
                    if rr.has_ranging:
                        res.solution._rng = dict(
                            cost_down=arr(rr.cost_down, rr.n_cost), cost_up=arr(rr.cost_up, rr.n_cost),
                            cost_blocking_down=arr(rr.cost_blocking_down, rr.n_cost), cost_blocking_up=arr(rr.cost_blocking_up, rr.n_cost),
                            rhs_down=arr(rr.rhs_down, rr.n_rhs), rhs_up=arr(rr.rhs_up, rr.n_rhs),
                            rhs_blocking_down=arr(rr.rhs_blocking_down, rr.n_rhs), rhs_blocking_up=arr(rr.rhs_blocking_up, rr.n_rhs),
                            B=arr(rr.B_index, rr.n_B), N=arr(rr.N_index, rr.n_N), Nb=arr(rr.N_bound, rr.n_N),
                            x=arr(rr.x_std, rr.n_x_std), row_origin=arr(rr.row_origin, rr.n_B),
                            inverse_residual=float(rr.inverse_residual))
                return res
            finally:
                host_lib().ellp_result_rng_free(C.byref(rr))
        if postsolve:
            rx = _ResultEx()
            host_lib().ellp_solve_ex(prob._h, self._KIND, self.max_iter,
                                     C.byref(self._opts) if self._opts is not None else None, 1, C.byref(rx))
            try:
                res = _to_result(rx.result)
                if res.kind == SolverResult.Optimal and rx.has_postsolve:
                    y = np.ctypeslib.as_array(rx.duals, shape=(rx.n_duals,)).copy() if rx.n_duals else np.zeros(0)
                    d = (np.ctypeslib.as_array(rx.reduced_costs, shape=(rx.n_reduced_costs,)).copy()
                         if rx.n_reduced_costs else np.zeros(0))
                    res.solution._post = (y, d, rx.kkt.as_dict())
                return res
            finally:
                host_lib().ellp_result_ex_free(C.byref(rx))
        r = _Result()
        host_lib().ellp_solve(prob._h, self._KIND, self.max_iter,
                              C.byref(self._opts) if self._opts is not None else None, C.byref(r))
        try:
            return _to_result(r)
        finally:
            host_lib().ellp_result_free(C.byref(r))

    def _solve_start(self, prob, start, flags):
        st, keep = _start_struct(start)
        rr, rep = _ResultRng(), _StartReport()
        host_lib().ellp_solve_start(prob._h, self._KIND, self.max_iter, C.byref(self._opts) if self._opts is not None else None,
                                    flags, C.byref(st), C.byref(rr), C.byref(rep))
        del keep
        try:
            return _started_result(rr, rep)
        finally:
            host_lib().ellp_result_rng_free(C.byref(rr))

    def solve_batch(self, problems, starts=None, postsolve=False, ranging=False):
        """solve() of every problem in `problems`: the device loops of all problems the LU-per-iteration kernels take run
        in batched launches, one workgroup per problem; the others are solved one by one.  The primal solver sends a
        problem to the device once and runs both of its phases there (ellp_batch_primal_solve): the workgroup that ends
        phase 1 makes the checks, hands off and goes on into phase 2, so no problem waits for another one's phase 1
        (_engine.batch_primal_info() reports the call's launch rounds and uploaded bytes).  The dual solver runs phase by
        phase, in lock step.  The batch takes 1 to 128 rows (k_small), and for the primal solver also 129 to 1,024 rows
        where solve() runs the exact kernel k_mid for the whole solve (pipeline=3, or pipeline 0 with m <=
        ELLP_MID_AUTO_MAX; for the dual solver also bound flipping).  The dual's phase-1 starts of those problems, which solve() builds on the device,
        are built for all of them in one batched call (ellp_batch_dual_phase1_start).  Returns a list with one entry per problem: the SolverResult
        solve(p) returns, or, where solve(p) would raise, the exception instance it would raise (returned, not raised).
        Results are those of solve(p) to the bit.

        postsolve=True: every Optimal entry's Solution also has duals(), reduced_costs() and kkt(), with the bits of
        solve(p, postsolve=True), from ONE batched call for the whole batch (ellp_batch_postsolve: one workgroup per problem
        up to 128 rows; _engine.batch_postsolve_info() reports its launches, items and chunks); where
        solve(p, postsolve=True) would raise, the entry is that exception.  Off by default, and off means not one extra
        device call.

        starts: a list as long as `problems` whose entries are None, a dict or a Solution with a basis, as solve(p, start=s)
        takes them.  Entry k is then solve(problems[k], start=starts[k]) to the bit, and carries its .start where a start was
        given — but the points of all starts are made in ONE batched call (ellp_batch_basis_start: one workgroup per problem
        up to 128 rows; _engine.batch_basis_start_info() reports its launches, items and chunks), and phase 2 of the usable
        starts the batch takes runs in ONE batched call of its own; unusable starts and entries without one join the cold
        batch.  With starts given — even if every entry is None — every Optimal entry has basis(), so batches chain:
        r1 = solve_batch(ps, starts=[None] * n); solve_batch(ps2, starts=[r.solution if r.kind == "optimal" else None
        for r in r1]).  A length mismatch raises ValueError.  starts=None: the call path without starts, not one extra
        device call.

        ranging=True (implies the postsolve): every Optimal entry's Solution also has cost_ranging(), rhs_ranging() and
        basis(), besides duals(), reduced_costs() and kkt(), with the bits of solve(p, ranging=True) — with starts, of
        solve(p, start=s, ranging=True) — from ONE batched call for the whole batch (ellp_batch_ranging: five launches per
        chunk for the problems up to 128 rows, whatever their number; _engine.batch_ranging_info() reports its launches,
        items and chunks) and no batched postsolve call: the ranging's own duals, reduced costs and report are the
        postsolve.  Where solve(p, ranging=True) would raise, the entry is that exception.  solve_batch(ps2, starts=r1,
        ranging=True) gives a re-solved batch with its ranges in one call.  Off by default, and off takes the paths above
        unchanged, with not one extra device call."""
        problems = list(problems)
        n = len(problems)
        if ranging:
            return self._solve_batch_start(problems, None if starts is None else list(starts), True, ranging=True)
        if starts is not None:
            return self._solve_batch_start(problems, list(starts), postsolve)
        if n == 0:
            return []
        handles = (C.c_void_p * n)(*[p._h for p in problems])
        if postsolve:
            rxs = (_ResultEx * n)()
            L = host_lib()
            s = L.ellp_solve_batch_ex(handles, n, self._KIND, self.max_iter,
                                      C.byref(self._opts) if self._opts is not None else None, 1, rxs)
            if s == _engine.ERR_ARG:
                raise ValueError("solve_batch: invalid arguments")
            out = []
            try:
                for rx in rxs:
                    try:
                        res = _to_result(rx.result)
                    except Exception as e:  # noqa: BLE001 — the exception solve() would raise, handed back
                        out.append(e)
                        continue
                    if res.kind == SolverResult.Optimal and rx.has_postsolve:
                        y = np.ctypeslib.as_array(rx.duals, shape=(rx.n_duals,)).copy() if rx.n_duals else np.zeros(0)
                        d = (np.ctypeslib.as_array(rx.reduced_costs, shape=(rx.n_reduced_costs,)).copy()
                             if rx.n_reduced_costs else np.zeros(0))
                        res.solution._post = (y, d, rx.kkt.as_dict())
                    out.append(res)
            finally:
                for rx in rxs:
                    L.ellp_result_ex_free(C.byref(rx))
            return out
        rs = (_Result * n)()
        L = host_lib()
        s = L.ellp_solve_batch(handles, n, self._KIND, self.max_iter,
                               C.byref(self._opts) if self._opts is not None else None, rs)
        if s == _engine.ERR_ARG:
            raise ValueError("solve_batch: invalid arguments")
        out = []
        try:
            for r in rs:
                try:
                    out.append(_to_result(r))
                except Exception as e:  # noqa: BLE001 — the exception solve() would raise, handed back
                    out.append(e)
        finally:
            for r in rs:
                L.ellp_result_free(C.byref(r))
        return out


    def _solve_batch_start(self, problems, starts, postsolve, ranging=False):
        """the batch through ellp_solve_batch_start, or with ranging=True through ellp_solve_batch_flags (starts may then be
        None: no problem has a start)"""
        n = len(problems)
        given = starts is not None
        if not given:
            starts = [None] * n
        if len(starts) != n:
            raise ValueError(f"solve_batch: {len(starts)} starts for {n} problems")
        for s in starts:
            if s is not None and not isinstance(s, (dict, Solution)):
                raise TypeError("solve_batch: a start is None, a dict(B[, N, Nb]) or a Solution with a basis")
        if n == 0:
            return []
        structs = [None if s is None else _start_struct(s) for s in starts]  # (ellp_start, the arrays it points into)
        handles = (C.c_void_p * n)(*[p._h for p in problems])
        sptr = (C.POINTER(_Start) * n)(*[None if st is None else C.pointer(st[0]) for st in structs])
        rrs, reps = (_ResultRng * n)(), (_StartReport * n)()
        L = host_lib()
        o = C.byref(self._opts) if self._opts is not None else None
        if ranging:
            s = L.ellp_solve_batch_flags(handles, n, self._KIND, self.max_iter, o, 3, sptr if given else None, rrs, reps if given else None)
        else:
            s = L.ellp_solve_batch_start(handles, n, self._KIND, self.max_iter, o, 1 if postsolve else 0, sptr, rrs, reps)
        del structs
        if s == _engine.ERR_ARG:
            raise ValueError("solve_batch: invalid arguments")
        out = []
        try:
            for k in range(n):
                try:
                    out.append(_started_result(rrs[k], reps[k] if starts[k] is not None else None))
                except Exception as e:  # noqa: BLE001 — the exception solve() would raise, handed back
                    out.append(e)
        finally:
            for rr in rrs:
                L.ellp_result_rng_free(C.byref(rr))
        return out


def _started_result(rr, rep, basis=True):
    """SolverResult from a filled ellp_result_rng of ellp_solve_start / ellp_solve_batch_start: .start from the report (None: the
    problem had no start), and on Optimal the postsolve, the basis and the ranging that came with it (basis False: a result of
    ellp_solve_cert without a start, which carries the basis only with the ranging)"""
    res = _to_result(rr.ex.result)
    if rep is not None:
        res.start = dict(rep.info.as_dict(), used=bool(rep.used), reason=int(rep.reason))
    if res.kind == SolverResult.Optimal:
        rx = rr.ex
        arr = lambda p, n: np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, dtype=p._type_)
        if rx.has_postsolve:
            res.solution._post = (arr(rx.duals, rx.n_duals), arr(rx.reduced_costs, rx.n_reduced_costs), rx.kkt.as_dict())
        if not basis and not rr.has_ranging:
            return res
        res.solution._basis = dict(B=arr(rr.B_index, rr.n_B), N=arr(rr.N_index, rr.n_N), Nb=arr(rr.N_bound, rr.n_N),
                                   x=arr(rr.x_std, rr.n_x_std), row_origin=arr(rr.row_origin, rr.n_B))
        if rr.has_ranging:
            res.solution._rng = dict(
                cost_down=arr(rr.cost_down, rr.n_cost), cost_up=arr(rr.cost_up, rr.n_cost),
                cost_blocking_down=arr(rr.cost_blocking_down, rr.n_cost), cost_blocking_up=arr(rr.cost_blocking_up, rr.n_cost),
                rhs_down=arr(rr.rhs_down, rr.n_rhs), rhs_up=arr(rr.rhs_up, rr.n_rhs),
                rhs_blocking_down=arr(rr.rhs_blocking_down, rr.n_rhs), rhs_blocking_up=arr(rr.rhs_blocking_up, rr.n_rhs),
                inverse_residual=float(rr.inverse_residual), **res.solution._basis)
    return res


def _start_struct(start):
    """ellp_start from a dict(B[, N, Nb]) or a Solution with a basis; the second value keeps the arrays alive"""
    if isinstance(start, Solution):
        start = start.basis()
    B = np.ascontiguousarray(start["B"], dtype=np.int64)
    N = np.ascontiguousarray(start["N"], dtype=np.int64) if start.get("N") is not None else None
    Nb = np.ascontiguousarray(start["Nb"], dtype=np.uint8) if N is not None and start.get("Nb") is not None else None
    if Nb is not None and len(Nb) != len(N):
        raise ValueError("start: N and Nb differ in length")
    st = _Start(len(B), B.ctypes.data, 0 if N is None else len(N), None if N is None else max(N.ctypes.data, 1),
                None if Nb is None else Nb.ctypes.data)
    return st, (B, N, Nb)


def _debug_map_start(prob, start):
    """the start as solve(prob, start=...) maps it into the standard form, on the host: (reason, rows, cols, B, N, Nb)"""
    st, keep = _start_struct(start)
    cap = prob.num_vars + prob.num_constraints + 1
    B, N, Nb = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.uint8)
    rows, cols = C.c_int64(0), C.c_int64(0)
    rc = host_lib().ellp_debug_map_start(prob._h, C.byref(st), C.byref(rows), C.byref(cols), B.ctypes.data, N.ctypes.data,
                                         Nb.ctypes.data, cap)
    del keep
    m, n = rows.value, cols.value
    if rc != 0:
        return rc, m, n, None, None, None
    return 0, m, n, B[:m].copy(), N[:n - m].copy(), Nb[:n - m].copy()


def _to_result(r):
    """SolverResult from a filled ellp_result; raises what solve() raises for it"""
    st, msg = r.status, r.err.decode()
    iters = (r.iters_phase1, r.iters_phase2)
    if st == _engine.OPTIMAL:
        x = np.ctypeslib.as_array(r.x, shape=(r.nx,)).copy() if r.nx else np.zeros(0)
        return SolverResult(SolverResult.Optimal, Solution(r.obj, x), iters=iters)
    if st == _engine.INFEASIBLE:
        return SolverResult(SolverResult.Infeasible, iters=iters)
    if st == _engine.UNBOUNDED:
        return SolverResult(SolverResult.Unbounded, iters=iters)
    if st == _engine.MAXITER:
        return SolverResult(SolverResult.MaxIter, obj=r.obj, iters=iters)
    if st in (_engine.ERR_BAD_DIMS, _engine.ERR_SINGULAR):
        raise EllPError(msg)
    if st == _engine.ERR_DEVICE:
        raise _engine.EllpHipError(st, msg)
    raise RuntimeError(f"panic: {msg}")


class PrimalSimplexSolver(_Solver):
    """src/solvers/primal/primal_simplex_solver.rs:15-93"""
    _KIND = 0


class DualSimplexSolver(_Solver):
    """src/solvers/dual/dual_simplex_solver.rs:16-108"""
    _KIND = 1


def parse_mps(text):
    """src/parse_mps.rs:23"""
    err = C.create_string_buffer(512)
    h = host_lib().ellp_parse_mps(text.encode(), err, 512)
    if not h:
        raise MpsParsingError(err.value.decode())
    return Problem(h)

"""ctypes binding of the C ABI in include/ellp_hip.h (libellp_hip.so).

The library is the product's compute path; there is no Python or CPU substitute.  If it is
missing or cannot be loaded this module raises — it never falls back.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ELLP_HIP_LIB") or os.path.join(_HERE, "libellp_hip.so")  # override: dev builds only

OPTIMAL, INFEASIBLE, UNBOUNDED, MAXITER = 0, 1, 2, 3
ERR_BAD_DIMS, ERR_SINGULAR, ERR_NAN, ERR_DEVICE, ERR_ARG, ERR_PANIC = -1, -2, -3, -4, -5, -6
STATUS_NAME = {0: "optimal", 1: "infeasible", 2: "unbounded", 3: "maxiter", -1: "err_bad_dims",
               -2: "err_singular", -3: "err_nan", -4: "err_device", -5: "err_arg", -6: "err_panic"}
MAX_ITER_NONE = 2**64 - 1
ENGINE_PRIMAL, ENGINE_DUAL = 0, 1
# ellp_opts.flags (include/ellp_hip.h)
FLAG_DENSE_PRICING, FLAG_DUAL_MAX_VIOLATION, FLAG_PRIMAL_STEEPEST_EDGE, FLAG_NO_CERTIFY, FLAG_DUAL_BOUND_FLIPPING = 1, 2, 4, 8, 16
K_NAMES = ["price", "select", "ftran", "ratio", "update", "btran", "refactor", "dleave", "dprice",
           "dselect", "dupdate", "event_cost"]
K_COUNT = 12
TAP_U, TAP_R, TAP_D, TAP_BINV, TAP_KEY, TAP_ALPHA, TAP_STATE = range(7)
TAP_SE_GAMMA = 7  # steepest-edge weights by nonbasic position, as the LAST pricing launch left them (include/ellp_hip.h)
TAP_RESYNC_T, TAP_RESYNC_CAND = 8, 9  # t = b - A_N x_N and cand = B^-1 t of the last x_B resync, m doubles each
TAP_REBUILD_PERM = 10  # test hook: pivot row of each basic column in the last rebuild of B^-1, m doubles; ERR_ARG after the shortcut


class Opts(C.Structure):
    _fields_ = [("max_iter", C.c_uint64), ("eps", C.c_double), ("device", C.c_int32),
                ("refactor_period", C.c_int32), ("btran_mode", C.c_int32),
                ("poll_interval", C.c_int32), ("profile", C.c_int32), ("use_graph", C.c_int32),
                ("pipeline", C.c_int32), ("trace_len", C.c_int32), ("partial_segments", C.c_int32),
                ("flags", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("iters", C.c_uint64), ("pivots", C.c_uint64), ("bound_flips", C.c_uint64),
                ("refactors", C.c_uint64), ("obj", C.c_double), ("t_loop_s", C.c_double),
                ("t_setup_s", C.c_double), ("kernel_ms", C.c_double * K_COUNT),
                ("kernel_calls", C.c_uint64 * K_COUNT)]

    def as_dict(self):
        d = {k: getattr(self, k) for k in ("iters", "pivots", "bound_flips", "refactors", "obj",
                                           "t_loop_s", "t_setup_s")}
        d["kernel_ms"] = {K_NAMES[i]: self.kernel_ms[i] for i in range(K_COUNT) if self.kernel_calls[i]}
        d["kernel_calls"] = {K_NAMES[i]: self.kernel_calls[i] for i in range(K_COUNT) if self.kernel_calls[i]}
        return d


class Kkt(C.Structure):
    """ellp_kkt (include/ellp_hip.h): the report of a postsolve"""
    _fields_ = [("primal_residual", C.c_double), ("bound_violation", C.c_double), ("dual_infeasibility", C.c_double),
                ("basic_reduced_cost", C.c_double), ("y_backward_error", C.c_double), ("primal_obj", C.c_double),
                ("dual_obj", C.c_double), ("worst_row", C.c_int64), ("worst_bound_var", C.c_int64),
                ("worst_dual_var", C.c_int64), ("refinement_steps", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


START_KEEP_LABELS, START_LABELS_BY_D = 0, 1


class StartInfo(C.Structure):
    """ellp_start_info (include/ellp_hip.h): the measures of a point made from a basis"""
    _fields_ = [("primal_infeasibility", C.c_double), ("primal_infeasibility_sum", C.c_double),
                ("dual_infeasibility", C.c_double), ("x_backward_error", C.c_double), ("worst_primal_var", C.c_int64),
                ("worst_dual_var", C.c_int64), ("labels_changed", C.c_int64), ("primal_feasible", C.c_int32),
                ("dual_feasible", C.c_int32), ("x_refinement_steps", C.c_int32), ("reserved", C.c_int32), ("kkt", Kkt)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("reserved", "kkt")}
        d["kkt"] = self.kkt.as_dict()
        return d


CERT_FARKAS_COSTS, CERT_FARKAS_ROW, CERT_RAY_COLUMN = 0, 1, 2
CERT_KIND_NAME = {0: None, 1: "farkas", 2: "ray"}


class CertInfo(C.Structure):
    """ellp_cert_info (include/ellp_hip.h): what a certificate call found and how good a proof it is"""
    _fields_ = [("kind", C.c_int32), ("found", C.c_int32), ("source", C.c_int64), ("qualifying", C.c_int64),
                ("gap", C.c_double), ("y_b", C.c_double), ("sup", C.c_double), ("dir_violation", C.c_double),
                ("residual", C.c_double), ("c_r", C.c_double), ("bound_dir_violation", C.c_double), ("norm", C.c_double),
                ("worst_dir_var", C.c_int64), ("worst_row", C.c_int64), ("worst_bound_var", C.c_int64),
                ("refine_steps", C.c_int32), ("reserved", C.c_int32)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}
        d["kind"] = CERT_KIND_NAME.get(d["kind"])
        return d


# int fn(void *user, void *host_buffer, int64_t segment_bytes, int world)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int)


class RangingInfo(C.Structure):
    """ellp_ranging_info (include/ellp_hip.h)"""
    _fields_ = [("inverse_residual", C.c_double), ("reserved", C.c_int64), ("kkt", Kkt)]


class RangingOut(C.Structure):
    """ellp_ranging_out (include/ellp_hip.h): caller-owned arrays, any of which may be NULL"""
    _fields_ = [("cost_down", C.c_void_p), ("cost_up", C.c_void_p), ("cost_blocking_down", C.c_void_p),
                ("cost_blocking_up", C.c_void_p), ("rhs_down", C.c_void_p), ("rhs_up", C.c_void_p),
                ("rhs_blocking_down", C.c_void_p), ("rhs_blocking_up", C.c_void_p), ("d", C.c_void_p),
                ("y", C.c_void_p), ("info", C.POINTER(RangingInfo))]


class Ranging:
    """The arrays of one ranging call.  cost_*: n_c entries by variable; rhs_*: m entries by row; all limits are changes with
    down <= 0 <= up, -+inf unlimited, blocking -1 then; d, y: the reduced costs the ratios were formed from and the duals behind
    them; kkt: the report of the underlying postsolve."""

    def __init__(self, m, n_c):
        self.cost_down, self.cost_up = np.zeros(n_c), np.zeros(n_c)
        self.cost_blocking_down, self.cost_blocking_up = np.zeros(n_c, dtype=np.int64), np.zeros(n_c, dtype=np.int64)
        self.rhs_down, self.rhs_up = np.zeros(m), np.zeros(m)
        self.rhs_blocking_down, self.rhs_blocking_up = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
        self.d, self.y = np.zeros(n_c), np.zeros(m)
        self._info = RangingInfo()
        self.inverse_residual, self.kkt = float("nan"), None

    ARRAYS = ("cost_down", "cost_up", "cost_blocking_down", "cost_blocking_up", "rhs_down", "rhs_up", "rhs_blocking_down",
              "rhs_blocking_up", "d", "y")

    def _out(self):
        o = RangingOut()
        for name in self.ARRAYS:
            setattr(o, name, getattr(self, name).ctypes.data)
        o.info = C.pointer(self._info)
        return o

    def _done(self):
        self.inverse_residual, self.kkt = float(self._info.inverse_residual), self._info.kkt.as_dict()
        return self


class EllpHipError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"{STATUS_NAME.get(status, status)}: {msg}")
        self.status = status
        self.msg = msg


_lib = None
_PROBLEM_ARGS = [C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                 C.c_int64]


def lib():
    """Loads libellp_hip.so; raises if it is missing (build it with `python -m ellp_amd.build`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP engine is the only compute path of ellp_amd. "
            "Build it with `python -m ellp_amd.build` (hipcc --offload-arch=gfx950).")
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    L.ellp_default_opts.argtypes = [C.POINTER(Opts)]
    L.ellp_hip_device_count.restype = C.c_int
    L.ellp_hip_abi_version.restype = C.c_int
    tail = [C.POINTER(Opts), C.POINTER(Stats), C.c_char_p, C.c_size_t]
    L.ellp_primal_solve_with_initial.restype = C.c_int
    L.ellp_primal_solve_with_initial.argtypes = _PROBLEM_ARGS + tail
    L.ellp_dual_solve_with_initial.restype = C.c_int
    L.ellp_dual_solve_with_initial.argtypes = _PROBLEM_ARGS + [C.c_void_p, C.c_void_p] + tail
    L.ellp_batch_solve_with_initial.restype = C.c_int
    L.ellp_batch_solve_with_initial.argtypes = [C.c_int, C.c_int64, C.c_void_p, C.POINTER(Opts), C.c_void_p, C.c_void_p,
                                                C.c_char_p, C.c_size_t]
    L.ellp_batch_primal_solve.restype = C.c_int
    L.ellp_batch_primal_solve.argtypes = [C.c_int64, C.c_void_p, C.POINTER(Opts), C.c_void_p, C.c_char_p, C.c_size_t]
    L.ellp_batch_primal_info.restype = None
    L.ellp_batch_primal_info.argtypes = [C.c_void_p]
    L.ellp_batch_dual_phase1_start.restype = C.c_int
    L.ellp_batch_dual_phase1_start.argtypes = [C.c_int64, C.c_void_p, C.POINTER(Opts), C.c_void_p, C.c_void_p, C.c_char_p,
                                               C.c_size_t]
    L.ellp_engine_create.restype = C.c_int
    L.ellp_engine_create.argtypes = ([C.c_int] + _PROBLEM_ARGS + [C.c_void_p, C.c_void_p] +
                                     [C.POINTER(Opts), C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t])
    L.ellp_engine_plan.restype = C.c_int
    L.ellp_engine_plan.argtypes = [C.c_int, C.c_int64, C.c_int64, C.POINTER(Opts), C.c_int, C.c_void_p, C.c_int64, C.c_char_p, C.c_size_t]
    L.ellp_engine_run.restype = C.c_int
    L.ellp_engine_run.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(Stats), C.c_char_p, C.c_size_t]
    L.ellp_engine_read_point.restype = C.c_int
    L.ellp_engine_read_point.argtypes = [C.c_void_p] + [C.c_void_p] * 6 + [C.c_char_p, C.c_size_t]
    L.ellp_engine_tap.restype = C.c_int64
    L.ellp_engine_tap.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    L.ellp_engine_refactor.restype = C.c_int
    L.ellp_engine_refactor.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.ellp_engine_refresh.restype = C.c_double
    L.ellp_engine_refresh.argtypes = [C.c_void_p]
    L.ellp_engine_inverse_residual.restype = C.c_double
    L.ellp_engine_inverse_residual.argtypes = [C.c_void_p]
    L.ellp_engine_destroy.argtypes = [C.c_void_p]
    L.ellp_engine_read_trace.restype = C.c_int64
    L.ellp_engine_read_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    L.ellp_engine_request_maintenance.restype = C.c_int
    L.ellp_engine_request_maintenance.argtypes = [C.c_void_p]
    L.ellp_engine_debug_scale_inverse.restype = C.c_int
    L.ellp_engine_debug_scale_inverse.argtypes = [C.c_void_p, C.c_double]
    L.ellp_engine_debug_set_inverse.restype = C.c_int
    L.ellp_engine_debug_set_inverse.argtypes = [C.c_void_p, C.c_void_p]
    L.ellp_engine_debug_set_x.restype = C.c_int
    L.ellp_engine_debug_set_x.argtypes = [C.c_void_p, C.c_void_p]
    L.ellp_engine_set_shard.restype = C.c_int
    L.ellp_engine_set_shard.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_char_p, C.c_size_t]
    L.ellp_engine_segment_doubles.restype = C.c_int64
    L.ellp_engine_segment_doubles.argtypes = [C.c_void_p, C.c_int]
    L.ellp_engine_exchange_info.restype = C.c_int
    L.ellp_engine_exchange_info.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                            C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.ellp_engine_set_stream.restype = C.c_int
    L.ellp_engine_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.ellp_engine_step.restype = C.c_int
    L.ellp_engine_step.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]
    L.ellp_engine_poll.restype = C.c_int
    L.ellp_engine_poll.argtypes = [C.c_void_p, C.POINTER(Stats), C.c_char_p, C.c_size_t]
    L.ellp_engine_rephase.restype = C.c_int
    L.ellp_engine_rephase.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    L.ellp_engine_create_primal_phase1.restype = C.c_int
    L.ellp_engine_create_primal_phase1.argtypes = [C.c_int64, C.c_int64] + [C.c_void_p] * 7 + [
        C.POINTER(Opts), C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
    L.ellp_engine_create_dual_phase1.restype = C.c_int
    L.ellp_engine_create_dual_phase1.argtypes = [C.c_int64, C.c_int64] + [C.c_void_p] * 8 + [
        C.POINTER(Opts), C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
    L.ellp_engine_dual_rephase.restype = C.c_int
    L.ellp_engine_dual_rephase.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_char_p, C.c_size_t]
    L.ellp_hip_qr_transposed.restype = C.c_int
    L.ellp_hip_qr_transposed.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]
    L.ellp_comm_unique_id.restype = C.c_int
    L.ellp_comm_unique_id.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_size_t]
    L.ellp_engine_comm_init.restype = C.c_int
    L.ellp_engine_comm_init.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.ellp_engine_run_sharded.restype = C.c_int
    L.ellp_engine_run_sharded.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(Stats), C.c_char_p, C.c_size_t]
    L.ellp_engine_shard_columns.restype = C.c_int
    L.ellp_engine_shard_columns.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.ellp_engine_set_exchange_callback.restype = C.c_int
    L.ellp_engine_set_exchange_callback.argtypes = [C.c_void_p, EXCHANGE_FN, C.c_void_p]
    L.ellp_engine_mailbox_export.restype = C.c_int
    L.ellp_engine_mailbox_export.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_size_t]
    L.ellp_engine_mailbox_connect.restype = C.c_int
    L.ellp_engine_mailbox_connect.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_size_t]
    L.ellp_engine_mailbox_selftest.restype = C.c_int
    L.ellp_engine_mailbox_selftest.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]
    L.ellp_shard_select_compact.restype = C.c_int
    L.ellp_shard_select_compact.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_double, C.POINTER(C.c_int64),
                                            C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.ellp_shard_pack_doubles.restype = C.c_int64
    L.ellp_shard_pack_doubles.argtypes = [C.c_int64]
    L.ellp_hip_lu_transposed.restype = C.c_int
    L.ellp_hip_lu_transposed.argtypes = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]
    L.ellp_hip_lu_rows.restype = C.c_int
    L.ellp_hip_lu_rows.argtypes = [C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_size_t]
    L.ellp_hip_lu_rows_last_ms.restype = C.c_double
    L.ellp_hip_lu_rows_last_ms.argtypes = []
    L.ellp_engine_shard_info.restype = C.c_int
    L.ellp_engine_shard_info.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.ellp_engine_postsolve.restype = C.c_int
    L.ellp_engine_postsolve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Kkt), C.c_char_p, C.c_size_t]
    L.ellp_engine_ranging.restype = C.c_int
    L.ellp_engine_ranging.argtypes = [C.c_void_p, C.POINTER(RangingOut), C.c_char_p, C.c_size_t]
    L.ellp_ranging.restype = C.c_int
    L.ellp_ranging.argtypes = _PROBLEM_ARGS + [C.POINTER(Opts), C.POINTER(RangingOut), C.c_char_p, C.c_size_t]
    L.ellp_engine_tableau_rows.restype = C.c_int
    L.ellp_engine_tableau_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    L.ellp_postsolve.restype = C.c_int
    L.ellp_postsolve.argtypes = _PROBLEM_ARGS + [C.POINTER(Opts), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Kkt),
                                                 C.c_char_p, C.c_size_t]
    L.ellp_batch_postsolve.restype = C.c_int
    L.ellp_batch_postsolve.argtypes = [C.c_int64, C.c_void_p, C.POINTER(Opts), C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    L.ellp_batch_postsolve_info.restype = None
    L.ellp_batch_postsolve_info.argtypes = [C.POINTER(C.c_uint64)]
    L.ellp_batch_ranging.restype = C.c_int
    L.ellp_batch_ranging.argtypes = [C.c_int64, C.c_void_p, C.POINTER(Opts), C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    L.ellp_batch_ranging_info.restype = None
    L.ellp_batch_ranging_info.argtypes = [C.POINTER(C.c_uint64)]
    L.ellp_batch_solve_info.restype = None
    L.ellp_batch_solve_info.argtypes = [C.POINTER(C.c_uint64)]
    L.ellp_batch_basis_start.restype = C.c_int
    L.ellp_batch_basis_start.argtypes = [C.c_int64, C.c_void_p, C.c_int, C.POINTER(Opts), C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    L.ellp_batch_basis_start_info.restype = None
    L.ellp_batch_basis_start_info.argtypes = [C.POINTER(C.c_uint64)]
    L.ellp_basis_start.restype = C.c_int
    L.ellp_basis_start.argtypes = [C.c_int64, C.c_int64] + [C.c_void_p] * 7 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                   C.POINTER(Opts), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(StartInfo), C.c_char_p, C.c_size_t]
    cert_tail = [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CertInfo), C.c_char_p, C.c_size_t]
    L.ellp_engine_certificate.restype = C.c_int
    L.ellp_engine_certificate.argtypes = [C.c_void_p] + cert_tail
    L.ellp_certificate.restype = C.c_int
    L.ellp_certificate.argtypes = _PROBLEM_ARGS + [C.POINTER(Opts)] + cert_tail
    L.ellp_certificate_info.restype = None
    L.ellp_certificate_info.argtypes = [C.POINTER(C.c_uint64)]
    _lib = L
    return L


def _cert_args(m, n, source, n_check, chk, vec):
    """the trailing arguments of the two certificate calls: (source, n_check, chk_kind, chk_lb, chk_ub, vec, info) and what
    keeps the arrays alive"""
    n_check = int(n if n_check is None else n_check)
    if chk is None:
        keep = (None, None, None)
    else:
        keep = (np.ascontiguousarray(chk[0], dtype=np.uint8), _f64(chk[1]), _f64(chk[2]))
        if min(a.size for a in keep) < n_check:
            raise ValueError("certificate: chk arrays shorter than n_check")
    if vec is None:
        vec = np.zeros(max(m if source != CERT_RAY_COLUMN else n_check, 1))
    return n_check, keep, vec, CertInfo()


def certificate(fp, source, n_check=None, chk=None, opts=None, vec=None):
    """ellp_certificate on the basis, labels and point a FlatProblem holds: (vec or None, info_dict).  source: CERT_FARKAS_COSTS,
    CERT_FARKAS_ROW (vec: m entries by row) or CERT_RAY_COLUMN (vec: n_check entries by variable); n_check: the leading columns
    the report is made on (default all); chk = (kind, lb, ub): the bounds it is made against (default the problem's own);
    vec: an array to fill (left as it is unless info["found"]).  Raises EllpHipError on any status but OPTIMAL."""
    o = opts or default_opts()
    n_check, keep, vec, info = _cert_args(fp.m, fp.n, source, n_check, chk, vec)
    err = C.create_string_buffer(512)
    s = lib().ellp_certificate(*fp._args(), C.byref(o), int(source), n_check, _p(keep[0]), _p(keep[1]), _p(keep[2]), _p(vec),
                               C.byref(info), err, 512)
    if s != OPTIMAL:
        raise EllpHipError(s, err.value.decode())
    return (vec if info.found else None), info.as_dict()


def certificate_info():
    """ellp_certificate_info: calls of the two certificate entry points so far in this process, and the kernel launches and
    refinement steps of the last one"""
    out = (C.c_uint64 * 4)()
    lib().ellp_certificate_info(out)
    return {"calls": int(out[0]), "launches": int(out[1]), "refine_steps": int(out[2])}


def qr_transposed(A, device=-1):
    """Column-pivoted Householder QR of A^T on the device (standard_form.rs:142).  A: (m, nv) array.
    Returns (pivots, |R_ii|), both of length min(m, nv)."""
    A = np.asfortranarray(A, dtype=np.float64)
    m, nv = A.shape
    mn = min(m, nv)
    piv = np.zeros(mn, dtype=np.int64)
    rd = np.zeros(mn, dtype=np.float64)
    err = C.create_string_buffer(512)
    s = lib().ellp_hip_qr_transposed(m, nv, A.ctypes.data_as(C.c_void_p), _p(piv), _p(rd), int(device), err, 512)
    if s != OPTIMAL:
        raise EllpHipError(s, err.value.decode())
    return piv, rd


def lu_transposed(A, device=-1):
    """LU with partial pivoting of A^T on the device (dual_problem.rs:141).  A: (m, nv) array, nv >= m.
    Returns (pivots, U_ii), both of length m."""
    A = np.asfortranarray(A, dtype=np.float64)
    m, nv = A.shape
    piv = np.zeros(m, dtype=np.int64)
    ud = np.zeros(m, dtype=np.float64)
    err = C.create_string_buffer(512)
    s = lib().ellp_hip_lu_transposed(m, nv, A.ctypes.data_as(C.c_void_p), _p(piv), _p(ud), int(device), err, 512)
    if s != OPTIMAL:
        raise EllpHipError(s, err.value.decode())
    return piv, ud


def lu_rows(M, blocked=True, device=-1):
    """LU with partial pivoting of a square matrix by rows on the device, as the exact loop above 1,024 rows factors the basis
    (ellp_hip_lu_rows): blocked (panels of 16 columns) or the unblocked form, the same bytes either way.
    Returns (factors, pivots, U_ii); lu_rows_last_ms() is the device time of the factorisation alone."""
    M = np.ascontiguousarray(M, dtype=np.float64)
    if M.ndim != 2 or M.shape[0] != M.shape[1]:
        raise ValueError("lu_rows needs a square matrix")
    m = M.shape[0]
    fac = np.zeros((m, m), dtype=np.float64)
    piv = np.zeros(m, dtype=np.int64)
    ud = np.zeros(m, dtype=np.float64)
    err = C.create_string_buffer(512)
    s = lib().ellp_hip_lu_rows(m, _p(M), 1 if blocked else 0, _p(fac), _p(piv), _p(ud), int(device), err, 512)
    if s != OPTIMAL:
        raise EllpHipError(s, err.value.decode())
    return fac, piv, ud


def lu_rows_last_ms():
    return float(lib().ellp_hip_lu_rows_last_ms())


def shard_pack_doubles(ld):
    return int(lib().ellp_shard_pack_doubles(int(ld)))


def shard_select_compact(packs, world, ld, eps=1e-10):
    """The ranks' selection on gathered packs (host build of the kernel's code).  Returns (verdict, q,
    src_rank, src_slot): verdict 1 = the full exchange is needed."""
    packs = np.ascontiguousarray(packs, dtype=np.float64)
    q, sr, sc = C.c_int64(-1), C.c_int(-1), C.c_int(0)
    v = lib().ellp_shard_select_compact(_p(packs), int(world), int(ld), float(eps), C.byref(q), C.byref(sr), C.byref(sc))
    return int(v), int(q.value), int(sr.value), int(sc.value)


def comm_unique_id(rccl_path=None):
    """128-byte RCCL unique id (rank 0 creates it, the other ranks receive it)."""
    buf = C.create_string_buffer(128)
    err = C.create_string_buffer(512)
    path = rccl_path.encode() if rccl_path else None
    s = lib().ellp_comm_unique_id(path, buf, err, 512)
    if s != OPTIMAL:
        raise EllpHipError(s, err.value.decode())
    return buf.raw


def default_opts(**kw):
    o = Opts()
    lib().ellp_default_opts(C.byref(o))
    for k, v in kw.items():
        if k == "max_iter" and v is None:
            v = MAX_ITER_NONE
        setattr(o, k, v)
    return o


# what ellp_engine_plan writes, in its order (include/ellp_hip.h)
PLAN_FIELDS = ("ld", "cpb", "nblocks", "priceT", "price_nt", "price_wave", "upd_rows", "upd_blocks", "upd2_rows", "upd2_blocks",
               "ftran_blocks", "btran_rows", "btran_tiles", "upd_stage", "upd_lds", "ftran_lds", "price2_lds", "bl_splits", "nbs",
               "seg", "refactor_period", "ill_tol", "drift_every", "drift_tol", "pp_P", "pp_S", "se", "se_vpart", "dual_maxviol",
               "dual_bflip", "small", "mid", "small_lds", "mid_lds", "small_nt", "mid_nt", "ldn", "hybrid", "cert_large",
               "guard_abs", "exact_K", "exact_large_always", "lagged", "dual_fused", "dual_fold", "unit_table", "stamps")
PLAN_AVAIL_SMALL, PLAN_AVAIL_MID, PLAN_AVAIL_ALL = 1, 2, 3


def engine_plan(kind, m, n_N, opts=None, avail=PLAN_AVAIL_ALL):
    """The engine ellp_engine_create would make for these sizes and options, decided without a device: (status, dict of
    PLAN_FIELDS or None, message).  The environment is read as creation reads it."""
    out = np.zeros(len(PLAN_FIELDS))
    err = C.create_string_buffer(512)
    s = lib().ellp_engine_plan(int(kind), int(m), int(n_N), C.byref(opts) if opts is not None else None, int(avail), _p(out),
                               out.size, err, 512)
    return int(s), (dict(zip(PLAN_FIELDS, out.tolist())) if s == OPTIMAL else None), err.value.decode()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class FlatProblem:
    """The arrays solve_with_initial has in hand (standard_form.rs:21-34), C-ABI shaped.
    A: (m*n,) column-major.  x/B/N/Nb (and y/d) are mutated in place by the solve calls."""

    def __init__(self, m, n, n_c, A, c, b, kind, lb, ub, x, B, N, Nb, y=None, d=None, nN=None):
        self.m, self.n, self.n_c = int(m), int(n), int(n_c)
        self.A, self.c, self.b = _f64(A).reshape(-1), _f64(c), _f64(b)
        self.kind = np.ascontiguousarray(kind, dtype=np.uint8)
        self.lb, self.ub = _f64(lb), _f64(ub)
        self.x = _f64(x).copy()
        self.B = np.ascontiguousarray(B, dtype=np.int64).copy()
        self.N = np.ascontiguousarray(N, dtype=np.int64).copy()
        self.Nb = np.ascontiguousarray(Nb, dtype=np.uint8).copy()
        self.nB = len(self.B)
        self.nN = len(self.N) if nN is None else int(nN)
        self.y = None if y is None else _f64(y).copy()
        self.d = None if d is None else _f64(d).copy()

    def _args(self):
        return [self.m, self.n, self.n_c, _p(self.A), _p(self.c), _p(self.b), _p(self.kind),
                _p(self.lb), _p(self.ub), _p(self.x), _p(self.B), self.nB, _p(self.N), _p(self.Nb),
                self.nN]

    def obj(self):
        return float(np.dot(self.c, self.x))


def primal_solve_with_initial(fp, opts=None):
    """PrimalSimplexSolver::solve_with_initial on the GPU. Returns (status, Stats, errmsg)."""
    o = opts or default_opts()
    st = Stats()
    err = C.create_string_buffer(512)
    s = lib().ellp_primal_solve_with_initial(*fp._args(), C.byref(o), C.byref(st), err, 512)
    return s, st, err.value.decode()


def dual_solve_with_initial(fp, opts=None):
    o = opts or default_opts()
    st = Stats()
    err = C.create_string_buffer(512)
    s = lib().ellp_dual_solve_with_initial(*fp._args(), _p(fp.y), _p(fp.d), C.byref(o), C.byref(st),
                                           err, 512)
    return s, st, err.value.decode()


def postsolve(fp, opts=None):
    """ellp_postsolve: duals, reduced costs, the row residual and the KKT report of the point a FlatProblem holds (the arrays
    a solve_with_initial call left).  Returns (y, d, r, kkt_dict); raises EllpHipError on any status but OPTIMAL."""
    o = opts or default_opts()
    y, d, r, k = np.zeros(max(fp.m, 0)), np.zeros(max(fp.n_c, 0)), np.zeros(max(fp.m, 0)), Kkt()
    err = C.create_string_buffer(512)
    s = lib().ellp_postsolve(*fp._args(), C.byref(o), _p(y), _p(d), _p(r), C.byref(k), err, 512)
    if s != OPTIMAL:
        raise EllpHipError(s, err.value.decode())
    return y, d, r, k.as_dict()


def basis_start(fp, mode=START_KEEP_LABELS, opts=None):
    """ellp_basis_start: the point of the basis a FlatProblem holds (its B, N and Nb; its x is not read; n_c == n): x, y, d and
    the repaired labels, made on the device.  Returns (status, x, y, d, Nb, info_dict) with status OPTIMAL, ERR_SINGULAR or
    ERR_ARG (x, y, d, Nb are then None and info_dict holds only the message); raises EllpHipError on a device error."""
    o = opts or default_opts()
    x, y, d, info = np.zeros(max(fp.n, 0)), np.zeros(max(fp.m, 0)), np.zeros(max(fp.n, 0)), StartInfo()
    Nb = fp.Nb.copy()
    err = C.create_string_buffer(512)
    s = lib().ellp_basis_start(fp.m, fp.n, _p(fp.A), _p(fp.c), _p(fp.b), _p(fp.kind), _p(fp.lb), _p(fp.ub), _p(fp.B), fp.nB,
                               _p(fp.N), _p(Nb), fp.nN, int(mode), C.byref(o), _p(x), _p(y), _p(d), C.byref(info), err, 512)
    if s in (ERR_ARG, ERR_SINGULAR):
        return s, None, None, None, None, {"message": err.value.decode()}
    if s != OPTIMAL:
        raise EllpHipError(s, err.value.decode())
    out = info.as_dict()
    out["message"] = ""
    return s, x, y, d, Nb, out


def ranging(fp, opts=None):
    """ellp_ranging: the cost and right-hand-side ranges of the point a FlatProblem holds (the arrays a solve_with_initial call
    left), by the kernels and with the bits of Engine.ranging.  Returns a Ranging; raises EllpHipError on any status but
    OPTIMAL."""
    o = opts or default_opts()
    rg = Ranging(max(fp.m, 0), max(fp.n_c, 0))
    err = C.create_string_buffer(512)
    s = lib().ellp_ranging(*fp._args(), C.byref(o), C.byref(rg._out()), err, 512)
    if s != OPTIMAL:
        raise EllpHipError(s, err.value.decode())
    return rg._done()


class BatchItem(C.Structure):
    """ellp_batch_item (include/ellp_hip.h)"""
    _fields_ = [("m", C.c_int64), ("n", C.c_int64), ("n_c", C.c_int64), ("A", C.c_void_p), ("c", C.c_void_p),
                ("b", C.c_void_p), ("bound_kind", C.c_void_p), ("lb", C.c_void_p), ("ub", C.c_void_p), ("x", C.c_void_p),
                ("B_index", C.c_void_p), ("n_B", C.c_int64), ("N_index", C.c_void_p), ("N_bound", C.c_void_p),
                ("n_N", C.c_int64), ("y", C.c_void_p), ("d", C.c_void_p), ("err", C.c_char * 256)]


def _fill_item(it, fp, *, x=None, Nb=None, y=None, d=None):
    """A BatchItem from a FlatProblem; x, Nb, y, d: the caller's arrays where the call writes into its own (fp's x and Nb
    otherwise; y and d stay NULL where none is given)."""
    it.m, it.n, it.n_c = fp.m, fp.n, fp.n_c
    it.A, it.c, it.b, it.bound_kind = _p(fp.A), _p(fp.c), _p(fp.b), _p(fp.kind)
    it.lb, it.ub, it.x = _p(fp.lb), _p(fp.ub), _p(fp.x if x is None else x)
    it.B_index, it.n_B = _p(fp.B), fp.nB
    it.N_index, it.N_bound, it.n_N = _p(fp.N), _p(fp.Nb if Nb is None else Nb), fp.nN
    it.y, it.d = _p(y), _p(d)


def _info4(fn, names):
    """The four counters a batched call keeps per thread, under the given names."""
    out = (C.c_uint64 * 4)()
    fn(out)
    return {name: int(v) for name, v in zip(names, out)}


_BATCH_INFO = ("launches", "batched", "single", "chunks")


def batch_solve_with_initial(kind, flat_problems, opts=None):
    """solve_with_initial of every FlatProblem in one batched call (ENGINE_PRIMAL or ENGINE_DUAL).  Returns one
    (status, Stats, errmsg) per problem, as the single-call wrappers do, and mutates the problems in place.  Raises
    EllpHipError if the call as a whole is refused (options, device)."""
    fps = list(flat_problems)
    n = len(fps)
    items = (BatchItem * max(n, 1))()
    for it, fp in zip(items, fps):
        _fill_item(it, fp, y=fp.y, d=fp.d)
    status = (C.c_int * max(n, 1))()
    stats = (Stats * max(n, 1))()
    o = opts or default_opts()
    err = C.create_string_buffer(512)
    s = lib().ellp_batch_solve_with_initial(kind, n, items, C.byref(o), status, stats, err, 512)
    if s != OPTIMAL:
        raise EllpHipError(s, err.value.decode())
    return [(status[k], stats[k], items[k].err.decode()) for k in range(n)]


def batch_solve_info():
    """ellp_batch_solve_info: the calling thread's calls of ellp_batch_solve_with_initial: how many so far, the items and the
    kind of the last one."""
    return _info4(lib().ellp_batch_solve_info, ("calls", "items", "kind"))


class BatchPostOut(C.Structure):
    """ellp_batch_post_out (include/ellp_hip.h)"""
    _fields_ = [("y", C.c_void_p), ("d", C.c_void_p), ("r", C.c_void_p), ("kkt", C.POINTER(Kkt))]


def batch_postsolve(flat_problems, opts=None, fill=0.0):
    """ellp_batch_postsolve: the postsolve of every FlatProblem (the arrays a solve_with_initial call left) in one batched
    call, with the bits of postsolve(fp) per problem.  Returns one (status, y, d, r, kkt_dict, msg) per problem; status is
    OPTIMAL, ERR_ARG or ERR_SINGULAR, and where it is not OPTIMAL y, d and r are as they were made (every entry `fill`: the
    call does not touch them) and kkt_dict is None.  Raises EllpHipError if the call as a whole is refused (device)."""
    fps = list(flat_problems)
    n = len(fps)
    items = (BatchItem * max(n, 1))()
    outs = (BatchPostOut * max(n, 1))()
    kkts = (Kkt * max(n, 1))()
    arrays = []
    for k, (it, fp) in enumerate(zip(items, fps)):
        _fill_item(it, fp)
        y, d, r = np.full(max(fp.m, 0), fill), np.full(max(fp.n_c, 0), fill), np.full(max(fp.m, 0), fill)
        arrays.append((y, d, r))
        outs[k].y, outs[k].d, outs[k].r = y.ctypes.data, d.ctypes.data, r.ctypes.data
        outs[k].kkt = C.pointer(kkts[k])
    status = (C.c_int * max(n, 1))()
    o = opts or default_opts()
    err = C.create_string_buffer(512)
    s = lib().ellp_batch_postsolve(n, items, C.byref(o), outs, status, err, 512)
    if s != OPTIMAL:
        raise EllpHipError(s, err.value.decode())
    return [(status[k], *arrays[k], kkts[k].as_dict() if status[k] == OPTIMAL else None, items[k].err.decode())
            for k in range(n)]


def batch_postsolve_info():
    """ellp_batch_postsolve_info: the calling thread's last ellp_batch_postsolve: kernel launches of the batched path, items
    on the batched kernel, items on the single path (inside the call), chunks."""
    return _info4(lib().ellp_batch_postsolve_info, _BATCH_INFO)


class BatchRangeOut(C.Structure):
    """ellp_batch_range_out (include/ellp_hip.h)"""
    _fields_ = [("out", RangingOut), ("W", C.c_void_p)]


def batch_ranging(flat_problems, opts=None, want_W=False):
    """ellp_batch_ranging: the ranging of every FlatProblem (the arrays a solve_with_initial call left) in one batched call,
    with the bits of ranging(fp) per problem.  Returns one (status, Ranging, W, msg) per problem; status is OPTIMAL, ERR_ARG
    or ERR_SINGULAR, and where it is not OPTIMAL Ranging and W are None.  W (want_W=True, else None): B^-1 as the ranging
    formed it, (m, m) by rows.  Raises EllpHipError if the call as a whole is refused (device)."""
    return [(s, rg if s == OPTIMAL else None, W if s == OPTIMAL else None, msg)
            for s, rg, W, msg in _batch_ranging_raw(flat_problems, opts, want_W)]


def _batch_ranging_raw(flat_problems, opts=None, want_W=False, fill=0.0, wanted=None):
    """batch_ranging with the output arrays handed back whatever the status (for the tests: a failing item leaves them as
    they were made, every entry `fill`).  wanted: per problem None (everything) or the names of Ranging.ARRAYS / "info" asked for; an
    empty list with want_W=False asks for nothing."""
    fps = list(flat_problems)
    n = len(fps)
    items = (BatchItem * max(n, 1))()
    outs = (BatchRangeOut * max(n, 1))()
    keep = []
    for k, (it, fp) in enumerate(zip(items, fps)):
        _fill_item(it, fp)
        rg = Ranging(max(fp.m, 0), max(fp.n_c, 0))
        for name in Ranging.ARRAYS:
            a = getattr(rg, name)
            a[...] = fill if a.dtype != np.int64 else (int(fill) if fill == fill else -7)
        want = None if wanted is None else wanted[k]
        o = rg._out()
        if want is not None:
            for name in Ranging.ARRAYS:
                if name not in want:
                    setattr(o, name, None)
            if "info" not in want:
                o.info = None
        W = np.full((max(fp.m, 0), max(fp.m, 0)), fill) if want_W else None
        outs[k].out = o
        outs[k].W = None if W is None else W.ctypes.data
        keep.append((rg, W))
    status = (C.c_int * max(n, 1))()
    o = opts or default_opts()
    err = C.create_string_buffer(512)
    s = lib().ellp_batch_ranging(n, items, C.byref(o), outs, status, err, 512)
    if s != OPTIMAL:
        raise EllpHipError(s, err.value.decode())
    return [(status[k], keep[k][0]._done() if status[k] == OPTIMAL else keep[k][0], keep[k][1], items[k].err.decode())
            for k in range(n)]


def batch_ranging_info():
    """ellp_batch_ranging_info: the calling thread's last ellp_batch_ranging: kernel launches of the batched path (5 per
    chunk, whatever the item count and the items' shapes: k_brange_front, k_brange_solve, k_brange_tab, k_brange_fold,
    k_post_report_batch), items on the batched kernels, items on the single path (inside the call), chunks."""
    return _info4(lib().ellp_batch_ranging_info, _BATCH_INFO)


def batch_basis_start(flat_problems, mode=START_KEEP_LABELS, opts=None, fill=0.0):
    """ellp_batch_basis_start: the point of the basis of every FlatProblem (as basis_start reads it: B, N and Nb; n_c == n) in
    one batched call, with the bits of basis_start(fp, mode) per problem.  Returns one (status, x, y, d, Nb, info_dict) per
    problem; status is OPTIMAL, ERR_ARG or ERR_SINGULAR, and where it is not OPTIMAL x, y, d are as they were made (every
    entry `fill`), Nb is the copy of the given labels (the call does not touch either) and info_dict holds only the message.
    The problems themselves are not changed.  Raises EllpHipError if the call as a whole is refused (mode, device)."""
    fps = list(flat_problems)
    n = len(fps)
    items = (BatchItem * max(n, 1))()
    infos = (StartInfo * max(n, 1))()
    arrays = []
    for it, fp in zip(items, fps):
        x, y, d = np.full(max(fp.n, 0), fill), np.full(max(fp.m, 0), fill), np.full(max(fp.n, 0), fill)
        Nb = fp.Nb.copy()
        arrays.append((x, y, d, Nb))
        _fill_item(it, fp, x=x, Nb=Nb, y=y, d=d)
    status = (C.c_int * max(n, 1))()
    o = opts or default_opts()
    err = C.create_string_buffer(512)
    s = lib().ellp_batch_basis_start(n, items, int(mode), C.byref(o), infos, status, err, 512)
    if s != OPTIMAL:
        raise EllpHipError(s, err.value.decode())
    out = []
    for k in range(n):
        if status[k] == OPTIMAL:
            info = infos[k].as_dict()
            info["message"] = ""
        else:
            info = {"message": items[k].err.decode()}
        out.append((status[k], *arrays[k], info))
    return out


def batch_basis_start_info():
    """ellp_batch_basis_start_info: the calling thread's last ellp_batch_basis_start: kernel launches of the batched path,
    items on the batched kernel, items on the single path (inside the call), chunks."""
    return _info4(lib().ellp_batch_basis_start_info, _BATCH_INFO)


class BatchPrimalItem(C.Structure):
    """ellp_batch_primal_item (include/ellp_hip.h)"""
    _fields_ = [("p1", BatchItem), ("c2", C.c_void_p), ("bound_kind2", C.c_void_p), ("lb2", C.c_void_p), ("ub2", C.c_void_p)]


class BatchPrimalResult(C.Structure):
    """ellp_batch_primal_result (include/ellp_hip.h)"""
    _fields_ = [("status", C.c_int), ("stage", C.c_int32), ("iters_phase1", C.c_uint64), ("iters_phase2", C.c_uint64),
                ("obj_phase1", C.c_double), ("obj", C.c_double)]


def batch_primal_solve(items, opts=None):
    """ellp_batch_primal_solve: both phases of every primal solve in one batched call.  items: (fp, c2, kind2, lb2, ub2) with
    fp the phase-1 FlatProblem (mutated in place: the point of the phase that ended the solve) and the phase-2 costs and
    bounds (n_c entries each).  Returns one (status, stage, iters_phase1, iters_phase2, obj_phase1, obj, errmsg) per item.
    Raises EllpHipError if the call as a whole is refused (options, arguments, device)."""
    items = list(items)
    n = len(items)
    arr = (BatchPrimalItem * max(n, 1))()
    keep = []
    for it, (fp, c2, kind2, lb2, ub2) in zip(arr, items):
        c2, lb2, ub2 = _f64(c2), _f64(lb2), _f64(ub2)
        kind2 = np.ascontiguousarray(kind2, dtype=np.uint8)
        keep.append((c2, kind2, lb2, ub2))
        _fill_item(it.p1, fp)
        it.c2, it.bound_kind2, it.lb2, it.ub2 = _p(c2), _p(kind2), _p(lb2), _p(ub2)
    res = (BatchPrimalResult * max(n, 1))()
    o = opts or default_opts()
    err = C.create_string_buffer(512)
    s = lib().ellp_batch_primal_solve(n, arr, C.byref(o), res, err, 512)
    if s != OPTIMAL:
        raise EllpHipError(s, err.value.decode())
    return [(res[k].status, res[k].stage, res[k].iters_phase1, res[k].iters_phase2, res[k].obj_phase1, res[k].obj,
             arr[k].p1.err.decode()) for k in range(n)]


def batch_primal_info():
    """ellp_batch_primal_info: the calling thread's last ellp_batch_primal_solve (solve_batch of the primal solver makes one
    per batch): launch rounds, bytes uploaded by the last chunk and by all chunks, chunks."""
    return _info4(lib().ellp_batch_primal_info, ("rounds", "upload_bytes", "upload_bytes_total", "chunks"))


def batch_dual_phase1_start(problems, opts=None):
    """ellp_batch_dual_phase1_start: DualPhase1::new's point for every (m, n, A, c, b, kind, lb, ub, B, N) in one batched
    call.  Returns one (status, obj, errmsg, FlatProblem) per problem; the FlatProblem holds x, Nb, y and d (as
    Engine.dual_phase1 + read_point would).  Raises EllpHipError if the call as a whole is refused (options, device)."""
    fps = []
    for m, n, A, c, b, kind, lb, ub, B, N in problems:
        m, n = int(m), int(n)
        fps.append(FlatProblem(m, n, n, A, c, b, kind, lb, ub, np.zeros(n), B, N, np.zeros(max(n - m, 0), dtype=np.uint8),
                               y=np.zeros(m), d=np.zeros(n)))
    k = len(fps)
    items = (BatchItem * max(k, 1))()
    for it, fp in zip(items, fps):
        _fill_item(it, fp, y=fp.y, d=fp.d)
    status = (C.c_int * max(k, 1))()
    obj = (C.c_double * max(k, 1))()
    o = opts or default_opts()
    err = C.create_string_buffer(512)
    s = lib().ellp_batch_dual_phase1_start(k, items, C.byref(o), status, obj, err, 512)
    if s != OPTIMAL:
        raise EllpHipError(s, err.value.decode())
    return [(status[j], obj[j], items[j].err.decode(), fps[j]) for j in range(k)]


class Engine:
    """Resident engine: tableau stays in HBM between run() slices."""

    def __init__(self, kind, fp, opts=None):
        self.fp = fp
        self.kind = kind
        self._h = C.c_void_p()
        o = opts or default_opts()
        err = C.create_string_buffer(512)
        s = lib().ellp_engine_create(kind, *fp._args(), _p(fp.y), _p(fp.d), C.byref(o),
                                     C.byref(self._h), err, 512)
        if s != OPTIMAL:
            self._h = C.c_void_p()
            raise EllpHipError(s, err.value.decode())

    @classmethod
    def primal_phase1(cls, m, n, A, b, kind, lb, ub, x, Nb, opts=None):
        """Primal phase 1 built on the device (ellp_engine_create_primal_phase1): the standard form and the
        nonbasic start of the n original variables in, an engine with n + m columns out.  Its FlatProblem holds
        the phase-1 arrays as the engine defines them (A is not materialised on the host: fp.A is empty)."""
        m, n = int(m), int(n)
        nt = n + m
        A_ = _f64(A).reshape(-1)
        assert A_.size == m * n
        kind_ = np.concatenate([np.ascontiguousarray(kind, dtype=np.uint8)[:n], np.full(m, 1, dtype=np.uint8)])
        fp = FlatProblem(m, nt, nt, np.zeros(0), np.concatenate([np.zeros(n), np.ones(m)]), b, kind_,
                         np.concatenate([_f64(lb)[:n], np.zeros(m)]), np.concatenate([_f64(ub)[:n], np.zeros(m)]),
                         np.concatenate([_f64(x)[:n], np.zeros(m)]), np.arange(n, nt, dtype=np.int64),
                         np.arange(n, dtype=np.int64), np.ascontiguousarray(Nb, dtype=np.uint8)[:n])
        self = cls.__new__(cls)
        self.fp, self.kind, self._h = fp, ENGINE_PRIMAL, C.c_void_p()
        o = opts or default_opts()
        err = C.create_string_buffer(512)
        xs, Nbs = _f64(x)[:n].copy(), np.ascontiguousarray(Nb, dtype=np.uint8)[:n].copy()
        s = lib().ellp_engine_create_primal_phase1(m, n, _p(A_), _p(fp.b), _p(kind_), _p(fp.lb), _p(fp.ub), _p(xs), _p(Nbs),
                                                   C.byref(o), C.byref(self._h), err, 512)
        if s != OPTIMAL:
            self._h = C.c_void_p()
            raise EllpHipError(s, err.value.decode())
        return self

    @classmethod
    def dual_phase1(cls, m, n, A, c, b, kind, lb, ub, B, N, opts=None):
        """DualPhase1::new's point made on the device (ellp_engine_create_dual_phase1): the box problem's standard
        form and the basis the LU of A^T picked in, a dual engine with y, d, x and the nonbasic labels out
        (read_point brings them into self.fp)."""
        m, n = int(m), int(n)
        fp = FlatProblem(m, n, n, A, c, b, kind, lb, ub, np.zeros(n), B, N, np.zeros(n - m, dtype=np.uint8),
                         y=np.zeros(m), d=np.zeros(n))
        self = cls.__new__(cls)
        self.fp, self.kind, self._h = fp, ENGINE_DUAL, C.c_void_p()
        o = opts or default_opts()
        err = C.create_string_buffer(512)
        s = lib().ellp_engine_create_dual_phase1(m, n, _p(fp.A), _p(fp.c), _p(fp.b), _p(fp.kind), _p(fp.lb), _p(fp.ub),
                                                 _p(fp.B), _p(fp.N), C.byref(o), C.byref(self._h), err, 512)
        if s != OPTIMAL:
            self._h = C.c_void_p()
            raise EllpHipError(s, err.value.decode())
        return self

    def run(self, max_iters):
        st = Stats()
        err = C.create_string_buffer(512)
        s = lib().ellp_engine_run(self._h, int(max_iters), C.byref(st), err, 512)
        if s == ERR_DEVICE:
            raise EllpHipError(s, err.value.decode())
        return s, st, err.value.decode()

    def read_point(self):
        fp = self.fp
        err = C.create_string_buffer(512)
        s = lib().ellp_engine_read_point(self._h, _p(fp.x), _p(fp.B), _p(fp.N), _p(fp.Nb), _p(fp.y),
                                         _p(fp.d), err, 512)
        # OPTIMAL: delivered.  UNBOUNDED / MAXITER: delivered, and completing the iteration the two-launch pipeline had left
        # open ended the solve that way (include/ellp_hip.h) — kept in closing_status.  Every error code raises (the arrays
        # are filled all the same: the caller may look at fp after catching): a point that came with ERR_NAN / ERR_PANIC /
        # ERR_SINGULAR or any code this binding does not know is never returned as a success.
        self.closing_status = s
        if s not in (OPTIMAL, UNBOUNDED, MAXITER):
            raise EllpHipError(s, err.value.decode())
        return fp

    def postsolve(self):
        """ellp_engine_postsolve on the basis and point the engine stands on: (y, d, r, kkt_dict) — y = B^-T c_B from a fresh
        LU, refined; d = c - A^T y by variable; r = b - A x; the report of include/ellp_hip.h.  The engine's state is not
        touched.  closing_status as for read_point (an open iteration of the two-launch pipeline is completed first)."""
        fp = self.fp
        y, d, r, k = np.zeros(fp.m), np.zeros(fp.n_c), np.zeros(fp.m), Kkt()
        err = C.create_string_buffer(512)
        s = lib().ellp_engine_postsolve(self._h, _p(y), _p(d), _p(r), C.byref(k), err, 512)
        self.closing_status = s
        if s not in (OPTIMAL, UNBOUNDED, MAXITER):
            raise EllpHipError(s, err.value.decode())
        return y, d, r, k.as_dict()

    def ranging(self):
        """ellp_engine_ranging on the basis and point the engine stands on: a Ranging (include/ellp_hip.h has the definitions).
        The engine's state is not touched.  closing_status as for postsolve."""
        fp = self.fp
        rg = Ranging(fp.m, fp.n_c)
        err = C.create_string_buffer(512)
        s = lib().ellp_engine_ranging(self._h, C.byref(rg._out()), err, 512)
        self.closing_status = s
        if s not in (OPTIMAL, UNBOUNDED, MAXITER):
            raise EllpHipError(s, err.value.decode())
        return rg._done()

    def certificate(self, source, n_check=None, chk=None, vec=None):
        """ellp_engine_certificate on the basis, labels and point the engine stands on: (vec or None, info_dict), the
        arguments of certificate().  The engine's state is not touched."""
        fp = self.fp
        n_check, keep, vec, info = _cert_args(fp.m, fp.n, source, n_check, chk, vec)
        err = C.create_string_buffer(512)
        s = lib().ellp_engine_certificate(self._h, int(source), n_check, _p(keep[0]), _p(keep[1]), _p(keep[2]), _p(vec),
                                          C.byref(info), err, 512)
        if s != OPTIMAL:
            raise EllpHipError(s, err.value.decode())
        return (vec if info.found else None), info.as_dict()

    def tableau_rows(self, positions, want_rho=True):
        """ellp_engine_tableau_rows: (alpha, rho) — alpha[p] = row positions[p] of the tableau B^-1 A_N by nonbasic position,
        rho[p] = that row of the computed B^-1 (None unless want_rho) — with the bits the ranging forms them with."""
        fp = self.fp
        pos = np.ascontiguousarray(positions, dtype=np.int64).reshape(-1)
        alpha = np.zeros((pos.size, fp.nN))
        rho = np.zeros((pos.size, fp.m)) if want_rho else None
        err = C.create_string_buffer(512)
        s = lib().ellp_engine_tableau_rows(self._h, _p(pos), pos.size, _p(alpha), _p(rho), err, 512)
        self.closing_status = s
        if s not in (OPTIMAL, UNBOUNDED, MAXITER):
            raise EllpHipError(s, err.value.decode())
        return alpha, rho

    def tap(self, what, count):
        out = np.zeros(int(count), dtype=np.float64)
        n = lib().ellp_engine_tap(self._h, what, _p(out), out.size)
        if n < 0:
            raise EllpHipError(int(n), "tap failed")
        return out[:n]

    def refactor(self):
        err = C.create_string_buffer(512)
        s = lib().ellp_engine_refactor(self._h, err, 512)
        if s != OPTIMAL:
            raise EllpHipError(s, err.value.decode())

    def refresh(self):
        """One Newton-Schulz step on B^-1; returns the residual before the step."""
        return lib().ellp_engine_refresh(self._h)

    def inverse_residual(self):
        return lib().ellp_engine_inverse_residual(self._h)

    def read_trace(self, cap=1 << 16):
        """(iterations, objectives) of the ring buffer kept with opts.trace_len > 0, oldest first"""
        it = np.zeros(int(cap), dtype=np.uint64)
        ob = np.zeros(int(cap), dtype=np.float64)
        n = lib().ellp_engine_read_trace(self._h, _p(it), _p(ob), int(cap))
        if n < 0:
            raise EllpHipError(int(n), "read_trace failed")
        return it[:n], ob[:n]

    def request_maintenance(self):
        """test hook: what a kernel does after a tiny pivot (the next run()/poll() services it)"""
        s = lib().ellp_engine_request_maintenance(self._h)
        if s != OPTIMAL:
            raise EllpHipError(s, "request_maintenance failed")

    def debug_scale_inverse(self, factor):
        """test hook: B^-1 <- factor * B^-1"""
        s = lib().ellp_engine_debug_scale_inverse(self._h, float(factor))
        if s != OPTIMAL:
            raise EllpHipError(s, "debug_scale_inverse failed")

    def debug_set_inverse(self, W):
        """test hook: B^-1 <- W (m x m, row-major): the mirror of tap(TAP_BINV)"""
        W_ = _f64(W).reshape(-1)
        assert W_.size == self.fp.m * self.fp.m
        s = lib().ellp_engine_debug_set_inverse(self._h, _p(W_))
        if s != OPTIMAL:
            raise EllpHipError(s, "debug_set_inverse failed")

    def debug_set_x(self, x):
        """test hook: x <- x (n_c doubles by variable index): the mirror of the x read_point returns"""
        x_ = _f64(x).reshape(-1)
        assert x_.size == self.fp.n_c
        s = lib().ellp_engine_debug_set_x(self._h, _p(x_))
        if s != OPTIMAL:
            raise EllpHipError(s, "debug_set_x failed")

    def counters(self):
        """host-side maintenance counters (TAP_STATE tail)"""
        v = self.tap(TAP_STATE, 30)
        return dict(drift=v[12], drift_checks=int(v[13]), maint_requests=int(v[14]), refreshes=int(v[15]),
                    rebuilds=int(v[16]), resyncs=int(v[17]), last_refresh_residual=v[18], launches_per_iteration=int(v[19]),
                    rebuild_shortcuts=int(v[20]), t_setup_s=float(v[21]),
                    # certified hybrid: is it on, guarded pivots handed to the exact kernel, terminal statuses
                    # examined, of those not confirmed, loop bodies run by the exact kernel, rebuilds after a hand-over
                    hybrid=(int(v[22]) == 1), certified_by_exact_lu_iteration=(int(v[22]) == 2), hybrid_guards=int(v[23]), hybrid_certs=int(v[24]), hybrid_disagreed=int(v[25]),
                    hybrid_exact_iters=int(v[26]), hybrid_rebuilds=int(v[27]), hybrid_redos=int(v[28]),
                    # end points returned NOT certified (a redo above 1,024 rows ruled out by ELLP_REDO_MAX_SECONDS, a singular LU)
                    hybrid_uncertified=int(v[29]))

    # ---- sharded / stepped driving (see ellp_amd/dist.py)
    def segment_doubles(self, world):
        return int(lib().ellp_engine_segment_doubles(self._h, int(world)))

    def set_shard(self, rank, world, buffer_ptr=None):
        err = C.create_string_buffer(512)
        s = lib().ellp_engine_set_shard(self._h, int(rank), int(world), C.c_void_p(buffer_ptr), err, 512)
        if s != OPTIMAL:
            raise EllpHipError(s, err.value.decode())

    def exchange_info(self):
        base, seg, rank, world = C.c_void_p(), C.c_int64(), C.c_int(), C.c_int()
        lib().ellp_engine_exchange_info(self._h, C.byref(base), C.byref(seg), C.byref(rank), C.byref(world))
        return base.value, seg.value, rank.value, world.value

    def set_stream(self, stream_handle):
        lib().ellp_engine_set_stream(self._h, C.c_void_p(stream_handle))

    def step(self, phase):
        err = C.create_string_buffer(512)
        s = lib().ellp_engine_step(self._h, int(phase), err, 512)
        if s != OPTIMAL:
            raise EllpHipError(s, err.value.decode())

    def poll(self):
        st = Stats()
        err = C.create_string_buffer(512)
        s = lib().ellp_engine_poll(self._h, C.byref(st), err, 512)
        if s == ERR_DEVICE:
            raise EllpHipError(s, err.value.decode())
        return s, st, err.value.decode()

    def rephase(self, c, kind, lb, ub):
        """Primal phase-1 -> phase-2 hand-off on the device (costs and bounds replaced; basis, point
        and B^-1 stay).  The FlatProblem's c/kind/lb/ub are updated too."""
        fp = self.fp
        fp.c = _f64(c)
        fp.kind = np.ascontiguousarray(kind, dtype=np.uint8)
        fp.lb, fp.ub = _f64(lb), _f64(ub)
        assert fp.c.size == fp.n_c == fp.kind.size == fp.lb.size == fp.ub.size
        err = C.create_string_buffer(512)
        s = lib().ellp_engine_rephase(self._h, _p(fp.c), _p(fp.kind), _p(fp.lb), _p(fp.ub), err, 512)
        if s != OPTIMAL:
            raise EllpHipError(s, err.value.decode())

    def dual_rephase(self, c, b, kind, lb, ub):
        """Dual phase-1 -> phase-2 hand-off on the device (same matrix in both phases).  The FlatProblem's
        c/b/kind/lb/ub are replaced; read_point() afterwards brings x, N (in variable order), y, d back."""
        fp = self.fp
        fp.c, fp.b = _f64(c), _f64(b)
        fp.kind = np.ascontiguousarray(kind, dtype=np.uint8)
        fp.lb, fp.ub = _f64(lb), _f64(ub)
        err = C.create_string_buffer(512)
        s = lib().ellp_engine_dual_rephase(self._h, _p(fp.c), _p(fp.b), _p(fp.kind), _p(fp.lb), _p(fp.ub), err, 512)
        if s != OPTIMAL:
            raise EllpHipError(s, err.value.decode())

    # ---- sharded loop inside the library, exchange by RCCL on the engine's stream
    def comm_init(self, unique_id, rank, world, rccl_path=None):
        err = C.create_string_buffer(512)
        path = rccl_path.encode() if rccl_path else None
        s = lib().ellp_engine_comm_init(self._h, path, bytes(unique_id), int(rank), int(world), err, 512)
        if s != OPTIMAL:
            raise EllpHipError(s, err.value.decode())

    def run_sharded(self, max_iters):
        st = Stats()
        err = C.create_string_buffer(512)
        s = lib().ellp_engine_run_sharded(self._h, C.c_uint64(int(max_iters)), C.byref(st), err, 512)
        if s == ERR_DEVICE or s == ERR_ARG:
            raise EllpHipError(s, err.value.decode())
        return s, st, err.value.decode()

    # ---- column-sharded storage (include/ellp_hip.h, ellp_engine_shard_columns)
    def shard_columns(self, rank, world):
        err = C.create_string_buffer(512)
        s = lib().ellp_engine_shard_columns(self._h, int(rank), int(world), err, 512)
        if s != OPTIMAL:
            raise EllpHipError(s, err.value.decode())

    def set_exchange_callback(self, fn):
        """fn(host_buffer_address, segment_bytes, world) -> 0 on success; all-gathers in place"""
        def _cb(user, buf, seg, world):
            try:
                return int(fn(buf, seg, world))
            except Exception:  # never unwind into C
                import traceback
                traceback.print_exc()
                return 1
        self._xcb = EXCHANGE_FN(_cb)  # keep it alive as long as the engine
        lib().ellp_engine_set_exchange_callback(self._h, self._xcb, None)

    def mailbox_export(self):
        buf = C.create_string_buffer(128)
        err = C.create_string_buffer(512)
        s = lib().ellp_engine_mailbox_export(self._h, buf, err, 512)
        if s != OPTIMAL:
            raise EllpHipError(s, err.value.decode())
        return buf.raw

    def mailbox_connect(self, all_handles):
        err = C.create_string_buffer(512)
        s = lib().ellp_engine_mailbox_connect(self._h, bytes(all_handles), err, 512)
        if s != OPTIMAL:
            raise EllpHipError(s, err.value.decode())

    def mailbox_selftest(self, rounds=8):
        err = C.create_string_buffer(512)
        s = lib().ellp_engine_mailbox_selftest(self._h, int(rounds), err, 512)
        if s != OPTIMAL:
            raise EllpHipError(s, err.value.decode())

    def shard_info(self):
        out = (C.c_double * 6)()
        lib().ellp_engine_shard_info(self._h, out)
        return dict(full_exchanges=int(out[0]), column_requests=int(out[1]),
                    transport={0: "none", 1: "rccl", 2: "mailbox", 3: "callback"}[int(out[2])],
                    pack_doubles=int(out[3]), own=(int(out[4]), int(out[5])))

    def close(self):
        if self._h:
            lib().ellp_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

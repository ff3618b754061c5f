"""The blocked LU of a device-resident square matrix by rows (ellp_lu.hip: k_lup_panel_reg / k_lup_panel_mem / k_lup_update,
DESIGN.md §3.1d), through ellp_hip_lu_rows.  Bar: the factors, the pivots and U's diagonal are BYTE FOR BYTE what the host
loop of ellp_amd/csrc/host/dense.h (= oracle lu_factor_inplace) leaves, for the blocked form and for the unblocked one it
replaces — so the exact loop above 1,024 rows decides every iteration from the same numbers whichever form factored the
basis."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def host_lu_rows(M_in):
    """test_gpu_lu.py's host_lu_of_transpose on a square row-major matrix, also returning the full factor matrix: first
    maximum (strict >, a NaN is never greater), zero pivot column skipped, whole rows exchanged, multipliers a * (1 / diag),
    update (-M[i,k]) * M[r,i] + M[r,k] rounded separately and skipped for a zero -M[i,k]."""
    M = np.array(M_in, dtype=np.float64, order="C")
    m = M.shape[0]
    piv, ud = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(m):
            col = np.abs(M[i:, i])
            p, best = i, col[0]
            for r in range(1, len(col)):
                if col[r] > best:
                    best, p = col[r], i + r
            diag = M[p, i]
            if diag == 0.0:
                piv.append(i)
                ud.append(M[i, i])
                continue
            if p != i:
                M[[i, p], :] = M[[p, i], :]
            piv.append(p)
            inv = 1.0 / diag
            M[i + 1:, i] = M[i + 1:, i] * inv
            for k in range(i + 1, m):
                f = -M[i, k]
                if f == 0.0:
                    continue
                M[i + 1:, k] = f * M[i + 1:, i] + M[i + 1:, k]
            ud.append(M[i, i])
    return M, np.array(piv, dtype=np.int64), np.array(ud, dtype=np.float64)


def _cases():
    rng = np.random.default_rng(2024)
    for m in (1, 15, 16, 17, 33, 48):                                   # one panel, the panel boundary, a short last panel
        yield "uniform-%d" % m, rng.uniform(-1, 1, size=(m, m))
    yield "ties-24", rng.integers(-2, 3, size=(24, 24)).astype(float)   # exact ties, zeros in pivot rows: the FIRST maximum decides
    A = rng.uniform(-1, 1, size=(40, 40))
    A[:, 21] = 0.0                                                       # an exactly zero column met mid-panel: a skipped step
    yield "zero-column-mid-panel", A
    A = rng.uniform(-1, 1, size=(40, 40))
    A[:, 16] = 0.0                                                       # ... and one met as a panel's first column
    yield "zero-column-first-of-panel", A
    yield "permutation-40", np.eye(40)[rng.permutation(40)]             # every step exchanges, every update is skipped
    yield "sparse-130", rng.uniform(-1, 1, size=(130, 130)) * (rng.random((130, 130)) < 0.1)
    yield "uniform-130", rng.uniform(-1, 1, size=(130, 130))            # pivots chain through rows earlier panels exchanged
    yield "uniform-300", rng.uniform(-1, 1, size=(300, 300))
    A = rng.uniform(-1, 1, size=(37, 37))
    A[rng.random((37, 37)) < 0.3] = -0.0                                 # entries of -0.0 (the sign of a zero is a bit too)
    yield "minus-zero", A


CASES = list(_cases())
_HOST = {}


def _host(name, A):
    if name not in _HOST:
        _HOST[name] = host_lu_rows(A)
    return _HOST[name]


@pytest.mark.parametrize("blocked", [False, True], ids=["unblocked", "blocked"])
@pytest.mark.parametrize("name,A", CASES, ids=[c[0] for c in CASES])
def test_both_forms_are_bitwise_the_host_loop(name, A, blocked):
    from ellp_amd import _engine as E
    fac_h, piv_h, ud_h = _host(name, A)
    fac, piv, ud = E.lu_rows(A, blocked=blocked)
    np.testing.assert_array_equal(piv, piv_h)
    assert ud.tobytes() == ud_h.tobytes(), name
    assert fac.tobytes() == fac_h.tobytes(), (name, np.argwhere(fac.view(np.uint64) != fac_h.view(np.uint64))[:5])


# device against device where the Python loop is too slow: one size inside every tier of rows left in a panel
# (k_lup_panel_reg<1>: <= 1,024, <2>: <= 2,048, k_lup_panel_mem above; a factorisation walks down through the tiers below its size)
@pytest.mark.parametrize("m", [1030, 2100, 4100])
def test_blocked_equals_unblocked_on_the_device(m):
    from ellp_amd import _engine as E
    A = np.random.default_rng(m).uniform(-1, 1, size=(m, m))
    f0, p0, u0 = E.lu_rows(A, blocked=False)
    f1, p1, u1 = E.lu_rows(A, blocked=True)
    np.testing.assert_array_equal(p1, p0)
    assert u1.tobytes() == u0.tobytes()
    assert f1.tobytes() == f0.tobytes()
    assert int((p0 != np.arange(m)).sum()) > m // 2  # it did pivot


def test_a_nan_on_a_later_diagonal_candidate_gives_the_same_pivots():
    """k_lut_step's rule for a NaN (never greater; on the diagonal it stands for itself) is the panel kernels' rule"""
    from ellp_amd import _engine as E
    A = np.random.default_rng(77).uniform(-1, 1, size=(50, 50))
    A[20, 20] = np.nan
    A[35, 18] = np.nan
    _, p0, _ = E.lu_rows(A, blocked=False)
    _, p1, _ = E.lu_rows(A, blocked=True)
    np.testing.assert_array_equal(p1, p0)

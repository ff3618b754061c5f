"""The blocked rebuild of B^-1 (ellp_amd/csrc/engine/ellp_rebuild.inc): the same
Gauss-Jordan elimination with partial pivoting as the column-by-column rebuild of round 1 (whose pivots
are partial-pivot LU's U_kk, so that the reference's singularity guard primal…:175-179 applies), done 64
columns at a time.  Checked against numpy's inverse within a multiple of the condition number, against the
column-by-column rebuild, on sizes around the tile edges (the 8- and 4-column sub-panels only at m = 2100 and
4100, the 512-thread kernels only), on singular bases far below the guard, and on the permutation shortcut.
The exact checks - every k_bl_factor instantiation, the pivot rows, the guard at its edge, NaN and Inf - are
in tests/test_gpu_rebuild_model.py."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _E():
    from ellp_amd import _engine as E
    return E


def dense_basis_problem(m, seed, nstruct=None, scale_col=None):
    """[B | I] with B a dense random m x m block taken as the basis (its point need not be feasible: only
    the inverse is looked at)"""
    rng = np.random.default_rng(seed)
    B = rng.uniform(0.1, 1.1, size=(m, m)) + np.diag(rng.uniform(0.5, 1.5, size=m))
    if scale_col is not None:
        B[:, scale_col[0]] *= scale_col[1]
    n = 2 * m
    A = np.zeros((m, n), order="F")
    A[:, :m] = B
    A[:, m:] = np.eye(m)
    E = _E()
    fp = E.FlatProblem(m, n, n, A.reshape(-1, order="F"), np.zeros(n), np.ones(m), np.full(n, 1, dtype=np.uint8),
                       np.zeros(n), np.zeros(n), np.zeros(n), np.arange(m, dtype=np.int64),
                       np.arange(m, n, dtype=np.int64), np.zeros(m, dtype=np.uint8))
    return fp, B


@pytest.mark.parametrize("m", [1, 3, 63, 64, 65, 129, 300, 1000, 2000, 2100, 4100])
def test_blocked_rebuild_inverts_a_dense_basis(m):
    E = _E()
    fp, B = dense_basis_problem(m, 100 + m)
    eng = E.Engine(E.ENGINE_PRIMAL, fp, E.default_opts(max_iter=None, pipeline=1))
    c = eng.counters()
    assert c["rebuild_shortcuts"] == (1 if m == 1 else 0)  # a 1 x 1 basis is a permutation
    res = eng.inverse_residual()
    W = eng.tap(E.TAP_BINV, m * m).reshape(m, m)
    eng.close()
    cond = np.linalg.cond(B)
    assert res < 1e-13 * max(cond, 10.0) * 10, (res, cond)
    Wn = np.linalg.inv(B)
    assert np.abs(W - Wn).max() <= 1e-12 * cond * np.abs(Wn).max() + 1e-13, (np.abs(W - Wn).max(), cond)


@pytest.mark.parametrize("m", [70, 500, 2100])
def test_blocked_rebuild_equals_the_columnwise_rebuild(m, monkeypatch):
    """same pivots, same inverse up to the order of the additions"""
    E = _E()
    fp, B = dense_basis_problem(m, 7 + m)
    eng = E.Engine(E.ENGINE_PRIMAL, fp, E.default_opts(max_iter=None, pipeline=1))
    W_blocked = eng.tap(E.TAP_BINV, m * m).reshape(m, m).copy()
    monkeypatch.setenv("ELLP_REBUILD", "columnwise")
    eng.refactor()
    W_col = eng.tap(E.TAP_BINV, m * m).reshape(m, m).copy()
    monkeypatch.delenv("ELLP_REBUILD")
    eng.refactor()
    W_again = eng.tap(E.TAP_BINV, m * m).reshape(m, m)
    eng.close()
    scale = np.abs(W_col).max()
    assert np.abs(W_blocked - W_col).max() <= 1e-11 * scale * np.linalg.cond(B)
    np.testing.assert_array_equal(W_blocked, W_again)  # deterministic: no atomics in the sums


def test_blocked_rebuild_applies_the_reference_singularity_guard():
    """primal: any |U_ii| < 1e-10 is Err("invalid B, A_B is not invertible") (primal…:175-179); an exactly
    singular basis in the dual engine too"""
    E = _E()
    m = 200
    # a column that is a combination of two others: exactly singular up to rounding -> U_kk ~ 1e-16
    fp, B = dense_basis_problem(m, 5)
    A = fp.A.reshape(fp.n, m)
    A[150] = 0.5 * A[3] + 0.25 * A[77]
    with pytest.raises(E.EllpHipError) as ei:
        E.Engine(E.ENGINE_PRIMAL, fp, E.default_opts(max_iter=None, pipeline=1))
    assert ei.value.status == E.ERR_SINGULAR and "not invertible" in ei.value.msg
    # a tiny but honest pivot: a column scaled by 1e-12 makes one U_kk < EPS -> the reference rejects it too
    fp2, _ = dense_basis_problem(m, 6, scale_col=(190, 1e-12))
    with pytest.raises(E.EllpHipError) as ei:
        E.Engine(E.ENGINE_PRIMAL, fp2, E.default_opts(max_iter=None, pipeline=1))
    assert ei.value.status == E.ERR_SINGULAR


def test_permutation_shortcut():
    """signed, scaled permutation basis (what phase 1 starts from): inverted by inspection, exactly"""
    E = _E()
    m = 777
    rng = np.random.default_rng(3)
    perm = rng.permutation(m)
    vals = rng.choice([-1.0, 1.0, 2.5, -0.125], size=m)
    n = 2 * m
    A = np.zeros((m, n), order="F")
    A[perm, np.arange(m)] = vals           # basic column k has vals[k] in row perm[k]
    A[:, m:] = rng.normal(size=(m, m))
    fp = E.FlatProblem(m, n, n, A.reshape(-1, order="F"), np.zeros(n), np.ones(m), np.full(n, 1, dtype=np.uint8),
                       np.zeros(n), np.zeros(n), np.zeros(n), np.arange(m, dtype=np.int64),
                       np.arange(m, n, dtype=np.int64), np.zeros(m, dtype=np.uint8))
    eng = E.Engine(E.ENGINE_PRIMAL, fp, E.default_opts(max_iter=None, pipeline=1))
    assert eng.counters()["rebuild_shortcuts"] == 1
    W = eng.tap(E.TAP_BINV, m * m).reshape(m, m)
    eng.close()
    want = np.zeros((m, m))
    want[np.arange(m), perm] = 1.0 / vals
    np.testing.assert_array_equal(W, want)
    # a zero "pivot" below EPS is still the reference's error
    A[perm[5], 5] = 1e-11
    fp.A = A.reshape(-1, order="F").copy()
    with pytest.raises(E.EllpHipError) as ei:
        E.Engine(E.ENGINE_PRIMAL, fp, E.default_opts(max_iter=None, pipeline=1))
    assert ei.value.status == E.ERR_SINGULAR


def test_rebuild_times(monkeypatch):
    """a rebuild of a general dense basis: measured 14 ms at m = 2000 and 54 ms at m = 4000 on an MI355X
    (the column-by-column rebuild of round 1: 45 and 250 ms).  The round-1 review asked for 5 / 25 ms: not
    reached — the m sequential pivot steps cost about 6 us each inside one workgroup (profiles/r02_rebuild_*).
    Asserted: at least twice as fast as the column-by-column rebuild on the same box, and generous absolute
    bounds for a shared box."""
    import time
    E = _E()
    out = {}
    for m, bound in ((2000, 0.035), (4000, 0.130)):
        fp, _ = dense_basis_problem(m, 11)
        eng = E.Engine(E.ENGINE_PRIMAL, fp, E.default_opts(max_iter=None, pipeline=1))
        best = {}
        for mode in ("blocked", "columnwise"):
            if mode == "columnwise":
                monkeypatch.setenv("ELLP_REBUILD", "columnwise")
            else:
                monkeypatch.delenv("ELLP_REBUILD", raising=False)
            b = 1e9
            for _ in range(3 if mode == "blocked" else 1):
                t0 = time.perf_counter()
                eng.refactor()
                b = min(b, time.perf_counter() - t0)
            best[mode] = b
        monkeypatch.delenv("ELLP_REBUILD", raising=False)
        eng.close()
        out[m] = best
        assert best["blocked"] < bound, (m, best)
        assert best["blocked"] < 0.5 * best["columnwise"], (m, best)
    print("rebuild seconds", out)

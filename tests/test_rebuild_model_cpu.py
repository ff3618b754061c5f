"""tests/rebuild_model.py without a device: the exact family's model against the closed form and against rational
arithmetic; the exactness proof for every matrix tests/test_gpu_rebuild_model.py sends to the device; and the proof that
those tests could fail - a wrong tie-break, a dropped -1 and a swapped ping-pong buffer, injected into the blocked replay,
are each noticed."""
from fractions import Fraction

import numpy as np
import pytest

import rebuild_model as R


def fraction_eliminate(B):
    """the operation in rational arithmetic: (W, perm)"""
    m = B.shape[0]
    A = [[Fraction(float(v)) for v in row] for row in B]
    W = [[Fraction(int(i == j)) for j in range(m)] for i in range(m)]
    used, perm = [False] * m, []
    for k in range(m):
        alpha = [sum(W[i][t] * A[t][k] for t in range(m)) for i in range(m)]
        best, p = Fraction(-1), -1
        for i in range(m):
            if not used[i] and abs(alpha[i]) > best:
                best, p = abs(alpha[i]), i
        assert best > 0
        rowp = W[p]
        for i in range(m):
            if i != p and alpha[i] != 0:
                f = alpha[i] / alpha[p]
                W[i] = [W[i][j] - f * rowp[j] for j in range(m)]
        W[p] = [v / alpha[p] for v in rowp]
        used[p] = True
        perm.append(p)
    return np.array([[float(v) for v in W[p]] for p in perm]), np.array(perm)


@pytest.mark.parametrize("m", [2, 3, 17, 40])
def test_exact_model_equals_rational_arithmetic_and_the_closed_form(m):
    for seed in range(6):
        B, Binv = R.exact_basis(m, 100 * m + seed)
        W, perm, _ = R.eliminate(B, prove=True)
        Wf, pf = fraction_eliminate(B)
        np.testing.assert_array_equal(perm, pf)
        np.testing.assert_array_equal(W, Wf)
        np.testing.assert_array_equal(W, Binv)
        np.testing.assert_array_equal(B @ W, np.eye(m))


@pytest.mark.parametrize("m", R.EXACT_SIZES + [R.GUARD_M - 1])
def test_every_modelled_matrix_is_proved_exact_in_both_orders(m):
    """exact_case runs the proof (columnwise, and the blocked replay with 16-, 8- and 4-column sub-panels, which must equal
    the columnwise model bit for bit, which must equal the closed form) and raises NotExact otherwise"""
    c = R.exact_case(m)
    assert sorted(c.perm.tolist()) == list(range(m))
    assert np.abs(c.W).max() <= 8.0


def test_the_family_has_tied_steps_and_exchanged_rows():
    tied = {m: len(R.exact_case(m).ties) for m in R.EXACT_SIZES}
    assert all(tied[m] >= 1 for m in R.EXACT_SIZES if m >= 17), tied
    c = R.exact_case(130)
    assert (c.perm != np.arange(130)).sum() > 100  # the pivot rows are nowhere near the identity


@pytest.mark.parametrize("i", range(len(R.TIE_ROWS)))
def test_directed_ties_are_proved_and_pivot_on_the_smaller_row(i):
    rows = R.TIE_ROWS[i]
    c = R.tie_case(rows, flip=bool(i & 1))  # asserts that step TIE_POS is a tie of exactly these rows, taken at min(rows)
    col = c.B[:, R.TIE_POS]
    assert col[rows[0]] == -col[rows[1]] != 0.0  # mixed signs
    assert np.abs(col).max() == abs(col[rows[0]]) and (np.abs(col) == abs(col[rows[0]])).sum() == 2
    assert c.perm[R.TIE_POS] == min(rows)


@pytest.mark.parametrize("m", R.NATURAL_SIZES)
def test_natural_sizes_are_proved_in_the_width_they_run_at(m):
    """no columnwise model above 1,030 rows: the blocked replay in the size's own width, proved, against the closed form
    (the 1,024-thread kernels do the same arithmetic on other threads).  The slowest test here: 4,100 rows take 20 s."""
    c = R.natural_case(m)
    W, perm = R.blocked_replay(c.B, nbw_max=R.natural_width(m), prove=True)
    np.testing.assert_array_equal(W, c.Binv)
    assert sorted(perm.tolist()) == list(range(m))


def test_the_proof_rejects_a_matrix_that_is_not_exact():
    B = R.exact_case(65).B.copy()
    B[B == 1.0] = 3.0
    with pytest.raises(R.NotExact):
        R.eliminate(B, prove=True)
    with pytest.raises(R.NotExact):
        R.blocked_replay(B, prove=True)


@pytest.mark.parametrize("nbw", [16, 8, 4])
@pytest.mark.parametrize("m", [17, 65, 130, 513])
def test_injected_bugs_are_caught(m, nbw):
    """what the device tests compare - W and perm - differs from the model for each of the three"""
    c = R.exact_case(m)
    W, perm = R.blocked_replay(c.B, nbw_max=nbw, bug="tie")
    np.testing.assert_array_equal(W, c.W)  # B^-1 does not depend on the pivot order: only perm can show it
    assert not np.array_equal(perm, c.perm)
    if m > nbw:  # the second sub-panel exists
        W, perm = R.blocked_replay(c.B, nbw_max=nbw, bug="minus1")
        assert not np.array_equal(W, c.W)
    W, perm = R.blocked_replay(c.B, nbw_max=nbw, bug="pingpong")
    assert not np.array_equal(W, c.W)


def test_tap_number_is_the_header_s():
    import os
    import re
    from ellp_amd import _engine as E
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "include", "ellp_hip.h")) as f:
        taps = dict(re.findall(r"ELLP_TAP_([A-Z_]+) = (\d+)", f.read()))
    assert taps["REBUILD_PERM"] == "10" and E.TAP_REBUILD_PERM == 10
    assert sorted(int(v) for v in taps.values()) == list(range(11))  # no number twice, none left out
    for name, v in taps.items():
        assert getattr(E, "TAP_" + name) == int(v), name


def test_guard_model():
    B, want = R.guard_basis(1e-10, 63)
    W, perm, _ = R.eliminate(B, eps=1e-10)
    np.testing.assert_array_equal(W, want)
    assert perm[63] == R.GUARD_M - 1
    with pytest.raises(R.Singular) as ei:
        R.eliminate(R.guard_basis(np.nextafter(1e-10, 0.0), 63)[0], eps=1e-10)
    assert ei.value.k == 63
    with pytest.raises(R.Singular):
        R.blocked_replay(R.guard_basis(0.0, 64)[0], eps=0.0)
    W, _ = R.blocked_replay(R.guard_basis(1e-300, 129)[0], eps=0.0, nbw_max=4)
    np.testing.assert_array_equal(W, R.guard_basis(1e-300, 129)[1])


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("col", [0, 64, 129])
def test_model_refuses_nan_and_inf(bad, col):
    rng = np.random.default_rng(1)
    B = rng.uniform(0.1, 1.1, size=(130, 130)) + np.eye(130)
    B[(3 * col + 7) % 130, col] = bad
    with np.errstate(invalid="ignore"):
        with pytest.raises(R.Singular):
            R.eliminate(B)
        with pytest.raises(R.Singular):
            R.blocked_replay(B)


# ------------------------------------------------------------------ wide mode
WIDE_ORDERS = [dict(parts=1), dict(parts=1, reverse=True), dict(parts=2), dict(parts=3), dict(parts=16)]


@pytest.mark.parametrize("m,scaled", R.WIDE_CASES, ids=[f"m{m}{'-scaled' if s else ''}" for m, s in R.WIDE_CASES])
def test_wide_bound_covers_f64_runs_in_several_orders(m, scaled):
    """forward, reversed, split in 2, 3 and 16 parts, and the blocked replay with 16- and 4-column sub-panels; the reference
    alone meets the cap on ambiguous steps and the 1e-6 max|W| limit on the bound"""
    B = R.wide_basis(m, scaled)
    W, perm, _ = R.eliminate(B)
    w = R.wide_model(B, perm)
    assert w.ok.all()
    assert w.ambiguous.sum() <= m // 100
    assert float(w.bound.max()) <= 1e-6 * float(np.abs(w.W).max())
    assert (perm != np.arange(m)).sum() > m // 2  # rows really get exchanged
    runs = [W] + [R.blocked_replay(B, nbw_max=nbw)[0] for nbw in (16, 4)]
    if m <= 130:  # the explicit orders are Python loops over the terms
        runs += [R.f64_eliminate(B, perm, **o) for o in WIDE_ORDERS]
    worst = 0.0
    for X in runs:
        ratio = float((np.abs(X - w.W) / w.bound).max())
        assert ratio <= 1.0
        worst = max(worst, ratio)
    assert worst > 1e-9  # the runs do differ from the model: the comparison is not vacuous


def test_wide_model_notices_a_wrong_pivot_row_and_a_wrong_entry():
    B = R.wide_basis(65)
    W, perm, _ = R.eliminate(B)
    w = R.wide_model(B, perm)
    X = W.copy()
    i, j = np.unravel_index(np.argmax(np.abs(W)), W.shape)
    X[i, j] *= 1.0 + 1e-6  # one entry off in its seventh digit
    assert float((np.abs(X - w.W) / w.bound).max()) > 1.0
    bad = perm.copy()
    k = 10
    j = int(np.flatnonzero(perm == np.setdiff1d(np.arange(65), perm[:k + 1])[0])[0])
    bad[k], bad[j] = bad[j], bad[k]  # a row that is not the maximum of step k
    assert not R.wide_model(B, bad).ok[k]

"""The rebuild of B^-1 (ellp_amd/csrc/engine/ellp_rebuild.inc, dispatched by launch_refactor; the column-by-column form
of ellp_engine.hip) against the model of tests/rebuild_model.py: bit for bit on the exact family, in every one of the six
k_bl_factor instantiations (ELLP_BL_NT x ELLP_BL_NBW) and column by column; the pivot rows (ELLP_TAP_REBUILD_PERM)
against the model's first-maximum rule, with directed ties across the three levels of the search; the singularity guard
at its edge; NaN and Inf in a basis; and general dense matrices entry by entry within the rounding bound of the model's
wide mode.  tests/test_rebuild_model_cpu.py proves, without a device, that the matrices used
here are exact in any order of the additions and that the model's blocked replay notices a wrong tie-break, a dropped
-1 and a swapped ping-pong buffer."""
import numpy as np
import pytest

import rebuild_model as R

pytestmark = pytest.mark.gpu

# (ELLP_BL_NT, ELLP_BL_NBW): None = unset, i.e. 512 threads and the width the size asks for (16 up to 2,048 rows)
VARIANTS = [(nt, nbw) for nt in (None, 1024) for nbw in (None, 8, 4)]


def vid(v):
    return "columnwise" if v == "columnwise" else f"NT{v[0] or 512}-NBW{v[1] or 'natural'}"


def _E():
    from ellp_amd import _engine as E
    return E


def set_variant(monkeypatch, v):
    for k in ("ELLP_BL_NT", "ELLP_BL_NBW", "ELLP_REBUILD"):
        monkeypatch.delenv(k, raising=False)
    if v == "columnwise":
        monkeypatch.setenv("ELLP_REBUILD", "columnwise")
        return
    if v[0]:
        monkeypatch.setenv("ELLP_BL_NT", str(v[0]))
    if v[1]:
        monkeypatch.setenv("ELLP_BL_NBW", str(v[1]))


def problem_of(B, dual=False):
    """[B | I] with B taken as the basis, as tests/test_gpu_rebuild.py builds it (only the inverse is looked at)"""
    E = _E()
    m = B.shape[0]
    n = 2 * m
    A = np.zeros((m, n), order="F")
    A[:, :m] = B
    A[:, m:] = np.eye(m)
    return E.FlatProblem(m, n, n, A.reshape(-1, order="F"), np.zeros(n), np.ones(m), np.full(n, 1, dtype=np.uint8),
                         np.zeros(n), np.zeros(n), np.zeros(n), np.arange(m, dtype=np.int64),
                         np.arange(m, n, dtype=np.int64), np.zeros(m, dtype=np.uint8),
                         y=np.zeros(m) if dual else None, d=np.zeros(n) if dual else None)


def engine_of(B, dual=False):
    E = _E()
    return E.Engine(E.ENGINE_DUAL if dual else E.ENGINE_PRIMAL, problem_of(B, dual), E.default_opts(max_iter=None, pipeline=1))


def rebuilt(B, monkeypatch, v, dual=False):
    """(W, perm) of a rebuild in variant v: the engine is created in the default form, then rebuilt in the variant (the
    variant is read per rebuild)"""
    E = _E()
    m = B.shape[0]
    set_variant(monkeypatch, (None, None))
    eng = engine_of(B, dual)
    try:
        set_variant(monkeypatch, v)
        eng.refactor()
        W = eng.tap(E.TAP_BINV, m * m).reshape(m, m).copy()
        perm = eng.tap(E.TAP_REBUILD_PERM, m).astype(np.int64)
    finally:
        eng.close()
    return W, perm


def test_tap_number_and_refusals():
    E = _E()
    assert E.TAP_REBUILD_PERM == 10
    m = 5
    eng = engine_of(np.diag([2.0, -1.0, 4.0, 0.5, 1.0])[:, ::-1].copy())  # a generalised permutation: the shortcut
    try:
        assert eng.counters()["rebuild_shortcuts"] == 1
        with pytest.raises(E.EllpHipError) as ei:
            eng.tap(E.TAP_REBUILD_PERM, m)
        assert ei.value.status == E.ERR_ARG
    finally:
        eng.close()
    eng = engine_of(R.exact_case(17).B)
    try:
        with pytest.raises(E.EllpHipError) as ei:
            eng.tap(E.TAP_REBUILD_PERM, 16)  # m doubles or nothing
        assert ei.value.status == E.ERR_ARG
        np.testing.assert_array_equal(eng.tap(E.TAP_REBUILD_PERM, 17), R.exact_case(17).perm)
    finally:
        eng.close()


EXACT_CASES = [(m, v) for m in R.EXACT_SIZES for v in VARIANTS] + [(65, "columnwise"), (513, "columnwise")]


@pytest.mark.parametrize("m,v", EXACT_CASES, ids=[f"m{m}-{vid(v)}" for m, v in EXACT_CASES])
def test_exact_family_bit_for_bit(m, v, monkeypatch):
    """tail panels of 1, 2 and odd widths, a macro panel of 1 column (m = 65, 513), register slots 0..2 (m = 1030)"""
    c = R.exact_case(m)
    W, perm = rebuilt(c.B, monkeypatch, v)
    np.testing.assert_array_equal(perm, c.perm)
    np.testing.assert_array_equal(W, c.W)


NATURAL_CASES = [(m, nt) for m in R.NATURAL_SIZES for nt in (None, 1024)]


@pytest.mark.parametrize("m,nt", NATURAL_CASES, ids=[f"m{m}-NT{nt or 512}-NBW{R.natural_width(m)}" for m, nt in NATURAL_CASES])
def test_natural_widths_bit_for_bit(m, nt, monkeypatch):
    """the widths the sizes ask for by themselves: 16 columns at 2,048 rows (all four register slots of <16,4,512> full), 8 at
    2,050, 4 at 4,100; against the closed form (the O(m^3) model stays below)"""
    c = R.natural_case(m)
    W, perm = rebuilt(c.B, monkeypatch, (nt, None))
    np.testing.assert_array_equal(np.sort(perm), np.arange(m))
    np.testing.assert_array_equal(W, c.Binv)


TIE_CASES = [(i, v) for i in range(len(R.TIE_ROWS)) for v in VARIANTS + ["columnwise"]]


@pytest.mark.parametrize("i,v", TIE_CASES, ids=[f"rows{R.TIE_ROWS[i][0]}_{R.TIE_ROWS[i][1]}-{vid(v)}" for i, v in TIE_CASES])
def test_directed_ties_take_the_first_maximum(i, v, monkeypatch):
    """+d and -d in two rows that two lanes at a wave edge, two waves, or two register slots of one thread hold"""
    rows = R.TIE_ROWS[i]
    c = R.tie_case(rows, flip=bool(i & 1))
    W, perm = rebuilt(c.B, monkeypatch, v)
    assert perm[R.TIE_POS] == min(rows), (perm[R.TIE_POS], rows)
    np.testing.assert_array_equal(perm, c.perm)
    np.testing.assert_array_equal(W, c.W)


# ------------------------------------------------------------------ the guard at its edge
FORMS = [(None, None), (None, 4), "columnwise"]


def created(B, monkeypatch, v, dual=False):
    """(W, perm) of the rebuild at creation, in form v; EllpHipError if the basis is refused"""
    E = _E()
    m = B.shape[0]
    set_variant(monkeypatch, v)
    eng = engine_of(B, dual)
    try:
        return eng.tap(E.TAP_BINV, m * m).reshape(m, m).copy(), eng.tap(E.TAP_REBUILD_PERM, m).astype(np.int64)
    finally:
        eng.close()


@pytest.mark.parametrize("v", FORMS, ids=vid)
@pytest.mark.parametrize("pos", R.GUARD_POS)
def test_primal_guard_at_eps(pos, v, monkeypatch):
    """|pivot| < eps is refused, |pivot| == eps is not; eps is the engine's own.  WHICH column was refused cannot be read: a
    refused basis leaves no engine to ask (the blocked kernel notes the column in its device state, the columnwise one does
    not).  By construction every other pivot of these bases is a power of two of at least 2, and the same bases with t = +-eps
    are accepted above; the model's Singular.k names the column (tests/test_rebuild_model_cpu.py::test_guard_model)."""
    E = _E()
    eps = float(E.default_opts().eps)
    assert 0.0 < eps < 1e-6
    m = R.GUARD_M
    for t in (eps, -eps):
        B, want = R.guard_basis(t, pos)
        W, perm = created(B, monkeypatch, v)
        assert perm[pos] == m - 1
        assert W[pos, m - 1] == 1.0 / t
        np.testing.assert_array_equal(W, want)
    for t in (np.nextafter(eps, 0.0), -np.nextafter(eps, 0.0)):
        B, _ = R.guard_basis(t, pos)
        with pytest.raises(E.EllpHipError) as ei:
            created(B, monkeypatch, v)
        assert ei.value.status == E.ERR_SINGULAR and "not invertible" in ei.value.msg


@pytest.mark.parametrize("v", FORMS, ids=vid)
@pytest.mark.parametrize("pos", R.GUARD_POS)
def test_dual_guard_is_zero_only(pos, v, monkeypatch):
    """the dual engine rebuilds with eps = 0: a pivot of 1e-300 passes, a zero column does not"""
    E = _E()
    m = R.GUARD_M
    B, want = R.guard_basis(1e-300, pos)
    W, perm = created(B, monkeypatch, v, dual=True)
    assert perm[pos] == m - 1
    np.testing.assert_array_equal(W, want)
    B, _ = R.guard_basis(0.0, pos)
    with pytest.raises(E.EllpHipError) as ei:
        created(B, monkeypatch, v, dual=True)
    assert ei.value.status == E.ERR_SINGULAR and "not invertible" in ei.value.msg


# ------------------------------------------------------------------ NaN and Inf
@pytest.mark.parametrize("v", [(None, None), "columnwise"], ids=vid)
@pytest.mark.parametrize("dual", [False, True], ids=["primal", "dual"])
@pytest.mark.parametrize("col", [0, 64, 129])
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_nan_or_inf_in_a_basis_is_singular(bad, col, dual, v, monkeypatch):
    """The ABI does not look at the values of A before the device does; the rebuild has to refuse them.  No W comes back."""
    from test_gpu_rebuild import dense_basis_problem
    E = _E()
    m = 130
    _, B = dense_basis_problem(m, 31)
    B[(3 * col + 7) % m, col] = bad
    try:
        W, _ = created(B, monkeypatch, v, dual)
    except E.EllpHipError as e:
        assert e.status == E.ERR_SINGULAR and "not invertible" in e.msg
    else:
        pytest.fail(f"the rebuild accepted the basis; its W is {'finite' if np.isfinite(W).all() else 'not finite'}")


@pytest.mark.parametrize("v", [(None, None), "columnwise"], ids=vid)
@pytest.mark.parametrize("dual", [False, True], ids=["primal", "dual"])
@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
def test_nan_or_inf_in_a_permutation_basis_is_singular(bad, dual, v, monkeypatch):
    """the shortcut's own check (and, column by column, the elimination's): 1 / Inf would be a finite, singular W"""
    E = _E()
    m = 130
    rng = np.random.default_rng(8)
    B = np.zeros((m, m))
    B[rng.permutation(m), np.arange(m)] = rng.choice([-1.0, 1.0, 2.5], size=m)
    B[np.flatnonzero(B[:, 77])[0], 77] = bad
    with pytest.raises(E.EllpHipError) as ei:
        created(B, monkeypatch, v, dual)
    assert ei.value.status == E.ERR_SINGULAR and "not invertible" in ei.value.msg


# ------------------------------------------------------------------ wide mode
WIDE_FORMS = [(None, None), (1024, 4), "columnwise"]


@pytest.mark.parametrize("m,scaled", R.WIDE_CASES, ids=[f"m{m}{'-scaled' if sc else ''}" for m, sc in R.WIDE_CASES])
def test_general_dense_matrices_within_the_derived_bound(m, scaled, monkeypatch):
    """N(0, 1) entries (and one matrix with rows times 10^+-3): mixed signs, rows exchanged, growth.  Each form's W against
    the long-double model run with that form's own pivot rows, entry by entry within the model's rounding bound (derived in
    tests/rebuild_model.py, not measured); each pivot row a maximiser within the margins; the three forms agree on the pivot
    rows up to the first step the model calls ambiguous.
    Largest |W_dev - W_model| / bound on an MI355X (default form, NT1024-NBW4, columnwise), no ambiguous step anywhere:
        m = 17: 8.7e-4, 9.7e-4, 8.1e-4      m = 65: 3.2e-5, 1.9e-5, 1.8e-5      m = 130: 4.8e-6, 4.3e-6, 1.5e-6
        m = 300: 5.1e-7, 3.4e-7, 1.3e-7     m = 65 with scaled rows: 1.5e-4, 1.2e-4, 2.3e-7
    with the bound at 1.5e-12, 1.1e-9, 9.8e-9, 6.4e-7 and 9.5e-8 of max|W|: a worst-case bound, far above what
    happens, and still six to twelve digits below the entries."""
    B = R.wide_basis(m, scaled)
    perms, models = [], {}
    for v in WIDE_FORMS:
        W, perm = rebuilt(B, monkeypatch, v)
        key = perm.tobytes()
        if key not in models:
            models[key] = R.wide_model(B, perm)
        w = models[key]
        ratio = float((np.abs(W - w.W) / w.bound).max())
        print(f"wide m={m} scaled={scaled} {vid(v)}: max error/bound {ratio:.3e}, bound/max|W| "
              f"{float(w.bound.max()) / float(np.abs(w.W).max()):.3e}, ambiguous {int(w.ambiguous.sum())}")
        assert float(w.bound.max()) <= 1e-6 * float(np.abs(w.W).max())
        bad = np.flatnonzero(~w.ok)
        assert bad.size == 0, f"{vid(v)}: the pivot row of step {bad[:5]} is no maximiser within the margins"
        assert int(w.ambiguous.sum()) <= m // 100
        assert ratio <= 1.0, (vid(v), ratio)
        perms.append((perm, w))
    p0, w0 = perms[0]
    for (p, w), v in zip(perms[1:], WIDE_FORMS[1:]):
        diff = np.flatnonzero(p != p0)
        if diff.size:  # the first step that differs has to be one the margins cannot decide
            k = int(diff[0])
            assert w0.ambiguous[k] and w.ambiguous[k], (vid(v), k)

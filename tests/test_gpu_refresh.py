"""The Newton-Schulz refresh of B^-1 (ellp_amd/csrc/engine/ellp_gemm.inc: k_gemm_mfma<0> and <1>, k_resid_reduce,
k_copy_to_other, k_refresh_finish) entry by entry against the extended-precision model of tests/refresh_model.py.
A chosen W is put on the device with Engine.debug_set_inverse, one step is taken, and every entry of the result
must lie within the rounding bound of an f64 evaluation in any order: no factor on it.  The residual W E is six
orders of magnitude above that bound, so a wrong operand, layout, k range or edge fill shows
(tests/test_refresh_model_cpu.py shows that the bound stops them).  Then: the step from the other buffer (cur == 1),
the 1e-4 threshold from both sides, NaN and Inf in W (seen, refused, nothing changed) and a loop that meets a NaN
(it rebuilds and finishes)."""
import numpy as np
import pytest

import refresh_model as rm
from test_gpu_rebuild import dense_basis_problem

pytestmark = pytest.mark.gpu


def _E():
    from ellp_amd import _engine as E
    return E


def _opts():
    return _E().default_opts(max_iter=None, pipeline=1, refactor_period=1 << 30)


def _engine(m):
    E = _E()
    fp, _ = dense_basis_problem(m, rm.seed_of(m))
    return E.Engine(E.ENGINE_PRIMAL, fp, _opts())


def _tap(eng, m):
    return eng.tap(_E().TAP_BINV, m * m).reshape(m, m).copy()


def _cur(eng):
    return int(eng.tap(_E().TAP_STATE, 12)[1])


def _same_bits(X, Y):
    return np.array_equal(np.ascontiguousarray(X).view(np.uint64), np.ascontiguousarray(Y).view(np.uint64))


def _check_step(eng, m, model, label):
    """one refresh of the inverse that is resident, against its model; returns the tapped result"""
    r = eng.refresh()
    W_dev = _tap(eng, m)
    excess = np.abs(W_dev.astype(np.longdouble) - model.Wn) / model.dW
    print(f"{label}: m={m}: max |W_dev - W'| / dW = {float(excess.max()):.3f}; residual {r!r}, model {model.resid!r} "
          f"(|difference| {abs(r - model.resid):.3e}, bound {model.dresid:.3e})")
    assert np.isfinite(W_dev).all()
    worst = np.unravel_index(np.argmax(excess), excess.shape)
    assert (excess <= 1).all(), (label, m, worst, float(excess.max()))
    assert abs(r - model.resid) <= model.dresid, (label, m, r, model.resid, model.dresid)
    assert eng.counters()["last_refresh_residual"] == r
    return W_dev


@pytest.mark.parametrize("m", rm.SIZES)
def test_both_gemms_against_the_model(m):
    B, W, model = rm.case(m)
    eng = _engine(m)
    try:
        eng.debug_set_inverse(W)
        assert _same_bits(_tap(eng, m), W)
        assert model.resid < 1e-4  # the step is taken
        _check_step(eng, m, model, "step from the set inverse")
    finally:
        eng.close()


@pytest.mark.parametrize("m", [2, 17, 129, 300])
def test_second_refresh_reads_the_other_buffer(m):
    """after one step the inverse lives in the other buffer (cur flipped): the next step, the hook and the tap must follow"""
    B, W, model = rm.case(m)
    eng = _engine(m)
    try:
        eng.debug_set_inverse(W)
        cur0 = _cur(eng)
        W1 = _check_step(eng, m, model, "first step")
        assert _cur(eng) == 1 - cur0
        _check_step(eng, m, rm.refresh_model(B, W1), "second step")
        assert _cur(eng) == cur0
        # both values of cur have now been the source of a step.  The hook and the tap where cur is not what it was at the first set:
        eng.refresh()
        assert _cur(eng) == 1 - cur0
        eng.debug_set_inverse(W)
        assert _same_bits(_tap(eng, m), W)
        assert _cur(eng) == 1 - cur0
        _check_step(eng, m, model, "step from the set inverse in the other buffer")
    finally:
        eng.close()


@pytest.mark.parametrize("delta,taken", [(0.9e-4, True), (1.1e-4, False)])
def test_threshold_of_the_step(delta, taken):
    """max|E| >= 1e-4: nothing is changed; below: the step is taken"""
    m = 129
    B, _, _ = rm.case(m)
    W = np.ascontiguousarray((1.0 - delta) * np.linalg.inv(B))
    model = rm.refresh_model(B, W)
    assert (model.resid < 1e-4) == taken and abs(model.resid - 1e-4) > 100 * model.dresid
    eng = _engine(m)
    try:
        eng.debug_set_inverse(W)
        if taken:
            _check_step(eng, m, model, f"delta={delta}")
        else:
            r = eng.refresh()
            print(f"delta={delta}: residual {r!r}, model {model.resid!r}, bound {model.dresid:.3e}")
            assert r >= 1e-4 and abs(r - model.resid) <= model.dresid, (r, model.resid, model.dresid)
            assert eng.counters()["last_refresh_residual"] == r
            assert _same_bits(_tap(eng, m), W)
    finally:
        eng.close()


BAD = [(129, (0, 0), np.nan), (129, (128, 128), np.nan), (129, (128, 0), np.inf),
       (300, (0, 0), np.nan), (300, (299, 299), np.nan), (300, (130, 5), np.nan), (300, (299, 0), np.inf)]


@pytest.mark.parametrize("m,pos,val", BAD, ids=[f"{m}-{p[0]}-{p[1]}-{v}" for m, p, v in BAD])
def test_nan_and_inf_in_the_inverse_are_seen(m, pos, val):
    """one NaN (one +Inf) anywhere in W: the residual is not finite, the step is refused, W stays as it is, and the
    drift monitor's residual max|W A_B - I| is not a finite number either"""
    _, W0, _ = rm.case(m)
    W = W0.copy()
    W[pos] = val
    eng = _engine(m)
    try:
        eng.debug_set_inverse(W)
        r = eng.refresh()
        after = _tap(eng, m)
        res = eng.inverse_residual()
    finally:
        eng.close()
    print(f"m={m} {val} at {pos}: refresh {r!r}, inverse_residual {res!r}")
    assert not np.isfinite(r), r
    assert _same_bits(after, W)
    if np.isnan(val):
        assert np.isnan(res), res
    else:
        assert np.isnan(res) or np.isposinf(res), res


def test_loop_recovers_from_a_nan_in_the_inverse():
    """a NaN in B^-1 mid-solve: the maintenance that follows sees a residual that is not small, refuses the step, the
    host rebuilds from A_B and the solve ends where it should"""
    E = _E()
    from ellp_amd import synth
    f = synth.primal_phase1_flat(20260301, 200, 500)
    fp = E.FlatProblem(f["m"], f["n"], f["n_c"], f["A"], f["c"], f["b"], f["kind"], f["lb"], f["ub"],
                       f["x"], f["B"], f["N"], f["Nb"])
    m = f["m"]
    eng = E.Engine(E.ENGINE_PRIMAL, fp, _opts())
    try:
        st, stats, _ = eng.run(50)
        assert st == E.MAXITER and stats.iters == 50
        W = _tap(eng, m)
        W[m // 2, m // 3] = np.nan
        eng.debug_set_inverse(W)
        c0 = eng.counters()
        eng.request_maintenance()
        st, stats, msg = eng.run(1 << 40)
        c1 = eng.counters()
        eng.read_point()
    finally:
        eng.close()
    assert st == E.OPTIMAL, msg
    assert c1["rebuilds"] >= c0["rebuilds"] + 1, (c0, c1)
    assert abs(fp.obj()) < 1e-8

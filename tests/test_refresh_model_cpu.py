"""The checker of tests/test_gpu_refresh.py, checked without a GPU: the extended-precision model of one
Newton-Schulz refresh and its componentwise rounding bounds (tests/refresh_model.py) must let a correct f64
evaluation through and must stop the mistakes a GEMM kernel makes: the operands of the second product swapped,
the first operand read in the other layout, one term of one dot product lost, the last k lost at a ragged edge."""
import numpy as np
import pytest

import refresh_model as rm


def _ratios(model, E64, W64):
    """how far an f64 result is from the model, in units of the bound (<= 1: inside)"""
    L = np.longdouble
    rE = float((np.abs(E64.astype(L) - model.E) / model.dE).max())
    rW = float((np.abs(W64.astype(L) - model.Wn) / model.dW).max())
    return rE, rW


@pytest.mark.parametrize("m", rm.SIZES)
def test_plain_f64_is_inside_and_mutations_are_far_outside(m):
    B, W, model = rm.case(m)
    assert (model.dE > 0).all() and (model.dW > 0).all()
    I = np.eye(m)
    E64 = I - B @ W
    W64 = W + W @ E64
    rE, rW = _ratios(model, E64, W64)
    print(f"m={m}: plain f64 at {rE:.3f} of dE, {rW:.3f} of dW")
    assert rE <= 1.0 and rW <= 1.0, (rE, rW)
    assert abs(float(np.abs(E64).max()) - model.resid) <= model.dresid

    # every mutation is judged on W', what the device test sees of the step
    found = {}
    if m >= 2:
        found["E W for W E"] = _ratios(model, E64, W + E64 @ W)[1]
        Et = I - B.T @ W
        found["A_B transposed"] = _ratios(model, Et, W + W @ Et)[1]
    i, j, k = m // 2, m // 3, (2 * m) // 3
    Ek = E64.copy()
    Ek[i, j] += B[i, k] * W[k, j]  # E_ij = delta_ij - sum_k: that k is not subtracted
    found["one k-term missing from one entry of E"] = _ratios(model, Ek, W + W @ Ek)[1]
    WE = W @ E64
    WE[:, m - 1] -= W[:, m - 1] * E64[m - 1, m - 1]
    found["last k-term missing from the last column of W E"] = _ratios(model, E64, W + WE)[1]
    for name, r in found.items():
        print(f"m={m}: {name}: {r:.3g} x dW")
        assert r >= 100.0, (name, r)


@pytest.mark.parametrize("m", [1, 2, 17, 129])
def test_double_double_model_agrees_with_the_long_double_model(m):
    """the fall-back arithmetic of refresh_model (used where np.longdouble is not wider than 2^-60): the same E and W'
    to a small fraction of the bounds"""
    if not rm.LONGDOUBLE_IS_WIDE:
        pytest.skip("np.longdouble is no wider than f64 here: there is nothing to compare the double-double model with")
    B, W, model = rm.case(m)
    dd = rm.refresh_model(B, W, arith=rm._DD)
    assert (np.abs(dd.E - model.E) <= model.dE / 256).all()
    assert (np.abs(dd.Wn - model.Wn) <= model.dW / 256).all()

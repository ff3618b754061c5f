"""The engine ellp_engine_create makes is the one ellp_engine_plan predicts: launches per iteration (ELLP_TAP_STATE entry 19:
0 inside one persistent launch, 2, 3) and the certificate (entry 22: 1 the hybrid, 2 the exact-LU iteration above 1,024 rows).
Creation only, on unit bases; what each mode should be is tests/test_plan_cpu.py's subject."""
import pytest

from ellp_amd import _engine as E
from helpers import unit_basis_problem

pytestmark = pytest.mark.gpu
P, D = E.ENGINE_PRIMAL, E.ENGINE_DUAL

INPUTS = [(kind, m, nN, opts) for kind in (P, D) for m, nN, opts in
          ((3, 5, {}), (129, 200, {}), (384, 500, dict(flags=E.FLAG_NO_CERTIFY)), (1025, 2, {}), (129, 200, dict(pipeline=3)))]
INPUTS.append((P, 17, 30, dict(flags=E.FLAG_PRIMAL_STEEPEST_EDGE)))


@pytest.mark.parametrize("kind,m,nN,opts", INPUTS, ids=lambda v: str(v).replace(" ", ""))
def test_created_engine_is_the_planned_one(kind, m, nN, opts):
    s, p, msg = E.engine_plan(kind, m, nN, E.default_opts(**opts))
    assert s == E.OPTIMAL, msg
    eng = E.Engine(kind, unit_basis_problem(kind, m, nN), E.default_opts(**opts))
    try:
        st = eng.tap(E.TAP_STATE, 30)
    finally:
        eng.close()
    assert st[19] == (0.0 if p["small"] else 2.0 if (p["lagged"] or p["dual_fused"]) else 3.0)
    assert st[22] == (1.0 if p["hybrid"] else 2.0 if p["cert_large"] else 0.0)


def test_refused_combination_has_the_plans_status_and_text():
    opts = dict(flags=E.FLAG_DUAL_BOUND_FLIPPING, pipeline=2)
    s, p, msg = E.engine_plan(D, 5, 7, E.default_opts(**opts))
    assert s == E.ERR_ARG and p is None and "ELLP_FLAG_DUAL_BOUND_FLIPPING" in msg
    with pytest.raises(E.EllpHipError) as ei:
        E.Engine(D, unit_basis_problem(D, 5, 7), E.default_opts(**opts))
    assert ei.value.status == E.ERR_ARG and ei.value.msg == msg

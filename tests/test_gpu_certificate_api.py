"""solve(prob, certificate=True): the certificate an Infeasible or Unbounded result carries, checked at Problem level in exact
rational arithmetic (tests/cert_model.py: straight from the fixture's vars and constraints, no standard form in between).

Every case asserts: kind and iters equal those of solve(prob) without the option; the certificate is found and is a proof —
Farkas: gap > 0 and dir_violation <= eps max(1, max |y|); ray: c . r < 0, bound_dir_violation <= eps max |r|, and no row moves the
wrong way by more than eps S, S = max(1, max |r|) (1 + max_i sum_j |a_ij|): in the standard form a row's movement is taken up
by its slack, whose entry of the ray is at most S in size and may point the wrong way by eps times that (the seam's
threshold), the row residual of the standard form being of the order of u S; solve(prob) and solve(prob, postsolve=True) make
no certificate call.  eps = 1e-10, the loops' EPS.

The golden fixtures that reach the device (the endings the set-up decides are in tests/test_cert_abi_cpu.py); AFIRO made
infeasible by a row that contradicts its row 2 (x0 <= 80 and x0 >= 81) and unbounded by freeing variable 31; the same two as
five block-diagonal copies (140 and 135 rows: the resident engines above 128 rows, not the one-workgroup kernel); a warm-started
dual re-solve after a changed right-hand side (x0 <= -5) that ends Infeasible.  The CPU oracle confirms each status."""
import copy
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cert_model as CM  # noqa: E402
from helpers import GOLDEN, blockdiag, known_answers, read_mps  # noqa: E402

from ellp_amd import DualSimplexSolver, PrimalSimplexSolver, Problem  # noqa: E402
from ellp_amd import _engine as E  # noqa: E402

pytestmark = pytest.mark.gpu
SOLVERS = {"primal": PrimalSimplexSolver, "dual": DualSimplexSolver}
EPS = Fraction(1e-10)
FX = {p["name"]: p for p in known_answers()["problems"]}


def _afiro():
    return read_mps(os.path.join(GOLDEN, "netlib", "afiro.mps"))


def _afiro_infeasible():
    fx = _afiro()
    coeffs, op, rhs = fx["constraints"][2]
    assert op == "Lte"
    fx["constraints"].append([copy.deepcopy(coeffs), "Gte", rhs + 1.0])
    return fx


def _afiro_unbounded():
    fx = _afiro()
    fx["vars"][31][1] = ["Free", 0.0, 0.0]
    return fx


CASES = {
    "one_variable_infeasible": (lambda: FX["one_variable_infeasible"], "infeasible"),
    "two_variables_infeasible_with_bounds": (lambda: FX["two_variables_infeasible_with_bounds"], "infeasible"),
    "small_prob_unbounded_1": (lambda: FX["small_prob_unbounded_1"], "unbounded"),
    "small_prob_unbounded_2": (lambda: FX["small_prob_unbounded_2"], "unbounded"),
    "afiro_infeasible": (_afiro_infeasible, "infeasible"),
    "afiro_unbounded": (_afiro_unbounded, "unbounded"),
    "afiro_infeasible_x5": (lambda: blockdiag(_afiro_infeasible(), 5), "infeasible"),
    "afiro_unbounded_x5": (lambda: blockdiag(_afiro_unbounded(), 5), "unbounded"),
}


def _oracle_status(fx, solver):
    from oracle import ellp_oracle as eo
    return {1: "infeasible", 2: "unbounded", 0: "optimal"}.get(eo.solve(eo.Problem.from_fixture(fx), solver, 100000).status)


def _check_certificate(fx, res, name):
    cert = res.certificate
    assert cert is not None, (name, res.kind, res.certificate_reason)
    assert cert["found"] == 1 and cert["reason"] == res.certificate_reason
    if res.kind == "infeasible":
        assert cert["kind"] == "farkas" and len(cert["y"]) == len(fx["constraints"])
        k = CM.problem_farkas_check(fx, cert["y"])
        print(f"{name}: {cert['reason']}; gap {float(k['gap']):.6g} (reported on the standard form {cert['gap']:.6g}), dir_violation "
              f"{float(k['dir_violation']):.3e}, max |y| {float(k['norm']):.3g}, source {cert['source']}, qualifying {cert['qualifying']}")
        assert k["gap"] > 0, name
        assert k["dir_violation"] <= EPS * max(1, k["norm"]), name
    else:
        assert cert["kind"] == "ray" and len(cert["ray"]) == len(fx["vars"])
        k = CM.problem_ray_check(fx, cert["ray"])
        rowsum = max([sum(abs(Fraction(a)) for _, a in coeffs) for coeffs, _, _ in fx["constraints"]] + [Fraction(0)])
        S = max(1, k["norm"]) * (1 + rowsum)
        print(f"{name}: {cert['reason']}; c.r {float(k['c_r']):.6g} (reported {cert['c_r']:.6g}), rows moving the wrong way by "
              f"{float(k['residual']):.3e}, bound_dir_violation {float(k['bound_dir_violation']):.3e}, max |r| {float(k['norm']):.3g}, "
              f"source {cert['source']}, qualifying {cert['qualifying']}")
        assert k["c_r"] < 0, name
        assert k["bound_dir_violation"] <= EPS * k["norm"], name
        assert k["residual"] <= EPS * S, name
        # the refinement itself, at the level of u: the standard form's rows are the fixture's with a slack of +-1, so row i
        # of |a_q| + |A_B| |z| is at most 2 (1 + rowsum) max(1, max |r_std|), and the warm start's stop rule leaves a
        # componentwise backward error of at most 2u as reported and 2u more as tests/test_gpu_start.py bounds the exact one;
        # the device's residual (held to the exact one at the seam, tests/test_gpu_certificate.py) is the only view of the
        # slack entries from here
        u = Fraction(2.0 ** -53)
        assert Fraction(cert["residual"]) <= 4 * u * 2 * (1 + rowsum) * max(1, Fraction(cert["norm"])), (name, cert["residual"])


@pytest.mark.parametrize("solver", ["primal", "dual"])
@pytest.mark.parametrize("name", list(CASES))
def test_the_result_carries_its_proof(name, solver):
    make, want = CASES[name]
    fx = make()
    if name.endswith("_x5"):
        assert len(fx["constraints"]) > 128
    assert _oracle_status(fx, solver) == want, name
    S = SOLVERS[solver]
    before = E.certificate_info()["calls"]
    plain = S.default().solve(Problem.from_fixture(fx))
    S.default().solve(Problem.from_fixture(fx), postsolve=True)
    assert E.certificate_info()["calls"] == before  # off: not one certificate call
    assert plain.certificate is None and plain.certificate_reason is None
    res = S.default().solve(Problem.from_fixture(fx), certificate=True)
    assert E.certificate_info()["calls"] == before + 1
    assert res.kind == plain.kind == want and res.iters == plain.iters, (name, res.kind, plain.kind, res.iters, plain.iters)
    _check_certificate(fx, res, f"{name} ({solver})")


def test_a_warm_started_dual_resolve_that_ends_infeasible():
    fx = _afiro()
    first = DualSimplexSolver.default().solve(Problem.from_fixture(fx), ranging=True)
    assert first.kind == "optimal"
    basis = first.solution.basis()
    fx2 = _afiro()
    assert fx2["constraints"][2][0] == [[0, 1.0]] and fx2["constraints"][2][1] == "Lte"
    fx2["constraints"][2][2] = -5.0  # x0 <= -5 with x0 >= 0
    assert _oracle_status(fx2, "dual") == "infeasible"
    plain = DualSimplexSolver.default().solve(Problem.from_fixture(fx2), start=basis)
    res = DualSimplexSolver.default().solve(Problem.from_fixture(fx2), start=basis, certificate=True)
    assert plain.start["used"] and res.start["used"] and res.iters[0] == 0
    assert res.kind == plain.kind == "infeasible" and res.iters == plain.iters
    _check_certificate(fx2, res, "afiro, x0 <= -5, from the optimal basis (dual)")


@pytest.mark.parametrize("solver", ["primal", "dual"])
def test_an_optimal_result_has_none_and_says_so(solver):
    fx = _afiro()
    before = E.certificate_info()["calls"]
    plain = SOLVERS[solver].default().solve(Problem.from_fixture(fx))
    res = SOLVERS[solver].default().solve(Problem.from_fixture(fx), certificate=True, postsolve=True)
    assert res.kind == plain.kind == "optimal" and res.iters == plain.iters
    assert (res.solution.x() == plain.solution.x()).all() and res.solution.obj() == plain.solution.obj()
    assert res.certificate is None and res.certificate_reason == "Optimal" and len(res.solution.duals()) == len(fx["constraints"])
    assert E.certificate_info()["calls"] == before

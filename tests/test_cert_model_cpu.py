"""tests/cert_model.py on hand-worked cases: the exact checks at Problem level and on a standard form, the flag model of the
two searches, and the designed family (its tableau is the designed T, exactly, and the searches find what was planted)."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cert_model as CM  # noqa: E402
from helpers import known_answers  # noqa: E402

FX = {p["name"]: p for p in known_answers()["problems"]}


def test_one_variable_infeasible_by_hand():
    """x <= 0 and x >= 1: y = +1 on the >= row gives z = 1 > 0, sup = 1 * ub = 0, gap = 1"""
    k = CM.problem_farkas_check(FX["one_variable_infeasible"], [1.0])
    assert k["gap"] == 1 and k["dir_violation"] == 0 and k["y_b"] == 1 and k["sup"] == 0 and k["norm"] == 1


def test_two_variables_infeasible_with_bounds_by_hand():
    """x0 >= 0, x1 >= 1, x0 + x1 <= 0: y = -1 gives z = (-1, -1), sup = -1 * 0 + -1 * 1 = -1, y . b = 0, gap = 1"""
    k = CM.problem_farkas_check(FX["two_variables_infeasible_with_bounds"], [-1.0])
    assert k["gap"] == 1 and k["dir_violation"] == 0 and k["sup"] == -1
    assert CM.problem_farkas_check(FX["two_variables_infeasible_with_bounds"], [-0.5])["gap"] == Fraction(1, 2)


def test_a_wrong_signed_y_is_rejected():
    """y = -1 on the >= row: the sign convention is broken (1) and z = -1 needs the lower bound an Upper variable lacks"""
    k = CM.problem_farkas_check(FX["one_variable_infeasible"], [-1.0])
    assert k["gap"] < 0 and k["dir_violation"] == 1
    k = CM.problem_farkas_check(FX["two_variables_infeasible_with_bounds"], [1.0])  # z = (1, 1): Lower has no upper bound
    assert k["dir_violation"] == 1 and not k["gap"] > 0


@pytest.mark.parametrize("name,ray,c_r", [("small_prob_unbounded_1", [1.0, 1.0, 0.0], -5), ("small_prob_unbounded_2", [1.0, 1.0, 0.0, 0.0], -5)])
def test_small_prob_unbounded_rays_by_hand(name, ray, c_r):
    """(1, 1, 0[, 0]): every >= row moves by >= 0 (1: 2, 0, 0; 2: 1, 1, 0), every variable is Lower and moves up, c . r = -5"""
    k = CM.problem_ray_check(FX[name], ray)
    assert k["c_r"] == c_r and k["residual"] == 0 and k["bound_dir_violation"] == 0 and k["norm"] == 1


def test_a_blocked_ray_is_rejected():
    """(1, 0, 0) on small_prob_unbounded_1: row 2 (-x0 + x1 - x2 >= -4) shrinks by 1; (-1, 0, 0) runs into x0 >= 0"""
    k = CM.problem_ray_check(FX["small_prob_unbounded_1"], [1.0, 0.0, 0.0])
    assert k["c_r"] == -2 and k["residual"] == 1
    k = CM.problem_ray_check(FX["small_prob_unbounded_1"], [-1.0, 0.0, 0.0])
    assert k["bound_dir_violation"] == 1 and k["worst_bound_var"] == 0


def test_standard_form_checks_agree_with_the_problem_level_ones():
    """one_variable_infeasible as a standard form: x - s = 1, x Upper(0), s Lower(0); y = 1: z = (1, -1), gap = 1"""
    std = {"A": np.array([[1.0, -1.0]]), "b": [1.0], "c": [2.0, 0.0], "kind": [CM.UPPER, CM.LOWER], "lb": [0.0, 0.0], "ub": [0.0, 0.0]}
    k = CM.farkas_check(std, [1.0])
    assert k["gap"] == 1 and k["dir_violation"] == 0
    k = CM.farkas_check(std, [-1.0])  # the slack column shows the wrong sign
    assert k["dir_violation"] == 1 and k["gap"] == -1
    std = {"A": np.array([[1.0, -1.0]]), "b": [0.0], "c": [-1.0, 0.0], "kind": [CM.LOWER, CM.LOWER], "lb": [0.0, 0.0], "ub": [0.0, 0.0]}
    k = CM.ray_check(std, [1.0, 1.0])
    assert k["c_r"] == -1 and k["residual"] == 0 and k["bound_dir_violation"] == 0
    k = CM.ray_check(std, [1.0, 0.0])
    assert k["residual"] == 1
    std["kind"] = [CM.TWOSIDED, CM.FIXED]
    k = CM.ray_check(std, [1.0, -1.0])
    assert k["bound_dir_violation"] == 1 and k["worst_bound_var"] == 0


def test_the_rules_of_the_flag_model():
    eps = 2.0 ** -20
    assert CM.dual_violation(-1.0, CM.LOWER, 0.0, 0.0, eps) == CM.NB_LOWER and CM.dual_violation(-eps, CM.LOWER, 0.0, 0.0, eps) is None
    assert CM.dual_violation(5.0, CM.TWOSIDED, 0.0, 4.0, eps) == CM.NB_UPPER and CM.dual_violation(9.0, CM.FREE, 0.0, 0.0, eps) is None
    assert CM.dual_violation(9.0, CM.FIXED, 0.0, 0.0, eps) is None  # Free and Fixed basics never leave
    assert CM.dual_keep(2 * eps, CM.NB_LOWER, eps) and not CM.dual_keep(eps, CM.NB_LOWER, eps)  # strict
    assert CM.dual_keep(-2 * eps, CM.NB_UPPER, eps) and not CM.dual_keep(-eps, CM.NB_UPPER, eps) and CM.dual_keep(0.0, CM.NB_FREE, eps)
    assert CM.primal_key(-1.0, CM.NB_LOWER, eps) == 1.0 and CM.primal_key(1.0, CM.NB_LOWER, eps) == -np.inf
    assert CM.primal_key(eps, CM.NB_UPPER, eps) == eps and CM.primal_key(eps / 2, CM.NB_FREE, eps) == -np.inf
    assert CM.primal_lambda(eps / 2, 5.0, 0.0, 0.0, CM.LOWER, eps) == np.inf and CM.primal_lambda(-eps, 5.0, 0.0, 0.0, CM.LOWER, eps) == 5.0 / eps
    assert CM.primal_lambda(1.0, 5.0, 0.0, 0.0, CM.LOWER, eps) == np.inf and CM.primal_lambda(1.0, 5.0, 0.0, 0.0, CM.FIXED, eps) == 0.0
    assert CM.ray_up(CM.NB_LOWER, 9.0) and not CM.ray_up(CM.NB_UPPER, -9.0) and CM.ray_up(CM.NB_FREE, -1.0) and not CM.ray_up(CM.NB_FREE, 1.0)


def _searches(inst, eps):
    m, nN = inst["m"], inst["nN"]
    B, N = inst["B"], inst["N"]
    f = CM.farkas_row_search(inst["T"], inst["x"][B], inst["kind"][B], inst["lb"][B], inst["ub"][B], inst["Nb"], eps)
    d = inst["c"] - inst["A"].T @ inst["y"]
    r = CM.ray_search(inst["T"], d[N], inst["Nb"], inst["kind"][N], inst["x"][B], inst["kind"][B], inst["lb"][B], inst["ub"][B], eps)
    return f, r, d


@pytest.mark.parametrize("m,nN", [(3, 4), (129, 130)])
def test_the_designed_family_is_exact_and_finds_what_was_planted(m, nN):
    eps = 2.0 ** -20
    inst = CM.farkas_family(m, nN, {m - 1: CM.NB_UPPER, 1: CM.NB_LOWER}, 5, eps)
    assert (inst["W"] @ inst["A"][:, :nN] == inst["T"]).all() and (inst["W"] @ inst["b"] - inst["T"] @ inst["x"][:nN] == inst["x"][nN:]).all()
    f, r, d = _searches(inst, eps)
    assert f == (1, 2, CM.NB_LOWER, False) and (d[:nN] == 0).all() and r[0] == -1
    y = -inst["W"][1]
    k = CM.farkas_check(inst, y)
    assert k["gap"] == 3 and k["dir_violation"] == 0  # the violation of row 1: x = -3 below 0
    f, _, _ = _searches(CM.farkas_family(m, nN, {1: CM.NB_LOWER}, 5, eps, blocker=(1, nN - 1)), eps)
    assert f[0] == -1 and f[1] == 0
    f, _, _ = _searches(CM.farkas_family(m, nN, {1: CM.NB_LOWER}, 5, eps, at_eps=(1, nN - 1)), eps)
    assert f[0] == 1
    inst = CM.ray_family(m, nN, {nN - 1: CM.NB_FREE, 2: CM.NB_UPPER}, 6, eps)
    f, r, d = _searches(inst, eps)
    assert r == (2, 2, False, False) and f[0] == -1
    ray = np.zeros(inst["n"])
    ray[2], ray[inst["B"]] = -1.0, inst["T"][:, 2]
    k = CM.ray_check(inst, ray)
    assert k["c_r"] == -2 and k["residual"] == 0 and k["bound_dir_violation"] == 0
    _, r, _ = _searches(CM.ray_family(m, nN, {2: CM.NB_UPPER}, 6, eps, blocker=(m - 1, 2)), eps)
    assert r[0] == -1
    _, r, _ = _searches(CM.ray_family(m, nN, {2: CM.NB_UPPER}, 6, eps, at_eps=(m - 1, 2)), eps)
    assert r[0] == -1  # an entry of exactly eps counts

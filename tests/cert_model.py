"""The model of the certificates (include/ellp_hip.h).

1. farkas_check / ray_check: the report of a vector in EXACT rational arithmetic on a standard form A x = b, bounds
   (kind, lb, ub), minimise c . x.  A bound counts as infinite by its KIND (Free, Lower's upper side, Upper's lower side),
   never by the value stored for it.
2. problem_farkas_check / problem_ray_check: the same at Problem level, straight from a fixture's vars and constraints (no
   standard form in between): y by constraint with the sign convention of duals() (<= 0 on a `<=` row, >= 0 on a `>=`
   row; a wrong sign counts |y_i| into dir_violation), a ray by variable (a `<=` row must not grow, a `>=` row not shrink, an
   `==` row not move: what it does instead is the residual).
3. The flag model of the two searches, on values in hand (the device's rules, ellp_rules.inc, stated once more):
   farkas_row_search and ray_search.
4. exact_family: designed instances on which every alpha_ij, d_j and x_i is an integer of a few digits — exact in f64 in any
   summation order: block-diagonal bases of unit upper triangular 3 x 3 integer blocks (no pivoting, integer inverse),
   A_N = A_B T for a designed integer T, so the tableau IS T.  dense=True: the same plan on a general dense basis with real
   entries, where nothing is exact (the signs of the planted entries hold, with a margin far above rounding)."""
from fractions import Fraction

import numpy as np

FREE, LOWER, UPPER, TWOSIDED, FIXED = 0, 1, 2, 3, 4
NB_LOWER, NB_UPPER, NB_FREE = 0, 1, 2
KIND_BY_NAME = {"Free": FREE, "Lower": LOWER, "Upper": UPPER, "TwoSided": TWOSIDED, "Fixed": FIXED}


def has_ub(kind):
    return kind in (UPPER, TWOSIDED, FIXED)


def has_lb(kind):
    return kind in (LOWER, TWOSIDED, FIXED)


def _fr(v):
    return Fraction(float(v))


def _sup_terms(z, kinds, lbs, ubs):
    """sum of sup_j and the (dir_violation, first index) of z"""
    sup, dirv, worst = Fraction(0), Fraction(0), -1
    for j, zj in enumerate(z):
        k = int(kinds[j])
        ub = ubs[j] if k != FIXED else lbs[j]
        if zj > 0:
            if has_ub(k):
                sup += zj * _fr(ub)
            elif zj > dirv:
                dirv, worst = zj, j
        elif zj < 0:
            if has_lb(k):
                sup += zj * _fr(lbs[j])
            elif -zj > dirv:
                dirv, worst = -zj, j
    return sup, dirv, worst


def farkas_check(std, y):
    """std: dict A (m x n), b, kind, lb, ub (n_check = len(kind) leading columns take part).  Fractions."""
    A, n = np.asarray(std["A"]), len(std["kind"])
    yf = [_fr(v) for v in y]
    z = [sum((yf[i] * _fr(A[i, j]) for i in range(A.shape[0]) if A[i, j] != 0.0 and yf[i] != 0), Fraction(0)) for j in range(n)]
    y_b = sum((yf[i] * _fr(std["b"][i]) for i in range(A.shape[0])), Fraction(0))
    sup, dirv, worst = _sup_terms(z, std["kind"], std["lb"], std["ub"])
    return {"gap": y_b - sup, "y_b": y_b, "sup": sup, "dir_violation": dirv, "worst_dir_var": worst,
            "norm": max([abs(v) for v in yf] + [Fraction(0)])}


def _bound_dir(r, kinds):
    bd, worst = Fraction(0), -1
    for j, rj in enumerate(r):
        k = int(kinds[j])
        if ((rj > 0 and has_ub(k)) or (rj < 0 and has_lb(k))) and abs(rj) > bd:
            bd, worst = abs(rj), j
    return bd, worst


def ray_check(std, r):
    """std as above with c; r: n_check entries."""
    A, n = np.asarray(std["A"]), len(std["kind"])
    rf = [_fr(v) for v in r[:n]]
    rows = [sum((_fr(A[i, j]) * rf[j] for j in range(n) if A[i, j] != 0.0 and rf[j] != 0), Fraction(0)) for i in range(A.shape[0])]
    res = max([abs(v) for v in rows] + [Fraction(0)])
    bd, worst = _bound_dir(rf, std["kind"])
    return {"residual": res, "rows": rows, "c_r": sum((_fr(std["c"][j]) * rf[j] for j in range(n)), Fraction(0)),
            "bound_dir_violation": bd, "worst_bound_var": worst, "norm": max([abs(v) for v in rf] + [Fraction(0)])}


def _fx_bounds(fx):
    kinds = [KIND_BY_NAME[b[0]] for _, b in fx["vars"]]
    return kinds, [b[1] for _, b in fx["vars"]], [b[2] for _, b in fx["vars"]]


def problem_farkas_check(fx, y):
    """y: one entry per constraint of the fixture"""
    n = len(fx["vars"])
    yf = [_fr(v) for v in y]
    z = [Fraction(0)] * n
    y_b, dirv, worst = Fraction(0), Fraction(0), -1
    for i, (coeffs, op, rhs) in enumerate(fx["constraints"]):
        for j, a in coeffs:
            z[j] += yf[i] * _fr(a)
        y_b += yf[i] * _fr(rhs)
        if (op == "Lte" and yf[i] > 0) or (op == "Gte" and yf[i] < 0):
            dirv = max(dirv, abs(yf[i]))
    kinds, lbs, ubs = _fx_bounds(fx)
    sup, dv, worst = _sup_terms(z, kinds, lbs, ubs)
    return {"gap": y_b - sup, "y_b": y_b, "sup": sup, "dir_violation": max(dirv, dv), "worst_dir_var": worst,
            "norm": max([abs(v) for v in yf] + [Fraction(0)])}


def problem_ray_check(fx, r):
    """r: one entry per variable of the fixture"""
    rf = [_fr(v) for v in r]
    res = Fraction(0)
    for coeffs, op, rhs in fx["constraints"]:
        ar = sum((_fr(a) * rf[j] for j, a in coeffs), Fraction(0))
        res = max(res, ar if op == "Lte" else (-ar if op == "Gte" else abs(ar)))
    kinds, _, _ = _fx_bounds(fx)
    bd, worst = _bound_dir(rf, kinds)
    return {"residual": res, "c_r": sum((_fr(obj) * rf[j] for j, (obj, _) in enumerate(fx["vars"])), Fraction(0)),
            "bound_dir_violation": bd, "worst_bound_var": worst, "norm": max([abs(v) for v in rf] + [Fraction(0)])}


# ---------------------------------------------------------------- the flag model of the searches
def dual_violation(x, kind, lb, ub, eps):
    """the dual loop's leaving rule: the side (NB_LOWER / NB_UPPER) outside which x lies by more than eps, or None"""
    if kind == LOWER:
        return NB_LOWER if x < lb - eps else None
    if kind == UPPER:
        return NB_UPPER if x > ub + eps else None
    if kind == TWOSIDED:
        if x > ub + eps:
            return NB_UPPER
        return NB_LOWER if x < lb - eps else None
    return None


def dual_keep(al, nb, eps):
    if nb == NB_LOWER:
        return al > eps
    if nb == NB_UPPER:
        return al < -eps
    return True


def farkas_row_search(alpha, xB, kindB, lbB, ubB, Nb, eps):
    """alpha: m x nN; the basic variables' values, kinds and bounds by position.  (first, count, side of first, nan)"""
    alpha = np.asarray(alpha, dtype=np.float64).reshape(len(xB), -1)
    nan = bool(np.isnan(alpha).any() or np.isnan(np.asarray(xB, dtype=np.float64)).any())
    first, count, side0 = -1, 0, None
    for i in range(len(xB)):
        side = dual_violation(xB[i], int(kindB[i]), lbB[i], ubB[i], eps)
        if side is None:
            continue
        sg = -1.0 if side == NB_LOWER else 1.0
        if any(dual_keep(sg * alpha[i, j], int(Nb[j]), eps) for j in range(alpha.shape[1])):
            continue
        count += 1
        if first < 0:
            first, side0 = i, side
    return first, count, side0, nan


def primal_key(rj, nb, eps):
    if rj != rj or abs(rj) < eps:
        return -np.inf
    if rj > 0 and nb == NB_UPPER:
        return rj
    if not rj > 0 and nb == NB_LOWER:
        return -rj
    if nb == NB_FREE:
        return abs(rj)
    return -np.inf


def primal_lambda(di, xi, lbi, ubi, kind, eps):
    if abs(di) < eps:
        return np.inf
    if kind == FREE:
        return np.inf
    if kind == LOWER:
        if di > 0:
            return np.inf
        return (lbi - xi) / di if xi > lbi else 0.0
    if kind == UPPER:
        if di > 0:
            return (ubi - xi) / di if xi < ubi else 0.0
        return np.inf
    if kind == TWOSIDED:
        if di > 0:
            return (ubi - xi) / di if xi < ubi else 0.0
        return (lbi - xi) / di if xi < lbi else 0.0
    return 0.0


def ray_up(nb, dj):
    """the direction of the step: up from a Lower label, down from an Upper one, a Free one against the sign of d"""
    return nb == NB_LOWER or (nb == NB_FREE and dj < 0.0)


def ray_search(alpha, dN, Nb, kindN, xB, kindB, lbB, ubB, eps):
    """dN, Nb, kindN by nonbasic position.  (first, count, up of first, nan)"""
    alpha = np.asarray(alpha, dtype=np.float64).reshape(len(xB), -1)
    nan = bool(np.isnan(alpha).any() or np.isnan(np.asarray(dN, dtype=np.float64)).any() or
               (alpha.shape[1] > 0 and np.isnan(np.asarray(xB, dtype=np.float64)).any()))
    first, count, up0 = -1, 0, None
    for j in range(alpha.shape[1]):
        if not primal_key(dN[j], int(Nb[j]), eps) > -np.inf or int(kindN[j]) not in (FREE, LOWER, UPPER):
            continue
        up = ray_up(int(Nb[j]), dN[j])
        if any(primal_lambda(-alpha[i, j] if up else alpha[i, j], xB[i], lbB[i], ubB[i], int(kindB[i]), eps) != np.inf
               for i in range(len(xB))):
            continue
        count += 1
        if first < 0:
            first, up0 = j, up
    return first, count, up0, nan


# ---------------------------------------------------------------- the exact family
def exact_basis(m, rng):
    """(A_B, W): block-diagonal, unit upper triangular 3 x 3 blocks (the last one smaller) with entries in -2 .. 2 above the
    diagonal, and its integer inverse"""
    A_B, W = np.zeros((m, m)), np.zeros((m, m))
    for s in range(0, m, 3):
        k = min(3, m - s)
        blk = np.eye(k) + np.triu(rng.integers(-2, 3, (k, k)).astype(np.float64), 1)
        A_B[s:s + k, s:s + k] = blk
        W[s:s + k, s:s + k] = np.round(np.linalg.inv(blk))
    assert (A_B @ W == np.eye(m)).all()
    return A_B, W


def dense_basis(m, rng):
    """a general dense basis (nothing about it is exact) and numpy's inverse of it"""
    A_B = rng.uniform(-1.0, 1.0, (m, m)) + 3.0 * np.diag(rng.choice([-1.0, 1.0], m))
    return A_B, np.linalg.inv(A_B)


def exact_instance(m, nN, T, xB, kindB, lbB, ubB, Nb, kindN, lbN, ubN, dN, rng, dense=False):
    """The standard form whose tableau is T, whose basic values are xB and whose nonbasic reduced costs are dN, all exactly:
    columns [A_N | A_B] (nonbasic variables 0 .. nN-1 first), x_N on the bound its label names (0 for a Free one),
    b = A_B xB + A_N x_N, c_B drawn, c_N = dN + A_N^T y.  Returns a dict of arrays."""
    A_B, W = dense_basis(m, rng) if dense else exact_basis(m, rng)
    T = np.asarray(T, dtype=np.float64).reshape(m, nN)
    if dense:  # the signs stay, nothing else: A_N = fl(A_B T), so the tableau is T only to rounding
        T = T * rng.uniform(0.5, 1.5, T.shape)
    A_N = A_B @ T
    xN = np.array([ubN[j] if Nb[j] == NB_UPPER else (0.0 if Nb[j] == NB_FREE else lbN[j]) for j in range(nN)], dtype=np.float64)
    b = A_B @ np.asarray(xB, dtype=np.float64) + (A_N @ xN if nN else 0.0)
    cB = rng.integers(-3, 4, m).astype(np.float64)
    y = W.T @ cB
    cN = np.asarray(dN, dtype=np.float64) + (A_N.T @ y if nN else np.zeros(0))
    n = m + nN
    return {"m": m, "n": n, "nN": nN, "A": np.concatenate([A_N, A_B], axis=1), "A_B": A_B, "W": W, "T": T, "b": b,
            "c": np.concatenate([cN, cB]), "kind": np.concatenate([kindN, kindB]).astype(np.uint8),
            "lb": np.concatenate([lbN, lbB]).astype(np.float64), "ub": np.concatenate([ubN, ubB]).astype(np.float64),
            "x": np.concatenate([xN, np.asarray(xB, dtype=np.float64)]), "B": nN + np.arange(m, dtype=np.int64),
            "N": np.arange(nN, dtype=np.int64), "Nb": np.asarray(Nb, dtype=np.uint8), "y": y}


def farkas_family(m, nN, rows, seed, eps=1e-10, blocker=None, at_eps=None, dense=False):
    """Every basic variable Lower(0) at 5 except `rows`: {position: side}, outside that side by 3.  T in -3 .. 3 drawn, then
    in every row of `rows` the entries a label would keep are taken away (NB_LOWER: sign * alpha <= 0, NB_UPPER: >= 0), so each
    of them qualifies; in every other row nothing is arranged (they do not violate).  blocker = (row, column): one entry
    put back that passes the filter; at_eps = (row, column): one entry of magnitude exactly eps on the keeping side (it does
    not pass: the rule is strict)."""
    rng = np.random.default_rng(seed)
    Nb = rng.integers(0, 2, nN).astype(np.uint8)  # no Free label: dual_keep keeps such a column whatever alpha is
    kindN = np.where(Nb == NB_LOWER, LOWER, UPPER)
    lbN, ubN = np.where(Nb == NB_LOWER, 1.0, 0.0), np.where(Nb == NB_UPPER, 2.0, 0.0)
    T = rng.integers(-3, 4, (m, nN)).astype(np.float64)
    kindB, lbB, ubB, xB = np.full(m, LOWER), np.zeros(m), np.zeros(m), np.full(m, 5.0)
    for r, side in rows.items():
        sg = -1.0 if side == NB_LOWER else 1.0
        keepsign = np.where(Nb == NB_LOWER, 1.0, -1.0) * sg  # alpha of this sign would pass
        T[r] = np.where(T[r] * keepsign > 0, -T[r], T[r])
        if side == NB_LOWER:
            xB[r] = -3.0
        else:
            kindB[r], ubB[r], xB[r] = UPPER, 4.0, 7.0
    for spec, mag in ((blocker, 2.0), (at_eps, eps)):
        if spec is not None:
            r, j = spec
            sg = -1.0 if rows[r] == NB_LOWER else 1.0
            T[r, j] = mag * sg * (1.0 if Nb[j] == NB_LOWER else -1.0)
    return exact_instance(m, nN, T, xB, kindB, lbB, ubB, Nb, kindN, lbN, ubN, np.zeros(nN), rng, dense)


def ray_family(m, nN, cols, seed, eps=1e-10, blocker=None, at_eps=None, dense=False):
    """Every basic variable Lower(0) at 5 (a row bounds a step that lowers it), every nonbasic column Lower(0) with d = +2 (no
    candidate) except `cols`: {position: label}: d of the sign that label asks for (a Free one: -2, so the step goes up) and
    a column of T that lowers no basic variable.  blocker = (row, column): one entry that does; at_eps: one of magnitude
    exactly eps that does (it counts: the rule treats only |alpha| < eps as zero)."""
    rng = np.random.default_rng(seed)
    Nb, kindN = np.zeros(nN, dtype=np.uint8), np.full(nN, LOWER)
    lbN, ubN, dN = np.zeros(nN), np.zeros(nN), np.full(nN, 2.0)
    T = rng.integers(-3, 4, (m, nN)).astype(np.float64)
    for q, label in cols.items():
        Nb[q] = label
        kindN[q] = {NB_LOWER: LOWER, NB_UPPER: UPPER, NB_FREE: FREE}[label]
        dN[q] = 2.0 if label == NB_UPPER else -2.0
        up = ray_up(label, dN[q])
        T[:, q] = -np.abs(T[:, q]) if up else np.abs(T[:, q])  # x_B moves by -+T: never down
    for spec, mag in ((blocker, 2.0), (at_eps, eps)):
        if spec is not None:
            i, q = spec
            T[i, q] = mag if ray_up(int(Nb[q]), dN[q]) else -mag
    kindB, lbB, ubB, xB = np.full(m, LOWER), np.zeros(m), np.zeros(m), np.full(m, 5.0)
    return exact_instance(m, nN, T, xB, kindB, lbB, ubB, Nb, kindN, lbN, ubN, dN, rng, dense)

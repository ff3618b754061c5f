"""Models of the sensitivity ranging (ellp_amd/csrc/engine/ellp_range.inc) for the tests.  The definitions
are those of include/ellp_hip.h, applied twice.

F64 MODEL.  Given the tableau rows alpha, the rows of W, d and the point as f64 arrays, the limits and blocking indices in
plain numpy f64: comparisons against eps, one division per candidate, "+ 0.0" (every zero is +0.0), min / max with ties to the
smallest position, NaN as stated there.  None of it depends on an order of summation, so the device must give these bits.
inverse_residual_f64 forms I - A_B W with every entry summed in ascending k, product and sum rounded separately, as
k_range_resid does.

EXACT MODEL.  The same definitions in rational arithmetic from the problem's f64 data: the exact inverse of A_B (fraction-free
elimination), exact y, d, tableau and W; fl(.) is the identity.  Unlimited is +-math.inf, blocking -1.  check_meaning states
what a limit means: just inside it every nonbasic reduced cost (every basic variable) keeps the sign (the bound) its label
(its kind) demands, just outside the blocking one has lost it.
"""
import math
from fractions import Fraction

import numpy as np

from postsolve_model import exact_dot

INF = math.inf
FREE, LOWER, UPPER, TWOSIDED, FIXED = 0, 1, 2, 3, 4  # bound kinds
NB_LOWER, NB_UPPER, NB_FREE = 0, 1, 2               # nonbasic labels


# ---------------------------------------------------------------------------------------------------------- f64 model
def _pos(v):
    return np.where(np.isnan(v), v, np.where(v > 0.0, v, 0.0))


def _neg(v):
    return np.where(np.isnan(v), v, np.where(v < 0.0, v, 0.0))


def cost_candidates(al, dv, code, eps):
    """(qu, qd) of tableau entries al (rows x positions) against d (by position) and code (label, or 3: Fixed / not read);
    +inf / -inf: no candidate"""
    al = np.asarray(al, dtype=np.float64)
    with np.errstate(all="ignore"):
        ps, ns = al > eps, al < -eps
        lower, upper, skip = code == NB_LOWER, code == NB_UPPER, code == 3
        p, n = _pos(dv), _neg(dv)
        nu = np.where(lower, p, np.where(upper, n, np.where(ps, p, n)))
        nd = np.where(lower, p, np.where(upper, n, np.where(ps, n, p)))
        cu = np.where(lower, ps, np.where(upper, ns, ps | ns))
        cd = np.where(lower, ns, np.where(upper, ps, ps | ns))
        u, d = nu / al + 0.0, nd / al + 0.0
        bad = np.isnan(al) | (cu & np.isnan(u)) | (cd & np.isnan(d))
        qu = np.where(bad, np.nan, np.where(cu, u, INF))
        qd = np.where(bad, np.nan, np.where(cd, d, -INF))
        return np.where(skip, INF, qu), np.where(skip, -INF, qd)


def rhs_candidates(W, xB, lbB, ubB, kindB, eps):
    """(qu, qd)[i][k] of W[i][k] against the basic variable of row i"""
    W = np.asarray(W, dtype=np.float64)
    col = lambda a: np.asarray(a)[:, None]
    x, lb, ub, kind = col(xB), col(lbB), col(ubB), col(kindB)
    with np.errstate(all="ignore"):
        ps, ns = W > eps, W < -eps
        has_u = (kind == UPPER) | (kind == TWOSIDED) | (kind == FIXED)
        has_l = (kind == LOWER) | (kind == TWOSIDED) | (kind == FIXED)
        to_u = np.where(has_u, _pos(ub - x), 0.0) + np.zeros_like(W)
        to_l = np.where(has_l, _pos(x - lb), 0.0) + np.zeros_like(W)
        cu = np.where(ps, has_u, has_l) & (ps | ns)
        cd = np.where(ps, has_l, has_u) & (ps | ns)
        u = np.where(ps, to_u / W, to_l / -W) + 0.0
        d = np.where(ps, to_l / -W, to_u / W) + 0.0
        bad = np.isnan(W) | (cu & np.isnan(u)) | (cd & np.isnan(d))
        return np.where(bad, np.nan, np.where(cu, u, INF)), np.where(bad, np.nan, np.where(cd, d, -INF))


def fold(q, up):
    """per row of q: (limit, position) — NaN wins (its first position), else the smallest (up) or largest value at its first
    position; position -1 for an infinite limit"""
    q = np.asarray(q, dtype=np.float64)
    rows = q.shape[0]
    if q.shape[1] == 0:
        return np.full(rows, INF if up else -INF), np.full(rows, -1, dtype=np.int64)
    nanm = np.isnan(q)
    anyn = nanm.any(axis=1)
    qq = np.where(nanm, INF if up else -INF, q)
    p = qq.argmin(axis=1) if up else qq.argmax(axis=1)
    v = qq[np.arange(rows), p]
    v = np.where(anyn, np.nan, v)
    p = np.where(anyn, nanm.argmax(axis=1), p)
    return v, np.where(np.isinf(v), -1, p).astype(np.int64)


def _blocking(p, index):
    index = np.asarray(index, dtype=np.int64)
    return np.where(p < 0, -1, index[np.maximum(p, 0)]) if len(index) else np.full(len(p), -1, dtype=np.int64)


def cost_ranging_f64(alpha, d, B, N, Nb, kind, n, n_c, eps):
    """(down, up, blocking_down, blocking_up), n_c entries by variable.  alpha: m x n_N, every tableau row by nonbasic position"""
    d, B, N = np.asarray(d, dtype=np.float64), np.asarray(B, dtype=np.int64), np.asarray(N, dtype=np.int64)
    Nb, kind = np.asarray(Nb).astype(np.int64), np.asarray(kind).astype(np.int64)
    down, up = np.full(n_c, -INF), np.full(n_c, INF)
    bdown, bup = np.full(n_c, -1, dtype=np.int64), np.full(n_c, -1, dtype=np.int64)
    dN = d[N]
    code = np.where(kind[N] == FIXED, 3, Nb)
    # the basic variables
    qu, qd = cost_candidates(np.asarray(alpha, dtype=np.float64).reshape(len(B), len(N)), dN, code, eps)
    vu, pu = fold(qu, True)
    vd, pd = fold(qd, False)
    up[B], down[B], bup[B], bdown[B] = vu, vd, _blocking(pu, N), _blocking(pd, N)
    # the nonbasic variables
    with np.errstate(all="ignore"):
        lower, upper, free = code == NB_LOWER, code == NB_UPPER, code == NB_FREE
        u = np.where(upper, 0.0 - _neg(dN), np.where(free, _pos(-dN), INF))
        dn = np.where(lower, 0.0 - _pos(dN), np.where(free, _neg(-dN), -INF))
        nan = np.isnan(dN) & (code != 3)
        u, dn = np.where(nan, np.nan, u), np.where(nan, np.nan, dn)
    up[N], down[N] = u, dn
    bup[N], bdown[N] = np.where(u == INF, -1, N), np.where(dn == -INF, -1, N)
    return down, up, bdown, bup


def rhs_ranging_f64(W, x, B, kind, lb, ub, eps):
    """(down, up, blocking_down, blocking_up), m entries by row.  W: m x m, the computed inverse by rows"""
    B = np.asarray(B, dtype=np.int64)
    x, lb, ub, kind = (np.asarray(a) for a in (x, lb, ub, kind))
    qu, qd = rhs_candidates(W, x[B], lb[B], ub[B], kind[B].astype(np.int64), eps)
    vu, pu = fold(qu.T, True)
    vd, pd = fold(qd.T, False)
    return vd, vu, _blocking(pd, B), _blocking(pu, B)


def inverse_residual_f64(A_B, W):
    """NaN-propagating max |I - A_B W|, each entry one sum over k ascending, products and sums rounded one by one"""
    A_B, W = np.asarray(A_B, dtype=np.float64), np.asarray(W, dtype=np.float64)
    m = A_B.shape[0]
    with np.errstate(all="ignore"):
        S = np.zeros((m, m))
        for k in range(m):
            S = S + np.outer(A_B[:, k], W[k, :])
        E = np.abs(np.eye(m) - S)
    return float("nan") if np.isnan(E).any() else float(E.max())


# -------------------------------------------------------------------------------------------------------- exact model
def int_matrix(a):
    """(Z, e): an object array of Python integers and an exponent with a = Z * 2^e exactly, for any f64 array a"""
    a = np.asarray(a, dtype=np.float64)
    mant, ex = np.frexp(a)
    nz = a != 0.0
    emin = int(ex[nz].min()) if nz.any() else 0
    z = (mant * 9007199254740992.0).astype(np.int64).astype(object)  # 2^53 * mantissa: an integer
    up = np.where(nz, ex - emin, 0).astype(object)
    return z * (2 ** up), emin - 53


def exact_inverse_int(M):
    """(Z, scale): the inverse of a square f64 matrix is Z * scale exactly, Z an object array of integers, scale a Fraction
    (fraction-free Gauss-Jordan: every division is exact and all diagonal entries end equal)"""
    Z, e = int_matrix(M)
    m = Z.shape[0]
    T = np.concatenate([Z, np.array([[int(i == j) for j in range(m)] for i in range(m)], dtype=object).reshape(m, m)], axis=1)
    prev = 1
    for c in range(m):
        piv = next((r for r in range(c, m) if T[r, c] != 0), None)
        if piv is None:
            raise ZeroDivisionError("singular matrix")
        if piv != c:
            T[[c, piv]] = T[[piv, c]]
        pc = T[c].copy()
        T = (pc[c] * T - np.outer(T[:, c], pc)) // prev
        T[c] = pc
        prev = pc[c]
    # T = [D I | D * (Z 2^e)^-1]
    return T[:, m:], Fraction(1, prev) / (Fraction(2) ** e)


def exact_inverse(M):
    """the inverse of a square f64 matrix as a list of rows of Fractions"""
    Z, scale = exact_inverse_int(M)
    return [[v * scale for v in row] for row in Z]


def _fr(v):
    return Fraction(float(v))


class ExactRanging:
    """The exact ranges of one basis and point.  A: (m, n) array or the column-major vector of a FlatProblem."""

    def __init__(self, m, n, n_c, A, c, b, kind, lb, ub, x, B, N, Nb, eps=1e-10):
        self.m, self.n, self.n_c = int(m), int(n), int(n_c)
        self.A = np.asarray(A, dtype=np.float64).reshape(self.n, self.m).T if np.ndim(A) == 1 else np.asarray(A, dtype=np.float64)
        self.c, self.b, self.x = (np.asarray(v, dtype=np.float64) for v in (c, b, x))
        self.kind, self.lb, self.ub = np.asarray(kind).astype(np.int64), np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
        self.B, self.N, self.Nb = np.asarray(B, dtype=np.int64), np.asarray(N, dtype=np.int64), np.asarray(Nb).astype(np.int64)
        self.eps = Fraction(float(eps))
        Wz, ws = exact_inverse_int(self.A[:, self.B])
        self.W = [[v * ws for v in row] for row in Wz]                  # rows rho_i
        Az, ae = int_matrix(self.A[:, self.N])
        cz, ce = int_matrix(self.c[self.B])
        asc = Fraction(2) ** ae
        self.y = [v * ws * Fraction(2) ** ce for v in cz.dot(Wz)]
        yA = cz.dot(Wz).dot(Az) if len(self.N) else []
        self.dN = [_fr(self.c[v]) - t * ws * Fraction(2) ** ce * asc for v, t in zip(self.N, yA)]
        self._alpha_z, self._alpha_scale = (Wz.dot(Az) if len(self.N) else np.zeros((self.m, 0), dtype=object)), ws * asc
        self._alpha = {}

    @classmethod
    def of(cls, fp, eps=1e-10):
        return cls(fp.m, fp.n, fp.n_c, fp.A, fp.c, fp.b, fp.kind, fp.lb, fp.ub, fp.x, fp.B, fp.N[:fp.nN], fp.Nb[:fp.nN], eps)

    def alpha(self, i):
        """row i of the tableau, by nonbasic position"""
        if i not in self._alpha:
            self._alpha[i] = [v * self._alpha_scale for v in self._alpha_z[i]]
        return self._alpha[i]

    def code(self, j):
        return 3 if self.kind[self.N[j]] == FIXED else int(self.Nb[j])

    def numerators(self, j, a):
        """(numerator for up, numerator for down) of position j against an entry of sign a: d_v clamped to the sign its label
        demands (Free: so that up >= 0 >= down)"""
        d, code = self.dN[j], self.code(j)
        p, n = max(d, Fraction(0)), min(d, Fraction(0))
        if code == NB_LOWER:
            return p, p
        if code == NB_UPPER:
            return n, n
        return (p, n) if a > 0 else (n, p)

    def cost_basic(self, i):
        """(down, up, blocking_down, blocking_up) of the basic variable at position i"""
        up, dn, bu, bd = INF, -INF, -1, -1
        for j, a in enumerate(self.alpha(i)):
            code = self.code(j)
            if code == 3 or abs(a) <= self.eps:
                continue
            nu, nd = self.numerators(j, a)
            cu = a > 0 if code == NB_LOWER else (a < 0 if code == NB_UPPER else True)
            cd = a < 0 if code == NB_LOWER else (a > 0 if code == NB_UPPER else True)
            if cu and nu / a < up:
                up, bu = nu / a, int(self.N[j])
            if cd and nd / a > dn:
                dn, bd = nd / a, int(self.N[j])
        return dn, up, bd, bu

    def cost_nonbasic(self, j):
        d, code, v = self.dN[j], self.code(j), int(self.N[j])
        if code == 3:
            return -INF, INF, -1, -1
        if code == NB_LOWER:
            return -max(d, Fraction(0)), INF, v, -1
        if code == NB_UPPER:
            return -INF, -min(d, Fraction(0)), -1, v
        return min(-d, Fraction(0)), max(-d, Fraction(0)), v, v

    def rhs(self, k):
        """(down, up, blocking_down, blocking_up) of right-hand side k, from the point's own x"""
        up, dn, bu, bd = INF, -INF, -1, -1
        for i in range(self.m):
            w, v = self.W[i][k], int(self.B[i])
            if abs(w) <= self.eps:
                continue
            kd = self.kind[v]
            to_u = max(_fr(self.ub[v]) - _fr(self.x[v]), Fraction(0)) if kd in (UPPER, TWOSIDED, FIXED) else None
            to_l = max(_fr(self.x[v]) - _fr(self.lb[v]), Fraction(0)) if kd in (LOWER, TWOSIDED, FIXED) else None
            cu = (to_u / w) if (w > 0 and to_u is not None) else ((to_l / -w) if (w < 0 and to_l is not None) else None)
            cd = (to_l / -w) if (w > 0 and to_l is not None) else ((to_u / w) if (w < 0 and to_u is not None) else None)
            if cu is not None and cu < up:
                up, bu = cu, v
            if cd is not None and cd > dn:
                dn, bd = cd, v
        return dn, up, bd, bu

    # ---- what a limit means
    def check_cost_limit(self, i, L, blocking, up, margin=Fraction(1, 1 << 20)):
        """a finite limit L (a float, up or down) on the cost of the basic variable at position i: inside it every non-Fixed
        nonbasic reduced cost d_j - delta alpha_ij keeps its sign, outside it the blocking one has lost it.  Positions with
        0 < |alpha| <= 2 eps are left out (exact zeros are checked).  Returns the number of positions left out."""
        L = _fr(L)
        al = self.alpha(i)
        pos = {int(v): j for j, v in enumerate(self.N)}
        jb = pos[int(blocking)]
        ab = al[jb]
        assert self.code(jb) != 3, ("blocking variable is Fixed", i, blocking)
        assert ab != 0, ("the blocking entry is exactly zero", i, blocking)
        # the blocker is eligible on this side
        cb = self.code(jb)
        want_pos = (cb == NB_LOWER) == bool(up) if cb != NB_FREE else None
        if abs(ab) > 2 * self.eps and want_pos is not None:
            assert (ab > 0) == want_pos, ("the blocking entry has the wrong sign", i, blocking, float(ab))
        skipped = 0
        if L == 0:
            return sum(1 for a in al if 0 < abs(a) <= 2 * self.eps)
        inside, outside = L * (1 - margin), L * (1 + margin)
        for j, a in enumerate(al):
            code = self.code(j)
            if code == 3:
                continue
            if 0 < abs(a) <= 2 * self.eps:  # an exact zero is checked: it moves nothing
                skipped += 1
                continue
            nu, nd = self.numerators(j, a)
            num = nu if up else nd
            if code == NB_FREE:
                continue  # a Free nonbasic pins the limit at 0 (d_v = 0 at an optimum): L == 0 above
            val = num - inside * a
            assert (val >= 0) if code == NB_LOWER else (val <= 0), ("sign lost inside the limit", i, j, float(val), float(L))
        nu, nd = self.numerators(jb, ab)
        val = (nu if up else nd) - outside * ab
        if abs(ab) > 2 * self.eps and cb != NB_FREE:
            assert (val < 0) if cb == NB_LOWER else (val > 0), ("the blocker keeps its sign outside the limit", i, blocking, float(val))
        return skipped

    def check_rhs_limit(self, k, L, blocking, up, margin=Fraction(1, 1 << 20)):
        """the same for right-hand side k: x_B + delta W[:, k] stays within the bounds inside the limit, the blocking basic
        variable has left its bound outside.  Returns the number of rows left out (0 < |w| <= 2 eps)."""
        L = _fr(L)
        ib = [i for i in range(self.m) if int(self.B[i]) == int(blocking)][0]
        skipped = 0
        inside, outside = L * (1 - margin), L * (1 + margin)

        def slack(i, delta):
            """(distance to the upper bound, distance to the lower bound) after the change, bounds clamped as the definition
            clamps them; None: no such bound"""
            v, w = int(self.B[i]), self.W[i][k]
            kd = self.kind[v]
            su = max(_fr(self.ub[v]) - _fr(self.x[v]), Fraction(0)) - delta * w if kd in (UPPER, TWOSIDED, FIXED) else None
            sl = max(_fr(self.x[v]) - _fr(self.lb[v]), Fraction(0)) + delta * w if kd in (LOWER, TWOSIDED, FIXED) else None
            return su, sl

        for i in range(self.m):
            if 0 < abs(self.W[i][k]) <= 2 * self.eps:  # an exact zero is checked: it moves nothing
                skipped += 1
                continue
            if L == 0:
                continue
            su, sl = slack(i, inside)
            assert (su is None or su >= 0) and (sl is None or sl >= 0), ("a bound lost inside the limit", k, i, float(L))
        wb = self.W[ib][k]
        assert wb != 0, ("the blocking entry is exactly zero", k, blocking)
        if abs(wb) > 2 * self.eps:
            toward_upper = (wb > 0) == bool(up)
            su, sl = slack(ib, outside)
            s = su if toward_upper else sl
            assert s is not None, ("the blocker has no bound on this side", k, blocking)
            assert L == 0 or s < 0, ("the blocker keeps its bound outside the limit", k, blocking, float(L))
        return skipped

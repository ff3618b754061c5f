"""Models of the postsolve (ellp_amd/csrc/engine/ellp_post.inc) for the tests.

EXACT MODEL.  r = b - A x, d = c - A^T y, omega, the objectives and the report's maxima in rational arithmetic on the f64
inputs, by the definitions of include/ellp_hip.h.  Every f64 is a dyadic rational, so a sum of products is accumulated as
one Python integer over the common denominator 2^SHIFT and turned into a fractions.Fraction at the end: the same value
Fraction arithmetic term by term gives, much faster.  Zero entries are skipped (they contribute exactly nothing).

BOUND on an entry of d or r:  |got - exact| <= u |exact| + gamma_K^2 S,  u = 2^-53, S the sum of the absolute values of the
terms (|c_v| + sum_i |a_iv| |y_i|, resp. |b_i| + sum_v |x_v| |a_iv|), gamma_K = K u / (1 - K u): the Dot2 bound of Ogita,
Rump and Oishi (Accurate sum and dot product, SIAM J. Sci. Comput. 26 (2005), Prop. 5.5) for a compensated dot product whose
longest chain has K compensated operations, with one rounding of the result.  K from the kernel's geometry
(k_post_pass: row tiles of 512 rows, a lane owns 8 rows of a tile; column blocks of cpb columns, 4 waves a block, cpb = 64
doubled until a pass has at most 1,024 blocks):
    d_v:  8 products in the lane + 6 butterfly steps over the wave + ceil(m / 512) row tiles + the cost  c_v
          K_d = 8 + 6 + ceil(m / 512) + 1
    r_i:  cpb / 4 columns of a wave + 3 merges of the 4 waves + every column block of A_B and of A_N + b_i
          K_r = max(cpb_B, cpb_N) / 4 + 3 + blocks(m) + blocks(n_N) + 1
The bound is used as stated, with no slack factor.

FLOAT MODEL of steps 2 to 4: y = B^-T c_B by numpy's LU (LAPACK getrf/getrs), then refinement with EXACT residuals rounded
once — rho = fl(c_B - A_B^T y), delta = B^-T rho, y += delta — while omega > 2u, fewer than 4 steps were taken and the last
step at least halved omega.  After the solve and after every step the components a singleton basic column a e_k fixes on
its own are set to y_k = fl(c / a), as k_post_snap does: where such a component is 0 in exact arithmetic, a computed 1e-17
is a componentwise backward error of 1 that no refinement step removes.  It shows what the algorithm reaches when the residual is as good as the compensated pass makes
it: omega <= 2u (rounding y to f64 alone accounts for u).
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
SHIFT = 2300  # 2 * 1074 + head-room: every product of two f64 is an integer over 2^SHIFT


def _int(v):
    """f64 -> (integer numerator, log2 of the denominator)"""
    n, d = float(v).as_integer_ratio()
    return n, d.bit_length() - 1


def exact_dot(a, b, absolute=False):
    """sum_k a_k b_k (or of |a_k| |b_k|) as a Fraction; a, b: sequences of f64"""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    tot = 0
    for k in np.nonzero((a != 0.0) & (b != 0.0))[0]:
        na, ea = _int(a[k])
        nb, eb = _int(b[k])
        t = (na * nb) << (SHIFT - ea - eb)
        tot += abs(t) if absolute else t
    return Fraction(tot, 1 << SHIFT)


def post_cpb(ncols):
    cpb = 64
    while (ncols + cpb - 1) // cpb > 1024:
        cpb *= 2
    return cpb


def post_blocks(ncols):
    return (ncols + post_cpb(ncols) - 1) // post_cpb(ncols) if ncols > 0 else 0


def chain_lengths(m, nN):
    """(K_d, K_r): the longest chains of compensated operations of the pass (module docstring)"""
    kd = 8 + 6 + (m + 511) // 512 + 1
    kr = max(post_cpb(m), post_cpb(max(nN, 1))) // 4 + 3 + post_blocks(m) + post_blocks(nN) + 1
    return kd, kr


def gamma(K):
    return K * U / (1.0 - K * U)


def entry_bound(exact, S, K):
    """u |exact| + gamma_K^2 S, as a Fraction (no rounding in the bound itself)"""
    g = Fraction(gamma(K))
    return Fraction(U) * abs(exact) + g * g * S


class Exact:
    """The exact quantities of one point.  A: (m, n) array; c, x, kind, lb, ub: n_c entries; B, N, Nb: the index sets;
    y: the duals whose d is wanted (the y a postsolve returned)."""

    def __init__(self, m, n, n_c, A, c, b, kind, lb, ub, x, B, N, Nb, y):
        self.m, self.n, self.n_c = int(m), int(n), int(n_c)
        self.A = np.asarray(A, dtype=np.float64).reshape(self.n, self.m).T if np.ndim(A) == 1 else np.asarray(A, dtype=np.float64)
        self.c, self.b, self.x, self.y = (np.asarray(v, dtype=np.float64) for v in (c, b, x, y))
        self.kind, self.lb, self.ub = np.asarray(kind), np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
        self.B, self.N, self.Nb = np.asarray(B, dtype=np.int64), np.asarray(N, dtype=np.int64), np.asarray(Nb)
        self.nN = len(self.N)

    @classmethod
    def of(cls, fp, y):
        return cls(fp.m, fp.n, fp.n_c, fp.A, fp.c, fp.b, fp.kind, fp.lb, fp.ub, fp.x, fp.B, fp.N[:fp.nN], fp.Nb[:fp.nN], y)

    def d(self, v):
        """(d_v, S_v) exactly"""
        cv = Fraction(float(self.c[v]))
        if v >= self.n:
            return cv, abs(cv)
        return cv - exact_dot(self.A[:, v], self.y), abs(cv) + exact_dot(self.A[:, v], self.y, absolute=True)

    def r(self, i):
        """(r_i, S_i) exactly"""
        bi = Fraction(float(self.b[i]))
        return bi - exact_dot(self.A[i, :], self.x[:self.n]), abs(bi) + exact_dot(self.A[i, :], self.x[:self.n], absolute=True)

    def omega(self):
        """max_i |rho_i| / (|c_B| + |A_B|^T |y|)_i over the basic positions (0 / 0 = 0)"""
        w = Fraction(0)
        for v in self.B:
            rho, S = self.d(int(v))
            if rho != 0:
                w = max(w, abs(rho) / S)
        return w

    def primal_obj(self):
        return exact_dot(self.c, self.x)

    def dual_obj(self, d):
        """b . y + the bound terms (standard_form.rs:52-68) for a given f64 d by variable"""
        coef = np.zeros(self.n_c)
        for v in range(self.n_c):
            k = int(self.kind[v])
            if k in (1, 4):
                coef[v] = self.lb[v]
            elif k == 2:
                coef[v] = self.ub[v]
            elif k == 3:
                coef[v] = self.lb[v] if d[v] > 0.0 else self.ub[v]
        return exact_dot(self.b, self.y) + exact_dot(coef, d)


def _nanmax_first(values, indices):
    """NaN wins (its first index), else the largest value at its smallest index; (0.0, -1) when the maximum is 0"""
    best, where = 0.0, -1
    order = np.argsort(np.asarray(indices), kind="stable")
    for k in order:
        v, i = float(values[k]), int(indices[k])
        if v != v:
            return v, i
        if v > best:
            best, where = v, i
    return best, where


def _pos(v):
    """max(v, 0) that keeps a NaN and never gives -0.0"""
    return v if v != v else (v if v > 0.0 else 0.0)


def report_from(fp, d, r):
    """The report's maxima by the definitions of include/ellp_hip.h applied in f64 to the RETURNED d and r and the point:
    what k_post_report must give bit for bit (max, abs and one subtraction are exact or correctly rounded on both sides)."""
    x, kind, lb, ub = fp.x, fp.kind, fp.lb, fp.ub
    out = {}
    out["primal_residual"], out["worst_row"] = _nanmax_first(np.abs(r), np.arange(fp.m))
    viol = np.zeros(fp.n_c)
    for v in range(fp.n_c):
        k = int(kind[v])
        if k == 1:
            viol[v] = _pos(lb[v] - x[v])
        elif k == 2:
            viol[v] = _pos(x[v] - ub[v])
        elif k == 3:
            viol[v] = _pos(max(lb[v] - x[v], x[v] - ub[v])) if x[v] == x[v] else np.nan
        elif k == 4:
            viol[v] = abs(x[v] - lb[v])
        else:
            viol[v] = x[v] if x[v] != x[v] else 0.0
    out["bound_violation"], out["worst_bound_var"] = _nanmax_first(viol, np.arange(fp.n_c))
    N, Nb = fp.N[:fp.nN], fp.Nb[:fp.nN]
    inf = np.zeros(fp.nN)
    for j in range(fp.nN):
        dv = d[N[j]]
        if int(kind[N[j]]) == 4:
            inf[j] = dv if dv != dv else 0.0
        elif Nb[j] == 0:
            inf[j] = _pos(-dv)
        elif Nb[j] == 1:
            inf[j] = _pos(dv)
        else:
            inf[j] = abs(dv)
    out["dual_infeasibility"], out["worst_dual_var"] = _nanmax_first(inf, N)
    out["basic_reduced_cost"], _ = _nanmax_first(np.abs(d[fp.B]), np.arange(fp.m))
    return out


def float_model(A_B, c_B):
    """Steps 2 to 4 in f64 with exact residuals: returns (y, omega as a float, refinement steps).  A_B: (m, m) array."""
    A_B = np.asarray(A_B, dtype=np.float64)
    c_B = np.asarray(c_B, dtype=np.float64)
    m = A_B.shape[0]

    def residual(y):
        rho = np.zeros(m)
        w = Fraction(0)
        for i in range(m):
            ex = Fraction(float(c_B[i])) - exact_dot(A_B[:, i], y)
            S = abs(Fraction(float(c_B[i]))) + exact_dot(A_B[:, i], y, absolute=True)
            rho[i] = float(ex)
            if ex != 0:
                w = max(w, abs(ex) / S)
        return rho, float(w)

    def snap(y):
        for j in range(m):
            nz = np.nonzero(A_B[:, j])[0]
            if len(nz) == 1:
                y[nz[0]] = c_B[j] / A_B[nz[0], j]
        return y

    y = snap(np.linalg.solve(A_B.T, c_B))
    steps, last = 0, 0.0
    while True:
        rho, w = residual(y)
        if not (w > 2 * U) or steps >= 4 or (steps > 0 and not (w <= 0.5 * last)):
            return y, w, steps
        y = snap(y + np.linalg.solve(A_B.T, rho))
        last = w
        steps += 1

"""An LP family with a dense, closed-form basis and a wide model of the two explicit-inverse loops, for the sizes (2,049 to
8,192 rows) where neither CPU oracle is affordable: the LU-per-iteration loop is too slow, and the explicit-inverse loop
inverts the start basis in O(m^3).

The family (make_case).  The start basis is A_B = (I - 2 v v^T) D with v a dense unit vector and D a diagonal in [1/2, 2]:
a Householder reflection times a scaling, so every row and column of A_B and of B^-1 = D^-1 (I - 2 v v^T) is dense, the
condition is <= 4, and the inverse needs no factorisation.  (A_B is stored rounded to f64; the closed form is the inverse of
the unrounded matrix, off by a few units of 2^-53 in norm: three orders below the smallest tolerance used with it.)  The
nonbasic columns are dense uniform(-1, 1), except eight with a single nonzero (rows 0 and m - 1 among them) for the
unit-column table.  The basic variables sit at random positions of the variable range, so B and N interleave.  Bound kinds
are mixed over basic and nonbasic variables.  Primal cases: x_B strictly inside its bounds, b = A x, and c chosen so that the
reduced costs are what the case asks for: `attractive` columns with the sign their label makes attractive, the rest with the
other sign (a free nonbasic column is always attractive: its reduced cost cannot be made an exact zero).  Dual cases: y
random, c = A^T y + d with d of the sign each label requires (0 for the free nonbasic column), and `outside` basic variables
outside their bounds.  The arrays are FlatProblem-shaped; ellp_amd/synth.py (whose draw order is pinned) is not involved.

The model (Model).  The reference's pivot rules as ellp_rules.inc and oracle/ellp_oracle.c (eo_primal_binv_… /
eo_dual_binv_…) state them — primal: Dantzig's choice through the reference's fold, the bounded ratio test with its
lowest-index tie rule and quirk Q1; dual: the first violated row, the ratio test whose first minimum wins — on a B^-1 kept in
PRODUCT FORM: the closed-form W0 and one eta vector per pivot.  FTRAN and BTRAN of a vector cost O(k m), pricing O(m n_N),
a row of B^-1 O(m + k^2); nothing m x m is formed.  It runs in np.longdouble or, with dtype=np.float64, in plain doubles: the
GPU tests derive their tolerances from the distance between the two runs (tolerance()).  It predicts pivots, it follows
nobody: the engine is compared with it, never fed into it.

Every decision is logged with its separation from the runner-up (Model.decisions), and every quantity a rule compares with
eps or with zero is kept if it is not an exact zero (Model.compared_min_outside): the CPU tests demand separation >= SEP_MIN
and nothing in [NEAR_LO, NEAR_HI] for every committed case, so the GPU tests may demand identical pivots without any
allowance for ties.  If a seed fails that, the seed is changed here, not the threshold."""
import numpy as np

L = np.longdouble
EPS = 1e-10          # ellp_opts.eps' default, src/util.rs:1
MARGIN = 64          # the one factor of every tolerance of tests/test_gpu_large_pivots.py; may never exceed 1,024
SEP_MIN = 1e-6       # relative separation of every decision from its runner-up
NEAR_LO, NEAR_HI = 1e-13, 1e-7  # no compared quantity may lie in here (eps = 1e-10 sits in the middle, the pivot guard 1e-7 at the top)

FREE, LOWER, UPPER, TWOSIDED, FIXED = 0, 1, 2, 3, 4
NB_LOWER, NB_UPPER, NB_FREE = 0, 1, 2
OPTIMAL, INFEASIBLE, UNBOUNDED, MAXITER = 0, 1, 2, 3
PRIMAL, DUAL = 0, 1

# name -> (kind, m, n_N, seed, attractive / outside, scale, window, fixed basic variables).  scale, primal: the factor on the reduced costs of the
# columns that are not attractive (large: few of them turn attractive later, the solve ends); dual: the factor on the
# distance of the outside variables from their bounds (small: a pivot pushes few others out, the solve ends).  The seeds are
# those at which test_large_model_cpu.py's separation conditions hold over the whole window and, for the two cases that run
# to the end, at which that end is a vertex within its bounds (the reference's quirks can leave a two-sided variable nonbasic
# off its bound; an end like that satisfies no KKT check).
CASES = {
    "p2049": (PRIMAL, 2049, 272, 3, 60, 1.0, 40, 0),
    "p3120": (PRIMAL, 3120, 272, 6, 60, 1.0, 40, 0),
    "p4096": (PRIMAL, 4096, 272, 3, 60, 1.0, 40, 0),
    "p4097": (PRIMAL, 4097, 272, 4, 60, 1.0, 40, 0),
    "p4097w": (PRIMAL, 4097, 4200, 1, 60, 1.0, 24, 0),
    "p8192": (PRIMAL, 8192, 272, 2, 60, 1.0, 12, 0),
    "p4097end": (PRIMAL, 4097, 272, 17, 12, 8.0, 80, 0),
    "d2049": (DUAL, 2049, 272, 2, 60, 1.0, 40, 3),
    "d3120": (DUAL, 3120, 272, 1, 60, 1.0, 40, 3),
    "d4096": (DUAL, 4096, 272, 1, 60, 1.0, 40, 3),
    "d4097": (DUAL, 4097, 272, 1, 60, 1.0, 40, 3),
    "d8192": (DUAL, 8192, 272, 2, 60, 1.0, 12, 3),
    "d4096end": (DUAL, 4096, 272, 2, 10, 0.02, 80, 0),
}
_CHUNK = 256


class Case:
    """FlatProblem-shaped arrays of one LP of the family, and the closed form of its start basis (v, D)"""

    def flat(self, E):
        dual = self.kind_of == DUAL
        return E.FlatProblem(self.m, self.n, self.n, self.A.reshape(-1, order="F"), self.c, self.b, self.kind, self.lb, self.ub,
                             self.x, self.B, self.N, self.Nb, self.y if dual else None, self.d if dual else None)

    def view(self):
        """a copy shaped like oracle.ellp_oracle.Phase, for the eo_*_solve_with_initial calls"""
        class V:
            pass
        o = V()
        o.m, o.n, o.n_c, o.nB, o.nN = self.m, self.n, self.n, self.m, self.nN
        o.A = np.ascontiguousarray(self.A.reshape(-1, order="F"))
        for k in ("c", "b", "kind", "lb", "ub", "x", "B", "N", "Nb"):
            setattr(o, k, getattr(self, k).copy())
        o.y = self.y.copy() if self.kind_of == DUAL else None
        o.d = self.d.copy() if self.kind_of == DUAL else None
        return o


def _matvec_T(A, cols, y):
    """A[:, cols]^T y in long double, a chunk of columns at a time"""
    out = np.zeros(len(cols), dtype=L)
    for j0 in range(0, len(cols), _CHUNK):
        out[j0:j0 + _CHUNK] = A[:, cols[j0:j0 + _CHUNK]].astype(L).T @ y
    return out


def make_case(kind_of, m, nN, seed, count, scale=1.0, quirks=False, fixed_basics=3):
    """One LP of the family.  count: the attractive nonbasic columns (primal) or the basic variables outside their bounds
    (dual).  quirks (primal; for the comparison with the oracle at small size, where no separation is asked for): fixed and
    two-sided basic variables and wide two-sided nonbasic ones too, so that the exact-zero ties of the ratio test occur.
    fixed_basics (dual, and primal with quirks): how many basic variables are fixed.  The dual rule never looks at a fixed
    basic variable, so its x drifts off its bound: a dual case meant to end at a true optimum has none, and no fixed
    nonbasic variable that could enter either (fixed_basics = 0)."""
    assert m >= 16 and nN >= 32
    rng = np.random.default_rng([int(seed), int(m), int(nN), int(kind_of)])
    n = m + nN
    perm = rng.permutation(n)
    B, N = perm[:m].astype(np.int64), perm[m:].astype(np.int64)
    v = rng.normal(size=m).astype(L)
    v /= np.sqrt(v @ v)
    D = rng.uniform(0.5, 2.0, size=m)
    A = np.empty((m, n), order="F")
    for i0 in range(0, m, _CHUNK):
        i1 = min(m, i0 + _CHUNK)
        cols = -2 * v[:, None] * v[None, i0:i1]
        cols[np.arange(i0, i1), np.arange(i1 - i0)] += 1
        A[:, B[i0:i1]] = (cols * D[i0:i1].astype(L)[None, :]).astype(np.float64)
    A[:, N] = rng.uniform(-1.0, 1.0, size=(nN, m)).T
    upos = rng.choice(nN, size=8, replace=False)
    urow = np.concatenate([[0, m - 1], rng.integers(0, m, size=6)])
    uval = np.concatenate([rng.choice([-1.0, 1.0], size=4), rng.choice([-1.0, 1.0], size=4) * rng.uniform(0.5, 2.0, size=4)])
    for p, i, a in zip(upos, urow, uval):
        A[:, N[p]] = 0.0
        A[i, N[p]] = a

    kind = np.zeros(n, dtype=np.uint8)
    # A two-sided basic variable strictly inside its bounds gives the primal ratio test an exact 0 whenever d_i < 0 (quirk
    # Q1, primal…:359), as a fixed one does whatever the sign, and a fixed entering column starts the test at exactly 0: two
    # of these tie at 0 and the index decides.  So that every decision has a runner-up at a distance, a primal case starts
    # without fixed or two-sided basic variables, and its two-sided nonbasic columns are narrow (they flip, and fixed ones
    # flip too); `quirks` puts them in.  A dual case has two-sided basics and three fixed ones (those never leave).
    plain = kind_of == PRIMAL and not quirks
    kind[B] = rng.choice([FREE, LOWER, UPPER, TWOSIDED], size=m, p=[0.1, 0.45, 0.45, 0.0] if plain else [0.1, 0.3, 0.3, 0.3])
    if not plain and fixed_basics:
        kind[B[rng.choice(m, size=fixed_basics, replace=False)]] = FIXED
    kind[N] = rng.choice([LOWER, UPPER, TWOSIDED, FIXED], size=nN, p=[0.3, 0.3, 0.3, 0.1])
    if kind_of == DUAL and not fixed_basics:
        kind[N[kind[N] == FIXED]] = TWOSIDED
    nfree = 2 if kind_of == PRIMAL else 1
    free_pos = rng.choice(np.setdiff1d(np.arange(nN), upos[:4]), size=nfree, replace=False)
    kind[N[free_pos]] = FREE

    lb, ub, x = np.zeros(n), np.zeros(n), np.zeros(n)
    base = rng.uniform(-1.0, 1.0, size=n)
    width = rng.uniform(0.05, 4.0, size=n)
    if plain:
        width[N] = rng.uniform(0.02, 0.2, size=nN)
    is_l, is_u, is_t, is_x = kind == LOWER, kind == UPPER, kind == TWOSIDED, kind == FIXED
    lb[is_l | is_t | is_x] = base[is_l | is_t | is_x]
    ub[is_u] = base[is_u]
    ub[is_t] = lb[is_t] + width[is_t]
    ub[is_x] = lb[is_x]
    Nb = np.zeros(nN, dtype=np.uint8)
    kN = kind[N]
    Nb[kN == UPPER] = NB_UPPER
    Nb[kN == FREE] = NB_FREE
    both = (kN == TWOSIDED) | (kN == FIXED)
    Nb[both] = rng.choice([NB_LOWER, NB_UPPER], size=int(both.sum()))
    x[N] = np.where(Nb == NB_LOWER, lb[N], np.where(Nb == NB_UPPER, ub[N], 0.0))
    # basic variables strictly inside
    gap = rng.uniform(0.5, 2.0, size=m)
    frac = rng.uniform(0.3, 0.7, size=m)
    kB = kind[B]
    x[B] = np.where(kB == LOWER, lb[B] + gap, np.where(kB == UPPER, ub[B] - gap,
                    np.where(kB == TWOSIDED, lb[B] + frac * (ub[B] - lb[B]), np.where(kB == FIXED, lb[B], base[B]))))
    if kind_of == DUAL:
        bounded = np.flatnonzero((kB == LOWER) | (kB == UPPER) | (kB == TWOSIDED))
        out = rng.choice(bounded, size=count, replace=False)
        for i in out:
            j = B[i]
            below = kB[i] == LOWER or (kB[i] == TWOSIDED and rng.random() < 0.5)
            x[j] = lb[j] - scale * gap[i] if below else ub[j] + scale * gap[i]
    b = np.zeros(m, dtype=L)
    for j0 in range(0, n, _CHUNK):
        b += A[:, j0:j0 + _CHUNK].astype(L) @ x[j0:j0 + _CHUNK].astype(L)

    c = np.zeros(n)
    cs = Case()
    mag = rng.uniform(0.5, 2.0, size=nN)
    if kind_of == PRIMAL:
        c[B] = rng.uniform(-1.0, 1.0, size=m)
        z = c[B].astype(L) / D.astype(L)
        y = z - 2 * v * (v @ z)                       # B^-T c_B = (I - 2 v v^T) D^-1 c_B
        others = np.setdiff1d(np.arange(nN), free_pos)
        att = np.zeros(nN, dtype=bool)
        att[free_pos] = True
        att[rng.choice(others, size=count - nfree, replace=False)] = True
        want_neg = np.where(Nb == NB_LOWER, att, np.where(Nb == NB_UPPER, ~att, rng.random(nN) < 0.5))
        r = np.where(att, mag, scale * mag) * np.where(want_neg, -1.0, 1.0)
        c[N] = (r.astype(L) + _matvec_T(A, N, y)).astype(np.float64)
        cs.y = cs.d = None
    else:
        y = rng.uniform(-1.0, 1.0, size=m)
        d = np.zeros(n)
        d[N] = np.where(Nb == NB_LOWER, mag, np.where(Nb == NB_UPPER, -mag, 0.0))
        c[:] = (_matvec_T(A, np.arange(n), y.astype(L)) + d.astype(L)).astype(np.float64)
        cs.y, cs.d = y, d
    cs.kind_of, cs.m, cs.n, cs.nN = kind_of, m, n, nN
    cs.A, cs.c, cs.b, cs.kind, cs.lb, cs.ub, cs.x, cs.B, cs.N, cs.Nb = A, c, b.astype(np.float64), kind, lb, ub, x, B, N, Nb
    cs.v, cs.D = v, D
    return cs


def case(name):
    kind_of, m, nN, seed, count, scale, _, fixed_basics = CASES[name]
    return make_case(kind_of, m, nN, seed, count, scale, fixed_basics=fixed_basics)


def _rel(a, b):
    """|a - b| relative to the larger of the two (1 where one of them is infinite or both are zero)"""
    a, b = float(a), float(b)
    if not (np.isfinite(a) and np.isfinite(b)):
        return 1.0
    s = max(abs(a), abs(b))
    return abs(a - b) / s if s > 0 else 0.0


class Model:
    """The explicit-inverse loop of `case` (primal or dual by its kind) in `dtype`, B^-1 in product form.  step() runs one
    loop body; run(k) up to k; status / iters as ellp_engine_run reports them (iters counts loop bodies, the one that finds
    the terminal status included)."""

    def __init__(self, cs, dtype=L, steepest_edge=False, eps=EPS):
        T = self.T = dtype
        self.cs, self.eps, self.se = cs, eps, bool(steepest_edge)
        self.m, self.n, self.nN, self.dual = cs.m, cs.n, cs.nN, cs.kind_of == DUAL
        self.A = cs.A
        self.v, self.Dinv = cs.v.astype(T), (1 / cs.D.astype(L)).astype(T)
        self.c, self.lb, self.ub, self.kind = cs.c.astype(T), cs.lb.astype(T), cs.ub.astype(T), cs.kind
        self.x = cs.x.astype(T)
        self.B, self.N, self.Nb = cs.B.copy(), cs.N.copy(), cs.Nb.copy()
        self.AN = np.asfortranarray(cs.A[:, cs.N].astype(T))
        if self.dual:
            self.y, self.d = cs.y.astype(T), cs.d.astype(T)
        self.etas = []  # (r, alpha, alpha_r): B^-1 = E_k ... E_1 W0, E = I - (alpha - e_r) e_r^T / alpha_r
        self.B_after = [self.B.copy()]  # the basis after k etas
        self.iters, self.status = 0, MAXITER
        self.decisions = []   # (loop body, "enter" / "leave", relative separation from the runner-up)
        self.compared_min_outside = np.inf  # the smallest distance, in decades, of a compared quantity from [NEAR_LO, NEAR_HI]; < 0: inside
        self.near = []        # (loop body, what, value) of every compared quantity inside [NEAR_LO, NEAR_HI]
        self.gamma = None     # steepest edge: the weights the LAST pricing used, by the nonbasic position order it priced
        self.pivots = []      # (loop body, entering position q, leaving row r or -1 for a bound flip)

    # ---- B^-1 in product form
    def ftran(self, Z):
        """B^-1 Z, Z a vector or a matrix of columns"""
        Z = np.array(Z, dtype=self.T)
        one = Z.ndim == 1
        if one:
            Z = Z[:, None]
        Z = (Z - 2 * self.v[:, None] * (self.v @ Z)[None, :]) * self.Dinv[:, None]
        for r, al, ar in self.etas:
            zr = Z[r, :] / ar
            Z -= al[:, None] * zr[None, :]
            Z[r, :] = zr
        return Z[:, 0] if one else Z

    def btran(self, p):
        """p^T B^-1 of a vector p"""
        p = np.array(p, dtype=self.T)
        for r, al, ar in reversed(self.etas):
            p[r] = (p[r] - (p @ al - p[r] * ar)) / ar
        z = p * self.Dinv
        return z - 2 * (z @ self.v) * self.v

    def rows(self, idx, upto=None):
        """rows idx of B^-1 (upto: as it was after that many etas; B_after[upto] is its basis), len(idx) x m.
        e_i^T E_k ... E_1 differs from e_i^T only at the pivot rows, so the etas cost O(k^2) per row and the closed-form W0
        O(m)."""
        T = self.T
        idx = np.asarray(idx, dtype=np.int64)
        etas = self.etas if upto is None else self.etas[:upto]
        R = np.array(sorted({r for r, _, _ in etas}), dtype=np.int64)
        col = {int(r): k for k, r in enumerate(R)}
        own = np.ones(len(idx), dtype=T)               # coefficient at column idx[i], where that is no pivot row
        own_live = ~np.isin(idx, R)
        Q = np.zeros((len(idx), len(R)), dtype=T)      # coefficients at the pivot rows
        for i in np.flatnonzero(~own_live):
            Q[i, col[int(idx[i])]] = 1
        for r, al, ar in reversed(etas):
            k = col[int(r)]
            s = Q @ al[R] + np.where(own_live, own * al[idx], 0)  # p . alpha
            Q[:, k] = (Q[:, k] - (s - Q[:, k] * ar)) / ar
        out = np.empty((len(idx), self.m), dtype=T)
        for i0 in range(0, len(idx), _CHUNK):
            sl = slice(i0, min(len(idx), i0 + _CHUNK))
            P = np.zeros((sl.stop - sl.start, self.m), dtype=T)
            if len(R):
                P[:, R] = Q[sl]
            live = np.flatnonzero(own_live[sl])
            P[live, idx[sl][live]] = own[sl][live]
            P *= self.Dinv[None, :]
            s = P[:, R] @ self.v[R] if len(R) else np.zeros(P.shape[0], dtype=T)
            s[live] += P[live, idx[sl][live]] * self.v[idx[sl][live]]
            out[sl] = P - 2 * s[:, None] * self.v[None, :]
        return out

    def row(self, i, upto=None):
        return self.rows([i], upto)[0]

    def gamma_now(self):
        """gamma_j = 1 + |B^-1 a_j|^2 by nonbasic position, from the definition"""
        Z = self.ftran(self.AN)
        return 1 + (Z * Z).sum(axis=0)

    # ---- bookkeeping of what the rules compare
    def _compared(self, what, vals):
        a = np.abs(np.asarray(vals, dtype=np.float64)).ravel()
        a = a[(a > 0) & np.isfinite(a)]
        if not a.size:
            return
        lg = np.log10(a)
        dist = np.where(lg < np.log10(NEAR_LO), np.log10(NEAR_LO) - lg, np.where(lg > np.log10(NEAR_HI), lg - np.log10(NEAR_HI), -1.0))
        self.compared_min_outside = min(self.compared_min_outside, float(dist.min()))
        for val in a[dist < 0][:4]:
            self.near.append((self.iters, what, float(val)))

    def _swap(self, q, r, side):
        t = self.B[r]
        self.B[r] = self.N[q]
        self.N[q] = t
        self.AN[:, q] = self.A[:, t].astype(self.T)
        self.Nb[q] = side
        self.B_after.append(self.B.copy())

    def run(self, k):
        for _ in range(int(k)):
            if self.status != MAXITER:
                break
            self.step()
        return self.status

    def step(self):
        assert self.status == MAXITER
        self.iters += 1
        self.status = self._dual_body() if self.dual else self._primal_body()
        return self.status

    # ---- eo_primal_binv_solve_with_initial's loop body
    def _primal_body(self):
        T, eps, B, N, Nb = self.T, self.eps, self.B, self.N, self.Nb
        u = self.btran(self.c[B])
        r = self.c[N] - self.AN.T @ u
        assert not np.isnan(r).any()
        self._compared("r_j", r)
        key = np.full(self.nN, -np.inf, dtype=T)
        big = ~(np.abs(r) < eps)
        pos = r > 0
        key = np.where(big & pos & (Nb == NB_UPPER), r, key)
        key = np.where(big & ~pos & (Nb == NB_LOWER), -r, key)
        key = np.where(big & (Nb == NB_FREE), np.abs(r), key)
        if self.se:
            self.gamma = self.gamma_now()
            key = np.where(np.isfinite(key), np.abs(r) / np.sqrt(self.gamma), key)
        cand = np.flatnonzero(np.isfinite(key))
        if not cand.size:
            return OPTIMAL
        q, r1 = int(cand[0]), key[cand[0]]
        for j in cand[1:]:      # the sequential max_by fold (primal…:271-287)
            kj = key[j]
            acc_greater = (r1 > kj) if abs(r1 - kj) >= eps else (N[q] > N[j])
            if not acc_greater:
                q, r1 = int(j), kj
        rest = np.delete(key[cand], np.flatnonzero(cand == q))
        if rest.size:
            self.decisions.append((self.iters, "enter", _rel(r1, rest.max())))
            self._compared("key difference", r1 - rest.max())
        jq = int(N[q])
        at_lower = Nb[q] == NB_LOWER
        d = self.ftran(self.AN[:, q]) * (-1 if at_lower else 1)
        self._compared("d_i", d)
        kq = self.kind[jq]
        lam = (self.ub[jq] - self.lb[jq]) if kq == TWOSIDED else (T(0) if kq == FIXED else T(np.inf))
        lam0 = lam
        xB, lbB, ubB, kB = self.x[B], self.lb[B], self.ub[B], self.kind[B]
        live = ~(np.abs(d) < eps)
        has_l = (kB == LOWER) | (kB == TWOSIDED)
        has_u = (kB == UPPER) | (kB == TWOSIDED)
        self._compared("x_i - lb_i", (xB - lbB)[has_l])
        self._compared("ub_i - x_i", (ubB - xB)[has_u])
        li = np.full(self.m, np.inf, dtype=T)
        with np.errstate(divide="ignore", invalid="ignore"):
            up = np.where(xB < ubB, (ubB - xB) / d, 0)
            dn_l = np.where(xB > lbB, (lbB - xB) / d, 0)
            dn_t = np.where(xB < lbB, (lbB - xB) / d, 0)  # quirk Q1 (primal…:359)
        li = np.where((kB == LOWER) & (d < 0), dn_l, li)
        li = np.where((kB == UPPER) & (d > 0), up, li)
        li = np.where((kB == TWOSIDED) & (d > 0), up, li)
        li = np.where((kB == TWOSIDED) & ~(d > 0), dn_t, li)
        li = np.where(kB == FIXED, 0, li)
        li = np.where(live, li, np.inf)
        new_basic, side, have_nbi, nbi = -1, NB_LOWER, False, 0
        for i in np.flatnonzero(np.isfinite(li)):   # primal…:320-400
            if li[i] < lam - eps:
                lam, new_basic, side = li[i], int(i), (NB_UPPER if d[i] > 0 else NB_LOWER)
            elif abs(li[i] - lam) < eps:
                if not have_nbi or B[i] < nbi:
                    have_nbi, nbi = True, B[i]
                    lam, new_basic, side = li[i], int(i), (NB_UPPER if d[i] > 0 else NB_LOWER)
        assert lam >= 0
        if np.isinf(lam):
            return UNBOUNDED
        others = np.delete(li, new_basic) if new_basic >= 0 else li
        runner = min(float(others.min()), float(lam0)) if new_basic >= 0 else float(others.min())
        self.decisions.append((self.iters, "leave", _rel(lam, runner)))
        self._compared("lambda difference", float(runner) - float(lam))
        if lam > 0:
            self.x[B] += lam * d
            self.x[jq] += lam if at_lower else -lam
        self.pivots.append((self.iters, q, new_basic))
        if new_basic >= 0:
            al = -d if at_lower else d          # B^-1 a_q itself
            self.etas.append((new_basic, al, al[new_basic]))
            self._swap(q, new_basic, side)
        else:
            assert Nb[q] != NB_FREE, "pivot should have been unbounded"
            Nb[q] = NB_UPPER if Nb[q] == NB_LOWER else NB_LOWER
        return MAXITER

    # ---- eo_dual_binv_solve_with_initial's loop body
    def _dual_body(self):
        T, eps, B, N, Nb = self.T, self.eps, self.B, self.N, self.Nb
        xB, lbB, ubB, kB = self.x[B], self.lb[B], self.ub[B], self.kind[B]
        has_l = (kB == LOWER) | (kB == TWOSIDED)
        has_u = (kB == UPPER) | (kB == TWOSIDED)
        self._compared("x_i - lb_i", (xB - lbB)[has_l])
        self._compared("x_i - ub_i", (xB - ubB)[has_u])
        low = has_l & (xB < lbB - eps)
        high = has_u & (xB > ubB + eps)
        viol = np.flatnonzero(low | high)        # dual…:200-236: the first violated position
        if not viol.size:
            return OPTIMAL
        r = int(viol[0])
        if high[r]:                              # TwoSided: the upper bound is looked at first
            delta, side = xB[r] - ubB[r], NB_UPPER
        else:
            delta, side = xB[r] - lbB[r], NB_LOWER
        rho = self.btran(np.eye(1, self.m, r, dtype=T)[0])
        dot = self.AN.T @ rho
        alpha = -dot if delta < 0 else dot
        self._compared("alpha_j", alpha[Nb != NB_FREE])
        keep = np.where(Nb == NB_LOWER, alpha > eps, np.where(Nb == NB_UPPER, alpha < -eps, True))
        cand = np.flatnonzero(keep)
        if not cand.size:
            return INFEASIBLE
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = self.d[N[cand]] / alpha[cand]
        assert not np.isnan(ratio).any()
        q, theta = int(cand[0]), ratio[0]
        for j, rt in zip(cand[1:], ratio[1:]):   # dual…:263-279: the first minimum wins
            if theta > rt:
                q, theta = int(j), rt
        rest = np.delete(ratio, np.flatnonzero(cand == q))
        if rest.size:
            self.decisions.append((self.iters, "enter", _rel(theta, rest.min())))
            self._compared("ratio difference", float(rest.min()) - float(theta))
        if delta < 0:
            alpha, theta = -alpha, -theta
        lv, ev = int(B[r]), int(N[q])
        aq = self.ftran(self.AN[:, q])
        self._compared("pivot", aq[r])
        assert aq[r] != 0
        self.d[lv] = -theta
        self.d[N] -= theta * alpha
        self.d[ev] = 0
        self.y += theta * rho
        tp = delta / aq[r]
        self.x[B] -= tp * aq
        self.x[ev] += tp
        self.pivots.append((self.iters, q, r))
        self.etas.append((r, aq, aq[r]))
        self._swap(q, r, side)
        return MAXITER


def tolerance(ref, low, m, margin=MARGIN):
    """The tolerance of one compared quantity: margin x max(|f64 model - long-double model|, m 2^-52 (1 + max|.|)), from
    the reference in two precisions and never from the engine."""
    assert margin <= 1024
    ref = np.asarray(ref, dtype=L)
    diff = float(np.abs(ref - np.asarray(low).astype(L)).max()) if ref.size else 0.0
    scale = 1.0 + (float(np.abs(ref).max()) if ref.size else 0.0)
    return margin * max(diff, m * 2.0 ** -52 * scale)

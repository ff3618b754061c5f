"""A model of the rebuild of B^-1 from A_B (ellp_amd/csrc/engine/ellp_rebuild.inc, and the column-by-column form in
ellp_engine.hip), stated plainly:

    Gauss-Jordan on W = I, the basic columns in their order.  Step k: alpha = W a_k; p = the FIRST maximum of
    |alpha_i| over the rows not used yet; the guard (a pivot that is not finite, is zero, or is below eps is refused);
    the eta update with row p.  At the end the rows are permuted so that row k belongs to basic position k.

`eliminate` is that, column by column.  `blocked_replay` does the same pivots in the order of the blocked kernels:
C = W A_B[:, K] for a macro panel K of 64 columns, sub-panels of 16 / 8 / 4 columns factored to V_s = T_s[:, P_s] - I[:, P_s],
M <- M + V_s M[P_s, :] on the rest of the panel and on the accumulated V (two ping-pong buffers), and one rank-64 update
W <- W + V_acc W[P, :].

The exact family.  exact_basis() makes matrices B = P L Q on which both forms work in exact arithmetic: L is lower
triangular with a diagonal from {+-2, +-4, 8} and, in L[m/2:, :m/2] only, entries from {-1, 0, 1} at 15 % density plus a
few ties L[i, k] = +-L[k, k].  Every pivot is then a power of two and every number formed is a small dyadic rational, so
the inverse has the closed form [[D1^-1, 0], [-D2^-1 F D1^-1, D2^-1]] under the permutations.  That is PROVED per
matrix, not assumed: with prove=True both functions assert

    every stored value (W, C, V, V_s, the eta columns) is a multiple of 2^-KS, and
    every sum the kernels form - sum |x_t| |y_t| over the terms of a dot product, |f| |row p| + |w| for an eta update -
    stays below 2^(53 - 2 KS),

KS = 20.  A product of two stored values is a multiple of 2^-2KS, so is every partial sum of such products in any order,
and below 2^(53 - 2KS) in magnitude every multiple of 2^-2KS is an f64 number: no addition, fused or not, in any order,
rounds.  (Division is by a power of two.)  The device's B^-1 then has to equal the model's as numbers, entry for entry, and
its pivot rows the model's.  A matrix that fails the proof raises NotExact: it is rejected on the host."""
import functools
from types import SimpleNamespace

import numpy as np

KS = 20
NB = 64                        # macro panel (BL_NB)
SUM_CAP = 2.0 ** (53 - 2 * KS)
NTIES_MAX = 13


class NotExact(AssertionError):
    pass


class Singular(Exception):
    def __init__(self, k, p, v):
        super().__init__(f"column {k}: pivot {v!r} in row {p} refused")
        self.k, self.p, self.v = k, p, v


def _stored(x, what):
    s = np.asarray(x) * 2.0 ** KS
    if not (np.all(np.isfinite(s)) and np.array_equal(s, np.rint(s))):
        raise NotExact(f"{what}: not a multiple of 2^-{KS}")


def _sum_ok(abs_sum, what):
    if not np.all(np.asarray(abs_sum) < SUM_CAP):
        raise NotExact(f"{what}: a sum of absolute terms reaches {float(np.max(abs_sum))!r} >= 2^{53 - 2 * KS}")


def _pick(col, used, first=True):
    """(p, v, rows holding the maximum): the first maximum of |col| over the unused rows.  A NaN is never a candidate
    (v > best is false for it); p = -1 if no row is left"""
    a = np.abs(col)
    a = np.where(used | np.isnan(a), -1.0, a)
    v = a.max()
    if v < 0:
        return -1, v, np.zeros(0, dtype=np.int64)
    rows = np.flatnonzero(a == v)
    return int(rows[0] if first else rows[-1]), float(v), rows


def _guard(k, p, v, eps):
    if p < 0 or not np.isfinite(v) or v == 0.0 or v < eps:
        raise Singular(k, p, v)


def eliminate(B, eps=0.0, prove=False):
    """The operation, column by column, in f64.  Returns W (rows permuted: row k belongs to basic position k), perm and
    ties = {k: rows that held the maximum of step k} for the steps where more than one did.  Raises Singular."""
    B = np.ascontiguousarray(B, dtype=np.float64)
    m = B.shape[0]
    W = np.eye(m)
    used = np.zeros(m, dtype=bool)
    perm = np.zeros(m, dtype=np.int64)
    ties = {}
    for k in range(m):
        a = B[:, k]
        nz = np.flatnonzero(a != 0.0)  # NaN counts
        alpha = W[:, nz] @ a[nz]
        if prove:
            _sum_ok(np.abs(W[:, nz]) @ np.abs(a[nz]), f"alpha of column {k}")
            _stored(alpha, f"alpha of column {k}")
        p, v, rows = _pick(alpha, used)
        _guard(k, p, v, eps)
        if len(rows) > 1:
            ties[k] = rows
        if prove and np.frexp(v)[0] != 0.5:
            raise NotExact(f"pivot {v!r} of column {k} is no power of two")
        inv = 1.0 / alpha[p]
        f = -(alpha * inv)
        f[p] = 0.0
        rowp = W[p].copy()
        t = np.flatnonzero(f != 0.0)
        if prove:
            _stored(f, f"eta column {k}")
            _sum_ok(np.abs(f[t])[:, None] * np.abs(rowp)[None, :] + np.abs(W[t]), f"eta update {k}")
        W[t] += f[t][:, None] * rowp[None, :]
        W[p] = rowp * inv
        if prove:
            _stored(W[t], f"W after column {k}")
            _stored(W[p], f"pivot row after column {k}")
        used[p] = True
        perm[k] = p
    return W[perm], perm, ties


def blocked_replay(B, eps=0.0, nbw_max=16, prove=False, bug=None):
    """The same elimination in the order of the blocked kernels (see the module's docstring).  Returns W, perm.
    bug (for the tests of the tests): "tie" takes the LAST maximum; "minus1" leaves out the -1 of V_s on the first pivot
    row of the second sub-panel; "pingpong" lets the rank-64 update read the accumulated V from the wrong buffer."""
    B = np.ascontiguousarray(B, dtype=np.float64)
    m = B.shape[0]
    W = np.eye(m)
    used = np.zeros(m, dtype=bool)
    perm = np.zeros(m, dtype=np.int64)
    Cb = [np.zeros((m, NB)), np.zeros((m, NB))]   # the device's buffers live across macro panels; so do these
    Vb = [np.zeros((m, NB)), np.zeros((m, NB))]
    nsub = 0
    for k0 in range(0, m, NB):
        nbc = min(NB, m - k0)
        sel = 0
        Cb[sel][:, :nbc] = W @ B[:, k0:k0 + nbc]
        Cb[sel][:, nbc:] = 0.0
        Vb[sel][:] = 0.0
        if prove:
            _sum_ok(np.abs(W) @ np.abs(B[:, k0:k0 + nbc]), f"C of panel {k0}")
            _stored(Cb[sel], f"C of panel {k0}")
        Pm = np.zeros(nbc, dtype=np.int64)
        for j0 in range(0, nbc, nbw_max):
            nbw = min(nbw_max, nbc - j0)
            Cin, Vin, Cout, Vout = Cb[sel], Vb[sel], Cb[sel ^ 1], Vb[sel ^ 1]
            # ---- k_bl_factor: nbw pivot steps on the m x nbw tile
            tile = Cin[:, j0:j0 + nbw].copy()
            Ps = np.zeros(nbw, dtype=np.int64)
            for j in range(nbw):
                p, v, _ = _pick(tile[:, j], used, first=(bug != "tie"))
                _guard(k0 + j0 + j, p, v, eps)
                if prove and np.frexp(v)[0] != 0.5:
                    raise NotExact(f"pivot {v!r} of column {k0 + j0 + j} is no power of two")
                prow = tile[p].copy()
                inv = 1.0 / prow[j]
                f = -(tile[:, j] * inv)
                f[p] = inv
                keep = np.ones(m)
                keep[p] = 0.0
                if prove:
                    _stored(f, f"eta column {k0 + j0 + j}")
                    _sum_ok(np.abs(f)[:, None] * np.abs(prow)[None, :] + np.abs(tile) * keep[:, None], f"tile step {k0 + j0 + j}")
                tile = f[:, None] * prow[None, :] + tile * keep[:, None]
                tile[:, j] = f
                if prove:
                    _stored(tile, f"tile after step {k0 + j0 + j}")
                used[p] = True
                Ps[j] = p
            perm[k0 + j0:k0 + j0 + nbw] = Ps
            Pm[j0:j0 + nbw] = Ps
            Vs = tile
            for j in range(nbw):
                if not (bug == "minus1" and nsub == 1 and j == 0):
                    Vs[Ps[j], j] -= 1.0
            nsub += 1
            # ---- k_bl_apply: out of place, input buffer sel, output buffer sel ^ 1
            c_lo = j0 + nbw
            Cout[:, c_lo:nbc] = Cin[:, c_lo:nbc] + Vs @ Cin[Ps, c_lo:nbc]
            Vout[:, :j0] = Vin[:, :j0] + Vs @ Vin[Ps, :j0]
            Vout[:, j0:j0 + nbw] = Vs
            if prove:
                _sum_ok(np.abs(Cin[:, c_lo:nbc]) + np.abs(Vs) @ np.abs(Cin[Ps, c_lo:nbc]), f"apply to C at {k0 + j0}")
                _sum_ok(np.abs(Vin[:, :j0]) + np.abs(Vs) @ np.abs(Vin[Ps, :j0]), f"apply to V at {k0 + j0}")
                _stored(Cout[:, c_lo:nbc], f"C after sub-panel {k0 + j0}")
                _stored(Vout[:, :j0 + nbw], f"V after sub-panel {k0 + j0}")
            sel ^= 1
        # ---- k_bl_gather, k_bl_gemm2
        V = Vb[sel ^ 1 if bug == "pingpong" else sel][:, :nbc]
        Wp = W[Pm].copy()
        if prove:
            _sum_ok(np.abs(W) + np.abs(V) @ np.abs(Wp), f"rank-{nbc} update of panel {k0}")
        W = W + V @ Wp
        if prove:
            _stored(W, f"W after panel {k0}")
    return W[perm], perm


# ------------------------------------------------------------------ the exact family
def _exact_parts(m, seed):
    rng = np.random.default_rng(seed)
    h = m // 2
    d = rng.choice([2.0, -2.0, 4.0, -4.0, 8.0], size=m)
    F = rng.choice([-1.0, 0.0, 1.0], p=[0.075, 0.85, 0.075], size=(m - h, h))
    if h > 0:
        for _ in range(min(3 + m // 100, NTIES_MAX)):  # deliberate ties: L[i, k] = +-L[k, k]
            i, k = int(rng.integers(m - h)), int(rng.integers(h))
            F[i, k] = rng.choice([-1.0, 1.0]) * d[k]
    return d, F, rng.permutation(m), rng.permutation(m)


def _assemble(d, F, rp, cq):
    m = len(d)
    h = m // 2
    L = np.diag(d)
    L[h:, :h] = F
    Li = np.diag(1.0 / d)
    Li[h:, :h] = -((1.0 / d[h:])[:, None] * F * (1.0 / d[:h])[None, :])
    # B[i, j] = L[rp[i], cq[j]]  ->  B^-1[j, i] = L^-1[cq[j], rp[i]]
    return np.ascontiguousarray(L[np.ix_(rp, cq)]), np.ascontiguousarray(Li[np.ix_(cq, rp)])


def exact_basis(m, seed):
    """(B, B^-1 in closed form) of the exact family"""
    return _assemble(*_exact_parts(m, seed))


def tie_basis(m, seed, R, pos=5, flip=False):
    """The exact family with a directed tie: basic column `pos` holds its largest entries, +d and -d, in the rows R
    (the diagonal entry of L in R[0], or in R[1] with flip), so that the first maximum is min(R)."""
    d, F, rp, cq = _exact_parts(m, seed)
    h = m // 2
    F[0, 0] = -d[0]  # L[h, 0] = -L[0, 0]
    rp, cq = rp.copy(), cq.copy()

    def place(perm, where, what):
        j = int(np.flatnonzero(perm == what)[0])
        perm[j], perm[where] = perm[where], perm[j]

    r_diag, r_tie = (R[1], R[0]) if flip else (R[0], R[1])
    place(rp, r_diag, 0)
    place(rp, r_tie, h)
    place(cq, pos, 0)
    j = int(np.flatnonzero(cq == h)[0])
    if j < pos:  # row h's own column must come later, or the row is used up before the tie
        cq[j], cq[m - 1] = cq[m - 1], cq[j]
    return _assemble(d, F, rp, cq)


def seed_of(m):
    return 9000 + m


EXACT_SIZES = [2, 17, 63, 64, 65, 130, 513, 1030]   # modelled on the host (O(m^3))
NATURAL_SIZES = [2048, 2050, 4100]                  # closed form only
TIE_M = 1030
TIE_ROWS = [(63, 64), (5, 700), (3, 515), (3, 1027), (511, 512), (1023, 1024)]
TIE_POS = 5
TIE_SEED = 701  # one of the seeds the proof accepts for every row set (tests/test_rebuild_model_cpu.py runs it)


@functools.lru_cache(maxsize=None)
def exact_case(m):
    """B, its closed-form inverse, and the model's W, perm, ties - proved exact in both orders of the arithmetic and for
    every sub-panel width; made once and shared (read-only)"""
    B, Binv = exact_basis(m, seed_of(m))
    return _proved(B, Binv)


@functools.lru_cache(maxsize=None)
def tie_case(R, flip=False):
    B, Binv = tie_basis(TIE_M, TIE_SEED, R, TIE_POS, flip)
    c = _proved(B, Binv)
    assert TIE_POS in c.ties and tuple(c.ties[TIE_POS]) == tuple(sorted(R)), (R, c.ties.get(TIE_POS))
    assert c.perm[TIE_POS] == min(R)
    return c


def _proved(B, Binv):
    W, perm, ties = eliminate(B, prove=True)
    for nbw in (16, 8, 4):
        Wb, pb = blocked_replay(B, nbw_max=nbw, prove=True)
        if not (np.array_equal(Wb, W) and np.array_equal(pb, perm)):
            raise NotExact(f"the blocked replay with {nbw}-column sub-panels differs from the columnwise model")
    if not np.array_equal(W, Binv):
        raise NotExact("the model differs from the closed form")
    for a in (B, Binv, W, perm):
        a.setflags(write=False)
    return SimpleNamespace(B=B, Binv=Binv, W=W, perm=perm, ties=ties)


NATURAL_SEED = 9001  # accepted by the proof at the three sizes (tests/test_rebuild_model_cpu.py runs it)


def natural_width(m):
    """the sub-panel width the rebuild picks for m rows by itself"""
    return 16 if m <= 2048 else (8 if m <= 4096 else 4)


@functools.lru_cache(maxsize=None)
def natural_case(m):
    """B and its closed-form inverse at a size the O(m^3) columnwise model is not run at; the proof is the blocked replay
    in the width the size asks for (prove_natural)"""
    B, Binv = exact_basis(m, NATURAL_SEED)
    B.setflags(write=False)
    Binv.setflags(write=False)
    return SimpleNamespace(B=B, Binv=Binv)


# ------------------------------------------------------------------ the guard at its edge
GUARD_M = 130
GUARD_POS = [0, 63, 64, GUARD_M - 1]


def guard_basis(t, pos):
    """B = diag(exact-family block, t) with the t column at basic position pos: alpha of that column is t e_(m-1) exactly.
    Returns B and the inverse it has if t is accepted (the block's entries meet only zeros of the new row and column)."""
    m = GUARD_M
    c = exact_case(m - 1)
    cols = [j for j in range(m - 1)]
    cols.insert(pos, m - 1)
    full = np.zeros((m, m))
    full[:m - 1, :m - 1] = c.B
    full[m - 1, m - 1] = t
    inv = np.zeros((m, m))
    inv[:m - 1, :m - 1] = c.Binv
    with np.errstate(divide="ignore"):
        inv[m - 1, m - 1] = np.float64(1.0) / np.float64(t)
    return np.ascontiguousarray(full[:, cols]), np.ascontiguousarray(inv[cols, :])


# ------------------------------------------------------------------ wide mode: general dense matrices
# The same elimination in np.longdouble, the pivot rows GIVEN (the device's), with a componentwise bound on what an f64
# evaluation of it - column by column OR blocked - may differ from the model's final W by.  First order in u = 2^-53;
# dot products are bounded by gamma_n sum |terms| in ANY order (Higham, Accuracy and Stability, par. 3.1).
#
# Propagation.  Write step s as W' = E_s W with the eta matrix E_s (column p: f_i = -alpha_i / alpha_p, and 1 / alpha_p).
# The later steps are exact functions of the state they meet.  If the state after step s is off by d, the final W~ still
# has W~ a_j = e_perm[j] for j > s (those steps enforce it, and later etas leave the unit columns of used rows alone),
# while W~ a_j = e_perm[j] + T d a_j for j <= s, with T = E_(m-1) ... E_(s+1) = W_m W_(s+1)^-1.  So, to first order,
#
#     W~ - W_m = T d Q_s ,     Q_s = A_B[:, :s+1] (A_B^-1)[:s+1, :] .
#
# An entrywise recurrence |E_s| |d| would grow by a factor per step (it ignores that the next pivot column is formed
# from the same perturbed state); the collapsed products T and Q_s do not.  The bound is the sum of |T| rho |Q_s| over the
# local errors rho below.  W_(s+1)^-1 needs no inversion: column perm[j] is a_j for j <= s, the rest are unit columns.
#
# Local errors, column by column (k_ref_ftran, k_ref_pick, k_ref_update):
#     d_alpha = gamma_m (|W_s| |a_s|)
#     d_f_i   = ((d_alpha_i + |f_i| d_alpha_p) / |alpha_p|) / (1 - d_alpha_p / |alpha_p|) + 2 u |f_i|
#     d_f_p   = (d_alpha_p / alpha_p^2) / (1 - d_alpha_p / |alpha_p|) + 2 u / |alpha_p|       (of 1 / alpha_p)
#     rho_s   = d_f (x) |W_s[p, :]|  +  2 u (|W_(s+1)| + |f| (x) |W_s[p, :]|)                   (the update, fused or not)
# Local errors, blocked, macro panel K = [k0, k1) with W_0 = W_k0 and T_(r->t) = E_(t-1) ... E_r inside the panel; let
# Theta >= |T_(r->t)| entrywise for all k0 <= r <= t <= k1.  The panel's steps act on the EFFECTIVE state, the exact
# product of the computed etas with W_0; step t forms its pivot column not from that state but from C = W_0 A_K carried
# through the earlier etas, so
#     d_alpha = |T_(k0->t)| gamma_m (|W_0| |a_t|) + Theta (u sum_r |c_t^(r)|)    c_t^(r): column t of the tile after r etas
#     rho_t   = d_f (x) |W_t[p, :]|                                     d_f as above
# and at the panel's end the effective state is replaced by fl(W_0 + V W_0[P, :]), V the computed product of the etas:
#     rho_end = gamma_(NB + 2) (|W_0| + |V| |W_0[P, :]|)  +  (Theta (u sum_t |V^(t)|)) |W_0[P, :]|
# (each entry of V is rounded once per eta that touches it, and the later etas of the panel carry that on).
# The bound returned covers BOTH forms: the columnwise and the blocked local errors are added.  The per-step 2 u (...)
# terms are summed per macro panel with the entrywise maxima of |T| and |Q_s| over the panel's steps.  Nothing is
# measured.  The model's own rounding (2^-64 per operation where longdouble is the x87 format) and the f64 evaluation
# of the bound's non-negative sums are covered by a factor 1 + 2^-8.
#
# The pivot check uses d_alpha alone: the margin leaves out what the state's accumulated error adds to alpha, so it is
# SMALLER than the true uncertainty.  That makes "ok" stricter and "ambiguous" rarer than the bounds warrant, never laxer.
U = 2.0 ** -53


def _eta_rows(X, f, p, inv):
    """E X for the eta matrix with column p = (f, inv at p); f[p] is 0"""
    Xp = X[p].copy()
    X = X + f[:, None] * Xp[None, :]
    X[p] = Xp * inv
    return X


def wide_model(B, perm, eps=0.0):
    """B: m x m f64; perm: the pivot rows to take.  Returns W (rows permuted), bound (same shape, f64), and per step
    ok[k] (the given row is a maximiser of |alpha| over the unused rows within the margins) and ambiguous[k] (the margins
    cannot tell it from another row)."""
    Lf = np.longdouble
    assert float(np.finfo(Lf).eps) < 2.0 ** -60, "np.longdouble is not wider than f64 here"
    B = np.ascontiguousarray(B, dtype=np.float64)
    aB = np.abs(B)
    perm = np.asarray(perm, dtype=np.int64)
    m = B.shape[0]
    assert sorted(perm.tolist()) == list(range(m))
    # ---- pass 1: the trajectory
    W = np.eye(m, dtype=Lf)
    F, INV, ALPHA, PROW, W0 = [], [], [], [], []
    for k in range(m):
        if k % NB == 0:
            W0.append(W.astype(np.float64))
        alpha = W @ B[:, k].astype(Lf)
        p = int(perm[k])
        if not np.abs(alpha[p]) > 0:
            raise Singular(k, p, float(alpha[p]))
        f = -alpha / alpha[p]
        f[p] = 0
        PROW.append(np.abs(W[p]).astype(np.float64))
        W = _eta_rows(W, f, p, 1 / alpha[p])
        F.append(f.astype(np.float64))
        INV.append(float(1 / alpha[p]))
        ALPHA.append(np.abs(alpha).astype(np.float64))
    Wm = W.astype(np.float64)
    Binv = W[perm]
    Binv64 = Binv.astype(np.float64)
    # ---- pass 2: the bound
    gm = m * U / (1.0 - m * U)
    gnb = (NB + 2) * U / (1.0 - (NB + 2) * U)
    used = np.zeros(m, dtype=bool)
    ok = np.zeros(m, dtype=bool)
    amb = np.zeros(m, dtype=bool)
    Winv = np.eye(m)
    Q = np.zeros((m, m))
    bound = np.zeros((m, m))
    for k0 in range(0, m, NB):
        k1 = min(m, k0 + NB)
        Wk0 = W0[k0 // NB]
        aW0 = np.abs(Wk0)
        # Theta: entrywise maximum of |T_(r->t)| over the pairs of the panel
        Theta = np.eye(m)
        for r in range(k0, k1):
            T = np.eye(m)
            for t in range(r, k1):
                T = _eta_rows(T, F[t], int(perm[t]), INV[t])
                np.maximum(Theta, np.abs(T), out=Theta)
        # the tile's columns and V through the panel's etas
        C = Wk0 @ B[:, k0:k1]
        Csum = np.abs(C)
        Tp = np.eye(m)
        Vsum = np.zeros((m, m))
        D1 = np.zeros((m, k1 - k0))
        for t in range(k0, k1):
            D1[:, t - k0] = np.abs(Tp) @ (gm * (aW0 @ aB[:, t]))  # Tp is T_(k0->t) here
            C = _eta_rows(C, F[t], int(perm[t]), INV[t])
            Csum += np.abs(C)
            Tp = _eta_rows(Tp, F[t], int(perm[t]), INV[t])
            Vsum += np.abs(Tp - np.eye(m))
        V = np.abs(Tp - np.eye(m))
        d_alpha_bl = D1 + Theta @ (U * Csum)
        # the steps
        Wabs = aW0.copy()
        Wt = Wk0.copy()
        Tmax, Qmax, Rsum = np.zeros((m, m)), np.zeros((m, m)), np.zeros((m, m))
        for k in range(k0, k1):
            alpha, p = ALPHA[k], int(perm[k])
            ap = alpha[p]
            d_col = gm * (Wabs @ aB[:, k])
            d_bl = d_alpha_bl[:, k - k0]
            margin = np.maximum(d_col, d_bl)
            others = ~used
            others[p] = False
            ok[k] = bool(np.all(ap + margin[p] >= alpha[others] - margin[others]))
            amb[k] = bool(np.any(alpha[others] + margin[others] >= ap - margin[p]))
            d_alpha = d_col + d_bl
            if not (ap - d_alpha[p] > eps):
                raise Singular(k, p, float(ap))
            rel = d_alpha[p] / ap
            af = alpha / ap
            d_f = ((d_alpha + af * d_alpha[p]) / ap) / (1.0 - rel) + 2 * U * af
            d_f[p] = (rel / ap) / (1.0 - rel) + 2 * U / ap
            af[p] = 0.0
            Wt = _eta_rows(Wt, F[k], p, INV[k])
            Wabs = np.abs(Wt)
            used[p] = True
            Winv[:, p] = B[:, k]
            Q += B[:, k][:, None] * Binv64[k][None, :]
            T = np.abs(Wm @ Winv)
            aQ = np.abs(Q)
            bound += (T @ d_f)[:, None] * (PROW[k] @ aQ)[None, :]
            np.maximum(Tmax, T, out=Tmax)
            np.maximum(Qmax, aQ, out=Qmax)
            Rsum += Wabs + af[:, None] * PROW[k][None, :]
        bound += 2 * U * (Tmax @ Rsum @ Qmax)
        rho_end = gnb * (aW0 + V @ aW0) + (Theta @ (U * Vsum)) @ aW0
        bound += T @ rho_end @ aQ
    bound = bound[perm] * (1.0 + 2.0 ** -8)
    return SimpleNamespace(W=Binv, bound=bound, ok=ok, ambiguous=amb)


def f64_eliminate(B, perm, parts=1, reverse=False):
    """the elimination in f64 with the dot products summed in a chosen order: forward or reversed, in `parts` partial sums
    that are then added (what a wave sum or a K-split does)"""
    B = np.ascontiguousarray(B, dtype=np.float64)
    m = B.shape[0]
    W = np.eye(m)
    order = np.arange(m)[::-1] if reverse else np.arange(m)
    chunks = np.array_split(order, parts)
    for k in range(m):
        a = B[:, k]
        partial = []
        for ch in chunks:
            s = np.zeros(m)
            for t in ch:
                s = s + W[:, t] * a[t]
            partial.append(s)
        alpha = partial[0]
        for s in partial[1:]:
            alpha = alpha + s
        p = int(perm[k])
        f = -(alpha / alpha[p])
        rowp = W[p].copy()
        f[p] = 0.0
        W = W + f[:, None] * rowp[None, :]
        W[p] = rowp / alpha[p]
    return W[np.asarray(perm)]


WIDE_SIZES = [17, 65, 130, 300]
WIDE_SCALED_M = 65  # at 130 rows the scaled matrix's bound is 1.8e-6 max|W|: above the 1e-6 that still proves something


def wide_seed(m):
    return 5100 + m


@functools.lru_cache(maxsize=None)
def wide_basis(m, scaled=False):
    """entries from N(0, 1): mixed signs, rows really exchanged, growth above 1; scaled: rows times 10^+-3"""
    rng = np.random.default_rng(wide_seed(m) + (7 if scaled else 0))
    B = rng.normal(size=(m, m))
    if scaled:
        B *= (10.0 ** rng.integers(-3, 4, size=m))[:, None]
    B.setflags(write=False)
    return B


WIDE_CASES = [(m, False) for m in WIDE_SIZES] + [(WIDE_SCALED_M, True)]

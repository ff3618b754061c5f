"""A model of the steepest-edge weights of the primal loop (ellp_amd/csrc/engine/ellp_se.inc): every nonbasic position j
carries gamma_j = 1 + |B^-1 a_j|^2 of the current basis.

    definition(A, B_index, N_index)      the weights from their definition (a refined solve in extended precision)
    start_perm(A_N)                      the creation formula at a signed-permutation basis, 1 + sum a^2         (k_se_init)
    start_general(W, A_N)                the creation formula at any other basis, 1 + |W a_j|^2 from the inverse W
                                         the engine has just built                                                (k_se_exact_*)
    step(G, W_old, A_N, q, r, d)         one Goldfarb-Reid update from the DEVICE'S OWN numbers                   (k_price_se)

step: with alpha = +-d (the device's FTRAN result is +-alpha_q; the sign is resolved against W_old a_q and cancels in every
formula), rho = row r of W_old, v = W_old^T alpha, gq = 1 + |alpha|^2 and abar_j = (rho . a_j) / alpha_r,

    G'_j = max(G_j - 2 abar_j (a_j . v) + abar_j^2 gq, 1 + abar_j^2)   (j != q),      G'_q = max(gq / alpha_r^2, 1).

The recurrence cancels: over a whole solve no fixed tolerance against the definition can hold (a plain f64 numpy evaluation
with a fresh inverse per pivot is 1e-11 off after 10 pivots and 1e-4 after some hundreds).  So the check is made per step,
from the weights the device held before the step, with a componentwise bound dG on what ANY f64 evaluation of the step may
differ from the model by: whatever the order of the additions, fused or not, as tests/refresh_model.py does it for the
refresh.  With u = 2^-53 and gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of Numerical Algorithms, §3.1):

    |d|^2        :  d_n2  = gamma_m sum d_i^2                     gq = 1 + n2: one rounding more
    rho . a_j    :  d_ar  = gamma_m sum |rho_i| |a_ij|
    v = W^T alpha:  d_v   = gamma_m |W|^T |alpha|
    a_j . v      :  d_av  = |a_j| . d_v  +  gamma_m |a_j| . (|v| + d_v)        (the inherited error of v, and the product with it)

and through the epilogue every scalar operation z = x op y on computed operands (|x^ - x| <= dx, |y^ - y| <= dy) adds one
rounding to what it inherits:

    x + y :  dz = dx + dy + u (|x + y| + dx + dy)
    x * y :  dz = e + u (|x y| + e),           e = |x| dy + |y| dx + dx dy
    x / y :  dz = e + u (|x / y| + e),         e = (dx + |x / y| dy) / (|y| - dy)
    max(x, y) :  dz = max(dx, dy)              (|max(x^, y^) - max(x, y)| <= max(dx, dy))

The multiplication by 2 is exact.  The operations are those of the kernel, in its order: abar = ar / alpha_r;
gn = (G - (2 abar) av) + (abar abar) gq;  lo = 1 + abar abar;  gl = gq / (alpha_r alpha_r).  A fused operation rounds once
where the bound allows two.  Nothing in the bounds is measured and they carry no factor.

Arithmetic: np.longdouble where that is the x87 80-bit format, double-double elsewhere (refresh_model's two classes,
extended here by the elementwise product, quotient and maximum the epilogue needs).  The bounds themselves are sums of
non-negative terms, evaluated in np.longdouble."""
from types import SimpleNamespace

import numpy as np

import refresh_model as rm

U = rm.U
L = np.longdouble


class _Wide(rm._Wide):
    @staticmethod
    def mul(X, Y):
        return X * Y

    @staticmethod
    def div(X, Y):
        return X / Y

    @staticmethod
    def maximum(X, Y):
        return np.maximum(X, Y)

    @staticmethod
    def reshape(X, shape):
        return X.reshape(shape)

    @staticmethod
    def colsum(X):
        return X.sum(axis=0)

    @staticmethod
    def broadcast(X, n):
        return np.broadcast_to(X, (n,)).copy()


class _DD(rm._DD):
    @staticmethod
    def mul(X, Y):
        p, e = rm._two_prod(X[0], Y[0])
        e = e + (X[0] * Y[1] + X[1] * Y[0])
        return rm._two_sum(p, e)

    @staticmethod
    def div(X, Y):
        q1 = X[0] / Y[0]
        r = _DD.add(X, _DD.neg(_DD.mul((q1, np.zeros_like(q1)), Y)))
        q2 = r[0] / Y[0]
        r = _DD.add(r, _DD.neg(_DD.mul((q2, np.zeros_like(q2)), Y)))
        q3 = r[0] / Y[0]
        s, e = rm._two_sum(q1, q2)
        return rm._two_sum(s, e + q3)

    @staticmethod
    def maximum(X, Y):
        first = (X[0] > Y[0]) | ((X[0] == Y[0]) & (X[1] >= Y[1]))
        return np.where(first, X[0], Y[0]), np.where(first, X[1], Y[1])

    @staticmethod
    def reshape(X, shape):
        return X[0].reshape(shape), X[1].reshape(shape)

    @staticmethod
    def colsum(X):
        hi, lo = np.zeros(X[0].shape[1:]), np.zeros(X[0].shape[1:])
        for i in range(X[0].shape[0]):
            hi, lo = rm._dd_add(hi, lo, X[0][i], X[1][i])
        return hi, lo

    @staticmethod
    def broadcast(X, n):
        return np.broadcast_to(X[0], (n,)).copy(), np.broadcast_to(X[1], (n,)).copy()


def _arith(arith):
    return arith or (_Wide if rm.LONGDOUBLE_IS_WIDE else _DD)


def _gamma(k):
    return L(k) * L(U) / (L(1) - L(k) * L(U))


# ---- the rounding bounds of the scalar operations (values and bounds in np.longdouble)
def _add(x, dx, y, dy):
    z = x + y
    e = dx + dy
    return z, e + L(U) * (np.abs(z) + e)


def _mul(x, dx, y, dy):
    z = x * y
    e = np.abs(x) * dy + np.abs(y) * dx + dx * dy
    return z, e + L(U) * (np.abs(z) + e)


def _div(x, dx, y, dy):
    z = x / y
    e = (dx + np.abs(z) * dy) / (np.abs(y) - dy)
    return z, e + L(U) * (np.abs(z) + e)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _frozen(**kw):
    for a in kw.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return SimpleNamespace(**kw)


def definition(A, B_index, N_index, arith=None, tol=2.0 ** -60):
    """1 + |B^-1 a_j|^2 per nonbasic position, np.longdouble.  A: m x n f64.  X = B^-1 A_N from an f64 solve, refined with
    residuals formed in the wide type until the correction is below 2^-60 of max|X| column by column.  The wide type here
    is double-double whatever the platform: a residual formed in the 80-bit format is itself only good to 2^-63 |B||X|,
    which leaves the correction at cond(B) 2^-63 — above 2^-60 for every basis worth testing."""
    ar = arith or _DD
    A = _f64(A)
    Bm = np.ascontiguousarray(A[:, np.asarray(B_index)])
    AN = np.ascontiguousarray(A[:, np.asarray(N_index)])
    X = ar.lift(np.linalg.solve(Bm, AN))
    for _ in range(12):
        R = ar.add(ar.lift(AN), ar.neg(ar.matmul(Bm, X)))
        C = np.linalg.solve(Bm, np.asarray(ar.to_longdouble(R), dtype=np.float64))
        X = ar.add(X, ar.lift(C))
        scale = np.abs(np.asarray(ar.to_longdouble(X), dtype=np.float64)).max(axis=0)
        if (np.abs(C).max(axis=0) <= tol * scale).all():
            break
    else:
        raise AssertionError("definition: the refinement did not settle (an ill-conditioned basis)")
    g = ar.add(ar.lift(np.ones(AN.shape[1])), ar.colsum(ar.mul(X, X)))
    return ar.to_longdouble(g)


def start_perm(A_N, arith=None):
    """1 + sum_i a_ij^2: m + 1 non-negative terms in any order: dG = gamma_(m+1) G"""
    ar = _arith(arith)
    A_N = _f64(A_N)
    m = A_N.shape[0]
    X = ar.lift(A_N)
    G = ar.to_longdouble(ar.add(ar.lift(np.ones(A_N.shape[1])), ar.colsum(ar.mul(X, X))))
    return _frozen(G=G, dG=_gamma(m + 1) * G)


def start_general(W, A_N, arith=None):
    """1 + sum_i T_ij^2, T = W A_N.  Every computed entry of T is within dT = gamma_m (|W| |A_N|) of T; its square is then
    within 2 |T| dT + dT^2 of T^2, and the m + 1 non-negative terms 1, T^_ij^2 <= (|T_ij| + dT_ij)^2 are added in any order:
    dG = sum_i (2 |T| dT + dT^2) + gamma_(m+1) (1 + sum_i (|T| + dT)^2)."""
    ar = _arith(arith)
    W, A_N = _f64(W), _f64(A_N)
    m = W.shape[0]
    Tw = ar.matmul(W, ar.lift(A_N))
    G = ar.to_longdouble(ar.add(ar.lift(np.ones(A_N.shape[1])), ar.colsum(ar.mul(Tw, Tw))))
    T = np.abs(ar.to_longdouble(Tw))
    dT = _gamma(m) * (np.abs(W).astype(L) @ np.abs(A_N).astype(L))
    dG = (2 * T * dT + dT * dT).sum(axis=0) + _gamma(m + 1) * (L(1) + ((T + dT) ** 2).sum(axis=0))
    return _frozen(G=G, dG=dG)


def alpha_of(W_old, a_q, d):
    """the device's d is +-alpha_q: the sign that agrees with W_old a_q"""
    d = _f64(d)
    return d if float(np.dot(d, _f64(W_old) @ _f64(a_q))) >= 0.0 else -d


def step(G, W_old, A_N, q, r, d, arith=None):
    """One Goldfarb-Reid update (module docstring).  G: the nN weights before; W_old: the m x m inverse the iteration's FTRAN
    used; A_N: m x nN, the nonbasic columns in the position order of that iteration; q, r: entering position, leaving row;
    d: the device's +-alpha_q.  Returns G (= G') and dG as np.longdouble arrays (read-only)."""
    ar = _arith(arith)
    G, W, A_N = _f64(G), _f64(W_old), _f64(A_N)
    m, nN = A_N.shape
    assert W.shape == (m, m) and G.shape == (nN,) and 0 <= q < nN and 0 <= r < m
    alpha = alpha_of(W, A_N[:, q], d)
    alpha_r = float(alpha[r])
    rho = np.ascontiguousarray(W[r])
    # ---- the model, in the wide type
    one = ar.lift(np.ones(1))
    n2_w = ar.reshape(ar.matmul(alpha[None, :], ar.lift(alpha[:, None])), (1,))
    gq_w = ar.add(one, n2_w)
    ar_w = ar.reshape(ar.matmul(rho[None, :], ar.lift(A_N)), (nN,))
    v_w = ar.matmul(np.ascontiguousarray(W.T), ar.lift(alpha[:, None]))
    av_w = ar.reshape(ar.matmul(np.ascontiguousarray(A_N.T), v_w), (nN,))
    ab_w = ar.div(ar_w, ar.lift(np.full(nN, alpha_r)))
    t_w = ar.mul(ab_w, av_w)
    ab2_w = ar.mul(ab_w, ab_w)
    gq_n = ar.broadcast(gq_w, nN)
    gn_w = ar.add(ar.add(ar.lift(G), ar.neg(ar.add(t_w, t_w))), ar.mul(ab2_w, gq_n))
    lo_w = ar.add(ar.lift(np.ones(nN)), ab2_w)
    Gn = np.array(ar.to_longdouble(ar.maximum(gn_w, lo_w)))
    a2_w = ar.mul(ar.lift(np.full(1, alpha_r)), ar.lift(np.full(1, alpha_r)))
    gl_w = ar.maximum(ar.div(gq_w, a2_w), one)
    Gn[q] = ar.to_longdouble(gl_w)[0]
    # ---- the bounds
    lw = lambda X: np.asarray(ar.to_longdouble(X), dtype=L)
    z = L(0)
    gm = _gamma(m)
    aW, aA, aal = np.abs(W).astype(L), np.abs(A_N).astype(L), np.abs(alpha).astype(L)
    n2 = lw(n2_w)[0]
    gq, dgq = _add(L(1), z, n2, gm * n2)
    arv, dar = lw(ar_w), gm * (np.abs(rho).astype(L) @ aA)
    ab, dab = _div(arv, dar, L(alpha_r), z)
    v = lw(v_w)[:, 0]
    dv = gm * (aW.T @ aal)
    av, dav = lw(av_w), aA.T @ dv + gm * (aA.T @ (np.abs(v) + dv))
    t, dt = _mul(2 * ab, 2 * dab, av, dav)
    s1, ds1 = _add(G.astype(L), z, -t, dt)
    ab2, dab2 = _mul(ab, dab, ab, dab)
    t5, dt5 = _mul(ab2, dab2, gq, dgq)
    _, dgn = _add(s1, ds1, t5, dt5)
    _, dlo = _add(L(1), z, ab2, dab2)
    dG = np.maximum(dgn, dlo)
    a2, da2 = _mul(L(alpha_r), z, L(alpha_r), z)
    _, dgl = _div(gq, dgq, a2, da2)
    dG[q] = dgl
    return _frozen(G=Gn, dG=dG, gq=gq, dgq=dgq)


# ---- the plain f64 numpy evaluation of the same formulas, and the five mistakes the bounds must stop
MISTAKES = ("sign", "dropped", "stored_gq", "q_kept", "again_after_flip")


def start_perm_f64(A_N):
    A_N = _f64(A_N)
    return 1.0 + (A_N * A_N).sum(axis=0)


def start_general_f64(W, A_N):
    T = _f64(W) @ _f64(A_N)
    return 1.0 + (T * T).sum(axis=0)


def step_f64(G, W_old, A_N, q, r, d, mistake=None):
    """mistake: "sign" (+ 2 abar (a_j . v)), "dropped" (that term left out), "stored_gq" (G[q] for 1 + |alpha|^2),
    "q_kept" (position q not rewritten).  "again_after_flip" is a mistake of the loop, not of the step: the caller applies
    the last pivot's step once more at a bound flip."""
    G, W, A_N = _f64(G), _f64(W_old), _f64(A_N)
    alpha = alpha_of(W, A_N[:, q], d)
    arq = alpha[r]
    gq = G[q] if mistake == "stored_gq" else 1.0 + float(alpha @ alpha)
    ab = (W[r] @ A_N) / arq
    av = A_N.T @ (W.T @ alpha)
    cross = {"sign": 2.0, "dropped": 0.0}.get(mistake, -2.0)
    out = np.maximum(G + cross * ab * av + ab * ab * gq, 1.0 + ab * ab)
    out[q] = G[q] if mistake == "q_kept" else max(gq / (arq * arq), 1.0)
    return out


# ---- the LPs
def boxed_lp(seed, m, n, nfree=3):
    """A small LP with every kind of bound, as a fixture dict (tests/helpers.py): A uniform(-1, 1), rows A x <= A x0 + slack
    with x0 uniform(0.2, 0.8) and slack uniform(0.1, 0.5), c normal.  Variable j < nfree is Free with the two rows
    +-x_j <= 5; of the others j % 3 == 0 is TwoSided(0, 1), 1 is Lower(0) with c_j = |c_j|, 2 is Upper(1) with c_j = -|c_j|.
    The standard form has m + 2 nfree rows."""
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1.0, 1.0, size=(m, n))
    x0 = rng.uniform(0.2, 0.8, size=n)
    b = A @ x0 + rng.uniform(0.1, 0.5, size=m)
    c = rng.normal(size=n)
    fx = {"vars": [], "constraints": []}
    for j in range(n):
        if j < nfree:
            fx["vars"].append([float(c[j]), ["Free", 0.0, 0.0]])
        elif j % 3 == 0:
            fx["vars"].append([float(c[j]), ["TwoSided", 0.0, 1.0]])
        elif j % 3 == 1:
            fx["vars"].append([abs(float(c[j])), ["Lower", 0.0, 0.0]])
        else:
            fx["vars"].append([-abs(float(c[j])), ["Upper", 0.0, 1.0]])
    for i in range(m):
        fx["constraints"].append([[[j, float(A[i, j])] for j in range(n)], "Lte", float(b[i])])
    for j in range(nfree):
        fx["constraints"].append([[[j, 1.0]], "Lte", 5.0])
        fx["constraints"].append([[[j, -1.0]], "Lte", 5.0])
    return fx


# the boxed LPs the GPU test solves step by step: standard-form rows -> (seed, m, n).  16 / 17 rows: the row blocks of
# k_se_vreduce; 64 / 65: an ld edge; 39, 70: the sizes the recurrence's drift was first measured at.
# tests/test_se_model_cpu.py checks what the GPU test relies on: both phases end Optimal, phase 2 takes bound flips.
SOLVES = {16: (7, 10, 26), 17: (7, 11, 28), 39: (7, 33, 70), 64: (7, 58, 120), 65: (7, 59, 122), 70: (7, 64, 130)}
# 64 and 65 row blocks of k_update2 (4 rows each), n about m: the first steps of phase 1 only
BLOCK_EDGES = {256: (7, 250, 256), 260: (7, 254, 260)}

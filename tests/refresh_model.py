"""A model of one Newton-Schulz refresh of B^-1 (ellp_amd/csrc/engine/ellp_gemm.inc),

    E = I - A_B W ,   W' = W + W E ,

in extended precision, with componentwise bounds on what ANY f64 evaluation of the two products may differ
from it by: whatever the order of the additions, fused or not (Higham, Accuracy and Stability of Numerical
Algorithms, §3.1: a dot product of m terms has the relative error gamma_m = m u / (1 - m u) on sum |x_k||y_k|),
plus the one rounding of each epilogue (delta_ij - acc, W_ij + acc):

    dE = gamma (|A_B||W|) + u |E|
    dW = |W| dE + gamma (|W| (|E| + dE)) + u |W'|          u = 2^-53

|W| dE is what the second product inherits from the computed E, |E| + dE bounds that computed E.  Nothing in
the bounds is measured.

The products are formed in np.longdouble where that is the x87 80-bit format (eps = 2^-63: the model's own
error is 2^-11 of the bounds); elsewhere (eps not below 2^-60) in double-double arithmetic, with error-free
products and sums, vectorised over the entries (about 2^-100).  tests/test_refresh_model_cpu.py checks the
second against the first where both exist."""
import functools
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -53
LONGDOUBLE_IS_WIDE = float(np.finfo(np.longdouble).eps) < 2.0 ** -60


# ---- double-double: a value is hi + lo, two f64 arrays with |lo| <= ulp(hi) / 2
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    sp = 134217729.0  # 2^27 + 1 (Veltkamp)
    t = sp * a
    ah = t - (t - a)
    al = a - ah
    t = sp * b
    bh = t - (t - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dd_add(ah, al, bh, bl):
    s, e = _two_sum(ah, bh)
    e = e + (al + bl)
    return _two_sum(s, e)


def _dd_matmul(A, Bh, Bl=None):
    """(hi, lo) of A (f64) times Bh + Bl (double-double), one error-free rank-1 update per k"""
    m, n = A.shape[0], Bh.shape[1]
    hi, lo = np.zeros((m, n)), np.zeros((m, n))
    for k in range(A.shape[1]):
        p, e = _two_prod(A[:, k:k + 1], Bh[k:k + 1, :])
        if Bl is not None:
            e = e + A[:, k:k + 1] * Bl[k:k + 1, :]
        hi, lo = _dd_add(hi, lo, p, e)
    return hi, lo


class _Wide:
    """the few operations the model needs, in np.longdouble"""

    @staticmethod
    def lift(a):
        return np.asarray(a, dtype=np.float64).astype(np.longdouble)

    @staticmethod
    def matmul(A, X):  # A f64, X wide
        return A.astype(np.longdouble) @ X

    @staticmethod
    def add(X, Y):
        return X + Y

    @staticmethod
    def neg(X):
        return -X

    @staticmethod
    def to_longdouble(X):
        return X


class _DD:
    """the same in double-double: a wide value is the pair (hi, lo)"""

    @staticmethod
    def lift(a):
        a = np.asarray(a, dtype=np.float64)
        return a, np.zeros_like(a)

    @staticmethod
    def matmul(A, X):
        return _dd_matmul(A, X[0], X[1])

    @staticmethod
    def add(X, Y):
        return _dd_add(X[0], X[1], Y[0], Y[1])

    @staticmethod
    def neg(X):
        return -X[0], -X[1]

    @staticmethod
    def to_longdouble(X):
        return X[0].astype(np.longdouble) + X[1].astype(np.longdouble)


def refresh_model(A_B, W, arith=None):
    """A_B, W: m x m f64.  Returns E, Wn (= W'), dE, dW as np.longdouble arrays (read-only), and
    resid = max|E|, dresid = max dE as Python floats rounded up."""
    ar = arith or (_Wide if LONGDOUBLE_IS_WIDE else _DD)
    A_B = np.ascontiguousarray(A_B, dtype=np.float64)
    W = np.ascontiguousarray(W, dtype=np.float64)
    m = A_B.shape[0]
    assert A_B.shape == (m, m) and W.shape == (m, m)
    E_w = ar.add(ar.lift(np.eye(m)), ar.neg(ar.matmul(A_B, ar.lift(W))))
    Wn_w = ar.add(ar.lift(W), ar.matmul(W, E_w))
    E, Wn = ar.to_longdouble(E_w), ar.to_longdouble(Wn_w)
    # the bounds: sums of non-negative terms, so any accurate evaluation will do
    L = np.longdouble
    u = L(U)
    gamma = L(m) * u / (L(1) - L(m) * u)
    aA, aW = np.abs(A_B).astype(L), np.abs(W).astype(L)
    dE = gamma * (aA @ aW) + u * np.abs(E)
    dW = aW @ dE + gamma * (aW @ (np.abs(E) + dE)) + u * np.abs(Wn)
    out = SimpleNamespace(E=E, Wn=Wn, dE=dE, dW=dW, resid=float(np.abs(E).max()),
                          dresid=float(np.nextafter(np.float64(dE.max()), np.inf)))
    for a in (E, Wn, dE, dW):
        a.setflags(write=False)
    return out


def perturbed_inverse(B, seed, rel=1e-6):
    """inv(B) (I + rel G), G uniform in [-1, 1]: the residual E ~ -rel G is dense and unsymmetric, and W E is six
    orders of magnitude above the rounding bound dW"""
    m = B.shape[0]
    G = np.random.default_rng(seed).uniform(-1.0, 1.0, size=(m, m))
    return np.ascontiguousarray(np.linalg.inv(B) @ (np.eye(m) + rel * G))


SIZES = [1, 2, 15, 16, 17, 127, 128, 129, 143, 145, 255, 257, 300]  # around the K stage of 16 and the 128 tile; odd m; m = 1


def seed_of(m):
    return 4100 + m


@functools.lru_cache(maxsize=None)
def case(m):
    """(B, W, model) of size m, made once and shared: the arrays are read-only.  B is the basis of
    dense_basis_problem(m, seed_of(m))."""
    from test_gpu_rebuild import dense_basis_problem
    _, B = dense_basis_problem(m, seed_of(m))
    W = perturbed_inverse(B, seed_of(m) + 1)
    B.setflags(write=False)
    W.setflags(write=False)
    return B, W, refresh_model(B, W)

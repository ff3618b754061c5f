"""A model of the kernels that keep an explicit-inverse engine right between two rebuilds of B^-1
(ellp_amd/csrc/engine/ellp_engine.hip):

    btran(W, c_B)                         u = W^T c_B                                    (k_btran_part / _reduce)
    drift(A_B, d, a_q, sgn)               max|sgn A_B d - a_q| / max|a_q|                 (k_drift_part / _reduce)
    rhs(A_N, x_N, b)                      t = b - A_N x_N                                 (k_resync_gather / _part / _rhs)
    resync(W, A_N, x_N, b, x_B_old)       cand = W t, the two maxima, the adoption        (k_resync_xb / _apply)
    dual_point(W, A, c, b, kinds, ...)    y, d = c - A^T y, labels, x_N, x_B              (the three together + k_dual_rephase)
    phase1_rhs(A, x, b)                   b~ = b - A x of the device-made primal phase 1  (the front of the resync again)

in extended precision, each with a componentwise bound on what ANY f64 evaluation of it may differ from the model by:
whatever the order of the additions, tree or serial, in tiles or not, fused or not (Higham, Accuracy and Stability of
Numerical Algorithms, §3.1: a dot product of k products has the relative error gamma_k = k u / (1 - k u) on sum |x||y|,
u = 2^-53), plus one u per scalar operation on what it inherits.  A term that is exactly zero (the padding up to ld, a
skipped c_B[i] == 0 or x_N[j] == 0) and a zero initial accumulator add nothing.

    btran   du    = gamma_m |W|^T |c_B|
    drift   dt    = gamma_m |A_B| |d|          r_i = sgn t_i - q_i:  dr_i = dt_i + u (|r_i| + dt_i)
            dres  = max dr                     (|max x^ - max x| <= max dx);   scale = max|q| is exact
            drel  = dres / scale + u (rel + dres / scale)
    rhs     ds    = gamma_nN |A_N| |x_N|       dt = ds + u (|t| + ds)
    resync  dcand = |W| dt + gamma_m |W| (|t| + dt)
            diff_i = |cand_i - x_i|:  ddiff_i = dcand_i + u (diff_i + dcand_i);   max|x_B| is exact
            threshold 1e-11 (1 + max|x_B|): two roundings, dthr = thr ((1 + u)^2 - 1)
            adopted: max diff > threshold; None ("undecided") where the two are within ddiff + dthr of each other
    dual_point
            y = btran;  d_i = c_i - a_i . y:  e_i = |a_i| . dy + gamma_m |a_i| . (|y| + dy),  dd_i = e_i + u (|d_i| + e_i)
            labels and nonbasic values by the rules of dual_rephase_body; a nonbasic variable is undecided where a
            comparison the kernel makes with d_i (against 0, or against +-eps) has its two sides within dd_i
            x_B = the cand of resync with those x_N (forced: adopted whatever the difference)

Nothing in the bounds is measured and they carry no factor.  The arithmetic is that of tests/refresh_model.py (np.longdouble
where it is the x87 80-bit format, double-double elsewhere); the bounds are sums of non-negative terms in np.longdouble.
Values come back as np.longdouble arrays (an f64 array compares with them without a rounding of the model in between).

The second half of the module makes the inputs of tests/test_gpu_maint.py (numpy only, made once and shared), so that
tests/test_maint_model_cpu.py can check them, and the checker, without a device."""
import functools
from types import SimpleNamespace

import numpy as np

import refresh_model as rm

U = rm.U
L = np.longdouble
FREE, LOWER, UPPER, TWOSIDED, FIXED = 0, 1, 2, 3, 4  # ellp_bound_kind (include/ellp_hip.h)
NB_LOWER, NB_UPPER, NB_FREE = 0, 1, 2                # ellp_nb_label


def _arith(arith):
    return arith or (rm._Wide if rm.LONGDOUBLE_IS_WIDE else rm._DD)


def _gamma(k):
    return L(k) * L(U) / (L(1) - L(k) * L(U))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _matvec(ar, A, xw):
    """A (f64, r x k) times the wide vector xw (k x 1), as np.longdouble of length r"""
    return ar.to_longdouble(ar.matmul(_f64(A), xw)).reshape(-1)


def _col(ar, v):
    return ar.lift(_f64(v).reshape(-1, 1))


def _ro(ns):
    for v in vars(ns).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ns


def _btran_wide(ar, W, c_B):
    return ar.matmul(np.ascontiguousarray(_f64(W).T), _col(ar, c_B))


def btran(W, c_B, arith=None):
    """u_j = sum_i c_B[i] W[i, j]"""
    ar = _arith(arith)
    W, c_B = _f64(W), _f64(c_B)
    m = W.shape[0]
    assert W.shape == (m, m) and c_B.shape == (m,)
    u = ar.to_longdouble(_btran_wide(ar, W, c_B)).reshape(-1)
    du = _gamma(m) * (np.abs(W).astype(L).T @ np.abs(c_B).astype(L))
    return _ro(SimpleNamespace(u=u, du=du))


def drift(A_B, d, a_q, sgn, arith=None):
    """the drift monitor: t = A_B d, res = max|sgn t - a_q|, scale = max|a_q| (1 where that is 0), rel = res / scale"""
    ar = _arith(arith)
    A_B, d, q = _f64(A_B), _f64(d), _f64(a_q).astype(L)
    m = A_B.shape[0]
    assert A_B.shape == (m, m) and d.shape == (m,) and q.shape == (m,) and sgn in (-1.0, 1.0)
    t = _matvec(ar, A_B, _col(ar, d))
    dt = _gamma(m) * (np.abs(A_B).astype(L) @ np.abs(d).astype(L))
    r = np.abs(L(sgn) * t - q)
    dr = dt + L(U) * (r + dt)
    res, dres = r.max(), dr.max()
    scale = np.abs(q).max()
    if not scale > 0:
        scale = L(1)
    rel = res / scale
    drel = dres / scale + L(U) * (rel + dres / scale)
    return _ro(SimpleNamespace(t=t, dt=dt, res=res, dres=dres, scale=scale, rel=rel, drel=drel))


def _rhs_wide(ar, A_N, x_N, b):
    s_w = ar.matmul(_f64(A_N), _col(ar, x_N))
    return s_w, ar.add(_col(ar, b), ar.neg(s_w))


def rhs(A_N, x_N, b, arith=None):
    """s = A_N x_N (nN products a row), t = b - s"""
    ar = _arith(arith)
    A_N, x_N, b = _f64(A_N), _f64(x_N), _f64(b)
    m, nN = A_N.shape
    assert x_N.shape == (nN,) and b.shape == (m,)
    s_w, t_w = _rhs_wide(ar, A_N, x_N, b)
    s, t = ar.to_longdouble(s_w).reshape(-1), ar.to_longdouble(t_w).reshape(-1)
    ds = _gamma(nN) * (np.abs(A_N).astype(L) @ np.abs(x_N).astype(L))
    dt = ds + L(U) * (np.abs(t) + ds)
    return _ro(SimpleNamespace(s=s, ds=ds, t=t, dt=dt, t_wide=t_w))


def phase1_rhs(A, x, b, arith=None):
    """b~ = b - A x over the structural columns: the right-hand side the artificial columns and values are made from"""
    return rhs(A, x, b, arith)


RESYNC_TOL = 1e-11  # k_resync_apply


def resync(W, A_N, x_N, b, x_B_old, arith=None):
    """cand = W (b - A_N x_N); maxdiff = max|cand - x_B_old|, maxx = max|x_B_old|, thr = 1e-11 (1 + maxx);
    adopt: True / False, None where maxdiff is within its bound of the threshold"""
    ar = _arith(arith)
    W, x_B_old = _f64(W), _f64(x_B_old)
    m = W.shape[0]
    assert W.shape == (m, m) and x_B_old.shape == (m,)
    front = rhs(A_N, x_N, b, ar)
    cand = _matvec(ar, W, front.t_wide)
    aW = np.abs(W).astype(L)
    dcand = aW @ front.dt + _gamma(m) * (aW @ (np.abs(front.t) + front.dt))
    xo = x_B_old.astype(L)
    diff = np.abs(cand - xo)
    ddiff = dcand + L(U) * (diff + dcand)
    maxdiff, dmaxdiff = diff.max(), ddiff.max()
    maxx = np.abs(xo).max()
    thr = L(RESYNC_TOL) * (L(1) + maxx)
    dthr = thr * ((L(1) + L(U)) ** 2 - L(1))
    adopt = None if abs(maxdiff - thr) <= dmaxdiff + dthr else bool(maxdiff > thr)
    return _ro(SimpleNamespace(t=front.t, dt=front.dt, cand=cand, dcand=dcand, maxdiff=maxdiff, dmaxdiff=dmaxdiff, maxx=maxx,
                               thr=thr, dthr=dthr, adopt=adopt))


def dual_point(W, A, c, b, kinds, lb, ub, B, N, phase1, eps=1e-10, arith=None):
    """The start of a dual phase from the inverse W of the basis B (A: m x n by variable, N: the nonbasic variables in the
    engine's order).  y, dy (m); d, dd (n, by variable); labels, x_N, undecided (by nonbasic position); x_B, dx_B (m).
    phase1: DualPhase1::new's labelling (TwoSided and Fixed only), else DualPhase2::from's; panics: nonbasic positions at
    which the kernel's assertion on d fails."""
    ar = _arith(arith)
    W, A, c, b, lb, ub = _f64(W), _f64(A), _f64(c), _f64(b), _f64(lb), _f64(ub)
    B, N = np.asarray(B, dtype=np.int64), np.asarray(N, dtype=np.int64)
    kinds = np.asarray(kinds)
    m, n = A.shape
    assert W.shape == (m, m) and B.shape == (m,)
    y_w = _btran_wide(ar, W, c[B])
    y = ar.to_longdouble(y_w).reshape(-1)
    dy = _gamma(m) * (np.abs(W).astype(L).T @ np.abs(c[B]).astype(L))
    At = np.ascontiguousarray(A.T)
    d = ar.to_longdouble(ar.add(_col(ar, c), ar.neg(ar.matmul(At, y_w)))).reshape(-1)
    aAt = np.abs(At).astype(L)
    e = aAt @ dy + _gamma(m) * (aAt @ (np.abs(y) + dy))
    dd = e + L(U) * (np.abs(d) + e)
    nN = N.size
    labels, x_N = np.zeros(nN, dtype=np.uint8), np.zeros(nN)
    undecided, panics = np.zeros(nN, dtype=bool), np.zeros(nN, dtype=bool)
    for w, j in enumerate(N):
        dj, ej, k = d[j], dd[j], int(kinds[j])
        at_zero, at_p, at_m = abs(dj) <= ej, abs(dj - L(eps)) <= ej, abs(dj + L(eps)) <= ej
        if phase1:
            labels[w] = NB_LOWER if dj >= 0 else NB_UPPER
            undecided[w] = at_zero
            if k == TWOSIDED:
                x_N[w] = lb[j] if dj >= 0 else ub[j]
            elif k == FIXED:
                x_N[w] = lb[j]
            else:
                panics[w] = True
        elif k == FREE:
            labels[w], x_N[w], panics[w], undecided[w] = NB_FREE, 0.0, not abs(dj) < eps, at_p or at_m
        elif k == LOWER:
            labels[w], x_N[w], panics[w], undecided[w] = NB_LOWER, lb[j], not dj > -eps, at_m
        elif k == UPPER:
            labels[w], x_N[w], panics[w], undecided[w] = NB_UPPER, ub[j], not dj < eps, at_p
        elif k == TWOSIDED:
            labels[w], x_N[w], undecided[w] = (NB_LOWER, lb[j], at_zero) if dj >= 0 else (NB_UPPER, ub[j], at_zero)
        else:
            labels[w], x_N[w] = NB_LOWER, lb[j]
    rs = resync(W, A[:, N], x_N, b, np.zeros(m), ar)
    return _ro(SimpleNamespace(y=y, dy=dy, d=d, dd=dd, labels=labels, x_N=x_N, undecided=undecided, panics=panics,
                               x_B=rs.cand, dx_B=rs.dcand))


def worst(dev, model, bound):
    """max over the entries of |dev - model| / bound (0 / 0 counts as 0: an entry that must be, and is, exact)"""
    dev = np.asarray(dev, dtype=np.float64).astype(L).reshape(-1)
    err, bound = np.abs(dev - np.asarray(model, dtype=L).reshape(-1)), np.asarray(bound, dtype=L).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where((err == 0) & (bound == 0), L(0), err / bound)
    return float(np.max(r)) if r.size else 0.0


def outside(dev, model, bound):
    """how many entries of dev lie outside the bound"""
    dev = np.asarray(dev, dtype=np.float64).astype(L).reshape(-1)
    return int((np.abs(dev - np.asarray(model, dtype=L).reshape(-1)) > np.asarray(bound, dtype=L).reshape(-1)).sum())


# ------------------------------------------------------------------------------------------------ the inputs of the GPU tests
def geometry(m):
    """(ld, btran_rows, btran_tiles) as plan_engine sets them (ellp_plan.inc; tests/test_gpu_maint.py compares with engine_plan)"""
    rows = max(8, (m + 63) // 64)
    return (m + 15) // 16 * 16, rows, (m + rows - 1) // rows


# size -> what it is there for (the names of the parametrisation)
SIZES = {1: "1-tile-ragged-m=ld-15", 2: "1-tile-ragged", 16: "2-tiles-m=ld", 17: "3-tiles-ragged-m=ld-15", 64: "8-tiles-m=ld",
         65: "9-tiles-ragged-m=ld-15", 129: "17-tiles-ragged-m=ld-15", 257: "33-tiles-ragged-m=ld-15", 512: "64-tiles-m=ld",
         513: "57-tiles-m=ld-15", 520: "58-tiles-ragged", 1030: "61-tiles-ragged"}
N_NONBASIC = 24  # nonbasic columns of the square cases: fewer than btran_tiles at the larger sizes (empty resync tiles), more at the smaller


def size_id(m):
    return f"{m}-{SIZES[m]}"


def dense_basis(m, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.1, 1.1, size=(m, m)) + np.diag(rng.uniform(0.5, 1.5, size=m))


def conditioned_basis(m, seed):
    """diagonal in (1, 2) plus a dense part of spectral norm about 0.6: |B^-1| |t| stays near |t|, so that the rounding bound
    of the resync's candidate (gamma_m |W| |t|) is far below its threshold 1e-11 (1 + max|x_B|) at every size used (with the
    dense positive basis above, whose inverse cancels, the bound reaches the threshold at 64 rows: nothing could be decided)"""
    rng = np.random.default_rng(seed)
    return np.diag(rng.uniform(1.0, 2.0, size=m)) + rng.uniform(-1.0, 1.0, size=(m, m)) / (2.0 * np.sqrt(m))


C_PATTERNS = ("phase1", "dense")


@functools.lru_cache(maxsize=None)
def btran_case(m, pattern):
    """A = [B | A_N] with the dense block basic, c_B in the phase-1 pattern (mostly zeros: the skip branch; the last row,
    which lies in the ragged tile, carries cost) or all nonzero, and the dense random matrix that stands in for B^-1"""
    rng = np.random.default_rng(7100 + 2 * m + C_PATTERNS.index(pattern))
    Bm = dense_basis(m, 7000 + m)
    A = np.concatenate([Bm, rng.uniform(0.1, 1.1, size=(m, N_NONBASIC))], axis=1)
    n = m + N_NONBASIC
    if pattern == "phase1":
        c_B = np.where((np.arange(m) % 7 == 3) | (np.arange(m) == m - 1), rng.uniform(0.5, 1.5, size=m), 0.0)
    else:
        c_B = rng.uniform(0.1, 1.0, size=m) * rng.choice([-1.0, 1.0], size=m)
    c = np.concatenate([c_B, -np.ones(N_NONBASIC)])
    x0 = rng.uniform(0.5, 1.5, size=m)
    W = rng.uniform(-1.0, 1.0, size=(m, m))
    return _ro(SimpleNamespace(m=m, n=n, A=A, c=c, c_B=c_B, b=Bm @ x0, x=np.concatenate([x0, np.zeros(N_NONBASIC)]),
                               kind=np.full(n, LOWER, dtype=np.uint8), lb=np.zeros(n), ub=np.zeros(n),
                               B=np.arange(m, dtype=np.int64), N=np.arange(m, n, dtype=np.int64),
                               Nb=np.zeros(N_NONBASIC, dtype=np.uint8), W_random=W))


DRIFT_SIZES = (17, 129, 520)
DRIFT_SCALE = 1.0 + 1e-6


@functools.lru_cache(maxsize=None)
def pivot_case(m, dual):
    """An LP that pivots from a dense, well-conditioned basis.  Primal: every nonbasic column is a positive combination of the basic ones (the
    step is bounded), all costs -1 on them (every one is a candidate), nonbasic variables at the lower bound 0, at a nonzero
    lower bound, and TwoSided ones at their upper bound (so that b - A_N x_N has content).  Dual: y and d >= 0.2 chosen, c
    made from them, x_B with negative entries (a leaving row exists)."""
    rng = np.random.default_rng(7300 + 2 * m + int(dual))
    Bm = conditioned_basis(m, 7200 + m)
    nN = N_NONBASIC
    n = m + nN
    A_N = Bm @ rng.uniform(0.1, 1.0, size=(m, nN)) if not dual else rng.uniform(-0.5, 1.1, size=(m, nN))
    A = np.concatenate([Bm, A_N], axis=1)
    kind = np.full(n, LOWER, dtype=np.uint8)
    lb, ub = np.zeros(n), np.zeros(n)
    Nb = np.zeros(nN, dtype=np.uint8)
    x_N = np.zeros(nN)
    for w in range(nN):  # a third at 0 (the skip branch), a third at a nonzero lower bound, a third TwoSided at the upper bound
        if w % 3 == 1:
            lb[m + w] = x_N[w] = 0.25 * (1 + w % 4)
        elif w % 3 == 2 and not dual:
            kind[m + w], ub[m + w], Nb[w], x_N[w] = TWOSIDED, 1.5, NB_UPPER, 1.5
    x0 = rng.uniform(0.5, 1.5, size=m)
    if dual:
        x0[rng.random(m) < 0.3] *= -1.0
        x0[m // 2] = -abs(x0[m // 2])
    b = Bm @ x0 + A_N @ x_N
    if dual:
        y = rng.uniform(-1.0, 1.0, size=m)
        d = np.concatenate([np.zeros(m), rng.uniform(0.2, 1.0, size=nN)])
        c = A.T @ y + d
    else:
        y, d, c = None, None, np.concatenate([np.zeros(m), -np.ones(nN)])
    return _ro(SimpleNamespace(m=m, n=n, A=A, c=c, b=b, x=np.concatenate([x0, x_N]), kind=kind, lb=lb, ub=ub,
                               B=np.arange(m, dtype=np.int64), N=np.arange(m, n, dtype=np.int64), Nb=Nb, y=y, d=d, x_N=x_N,
                               Binv=np.linalg.inv(Bm)))


RESYNC_SIZES = (17, 129, 520)
BOX_SIZES = (17, 64, 65, 257)
MIXED_SIZE = (140, 260)


@functools.lru_cache(maxsize=None)
def box_case(m):
    """a box LP (TwoSided and Fixed, b = 0) with a dense basis and reduced costs of both signs, 0.2 and more from 0: what
    Engine.dual_phase1 starts from"""
    rng = np.random.default_rng(7400 + m)
    nN = m + 7
    n = m + nN
    A = np.concatenate([dense_basis(m, 7500 + m), rng.uniform(-0.5, 1.1, size=(m, nN))], axis=1)
    kind = np.where(np.arange(n) % 5 == 2, FIXED, TWOSIDED).astype(np.uint8)
    lb = np.where(kind == FIXED, 0.0, -1.0)
    ub = np.where(kind == FIXED, 0.0, 1.0)
    y = rng.uniform(-1.0, 1.0, size=m)
    d = np.concatenate([np.zeros(m), rng.uniform(0.2, 1.0, size=nN) * rng.choice([-1.0, 1.0], size=nN)])
    return _ro(SimpleNamespace(m=m, n=n, A=A, c=A.T @ y + d, b=np.zeros(m), kind=kind, lb=lb, ub=ub,
                               B=np.arange(m, dtype=np.int64), N=np.arange(m, n, dtype=np.int64)))


@functools.lru_cache(maxsize=None)
def mixed_case():
    """The LP family of tests/test_gpu_dual_rephase.py::test_dual_rephase_with_upper_bounds_and_free_variables (140 rows, a
    dense matrix in (0.1, 1.1), Lower / Upper / Free variables) with TwoSided ones added, and a well-conditioned basis, dual
    feasible by construction (y and d chosen, c made from them) instead of by a phase-1 solve: Lower d >= 0.2, Upper
    d <= -0.2, TwoSided either sign, Free nonbasic d = 0 up to the rounding of c.  The phase-1 problem the engine is created
    with is the box problem of the same matrix."""
    rng = np.random.default_rng(5)
    m, n = MIXED_SIZE
    A = rng.uniform(0.1, 1.1, size=(m, n))
    A[:, :m] = conditioned_basis(m, 7700)  # with a basis out of the family itself the bound on d reaches eps = 1e-10
    u = rng.random(n)
    kind = np.select([u < 0.45, u < 0.7, u < 0.8], [LOWER, UPPER, FREE], TWOSIDED).astype(np.uint8)
    kind[m + 3] = FREE  # a nonbasic free variable whatever the draw
    lb = np.where(kind == LOWER, 0.5, np.where(kind == TWOSIDED, -1.0, 0.0))
    ub = np.where(kind == UPPER, 2.0, np.where(kind == TWOSIDED, 1.5, 0.0))
    y = rng.uniform(-1.0, 1.0, size=m)
    mag = rng.uniform(0.2, 1.0, size=n)
    d = np.select([kind == LOWER, kind == UPPER, kind == FREE], [mag, -mag, 0.0], mag * rng.choice([-1.0, 1.0], size=n))
    d[:m] = 0.0
    x0 = rng.uniform(0.2, 1.0, size=n)
    return _ro(SimpleNamespace(m=m, n=n, A=A, c=A.T @ y + d, b=A @ x0, kind=kind, lb=lb, ub=ub,
                               B=np.arange(m, dtype=np.int64), N=np.arange(m, n, dtype=np.int64)))


PHASE1_SIZES = ((17, 40), (129, 150), (520, 90))


@functools.lru_cache(maxsize=None)
def phase1_case(m, n):
    """the standard form and nonbasic start Engine.primal_phase1 takes.  Row 0 is all zeros with b = +0.0 and row 1 all zeros
    with b = -0.0: there b~ = b - 0 is exact, +0.0 and -0.0 (f64::signum gives +1 and -1)"""
    rng = np.random.default_rng(7600 + m)
    A = rng.uniform(-0.5, 1.1, size=(m, n))
    kind = np.where(np.arange(n) % 3 == 2, TWOSIDED, LOWER).astype(np.uint8)
    lb = np.where(np.arange(n) % 3 == 1, 0.0, 0.5)
    ub = np.where(kind == TWOSIDED, 2.0, 0.0)
    Nb = np.where((kind == TWOSIDED) & (np.arange(n) % 2 == 1), NB_UPPER, NB_LOWER).astype(np.uint8)
    x = np.where(Nb == NB_UPPER, ub, lb)
    b = A @ rng.uniform(-1.0, 1.0, size=n)
    if m >= 2:
        A[0], A[1] = 0.0, 0.0
        b[0], b[1] = 0.0, -0.0
    return _ro(SimpleNamespace(m=m, n=n, A=A, b=b, kind=kind, lb=lb, ub=ub, x=x, Nb=Nb))

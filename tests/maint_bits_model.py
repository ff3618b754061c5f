"""A model of the periodic maintenance passes of an explicit-inverse engine (ellp_amd/csrc/engine/ellp_engine.hip) that
reproduces each of them BIT FOR BIT: the same operations on the same operands in the same order.  tests/maint_model.py
bounds what any f64 evaluation may differ by; this one pins the evaluation itself, so that the kernels can be reshaped
(when loads are issued, how rows and tiles are spread over threads and workgroups) and shown to compute what they did.

    btran(W, c_B)                    k_btran_part / _reduce       u = B^-T c_B
    drift(A_B, d, a_q, sgn)          k_drift_part / _reduce       DevState::drift
    rhs(A_N, x_N, b)                 k_resync_part / _rhs         t = b - A_N x_N
    resync(W, t, x_B_old, force)     k_resync_xb / _apply         cand = B^-1 t, the two maxima, the adopted x_B

The arithmetic, as the kernels state it:

    tiles       a tiled GEMV folds, per tile of `rows` consecutive indices i (ascending) and per output entry,
                acc = fma(coef[i], M[i], acc) from acc = +0.0; BTRAN and the resync's front skip coef[i] == 0 (so -0.0 too; a
                NaN is not skipped), the drift monitor skips nothing
    fold        s = 0.0; s += partial[t] for t ascending: plain f64 additions
    wave_sum    v += shfl_xor(v, o) for o = 32, 16, 8, 4, 2, 1 over the 64 lanes (every lane ends with the same bits)
    k_resync_xb lane l of a row's wave folds acc0 / acc1 = fma(W[i][2t], tv[2t], acc0) / fma(W[i][2t+1], tv[2t+1], acc1) over
                t = l, l + 64, ... < ld / 2, the padding up to ld being zeros; cand = wave_sum(acc0 + acc1)
    maxima      exact in any order; NaN wins (nanmax) in the drift monitor, |cand - x| = NaN counts as +Inf in the resync

An fma is float(Fraction(a) * Fraction(b) + Fraction(c)): one correct rounding of the exact value (`fma`).  `vfma` is the
same thing on arrays without Python-speed rationals: the product exactly as a sum of two doubles (Veltkamp / Dekker), the
three-term sum rounded once by way of rounding to odd (Boldo and Melquiond, Emulation of FMA and correctly rounded sums,
IEEE TC 57(4), 2008, Alg. 5).  It is exact for finite operands whose product neither overflows nor falls below 2^-968; an
entry with a non-finite operand gets a * b + c, which has the IEEE special values of an fma.  tests/test_maint_bits_cpu.py
holds vfma against fma.  Numpy only."""
from fractions import Fraction

import numpy as np

from maint_model import geometry

WAVE = 64


def fma(a, b, c):
    """correctly rounded a * b + c of three finite doubles"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _split(a):
    t = 134217729.0 * a  # 2^27 + 1
    hi = t - (t - a)
    return hi, a - hi


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def vfma(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    with np.errstate(all="ignore"):
        plain = a * b + c
        ah, al = _split(a)
        bh, bl = _split(b)
        uh = a * b
        ul = ((ah * bh - uh) + ah * bl + al * bh) + al * bl  # uh + ul = a b exactly
        th, tl = _two_sum(c, uh)
        v, e = _two_sum(tl, ul)  # round tl + ul to odd: where it is inexact and v is even, v's neighbour on e's side
        even = (v.view(np.int64) & 1) == 0
        v = np.where((e != 0) & even, np.nextafter(v, np.where(e > 0, np.inf, -np.inf)), v)
        z = th + v
    ok = np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & np.isfinite(z)
    return np.where(ok, z, plain)


def nanmax(a, b):
    """the kernels' nanmax: NaN if either is NaN, else the larger"""
    return a if a != a else (b if (b > a or b != b) else a)


def _nanmax_all(v):
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if np.isnan(v).any():
        return float("nan")
    return float(max(0.0, v.max())) if v.size else 0.0


def tile_partials(M, coef, rows, ntiles, skip):
    """partial[t] = the fold of fma(coef[i], M[i], acc) over tile t = [t rows, min((t + 1) rows, K)), i ascending; M is K x R"""
    M, coef = np.asarray(M, dtype=np.float64), np.asarray(coef, dtype=np.float64)
    K, R = M.shape
    out = np.zeros((ntiles, R))
    for t in range(ntiles):
        acc = np.zeros(R)
        for i in range(t * rows, min((t + 1) * rows, K)):
            if skip and not coef[i] != 0.0:
                continue
            acc = vfma(coef[i], M[i], acc)
        out[t] = acc
    return out


def fold(partials):
    s = np.zeros(partials.shape[1])
    with np.errstate(all="ignore"):
        for p in partials:
            s = s + p
    return s


def btran(W, c_B):
    m = W.shape[0]
    _, rows, tiles = geometry(m)
    return fold(tile_partials(W, c_B, rows, tiles, True))


def drift(A_B, d, a_q, sgn):
    """DevState::drift after one check: t = A_B d in tiles of basis columns, res = max|sgn t - a_q|, scale = max|a_q|"""
    m = A_B.shape[0]
    _, rows, tiles = geometry(m)
    t = fold(tile_partials(np.ascontiguousarray(np.asarray(A_B, dtype=np.float64).T), d, rows, tiles, False))
    q = np.asarray(a_q, dtype=np.float64)
    with np.errstate(all="ignore"):
        res = _nanmax_all(np.abs(sgn * t - q))
        scale = _nanmax_all(np.abs(q))
        return float(np.float64(res) / np.float64(scale if scale > 0.0 else 1.0))


def rhs(A_N, x_N, b):
    """t = b - s, s = A_N x_N in btran_tiles tiles of ceil(nN / btran_tiles) columns (the last ones may be empty)"""
    A_N = np.asarray(A_N, dtype=np.float64)
    m, nN = A_N.shape
    _, _, tiles = geometry(m)
    cols = (nN + tiles - 1) // tiles
    s = fold(tile_partials(np.ascontiguousarray(A_N.T), x_N, cols, tiles, True))
    with np.errstate(all="ignore"):
        return np.asarray(b, dtype=np.float64) - s


def wave_sum(v):
    """v: (..., 64); the butterfly of wave_sum, every lane's result"""
    lanes = np.arange(WAVE)
    with np.errstate(all="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[..., lanes ^ o]
    return v


def resync_cand(W, t):
    m = W.shape[0]
    ld = geometry(m)[0]
    half = ld // 2
    Wp, tp = np.zeros((m, ld)), np.zeros(ld)
    Wp[:, :m], tp[:m] = W, t
    acc0, acc1 = np.zeros((m, WAVE)), np.zeros((m, WAVE))
    for s in range((half + WAVE - 1) // WAVE):
        tt = np.arange(WAVE) + s * WAVE
        ok = tt < half
        tc = np.where(ok, tt, 0)
        acc0 = np.where(ok, vfma(Wp[:, 2 * tc], tp[2 * tc], acc0), acc0)
        acc1 = np.where(ok, vfma(Wp[:, 2 * tc + 1], tp[2 * tc + 1], acc1), acc1)
    with np.errstate(all="ignore"):
        return wave_sum(acc0 + acc1)[:, 0].copy()


def resync(W, t, x_B_old, force=False):
    """(cand, maxdiff, maxx, adopt, x_B): k_resync_xb's candidate and maxima, k_resync_apply's decision and what x_B is then"""
    cand = resync_cand(W, t)
    xo = np.asarray(x_B_old, dtype=np.float64)
    with np.errstate(all="ignore"):
        df, ax = np.abs(cand - xo), np.abs(xo)
    df = np.where(np.isnan(df), np.inf, df)
    maxdiff = float(max(0.0, df.max()))
    ax = ax[~np.isnan(ax)]
    maxx = float(max(0.0, ax.max())) if ax.size else 0.0
    thr = float(np.float64(1e-11) * (np.float64(1.0) + np.float64(maxx)))
    adopt = bool(force or (maxdiff > thr and not np.isinf(maxdiff)))
    return cand, maxdiff, maxx, adopt, (cand.copy() if adopt else xo.copy())

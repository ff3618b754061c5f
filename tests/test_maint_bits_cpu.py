"""tests/maint_bits_model.py against closed cases, without a device: its fma against the rational definition, the skip rule,
a NaN, a ragged last tile, the butterfly of wave_sum, and that the order it pins is one that matters (another order gives
other bits on the same data, so a GPU test that compares bits with it can fail)."""
from fractions import Fraction

import numpy as np

import maint_bits_model as bm
import maint_model as mm


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_vfma_is_the_correctly_rounded_fma():
    rng = np.random.default_rng(1)
    a = rng.uniform(-2, 2, 4000) * 2.0 ** rng.integers(-30, 30, 4000)
    b = rng.uniform(-2, 2, 4000) * 2.0 ** rng.integers(-30, 30, 4000)
    c = rng.uniform(-2, 2, 4000) * 2.0 ** rng.integers(-60, 60, 4000)
    c[:1000] = -(a[:1000] * b[:1000])                                   # cancellation: the result is the product's rounding error
    c[1000:1500] = -(a[1000:1500] * b[1000:1500]) * (1 + 2.0 ** -52)
    a[1500:1600], c[1600:1700] = 0.0, 0.0
    # halfway cases: a b = 1 + 2^-53 + 2^-80 exactly needs the low part to break the tie of 1 + 2^-53
    a[1700], b[1700], c[1700] = 1.0 + 2.0 ** -26, 1.0 + 2.0 ** -27, -(2.0 ** -26 + 2.0 ** -27) + 2.0 ** -53
    a[1701], b[1701], c[1701] = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, 2.0 ** -53
    a[1702], b[1702], c[1702] = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30, 2.0 ** -53 + 2.0 ** -60
    want = np.array([bm.fma(x, y, z) for x, y, z in zip(a, b, c)])
    assert np.array_equal(_bits(bm.vfma(a, b, c)), _bits(want))
    assert (want[:1000] != 0).any() and (bm.vfma(a, b, c) != a * b + c).any()  # it is not the two-rounding a * b + c


def test_fma_is_one_rounding():
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30  # a b = 1 - 2^-60: a * b rounds to 1.0, the fma keeps the 2^-60
    assert a * b - 1.0 == 0.0 and bm.fma(a, b, -1.0) == -(2.0 ** -60) == float(bm.vfma(a, b, -1.0))
    assert bm.fma(3.0, 5.0, 7.0) == 22.0 and Fraction(bm.fma(0.1, 0.1, 0.0)) != Fraction(0.1) * Fraction(0.1)


def test_vfma_special_values():
    z = bm.vfma(np.array([np.nan, np.inf, np.inf, 1.0, 0.0]), np.array([1.0, 2.0, 0.0, np.inf, 5.0]),
                np.array([1.0, 1.0, 1.0, -np.inf, -0.0]))
    assert np.isnan(z[0]) and z[1] == np.inf and np.isnan(z[2]) and np.isnan(z[3]) and z[4] == 0.0


def test_skip_rule_and_ragged_last_tile():
    """m = 17: ld 32, 8 rows a tile, 3 tiles of which the last has one row.  A skipped row's content must not matter, not
    even a NaN or an Inf in it (0 * Inf would be NaN); -0.0 is skipped too; a NaN in c_B is not."""
    m = 17
    assert mm.geometry(m) == (32, 8, 3)
    rng = np.random.default_rng(2)
    W = rng.uniform(-1, 1, (m, m))
    c = np.where(np.arange(m) % 3 == 0, rng.uniform(0.5, 1.5, m), 0.0)
    c[4] = -0.0
    c[16] = 0.75  # the ragged tile's only row
    u = bm.btran(W, c)
    W2 = W.copy()
    W2[1], W2[4], W2[5] = np.nan, np.inf, 1e300
    assert np.array_equal(_bits(bm.btran(W2, c)), _bits(u))
    want = np.zeros(m)
    for j in range(m):  # by the definition, with rationals
        s = 0.0
        for t in range(3):
            acc = 0.0
            for i in range(8 * t, min(8 * t + 8, m)):
                if c[i] != 0.0:
                    acc = bm.fma(c[i], W[i, j], acc)
            s = s + acc
        want[j] = s
    assert np.array_equal(_bits(u), _bits(want))
    # the last tile is there: without row 16 the result differs
    c0 = c.copy()
    c0[16] = 0.0
    assert not np.array_equal(_bits(bm.btran(W, c0)), _bits(u))
    cn = c.copy()
    cn[2] = np.nan
    assert np.isnan(bm.btran(W, cn)).all()
    assert np.array_equal(_bits(bm.btran(W, np.zeros(m))), _bits(np.zeros(m)))


def test_the_pinned_order_matters():
    """the same sums in one tile instead of three, or folded in descending tile order, give other bits somewhere: the model
    is the tiling, not just a sum"""
    m = 129
    c = mm.btran_case(m, "dense")
    u = bm.btran(c.W_random, c.c_B)
    one = bm.fold(bm.tile_partials(c.W_random, c.c_B, m, 1, True))
    _, rows, tiles = mm.geometry(m)
    back = bm.fold(bm.tile_partials(c.W_random, c.c_B, rows, tiles, True)[::-1])
    assert not np.array_equal(_bits(u), _bits(one)) and not np.array_equal(_bits(u), _bits(back))
    assert mm.worst(u, mm.btran(c.W_random, c.c_B).u, mm.btran(c.W_random, c.c_B).du) <= 1.0  # and it is a BTRAN


def test_wave_sum_is_the_butterfly():
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, 64) * 2.0 ** rng.integers(-20, 20, 64)
    w = list(v)
    for o in (32, 16, 8, 4, 2, 1):
        w = [w[l] + w[l ^ o] for l in range(64)]
    got = bm.wave_sum(v[None, :])[0]
    assert np.array_equal(_bits(got), _bits(np.array(w))) and len(set(_bits(got).tolist())) == 1
    assert got[0] != float(np.sum(v[::-1])) or got[0] != float(sum(v))  # not a serial sum


def test_drift_nan_wins_and_inf():
    m = 17
    c = mm.pivot_case(m, False)
    A_B = c.A[:, c.B]
    d = np.linspace(-1.0, 1.0, m)
    a_q = c.A[:, c.N[0]]
    rel = bm.drift(A_B, d, a_q, 1.0)
    wide = mm.drift(A_B, d, a_q, 1.0)
    assert abs(np.longdouble(rel) - wide.rel) <= wide.drel
    dn = d.copy()
    dn[5] = np.nan
    assert np.isnan(bm.drift(A_B, dn, a_q, 1.0))
    di = d.copy()
    di[5] = np.inf
    assert np.isposinf(bm.drift(A_B, di, a_q, 1.0))
    assert bm.drift(A_B, np.zeros(m), np.zeros(m), 1.0) == 0.0  # scale 0: divided by 1
    assert np.isnan(bm.nanmax(np.nan, 1.0)) and np.isnan(bm.nanmax(1.0, np.nan)) and bm.nanmax(1.0, 2.0) == 2.0


def test_resync_against_the_wide_model_and_its_rules():
    m = 129
    c = mm.pivot_case(m, False)
    W, A_N, x_N, x_B = c.Binv, c.A[:, c.N], c.x[c.N], c.x[c.B]
    t = bm.rhs(A_N, x_N, c.b)
    wide = mm.resync(W, A_N, x_N, c.b, x_B)
    assert mm.worst(t, wide.t, wide.dt) <= 1.0
    cand, maxdiff, maxx, adopt, x_new = bm.resync(W, t, x_B)
    assert mm.worst(cand, wide.cand, wide.dcand) <= 1.0
    assert maxx == np.abs(x_B).max() and adopt is False and np.array_equal(_bits(x_new), _bits(x_B))
    pushed = x_B.copy()
    pushed[7] += 1e-9
    assert bm.resync(W, t, pushed)[3] is True and np.array_equal(_bits(bm.resync(W, t, pushed)[4]), _bits(cand))
    bad = x_B.copy()
    bad[7] = np.nan  # |cand - x| = NaN counts as +Inf, and +Inf adopts nothing
    _, md, mx, ad, xn = bm.resync(W, t, bad)
    assert np.isposinf(md) and mx == np.abs(np.delete(x_B, 7)).max() and ad is False and np.array_equal(_bits(xn), _bits(bad))
    assert bm.resync(W, t, bad, force=True)[3] is True
    # skipped columns: what stands in a column whose x_N is 0 does not matter
    A2 = A_N.copy()
    A2[:, x_N == 0.0] = np.inf
    assert (x_N == 0.0).any() and np.array_equal(_bits(bm.rhs(A2, x_N, c.b)), _bits(t))

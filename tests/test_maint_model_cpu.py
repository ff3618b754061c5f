"""The checker of tests/test_gpu_maint.py, checked without a GPU: the extended-precision model of BTRAN, the drift
monitor, the resync of x_B and the dual start (tests/maint_model.py) must let a correct f64 evaluation through, in
whatever order it adds (BLAS, pairwise, serial from the last term to the first), and must stop the mistakes such kernels
make.  Entries outside the bound on the inputs of this module, of all entries (u: BTRAN with the all-nonzero c_B; cand:
the resync's candidate; rel: the drift, one number, as |rel' - rel| / drel):

    mistake                                        seen in   m=1   2    15    16    17     64     65     129     257     520
    last tile dropped                              u         1/1  2/2 15/15 16/16 17/17  64/64  65/65 129/129 257/257 520/520
    tile 0 counted twice                           u         1/1  2/2 15/15 16/16 17/17  64/64  65/65 129/129 257/257 520/520
    a row with c_B[i] != 0 skipped                 u         1/1  2/2 15/15 16/16 17/17  64/64  65/65 129/129 257/257 520/520
    last element before the ld padding omitted     cand      1/1  2/2 15/15 16/16 17/17  64/64  65/65 129/129 257/257 520/520
    b + s for b - s                                cand      1/1  2/2 15/15 16/16 17/17  64/64  65/65 129/129 257/257 520/520
    W transposed in cand                           cand       -   2/2 15/15 16/16 17/17  64/64  65/65 129/129 257/257 520/520
    sgn flipped in the drift                       rel       every size: |rel' - rel| / drel from 1.4e13 (m=520) to 1.8e16 (m=1)

(test_seeded_mistakes_land_outside prints the counts and asserts them: every entry, since the matrices are dense.)  And
the inputs of the GPU tests are such that the model decides every label and every adoption: a condition on the inputs,
asserted here."""
import numpy as np
import pytest

import maint_model as mm

L = np.longdouble
ROWS = [1, 2, 15, 16, 17, 64, 65, 129, 257, 520]


def _pairwise(P):
    """sum over axis 1 by halving"""
    while P.shape[1] > 1:
        if P.shape[1] % 2:
            P = np.concatenate([P, np.zeros((P.shape[0], 1))], axis=1)
        P = P[:, 0::2] + P[:, 1::2]
    return P[:, 0]


def _reversed(M, v):
    acc = np.zeros(M.shape[0])
    for k in range(M.shape[1] - 1, -1, -1):
        acc = acc + M[:, k] * v[k]
    return acc


ORDERS = {"blas": lambda M, v: M @ v, "pairwise": lambda M, v: _pairwise(M * v[None, :]), "reversed": _reversed}


def _tiled(M, v, tiles, twice=None):
    """sum over the column tiles [k0, k1) of M[:, k0:k1] @ v[k0:k1]; `twice`: that tile is added once more"""
    acc = np.zeros(M.shape[0])
    for t, (k0, k1) in enumerate(tiles):
        part = M[:, k0:k1] @ v[k0:k1]
        acc = acc + part
        if t == twice:
            acc = acc + part
    return acc


def _tiles(m):
    _, rows, nt = mm.geometry(m)
    return [(t * rows, min(m, (t + 1) * rows)) for t in range(nt)]


def _inputs(m):
    """one set of inputs per size: the BTRAN cases, and the primal pivot case with its exact-in-f64 inverse"""
    p = mm.pivot_case(m, False)
    W = p.Binv
    A_N = p.A[:, p.N]
    return p, W, A_N


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("m", ROWS)
def test_plain_f64_is_inside_every_bound(m, order):
    mv = ORDERS[order]
    out = {}
    for pat in mm.C_PATTERNS:
        c = mm.btran_case(m, pat)
        mdl = mm.btran(c.W_random, c.c_B)
        assert (mdl.du > 0).all()
        out[f"u/{pat}"] = mm.worst(mv(np.ascontiguousarray(c.W_random.T), c.c_B), mdl.u, mdl.du)
    p, W, A_N = _inputs(m)
    # drift: d as an FTRAN with a slightly wrong inverse gives it (entering at its lower bound: d = -alpha)
    a_q = A_N[:, 3]
    d = -((W * mm.DRIFT_SCALE) @ a_q)
    dm = mm.drift(p.A[:, p.B], d, a_q, -1.0)
    t64 = mv(p.A[:, p.B], d)
    out["t"] = mm.worst(t64, dm.t, dm.dt)
    rel64 = np.abs(-t64 - a_q).max() / np.abs(a_q).max()
    out["rel"] = float(abs(L(rel64) - dm.rel) / dm.drel)
    assert 0.9e-6 < float(dm.rel) < 1.1e-6 and float(dm.drel) < 1e-12
    # resync
    x_old = p.x[p.B]
    rs = mm.resync(W, A_N, p.x_N, p.b, x_old)
    s64 = mv(A_N, p.x_N)
    t64 = p.b - s64
    out["t_rhs"] = mm.worst(t64, rs.t, rs.dt)
    cand64 = mv(W, t64)
    out["cand"] = mm.worst(cand64, rs.cand, rs.dcand)
    md64 = np.abs(cand64 - x_old).max()
    out["maxdiff"] = float(abs(L(md64) - rs.maxdiff) / rs.dmaxdiff)
    assert float(rs.maxx) == np.abs(x_old).max() and rs.adopt is False
    # dual start: y, d, x_B
    bx = mm.box_case(m) if m >= 2 else None
    if bx is not None:
        Wb = np.linalg.inv(bx.A[:, bx.B])
        dp = mm.dual_point(Wb, bx.A, bx.c, bx.b, bx.kind, bx.lb, bx.ub, bx.B, bx.N, True)
        y64 = mv(np.ascontiguousarray(Wb.T), bx.c[bx.B])
        out["y"] = mm.worst(y64, dp.y, dp.dy)
        d64 = bx.c - mv(np.ascontiguousarray(bx.A.T), y64)
        out["d"] = mm.worst(d64, dp.d, dp.dd)
        out["d_basic"] = mm.worst(d64[bx.B], 0.0 * dp.d[bx.B], dp.dd[bx.B] + np.abs(dp.d[bx.B]))
        xB64 = mv(Wb, bx.b - mv(bx.A[:, bx.N], dp.x_N))
        out["x_B"] = mm.worst(xB64, dp.x_B, dp.dx_B)
    print(f"m={m} {order}: " + ", ".join(f"{k} {v:.3f}" for k, v in out.items()))
    assert all(v <= 1.0 for v in out.values()), out


@pytest.mark.parametrize("m", ROWS)
def test_seeded_mistakes_land_outside(m):
    tiles = _tiles(m)
    c = mm.btran_case(m, "dense")
    Wt = np.ascontiguousarray(c.W_random.T)
    mdl = mm.btran(c.W_random, c.c_B)
    assert mm.outside(_tiled(Wt, c.c_B, tiles), mdl.u, mdl.du) == 0  # the tiled sum itself is inside
    found = {}
    found["last tile dropped"] = mm.outside(_tiled(Wt, c.c_B, tiles[:-1]), mdl.u, mdl.du)
    found["tile 0 counted twice"] = mm.outside(_tiled(Wt, c.c_B, tiles, twice=0), mdl.u, mdl.du)
    skipped = c.c_B.copy()
    skipped[m // 2] = 0.0
    found["a row with c_B[i] != 0 skipped"] = mm.outside(Wt @ skipped, mdl.u, mdl.du)
    p, W, A_N = _inputs(m)
    x_old = p.x[p.B]
    rs = mm.resync(W, A_N, p.x_N, p.b, x_old)
    s64 = A_N @ p.x_N
    t64 = p.b - s64
    found["last element before the ld padding omitted"] = mm.outside(W[:, :m - 1] @ t64[:m - 1], rs.cand, rs.dcand)
    found["b + s for b - s"] = mm.outside(W @ (p.b + s64), rs.cand, rs.dcand)
    if m >= 2:
        found["W transposed in cand"] = mm.outside(W.T @ t64, rs.cand, rs.dcand)
    for name, k in found.items():
        print(f"m={m}: {name}: {k} of {m} entries outside")
        assert k == m, (name, k)
    a_q = A_N[:, 3]
    d = -((W * mm.DRIFT_SCALE) @ a_q)
    dm = mm.drift(p.A[:, p.B], d, a_q, -1.0)
    flipped = np.abs((p.A[:, p.B] @ d) - a_q).max() / np.abs(a_q).max()  # sgn = +1 for -1
    r = float(abs(L(flipped) - dm.rel) / dm.drel)
    print(f"m={m}: sgn flipped in the drift: |rel' - rel| / drel = {r:.3g}")
    assert r > 1e6, r


def test_the_geometry_of_the_sizes_is_what_their_names_say():
    """btran_tiles in {1, fewer than 8, exactly 8, 8k + 1, 64}, a ragged last tile, m = ld and m = ld - 15"""
    geo = {m: mm.geometry(m) for m in mm.SIZES}
    for m, (ld, rows, nt) in geo.items():
        name = mm.SIZES[m]
        assert name.startswith(f"{nt}-tile"), (m, nt, name)
        assert ("ragged" in name) == (rows * nt > m), (m, rows, nt)
        assert ("m=ld-15" in name) == (m == ld - 15) and (name.endswith("m=ld")) == (m == ld), (m, ld)
    tiles = {nt for _, _, nt in geo.values()}
    assert 1 in tiles and 8 in tiles and 64 in tiles and any(1 < t < 8 for t in tiles) and 57 in tiles
    assert any(t > 8 and t % 8 == 1 for t in tiles)
    for m in mm.DRIFT_SIZES + mm.RESYNC_SIZES:
        assert m in mm.SIZES


def test_the_inputs_of_the_gpu_tests_leave_nothing_undecided():
    for m in mm.BOX_SIZES:
        bx = mm.box_case(m)
        dp = mm.dual_point(np.linalg.inv(bx.A[:, bx.B]), bx.A, bx.c, bx.b, bx.kind, bx.lb, bx.ub, bx.B, bx.N, True)
        assert not dp.undecided.any() and not dp.panics.any()
        assert set(np.unique(dp.labels)) == {mm.NB_LOWER, mm.NB_UPPER}
        assert (np.abs(dp.d[bx.N]) > 1e6 * dp.dd[bx.N]).all()
    mx = mm.mixed_case()
    dp = mm.dual_point(np.linalg.inv(mx.A[:, mx.B]), mx.A, mx.c, mx.b, mx.kind, mx.lb, mx.ub, mx.B, mx.N, False)
    assert not dp.undecided.any() and not dp.panics.any()
    assert set(np.unique(dp.labels)) == {mm.NB_LOWER, mm.NB_UPPER, mm.NB_FREE}
    assert set(np.unique(mx.kind[mx.N])) == {mm.FREE, mm.LOWER, mm.UPPER, mm.TWOSIDED}
    for dual in (False, True):
        for m in mm.RESYNC_SIZES:
            p = mm.pivot_case(m, dual)
            x_B = p.x[p.B]
            assert (p.x_N == 0).any() and (p.x_N != 0).any()
            scale = 1.0 + np.abs(x_B).max()
            for delta, adopt in ((0.0, False), (0.5e-11 * scale, False), (2e-11 * scale, True)):
                x_old = x_B.copy()
                x_old[m // 3] += delta
                rs = mm.resync(p.Binv, p.A[:, p.N], p.x_N, p.b, x_old)
                assert rs.adopt is adopt, (m, dual, delta, rs.maxdiff, rs.thr)
            rs = mm.resync(p.Binv, p.A[:, p.N], p.x_N, p.b, x_B)
            assert rs.maxdiff <= 0.1e-11 * scale
    for m, n in mm.PHASE1_SIZES:
        c = mm.phase1_case(m, n)
        r = mm.phase1_rhs(c.A, c.x, c.b)
        assert r.t[0] == 0 and not np.signbit(np.float64(r.t[0])) and r.dt[0] == 0
        assert r.t[1] == 0 and np.signbit(c.b[1]) and r.dt[1] == 0
        assert (np.abs(r.t[2:]) > 1e6 * r.dt[2:]).all()  # the sign of every other b~_i is decided
        assert (c.x == 0).any() and (c.x != 0).any()


@pytest.mark.parametrize("m", [1, 2, 17, 129])
def test_double_double_model_agrees_with_the_long_double_model(m):
    if not mm.rm.LONGDOUBLE_IS_WIDE:
        pytest.skip("np.longdouble is no wider than f64 here: there is nothing to compare the double-double model with")
    c = mm.btran_case(m, "dense")
    a, b = mm.btran(c.W_random, c.c_B), mm.btran(c.W_random, c.c_B, arith=mm.rm._DD)
    assert (np.abs(a.u - b.u) <= a.du / 256).all()
    p, W, A_N = _inputs(m)
    a, b = mm.resync(W, A_N, p.x_N, p.b, p.x[p.B]), mm.resync(W, A_N, p.x_N, p.b, p.x[p.B], arith=mm.rm._DD)
    assert (np.abs(a.cand - b.cand) <= a.dcand / 256).all() and (np.abs(a.t - b.t) <= a.dt / 256).all()

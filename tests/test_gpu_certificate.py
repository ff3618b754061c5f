"""ellp_certificate / ellp_engine_certificate on the device against tests/cert_model.py.

THE EXACT FAMILY (cert_model.exact_instance): every alpha_ij, d_j and x_i is a small integer (or, in the at-eps cases, a
multiple of 2^-20), exact in f64 in any summation order.  There source, qualifying, found, the vector and every reported number
equal the model's exactly.  Shapes (m, n_N): (3, 4); (128, 128); (129, 130): two row blocks and two column blocks of the
tableau pass with ragged edges; (130, 257); (513, 40): the second row tile of the compensated pass.  Planted: two qualifying
rows / columns in different lanes, v slots, waves and blocks (the smallest position must win); one entry that takes the only
qualifying row / column away, in the last ragged row / column; an entry of exactly +-eps; nothing qualifying (found == 0, vec
untouched); a NaN in A_N, in c_N (d's input), in b and in x: ELLP_ERR_NAN, outputs untouched.

GENERAL DENSE INSTANCES (the same plan on a random dense basis with real entries; 20, 77 and 200 rows): the chosen index is not
asserted, only the proof, in exact rationals on the returned f64 vector.  Farkas: gap > 0 and dir_violation <= eps
max(1, max |y|).  Ray: c . r < 0, bound_dir_violation <= eps max |r|, and the componentwise backward error of r_B as a solution of
A_B z = a_q within what tests/test_gpu_start.py asserts of the warm start's x_B (the same refinement and stop rule): omega <= 2u
reported there and |reported - exact| <= omega (3u + 2 gamma_{m+1}) + 2 gamma_{K_r}^2 + u, so exact omega <= 2u + that.  eps is
ellp_opts.eps: the loops treat smaller entries as zero, so no certificate from their bases can promise more.

On the same instances (and on the cost-based vector of one of them) every reported number is held to the exact one of the
returned vector: y . b, c . r and the residual within u |exact| + gamma_K^2 S (postsolve_model.entry_bound) with K the chain
lengths of the launch geometry, no slack factor; sup and gap within that plus what the rounding of z = A^T y itself (the pass's
own entry bound) can move them, derived in _check_farkas_numbers; the maxima that take no arithmetic exactly.

STATE AND REPEATABILITY: two calls give the same bits; the host-memory form and the engine form give the same bits; after a
call on an engine that has run (one of them with an iteration of the two-launch pipeline left open), its taps and read_point
are what they were before."""
import os
import sys
from fractions import Fraction
from functools import lru_cache

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cert_model as CM  # noqa: E402
import postsolve_model as PM  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
EPS2 = 2.0 ** -20
SHAPES = [(3, 4), (128, 128), (129, 130), (130, 257), (513, 40)]
NUMBERS = ("gap", "y_b", "sup", "dir_violation", "residual", "c_r", "bound_dir_violation", "norm")


def _E():
    from ellp_amd import _engine as E
    return E


def _fp(inst):
    E = _E()
    return E.FlatProblem(inst["m"], inst["n"], inst["n"], np.asfortranarray(inst["A"]).reshape(-1, order="F"), inst["c"], inst["b"],
                         inst["kind"], inst["lb"], inst["ub"], inst["x"].copy(), inst["B"].copy(), inst["N"].copy(), inst["Nb"].copy())


def _opts(eps=None):
    o = _E().default_opts()
    if eps is not None:
        o.eps = eps
    return o


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_info(a, b):
    return all((_bits([a[k]]) == _bits([b[k]])).all() if isinstance(a[k], float) else a[k] == b[k] for k in a)


def _farkas_rows(m):
    return {m - 1: CM.NB_UPPER, m // 2: CM.NB_LOWER}


def _ray_cols(nN):
    return {nN - 1: CM.NB_FREE, nN // 2: CM.NB_UPPER}


@pytest.mark.parametrize("m,nN", SHAPES)
def test_exact_family_farkas_row(m, nN):
    E = _E()
    inst = CM.farkas_family(m, nN, _farkas_rows(m), 11 + m)
    B = inst["B"]
    first, count, side, nan = CM.farkas_row_search(inst["T"], inst["x"][B], inst["kind"][B], inst["lb"][B], inst["ub"][B], inst["Nb"], 1e-10)
    assert (first, count, nan) == (m // 2, 2, False)
    fp = _fp(inst)
    fp.x[B] = 99.0  # x_B is recomputed from b and the labels: what the point holds there is not read
    vec, info = E.certificate(fp, E.CERT_FARKAS_ROW)
    assert info["kind"] == "farkas" and info["found"] == 1 and info["source"] == first and info["qualifying"] == count, info
    want = (-1.0 if side == CM.NB_LOWER else 1.0) * inst["W"][first]
    assert (_bits(vec + 0.0) == _bits(want + 0.0)).all()
    k = CM.farkas_check(inst, vec)
    assert k["gap"] == 3 and k["dir_violation"] == 0  # the violation of the row
    assert info["gap"] == 3.0 and info["dir_violation"] == 0.0 and info["worst_dir_var"] == -1 and info["refine_steps"] == 0
    assert Fraction(info["y_b"]) == k["y_b"] and Fraction(info["sup"]) == k["sup"] and Fraction(info["norm"]) == k["norm"]
    vec2, info2 = E.certificate(fp, E.CERT_FARKAS_ROW)
    assert (_bits(vec) == _bits(vec2)).all() and _same_info(info, info2)


@pytest.mark.parametrize("m,nN", SHAPES)
def test_exact_family_ray_column(m, nN):
    E = _E()
    inst = CM.ray_family(m, nN, _ray_cols(nN), 21 + m)
    B, N = inst["B"], inst["N"]
    d = inst["c"] - inst["A"].T @ inst["y"]
    first, count, up, nan = CM.ray_search(inst["T"], d[N], inst["Nb"], inst["kind"][N], inst["x"][B], inst["kind"][B], inst["lb"][B],
                                          inst["ub"][B], 1e-10)
    assert (first, count, up, nan) == (nN // 2, 2, False, False)
    vec, info = E.certificate(_fp(inst), E.CERT_RAY_COLUMN)
    assert info["kind"] == "ray" and info["found"] == 1 and info["source"] == first and info["qualifying"] == count, info
    want = np.zeros(inst["n"])
    want[N[first]], want[B] = -1.0, inst["T"][:, first]
    assert (_bits(vec + 0.0) == _bits(want + 0.0)).all()
    k = CM.ray_check(inst, vec)
    assert k["c_r"] == -2 and k["residual"] == 0 and k["bound_dir_violation"] == 0
    assert info["c_r"] == -2.0 and info["residual"] == 0.0 and info["bound_dir_violation"] == 0.0 and info["refine_steps"] == 0
    assert info["worst_row"] == -1 and info["worst_bound_var"] == -1 and Fraction(info["norm"]) == k["norm"]
    # the other planted column alone: a Free label with d < 0 steps up
    inst = CM.ray_family(m, nN, {nN - 1: CM.NB_FREE}, 21 + m)
    vec, info = E.certificate(_fp(inst), E.CERT_RAY_COLUMN)
    assert info["found"] == 1 and info["source"] == nN - 1 and info["qualifying"] == 1 and vec[nN - 1] == 1.0 and info["c_r"] == -2.0
    assert (vec[inst["B"]] == -inst["T"][:, nN - 1]).all()


@pytest.mark.parametrize("m,nN", SHAPES)
def test_exact_family_one_entry_decides(m, nN):
    """the only qualifying row / column is taken away by one entry in the last (ragged) column / row; an entry of exactly eps
    on the deciding side does not pass the strict Farkas filter and does bound a ray's step"""
    E = _E()
    r = m - 1
    marker = np.full(m + nN, 7.0)
    vec, info = E.certificate(_fp(CM.farkas_family(m, nN, {r: CM.NB_LOWER}, 31, blocker=(r, nN - 1))), E.CERT_FARKAS_ROW, vec=marker)
    assert vec is None and info["found"] == 0 and info["qualifying"] == 0 and info["source"] == -1 and info["kind"] == "farkas"
    assert (marker == 7.0).all()
    vec, info = E.certificate(_fp(CM.farkas_family(m, nN, {r: CM.NB_LOWER}, 31, EPS2, at_eps=(r, nN - 1))), E.CERT_FARKAS_ROW, opts=_opts(EPS2))
    assert info["found"] == 1 and info["source"] == r and info["qualifying"] == 1 and info["gap"] > 0
    q = nN - 1
    vec, info = E.certificate(_fp(CM.ray_family(m, nN, {q: CM.NB_LOWER}, 32, blocker=(m - 1, q))), E.CERT_RAY_COLUMN, vec=marker)
    assert vec is None and info["found"] == 0 and info["qualifying"] == 0 and info["source"] == -1 and info["kind"] == "ray"
    assert (marker == 7.0).all()
    vec, info = E.certificate(_fp(CM.ray_family(m, nN, {q: CM.NB_LOWER}, 32, EPS2, at_eps=(m - 1, q))), E.CERT_RAY_COLUMN, opts=_opts(EPS2))
    assert vec is None and info["found"] == 0
    vec, info = E.certificate(_fp(CM.ray_family(m, nN, {q: CM.NB_LOWER}, 32, EPS2)), E.CERT_RAY_COLUMN, opts=_opts(EPS2))
    assert info["found"] == 1 and info["source"] == q and vec[q] == 1.0


def test_farkas_costs_is_the_postsolve_y():
    E = _E()
    inst = CM.farkas_family(129, 130, {5: CM.NB_LOWER}, 41)
    fp = _fp(inst)
    y, d, r, kkt = E.postsolve(fp)
    vec, info = E.certificate(fp, E.CERT_FARKAS_COSTS)
    assert (_bits(vec) == _bits(y)).all() and info["found"] == 1 and info["source"] == -1 and info["qualifying"] == 0
    k = CM.farkas_check(inst, vec)
    assert Fraction(info["gap"]) == k["gap"] and Fraction(info["dir_violation"]) == k["dir_violation"] and info["worst_dir_var"] == k["worst_dir_var"]
    # n_check and chk_*: only the leading columns, against other bounds
    chk = (np.full(4, CM.TWOSIDED, dtype=np.uint8), np.full(4, -1.0), np.full(4, 2.0))
    vec, info = E.certificate(fp, E.CERT_FARKAS_COSTS, n_check=4, chk=chk)
    std = dict(inst, kind=chk[0], lb=chk[1], ub=chk[2])
    k = CM.farkas_check(std, vec)
    assert Fraction(info["gap"]) == k["gap"] and info["dir_violation"] == 0.0


@pytest.mark.parametrize("what", ["A_N", "c_N", "b", "x"])
def test_a_nan_is_an_error_and_writes_nothing(what):
    E = _E()
    m, nN = 129, 130
    for source, inst in ((E.CERT_FARKAS_ROW, CM.farkas_family(m, nN, _farkas_rows(m), 51)), (E.CERT_RAY_COLUMN, CM.ray_family(m, nN, _ray_cols(nN), 52))):
        if (what == "c_N" and source == E.CERT_FARKAS_ROW) or (what == "b" and source == E.CERT_RAY_COLUMN) or \
                (what == "x" and source == E.CERT_FARKAS_ROW):
            continue  # not an input of that search: d is not read by the Farkas search, b and the given x_B not by the other
        if what == "A_N":
            inst["A"][m - 1, nN - 1] = np.nan
        elif what == "c_N":
            inst["c"][nN - 1] = np.nan
        elif what == "b":
            inst["b"][m - 1] = np.nan
        else:
            inst["x"][inst["B"][m - 1]] = np.nan
        marker = np.full(m + nN, 7.0)
        with pytest.raises(E.EllpHipError) as ei:
            E.certificate(_fp(inst), source, vec=marker)
        assert ei.value.status == E.ERR_NAN and (marker == 7.0).all(), (what, source)


def test_a_singular_basis_is_refused():
    E = _E()
    inst = CM.farkas_family(9, 5, {2: CM.NB_LOWER}, 61)
    inst["A"][:, inst["B"][4]] = inst["A"][:, inst["B"][3]]
    marker = np.full(14, 7.0)
    for source in (E.CERT_FARKAS_COSTS, E.CERT_FARKAS_ROW, E.CERT_RAY_COLUMN):
        with pytest.raises(E.EllpHipError) as ei:
            E.certificate(_fp(inst), source, vec=marker)
        assert ei.value.status == E.ERR_SINGULAR and (marker == 7.0).all()


# ---------------------------------------------------------------- general dense instances
@lru_cache(maxsize=None)
def _dense(kind, m, nN):
    E = _E()
    if kind == "farkas":
        inst = CM.farkas_family(m, nN, {m // 3: CM.NB_UPPER, m - 2: CM.NB_LOWER}, 71 + m, dense=True)
        vec, info = E.certificate(_fp(inst), E.CERT_FARKAS_ROW)
    else:
        inst = CM.ray_family(m, nN, {nN // 3: CM.NB_LOWER, nN - 2: CM.NB_UPPER}, 72 + m, dense=True)
        vec, info = E.certificate(_fp(inst), E.CERT_RAY_COLUMN)
    return inst, vec, info


def _k_sum(count):
    """chain length of a compensated sum of k_cert_farkas / k_cert_ray: thread t of 1,024 takes t, t + 1024, .. (one Dot2 step
    each), the tree of post_block_sum (10 merges), the final s + c"""
    return (count + 1023) // 1024 + 10 + 1


def _within(name, got, exact, tol, what):
    err = abs(Fraction(float(got)) - exact)
    print(f"  {name} {what}: reported {float(got):.17g}, exact {float(exact):.17g}, |error| {float(err):.3e}, bound {float(tol):.3e}")
    assert err <= tol, (name, what, float(got), float(exact), float(err), float(tol))


def _check_farkas_numbers(name, inst, y, info, m, nN):
    """Every reported number against the exact one of the returned y.  y . b is one compensated sum of exact products: within
    u |exact| + gamma_K^2 S (postsolve_model.entry_bound, K = _k_sum(m + n), S = sum |y_i b_i|), as stated.  sup and gap are sums
    of z~_v B_v with the device's z~_v = fl(a_v . y), itself within e_v = u |z_v| + gamma_Kd^2 sum |a||y| of the exact z_v (the
    pass, chain K_d); B_v is the bound the sign of z~_v picks.  Where z~_v and z_v differ in sign both are at most e_v in size,
    so term by term |z~_v B~_v - z_v B_v| <= e_v max(|lb_v|, |ub_v|) =: e_v M_v over the bounds the kind has, and a term that moves
    between the sum and dir_violation moves at most that.  With T = sum e_v M_v:  |reported - exact| <= u (|exact| + T) +
    gamma_K^2 (S + T) + T,  S = sum |z_v| M_v (+ sum |y_i b_i| for the gap).  dir_violation is |z~_v| of one v: within max e_v.
    norm is exact."""
    kd, _ = PM.chain_lengths(m, nN)
    A, n = inst["A"], inst["n"]
    yf = [Fraction(float(v)) for v in y]
    nz = [i for i in range(m) if yf[i] != 0]
    T, S_sup, e_max = Fraction(0), Fraction(0), Fraction(0)
    for v in range(n):
        col = [Fraction(float(A[i, v])) for i in nz]
        z = sum((yf[i] * c for i, c in zip(nz, col)), Fraction(0))
        S = sum((abs(yf[i]) * abs(c) for i, c in zip(nz, col)), Fraction(0))
        e = PM.entry_bound(z, S, kd)
        kind = int(inst["kind"][v])
        M = max([abs(Fraction(float(inst["lb"][v])))] * (CM.has_lb(kind) or kind == CM.FIXED) +
                [abs(Fraction(float(inst["ub"][v])))] * (CM.has_ub(kind) and kind != CM.FIXED) + [Fraction(0)])
        T += e * M
        S_sup += abs(z) * M
        e_max = max(e_max, e)
    k = CM.farkas_check(inst, y)
    S_yb = sum((abs(yf[i]) * abs(Fraction(float(inst["b"][i]))) for i in nz), Fraction(0))
    u, g = Fraction(U), Fraction(PM.gamma(_k_sum(m + n))) ** 2
    _within(name, info["y_b"], k["y_b"], PM.entry_bound(k["y_b"], S_yb, _k_sum(m + n)), "y_b")
    _within(name, info["sup"], k["sup"], u * (abs(k["sup"]) + T) + g * (S_sup + T) + T, "sup")
    _within(name, info["gap"], k["gap"], u * (abs(k["gap"]) + T) + g * (S_yb + S_sup + T) + T, "gap")
    _within(name, info["dir_violation"], k["dir_violation"], e_max, "dir_violation")
    assert Fraction(info["norm"]) == k["norm"]
    assert info["residual"] == 0.0 and info["c_r"] == 0.0 and info["bound_dir_violation"] == 0.0  # not a ray's


def _check_ray_numbers(name, inst, r, info, m, nN):
    """residual is max_i |res~_i| with res~_i the pass's compensated -(A r)_i (chain K_r): within max_i (u |exact_i| +
    gamma_Kr^2 sum_j |a_ij r_j|) of the exact maximum.  c . r is one compensated sum of exact products: within u |exact| +
    gamma_K^2 sum |c_j r_j|, K = _k_sum(m + nN).  bound_dir_violation and norm take no arithmetic: exact."""
    _, kr = PM.chain_lengths(m, nN)
    A, n = inst["A"], inst["n"]
    rf = [Fraction(float(v)) for v in r]
    nz = [j for j in range(n) if rf[j] != 0]
    k = CM.ray_check(inst, r)
    tol_res = Fraction(0)
    for i in range(m):
        S = sum((abs(Fraction(float(A[i, j]))) * abs(rf[j]) for j in nz), Fraction(0))
        tol_res = max(tol_res, PM.entry_bound(k["rows"][i], S, kr))
    S_c = sum((abs(Fraction(float(inst["c"][j]))) * abs(rf[j]) for j in nz), Fraction(0))
    _within(name, info["residual"], k["residual"], tol_res, "residual")
    _within(name, info["c_r"], k["c_r"], PM.entry_bound(k["c_r"], S_c, _k_sum(m + nN)), "c_r")
    assert Fraction(info["bound_dir_violation"]) == k["bound_dir_violation"] and Fraction(info["norm"]) == k["norm"]
    assert info["worst_bound_var"] == k["worst_bound_var"]
    assert info["gap"] == 0.0 and info["y_b"] == 0.0 and info["sup"] == 0.0 and info["dir_violation"] == 0.0  # not a Farkas vector's


@pytest.mark.parametrize("m,nN", [(20, 33), (77, 150), (200, 130)])
def test_dense_reported_numbers_are_the_exact_ones_within_the_bound(m, nN):
    inst, y, info = _dense("farkas", m, nN)
    _check_farkas_numbers(f"farkas {m} x {nN}", inst, y, info, m, nN)
    inst, r, info = _dense("ray", m, nN)
    _check_ray_numbers(f"ray {m} x {nN}", inst, r, info, m, nN)
    # the cost-based vector, whose z has no planted signs: every nonbasic d is its own term
    E = _E()
    y, info = E.certificate(_fp(inst), E.CERT_FARKAS_COSTS)
    _check_farkas_numbers(f"costs {m} x {nN}", inst, y, info, m, nN)


@pytest.mark.parametrize("m,nN", [(20, 33), (77, 150), (200, 130)])
def test_dense_farkas_is_a_proof(m, nN):
    inst, y, info = _dense("farkas", m, nN)
    assert info["found"] == 1 and info["qualifying"] >= 1
    k = CM.farkas_check(inst, y)
    print(f"farkas {m} x {nN}: row {info['source']}, gap {float(k['gap']):.6g} (reported {info['gap']:.6g}), dir_violation "
          f"{float(k['dir_violation']):.3e} (reported {info['dir_violation']:.3e}), max |y| {float(k['norm']):.3g}, {info['refine_steps']} steps")
    assert k["gap"] > 0
    assert k["dir_violation"] <= Fraction(1e-10) * max(1, k["norm"])


@pytest.mark.parametrize("m,nN", [(20, 33), (77, 150), (200, 130)])
def test_dense_ray_is_a_proof(m, nN):
    inst, r, info = _dense("ray", m, nN)
    assert info["found"] == 1 and info["qualifying"] >= 1
    k = CM.ray_check(inst, r)
    q = int(info["source"])
    B = inst["B"]
    # componentwise backward error of z = -+r_B as a solution of A_B z = a_q (r_q = +-1: A r = +-(a_q - A_B z))
    A_B, aq, z = np.abs(inst["A"][:, B]), np.abs(inst["A"][:, inst["N"][q]]), np.abs(r[B])
    omega = Fraction(0)
    for i in range(m):
        den = Fraction(float(aq[i])) + sum((Fraction(float(A_B[i, j])) * Fraction(float(z[j])) for j in range(m)), Fraction(0))
        if k["rows"][i] != 0:
            omega = max(omega, abs(k["rows"][i]) / den)
    kd, kr = PM.chain_lengths(m, nN)
    gm, gr = Fraction(PM.gamma(m + 1)), Fraction(PM.gamma(kr))
    tol = omega * (3 * Fraction(U) + 2 * gm) + 2 * gr * gr + Fraction(U)
    print(f"ray {m} x {nN}: column {q}, c.r {float(k['c_r']):.6g} (reported {info['c_r']:.6g}), residual {float(k['residual']):.3e} (reported "
          f"{info['residual']:.3e}), omega {float(omega) / U:.3f} u, bound_dir_violation {float(k['bound_dir_violation']):.3e}, "
          f"{info['refine_steps']} steps")
    assert k["c_r"] < 0
    assert k["bound_dir_violation"] <= Fraction(1e-10) * k["norm"]
    assert omega <= 2 * Fraction(U) + tol


# ---------------------------------------------------------------- state and repeatability
def _taps(eng, fp):
    E = _E()
    out = []
    for what, count in ((E.TAP_U, fp.m), (E.TAP_D, fp.m), (E.TAP_BINV, fp.m * fp.m), (E.TAP_STATE, 12)):
        try:
            out.append(eng.tap(what, count).copy())
        except E.EllpHipError:
            out.append(None)  # an engine without that buffer: before and after alike
    return out


def _vec_bits(v):
    return None if v is None else _bits(v).tolist()


@pytest.mark.parametrize("m,n,pipeline", [(20, 50, 0), (200, 400, 0), (200, 400, 2)])
def test_the_engine_form_gives_the_same_bits_and_touches_nothing(m, n, pipeline):
    """A primal phase-1 engine that HAS run (7 iterations of the synthetic LP; pipeline 2 leaves its last iteration open, and the
    first call completes it as read_point would).  After that first call: the taps, then a second call, then the taps again —
    equal, and at least the state tap was really read; read_point then gives a point on which the host-memory form returns
    the bits of both engine calls."""
    from ellp_amd import synth
    E = _E()
    for source in (E.CERT_FARKAS_ROW, E.CERT_RAY_COLUMN, E.CERT_FARKAS_COSTS):
        f = synth.primal_phase1_flat(20260301, m, n)
        fp = E.FlatProblem(f["m"], f["n"], f["n_c"], f["A"], f["c"], f["b"], f["kind"], f["lb"], f["ub"], f["x"], f["B"], f["N"], f["Nb"])
        n_check = fp.n - fp.m  # the problem's own columns: the artificial ones stand behind them
        eng = E.Engine(E.ENGINE_PRIMAL, fp, E.default_opts(max_iter=None, pipeline=pipeline))
        try:
            s, st, msg = eng.run(7)
            assert s >= 0 and st.iters >= 1, (s, msg)
            vec, info = eng.certificate(source, n_check=n_check)
            before = _taps(eng, fp)
            vec2, info2 = eng.certificate(source, n_check=n_check)
            after = _taps(eng, fp)
            eng.read_point()
            x1, B1 = fp.x.copy(), fp.B.copy()
            eng.read_point()
        finally:
            eng.close()
        assert before[3] is not None and sum(t is not None for t in before) >= 1
        if pipeline == 2:
            assert before[2] is not None  # the explicit inverse of the two-launch engine
        for a, b in zip(before, after):
            assert (a is None and b is None) or (_bits(a) == _bits(b)).all(), source
        assert (_bits(fp.x) == _bits(x1)).all() and (fp.B == B1).all()
        want_vec, want_info = E.certificate(fp, source, n_check=n_check)
        assert _vec_bits(vec) == _vec_bits(vec2) == _vec_bits(want_vec), source
        assert _same_info(info, info2) and _same_info(info, want_info), (source, info, want_info)


def test_the_call_counter_counts_certificate_calls_only():
    E = _E()
    inst = _dense("farkas", 20, 33)[0]
    fp = _fp(inst)
    before = E.certificate_info()["calls"]
    E.postsolve(fp)
    assert E.certificate_info()["calls"] == before
    E.certificate(fp, E.CERT_FARKAS_ROW)
    ci = E.certificate_info()
    assert ci["calls"] == before + 1 and ci["launches"] > 0
    # on the exact family no solve is refined: the launch count is then the same at every n and every m
    counts, rcounts = set(), set()
    for m, nN in SHAPES:
        E.certificate(_fp(CM.farkas_family(m, nN, _farkas_rows(m), 11 + m)), E.CERT_FARKAS_ROW)
        counts.add(E.certificate_info()["launches"])
        E.certificate(_fp(CM.ray_family(m, nN, _ray_cols(nN), 21 + m)), E.CERT_RAY_COLUMN)
        rcounts.add(E.certificate_info()["launches"])
    assert len(counts) == 1 and len(rcounts) == 1, (counts, rcounts)

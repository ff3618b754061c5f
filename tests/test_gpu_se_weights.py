"""The steepest-edge weights of the primal loop (ELLP_FLAG_PRIMAL_STEEPEST_EDGE, ellp_amd/csrc/engine/ellp_se.inc: k_se_init,
k_se_exact_part / _reduce, k_price_se's folded Goldfarb-Reid update, k_se_vreduce and the k_btran GEMV behind it), read
with ELLP_TAP_SE_GAMMA and held entry by entry against the extended-precision model of tests/se_model.py.

Per step: tap W, run(1), tap d and the weights, read_point.  The weights read after step k + 1 must lie within the
derived rounding bound dG (no factor, nothing measured: se_model's docstring) of step(weights read after step k, W
tapped before step k, the columns in step k's position order, q, r, d of step k), and must be the same bits when step k
was a bound flip, and across the phase hand-off.  The exact starts are held to start_perm / start_general in the same way,
and to the definition 1 + |B^-1 a_j|^2 itself within dG plus the first-order effect of the inverse's measured residual:
with R = W B - I, W a = (I + R) x for x = B^-1 a, so |W a|^2 - |x|^2 = 2 x.Rx + |Rx|^2 and, |Rx|_i <= res |x|_1 with
res = inverse_residual() (plus the rounding gamma_m max_i (|W||B|)_i. of that measurement itself),
    | |W a|^2 - |x|^2 |  <=  2 res |x|_1^2 + m res^2 |x|_1^2 .

ELLP_SE_BTRAN=1 forms v = B^-T d with the k_btran_part / _reduce GEMV in place of k_se_vreduce over k_update2's row
blocks: the runs with it here cover, step by step, the path that engines with ld > 4096 must take; an engine of that size
itself (se_vpart = 0 by the plan, 4,097 rows) is held to the definition of the weights over 16 pivots by
tests/test_gpu_large_pivots.py, case primal-p1-4097-se.

Measured on an MI355X, the largest |G_dev - G_model| / dG: exact starts 0.17 (2 x 2; 0.13 and less from 16 rows up); every
update of both phases at 16 / 17 / 39 / 64 / 65 / 70 rows 0.38 / 0.50 / 0.66 / 0.73 / 0.58 / 0.54 (the same with every column
streamed and with the GEMV at 17 and 65 rows); 256 / 260 rows 0.50; across a refresh / a rebuild 0.35 / 0.49; the mixed
pairs 0.72 (start 0.11), the same bits with and without the shortcut; the phase 1 made on the device 0.24.

The largest relative distance from the definition over each whole solve (every step; not asserted, the recurrence cancels),
the device's next to that of a plain f64 numpy recurrence along the same pivots with a fresh inverse per pivot:

    rows   phase 1: device / f64 recurrence     phase 2: device / f64 recurrence
     16        9.4e-15 / 4.4e-14                    2.5e-14 / 2.0e-13
     17        2.6e-14 / 3.2e-14                    1.7e-10 / 7.9e-08
     39        1.0e-11 / 5.6e-10                    1.0e-11 / 5.6e-10
     64        4.0e-07 / 1.4e-09                    9.0e-04 / 6.1e-06
     65        8.0e-06 / 2.7e-07                    1.1e-05 / 1.2e-05
     70        8.1e-10 / 1.1e-06                    1.5e-03 / 2.5e-04

After 10 pivots from an exact start (test_first_ten_pivots_against_the_definition) both are between 4e-15 and 5e-8, the
device at most 1.5 x the recurrence and mostly below it (at the general start itself up to 4 x, at 6e-14)."""
import numpy as np
import pytest

import se_model as sm
from oracle import ellp_oracle as eo
from test_gpu_rebuild import dense_basis_problem

pytestmark = pytest.mark.gpu
L = np.longdouble
SE, DENSE = 4, 1


def _E():
    from ellp_amd import _engine as E
    return E


def _engine(fp, flags=SE, pipeline=1):
    E = _E()
    return E.Engine(E.ENGINE_PRIMAL, fp, E.default_opts(max_iter=None, pipeline=pipeline, refactor_period=1 << 30, flags=flags))


def _gamma(eng):
    return eng.tap(_E().TAP_SE_GAMMA, eng.fp.nN).copy()


def _W(eng):
    m = eng.fp.m
    return eng.tap(_E().TAP_BINV, m * m).reshape(m, m).copy()


def _A(fp):
    return np.ascontiguousarray(fp.A.reshape(fp.n, fp.m).T)


def _same_bits(X, Y):
    return np.array_equal(np.ascontiguousarray(X).view(np.uint64), np.ascontiguousarray(Y).view(np.uint64))


def _inside(G_dev, mdl, what):
    assert np.isfinite(G_dev).all(), what
    ratio = np.abs(G_dev.astype(L) - mdl.G) / mdl.dG
    j = int(np.argmax(ratio))
    assert (ratio <= 1).all(), (what, j, float(ratio[j]), float(G_dev[j]), float(mdl.G[j]), float(mdl.dG[j]))
    return float(ratio[j])


def _against_definition(eng, A, G_dev, mdl, what):
    fp = eng.fp
    m = fp.m
    W = _W(eng)
    Bm = A[:, fp.B]
    res = L(eng.inverse_residual()) + sm._gamma(m) * (np.abs(W).astype(L) @ np.abs(Bm).astype(L)).sum(axis=1).max()
    X = np.linalg.solve(Bm, A[:, fp.N[:fp.nN]])
    x1 = np.abs(X).astype(L).sum(axis=0) * (1 + L(2.0) ** -20)  # |x|_1 from an f64 solve, rounded up
    ref = sm.definition(A, fp.B, fp.N[:fp.nN])
    tol = mdl.dG + 2 * res * x1 * x1 + m * res * res * x1 * x1
    dev = np.abs(G_dev.astype(L) - ref)
    j = int(np.argmax(dev / tol))
    assert (dev <= tol).all(), (what, j, float(dev[j]), float(tol[j]), float(res))


# ---------------------------------------------------------------------------------------------------------------- the tap
def test_tap_is_refused_without_the_flag():
    E = _E()
    fp, _ = dense_basis_problem(5, 1)
    eng = _engine(fp, flags=0)
    try:
        with pytest.raises(E.EllpHipError) as ei:
            eng.tap(E.TAP_SE_GAMMA, fp.nN)
        assert ei.value.status == E.ERR_ARG
    finally:
        eng.close()
    assert E.TAP_SE_GAMMA == 7


# ------------------------------------------------------------------------------------------------------------ exact starts
def _flat(A, m, n, B, N):
    E = _E()
    return E.FlatProblem(m, n, n, np.asfortranarray(A).reshape(-1, order="F"), np.zeros(n), np.ones(m), np.full(n, 1, dtype=np.uint8),
                         np.zeros(n), np.zeros(n), np.zeros(n), np.asarray(B, dtype=np.int64), np.asarray(N, dtype=np.int64),
                         np.zeros(len(N), dtype=np.uint8))


def _perm_problem(m, nN, scale=None, seed=0):
    """basis: m unit columns +-1 (or +-scale) in a random row order; nN dense nonbasic columns, some of them units"""
    rng = np.random.default_rng(1000 * m + nN + seed)
    n = m + nN
    A = np.zeros((m, n))
    vals = rng.choice([-1.0, 1.0], size=m) * (scale or 1.0)
    A[rng.permutation(m), np.arange(m)] = vals
    A[:, m:] = rng.normal(size=(m, nN))
    for j in range(m + 1, n, 5):  # unit columns among the nonbasic ones
        A[:, j] = 0.0
        A[rng.integers(m), j] = -1.0
    return _flat(A, m, n, np.arange(m), np.arange(m, n)), A


@pytest.mark.parametrize("m", [1, 16, 17, 130])
def test_start_at_a_signed_permutation(m):
    for nN in (1, 2, 3, 63, 64, 65, 257):
        fp, A = _perm_problem(m, nN)
        eng = _engine(fp)
        try:
            G = _gamma(eng)
            mdl = sm.start_perm(A[:, fp.N])
            worst = _inside(G, mdl, ("perm", m, nN))
            _against_definition(eng, A, G, mdl, ("perm, definition", m, nN))
        finally:
            eng.close()
        print(f"signed permutation m={m} nN={nN}: max |G_dev - G_model| / dG = {worst:.3f}")


def _general_problem(m, nN):
    if (m, nN) == (1, 1):
        A = np.array([[2.0, -3.0]])  # a 1 x 1 basis with entry 2.0: not +-1, the general path
        return _flat(A, 1, 2, [0], [1]), A
    rng = np.random.default_rng(77 * m + nN)
    _, Bm = dense_basis_problem(m, 500 + m)
    A = np.zeros((m, m + nN))
    A[:, :m] = Bm
    A[:, m:] = rng.uniform(-1.0, 1.0, size=(m, nN))
    for j in range(m + 2, m + nN, 7):
        A[:, j] = 0.0
        A[rng.integers(m), j] = 1.0
    return _flat(A, m, m + nN, np.arange(m), np.arange(m, m + nN)), A


@pytest.mark.parametrize("m,nN", [(1, 1), (2, 3), (17, 5), (63, 65), (64, 64), (65, 63), (130, 257)])
def test_start_at_a_general_basis(m, nN):
    fp, A = _general_problem(m, nN)
    eng = _engine(fp)
    try:
        G = _gamma(eng)
        mdl = sm.start_general(_W(eng), A[:, fp.N])
        worst = _inside(G, mdl, ("general", m, nN))
        _against_definition(eng, A, G, mdl, ("general, definition", m, nN))
    finally:
        eng.close()
    print(f"general basis m={m} nN={nN}: max |G_dev - G_model| / dG = {worst:.3f}")
    assert (G > 1.0).any()


def test_start_at_a_scaled_permutation_takes_the_general_path():
    """units of +-2.5: a permutation for the rebuild's shortcut, not for the weights (1 + |a_j|^2 would be wrong by 2.5^2)"""
    m, nN = 17, 33
    fp, A = _perm_problem(m, nN, scale=2.5)
    eng = _engine(fp)
    try:
        G = _gamma(eng)
        mdl = sm.start_general(_W(eng), A[:, fp.N])
        _inside(G, mdl, "scaled permutation")
        _against_definition(eng, A, G, mdl, "scaled permutation, definition")
    finally:
        eng.close()
    assert np.abs(G - sm.start_perm_f64(A[:, fp.N])).max() > 0.1


# ------------------------------------------------------------------------------------------------------- every step of solves
def _is_signed_perm(Bm):
    nz = Bm != 0.0
    return bool((nz.sum(axis=0) == 1).all() and (nz.sum(axis=1) == 1).all() and (np.abs(Bm[nz]) == 1.0).all())


def _check_start(eng, A, what):
    """the weights of a fresh engine against the creation formula its basis calls for, and against the definition"""
    fp = eng.fp
    G = _gamma(eng)
    A_N = np.ascontiguousarray(A[:, fp.N[:fp.nN]])
    perm = _is_signed_perm(A[:, fp.B])
    mdl = sm.start_perm(A_N) if perm else sm.start_general(_W(eng), A_N)
    worst = _inside(G, mdl, (what, "start"))
    _against_definition(eng, A, G, mdl, (what, "start, definition"))
    return G, mdl, perm, worst


class _Walk:
    """the protocol of the module docstring on one resident engine; carries the weights and the pivot whose update is pending.
    fresh: the engine has just been created: its weights are checked as an exact start (_check_start), and a plain f64
    numpy recurrence (a fresh np.linalg.inv per pivot) is started beside the device's, along the device's own pivots.
    after: the walk of the phase before on the same engine (the recurrence and the sums go on).
    track = t > 0: at every t-th step (and at the phase's last) the device's and the recurrence's relative distance from
    the definition is measured; horizon: the short-horizon assertion over the first 10 pivots (see the test)."""

    def __init__(self, eng, label, fresh=False, after=None, track=0, horizon=False):
        self.eng, self.label = eng, label
        self.A = _A(eng.fp)
        self.pending = None      # (W_old, A_N, q, r, d) of the last pivot, to be applied by the next pricing launch
        self.unknown = False     # the last steps were not watched: adopt the next read
        self.worst, self.flips, self.pivots, self.checked = 0.0, 0, 0, 0
        self.track, self.horizon = track, horizon
        self.dev_max, self.f64_max, self.start_worst = 0.0, 0.0, None
        self.Gf, self.sum_dG, self.horizon_rows = None, L(0), []
        if fresh:
            fp = eng.fp
            self.G, mdl, perm, self.start_worst = _check_start(eng, self.A, label)
            A_N = np.ascontiguousarray(self.A[:, fp.N[:fp.nN]])
            self.Gf = sm.start_perm_f64(A_N) if perm else sm.start_general_f64(np.linalg.inv(self.A[:, fp.B]), A_N)
            self.sum_dG = mdl.dG.max()
        else:
            self.G = _gamma(eng)
            if after is not None:
                self.Gf, self.sum_dG = after.Gf, after.sum_dG

    def expect(self, G_new, what):
        if self.unknown:
            self.unknown = False
        elif self.pending is None:
            assert _same_bits(G_new, self.G), (self.label, what, "the weights moved without a pivot")
        else:
            mdl = sm.step(self.G, *self.pending)
            self.worst = max(self.worst, _inside(G_new, mdl, (self.label, what)))
            self.sum_dG = self.sum_dG + mdl.dG.max()
            self.checked += 1
        self.G, self.pending = G_new, None

    def measure(self, B0, N0, exact):
        """the weights just read belong to (B0, N0): their and the f64 recurrence's distance from the definition"""
        ref = sm.definition(self.A, B0, N0) if exact else sm.definition(self.A, B0, N0, arith=sm._Wide, tol=2.0 ** -40)
        dev = np.abs(self.G.astype(L) - ref)
        f64 = np.abs(self.Gf.astype(L) - ref)
        self.dev_max = max(self.dev_max, float((dev / ref).max()))
        self.f64_max = max(self.f64_max, float((f64 / ref).max()))
        return dev, f64, ref

    def step(self, k):
        """returns the status of run(1)"""
        E, eng, fp = _E(), self.eng, self.eng.fp
        W = _W(eng)
        B0, N0, Nb0 = fp.B.copy(), fp.N[:fp.nN].copy(), fp.Nb[:fp.nN].copy()
        st, _, msg = eng.run(1)
        self.expect(_gamma(eng), k)
        if self.horizon and self.checked <= 10 and self.Gf is not None:
            dev, f64, ref = self.measure(B0, N0, True)
            self.horizon_rows.append((self.checked, float((dev / ref).max()), float((f64 / ref).max())))
            assert dev.max() <= 10 * f64.max() + self.sum_dG, (self.label, k, self.checked, float(dev.max()), float(f64.max()),
                                                                float(self.sum_dG))
        elif self.track and self.Gf is not None and (k % self.track == 0 or st != E.MAXITER):
            self.measure(B0, N0, False)
        if st != E.MAXITER:
            assert st == E.OPTIMAL, (self.label, k, st, msg)
            return st
        d = eng.tap(E.TAP_D, fp.m).copy()
        eng.read_point()
        rr = np.flatnonzero(B0 != fp.B)
        if rr.size:
            qq = np.flatnonzero(N0 != fp.N[:fp.nN])
            assert rr.size == 1 and qq.size == 1, (self.label, k)
            q, r = int(qq[0]), int(rr[0])
            A_N = np.ascontiguousarray(self.A[:, N0])
            self.pending = (W, A_N, q, r, d)
            self.pivots += 1
            if self.Gf is not None:  # the plain recurrence, with a fresh inverse of the basis
                Wf = np.linalg.inv(self.A[:, B0])
                self.Gf = sm.step_f64(self.Gf, Wf, A_N, q, r, Wf @ A_N[:, q])
        else:
            assert (N0 == fp.N[:fp.nN]).all() and (Nb0 != fp.Nb[:fp.nN]).sum() == 1, (self.label, k)
            self.flips += 1
        return st

    def to_the_end(self, limit=300):
        E = _E()
        for k in range(limit):
            if self.step(k) == E.OPTIMAL:
                return k
        raise AssertionError((self.label, "no end within", limit))


def _boxed(rows, table=None):
    seed, m, n = (table or sm.SOLVES)[rows]
    p1, err = eo.primal_phase1(eo.Problem.from_fixture(sm.boxed_lp(seed, m, n)))
    assert p1 is not None and not err
    v = p1.view()
    assert v.m == rows
    E = _E()
    fp = E.FlatProblem(v.m, v.n, v.n_c, v.A, v.c, v.b, v.kind, v.lb, v.ub, v.x, v.B, v.N[:v.nN], v.Nb[:v.nN])
    return p1, v, fp


def _both_phases(rows, flags, label, track=0):
    p1, v, fp = _boxed(rows)
    eng = _engine(fp, flags=flags)
    try:
        w = _Walk(eng, f"{label} rows {rows} phase 1", fresh=True, track=track)
        w.to_the_end()
        eng.read_point()
        assert abs(fp.obj()) < 1e-9
        ov = v.copy()
        ov.x[:], ov.B[:], ov.N[:v.nN], ov.Nb[:v.nN] = fp.x, fp.B, fp.N[:fp.nN], fp.Nb[:fp.nN]
        p1.store_point(ov)
        v2 = eo.primal_phase2(p1).view()
        G1, worst1, steps1 = w.G, w.worst, w.checked
        eng.rephase(v2.c, v2.kind, v2.lb, v2.ub)
        assert _same_bits(_gamma(eng), G1), "the hand-off changed the weights"
        w2 = _Walk(eng, f"{label} rows {rows} phase 2", after=w, track=track)
        w2.to_the_end()
        assert w2.flips >= 1, "phase 2 took no bound flip"
        print(f"{label} rows {rows}: start {w.start_worst:.3f}; phase 1 {steps1} updates, max |G_dev - G_model| / dG = {worst1:.3f}; "
              f"phase 2 {w2.checked} updates, {w2.flips} flips, max {w2.worst:.3f}")
        if track:
            print(f"{label} rows {rows}: largest relative distance from the definition, device / plain f64 recurrence: phase 1 "
                  f"{w.dev_max:.2e} / {w.f64_max:.2e}, phase 2 {w2.dev_max:.2e} / {w2.f64_max:.2e}")
        assert steps1 >= 1 and w2.checked >= 1
    finally:
        eng.close()


@pytest.mark.parametrize("rows", sorted(sm.SOLVES))
def test_every_step_of_both_phases(rows):
    """also measured (not asserted: the recurrence cancels, se_model's docstring): the largest distance from the definition
    over each phase, at every step, the device's next to a plain f64 recurrence's along the same pivots"""
    _both_phases(rows, SE, "default", track=1)


@pytest.mark.parametrize("rows", [17, 65])
def test_every_step_with_every_column_streamed(rows):
    """flags | ELLP_FLAG_DENSE_PRICING: no unit-column shortcut in k_price_se"""
    _both_phases(rows, SE | DENSE, "dense pricing")


@pytest.mark.parametrize("rows", [17, 65])
def test_every_step_with_the_btran_gemv(rows, monkeypatch):
    """ELLP_SE_BTRAN=1: v from k_btran_part / _reduce, the path engines with ld > 4096 take (module docstring)"""
    monkeypatch.setenv("ELLP_SE_BTRAN", "1")
    _both_phases(rows, SE, "btran gemv")


@pytest.mark.parametrize("rows", sorted(sm.BLOCK_EDGES))
def test_row_block_edges_of_the_fold(rows):
    """64 and 65 row blocks of k_update2 under k_se_vreduce: 12 steps, 100 unwatched, 8 more"""
    E = _E()
    _, _, fp = _boxed(rows, sm.BLOCK_EDGES)
    eng = _engine(fp)
    try:
        w = _Walk(eng, f"rows {rows}", fresh=True)
        for k in range(12):
            assert w.step(k) == E.MAXITER
        st, _, msg = eng.run(100)
        assert st == E.MAXITER, msg
        eng.read_point()
        w.unknown = True
        for k in range(112, 121):  # the first read is adopted, 8 updates are checked
            assert w.step(k) == E.MAXITER
        print(f"rows {rows}: {w.checked} updates checked, max |G_dev - G_model| / dG = {w.worst:.3f}")
        assert w.checked >= 16
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- life cycle
@pytest.mark.parametrize("how", ["request_maintenance", "refactor"])
def test_pending_update_survives_maintenance(how):
    """between a pivot and the pricing launch that applies its update, the inverse is refreshed (the launch stops at the
    request first) or rebuilt: the update must still be the one of the pivot that was pending, applied once"""
    E = _E()
    _, _, fp = _boxed(39)
    eng = _engine(fp)
    try:
        w = _Walk(eng, how, fresh=True)
        k = 0
        while k < 8 or w.pending is None:
            assert w.step(k) == E.MAXITER
            k += 1
        c0, checked0, G0 = eng.counters(), w.checked, w.G
        getattr(eng, how)()
        assert _same_bits(_gamma(eng), G0), "the maintenance call itself moved the weights"
        st, stats, msg = eng.run(1)
        assert st == E.MAXITER, msg
        c1 = eng.counters()
        if how == "request_maintenance":  # the pricing launch stopped at the request, the host serviced it, then one loop body ran
            assert c1["maint_requests"] == c0["maint_requests"] + 1 and c1["refreshes"] + c1["rebuilds"] > c0["refreshes"] + c0["rebuilds"]
        else:
            assert c1["rebuilds"] == c0["rebuilds"] + 1
        w.expect(_gamma(eng), "the step after " + how)
        assert w.checked == checked0 + 1  # the pending update, held to the model of the pivot it belongs to: applied, and once
        eng.read_point()
        # the step after that was decided with an inverse that was not tapped: adopt, then go on checking
        w.unknown = True
        for k2 in range(5):
            assert w.step(100 + k2) == E.MAXITER
        print(f"{how}: max |G_dev - G_model| / dG = {w.worst:.3f}")
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------- phase 1 made on the device
def test_phase1_built_on_the_device():
    """Engine.primal_phase1 with the flag: either the engine refuses it (ELLP_ERR_ARG), or its weights at the artificial basis
    it has made itself — a signed permutation — are start_perm's of the standard form's columns, and the first updates follow
    the model"""
    E = _E()
    from test_gpu_phase1_device import _problem
    p1, err = eo.primal_phase1(_problem(40, 90, 47, True))
    assert p1 is not None and not err
    v = p1.view()
    ns = v.n - v.m
    A = np.asarray(v.A).reshape(v.n, v.m)
    opts = E.default_opts(max_iter=None, pipeline=1, refactor_period=1 << 30, flags=SE)
    try:
        eng = E.Engine.primal_phase1(v.m, ns, A[:ns].reshape(-1), v.b, v.kind[:ns], v.lb[:ns], v.ub[:ns], v.x[:ns], v.Nb[:ns], opts)
    except E.EllpHipError as ex:
        assert ex.status == E.ERR_ARG, ex
        return
    try:
        eng.read_point()
        eng.fp.A = np.ascontiguousarray(v.A)  # the host copy the binding does not materialise: the oracle's, same columns
        np.testing.assert_array_equal(eng.fp.N, v.N[:v.nN])
        G = _gamma(eng)
        worst = _inside(G, sm.start_perm(_A(eng.fp)[:, eng.fp.N]), "device-made phase 1")
        w = _Walk(eng, "device-made phase 1")
        for k in range(10):
            assert w.step(k) == E.MAXITER
        print(f"device-made phase 1: start {worst:.3f}, {w.checked} updates, max |G_dev - G_model| / dG = {w.worst:.3f}")
        assert w.checked >= 5
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------ short horizon, the definition
@pytest.mark.parametrize("rows", sorted(sm.SOLVES))
def test_first_ten_pivots_against_the_definition(rows):
    """The guard against a mistake that model and kernel share.  From each exact start — the phase-1 start, and the phase-2
    start of a FRESH engine created at phase 1's end basis (k_se_exact_* on a real basis, nonbasic variables at every kind of
    bound) — after each of the first 10 pivots: max_j |G_dev - definition| <= 10 max_j |G_f64 - definition| + the summed
    max_j dG of the start and the steps so far, G_f64 being the plain numpy recurrence from the same start along the device's
    pivots with a fresh inverse per pivot.  The factor 10 is for an inverse that carries eta-update rounding where the host
    has a fresh one; the mistakes of tests/test_se_model_cpu.py are 12 orders of magnitude away."""
    E = _E()
    p1, v, fp = _boxed(rows)
    eng = _engine(fp)
    try:
        w = _Walk(eng, f"rows {rows} phase-1 start", fresh=True, horizon=True)
        k, st = 0, E.MAXITER
        while w.checked < 10 and st == E.MAXITER:
            st = w.step(k)
            k += 1
        if st == E.MAXITER:
            st, _, msg = eng.run(1 << 20)
            assert st == E.OPTIMAL, msg
        eng.read_point()
    finally:
        eng.close()
    ov = v.copy()
    ov.x[:], ov.B[:], ov.N[:v.nN], ov.Nb[:v.nN] = fp.x, fp.B, fp.N[:fp.nN], fp.Nb[:fp.nN]
    p1.store_point(ov)
    v2 = eo.primal_phase2(p1).view()
    fp2 = E.FlatProblem(v2.m, v2.n, v2.n_c, v2.A, v2.c, v2.b, v2.kind, v2.lb, v2.ub, v2.x, v2.B, v2.N[:v2.nN], v2.Nb[:v2.nN])
    eng2 = _engine(fp2)
    try:
        assert not _is_signed_perm(_A(fp2)[:, fp2.B])
        w2 = _Walk(eng2, f"rows {rows} phase-2 start, fresh engine", fresh=True, horizon=True)
        k, st = 0, E.MAXITER
        while w2.checked < 10 and st == E.MAXITER:  # a phase with fewer pivots: all of them
            st = w2.step(k)
            k += 1
    finally:
        eng2.close()
    assert w.checked >= 10 and w2.checked >= 8
    for ww in (w, w2):
        print(ww.label + ": relative distance from the definition after n pivots, device / f64 recurrence: " +
              ", ".join(f"{n}: {a:.1e} / {b:.1e}" for n, (a, b) in sorted({n: (a, b) for n, a, b in ww.horizon_rows}.items())
                        if n in (0, 1, 5, 10)))


# ------------------------------------------------------------------------------------------------------------------ mixed pairs
def _mixed_pairs_problem():
    """k_price_se takes its columns in pairs only where a block has more than one: cpb = ceil(nN / 1024) columns per block,
    so nN = 2051 gives 3 (684 blocks: a pair and a single each, the last block 2 columns; 2051 is odd and no multiple of 3).
    Nonbasic position 3 b + i: the pair (3 b, 3 b + 1) is unit-unit, unit-dense, dense-unit, dense-dense for b mod 4 = 0, 1,
    2, 3; the single 3 b + 2 is a unit for even b.  Unit columns have one entry 0.5, 1 or 2.5; 20 rows, x >= 0, the slack
    basis feasible at 0, negative costs: bounded, with pivots to make."""
    m, nN = 20, 2051
    rng = np.random.default_rng(31)
    n = m + nN
    A = np.zeros((m, n))
    A[:, :m] = np.eye(m)
    unit = np.zeros(nN, dtype=bool)
    for j in range(nN):
        b, i = divmod(j, 3)
        unit[j] = (b % 4 in (0, 1)) if i == 0 else (b % 4 in (0, 2)) if i == 1 else (b % 2 == 0)
        if unit[j]:
            A[rng.integers(m), m + j] = rng.choice([0.5, 1.0, 2.5])
        else:
            A[:, m + j] = rng.uniform(0.1, 1.1, size=m)
    c = np.concatenate([np.zeros(m), -rng.uniform(0.5, 1.5, size=nN)])
    b = rng.uniform(1.0, 2.0, size=m)
    E = _E()
    x = np.concatenate([b, np.zeros(nN)])
    fp = E.FlatProblem(m, n, n, A.reshape(-1, order="F"), c, b, np.full(n, 1, dtype=np.uint8), np.zeros(n), np.zeros(n), x,
                       np.arange(m, dtype=np.int64), np.arange(m, n, dtype=np.int64), np.zeros(nN, dtype=np.uint8))
    pats = {(bool(unit[3 * k]), bool(unit[3 * k + 1])) for k in range(nN // 3)}
    assert len(pats) == 4 and nN % 2 == 1 and nN % 3 != 0
    return fp


@pytest.mark.parametrize("flags", [SE, SE | DENSE], ids=["shortcut", "streamed"])
def test_mixed_pairs(flags):
    """all four unit / dense pair patterns, the pointer swap of the mixed ones and the odd last column, with the unit-column
    shortcut and with every column streamed: the start and 12 steps"""
    E = _E()
    eng = _engine(_mixed_pairs_problem(), flags=flags)
    try:
        w = _Walk(eng, f"mixed pairs, flags {flags}", fresh=True)
        for k in range(12):
            assert w.step(k) == E.MAXITER
        print(f"mixed pairs, flags {flags}: start {w.start_worst:.3f}, {w.checked} updates, max |G_dev - G_model| / dG = {w.worst:.3f}")
        assert w.checked >= 8
    finally:
        eng.close()

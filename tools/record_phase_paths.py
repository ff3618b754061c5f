"""tools/record_phase_paths.py — what the phase hand-offs of the resident engine decide, path by path, as exact values.

    python tools/record_phase_paths.py [--out tests/golden/phase_paths_parent.json]

Run on the build whose hand-offs are the reference (the commit BEFORE a change to ellp_engine_rephase,
ellp_engine_dual_rephase, the phase-1 constructors, redo_from_snapshot or the re-arms of the certified hybrid that must not
move a decision); tests/test_gpu_phase_paths.py replays the same cases on the current build and compares for equality.  The
cases and the way each is driven are defined here and imported by the test, so that the recording and the replay cannot
drift apart.  The digests and the per-run record are those of tools/record_run_paths.py (imported, not copied).

A two-phase case is: the phase-1 constructor on the device (Engine.primal_phase1 / Engine.dual_phase1), ellp_engine_run,
the hand-off (rephase / dual_rephase), ellp_engine_run.  Its record holds, per phase, the status / iters / pivots /
bound_flips / bits of obj of every run call, the sha256 digests of x, B_index, N_index, N_bound (dual: y and d too) from
ellp_engine_read_point and the host counters of ELLP_TAP_STATE; and the status and message of every hand-off call (0 and ""
where it went through).  The refusals case holds statuses and messages alone.  The recorder refuses a golden in which a
case did not take its path (took_path), or whose two runs differ.

Two cases do not end the way one might expect.  A redo at or below 1,024 rows leaves the hybrid for good (the engine is
the LU-per-iteration kernel from there on), so a forced redo in phase 1 (g) cannot be followed by one in phase 2; g2
forces the redo in phase 2 alone, where it goes back to the snapshot the run behind the rephase took.  And a dual phase 1
stopped after three iterations (k: the exact loop at 1,040 rows needs minutes to finish one) is not dual feasible for
phase 2: dual_rephase makes the point — the branch the case is there for — and the reference's assertion on the sign of d
refuses it; the record holds that status and text, and what the next run call answers.

took_path sees what can be seen from outside: launches per iteration, the hybrid's and the redo's counters, a pivot in
the phase before each hand-off.  Which branch a hand-off took inside is not visible there and no hook is made for it:
whether dual_rephase had to permute the nonbasic columns into variable order (it does whenever phase 1 pivoted, which the
pivot count shows only indirectly), and whether the dual point took y from BTRAN, from k_mid's LU or from the rows-LU (that
follows from the plan: pipeline 1, the hybrid, pipeline 3 above 1,024 rows; the counters show the plan, not the branch)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from record_run_paths import COUNTERS, SEED, TO_END, _bits, _sha, _slice_record, _with_env  # noqa: E402,F401

GOLDEN = os.path.join(ROOT, "tests", "golden", "phase_paths_parent.json")
STEEPEST_EDGE = 4  # ELLP_FLAG_PRIMAL_STEEPEST_EDGE
DUAL_SWAPS = 8     # the dual phase-1 start: the slack basis with this many slacks replaced by structural columns

# name -> kind, m, n (structural columns), engine options, environment (set before creation, kept to the end);
# per_phase: the budget of each phase's one run call (None: to the end)
CASES = {
    # three launches: the plain re-arm
    "a_primal3": dict(kind="primal", m=48, n=120, opts=dict(pipeline=1), env={}),
    # two launches: the lagged fields open, pe_valid, mv_pending
    "b_primal2": dict(kind="primal", m=48, n=120, opts=dict(pipeline=2), env={}),
    # partial pricing: the pp_* window restarts
    "c_primal3_partial4": dict(kind="primal", m=48, n=120, opts=dict(pipeline=1, partial_segments=4), env={}),
    # steepest edge: se_valid
    "d_primal3_steepest_edge": dict(kind="primal", m=48, n=120, opts=dict(pipeline=1, flags=STEEPEST_EDGE), env={}),
    # default options at 48 rows: k_small
    "e_primal_small": dict(kind="primal", m=48, n=120, opts={}, env={}),
    # the certified hybrid: the rephase after a certified phase 1
    "f_primal_hybrid": dict(kind="primal", m=160, n=400, opts={}, env={}),
    # ... a redo in phase 1: from there on the engine is the LU-per-iteration kernel, which the rephase hands on
    "g_primal_hybrid_redo": dict(kind="primal", m=160, n=400, opts={}, env={"ELLP_FORCE_REDO": "1"}),
    # ... a redo in phase 2 alone: it goes back to the start of phase 2, so the rephase has dropped phase 1's snapshot and the
    # run behind it has taken another
    "g2_primal_hybrid_redo_phase2": dict(kind="primal", m=160, n=400, opts={}, env={}, env_phase2={"ELLP_FORCE_REDO": "1"}),
    # dual, three launches: y from BTRAN
    "h_dual3": dict(kind="dual", m=150, n=300, opts=dict(pipeline=1), env={}),
    # dual, the certified hybrid: y and x_B from k_mid's LU
    "i_dual_hybrid": dict(kind="dual", m=150, n=300, opts={}, env={}),
    # dual, k_small: the inverse is built before the point is made; dual_rephase is refused
    "j_dual_small": dict(kind="dual", m=48, n=120, opts={}, env={}),
    # dual, the exact loop above 1,024 rows: y from the rows-LU; three iterations per phase
    "k_dual_exact_large": dict(kind="dual", m=1040, n=1300, opts=dict(pipeline=3), env={}, per_phase=3),
    # what the hand-offs refuse
    "l_refusals": dict(kind="refusals", env={}),
}


def _phase_record(eng, runs, dual):
    fp = eng.read_point()
    cnt = eng.counters()
    rec = {"runs": runs, "closing_status": int(eng.closing_status), "x": _sha(fp.x), "B": _sha(fp.B), "N": _sha(fp.N),
           "Nb": _sha(fp.Nb), "counters": {k: int(cnt[k]) for k in COUNTERS}}
    if dual:
        rec["y"], rec["d"] = _sha(fp.y), _sha(fp.d)
    return rec


def _call(E, fn):
    """(status, message, result) of a constructor or hand-off of the binding, which raises on a refusal"""
    try:
        return 0, "", fn()
    except E.EllpHipError as err:
        return int(err.status), str(err.msg), None


def _primal_start(E, synth, m, n, opts, bad_kind=False):
    f = synth.primal_phase1_flat(SEED, m, n)
    ns = n + m  # the standard form's columns; the engine adds the artificials
    kind = f["kind"][:ns].copy()
    if bad_kind:
        kind[0] = 5
    st, msg, eng = _call(E, lambda: E.Engine.primal_phase1(m, ns, f["A"][:m * ns], f["b"], kind, f["lb"][:ns], f["ub"][:ns],
                                                           f["x"][:ns], f["Nb"], E.default_opts(max_iter=None, **opts)))
    return f, st, msg, eng


def _dual_start(E, synth, m, n, opts, bad_kind=False):
    """the box problem of covering_lp's standard form (dual_problem.rs:98-106: Lower -> TwoSided(0, 1), b = 0) on a basis that
    is not dual feasible for it at the start: the slack basis with DUAL_SWAPS slacks replaced by structural columns"""
    f = synth.dual_start_flat(SEED, m, n)
    nc = f["n"]
    B = f["B"].copy()
    B[:DUAL_SWAPS] = np.arange(DUAL_SWAPS)
    N = np.setdiff1d(np.arange(nc, dtype=np.int64), B)
    kind = np.full(nc, 3, dtype=np.uint8)
    if bad_kind:
        kind[0] = 5
    st, msg, eng = _call(E, lambda: E.Engine.dual_phase1(m, nc, f["A"], f["c"], np.zeros(m), kind, np.zeros(nc), np.ones(nc), B, N,
                                                         E.default_opts(max_iter=None, **opts)))
    return f, st, msg, eng


def _two_phases(E, case):
    from ellp_amd import synth
    dual = case["kind"] == "dual"
    budget = case.get("per_phase") or TO_END
    prof = False
    f, st, msg, eng = (_dual_start if dual else _primal_start)(E, synth, case["m"], case["n"], case["opts"])
    rec = {"create": {"status": st, "message": msg}}
    if eng is None:
        return rec
    try:
        st, stats, _ = eng.run(budget)
        rec["phase1"] = _phase_record(eng, [_slice_record(st, stats, prof)], dual)
        fp = eng.fp
        if dual:
            nc = f["n"]
            st, msg, _ = _call(E, lambda: eng.dual_rephase(f["c"], f["b"], f["kind"], np.zeros(nc), np.zeros(nc)))
        else:
            p2 = synth.primal_phase2_from(f, fp.x, fp.B, fp.N, fp.Nb)
            st, msg, _ = _call(E, lambda: eng.rephase(p2["c"], p2["kind"], p2["lb"], p2["ub"]))
        rec["handoff"] = {"status": st, "message": msg}
        st, stats, _ = _with_env(case.get("env_phase2", {}), lambda: eng.run(budget))  # ELLP_FORCE_REDO is read when a solve ends
        rec["phase2"] = _phase_record(eng, [_slice_record(st, stats, prof)], dual)
    finally:
        eng.close()
    return rec


def _refusals(E):
    from ellp_amd import synth
    rec = {}
    m, n = 48, 120
    # rephase on a dual engine
    f = synth.dual_start_flat(SEED, m, n)
    fp = E.FlatProblem(f["m"], f["n"], f["n_c"], f["A"], f["c"], f["b"], f["kind"], f["lb"], f["ub"], f["x"], f["B"], f["N"],
                       f["Nb"], y=f["y"], d=f["d"])
    eng = E.Engine(E.ENGINE_DUAL, fp, E.default_opts(max_iter=None, pipeline=1))
    try:
        st, msg, _ = _call(E, lambda: eng.rephase(f["c"], f["kind"], f["lb"], f["ub"]))
        rec["rephase_on_a_dual_engine"] = {"status": st, "message": msg}
        bad = f["kind"].copy()
        bad[3] = 5
        st, msg, _ = _call(E, lambda: eng.dual_rephase(f["c"], f["b"], bad, f["lb"], f["ub"]))
        rec["dual_rephase_bound_kind_5"] = {"status": st, "message": msg}
    finally:
        eng.close()
    # a bound_kind of 5 in the primal hand-off and in the two constructors
    f, st, msg, eng = _primal_start(E, synth, m, n, dict(pipeline=1))
    try:
        bad = eng.fp.kind.copy()
        bad[3] = 5
        st, msg, _ = _call(E, lambda: eng.rephase(eng.fp.c, bad, eng.fp.lb, eng.fp.ub))
        rec["rephase_bound_kind_5"] = {"status": st, "message": msg}
    finally:
        eng.close()
    for name, start in (("primal_phase1_bound_kind_5", _primal_start), ("dual_phase1_bound_kind_5", _dual_start)):
        _, st, msg, eng = start(E, synth, m, n, dict(pipeline=1), bad_kind=True)
        if eng is not None:
            eng.close()
        rec[name] = {"status": st, "message": msg}
    return rec


def run_case(E, name):
    """the record of one case; the caller has put CASES[name]["env"] into the environment"""
    case = CASES[name]
    return _refusals(E) if case["kind"] == "refusals" else _two_phases(E, case)


def took_path(E, name, rec):
    """None, or what shows that the case did not take the path it is there for"""
    key = name.split("_")[0]
    if key == "l":
        if any(r["status"] != E.ERR_ARG or not r["message"] for r in rec.values()):
            return "every call refused with ERR_ARG and a message"
        return None
    if rec["create"]["status"] != 0 or "phase2" not in rec:
        return "the phase-1 constructor, both phases run"
    p1, p2, h = rec["phase1"], rec["phase2"], rec["handoff"]
    c1, c2 = p1["counters"], p2["counters"]
    r1, r2 = p1["runs"][-1], p2["runs"][-1]
    if r1["pivots"] < 1:
        return "a pivot in phase 1, before the hand-off"
    # launches_per_iteration is 0 where the loop is the LU-per-iteration kernel (k_small / k_mid: no launch per iteration)
    if key == "j":
        if c1["launches_per_iteration"] != 0 or h["status"] != E.ERR_ARG or not h["message"] or r1["status"] != E.OPTIMAL:
            return "k_small to the optimal end of phase 1, dual_rephase refused with ERR_ARG"
        return None
    if key == "k":
        # A phase 1 stopped after three iterations is not dual feasible for phase 2: the point is made (y from the rows-LU,
        # behind the hand-off's rebuild) and the reference's assertion on the sign of d then refuses it.
        if not (r1["status"] == E.MAXITER and r1["iters"] == 3 and c1["hybrid_exact_iters"] == 3 and h["status"] == E.ERR_PANIC and
                h["message"] and c2["rebuilds"] == c1["rebuilds"] + 1 and c2["resyncs"] == c1["resyncs"] + 1):
            return "three iterations of the exact loop, MaxIter; the point made behind a rebuild, then refused by the assertion on d"
        return None
    if h["status"] != 0:
        return "the hand-off went through"
    if r1["status"] != E.OPTIMAL or r2["status"] != E.OPTIMAL or r2["pivots"] < 1:
        return "both phases to the optimal end, with pivots"
    lpi = c2["launches_per_iteration"]
    if key in "acdh" and lpi != 3:
        return "three launches per iteration"
    if key == "b" and lpi != 2:
        return "two launches per iteration"
    if key == "e" and lpi != 0:
        return "k_small"
    if key in "fi":
        if not c1["hybrid"] or c1["hybrid_certs"] < 1 or c2["hybrid_certs"] <= c1["hybrid_certs"] or c2["hybrid_redos"] != 0:
            return "the hybrid, a certified end of each phase, no redo"
    if key == "g":
        if c1["hybrid_redos"] != 1 or c1["hybrid"] or c2["hybrid_redos"] != 1 or lpi != 0:
            return "a redo in phase 1, the exact kernel alone from there on, through the rephase"
    if key == "g2":
        if not c1["hybrid"] or c1["hybrid_redos"] != 0 or c2["hybrid_redos"] != 1 or c2["hybrid_certs"] <= c1["hybrid_certs"]:
            return "the hybrid through phase 1 and the rephase, a certified end of phase 2, then its redo"
    return None


def main():
    import time
    from ellp_amd import _engine as E
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    gold = {"seed": SEED, "cases": {}}
    bad = []
    for name, case in CASES.items():
        t0 = time.time()
        rec = _with_env(case["env"], lambda: run_case(E, name))
        t1 = time.time()
        again = _with_env(case["env"], lambda: run_case(E, name))
        print("%-26s %.1f s %s" % (name, t1 - t0, json.dumps(rec, sort_keys=True)), flush=True)
        miss = took_path(E, name, rec)
        if miss:
            bad.append("%s did not take its path (%s)" % (name, miss))
        if again != rec:
            bad.append("%s: two runs differ\n%s" % (name, json.dumps(again, sort_keys=True)))
        gold["cases"][name] = rec
    if bad:
        sys.exit("\n".join(bad) + "\nno golden written")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(gold, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()

"""tools/record_run_paths.py — what the host driver of the explicit-inverse engine decides, path by path, as exact values.

    python tools/record_run_paths.py [--out tests/golden/run_paths_parent.json]

Run on the build whose driver is the reference (the commit BEFORE a change to ellp_engine_run and its helpers that must
not move a decision); tests/test_gpu_run_paths.py replays the same cases on the current build and compares for equality.
The cases and the way each is driven are defined here and imported by the test, so that the recording and the replay
cannot drift apart.

A record holds, per ellp_engine_run call, the status, iters, pivots, bound_flips and the bits of obj; at the end the
sha256 digests of x, B_index, N_index, N_bound (dual: y and d too) from ellp_engine_read_point, and the host counters of
ELLP_TAP_STATE (maintenance requests serviced, refreshes, rebuilds, resyncs, drift checks, launches per iteration, the
certified hybrid's counters).  A driver that refreshes one iteration late ends on the same vertex: the counters see it.
Set-up seconds and kernel times are left out.  The recorder refuses a golden in which a case did not take its path
(took_path), or whose two runs differ."""
import hashlib
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 20260301
GOLDEN = os.path.join(ROOT, "tests", "golden", "run_paths_parent.json")
TO_END = 100000  # a slice no case uses up

# name -> kind ("primal" / "dual"), m, n, engine options, environment (set before creation, kept to the end), slices.
# slices None: one ellp_engine_run to the end; a tuple (step, budget): max_iter = budget, slices of `step` until it is spent.
# maint_at k: a first slice of k iterations, ellp_engine_request_maintenance, then on to the end.
CASES = {
    # primal, three launches, polled, reactive maintenance (the plan's ill_tol = 1e-3 at 48 rows)
    "a_primal3_polled_maint": dict(kind="primal", m=48, n=120, opts=dict(pipeline=1), env={}, maint_at=20),
    # primal, two launches, look-ahead
    "b_primal2_lookahead": dict(kind="primal", m=48, n=120, opts=dict(pipeline=2), env={"ELLP_ILL_TOL": "0"}),
    # ... in slices: the hst_fresh shortcut, an open iteration carried across slices, the budget close
    "c_primal2_slices": dict(kind="primal", m=48, n=120, opts=dict(pipeline=2), env={"ELLP_ILL_TOL": "0"}, slices=(7, 40)),
    # dual, fused, closing work folded into the next pricing launch
    "d_dual_fused_fold": dict(kind="dual", m=48, n=120, opts=dict(pipeline=2), env={"ELLP_ILL_TOL": "0"}),
    # ... without the fold: launch_dual_close per iteration, polled
    "e_dual_fused_close": dict(kind="dual", m=48, n=120, opts=dict(pipeline=2), env={}),
    # the certified hybrid: a takeover at the terminal status
    "f_hybrid": dict(kind="primal", m=160, n=400, opts=dict(pipeline=0), env={}),
    # ... and the redo from the snapshot
    "g_hybrid_redo": dict(kind="primal", m=160, n=400, opts=dict(pipeline=0), env={"ELLP_FORCE_REDO": "1"}),
    # (a) with event brackets: kernel_calls per id
    "h_profile": dict(kind="primal", m=48, n=120, opts=dict(pipeline=1, profile=1), env={}, maint_at=20),
    # a periodic refresh and a drift check inside one batch
    "i_period5_drift3": dict(kind="primal", m=48, n=120, opts=dict(pipeline=1, refactor_period=5), env={"ELLP_DRIFT_EVERY": "3"}),
}
# counters() entries that are compared (t_setup_s is a time; the rest are host counters or device values of identical kernels)
COUNTERS = ("drift_checks", "maint_requests", "refreshes", "rebuilds", "resyncs", "launches_per_iteration", "rebuild_shortcuts",
            "hybrid", "certified_by_exact_lu_iteration", "hybrid_guards", "hybrid_certs", "hybrid_disagreed", "hybrid_exact_iters",
            "hybrid_rebuilds", "hybrid_redos", "hybrid_uncertified")


def _sha(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


def _bits(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def _slice_record(st, stats, with_calls):
    r = {"status": int(st), "iters": int(stats.iters), "pivots": int(stats.pivots), "bound_flips": int(stats.bound_flips),
         "obj": _bits(stats.obj)}
    if with_calls:
        r["kernel_calls"] = [int(stats.kernel_calls[k]) for k in range(len(stats.kernel_calls))]
    return r


def run_case(E, name):
    """the record of one case; the caller has put CASES[name]["env"] into the environment"""
    from ellp_amd import synth
    case = CASES[name]
    dual = case["kind"] == "dual"
    f = (synth.dual_start_flat if dual else synth.primal_phase1_flat)(SEED, case["m"], case["n"])
    fp = E.FlatProblem(f["m"], f["n"], f["n_c"], f["A"], f["c"], f["b"], f["kind"], f["lb"], f["ub"], f["x"], f["B"], f["N"],
                       f["Nb"], y=f.get("y"), d=f.get("d"))
    slices = case.get("slices")
    opts = dict(case["opts"], max_iter=slices[1] if slices else None)
    prof = bool(opts.get("profile"))
    eng = E.Engine(E.ENGINE_DUAL if dual else E.ENGINE_PRIMAL, fp, E.default_opts(**opts))
    runs = []
    try:
        if slices:
            step, budget = slices
            done, st = 0, E.MAXITER
            while st == E.MAXITER and done < budget:
                k = min(step, budget - done)
                st, stats, _ = eng.run(k)
                runs.append(_slice_record(st, stats, prof))
                done += k
        else:
            st = E.MAXITER
            if case.get("maint_at"):
                st, stats, _ = eng.run(case["maint_at"])
                runs.append(_slice_record(st, stats, prof))
                eng.request_maintenance()
            if st == E.MAXITER:
                st, stats, _ = eng.run(TO_END)
                runs.append(_slice_record(st, stats, prof))
        eng.read_point()
        cnt = eng.counters()
    finally:
        eng.close()
    rec = {"runs": runs, "closing_status": int(eng.closing_status), "x": _sha(fp.x), "B": _sha(fp.B), "N": _sha(fp.N),
           "Nb": _sha(fp.Nb), "counters": {k: int(cnt[k]) for k in COUNTERS}}
    if dual:
        rec["y"], rec["d"] = _sha(fp.y), _sha(fp.d)
    return rec


def took_path(E, name, rec):
    """None, or what shows that the case did not take the path it is there for"""
    c, last = rec["counters"], rec["runs"][-1]
    lpi = c["launches_per_iteration"]
    if name[0] in "ah":
        if lpi != 3 or c["maint_requests"] < 1 or last["status"] != E.OPTIMAL:
            return "three launches, a serviced maintenance request, the optimal end"
        if name[0] == "h" and not (sum(last["kernel_calls"]) > 0 and sum(rec["runs"][0]["kernel_calls"]) > 0):
            return "event brackets collected"
    elif name[0] == "b":
        if lpi != 2 or last["status"] != E.OPTIMAL:
            return "two launches, the optimal end"
    elif name[0] == "c":
        step, budget = CASES[name]["slices"]
        if lpi != 2 or len(rec["runs"]) != -(-budget // step) or last["status"] != E.MAXITER or last["iters"] != budget:
            return "two launches, every slice used up, the budget spent"
    elif name[0] in "de":
        if lpi != 2 or last["status"] != E.OPTIMAL or last["pivots"] < 1:
            return "the fused dual loop with pivots, the optimal end"
    elif name[0] == "f":
        if not c["hybrid"] or c["hybrid_certs"] < 1 or c["hybrid_redos"] != 0 or last["status"] != E.OPTIMAL:
            return "the hybrid, a takeover at the terminal status, no redo"
    elif name[0] == "g":
        if c["hybrid_certs"] < 1 or c["hybrid_redos"] != 1 or last["status"] != E.OPTIMAL:
            return "a takeover at the terminal status, then the redo"
    elif name[0] == "i":
        if lpi != 3 or c["refreshes"] < 2 or c["drift_checks"] < 2 or last["status"] != E.OPTIMAL:
            return "periodic refreshes and drift checks, the optimal end"
    return None


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def main():
    from ellp_amd import _engine as E
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    gold = {"seed": SEED, "cases": {}}
    for name, case in CASES.items():
        rec = _with_env(case["env"], lambda: run_case(E, name))
        again = _with_env(case["env"], lambda: run_case(E, name))
        print("%-26s %s" % (name, json.dumps(rec, sort_keys=True)), flush=True)
        miss = took_path(E, name, rec)
        if miss:
            sys.exit("%s did not take its path (%s): no golden written" % (name, miss))
        if again != rec:
            sys.exit("%s: two runs differ: no golden written\n%s" % (name, json.dumps(again, sort_keys=True)))
        gold["cases"][name] = rec
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(gold, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()

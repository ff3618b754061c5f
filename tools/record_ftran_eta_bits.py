"""tools/record_ftran_eta_bits.py — the bytes the two-launch primal loop leaves, slice by slice, as sha256 digests.

    python tools/record_ftran_eta_bits.py [--out tests/golden/ftran_eta_parent_bits.json]

Run on the build whose results are the reference (the commit BEFORE a change to k_ftran_eta that must not move a bit);
tests/test_gpu_ftran_eta_handoff.py replays the same walks on the current build and compares.  The cases and the walk
are defined here and imported by the test, so that the recording and the replay cannot drift apart.

A walk: synth.primal_phase1_flat(SEED, m, n), default engine options except pipeline = 2 where the planner would not
choose the two-launch loop; 300 pivots taken as slices of 1, 2, 7 and 64 (repeated, the last one cut to end at 300), with
the point read back after every slice (which closes the open iteration); once with the default maintenance and once
with refactor_period = 50.  `to_end` walks run on to the optimal end in slices of 64."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 20260301
PIVOTS = 300
SLICES = (1, 2, 7, 64)
# m, n, and the double2 per thread per row k_ftran_eta holds in registers at that ld (its template parameter NR)
SHAPES = ((384, 600, 1),     # 192 of 256 lanes live
          (520, 800, 2),     # ld = 528: 8 live lanes in the last chunk, m != ld
          (1041, 1500, 4))   # ld = 1056 = m + 15, the last block has one row
# name -> (m, n, extra options, run to the optimal end)
CASES = {}
for _m, _n, _nr in SHAPES:
    CASES["%dx%d" % (_m, _n)] = (_m, _n, {}, False)
    CASES["%dx%d_refactor50" % (_m, _n)] = (_m, _n, {"refactor_period": 50}, False)
CASES["384x600_to_end"] = (384, 600, {}, True)
GOLDEN = os.path.join(ROOT, "tests", "golden", "ftran_eta_parent_bits.json")


def _sha(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


def make_engine(E, m, n, extra):
    """(engine, FlatProblem) for a case: the two-launch primal loop, by the planner's choice or by pipeline = 2"""
    from ellp_amd import synth
    f = synth.primal_phase1_flat(SEED, m, n)
    fp = E.FlatProblem(f["m"], f["n"], f["n_c"], f["A"], f["c"], f["b"], f["kind"], f["lb"], f["ub"], f["x"], f["B"], f["N"],
                       f["Nb"])
    kw = dict(max_iter=None, **extra)
    s, plan, msg = E.engine_plan(E.ENGINE_PRIMAL, fp.m, fp.nN, E.default_opts(**kw))
    assert s == E.OPTIMAL, msg
    if not plan["lagged"]:
        kw["pipeline"] = 2
    eng = E.Engine(E.ENGINE_PRIMAL, fp, E.default_opts(**kw))
    return eng, fp


def walk(E, m, n, extra, to_end):
    """the records of one case: after every slice the status, the iteration count and the digests of x, B, N, Nb"""
    eng, fp = make_engine(E, m, n, extra)
    out = []
    try:
        assert eng.counters()["launches_per_iteration"] == 2
        done, k, st = 0, 0, E.MAXITER
        while st == E.MAXITER and (to_end or done < PIVOTS):
            step = 64 if to_end else min(SLICES[k % len(SLICES)], PIVOTS - done)
            st, stats, msg = eng.run(step)
            eng.read_point()
            done += step
            k += 1
            assert k < 100000
            out.append({"status": int(st), "closing_status": int(eng.closing_status), "iters": int(stats.iters),
                        "x": _sha(fp.x), "B": _sha(fp.B), "N": _sha(fp.N), "Nb": _sha(fp.Nb)})
    finally:
        eng.close()
    return out if not to_end else out[-1:]


def main():
    from ellp_amd import _engine as E
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    rec = {"seed": SEED, "pivots": PIVOTS, "slices": list(SLICES), "cases": {}}
    for name, (m, n, extra, to_end) in CASES.items():
        rec["cases"][name] = walk(E, m, n, extra, to_end)
        last = rec["cases"][name][-1]
        print("%-24s %3d records, last: status %d after %d iterations" % (name, len(rec["cases"][name]), last["status"], last["iters"]),
              flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(rec, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()

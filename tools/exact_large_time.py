"""Milliseconds per loop body of the LU-per-iteration loop above 1,024 rows (run_exact_large: an LU of the basis, two or three
solves and the engine's bandwidth kernels per body), primal and dual, at m = 1,100 and m = 1,850, best of 5 and the spread.
Two ways to reach the loop: as the repetition of a phase (ELLP_FORCE_REDO=1 on default options: the time of a forced run minus
the time of the same run without the repetition, over the repetition's loop bodies) — every checkout has that one — and, where
the engine offers it, as the engine itself (pipeline = 3).  Where the library exports ellp_hip_lu_rows, also the device time
of the LU alone, unblocked and blocked.  Prints one JSON line per case with a digest of the outcomes (status, loop bodies,
basis, the bits of x), so that runs of two checkouts can be compared.  --alternate PARENT_CHECKOUT does the comparison in
one session: the parent, this checkout, the parent again, each in a process of its own, merged into --out under the labels
parent / this / parent_again; it fails if a digest differs between the builds.

    python tools/exact_large_time.py --alternate PARENT_CHECKOUT --out profiles/exact_lu_blocked_time.json
    python tools/exact_large_time.py [--tree OTHER_CHECKOUT] [--label NAME --out FILE]      # one checkout
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def quick_primal_start(synth, seed, m, n, k):
    """tests/test_gpu_hybrid.py's start: the slack basis on every row but the first k, a few hundred pivots from the end"""
    f = synth.primal_phase1_flat(seed, m, n)
    ntot = n + m
    B, N, x = f["B"].copy(), f["N"].copy(), f["x"].copy()
    for i in range(k, m):
        s, a = n + m - 1 - i, ntot + i
        B[i] = s
        N[np.where(N == s)[0][0]] = a
        x[s], x[a] = f["b"][i], 0.0
    f.update(B=B, N=N, x=x)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="the checkout whose ellp_amd package is measured (built); default: this one")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None, help="JSON file to merge the rows into, under --label")
    ap.add_argument("--alternate", metavar="PARENT_CHECKOUT", default=None,
                    help="measure PARENT_CHECKOUT, this checkout and PARENT_CHECKOUT again, one process each, into --out")
    a = ap.parse_args()
    if a.alternate:
        if not a.out:
            ap.error("--alternate needs --out")
        if os.path.exists(a.out):
            os.remove(a.out)
        for label, tree in (("parent", a.alternate), ("this", ROOT), ("parent_again", a.alternate)):
            subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", tree, "--label", label, "--out", a.out,
                            "--reps", str(a.reps)], check=True)
        doc = json.load(open(a.out))
        this = {r["case"]: r for r in doc["this"]}
        for label in ("parent", "parent_again"):
            for r in doc[label]:
                if r["digest"] != this[r["case"]]["digest"]:
                    sys.exit(f"{r['case']}: the outcome digest of {label} differs from this checkout's")
        print("outcome digests equal on both builds", flush=True)
        return
    sys.path.insert(0, os.path.abspath(a.tree))
    from ellp_amd import _engine as E
    from ellp_amd import synth

    def one_run(kind, f, env, **opts):
        fp = E.FlatProblem(f["m"], f["n"], f["n_c"], f["A"], f["c"], f["b"], f["kind"], f["lb"], f["ub"], f["x"], f["B"], f["N"], f["Nb"],
                           f.get("y"), f.get("d"))
        for k, v in env.items():
            os.environ[k] = v
        try:
            eng = E.Engine(kind, fp, E.default_opts(max_iter=1000000, **opts))
            try:
                t0 = time.perf_counter()
                st, stats, _ = eng.run(1000000)
                t = time.perf_counter() - t0
                eng.read_point()
                c = eng.counters()
            finally:
                eng.close()
        finally:
            for k in env:
                del os.environ[k]
        h = hashlib.sha1(f"{st} {int(stats.iters)}".encode())
        h.update(np.ascontiguousarray(fp.B).tobytes())
        h.update(np.ascontiguousarray(fp.x).tobytes())
        return t, int(stats.iters), c, h.hexdigest()[:16]

    rows = []
    cases = [(1100, 40, 5), (1850, 20, 4)]  # m, structural columns, rows that start on their artificial (primal)
    for m, n, k in cases:
        for which in ("primal", "dual"):
            kind = E.ENGINE_PRIMAL if which == "primal" else E.ENGINE_DUAL
            f = quick_primal_start(synth, 9, m, n, k) if which == "primal" else synth.dual_start_flat(9, m, n)
            one_run(kind, f, {})  # warm-up: code objects
            plain = [one_run(kind, f, {}) for _ in range(a.reps)]
            redo = [one_run(kind, f, {"ELLP_FORCE_REDO": "1"}) for _ in range(a.reps)]
            bodies = redo[-1][2]["hybrid_exact_iters"]
            # the fast loop's share of a forced run: the same run without the repetition — unless that run repeats the phase of
            # its own accord (its end point fails the check), in which case the fast loop's few milliseconds stay in
            plain_redid = plain[-1][2]["hybrid_redos"] > 0
            fast = 0.0 if plain_redid else min(p[0] for p in plain)
            per = [1e3 * (r[0] - fast) / max(bodies, 1) for r in redo]
            row = dict(case=f"{which} m={m}", loop_bodies=bodies, redo_ms_per_body=round(min(per), 4), redo_spread_ms=round(max(per) - min(per), 4),
                       redo_times_s=[round(r[0], 4) for r in redo], plain_best_s=round(min(p[0] for p in plain), 4), plain_redid=plain_redid,
                       redos=redo[-1][2]["hybrid_redos"], digest=redo[-1][3])
            p3 = [one_run(kind, f, {}, pipeline=3) for _ in range(a.reps)]
            if p3[-1][2]["hybrid_exact_iters"] == p3[-1][1] and p3[-1][1] > 0:  # pipeline 3 is the exact loop on this checkout
                per3 = [1e3 * r[0] / r[1] for r in p3]
                row.update(pipeline3_ms_per_body=round(min(per3), 4), pipeline3_spread_ms=round(max(per3) - min(per3), 4),
                           pipeline3_bodies=p3[-1][1], pipeline3_digest=p3[-1][3])
            rows.append(row)
            print(json.dumps(row), flush=True)
        if hasattr(E, "lu_rows"):
            A = np.random.default_rng(m).uniform(-1, 1, size=(m, m))
            row = dict(case=f"LU alone m={m}")
            for name, blocked in (("unblocked", False), ("blocked", True)):
                E.lu_rows(A, blocked=blocked)
                ts = []
                for _ in range(a.reps):
                    fac, piv, ud = E.lu_rows(A, blocked=blocked)
                    ts.append(E.lu_rows_last_ms())
                row[name + "_ms"] = round(min(ts), 4)
                row[name + "_spread_ms"] = round(max(ts) - min(ts), 4)
                row[name + "_digest"] = hashlib.sha1(fac.tobytes() + piv.tobytes() + ud.tobytes()).hexdigest()[:16]
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
        doc[a.label] = rows
        with open(a.out, "w") as fo:
            json.dump(doc, fo, indent=1)
            fo.write("\n")


if __name__ == "__main__":
    main()

"""Device time of one ellp_engine_postsolve at the shapes of configs 3 and 5 (m = 2000, n = 5000; m = 4000, n = 40000; the
synthetic primal phase 1 of bench.py), split into the LU of the basis, the triangular solves, the pass over the stored
columns and the rest (ELLP_POST_PROFILE=1: HIP events around the stages, one line on stderr per call), and beside it the
engine's own pricing launch at that shape from the same run (opts.profile).  Writes profiles/postsolve_time.json.

    python tools/postsolve_time.py [--out profiles/postsolve_time.json] [--iters 200] [--reps 5]

The measuring runs in a child process (its stderr is what is parsed); best of --reps calls and the spread.
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [("config3", 2000, 5000), ("config5", 4000, 40000)]
LINE = re.compile(r"postsolve_profile m=(\d+) nN=(\d+) steps=(\d+) passes=(\d+) lu_ms=([\d.]+) solve_ms=([\d.]+) pass_ms=([\d.]+) rest_ms=([\d.]+)")


def child(iters, reps):
    sys.path.insert(0, ROOT)
    from ellp_amd import _engine as E
    from ellp_amd import synth
    for name, m, n in SHAPES:
        f = synth.primal_phase1_flat(20260301, m, n)
        fp = E.FlatProblem(f["m"], f["n"], f["n_c"], f["A"], f["c"], f["b"], f["kind"], f["lb"], f["ub"], f["x"], f["B"], f["N"], f["Nb"])
        eng = E.Engine(E.ENGINE_PRIMAL, fp, E.default_opts(max_iter=None, profile=1))
        try:
            st, stats, msg = eng.run(iters)
            s = stats.as_dict()
            eng.postsolve()  # warm-up: the workspace, the code objects
            for _ in range(reps):
                y, d, r, k = eng.postsolve()
        finally:
            eng.close()
        print(json.dumps(dict(name=name, m=m, n=n, columns=int(fp.n), iters=int(stats.iters),
                              price_ms=s["kernel_ms"].get("price", 0.0), price_calls=int(s["kernel_calls"].get("price", 0)),
                              kkt=k)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "postsolve_time.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.iters, a.reps)
        return
    env = dict(os.environ, ELLP_POST_PROFILE="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(a.iters), "--reps", str(a.reps)],
                       env=env, capture_output=True, text=True, check=True)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    prof = [LINE.search(l) for l in p.stderr.splitlines()]
    prof = [tuple(float(g) for g in mm.groups()) for mm in prof if mm]
    sys.path.insert(0, ROOT)
    from ellp_amd.build import engine_source_hash
    out = dict(engine_source_hash=engine_source_hash(), reps=a.reps, shapes=[])
    for row in rows:
        mine = [q for q in prof if int(q[0]) == row["m"]][1:]  # without the warm-up call
        tot = [q[4] + q[5] + q[6] + q[7] for q in mine]
        best = mine[tot.index(min(tot))]
        passes = int(best[3])
        per_price = row["price_ms"] / max(row["price_calls"], 1)
        # bytes: one pass reads the m basic columns once per refinement round and the nonbasic columns once
        m, nN = row["m"], row["columns"] - row["m"]
        ld = (m + 15) // 16 * 16
        nb_bytes = 8 * ld * nN
        # the nonbasic share of the pass by bytes (the basic passes read m of the m + nN columns each)
        basic_passes = passes - 1
        share = nN / (nN + basic_passes * m)
        shape = dict(row, n_N=nN, postsolve_ms=round(min(tot), 4), spread_ms=round(max(tot) - min(tot), 4), lu_ms=best[4], solve_ms=best[5],
                     pass_ms=best[6], rest_ms=best[7], refinement_steps=int(best[2]), pass_launches=passes,
                     price_ms_per_launch=round(per_price, 4), nonbasic_bytes=nb_bytes,
                     pass_over_nonbasic_ms=round(best[6] * share, 4),
                     pass_GBps=round(8 * ld * (nN + basic_passes * m) / (best[6] * 1e-3) / 1e9, 1) if best[6] > 0 else None,
                     ratio_pass_to_price=round(best[6] * share / per_price, 3) if per_price > 0 else None)
        out["shapes"].append(shape)
        print(json.dumps(shape), flush=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")


if __name__ == "__main__":
    main()

"""Device time of one ellp_engine_certificate by stage, at the shapes of configs 3 and 5 (m = 2000, n = 5000; m = 4000,
n = 40000; the synthetic primal phase 1 of bench.py, after --iters iterations), for the two sources that search the tableau,
beside the ranging's tableau pass (k_range_tab<0> and its fold) on the same engine in the same process.  The stages are
bracketed with HIP events (ELLP_CERT_PROFILE=1 and ELLP_RANGE_PROFILE=1: one line on stderr per call each): base (the
postsolve and W = B^-1), point (x_B recomputed, Farkas only), tableau (k_cert_tab and its fold), vector (the refined solve of the
vector, when something qualified), verify (the compensated pass and the report).  At a mid-run point nothing qualifies, so
the last two stages do not run there; they are timed on a planted instance of the same shape (tests/cert_model.py: a random
dense basis with one row no column can repair / one column no row bounds), through ellp_certificate.  Writes
profiles/certificate_time.json.

    python tools/certificate_time.py [--out profiles/certificate_time.json] [--iters 200] [--reps 3]

The measuring runs in a child process (its stderr is what is parsed); best of --reps calls.  A record, not a gate.
"""
import argparse
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [("config3", 2000, 5000), ("config5", 4000, 40000)]
CLINE = re.compile(r"certificate_profile source=(\d+) m=(\d+) nN=(\d+) base_ms=([\d.]+) point_ms=([\d.]+) tableau_ms=([\d.]+) "
                   r"vector_ms=([\d.]+) verify_ms=([\d.]+)")
RLINE = re.compile(r"ranging_profile m=(\d+) nN=(\d+) solve_ms=([\d.]+) resid_ms=([\d.]+) tableau_ms=([\d.]+) rhs_ms=([\d.]+)")


def child(iters, reps):
    sys.path.insert(0, ROOT)
    from ellp_amd import _engine as E
    from ellp_amd import synth
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cert_model as CM
    import numpy as np
    for name, m, n in SHAPES:
        f = synth.primal_phase1_flat(20260301, m, n)
        fp = E.FlatProblem(f["m"], f["n"], f["n_c"], f["A"], f["c"], f["b"], f["kind"], f["lb"], f["ub"], f["x"], f["B"], f["N"], f["Nb"])
        eng = E.Engine(E.ENGINE_PRIMAL, fp, E.default_opts(max_iter=None))
        found = {}
        try:
            st, stats, msg = eng.run(iters)
            for _ in range(reps + 1):  # the first call of each makes the workspace
                eng.ranging()
                for source in (E.CERT_FARKAS_ROW, E.CERT_RAY_COLUMN):
                    vec, info = eng.certificate(source)
                    found[source] = (info["found"], info["qualifying"])
        finally:
            eng.close()
        # the planted instance of the same shape: both searches find their vector, so every stage runs
        nN = int(fp.n) - m
        planted = {}
        for source, inst in ((E.CERT_FARKAS_ROW, CM.farkas_family(m, nN, {m // 3: CM.NB_UPPER}, 7, dense=True)),
                             (E.CERT_RAY_COLUMN, CM.ray_family(m, nN, {nN // 3: CM.NB_LOWER}, 8, dense=True))):
            pf = E.FlatProblem(inst["m"], inst["n"], inst["n"], np.asfortranarray(inst["A"]).reshape(-1, order="F"), inst["c"], inst["b"],
                               inst["kind"], inst["lb"], inst["ub"], inst["x"], inst["B"], inst["N"], inst["Nb"])
            del inst
            for _ in range(reps + 1):
                vec, info = E.certificate(pf, source)
            planted[source] = (info["found"], info["qualifying"], info["refine_steps"])
            del pf
        print(json.dumps(dict(name=name, m=m, n=n, columns=int(fp.n), iters=int(stats.iters),
                              farkas_row=found[E.CERT_FARKAS_ROW], ray_column=found[E.CERT_RAY_COLUMN],
                              planted_farkas_row=planted[E.CERT_FARKAS_ROW], planted_ray_column=planted[E.CERT_RAY_COLUMN])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "certificate_time.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.iters, a.reps)
        return
    env = dict(os.environ, ELLP_CERT_PROFILE="1", ELLP_RANGE_PROFILE="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(a.iters), "--reps", str(a.reps)],
                       env=env, capture_output=True, text=True, timeout=1500)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit(p.returncode)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    cprof = [tuple(float(g) for g in mm.groups()) for mm in (CLINE.search(l) for l in p.stderr.splitlines()) if mm]
    rprof = [tuple(float(g) for g in mm.groups()) for mm in (RLINE.search(l) for l in p.stderr.splitlines()) if mm]
    sys.path.insert(0, ROOT)
    from ellp_amd.build import engine_source_hash
    out = dict(engine_source_hash=engine_source_hash(), reps=a.reps, shapes=[])
    for row in rows:
        m = row["m"]
        shape = dict(row, n_N=row["columns"] - m, range_tableau_ms=min(q[4] for q in rprof if int(q[0]) == m))
        for source, label in ((1, "farkas_row"), (2, "ray_column")):
            both = [q for q in cprof if int(q[0]) == source and int(q[1]) == m]  # reps + 1 mid-run calls, then as many planted
            half = len(both) // 2
            for mine, key in ((both[1:half], label + "_ms"), (both[half + 1:], "planted_" + label + "_ms")):  # without the first call
                best = min(mine, key=lambda q: sum(q[3:]))
                shape[key] = dict(base=best[3], point=best[4], tableau=best[5], vector=best[6], verify=best[7], total=round(sum(best[3:]), 4))
        out["shapes"].append(shape)
        print(json.dumps(shape), flush=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")


if __name__ == "__main__":
    main()

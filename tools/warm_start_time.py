"""What a warm start costs and what it saves, at the shapes of configs 3 and 5 (m = 2000, n = 5000; m = 4000, n = 40000; the
seeds of bench.py).  Writes profiles/warm_start_time.json.

  start    device time of ellp_basis_start next to ellp_postsolve on the same point (the synthetic primal phase 1 of bench.py
           after --iters iterations, read back), both in their host-memory forms, alternated in one process after a warm-up,
           best of --reps.  ELLP_POST_PROFILE=1 brackets the stages of both with HIP events (one line on stderr per call: the LU,
           the triangular solves, the pass over the stored columns, the rest); the wall time of each call, which holds the
           upload of A as well, is taken beside it.
  resolve  one end-to-end re-solve through the user API: the LP of bench.py's family (min c.x, A x <= b, x >= 0) solved cold
           by the primal solver, its right-hand sides perturbed (b_k * (1 + 0.05 sin(k + 1))), then solved warm from the old
           basis by the dual solver and cold by the primal solver, with loop bodies and wall time for both.  --resolve names the shapes it runs at (a cold solve of
           config 5 takes minutes).

    python tools/warm_start_time.py [--out profiles/warm_start_time.json] [--iters 200] [--reps 3] [--shapes config3,config5]
                                    [--resolve config3]

The measuring runs in a child process (its stderr is what is parsed).
"""
import argparse
import json
import math
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"config3": (2000, 5000, 20260301), "config5": (4000, 40000, 20260305)}
LINE = re.compile(r"(postsolve|basis_start)_profile m=(\d+) nN=(\d+) steps=(\d+) passes=(\d+) lu_ms=([\d.]+) solve_ms=([\d.]+) "
                  r"pass_ms=([\d.]+) rest_ms=([\d.]+)")


def child(shapes, resolve, iters, reps):
    sys.path.insert(0, ROOT)
    import numpy as np
    import ellp_amd
    from ellp_amd import _engine as E
    from ellp_amd import synth
    for name in shapes:
        m, n, seed = SHAPES[name]
        f = synth.primal_phase1_flat(seed, m, n)
        fp = E.FlatProblem(f["m"], f["n"], f["n_c"], f["A"], f["c"], f["b"], f["kind"], f["lb"], f["ub"], f["x"], f["B"], f["N"], f["Nb"])
        eng = E.Engine(E.ENGINE_PRIMAL, fp, E.default_opts(max_iter=None))
        try:
            eng.run(iters)
            eng.read_point()  # fills fp.x, fp.B, fp.N, fp.Nb
        finally:
            eng.close()
        x = fp.x.copy()
        E.postsolve(fp)  # warm-up: the code objects
        E.basis_start(fp, E.START_KEEP_LABELS)
        wall = {"postsolve": [], "basis_start": []}
        for _ in range(reps):
            sys.stderr.write("mark %s\n" % name)
            t0 = time.perf_counter()
            E.postsolve(fp)
            wall["postsolve"].append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            s, xs, ys, ds, Nbs, info = E.basis_start(fp, E.START_KEEP_LABELS)
            wall["basis_start"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        E.basis_start(fp, E.START_LABELS_BY_D)
        wall_by_d = time.perf_counter() - t0
        row = dict(kind="start", name=name, m=m, columns=int(fp.n), n_N=int(fp.nN), iters=iters,
                   wall_postsolve_ms=round(1e3 * min(wall["postsolve"]), 3), wall_basis_start_ms=round(1e3 * min(wall["basis_start"]), 3),
                   wall_basis_start_by_d_ms=round(1e3 * wall_by_d, 3), x_refinement_steps=info["x_refinement_steps"],
                   y_refinement_steps=info["kkt"]["refinement_steps"], x_backward_error=info["x_backward_error"],
                   max_abs_x_difference=float(np.abs(xs - x).max()))
        print(json.dumps(row), flush=True)
    for name in resolve:
        m, n, seed = SHAPES[name]
        A, b, c = synth.dense_lp(seed, m, n)

        def problem(rhs):
            p = ellp_amd.Problem()
            ids = [p.add_var(float(c[j]), ellp_amd.Bound.Lower(0.0)) for j in range(n)]
            for i in range(m):
                p.add_constraint(list(zip(ids, A[i].tolist())), ellp_amd.ConstraintOp.Lte, float(rhs[i]))
            return p
        # the cold solves are the primal solver's: on this family the dual solver's phase 1 needs some fifty times the loop
        # bodies of the whole primal solve (9.1e5 against 1.9e4 at 400 x 900), so the primal is the cold solve a user would run
        solver, cold_solver = ellp_amd.DualSimplexSolver(max_iter=None), ellp_amd.PrimalSimplexSolver(max_iter=None)
        t0 = time.perf_counter()
        base = cold_solver.solve(problem(b), ranging=True)
        t_base = time.perf_counter() - t0
        b2 = np.array([b[k] * (1.0 + 0.05 * math.sin(k + 1)) for k in range(m)])
        p2 = problem(b2)
        t0 = time.perf_counter()
        warm = solver.solve(p2, start=base.solution)
        t_warm = time.perf_counter() - t0
        t0 = time.perf_counter()
        cold = cold_solver.solve(p2)
        t_cold = time.perf_counter() - t0
        print(json.dumps(dict(kind="resolve", name=name, m=m, n=n, cold_solver="primal", warm_solver="dual", base_iters=list(base.iters), base_wall_s=round(t_base, 3),
                              warm_used=bool(warm.start["used"]), warm_reason=warm.start["reason"], warm_iters=list(warm.iters),
                              warm_wall_s=round(t_warm, 3), cold_iters=list(cold.iters), cold_wall_s=round(t_cold, 3),
                              warm_obj=warm.solution.obj() if warm.solution else None, cold_obj=cold.solution.obj() if cold.solution else None,
                              labels_changed=warm.start["labels_changed"], start_primal_infeasibility=warm.start["primal_infeasibility"],
                              start_dual_infeasibility=warm.start["dual_infeasibility"])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warm_start_time.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="config3,config5")
    ap.add_argument("--resolve", default="config3,config5")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    shapes = [s for s in a.shapes.split(",") if s]
    resolve = [s for s in a.resolve.split(",") if s]
    if a.child:
        child(shapes, resolve, a.iters, a.reps)
        return
    env = dict(os.environ, ELLP_POST_PROFILE="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(a.iters), "--reps", str(a.reps), "--shapes",
                        a.shapes, "--resolve", a.resolve], env=env, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        sys.exit(p.returncode)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    # the profile lines of the measured calls: those after a shape's first "mark" line, before the resolves
    prof, cur = {}, None
    for l in p.stderr.splitlines():
        if l.startswith("mark "):
            cur = l.split()[1]
            prof.setdefault(cur, {"postsolve": [], "basis_start": []})
            continue
        mm = LINE.search(l)
        if mm and cur:
            prof[cur][mm.group(1)].append([float(g) for g in mm.groups()[1:]])
    sys.path.insert(0, ROOT)
    from ellp_amd.build import engine_source_hash
    out = dict(engine_source_hash=engine_source_hash(), reps=a.reps, start=[], resolve=[])
    for row in rows:
        if row["kind"] == "resolve":
            out["resolve"].append(row)
            continue
        m, nN = row["m"], row["n_N"]
        ld = (m + 15) // 16 * 16
        shape = dict(row)
        for who in ("postsolve", "basis_start"):
            calls = prof.get(row["name"], {}).get(who, [])[:a.reps]  # KEEP_LABELS calls only (the LABELS_BY_D call comes last)
            if not calls:
                continue
            tot = [q[4] + q[5] + q[6] + q[7] for q in calls]
            best = calls[tot.index(min(tot))]
            shape[who] = dict(device_ms=round(min(tot), 4), spread_ms=round(max(tot) - min(tot), 4), lu_ms=best[4], solve_ms=best[5],
                              pass_ms=best[6], rest_ms=best[7], steps=int(best[2]), pass_launches=int(best[3]))
        by_d = prof.get(row["name"], {}).get("basis_start", [])[a.reps:]
        if by_d:
            q = by_d[0]
            shape["basis_start_by_d"] = dict(device_ms=round(q[4] + q[5] + q[6] + q[7], 4), lu_ms=q[4], solve_ms=q[5], pass_ms=q[6], rest_ms=q[7],
                                             pass_launches=int(q[3]))
        if "postsolve" in shape and "basis_start" in shape:
            shape["ratio_start_to_postsolve"] = round(shape["basis_start"]["device_ms"] / shape["postsolve"]["device_ms"], 3)
            shape["upload_bytes_of_A"] = 8 * m * (m + nN)
            shape["wall_minus_device_ms"] = round(row["wall_basis_start_ms"] - shape["basis_start"]["device_ms"], 3)
        shape["stored_bytes"] = 8 * ld * (m + nN)
        out["start"].append(shape)
    for s in out["start"] + out["resolve"]:
        print(json.dumps(s), flush=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")


if __name__ == "__main__":
    main()

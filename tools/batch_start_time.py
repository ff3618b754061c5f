"""What a batched warm start saves: wall time of ONE batched call against the loop of single calls over the same items, in the
same process, after a warm-up of each; best of --reps with the spread.  Per row count (32, 64, 128; m + m / 2 structural
columns of the synthetic family of ellp_amd.synth) and --items items (1,000):

  engine   ellp_batch_basis_start (LABELS_BY_D) against a loop of ellp_basis_start.  The items are the synthetic phase-1
           family after a batch_solve_with_initial (the bases are the solves' own), their right-hand sides then scaled by
           1 + 0.05 sin(k + 1); the bits of both sides are compared.  Device time of both from a second child process with
           ELLP_POST_PROFILE=1 (HIP events around the stages; for the loop without the uploads of the engine each call builds).
  api      DualSimplexSolver.solve_batch(ps2, starts=ss) against the loop of solve(p, start=s): min c.x, A x <= b, x >= 0 of the
           same family, ss the bases of a first PrimalSimplexSolver.solve_batch(ps, starts=[None] * n), ps2 the same problems
           with the right-hand sides scaled by 1 + 0.05 sin(k + 1); the entries of both sides are compared.

--loops-only times the two loops alone (they need nothing of the batched start: a build without it can run them); the bases of
the api loop then come from --bases, the file a full run wrote with --save-bases, so that both runs time the same items.

    python tools/batch_start_time.py [--reps 3] [--items 1000] [--out profiles/batch_start_time.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCALE = 0.05
LINE = re.compile(r"^(batch_basis_start_profile|basis_start_profile) .*lu_ms=([\d.]+) solve_ms=([\d.]+) pass_ms=([\d.]+) rest_ms=([\d.]+)")


def engine_items(E, count, m, seed):
    from ellp_amd import synth
    fps = []
    for k in range(count):
        f = synth.primal_phase1_flat(seed + k, m, m + m // 2)
        fps.append(E.FlatProblem(f["m"], f["n"], f["n_c"], f["A"], f["c"], f["b"], f["kind"], f["lb"], f["ub"], f["x"], f["B"], f["N"], f["Nb"]))
    res = E.batch_solve_with_initial(E.ENGINE_PRIMAL, fps, E.default_opts(max_iter=5000))
    assert all(st >= 0 for st, _, _ in res)
    for fp in fps:
        assert fp.n_c == fp.n
        fp.b = fp.b * (1.0 + SCALE * np.sin(np.arange(fp.m) + 1.0))
    return fps


def api_problem(A, b, c):
    """min c.x, A x <= b, x >= 0 (the rows go in through the C ABI directly: a million coefficients per size)"""
    import ellp_amd
    L = ellp_amd.host_lib()
    p = ellp_amd.Problem()
    for cj in c:
        p.add_var(float(cj), ellp_amd.Bound.Lower(0.0))
    ids = np.arange(A.shape[1], dtype=np.int64)
    err = C.create_string_buffer(512)
    for i in range(A.shape[0]):
        row = np.ascontiguousarray(A[i])
        rc = L.ellp_problem_add_constraint(p._h, len(ids), ids.ctypes.data_as(C.c_void_p), row.ctypes.data_as(C.c_void_p), 0, float(b[i]), err, 512)
        assert rc == 0, err.value
    return p


def api_items(count, m, seed):
    from ellp_amd import synth
    ps, ps2 = [], []
    scale = 1.0 + SCALE * np.array([math.sin(k + 1) for k in range(m)])
    for k in range(count):
        A, b, c = synth.dense_lp(seed + k, m, m + m // 2)
        ps.append(api_problem(A, b, c))
        ps2.append(api_problem(A, b * scale, c))
    return ps, ps2


def same_result(g, r):
    if isinstance(g, Exception) or isinstance(r, Exception):
        return type(g) is type(r) and str(g) == str(r)
    if (g.kind, tuple(g.iters), g.start) != (r.kind, tuple(r.iters), r.start):
        return False
    return g.kind != "optimal" or g.solution.x().tobytes() == r.solution.x().tobytes()


def timed(reps, mark, f):
    ts, out = [], None
    for rep in range(reps):
        sys.stderr.write(f"MARK {mark} {rep}\n")
        sys.stderr.flush()
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    sys.stderr.write("MARK end\n")
    sys.stderr.flush()
    return [round(1e3 * t, 3) for t in ts], out


def child(a):
    import ellp_amd
    from ellp_amd import _engine as E
    sizes = [int(v) for v in a.sizes.split(",")]
    bases = dict(np.load(a.bases, allow_pickle=False)) if a.bases else {}
    saved, out = {}, []
    for m in sizes:
        row = dict(rows=m, items=a.items)
        # ---- engine level
        fps = engine_items(E, a.items, m, 20260800 + m)
        E.basis_start(fps[0], E.START_LABELS_BY_D)  # warm-up: code objects, the pools
        row["engine_loop_wall_ms"], one = timed(a.reps, f"{m} eloop", lambda: [E.basis_start(fp, E.START_LABELS_BY_D) for fp in fps])
        row["x_refinement_steps_total"] = int(sum(o[5]["x_refinement_steps"] for o in one))
        row["dual_feasible"] = int(sum(o[5]["dual_feasible"] for o in one))
        if not a.loops_only:
            E.batch_basis_start(fps[:2], E.START_LABELS_BY_D)
            row["engine_batch_wall_ms"], res = timed(a.reps, f"{m} ebatch", lambda: E.batch_basis_start(fps, E.START_LABELS_BY_D))
            info = E.batch_basis_start_info()
            row.update(launches=info["launches"], chunks=info["chunks"], batched=info["batched"])
            row["engine_identical"] = bool(all(
                r[0] == o[0] == E.OPTIMAL and all(r[q].tobytes() == o[q].tobytes() for q in (1, 2, 3, 4)) and
                all(np.float64(r[5][key]).tobytes() == np.float64(o[5][key]).tobytes() for key in o[5] if isinstance(o[5][key], float)) and
                r[5]["kkt"] == o[5]["kkt"] for r, o in zip(res, one)))
        # ---- the user API (not under ELLP_POST_PROFILE: the second child only takes the device times above)
        if not a.profile_child:
            ps, ps2 = api_items(a.items, m, 20260900 + m)
            primal, dual = ellp_amd.PrimalSimplexSolver(max_iter=100000), ellp_amd.DualSimplexSolver(max_iter=100000)
            if a.loops_only:
                ss = [dict(B=bases[f"B{m}"][k], N=bases[f"N{m}"][k], Nb=bases[f"Nb{m}"][k]) for k in range(a.items)]
            else:
                t0 = time.perf_counter()
                r1 = primal.solve_batch(ps, starts=[None] * len(ps))
                row["api_first_round_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
                assert all(not isinstance(r, Exception) and r.kind == "optimal" for r in r1)
                ss = [r.solution.basis() for r in r1]
                for key in ("B", "N", "Nb"):
                    saved[f"{key}{m}"] = np.stack([s[key] for s in ss])
            dual.solve(ps2[0], start=ss[0])
            row["api_loop_wall_ms"], one = timed(a.reps, f"{m} aloop", lambda: [dual.solve(p, start=s) for p, s in zip(ps2, ss)])
            row["api_used"] = int(sum(r.start["used"] for r in one))
            row["api_loop_iters_phase2"] = int(sum(r.iters[1] for r in one))
            if not a.loops_only:
                dual.solve_batch(ps2[:2], starts=ss[:2])
                row["api_batch_wall_ms"], res = timed(a.reps, f"{m} abatch", lambda: dual.solve_batch(ps2, starts=ss))
                row["api_identical"] = bool(all(same_result(g, r) for g, r in zip(res, one)))
        out.append(row)
        sys.stderr.write(f"DONE {json.dumps(row)}\n")
        sys.stderr.flush()
    if a.save_bases and saved:
        np.savez(a.save_bases, **saved)
    print(json.dumps(out))


def run_child(a, profile):
    env = dict(os.environ)
    env.pop("ELLP_POST_PROFILE", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--items", str(a.items), "--sizes", a.sizes]
    if a.loops_only:
        cmd.append("--loops-only")
    if profile:
        env["ELLP_POST_PROFILE"] = "1"
        cmd.append("--profile-child")
    else:
        if a.bases:
            cmd += ["--bases", a.bases]
        if a.save_bases:
            cmd += ["--save-bases", a.save_bases]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit(p.returncode)
    return json.loads(p.stdout.strip().splitlines()[-1]), p.stderr


def device_ms(stderr):
    """{(rows, which): [ms of each repetition]} from the profile lines between the marks"""
    out, key = {}, None
    for line in stderr.splitlines():
        if line.startswith("MARK"):
            w = line.split()
            key = (w[1], w[2]) if len(w) == 4 else None
            if key:
                out.setdefault(key, []).append(0.0)
            continue
        m = LINE.match(line)
        if m and key:
            out[key][-1] += sum(float(v) for v in m.groups()[1:])
    return out


def best(v):
    return dict(best=round(min(v), 3), spread=round(max(v) - min(v), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--items", type=int, default=1000)
    ap.add_argument("--sizes", default="32,64,128")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_start_time.json"))
    ap.add_argument("--loops-only", action="store_true")
    ap.add_argument("--bases", default="")
    ap.add_argument("--save-bases", default="")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--profile-child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a)
        return
    wall, _ = run_child(a, False)
    _, err = run_child(a, True)
    dev = device_ms(err)
    rows = []
    for w in wall:
        row = dict(w)
        for key in ("engine_loop", "engine_batch", "api_loop", "api_batch"):
            if key + "_wall_ms" in row:
                row[key + "_wall_ms"] = best(row[key + "_wall_ms"])
        for which, key in (("eloop", "engine_loop_device_ms"), ("ebatch", "engine_batch_device_ms")):
            if (str(w["rows"]), which) in dev:
                row[key] = best(dev[(str(w["rows"]), which)])
        if "engine_batch_wall_ms" in row:
            row["engine_wall_ratio"] = round(row["engine_loop_wall_ms"]["best"] / row["engine_batch_wall_ms"]["best"], 1)
            row["engine_device_ratio"] = round(row["engine_loop_device_ms"]["best"] / row["engine_batch_device_ms"]["best"], 1)
        if "api_batch_wall_ms" in row:
            row["api_wall_ratio"] = round(row["api_loop_wall_ms"]["best"] / row["api_batch_wall_ms"]["best"], 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump(dict(reps=a.reps, loops_only=bool(a.loops_only), sets=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

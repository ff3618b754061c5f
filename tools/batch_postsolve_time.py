"""What a batched postsolve saves: wall and device time of ONE ellp_batch_postsolve against a loop of ellp_postsolve over the
same items, in the same process, after a warm-up call of each; best of --reps with the spread.

Two sets, solved by batch_solve_with_initial first (so the bases are the solves' own): 1,000 random LPs of 20 to 60 rows,
and 200 of 100 to 128 rows (the synthetic phase-1 family of ellp_amd.synth, 1.5 m structural columns).  Wall time is taken
in a child process without profiling; device time in a second child with ELLP_POST_PROFILE=1 (HIP events around the stages,
lines on stderr: the sum of a call's lines; for the loop this leaves out the uploads and gathers of the minimal engine each
call builds, for the batch the one upload and read-back).  Checks that both give the same bits.

    python tools/batch_postsolve_time.py [--reps 5] [--out profiles/batch_postsolve_time.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = [("small", 1000, 20, 60), ("large", 200, 100, 128)]
LINE = re.compile(r"^(batch_postsolve_profile|postsolve_profile) .*lu_ms=([\d.]+) solve_ms=([\d.]+) pass_ms=([\d.]+) rest_ms=([\d.]+)")


def make_items(E, count, lo, hi, seed):
    from ellp_amd import synth
    rng = np.random.default_rng(seed)
    fps = []
    for k in range(count):
        m = int(rng.integers(lo, hi + 1))
        f = synth.primal_phase1_flat(seed + k, m, m + m // 2)
        fps.append(E.FlatProblem(f["m"], f["n"], f["n_c"], f["A"], f["c"], f["b"], f["kind"], f["lb"], f["ub"], f["x"], f["B"], f["N"], f["Nb"]))
    res = E.batch_solve_with_initial(E.ENGINE_PRIMAL, fps, E.default_opts(max_iter=5000))
    assert all(st >= 0 for st, _, _ in res)
    return fps


def child(reps):
    from ellp_amd import _engine as E
    out = []
    for name, count, lo, hi in SETS:
        fps = make_items(E, count, lo, hi, 20260700 + lo)
        E.batch_postsolve(fps[:2])  # warm-up: code objects, the pinned pool
        E.postsolve(fps[0])
        tb, tl = [], []
        for rep in range(reps):
            sys.stderr.write(f"MARK {name} batch {rep}\n")
            sys.stderr.flush()
            t0 = time.perf_counter()
            res = E.batch_postsolve(fps)
            tb.append(time.perf_counter() - t0)
            sys.stderr.write(f"MARK {name} loop {rep}\n")
            sys.stderr.flush()
            t0 = time.perf_counter()
            one = [E.postsolve(fp) for fp in fps]
            tl.append(time.perf_counter() - t0)
        sys.stderr.write("MARK end\n")
        sys.stderr.flush()
        same = all(r[0] == E.OPTIMAL and r[1].tobytes() == o[0].tobytes() and r[2].tobytes() == o[1].tobytes() and
                   r[3].tobytes() == o[2].tobytes() and r[4] == o[3] for r, o in zip(res, one))
        info = E.batch_postsolve_info()
        out.append(dict(set=name, items=count, rows=[lo, hi], identical=bool(same), launches=info["launches"], chunks=info["chunks"],
                        refinement_steps_total=int(sum(o[3]["refinement_steps"] for o in one)),
                        batch_wall_ms=[round(1e3 * t, 3) for t in tb], loop_wall_ms=[round(1e3 * t, 3) for t in tl]))
    print(json.dumps(out))


def run_child(reps, profile):
    env = dict(os.environ)
    env.pop("ELLP_POST_PROFILE", None)
    if profile:
        env["ELLP_POST_PROFILE"] = "1"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps)], env=env, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit(p.returncode)
    return json.loads(p.stdout.strip().splitlines()[-1]), p.stderr


def device_ms(stderr):
    """{(set, which): [ms of each repetition]} from the profile lines between the marks"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_postsolve_time.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.reps)
        return
    wall, _ = run_child(a.reps, False)
    _, err = run_child(a.reps, True)
    dev = device_ms(err)
    rows = []
    for w in wall:
        name = w["set"]
        row = dict(set=name, items=w["items"], rows=w["rows"], identical=w["identical"], launches=w["launches"], chunks=w["chunks"],
                   refinement_steps_total=w["refinement_steps_total"],
                   batch_wall_ms=best(w["batch_wall_ms"]), loop_wall_ms=best(w["loop_wall_ms"]),
                   batch_device_ms=best(dev[(name, "batch")]), loop_device_ms=best(dev[(name, "loop")]))
        row["wall_ratio"] = round(row["loop_wall_ms"]["best"] / row["batch_wall_ms"]["best"], 1)
        row["device_ratio"] = round(row["loop_device_ms"]["best"] / row["batch_device_ms"]["best"], 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump(dict(reps=a.reps, sets=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

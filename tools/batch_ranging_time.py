"""What a batched ranging saves: wall and device time of ONE ellp_batch_ranging against a loop of ellp_ranging over the same
items, and of solve_batch(ps, ranging=True) against a loop of solve(p, ranging=True), in the same process, after a warm-up
call of each; best of --reps with the spread.

Three sets of --items (1,000) LPs of exactly 32, 64 and 128 rows (the synthetic family of ellp_amd.synth, 1.5 m structural
columns).  For the first comparison the phase-1 arrays are solved by batch_solve_with_initial first, so the points are
optimal and the bases the solves' own; for the second the same LPs are built as Problems (all rows `<=`, all variables
Lower(0)) and solved by the primal solver.  Wall time is taken in a child process without profiling; device time in a
second child with ELLP_RANGE_PROFILE=1 and ELLP_POST_PROFILE=1 (HIP events around the stages, lines on stderr: for the
batch the five launches of a chunk one by one; for the loop the sum of a call's postsolve and ranging lines, which leaves
out the uploads of the minimal engine each call builds, as the batch's figure leaves out its one upload and read-back).
Checks that both give the same bits.

    python tools/batch_ranging_time.py [--reps 3] [--items 1000] [--api-items 1000,1000,1000] [--out profiles/batch_ranging_time.json]
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

ROWS = [32, 64, 128]
STAGES = ("front", "solve", "tableau", "fold", "report")
BATCH_LINE = re.compile(r"^batch_ranging_profile .*front_ms=([\d.]+) solve_ms=([\d.]+) tableau_ms=([\d.]+) fold_ms=([\d.]+) report_ms=([\d.]+)")
POST_LINE = re.compile(r"^postsolve_profile .*lu_ms=([\d.]+) solve_ms=([\d.]+) pass_ms=([\d.]+) rest_ms=([\d.]+)")
RANGE_LINE = re.compile(r"^ranging_profile .*solve_ms=([\d.]+) resid_ms=([\d.]+) tableau_ms=([\d.]+) rhs_ms=([\d.]+)")


def make_items(E, count, m, seed):
    from ellp_amd import synth
    fps = []
    for k in range(count):
        f = synth.primal_phase1_flat(seed + k, m, m + m // 2)
        fps.append(E.FlatProblem(f["m"], f["n"], f["n_c"], f["A"], f["c"], f["b"], f["kind"], f["lb"], f["ub"], f["x"], f["B"], f["N"], f["Nb"]))
    res = E.batch_solve_with_initial(E.ENGINE_PRIMAL, fps, E.default_opts(max_iter=100000))
    assert all(st == E.OPTIMAL for st, _, _ in res)
    return fps


def make_problems(count, m, seed):
    import ellp_amd
    from ellp_amd import synth
    ps = []
    for k in range(count):
        A, b, c = synth.dense_lp(seed + k, m, m + m // 2)
        p = ellp_amd.Problem()
        for j in range(A.shape[1]):
            p.add_var(float(c[j]), ellp_amd.Bound.Lower(0.0))
        for i in range(m):
            p.add_constraint([[j, float(A[i, j])] for j in range(A.shape[1])], "Lte", float(b[i]))
        ps.append(p)
    return ps


def _same_rg(a, b):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in a.ARRAYS) and a.kkt == b.kkt and \
        np.float64(a.inverse_residual).tobytes() == np.float64(b.inverse_residual).tobytes()


def _same_result(a, b):
    if a.kind != b.kind or a.iters != b.iters:
        return False
    if a.kind != "optimal":
        return True
    sa, sb = a.solution, b.solution
    return sa.x().tobytes() == sb.x().tobytes() and all(u.tobytes() == v.tobytes() for u, v in zip(sa.cost_ranging() + sa.rhs_ranging(),
                                                                                                     sb.cost_ranging() + sb.rhs_ranging()))


def mark(text):
    sys.stderr.write(f"MARK {text}\n")
    sys.stderr.flush()


def ticking(seq, every=100):
    """seq, with a TICK line on stderr every `every` entries: a loop of slow single calls shows that it is alive"""
    for k, v in enumerate(seq):
        if k and k % every == 0:
            sys.stderr.write(f"TICK {k}\n")
            sys.stderr.flush()
        yield v


def child(reps, items, api_items):
    """api_items: the problems of the second comparison per row count (0: left out, as in the profiled run)"""
    import ellp_amd
    from ellp_amd import _engine as E
    out = []
    solver = ellp_amd.PrimalSimplexSolver()
    for m, n_api in zip(ROWS, api_items):
        fps = make_items(E, items, m, 20260900 + 1000 * m)
        ps = make_problems(n_api, m, 20260900 + 1000 * m)
        E.batch_ranging(fps[:2])  # warm-up: code objects, the pinned pool
        E.ranging(fps[0])
        if ps:
            solver.solve_batch(ps[:2], ranging=True)
            solver.solve(ps[0], ranging=True)
        got = ref = []
        tb, tl, sb, sl = [], [], [], []
        for rep in range(reps):
            mark(f"{m} batch {rep}")
            t0 = time.perf_counter()
            res = E.batch_ranging(fps)
            tb.append(time.perf_counter() - t0)
            info = E.batch_ranging_info()
            mark(f"{m} loop {rep}")
            t0 = time.perf_counter()
            one = [E.ranging(fp) for fp in ticking(fps, 250)]
            tl.append(time.perf_counter() - t0)
            if not ps:
                continue
            mark(f"{m} api-batch {rep}")
            t0 = time.perf_counter()
            got = solver.solve_batch(ps, ranging=True)
            sb.append(time.perf_counter() - t0)
            mark(f"{m} api-loop {rep}")
            t0 = time.perf_counter()
            ref = [solver.solve(p, ranging=True) for p in ticking(ps, 50)]
            sl.append(time.perf_counter() - t0)
        mark("end")
        same = all(r[0] == E.OPTIMAL and _same_rg(r[1], o) for r, o in zip(res, one))
        same_api = all(not isinstance(g, Exception) and _same_result(g, r) for g, r in zip(got, ref))
        ms = lambda v: [round(1e3 * t, 3) for t in v]
        out.append(dict(rows=m, items=items, api_items=n_api, nonbasic=int(fps[0].nN), identical=bool(same), api_identical=bool(same_api),
                        launches=info["launches"], chunks=info["chunks"], batch_wall_ms=ms(tb), loop_wall_ms=ms(tl),
                        api_batch_wall_ms=ms(sb), api_loop_wall_ms=ms(sl)))
    print(json.dumps(out))


def run_child(reps, items, api_items, profile):
    env = dict(os.environ)
    for key in ("ELLP_RANGE_PROFILE", "ELLP_POST_PROFILE"):
        env.pop(key, None)
        if profile:
            env[key] = "1"
    p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps), "--items", str(items), "--api-items",
                          ",".join(str(v) for v in api_items)], env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    lines = []
    for line in p.stderr:  # the marks as they come: a long run shows where it is
        lines.append(line)
        if line.startswith(("MARK", "TICK")):
            sys.stderr.write(("profiled " if profile else "wall ") + line)
            sys.stderr.flush()
    stdout = p.stdout.read()
    if p.wait() != 0:
        sys.stderr.write("".join(lines)[-4000:])
        raise SystemExit(p.returncode)
    return json.loads(stdout.strip().splitlines()[-1]), "".join(lines)


def device_ms(stderr):
    """{(rows, which): [per repetition: total ms, and for the batch the ms of each launch]} from the lines between the marks"""
    out, key = {}, None
    for line in stderr.splitlines():
        if line.startswith("MARK"):
            w = line.split()
            key = (int(w[1]), w[2]) if len(w) == 4 and w[2] in ("batch", "loop") else None
            if key:
                out.setdefault(key, []).append(dict(total=0.0, **{s: 0.0 for s in STAGES}))
            continue
        if not key:
            continue
        m = BATCH_LINE.match(line)
        if m and key[1] == "batch":
            for s, v in zip(STAGES, m.groups()):
                out[key][-1][s] += float(v)
                out[key][-1]["total"] += float(v)
        m = POST_LINE.match(line) or RANGE_LINE.match(line)
        if m and key[1] == "loop":
            out[key][-1]["total"] += sum(float(v) for v in m.groups())
    return out


def best(v):
    return dict(best=round(min(v), 3), spread=round(max(v) - min(v), 3)) if v else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--items", type=int, default=1000)
    ap.add_argument("--api-items", default=None, help="problems of the solve_batch comparison per row count, e.g. 1000,1000,200 (default: --items)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_ranging_time.json"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    api_items = [a.items] * len(ROWS) if a.api_items is None else [int(v) for v in a.api_items.split(",")]
    assert len(api_items) == len(ROWS)
    if a.child:
        child(a.reps, a.items, api_items)
        return
    wall, _ = run_child(a.reps, a.items, api_items, False)
    _, err = run_child(a.reps, a.items, [0] * len(ROWS), True)
    dev = device_ms(err)
    rows = []
    for w in wall:
        m = w["rows"]
        row = {k: w[k] for k in ("rows", "items", "api_items", "nonbasic", "identical", "api_identical", "launches", "chunks")}
        for k in ("batch_wall_ms", "loop_wall_ms", "api_batch_wall_ms", "api_loop_wall_ms"):
            row[k] = best(w[k])
        b = min(dev[(m, "batch")], key=lambda r: r["total"])
        row["batch_device_ms"] = best([r["total"] for r in dev[(m, "batch")]])
        row["batch_device_ms_by_launch"] = {s: round(b[s], 3) for s in STAGES}
        row["loop_device_ms"] = best([r["total"] for r in dev[(m, "loop")]])
        row["wall_ratio"] = round(row["loop_wall_ms"]["best"] / row["batch_wall_ms"]["best"], 1)
        row["device_ratio"] = round(row["loop_device_ms"]["best"] / row["batch_device_ms"]["best"], 1)
        if row["api_batch_wall_ms"]:
            row["api_wall_ratio"] = round(row["api_loop_wall_ms"]["best"] / row["api_batch_wall_ms"]["best"], 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(reps=a.reps, sets=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

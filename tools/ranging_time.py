"""Device time of one ellp_engine_ranging at the shapes of configs 3 and 5 (m = 2000, n = 5000; m = 4000, n = 40000; the
synthetic primal phase 1 of bench.py), split into its stages by HIP events (ELLP_RANGE_PROFILE=1 and ELLP_POST_PROFILE=1: one
line on stderr per call each): the multi-right-hand-side solve that makes W = B^-1, the residual |I - A_B W|, the tableau pass
(the f64 MFMA GEMM with the ratio test in its epilogue, and its fold) and the right-hand-side pass.  Beside them, from the
same run: one k_lu_solve (the postsolve's own transposed solves) times m — what W would cost solved one row at a time — and
the achieved f64 FLOP rate of the tableau pass, 2 m^2 n_N over its time.  Writes profiles/ranging_time.json.

    python tools/ranging_time.py [--out profiles/ranging_time.json] [--iters 200] [--reps 3] [--kernel-stats config3=FILE.csv] [--kernel-stats config5=FILE.csv]

--kernel-stats NAME=FILE.csv: for the shape NAME, a kernel_stats CSV of
`rocprofv3 --kernel-trace --stats -- python tools/ranging_time.py --child --only NAME` taken in the same session; the average times of k_range_tab<0>, k_range_solve, k_lu_solve and of k_gemm_mfma<1> (the Newton-Schulz
refresh's m x m x m GEMM, which the child runs once per shape through Engine.refresh) go into the file per kernel, and
k_gemm_mfma<1>'s FLOP rate (2 m^3 over its time) next to the tableau pass's.  A CSV holds one average per kernel name, so each
traced child, started by hand, takes --only with one shape; the event-timed child this tool starts itself runs both.

The measuring runs in a child process (its stderr is what is parsed); best of --reps calls and the spread.
"""
import argparse
import csv
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [("config3", 2000, 5000), ("config5", 4000, 40000)]
RLINE = re.compile(r"ranging_profile m=(\d+) nN=(\d+) solve_ms=([\d.]+) resid_ms=([\d.]+) tableau_ms=([\d.]+) rhs_ms=([\d.]+)")
PLINE = re.compile(r"postsolve_profile m=(\d+) nN=(\d+) steps=(\d+) passes=(\d+) lu_ms=([\d.]+) solve_ms=([\d.]+) pass_ms=([\d.]+) rest_ms=([\d.]+)")


def child(iters, reps, only):
    sys.path.insert(0, ROOT)
    from ellp_amd import _engine as E
    from ellp_amd import synth
    for name, m, n in SHAPES:
        if only and name != only:
            continue
        f = synth.primal_phase1_flat(20260301, m, n)
        fp = E.FlatProblem(f["m"], f["n"], f["n_c"], f["A"], f["c"], f["b"], f["kind"], f["lb"], f["ub"], f["x"], f["B"], f["N"], f["Nb"])
        eng = E.Engine(E.ENGINE_PRIMAL, fp, E.default_opts(max_iter=None))
        try:
            st, stats, msg = eng.run(iters)
            rg = eng.ranging()  # warm-up: the workspace, the code objects
            for _ in range(reps):
                rg = eng.ranging()
            resid = eng.refresh()  # one Newton-Schulz step: k_gemm_mfma<0> and <1> at this m, for the kernel trace
        finally:
            eng.close()
        import numpy as np
        print(json.dumps(dict(name=name, m=m, n=n, columns=int(fp.n), iters=int(stats.iters), inverse_residual=rg.inverse_residual,
                              refresh_residual=float(resid), basic_costs_limited=int(np.isfinite(rg.cost_up[fp.B]).sum()),
                              rhs_limited=int(np.isfinite(rg.rhs_up).sum()))), flush=True)


def kernel_stats(path):
    """{kernel name without arguments: (calls, average ns)} of a rocprofv3 kernel_stats CSV"""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = re.sub(r"\(.*", "", row["Name"].replace("(anonymous namespace)::", "").replace("void ", ""))
            out[name] = (int(row["Calls"]), float(row["AverageNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ranging_time.json"))
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="")
    ap.add_argument("--kernel-stats", action="append", default=[], help="NAME=FILE.csv, NAME a shape (config3, config5)")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.iters, a.reps, a.only)
        return
    env = dict(os.environ, ELLP_RANGE_PROFILE="1", ELLP_POST_PROFILE="1")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--iters", str(a.iters), "--reps", str(a.reps)],
                       env=env, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit(p.returncode)
    rows = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    rprof = [tuple(float(g) for g in mm.groups()) for mm in (RLINE.search(l) for l in p.stderr.splitlines()) if mm]
    pprof = [tuple(float(g) for g in mm.groups()) for mm in (PLINE.search(l) for l in p.stderr.splitlines()) if mm]
    traces = dict(kv.split("=", 1) for kv in a.kernel_stats)
    sys.path.insert(0, ROOT)
    from ellp_amd.build import engine_source_hash
    out = dict(engine_source_hash=engine_source_hash(), reps=a.reps, shapes=[])
    for row in rows:
        m, nN = row["m"], row["columns"] - row["m"]
        mine = [q for q in rprof if int(q[0]) == m][1:]  # without the warm-up call
        post = [q for q in pprof if int(q[0]) == m][1:]
        tot = [q[2] + q[3] + q[4] + q[5] for q in mine]
        best = mine[tot.index(min(tot))]
        one_solve = min(q[5] / (q[2] + 1) for q in post)  # the postsolve's solves: one for y, one per refinement step
        flops = 2.0 * m * m * nN
        shape = dict(row, n_N=nN, ranging_stages_ms=round(min(tot), 4), spread_ms=round(max(tot) - min(tot), 4),
                     multi_solve_ms=best[2], residual_ms=best[3], tableau_ms=best[4], rhs_ms=best[5],
                     postsolve_ms=round(min(q[4] + q[5] + q[6] + q[7] for q in post), 4),
                     one_lu_solve_ms=round(one_solve, 4), m_lu_solves_ms=round(one_solve * m, 1),
                     multi_solve_speedup=round(one_solve * m / best[2], 1) if best[2] > 0 else None,
                     tableau_flop=flops, tableau_TFLOPs=round(flops / (best[4] * 1e-3) / 1e12, 2) if best[4] > 0 else None,
                     rhs_GBps=round(8.0 * m * m / (best[5] * 1e-3) / 1e9, 1) if best[5] > 0 else None)
        if row["name"] in traces:
            ks = kernel_stats(traces[row["name"]])
            want = {"k_range_tab<0>": "tableau_kernel", "k_gemm_mfma<1>": "gemm_mfma_1", "k_lu_solve": "lu_solve"}
            want.update({k: "range_solve" for k in ks if k.startswith("k_range_solve")})
            tr = {label: dict(kernel=k, calls=ks[k][0], avg_ms=round(ks[k][1] * 1e-6, 4)) for k, label in want.items() if k in ks}
            if "tableau_kernel" in tr:
                tr["tableau_kernel"]["TFLOPs"] = round(flops / (tr["tableau_kernel"]["avg_ms"] * 1e-3) / 1e12, 2)
            if "gemm_mfma_1" in tr:
                tr["gemm_mfma_1"]["TFLOPs"] = round(2.0 * m ** 3 / (tr["gemm_mfma_1"]["avg_ms"] * 1e-3) / 1e12, 2)
            shape["kernel_trace"] = tr
        out["shapes"].append(shape)
        print(json.dumps(shape), flush=True)
    with open(a.out, "w") as fo:
        json.dump(out, fo, indent=1)
        fo.write("\n")


if __name__ == "__main__":
    main()

"""tools/batch_dual_mid_throughput.py — LPs per second of the dual solve_batch on mid-size LPs (129 to 1,024 rows: phase-1
starts from ellp_batch_dual_phase1_start, both phases on k_mid_batch) against loops of solve(), for N permuted orders
(tests/helpers.permuted_fixture) of BLEND x 2 (148 rows), ADLITTLE x 3 (168 rows) and ADLITTLE x 6 (336 rows); N in
{1, 64, 256, 1024}; two option sets: bound flipping + max violation, and pipeline = 3.  Prints one JSON line.

Three rates side by side: the batch with the option set; a loop of solve() with the same options (k_mid alone, the same
bits); a loop of default solve() (the certified hybrid).  Next to them two wall-clock figures per iteration: `batch_us_per_iter` is
the wall time of the whole solve_batch call over the iterations of its longest item — host set-up and packing of all N
problems in both phases included, and more than one wave of workgroups when N exceeds what the chip holds at once, so it
is NOT a per-item device time; `single_us_per_iter` is the same-option loop's wall time over its iterations.  Device time
per iteration needs a kernel trace (rocprofv3 --kernel-trace).  The loops run one solve()
after another, so their rates do not depend on N: they are timed on the first min(N, --loop-max) problems.  The batch's
outcomes are checked against both loops on the problems the loops timed (kind and iteration counts against the same-option
loop, kind against the hybrid's)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ellp_amd import DualSimplexSolver, Problem  # noqa: E402
from helpers import GOLDEN, blockdiag, permuted_fixture, read_mps  # noqa: E402


def outcome(r):
    return ("error", type(r).__name__) if isinstance(r, Exception) else (r.kind, tuple(r.iters))


def solve_all(solver, ps):
    out = []
    for p in ps:
        try:
            out.append(solver.solve(p))
        except Exception as e:  # noqa: BLE001 — an outcome like any other
            out.append(e)
    return out


def timed(fn):
    fn()  # warm-up of the same shape
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def iters(r):
    return 0 if isinstance(r, Exception) else int(sum(r.iters))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,256,1024")
    ap.add_argument("--loop-max", type=int, default=8)
    ap.add_argument("--lps", default="blend_x2,adlittle_x3,adlittle_x6", help="which LP sets to run")
    ap.add_argument("--modes", default="bflip_maxviol,pipeline3", help="which option sets to run")
    a = ap.parse_args()
    netlib = {nm: read_mps(os.path.join(GOLDEN, "netlib", nm + ".mps")) for nm in ("blend", "adlittle")}
    sets = [("blend_x2", blockdiag(netlib["blend"], 2)), ("adlittle_x3", blockdiag(netlib["adlittle"], 3)),
            ("adlittle_x6", blockdiag(netlib["adlittle"], 6))]
    modes = {"bflip_maxviol": dict(flags=16 | 2), "pipeline3": dict(pipeline=3)}
    out = {"what": "dual LPs per second, 129-1,024 rows: solve_batch against loops of solve() with the same options and at "
                   "the defaults (certified hybrid)", "rows": []}
    max_iter = 100000
    hybrid = DualSimplexSolver.new(max_iter)
    for name, fx in [t for t in sets if t[0] in a.lps.split(",")]:
        for n in [int(s) for s in a.sizes.split(",")]:
            rng = np.random.default_rng(3000 + n)
            ps = [Problem.from_fixture(permuted_fixture(fx, rng)) for _ in range(n)]
            k = min(n, a.loop_max)
            t_h, loop_h = timed(lambda: solve_all(hybrid, ps[:k]))
            for mode in a.modes.split(","):
                exact = DualSimplexSolver.new(max_iter, **modes[mode])
                t_b, batch = timed(lambda: exact.solve_batch(ps))
                t_e, loop_e = timed(lambda: solve_all(exact, ps[:k]))
                it_b = max(iters(r) for r in batch)
                it_e = sum(iters(r) for r in loop_e)
                row = {"lp": name, "mode": mode, "n": n, "max_iter": max_iter,
                       "batch_lps_per_s": round(n / t_b, 2), "loop_same_opts_lps_per_s": round(k / t_e, 2),
                       "loop_hybrid_lps_per_s": round(k / t_h, 2),
                       "speedup_vs_same_opts": round((n / t_b) / (k / t_e), 2), "speedup_vs_hybrid": round((n / t_b) / (k / t_h), 2),
                       "batch_us_per_iter": round(1e6 * t_b / max(it_b, 1), 1), "single_us_per_iter": round(1e6 * t_e / max(it_e, 1), 1),
                       "batch_ms": round(t_b * 1e3, 1), "loop_timed": k,
                       "same_as_same_opts": all(outcome(x) == outcome(y) for x, y in zip(batch[:k], loop_e)),
                       "same_kind_as_hybrid": all(outcome(x)[0] == outcome(y)[0] for x, y in zip(batch[:k], loop_h))}
                out["rows"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

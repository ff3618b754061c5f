"""tools/batch_throughput.py — LPs per second of solve_batch against a loop of solve(), for N permuted copies of AFIRO and
ADLITTLE (tests/helpers.permuted_fixture), N in {1, 64, 256, 1024}, both solvers.  Prints one JSON line.

Solvers are default-constructed (max_iter 1000, as ::default()).  The loop runs one solve() after another, so its rate does not depend on N: it is timed on the first min(N, 64) problems
of each set (`loop_timed`).  Each timing is the best of `--reps` after one untimed warm-up call of the same shape.
The batch's outcomes are checked against the loop's on the problems the loop timed (kind and iteration counts)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ellp_amd import DualSimplexSolver, PrimalSimplexSolver, Problem  # noqa: E402
from helpers import GOLDEN, permuted_fixture, read_mps  # noqa: E402


def outcome(r):
    return ("error", type(r).__name__) if isinstance(r, Exception) else (r.kind, tuple(r.iters))


def best_of(fn, reps):
    fn()  # warm-up
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,256,1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-max", type=int, default=64)
    a = ap.parse_args()
    out = {"what": "LPs per second through the user API: solve_batch(ps) against [solve(p) for p in ps]", "rows": []}
    for name in ("afiro", "adlittle"):
        fx = read_mps(os.path.join(GOLDEN, "netlib", name + ".mps"))
        for n in [int(s) for s in a.sizes.split(",")]:
            rng = np.random.default_rng(1000 + n)
            ps = [Problem.from_fixture(permuted_fixture(fx, rng)) for _ in range(n)]
            for sname, S in (("primal", PrimalSimplexSolver), ("dual", DualSimplexSolver)):
                solver = S()  # max_iter 1000 per phase: some orders make the dual cycle
                batch = []
                t_b = best_of(lambda: batch.__setitem__(slice(None), solver.solve_batch(ps)), a.reps)
                k = min(n, a.loop_max)
                loop = []

                def run_loop():
                    loop.clear()
                    for p in ps[:k]:
                        try:
                            loop.append(solver.solve(p))
                        except Exception as e:  # noqa: BLE001 — an outcome like any other
                            loop.append(e)
                t_l = best_of(run_loop, a.reps)
                same = all(outcome(x) == outcome(y) for x, y in zip(batch[:k], loop))
                row = {"lp": name, "n": n, "solver": sname, "batch_lps_per_s": round(n / t_b, 1),
                       "loop_lps_per_s": round(k / t_l, 1), "speedup": round((n / t_b) / (k / t_l), 2),
                       "batch_ms": round(t_b * 1e3, 2), "loop_timed": k, "same_outcomes": same}
                out["rows"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Wall time of PrimalSimplexSolver.solve_batch (both phases of every problem in one ellp_batch_primal_solve call), best of
5, on homogeneous batches (permuted AFIRO, permuted ADLITTLE), on a heterogeneous batch of random LPs of 3 to 120 rows —
where problems whose phase 1 is short no longer wait for the longest one — and on ADLITTLE x 3 (k_mid, pipeline 3).  Prints
one JSON line per batch, with the launch rounds and the uploaded bytes of the call where the library reports them, and a
digest of the outcomes (kinds, iteration counts, objective bits), so that runs of two checkouts can be compared.

    python tools/batch_two_phase_time.py [--tree OTHER_CHECKOUT] [--label NAME --out profiles/batch_two_phase_time.json]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="the checkout whose ellp_amd package is measured (built); default: this one")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None, help="JSON file to merge the rows into, under --label")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    sys.path.append(ROOT)  # the oracle package the test helpers import
    import ellp_amd
    from ellp_amd import _engine as E
    from helpers import GOLDEN, blockdiag, permuted_fixture, read_mps
    from test_gpu_batch import random_lp

    afiro = read_mps(os.path.join(GOLDEN, "netlib", "afiro.mps"))
    adl = read_mps(os.path.join(GOLDEN, "netlib", "adlittle.mps"))
    rng = np.random.default_rng(20260)
    batches = [
        ("256 x permuted AFIRO", {}, [permuted_fixture(afiro, np.random.default_rng(500 + s)) for s in range(256)]),
        ("256 x permuted ADLITTLE", {}, [permuted_fixture(adl, np.random.default_rng(600 + s)) for s in range(256)]),
        ("256 x random LPs of 3-120 rows", {}, [random_lp(np.random.default_rng(700 + s), int(rng.integers(3, 121))) for s in range(256)]),
        ("16 x ADLITTLE x 3, pipeline 3", {"pipeline": 3}, [permuted_fixture(blockdiag(adl, 3), np.random.default_rng(800 + s)) for s in range(16)]),
    ]
    rows = []
    for name, eng, fxs in batches:
        ps = [ellp_amd.Problem.from_fixture(fx) for fx in fxs]
        solver = ellp_amd.PrimalSimplexSolver.new(100000, **eng)
        solver.solve_batch(ps[:2])  # warm-up: code objects, pinned pool
        solver.solve_batch(ps)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            res = solver.solve_batch(ps)
            ts.append(time.perf_counter() - t0)
        h = hashlib.sha1()
        kinds = {}
        for r in res:
            if isinstance(r, Exception):
                h.update(repr(r).encode())
                kinds["error"] = kinds.get("error", 0) + 1
                continue
            kinds[r.kind] = kinds.get(r.kind, 0) + 1
            h.update(f"{r.kind} {r.iters}".encode())
            if r.kind == ellp_amd.SolverResult.Optimal:
                h.update(np.float64(r.solution.obj()).tobytes())
                h.update(r.solution.x().tobytes())
        row = dict(batch=name, N=len(ps), best_ms=round(1e3 * min(ts), 3), times_ms=[round(1e3 * t, 3) for t in ts],
                   spread_ms=round(1e3 * (max(ts) - min(ts)), 3), kinds=kinds, digest=h.hexdigest()[:16],
                   max_iters=[max((r.iters[k] for r in res if not isinstance(r, Exception)), default=0) for k in (0, 1)])
        if hasattr(E, "batch_primal_info"):
            info = E.batch_primal_info()
            row.update(launch_rounds=info["rounds"], upload_bytes=info["upload_bytes_total"], chunks=info["chunks"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
        doc[a.label] = rows
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

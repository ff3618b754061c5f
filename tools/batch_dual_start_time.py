"""Wall time of the dual's batched phase-1 starts (ellp_batch_dual_phase1_start) against N sequential
ellp_engine_create_dual_phase1 + ellp_engine_read_point calls, on permuted netlib replications, with the options that give
the dual k_mid above 128 rows (bound flipping).  Checks that both give the same bits.  Prints one JSON line per row.

    python tools/batch_dual_start_time.py [--sizes 1,64,256] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import GOLDEN, blockdiag, known_answers, permuted_fixture, read_mps  # noqa: E402
from oracle import ellp_oracle as eo  # noqa: E402
from ellp_amd import _engine as E  # noqa: E402

LPS = [("blend", 2), ("adlittle", 3), ("adlittle", 6)]


def args_of(name, copies, seed):
    ka = next(p for p in known_answers()["netlib"] if p["name"] == name)
    fx = permuted_fixture(blockdiag(read_mps(os.path.join(GOLDEN, ka["file"])), copies), np.random.default_rng(seed))
    d1, err = eo.dual_phase1(eo.Problem.from_fixture(fx))
    assert d1 is not None and not err, err
    v = d1.view()
    return (v.m, v.n, v.A.copy(), v.c.copy(), v.b.copy(), v.kind.copy(), v.lb.copy(), v.ub.copy(), v.B.copy(), v.N[:v.nN].copy())


def sequential(problems, opts):
    out = []
    for m, n, A, c, b, kind, lb, ub, B, N in problems:
        eng = E.Engine.dual_phase1(m, n, A, c, b, kind, lb, ub, B, N, opts)
        fp = eng.read_point()
        out.append((fp.x.copy(), fp.Nb.copy(), fp.y.copy(), fp.d.copy()))
        eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,256")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    opts = E.default_opts(flags=E.FLAG_DUAL_BOUND_FLIPPING | E.FLAG_DUAL_MAX_VIOLATION)
    for name, copies in LPS:
        pool = [args_of(name, copies, 100 + s) for s in range(8)]  # 8 variable orders, reused round-robin
        for N in [int(s) for s in a.sizes.split(",")]:
            probs = [pool[k % len(pool)] for k in range(N)]
            E.batch_dual_phase1_start(probs[:1], opts)  # warm-up: code objects, pinned pool
            sequential(probs[:1], opts)
            tb, ts = [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                res = E.batch_dual_phase1_start(probs, opts)
                tb.append(time.perf_counter() - t0)
                t0 = time.perf_counter()
                seq = sequential(probs, opts)
                ts.append(time.perf_counter() - t0)
            same = all(r[0] == E.OPTIMAL and r[3].x.tobytes() == s[0].tobytes() and r[3].Nb.tobytes() == s[1].tobytes() and
                       r[3].y.tobytes() == s[2].tobytes() and r[3].d.tobytes() == s[3].tobytes() for r, s in zip(res, seq))
            print(json.dumps(dict(lp=f"{name}x{copies}", m=probs[0][0], n=probs[0][1], N=N, batch_ms=round(1e3 * min(tb), 2),
                                  sequential_ms=round(1e3 * min(ts), 2), speedup=round(min(ts) / min(tb), 2),
                                  starts_per_s_batch=round(N / min(tb), 1), identical=same)), flush=True)


if __name__ == "__main__":
    main()

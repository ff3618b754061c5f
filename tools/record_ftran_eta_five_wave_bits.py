"""tools/record_ftran_eta_five_wave_bits.py — digests of the two-launch primal loop at the shapes that bound the
320-thread k_ftran_eta (a store-free deciding wave beside four streaming waves).

    python tools/record_ftran_eta_five_wave_bits.py [--out tests/golden/ftran_eta_five_wave_bits.json]

Run on the build whose results are the reference (the commit BEFORE the fifth wave); tests/test_gpu_ftran_eta_five_waves.py
replays the same walks on the current build and compares.  The walk is tools/record_ftran_eta_bits.py's (300 pivots in
slices of 1, 2, 7 and 64, the point read back after every slice); only the case table is this file's: shapes that fixture
does not reach."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from record_ftran_eta_bits import PIVOTS, SEED, SLICES, walk  # noqa: E402

# m, n, ld, the template parameter NR of k_ftran_eta at that ld (ceil(ld / 512), the next of 1, 2, 4, 8), rows per block
SHAPES = ((1559, 1700, 1568, 4, 4),   # half = 784: 16 live lanes in the fourth chunk; the last block has 3 rows
          (2048, 2200, 2048, 4, 4),   # the upper edge of the 320-thread kernel: every lane of all four chunks live
          (2049, 2200, 2064, 8, 4))   # the first ld of the 256-thread whole-block body: guards the launch-geometry switch
# name -> (m, n, extra options)
CASES = {"%dx%d" % (_m, _n): (_m, _n, {}) for _m, _n, _ld, _nr, _rows in SHAPES}
CASES["1559x1700_refactor50"] = (1559, 1700, {"refactor_period": 50})  # maintenance drops an open iteration
GOLDEN = os.path.join(ROOT, "tests", "golden", "ftran_eta_five_wave_bits.json")


def main():
    from ellp_amd import _engine as E
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    rec = {"seed": SEED, "pivots": PIVOTS, "slices": list(SLICES), "cases": {}}
    for name, (m, n, extra) in CASES.items():
        rec["cases"][name] = walk(E, m, n, extra, False)
        last = rec["cases"][name][-1]
        print("%-24s %3d records, last: status %d after %d iterations" % (name, len(rec["cases"][name]), last["status"], last["iters"]),
              flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(rec, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()

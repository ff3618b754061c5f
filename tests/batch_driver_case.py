"""The items of the one call that walks every branch of the batched calls' shared chunk driver, used by
test_gpu_batch_postsolve.py, test_gpu_batch_start.py and test_gpu_batch_ranging.py: a refused item (made by each test from
the 17-row one), two batched items, one on the single path inside the call, one more batched item, cut into chunks by the
budget."""
_DRIVER = {}

# the 128-row item (A_B alone: 128 KiB) is a chunk of its own behind the other two batched items
DRIVER_BUDGET = 64 << 10


def driver_items():
    """[3 rows, 17 rows, 129 rows, 128 rows] as FlatProblems, n_c == n, a few pivots from their starts.  3 rows: the smallest
    odd m under one 16-row pad; 128 / 129: the boundary between the batched kernel and the single path"""
    if not _DRIVER:
        from ellp_amd import _engine as E
        from ellp_amd import synth
        fps = []
        for m, n in ((3, 8), (17, 20), (129, 40), (128, 40)):
            f = synth.primal_phase1_flat(20260601 + m, m, n)
            fps.append(E.FlatProblem(f["m"], f["n"], f["n_c"], f["A"], f["c"], f["b"], f["kind"], f["lb"], f["ub"], f["x"], f["B"], f["N"], f["Nb"]))
        res = E.batch_solve_with_initial(E.ENGINE_PRIMAL, [fps[0], fps[1], fps[3]], E.default_opts(max_iter=60))
        assert all(st >= 0 for st, _, _ in res), res
        s, _, msg = E.primal_solve_with_initial(fps[2], E.default_opts(max_iter=40))
        assert s >= 0, (s, msg)
        assert [fp.m for fp in fps] == [3, 17, 129, 128] and all(fp.n_c == fp.n for fp in fps)
        _DRIVER["fps"] = fps
    return _DRIVER["fps"]

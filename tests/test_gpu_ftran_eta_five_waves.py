"""k_ftran_eta<1,2,4> with 320 threads: a fifth, store-free wave folds and hands the entering column to four streaming
waves.  The two-launch primal loop must leave the bytes it left before, slice for slice, at the shapes
tests/test_gpu_ftran_eta_handoff.py does not reach.

tests/golden/ftran_eta_five_wave_bits.json holds sha256 digests of x, B, N and Nb (plus status and iteration count) after
every slice of the walks tools/record_ftran_eta_five_wave_bits.py defines, recorded on the GPU from the build of the commit
before the fifth wave (256 threads, wave 0 folds and stores).  Each walk: 300 pivots in slices of 1, 2, 7 and 64 with the
point read back after every slice.  The shapes: ld = 1568 (NR = 4 with 16 live lanes in the fourth chunk, a last block of
three rows), once more with refactor_period = 50 (maintenance drops an open iteration); ld = 2048 (the upper edge of the
320-thread kernel, every lane live); ld = 2064 (NR = 8: still the 256-thread whole-block body, so a launch that took 320
threads one instantiation too far, or 256 one too early, shows here and at 2048)."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import record_ftran_eta_five_wave_bits as rec  # noqa: E402

with open(rec.GOLDEN) as _fh:
    GOLD = json.load(_fh)


def _engine():
    from ellp_amd import _engine as E
    return E


def test_fixture_covers_the_cases():
    assert GOLD["seed"] == rec.SEED and GOLD["pivots"] == rec.PIVOTS and tuple(GOLD["slices"]) == rec.SLICES
    assert sorted(GOLD["cases"]) == sorted(rec.CASES)


@pytest.mark.parametrize("m,n,ld,nr,rows", rec.SHAPES)
def test_shapes_run_the_intended_instantiation(m, n, ld, nr, rows):
    """the two-launch loop, the instantiation that holds ceil(ld / 512) double2 per thread and row (the next of 1, 2, 4, 8),
    the rows per block, and the geometry the shape was chosen for"""
    E = _engine()
    s, plan, msg = E.engine_plan(E.ENGINE_PRIMAL, m, n + m, E.default_opts(max_iter=None, pipeline=2))
    assert s == E.OPTIMAL, msg
    assert plan["lagged"] == 1 and int(plan["ld"]) == ld and int(plan["upd2_rows"]) == rows
    need = ((ld >> 1) + 255) // 256
    assert min(k for k in (1, 2, 4, 8) if need <= k) == nr
    if m == 1559:
        assert ld // 2 - 3 * 256 == 16 and m % rows == 3  # 16 live lanes in the fourth chunk; a last block of three rows
    if m == 2048:
        assert ld // 2 == 4 * 256                          # every lane of all four chunks holds a double2
    if m == 2049:
        assert ld // 2 > 4 * 256                           # one double2 too many for four chunks: the whole-block body


@pytest.mark.parametrize("name", sorted(rec.CASES))
def test_same_bytes_as_before_the_fifth_wave(name):
    E = _engine()
    m, n, extra = rec.CASES[name]
    got = rec.walk(E, m, n, extra, False)
    want = GOLD["cases"][name]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "slice %d of %s: %r != %r" % (k, name, g, w)
    assert got[-1]["status"] == E.MAXITER

"""k_ftran_eta with the entering column handed from one deciding wave to three streaming waves through LDS: the
two-launch primal loop must leave the bytes it left before, slice for slice.

tests/golden/ftran_eta_parent_bits.json holds sha256 digests of x, B, N and Nb (plus status and iteration count) after
every slice of the walks tools/record_ftran_eta_bits.py defines, recorded on the GPU from the build of the commit before
the hand-off.  Each walk: 300 pivots in slices of 1, 2, 7 and 64 with the point read back after every slice (open
iterations, the closing kernel, a first launch that has no eta update to apply), once with the default maintenance and once
with refactor_period = 50 (maintenance drops an open iteration); at 384 x 600 also to the optimal end (no entering
candidate: all four waves leave together, the end is handed to the next kernel).  The shapes take the unsharded
k_ftran_eta<1>, <2> and <4> through partly filled waves, ld != m and a last block of one row."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import record_ftran_eta_bits as rec  # noqa: E402

with open(rec.GOLDEN) as _fh:
    GOLD = json.load(_fh)


def _engine():
    from ellp_amd import _engine as E
    return E


def test_fixture_covers_the_cases():
    assert GOLD["seed"] == rec.SEED and GOLD["pivots"] == rec.PIVOTS and tuple(GOLD["slices"]) == rec.SLICES
    assert sorted(GOLD["cases"]) == sorted(rec.CASES)


@pytest.mark.parametrize("m,n,nr", rec.SHAPES)
def test_shapes_run_the_intended_instantiation(m, n, nr):
    """the two-launch loop, the instantiation that holds ceil(ld / 512) double2 per thread and row (the next of 1, 2, 4),
    and the geometry the shape was chosen for"""
    E = _engine()
    s, plan, msg = E.engine_plan(E.ENGINE_PRIMAL, m, n + m, E.default_opts(max_iter=None, pipeline=2))
    assert s == E.OPTIMAL, msg
    ld = int(plan["ld"])
    need = ((ld >> 1) + 255) // 256
    assert plan["lagged"] == 1 and min(k for k in (1, 2, 4) if need <= k) == nr
    if m == 384:
        assert ld == 384 and ld // 2 == 192            # 192 of 256 lanes hold a double2
    if m == 520:
        assert ld == 528 and ld // 2 - 256 == 8        # 8 live lanes in the second chunk
    if m == 1041:
        assert ld == 1056 and m % int(plan["upd2_rows"]) == 1 and int(plan["upd2_rows"]) == 4  # a last block of one row


@pytest.mark.parametrize("name", sorted(rec.CASES))
def test_same_bytes_as_before_the_handoff(name):
    E = _engine()
    m, n, extra, to_end = rec.CASES[name]
    got = rec.walk(E, m, n, extra, to_end)
    want = GOLD["cases"][name]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "slice %d of %s: %r != %r" % (k, name, g, w)
    if to_end:
        assert got[-1]["status"] == E.OPTIMAL
    else:
        assert got[-1]["status"] == E.MAXITER

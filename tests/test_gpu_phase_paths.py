"""The phase hand-offs of the resident engine (ellp_engine_create_primal_phase1 / _dual_phase1, ellp_engine_rephase,
ellp_engine_dual_rephase, and the re-arms inside ellp_engine_run: the redo from the snapshot, the certified hybrid's
hand-over) decide what they decided before: per path the same statuses, iteration / pivot / bound-flip counts and
objective bits of every run call, the same status and message of every hand-off call, and after each phase the same
point (digests of x, B, N, Nb; dual: y and d) and the same host counters.

tests/golden/phase_paths_parent.json holds those values as tools/record_phase_paths.py recorded them on the GPU from the
build of the commit before the hand-offs were taken apart; every value is compared for equality.  The cases (defined in
the recorder): primal phase 1 -> rephase -> phase 2 at 48 rows on (a) three launches, (b) two launches (the lagged fields),
(c) partial pricing in four segments (the window restarts), (d) steepest edge, (e) k_small; at 160 rows (f) the certified
hybrid, (g) the same with a forced redo in phase 1 and (g2) with one in phase 2 alone; dual phase 1 -> dual_rephase ->
phase 2 at 150 rows on (h) three launches (y from BTRAN) and (i) the hybrid (y from k_mid's LU); (j) k_small at 48 rows,
where dual_rephase is refused; (k) the exact loop at 1,040 rows, three iterations, then the point made from the rows-LU
and refused by the assertion on d; (l) what the hand-offs refuse, status and text."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import record_phase_paths as rec  # noqa: E402

with open(rec.GOLDEN) as _fh:
    GOLD = json.load(_fh)


def test_fixture_covers_the_cases():
    assert GOLD["seed"] == rec.SEED
    assert sorted(GOLD["cases"]) == sorted(rec.CASES)


@pytest.mark.parametrize("name", sorted(rec.CASES))
def test_same_hand_offs_as_the_parent(name, monkeypatch):
    from ellp_amd import _engine as E
    for k, v in rec.CASES[name]["env"].items():
        monkeypatch.setenv(k, v)  # ELLP_FORCE_REDO is read when a solve ends
    got = rec.run_case(E, name)
    want = GOLD["cases"][name]
    assert rec.took_path(E, name, got) is None, (name, got)
    assert sorted(got) == sorted(want)
    for part in sorted(want):
        assert got[part] == want[part], "%s of %s: %r != %r" % (part, name, got[part], want[part])
    assert got == want

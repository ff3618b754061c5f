"""The host driver of the explicit-inverse engine (ellp_engine_run and what it calls) decides what it decided before: per
path the same statuses, iteration / pivot / bound-flip counts and objective bits slice by slice, the same end point, and
the same host counters (maintenance requests serviced, refreshes, rebuilds, resyncs, drift checks, the hybrid's takeovers
and redos) — a driver that refreshes one iteration late ends on the same vertex, its counters differ.

tests/golden/run_paths_parent.json holds those values as tools/record_run_paths.py recorded them on the GPU from the
build of the commit before the run loop was taken apart; every value is compared for equality.  The cases (defined in the
recorder): (a) primal, three launches, polled, with a serviced maintenance request; (b) primal, two launches, look-ahead;
(c) the same in slices of 7 up to max_iter = 40 (the hst_fresh shortcut, an open iteration carried across slices, the
budget close); (d) dual, fused with the folded close; (e) dual, fused, a closing launch per iteration, polled; (f) the
certified hybrid with a takeover at the terminal status; (g) the same with the redo from the snapshot; (h) (a) with event
brackets, the kernel_calls per id; (i) periodic refreshes and drift checks inside the batches."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import record_run_paths as rec  # noqa: E402

with open(rec.GOLDEN) as _fh:
    GOLD = json.load(_fh)


def test_fixture_covers_the_cases():
    assert GOLD["seed"] == rec.SEED
    assert sorted(GOLD["cases"]) == sorted(rec.CASES)


@pytest.mark.parametrize("name", sorted(rec.CASES))
def test_same_decisions_as_the_parent(name, monkeypatch):
    from ellp_amd import _engine as E
    for k, v in rec.CASES[name]["env"].items():
        monkeypatch.setenv(k, v)  # read at creation (ELLP_ILL_TOL, ELLP_DRIFT_EVERY) or when the solve ends (ELLP_FORCE_REDO)
    got = rec.run_case(E, name)
    want = GOLD["cases"][name]
    assert rec.took_path(E, name, got) is None, (name, got)
    assert len(got["runs"]) == len(want["runs"])
    for k, (g, w) in enumerate(zip(got["runs"], want["runs"])):
        assert g == w, "ellp_engine_run call %d of %s: %r != %r" % (k, name, g, w)
    assert got["counters"] == want["counters"]
    assert got == want

"""Which status every Winograd entry point returns for a defective call -- and which one wins where two defects meet -- held to the
recorded tests/golden/wino_status.json (cases: tests/wino_status_cases.py)."""
import ctypes as C
import json

import pytest
import torch

import wino_status_cases as W


def test_winograd_entry_points_return_the_recorded_status_for_every_defect_and_pair():
    """Every case is refused before anything is enqueued, so made-up pointers are never dereferenced; where a GPU is present the test
    still does not run, so that a tuple some change made acceptable can never reach a launch on a shared machine."""
    if torch.cuda.is_available():
        pytest.skip("made-up pointers: only where no launch can succeed")
    from objectdetection_ssd_amd import _lib, ops
    with open(W.FIXTURE) as f:
        want = json.load(f)
    assert set(want) == set(W.ENTRIES)
    for entry in W.ENTRIES:
        assert list(want[entry]) == sorted(la for la, _ in W.cases(entry)), entry      # the fixture covers exactly the grid
        assert not [la for la, s in want[entry].items() if s in (0, -4)], entry           # ... and holds refusals only
    got = W.statuses(_lib.load(), ops.make_geom, C.byref)
    wrong = [(e, la, got[e][la], s) for e in want for la, s in want[e].items() if got[e][la] != s]
    assert not wrong, f"{len(wrong)} statuses differ (entry, defects, got, recorded): {wrong[:20]}"

"""Which status every direct-convolution entry point returns for a defective call -- and which one wins where two defects meet -- held
to the recorded tests/golden/conv_status.json (cases: tests/conv_status_cases.py), and the refusals that recording could not hold."""
import ctypes as C
import json

import pytest
import torch

import conv_status_cases as V
from status_grid import ODD_PTR

SSD_ERR_BAD_SHAPE, SSD_ERR_ALIGN = -1, -5                 # include/ssd_gfx950.h


def _lib_or_skip():
    """Every case is refused before anything is enqueued, so made-up pointers are never dereferenced; where a GPU is present the tests
    still do not run, so that a tuple some change made acceptable can never reach a launch on a shared machine."""
    if torch.cuda.is_available():
        pytest.skip("made-up pointers: only where no launch can succeed")
    from objectdetection_ssd_amd import _lib, ops
    return _lib.load(), ops


def test_direct_convolution_entry_points_return_the_recorded_status_for_every_defect_and_pair():
    lib, ops = _lib_or_skip()
    grid = V.GRID
    with open(grid.fixture) as f:
        want = json.load(f)
    assert set(want) == set(V.ENTRIES)
    for entry in V.ENTRIES:
        assert list(want[entry]) == sorted(la for la, _ in grid.cases(entry)), entry   # the fixture covers exactly the grid
        assert not [la for la, s in want[entry].items() if s in (0, -4)], entry           # ... and holds refusals only
    got = grid.statuses(lib, ops.make_geom, C.byref)
    wrong = [(e, la, got[e][la], s) for e in want for la, s in want[e].items() if got[e][la] != s]
    assert not wrong, f"{len(wrong)} statuses differ (entry, defects, got, recorded): {wrong[:20]}"


def test_halo_entries_refuse_misaligned_operands_and_weight_gradients_refuse_64_taps_before_any_launch():
    """The halo entries launch the kernel the f32x3 entries launch and share their alignment rule.  More than 49 taps are refused
    before the main kernel is enqueued: on a machine without a GPU a launch would answer SSD_ERR_LAUNCH instead."""
    lib, ops = _lib_or_skip()
    grid = V.GRID
    sizes = grid.sizes(lib, ops.make_geom, C.byref)
    for entry, source, planes in (("ssd_conv3x3_halo_fwd_bf16", "x", "w_ohwi"), ("ssd_conv3x3_halo_dgrad_bf16", "dy", "w_ihwo")):
        for name in (source, planes):
            args, keep = grid.arguments(entry, {name: ODD_PTR}, sizes, ops.make_geom, C.byref)
            assert getattr(lib, entry)(*args) == SSD_ERR_ALIGN, (entry, name)
    taps64 = {"g.k": 8, "g.pad": 3}
    sizes = {"Zw": lib.ssd_conv2d_wgrad_workspace(C.byref(ops.make_geom(**dict(V.GEOM, k=8, pad=3))))}     # so the workspace is no defect
    assert 0 < sizes["Zw"] <= 1 << 24                        # ... nor the fixed size ssd_conv2d_wgrad's tuple carries
    for entry in ("ssd_conv2d_wgrad", "ssd_conv2d_wgrad_bf16", "ssd_conv3x3_wgrad_bf16t"):
        args, keep = grid.arguments(entry, taps64, sizes, ops.make_geom, C.byref)
        assert getattr(lib, entry)(*args) == SSD_ERR_BAD_SHAPE, entry

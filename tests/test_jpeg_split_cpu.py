"""Host side of the many-lanes-per-segment JPEG decode (no GPU): the two C symbols are declared, bound and exported; ops.jpeg_decode_
refuses a bad `entropy` and a bad `subsequence_bytes` before it touches a device; the split workspace keeps the segment workspace's
layout in front; `jpeg_entropy_auto` chooses by the batch's longest segment."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import jpeg_ref as J
import jpeg_split_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_split_symbols_are_declared_bound_and_exported():
    from objectdetection_ssd_amd import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ssd_gfx950.h")).read()
    declared = set(re.findall(r"\b(ssd_[a-z0-9_]+)\s*\(", hdr))
    for name, n_args in (("ssd_jpeg_decode_split_workspace", 5), ("ssd_jpeg_decode_split_u8", 15)):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name][1]) == n_args
    assert len(_lib.SIGNATURES["ssd_jpeg_decode_u8"][1]) == 13 and lib.ssd_abi_version() == 1
    assert _lib.SIGNATURES["ssd_jpeg_decode_split_u8"][1][:13] == _lib.SIGNATURES["ssd_jpeg_decode_u8"][1]


def test_jpeg_decode_refuses_bad_modes_before_touching_a_device():
    from objectdetection_ssd_amd import ops
    host, descs, segs, _ = S.layout([J.matrix()[0][2]])
    arena = torch.from_numpy(host)                                   # a host tensor: the device check would raise RuntimeError
    for bad in ("lanes", "", None, "SPLIT"):
        with pytest.raises(ValueError, match="entropy"):
            ops.jpeg_decode_(arena, descs, segs, entropy=bad)
    for bad in (0, 4, 6, 10, 4100, -8, 128.0, "128", True):
        with pytest.raises(ValueError, match="subsequence_bytes"):
            ops.jpeg_decode_(arena, descs, segs, entropy="split", subsequence_bytes=bad)
    with pytest.raises(RuntimeError):
        ops.jpeg_decode_(arena, descs, segs, entropy="split", subsequence_bytes=8)
    assert ops.JPEG_SUBSEQUENCE_BYTES % 4 == 0 and 8 <= ops.JPEG_SUBSEQUENCE_BYTES <= 4096


def test_split_workspace_keeps_the_segment_layout_in_front():
    from objectdetection_ssd_amd import _lib
    lib = _lib.load()
    streams = [d for _, _, d in J.matrix()][::5] + [S.voc_like()]
    _, descs, segs, _ = S.layout(streams)
    B = len(streams)
    base = lib.ssd_jpeg_decode_workspace(C.byref(descs), B)
    want = [(d.coef_offset, d.plane_offset) for d in descs]
    assert base > 0
    sizes = []
    for sub in (8, 128, 4096):
        for d in descs:
            d.coef_offset = d.plane_offset = -1
        n = lib.ssd_jpeg_decode_split_workspace(C.byref(descs), B, segs.ctypes.data, int(segs.size), sub)
        assert n >= base and [(d.coef_offset, d.plane_offset) for d in descs] == want, sub
        sizes.append(n)
    assert sizes[0] > sizes[1] >= sizes[2]                           # more subsequences, more records
    for sub in (0, 4, 10, 4100):
        assert lib.ssd_jpeg_decode_split_workspace(C.byref(descs), B, segs.ctypes.data, int(segs.size), sub) == 0
    assert lib.ssd_jpeg_decode_split_workspace(None, B, segs.ctypes.data, int(segs.size), 128) == 0
    assert lib.ssd_jpeg_decode_split_workspace(C.byref(descs), B, None, int(segs.size), 128) == 0
    assert lib.ssd_jpeg_decode_split_workspace(C.byref(descs), B, segs.ctypes.data, int(segs.size) - 1, 128) == 0
    descs[1].h_samp = 4
    assert lib.ssd_jpeg_decode_split_workspace(C.byref(descs), B, segs.ctypes.data, int(segs.size), 128) == 0


def test_entropy_auto_chooses_by_the_longest_segment():
    from objectdetection_ssd_amd import _lib, ops
    limit = ops.JPEG_SPLIT_AUTO_BYTES
    assert isinstance(limit, int) and limit > 0
    descs = (_lib.JpegDesc * 2)()
    descs[0].seg_first, descs[0].n_segments, descs[0].stream_bytes = 0, 1, 100
    descs[1].seg_first, descs[1].n_segments, descs[1].stream_bytes = 1, 1, limit
    segs = np.zeros(2, np.int32)
    assert ops.jpeg_entropy_auto(descs, segs) == "segment"
    descs[1].stream_bytes = limit + 1
    assert ops.jpeg_entropy_auto(descs, segs) == "split"
    # the same bytes behind restart markers: three segments, none longer than the limit (a segment ends 2 bytes before the next)
    descs[1].n_segments, descs[1].stream_bytes = 3, 3 * limit
    segs = np.asarray([0, 0, limit, 2 * limit], np.int32)
    assert ops.jpeg_entropy_auto(descs, segs) == "segment"
    descs[1].stream_bytes = 3 * limit + 1                            # the last segment is one byte over
    assert ops.jpeg_entropy_auto(descs, segs) == "split"
    with pytest.raises(ValueError):
        ops.jpeg_entropy_auto(descs, segs[:3])

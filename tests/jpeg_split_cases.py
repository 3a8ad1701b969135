"""Fixtures of the many-lanes-per-segment JPEG tests, beside `jpeg_ref.matrix()`: the VOC-like image (500 x 375, quality 75, 4:2:0, no
restart markers: about 40 KB of entropy-coded data in ONE segment), the two chunk-boundary streams (an FF at entropy offset = 1023 and
1022 mod 1024, so that a stuffed pair straddles a de-stuffing step of any power of two up to 1024), and the case file of
tools/jpeg_split_host_check.cpp."""
import struct

import numpy as np

import jpeg_ref as J

SUBSEQ_SIZES = (8, 12, 32, 128, 256)
_cache = {}


def voc_like_pixels():
    if "px" not in _cache:
        rng = np.random.default_rng(3)
        yy, xx = np.mgrid[0:375, 0:500]
        base = np.stack([127.5 + 100 * np.sin(xx / 9.0 + yy / 17.0), 127.5 + 100 * np.cos(xx / 23.0), 127.5 + 100 * np.sin(yy / 11.0)], -1)
        _cache["px"] = np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)
    return _cache["px"]


def voc_like(**kw):
    key = ("voc", tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = J.encode(voc_like_pixels(), quality=75, subsampling="4:2:0", **kw)
    return _cache[key]


def chunk_boundary_streams():
    """[(bytes, entropy offset of an FF, that offset mod 1024)] for seeds 6 and 2"""
    if "cb" not in _cache:
        out = []
        for s, at in ((6, 13311), (2, 11262)):
            px = np.random.default_rng(1000 + s).integers(0, 256, (75, 97, 3), dtype=np.uint8)
            out.append((J.encode(px, quality=95, subsampling="4:4:4"), at, at % 1024))
        _cache["cb"] = out
    return _cache["cb"]


def entropy_bytes(data):
    hdr = J.parse(data)
    return data[hdr["data_begin"]:hdr["data_end"]]


def case(data, expect_good):
    """one case of the file tools/jpeg_host_check.cpp and tools/jpeg_split_host_check.cpp read"""
    hdr = J.parse(data)
    assert hdr is not None
    nc = hdr["n_components"]
    stream = data[hdr["data_begin"]:hdr["data_end"]]
    segs = [o - hdr["data_begin"] for o in hdr["seg_offsets"]]
    out = struct.pack("<9i", hdr["width"], hdr["height"], nc, hdr["h_samp"], hdr["v_samp"], hdr["restart_interval"], len(segs),
                      len(stream), 0 if expect_good else 1)
    out += struct.pack("<6i", *(hdr["dc_sel"] + [0] * (3 - nc)), *(hdr["ac_sel"] + [0] * (3 - nc)))
    for key in ((0, 0), (0, 1), (1, 0), (1, 1)):
        if key in hdr["huff_tables"]:
            bits, vals = hdr["huff_tables"][key]
            out += struct.pack("<i", len(vals)) + bits.tobytes() + vals.tobytes()
        else:
            out += struct.pack("<i", 0) + bytes(16)
    out += struct.pack(f"<{len(segs)}i", *segs) + stream
    if expect_good:
        out += b"".join(c.astype("<i2").tobytes() for c in J.decode_coefficients(data, hdr))
    return out


def ref_says_corrupt(data):
    try:
        J.decode_coefficients(data, J.parse(data))
        return False
    except J.Corrupt:
        return True


GUARD = 64
PATTERN = 0xA5


def layout(streams):
    """The guard-byte arena of tests/test_jpeg_decode_gpu.py: GUARD bytes of PATTERN on either side of every pixel slot (slots at
    odd, unaligned offsets), the entropy-coded data behind them.  -> (host arena, descs, segs, [(slot offset, h, w)])"""
    from objectdetection_ssd_amd import _lib, ops
    from objectdetection_ssd_amd.Dataset import parse_jpeg
    hdrs = [parse_jpeg(d) for d in streams]
    assert all(h is not None for h in hdrs)
    at, slots = 0, []
    for h in hdrs:
        at += GUARD
        slots.append((at, h.height, h.width))
        at += h.height * h.width * 3
    at += GUARD
    stream_at = []
    for h in hdrs:
        stream_at.append(at)
        at += h.data_end - h.data_begin + 3                                       # unaligned on purpose
    host = np.full(at + GUARD, PATTERN, np.uint8)
    descs = (_lib.JpegDesc * len(hdrs))()
    segs = []
    for d, h, data, (so, hh, ww), sa in zip(descs, hdrs, streams, slots, stream_at):
        host[sa:sa + h.data_end - h.data_begin] = np.frombuffer(data, np.uint8)[h.data_begin:h.data_end]
        ops.jpeg_fill_desc(d, h, sa, so, hh * ww * 3, len(segs))
        segs.extend(int(o) - h.data_begin for o in h.seg_offsets)
    return host, descs, np.asarray(segs, np.int32), slots

"""csrc/jpeg_entropy.h -- the segment decoder the GPU runs one lane per restart segment -- compiled for the CPU inside
tools/jpeg_host_check.cpp, a stand-alone program, with the host compiler's address and undefined-behaviour sanitizers, and run as a
subprocess on streams dumped here: the fixture matrix (coefficients must equal tests/jpeg_ref.py's) and the corrupt streams
(truncated, bit-flipped; must end clean under the sanitizers with a non-zero status wherever the restatement finds the stream
corrupt).  The GPU test feeds the device only corrupt streams that went through this program."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import jpeg_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(data, expect_good):
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


def _ref_says_corrupt(data):
    try:
        J.decode_coefficients(data, J.parse(data))
        return False
    except J.Corrupt:
        return True


def test_segment_decoder_under_host_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "jpeg_host_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tools", "jpeg_host_check.cpp"), "-o", exe]
    # the sanitizer runtimes linked into the program itself where the compiler can (gcc's flags; clang does so by default)
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    good = J.matrix()
    bad = J.corrupt_streams()
    assert len(bad) == 6 * 4
    corrupt = [_ref_says_corrupt(d) for _, d in bad]
    assert sum(corrupt) >= 18                     # every truncation; a bit flip may happen to decode
    cases = [_case(d, True) for _, _, d in good] + [_case(d, not c) for (_, d), c in zip(bad, corrupt)]
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<2i", 0x4A504743, len(cases)) + b"".join(cases))
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert f"OK {len(cases)} cases" in lines
    status = [int(l.split()[1]) for l in lines if l and l[0].isdigit()]
    assert len(status) == len(cases)
    assert all(s == 0 for s in status[:len(good)])
    assert all((s != 0) == c for s, c in zip(status[len(good):], corrupt))

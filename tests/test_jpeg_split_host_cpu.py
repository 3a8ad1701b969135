"""csrc/jpeg_split.h -- de-stuffing rule, bit reader, the walk with and without stores, repair rule, write pass: what the lanes of
csrc/jpeg_split.hip run -- compiled for the CPU inside tools/jpeg_split_host_check.cpp, a stand-alone program that emulates the lanes
in loops, with the host compiler's address and undefined-behaviour sanitizers, and run as a subprocess on the fixture matrix, the
corrupt streams, a VOC-like image and the two chunk-boundary streams at subsequence sizes 8, 12, 32, 128 and 256.  The program itself
holds the coefficients to the file's (tests/jpeg_ref.py) and to jpeg_decode_segment's, and the status to jpeg_decode_segment's; here
the round counts are checked too.  The GPU test feeds the device only corrupt streams that went through this program."""
import os
import shutil
import struct
import subprocess

import pytest

import jpeg_ref as J
import jpeg_split_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_boundary_streams_still_straddle():
    for data, at, residue in S.chunk_boundary_streams():
        ent = S.entropy_bytes(data)
        assert ent[at] == 0xFF and ent[at + 1] == 0x00 and at % 1024 == residue
    assert [r for _, _, r in S.chunk_boundary_streams()] == [1023, 1022]


def test_split_decoder_under_host_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "jpeg_split_host_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tools", "jpeg_split_host_check.cpp"), "-o", exe]
    # the sanitizer runtimes linked into the program itself where the compiler can (gcc's flags; clang does so by default)
    r = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    good = [d for _, _, d in J.matrix()] + [S.voc_like()] + [d for d, _, _ in S.chunk_boundary_streams()]
    voc = len(J.matrix())
    bad = J.corrupt_streams()
    corrupt = [S.ref_says_corrupt(d) for _, d in bad]
    assert len(bad) == 6 * 4 and sum(corrupt) >= 18
    cases = [S.case(d, True) for d in good] + [S.case(d, not c) for (_, d), c in zip(bad, corrupt)]
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<2i", 0x4A504743, len(cases)) + b"".join(cases))
    r = subprocess.run([exe, path, ",".join(str(s) for s in S.SUBSEQ_SIZES)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    assert "DESTUFF OK" in lines and f"OK {len(cases)} cases" in lines
    rows = [tuple(int(v) for v in l.split()) for l in lines if l and l[0].isdigit()]
    assert len(rows) == len(cases) * len(S.SUBSEQ_SIZES)
    by = {(ci, sub): (status, n_sub, rounds, walks) for ci, sub, status, n_sub, rounds, walks in rows}
    for ci in range(len(cases)):
        for sub in S.SUBSEQ_SIZES:
            status, n_sub, rounds, walks = by[(ci, sub)]
            assert rounds <= n_sub and walks >= n_sub >= 1, (ci, sub, by[(ci, sub)])
            if ci < len(good):
                assert status == 0, (ci, sub, status)
            else:
                assert (status != 0) == corrupt[ci - len(good)], (ci, sub, status)
    # the VOC-like image synchronises: a handful of rounds for some three hundred subsequences.  Handing an errored exit down as the
    # next entry would take all but two of them.
    status, n_sub, rounds, walks = by[(voc, 128)]
    assert n_sub > 100 and rounds <= n_sub // 4, (n_sub, rounds, walks)
    # the quality-100 noise fixtures have no end-of-block symbols and never synchronise: still correct (above), rounds about n
    names = [n for n, _, _ in J.matrix()]
    q100 = names.index("75x97_q100_420_opt")
    assert by[(q100, 8)][2] > by[(q100, 8)][1] // 2, by[(q100, 8)]

"""csrc/jpeg_split.hip (ops.jpeg_decode_(entropy="split"), RawBatch.to) against Pillow, bit for bit, in the guard-byte arena of
tests/test_jpeg_decode_gpu.py: the fixture matrix as ONE mixed batch at 8, 32 and 128 bytes per subsequence and one image per call;
the chunk-boundary and VOC-like streams with their counters; corrupt streams (only those tools/jpeg_split_host_check.cpp has run under
the host sanitizers, see tests/test_jpeg_split_host_cpu.py) next to a good one, held to the status of the "segment" path; the C entry's
refusals; and a pack_batch of files without restart markers end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

import jpeg_ref as J
import jpeg_split_cases as S

pytestmark = pytest.mark.gpu


def _run(streams, entropy="split", sub=None, want_stats=False):
    """-> (slot pixels per image, status, True if nothing outside the slots changed[, stats])"""
    from objectdetection_ssd_amd import ops
    host, descs, segs, slots = S.layout(streams)
    arena = torch.from_numpy(host.copy()).cuda()
    stats = torch.full((len(streams), 4), -1, dtype=torch.int32, device="cuda") if want_stats else None
    status = ops.jpeg_decode_(arena, descs, segs, entropy=entropy, subsequence_bytes=sub, stats=stats)
    after = arena.cpu().numpy()
    outside = np.ones(host.size, bool)
    out = []
    for so, h, w in slots:
        outside[so:so + h * w * 3] = False
        out.append(after[so:so + h * w * 3].reshape(h, w, 3))
    res = (out, status.cpu().numpy(), bool(np.array_equal(after[outside], host[outside])))
    return res + (stats.cpu().numpy(),) if want_stats else res


@pytest.fixture(scope="module")
def pillow_ref():
    return [J.pillow(d) for _, _, d in J.matrix()]


@pytest.mark.parametrize("sub", [8, 32, 128])
def test_matrix_as_one_mixed_batch(sub, pillow_ref):
    streams = [d for _, _, d in J.matrix()]
    out, status, intact, stats = _run(streams, sub=sub, want_stats=True)
    assert status.dtype == np.int32 and status.shape == (len(streams),) and not status.any(), status
    assert intact, "bytes outside the pixel slots changed"
    for (name, _, _), got, ref in zip(J.matrix(), out, pillow_ref):
        assert np.array_equal(got, ref), (name, int((got != ref).sum()))
    assert (stats[:, 0] >= 1).all() and (stats[:, 1] <= stats[:, 0]).all() and (stats[:, 2] >= stats[:, 0]).all() and not stats[:, 3].any()
    again, status2, _ = _run(streams, sub=sub)
    assert all(np.array_equal(a, b) for a, b in zip(out, again)) and not status2.any()


@pytest.mark.parametrize("size", [(1, 1), (75, 97)])
def test_one_image_per_call(size, pillow_ref):
    n = 0
    for (name, hw, data), ref in zip(J.matrix(), pillow_ref):
        if hw != size:
            continue
        out, status, intact = _run([data], sub=8)
        assert status.tolist() == [0] and intact, name
        assert np.array_equal(out[0], ref), (name, int((out[0] != ref).sum()))
        n += 1
    assert n >= 6


def test_large_streams_and_their_counters():
    from objectdetection_ssd_amd import ops
    cb = S.chunk_boundary_streams()
    for data, at, residue in cb:
        ent = S.entropy_bytes(data)
        assert ent[at] == 0xFF and at % 1024 == residue
    rng = np.random.default_rng(4)
    second = np.clip(S.voc_like_pixels().astype(np.int32) + rng.integers(-20, 21, (375, 500, 3)), 0, 255).astype(np.uint8)
    streams = [cb[0][0], cb[1][0], S.voc_like(), J.encode(second, quality=75, subsampling="4:2:0"), S.voc_like(restart_marker_rows=1)]
    out, status, intact, stats = _run(streams, want_stats=True)                   # the default subsequence size
    assert not status.any() and intact
    for data, got in zip(streams, out):
        assert np.array_equal(got, J.pillow(data))
    assert (stats[2:4, 0] > 100).all(), stats
    assert (stats[:, 1] <= stats[:, 0]).all() and (stats[:, 0] >= 1).all(), stats
    assert stats[4, 0] >= 24 and stats[4, 1] <= stats[4, 0]                       # one segment per MCU row
    assert ops.JPEG_SUBSEQUENCE_BYTES in (64, 128, 256, 512)


@pytest.mark.parametrize("sub", [8, 128])
def test_corrupt_streams_next_to_a_good_one(sub, pillow_ref):
    bad = J.corrupt_streams()
    good_at = len(J.MODES) * 5 + 3                                                # 75x97, quality 100: one long segment
    good_name, _, good = J.matrix()[good_at]
    assert good_name == "75x97_q100_420_opt"
    streams = [d for _, d in bad[:12]] + [good] + [d for _, d in bad[12:]]
    _, want_status, _ = _run(streams, entropy="segment")
    out, status, intact = _run(streams, sub=sub)
    assert intact, "bytes outside the pixel slots changed"
    assert np.array_equal(status, want_status), (status, want_status)
    assert (status != 0).sum() >= 18
    assert status[12] == 0 and np.array_equal(out[12], pillow_ref[good_at])
    for (name, d), got, st in zip(bad, out[:12] + out[13:], np.concatenate([status[:12], status[13:]])):
        if st != 0:
            assert not got.any(), (name, int(st))
        else:
            assert np.array_equal(got, J.decode(d)), name                         # a flip that happens to decode


def test_c_entry_refuses_before_it_launches():
    from objectdetection_ssd_amd import _lib
    lib = _lib.load()
    data = dict((n, d) for n, _, d in J.matrix())["31x33_q75_420_rstblk1"]
    host, descs, segs, slots = S.layout([data, data])
    arena = torch.from_numpy(host.copy()).cuda()
    base = lib.ssd_jpeg_decode_workspace(C.byref(descs), 2)
    nbytes = lib.ssd_jpeg_decode_split_workspace(C.byref(descs), 2, segs.ctypes.data, int(segs.size), 32)
    assert nbytes > base > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    status = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    stats = torch.full((2, 4), 77, dtype=torch.int32, device="cuda")
    d_dev = torch.from_numpy(np.frombuffer(bytes(descs), np.uint8).copy()).cuda()
    s_dev = torch.from_numpy(segs).cuda()

    def call(arena_p=arena.data_ptr(), descs_host=descs, segs_host=segs, status_p=status.data_ptr(), ws_p=ws.data_ptr(), ws_n=nbytes,
             stages=7, d_dev_p=d_dev.data_ptr(), sub=32, stats_p=stats.data_ptr()):
        return lib.ssd_jpeg_decode_split_u8(arena_p, arena.numel(), d_dev_p, C.byref(descs_host), s_dev.data_ptr(), segs_host.ctypes.data,
                                            int(segs_host.size), 2, status_p, ws_p, ws_n, stages,
                                            torch.cuda.current_stream().cuda_stream, sub, stats_p)

    def mutated(fn):
        m = (_lib.JpegDesc * 2)()
        C.memmove(m, descs, C.sizeof(m))
        fn(m[1])
        return m

    assert call(arena_p=None) == -3 and call(status_p=None) == -3 and call(ws_p=None) == -3 and call(d_dev_p=None) == -3
    for sub in (0, 4, 6, 30, 4100, -32):
        assert call(sub=sub) == -1, sub
    assert call(ws_n=base) == -2 and call(ws_n=nbytes - 512) == -2                 # the segment path's size is too small
    far = segs.copy()
    far[-1] = descs[1].stream_bytes + 1
    assert call(segs_host=far) == -1                                              # the validations of the segment entry
    assert call(descs_host=mutated(lambda d: setattr(d, "dst_bytes", 31 * 33 * 3 - 1))) == -1
    assert call(descs_host=mutated(lambda d: d.bits[0].__setitem__(0, 3))) == -1
    assert call(descs_host=mutated(lambda d: setattr(d, "coef_offset", d.coef_offset + 256))) == -1
    assert call(stages=0) == -1 and call(stages=8) == -1
    torch.cuda.synchronize()
    assert np.array_equal(arena.cpu().numpy(), host) and status.tolist() == [77, 77] and (stats == 77).all()      # nothing was enqueued
    assert call() == 0
    assert status.tolist() == [0, 0] and stats[:, 3].tolist() == [0, 0] and (stats[:, 0] >= descs[0].n_segments).all()
    assert call(stats_p=None) == 0 and status.tolist() == [0, 0]
    ref = J.pillow(data)
    after = arena.cpu().numpy()
    for so, h, w in slots:
        assert np.array_equal(after[so:so + h * w * 3].reshape(h, w, 3), ref)


def test_pack_batch_of_files_without_restart_markers_end_to_end():
    """VOC-like files as they are on disk (no restart markers: "auto" says "split"), one with restart markers and a progressive one
    (which PIL decodes on the host) in one batch: RawBatch.to() equals the same batch packed from host-decoded pixels."""
    import io
    from PIL import Image
    from objectdetection_ssd_amd import Dataset, ops
    rng = np.random.default_rng(5)
    px = S.voc_like_pixels()
    other = np.clip(px.astype(np.int32) + rng.integers(-25, 26, px.shape), 0, 255).astype(np.uint8)
    prog = io.BytesIO()
    Image.fromarray(px[:96, :128]).save(prog, "JPEG", quality=80, progressive=True)
    blobs = [S.voc_like(), J.encode(other, quality=75, subsampling="4:2:0"), S.voc_like(restart_marker_rows=1), prog.getvalue()]
    assert Dataset.parse_jpeg(blobs[3]) is None and all(Dataset.parse_jpeg(b) is not None for b in blobs[:3])
    _, descs, segs, _ = S.layout(blobs[:3])
    assert ops.jpeg_entropy_auto(descs, segs) == "split"
    pixels = [J.pillow(b) for b in blobs]
    plans = []
    for i, p in enumerate(pixels):
        h, w = p.shape[:2]
        plans.append(Dataset.GeomPlan(h, w, (h + 7 + i, w + 5, 3, 2 + i), (1 + i, 2, h, w - 3), i % 2 == 1, (((0, 1.1),), (), ((1, 0.8),), ())[i]))
    rb = Dataset.pack_batch(blobs, plans)
    assert [h is not None for h in rb.headers] == [True, True, True, False]
    want = Dataset.pack_batch(pixels, plans).to("cuda")                            # what decode="host" hands over: pixels
    got = rb.to("cuda")
    assert got.shape == (4, 3, 300, 300) and rb.decode_status.tolist() == [0] * 4
    assert torch.equal(got, want)

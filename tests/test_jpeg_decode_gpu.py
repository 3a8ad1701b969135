"""csrc/jpeg.hip (ops.jpeg_decode_, RawBatch.to) against Pillow, bit for bit, on the fixture matrix of tests/jpeg_ref.py: every
size x (quality, sampling, optimised tables, restart interval) as ONE mixed batch and one image per call; guard bytes around every
pixel slot; corrupt streams (only those tools/jpeg_host_check.cpp has run under the host sanitizers, see
tests/test_jpeg_entropy_host_cpu.py) next to a good one; the C entry's refusals; and a mixed pack_batch end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

import jpeg_ref as J

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN = 0xA5


def _layout(streams):
    """An arena with GUARD bytes of PATTERN on either side of every pixel slot (slots at odd, unaligned offsets), the entropy-coded
    data behind them.  -> (host arena, descs, segs, [(slot offset, h, w)])"""
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


def _run(streams):
    """-> (slot pixels per image, status, True if nothing outside the slots changed)"""
    from objectdetection_ssd_amd import ops
    host, descs, segs, slots = _layout(streams)
    arena = torch.from_numpy(host.copy()).cuda()
    status = ops.jpeg_decode_(arena, descs, segs)
    after = arena.cpu().numpy()
    outside = np.ones(host.size, bool)
    out = []
    for so, h, w in slots:
        outside[so:so + h * w * 3] = False
        out.append(after[so:so + h * w * 3].reshape(h, w, 3))
    return out, status.cpu().numpy(), bool(np.array_equal(after[outside], host[outside]))


@pytest.fixture(scope="module")
def pillow_ref():
    return [J.pillow(d) for _, _, d in J.matrix()]


def test_matrix_as_one_mixed_batch(pillow_ref):
    streams = [d for _, _, d in J.matrix()]
    out, status, intact = _run(streams)
    assert status.dtype == np.int32 and status.shape == (len(streams),) and not status.any(), status
    assert intact, "bytes outside the pixel slots changed"
    for (name, _, _), got, ref in zip(J.matrix(), out, pillow_ref):
        assert np.array_equal(got, ref), (name, int((got != ref).sum()))
    again, status2, _ = _run(streams)
    assert all(np.array_equal(a, b) for a, b in zip(out, again)) and not status2.any()


@pytest.mark.parametrize("size", [(1, 1), (75, 97)])
def test_one_image_per_call(size, pillow_ref):
    n = 0
    for (name, hw, data), ref in zip(J.matrix(), pillow_ref):
        if hw != size:
            continue
        out, status, intact = _run([data])
        assert status.tolist() == [0] and intact, name
        assert np.array_equal(out[0], ref), (name, int((out[0] != ref).sum()))
        n += 1
    assert n >= 6


def test_corrupt_streams_next_to_a_good_one(pillow_ref):
    bad = J.corrupt_streams()
    good_name, _, good = J.matrix()[len(J.MODES) * 5 + 4]                          # 75x97, restart interval 1: 35 segments
    assert good_name == "75x97_q75_420_rstblk1"
    want = []
    for _, d in bad:
        try:
            hdr = J.parse(d)
            J.decode_coefficients(d, hdr)
            want.append(J.decode(d))              # a flip that happens to decode: the pixels of the flipped stream
        except J.Corrupt:
            want.append(None)
    assert sum(w is None for w in want) >= 18
    out, status, intact = _run([d for _, d in bad[:12]] + [good] + [d for _, d in bad[12:]])
    assert intact, "bytes outside the pixel slots changed"
    assert status[12] == 0 and np.array_equal(out[12], pillow_ref[len(J.MODES) * 5 + 4])
    for (name, _), w, got, st in zip(bad, want, out[:12] + out[13:], np.concatenate([status[:12], status[13:]])):
        if w is None:
            assert st != 0 and not got.any(), (name, int(st))
        else:
            assert st == 0 and np.array_equal(got, w), (name, int(st))


def test_c_entry_refuses_before_it_launches():
    from objectdetection_ssd_amd import _lib, ops
    lib = _lib.load()
    data = dict((n, d) for n, _, d in J.matrix())["31x33_q75_420_rstblk1"]
    host, descs, segs, slots = _layout([data, data])
    arena = torch.from_numpy(host.copy()).cuda()
    nbytes = lib.ssd_jpeg_decode_workspace(C.byref(descs), 2)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    status = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    d_dev = torch.from_numpy(np.frombuffer(bytes(descs), np.uint8).copy()).cuda()
    s_dev = torch.from_numpy(segs).cuda()

    def call(arena_p=arena.data_ptr(), descs_host=descs, segs_host=segs, status_p=status.data_ptr(), ws_p=ws.data_ptr(), ws_n=nbytes,
             stages=7, d_dev_p=d_dev.data_ptr()):
        return lib.ssd_jpeg_decode_u8(arena_p, arena.numel(), d_dev_p, C.byref(descs_host), s_dev.data_ptr(), segs_host.ctypes.data,
                                      int(segs_host.size), 2, status_p, ws_p, ws_n, stages, torch.cuda.current_stream().cuda_stream)

    def mutated(fn):
        m = (_lib.JpegDesc * 2)()
        C.memmove(m, descs, C.sizeof(m))
        fn(m[1])
        return m

    assert call(arena_p=None) == -3 and call(status_p=None) == -3 and call(ws_p=None) == -3 and call(d_dev_p=None) == -3
    far = segs.copy()
    far[-1] = descs[1].stream_bytes + 1
    assert call(segs_host=far) == -1                                              # a segment offset outside the stream
    back = segs.copy()
    back[3] = back[2] + 1
    assert call(segs_host=back) == -1                                             # segments out of order
    assert call(descs_host=mutated(lambda d: d.n_huffval.__setitem__(2, 257))) == -1          # a table longer than 256 values
    assert call(descs_host=mutated(lambda d: d.bits[0].__setitem__(0, 3))) == -1              # no canonical code
    assert call(descs_host=mutated(lambda d: setattr(d, "dst_bytes", 31 * 33 * 3 - 1))) == -1     # a slot smaller than h * w * 3
    assert call(descs_host=mutated(lambda d: setattr(d, "dst_offset", descs[0].dst_offset + 8))) == -1      # slots overlap
    assert call(descs_host=mutated(lambda d: setattr(d, "stream_offset", arena.numel() - 4))) == -1
    assert call(descs_host=mutated(lambda d: setattr(d, "width", 4097))) == -1
    assert call(descs_host=mutated(lambda d: setattr(d, "v_samp", 3))) == -1
    assert call(descs_host=mutated(lambda d: setattr(d, "n_segments", d.n_segments + 1))) == -1
    assert call(descs_host=mutated(lambda d: d.dc_sel.__setitem__(1, 2))) == -1
    assert call(descs_host=mutated(lambda d: setattr(d, "coef_offset", d.coef_offset + 256))) == -1
    assert call(ws_n=nbytes - 512) == -2
    assert call(stages=0) == -1 and call(stages=8) == -1
    torch.cuda.synchronize()
    assert np.array_equal(arena.cpu().numpy(), host) and status.tolist() == [77, 77]          # nothing was enqueued
    assert call() == 0
    assert status.tolist() == [0, 0]
    with pytest.raises(ValueError):
        ops.jpeg_decode_(arena, mutated(lambda d: setattr(d, "h_samp", 4)), segs)
    with pytest.raises(RuntimeError):
        ops.jpeg_decode_(arena.cpu(), descs, segs)


def test_mixed_pack_batch_end_to_end():
    """four encoded images and one host-decoded RawImage, each with an expand / crop / flip and a photometric plan: RawBatch.to()
    equals the same batch packed from Pillow-decoded pixels."""
    from objectdetection_ssd_amd import Dataset
    m = dict((n, d) for n, _, d in J.matrix())
    names = ["75x97_q30_420", "48x64_q75_422", "75x97_q90_420_rstrow1", "31x33_gray", "48x64_q95_444"]
    blobs = [m[n] for n in names]
    pixels = [J.pillow(b) for b in blobs]
    plans = []
    for i, px in enumerate(pixels):
        h, w = px.shape[:2]
        canvas = (2 * h + i, 2 * w + 3, 5 + i, 7)
        crop = (3 + i, 4, h + 10, w + 9 - i)
        photo = (((0, 1.2), (3, 0.05)), ((1, 0.7),), ((2, 1.4), (1, 1.1), (0, 0.8)), ((3, -0.04), (2, 0.6)), ())[i]
        plans.append(Dataset.GeomPlan(h, w, canvas, crop, i % 2 == 0, photo))
    mixed = [Dataset.EncodedImage(b, Dataset.parse_jpeg(b), p) for b, p in zip(blobs[:4], plans[:4])] + [pixels[4]]
    rb = Dataset.pack_batch(mixed, plans)
    assert [h is not None for h in rb.headers] == [True] * 4 + [False]
    want = Dataset.pack_batch(pixels, plans).to("cuda")
    got = rb.to("cuda")
    assert got.shape == (5, 3, 300, 300) and got.dtype == torch.float32
    assert rb.decode_status.dtype == torch.int32 and rb.decode_status.tolist() == [0] * 5
    assert torch.equal(got, want)
    # bytes entries through preprocess_batch, all encoded: the status comes straight from the decoder
    rb2 = Dataset.pack_batch(blobs[:4], plans[:4])
    assert torch.equal(rb2.pin_memory().to("cuda"), want[:4])
    assert torch.equal(Dataset.preprocess_batch(blobs, plans), want)

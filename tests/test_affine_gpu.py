"""Random affine augmentation on the device: `ssd_affine_warp_f32` (csrc/warp.hip) through `ops.affine_warp` and `RawBatch.to`, bit for
bit against the numpy float32 restatement of tests/affine_ref.py."""
import dataclasses

import numpy as np
import pytest
import torch

import affine_ref as R

pytestmark = pytest.mark.gpu


def _matrices(H, W, seed):
    """identity; integer shift (-3, +2); a quarter turn where the frame is square, else a drawn matrix; translation by 1e6; a 1e30
    coefficient; coefficients that make the coordinate +-inf and NaN; two draws in the default ranges"""
    drawn = R.drawn_mats(3, W, H, seed)
    turn = (0, 1, 0, -1, 0, W) if H == W else drawn[2]
    return np.asarray([R.IDENTITY, (1, 0, -3, 0, 1, 2), turn, (1, 0, 1e6, 0, 1, 0), (1e30, 0, 0, 0, 1, 0), (3e38, -3e38, 3e38, 0, 1, 0),
                       drawn[0], drawn[1]], np.float32)


def _warp(x, mats):
    from objectdetection_ssd_amd import ops
    out = ops.affine_warp(torch.from_numpy(x).cuda(), mats, R.fill())
    assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous()
    return out.cpu()


@pytest.mark.parametrize("shape", [(6, 13, 17), (6, 64, 48), (2, 300, 300)], ids=lambda s: "x".join(map(str, s)))
def test_warp_equals_the_restatement(shape):
    """every matrix kind at every shape: the eight matrices go through in calls of B images (the last call filled up with draws)"""
    B, H, W = shape
    mats = _matrices(H, W, 7)
    mats = np.concatenate([mats, R.drawn_mats(-len(mats) % B, W, H, 8).reshape(-1, 6)])
    x = R.noise(len(mats), H, W, 11)
    want = R.warp(x, mats)
    fl = R.fill().reshape(3, 1, 1)
    assert np.array_equal(want[0], x[0]) and all(np.array_equal(want[k], np.broadcast_to(fl, (3, H, W))) for k in (3, 4, 5))
    assert not np.array_equal(want[6], x[6]) and np.isfinite(want).all()
    for at in range(0, len(mats), B):
        got = _warp(x[at:at + B], mats[at:at + B])
        assert got.shape == (B, 3, H, W)
        for k in range(B):
            assert torch.equal(got[k], torch.from_numpy(want[at + k])), (at + k, mats[at + k])
    # a CPU tensor of matrices is taken like an array
    got = _warp(x[:B], torch.from_numpy(mats[:B].copy()))
    assert torch.equal(got, torch.from_numpy(want[:B]))


@pytest.mark.parametrize("hw", [(1, 1), (1, 7)], ids=["1x1", "1x7"])
def test_smallest_frames(hw):
    """every tap but one (or one row of them) is outside the image: the four-tap border logic alone"""
    H, W = hw
    mats = np.asarray([R.IDENTITY, (1, 0, 0.5, 0, 1, 0), (1, 0, 0, 0, 1, -0.25), (1, 0, -0.75, 0, 1, 0.75), (1, 0, -1, 0, 1, 0), (1, 0, 1, 0, 1, 1),
                       (0.5, 0.25, 0.1, -0.25, 0.5, 0.2), (1, 0, -7, 0, 1, 0)], np.float32)
    x = R.noise(len(mats), H, W, 3)
    want = R.warp(x, mats)
    assert np.array_equal(want[0], x[0])
    assert torch.equal(_warp(x, mats), torch.from_numpy(want))


def test_ops_front_end_refuses_what_the_kernel_assumes_away():
    from objectdetection_ssd_amd import ops
    x = torch.zeros((2, 3, 8, 8), device="cuda")
    ident = np.tile(np.asarray(R.IDENTITY, np.float32), (2, 1))
    for bad in (ident[:1], ident.astype(np.float64), ident.reshape(-1), np.full((2, 6), np.nan, np.float32)):
        with pytest.raises(ValueError):
            ops.affine_warp(x, bad, R.fill())
    with pytest.raises(ValueError):
        ops.affine_warp(x, torch.from_numpy(ident).cuda(), R.fill())
    with pytest.raises(ValueError):
        ops.affine_warp(x[:, :, :, ::2], ident, R.fill())
    with pytest.raises(ValueError):
        ops.affine_warp(torch.zeros((2, 4, 8, 8), device="cuda"), ident, R.fill())
    with pytest.raises(ValueError):
        ops.affine_warp(x.half(), ident, R.fill())
    with pytest.raises(ValueError):
        ops.affine_warp(x, ident, (0.0, 0.0))


def test_through_rawbatch_plain_warped_plain_warped_mosaic_and_warped_stream():
    """a plain image, a warped plain image, a warped mosaic and a warped baseline JPEG decoded on the device in one batch: the restatement
    applied to the `.to()` output of the same batch with the matrices removed; the un-warped entry is that output's, bit for bit"""
    import jpeg_ref as J
    from objectdetection_ssd_amd import Dataset
    rng = np.random.default_rng(17)
    a = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((75, 97), (120, 90), (64, 200), (37, 53), (90, 61), (48, 64))]
    P = Dataset.GeomPlan
    mats = R.drawn_mats(3, 300, 300, 23)
    warp = [tuple(float(v) for v in m) + (300.0, 300.0) for m in mats]
    mosaic = Dataset.MosaicImage((Dataset.RawImage(a[2], Dataset.identity_plan(64, 200)), Dataset.RawImage(a[3], P(37, 53, (60, 80, 9, 13), (2, 3, 55, 70), True)),
                                  Dataset.RawImage(a[4], Dataset.identity_plan(90, 61)), Dataset.RawImage(a[5], Dataset.identity_plan(48, 64))),
                                 ((0, 0, 120, 170), (0, 170, 120, 130), (120, 0, 180, 170), (120, 170, 180, 130)), (300, 300), warp[1])
    blob = dict((n, d) for n, _, d in J.matrix())["75x97_q30_420"]
    stream = Dataset.EncodedImage(blob, Dataset.parse_jpeg(blob), P(75, 97, (75, 97, 0, 0), (2, 3, 70, 93), True, ((1, 0.8),)), warp[2])
    plans = [P(75, 97, (150, 200, 20, 30), (10, 12, 120, 160), True), P(120, 90, (120, 90, 0, 0), (3, 4, 100, 70), False, ((0, 1.2),)), None, stream.plan]
    entries = [a[0], a[1], mosaic, stream]
    rb = Dataset.pack_batch(entries, plans, warps=[None, warp[0], warp[1], warp[2]])
    assert rb.warps == [None] + [w[:6] for w in warp] and rb.headers is not None and len(rb.tiles) == 7
    got = rb.to("cuda")
    bare = Dataset.pack_batch([a[0], a[1], dataclasses.replace(mosaic, warp=None), dataclasses.replace(stream, warp=None)], plans)
    assert bare.warps is None
    base = bare.to("cuda")
    assert rb.decode_status.tolist() == bare.decode_status.tolist() and not any(rb.decode_status.tolist())
    assert got.shape == base.shape == (4, 3, 300, 300) and got.dtype == torch.float32
    assert torch.equal(got[0], base[0])
    want = R.warp(base.cpu().numpy(), np.asarray([R.IDENTITY] + [w[:6] for w in warp], np.float32))
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert not torch.equal(got[1], base[1])
    # all warped, no tile list, pinned first: the plain resize entry, then the warp
    rb = Dataset.pack_batch(a[:2], plans[:2], warps=[warp[2], warp[0]]).pin_memory()
    assert rb.tiles is None and rb.arena.is_pinned()
    base = Dataset.pack_batch(a[:2], plans[:2]).to("cuda")
    want = R.warp(base.cpu().numpy(), np.asarray([warp[2][:6], warp[0][:6]], np.float32))
    assert torch.equal(rb.to("cuda").cpu(), torch.from_numpy(want))


def test_end_to_end_with_workers(tmp_path):
    from PIL import Image
    from objectdetection_ssd_amd import Dataset
    dev = torch.device("cuda")
    torch.zeros(1, device=dev)
    rng = np.random.default_rng(2)
    paths, n = [], 8
    for i in range(n):
        h, w = int(rng.integers(40, 160)), int(rng.integers(40, 160))
        pth = str(tmp_path / f"e{i}.png")
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(pth)
        paths.append(pth)
    bboxes = [[[2., 3., 30., 35.], [10., 8., 38., 39.]] for _ in range(n)]
    ds = Dataset.MultiImageMultiBBoxDataset(paths, bboxes, [["dog", "person"]] * n, [[0, 0]] * n, list(range(n)), mosaic=0.5, affine=0.75)
    dl = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=True, num_workers=2, collate_fn=Dataset.collate_fn)
    seen, warped = [], 0
    for inputs, classes, boxes, indices in dl:
        assert isinstance(inputs, Dataset.RawBatch) and inputs.shape == (4, 3, 300, 300)
        warped += 0 if inputs.warps is None else sum(w is not None for w in inputs.warps)
        x = inputs.to(dev)
        assert x.is_cuda and tuple(x.shape) == (4, 3, 300, 300) and bool(torch.isfinite(x).all())
        assert all(b.shape[0] >= 1 and b.shape[1] == 4 and b.shape[0] == c.shape[0] for b, c in zip(boxes, classes))
        for b, w in zip(boxes, inputs.warps or [None] * 4):                          # a warped sample's boxes are clipped to the frame
            assert w is None or (float(b.min()) >= 0.0 and float(b.max()) <= 1.0)
        seen += indices
    assert sorted(seen) == list(range(n)) and warped >= 1

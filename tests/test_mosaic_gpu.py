"""Mosaic augmentation on the device: `ssd_preprocess_tiles_u8` (csrc/preprocess.hip) through `ops.preprocess_tiles_u8` and
`RawBatch.to`, bit for bit against `ssd_preprocess_u8` (one full-frame tile per image) and against the pixel restatement of
tests/mosaic_ref.py (each tile the oracle's `preprocess_image` at the tile's size, pasted at its rectangle)."""
import random

import numpy as np
import pytest
import torch

import mosaic_ref as R
import ssd_oracle as O

pytestmark = pytest.mark.gpu


def _descs(rb):
    from objectdetection_ssd_amd import _lib
    descs = (_lib.ImageDesc * len(rb.plans))()
    for d, p, o in zip(descs, rb.plans, rb.offsets):
        d.src_offset, d.src_h, d.src_w = o, p.src_h, p.src_w
        d.canvas_h, d.canvas_w, d.place_top, d.place_left = p.canvas
        d.crop_top, d.crop_left, d.crop_h, d.crop_w = p.crop
        d.flip = int(p.flip)
    return descs


def _mosaic(sources, plans, rects, out_hw=(300, 300)):
    from objectdetection_ssd_amd import Dataset
    return Dataset.MosaicImage(tuple(Dataset.RawImage(a, p) for a, p in zip(sources, plans)), tuple(rects), out_hw)


def _reference(m, photometric=False):
    srcs = [O.photometric_apply(s.pixels, s.plan.photo) if photometric else s.pixels for s in m.sources]
    return R.compose(srcs, [(s.plan.canvas, s.plan.crop, s.plan.flip) for s in m.sources], m.rects, m.out_hw)


def _sources(rng, shapes):
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]


def test_one_full_frame_tile_per_image_equals_the_resize_entry():
    from objectdetection_ssd_amd import Dataset, _lib, ops
    rng = np.random.default_rng(21)
    shapes = [(375, 500), (500, 333), (120, 90), (300, 300), (300, 451), (900, 1300), (37, 53), (301, 299), (500, 500)]
    rb = Dataset.pack_batch(_sources(rng, shapes))
    arena = rb.arena.cuda()
    descs = _descs(rb)
    for oh, ow in ((300, 300), (64, 48)):
        want = ops.preprocess_u8(arena, descs, (oh, ow), Dataset.MEAN, Dataset.STD, Dataset.FILLER_U8)
        tiles = (_lib.TileDesc * len(shapes))()
        for i, t in enumerate(tiles):
            t.src = descs[i]
            t.out_image, t.dst_top, t.dst_left, t.dst_h, t.dst_w = i, 0, 0, oh, ow
        got = ops.preprocess_tiles_u8(arena, tiles, len(shapes), (oh, ow), Dataset.MEAN, Dataset.STD, Dataset.FILLER_U8)
        assert got.shape == want.shape and got.dtype == torch.float32 and torch.equal(got, want), (oh, ow)


def test_mosaics_equal_the_restatement():
    """Three mosaics in one batch: a centred one of a down-scaled, an up-scaled (source smaller than its tile), a cropped + mirrored and
    an expanded (canvas in the descriptor) + cropped source; cx = 1, cy = H-1 (tiles one pixel wide, high, and both); and one whose
    top-left tile takes 31 source pixels per output pixel on both axes, the tap bound exactly."""
    from objectdetection_ssd_amd import Dataset
    P = Dataset.GeomPlan
    rng = np.random.default_rng(5)
    a = _sources(rng, [(375, 500), (37, 53), (120, 90), (64, 200)])
    centred = _mosaic(a, [Dataset.identity_plan(375, 500), Dataset.identity_plan(37, 53), P(120, 90, (120, 90, 0, 0), (11, 7, 80, 61), True),
                          P(64, 200, (150, 420, 40, 100), (20, 60, 121, 333), True)], R.rectangles(150, 150, 300, 300))
    b = _sources(rng, [(200, 31), (100, 140), (25, 30), (31, 333)])
    thin = _mosaic(b, [Dataset.identity_plan(200, 31), P(100, 140, (100, 140, 0, 0), (0, 0, 100, 140), True),
                       P(25, 30, (40, 50, 10, 15), (5, 9, 31, 31), False), Dataset.identity_plan(31, 333)], R.rectangles(1, 299, 300, 300))
    c = _sources(rng, [(310, 620), (90, 61), (300, 300), (500, 375)])
    bound = _mosaic(c, [Dataset.identity_plan(310, 620), Dataset.identity_plan(90, 61), P(300, 300, (300, 300, 0, 0), (1, 2, 290, 280), True),
                        Dataset.identity_plan(500, 375)], R.rectangles(20, 10, 300, 300))
    rb = Dataset.pack_batch([centred, thin, bound])
    assert rb.shape == (3, 3, 300, 300) and len(rb.tiles) == 12
    out = rb.to("cuda")
    assert out.shape == (3, 3, 300, 300) and out.dtype == torch.float32
    for i, m in enumerate((centred, thin, bound)):
        assert np.array_equal(out[i].cpu().numpy(), _reference(m)), i


def test_mixed_batch_and_a_non_square_output():
    """a plain image (with a drawn geometry) between two mosaics, at 300 x 300 and into a 40 x 72 frame, pinned first"""
    from objectdetection_ssd_amd import Dataset
    P = Dataset.GeomPlan
    rng = np.random.default_rng(8)
    a = _sources(rng, [(120, 90), (64, 200), (37, 53), (90, 61), (75, 97)])
    plans = [P(120, 90, (120, 90, 0, 0), (3, 4, 100, 70), False), Dataset.identity_plan(64, 200), P(37, 53, (60, 80, 9, 13), (2, 3, 55, 70), True),
             Dataset.identity_plan(90, 61)]
    plain_plan = P(75, 97, (150, 200, 20, 30), (10, 12, 120, 160), True)
    for (H, W), (cx, cy) in (((300, 300), (101, 222)), ((40, 72), (50, 7))):
        m1 = _mosaic(a[:4], plans, R.rectangles(cx, cy, H, W), (H, W))
        m2 = _mosaic(a[:4][::-1], plans[::-1], R.rectangles(W - cx, H - cy, H, W), (H, W))
        rb = Dataset.pack_batch([m1, a[4], m2], [None, plain_plan, None], size=(H, W)).pin_memory()
        assert rb.arena.is_pinned() and rb.tiles[4] == (4, 1, 0, 0, H, W) and rb.n_images == 3
        out = rb.to("cuda").cpu().numpy()
        assert out.shape == (3, 3, H, W)
        assert np.array_equal(out[0], _reference(m1)) and np.array_equal(out[2], _reference(m2))
        assert np.array_equal(out[1], O.preprocess_image(a[4], H, W, canvas=plain_plan.canvas, crop=plain_plan.crop, flip=True))
        assert torch.equal(Dataset.preprocess_batch([a[4]], [plain_plan], size=(H, W))[0].cpu(), torch.from_numpy(out[1]))


def test_photometric_plans_on_the_sources_then_the_mosaic():
    from objectdetection_ssd_amd import Dataset
    rng = np.random.default_rng(13)
    a = _sources(rng, [(64, 48), (31, 33), (75, 97), (48, 64)])
    photo = (((0, 1.2), (3, 0.05)), ((1, 0.7),), ((2, 1.4), (1, 1.1), (0, 0.8), (3, -0.04)), ())
    plans = [Dataset.GeomPlan(x.shape[0], x.shape[1], (x.shape[0] + 9, x.shape[1] + 5, 4, 2), (1, 1, x.shape[0] + 3, x.shape[1] + 2), i % 2 == 1, ph)
             for i, (x, ph) in enumerate(zip(a, photo))]
    m = _mosaic(a, plans, R.rectangles(70, 50, 96, 128), (96, 128))
    out = Dataset.pack_batch([m], size=(96, 128)).to("cuda")
    assert np.array_equal(out[0].cpu().numpy(), _reference(m, photometric=True))


def test_sources_decoded_on_the_device_equal_host_decoded_ones():
    import jpeg_ref as J
    from objectdetection_ssd_amd import Dataset
    blobs = dict((n, d) for n, _, d in J.matrix())
    names = ["75x97_q30_420", "48x64_q75_422", "31x33_gray", "48x64_q95_444"]
    px = [J.pillow(blobs[n]) for n in names]
    plans = [Dataset.GeomPlan(p.shape[0], p.shape[1], (p.shape[0], p.shape[1], 0, 0), (2, 3, p.shape[0] - 5, p.shape[1] - 4), i % 2 == 0,
                              ((1, 0.8),) if i == 1 else ()) for i, p in enumerate(px)]
    rects = R.rectangles(120, 170, 300, 300)
    enc = Dataset.MosaicImage(tuple(Dataset.EncodedImage(blobs[n], Dataset.parse_jpeg(blobs[n]), p) for n, p in zip(names, plans)), rects, (300, 300))
    host = _mosaic(px, plans, rects)
    rb = Dataset.pack_batch([enc, enc])
    assert all(h is not None for h in rb.headers) and len(rb.tiles) == 8
    got = rb.to("cuda")
    assert rb.decode_status.tolist() == [0] * 8
    want = Dataset.pack_batch([host]).to("cuda")
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[0])
    assert np.array_equal(want[0].cpu().numpy(), _reference(host, photometric=True))


def test_end_to_end_with_workers_model_and_loss(tmp_path):
    from PIL import Image
    from objectdetection_ssd_amd import Dataset, Losses, Model
    dev = torch.device("cuda")
    torch.zeros(1, device=dev)
    rng = np.random.default_rng(2)
    paths, n = [], 12
    for i in range(n):
        h, w = int(rng.integers(40, 160)), int(rng.integers(40, 160))
        pth = str(tmp_path / f"e{i}.png")
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(pth)
        paths.append(pth)
    bboxes = [[[2., 3., 30., 35.], [10., 8., 38., 39.]] for _ in range(n)]
    labels = [["dog", "person"] for _ in range(n)]
    ds = Dataset.MultiImageMultiBBoxDataset(paths, bboxes, labels, [[0, 0]] * n, list(range(n)), mosaic=1.0)
    dl = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=True, num_workers=2, collate_fn=Dataset.collate_fn)
    torch.manual_seed(0)
    net = Model.SSD_300().to(dev).eval()
    seen = []
    for inputs, classes, boxes, indices in dl:
        assert isinstance(inputs, Dataset.RawBatch) and len(inputs.tiles) == 16 and inputs.shape == (4, 3, 300, 300)
        x = inputs.to(dev)
        assert x.is_cuda and tuple(x.shape) == (4, 3, 300, 300) and bool(torch.isfinite(x).all())
        assert all(b.shape[0] >= 1 and b.shape[1] == 4 and b.shape[0] == c.shape[0] for b, c in zip(boxes, classes))
        with torch.no_grad():
            loc, conf = net(x)
        assert tuple(loc.shape) == (4, 8732, 4) and tuple(conf.shape) == (4, 8732, 21)
        l1, l2 = Losses.ssd((loc, conf), [c.to(dev) for c in classes], [b.to(dev) for b in boxes])
        assert bool(torch.isfinite(l1)) and bool(torch.isfinite(l2))
        seen += indices
    assert sorted(seen) == list(range(n))

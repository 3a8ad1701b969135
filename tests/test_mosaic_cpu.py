"""Mosaic augmentation, host half (no GPU): the restatement of tests/mosaic_ref.py against PIL done literally; the draws, boxes, labels
and ignore boxes of `Dataset.MultiImageMultiBBoxDataset(mosaic=...)` against the restatement; `mosaic=0.0` and `plan_transform`'s
default against today's draw sequence; the tile list through `collate_fn`, pickle and `pin_memory()`; and every refusal of
`ssd_preprocess_tiles_u8`, which is made before anything is enqueued."""
import ctypes as C
import os
import pickle
import random

import numpy as np
import pytest
import torch

import mosaic_ref as R
import ssd_oracle as O

SIZES = [(37, 53), (120, 90), (375, 500), (64, 200), (300, 300), (90, 61)]          # (h, w)
LABELS = ["dog", "cat", "person", "car", "bus", "bird"]


def _boxes(h, w, rng, n):
    """n boxes of an h x w image; the first touches the right and bottom edges (a mirrored plan carries it to x = -1: the clamp), the
    last is one pixel small (the minimum-size filter)"""
    out = [[w * 0.4, h * 0.3, float(w), float(h)]]
    for _ in range(n - 2):
        x0, y0 = rng.uniform(0, w * 0.6), rng.uniform(0, h * 0.6)
        out.append([x0, y0, x0 + rng.uniform(w * 0.2, w * 0.4), y0 + rng.uniform(h * 0.2, h * 0.4)])
    out.append([w * 0.5, h * 0.5, w * 0.5 + 1.0, h * 0.5 + 1.0])
    return np.asarray(out, np.float32).tolist()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from PIL import Image
    from objectdetection_ssd_amd.Util import label_to_class
    d = tmp_path_factory.mktemp("mosaic")
    rng = np.random.default_rng(12)
    paths, boxes, labels, difficult, pixels = [], [], [], [], []
    for i, (h, w) in enumerate(SIZES):
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        p = str(d / f"m{i}.png")
        Image.fromarray(a).save(p)
        paths.append(p); pixels.append(a)
        boxes.append(_boxes(h, w, rng, 4))
        labels.append([LABELS[(i + k) % len(LABELS)] for k in range(4)])
        difficult.append([0, 1 if i % 2 else 0, 0, 0])
    classes = [[float(label_to_class[n]) for n in ls] for ls in labels]
    return {"paths": paths, "boxes": boxes, "labels": labels, "difficult": difficult, "pixels": pixels, "classes": classes}


def _dataset(f, **kw):
    from objectdetection_ssd_amd import Dataset
    return Dataset.MultiImageMultiBBoxDataset(f["paths"], f["boxes"], f["labels"], f["difficult"], list(range(100, 100 + len(SIZES))), **kw)


def _kept(f, keep_difficult):
    """boxes, class numbers and ignore boxes per image as the dataset hands them to the plan"""
    b, c, ig = [], [], []
    for bx, cl, df in zip(f["boxes"], f["classes"], f["difficult"]):
        bx, cl, df = np.asarray(bx, np.float32), np.asarray(cl, np.float32), np.asarray(df) != 0
        easy = ~df if keep_difficult is not True else np.ones_like(df)
        b.append(bx[easy]); c.append(cl[easy]); ig.append(bx[~easy])
    return b, c, ig


def _plan_tuple(p):
    return (tuple(p.photo), tuple(p.canvas), tuple(p.crop), bool(p.flip))


# ---- the restatement itself ----------------------------------------------------------------------------------------------------
def test_restatement_with_identity_plans_is_pil_done_literally():
    """Image.new, then per tile crop().resize((w, h), BILINEAR) and paste: equal to the 8-bit tiles of the restatement, and the float
    restatement is their ToTensor + Normalize."""
    from PIL import Image
    rng = np.random.default_rng(3)
    srcs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in ((375, 500), (37, 53), (120, 90), (64, 200))]
    for (H, W), (cx, cy) in (((300, 300), (150, 150)), ((300, 300), (76, 201)), ((64, 48), (5, 60)), ((40, 72), (71, 1))):
        rects = R.rectangles(cx, cy, H, W)
        frame = Image.new("RGB", (W, H))
        for a, (top, left, h, w) in zip(srcs, rects):
            frame.paste(Image.fromarray(a).crop((0, 0, a.shape[1], a.shape[0])).resize((w, h), Image.BILINEAR), (left, top))
        u8 = np.zeros((H, W, 3), np.uint8)
        for a, (top, left, h, w) in zip(srcs, rects):
            u8[top:top + h, left:left + w] = O.resize_bilinear_u8(O.compose_input(a), h, w)
        assert np.array_equal(u8, np.asarray(frame)), (H, W, cx, cy)
        got = R.compose(srcs, [(None, None, False)] * 4, rects, (H, W))
        t = torch.from_numpy(u8).permute(2, 0, 1).contiguous().float().div(255)
        want = t.sub_(torch.tensor(O.IMAGENET_MEAN).view(3, 1, 1)).div_(torch.tensor(O.IMAGENET_STD).view(3, 1, 1)).numpy()
        assert np.array_equal(got, want)
    with pytest.raises(AssertionError):
        R.compose(srcs, [(None, None, False)] * 4, ((0, 0, 10, 10),) * 4, (20, 20))


# ---- what must not change ------------------------------------------------------------------------------------------------------
def _same_item(a, b):
    assert len(a) == len(b) and type(a[0]) is type(b[0])
    assert np.array_equal(a[0].pixels, b[0].pixels) and a[0].plan == b[0].plan and a[3] == b[3]
    assert all(torch.equal(x, y) for x, y in zip(a[1:3] + a[4:], b[1:3] + b[4:]))


@pytest.mark.parametrize("seed", [0, 1, 7, 1234])
def test_mosaic_zero_draws_nothing_and_changes_nothing(files, seed):
    for kw in ({}, {"keep_difficult": "ignore"}):
        plain, zero = _dataset(files, **kw), _dataset(files, mosaic=0.0, **kw)
        random.seed(seed)
        a = [plain[i] for i in range(len(SIZES))]
        state = random.getstate()
        random.seed(seed)
        b = [zero[i] for i in range(len(SIZES))]
        assert random.getstate() == state
        for x, y in zip(a, b):
            _same_item(x, y)
    random.seed(seed)
    t = _dataset(files, isTest=True, mosaic=1.0)[2]                    # test items are never composed, and draw nothing
    assert type(t[0]).__name__ == "RawImage" and random.random() == random.Random(seed).random()


def test_plan_transform_without_expand_and_its_default(files, gold_dir):
    from objectdetection_ssd_amd import Dataset
    b, c, _ = _kept(files, False)
    seen = set()
    for seed in range(40):
        i = seed % len(SIZES)
        h, w = SIZES[i]
        random.seed(seed)
        plan, pb, pl = Dataset.plan_transform(w, h, torch.from_numpy(b[i]), torch.from_numpy(c[i]), expand=False)
        state = random.getstate()
        random.seed(seed)
        photo, canvas, crop, flip, rb, rl = R.plan_without_expand(w, h, b[i], c[i])
        assert random.getstate() == state                                    # the same number of draws
        assert plan.canvas == (h, w, 0, 0) == canvas and _plan_tuple(plan) == (photo, canvas, crop, flip)
        assert np.array_equal(pb.numpy(), rb) and np.array_equal(pl.numpy(), rl)
        seen.add((crop != (0, 0, h, w), flip))
    assert len(seen) == 4
    z = np.load(os.path.join(gold_dir, "augment.npz"))
    for ci in range(int(z["n_cases"])):                                      # expand=True is the default, and today's result
        p = f"c{ci}_"
        img = z[p + "img"]
        args = (img.shape[1], img.shape[0], torch.from_numpy(z[p + "boxes"]), torch.from_numpy(z[p + "labels"]))
        random.seed(int(z[p + "seed"]))
        plan, pb, pl = Dataset.plan_transform(*args, photometric=False, expand=True)
        state = random.getstate()
        random.seed(int(z[p + "seed"]))
        assert Dataset.plan_transform(*args, photometric=False)[0] == plan and random.getstate() == state
        assert (plan.size[1], plan.size[0]) == tuple(z[p + "out_shape"]) and plan.flip == bool(z[p + "flipped"])
        assert np.array_equal(pb.numpy(), z[p + "out_boxes"]) and np.array_equal(pl.numpy(), z[p + "out_labels"])


# ---- seeded mosaic samples -----------------------------------------------------------------------------------------------------
def _reference(files, index, seed, keep_difficult=False, **kw):
    b, c, ig = _kept(files, keep_difficult)
    random.seed(seed)
    assert random.random() < 1.0                                             # the coin of mosaic=1.0
    return R.sample(index, SIZES, b, c, ig if keep_difficult == "ignore" else None, **kw)


def _check_sample(files, item, ref, out_hw=(300, 300)):
    from objectdetection_ssd_amd import Dataset
    im = item[0]
    assert isinstance(im, Dataset.MosaicImage) and im.size == (out_hw[1], out_hw[0]) and tuple(im.out_hw) == out_hw
    assert tuple(im.rects) == ref["rects"] and len(im.sources) == 4
    hits = np.zeros(out_hw, np.int32)
    for top, left, h, w in im.rects:
        assert h >= 1 and w >= 1
        hits[top:top + h, left:left + w] += 1
    assert (hits == 1).all()                                                 # the rectangles tile the frame
    for src, m, plan in zip(im.sources, ref["members"], ref["plans"]):
        assert np.array_equal(src.pixels, files["pixels"][m]) and _plan_tuple(src.plan) == plan
    assert item[2].dtype == torch.float32 and np.array_equal(item[2].numpy(), ref["boxes"])
    assert np.array_equal(item[1].numpy(), ref["labels"]) and item[3] == 100 + ref["members"][0]
    assert float(item[2].min()) >= 0.0 and float(item[2].max()) <= 1.0 and item[2].shape[0] >= 1


def test_seeded_samples_equal_the_restatement(files):
    ds = _dataset(files, mosaic=1.0)
    clamped = filtered = 0
    for seed in range(24):
        index = seed % len(SIZES)
        ref = _reference(files, index, seed)
        state = random.getstate()
        random.seed(seed)
        item = ds[index]
        assert random.getstate() == state and len(item) == 4
        _check_sample(files, item, ref)
        filtered += len(ref["all_boxes"]) > len(ref["boxes"])
        for (photo, canvas, crop, flip), (top, left, h, w) in zip(ref["plans"], ref["rects"]):
            # the edge-touching box of a mirrored, uncropped tile sits at x = -1 before the clamp: it must start AT the rectangle
            if flip and crop[2:] == canvas[:2]:
                assert (ref["all_boxes"][:, 0] == np.float32(left) / np.float32(300)).any()
                clamped += 1
    assert clamped >= 1 and filtered >= 1                                    # both rules were at work


def test_other_centres_sizes_and_the_argument_checks(files):
    ds = _dataset(files, mosaic=1.0, mosaic_center=(0.5, 0.5), mosaic_min_box=5.0, mosaic_size=(64, 48))
    ref = _reference(files, 1, 5, center=(0.5, 0.5), min_box=5.0, out_hw=(64, 48))
    random.seed(5)
    item = ds[1]
    _check_sample(files, item, ref, (64, 48))
    assert item[0].rects == ((0, 0, 32, 24), (0, 24, 32, 24), (32, 0, 32, 24), (32, 24, 32, 24))
    for bad in ({"mosaic_center": (0.0, 0.5)}, {"mosaic_center": (0.6, 0.5)}, {"mosaic_center": (0.5, 1.0)},
                {"mosaic_center": (0.01, 0.5), "mosaic_size": (64, 48)}, {"mosaic": 1.5}):
        with pytest.raises(ValueError):
            _dataset(files, **bad)


def test_keep_largest_when_no_box_is_large_enough(files):
    """every box one source pixel small: none is `mosaic_min_box` wide once it is in its tile, and the sample keeps the largest one"""
    from objectdetection_ssd_amd import Dataset
    tiny = [[[w * 0.5, h * 0.5, w * 0.5 + 1.0, h * 0.5 + 1.0], [w * 0.25, h * 0.25, w * 0.25 + 1.0, h * 0.25 + 1.0]] for h, w in SIZES]
    labels = [["dog", "cat"]] * len(SIZES)
    ds = Dataset.MultiImageMultiBBoxDataset(files["paths"], tiny, labels, [[0, 0]] * len(SIZES), list(range(len(SIZES))), mosaic=1.0,
                                            mosaic_min_box=400.0)
    b = [np.asarray(t, np.float32) for t in tiny]
    c = [np.asarray([float(Dataset.label_to_class[n]) for n in ls], np.float32) for ls in labels]
    for seed in range(6):
        random.seed(seed)
        random.random()
        ref = R.sample(seed, SIZES, b, c, min_box=400.0)
        random.seed(seed)
        item = ds[seed]
        area = (ref["all_boxes"][:, 2] - ref["all_boxes"][:, 0]) * (ref["all_boxes"][:, 3] - ref["all_boxes"][:, 1])
        assert len(ref["all_boxes"]) >= 4 and item[2].shape == (1, 4)
        assert np.array_equal(item[2].numpy()[0], ref["all_boxes"][int(np.argmax(area))]) and np.array_equal(item[2].numpy(), ref["boxes"])
        assert np.array_equal(item[1].numpy(), ref["labels"])


def test_ignore_boxes_go_through_map_regions_and_the_same_mapping(files):
    from objectdetection_ssd_amd import Dataset
    ds = _dataset(files, mosaic=1.0, keep_difficult="ignore")
    some = 0
    for seed in range(12):
        index = seed % len(SIZES)
        ref = _reference(files, index, seed, keep_difficult="ignore")
        random.seed(seed)
        item = ds[index]
        assert len(item) == 5
        _check_sample(files, item, ref)
        assert item[4].dtype == torch.float32 and item[4].shape[1] == 4 and np.array_equal(item[4].numpy(), ref["ignore"])
        # the package's own map_regions, then the mapping, by hand
        want = []
        for src, m, rect in zip(item[0].sources, ref["members"], ref["rects"]):
            df = np.asarray(files["difficult"][m]) != 0
            g = Dataset.map_regions(src.plan, torch.tensor(files["boxes"][m])[torch.from_numpy(df)]).numpy()
            want.append(R.carry(g, src.plan.crop[2:], rect, 300, 300))
        want = np.concatenate(want)
        assert np.array_equal(item[4].numpy(), want[(want[:, 2] > want[:, 0]) & (want[:, 3] > want[:, 1])])
        some += item[4].shape[0]
    assert some >= 4


# ---- collation -----------------------------------------------------------------------------------------------------------------
def _same_batch(a, b):
    assert torch.equal(a.arena, b.arena) and a.offsets == b.offsets and a.plans == b.plans and a.out_hw == b.out_hw
    assert a.tiles == b.tiles and a.shape == b.shape and len(a) == len(b) and a.headers is None and b.headers is None


def test_mixed_batch_carries_its_tile_list(files, monkeypatch):
    from objectdetection_ssd_amd import Dataset
    random.seed(3)
    mos = _dataset(files, mosaic=1.0)
    plain = _dataset(files)
    items = [plain[0], mos[1], mos[2], plain[3]]
    x, classes, boxes, indices = Dataset.collate_fn(items)
    assert isinstance(x, Dataset.RawBatch) and indices == [100, 101, 102, 103] and len(classes) == len(boxes) == 4
    want = [(0, 0, 0, 0, 300, 300)]
    want += [(1 + k, 1) + r for k, r in enumerate(items[1][0].rects)] + [(5 + k, 2) + r for k, r in enumerate(items[2][0].rects)]
    want += [(9, 3, 0, 0, 300, 300)]
    assert x.tiles == want and len(x.plans) == len(x.offsets) == 10
    assert x.shape == torch.Size((4, 3, 300, 300)) and x.size(0) == len(x) == x.n_images == 4
    srcs = [items[0][0]] + list(items[1][0].sources) + list(items[2][0].sources) + [items[3][0]]
    assert x.plans == [s.plan for s in srcs]
    for s, o in zip(srcs, x.offsets):
        assert o % 256 == 0 and np.array_equal(x.arena.numpy()[o:o + s.pixels.size], s.pixels.reshape(-1))
    _same_batch(pickle.loads(pickle.dumps(x)), x)
    if not torch.cuda.is_available():                                        # pinning itself needs the device; the batch's part does not
        monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self.clone())
    _same_batch(x.pin_memory(), x)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            x.to("cpu")
    # samples with ignore boxes: the fifth list comes back beside a mixed batch too
    ig = _dataset(files, mosaic=1.0, keep_difficult="ignore")
    ip = _dataset(files, keep_difficult="ignore")
    out = Dataset.collate_fn([ig[0], ip[1]])
    assert len(out) == 5 and len(out[4]) == 2 and out[0].tiles is not None and out[0].shape[0] == 2


def test_batch_without_a_mosaic_is_todays_batch(files):
    from objectdetection_ssd_amd import Dataset
    ds = _dataset(files, mosaic=0.5)
    random.seed(0)
    items = []
    while len(items) < 4:                                                    # the plain samples of a dataset that also makes mosaics
        it = ds[len(items)]
        if not isinstance(it[0], Dataset.MosaicImage):
            items.append(it)
    x = Dataset.collate_fn(items)[0]
    ref = Dataset.pack_batch([it[0].pixels for it in items], [it[0].plan for it in items])
    assert x.tiles is None and ref.tiles is None and x.n_images == 4
    assert x.arena.numpy().tobytes() == ref.arena.numpy().tobytes()
    _same_batch(x, ref)
    # ... and what a RawBatch built with today's arguments holds
    old = Dataset.RawBatch(ref.arena, ref.offsets, ref.plans, (300, 300))
    assert vars(old).keys() == vars(x).keys() and old.tiles is None and old.shape == x.shape


def test_pack_batch_refuses_a_wrong_frame_and_a_crop_beyond_the_tap_bound():
    from objectdetection_ssd_amd import Dataset
    px = [np.zeros((h, w, 3), np.uint8) for h, w in ((40, 50), (40, 50), (40, 372), (40, 50))]
    rects = R.rectangles(12, 150, 300, 300)

    def mosaic(out_hw=(300, 300), r=rects):
        return Dataset.MosaicImage(tuple(Dataset.RawImage.of(a) for a in px), r, out_hw)
    assert Dataset.pack_batch([mosaic()]).tiles == [(k, 0) + r for k, r in enumerate(rects)]          # 372 columns into 12: 31 exactly
    with pytest.raises(ValueError, match="composed for"):
        Dataset.pack_batch([mosaic((64, 48))])
    with pytest.raises(ValueError, match="composed for"):
        Dataset.pack_batch([mosaic()], size=(64, 48))
    with pytest.raises(ValueError, match="31 source pixels"):
        Dataset.pack_batch([mosaic(r=R.rectangles(11, 150, 300, 300))])                               # into 11: beyond it
    with pytest.raises(ValueError, match="one plan per image"):
        Dataset.pack_batch([mosaic()], [None, None])


# ---- the C entry's refusals ----------------------------------------------------------------------------------------------------
OK_PTR, ODD_PTR = 0x10000, 0x10004
OK, BAD_SHAPE, WORKSPACE, NULL, ALIGN = 0, -1, -2, -3, -5
H, W = 30, 20


@pytest.fixture(scope="module")
def lib():
    """Every case is refused before anything is enqueued, so the made-up pointers are never dereferenced; where a GPU is present the
    tests do not run, so that no tuple can reach a launch on a shared machine (the manner of tests/test_elementwise_status_cpu.py)."""
    if torch.cuda.is_available():
        pytest.skip("made-up pointers: only where no launch can succeed")
    from objectdetection_ssd_amd import _lib
    return _lib.load()


def _tile(image, top, left, h, w, sh=40, sw=50):
    from objectdetection_ssd_amd import _lib
    t = _lib.TileDesc()
    d = t.src
    d.src_offset, d.src_h, d.src_w, d.canvas_h, d.canvas_w, d.crop_h, d.crop_w = 0, sh, sw, sh, sw, sh, sw
    t.out_image, t.dst_top, t.dst_left, t.dst_h, t.dst_w = image, top, left, h, w
    return t


def _array(tiles):
    """the tile list as the C entry wants it: reserved[] filled with the packed scratch layout the header states"""
    from objectdetection_ssd_amd import _lib
    a = (_lib.TileDesc * len(tiles))()
    rows = units = 0
    for i, t in enumerate(tiles):
        C.memmove(C.byref(a[i]), C.byref(t), C.sizeof(_lib.TileDesc))
        a[i].reserved[0], a[i].reserved[1], a[i].reserved[2] = rows, units, 0
        rows += max(t.dst_w, 0) + max(t.dst_h, 0)
        units += (max(t.src.crop_h, 0) * max(t.dst_w, 0) * 3 + 255) // 256
    return a


def _four(image=0):
    return [_tile(image, 0, 0, 10, 7), _tile(image, 0, 7, 10, 13), _tile(image, 10, 0, 20, 7), _tile(image, 10, 7, 20, 13)]


def _call(lib, tiles, B=1, ws_delta=0, **ptr):
    a = tiles if not isinstance(tiles, list) else _array(tiles)
    n = lib.ssd_preprocess_tiles_workspace(a, len(a), B, H, W)
    p = {k: OK_PTR for k in ("arena", "tiles_dev", "mean", "std", "filler", "out", "workspace")}
    p["tiles_host"] = C.cast(a, C.c_void_p).value
    p.update(ptr)
    return n, lib.ssd_preprocess_tiles_u8(p["arena"], p["tiles_dev"], p["tiles_host"], len(a), B, H, W, p["mean"], p["std"], p["filler"],
                                          p["out"], p["workspace"], max(n, 1 << 20) + ws_delta if ws_delta >= 0 else n + ws_delta, None)


def _changed(i, **fields):
    tiles = _four()
    for k, v in fields.items():
        if k in ("crop_w", "crop_h", "src_w", "canvas_w"):
            setattr(tiles[i].src, k, v)
        else:
            setattr(tiles[i], k, v)
    return tiles


def test_tiles_workspace_query_accepts_what_is_valid(lib):
    """the query only: a call that passes every refusal goes on to launch, which is the GPU tests' business"""
    a = _array(_four())
    n = lib.ssd_preprocess_tiles_workspace(a, 4, 1, H, W)
    rows, ks = 2 * (H + W), 2 * 8 + 1                                        # 50 columns into 7: ceil(7.14) = 8 -> 17 taps
    units = sum((40 * w * 3 + 255) // 256 for w in (7, 13, 7, 13))
    align = lambda v: (v + 255) & ~255                                       # noqa: E731
    assert n == align(rows * 2 * 4) + align(rows * ks * 4) + units * 256     # the sum of the tiles' needs
    # a one-pixel-wide tile (31 source columns: the tap bound exactly), and plain full-frame tiles of two images
    assert lib.ssd_preprocess_tiles_workspace(_array([_tile(0, 0, 0, H, 1, sw=31), _tile(0, 0, 1, H, W - 1)]), 2, 1, H, W) > 0
    assert lib.ssd_preprocess_tiles_workspace(_array([_tile(0, 0, 0, H, W), _tile(1, 0, 0, H, W)]), 2, 2, H, W) > 0
    assert lib.ssd_preprocess_tiles_workspace(_array(_four(1) + [_tile(0, 0, 0, H, W)]), 5, 2, H, W) > 0          # any order of the images
    # the 31 x 7 columns of the tap bound itself are taken
    assert lib.ssd_preprocess_tiles_workspace(_array(_changed(0, crop_w=7 * 31, src_w=7 * 31, canvas_w=7 * 31)), 4, 1, H, W) > 0


DEFECTS = {
    "gap": (_changed(3, dst_w=12), 1),
    "overlap": (_changed(3, dst_left=6, dst_w=14), 1),
    "overlap-same-area": (_changed(1, dst_left=6), 1),
    "outside-right": (_changed(3, dst_w=14), 1),
    "outside-bottom": (_changed(2, dst_h=21), 1),
    "negative-top": (_changed(0, dst_top=-1), 1),
    "image-1-of-1": (_changed(0, out_image=1), 1),
    "image-negative": (_changed(0, out_image=-1), 1),
    "image-without-a-tile": (_four(), 2),
    "twice": (_four() + _four(), 1),
    "dst_w-0": (_changed(0, dst_w=0), 1),
    "dst_h-0": (_changed(0, dst_h=0), 1),
    "taps": (_changed(0, crop_w=7 * 31 + 1, src_w=7 * 31 + 1, canvas_w=7 * 31 + 1), 1),
    "crop-outside-canvas": (_changed(0, crop_w=51), 1),
}


@pytest.mark.parametrize("name", list(DEFECTS))
def test_tiles_entry_refuses_for_shape(lib, name):
    tiles, B = DEFECTS[name]
    n, status = _call(lib, tiles, B=B)
    assert n == 0 and status == BAD_SHAPE
    assert _call(lib, tiles, B=B, workspace=ODD_PTR)[1] == BAD_SHAPE         # shape comes before alignment and workspace
    assert _call(lib, tiles, B=B, out=None)[1] == NULL                       # and a NULL pointer before shape


def test_tiles_entry_refuses_counts_pointers_layout_alignment_and_workspace(lib):
    a = _array(_four())
    for T, B, h, w in ((0, 1, H, W), (-1, 1, H, W), (4, 0, H, W), (4, 1, 0, W), (4, 1, H, -1), (65536, 1, H, W), (4, 65536, H, W)):
        assert lib.ssd_preprocess_tiles_workspace(a, T, B, h, w) == 0
        assert lib.ssd_preprocess_tiles_u8(OK_PTR, OK_PTR, a, T, B, h, w, OK_PTR, OK_PTR, OK_PTR, OK_PTR, OK_PTR, 1 << 30, None) == BAD_SHAPE
    assert lib.ssd_preprocess_tiles_workspace(None, 4, 1, H, W) == 0
    for name in ("arena", "tiles_dev", "tiles_host", "mean", "std", "filler", "out", "workspace"):
        assert _call(lib, _four(), **{name: None})[1] == NULL, name
    for k, v in ((0, 1), (1, 1), (2, 1)):                                    # reserved[] that is not the packed layout
        b = _array(_four())
        b[2].reserved[k] += v
        assert lib.ssd_preprocess_tiles_workspace(b, 4, 1, H, W) > 0 and _call(lib, b)[1] == BAD_SHAPE
    assert _call(lib, _four(), workspace=ODD_PTR)[1] == ALIGN
    assert _call(lib, _four(), ws_delta=-1)[1] == WORKSPACE
    assert _call(lib, _four(), ws_delta=-1, workspace=ODD_PTR)[1] == ALIGN   # alignment before workspace
    assert _call(lib, _four(), ws_delta=-1, workspace=None)[1] == NULL


def test_header_binding_and_library_agree_on_the_two_entries():
    import re
    from objectdetection_ssd_amd import _lib
    lib = _lib.load()
    with open(os.path.join(os.path.dirname(_lib.PKG), "include", "ssd_gfx950.h")) as f:
        hdr = f.read()
    for name, n_args in (("ssd_preprocess_tiles_workspace", 5), ("ssd_preprocess_tiles_u8", 14)):
        decl = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert decl and len(decl.group(1).split(",")) == n_args == len(_lib.SIGNATURES[name][1]) and hasattr(lib, name)
    assert C.sizeof(_lib.TileDesc) == C.sizeof(_lib.ImageDesc) + 8 * 4 == 88 and _lib.TileDesc.dst_w.offset == 72

"""Random affine augmentation, host half (no GPU): the restatement of tests/affine_ref.py against the exact consequences of the kernel
specification and against a float64 evaluation; the draws, matrix, boxes and ignore boxes of
`Dataset.MultiImageMultiBBoxDataset(affine=...)` against the test's own replay; `affine=0.0` against today's draw sequence; the
matrices through `pack_batch`, `collate_fn`, pickle and `pin_memory()`; and every refusal of `ssd_affine_warp_f32`, which is made
before anything is enqueued."""
import ctypes as C
import dataclasses
import json
import os
import pickle
import random

import numpy as np
import pytest
import torch

import affine_ref as R

SIZES = [(37, 53), (120, 90), (375, 500), (64, 200), (300, 300), (90, 61)]          # (h, w)
LABELS = ["dog", "cat", "person", "car", "bus", "bird"]
H300 = W300 = 300


# ---- the restatement itself ----------------------------------------------------------------------------------------------------
def test_restatement_identity_shift_quarter_turn_and_far_translation():
    fl = R.fill()
    x = R.noise(1, 24, 24, 1)
    assert np.array_equal(R.warp(x, [R.IDENTITY]), x)                                # a bit-exact copy
    y = R.noise(1, 13, 17, 2)
    assert np.array_equal(R.warp(y, [R.IDENTITY]), y)
    got = R.warp(y, [(1, 0, -3, 0, 1, 2)])[0]                                        # out[oy, ox] = in[oy + 2, ox - 3]
    want = np.broadcast_to(fl.reshape(3, 1, 1), (3, 13, 17)).copy()
    want[:, :11, 3:] = y[0][:, 2:, :14]
    assert np.array_equal(got, want)
    got = R.warp(x, [(0, 1, 0, -1, 0, 24)])[0]                                       # sx = oy, sy = 23 - ox: an exact permutation
    want = np.empty_like(x[0])
    for oy in range(24):
        for ox in range(24):
            want[:, oy, ox] = x[0][:, 23 - ox, oy]
    assert np.array_equal(got, want) and np.array_equal(np.sort(got.reshape(-1)), np.sort(x.reshape(-1)))
    for m in ((1, 0, 1e6, 0, 1, 0), (1, 0, 0, 0, 1, -1e6), (1e30, 0, 0, 0, 1, 0), (3e38, -3e38, 3e38, 0, 1, 0)):  # the last: +-inf, and inf - inf
        assert np.array_equal(R.warp(y, [m])[0], np.broadcast_to(fl.reshape(3, 1, 1), (3, 13, 17))), m
    # continuous across the border: half a pixel out, half filler
    half = R.warp(y, [(1, 0, -0.5, 0, 1, 0)])[0]
    assert np.array_equal(half[:, :, 0], (fl.reshape(3, 1) + (y[0][:, :, 0] - fl.reshape(3, 1)) * np.float32(0.5)).astype(np.float32))


def test_fill_is_the_vertical_pass_of_the_filler():
    import ssd_oracle as O
    from objectdetection_ssd_amd import Dataset
    u8 = np.empty((4, 4, 3), np.uint8)
    u8[:] = np.asarray(R.FILLER_U8, np.uint8)
    want = O.preprocess_image(u8, 4, 4)[:, 0, 0]
    assert np.array_equal(R.fill(), want) and np.array_equal(np.asarray(Dataset.affine_fill(), np.float32), want)


@pytest.mark.parametrize("shape", R.DISTANCE_SHAPES)
def test_restatement_against_float64_grid_sample(shape, gold_dir):
    """normalised 8-bit noise, matrices drawn in the default ranges: within 4 x the recorded distance of the float64 evaluation (the
    error is float32 coordinate rounding times the local gradient: it grows with the frame, not with the draw)"""
    Hh, Ww = shape
    with open(os.path.join(gold_dir, R.DISTANCE_FILE)) as f:
        bar = 4.0 * json.load(f)["distance"][f"{Hh}x{Ww}"]
    for seed in (0, 1):                                                              # the recorded draw, and another
        d = R.distance(Hh, Ww, seed)
        print(f"affine restatement vs float64 at {Hh}x{Ww}, seed {seed}: {d:.3e} (bar {bar:.3e})")
        assert 0 < d <= bar
    # the border too: the float64 evaluation of a shift by half a pixel is half filler
    x = R.noise(1, Hh, Ww, 5)
    m = [(1, 0, -0.5, 0, 1, 0.25)]
    assert np.abs(R.warp(x, m) - R.warp_f64(x, m)).max() <= bar


def test_closed_form_matrix_is_the_product_of_the_four_maps():
    rng = random.Random(4)
    for Ww, Hh in ((300, 300), (48, 64), (500, 375)):
        for _ in range(20):
            d = R.draw(Ww, Hh, rng, degrees=45.0, scale=(0.5, 2.0), shear=20.0, translate=0.3)
            M, coef = R.matrix(Ww, Hh, *d)
            P, Pinv = R.matrix_by_products(Ww, Hh, *d)
            assert np.allclose(np.asarray(M).reshape(2, 3), P[:2], rtol=1e-12, atol=1e-9)
            assert np.allclose(np.asarray(coef).reshape(2, 3), Pinv[:2], rtol=1e-6, atol=1e-4)
            assert all(float(np.float32(v)) == v for v in coef)                      # float32 values


# ---- the dataset ---------------------------------------------------------------------------------------------------------------
def _boxes(h, w, rng, n):
    out = [[w * 0.4, h * 0.3, float(w), float(h)]]
    for _ in range(n - 1):
        x0, y0 = rng.uniform(0, w * 0.6), rng.uniform(0, h * 0.6)
        out.append([x0, y0, x0 + rng.uniform(w * 0.2, w * 0.4), y0 + rng.uniform(h * 0.2, h * 0.4)])
    return np.asarray(out, np.float32).tolist()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp("affine")
    rng = np.random.default_rng(12)
    paths, boxes, labels, difficult = [], [], [], []
    for i, (h, w) in enumerate(SIZES):
        p = str(d / f"a{i}.png")
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(p)
        paths.append(p)
        boxes.append(_boxes(h, w, rng, 4))
        labels.append([LABELS[(i + k) % len(LABELS)] for k in range(4)])
        difficult.append([0, 1, 0, 0])
    return {"paths": paths, "boxes": boxes, "labels": labels, "difficult": difficult}


def _dataset(f, **kw):
    from objectdetection_ssd_amd import Dataset
    return Dataset.MultiImageMultiBBoxDataset(f["paths"], f["boxes"], f["labels"], f["difficult"], list(range(100, 100 + len(SIZES))), **kw)


def _pixels(im):
    from objectdetection_ssd_amd import Dataset
    return [s.pixels for s in im.sources] if isinstance(im, Dataset.MosaicImage) else [im.pixels]


def _plans(im):
    from objectdetection_ssd_amd import Dataset
    return [s.plan for s in im.sources] + [im.rects] if isinstance(im, Dataset.MosaicImage) else [im.plan]


def _same_image(a, b):
    assert type(a) is type(b) and _plans(a) == _plans(b)
    assert all(np.array_equal(p, q) for p, q in zip(_pixels(a), _pixels(b)))


def _same_item(a, b):
    assert len(a) == len(b) and a[3] == b[3] and a[0].warp == b[0].warp
    _same_image(a[0], b[0])
    assert all(torch.equal(x, y) for x, y in zip(a[1:3] + a[4:], b[1:3] + b[4:]))


@pytest.mark.parametrize("seed", [0, 3, 1234])
@pytest.mark.parametrize("kw", [{}, {"mosaic": 1.0}, {"mosaic": 0.5, "keep_difficult": "ignore"}], ids=["plain", "mosaic", "mixed-ignore"])
def test_affine_zero_draws_nothing_and_changes_nothing(files, seed, kw):
    without, zero = _dataset(files, **kw), _dataset(files, affine=0.0, **kw)
    random.seed(seed)
    a = [without[i] for i in range(len(SIZES))]
    state = random.getstate()
    random.seed(seed)
    b = [zero[i] for i in range(len(SIZES))]
    assert random.getstate() == state
    for x, y in zip(a, b):
        _same_item(x, y)
        assert y[0].warp is None
    random.seed(seed)
    t = _dataset(files, isTest=True, affine=1.0, **kw)[2]                            # test items are never warped, and draw nothing
    assert t[0].warp is None and random.random() == random.Random(seed).random()


@pytest.mark.parametrize("kw", [{}, {"mosaic": 1.0}, {"keep_difficult": "ignore"}, {"mosaic": 1.0, "keep_difficult": "ignore"}],
                         ids=["plain", "mosaic", "plain-ignore", "mosaic-ignore"])
def test_seven_draws_the_matrix_and_the_boxes_equal_the_replay(files, kw):
    """the sample is formed first, with today's draws; then the coin; then angle, scale, two shears, two translations"""
    base, ds = _dataset(files, **kw), _dataset(files, affine=1.0, **kw)
    warped = 0
    for seed in range(12):
        i = seed % len(SIZES)
        random.seed(seed)
        plain = base[i]
        assert random.random() < 1.0                                                 # the coin
        M, coef = R.matrix(W300, H300, *R.draw(W300, H300, random))
        state = random.getstate()
        random.seed(seed)
        item = ds[i]
        assert random.getstate() == state and len(item) == len(plain)
        _same_image(item[0], plain[0])
        want, keep = R.map_boxes(M, plain[2].numpy(), W300, H300)
        assert any(keep)
        assert item[0].warp == coef + (300.0, 300.0) and all(float(np.float32(v)) == v for v in item[0].warp)
        assert item[2].dtype == torch.float32 and np.array_equal(item[2].numpy(), want[keep])
        assert torch.equal(item[1], plain[1][torch.tensor(keep)]) and item[3] == plain[3]
        assert float(item[2].min()) >= 0.0 and float(item[2].max()) <= 1.0
        if len(item) == 5:
            ig, left = R.map_boxes(M, plain[4].numpy(), W300, H300, None)
            assert item[4].dtype == torch.float32 and np.array_equal(item[4].numpy(), ig[left])
        warped += 1
    assert warped == 12


def test_other_ranges_reach_the_draws_and_bad_arguments_are_refused(files):
    kw = dict(affine_degrees=30.0, affine_scale=(0.5, 0.6), affine_shear=10.0, affine_translate=0.25, affine_size=(64, 48),
              affine_min_box=1.0, affine_min_visible=0.1)
    base, ds = _dataset(files), _dataset(files, affine=1.0, **kw)
    random.seed(9)
    plain = base[2]
    random.random()
    M, coef = R.matrix(48, 64, *R.draw(48, 64, random, 30.0, (0.5, 0.6), 10.0, 0.25))
    random.seed(9)
    item = ds[2]
    want, keep = R.map_boxes(M, plain[2].numpy(), 48, 64, 1.0, 0.1)
    assert item[0].warp == coef + (64.0, 48.0) and np.array_equal(item[2].numpy(), want[keep])
    for bad in ({"affine": 1.5}, {"affine": -0.1}, {"affine_scale": (0.0, 1.0)}, {"affine_scale": (1.2, 1.1)}, {"affine_degrees": -1.0},
                {"affine_shear": -1.0}, {"affine_shear": 45.0}, {"affine_translate": -0.1}, {"affine_min_box": -1.0},
                {"affine_min_visible": -0.5}, {"affine_size": (0, 300)}, {"affine": 0.5, "mosaic": 0.5, "affine_size": (64, 48)}):
        with pytest.raises(ValueError):
            _dataset(files, **bad)
    import inspect
    from objectdetection_ssd_amd import Dataset
    names = list(inspect.signature(Dataset.MultiImageMultiBBoxDataset.__init__).parameters)
    assert names[-1] == "decode" and names[names.index("mosaic_size") + 1:-1] == [
        "affine", "affine_degrees", "affine_scale", "affine_shear", "affine_translate", "affine_min_box", "affine_min_visible", "affine_size"]


def test_coin_below_one_warps_some_samples(files):
    ds = _dataset(files, affine=0.5)
    random.seed(2)
    hits = [ds[i % len(SIZES)][0].warp is not None for i in range(40)]
    assert 8 <= sum(hits) <= 32


# ---- boxes ---------------------------------------------------------------------------------------------------------------------
BOXES = torch.tensor([[0.1, 0.2, 0.5, 0.7], [0.0, 0.0, 1.0, 1.0], [0.25, 0.5, 0.75, 0.625], [1 / 3, 1 / 7, 2 / 3, 6 / 7]], dtype=torch.float32)


def test_identity_leaves_boxes_bit_equal_and_a_quarter_turn_permutes_them():
    from objectdetection_ssd_amd import Dataset
    for Ww, Hh in ((300, 300), (48, 64), (517, 333)):
        new, keep = Dataset.affine_boxes((1, 0, 0, 0, 1, 0), BOXES, Ww, Hh)
        assert new.dtype == torch.float32 and torch.equal(new, BOXES) and keep.all()
    # forward quarter turn of a square frame: (x, y) -> (W - y, x)
    q = torch.tensor([[0.125, 0.25, 0.5, 0.75], [0.0, 0.0, 1.0, 1.0], [0.375, 0.5, 0.625, 0.5625]], dtype=torch.float32)
    for Ww in (300, 64):
        new, keep = Dataset.affine_boxes((0, -1, Ww, 1, 0, 0), q, Ww, Ww)
        want = torch.stack([1 - q[:, 3], q[:, 0], 1 - q[:, 1], q[:, 2]], 1)          # exact: the coordinates are dyadic
        assert torch.equal(new, want) and keep.all()
        ref, rkeep = R.map_boxes((0, -1, Ww, 1, 0, 0), q.numpy(), Ww, Ww)
        assert np.array_equal(new.numpy(), ref) and keep.tolist() == rkeep


def test_boxes_out_of_the_frame_and_barely_visible_ones_are_dropped():
    from objectdetection_ssd_amd import Dataset
    b = torch.tensor([[0.1, 0.1, 0.3, 0.3], [0.6, 0.1, 0.9, 0.3], [0.01, 0.45, 0.11, 0.55]], dtype=torch.float32)
    # 150 pixels to the right: the first stays whole, the second leaves the frame, the third stays
    new, keep = Dataset.affine_boxes((1, 0, 150, 0, 1, 0), b, 300, 300)
    assert keep.tolist() == [True, False, True] and np.allclose(new[0].numpy(), [0.6, 0.1, 0.8, 0.3], atol=1e-6)
    # 255: the first keeps 15 of its 60 columns, a quarter of the hull -- below 0.3, above 0.2
    shift = (1, 0, 255, 0, 1, 0)
    assert Dataset.affine_boxes(shift, b, 300, 300)[1].tolist() == [False, False, True]
    assert Dataset.affine_boxes(shift, b, 300, 300, 2.0, 0.2)[1].tolist() == [True, False, True]
    assert Dataset.affine_boxes(shift, b, 300, 300, 16.0, 0.2)[1].tolist() == [False, False, True]          # 15 columns wide
    # ignore regions: kept by whatever area is left
    new, keep = Dataset.affine_boxes(shift, b, 300, 300, None)
    assert keep.tolist() == [True, False, True] and np.allclose(new[0].numpy(), [0.95, 0.1, 1.0, 0.3], atol=1e-6) and new[0, 2] == 1.0
    # a rotated box: the hull is looser than the box
    M, _ = R.matrix(300, 300, 45.0, 1.0, 0.0, 0.0, 150.0, 150.0)
    new, keep = Dataset.affine_boxes(M, torch.tensor([[0.45, 0.45, 0.55, 0.55]]), 300, 300)
    assert keep.all() and np.allclose((new[0, 2:] - new[0, :2]).numpy(), 0.1 * np.sqrt(2.0), atol=1e-6)
    for args in ((2.0, 0.3), (None, 0.0)):
        ref, rkeep = R.map_boxes(M, b.numpy(), 300, 300, *args)
        new, keep = Dataset.affine_boxes(M, b, 300, 300, *args)
        assert np.array_equal(new.numpy(), ref) and keep.tolist() == rkeep
    new, keep = Dataset.affine_boxes(M, torch.zeros((0, 4)), 300, 300, None)
    assert new.shape == (0, 4) and keep.shape == (0,)


@pytest.mark.parametrize("kw", [{}, {"mosaic": 1.0, "keep_difficult": "ignore"}], ids=["plain", "mosaic-ignore"])
def test_no_survivor_returns_the_sample_unwarped_with_the_draws_consumed(files, kw):
    base, ds = _dataset(files, **kw), _dataset(files, affine=1.0, affine_min_box=1000.0, **kw)
    for seed in range(4):
        random.seed(seed)
        plain = base[seed]
        random.random()
        R.draw(W300, H300, random)
        state = random.getstate()
        random.seed(seed)
        item = ds[seed]
        assert random.getstate() == state and item[0].warp is None
        _same_item(item, plain)


# ---- collation -----------------------------------------------------------------------------------------------------------------
def _same_batch(a, b):
    assert torch.equal(a.arena, b.arena) and a.offsets == b.offsets and a.plans == b.plans and a.out_hw == b.out_hw
    assert a.tiles == b.tiles and a.warps == b.warps and a.shape == b.shape and len(a) == len(b)


def test_warps_travel_with_plain_mosaic_and_mixed_batches(files, monkeypatch):
    from objectdetection_ssd_amd import Dataset
    random.seed(3)
    plain, warped = _dataset(files), _dataset(files, affine=1.0)
    mosaic, warped_mosaic = _dataset(files, mosaic=1.0), _dataset(files, mosaic=1.0, affine=1.0)
    if not torch.cuda.is_available():                                                # pinning itself needs the device; the batch's part does not
        monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self.clone())
    cases = {"plain": [plain[0], warped[1], warped[2], plain[3]], "mosaic": [warped_mosaic[0], mosaic[1], warped_mosaic[2]],
             "mixed": [plain[0], warped_mosaic[1], warped[2], mosaic[3]]}
    for name, items in cases.items():
        x = Dataset.collate_fn(items)[0]
        want = [None if it[0].warp is None else it[0].warp[:6] for it in items]
        assert sum(w is not None for w in want) == 2 and x.warps == want and len(x.warps) == x.n_images == len(items), name
        assert (x.tiles is None) == (name == "plain")
        bare = Dataset.collate_fn([(dataclasses.replace(it[0], warp=None),) + tuple(it[1:]) for it in items])[0]
        assert bare.warps is None and torch.equal(bare.arena, x.arena) and bare.tiles == x.tiles and bare.plans == x.plans
        _same_batch(pickle.loads(pickle.dumps(x)), x)
        _same_batch(x.pin_memory(), x)
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError):
                x.to("cpu")
    # a batch without a warped entry is today's batch
    x = Dataset.collate_fn([plain[0], plain[1]])[0]
    old = Dataset.RawBatch(x.arena, x.offsets, x.plans, (300, 300))
    assert x.warps is None and old.warps is None and vars(old).keys() == vars(x).keys()
    with pytest.raises(RuntimeError):
        x.to("cpu")


def test_pack_batch_takes_warps_by_argument_or_from_the_entries_and_refuses_another_frame():
    from objectdetection_ssd_amd import Dataset
    px = [np.zeros((40, 50, 3), np.uint8), np.ones((30, 20, 3), np.uint8)]
    w = (1.0, 0.0, 2.0, 0.0, 1.0, -3.0)
    rb = Dataset.pack_batch(px, warps=[None, w + (300.0, 300.0)])
    assert rb.warps == [None, w] and rb.tiles is None
    assert Dataset.pack_batch(px, warps=[None, None]).warps is None and Dataset.pack_batch(px).warps is None
    rb = Dataset.pack_batch(px, size=(64, 48), warps=[w + (64.0, 48.0), None])
    assert rb.warps == [w, None] and rb.out_hw == (64, 48)
    m = Dataset.MosaicImage(tuple(Dataset.RawImage.of(a) for a in (px * 2)), ((0, 0, 100, 120), (0, 120, 100, 180), (100, 0, 200, 120),
                                                                            (100, 120, 200, 180)), (300, 300), w + (300.0, 300.0))
    rb = Dataset.pack_batch([px[0], m])                                              # the entry's own
    assert rb.warps == [None, w] and len(rb.tiles) == 5
    with pytest.raises(ValueError, match="affine_size"):
        Dataset.pack_batch(px, warps=[None, w + (64.0, 48.0)])
    with pytest.raises(ValueError, match="affine_size"):
        Dataset.pack_batch(px, size=(64, 48), warps=[None, w + (300.0, 300.0)])
    with pytest.raises(ValueError, match="one warp slot"):
        Dataset.pack_batch(px, warps=[None])
    with pytest.raises(ValueError, match="six coefficients"):
        Dataset.pack_batch(px, warps=[None, w])
    with pytest.raises(ValueError, match="six coefficients"):
        Dataset.RawBatch(rb.arena, rb.offsets, rb.plans, (300, 300), tiles=rb.tiles, warps=[None, w[:5]])
    with pytest.raises(ValueError, match="one warp slot"):
        Dataset.RawBatch(rb.arena, rb.offsets, rb.plans, (300, 300), tiles=rb.tiles, warps=[w] * 5)       # per output image, not per source
    # positional construction as before
    assert Dataset.RawImage(px[0], Dataset.identity_plan(40, 50)).warp is None
    assert Dataset.MosaicImage(m.sources, m.rects, (300, 300)).warp is None


# ---- the C entry's refusals ----------------------------------------------------------------------------------------------------
OK_PTR = 0x10000
OK, BAD_SHAPE, NULL = 0, -1, -3


@pytest.fixture(scope="module")
def lib():
    """Every case is refused before anything is enqueued, so the made-up pointers are never dereferenced; where a GPU is present the
    tests do not run, so that no tuple can reach a launch on a shared machine (the manner of tests/test_mosaic_cpu.py)."""
    if torch.cuda.is_available():
        pytest.skip("made-up pointers: only where no launch can succeed")
    from objectdetection_ssd_amd import _lib
    return _lib.load()


def _call(lib, B=2, H=30, W=20, mats=None, **ptr):
    m = np.tile(np.asarray(R.IDENTITY, np.float32), (max(B, 1), 1)) if mats is None else np.ascontiguousarray(mats, np.float32)
    fl = R.fill()
    n = max(B, 1) * 3 * max(H, 1) * max(W, 1) * 4
    p = {"in_": OK_PTR, "out": OK_PTR + n, "mats_dev": OK_PTR, "mats_host": m.ctypes.data, "fill": fl.ctypes.data}
    p.update(ptr)
    return lib.ssd_affine_warp_f32(p["in_"], p["out"], p["mats_dev"], p["mats_host"], B, H, W, p["fill"], None)


def test_warp_entry_refuses_pointers_shapes_overlap_and_non_finite_coefficients(lib):
    for name in ("in_", "out", "mats_dev", "mats_host", "fill"):
        assert _call(lib, **{name: None}) == NULL, name
        assert _call(lib, B=0, **{name: None}) == NULL, name                         # a NULL pointer before shape
    for kw in ({"B": 0}, {"B": -1}, {"H": 0}, {"W": 0}, {"H": -5}, {"W": -1}, {"B": 65536, "H": 1, "W": 1}, {"B": 1, "H": 65536, "W": 32768},
               {"B": 1, "H": 46341, "W": 46341}, {"B": 1, "H": 1, "W": 2 ** 31 - 1, "mats": [[np.nan] * 6]}):
        mats = kw.pop("mats", None)
        if mats is None and kw.get("B", 2) > 2:
            mats = np.zeros((1, 6), np.float32)                                      # never read: the shape is refused first
        assert _call(lib, mats=mats, **kw) == BAD_SHAPE, kw
    n = 2 * 3 * 30 * 20 * 4
    for out in (OK_PTR, OK_PTR + 4, OK_PTR + n - 4, OK_PTR - n + 4):
        assert _call(lib, out=out) == BAD_SHAPE, out
    for bad in (np.nan, np.inf, -np.inf):
        for k in (0, 5, 6, 11):
            m = np.tile(np.asarray(R.IDENTITY, np.float32), (2, 1))
            m.reshape(-1)[k] = bad
            assert _call(lib, mats=m) == BAD_SHAPE, (bad, k)


def test_header_binding_and_library_agree_on_the_entry():
    import re
    from objectdetection_ssd_amd import _lib
    lib = _lib.load()
    with open(os.path.join(os.path.dirname(_lib.PKG), "include", "ssd_gfx950.h")) as f:
        hdr = f.read()
    decl = re.search(r"\bint\s+ssd_affine_warp_f32\s*\(([^;]*?)\)\s*;", hdr, re.S)
    assert decl and len(decl.group(1).split(",")) == 9 == len(_lib.SIGNATURES["ssd_affine_warp_f32"][1]) and hasattr(lib, "ssd_affine_warp_f32")
    assert _lib.SIGNATURES["ssd_affine_warp_f32"][0] is C.c_int


def test_ops_front_end_refuses_host_tensors():
    from objectdetection_ssd_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.affine_warp(torch.zeros(1, 3, 4, 4), np.asarray([R.IDENTITY], np.float32), R.fill())

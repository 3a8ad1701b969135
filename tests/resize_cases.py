"""Host-only builders for tests/test_resize_entry_gpu.py: small images and geometries that take ssd_preprocess_u8's own bookkeeping (the
batch-wide tap stride ks, max_in_h, the [B][2][out_max] coefficient rows) to its edges.  The kernel's logic depends on the ratio of
crop to output, not on 300, so the outputs are a few pixels wide."""
import numpy as np

import ssd_oracle as O

GUARD = 64
PATTERN = 0xA5


class Item:
    """One image of a batch: its pixels and the geometry compose_input takes -- canvas = (canvas_h, canvas_w, top, left) or None,
    crop = (top, left, h, w) of the canvas or None, flip."""

    def __init__(self, img, canvas=None, crop=None, flip=False):
        self.img, self.canvas, self.crop, self.flip = np.ascontiguousarray(img), canvas, crop, bool(flip)

    def window(self):
        """(h, w) of what is resized."""
        if self.crop is not None:
            return self.crop[2], self.crop[3]
        return (self.canvas[0], self.canvas[1]) if self.canvas is not None else self.img.shape[:2]


def image(seed: int, h: int, w: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def layout(items):
    """-> (host arena with GUARD bytes of PATTERN around every image, slots at odd offsets; the _lib.ImageDesc array)"""
    from objectdetection_ssd_amd import _lib
    at, offs = 0, []
    for it in items:
        at += GUARD
        at += 1 - at % 2
        offs.append(at)
        at += it.img.size
    host = np.full(at + GUARD, PATTERN, np.uint8)
    descs = (_lib.ImageDesc * len(items))()
    for d, it, so in zip(descs, items, offs):
        h, w = it.img.shape[:2]
        host[so:so + it.img.size] = it.img.reshape(-1)
        d.src_offset, d.src_h, d.src_w = so, h, w
        d.canvas_h, d.canvas_w, d.place_top, d.place_left = it.canvas if it.canvas is not None else (h, w, 0, 0)
        d.crop_top, d.crop_left, d.crop_h, d.crop_w = it.crop if it.crop is not None else (0, 0, d.canvas_h, d.canvas_w)
        d.flip = int(it.flip)
    return host, descs


def ksize(in_size: int, out_size: int) -> int:
    """Pillow's tap count of one axis: 2 ceil(support) + 1."""
    support = max(in_size / out_size, 1.0)
    return int(np.ceil(support)) * 2 + 1


def oracle(it: Item, out_hw) -> np.ndarray:
    return O.preprocess_image(it.img, out_hw[0], out_hw[1], canvas=it.canvas, crop=it.crop, flip=it.flip)


def pillow(img: np.ndarray, out_hw) -> np.ndarray:
    """PIL resize -> /255 -> normalise, as tests/test_gpu_path.py::test_preprocess_batch_equals_pillow_resize_and_normalize does."""
    import torch
    from PIL import Image
    u8 = np.asarray(Image.fromarray(img).resize((out_hw[1], out_hw[0]), Image.BILINEAR))
    mean = torch.tensor(O.IMAGENET_MEAN).view(3, 1, 1)
    std = torch.tensor(O.IMAGENET_STD).view(3, 1, 1)
    return torch.from_numpy(u8.copy()).permute(2, 0, 1).contiguous().float().div(255).sub_(mean).div_(std).numpy()


# (source h, w), (out h, w): every axis ratio the entry treats differently
RATIOS = (
    ((248, 16), (8, 8)),         # rows 31:1 exactly (ks = 63 = MAX_KSIZE), columns 2:1
    ((24, 248), (8, 8)),         # columns 31:1, rows 3:1
    ((248, 248), (8, 8)),        # both at the bound
    ((8, 8), (8, 8)),            # 1:1: the identity taps
    ((1, 1), (8, 8)),            # 1 -> 8
    ((2, 2), (300, 300)),        # 2 -> 300
    ((1, 40), (8, 8)),           # one pixel high
    ((40, 1), (8, 8)),           # one pixel wide
    ((16, 2), (8, 300)),         # 2:1 down beside 2 -> 300 up
)

# one batch: the ks = 63 image, a ks = 3 image, the tallest crop, a one-row crop
STRIDE_SHAPES = ((8, 248), (5, 8), (248, 9), (1, 20))
STRIDE_OUT = (8, 8)

NONSQUARE_OUTS = ((8, 5), (3, 300), (300, 3), (1, 1))
NONSQUARE_SHAPES = ((20, 31), (7, 9), (31, 2), (1, 1), (13, 30))              # at most 31:1 on every axis of every output

# a 10 x 12 source at (8, 9) of a 30 x 34 canvas: rows 8..17, columns 9..20
GEOM_SRC, GEOM_CANVAS = (10, 12), (30, 34, 8, 9)
GEOM_OUT = (7, 8)
GEOMETRIES = (
    # crop (top, left, h, w), flip
    ((0, 0, 5, 6), False),           # wholly in the filler, above-left
    ((20, 25, 6, 5), True),          # wholly in the filler, below-right, flipped (odd width)
    ((4, 11, 8, 6), False),          # over the top side
    ((14, 11, 8, 6), True),          # over the bottom side, flipped (even width)
    ((10, 5, 5, 8), False),          # over the left side
    ((10, 17, 5, 8), True),          # over the right side, flipped (even width)
    ((3, 4, 9, 9), True),            # over the top-left corner, flipped (odd width)
    ((13, 16, 17, 18), False),       # over the bottom-right corner, to the canvas's last row and column
    ((10, 10, 1, 1), False),         # 1 x 1 inside the source
    ((10, 10, 1, 1), True),
    ((0, 0, 1, 1), False),           # 1 x 1 in the filler
    ((17, 20, 1, 1), False),         # 1 x 1 on the source's last pixel
    ((0, 0, 30, 34), True),          # the whole canvas, flipped
    (None, False),                   # the whole canvas
)


def geometry_items():
    img = image(5, *GEOM_SRC)
    return [Item(img, GEOM_CANVAS, crop, flip) for crop, flip in GEOMETRIES] + [Item(img, None, (2, 3, 5, 7), True), Item(img, None, None, True)]

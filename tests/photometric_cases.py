"""Host-only case builders for csrc/photometric.hip taken bare (ops.photometric_u8): numpy and ctypes, no GPU touched.

A Case is a batch: the 8-bit images, each image's (kind, factor) ops (kind 0 brightness, 1 contrast, 2 saturation, 3 hue) and, on
demand and computed once, the images oracle/ssd_oracle.py's photometric_apply makes of them (tests/test_oracle_golden.py and
tests/test_photometric_cases_cpu.py pin that oracle on Pillow itself).  layout() puts a case into one arena the way
tests/test_jpeg_decode_gpu.py lays out its pixel slots, with the descriptors Dataset.RawBatch.to would fill.

  cube     all 2^24 colours as one 4096 x 4096 image, one hue or saturation op: 64 grid-stride passes under the 256-block cap
  pivots   every contrast pivot 0..255, each image holding all 256 grey values: value x pivot x alpha, exhaustive over 8 bits
  ties     mean(L) exactly on k + 1/2 and one count below it, at 1000 x 1000 and 600 x 600 (both above the block cap)
  mixed    1-pixel to 512 x 513 images under one grid, 0 to 4 ops, every kind at every stage, contrast at differing stages
"""
import functools

import numpy as np

import ssd_oracle as O

GUARD = 64
PATTERN = 0xA5
BLOCK_CAP_PX = 256 * 1024        # ssd_photometric_u8 launches min(256, ceil(max_px / 1024)) blocks: the cap binds above this

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
KIND_NAMES = ("brightness", "contrast", "saturation", "hue")

# the blend's alphas: interpolation (truncation, & 255) on [0, 1] with both edges, the clipping path from the float32 next above 1
ALPHA_ABOVE_ONE = float(np.nextafter(np.float32(1), np.float32(2)))
ALPHAS = (0.5, 1.5, 1.0, 0.0, ALPHA_ABOVE_ONE, 0.75, 1.25)

CUBE_OPS = ((HUE, 0.031), (HUE, -18 / 255.), (SATURATION, 0.5), (SATURATION, 1.5), (SATURATION, 0.999))


class Case:
    def __init__(self, name, images, ops):
        assert len(images) == len(ops)
        for a in images:
            assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3 and a.size > 0
        self.name = name
        self.images = [np.ascontiguousarray(a) for a in images]
        self.ops = [tuple((int(k), float(f)) for k, f in o) for o in ops]
        assert all(len(o) <= 4 and all(0 <= k <= 3 for k, _ in o) for o in self.ops)
        self._expected = None

    def expected(self):
        """The oracle's images, computed once; an image without ops is the input itself."""
        if self._expected is None:
            self._expected = [np.ascontiguousarray(O.photometric_apply(a, o)) for a, o in zip(self.images, self.ops)]
            for e in self._expected:
                e.setflags(write=False)
        return self._expected

    def __repr__(self):
        return f"Case({self.name}, {len(self.images)} images)"


def pivot(img: np.ndarray) -> int:
    """The contrast pivot of an image by the oracle's own formula (photometric_apply, kind 1)."""
    lum = O.rgb_to_l(img)
    return int(float(lum.astype(np.int64).sum()) / float(lum.size) + 0.5)


def grey(values: np.ndarray) -> np.ndarray:
    """(H, W) -> (H, W, 3) with R = G = B, so L is the value itself."""
    return np.repeat(np.asarray(values, np.uint8)[..., None], 3, -1)


# ---- cube ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def cube_image() -> np.ndarray:
    """Pixel i of the flattened image is the colour (i >> 16, (i >> 8) & 255, i & 255)."""
    i = np.arange(1 << 24, dtype=np.uint32)
    a = np.empty((1 << 24, 3), np.uint8)
    a[:, 0] = i >> 16; a[:, 1] = (i >> 8) & 255; a[:, 2] = i & 255
    a = a.reshape(4096, 4096, 3)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def cube(op_index: int) -> Case:
    kind, factor = CUBE_OPS[op_index]
    assert O.hue_delta_u8(0.031) == 7 and O.hue_delta_u8(-18 / 255.) == 238          # a small step and the wrap-around
    return Case(f"cube[{KIND_NAMES[kind]} {factor!r}]", [cube_image()], [((kind, factor),)])


# ---- pivots ----------------------------------------------------------------------------------------------------------------
PIVOT_WIDTH = 37


@functools.lru_cache(maxsize=1)
def pivot_images():
    """images[m] has contrast pivot m.  For m in 1..254: all 256 grey values once, the fewest constant 0 (m < 128) or 255 pixels
    that bring the rounded mean to m -- so the mean lies close under m + 1/2 or over m - 1/2 -- and pixels of value m (which keep
    the mean on its side) up to a whole number of PIVOT_WIDTH-pixel rows; shuffled.  0 and 255 are constant images."""
    rng = np.random.default_rng(41)
    out = [grey(np.zeros((5, 7), np.uint8))]
    for m in range(1, 255):
        pad_value = 0 if m < 128 else 255
        n_pad = 0
        while int((32640.0 + pad_value * n_pad) / (256 + n_pad) + 0.5) != m:
            n_pad += 1
        n = -(-(256 + n_pad) // PIVOT_WIDTH) * PIVOT_WIDTH
        flat = np.concatenate([np.arange(256), np.full(n_pad, pad_value), np.full(n - 256 - n_pad, m)]).astype(np.uint8)
        rng.shuffle(flat)
        img = grey(flat.reshape(-1, PIVOT_WIDTH))
        assert pivot(img) == m and np.array_equal(np.unique(img), np.arange(256))
        out.append(img)
    out.append(grey(np.full((7, 5), 255, np.uint8)))
    assert pivot(out[0]) == 0 and pivot(out[255]) == 255 and len(out) == 256
    return out


@functools.lru_cache(maxsize=None)
def pivots(kind: int, alpha: float) -> Case:
    """All 256 pivot images in one batch under one op (contrast, or brightness on the same ramps)."""
    assert kind in (BRIGHTNESS, CONTRAST)
    imgs = pivot_images()
    return Case(f"pivots[{KIND_NAMES[kind]} {alpha!r}]", imgs, [((kind, alpha),)] * len(imgs))


# ---- ties ------------------------------------------------------------------------------------------------------------------
TIE_K = 100
TIE_SIDES = (1000, 600)


def tie_image(side: int, k: int, below: bool, seed: int) -> np.ndarray:
    """side x side grey pixels of k and k + 1 whose L sum is n k + n / 2 (mean exactly k + 1/2: Pillow's int(mean + .5) is k + 1),
    or with `below` one count less (pivot k)."""
    n = side * side
    assert n % 2 == 0
    ones = n // 2 - (1 if below else 0)
    flat = np.full(n, k, np.uint8)
    flat[:ones] = k + 1
    np.random.default_rng(seed).shuffle(flat)
    img = grey(flat.reshape(side, side))
    assert int(O.rgb_to_l(img).astype(np.int64).sum()) == n * k + ones and pivot(img) == (k if below else k + 1)
    return img


@functools.lru_cache(maxsize=1)
def tie_images():
    """[(image, pivot)]: the tie and one count below it at each side of TIE_SIDES."""
    return [(tie_image(s, TIE_K, below, 7 * s + below), TIE_K if below else TIE_K + 1) for s in TIE_SIDES for below in (False, True)]


@functools.lru_cache(maxsize=None)
def ties(alpha: float) -> Case:
    imgs = [a for a, _ in tie_images()]
    return Case(f"ties[contrast {alpha!r}]", imgs, [((CONTRAST, alpha),)] * len(imgs))


# ---- mixed -----------------------------------------------------------------------------------------------------------------
B_, C_, S_, H_ = BRIGHTNESS, CONTRAST, SATURATION, HUE
# (h, w), the kinds of its ops in order, what the pixels are
MIXED_PLAN = (
    ((1, 1), (), "random"),
    ((1, 7), (C_,), "random"),
    ((7, 1), (H_, C_), "random"),
    ((1, 257), (C_, B_, C_, S_), "random"),                # contrast twice in one image
    ((33, 31), (S_, H_, B_), "random"),                    # 1023 px
    ((32, 32), (B_, C_, S_, H_), "random"),                # 1024 px: the four 4-op lists are a Latin square, so every kind
    ((25, 41), (C_, S_, H_, B_), "random"),                # 1025 px  stands at every stage index
    ((511, 513), (S_, H_, B_, C_), "random"),              # 262 143 px, one below the block cap
    ((512, 512), (), "random"),                            # 262 144 px, on it, and untouched
    ((512, 513), (H_, B_, C_, S_), "random"),              # 262 656 px, above it
    ((40, 50), (C_, H_), "low"),                           # low contrast
    ((30, 20), (H_, S_, C_), "grey"),                      # s == 0 branch of the hue path
    ((1, 1), (B_, S_, C_, H_), "random"),
)
MIXED_CAP_SHAPES = ((511, 513), (512, 512), (512, 513))


@functools.lru_cache(maxsize=1)
def mixed() -> Case:
    rng = np.random.default_rng(43)
    imgs, ops = [], []
    for (h, w), kinds, what in MIXED_PLAN:
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if what == "low":
            a = (a // 16 + 120).astype(np.uint8)
        elif what == "grey":
            a[..., 1] = a[..., 0]; a[..., 2] = a[..., 0]
        imgs.append(a)
        ops.append(tuple((k, float(rng.uniform(-18 / 255., 18 / 255.)) if k == HUE else float(rng.uniform(.5, 1.5))) for k in kinds))
    return Case("mixed", imgs, ops)


# ---- the arena -------------------------------------------------------------------------------------------------------------
def layout(case: Case):
    """One arena with GUARD bytes of PATTERN on either side of every image slot, every slot at an odd offset, and the descriptors as
    Dataset.RawBatch.to fills them for an identity geometry.  -> (host arena, ImageDesc array, PhotoDesc array, [(offset, h, w)])"""
    from objectdetection_ssd_amd import _lib
    at, slots = 0, []
    for a in case.images:
        at += GUARD
        at += 1 - at % 2
        slots.append((at, a.shape[0], a.shape[1]))
        at += a.size
    host = np.full(at + GUARD, PATTERN, np.uint8)
    descs = (_lib.ImageDesc * len(slots))()
    photo = (_lib.PhotoDesc * len(slots))()
    for d, p, a, o, (so, h, w) in zip(descs, photo, case.images, case.ops, slots):
        host[so:so + a.size] = a.reshape(-1)
        d.src_offset, d.src_h, d.src_w = so, h, w
        d.canvas_h, d.canvas_w, d.place_top, d.place_left = h, w, 0, 0
        d.crop_top, d.crop_left, d.crop_h, d.crop_w = 0, 0, h, w
        d.flip = 0
        p.n_ops = len(o)
        for k, (kind, factor) in enumerate(o):
            p.kind[k] = int(kind)
            p.alpha[k] = float(factor)
            p.hue_delta[k] = O.hue_delta_u8(factor) if kind == HUE else 0
    return host, descs, photo, slots


def outside_mask(host_size: int, slots) -> np.ndarray:
    """True at every arena byte that belongs to no slot."""
    m = np.ones(host_size, bool)
    for so, h, w in slots:
        m[so:so + h * w * 3] = False
    return m


def describe_mismatch(case: Case, i: int, got: np.ndarray, want: np.ndarray) -> str:
    """The case, the image's op list, how many pixels differ and the first one as input, got and want."""
    bad = np.flatnonzero((got != want).any(-1).reshape(-1))
    src = case.images[i].reshape(-1, 3)
    j = int(bad[0])
    return (f"{case.name} image {i} {case.images[i].shape[:2]} ops {case.ops[i]}: {bad.size} of {src.shape[0]} pixels differ; first at "
            f"pixel {j}: input {src[j].tolist()} got {got.reshape(-1, 3)[j].tolist()} want {want.reshape(-1, 3)[j].tolist()}")

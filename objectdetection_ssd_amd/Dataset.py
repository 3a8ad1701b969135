"""Host-side mirror of the reference's `Dataset.py` / `Util.transform` geometry with the pixel work on the GPU
(SURVEY.md section 8(f) row 3).

The reference resizes and normalises every image on the CPU with PIL (Dataset.py:10-13,37) after its augmentations
(Util.py:566-607).  Here the host only decides the geometry -- the same `random` draws, in the same order, as
`expand` (Util.py:610-645), `random_crop` (:648-729) and `flip` (:732-749), and the same box arithmetic -- and the
images travel as raw 8-bit pixels; one kernel set (csrc/preprocess.hip) then produces the normalised
(B,3,300,300) batch, the resize being bit-identical to PIL's.

`photometric_distort` (Util.py:752-780) is drawn here too (`plan_photometric`: the same shuffle and factors as the
reference, pinned on its own function) and applied by csrc/photometric.hip.  Its arithmetic is torchvision's PIL back end,
i.e. Pillow's ImageEnhance / blend / HSV conversions, reproduced bit for bit against Pillow; torchvision itself is absent,
so its four thin wrappers are restated from their documented behaviour (see oracle/ssd_oracle.py).

Beyond the reference: mosaic augmentation (`MultiImageMultiBBoxDataset(mosaic=...)`, `MosaicImage`).  A training image is composed of
four sources, each with its own plan, resized into the quadrants around a drawn centre; the batch then carries a tile list and the
same kernel set writes every source into its rectangle (`ssd_preprocess_tiles_u8`).  And its usual companion, a random affine warp of
the formed frame (`affine=...`, `plan_affine`, `affine_boxes`): the host draws the matrix and maps the boxes, the batch carries one matrix
per warped image (`RawBatch.warps`), and `.to(device)` warps the normalised frames last (csrc/warp.hip, `ssd_affine_warp_f32`).
"""
from __future__ import annotations

import ctypes as C
import random
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops
from .Util import label_to_class

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
FILLER_U8 = (123, 116, 103)          # the ImageNet mean after to_pil_image's mul(255).byte() (Util.py:593,601)


@dataclass
class GeomPlan:
    """Geometry of one image: source (h, w) placed on a canvas, a crop window of the canvas, a mirror flag."""
    src_h: int
    src_w: int
    canvas: Tuple[int, int, int, int]          # canvas_h, canvas_w, place_top, place_left
    crop: Tuple[int, int, int, int]            # top, left, h, w (of the canvas)
    flip: bool = False
    photo: Tuple[Tuple[int, float], ...] = ()  # (kind, factor) in application order; kind 0 brightness, 1 contrast, 2 saturation, 3 hue

    @property
    def size(self) -> Tuple[int, int]:
        """(width, height) of the image handed to Resize -- what Dataset.py:35 reads as `image.size`"""
        return self.crop[3], self.crop[2]


def identity_plan(h: int, w: int) -> GeomPlan:
    return GeomPlan(h, w, (h, w, 0, 0), (0, 0, h, w), False)


def plan_photometric(rng=random) -> Tuple[Tuple[int, float], ...]:
    """The draws of reference Util.py:752-780: shuffle [brightness, contrast, saturation, hue], then per op a coin and one
    factor (hue: uniform(-18/255, 18/255), the others uniform(0.5, 1.5))."""
    order = [0, 1, 2, 3]
    rng.shuffle(order)
    out = []
    for kind in order:
        if rng.random() < 0.5:
            out.append((kind, rng.uniform(-18 / 255., 18 / 255.) if kind == 3 else rng.uniform(0.5, 1.5)))
    return tuple(out)


def _iou_1xn(crop: torch.Tensor, boxes: torch.Tensor) -> torch.Tensor:
    """reference Util.py:303-317 get_jaccard_tensor11 for one crop box"""
    lo = torch.max(crop[:2].unsqueeze(0), boxes[:, :2])
    hi = torch.min(crop[2:].unsqueeze(0), boxes[:, 2:])
    wh = torch.clamp(hi - lo, min=0)
    inter = wh[:, 0] * wh[:, 1]
    a1 = (crop[2] - crop[0]) * (crop[3] - crop[1])
    a2 = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    return inter / (a1 + a2 - inter)


def plan_transform(width: int, height: int, boxes: torch.Tensor, labels: torch.Tensor, photometric: bool = True,
                   rng=random, expand: bool = True):
    """The draws and box arithmetic of reference Util.py:566-607 `transform` for an image of the given size.
    Returns (GeomPlan, new_boxes, new_labels); boxes are pixel xyxy float32 like the reference's.
    expand=False (mosaic tiles: the mosaic is the zoom-out) leaves out the expand coin and its three draws: the canvas is the source."""
    boxes = boxes.clone().float()
    labels = labels.clone()
    photo = plan_photometric(rng) if photometric else ()
    h, w = height, width
    canvas = (h, w, 0, 0)
    if expand and rng.random() < .5:           # expand, Util.py:610-645
        scale = rng.uniform(1, 4)
        new_h, new_w = int(scale * h), int(scale * w)
        left = rng.randint(0, new_w - w)
        top = rng.randint(0, new_h - h)
        canvas = (new_h, new_w, top, left)
        boxes = boxes + torch.FloatTensor([left, top, left, top]).unsqueeze(0)
    ch, cw = canvas[0], canvas[1]
    crop = (0, 0, ch, cw)
    done = False
    while not done:                            # random_crop, Util.py:648-729
        min_overlap = rng.choice([0., .1, .3, .5, .7, .9, None])
        if min_overlap is None:
            break
        for _ in range(50):
            scale_h = rng.uniform(0.3, 1)
            scale_w = rng.uniform(0.3, 1)
            new_h, new_w = int(scale_h * ch), int(scale_w * cw)
            if not 0.5 < new_h / new_w < 2:
                continue
            left = rng.randint(0, cw - new_w)
            right = left + new_w
            top = rng.randint(0, ch - new_h)
            bottom = top + new_h
            cb = torch.FloatTensor([left, top, right, bottom])
            if _iou_1xn(cb, boxes).max().item() < min_overlap:
                continue
            centers = (boxes[:, :2] + boxes[:, 2:]) / 2.
            inside = (centers[:, 0] > left) * (centers[:, 0] < right) * (centers[:, 1] > top) * (centers[:, 1] < bottom)
            if not inside.any():
                continue
            boxes = boxes[inside, :]
            labels = labels[inside]
            boxes[:, :2] = torch.max(boxes[:, :2], cb[:2])
            boxes[:, :2] -= cb[:2]
            boxes[:, 2:] = torch.min(boxes[:, 2:], cb[2:])
            boxes[:, 2:] -= cb[:2]
            crop = (top, left, new_h, new_w)
            done = True
            break
    flip = False
    if rng.random() < .5:                      # flip, Util.py:732-749
        flip = True
        img_w = crop[3]
        x0 = img_w - boxes[:, 0] - 1
        x2 = img_w - boxes[:, 2] - 1
        boxes = torch.stack((x2, boxes[:, 1], x0, boxes[:, 3]), dim=1)
    return GeomPlan(height, width, canvas, crop, flip, photo), boxes, labels


def map_regions(plan: GeomPlan, boxes: torch.Tensor) -> torch.Tensor:
    """Pixel xyxy boxes that are NOT ground truth (ignore regions: VOC `difficult` objects, COCO crowd regions) carried through a
    drawn plan, with the f32 operations `plan_transform` applies to the ground truth: shift by the canvas placement; intersect with
    the crop window and translate to it (a region is kept by what is left of it, not by its centre: half an unlabelled object in
    the crop is still an unlabelled object); drop what is left with no area; mirror with the reference's flip arithmetic
    (Util.py:732-749).  No random draw: the plan, and so every other item of the sample, is that of the ground truth alone."""
    boxes = torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4).clone()
    ch, cw, top, left = plan.canvas
    boxes = boxes + torch.FloatTensor([left, top, left, top]).unsqueeze(0)
    ct, cl, crop_h, crop_w = plan.crop
    if (ct, cl, crop_h, crop_w) != (0, 0, ch, cw):
        cb = torch.FloatTensor([cl, ct, cl + crop_w, ct + crop_h])
        boxes[:, :2] = torch.max(boxes[:, :2], cb[:2])
        boxes[:, :2] -= cb[:2]
        boxes[:, 2:] = torch.min(boxes[:, 2:], cb[2:])
        boxes[:, 2:] -= cb[:2]
    boxes = boxes[(boxes[:, 2] > boxes[:, 0]) & (boxes[:, 3] > boxes[:, 1])]
    if plan.flip:
        x0 = crop_w - boxes[:, 0] - 1
        x2 = crop_w - boxes[:, 2] - 1
        boxes = torch.stack((x2, boxes[:, 1], x0, boxes[:, 3]), dim=1)
    return boxes


def plan_affine(W: int, H: int, rng=random, degrees: float = 10.0, scale=(0.8, 1.25), shear: float = 2.0, translate: float = 0.1):
    """The six draws of the random affine warp of a W x H frame, in this order: angle = uniform(-degrees, degrees), s = uniform(lo, hi),
    shx and shy = uniform(-shear, shear) (all angles in degrees), tx = uniform(0.5 - translate, 0.5 + translate) * W and ty likewise
    with H.  The forward map, in frame pixels and float64, is

        M = T(tx, ty) . Shear(tan shx, tan shy) . s R(angle) . T(-W/2, -H/2)      R = [[cos, -sin], [sin, cos]], Shear = [[1, kx], [ky, 1]]

    evaluated in closed form with scalar arithmetic (A = Shear . sR, then the translation column), and inverted in closed form too.
    Returns (M, coef): the top two rows of M as six float64 (m00, m01, m02, m10, m11, m12) -- what `affine_boxes` takes -- and the top
    two rows of M^-1 rounded to float32, the six coefficients of `ops.affine_warp` (output pixel centre -> input coordinates)."""
    import math
    lo, hi = scale
    angle = rng.uniform(-degrees, degrees)
    s = rng.uniform(lo, hi)
    shx = rng.uniform(-shear, shear)
    shy = rng.uniform(-shear, shear)
    tx = rng.uniform(0.5 - translate, 0.5 + translate) * W
    ty = rng.uniform(0.5 - translate, 0.5 + translate) * H
    c, sn = math.cos(math.radians(angle)), math.sin(math.radians(angle))
    kx, ky = math.tan(math.radians(shx)), math.tan(math.radians(shy))
    a00, a01 = s * (c + kx * sn), s * (kx * c - sn)
    a10, a11 = s * (ky * c + sn), s * (c - ky * sn)
    m02 = tx - (a00 * (W / 2) + a01 * (H / 2))
    m12 = ty - (a10 * (W / 2) + a11 * (H / 2))
    det = a00 * a11 - a01 * a10
    i00, i01, i10, i11 = a11 / det, -a01 / det, -a10 / det, a00 / det
    inv = (i00, i01, -(i00 * m02 + i01 * m12), i10, i11, -(i10 * m02 + i11 * m12))
    return (a00, a01, m02, a10, a11, m12), tuple(float(np.float32(v)) for v in inv)


def affine_boxes(M, boxes: torch.Tensor, W: int, H: int, min_box: Optional[float] = 2.0, min_visible: float = 0.3):
    """Standardised xyxy boxes of a W x H frame carried through the forward map M (six float64, see `plan_affine`), in float64: to frame
    pixels, the four corners through M, their axis-aligned hull, the hull clipped to [0, W] x [0, H], and standardised again as float32.
    -> (new boxes (n, 4) float32, keep (n,) bool).  A box is kept when its clipped width and height are at least `min_box` pixels and its
    clipped area at least `min_visible` times the area of its unclipped hull -- and never when nothing of it is left.  min_box=None is
    the rule of ignore regions: kept by whatever area is left.  The hull of a rotated box is LOOSER than the object it holds (by up to
    (|sin| + |cos|)^2 in area for a square one): the boxes grow with the angle, which is why the default angle is small."""
    b = torch.as_tensor(boxes).reshape(-1, 4).numpy().astype(np.float64) * np.array([W, H, W, H], np.float64)
    m00, m01, m02, m10, m11, m12 = (float(v) for v in M)
    xs, ys = b[:, [0, 2, 0, 2]], b[:, [1, 1, 3, 3]]                                  # the four corners
    px = (m00 * xs + m01 * ys) + m02
    py = (m10 * xs + m11 * ys) + m12
    hull = np.stack([px.min(1), py.min(1), px.max(1), py.max(1)], 1) if len(b) else np.zeros((0, 4))
    clip = np.clip(hull, 0.0, np.array([W, H, W, H], np.float64))
    cw, ch = clip[:, 2] - clip[:, 0], clip[:, 3] - clip[:, 1]
    keep = (cw > 0) & (ch > 0)
    if min_box is not None:
        full = (hull[:, 2] - hull[:, 0]) * (hull[:, 3] - hull[:, 1])
        keep &= (cw >= min_box) & (ch >= min_box) & (cw * ch >= min_visible * full)
    new = torch.from_numpy((clip / np.array([W, H, W, H], np.float64)).astype(np.float32))
    return new, torch.from_numpy(keep)


def affine_fill(mean=MEAN, std=STD, filler=FILLER_U8) -> Tuple[float, float, float]:
    """The filler as the resize's last pass normalises it, in float32: ((float)filler / 255 - mean) / std per channel -- what a tap of
    `ops.affine_warp` outside the image reads, so a warped frame's border is the colour of an expanded canvas."""
    return tuple(float((np.float32(f) / np.float32(255.0) - np.float32(m)) / np.float32(s)) for f, m, s in zip(filler, mean, std))


def _check_warps(warps: Optional[Sequence], n_images: int) -> Optional[list]:
    """`RawBatch.warps` of what a caller gave: None where no image is warped, else one slot per output image."""
    if warps is None or all(w is None for w in warps):
        return None
    if len(warps) != n_images or any(w is not None and len(w) != 6 for w in warps):
        raise ValueError("RawBatch: one warp slot per output image, six coefficients each")
    return [None if w is None else tuple(float(v) for v in w) for w in warps]


class RawBatch:
    """A batch as it leaves a DataLoader worker: the images' 8-bit pixels packed into ONE CPU uint8 tensor plus each image's
    geometry / photometric plan -- plain host data, picklable, no GPU touched (reference train.py:29,40 runs `collate_fn`
    inside `num_workers=2` forked workers, which must not initialise HIP).  The caller's own `inputs = inputs.to(device)`
    (train_function.py:61) is where the work happens, in the main process: one pinned upload, then the photometric and
    resize / normalise kernels -> the (B,3,H,W) float32 device tensor `cnn(inputs)` expects."""

    def __init__(self, arena: torch.Tensor, offsets: Sequence[int], plans: Sequence[GeomPlan], size: Tuple[int, int] = (300, 300),
                 headers: Optional[Sequence[Optional["JpegHeader"]]] = None, host_offsets: Optional[Sequence[int]] = None,
                 device_bytes: Optional[int] = None, tiles: Optional[Sequence[Tuple[int, int, int, int, int, int]]] = None,
                 warps: Optional[Sequence[Optional[Sequence[float]]]] = None):
        if arena.dtype != torch.uint8 or arena.dim() != 1 or arena.is_cuda:
            raise ValueError("RawBatch: arena must be a 1-D CPU uint8 tensor")
        if len(offsets) != len(plans) or not plans:
            raise ValueError("RawBatch: one offset and one plan per image, at least one image")
        self.arena, self.offsets, self.plans, self.out_hw = arena, list(offsets), list(plans), tuple(size)
        # A batch with a `MosaicImage` in it: offsets / plans / headers are per SOURCE image (four of a mosaic, one of a plain entry) and
        # tiles[k] = (source, out_image, top, left, h, w) is the rectangle of output image `out_image` that source fills, resized to
        # (h, w); a plain entry is one full-frame tile.  None: one source per output image, the whole frame (every batch without a mosaic).
        self.tiles = None if tiles is None else [tuple(int(v) for v in t) for t in tiles]
        self.n_images = len(self.plans) if tiles is None else 1 + max(t[1] for t in self.tiles)
        # Random affine augmentation: warps[i] is the six float32 coefficients of output image i (`plan_affine`'s second item), or None
        # for an image that is not warped.  None: no image of the batch is -- the batch never reaches `ops.affine_warp`.
        self.warps = _check_warps(warps, self.n_images)
        # A batch that holds JPEG streams (pack_batch): headers[i] is the image's JpegHeader, or None for one that came as pixels.
        # `offsets` are then the pixel slots of the DEVICE arena of `device_bytes` bytes; the host arena holds only what exists --
        # the pixels of the host-decoded images, then the entropy-coded data of the others -- at host_offsets[i].
        self.headers = None
        self.decode_status = None                # int32 (B,) on the device after .to() of a batch with streams; 0 = decoded
        if headers is not None and any(h is not None for h in headers):
            if host_offsets is None or device_bytes is None or len(headers) != len(plans) or len(host_offsets) != len(plans):
                raise ValueError("RawBatch: a batch with JPEG streams needs one header slot and one host offset per image")
            self.headers, self.host_offsets, self.device_bytes = list(headers), list(host_offsets), int(device_bytes)

    # what train_function.py reads from `inputs` (`.shape[0]`, `.size(0)`) also works before `.to(device)`
    @property
    def shape(self) -> torch.Size:
        return torch.Size((self.n_images, 3) + self.out_hw)

    def size(self, dim: Optional[int] = None):
        return self.shape if dim is None else self.shape[dim]

    def __len__(self) -> int:
        return self.n_images

    def pin_memory(self) -> "RawBatch":          # DataLoader(pin_memory=True) calls this in its pinning thread (main process)
        if self.headers is None:
            return RawBatch(self.arena.pin_memory(), self.offsets, self.plans, self.out_hw, tiles=self.tiles, warps=self.warps)
        return RawBatch(self.arena.pin_memory(), self.offsets, self.plans, self.out_hw, self.headers, self.host_offsets, self.device_bytes,
                        self.tiles, self.warps)

    def cuda(self, device=None) -> torch.Tensor:
        return self.to(torch.device("cuda", torch.cuda.current_device()) if device is None else device)

    def to(self, device, *args, **kwargs) -> torch.Tensor:
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("RawBatch.to(): the resize / normalise kernels run on the gfx950 GPU only (no CPU fallback); "
                               f"got device {device}")
        x = self._preprocess(device)
        if self.warps is None:
            return x
        mats = np.asarray([(1.0, 0.0, 0.0, 0.0, 1.0, 0.0) if w is None else w for w in self.warps], np.float32)
        with torch.cuda.device(device):              # the random affine warp comes last, on the composed, normalised frame
            return ops.affine_warp(x, mats, affine_fill())

    def _preprocess(self, device) -> torch.Tensor:
        descs = (_lib.ImageDesc * len(self.plans))()
        for d, p, o in zip(descs, self.plans, self.offsets):
            d.src_offset, d.src_h, d.src_w = o, p.src_h, p.src_w
            d.canvas_h, d.canvas_w, d.place_top, d.place_left = p.canvas
            d.crop_top, d.crop_left, d.crop_h, d.crop_w = p.crop
            d.flip = int(p.flip)
        host = self.arena if self.arena.is_pinned() else self.arena.pin_memory()
        with torch.cuda.device(device):
            arena = host.to(device, non_blocking=True) if self.headers is None else self._upload_and_decode(host, device)
            if any(p.photo for p in self.plans):       # photometric_distort comes first (Util.py:586), on the source pixels
                photo = (_lib.PhotoDesc * len(self.plans))()
                for i, p in enumerate(self.plans):
                    if len(p.photo) > 4:
                        raise ValueError("at most four photometric ops per image")
                    photo[i].n_ops = len(p.photo)
                    for k, (kind, factor) in enumerate(p.photo):
                        photo[i].kind[k] = int(kind)
                        photo[i].alpha[k] = float(factor)
                        photo[i].hue_delta[k] = (int(factor * 255) & 0xFF) if kind == 3 else 0
                ops.photometric_u8(arena, descs, photo)
            if self.tiles is None:
                return ops.preprocess_u8(arena, descs, self.out_hw, MEAN, STD, FILLER_U8)
            tiles = (_lib.TileDesc * len(self.tiles))()
            for t, (src, image, top, left, h, w) in zip(tiles, self.tiles):
                t.src = descs[src]
                t.out_image, t.dst_top, t.dst_left, t.dst_h, t.dst_w = image, top, left, h, w
            return ops.preprocess_tiles_u8(arena, tiles, self.n_images, self.out_hw, MEAN, STD, FILLER_U8)

    def _upload_and_decode(self, host: torch.Tensor, device) -> torch.Tensor:
        """The device arena of a batch with JPEG streams: upload what exists, then decode every stream into its pixel slot
        (csrc/jpeg.hip; files without restart markers through the many-lanes entropy decode of csrc/jpeg_split.hip, which
        `ops.jpeg_decode_` chooses by the batch's longest segment).  Enqueues only."""
        arena = torch.empty(self.device_bytes, device=device, dtype=torch.uint8)
        enc = [i for i, h in enumerate(self.headers) if h is not None]
        stream_host = min(self.host_offsets[i] for i in enc)              # streams lie behind the pixels, on both sides
        stream_dev = self.device_bytes - (host.numel() - stream_host)
        arena[stream_dev:].copy_(host[stream_host:], non_blocking=True)
        for i, (h, p) in enumerate(zip(self.headers, self.plans)):
            if h is None:
                n = p.src_h * p.src_w * 3
                arena[self.offsets[i]:self.offsets[i] + n].copy_(host[self.host_offsets[i]:self.host_offsets[i] + n], non_blocking=True)
        jd = (_lib.JpegDesc * len(enc))()
        segs = []
        for d, i in zip(jd, enc):
            h = self.headers[i]
            ops.jpeg_fill_desc(d, h, stream_dev + self.host_offsets[i] - stream_host, self.offsets[i], h.height * h.width * 3, len(segs))
            segs.extend(int(o) - h.data_begin for o in h.seg_offsets)
        status = ops.jpeg_decode_(arena, jd, np.asarray(segs, np.int32))
        if len(enc) == len(self.plans):
            self.decode_status = status
        else:
            self.decode_status = torch.zeros(len(self.plans), device=device, dtype=torch.int32)
            self.decode_status[torch.tensor(enc).to(device, non_blocking=True)] = status
        return arena


def _batch_warps(images: Sequence, warps: Optional[Sequence], size: Tuple[int, int]) -> Optional[list]:
    """The six coefficients per output image of a batch, or None where no entry is warped.  warps[i] -- or, where `warps` is None, the
    entry's own `.warp` -- is (m0 .. m5, H, W): a matrix is in the pixels of the frame it was drawn for, so another batch size is an error."""
    if warps is not None and len(warps) != len(images):
        raise ValueError("one warp slot per image")
    ws = [getattr(im, "warp", None) for im in images] if warps is None else list(warps)
    for i, w in enumerate(ws):
        if w is None:
            continue
        if len(w) != 8:
            raise ValueError(f"image {i}: a warp is six coefficients and the (H, W) frame they were drawn for")
        if (int(w[6]), int(w[7])) != tuple(size):
            raise ValueError(f"image {i}: warp drawn for a {(int(w[6]), int(w[7]))} frame (affine_size) in a batch of size {tuple(size)}")
    return [None if w is None else tuple(w[:6]) for w in ws] if any(w is not None for w in ws) else None


def pack_batch(images: Sequence, plans: Optional[Sequence[GeomPlan]] = None, size: Tuple[int, int] = (300, 300),
               warps: Optional[Sequence] = None) -> RawBatch:
    """images: HWC uint8 RGB arrays / tensors / PIL images of any sizes -> RawBatch (host only; safe in a DataLoader worker).
    An entry may also be an `EncodedImage`, or the `bytes` of an image file: a baseline JPEG `parse_jpeg` accepts stays
    compressed and is decoded on the device by `.to(device)`; any other file is decoded here with PIL.
    An entry may be a `MosaicImage` too (its `out_hw` must be `size`; `plans[i]` is not read: its sources carry theirs): every source
    gets a pixel slot, the batch a tile list (`RawBatch.tiles`), and a plain entry beside it is one full-frame tile.
    warps[i]: the `.warp` of a sample a dataset with `affine` > 0 made (None: not warped), for entries given as bare pixels; left out,
    the entries' own `.warp` are taken.  They travel as `RawBatch.warps`; one drawn for another frame than `size` raises ValueError."""
    warps = _batch_warps(images, warps, size)
    rb = _pack_tiles(images, plans, size) if any(isinstance(im, MosaicImage) for im in images) else _pack_sources(images, plans, size)
    rb.warps = _check_warps(warps, rb.n_images)
    return rb


def _pack_sources(images: Sequence, plans: Optional[Sequence[GeomPlan]], size: Tuple[int, int]) -> RawBatch:
    """`pack_batch` of entries that are one source each: the pixel slots, and the streams of the encoded ones behind them."""
    items = []                                   # per image: pixels (ndarray) or an EncodedImage
    for im in images:
        if isinstance(im, (bytes, bytearray, memoryview)):
            im = EncodedImage.of(bytes(im))
            if isinstance(im, RawImage):
                im = im.pixels
        if isinstance(im, EncodedImage):
            items.append(im)
            continue
        a = im.numpy() if torch.is_tensor(im) else np.asarray(im)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("images must be HWC uint8 RGB")
        items.append(np.ascontiguousarray(a))
    if not items:
        raise ValueError("empty batch")
    hw = [(a.header.height, a.header.width) if isinstance(a, EncodedImage) else a.shape[:2] for a in items]
    plans = [None] * len(items) if plans is None else list(plans)
    if len(plans) != len(items):
        raise ValueError("one plan per image")
    plans = [identity_plan(h, w) if p is None else p for p, (h, w) in zip(plans, hw)]
    for p, (h, w) in zip(plans, hw):
        if (p.src_h, p.src_w) != (h, w):
            raise ValueError("plan does not belong to this image")
    offs, total = [], 0                          # the pixel slots: one per image, encoded or not
    for h, w in hw:
        offs.append(total)
        total += (h * w * 3 + 255) & ~255
    if not any(isinstance(a, EncodedImage) for a in items):
        host = torch.zeros(total, dtype=torch.uint8)
        hv = host.numpy()
        for a, o in zip(items, offs):
            hv[o:o + a.size] = a.reshape(-1)
        return RawBatch(host, offs, plans, size)
    # pixels that exist first, the entropy-coded data of the encoded images behind them; their pixel slots exist on the device only
    host_offs, at = [None] * len(items), 0
    for i, a in enumerate(items):
        if not isinstance(a, EncodedImage):
            host_offs[i] = at
            at += (a.size + 255) & ~255
    for i, a in enumerate(items):
        if isinstance(a, EncodedImage):
            host_offs[i] = at
            at += (a.header.data_end - a.header.data_begin + 15) & ~15
    host = torch.zeros(at, dtype=torch.uint8)
    hv = host.numpy()
    for a, o in zip(items, host_offs):
        if isinstance(a, EncodedImage):
            n = a.header.data_end - a.header.data_begin
            hv[o:o + n] = np.frombuffer(a.data, np.uint8, n, a.header.data_begin)
        else:
            hv[o:o + a.size] = a.reshape(-1)
    stream_bytes = at - min(o for a, o in zip(items, host_offs) if isinstance(a, EncodedImage))
    return RawBatch(host, offs, plans, size, [a.header if isinstance(a, EncodedImage) else None for a in items], host_offs,
                    total + stream_bytes)


TILE_MAX_SCALE = 31                          # csrc/preprocess.hip: at most 63 taps = 2 * ceil(crop / rectangle) + 1, per axis


def _pack_tiles(images: Sequence, plans: Optional[Sequence[Optional[GeomPlan]]], size: Tuple[int, int]) -> RawBatch:
    """`pack_batch` of a batch that holds a `MosaicImage`: the sources of all entries packed as a plain batch, and the tile list."""
    if plans is not None and len(plans) != len(images):
        raise ValueError("one plan per image")
    sources, src_plans, tiles = [], [], []
    for i, im in enumerate(images):
        if isinstance(im, MosaicImage):
            if tuple(im.out_hw) != tuple(size):
                raise ValueError(f"MosaicImage composed for {tuple(im.out_hw)} in a batch of size {tuple(size)}")
            for src, (top, left, h, w) in zip(im.sources, im.rects):
                tiles.append((len(sources), i, top, left, h, w))
                sources.append(src.pixels if isinstance(src, RawImage) else src)
                src_plans.append(src.plan)
        else:
            tiles.append((len(sources), i, 0, 0, size[0], size[1]))
            sources.append(im)
            src_plans.append(None if plans is None else plans[i])
    rb = _pack_sources(sources, src_plans, size)
    for src, i, _, _, h, w in tiles:
        ch, cw = rb.plans[src].crop[2:]
        if ch > TILE_MAX_SCALE * h or cw > TILE_MAX_SCALE * w:
            raise ValueError(f"image {i}: a {ch} x {cw} crop into a {h} x {w} rectangle is beyond the resize's bound of "
                             f"{TILE_MAX_SCALE} source pixels per output pixel (63 taps)")
    if rb.headers is None:
        return RawBatch(rb.arena, rb.offsets, rb.plans, size, tiles=tiles)
    return RawBatch(rb.arena, rb.offsets, rb.plans, size, rb.headers, rb.host_offsets, rb.device_bytes, tiles)


def preprocess_batch(images: Sequence, plans: Optional[Sequence[GeomPlan]] = None, size: Tuple[int, int] = (300, 300),
                     device=None) -> torch.Tensor:
    """images: HWC uint8 RGB arrays / tensors / PIL images of any sizes -> (B,3,H,W) float32 on the GPU
    (Resize + ToTensor + Normalize of Dataset.py:10-13 after the plans' geometry).  One host->device copy."""
    if not torch.cuda.is_available():
        raise RuntimeError("preprocess_batch() runs on the gfx950 HIP kernels only (no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return pack_batch(images, plans, size).to(device)


class MultiImageMultiBBoxDataset(torch.utils.data.Dataset):
    """Reference Dataset.py:7-39 with the same constructor.  `__getitem__` returns the RAW 8-bit image and its
    geometry plan instead of a normalised tensor: `(RawImage, classes, standardized_bbox, index)` -- host work only, as it
    runs in DataLoader workers; `collate_fn` packs a batch's RawImages into a `RawBatch` whose `.to(device)` (the caller's
    own line train_function.py:61, main process) makes the normalised device tensor.
    keep_difficult: False (the reference's default: difficult objects are dropped), True (kept as ground truth), or "ignore":
    dropped from the ground truth as with False -- same draws, same four items -- and returned as a fifth item `ignore_bbox`
    (m, 4), carried through the sample's plan by `map_regions` and standardised like the boxes, for `Losses.ssd(ignore_bboxs=...)`.
    mosaic (pass it and its companions by keyword; `decode` stays the last parameter): the probability that a training sample is a
    `MosaicImage` of four files (see `_mosaic`).  The default 0.0 makes not one extra draw: the samples are exactly those without it.
    affine (keyword too): the probability that a training sample -- plain or mosaic, once it is formed -- is warped by a random affine
    map of the `affine_size` = (H, W) frame: rotation within +-affine_degrees, scale in affine_scale = (lo, hi), shear within
    +-affine_shear degrees per axis, the frame's centre moved to within +-affine_translate of the frame around its middle (see `_affine`,
    `plan_affine`).  The pixels are warped on the device, after the resize (`RawBatch.to`).  The default 0.0 makes no draw at all."""

    def __init__(self, all_images, all_multi_bboxes, all_multi_labels, all_difficulties, all_indices, isTest=False,
                 keep_difficult=False, mosaic: float = 0.0, mosaic_center=(0.25, 0.75), mosaic_min_box: float = 2.0,
                 mosaic_size=(300, 300), affine: float = 0.0, affine_degrees: float = 10.0, affine_scale=(0.8, 1.25),
                 affine_shear: float = 2.0, affine_translate: float = 0.1, affine_min_box: float = 2.0,
                 affine_min_visible: float = 0.3, affine_size=(300, 300), decode="host"):
        if decode not in ("host", "device"):
            raise ValueError("decode must be 'host' (PIL in the worker) or 'device' (baseline JPEG streams decoded on the GPU)")
        self.decode = decode
        self.images_list = all_images
        self.multi_labels_list = all_multi_labels
        self.isTest = isTest
        self.multi_bbox_list = all_multi_bboxes
        self.all_difficulties = [torch.tensor(i) for i in all_difficulties]
        self.keep_difficult = keep_difficult
        self.all_indices = all_indices
        # mosaic (training samples only): with probability `mosaic` a sample is composed of itself and three random partners around a
        # centre drawn in mosaic_center = (lo, hi) fractions of the mosaic_size = (H, W) frame; 0.0 draws nothing and changes nothing
        self.mosaic, self.mosaic_center, self.mosaic_min_box = float(mosaic), tuple(mosaic_center), float(mosaic_min_box)
        self.mosaic_size = tuple(int(v) for v in mosaic_size)
        lo, hi = self.mosaic_center
        if not 0.0 <= self.mosaic <= 1.0:
            raise ValueError("mosaic is a probability")
        if not 0 < lo <= hi < 1:
            raise ValueError("mosaic_center: 0 < lo <= hi < 1")
        if any(int(lo * n) < 1 or int(hi * n) > n - 1 for n in self.mosaic_size):
            raise ValueError("mosaic_center leaves a tile of mosaic_size without a pixel")
        # random affine warp (training samples only): with probability `affine`, after the sample is formed; 0.0 draws nothing
        self.affine, self.affine_degrees, self.affine_shear = float(affine), float(affine_degrees), float(affine_shear)
        self.affine_scale, self.affine_translate = tuple(float(v) for v in affine_scale), float(affine_translate)
        self.affine_min_box, self.affine_min_visible = float(affine_min_box), float(affine_min_visible)
        self.affine_size = tuple(int(v) for v in affine_size)
        if not 0.0 <= self.affine <= 1.0:
            raise ValueError("affine is a probability")
        if len(self.affine_scale) != 2 or not 0 < self.affine_scale[0] <= self.affine_scale[1]:
            raise ValueError("affine_scale: 0 < lo <= hi")
        if not (self.affine_degrees >= 0 and self.affine_translate >= 0 and self.affine_min_box >= 0 and self.affine_min_visible >= 0):
            raise ValueError("affine_degrees, affine_translate, affine_min_box and affine_min_visible are not negative")
        if not 0 <= self.affine_shear < 45:
            raise ValueError("affine_shear: 0 <= degrees < 45 (two shears of 45 degrees make the map singular)")
        if len(self.affine_size) != 2 or min(self.affine_size) < 1:
            raise ValueError("affine_size is the (H, W) of the batch")
        if self.affine > 0 and self.mosaic > 0 and self.affine_size != self.mosaic_size:
            raise ValueError("affine_size and mosaic_size are both the batch's frame: they must be equal")

    def __len__(self):
        return len(self.images_list)

    def _load(self, index):
        """(RawImage or EncodedImage, classes, boxes, ignore boxes or None) of one file, before any draw"""
        from PIL import Image
        if self.decode == "device":               # the file's bytes; anything but a baseline JPEG in scope is decoded here, as below
            with open(self.images_list[index], "rb") as f:
                image = EncodedImage.of(f.read())
        else:
            image = RawImage.of(Image.open(self.images_list[index]).convert("RGB"))
        c = torch.Tensor([label_to_class[i] for i in self.multi_labels_list[index]])
        bboxes = torch.Tensor(self.multi_bbox_list[index])
        ignore = None
        as_ignore = isinstance(self.keep_difficult, str) and self.keep_difficult == "ignore"
        if self.keep_difficult is False or as_ignore:
            keep = self.all_difficulties[index] == 0
            if as_ignore:
                ignore = bboxes[~keep]
            bboxes, c = bboxes[keep], c[keep]
        return image, c, bboxes, ignore

    def __getitem__(self, index):
        sample = self._sample(index)
        if self.isTest is False and self.affine > 0.0 and random.random() < self.affine:
            return self._affine(sample)
        return sample

    def _affine(self, sample):
        """The formed sample -- plain or mosaic -- under a random affine warp.  Six draws (`plan_affine`), always consumed.  The boxes go
        through `affine_boxes`: in the `affine_size` frame, the hull of the four mapped corners (LOOSER than the object once it is
        rotated or sheared), clipped to the frame, kept when at least `affine_min_box` pixels wide and high and at least
        `affine_min_visible` of the hull is still in the frame.  If no box survives the sample comes back as it was: un-warped, its boxes
        untouched, no matrix (`Losses.ssd` needs a box per image).  Otherwise the image carries the matrix as `.warp` = (m0 .. m5, H, W)
        and the pixels are warped on the device by `RawBatch.to`.  Ignore boxes take the same hull and clip; only those left without
        area are dropped."""
        import dataclasses
        H, W = self.affine_size
        M, coef = plan_affine(W, H, random, self.affine_degrees, self.affine_scale, self.affine_shear, self.affine_translate)
        boxes, keep = affine_boxes(M, sample[2], W, H, self.affine_min_box, self.affine_min_visible)
        if not keep.any():
            return sample
        image = dataclasses.replace(sample[0], warp=coef + (float(H), float(W)))
        out = (image, sample[1][keep], boxes[keep], sample[3])
        if len(sample) == 5:
            ignore, left = affine_boxes(M, sample[4], W, H, None)
            out += (ignore[left],)
        return out

    def _sample(self, index):
        from .Util import transform
        if self.isTest is False and self.mosaic > 0.0 and random.random() < self.mosaic:
            return self._mosaic(index)
        image, c, bboxes, ignore = self._load(index)
        if self.isTest is False:
            image, bboxes, c = transform(image, bboxes, c)            # Dataset.py:33
        w, h = image.size                                             # Dataset.py:35
        standardized_bbox = bboxes / torch.FloatTensor([w, h, w, h]).unsqueeze(0)
        if ignore is None:
            return image, c, standardized_bbox, self.all_indices[index]
        ignore_bbox = map_regions(image.plan, ignore) / torch.FloatTensor([w, h, w, h]).unsqueeze(0)
        return image, c, standardized_bbox, self.all_indices[index], ignore_bbox

    def _mosaic(self, index):
        """The sample `index` as a mosaic.  Draws, in this order: three partners, `randrange(len(self))` each; the centre,
        cx = randint(int(lo*W), int(hi*W)) and cy likewise with H; then for the sample itself and the partners -- the tiles top-left,
        top-right, bottom-left, bottom-right -- the plan of `plan_transform(expand=False)`, the photometric draw included.  A tile's
        boxes, in its plan's crop frame, are divided by the crop size, clamped to [0, 1] and carried into their rectangle; of all tiles'
        boxes those at least `mosaic_min_box` output pixels wide and high are kept (the largest one if none is: `Losses.ssd` needs a
        box per image).  Ignore boxes go through `map_regions` and the same mapping; only those without area are dropped."""
        H, W = self.mosaic_size
        lo, hi = self.mosaic_center
        members = [index] + [random.randrange(len(self)) for _ in range(3)]
        cx = random.randint(int(lo * W), int(hi * W))
        cy = random.randint(int(lo * H), int(hi * H))
        rects = ((0, 0, cy, cx), (0, cx, cy, W - cx), (cy, 0, H - cy, cx), (cy, cx, H - cy, W - cx))
        frame = torch.FloatTensor([W, H, W, H])
        sources, boxes, classes, ignores = [], [], [], []
        for i, (top, left, h, w) in zip(members, rects):
            image, c, bboxes, ignore = self._load(i)
            if isinstance(image, EncodedImage):
                plan, bboxes, c = plan_transform(image.header.width, image.header.height, bboxes, c, expand=False)
                sources.append(EncodedImage(image.data, image.header, plan))
            else:
                plan, bboxes, c = plan_transform(image.pixels.shape[1], image.pixels.shape[0], bboxes, c, expand=False)
                sources.append(RawImage(image.pixels, plan))
            cw, ch = plan.size

            def carry(b):
                s = torch.clamp(b / torch.FloatTensor([cw, ch, cw, ch]), 0, 1)
                return (s * torch.FloatTensor([w, h, w, h]) + torch.FloatTensor([left, top, left, top])) / frame
            boxes.append(carry(bboxes)); classes.append(c)
            if ignore is not None:
                ignores.append(carry(map_regions(plan, ignore)))
        boxes, classes = torch.cat(boxes), torch.cat(classes)
        keep = ((boxes[:, 2] - boxes[:, 0]) * W >= self.mosaic_min_box) & ((boxes[:, 3] - boxes[:, 1]) * H >= self.mosaic_min_box)
        if not keep.any():
            keep[torch.argmax((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1]))] = True
        image = MosaicImage(tuple(sources), rects, (H, W))
        if not ignores:
            return image, classes[keep], boxes[keep], self.all_indices[index]
        ignores = torch.cat(ignores)
        ignores = ignores[(ignores[:, 2] > ignores[:, 0]) & (ignores[:, 3] > ignores[:, 1])]
        return image, classes[keep], boxes[keep], self.all_indices[index], ignores


@dataclass
class RawImage:
    """8-bit HWC pixels of one image and the geometry / photometric plan drawn for it; `.size` = (width, height) of the
    augmented image, what the reference reads from its PIL image at Dataset.py:35."""
    pixels: np.ndarray
    plan: GeomPlan
    warp: Optional[Tuple[float, ...]] = None     # random affine warp of the resized frame: (m0 .. m5, H, W), see `_affine`; None: none

    @staticmethod
    def of(image) -> "RawImage":
        if isinstance(image, RawImage):
            return image
        a = np.ascontiguousarray(np.asarray(image.convert("RGB") if hasattr(image, "convert") else image))
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("image must be a PIL image or an HWC uint8 RGB array")
        return RawImage(a, identity_plan(a.shape[0], a.shape[1]))

    @property
    def size(self) -> Tuple[int, int]:
        return self.plan.size


# ---- baseline JPEG: the host parser of the device decoder (csrc/jpeg.hip) -------------------------------------------------------
JPEG_MAX_DIM = 4096
_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                    54, 47, 55, 62, 63])


@dataclass
class JpegHeader:
    """What the device decoder needs of one baseline JPEG file (all offsets are bytes from the start of the file)."""
    width: int
    height: int
    n_components: int                            # 1 (grayscale) or 3 (YCbCr)
    h_samp: int                                  # luma sampling 1x1, 2x1 or 2x2; chroma is 1x1
    v_samp: int
    restart_interval: int                        # MCUs per restart segment, 0 = no restart markers
    quant_tables: dict                           # id -> uint16[64], natural (row-major) order
    huff_tables: dict                            # (class 0 DC / 1 AC, id) -> (bits uint8[16], huffval uint8[n])
    quant_sel: Tuple[int, ...]                   # per component
    dc_sel: Tuple[int, ...]
    ac_sel: Tuple[int, ...]
    data_begin: int                              # entropy-coded data: [data_begin, data_end)
    data_end: int
    seg_offsets: np.ndarray                      # int32: first byte of every restart segment
    seg_first_mcu: np.ndarray                    # int32: the MCU each segment starts at


def parse_jpeg(data: bytes) -> Optional[JpegHeader]:
    """Walk the markers of a JPEG file.  A header for what the device decoder supports -- baseline sequential DCT (SOF0), 8-bit,
    Huffman, ONE interleaved scan, 1 component or 3 components YCbCr with luma sampling 1x1 / 2x1 / 2x2 and chroma 1x1, any DQT /
    DHT, restart intervals, 1 .. 4096 pixels a side -- and None for everything else (progressive, arithmetic, 12-bit, CMYK, RGB,
    other samplings, several scans, DNL, 16-bit quantisation tables, a file that cannot be walked to its EOI): such an image is
    decoded by PIL on the host.  Host work only."""
    a = np.frombuffer(data, np.uint8)
    n = a.size
    if n < 4 or a[0] != 0xFF or a[1] != 0xD8:
        return None
    pos, quant, huff, frame, restart, adobe = 2, {}, {}, None, 0, None
    while True:
        if pos + 2 > n or a[pos] != 0xFF:
            return None
        while pos < n and a[pos] == 0xFF:
            pos += 1
        if pos >= n:
            return None
        m = int(a[pos])
        pos += 1
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9 or pos + 2 > n:
            return None
        ln = (int(a[pos]) << 8) | int(a[pos + 1])
        if ln < 2 or pos + ln > n:
            return None
        seg = a[pos + 2:pos + ln]
        if m == 0xDB:                                                  # DQT
            q = 0
            while q < seg.size:
                if seg[q] >> 4 or (seg[q] & 15) > 3 or q + 65 > seg.size:
                    return None
                nat = np.zeros(64, np.uint16)
                nat[_ZIGZAG] = seg[q + 1:q + 65]
                quant[int(seg[q] & 15)] = nat
                q += 65
        elif m == 0xC4:                                                # DHT
            q = 0
            while q < seg.size:
                if q + 17 > seg.size:
                    return None
                tc, th = int(seg[q] >> 4), int(seg[q] & 15)
                bits = seg[q + 1:q + 17].copy()
                cnt = int(bits.sum())
                if tc > 1 or th > 1 or cnt > 256 or q + 17 + cnt > seg.size:
                    return None
                first = np.concatenate([[0], np.cumsum(bits.astype(np.int64) << (15 - np.arange(16)))[:-1]])      # first code of each length, as 16-bit
                if ((first + (bits.astype(np.int64) << (15 - np.arange(16)))) > 65536).any():
                    return None                                         # no canonical code
                huff[(tc, th)] = (bits, seg[q + 17:q + 17 + cnt].copy())
                q += 17 + cnt
        elif m == 0xC0:                                                # SOF0
            if frame is not None or seg.size < 6:
                return None
            h, w, nc = (int(seg[1]) << 8) | int(seg[2]), (int(seg[3]) << 8) | int(seg[4]), int(seg[5])
            if seg[0] != 8 or nc not in (1, 3) or seg.size != 6 + 3 * nc or not (1 <= h <= JPEG_MAX_DIM and 1 <= w <= JPEG_MAX_DIM):
                return None
            frame = (h, w, [(int(seg[6 + 3 * i]), int(seg[7 + 3 * i] >> 4), int(seg[7 + 3 * i] & 15), int(seg[8 + 3 * i])) for i in range(nc)])
        elif 0xC1 <= m <= 0xCF or m == 0xDC:                           # every other SOF, DAC, DNL
            return None
        elif m == 0xDD:
            if seg.size != 2:
                return None
            restart = (int(seg[0]) << 8) | int(seg[1])
        elif m == 0xEE and seg.size >= 12 and bytes(seg[:5]) == b"Adobe":
            adobe = int(seg[11])
        elif m == 0xDA:
            break
        pos += ln
    if frame is None:
        return None
    h, w, comps = frame
    nc = len(comps)
    if seg.size != 4 + 2 * nc or seg[0] != nc or seg[1 + 2 * nc] != 0 or seg[2 + 2 * nc] != 63 or seg[3 + 2 * nc] != 0:
        return None
    dc_sel, ac_sel = [], []
    for i, c in enumerate(comps):
        td, ta = int(seg[2 + 2 * i] >> 4), int(seg[2 + 2 * i] & 15)
        if seg[1 + 2 * i] != c[0] or (0, td) not in huff or (1, ta) not in huff or c[3] not in quant:
            return None
        dc_sel.append(td); ac_sel.append(ta)
    hs = vs = 1
    if nc == 3:
        hs, vs = comps[0][1], comps[0][2]
        if adobe == 0 or [c[0] for c in comps] == [82, 71, 66]:        # RGB, not YCbCr
            return None
        if (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            return None
    begin = pos + ln
    # the entropy-coded data ends at the first FF that is followed by neither a stuffed 00 nor a restart marker D0..D7
    e = a[begin:]
    at = np.flatnonzero((e[:-1] == 0xFF) & (e[1:] != 0)) if e.size > 1 else np.zeros(0, np.int64)
    other = np.flatnonzero((e[at + 1] & 0xF8) != 0xD0)
    if other.size == 0:
        return None
    end = begin + int(at[other[0]])
    if a[end + 1] != 0xD9:                                             # another scan, DNL, fill bytes: not walked
        return None
    segs = np.concatenate([[begin], begin + at[:other[0]] + 2]).astype(np.int32)
    total = -(-w // (8 * hs)) * -(-h // (8 * vs))
    if restart == 0:
        if segs.size != 1:
            return None
        first = np.zeros(1, np.int32)
    else:
        if segs.size > -(-total // restart):
            return None
        first = (np.arange(segs.size) * restart).astype(np.int32)
    return JpegHeader(w, h, nc, hs, vs, restart, quant, huff, tuple(c[3] for c in comps), tuple(dc_sel), tuple(ac_sel), begin, end, segs, first)


@dataclass
class MosaicImage:
    """A training image composed of four sources (Bochkovskiy et al. 2020, section 3.3): sources[k] -- a `RawImage` or `EncodedImage`
    with the plan drawn for it -- is resized into rects[k] = (top, left, h, w) of an out_hw = (H, W) frame; the four rectangles, in the
    order top-left, top-right, bottom-left, bottom-right, meet at the drawn centre and tile the frame.  `.size` = (W, H)."""
    sources: Tuple
    rects: Tuple[Tuple[int, int, int, int], ...]
    out_hw: Tuple[int, int]
    warp: Optional[Tuple[float, ...]] = None     # random affine warp of the composed frame: (m0 .. m5, H, W); None: none

    @property
    def size(self) -> Tuple[int, int]:
        return self.out_hw[1], self.out_hw[0]


@dataclass
class EncodedImage:
    """A sibling of `RawImage` for `decode="device"`: the bytes of a baseline JPEG file, its parsed header and the geometry /
    photometric plan drawn for it (a plan needs only the header's width and height).  The pixels first exist on the GPU."""
    data: bytes
    header: JpegHeader
    plan: GeomPlan
    warp: Optional[Tuple[float, ...]] = None     # as `RawImage.warp`

    @staticmethod
    def of(data: bytes):
        """-> EncodedImage, or a RawImage decoded by PIL where `parse_jpeg` does not accept the file"""
        header = parse_jpeg(data)
        if header is None:
            import io
            from PIL import Image
            return RawImage.of(Image.open(io.BytesIO(data)).convert("RGB"))
        return EncodedImage(data, header, identity_plan(header.height, header.width))

    @property
    def size(self) -> Tuple[int, int]:
        return self.plan.size


def collate_fn(batch):
    """Reference Dataset.py:41-53: (images, classes, boxes, indices) of a list of samples.  Host work only (it runs in the
    DataLoader's workers): RawImage entries are packed into one `RawBatch`; already-normalised tensors are stacked like the
    reference does.  Samples of `keep_difficult="ignore"` carry a fifth item: their ignore boxes come back as a fifth list.
    `MosaicImage` entries (a dataset with `mosaic` > 0) may stand beside plain ones: the batch then carries a tile list.
    The entries' `.warp` (a dataset with `affine` > 0) travel as `RawBatch.warps`."""
    images, classes, boxes, indices = [], [], [], []
    for b in batch:
        images.append(b[0]); classes.append(b[1]); boxes.append(b[2]); indices.append(b[3])
    ignore = [b[4] for b in batch] if batch and len(batch[0]) == 5 else None
    if images and isinstance(images[0], (RawImage, EncodedImage, MosaicImage)):
        x = pack_batch([r.pixels if isinstance(r, RawImage) else r for r in images],
                       [None if isinstance(r, MosaicImage) else r.plan for r in images], warps=[r.warp for r in images])
    else:
        x = torch.stack(images, dim=0)
    if ignore is not None:
        return x, classes, boxes, indices, ignore
    return x, classes, boxes, indices

"""Host-side mirror of the box utilities the hot path imports from the
reference's Util.py (names and argument meaning kept; bodies are ours).

What `Losses.py` / `train_function.py` pull in through `from Util import *` and what
`train.py:6` / `Dataset.py:4` import by name lives here: prior boxes, box coders, the
class table, `device`, the (empty) VOC lists, `transform` (as a geometry plan: the
pixels are made on the GPU) and `get_map`; `DetectionEvaluator` / `evaluate_detections` are build additions
beside it (VOC difficult objects, IoU sweeps, all-point AP), as are `CocoEvaluator` / `evaluate_coco` (COCO's
protocol: crowd regions, area ranges, maxDets, AP and AR).  VOC XML parsing and drawing are out of
scope.
"""
from __future__ import annotations

from math import sqrt

import torch

use_cuda = torch.cuda.is_available()
device = torch.device("cuda" if use_cuda else "cpu")

# reference Util.py:26-27 -- background is the last entry
class_to_label = ['aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow',
                  'diningtable', 'dog', 'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train',
                  'tvmonitor', 'bg']
label_to_class = {name: i for i, name in enumerate(class_to_label)}

# The VOC lists reference Util.py:16 re-exports from DataLists.py (train.py:6 imports all four): filled by callers that have a
# dataset; empty here (the VOC XML walk is host I/O outside the path -- SURVEY.md section 2 row 13)
all_images = {"train": [], "test": []}
all_multi_bboxes = {"train": [], "test": []}
all_multi_labels = {"train": [], "test": []}
all_difficulties = {"train": [], "test": []}

_GRID = (38, 19, 10, 5, 3, 1)
_SCALE = (0.1, 0.2, 0.375, 0.55, 0.725, 0.9)
_RATIO = ((1., 2., .5), (1., 2., 3., .5, .333), (1., 2., 3., .5, .333), (1., 2., 3., .5, .333), (1., 2., .5), (1., 2., .5))
ANCHORS_PER_CELL = (4, 6, 6, 6, 4, 4)


def create_priors_ssd300() -> torch.Tensor:
    """(8732,4) f32 cx,cy,w,h  (reference Util.py:105-137): per grid cell, row-major,
    boxes (s*sqrt(a), s/sqrt(a)) for each ratio with the sqrt(s_k*s_k+1) square right
    after a == 1; double arithmetic, rounded to f32, clamped to [0,1]."""
    out = []
    for k, g in enumerate(_GRID):
        s = _SCALE[k]
        extra = sqrt(s * _SCALE[k + 1]) if k + 1 < len(_SCALE) else 1.
        for row in range(g):
            cy = (row + 0.5) / float(g)
            for col in range(g):
                cx = (col + 0.5) / float(g)
                for a in _RATIO[k]:
                    out.append([cx, cy, s * sqrt(a), s / sqrt(a)])
                    if a == 1.:
                        out.append([cx, cy, extra, extra])
    return torch.tensor(out, dtype=torch.float64).to(torch.float32).clamp_(0, 1)


# SSD512 is NOT in the reference: build-defined extension in the reference's
# style -- seven maps 64..1, the standard SSD512 scales, the reference's per-cell ratio lists and rounding.
_GRID512 = (64, 32, 16, 8, 4, 2, 1)
_SCALE512 = (0.07, 0.15, 0.30, 0.45, 0.60, 0.75, 0.90)
_RATIO512 = ((1., 2., .5),) + ((1., 2., 3., .5, .333),) * 4 + ((1., 2., .5),) * 2
ANCHORS_PER_CELL_512 = (4, 6, 6, 6, 6, 4, 4)


def create_priors_ssd512() -> torch.Tensor:
    """(24564,4) f32 cx,cy,w,h: create_priors_ssd300's construction on the SSD512 grids (build-defined)."""
    out = []
    for k, g in enumerate(_GRID512):
        s = _SCALE512[k]
        extra = sqrt(s * _SCALE512[k + 1]) if k + 1 < len(_SCALE512) else 1.
        for row in range(g):
            cy = (row + 0.5) / float(g)
            for col in range(g):
                cx = (col + 0.5) / float(g)
                for a in _RATIO512[k]:
                    out.append([cx, cy, s * sqrt(a), s / sqrt(a)])
                    if a == 1.:
                        out.append([cx, cy, extra, extra])
    return torch.tensor(out, dtype=torch.float64).to(torch.float32).clamp_(0, 1)


def prior_levels(n_priors: int):
    """(cells, anchors) of the prior set with `n_priors` priors, per pyramid level: grid cells and priors per cell, in storage order
    (level after level, cell after cell, the priors of a cell contiguous) -- what `ops.multibox_loss(match="atss")` needs.
    8732: create_priors_ssd300, 24564: create_priors_ssd512; ValueError for any other count."""
    for grid, anchors in ((_GRID, ANCHORS_PER_CELL), (_GRID512, ANCHORS_PER_CELL_512)):
        if sum(g * g * a for g, a in zip(grid, anchors)) == n_priors:
            return tuple(g * g for g in grid), tuple(anchors)
    raise ValueError(f"prior_levels: no built-in prior set has {n_priors!r} priors (8732: SSD300, 24564: SSD512)")


def xywh_to_xyxy(box: torch.Tensor) -> torch.Tensor:
    """reference Util.py:93-96"""
    return torch.cat((box[:, :2] - box[:, 2:] / 2., box[:, :2] + box[:, 2:] / 2.), dim=1)


def xyxy_to_xywh(box: torch.Tensor) -> torch.Tensor:
    """reference Util.py:57-63 (without its host round trip)"""
    return torch.stack(((box[:, 2] + box[:, 0]) / 2., (box[:, 3] + box[:, 1]) / 2.,
                        box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]), dim=1)


def gcxgcy_to_cxcy(gcxgcy: torch.Tensor, priors_cxcy: torch.Tensor) -> torch.Tensor:
    """reference Util.py:86-91"""
    priors_cxcy = priors_cxcy.to(gcxgcy.device)
    return torch.cat([gcxgcy[:, :2] * priors_cxcy[:, 2:] / 10 + priors_cxcy[:, :2],
                      torch.exp(gcxgcy[:, 2:] / 5) * priors_cxcy[:, 2:]], 1)


def get_offsets_coords(cxcy: torch.Tensor, priors_cxcy: torch.Tensor) -> torch.Tensor:
    """reference Util.py:98-102"""
    priors_cxcy = priors_cxcy.to(cxcy.device)
    return torch.cat([(cxcy[:, :2] - priors_cxcy[:, :2]) / (priors_cxcy[:, 2:] / 10),
                      torch.log(cxcy[:, 2:] / priors_cxcy[:, 2:]) * 5], 1)


def subsampling(x: torch.Tensor, step) -> torch.Tensor:
    """keep every step[d]-th entry along dim d (None = keep all); reference Util.py:555-560"""
    for d, s in enumerate(step):
        if s is not None:
            x = x.index_select(d, torch.arange(0, x.shape[d], s, device=x.device))
    return x


def transform(image, boxes, labels):
    """Reference Util.py:566-607 (`from Util import transform`, Dataset.py:4): photometric distortion, expand, random crop,
    flip, with the reference's `random` draws in its order and its box arithmetic -- as a PLAN.  `image` is a PIL image, an HWC
    uint8 array or a `Dataset.RawImage`; the returned image is a `Dataset.RawImage` (source pixels + plan, `.size` = the
    augmented (width, height)): the pixels are produced later, on the GPU, by `Dataset.RawBatch.to(device)`."""
    from .Dataset import EncodedImage, RawImage, plan_transform
    if isinstance(image, EncodedImage):          # decode="device": the plan needs only the header's size
        plan, new_boxes, new_labels = plan_transform(image.header.width, image.header.height, boxes, labels)
        return EncodedImage(image.data, image.header, plan), new_boxes, new_labels
    raw = RawImage.of(image)
    h, w = raw.pixels.shape[:2]
    plan, new_boxes, new_labels = plan_transform(w, h, boxes, labels)
    return RawImage(raw.pixels, plan), new_boxes, new_labels


def create_ancs_xywh_zoom_ratio() -> torch.Tensor:
    """(189,4) f32 anchors of the SSD_resnet34 variant (reference Util.py:142-164): grids 4/2/1, nine zoom x ratio
    shapes per cell, centres at linspace(1/(2g), 1-1/(2g), g); the first returned coordinate varies fastest."""
    import numpy as np
    shapes = [(z * i, z * j) for z in (0.75, 1., 1.3) for (i, j) in ((1., 1.), (1., 0.5), (0.5, 1.))]
    rows = []
    for g in (4, 2, 1):
        ctr = np.linspace(1 / (g * 2), 1 - 1 / (g * 2), g)
        rows += [[fast, slow, o / g, p / g] for slow in ctr for fast in ctr for o, p in shapes]
    return torch.tensor(np.asarray(rows, np.float64), dtype=torch.float32)


def get_map(det_boxes, det_classes, det_scores, gt_boxes, gt_classes, n_classes=20):
    """Per-class 11-point interpolated AP (reference Util.py:783-885; same arguments: per-image lists of (n,4) boxes,
    (n,) classes, (n,) scores and the ground-truth boxes / classes).  Matching, the per-class sort and the
    precision/recall scan run on the GPU (csrc/map_eval.hip); returns {class: numpy.float64 AP} like the reference
    (which also prints each value).  Score ties are ordered lower flat index first.  `n_classes`: the foreground classes
    (1..256), the keys of the result are range(n_classes)."""
    import numpy as np
    from . import ops
    if not torch.cuda.is_available():
        raise RuntimeError("get_map() runs on the gfx950 HIP kernels only (no CPU fallback)")
    import numbers
    if isinstance(n_classes, bool) or not isinstance(n_classes, numbers.Integral) or not 1 <= n_classes <= 256:
        raise ValueError(f"n_classes must be an integer in 1..256, got {n_classes!r}")
    n_img = len(det_boxes)
    if not (n_img == len(det_classes) == len(det_scores) == len(gt_boxes) == len(gt_classes)) or n_img == 0:
        raise ValueError("get_map expects five lists with one entry per image")
    dev = next((t.device for t in list(det_boxes) + list(gt_boxes) if torch.is_tensor(t) and t.is_cuda), device)

    db, per_det = _cat(det_boxes, torch.float32, 4, dev)
    dc, _ = _cat(det_classes, torch.int32, 0, dev)
    ds, _ = _cat(det_scores, torch.float32, 0, dev)
    gb, per_gt = _cat(gt_boxes, torch.float32, 4, dev)
    gc, _ = _cat(gt_classes, torch.int32, 0, dev)
    d_start, g_start = _starts(per_det, dev), _starts(per_gt, dev)
    levels = torch.arange(0, 1.1, 0.1).double().numpy()                # Util.py:874, float32 levels compared in float64
    table, _, _ = ops.map_eval(db, dc, ds, d_start, gb, gc, g_start, levels, int(n_classes))
    t = table.cpu().numpy()
    return {cls: np.float64(np.mean(t[cls])) for cls in range(int(n_classes))}


# ---- detection evaluator: VOC 'difficult' objects, IoU-threshold sweep, 11- / 101- / all-point AP (not in the reference) ----------
COCO_IOU_THRESHOLDS = tuple(0.5 + 0.05 * k for k in range(10))
_INTERPOLATION_LEVELS = {"11point": 10, "101point": 100, "all": 0}


def _check_eval_args(n_classes, iou_thresholds, interpolation):
    import numbers
    import numpy as np
    if isinstance(n_classes, bool) or not isinstance(n_classes, numbers.Integral) or not 1 <= n_classes <= 256:
        raise ValueError(f"n_classes must be an integer in 1..256, got {n_classes!r}")
    try:
        thr = [float(t) for t in iou_thresholds]
    except TypeError:
        raise ValueError(f"iou_thresholds must be a sequence of 1..16 floats, got {iou_thresholds!r}") from None
    if not 1 <= len(thr) <= 16:
        raise ValueError(f"iou_thresholds must hold 1..16 values, got {len(thr)}")
    thr32 = np.asarray(thr, np.float32)                                  # converted once; the kernels compare iou > float32(thr)
    if not all(0.0 < float(t) < 1.0 for t in thr32):
        raise ValueError(f"iou_thresholds must lie in (0, 1), got {iou_thresholds!r}")
    if any(not thr32[i] < thr32[i + 1] for i in range(len(thr) - 1)):
        raise ValueError(f"iou_thresholds must be ascending and distinct, got {iou_thresholds!r}")
    if interpolation not in _INTERPOLATION_LEVELS:
        raise ValueError(f"interpolation must be '11point', '101point' or 'all', got {interpolation!r}")
    return int(n_classes), thr32


def _starts(counts, dev):
    start = [0]
    for n in counts:
        start.append(start[-1] + int(n))
    return torch.tensor(start, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)


def _cat(items, dtype, width, dev):
    parts = [torch.as_tensor(t).reshape((-1, width) if width else (-1,)).to(device=dev, dtype=dtype) for t in items]
    if not parts:
        return torch.zeros((0, width) if width else (0,), device=dev, dtype=dtype), []
    return torch.cat(parts).contiguous(), [int(p.shape[0]) for p in parts]


def _eval_batch_inputs(boxes, classes, scores, count, gt_boxes, gt_classes, gt_extras, gt_offsets, acc_dev):
    """The input layouts of `DetectionEvaluator.add_batch` / `CocoEvaluator.add_batch` as the kernels take them.  gt_extras: a list
    of (values or None, dtype, name), the optional per-object arrays.  -> (boxes, classes, scores, det_start or None, det_count or
    None, gt_boxes, gt_classes, [extras], gt_start, device).  Nothing here waits for the device when the detections are padded
    device tensors and the ground truth is packed."""
    dev = torch.device("cuda", torch.cuda.current_device())
    if count is not None:
        if not (torch.is_tensor(boxes) and boxes.is_cuda and boxes.dim() == 3 and boxes.shape[-1] == 4):
            raise ValueError("add_batch: with `count`, boxes must be a (B,K,4) device tensor")
        dev = boxes.device
        n_img = int(boxes.shape[0])
        db = boxes.detach().to(torch.float32).contiguous()
        dc = classes.detach().to(device=dev, dtype=torch.int32).contiguous()
        ds = scores.detach().to(device=dev, dtype=torch.float32).contiguous()
        d_count = count.detach().to(device=dev, dtype=torch.int32).contiguous()
        d_start = None
    else:
        if not (len(boxes) == len(classes) == len(scores)):
            raise ValueError("add_batch expects one entry per image in boxes, classes and scores")
        n_img = len(boxes)
        dev = next((t.device for t in list(boxes) + (list(gt_boxes) if gt_offsets is None else [gt_boxes])
                    if torch.is_tensor(t) and t.is_cuda), dev)
        db, per = _cat(boxes, torch.float32, 4, dev)
        dc, per_c = _cat(classes, torch.int32, 0, dev)
        ds, per_s = _cat(scores, torch.float32, 0, dev)
        if per != per_c or per != per_s:
            raise ValueError("add_batch: boxes, classes and scores disagree on the detections per image")
        d_start, d_count = _starts(per, dev), None
    if n_img == 0:
        raise ValueError("add_batch expects at least one image")
    if acc_dev is not None and dev != acc_dev:
        raise ValueError(f"add_batch: this evaluator accumulates on {acc_dev}, the batch is on {dev}")
    extras = []
    if gt_offsets is not None:
        if not (torch.is_tensor(gt_boxes) and gt_boxes.is_cuda and torch.is_tensor(gt_offsets) and gt_offsets.is_cuda):
            raise ValueError("add_batch: packed ground truth (gt_offsets given) must be device tensors")
        gb = gt_boxes.detach().reshape(-1, 4).to(torch.float32).contiguous()
        gc = gt_classes.detach().reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
        for values, dtype, _ in gt_extras:
            extras.append(None if values is None else values.detach().reshape(-1).to(device=dev, dtype=dtype).contiguous())
        g_start = gt_offsets.detach().to(torch.int32).contiguous()
        if g_start.numel() != n_img + 1:
            raise ValueError("add_batch: gt_offsets must have one entry per image plus one")
    else:
        if len(gt_boxes) != n_img or len(gt_classes) != n_img or any(v is not None and len(v) != n_img for v, _, _ in gt_extras):
            raise ValueError("add_batch expects one ground-truth entry per image")
        gb, per = _cat(gt_boxes, torch.float32, 4, dev)
        gc, per_c = _cat(gt_classes, torch.int32, 0, dev)
        for values, dtype, name in gt_extras:
            if values is None:
                extras.append(None)
                continue
            ge, per_e = _cat(values, dtype, 0, dev)
            if per_e != per:
                raise ValueError(f"add_batch: gt_boxes and {name} disagree on the objects per image")
            extras.append(ge)
        if per != per_c:
            raise ValueError("add_batch: gt_boxes and gt_classes disagree on the objects per image")
        g_start = _starts(per, dev)
    return db, dc, ds, d_start, d_count, gb, gc, extras, g_start, dev


class _BatchRecords:
    """What the two evaluators keep between `add_batch` and `compute`: per batch the record class, score and protocol fields of every
    detection row (`_FIELDS`, device tensors, one list per field), and the objects per class `_n_gt`, made on the first batch's
    device."""
    _FIELDS = ()

    def reset(self):
        """Forget every batch added so far."""
        for name in ("rec", "score") + self._FIELDS:
            setattr(self, "_" + name, [])
        self._n_gt = None
        self._padded = False
        self._dev = None

    def _n_gt_on(self, dev, shape):
        if self._n_gt is None:
            self._n_gt = torch.zeros(shape, device=dev, dtype=torch.int32)
            self._dev = dev
        return self._n_gt

    def _keep(self, padded, scores, rec, *fields):
        self._padded = self._padded or padded
        self._rec.append(rec)
        self._score.append(scores.reshape(-1).clone() if padded else scores)        # the caller may reuse its padded buffers
        for name, value in zip(self._FIELDS, fields):
            getattr(self, "_" + name).append(value)

    def _records(self):
        """-> [rec, score, *fields] over all batches in the order added, without the rows past count[b] of the padded batches."""
        if self._n_gt is None:
            raise RuntimeError(f"{type(self).__name__}.compute(): no batch has been added")
        with torch.cuda.device(self._dev):
            cols = [torch.cat(getattr(self, "_" + name)) for name in ("rec", "score") + self._FIELDS]
            if self._padded:
                keep = cols[0] != -2
                cols = [c[keep].contiguous() for c in cols]
        return cols


class DetectionEvaluator(_BatchRecords):
    """Average precision under the PASCAL VOC devkit's matching rule, on the GPU (csrc/map_eval.hip, the VOC rule), with what `get_map`
    lacks: 'difficult' objects, up to 16 IoU thresholds settled in one matching pass, 11-point, 101-point or all-point
    (VOC2010+) interpolation, and batch-wise accumulation without host synchronisation.

        ev = DetectionEvaluator(n_classes=20, iou_thresholds=(0.5,), interpolation="11point")
        ev.add_batch(boxes, classes, scores, count, gt_boxes, gt_classes, gt_difficult)      # per batch: enqueues only
        res = ev.compute()                                                                   # the only call that synchronises

    Protocol.  Per class and image the detections are visited in descending score order (ties: the one added first).  The best-IoU
    box among ALL ground-truth boxes of the class in the image, difficult ones included (first on ties; a NaN IoU among them makes
    the detection a false positive), does not depend on the threshold.  At threshold t: not `iou > t` -> false positive; the box
    is difficult -> ignored (neither true nor false positive, the box is never claimed); the box is unclaimed at t -> true positive
    and claimed at t; else false positive.  n_gt counts the non-difficult boxes.  Per class and threshold the detections of all
    images in descending (score, added first) order with the ignored ones removed give precision = cumTP / (cumTP + cumFP) in
    float64; recall is never formed in floating point: level k of L is reached iff cumTP * L >= k * n_gt in integers.  "11point" /
    "101point": AP = mean over k = 0..L of the maximum precision at the positions reaching level k (0 if none).  "all": AP = (sum
    over the true positives of the running maximum of precision from the end of the list) / n_gt, the area under the monotone
    precision-recall envelope.  A class without non-difficult ground truth has AP NaN and is left out of the mean.
    Example: one class, two objects, three detections scored TP, FP, TP -> precisions 1, 1/2, 2/3 -> "all" 0.8333333333333333,
    "11point" 0.8484848484848484, "101point" 0.8349834983498351; with the middle detection ignored, 1.0.

    With no difficult flags and thresholds (0.5,), bit 0 of `tp` and `n_gt` equal `get_map`'s true-positive flags and counts.  The AP
    values deliberately do NOT equal `get_map`'s, which keeps the reference's float32-reciprocal recall and scores a class without
    ground truth 0.

    Detection and ground-truth boxes must be in the SAME coordinate system; nothing is rescaled here.  `Losses.inference_batch_padded`
    emits pixel xyxy of the sizes it is given, the dataset yields fractions of the image: scale one of them, or decode with sizes (1, 1).

    Out of scope: precision-recall curve export, per-image reports.  A sweep here is "AP averaged over IoU thresholds under the VOC
    matching rule", not COCO mAP: COCO's own protocol (best still-unmatched object, crowd regions, area ranges, maxDets, AR) is
    `CocoEvaluator`.
    GPU only, like `get_map`: there is no CPU fallback."""

    _FIELDS = ("tp", "ign")

    def __init__(self, n_classes=20, iou_thresholds=(0.5,), interpolation="11point"):
        self.n_classes, self._thr32 = _check_eval_args(n_classes, iou_thresholds, interpolation)
        if not torch.cuda.is_available():
            raise RuntimeError("DetectionEvaluator runs on the gfx950 HIP kernels only (no CPU fallback)")
        self.iou_thresholds = tuple(float(t) for t in iou_thresholds)
        self.interpolation = interpolation
        self.reset()

    def add_batch(self, boxes, classes, scores, count, gt_boxes, gt_classes, gt_difficult=None, gt_offsets=None):
        """Score one batch of images against its ground truth and keep the per-detection records.

        Detections: the padded device tensors of `Losses.inference_batch_padded` -- boxes (B,K,4), classes (B,K) integer, scores
        (B,K), count (B,) int32; rows >= count[b] are not detections and are never read -- or, with count=None, per-image lists of
        (n,4) boxes, (n,) classes, (n,) scores as `get_map` takes them.  Ground truth: per-image lists of (n,4) boxes, (n,) classes
        and optionally (n,) 0/1 difficult flags, or packed device tensors (G,4), (G,), (G,) with gt_offsets = (B+1,) int32 device
        tensor of each image's first row.  Same coordinate system on both sides (see the class docstring).
        With padded device detections and packed device ground truth nothing here waits for the device."""
        from . import ops
        db, dc, ds, d_start, d_count, gb, gc, (gd,), g_start, dev = _eval_batch_inputs(
            boxes, classes, scores, count, gt_boxes, gt_classes, [(gt_difficult, torch.uint8, "gt_difficult")], gt_offsets, self._dev)
        with torch.cuda.device(dev):
            n_gt = self._n_gt_on(dev, self.n_classes)
            rec, tp, ign = ops.eval_match(db, dc, ds, d_start, d_count, gb, gc, gd, g_start, n_gt, self._thr32, self.n_classes)
        self._keep(count is not None, ds, rec, tp, ign)

    def compute(self):
        """-> dict: `ap` float64 (T, n_classes), NaN where a class has no non-difficult ground truth; `mean_ap` float64 (T,), nanmean
        over the classes; `mean_ap_over_thresholds`; `n_gt`, `n_det` int64 (n_classes,); `tp`, `ignored` device uint16 (D,), bit t =
        true positive / ignored at iou_thresholds[t], in the order the detections were added; `iou_thresholds`; `interpolation`.
        May be called repeatedly; more batches may be added afterwards."""
        import numpy as np
        from . import ops
        T, C, L = len(self._thr32), self.n_classes, _INTERPOLATION_LEVELS[self.interpolation]
        rec, score, tp, ign = self._records()
        with torch.cuda.device(self._dev):
            out, n_det = ops.eval_ap(rec, score, tp, ign, self._n_gt, T, L, C)
            out = out.cpu().numpy()
            n_gt = self._n_gt.cpu().numpy().astype(np.int64)
            n_det = n_det.cpu().numpy().astype(np.int64)
        ap = np.full((T, C), np.nan, np.float64)
        for t in range(T):
            for c in range(C):
                if n_gt[c] > 0:
                    ap[t, c] = np.mean(out[t, c]) if L else out[t, c]
        mean_ap = np.asarray([np.nanmean(ap[t]) if (n_gt > 0).any() else np.nan for t in range(T)], np.float64)
        return {"ap": ap, "mean_ap": mean_ap, "mean_ap_over_thresholds": np.float64(np.mean(mean_ap)), "n_gt": n_gt, "n_det": n_det,
                "tp": tp.view(torch.uint16), "ignored": ign.view(torch.uint16), "iou_thresholds": self.iou_thresholds,
                "interpolation": self.interpolation}


def evaluate_detections(det_boxes, det_classes, det_scores, gt_boxes, gt_classes, gt_difficulties=None, n_classes=20,
                        iou_thresholds=(0.5,), interpolation="11point"):
    """One-shot `DetectionEvaluator` over `get_map`'s per-image lists (plus optional per-image 0/1 difficult flags): the dict of
    `DetectionEvaluator.compute()`.  See the class for the protocol and for how its AP differs from `get_map`'s on purpose."""
    _check_eval_args(n_classes, iou_thresholds, interpolation)
    if not torch.cuda.is_available():
        raise RuntimeError("evaluate_detections() runs on the gfx950 HIP kernels only (no CPU fallback)")
    ev = DetectionEvaluator(n_classes, iou_thresholds, interpolation)
    ev.add_batch(det_boxes, det_classes, det_scores, None, gt_boxes, gt_classes, gt_difficulties)
    return ev.compute()


# ---- COCO evaluator: crowd regions, area ranges, maxDets, AP and AR (pycocotools' box protocol; not in the reference) ------------
COCO_AREA_RANGES = (("all", 0, 1e10), ("small", 0, 1024), ("medium", 1024, 9216), ("large", 9216, 1e10))
COCO_MAX_DETS = (1, 10, 100)


def _check_coco_args(n_classes, iou_thresholds, area_ranges, max_dets):
    import numbers
    import numpy as np
    n_classes, thr32 = _check_eval_args(n_classes, iou_thresholds, "101point")
    try:
        ranges = [(str(name), float(lo), float(hi)) for name, lo, hi in area_ranges]
    except (TypeError, ValueError):
        raise ValueError(f"area_ranges must be a sequence of 1..4 (name, lo, hi), got {area_ranges!r}") from None
    if not 1 <= len(ranges) <= 4:
        raise ValueError(f"area_ranges must hold 1..4 ranges, got {len(ranges)}")
    if len({name for name, _, _ in ranges}) != len(ranges):
        raise ValueError(f"area_ranges must have distinct names, got {area_ranges!r}")
    lo32 = np.asarray([lo for _, lo, _ in ranges], np.float32)           # converted once; the kernels compare against float32 bounds
    hi32 = np.asarray([hi for _, _, hi in ranges], np.float32)
    if not all(lo <= hi for lo, hi in zip(lo32, hi32)):                     # a NaN bound fails here too
        raise ValueError(f"area_ranges need lo <= hi, got {area_ranges!r}")
    try:
        md = list(max_dets)
    except TypeError:
        raise ValueError(f"max_dets must be a sequence of 1..4 integers, got {max_dets!r}") from None
    if not 1 <= len(md) <= 4:
        raise ValueError(f"max_dets must hold 1..4 values, got {len(md)}")
    if any(isinstance(m, bool) or not isinstance(m, numbers.Integral) or not 1 <= m <= 65535 for m in md):
        raise ValueError(f"max_dets must be integers in 1..65535, got {max_dets!r}")
    if any(not md[i] < md[i + 1] for i in range(len(md) - 1)):
        raise ValueError(f"max_dets must be ascending and distinct, got {max_dets!r}")
    return n_classes, thr32, tuple(ranges), lo32, hi32, tuple(int(m) for m in md)


def _nanmean(a):
    import numpy as np
    a = np.asarray(a, np.float64)
    return np.float64(np.nanmean(a)) if a.size and not np.isnan(a).all() else np.float64(np.nan)


def coco_stats(ap, recall, iou_thresholds32, area_names, max_dets):
    """COCO's summary numbers from `ap` (T, A, C) and `recall` (T, A, M, C): the first area range and the last maxDets value play
    COCO's "all" and 100 (see `CocoEvaluator`).  -> dict in COCO's order."""
    import numpy as np
    thr = np.asarray(iou_thresholds32, np.float32)
    stats = {"AP": _nanmean(ap[:, 0, :])}
    for name, v in (("AP50", 0.5), ("AP75", 0.75)):
        at = np.nonzero(thr == np.float32(v))[0]
        stats[name] = _nanmean(ap[at[0], 0, :]) if at.size else np.float64(np.nan)
    for a in range(1, len(area_names)):
        stats[f"AP_{area_names[a]}"] = _nanmean(ap[:, a, :])
    for m, v in enumerate(max_dets):
        stats[f"AR_{v}"] = _nanmean(recall[:, 0, m, :])
    for a in range(1, len(area_names)):
        stats[f"AR_{area_names[a]}"] = _nanmean(recall[:, a, -1, :])
    return stats


class CocoEvaluator(_BatchRecords):
    """COCO detection metrics for boxes -- pycocotools' `COCOeval` protocol: crowd regions, area ranges, maxDets, AP and AR -- on the
    GPU (csrc/map_eval.hip, the COCO rule), accumulated batch-wise without host synchronisation.

        ev = CocoEvaluator(n_classes=80, iou_thresholds=COCO_IOU_THRESHOLDS, area_ranges=COCO_AREA_RANGES, max_dets=COCO_MAX_DETS)
        ev.add_batch(boxes, classes, scores, count, gt_boxes, gt_classes, gt_crowd, gt_area)   # per batch: enqueues only
        res = ev.compute()                                                                     # the only call that synchronises

    Configuration: T = 1..16 ascending IoU thresholds in (0, 1); A = 1..4 area ranges (name, lo, hi), float32 bounds, inclusive; M =
    1..4 ascending maxDets values in 1..65535.  Boxes are xyxy, detections and ground truth in the SAME coordinate system; nothing is
    converted or rescaled, and the default area ranges assume pixels.  Each object has a class, optionally a crowd flag and
    optionally an area (default: (x2-x1)*(y2-y1) in float32; COCO's annotation area is the mask's, so the caller may pass it).

    Protocol.  Per image and class the detections go in descending score order (ties: the one added first); `rank` is the 0-based
    position in that list, and detections with rank >= max_dets[-1] take no part anywhere.  Per area range a an object is ignored if
    it is crowd or area < lo_a or area > hi_a; n_gt[a][c] counts the others.  Per threshold t, each (a, t) with its own claimed set,
    the detections are visited in rank order: the overlap is the float32 IoU, or for a crowd object intersection / area(detection); a
    NaN overlap never matches; the candidates are the class's objects of the image unclaimed at (a, t), plus every crowd object, with
    overlap >= float32(t); the match is the non-ignored candidate of largest overlap if there is one, else the ignored candidate of
    largest overlap, the later object on equal overlap; it becomes claimed.  Matched to a non-ignored object: true positive; to an
    ignored one: ignored; unmatched: ignored if the detection's own area is outside [lo_a, hi_a], else false positive.  Per class,
    area range and threshold the detections of all images with rank < max_dets[-1], in descending (score, added first) order and
    without the ignored ones, give precision = cumTP / position in float64; level k of 100 is reached iff cumTP * 100 >= k * n_gt in
    integers; AP = mean over k = 0..100 of the largest precision at a position reaching level k (0 if none), NaN where n_gt = 0.
    recall[t][a][m][c] = (true positives with rank < max_dets[m]) / n_gt, NaN where n_gt = 0.

    `stats`: the first area range and the last maxDets value play COCO's "all" and 100.  AP = nanmean of ap[:, 0, :]; AP50 / AP75 at
    the threshold equal to float32(0.5) / float32(0.75) (NaN if absent); AP_<name> for each further area range; AR_<m> = nanmean of
    recall at the first area range per maxDets value; AR_<name> for each further area range at the last maxDets value.  With the
    defaults: AP, AP50, AP75, AP_small, AP_medium, AP_large, AR_1, AR_10, AR_100, AR_small, AR_medium, AR_large.

    Deliberate differences from pycocotools: float32 overlaps (there: float64); `>= float32(t)` (there: `>= min(t, 1-1e-10)` in
    double); recall levels decided in integers (there: searchsorted of a float recall against linspace); precision without an
    epsilon (there: `+ eps` in the denominator); a NaN overlap never matches (there: it would); boxes are xyxy in the caller's units
    (there: xywh).  GPU only: there is no CPU fallback."""

    _FIELDS = ("tp", "ign", "rank")

    def __init__(self, n_classes=80, iou_thresholds=COCO_IOU_THRESHOLDS, area_ranges=COCO_AREA_RANGES, max_dets=COCO_MAX_DETS):
        self.n_classes, self._thr32, self.area_ranges, self._lo32, self._hi32, self.max_dets = _check_coco_args(
            n_classes, iou_thresholds, area_ranges, max_dets)
        if not torch.cuda.is_available():
            raise RuntimeError("CocoEvaluator runs on the gfx950 HIP kernels only (no CPU fallback)")
        self.iou_thresholds = tuple(float(t) for t in iou_thresholds)
        self.reset()

    def add_batch(self, boxes, classes, scores, count, gt_boxes, gt_classes, gt_crowd=None, gt_area=None, gt_offsets=None):
        """Score one batch of images against its ground truth and keep the per-detection records.  The layouts are those of
        `DetectionEvaluator.add_batch`, with (n,) 0/1 crowd flags in place of the difficult flags and optional (n,) float areas.
        With padded device detections and packed device ground truth nothing here waits for the device."""
        from . import ops
        db, dc, ds, d_start, d_count, gb, gc, (gcrowd, garea), g_start, dev = _eval_batch_inputs(
            boxes, classes, scores, count, gt_boxes, gt_classes,
            [(gt_crowd, torch.uint8, "gt_crowd"), (gt_area, torch.float32, "gt_area")], gt_offsets, self._dev)
        with torch.cuda.device(dev):
            n_gt = self._n_gt_on(dev, (len(self.area_ranges), self.n_classes))
            rec, tp, ign, rank = ops.coco_match(db, dc, ds, d_start, d_count, gb, gc, gcrowd, garea, g_start, n_gt, self._thr32,
                                                self._lo32, self._hi32, self.max_dets[-1], self.n_classes)
        self._keep(count is not None, ds, rec, tp, ign, rank)

    def compute(self):
        """-> dict: `ap` float64 (T, A, C), NaN where n_gt = 0; `precision` float64 (T, A, C, 101); `recall` float64 (T, A, M, C), NaN
        where n_gt = 0; `tp_count` int64 (T, A, M, C); `n_gt` int64 (A, C); `n_det` int64 (C,); `stats` (see the class); `tp`,
        `ignored` device uint16 (D, A), bit t = true positive / ignored in that area range at iou_thresholds[t], and `rank` device
        int32 (D,) (-1: class outside the range), in the order the detections were added; `iou_thresholds`, `area_ranges`, `max_dets`.
        May be called repeatedly; more batches may be added afterwards."""
        import numpy as np
        from . import ops
        T, A, C = len(self._thr32), len(self.area_ranges), self.n_classes
        rec, score, tp, ign, rank = self._records()
        with torch.cuda.device(self._dev):
            out, tp_count, n_det = ops.coco_ap(rec, score, tp, ign, rank, self._n_gt, T, A, self.max_dets, C)
            precision = out.cpu().numpy()
            tp_count = tp_count.cpu().numpy().astype(np.int64)
            n_gt = self._n_gt.cpu().numpy().astype(np.int64)
            n_det = n_det.cpu().numpy().astype(np.int64)
        with np.errstate(invalid="ignore", divide="ignore"):
            ap = np.where(n_gt[None] > 0, np.mean(precision, axis=-1), np.nan)     # per row the same pairwise sum as np.mean(row)
            recall = np.where(n_gt[None, :, None, :] > 0, tp_count / n_gt[None, :, None, :].astype(np.float64), np.nan)
        stats = coco_stats(ap, recall, self._thr32, [name for name, _, _ in self.area_ranges], self.max_dets)
        words = lambda w: w.view(torch.int16).reshape(-1, 4)[:, :A].contiguous().view(torch.uint16)   # noqa: E731  bit a*16 + t -> [:, a] bit t
        return {"ap": ap, "precision": precision, "recall": recall, "tp_count": tp_count, "n_gt": n_gt, "n_det": n_det, "stats": stats,
                "tp": words(tp), "ignored": words(ign), "rank": rank, "iou_thresholds": self.iou_thresholds,
                "area_ranges": self.area_ranges, "max_dets": self.max_dets}


def evaluate_coco(det_boxes, det_classes, det_scores, gt_boxes, gt_classes, gt_crowd=None, gt_area=None, n_classes=80,
                  iou_thresholds=COCO_IOU_THRESHOLDS, area_ranges=COCO_AREA_RANGES, max_dets=COCO_MAX_DETS):
    """One-shot `CocoEvaluator` over per-image lists (plus optional per-image crowd flags and areas): the dict of
    `CocoEvaluator.compute()`."""
    _check_coco_args(n_classes, iou_thresholds, area_ranges, max_dets)
    if not torch.cuda.is_available():
        raise RuntimeError("evaluate_coco() runs on the gfx950 HIP kernels only (no CPU fallback)")
    ev = CocoEvaluator(n_classes, iou_thresholds, area_ranges, max_dets)
    ev.add_batch(det_boxes, det_classes, det_scores, None, gt_boxes, gt_classes, gt_crowd, gt_area)
    return ev.compute()

"""Host-side mirror of the box utilities the hot path imports from the
reference's Util.py (names and argument meaning kept; bodies are ours).

What `Losses.py` / `train_function.py` pull in through `from Util import *` and what
`train.py:6` / `Dataset.py:4` import by name lives here: prior boxes, box coders, the
class table, `device`, the (empty) VOC lists, `transform` (as a geometry plan: the
pixels are made on the GPU) and `get_map`; `DetectionEvaluator` / `evaluate_detections` are build additions
beside it (VOC difficult objects, IoU sweeps, all-point AP).  VOC XML parsing and drawing are out of
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
    from .Dataset import RawImage, plan_transform
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

    def flat(items, dtype, width):
        parts = [torch.as_tensor(t).reshape((-1, width) if width else (-1,)).to(device=dev, dtype=dtype) for t in items]
        start = torch.tensor([0] + [int(p.shape[0]) for p in parts], dtype=torch.int64).cumsum(0).to(device=dev, dtype=torch.int32)
        return torch.cat(parts).contiguous(), start

    db, d_start = flat(det_boxes, torch.float32, 4)
    dc, _ = flat(det_classes, torch.int32, 0)
    ds, _ = flat(det_scores, torch.float32, 0)
    gb, g_start = flat(gt_boxes, torch.float32, 4)
    gc, _ = flat(gt_classes, torch.int32, 0)
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


class DetectionEvaluator:
    """Average precision under the PASCAL VOC devkit's matching rule, on the GPU (csrc/map_eval.hip E1-E4), with what `get_map`
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

    Out of scope: COCO's own matching rule (best still-unmatched object, crowd regions, area ranges, maxDets) -- a sweep here is "AP
    averaged over IoU thresholds under the VOC matching rule", not COCO mAP --; precision-recall curve export, per-image reports.
    GPU only, like `get_map`: there is no CPU fallback."""

    def __init__(self, n_classes=20, iou_thresholds=(0.5,), interpolation="11point"):
        self.n_classes, self._thr32 = _check_eval_args(n_classes, iou_thresholds, interpolation)
        if not torch.cuda.is_available():
            raise RuntimeError("DetectionEvaluator runs on the gfx950 HIP kernels only (no CPU fallback)")
        self.iou_thresholds = tuple(float(t) for t in iou_thresholds)
        self.interpolation = interpolation
        self.reset()

    def reset(self):
        """Forget every batch added so far."""
        self._rec, self._score, self._tp, self._ign = [], [], [], []
        self._n_gt = None
        self._padded = False
        self._dev = None

    @staticmethod
    def _starts(counts, dev):
        start = [0]
        for n in counts:
            start.append(start[-1] + int(n))
        return torch.tensor(start, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)

    @staticmethod
    def _cat(items, dtype, width, dev):
        parts = [torch.as_tensor(t).reshape((-1, width) if width else (-1,)).to(device=dev, dtype=dtype) for t in items]
        if not parts:
            return torch.zeros((0, width) if width else (0,), device=dev, dtype=dtype), []
        return torch.cat(parts).contiguous(), [int(p.shape[0]) for p in parts]

    def add_batch(self, boxes, classes, scores, count, gt_boxes, gt_classes, gt_difficult=None, gt_offsets=None):
        """Score one batch of images against its ground truth and keep the per-detection records.

        Detections: the padded device tensors of `Losses.inference_batch_padded` -- boxes (B,K,4), classes (B,K) integer, scores
        (B,K), count (B,) int32; rows >= count[b] are not detections and are never read -- or, with count=None, per-image lists of
        (n,4) boxes, (n,) classes, (n,) scores as `get_map` takes them.  Ground truth: per-image lists of (n,4) boxes, (n,) classes
        and optionally (n,) 0/1 difficult flags, or packed device tensors (G,4), (G,), (G,) with gt_offsets = (B+1,) int32 device
        tensor of each image's first row.  Same coordinate system on both sides (see the class docstring).
        With padded device detections and packed device ground truth nothing here waits for the device."""
        from . import ops
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
            self._padded = True
        else:
            if not (len(boxes) == len(classes) == len(scores)):
                raise ValueError("add_batch expects one entry per image in boxes, classes and scores")
            n_img = len(boxes)
            dev = next((t.device for t in list(boxes) + (list(gt_boxes) if gt_offsets is None else [gt_boxes])
                        if torch.is_tensor(t) and t.is_cuda), dev)
            db, per = self._cat(boxes, torch.float32, 4, dev)
            dc, per_c = self._cat(classes, torch.int32, 0, dev)
            ds, per_s = self._cat(scores, torch.float32, 0, dev)
            if per != per_c or per != per_s:
                raise ValueError("add_batch: boxes, classes and scores disagree on the detections per image")
            d_start, d_count = self._starts(per, dev), None
        if n_img == 0:
            raise ValueError("add_batch expects at least one image")
        if self._dev is not None and dev != self._dev:
            raise ValueError(f"add_batch: this evaluator accumulates on {self._dev}, the batch is on {dev}")
        if gt_offsets is not None:
            if not (torch.is_tensor(gt_boxes) and gt_boxes.is_cuda and torch.is_tensor(gt_offsets) and gt_offsets.is_cuda):
                raise ValueError("add_batch: packed ground truth (gt_offsets given) must be device tensors")
            gb = gt_boxes.detach().reshape(-1, 4).to(torch.float32).contiguous()
            gc = gt_classes.detach().reshape(-1).to(device=dev, dtype=torch.int32).contiguous()
            gd = None if gt_difficult is None else gt_difficult.detach().reshape(-1).to(device=dev, dtype=torch.uint8).contiguous()
            g_start = gt_offsets.detach().to(torch.int32).contiguous()
            if g_start.numel() != n_img + 1:
                raise ValueError("add_batch: gt_offsets must have one entry per image plus one")
        else:
            if len(gt_boxes) != n_img or len(gt_classes) != n_img or (gt_difficult is not None and len(gt_difficult) != n_img):
                raise ValueError("add_batch expects one ground-truth entry per image")
            gb, per = self._cat(gt_boxes, torch.float32, 4, dev)
            gc, per_c = self._cat(gt_classes, torch.int32, 0, dev)
            gd = None
            if gt_difficult is not None:
                gd, per_d = self._cat(gt_difficult, torch.uint8, 0, dev)
                if per_d != per:
                    raise ValueError("add_batch: gt_boxes and gt_difficult disagree on the objects per image")
            if per != per_c:
                raise ValueError("add_batch: gt_boxes and gt_classes disagree on the objects per image")
            g_start = self._starts(per, dev)
        with torch.cuda.device(dev):
            if self._n_gt is None:
                self._n_gt = torch.zeros(self.n_classes, device=dev, dtype=torch.int32)
                self._dev = dev
            rec, tp, ign = ops.eval_match(db, dc, ds, d_start, d_count, gb, gc, gd, g_start, self._n_gt, self._thr32, self.n_classes)
        self._rec.append(rec); self._tp.append(tp); self._ign.append(ign)
        self._score.append(ds.reshape(-1).clone() if count is not None else ds)      # the caller may reuse its padded buffers

    def compute(self):
        """-> dict: `ap` float64 (T, n_classes), NaN where a class has no non-difficult ground truth; `mean_ap` float64 (T,), nanmean
        over the classes; `mean_ap_over_thresholds`; `n_gt`, `n_det` int64 (n_classes,); `tp`, `ignored` device uint16 (D,), bit t =
        true positive / ignored at iou_thresholds[t], in the order the detections were added; `iou_thresholds`; `interpolation`.
        May be called repeatedly; more batches may be added afterwards."""
        import numpy as np
        from . import ops
        if self._n_gt is None:
            raise RuntimeError("DetectionEvaluator.compute(): no batch has been added")
        T, C, L = len(self._thr32), self.n_classes, _INTERPOLATION_LEVELS[self.interpolation]
        with torch.cuda.device(self._dev):
            rec, score = torch.cat(self._rec), torch.cat(self._score)
            tp, ign = torch.cat(self._tp), torch.cat(self._ign)
            if self._padded:
                keep = rec != -2                                              # rows past count[b] of the padded batches
                rec, score, tp, ign = rec[keep].contiguous(), score[keep].contiguous(), tp[keep].contiguous(), ign[keep].contiguous()
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

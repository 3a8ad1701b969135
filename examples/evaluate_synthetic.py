"""Scoring loop on synthetic data: SSD_300().eval() -> Losses.inference_batch_padded -> Util.DetectionEvaluator or, with
--protocol coco, Util.CocoEvaluator; nothing waits for the device until compute().  The network is untrained, so the numbers are
near zero; the loop is the point.

    python examples/evaluate_synthetic.py [--batches 4] [--batch 32] [--sweep] [--protocol voc|coco]
                                          [--nms hard|linear|gaussian] [--keep-score 0.001] [--ema]

See INTEGRATION.md section 3c for the VOC devkit protocol (difficult flags) and the coordinate systems, section 3d for COCO's
(crowd regions, area ranges in pixels, maxDets), section 3e for Soft-NMS (--nms; --keep-score: the decayed score below which a
box is dropped, default = the candidate threshold 0.02).  --ema: take a few training steps with `optim.SGD(ema_decay=...)` first and
score under `optimizer.ema_weights()`, the averaged weights swapped in place.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import objectdetection_ssd_amd as amd

amd.install_dropin()
from Losses import inference_batch_padded     # noqa: E402
from Model import SSD_300                     # noqa: E402
from Util import COCO_IOU_THRESHOLDS, CocoEvaluator, DetectionEvaluator   # noqa: E402


def ground_truth(bs, rng, dev, n_classes=20, scale=1.0):
    """Packed ground truth of one batch in fractions of the image times `scale`: boxes (G,4), classes (G,), difficult or crowd flags
    (G,), offsets (B+1,)."""
    n = 1 + np.minimum(rng.poisson(1.4, bs), 7)
    g = int(n.sum())
    xy, wh = rng.uniform(0, .6, (g, 2)), rng.uniform(.08, .4, (g, 2))
    boxes = torch.from_numpy((np.concatenate([xy, xy + wh], 1) * scale).astype(np.float32)).to(dev)
    classes = torch.from_numpy(rng.integers(0, n_classes, g).astype(np.int32)).to(dev)
    difficult = torch.from_numpy((rng.uniform(size=g) < .15).astype(np.uint8)).to(dev)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(n)]).astype(np.int32)).to(dev)
    return boxes, classes, difficult, offsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--sweep", action="store_true", help="IoU 0.50:0.05:0.95 instead of 0.5 alone")
    ap.add_argument("--protocol", choices=("voc", "coco"), default="voc", help="coco: the 81-column model and COCO's twelve numbers")
    ap.add_argument("--nms", choices=("hard", "linear", "gaussian"), default="hard", help="suppression rule of the decode")
    ap.add_argument("--score", choices=("softmax", "sigmoid"), default="softmax",
                    help="class probabilities of the decode: sigmoid for a model trained with --conf-loss focal")
    ap.add_argument("--keep-score", type=float, default=None, help="Soft-NMS: drop boxes whose decayed score falls below this")
    ap.add_argument("--ema", action="store_true", help="voc protocol: three training steps with a weight EMA, then score with the averaged weights")
    a = ap.parse_args()
    dev = torch.device("cuda")
    if a.protocol == "coco":
        return main_coco(a, dev)
    cnn = SSD_300().to(dev).eval()
    if a.ema:
        with averaged_weights(cnn, dev):
            return score_voc(a, cnn, dev)
    return score_voc(a, cnn, dev)


def averaged_weights(cnn, dev, steps=3, bs=4):
    """A few steps of the reference's optimizer set-up (train.py:44-55) with `ema_decay` -> the optimizer's `ema_weights()` context."""
    from Losses import ssd
    from objectdetection_ssd_amd.optim import SGD
    biases = [p for n, p in cnn.named_parameters() if p.requires_grad and n.endswith(".bias")]
    rest = [p for n, p in cnn.named_parameters() if p.requires_grad and not n.endswith(".bias")]
    opt = SGD([{"params": biases, "lr": 2e-4}, {"params": rest}], lr=1e-4, momentum=0.9, weight_decay=5e-4, ema_decay=0.99)
    rng, g = np.random.default_rng(1), torch.Generator().manual_seed(1)
    cnn.train()
    for _ in range(steps):
        boxes, classes, _, offsets = ground_truth(bs, rng, dev)
        off = offsets.tolist()
        opt.zero_grad()
        l1, l2 = ssd(cnn(torch.randn(bs, 3, 300, 300, generator=g).to(dev)), [classes[a:b].float() for a, b in zip(off, off[1:])],
                     [boxes[a:b] for a, b in zip(off, off[1:])])
        (l1 + l2).backward()
        opt.step()
    cnn.eval()
    return opt.ema_weights()


def score_voc(a, cnn, dev):
    ev = DetectionEvaluator(n_classes=20, iou_thresholds=COCO_IOU_THRESHOLDS if a.sweep else (0.5,), interpolation="all")
    rng = np.random.default_rng(0)
    g = torch.Generator().manual_seed(0)
    sizes = torch.ones(a.batch, 2, device=dev)          # decode to fractions: the ground truth's coordinate system
    for _ in range(a.batches):
        x = torch.randn(a.batch, 3, 300, 300, generator=g).to(dev)
        gt_boxes, gt_classes, gt_difficult, gt_offsets = ground_truth(a.batch, rng, dev)
        with torch.no_grad():
            loc, conf = cnn(x)
        boxes, classes, probs, _, count = inference_batch_padded(loc, conf, sizes, min_score=0.02, nms=a.nms, keep_score=a.keep_score, score=a.score)
        ev.add_batch(boxes, classes, probs, count, gt_boxes, gt_classes, gt_difficult, gt_offsets=gt_offsets)
    res = ev.compute()
    for t, m in zip(res["iou_thresholds"], res["mean_ap"]):
        print(f"IoU > {t:.2f}: mean AP {m:.4f}")
    print(f"mean over thresholds {res['mean_ap_over_thresholds']:.4f}; {int(res['n_det'].sum())} detections, "
          f"{int(res['n_gt'].sum())} non-difficult objects")


def main_coco(a, dev):
    """The COCO loop: 80 classes, detections decoded to the pixels of the 300 x 300 input, ground truth in the same pixels (the
    default area ranges are in pixels), crowd flags, and for each object a mask-like area below its box's."""
    cnn = SSD_300(n_classes=80).to(dev).eval()
    ev = CocoEvaluator(n_classes=80)
    rng = np.random.default_rng(0)
    g = torch.Generator().manual_seed(0)
    sizes = torch.full((a.batch, 2), 300.0, device=dev)
    for _ in range(a.batches):
        x = torch.randn(a.batch, 3, 300, 300, generator=g).to(dev)
        gt_boxes, gt_classes, gt_crowd, gt_offsets = ground_truth(a.batch, rng, dev, n_classes=80, scale=300.0)
        gt_area = (gt_boxes[:, 2] - gt_boxes[:, 0]) * (gt_boxes[:, 3] - gt_boxes[:, 1]) * 0.7
        with torch.no_grad():
            loc, conf = cnn(x)
        boxes, classes, probs, _, count = inference_batch_padded(loc, conf, sizes, min_score=0.02, nms=a.nms, keep_score=a.keep_score, score=a.score)
        ev.add_batch(boxes, classes, probs, count, gt_boxes, gt_classes, gt_crowd, gt_area, gt_offsets=gt_offsets)
    res = ev.compute()
    for k, v in res["stats"].items():
        print(f"{k:>10s} {v:.4f}")
    print(f"{int(res['n_det'].sum())} detections, {int(res['n_gt'][0].sum())} objects that are not crowd")


if __name__ == "__main__":
    main()

"""Scoring loop on synthetic data: SSD_300().eval() -> Losses.inference_batch_padded -> Util.DetectionEvaluator, nothing waiting
for the device until compute().  The network is untrained, so the numbers are near zero; the loop is the point.

    python examples/evaluate_synthetic.py [--batches 4] [--batch 32] [--sweep]

See INTEGRATION.md section 3c for the VOC devkit protocol (difficult flags) and the coordinate systems.
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
from Util import COCO_IOU_THRESHOLDS, DetectionEvaluator   # noqa: E402


def ground_truth(bs, rng, dev):
    """Packed ground truth of one batch in fractions of the image: boxes (G,4), classes (G,), difficult (G,), offsets (B+1,)."""
    n = 1 + np.minimum(rng.poisson(1.4, bs), 7)
    g = int(n.sum())
    xy, wh = rng.uniform(0, .6, (g, 2)), rng.uniform(.08, .4, (g, 2))
    boxes = torch.from_numpy(np.concatenate([xy, xy + wh], 1).astype(np.float32)).to(dev)
    classes = torch.from_numpy(rng.integers(0, 20, g).astype(np.int32)).to(dev)
    difficult = torch.from_numpy((rng.uniform(size=g) < .15).astype(np.uint8)).to(dev)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(n)]).astype(np.int32)).to(dev)
    return boxes, classes, difficult, offsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--sweep", action="store_true", help="IoU 0.50:0.05:0.95 instead of 0.5 alone")
    a = ap.parse_args()
    dev = torch.device("cuda")
    cnn = SSD_300().to(dev).eval()
    ev = DetectionEvaluator(n_classes=20, iou_thresholds=COCO_IOU_THRESHOLDS if a.sweep else (0.5,), interpolation="all")
    rng = np.random.default_rng(0)
    g = torch.Generator().manual_seed(0)
    sizes = torch.ones(a.batch, 2, device=dev)          # decode to fractions: the ground truth's coordinate system
    for _ in range(a.batches):
        x = torch.randn(a.batch, 3, 300, 300, generator=g).to(dev)
        gt_boxes, gt_classes, gt_difficult, gt_offsets = ground_truth(a.batch, rng, dev)
        with torch.no_grad():
            loc, conf = cnn(x)
        boxes, classes, probs, _, count = inference_batch_padded(loc, conf, sizes, min_score=0.02)
        ev.add_batch(boxes, classes, probs, count, gt_boxes, gt_classes, gt_difficult, gt_offsets=gt_offsets)
    res = ev.compute()
    for t, m in zip(res["iou_thresholds"], res["mean_ap"]):
        print(f"IoU > {t:.2f}: mean AP {m:.4f}")
    print(f"mean over thresholds {res['mean_ap_over_thresholds']:.4f}; {int(res['n_det'].sum())} detections, "
          f"{int(res['n_gt'].sum())} non-difficult objects")


if __name__ == "__main__":
    main()

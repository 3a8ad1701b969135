"""Drop-in usage on synthetic data: the reference's training loop shape (train_function.py:59-95) on the gfx950 path.

    python examples/train_synthetic.py [--steps 20] [--batch 20] [--fused-sgd] [--grad-clip 10.0]
                                       [--schedule none|multistep|cosine] [--warmup-steps 5] [--ema-decay 0.999]
                                       [--decode host|device] [--ignore-difficult]

With the reference checked out next to this repo, the same three lines (`install_dropin()`, then
`from train_function import train_model`) run its own `train_model` unchanged -- see INTEGRATION.md.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import objectdetection_ssd_amd as amd

amd.install_dropin()
from Losses import ssd            # noqa: E402  (reference import style)
from Model import SSD_300         # noqa: E402


def batches(n, bs, dev, seed=0, ignore_difficult=False):
    rng = np.random.default_rng(seed)
    g = torch.Generator().manual_seed(seed)
    for _ in range(n):
        x = torch.randn(bs, 3, 300, 300, generator=g)
        classes, boxes = [], []
        for _ in range(bs):
            k = 1 + min(int(rng.poisson(1.4)), 7)
            x1, y1 = rng.uniform(0, .6, k), rng.uniform(0, .6, k)
            w, h = rng.uniform(.08, .6, k), rng.uniform(.08, .6, k)
            boxes.append(torch.tensor(np.stack([x1, y1, np.minimum(x1 + w, 1), np.minimum(y1 + h, 1)], 1), dtype=torch.float32))
            classes.append(torch.tensor(rng.integers(0, 20, k), dtype=torch.float32))
        if not ignore_difficult:
            yield x, classes, boxes, None
            continue
        # every second object after an image's first counts as `difficult`: out of the ground truth, into the ignore list
        hard = [torch.arange(len(b)) % 2 == 1 for b in boxes]
        yield x, [c[~h] for c, h in zip(classes, hard)], [b[~h] for b, h in zip(boxes, hard)], [b[h] for b, h in zip(boxes, hard)]


def jpeg_batches(n, bs, decode, seed=0, ignore_difficult=False, mosaic=0.0, affine=0.0):
    """The reference's input side (train.py:29): synthetic JPEG files on disk, `MultiImageMultiBBoxDataset` + `collate_fn` in two
    DataLoader workers.  decode="host": PIL decodes in the workers and pixels travel; decode="device": the files' bytes travel and
    `inputs.to(device)` decodes them on the GPU (a progressive file among them takes the PIL path inside the same batch).
    mosaic > 0: that share of the samples is composed of four files each, resized into the quadrants around a random centre.
    affine > 0: that share of the samples -- plain or mosaic -- is rotated, scaled, sheared and shifted on the device after the resize."""
    import tempfile
    from PIL import Image
    from Dataset import MultiImageMultiBBoxDataset, collate_fn
    from Util import class_to_label
    rng = np.random.default_rng(seed)
    tmp = tempfile.TemporaryDirectory()
    paths, boxes, labels = [], [], []
    yy, xx = np.mgrid[0:375, 0:500]
    for i in range(n * bs):
        px = np.clip(np.stack([127 + 90 * np.sin(xx * rng.uniform(.01, .08) + yy * rng.uniform(.01, .08) + c) for c in range(3)], -1)
                     + rng.normal(0, 14, (375, 500, 3)), 0, 255).astype(np.uint8)
        paths.append(os.path.join(tmp.name, f"{i}.jpg"))
        Image.fromarray(px).save(paths[-1], "JPEG", quality=75, progressive=(i % 7 == 3), restart_marker_rows=1)
        k = 1 + min(int(rng.poisson(1.4)), 7)
        x1, y1 = rng.uniform(0, 300, k), rng.uniform(0, 225, k)
        boxes.append(np.stack([x1, y1, x1 + rng.uniform(40, 190, k), y1 + rng.uniform(40, 140, k)], 1).tolist())
        labels.append([class_to_label[int(c)] for c in rng.integers(0, 20, k)])
    # --ignore-difficult: every second object after an image's first is `difficult`; keep_difficult="ignore" leaves those out of the
    # ground truth (as the default False does) and hands them back, carried through the same augmentation, as a fifth list
    difficult = [[int(ignore_difficult and j % 2 == 1) for j in range(len(b))] for b in boxes]
    ds = MultiImageMultiBBoxDataset(paths, boxes, labels, difficult, list(range(len(paths))),
                                    keep_difficult="ignore" if ignore_difficult else False, decode=decode, mosaic=mosaic, affine=affine)
    dl = torch.utils.data.DataLoader(ds, batch_size=bs, shuffle=True, num_workers=2, collate_fn=collate_fn)
    for inputs, classes, bboxes, _, *ignore in dl:
        yield inputs, classes, bboxes, (ignore[0] if ignore else None)
    tmp.cleanup()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=20)        # train.py:29
    ap.add_argument("--fused-sgd", action="store_true", help="objectdetection_ssd_amd.optim.SGD in place of torch.optim.SGD (same results)")
    ap.add_argument("--optimizer", choices=("sgd", "adamw"), default="sgd",
                    help="adamw: objectdetection_ssd_amd.optim.AdamW (weight decay 1e-2) on the same flat buffers and device words as the "
                         "fused SGD step; takes --grad-clip, --schedule and --ema-decay as SGD does")
    ap.add_argument("--grad-clip", type=float, default=None, metavar="FLOAT",
                    help="clip the global gradient 2-norm to FLOAT inside the fused optimizer step and skip non-finite steps (implies "
                         "--fused-sgd; what torch.nn.utils.clip_grad_norm_ before optimizer.step() does, without leaving the device)")
    ap.add_argument("--schedule", choices=("none", "multistep", "cosine"), default="none",
                    help="a per-iteration learning-rate schedule over --steps, kept on the device (implies --fused-sgd): multistep drops "
                         "the rate tenfold at 2/3 and 8/9 of the run, cosine anneals it to zero")
    ap.add_argument("--warmup-steps", type=int, default=0, help="linear warm-up from a tenth of the rate over this many steps (with --schedule)")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="FLOAT",
                    help="keep an exponential moving average of the weights inside the optimizer step (implies --fused-sgd)")
    ap.add_argument("--decode", choices=("host", "device"), default=None,
                    help="feed the loop from synthetic JPEG files through Dataset / DataLoader workers instead of random tensors: "
                         "'host' decodes with PIL in the workers, 'device' ships the compressed bytes and decodes on the GPU")
    ap.add_argument("--ignore-difficult", action="store_true",
                    help="mark some objects `difficult` and train with them as ignore regions (Losses.ssd(ignore_bboxs=...)): the priors "
                         "over them are neither positives nor mined as hard negatives")
    ap.add_argument("--loc-loss", choices=("l1", "iou", "giou", "diou", "ciou"), default="l1",
                    help="the localisation term (Losses.ssd(loc_loss=...)): the reference's L1 over the encoded offsets, or a box-overlap "
                         "term on the decoded prediction")
    ap.add_argument("--conf-loss", choices=("ce", "focal"), default="ce",
                    help="the classification term (Losses.ssd(conf_loss=...)): the reference's cross entropy with hard-negative mining, or "
                         "the sigmoid focal loss over every prior; focal also starts the heads from SSD_300.init_conf_prior()")
    ap.add_argument("--focal-alpha", type=float, default=0.25, help="--conf-loss focal: weight of the positives (negative: no weighting)")
    ap.add_argument("--focal-gamma", type=float, default=2.0, help="--conf-loss focal: exponent of the modulating factor")
    ap.add_argument("--match", choices=("iou", "atss"), default="iou",
                    help="which priors are positives (Losses.ssd(match=...)): the reference's IoU >= 0.5 rule with one forced prior per "
                         "box, or ATSS (the candidates of the --atss-topk nearest cells per level above mean + std of their IoUs)")
    ap.add_argument("--atss-topk", type=int, default=9, help="--match atss: cells per pyramid level and box (1 .. 32)")
    ap.add_argument("--mosaic", type=float, default=0.0, metavar="P",
                    help="compose a sample with probability P of four files, each resized into one quadrant around a random centre "
                         "(mosaic augmentation; feeds from files: implies --decode host unless --decode is given)")
    ap.add_argument("--affine", type=float, default=0.0, metavar="P",
                    help="warp a sample with probability P by a random rotation, scale, shear and shift of the 300 x 300 frame (random "
                         "affine augmentation, after --mosaic where both are given; feeds from files like --mosaic)")
    a = ap.parse_args()
    if (a.mosaic > 0 or a.affine > 0) and a.decode is None:
        a.decode = "host"
    opt_kw = {}
    if a.schedule != "none" or a.warmup_steps or a.ema_decay is not None:
        from objectdetection_ssd_amd.optim import LRSchedule
        a.fused_sgd = True
        if a.schedule == "multistep":
            opt_kw["schedule"] = LRSchedule.multistep([a.steps * 2 // 3, a.steps * 8 // 9], total_steps=a.steps, warmup_steps=a.warmup_steps)
        elif a.schedule == "cosine":
            opt_kw["schedule"] = LRSchedule.cosine(max(a.steps, 1), warmup_steps=a.warmup_steps)
        elif a.warmup_steps:
            opt_kw["schedule"] = LRSchedule.constant(warmup_steps=a.warmup_steps)
        if a.ema_decay is not None:
            opt_kw["ema_decay"] = a.ema_decay
    if a.grad_clip is not None:
        a.fused_sgd = True
        opt_kw.update(max_grad_norm=a.grad_clip, skip_nonfinite=True)
    device = torch.device("cuda")
    cnn = SSD_300()
    conf_kw = {}
    if a.conf_loss == "focal":
        cnn.init_conf_prior()                                 # every prior starts at sigmoid score 0.01 (score with --score sigmoid)
        conf_kw = dict(conf_loss="focal", focal_alpha=a.focal_alpha, focal_gamma=a.focal_gamma)
    if a.match != "iou":
        conf_kw.update(match=a.match, atss_topk=a.atss_topk)
    cnn = cnn.to(device)
    biases = [p for n, p in cnn.named_parameters() if p.requires_grad and n.endswith(".bias")]
    not_biases = [p for n, p in cnn.named_parameters() if p.requires_grad and not n.endswith(".bias")]
    lr = 1e-4
    if a.fused_sgd:
        from objectdetection_ssd_amd.optim import SGD
    else:
        SGD = torch.optim.SGD
    groups = [{"params": biases, "lr": 2 * lr}, {"params": not_biases}]
    if a.optimizer == "adamw":
        from objectdetection_ssd_amd.optim import AdamW
        optimizer = AdamW(params=groups, lr=lr, weight_decay=1e-2, **opt_kw)
    else:
        optimizer = SGD(params=groups, lr=lr, momentum=0.9, weight_decay=5e-4, **opt_kw)      # train.py:53-55
    cnn.train()
    t0 = time.time()
    feed = (batches(a.steps, a.batch, device, ignore_difficult=a.ignore_difficult) if a.decode is None else
            jpeg_batches(a.steps, a.batch, a.decode, ignore_difficult=a.ignore_difficult, mosaic=a.mosaic, affine=a.affine))
    for count, (inputs, classes, bboxes, ignore) in enumerate(feed):
        raw = inputs
        inputs = inputs.to(device)                            # a RawBatch: upload, JPEG decode, photometric, resize + normalise, affine warp
        classes = [c.to(device) for c in classes]
        bboxes = [b.to(device) for b in bboxes]
        optimizer.zero_grad()
        outputs = cnn(inputs)
        if ignore is None:
            loss1, loss2 = ssd(outputs, classes, bboxes, loc_loss=a.loc_loss, **conf_kw)
        else:
            loss1, loss2 = ssd(outputs, classes, bboxes, loc_loss=a.loc_loss, ignore_bboxs=ignore, **conf_kw)
        loss = loss1 + loss2
        loss.backward()
        optimizer.step()
        if count % 5 == 0:
            norm = ""
            if "max_grad_norm" in opt_kw:                     # device values of the step just taken; reading them is this loop's sync
                norm = (f"  |g| {optimizer.grad_norm.item():.3f}  clip {optimizer.clip_coef.item():.3f}"
                        f"  skipped {optimizer.skipped_steps.item()}")
            if "schedule" in opt_kw or "ema_decay" in opt_kw:
                norm += f"  lr {optimizer.current_lr[1].item():.3g}  ema_w {optimizer.ema_weight.item():.3g}"
            if ignore is not None:                            # reading it is this loop's sync
                import Losses
                norm += f"  ignored priors {int(Losses.last_match['ignored'].sum())} ({sum(len(b) for b in ignore)} boxes)"
            if getattr(raw, "decode_status", None) is not None:   # reading it is this loop's sync
                norm += f"  decoded on the device {int((raw.decode_status == 0).sum())}/{len(raw)}"
            print(f"it {count:3d}  l1 {loss1.item():.4f}  l2 {loss2.item():.4f}{norm}  {time.time() - t0:.1f}s")
    if "ema_decay" in opt_kw:                                 # evaluate with the averaged weights: swapped in place, and back
        cnn.eval()
        with torch.no_grad(), optimizer.ema_weights():
            loc, _ = cnn(torch.randn(a.batch, 3, 300, 300, device=device))
        cnn.train()
        print(f"forward with the averaged weights: mean |loc| {loc.abs().mean().item():.4f}")
    torch.cuda.synchronize()
    print(f"{a.steps * a.batch / (time.time() - t0):.1f} images/s incl. host-side data generation")


if __name__ == "__main__":
    main()

"""Cost of the class count, interleaved on one device: the SSD300 train step (forward + MultiBox loss + backward, no optimizer) at
batch 32 for C = 21 and 81 columns in f32 and bf16, the loss call alone for C = 21 / 81 / 256 and the batched decode + NMS of 32
images for C = 21 / 81.  HIP events around each item, rounds interleaved (every item once per round, medians over the rounds); one
JSON line.  Run it under a kernel trace to attribute the time to kernels, e.g.

    rocprofv3 --kernel-trace --stats -d OUT -o cc -- python tools/class_count_bench.py --rounds 5
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from objectdetection_ssd_amd import Losses, Model

DEV = torch.device("cuda:0")


def gt_batch(bs, C, seed):
    rng = np.random.default_rng(seed)
    boxes, classes = [], []
    for _ in range(bs):
        n = 1 + min(int(rng.poisson(1.4)), 7)
        x1 = rng.uniform(0, .6, n); y1 = rng.uniform(0, .6, n)
        w = rng.uniform(.08, .6, n); h = rng.uniform(.08, .6, n)
        b = np.stack([x1, y1, np.minimum(x1 + w, 1.), np.minimum(y1 + h, 1.)], 1).astype(np.float32)
        boxes.append(torch.from_numpy(b).to(DEV))
        classes.append(torch.from_numpy(rng.integers(0, C - 1, n).astype(np.float32)).to(DEV))
    return classes, boxes


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bs", type=int, default=32)
    args = ap.parse_args()
    bs = args.bs
    torch.manual_seed(0)
    x = torch.randn(bs, 3, 300, 300, device=DEV)
    items = {}
    nets = {}
    for C in (21, 81):
        nets[C] = Model.SSD_300(n_classes=C - 1).to(DEV).train()
    for C in (21, 81):
        for dt in ("f32", "bf16"):
            cl, bx = gt_batch(bs, C, 7)

            def step(C=C, dt=dt, cl=cl, bx=bx):
                net = nets[C]
                net.conv_dtype = dt
                net.zero_grad(set_to_none=True)
                l1, l2 = Losses.ssd(net(x), cl, bx)
                (l1 + l2).backward()
            items[f"train_step_C{C}_{dt}_ms"] = (step, 3)
    for C in (21, 81, 256):
        cl, bx = gt_batch(bs, C, 11)
        loc = torch.randn(bs, 8732, 4, device=DEV).requires_grad_(True)
        conf = (torch.randn(bs, 8732, C, device=DEV) * 2).requires_grad_(True)

        def loss(loc=loc, conf=conf, cl=cl, bx=bx):
            l1, l2 = Losses.ssd((loc, conf), cl, bx)
            (l1 + l2).backward()
        items[f"loss_C{C}_ms"] = (loss, 20)
    sizes = torch.tensor([[300., 300.]] * bs, device=DEV)
    for C in (21, 81):
        l = torch.randn(bs, 8732, 4, device=DEV) * 0.5
        c = torch.randn(bs, 8732, C, device=DEV) * 3

        def decode(l=l, c=c):
            Losses.inference_batch_padded(l, c, sizes)
        items[f"decode_nms_b{bs}_C{C}_ms"] = (decode, 10)
    for fn, _ in items.values():                  # warm-up: weight layouts, workspaces, allocator pools
        fn()
        fn()
    res = {k: [] for k in items}
    for _ in range(args.rounds):
        for k, (fn, reps) in items.items():
            res[k].append(timed(fn, reps))
    for net in nets.values():
        net.conv_dtype = "f32"
    out = {k: round(statistics.median(v), 4) for k, v in res.items()}
    out.update(bs=bs, rounds=args.rounds, note="median over interleaved rounds of the per-call time (HIP events; train step = forward + "
               "loss + backward, no optimizer; loss = forward + backward of Losses.ssd on given loc / conf)")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

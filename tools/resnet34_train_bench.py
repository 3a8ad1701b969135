"""SSD_resnet34 at batch 32, 224x224, f32: the eval forward, the train forward, and the full train step (train forward + backward of
a fixed upstream gradient + torch.optim.SGD step), timed by device events, interleaved in one process.  Prints one JSON line with
the median milliseconds of each and the kernel-launch count of one train step (counted with torch's profiler when it is available).

    python tools/resnet34_train_bench.py [--bs 32] [--iters 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import ssd_oracle as O  # noqa: E402
from objectdetection_ssd_amd import Model  # noqa: E402


def _net(dev):
    net = Model.SSD_resnet34(20)
    state = O.ssd_resnet34_random_state(0)
    full = dict(state)
    for alias, trunk in O.ssd_resnet34_aliases().items():
        for k in state:
            if k.startswith(trunk):
                full[alias + k[len(trunk):]] = state[k]
    net.load_state_dict(full)
    return net.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    net = _net(dev)
    opt = torch.optim.SGD(net.parameters(), lr=1e-4, momentum=0.9)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(a.bs, 3, 224, 224, generator=g).to(dev)
    gl = torch.randn(a.bs, 63, 4, generator=g).to(dev)
    gc = torch.randn(a.bs, 63, 21, generator=g).to(dev)

    def eval_fwd():
        net.eval()
        with torch.no_grad():
            net(x)

    def train_fwd():
        net.train()
        with torch.no_grad():
            net(x)

    def train_step():
        net.train()
        opt.zero_grad(set_to_none=True)
        loc, conf = net(x)
        torch.autograd.backward((loc, conf), (gl, gc))          # the gradient of (loc*gl).sum() + (conf*gc).sum()
        opt.step()

    # the first eval call after a train call re-folds the BatchNorms (new running statistics): timed on its own, then the eval
    # forward proper on the folded weights
    cases = {"eval_forward_refold": eval_fwd, "eval_forward": eval_fwd, "train_forward": train_fwd, "train_step": train_step}
    for _ in range(a.warmup):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in cases}
    for _ in range(a.iters):
        for k, fn in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in times.items()}
    launches = None
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            train_step()
            torch.cuda.synchronize()
        launches = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as e:                     # the profiler is a convenience: the timings stand without it
        launches = f"unavailable: {type(e).__name__}"
    print(json.dumps({
        "metric": "SSD_resnet34 train mode, ms per call (median of device-event timings, interleaved)",
        "batch": a.bs, "hw": [224, 224], "conv_dtype": "f32", "iters": a.iters,
        "eval_forward_ms": round(med["eval_forward"], 4), "eval_forward_after_train_ms": round(med["eval_forward_refold"], 4), "train_forward_ms": round(med["train_forward"], 4),
        "train_step_ms": round(med["train_step"], 4),
        "train_step_over_eval_forward": round(med["train_step"] / med["eval_forward"], 3),
        "eval_images_per_s": round(a.bs / med["eval_forward"] * 1e3, 1),
        "train_step_images_per_s": round(a.bs / med["train_step"] * 1e3, 1),
        "device_kernels_per_train_step": launches,
        "device": torch.cuda.get_device_name(0),
    }))


if __name__ == "__main__":
    main()

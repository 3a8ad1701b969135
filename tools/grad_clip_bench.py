"""What gradient-norm clipping costs on the device.

    python tools/grad_clip_bench.py [--windows 7] [--launches 200] [--no-step]

1. The norm pass alone (`ssd_grad_norm_partials`, L2 and max) on the real flat gradient buffer of SSD300 (26.3 M floats, 105 MB), as
   the median of several event-timed windows of back-to-back launches.  "cold": the launches rotate over enough copies of the buffer
   to exceed the 256 MB Infinity Cache, so every launch streams from HBM -- its bytes / time is reported as a fraction of the chip's
   measured in-order HBM read rate (6.0 TB/s).  "warm": the same buffer again and again (largely cache resident; what the step sees
   depends on how much of the gradient the backward left in the cache).  Plus the finalise launch on its own.
2. The batch-32 f32 train step with and without clipping, interleaved in one process on one trainer (the protocol of
   tools/ab_step.py: alternating repetitions, 2 untimed + 15 timed steps each, median of 5).

Prints one JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from objectdetection_ssd_amd import Losses, Model, ops  # noqa: E402
from objectdetection_ssd_amd.ddp import FlatSGDDataParallel  # noqa: E402

HBM_READ_TBS = 6.0           # in-order HBM read rate measured for this chip (6.0 - 6.3 TB/s)
INFINITY_CACHE_BYTES = 256 << 20


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def windows(fn, n_windows, launches):
    """Median / min / max microseconds per call of fn(i) over event-timed windows of `launches` back-to-back calls."""
    for i in range(launches // 4 + 1):
        fn(i)
    torch.cuda.synchronize()
    out = []
    for _ in range(n_windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(launches):
            fn(i)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / launches)
    return median(out), min(out), max(out)


def norm_pass(tr, a):
    n = tr.n
    nbytes = n * 4
    slots = ops.grad_norm_slots(n)
    partials = torch.zeros(slots, device=tr.flat_grad.device, dtype=torch.float64)
    state = torch.zeros(ops.GRAD_CLIP_STATE_WORDS, device=tr.flat_grad.device)
    copies = INFINITY_CACHE_BYTES * 2 // nbytes + 1
    bufs = [torch.randn(n, device=tr.flat_grad.device) for _ in range(copies)]
    for norm_type, name in ((2.0, "l2"), (float("inf"), "max")):
        for mode, pick in (("cold", lambda i: bufs[i % copies]), ("warm", lambda i: bufs[0])):
            med, lo, hi = windows(lambda i: ops.grad_norm_partials_(pick(i), partials, 0, norm_type), a.windows, a.launches)
            tbs = nbytes / (med * 1e-6) / 1e12
            print(json.dumps({"what": f"grad_norm_partials_{name}_{mode}", "floats": n, "bytes": nbytes, "slots": slots,
                              "buffers_rotated": copies if mode == "cold" else 1, "us_median": round(med, 2), "us_min": round(lo, 2),
                              "us_max": round(hi, 2), "TB_per_s": round(tbs, 3), "fraction_of_hbm_read_rate": round(tbs / HBM_READ_TBS, 3),
                              "hbm_read_rate_TB_per_s": HBM_READ_TBS, "windows": a.windows, "launches_per_window": a.launches}))
    med, lo, hi = windows(lambda i: ops.grad_clip_finalize_(partials, slots, 2.0, 1.0, tr.inv_npos, True, state), a.windows, a.launches)
    print(json.dumps({"what": "grad_clip_finalize", "slots": slots, "us_median": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2)}))


def step_ab(net, tr, dev):
    x, classes, boxes = bench.synth_batch(32, 1234, dev)

    def steps(k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            tr.zero_grad()
            loc, conf = net(x)
            l1, l2, n_pos = Losses.ssd((loc, conf), classes, boxes, norm_mode=1, with_n_pos=True)
            (l1 + l2).backward()
            tr.reduce_and_step(n_pos)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3
    steps(5)
    variants = {"off": (None, False), "clip_l2": (1.0, True)}
    res = {k: [] for k in variants}
    for _ in range(5):
        for k, (mx, guard) in variants.items():
            tr.max_grad_norm, tr.skip_nonfinite = mx, guard
            steps(2)
            res[k].append(steps(15))
    out = {"what": "train_step_b32_f32_ms", "protocol": "interleaved, 5 x (2 untimed + 15 timed steps), median"}
    for k, v in res.items():
        out[k] = {"median": round(median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    out["clip_minus_off_ms"] = round(median(res["clip_l2"]) - median(res["off"]), 3)
    out["last_grad_norm"] = float(tr.grad_norm)
    out["last_clip_coef"] = float(tr.clip_coef)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--no-step", action="store_true", help="the norm pass only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grad_clip_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = Model.SSD_300().to(dev).train()
    tr = FlatSGDDataParallel(net, lr=1e-4, max_grad_norm=1.0, skip_nonfinite=True)
    norm_pass(tr, a)
    if not a.no_step:
        step_ab(net, tr, dev)


if __name__ == "__main__":
    main()

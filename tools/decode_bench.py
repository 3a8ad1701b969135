"""decode + NMS latency (l_ ~ 0.5*randn, c_ ~ 3*randn, one image)

    python tools/decode_bench.py [--nms hard|linear|gaussian] [--sigma S] [--keep-score K]

--nms linear / gaussian times the Soft-NMS decode instead, and then both rules against each other in this process: alternating
windows of --calls calls, device events, median over --rounds windows (batch 1 and batch 32, c_ ~ 3*randn)."""
import argparse, os, statistics, sys, time, torch, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from objectdetection_ssd_amd import Losses, ops
ap = argparse.ArgumentParser()
ap.add_argument("--nms", choices=("hard", "linear", "gaussian"), default="hard")
ap.add_argument("--sigma", type=float, default=0.5)
ap.add_argument("--keep-score", type=float, default=None)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--rounds", type=int, default=7)
args = ap.parse_args()
rule = dict(nms=args.nms, sigma=args.sigma, keep_score=args.keep_score)
print(f"rule: {rule}", flush=True)
dev = torch.device("cuda")
pri, _ = Losses._priors_on(dev)
for scale in (1.0, 2.0, 3.0, 4.0):
    g = torch.Generator().manual_seed(1)
    l_ = (torch.randn(8732, 4, generator=g) * 0.5).to(dev)
    c_ = (torch.randn(8732, 21, generator=g) * scale).to(dev)
    for _ in range(3):
        out = ops.decode_nms(l_, c_, pri, 500, 375, **rule)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    for _ in range(20):
        out = ops.decode_nms(l_, c_, pri, 500, 375, **rule)
    e1.record(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        b = Losses.inference(l_, c_, (500, 375), toDraw=False, **rule)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / 20
    p = torch.softmax(c_, 1)[:, :20]
    print(f"scale {scale}: candidates {(p >= 0.2).sum().item():6d}  kept {int(out[4].item()):4d}  gpu {e0.elapsed_time(e1) / 20 * 1e3:8.1f} us  inference() wall {wall * 1e6:8.1f} us", flush=True)
# batched
for B in (1, 8, 32):
    g = torch.Generator().manual_seed(2)
    L = (torch.randn(B, 8732, 4, generator=g) * 0.5).to(dev)
    C = (torch.randn(B, 8732, 21, generator=g) * 3.0).to(dev)
    wh = torch.tensor([[500., 375.]] * B, device=dev)
    for _ in range(2): ops.decode_nms_batch(L, C, pri, wh, **rule)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    for _ in range(10): ops.decode_nms_batch(L, C, pri, wh, **rule)
    e1.record(); torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 10
    print(f"batch {B:3d}: {ms * 1e3:8.1f} us per call = {ms * 1e3 / B:7.1f} us per image = {B / ms * 1e3:8.0f} images/s", flush=True)

# the two rules against each other: alternating windows in one process, device events, median (and range) of the windows
if args.nms != "hard":
    def window(fn):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        for _ in range(args.calls): fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.calls * 1e3
    p0 = ops.clock_probe(dev)
    for B in (1, 32):
        g = torch.Generator().manual_seed(2)
        L = (torch.randn(B, 8732, 4, generator=g) * 0.5).to(dev)
        C = (torch.randn(B, 8732, 21, generator=g) * 3.0).to(dev)
        wh = torch.tensor([[500., 375.]] * B, device=dev)
        fns = {"hard": lambda: ops.decode_nms_batch(L, C, pri, wh), args.nms: lambda: ops.decode_nms_batch(L, C, pri, wh, **rule)}
        for fn in fns.values():
            for _ in range(5): fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, fn in fns.items(): t[k].append(window(fn))
        for k, v in t.items():
            print(f"interleaved batch {B:3d} {k:9s}: median {statistics.median(v):8.1f} us per call = {statistics.median(v) / B:7.1f} us per image "
                  f"(min {min(v):.1f}, max {max(v):.1f}; {args.rounds} windows of {args.calls} calls, device events)", flush=True)
    print(f"shader clock between the probes: {ops.shader_mhz(p0, ops.clock_probe(dev)):.0f} MHz", flush=True)

"""What the fused Adam / AdamW step costs beside the fused SGD step it shares its flat buffers and device words with.

    python tools/adam_bench.py [--windows 7] [--launches 50] [--steps 10] [--no-step] [--out profiles/adam_bench.json]

1. Kernels, on flat buffers of SSD300's size (26.3 M floats, 105 MB each), streamed from HBM: the launches rotate over three sets of
   buffers, as tools/sched_ema_bench.py's "cold" mode does.  Interleaved in one process: every window times `launches` back-to-back
   launches of each form in turn between device events, medians over the windows; two clock probes bracket the section:
     sgd        ssd_sgd_momentum_sched without EMA      5 dword streams per element
     sgd_ema    ssd_sgd_momentum_sched with EMA         7
     adam       ssd_adam_step without EMA               7
     adam_ema   ssd_adam_step with EMA                  9
2. The batch-32 f32 train step, interleaved: SGD and AdamW, each eager and replayed (`GraphedTrainStep`), both under a cosine
   schedule with the weight EMA.  Host ms = the time three calls into an idle queue take to return, device ms = the time until the
   device has finished a window of steps, per step.  Plus the kernel-node counts of the captured graphs.

Prints one JSON line per measurement and writes all of them to --out.
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
from objectdetection_ssd_amd.ddp import FlatSGDDataParallel, GraphedTrainStep  # noqa: E402
from objectdetection_ssd_amd.optim import LRSchedule  # noqa: E402

COLD_SETS = 3               # buffer sets the launches rotate over: 3 x 525 MB, far beyond the 256 MB Infinity Cache
HOST_CALLS = 3
RESULTS = []


def emit(d):
    RESULTS.append(d)
    print(json.dumps(d), flush=True)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def stats(v, digits=2):
    return {"median": round(median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "spread_of_median": round((max(v) - min(v)) / median(v), 4)}


def kernels(n, a, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    # p, grad, first moment / momentum, second moment, ema
    sets = [[torch.randn(n, device=dev, generator=g) * s for s in (0.05, 1.0, 0.1, 0.0, 0.05)] for _ in range(COLD_SETS)]
    for s in sets:
        s[3].copy_(s[1] * s[1] * 0.5)
    scale = torch.tensor([1.0 / 300.0], device=dev)
    lr_dev, w_dev = torch.tensor([1e-6], device=dev), torch.tensor([0.1], device=dev)
    state = ops.adam_state(dev)
    for _ in range(100):
        ops.adam_advance_(state, 0.9, 0.999)

    def adam(ema):
        return lambda p, grad, m, v, e: ops.adam_step_(p, grad, m, v, e if ema else None, 1e-6, lr_dev, w_dev, state, 0.9, 0.999, 1e-8,
                                                       1e-2, True, scale, None)

    def sgd(ema):
        return lambda p, grad, m, v, e: ops.sgd_momentum_sched_(p, grad, m, e if ema else None, lr_dev, w_dev, 0.9, 5e-4, scale, False, None)
    forms = {"sgd": (5, sgd(False)), "sgd_ema": (7, sgd(True)), "adam": (7, adam(False)), "adam_ema": (9, adam(True))}
    us = {k: [] for k in forms}
    torch.cuda.synchronize()
    pa = ops.clock_probe(dev)
    for _ in range(a.windows):
        for name, (_, fn) in forms.items():
            for i in range(6):
                fn(*sets[i % COLD_SETS])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.launches):
                fn(*sets[i % COLD_SETS])
            e1.record()
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / a.launches)
    pb = ops.clock_probe(dev)
    torch.cuda.synchronize()
    clock = ops.shader_mhz(pa, pb)
    rate = {}
    for name, (streams, _) in forms.items():
        nbytes = streams * 4 * n
        rate[name] = nbytes / (median(us[name]) * 1e-6) / 1e12
        emit({"what": f"kernel_{name}", "floats": n, "dword_streams": streams, "bytes": nbytes, "us": stats(us[name]),
              "TB_per_s": round(rate[name], 3), "buffer_sets_rotated": COLD_SETS, "windows": a.windows, "launches_per_window": a.launches})
    emit({"what": "kernel_comparison", "adam_rate_over_sgd_rate": round(rate["adam"] / rate["sgd"], 3),
          "adam_ema_rate_over_sgd_ema_rate": round(rate["adam_ema"] / rate["sgd_ema"], 3),
          "adam_minus_sgd_us": round(median(us["adam"]) - median(us["sgd"]), 2),
          "adam_ema_minus_sgd_ema_us": round(median(us["adam_ema"]) - median(us["sgd_ema"]), 2),
          "shader_mhz_average": None if clock != clock else round(clock)})


def steps(a, dev):
    x, classes, boxes = bench.synth_batch(32, 1234, dev)

    def make(**kw):
        torch.manual_seed(0)
        net = Model.SSD_300().to(dev).train()
        return net, FlatSGDDataParallel(net, lr=1e-4, schedule=LRSchedule.cosine(100000, warmup_steps=500), ema_decay=0.9999, **kw)

    def eager_fn(net, tr):
        def fn():
            tr.zero_grad()
            loc, conf = net(x)
            l1, l2, n_pos = Losses.ssd((loc, conf), classes, boxes, norm_mode=1, with_n_pos=True)
            (l1 + l2).backward()
            tr.reduce_and_step(n_pos)
        return fn
    adamw = dict(optimizer="adamw", weight_decay=1e-2)
    (n_se, t_se), (n_ae, t_ae), (n_sg, t_sg), (n_ag, t_ag) = make(), make(**adamw), make(), make(**adamw)
    g_sgd, g_adam = GraphedTrainStep(n_sg, t_sg, warmup=2), GraphedTrainStep(n_ag, t_ag, warmup=2)
    forms = {"sgd_eager": eager_fn(n_se, t_se), "adamw_eager": eager_fn(n_ae, t_ae), "sgd_replayed": lambda: g_sgd(x, classes, boxes),
             "adamw_replayed": lambda: g_adam(x, classes, boxes)}
    for fn in forms.values():
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    graph0 = g_adam.graph
    host, devt, mhz = ({k: [] for k in forms} for _ in range(3))
    for _ in range(a.windows):
        for name, fn in forms.items():
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(HOST_CALLS):
                fn()
            host[name].append((time.perf_counter() - t0) / HOST_CALLS * 1e3)
            torch.cuda.synchronize()
            pa = ops.clock_probe(dev)
            t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            pb = ops.clock_probe(dev)
            torch.cuda.synchronize()
            devt[name].append((time.perf_counter() - t0) / a.steps * 1e3)
            mhz[name].append(ops.shader_mhz(pa, pb))
    for name in forms:
        m = median(mhz[name])
        emit({"what": f"train_step_b32_f32_{name}", "host_ms": stats(host[name], 3), "device_ms": stats(devt[name], 3),
              "shader_mhz_median": None if m != m else round(m), "windows": a.windows, "steps_per_window": a.steps,
              "host_calls_per_window": HOST_CALLS})
    emit({"what": "train_step_comparison_ms",
          "adamw_minus_sgd_eager_device": round(median(devt["adamw_eager"]) - median(devt["sgd_eager"]), 3),
          "adamw_minus_sgd_replayed_device": round(median(devt["adamw_replayed"]) - median(devt["sgd_replayed"]), 3),
          "adamw_minus_sgd_eager_host": round(median(host["adamw_eager"]) - median(host["sgd_eager"]), 3),
          "adamw_minus_sgd_replayed_host": round(median(host["adamw_replayed"]) - median(host["sgd_replayed"]), 3)})
    emit({"what": "graph", "adamw_captured_once": g_adam.graph is graph0, "kernel_nodes_adamw": g_adam.kernel_nodes,
          "kernel_nodes_sgd": g_sgd.kernel_nodes, "final_adam_steps": int(t_ag.adam_steps), "final_step_count": int(t_ag.step_count)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true", help="the kernels only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    probe = FlatSGDDataParallel(Model.SSD_300().to(dev).train(), lr=1e-4)
    n = probe.n
    probe.close()
    del probe
    kernels(n, a, dev)
    if not a.no_step:
        steps(a, dev)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/adam_bench.py", "device": torch.cuda.get_device_name(0), "results": RESULTS}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

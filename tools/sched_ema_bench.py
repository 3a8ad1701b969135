"""What the device-resident learning-rate schedule and the fused weight EMA cost, and what they buy a captured step.

    python tools/sched_ema_bench.py [--windows 7] [--launches 50] [--steps 10] [--no-step] [--out profiles/sched_ema_bench.json]

1. Kernels, on flat buffers of SSD300's size (26.3 M floats, 105 MB each).  "cold": the launches rotate over three sets of buffers,
   so every pass streams from HBM -- what the step sees, where a whole forward and backward lie between two optimizer passes.
   "warm": the same set again and again (partly resident in the 256 MB Infinity Cache).  Interleaved in one process: every window
   times `launches` back-to-back launches of each form in turn between device events, medians over the windows; two clock probes
   bracket the whole section:
     parent_sgd   ssd_sgd_momentum, lr a host float                          5 dword streams per element
     sched_sgd    ssd_sgd_momentum_sched without EMA, lr a device word       5
     fused_ema    ssd_sgd_momentum_sched with EMA                            7
     two_pass     ssd_sgd_momentum, then torch.Tensor.lerp_ over p and e     8
2. The batch-32 f32 train step, interleaved: eager without the feature, eager with schedule + EMA, `GraphedTrainStep` under a
   per-step cosine schedule from the device table (captured once), and the same schedule applied by writing
   `param_groups[*]['lr']` before every call (captured again at every call).  Host ms = the time three calls into an idle queue
   take to return, device ms = the time until the device has finished a window of steps, per step.  Plus the kernel-node counts of the captured graphs.

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

HBM_READ_TBS = 6.0           # in-order HBM read rate measured for this chip (6.0 - 6.3 TB/s), as tools/grad_clip_bench.py uses
COLD_SETS = 3               # buffer sets the "cold" launches rotate over: 3 x 420 MB, far beyond the 256 MB Infinity Cache
HOST_CALLS = 3
RESULTS = []


def emit(d):
    RESULTS.append(d)
    print(json.dumps(d), flush=True)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def mhz_of(v):
    m = median(v)
    return None if m != m else round(m)


def stats(v, digits=2):
    return {"median": round(median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "spread_of_median": round((max(v) - min(v)) / median(v), 4)}


def kernels(n, a, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    sets = [[torch.randn(n, device=dev, generator=g) * s for s in (0.05, 1.0, 0.1, 0.05)] for _ in range(COLD_SETS)]
    scale = torch.tensor([1.0 / 300.0], device=dev)
    lr, mo, wd, w = 1e-6, 0.9, 5e-4, 0.1
    lr_dev, w_dev = torch.tensor([lr], device=dev), torch.tensor([w], device=dev)

    def parent(p, grad, mom, ema):
        ops.sgd_momentum_(p, grad, mom, lr, mo, wd, scale, False)

    def two_pass(p, grad, mom, ema):
        ops.sgd_momentum_(p, grad, mom, lr, mo, wd, scale, False)
        ema.lerp_(p, w)
    forms = {
        "parent_sgd": (5, parent),
        "sched_sgd": (5, lambda p, grad, mom, ema: ops.sgd_momentum_sched_(p, grad, mom, None, lr_dev, None, mo, wd, scale, False, None)),
        "fused_ema": (7, lambda p, grad, mom, ema: ops.sgd_momentum_sched_(p, grad, mom, ema, lr_dev, w_dev, mo, wd, scale, False, None)),
        "two_pass": (8, two_pass),
    }
    us = {(m, k): [] for m in ("cold", "warm") for k in forms}
    torch.cuda.synchronize()
    pa = ops.clock_probe(dev)
    for _ in range(a.windows):
        for mode in ("cold", "warm"):
            for name, (_, fn) in forms.items():
                pick = (lambda i: sets[i % COLD_SETS]) if mode == "cold" else (lambda i: sets[0])
                for i in range(6):
                    fn(*pick(i))
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(a.launches):
                    fn(*pick(i))
                e1.record()
                e1.synchronize()
                us[(mode, name)].append(e0.elapsed_time(e1) * 1e3 / a.launches)
    pb = ops.clock_probe(dev)
    torch.cuda.synchronize()
    clock = ops.shader_mhz(pa, pb)
    for mode in ("cold", "warm"):
        for name, (streams, _) in forms.items():
            v = us[(mode, name)]
            nbytes = streams * 4 * n
            tbs = nbytes / (median(v) * 1e-6) / 1e12
            emit({"what": f"kernel_{name}_{mode}", "floats": n, "dword_streams": streams, "bytes": nbytes, "us": stats(v),
                  "TB_per_s": round(tbs, 3), "fraction_of_hbm_read_rate": round(tbs / HBM_READ_TBS, 3),
                  "buffer_sets_rotated": COLD_SETS if mode == "cold" else 1, "windows": a.windows, "launches_per_window": a.launches})
        m = {k: median(us[(mode, k)]) for k in forms}
        emit({"what": f"kernel_comparison_us_{mode}", "sched_minus_parent": round(m["sched_sgd"] - m["parent_sgd"], 2),
              "fused_minus_two_pass": round(m["fused_ema"] - m["two_pass"], 2), "ema_cost_fused": round(m["fused_ema"] - m["sched_sgd"], 2),
              "ema_cost_two_pass": round(m["two_pass"] - m["parent_sgd"], 2)})
    emit({"what": "kernel_section_clock", "shader_mhz_average": None if clock != clock else round(clock),
          "hbm_read_rate_TB_per_s": HBM_READ_TBS})


def steps(a, dev):
    x, classes, boxes = bench.synth_batch(32, 1234, dev)
    total = 100000                                                   # a cosine over a run's length: every step has another rate

    def make(**kw):
        torch.manual_seed(0)
        net = Model.SSD_300().to(dev).train()
        return net, FlatSGDDataParallel(net, lr=1e-4, **kw)

    def eager_fn(net, tr):
        def fn():
            tr.zero_grad()
            loc, conf = net(x)
            l1, l2, n_pos = Losses.ssd((loc, conf), classes, boxes, norm_mode=1, with_n_pos=True)
            (l1 + l2).backward()
            tr.reduce_and_step(n_pos)
        return fn
    feature = dict(schedule=LRSchedule.cosine(total, warmup_steps=500), ema_decay=0.9999)
    n_off, t_off = make()
    n_on, t_on = make(**feature)
    n_gd, t_gd = make(**feature)
    n_gh, t_gh = make()
    g_dev = GraphedTrainStep(n_gd, t_gd, warmup=2)
    g_host = GraphedTrainStep(n_gh, t_gh, warmup=2)
    host_sched = LRSchedule.cosine(total, warmup_steps=500)
    calls = [0]

    def graph_host():
        for grp, base in zip(t_gh.param_groups, (2e-4, 1e-4)):       # the parent's way: a new host lr before every call
            grp["lr"] = base * host_sched.factor(calls[0])
        calls[0] += 1
        g_host(x, classes, boxes)
    forms = {"eager_off": (eager_fn(n_off, t_off), a.steps), "eager_sched_ema": (eager_fn(n_on, t_on), a.steps),
             "graph_device_table": (lambda: g_dev(x, classes, boxes), a.steps), "graph_host_lr": (graph_host, max(2, a.steps // 3))}
    for fn, _ in forms.values():
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    graph0 = g_dev.graph
    host = {k: [] for k in forms}
    devt = {k: [] for k in forms}
    mhz = {k: [] for k in forms}
    for _ in range(a.windows):
        for name, (fn, k) in forms.items():
            fn()
            torch.cuda.synchronize()
            # host time: three calls into an idle queue (the graph step's staging ring lets the host run four steps ahead; beyond
            # that a call waits for the device and measures the device)
            t0 = time.perf_counter()
            for _ in range(HOST_CALLS):
                fn()
            host[name].append((time.perf_counter() - t0) / HOST_CALLS * 1e3)
            torch.cuda.synchronize()
            pa = ops.clock_probe(dev)
            t0 = time.perf_counter()
            for _ in range(k):
                fn()
            pb = ops.clock_probe(dev)
            torch.cuda.synchronize()
            devt[name].append((time.perf_counter() - t0) / k * 1e3)
            mhz[name].append(ops.shader_mhz(pa, pb))
    for name in forms:
        emit({"what": f"train_step_b32_f32_{name}", "host_ms": stats(host[name], 3), "device_ms": stats(devt[name], 3),
              "shader_mhz_median": mhz_of(mhz[name]), "windows": a.windows, "steps_per_window": forms[name][1],
              "host_calls_per_window": HOST_CALLS})
    emit({"what": "graph", "captured_once_under_the_schedule": g_dev.graph is graph0, "calls_of_graph_host_lr": calls[0],
          "kernel_nodes_with_schedule_and_ema": g_dev.kernel_nodes, "kernel_nodes_without": g_host.kernel_nodes,
          "final_step_count": int(t_gd.step_count), "final_lr_words": [float(v) for v in t_gd.current_lr]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-step", action="store_true", help="the kernels only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sched_ema_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sched_ema_bench needs the GPU: there is nothing to measure without one")
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
        json.dump({"tool": "tools/sched_ema_bench.py", "device": torch.cuda.get_device_name(0), "results": RESULTS}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

"""What the IoU / GIoU / DIoU / CIoU localisation terms cost in the MultiBox loss call, and that the two existing entries are the code
they were.

    python tools/box_loss_bench.py [--parent-lib PATH] [--windows 7] [--calls 200] [--out profiles/box_loss_bench.json]

Shape: batch 32, P = 8732 (SSD300's priors), C = 21 and C = 81 (one per kernel family), gradients on, norm_mode 1.  Paths, each the bare
C call on preallocated outputs (so that all of them carry the same host work):
    l1                        ssd_multibox_loss of this build
    iou, giou, diou, ciou     ssd_multibox_loss_box with loc_mode 1 .. 4 and no ignore regions
    ignore_2                  ssd_multibox_loss_ignore of this build, 2 ignore boxes per image ("iou", 0.5)
    parent, parent_ignore_2   the two existing entries of the library given by --parent-lib: libssd_gfx950.so built from the parent commit
                              (a worktree of it, `python -m objectdetection_ssd_amd.build` there), loaded beside this build's in the
                              same process
Interleaved in one process: every window times `calls` back-to-back calls of each path in turn between device events (three kernel
launches per call, the queue never empty: device time per call), medians over the windows, two clock probes around the whole run.
A measurement, not a bar: the tool reports what it finds and exits 0.  Prints one JSON line per measurement and writes all to --out.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from objectdetection_ssd_amd import Losses, _lib, ops  # noqa: E402

BS, P = 32, 8732
MODES = ("iou", "giou", "diou", "ciou")
RESULTS = []


def emit(d):
    RESULTS.append(d)
    print(json.dumps(d), flush=True)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def stats(v, digits=2):
    return {"median": round(median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "spread": round(max(v) - min(v), digits)}


def bind(path):
    """the parent's library with this build's bindings of the entries it has"""
    lib = ctypes.CDLL(path)
    for name in ("ssd_multibox_loss_workspace", "ssd_multibox_loss", "ssd_multibox_loss_ignore"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def boxes(rng, n):
    c = rng.random((n, 2), dtype=np.float32) * np.float32(0.6) + np.float32(0.2)
    s = rng.random((n, 2), dtype=np.float32) * np.float32(0.4) + np.float32(0.05)
    return np.concatenate([c - s / 2, c + s / 2], 1).astype(np.float32)


def paths_for(C, dev, parent):
    rng = np.random.default_rng(C)
    counts = rng.integers(1, 9, BS)
    gt = torch.tensor(boxes(rng, int(counts.sum()))).to(dev)
    cls = torch.tensor(rng.integers(0, C - 1, int(counts.sum())).astype(np.float32)).to(dev)
    start = torch.tensor(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(dev)
    ign2 = torch.tensor(boxes(rng, 2 * BS)).to(dev)
    start2 = torch.arange(0, 2 * BS + 1, 2, dtype=torch.int32).to(dev)
    g = torch.Generator().manual_seed(C)
    loc = torch.randn(BS, P, 4, generator=g).to(dev)
    conf = (torch.randn(BS, P, C, generator=g) * 2).to(dev)
    pri, pri_xyxy = Losses._priors_on(dev, P)
    n_gt = gt.shape[0]
    lib = _lib.load()
    ws = torch.empty(lib.ssd_multibox_loss_box_workspace(BS, P, n_gt, 2 * BS), dtype=torch.uint8, device=dev)
    losses, obj, cl = torch.empty(3, device=dev), torch.empty((BS, P), dtype=torch.int32, device=dev), torch.empty((BS, P), dtype=torch.int32, device=dev)
    ign, dloc, dconf = torch.empty((BS, P), dtype=torch.uint8, device=dev), torch.empty_like(loc), torch.empty_like(conf)
    stream = torch.cuda.current_stream().cuda_stream
    head = (loc.data_ptr(), conf.data_ptr(), gt.data_ptr(), cls.data_ptr(), start.data_ptr(), BS, n_gt, pri.data_ptr(), pri_xyxy.data_ptr(), P, C,
            Losses.IOU_THRESHOLD, Losses.NEG_POS_RATIO, 1)
    tail = (dloc.data_ptr(), dconf.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    out = (losses.data_ptr(), obj.data_ptr(), cl.data_ptr())

    def plain(which):
        return lambda: _lib.check(which.ssd_multibox_loss(*head, *out, *tail), "multibox_loss")

    def ignore(which):
        return lambda: _lib.check(which.ssd_multibox_loss_ignore(*head, ign2.data_ptr(), start2.data_ptr(), 2 * BS, 0.5, 0, *out, ign.data_ptr(), *tail),
                                  "multibox_loss_ignore")

    def box(mode):
        return lambda: _lib.check(lib.ssd_multibox_loss_box(*head, None, None, 0, 0.5, 0, mode, *out, None, *tail), "multibox_loss_box")
    forms = {"l1": plain(lib)}
    forms.update({name: box(ops.loc_loss_mode(name)) for name in MODES})
    forms["ignore_2"] = ignore(lib)
    if parent is not None:
        assert parent.ssd_multibox_loss_workspace(BS, P, n_gt) <= ws.numel()
        forms["parent"] = plain(parent)
        forms["parent_ignore_2"] = ignore(parent)
    keep = (gt, cls, start, ign2, start2, loc, conf, ws, losses, obj, cl, ign, dloc, dconf)
    return forms, keep, lambda: (losses.clone(), dloc.clone(), dconf.clone())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libssd_gfx950.so built from the parent commit")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "box_loss_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("box_loss_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    parent = bind(a.parent_lib) if a.parent_lib else None
    torch.cuda.synchronize()
    pa = ops.clock_probe(dev)
    for C in (21, 81):
        forms, keep, read = paths_for(C, dev, parent)
        seen = {}
        for name, fn in forms.items():                       # the results each path leaves (the same inputs)
            fn()
            torch.cuda.synchronize()
            seen[name] = read()
        us = {k: [] for k in forms}
        for _ in range(a.windows):
            for name, fn in forms.items():
                for _ in range(10):
                    fn()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    fn()
                e1.record()
                e1.synchronize()
                us[name].append(e0.elapsed_time(e1) * 1e3 / a.calls)
        for name in forms:
            emit({"what": f"loss_call_C{C}_{name}", "batch": BS, "priors": P, "classes": C, "us_per_call": stats(us[name]),
                  "windows": a.windows, "calls_per_window": a.calls})
        cmp = {"what": f"comparison_C{C}", "positives": int(seen["l1"][0][2].item()), "l1_window_spread_us": round(max(us["l1"]) - min(us["l1"]), 2)}
        for name in MODES:
            cmp[f"{name}_minus_l1_us"] = round(median(us[name]) - median(us["l1"]), 2)
            cmp[f"{name}_conf_side_bit_equal_l1"] = bool(torch.equal(seen[name][0][1:], seen["l1"][0][1:]) and torch.equal(seen[name][2], seen["l1"][2]))
        if parent is not None:
            for mine, theirs in (("l1", "parent"), ("ignore_2", "parent_ignore_2")):
                cmp[f"{mine}_minus_{theirs}_us"] = round(median(us[mine]) - median(us[theirs]), 2)
                cmp[f"{theirs}_window_spread_us"] = round(max(us[theirs]) - min(us[theirs]), 2)
                cmp[f"{mine}_bit_equal_{theirs}"] = all(bool(torch.equal(x, y)) for x, y in zip(seen[mine], seen[theirs]))
        else:
            cmp["against_parent"] = "not measured"
        emit(cmp)
    pb = ops.clock_probe(dev)
    torch.cuda.synchronize()
    clock = ops.shader_mhz(pa, pb)
    emit({"what": "clock", "shader_mhz_average_over_the_run": None if clock != clock else round(clock)})
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/box_loss_bench.py", "device": torch.cuda.get_device_name(0), "parent_lib": bool(a.parent_lib),
                   "results": RESULTS}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

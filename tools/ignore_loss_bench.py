"""What the ignore regions cost in the MultiBox loss call, and that the plain entry is the code it was.

    python tools/ignore_loss_bench.py [--parent-lib PATH] [--windows 9] [--calls 200] [--out profiles/ignore_loss_bench.json]

Shape: batch 32, P = 8732 (SSD300's priors), C = 21 and C = 81 (one per kernel family), gradients on, norm_mode 1.  Paths, each the
bare C call on preallocated outputs (so that all of them carry the same host work):
    existing        ssd_multibox_loss of this build
    ignore_0        ssd_multibox_loss_ignore with no ignore box in any image
    ignore_2        ssd_multibox_loss_ignore with 2 ignore boxes per image ("iou", 0.5)
    parent          ssd_multibox_loss of the library given by --parent-lib: libssd_gfx950.so built from the parent commit (a worktree
                    of it, `python -m objectdetection_ssd_amd.build` there), loaded beside this build's in the same process
Interleaved in one process: every window times `calls` back-to-back calls of each path in turn between device events (three kernel
launches per call, the queue never empty: device time per call), medians over the windows, two clock probes around the whole run.
Held: the existing entry is not slower than the parent's by more than the spread (max - min) of the parent's own windows; the tool
exits 1 if it is.  Prints one JSON line per measurement and writes all of them to --out.
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
    """the parent's library with this build's bindings of the two entries it has"""
    lib = ctypes.CDLL(path)
    for name in ("ssd_multibox_loss_workspace", "ssd_multibox_loss"):
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
    start0 = torch.zeros(BS + 1, dtype=torch.int32).to(dev)
    g = torch.Generator().manual_seed(C)
    loc = torch.randn(BS, P, 4, generator=g).to(dev)
    conf = (torch.randn(BS, P, C, generator=g) * 2).to(dev)
    pri, pri_xyxy = Losses._priors_on(dev, P)
    n_gt = gt.shape[0]
    lib = _lib.load()
    ws = torch.empty(lib.ssd_multibox_loss_ignore_workspace(BS, P, n_gt, 2 * BS), dtype=torch.uint8, device=dev)
    losses, obj, cl = torch.empty(3, device=dev), torch.empty((BS, P), dtype=torch.int32, device=dev), torch.empty((BS, P), dtype=torch.int32, device=dev)
    ign, dloc, dconf = torch.empty((BS, P), dtype=torch.uint8, device=dev), torch.empty_like(loc), torch.empty_like(conf)
    stream = torch.cuda.current_stream().cuda_stream
    head = (loc.data_ptr(), conf.data_ptr(), gt.data_ptr(), cls.data_ptr(), start.data_ptr(), BS, n_gt, pri.data_ptr(), pri_xyxy.data_ptr(), P, C,
            Losses.IOU_THRESHOLD, Losses.NEG_POS_RATIO, 1)
    tail = (dloc.data_ptr(), dconf.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    out = (losses.data_ptr(), obj.data_ptr(), cl.data_ptr())

    def plain(which):
        return lambda: _lib.check(which.ssd_multibox_loss(*head, *out, *tail), "multibox_loss")

    def ignore(b, st, n):
        return lambda: _lib.check(lib.ssd_multibox_loss_ignore(*head, b, st.data_ptr(), n, 0.5, 0, *out, ign.data_ptr(), *tail), "multibox_loss_ignore")
    forms = {"existing": plain(lib), "ignore_0": ignore(None, start0, 0), "ignore_2": ignore(ign2.data_ptr(), start2, 2 * BS)}
    if parent is not None:
        assert parent.ssd_multibox_loss_workspace(BS, P, n_gt) <= ws.numel()
        forms["parent"] = plain(parent)
    keep = (gt, cls, start, ign2, start2, start0, loc, conf, ws, losses, obj, cl, ign, dloc, dconf)
    return forms, keep, lambda: (losses.clone(), ign.sum().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libssd_gfx950.so built from the parent commit")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ignore_loss_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ignore_loss_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    parent = bind(a.parent_lib) if a.parent_lib else None
    held = True
    torch.cuda.synchronize()
    pa = ops.clock_probe(dev)
    for C in (21, 81):
        forms, keep, read = paths_for(C, dev, parent)
        seen = {}
        for name, fn in forms.items():                       # the results each path leaves (the same inputs)
            fn()
            torch.cuda.synchronize()
            seen[name] = read()
        same = [torch.equal(seen["existing"][0], seen[k][0]) for k in ("ignore_0", "parent") if k in seen]
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
        cmp = {"what": f"comparison_C{C}", "ignore_0_minus_existing_us": round(median(us["ignore_0"]) - median(us["existing"]), 2),
               "ignore_2_minus_existing_us": round(median(us["ignore_2"]) - median(us["existing"]), 2),
               "ignored_priors_with_2_boxes_per_image": seen["ignore_2"][1], "losses_bit_equal_existing_ignore_0_parent": all(same)}
        if parent is not None:
            diff, spread = median(us["existing"]) - median(us["parent"]), max(us["parent"]) - min(us["parent"])
            ok = diff <= spread
            held = held and ok
            cmp.update(existing_minus_parent_us=round(diff, 2), parent_window_spread_us=round(spread, 2), existing_not_slower_than_parent=ok)
        else:
            cmp.update(existing_minus_parent_us="not measured")
        emit(cmp)
    pb = ops.clock_probe(dev)
    torch.cuda.synchronize()
    clock = ops.shader_mhz(pa, pb)
    emit({"what": "clock", "shader_mhz_average_over_the_run": None if clock != clock else round(clock)})
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/ignore_loss_bench.py", "device": torch.cuda.get_device_name(0), "parent_lib": bool(a.parent_lib),
                   "results": RESULTS}, f, indent=1)
        f.write("\n")
    if not held:
        raise SystemExit("the existing entry is slower than the parent's by more than the parent's own spread")


if __name__ == "__main__":
    main()

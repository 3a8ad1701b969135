"""What ATSS matching costs in the MultiBox loss call, and that the existing entries are the code they were.

    python tools/atss_bench.py [--parent-lib PATH] [--windows 7] [--calls 200] [--out profiles/atss_bench.json]

Shape: batch 32, P = 8732 (SSD300's priors), C = 21 and C = 81, gradients on, norm_mode 1, 1 .. 8 boxes per image.  Paths, each the bare
C call on preallocated outputs (so that all of them carry the same host work), interleaved in one process:
    ce, ce_ignore_2, ce_ciou      ssd_multibox_loss, ssd_multibox_loss_ignore (2 ignore boxes per image), ssd_multibox_loss_box (CIoU)
    iou_ce, iou_focal             ssd_multibox_loss_atss with match_mode 0: cross entropy and the focal term (alpha 0.25, gamma 2)
    atss_ce, atss_focal           the same with match_mode 1, topk 9
    atss_assign                   ssd_atss_assign: the key memset, the assignment pass and the unpack pass alone
    parent, parent_ignore_2, parent_ciou   the three existing entries of the library given by --parent-lib (libssd_gfx950.so built from
                                  the parent commit), loaded beside this build's in the same process
Every window times `calls` back-to-back calls of each path in turn between device events, with a clock probe in front of and behind
it (outside the events): medians over the windows, and each path's shader clock inside its own windows where the probes give one (on
windows of a few milliseconds their 100 MHz ticks often give none: it is then recorded as unknown).  A measurement, not a bar: the
tool reports what it finds and exits 0.  Prints one JSON line per measurement and writes all to --out.
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
from objectdetection_ssd_amd import Losses, Util, _lib, ops  # noqa: E402

BS, P, TOPK = 32, 8732, 9
ALPHA, GAMMA = 0.25, 2.0
RESULTS = []
MHZ = {}        # path -> shader clock of each of its timed windows


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
    for name in ("ssd_multibox_loss_workspace", "ssd_multibox_loss", "ssd_multibox_loss_ignore", "ssd_multibox_loss_box"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def boxes(rng, n):
    c = rng.random((n, 2), dtype=np.float32) * np.float32(0.6) + np.float32(0.2)
    s = rng.random((n, 2), dtype=np.float32) * np.float32(0.4) + np.float32(0.05)
    return np.concatenate([c - s / 2, c + s / 2], 1).astype(np.float32)


def time_forms(forms, windows, calls):
    us = {k: [] for k in forms}
    dev = torch.device("cuda:0")
    for _ in range(windows):
        for name, fn in forms.items():
            for _ in range(min(10, calls)):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            pa = ops.clock_probe(dev)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            pb = ops.clock_probe(dev)
            e1.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / calls)
            MHZ.setdefault(name, []).append(ops.shader_mhz(pa, pb))
    return us


def window_mhz(names):
    """median shader clock over the timed windows of these paths ("unknown" where no probe pair landed)"""
    v = [x for n in names for x in MHZ.get(n, []) if x == x]
    return round(median(v)) if v else "unknown"


def loss_paths(C, dev, parent):
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
    ws = torch.empty(lib.ssd_multibox_loss_atss_workspace(BS, P, n_gt, 2 * BS), dtype=torch.uint8, device=dev)
    losses, obj, cl = torch.empty(3, device=dev), torch.empty((BS, P), dtype=torch.int32, device=dev), torch.empty((BS, P), dtype=torch.int32, device=dev)
    ign, dloc, dconf = torch.empty((BS, P), dtype=torch.uint8, device=dev), torch.empty_like(loc), torch.empty_like(conf)
    stream = torch.cuda.current_stream().cuda_stream
    head = (loc.data_ptr(), conf.data_ptr(), gt.data_ptr(), cls.data_ptr(), start.data_ptr(), BS, n_gt, pri.data_ptr(), pri_xyxy.data_ptr(), P, C,
            Losses.IOU_THRESHOLD, Losses.NEG_POS_RATIO, 1)
    tail = (dloc.data_ptr(), dconf.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    out = (losses.data_ptr(), obj.data_ptr(), cl.data_ptr())
    none = (None, None, 0, 0.5, 0)
    cells, anchors = ops.atss_levels(Util.prior_levels(P), P)

    def plain(which):
        return lambda: _lib.check(which.ssd_multibox_loss(*head, *out, *tail), "multibox_loss")

    def ignore(which):
        return lambda: _lib.check(which.ssd_multibox_loss_ignore(*head, ign2.data_ptr(), start2.data_ptr(), 2 * BS, 0.5, 0, *out, ign.data_ptr(), *tail),
                                  "multibox_loss_ignore")

    def ciou(which):
        return lambda: _lib.check(which.ssd_multibox_loss_box(*head, *none, 4, *out, None, *tail), "multibox_loss_box")

    def atss(conf_mode, match_mode):
        return lambda: _lib.check(lib.ssd_multibox_loss_atss(*head, *none, 0, conf_mode, ALPHA, GAMMA, match_mode, TOPK, len(cells), cells, anchors,
                                                             *out, None, *tail), "multibox_loss_atss")

    aws = torch.empty(lib.ssd_atss_assign_workspace(BS, P), dtype=torch.uint8, device=dev)
    assign = torch.empty((BS, P), dtype=torch.int32, device=dev)

    def assign_alone():
        _lib.check(lib.ssd_atss_assign(gt.data_ptr(), start.data_ptr(), BS, n_gt, pri.data_ptr(), pri_xyxy.data_ptr(), P, TOPK, len(cells), cells,
                                       anchors, assign.data_ptr(), None, None, None, None, aws.data_ptr(), aws.numel(), stream), "atss_assign")

    forms = {}
    if parent is not None:                                   # each existing entry next to the parent's, this build's first
        assert parent.ssd_multibox_loss_workspace(BS, P, n_gt) <= ws.numel()
        forms.update(ce=plain(lib), parent=plain(parent), ce_ignore_2=ignore(lib), parent_ignore_2=ignore(parent), ce_ciou=ciou(lib),
                     parent_ciou=ciou(parent))
    else:
        forms.update(ce=plain(lib), ce_ignore_2=ignore(lib), ce_ciou=ciou(lib))
    forms.update(iou_ce=atss(0, 0), atss_ce=atss(0, 1), iou_focal=atss(1, 0), atss_focal=atss(1, 1), atss_assign=assign_alone)
    keep = (gt, cls, start, ign2, start2, loc, conf, ws, losses, obj, cl, ign, dloc, dconf, aws, assign, cells, anchors)
    return forms, keep, lambda: (losses.clone(), dloc.clone(), dconf.clone(), cl.clone()), n_gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libssd_gfx950.so built from the parent commit")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "atss_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("atss_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    parent = bind(a.parent_lib) if a.parent_lib else None
    torch.cuda.synchronize()
    pa = ops.clock_probe(dev)
    for C in (21, 81):
        forms, keep, read, n_gt = loss_paths(C, dev, parent)
        seen = {}
        for name, fn in forms.items():                       # the results each path leaves (the same inputs)
            fn()
            torch.cuda.synchronize()
            seen[name] = read()
        us = time_forms(forms, a.windows, a.calls)
        for name in forms:
            emit({"what": f"loss_call_C{C}_{name}", "batch": BS, "priors": P, "classes": C, "boxes": n_gt, "us_per_call": stats(us[name]),
                  "shader_mhz_in_the_windows": window_mhz([name]), "windows": a.windows, "calls_per_window": a.calls})
        MHZ.clear()
        cmp = {"what": f"comparison_C{C}", "positives_iou": int(seen["iou_ce"][0][2].item()), "positives_atss": int(seen["atss_ce"][0][2].item()),
               "atss_minus_iou_ce_us": round(median(us["atss_ce"]) - median(us["iou_ce"]), 2),
               "atss_minus_iou_focal_us": round(median(us["atss_focal"]) - median(us["iou_focal"]), 2),
               "iou_ce_window_spread_us": round(max(us["iou_ce"]) - min(us["iou_ce"]), 2),
               "iou_focal_window_spread_us": round(max(us["iou_focal"]) - min(us["iou_focal"]), 2),
               "match_mode_0_bit_equal_ce": all(bool(torch.equal(x, y)) for x, y in zip(seen["iou_ce"], seen["ce"])),
               "atss_ce_and_atss_focal_same_classes": bool(torch.equal(seen["atss_ce"][3], seen["atss_focal"][3]))}
        if parent is not None:
            for mine, theirs in (("ce", "parent"), ("ce_ignore_2", "parent_ignore_2"), ("ce_ciou", "parent_ciou")):
                cmp[f"{mine}_minus_{theirs}_us"] = round(median(us[mine]) - median(us[theirs]), 2)
                cmp[f"{theirs}_window_spread_us"] = round(max(us[theirs]) - min(us[theirs]), 2)
                cmp[f"{mine}_bit_equal_{theirs}"] = all(bool(torch.equal(x, y)) for x, y in zip(seen[mine][:3], seen[theirs][:3]))
        else:
            cmp["against_parent"] = "not measured"
        emit(cmp)
        del forms, keep, read, seen
        torch.cuda.empty_cache()
    pb = ops.clock_probe(dev)
    torch.cuda.synchronize()
    clock = ops.shader_mhz(pa, pb)
    emit({"what": "clock", "shader_mhz_average_over_the_run_host_set_up_included": "unknown" if clock != clock else round(clock)})
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/atss_bench.py", "device": torch.cuda.get_device_name(0), "parent_lib": bool(a.parent_lib),
                   "results": RESULTS}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

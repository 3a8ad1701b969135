"""What the sigmoid focal classification term costs in the MultiBox loss call, in the decode and in the train step, and that the existing
entries are the code they were.

    python tools/focal_loss_bench.py [--parent-lib PATH] [--windows 7] [--calls 200] [--skip-train] [--out profiles/focal_loss_bench.json]

Shape: batch 32, P = 8732 (SSD300's priors), C = 21 and C = 81, gradients on, norm_mode 1.  Paths, each the bare C call on preallocated
outputs (so that all of them carry the same host work), interleaved in one process:
    ce, ce_ignore_2, ce_ciou      ssd_multibox_loss, ssd_multibox_loss_ignore (2 ignore boxes per image), ssd_multibox_loss_box (CIoU)
    focal                         ssd_multibox_loss_focal, conf_mode 1, alpha 0.25, gamma 2 (five launches)
    focal_dense                   ssd_focal_dense: the dense pass and its sum alone, on the classes the focal call left
    copy                          Tensor.copy_ of conf into dconf: the same bytes read and written as the dense pass, with no arithmetic;
                                  at 23.5 MB (C = 21) the tensors sit in the Infinity Cache, so this is the ceiling, not the HBM rate
    parent, parent_ignore_2, parent_ciou   the three existing entries of the library given by --parent-lib (libssd_gfx950.so built from
                                  the parent commit), loaded beside this build's in the same process
    decode_softmax, decode_sigmoid, parent_decode   ssd_decode_nms_batch, ssd_decode_nms_batch_score (score_mode 1) on logits shifted
                                  so that both make about as many candidates, and the parent's ssd_decode_nms_batch
Every window times `calls` back-to-back calls of each path in turn between device events, with a clock probe in front of and behind
it (outside the events): medians over the windows, and each path's shader clock inside its own windows (on windows of a few
milliseconds the probes' 100 MHz ticks give figures that say nothing; they are kept as measured).  The train step (SSD300, batch 32, f32, eager: forward, Losses.ssd, backward, fused SGD) is timed with and without
the focal term, windows of 3 steps.  A measurement, not a bar: the tool reports what it finds and exits 0.  Prints one JSON line per
measurement and writes all to --out.
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
ALPHA, GAMMA = 0.25, 2.0
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
    for name in ("ssd_multibox_loss_workspace", "ssd_multibox_loss", "ssd_multibox_loss_ignore", "ssd_multibox_loss_box",
                 "ssd_decode_nms_batch_workspace", "ssd_decode_nms_batch"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return lib


def boxes(rng, n):
    c = rng.random((n, 2), dtype=np.float32) * np.float32(0.6) + np.float32(0.2)
    s = rng.random((n, 2), dtype=np.float32) * np.float32(0.4) + np.float32(0.05)
    return np.concatenate([c - s / 2, c + s / 2], 1).astype(np.float32)


MHZ = {}        # path -> shader clock of each of its timed windows (a clock probe in front of and behind the window, outside the events)


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
    """median shader clock over the timed windows of these paths (None where no probe pair landed)"""
    v = [x for n in names for x in MHZ.get(n, []) if x == x]
    return round(median(v)) if v else None


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
    ws = torch.empty(lib.ssd_multibox_loss_focal_workspace(BS, P, n_gt, 2 * BS), dtype=torch.uint8, device=dev)
    losses, obj, cl = torch.empty(3, device=dev), torch.empty((BS, P), dtype=torch.int32, device=dev), torch.empty((BS, P), dtype=torch.int32, device=dev)
    ign, dloc, dconf = torch.empty((BS, P), dtype=torch.uint8, device=dev), torch.empty_like(loc), torch.empty_like(conf)
    stream = torch.cuda.current_stream().cuda_stream
    head = (loc.data_ptr(), conf.data_ptr(), gt.data_ptr(), cls.data_ptr(), start.data_ptr(), BS, n_gt, pri.data_ptr(), pri_xyxy.data_ptr(), P, C,
            Losses.IOU_THRESHOLD, Losses.NEG_POS_RATIO, 1)
    tail = (dloc.data_ptr(), dconf.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    out = (losses.data_ptr(), obj.data_ptr(), cl.data_ptr())
    none = (None, None, 0, 0.5, 0)

    def plain(which):
        return lambda: _lib.check(which.ssd_multibox_loss(*head, *out, *tail), "multibox_loss")

    def ignore(which):
        return lambda: _lib.check(which.ssd_multibox_loss_ignore(*head, ign2.data_ptr(), start2.data_ptr(), 2 * BS, 0.5, 0, *out, ign.data_ptr(), *tail),
                                  "multibox_loss_ignore")

    def ciou(which):
        return lambda: _lib.check(which.ssd_multibox_loss_box(*head, *none, 4, *out, None, *tail), "multibox_loss_box")

    def focal():
        _lib.check(lib.ssd_multibox_loss_focal(*head, *none, 0, 1, ALPHA, GAMMA, *out, None, *tail), "multibox_loss_focal")

    focal()
    torch.cuda.synchronize()
    n_pos = float(losses[2].item())
    cls_focal = cl.clone()
    dws = torch.empty(lib.ssd_focal_dense_workspace(BS, P), dtype=torch.uint8, device=dev)
    one = torch.empty(1, device=dev)

    def dense():
        _lib.check(lib.ssd_focal_dense(conf.data_ptr(), cls_focal.data_ptr(), None, BS, P, C, n_pos, 1, ALPHA, GAMMA, one.data_ptr(), dconf.data_ptr(),
                                       dws.data_ptr(), dws.numel(), stream), "focal_dense")

    forms = {}
    if parent is not None:                                   # each existing entry next to the parent's, this build's first
        assert parent.ssd_multibox_loss_workspace(BS, P, n_gt) <= ws.numel()
        forms.update(ce=plain(lib), parent=plain(parent), ce_ignore_2=ignore(lib), parent_ignore_2=ignore(parent), ce_ciou=ciou(lib),
                     parent_ciou=ciou(parent))
    else:
        forms.update(ce=plain(lib), ce_ignore_2=ignore(lib), ce_ciou=ciou(lib))
    forms.update(focal=focal, focal_dense=dense, copy=lambda: dconf.copy_(conf))
    keep = (gt, cls, start, ign2, start2, loc, conf, ws, losses, obj, cl, ign, dloc, dconf, cls_focal, dws, one)
    return forms, keep, lambda: (losses.clone(), dloc.clone(), dconf.clone(), one.clone())


def decode_paths(C, dev, parent):
    """logits N(-3, 4) in the foreground columns, N(1, 1) in the background column.  The two scores make different candidate sets from
    the same logits and everything behind D1 costs by the candidate, so the sigmoid decode reads the same logits with the foreground
    columns shifted by one constant, chosen so that as large a share of its scores reaches 0.2 as of the softmax scores: the
    difference that is left is the score arithmetic.  The shares are returned for the record."""
    g = torch.Generator().manual_seed(100 + C)
    l = (torch.randn(BS, P, 4, generator=g) * 0.5).to(dev)
    c = (torch.randn(BS, P, C, generator=g) * 2 - 3)
    c[..., -1] = torch.randn(BS, P, generator=g) + 1
    share = float((torch.softmax(c, -1)[..., :-1] >= 0.2).float().mean())
    fg = c[..., :-1].reshape(-1)
    cut = float(torch.kthvalue(fg, max(1, int(round((1 - share) * fg.numel())))).values)
    c_sig = c.clone()
    c_sig[..., :-1] += -1.3862943611198906 - cut                 # sigmoid(x) >= 0.2 from x = log(0.2 / 0.8) on
    shares = {"decode_softmax": share, "parent_decode": share, "decode_sigmoid": float((torch.sigmoid(c_sig[..., :-1]) >= 0.2).float().mean())}
    c, c_sig = c.to(dev), c_sig.to(dev)
    pri, _ = Losses._priors_on(dev, P)
    wh = torch.full((BS, 2), 300.0, device=dev)
    lib = _lib.load()
    top_k = 200
    ws = torch.empty(lib.ssd_decode_nms_batch_workspace(BS, P, C), dtype=torch.uint8, device=dev)
    o = (torch.zeros((BS, top_k, 4), device=dev), torch.zeros((BS, top_k), device=dev, dtype=torch.int64), torch.zeros((BS, top_k), device=dev),
         torch.zeros((BS, top_k), device=dev, dtype=torch.int32), torch.zeros((BS,), device=dev, dtype=torch.int32))
    stream = torch.cuda.current_stream().cuda_stream
    tail = (pri.data_ptr(), wh.data_ptr(), BS, P, C, 0.2, 0.45, top_k, *[t.data_ptr() for t in o], ws.data_ptr(), ws.numel(), stream)
    args, args_sig = (l.data_ptr(), c.data_ptr(), *tail), (l.data_ptr(), c_sig.data_ptr(), *tail)
    forms = {"decode_softmax": lambda: _lib.check(lib.ssd_decode_nms_batch(*args), "decode_nms_batch")}
    if parent is not None:
        forms["parent_decode"] = lambda: _lib.check(parent.ssd_decode_nms_batch(*args), "decode_nms_batch")
    forms["decode_sigmoid"] = lambda: _lib.check(lib.ssd_decode_nms_batch_score(*args_sig, 0, 0.5, 0.2, 1), "decode_nms_batch_score")
    return forms, (l, c, c_sig, wh, ws, o, shares), lambda: tuple(t.clone() for t in o)


def train_steps(dev, windows):
    """forward, Losses.ssd, backward and the fused SGD step of SSD300 at batch 32 in f32, eager, with the cross entropy and with the
    focal term, on two nets of the same weights, interleaved; ms per step over windows of 3 steps"""
    from objectdetection_ssd_amd import Model
    from objectdetection_ssd_amd.optim import SGD
    rng = np.random.default_rng(7)
    x = torch.randn(BS, 3, 300, 300, generator=torch.Generator().manual_seed(7)).to(dev)
    counts = rng.integers(1, 9, BS)
    bx = [torch.tensor(boxes(rng, int(n))).to(dev) for n in counts]
    cl = [torch.tensor(rng.integers(0, 20, int(n)).astype(np.float32)).to(dev) for n in counts]
    runs = {}
    for name, kw in (("train_step_ce", {}), ("train_step_focal", dict(conf_loss="focal", focal_alpha=ALPHA, focal_gamma=GAMMA))):
        torch.manual_seed(0)
        net = Model.SSD_300()
        if kw:
            net.init_conf_prior()
        net = net.to(dev).train()
        opt = SGD(params=[{"params": list(net.parameters())}], lr=1e-4, momentum=0.9, weight_decay=5e-4)

        def step(net=net, opt=opt, kw=kw):
            opt.zero_grad()
            l1, l2 = Losses.ssd(net(x), cl, bx, **kw)
            (l1 + l2).backward()
            opt.step()
        runs[name] = step
    ms = {k: [v / 1e3 for v in w] for k, w in time_forms(runs, windows, 3).items()}
    for name in runs:
        emit({"what": name, "batch": BS, "dtype": "f32", "ms_per_step": stats(ms[name], 3), "shader_mhz_in_the_windows": window_mhz([name]),
              "windows": windows, "steps_per_window": 3})
    emit({"what": "train_step_comparison", "focal_minus_ce_ms": round(median(ms["train_step_focal"]) - median(ms["train_step_ce"]), 3),
          "ce_window_spread_ms": round(max(ms["train_step_ce"]) - min(ms["train_step_ce"]), 3)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libssd_gfx950.so built from the parent commit")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "focal_loss_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("focal_loss_bench needs the GPU: there is nothing to measure without one")
    dev = torch.device("cuda:0")
    parent = bind(a.parent_lib) if a.parent_lib else None
    torch.cuda.synchronize()
    pa = ops.clock_probe(dev)
    for C in (21, 81):
        forms, keep, read = loss_paths(C, dev, parent)
        seen = {}
        for name, fn in forms.items():                       # the results each path leaves (the same inputs)
            fn()
            torch.cuda.synchronize()
            seen[name] = read()
        us = time_forms(forms, a.windows, a.calls)
        for name in forms:
            emit({"what": f"loss_call_C{C}_{name}", "batch": BS, "priors": P, "classes": C, "us_per_call": stats(us[name]),
                  "shader_mhz_in_the_windows": window_mhz([name]), "windows": a.windows, "calls_per_window": a.calls})
        MHZ.clear()
        mb = BS * P * C * 4 / 1e6
        cmp = {"what": f"comparison_C{C}", "positives": int(seen["ce"][0][2].item()), "conf_megabytes": round(mb, 2),
               "focal_minus_ce_us": round(median(us["focal"]) - median(us["ce"]), 2), "ce_window_spread_us": round(max(us["ce"]) - min(us["ce"]), 2),
               "focal_dense_gb_per_s": round(2 * mb / median(us["focal_dense"]) * 1e3, 1), "copy_gb_per_s": round(2 * mb / median(us["copy"]) * 1e3, 1),
               "focal_dense_over_copy": round(median(us["focal_dense"]) / median(us["copy"]), 3),
               "focal_loc_side_bit_equal_ce": bool(torch.equal(seen["focal"][0][[0, 2]], seen["ce"][0][[0, 2]]) and torch.equal(seen["focal"][1], seen["ce"][1])),
               "focal_dense_bit_equal_focal": bool(torch.equal(seen["focal_dense"][2], seen["focal"][2]) and
                                                   torch.equal(seen["focal_dense"][3][0], seen["focal"][0][1]))}
        if parent is not None:
            for mine, theirs in (("ce", "parent"), ("ce_ignore_2", "parent_ignore_2"), ("ce_ciou", "parent_ciou")):
                cmp[f"{mine}_minus_{theirs}_us"] = round(median(us[mine]) - median(us[theirs]), 2)
                cmp[f"{theirs}_window_spread_us"] = round(max(us[theirs]) - min(us[theirs]), 2)
                cmp[f"{mine}_bit_equal_{theirs}"] = all(bool(torch.equal(x, y)) for x, y in zip(seen[mine][:3], seen[theirs][:3]))
        else:
            cmp["against_parent"] = "not measured"
        emit(cmp)
        del forms, keep, read, seen
        forms, keep, read = decode_paths(C, dev, parent)
        seen = {}
        for name, fn in forms.items():
            fn()
            torch.cuda.synchronize()
            seen[name] = read()
        us = time_forms(forms, a.windows, max(1, a.calls // 4))
        for name in forms:
            emit({"what": f"decode_C{C}_{name}", "batch": BS, "priors": P, "classes": C, "us_per_call": stats(us[name]),
                  "shader_mhz_in_the_windows": window_mhz([name]), "detections": int(seen[name][4].sum().item()), "share_of_scores_that_are_candidates": round(keep[-1][name], 5), "windows": a.windows, "calls_per_window": max(1, a.calls // 4)})
        cmp = {"what": f"decode_comparison_C{C}", "sigmoid_minus_softmax_us": round(median(us["decode_sigmoid"]) - median(us["decode_softmax"]), 2),
               "softmax_window_spread_us": round(max(us["decode_softmax"]) - min(us["decode_softmax"]), 2),
               "note": "the sigmoid decode reads the same logits shifted so that as many scores are candidates as with softmax"}
        if parent is not None:
            cmp["softmax_minus_parent_us"] = round(median(us["decode_softmax"]) - median(us["parent_decode"]), 2)
            cmp["parent_window_spread_us"] = round(max(us["parent_decode"]) - min(us["parent_decode"]), 2)
            cmp["softmax_bit_equal_parent"] = all(bool(torch.equal(x, y)) for x, y in zip(seen["decode_softmax"], seen["parent_decode"]))
        else:
            cmp["against_parent"] = "not measured"
        emit(cmp)
        MHZ.clear()
        del forms, keep, read, seen
        torch.cuda.empty_cache()
    if not a.skip_train:
        train_steps(dev, a.windows)
    pb = ops.clock_probe(dev)
    torch.cuda.synchronize()
    clock = ops.shader_mhz(pa, pb)
    emit({"what": "clock", "shader_mhz_average_over_the_run_host_set_up_included": None if clock != clock else round(clock)})
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/focal_loss_bench.py", "device": torch.cuda.get_device_name(0), "parent_lib": bool(a.parent_lib),
                   "results": RESULTS}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

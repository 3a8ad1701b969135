"""Shared by tests/test_gpu_path.py and tools/grad_bars.py: the gradient-distance measurements whose results are committed
as tests/golden/grad_bars.json (measured on an MI355X by tools/grad_bars.py) and then held as per-tensor bars by the tests
(bar = max(2 x measured, floor)).  TEST INFRASTRUCTURE: imports the oracle."""
import ctypes
import json
import os

import numpy as np
import torch

import ssd_oracle as O
from helpers import synth_gt

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARS_PATH = os.path.join(ROOT, "tests", "golden", "grad_bars.json")
FLOOR_REL = 2e-5          # relative-L2 distances below this are summation-order noise
FLOOR_NORM = 1e-5         # same for | ||g|| - ||ref|| | / ||ref||
ENGINES = ("wino", "direct")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def load_bars():
    with open(BARS_PATH) as f:
        return json.load(f)


def bar(table, metric, name, floor=FLOOR_REL):
    return max(2.0 * float(table[metric][name]), floor)


def set_engine(net, engine, conv_dtype="f32"):
    net.conv_dtype = conv_dtype
    net.winograd = engine == "wino"


def train_step(net, x, classes, boxes):
    """one forward + loss + backward on device tensors -> (loc, conf, l1, l2, {name: grad})"""
    from objectdetection_ssd_amd import Losses
    net.train()
    net.zero_grad()
    loc, conf = net(x)
    l1, l2 = Losses.ssd((loc, conf), classes, boxes)
    (l1 + l2).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
    return loc.detach(), conf.detach(), float(l1.item()), float(l2.item()), grads


def f64_case():
    """bs 2, one GT per prior scale so that all six maps carry positives"""
    x = np.random.default_rng(515).standard_normal((2, 3, 300, 300), dtype=np.float32)
    boxes = [np.array([[.05, .05, .95, .95], [.1, .3, .475, .675], [.40, .40, .50, .52]], np.float32),
             np.array([[.0, .1, .9, 1.], [.55, .5, .75, .7], [.2, .2, .75, .75], [.15, .1, .875, .825]], np.float32)]
    classes = [np.array([1., 5., 12.], np.float32), np.array([7., 0., 19., 3.], np.float32)]
    return x, boxes, classes


def f64_oracle_grads(params, operand_round=None, dtype=torch.float64, store_round=False):
    x, boxes, classes = f64_case()
    P = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in params.items()}
    loc, conf = O.ssd300_forward(torch.from_numpy(x).to(dtype), P, operand_round=operand_round, store_round=store_round)
    a1, a2 = O.multibox_loss_torch(loc, conf, [torch.from_numpy(b) for b in boxes], [torch.from_numpy(c) for c in classes])
    (a1 + a2).backward()
    return loc.detach(), conf.detach(), float(a1), float(a2), {k: v.grad.double() for k, v in P.items()}


def rel_l2(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


def gpu_f64_case(net):
    x, boxes, classes = f64_case()
    return train_step(net, _t(x), [_t(c) for c in classes], [_t(b) for b in boxes])


def golden_case(z):
    bs = int(z["bs"])
    x = np.random.default_rng(int(z["x_seed"])).standard_normal((bs, 3, 300, 300), dtype=np.float32)
    boxes, classes = synth_gt(np.random.default_rng(int(z["gt_seed"])), bs)
    return _t(x), [_t(c) for c in classes], [_t(b) for b in boxes]


def bench_batch(bs=32, seed=1234, hw=300):
    """bench.py's synth_batch; hw=512: its SSD512 batch (512 x 512 images from the same seed)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(bs, 3, hw, hw, generator=g)
    rng = np.random.default_rng(seed)
    boxes, classes = [], []
    for _ in range(bs):
        n = 1 + min(int(rng.poisson(1.4)), 7)
        x1 = rng.uniform(0, .6, n); y1 = rng.uniform(0, .6, n)
        w = rng.uniform(.08, .6, n); h = rng.uniform(.08, .6, n)
        b = np.stack([x1, y1, np.minimum(x1 + w, 1.), np.minimum(y1 + h, 1.)], 1).astype(np.float32)
        boxes.append(_t(b))
        classes.append(_t(rng.integers(0, 20, n).astype(np.float32)))
    return x.to(DEV), classes, boxes


def layerwise_forward_distance(net, params, conv_dtype):
    """Relative L2 distance of every activation of the HIP forward (engine tensors, NHWC) to the oracle's activation of the same
    name on the f64-case input, the oracle run with the same operand rounding -> ({name: rel}, loc rel-max, conf rel-max)."""
    x, _, _ = f64_case()
    acts = {}
    with torch.no_grad():
        lo, co = O.ssd300_forward(torch.from_numpy(x), params, operand_round=None if conv_dtype == "f32" else conv_dtype, acts=acts,
                                  store_round=conv_dtype == "bf16" and net._engine.bf16_tensors)
    set_engine(net, "wino", conv_dtype)
    try:
        with torch.no_grad():
            loc, conf, saved = net._engine.forward(_t(x), net._forward_params(), save=True)
    finally:
        set_engine(net, "wino", "f32")
    out = {}
    for name, ref in acts.items():
        got = saved["T"].get(name)
        if got is None or not torch.is_tensor(got):           # consumed by a fused kernel without being written (f32 Winograd + pool)
            continue
        out[name] = rel_l2(got.float().permute(0, 3, 1, 2), ref)
    return out, float((loc.cpu() - lo).abs().max() / lo.abs().max().clamp_min(1)), float((conf.cpu() - co).abs().max() / co.abs().max().clamp_min(1))


# ---- decision-pinned comparison (independent of the code under test: no measured table) ------------------------------------
# relative L2 per gradient tensor; fixed numbers, NOT written by tools/grad_bars.py.  Measured on an MI355X (round 3): worst tensor
# 1.6e-6 on the direct engine (c_11_cl.weight), 7.7e-6 on the Winograd engine (conv1_1.weight); medians 2.9e-7 / 1.6e-6.
PINNED_BAR = {"direct": 1e-5, "wino": 5e-5}
# Images per chunk of the f64 evaluation: its graph holds ~1.3 GB per SSD300 image and ~3 GB per SSD512 image, so a whole batch of
# 32 (or 16 at 512) would need tens of GB of host memory.  What the HIP step exported stays on the device and crosses to the host one
# chunk at a time.
CHUNK = {300: 4, 512: 1}
# the rounding-pinned form holds the bf16-rounded operands and the pinned tensors of its chunk besides: one image per chunk
CHUNK_BF16 = {300: 1, 512: 1}


def chunk_spans(bs, variant=300, chunk=None, bf16=False):
    """[(lo, hi)] image ranges of the f64 evaluation: chunks of `chunk` (default CHUNK[variant], CHUNK_BF16[variant] for the
    rounding-pinned form) images, or the given list of sizes"""
    if isinstance(chunk, (list, tuple)):
        sizes = list(chunk)
    else:
        step = chunk or (CHUNK_BF16 if bf16 else CHUNK)[variant]
        sizes = [min(step, bs - lo) for lo in range(0, bs, step)]
    if sum(sizes) != bs or min(sizes) < 1:
        raise ValueError(f"chunk sizes {sizes} do not cover a batch of {bs}")
    ends = np.cumsum([0] + sizes)
    return [(int(ends[i]), int(ends[i + 1])) for i in range(len(sizes))]


def unpack_relu_bits(bits, n, h, w, c):
    """(tiles, c/4) int64 words of the Winograd input transform (bit (a*4+b)*4+e = x[4th+a][4tw+b][4c4+e] > 0) -> bool mask (n, c, h, w),
    on the device of `bits`"""
    th, tw = (h + 3) // 4, (w + 3) // 4
    b = bits.view(n, th, tw, c // 4, 1)
    sh = torch.arange(64, dtype=torch.int64, device=bits.device).view(1, 1, 1, 1, 64)
    m = ((b >> sh) & 1).bool().view(n, th, tw, c // 4, 4, 4, 4)            # (n, th, tw, c4, a, b, e)
    m = m.permute(0, 3, 6, 1, 4, 2, 5).reshape(n, c, 4 * th, 4 * tw)      # (n, c4, e, th, a, tw, b)
    return m[:, :, :h, :w].contiguous()


def _relu_mask_of(eng, T, aux, op, host=True):
    """ReLU mask (N,C,H,W bool; on the host, or host=False: on the device) of a convolution's output as the engine can reproduce it: from
    the stored activation, from the ReLU bit words the next layer's input transform kept when the activation itself was never stored
    (conv1_1 -> planes), or None (gate carried by a pool)."""
    from objectdetection_ssd_amd.Model import _Elided
    t = T[op["y"]]
    if not isinstance(t, _Elided):
        m = (t > 0).permute(0, 3, 1, 2)
        return m.cpu() if host else m
    nxt = next((o for o in eng.ops if o["op"] == "conv" and o["x"] == op["y"]), None)
    bits = aux.get("bits:" + nxt["p"]) if nxt is not None else None
    if bits is None or any(o["op"] == "pool" and o["x"] == op["y"] for o in eng.ops):
        return None
    n, h, w, c = t.shape
    m = unpack_relu_bits(bits, n, h, w, c)
    return m.cpu() if host else m


def _hip_loss(loc, conf, classes, boxes):
    """the HIP loss kernel with its gradients -> (its output dict, the hard negatives it selected (bs, P) bool)"""
    from objectdetection_ssd_amd import Losses, ops
    gt, cls_t, img_start = Losses._pack_targets(classes, boxes, loc.device)
    pri, pri_xyxy = Losses._priors_on(loc.device, loc.shape[1])
    out = ops.multibox_loss(loc.contiguous(), conf.contiguous(), gt, cls_t, img_start, pri, pri_xyxy, Losses.IOU_THRESHOLD,
                            Losses.NEG_POS_RATIO, 0, want_grads=True)
    torch.cuda.synchronize()
    return out, (out["cls"] == O.BG_CLASS) & (out["dconf"].abs().amax(-1) > 0)


def gpu_decisions(net, x, classes, boxes):
    """The discrete choices of the HIP forward + loss on this batch (the net's variant, in its conv_dtype): ReLU masks and max-pool arg-max
    codes as the engine saved them for its backward, and the hard negatives its loss kernel selected -> (decisions for O.ssd300_forward,
    neg_select).  Everything stays on the device (`f64_pinned_grads` moves one chunk of images at a time to the host);
    decisions["out"] = (loc, conf) of this forward, for the check that the train step compared made the same choices."""
    from objectdetection_ssd_amd.Model import _Elided
    net.train()
    eng = net._engine
    with torch.no_grad():
        loc, conf, saved = eng.forward(x, net._forward_params(), save=True)
    T, aux = saved["T"], saved["aux"]
    relu, pool = {}, {}
    for op in eng.ops:
        if op["op"] in ("conv", "conv_first") and op["y"] in eng.relu_out:
            relu[op["y"]] = _relu_mask_of(eng, T, aux, op, host=False)
        elif op["op"] == "pool":
            gate = (T[op["y"]] > 0).permute(0, 3, 1, 2) if isinstance(T[op["x"]], _Elided) else None
            pool[op["y"]] = (aux[op["y"]].permute(0, 3, 1, 2).clone(), gate)
    _, neg = _hip_loss(loc, conf, classes, boxes)
    return {"relu": relu, "pool": pool, "out": (loc.clone(), conf.clone())}, neg


def _host(t, lo, hi):
    """images lo:hi of an exported tensor (any device), on the host; bf16 widened to f32 (exactly)"""
    if t is None:
        return None
    t = torch.as_tensor(t)[lo:hi]
    if t.dtype == torch.bfloat16:
        t = t.float()
    return t.contiguous().cpu()


def _host_case(case):
    x, boxes, classes = case
    x = torch.as_tensor(x).detach().cpu()
    as_np = lambda a: np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.float32)      # noqa: E731
    return x, [as_np(b) for b in boxes], [as_np(c) for c in classes]


def _release_heap():
    """hand the freed heap of a chunk back to the system (glibc keeps it otherwise, and the next chunk's peak adds to it)"""
    try:
        ctypes.CDLL("libc.so.6").malloc_trim(0)
    except (OSError, AttributeError):
        pass


def _f64_pinned_eval(params, decisions, neg_select, case, variant, chunk, pinned, outputs):
    """f64 CPU evaluation of the oracle network on `case`, following `decisions` (and, pinned given, the stored values of the bf16-tensor
    mode), in chunks of images.  Each chunk's losses are divided by the positive count of the WHOLE batch, so the chunks' losses and
    gradients (accumulated in f64 by autograd) sum to the batch's, and a stored gradient (which carries that normalisation) is compared
    as it is.  outputs: None or a dict that receives the whole batch's "loc" and "conf".  -> (a1, a2, {name: grad f64})"""
    x, boxes, classes = _host_case(f64_case() if case is None else case)
    bs = x.shape[0]
    pri = O.create_priors_ssd300() if variant == 300 else O.create_priors_ssd512()
    _, cls, _, _, _ = O.match_priors(boxes, classes, O.xywh_to_xyxy(pri))
    n_pos = int((cls != O.BG_CLASS).sum())
    P = {k: v.detach().cpu().clone().double().requires_grad_(True) for k, v in params.items()}
    kw = {}
    if pinned is not None:
        kw = dict(operand_round="bf16", store_round=True)
        if "scale" not in pinned:
            pinned["scale"] = O.pin_scales(pinned)
    a1 = a2 = 0.0
    locs, confs = [], []
    for lo, hi in chunk_spans(bs, variant, chunk, pinned is not None):
        dec = {"relu": {k: _host(m, lo, hi) for k, m in decisions["relu"].items()},
               "pool": {k: (_host(c, lo, hi), _host(g, lo, hi)) for k, (c, g) in decisions["pool"].items()}}
        if pinned is not None:
            kw["pinned"] = {"fwd": {k: _host(t, lo, hi) for k, t in pinned["fwd"].items()},
                            "bwd": {k: _host(t, lo, hi) for k, t in pinned["bwd"].items()},
                            "bf16": pinned["bf16"], "report": pinned["report"], "scale": pinned["scale"]}
        loc, conf = O.ssd300_forward(x[lo:hi].double(), P, variant=variant, decisions=dec, **kw)
        l1, l2 = O.multibox_loss_torch(loc, conf, [torch.from_numpy(b) for b in boxes[lo:hi]], [torch.from_numpy(c) for c in classes[lo:hi]],
                                       pri_cxcywh=pri, neg_select=_host(neg_select, lo, hi), n_pos=n_pos)
        (l1 + l2).backward()
        if outputs is not None:
            locs.append(loc.detach())
            confs.append(conf.detach())
        a1 += float(l1.detach())
        a2 += float(l2.detach())
        del loc, conf, l1, l2, dec
        kw.pop("pinned", None)                     # this chunk's graph and host copies go before the next is built
        _release_heap()
    if outputs is not None:
        outputs["loc"], outputs["conf"] = torch.cat(locs), torch.cat(confs)
    return a1, a2, {k: v.grad for k, v in P.items()}


def f64_pinned_grads(params, decisions, neg_select, case=None, variant=300, chunk=None, outputs=None):
    """f64 CPU evaluation of the oracle network FOLLOWING the given decisions (`gpu_decisions` of an f32 or f32x3 step) on `case` =
    (x, boxes, classes) (default: the f64 case), SSD300 or SSD512, in chunks of images (`chunk_spans`) -> (a1, a2, {name: grad f64})."""
    return _f64_pinned_eval(params, decisions, neg_select, case, variant, chunk, None, outputs)


# ---- decision- AND rounding-pinned comparison of the bf16-tensor mode (round-3 review, weak 1) --------------------------------------
# One fixed bar for all 71 gradients, not produced by tools/grad_bars.py.  What is left between the two sides once every discrete
# choice of the HIP step is followed -- ReLU masks, arg-max codes, hard negatives and the bf16 value every stored tensor was rounded
# to -- is f32 accumulation order inside single layers.
BF16_PINNED_BAR = 1e-4


def gpu_pinned_step(net, x, classes, boxes, conv_dtype="bf16"):
    """One forward + loss + backward of the HIP engine (the net's variant) with everything a rounding-pinned oracle run needs exported:
    -> (decisions, neg_select, pinned dict for O.ssd300_forward, (l1, l2), {param name: gradient}).  The exported tensors stay on the
    device, as copies (`f64_rounding_pinned_grads` moves one chunk of images at a time to the host); decisions["out"] = (loc, conf)."""
    from objectdetection_ssd_amd.Model import _Elided
    set_engine(net, "wino", conv_dtype)
    net.train()
    eng = net._engine
    try:
        P = net._forward_params()
        eng.grad_tap = {}
        with torch.no_grad():
            loc, conf, saved = eng.forward(x, P, save=True)
            T, aux = saved["T"], saved["aux"]
            relu, pool, fwd, b16 = {}, {}, {}, set()
            for op in eng.ops:
                if op["op"] in ("conv", "conv_first") and op["y"] in eng.relu_out:
                    t = T[op["y"]]
                    relu[op["y"]] = None if isinstance(t, _Elided) else (t > 0).permute(0, 3, 1, 2)
                elif op["op"] == "pool":
                    gate = (T[op["y"]] > 0).permute(0, 3, 1, 2) if isinstance(T[op["x"]], _Elided) else None
                    pool[op["y"]] = (aux[op["y"]].permute(0, 3, 1, 2).clone(), gate)
            for name, t in T.items():
                if ":" in name or name in ("x", "x_col") or not torch.is_tensor(t):
                    continue
                fwd[name] = t.permute(0, 3, 1, 2).clone()
                if t.dtype == torch.bfloat16:
                    b16.add(name)
            out, neg = _hip_loss(loc, conf, classes, boxes)
            need = {n: True for n in eng.names}
            grads = eng.backward(saved, out["dloc"], out["dconf"], P, need)
            torch.cuda.synchronize()
            bwd = {n: g.permute(0, 3, 1, 2).clone() for n, g in eng.grad_tap.items() if n.split(":")[0] in fwd}
            losses = (float(out["losses"][0]), float(out["losses"][1]))
            grads = {n: g.detach().float().cpu().clone() for n, g in grads.items()}
            dec = {"relu": relu, "pool": pool, "out": (loc.clone(), conf.clone())}
    finally:
        eng.grad_tap = None
        set_engine(net, "wino", "f32")
    pinned = {"fwd": fwd, "bwd": bwd, "bf16": b16, "report": {}}
    return dec, neg, pinned, losses, grads


def f64_rounding_pinned_grads(params, decisions, neg_select, pinned, case=None, variant=300, chunk=None, outputs=None):
    """f64 CPU evaluation of the bf16-operand oracle network on `case` (default: the f64 case), SSD300 or SSD512, following the given
    decisions AND stored values (`gpu_pinned_step`), in chunks of images; pinned["report"] receives the per-layer distances over the whole
    batch (the norms they are measured against are those of the whole batch: `O.pin_scales`)."""
    return _f64_pinned_eval(params, decisions, neg_select, case, variant, chunk, pinned, outputs)


def bf16_tensor_heads(net):
    """the heads the engine's last training forward ran on the bf16-tensor kernels (weight-table entries `b16`)"""
    return {p for p, kind in net._engine._wcache.kinds().items() if kind == "b16" and p.startswith("c_")}


def weight_kinds(net):
    """{layer: x31 | wino_adj | wino | layout | b16 | first} of the engine's last training forward (its weight table)"""
    return net._engine._wcache.kinds()


def oracle_self_decisions(params, x, boxes, classes, variant=300, bf16=False):
    """The decisions (and, bf16=True, the stored tensors and their stored gradients) of an UNPINNED f64 oracle run on this batch, in the forms `gpu_decisions` /
    `gpu_pinned_step` export them (NCHW, on the host): pinned to them, the oracle evaluates itself.  For the CPU test of the chunked
    evaluation and for timing it without a GPU.  -> (decisions, neg_select, pinned or None, (a1, a2) of this run with these negatives)"""
    import torch.nn.functional as F
    x = torch.as_tensor(x).double()
    acts, live = {}, {}
    P = {k: v.detach().double().requires_grad_(bf16) for k, v in params.items()}
    kw = dict(operand_round="bf16", store_round=True, act_grads=live) if bf16 else {}
    with torch.set_grad_enabled(bf16):
        loc, conf = O.ssd300_forward(x, P, variant=variant, acts=acts, **kw)
    relu = {k: v > 0 for k, v in acts.items() if k.startswith("a")}
    pool = {}
    for p, (src, k, s, pad) in {"p1": ("a1_2", 2, 2, 0), "p2": ("a2_2", 2, 2, 0), "p3": ("a3_3", 2, 2, 0), "p4": ("a4_3", 2, 2, 0),
                                "p5": ("a5_3", 3, 1, 1)}.items():
        z = acts[src]
        _, idx = F.max_pool2d(z, k, s, padding=pad, ceil_mode=p == "p3", return_indices=True)
        ho, wo = idx.shape[2], idx.shape[3]
        r = idx // z.shape[3] - (torch.arange(ho).view(1, 1, ho, 1) * s - pad)
        c = idx % z.shape[3] - (torch.arange(wo).view(1, 1, 1, wo) * s - pad)
        pool[p] = (r * k + c, None)
    pri = O.create_priors_ssd300() if variant == 300 else O.create_priors_ssd512()
    neg = torch.from_numpy(O.multibox_loss(loc.detach().float().numpy(), conf.detach().float().numpy(), boxes, classes, pri_cxcywh=pri,
                                           want_grads=False)["hn_mask"])
    a1, a2 = O.multibox_loss_torch(loc, conf, [torch.from_numpy(np.asarray(b_, np.float32)) for b_ in boxes],
                                   [torch.from_numpy(np.asarray(c_, np.float32)) for c_ in classes], pri_cxcywh=pri, neg_select=neg)
    pinned = None
    if bf16:
        # the gradient every stored tensor would be stored as: masked by its producer's ReLU, rounded to bf16 on the trunk
        (a1 + a2).backward()
        trunk = {n for n in acts if n.startswith(("a1", "a2", "a3", "a4", "a5")) or n == "n4_3"}
        bwd = {}
        for n, t in live.items():
            g = t.grad * (acts[n] > 0) if n[0] == "a" else t.grad
            bwd[n] = O.bf16_round(g) if n in trunk else g
        pinned = {"fwd": dict(acts), "bwd": bwd, "bf16": trunk, "report": {}}
    return {"relu": relu, "pool": pool}, neg, pinned, (float(a1.detach()), float(a2.detach()))

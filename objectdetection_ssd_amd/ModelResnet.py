"""`SSD_resnet34` -- drop-in for reference Model.py:12-126 (BASELINE configs[4]): eval- and train-mode forward on the gfx950
kernels, and the train-mode backward.

The module tree mirrors the reference's so that `state_dict()` / `load_state_dict()` exchange checkpoints with it
(keys and shapes pinned by tests/golden/resnet34.npz): `resnet.*` is the torchvision ResNet-34 layer list (built from
torch.nn here -- torchvision is a download in the reference), `seq1..seq5` are views of it, and the SSD blocks keep the
reference's names including the unused `conv2d_03` / `bn4` / `bn2` / `bn1`.

Eval mode folds every BatchNorm into the convolution before it.  Train mode (f32 only) is the reference's: the trunk runs
without gradient but its 36 BatchNorms normalise with batch statistics and update their running buffers; x5e goes through
ReLU + Dropout; conv2d_0 / conv2d_01 (applied twice) / conv2d_02 are Conv -> ReLU -> BatchNorm -> Dropout2d, the loc heads
Conv -> BatchNorm -> Dropout2d, the conf heads plain convs.  Gradients reach the 30 tensors of that head section through one
autograd node (`_HeadSection`).  Dropout masks come from a Philox4x32-10 generator keyed by one seed per call, drawn from
torch's default CPU generator (so `torch.manual_seed` reproduces a train step bitwise); the backward regenerates them.
`dropout_masks()` returns the masks of the last train forward, as a testing aid.  The reference has no loss wired to this
model (Losses.py:6-7 are the SSD300 priors), so none is provided.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import ops

_STAGES = ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2))       # (channels, blocks, stride of the first block)
_BN_EPS = 1e-5
# dropout site ids of the train-mode generator (the Philox counter's third word; csrc/batchnorm.hip)
_SITES = {"drop": 0, "conv2d_0": 1, "conv2d_01.0": 2, "conv2d_01.1": 3, "conv2d_02": 4, "conv2d_02_bb4": 5, "conv2d_02_bb2": 6,
          "conv2d_02_bb1": 7}


class _BasicBlock(nn.Module):
    """Parameter container with torchvision's BasicBlock attribute names (conv1, bn1, conv2, bn2, downsample)."""

    def __init__(self, cin: int, c: int, stride: int):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, c, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(c)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(c, c, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(c)
        self.downsample = None
        if stride != 1 or cin != c:
            self.downsample = nn.Sequential(nn.Conv2d(cin, c, 1, stride, bias=False), nn.BatchNorm2d(c))
        self.stride = stride


class _ResNet34(nn.Module):
    """children() order conv1, bn1, relu, maxpool, layer1..4, avgpool, fc -- what Model.py:22-30 slices."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        cin = 64
        for li, (c, nblk, stride) in enumerate(_STAGES, start=1):
            blocks = []
            for b in range(nblk):
                blocks.append(_BasicBlock(cin, c, stride if b == 0 else 1))
                cin = c
            setattr(self, f"layer{li}", nn.Sequential(*blocks))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512, 1000)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")


def _bn_affine(bn: nn.BatchNorm2d) -> Tuple[torch.Tensor, torch.Tensor]:
    """eval-mode BatchNorm as y = x*scale + shift"""
    scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
    return scale, bn.bias.detach() - bn.running_mean * scale


class SSD_resnet34(nn.Module):
    """Reference Model.py:12-126: `SSD_resnet34(n_classes, dropout_p=0.4, k=3)`; input (bs,3,224,224) NCHW f32;
    returns (bs, 21k, 4), (bs, 21k, n_classes+1) with the reference's hard-coded `.view(..., 21)` (so n_classes = 20)."""

    def __init__(self, n_classes, dropout_p=0.4, k=3):
        super().__init__()
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.k = k
        self.n_classes = n_classes
        self.dropout_p = dropout_p
        if n_classes + 1 != 21:
            raise ValueError("the reference reshapes the class scores with a hard-coded 21 (Model.py:117): n_classes must be 20")
        self.resnet = _ResNet34()
        self.resnet_layers = list(self.resnet.children())
        self.relu = nn.ReLU()
        self.drop = nn.Dropout(p=0.4)
        L = self.resnet_layers
        self.seq1 = nn.Sequential(*L[0:3])
        self.seq2 = nn.Sequential(*L[3:5])
        self.seq3 = nn.Sequential(*L[5])
        self.seq4 = nn.Sequential(*L[6])
        self.seq5 = nn.Sequential(*L[7])
        self.conv2d_0 = self.conv2d(512, 256, kernel=3, stride=1, padding=1)
        self.conv2d_01 = self.conv2d(256, 256, kernel=3, stride=2, padding=1)
        self.conv2d_02 = self.conv2d(256, 256, kernel=3, stride=2, padding=1)
        self.conv2d_03 = self.conv2d(256, 256, kernel=3, stride=2, padding=1)
        for s in ("4", "2", "1"):
            setattr(self, f"conv2d_02_bb{s}", self.conv2d_final(256, 4 * k, kernel=3, stride=1, padding=1))
            c = nn.Conv2d(256, (n_classes + 1) * k, kernel_size=3, stride=1, padding=1)
            c.bias.data.zero_().add_(-2)                                   # Model.py:39,43,47
            setattr(self, f"conv2d_02_c{s}", c)
        self.bn4 = nn.BatchNorm2d((n_classes + 1) * k)
        self.bn2 = nn.BatchNorm2d((n_classes + 1) * k)
        self.bn1 = nn.BatchNorm2d((n_classes + 1) * k)
        self._cache: Dict[str, tuple] = {}
        self.conv_dtype = "f32"            # "bf16": bf16-operand MFMA kernels with f32 accumulation

    def conv2d(self, in_channels, out_channels, kernel=1, stride=1, padding=0):
        return nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size=kernel, stride=stride, padding=padding),
                             nn.ReLU(), nn.BatchNorm2d(out_channels), nn.Dropout2d(p=0.4))

    def conv2d_final(self, in_channels, out_channels, kernel=1, stride=1, padding=0):
        return nn.Sequential(nn.Conv2d(in_channels, out_channels, kernel_size=kernel, stride=stride, padding=padding),
                             nn.BatchNorm2d(out_channels), nn.Dropout2d(p=0.4))

    def invalidate_weight_cache(self) -> None:
        """Drop the BatchNorm-folded kernel-layout weights.  They are rebuilt when any tensor's `(data_ptr, _version)` changes;
        writes through `.data` change neither, so call this after such a write (same contract as `SSD_300`)."""
        self._cache.clear()

    # -- prepared (BatchNorm-folded, kernel-layout) weights, rebuilt when any tensor of the module changes ---------------------
    def _signature(self):
        return tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))

    def _prepared(self):
        sig = self._signature()
        ent = self._cache.get("w")
        if ent is not None and ent[0] == sig:
            return ent[1]
        W: Dict[str, tuple] = {}

        def fold(conv: nn.Conv2d, bn: Optional[nn.BatchNorm2d]):
            w = conv.weight.detach()
            b = conv.bias.detach() if conv.bias is not None else torch.zeros(w.shape[0], device=w.device)
            if bn is not None:
                scale, shift = _bn_affine(bn)
                w = w * scale.view(-1, 1, 1, 1)
                b = b * scale + shift
            return w.contiguous(), b.contiguous()

        with torch.no_grad():
            w, b = fold(self.resnet.conv1, self.resnet.bn1)
            W["stem"] = (ops.stem_weight_rows(w), b)
            for li in range(1, 5):
                for bi, blk in enumerate(getattr(self.resnet, f"layer{li}")):
                    p = f"layer{li}.{bi}."
                    for cname, bname in (("conv1", "bn1"), ("conv2", "bn2")):
                        w, b = fold(getattr(blk, cname), getattr(blk, bname))
                        W[p + cname] = (ops.weight_ohwi(w), b)
                    if blk.downsample is not None:
                        w, b = fold(blk.downsample[0], blk.downsample[1])
                        W[p + "down"] = (ops.weight_ohwi(w), b)
            for name in ("conv2d_0", "conv2d_01", "conv2d_02"):
                seq = getattr(self, name)
                w, b = fold(seq[0], None)
                scale, shift = _bn_affine(seq[2])
                W[name] = (ops.weight_ohwi(w), b, scale.contiguous(), shift.contiguous())
            for s in ("4", "2", "1"):
                bb = getattr(self, f"conv2d_02_bb{s}")
                wb, bbias = fold(bb[0], bb[1])                     # loc head: Conv -> BN folds
                wc, cbias = fold(getattr(self, f"conv2d_02_c{s}"), None)
                w = torch.cat((wb, wc), 0)
                W["head" + s] = (ops.weight_ohwi(w, ops.pad32(w.shape[0])), torch.cat((bbias, cbias)).contiguous())
        self._cache["w"] = (sig, W)
        return W

    # -- train mode -------------------------------------------------------------------------------------------------------------
    def _unfolded(self, key: str, convs) -> tuple:
        """kernel-layout copies of unfolded conv weights (the train path normalises with batch statistics, so nothing folds),
        cached on the weights' (data_ptr, _version)"""
        sig = tuple((c.weight.data_ptr(), c.weight._version) for c in convs)
        ent = self._cache.get(key)
        if ent is not None and ent[0] == sig:
            return ent[1]
        with torch.no_grad():
            if key == "train:stem":
                val = ops.stem_weight_rows(convs[0].weight.detach().contiguous())
            elif len(convs) == 1:
                val = ops.weight_ohwi(convs[0].weight.detach().contiguous())
            else:                                      # a loc head and its conf head share one packed convolution
                w = torch.cat([c.weight.detach() for c in convs], 0).contiguous()
                val = (ops.weight_ohwi(w, ops.pad32(w.shape[0])), ops.weight_ihwo(w, ops.pad32(w.shape[0])))
        self._cache[key] = (sig, val)
        return val

    def _bn_stats(self, bn: nn.BatchNorm2d, h: torch.Tensor, c: int, ld: Optional[int] = None) -> torch.Tensor:
        """training-mode statistics of `bn` over h's rows -> (4, c) mean / invstd / scale / shift; running buffers updated"""
        if not (bn.affine and bn.track_running_stats) or bn.momentum is None:
            raise ValueError("the train path supports affine BatchNorm2d with running statistics and a momentum (the reference's)")
        st = ops.bn_train_stats(h, c, bn.weight.detach(), bn.bias.detach(), bn.eps, bn.momentum, bn.running_mean, bn.running_var,
                                bn.num_batches_tracked, ld=ld)
        for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked):
            torch.autograd.graph.increment_version(t)        # written by a kernel: the eval cache keys on _version
        return st

    def _train_forward(self, x):
        if self.conv_dtype != "f32":
            raise ValueError("SSD_resnet34 train mode runs in f32 only (conv_dtype = 'f32')")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("SSD_resnet34 train mode cannot be graph-captured: each forward draws its dropout seed on the host")
        x = x.contiguous()
        bs, _, H, Wd = x.shape
        hw = [ops.conv_out_hw(H, Wd, 7, 2, 3, 1)]
        hw.append((ops.pool_out(hw[0][0], 3, 2, 1, False), ops.pool_out(hw[0][1], 3, 2, 1, False)))
        for _ in range(3):
            hw.append(ops.conv_out_hw(hw[-1][0], hw[-1][1], 3, 2, 1, 1))     # layer2..4
        for _ in range(3):
            hw.append(ops.conv_out_hw(hw[-1][0], hw[-1][1], 3, 2, 1, 1))     # conv2d_01 twice, conv2d_02
        if bs * min(h * w for h, w in hw) < 2:
            raise ValueError(f"Expected more than 1 value per channel when training: batch {bs} at {H}x{Wd} gives a "
                             f"{hw[-1][0]}x{hw[-1][1]} map for conv2d_02's BatchNorm")
        # one seed per call from torch's default CPU generator: torch.manual_seed(s) makes a train forward reproducible
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        with torch.no_grad():
            h5 = self._train_trunk(x, seed)
        params = self._head_params()
        need = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        if need:
            loc, conf = _HeadSection.apply(self, h5, seed, *params)
        else:
            with torch.no_grad():
                loc, conf, _ = self._train_heads(h5, seed, save=False)
        return loc, conf

    def _train_trunk(self, x, seed):
        """seq1..seq5 with training-mode BatchNorm, then relu + Dropout (Model.py:80-88) -> x5e (bs,h,w,512) NHWC"""
        bs = x.shape[0]
        r = self.resnet
        col = ops.im2col_nchw3(x, 7, 2, 3)
        g = ops.make_geom(bs, col.shape[1], col.shape[2], col.shape[3], 64, 1, 1, 0, 1)
        h = ops.conv2d_fwd(col, self._unfolded("train:stem", (r.conv1,)), None, g, False)
        st = self._bn_stats(r.bn1, h, 64)
        ops.bn_apply(h, 64, st[2], st[3], relu=True, out=h)
        h, _ = ops.maxpool_fwd(h, 3, 2, 1, False, want_argmax=False)
        cin = 64
        for li, (c, nblk, stride) in enumerate(_STAGES, start=1):
            for bi, blk in enumerate(getattr(r, f"layer{li}")):
                s = stride if bi == 0 else 1
                key = f"train:layer{li}.{bi}."
                g1 = ops.make_geom(bs, h.shape[1], h.shape[2], cin, c, 3, s, 1, 1)
                o = ops.conv2d_fwd(h, self._unfolded(key + "conv1", (blk.conv1,)), None, g1, False)
                st = self._bn_stats(blk.bn1, o, c)
                ops.bn_apply(o, c, st[2], st[3], relu=True, out=o)
                g2 = ops.make_geom(bs, o.shape[1], o.shape[2], c, c, 3, 1, 1, 1)
                o2 = ops.conv2d_fwd(o, self._unfolded(key + "conv2", (blk.conv2,)), None, g2, False)
                st2 = self._bn_stats(blk.bn2, o2, c)
                last = li == 4 and bi == nblk - 1
                # Model.py:88 relu (a no-op on the block's ReLU output) and nn.Dropout, folded into the pass that writes layer4's output
                drop = (ops.DROP_ELEMENT, float(self.drop.p), seed, _SITES["drop"], 1) if last else None
                if blk.downsample is not None:
                    gd = ops.make_geom(bs, h.shape[1], h.shape[2], cin, c, 1, s, 0, 1)
                    d = ops.conv2d_fwd(h, self._unfolded(key + "down", (blk.downsample[0],)), None, gd, False)
                    std = self._bn_stats(blk.downsample[1], d, c)
                    ops.bn_apply(o2, c, st2[2], st2[3], relu=True, res=d, res_scale=std[2], res_shift=std[3], drop=drop, out=o2)
                else:
                    ops.bn_apply(o2, c, st2[2], st2[3], relu=True, res=h, drop=drop, out=o2)
                h = o2
                cin = c
        return h

    def _head_params(self):
        """the 30 trainable tensors of the head section, in _HeadSection's argument order"""
        out = []
        for name in ("conv2d_0", "conv2d_01", "conv2d_02"):
            seq = getattr(self, name)
            out += [seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias]
        for s in ("4", "2", "1"):
            bb, cl = getattr(self, f"conv2d_02_bb{s}"), getattr(self, f"conv2d_02_c{s}")
            out += [bb[0].weight, bb[0].bias, bb[1].weight, bb[1].bias, cl.weight, cl.bias]
        return out

    def _train_heads(self, h5, seed, save: bool):
        """Model.py:89-126 in train mode on x5e -> (loc, conf, saved state for the backward or None)"""
        bs = h5.shape[0]
        k = self.k
        co = 25 * k
        ld = ops.pad32(co)
        sv = {"seed": seed, "x5": h5}
        feats = []
        h = h5
        for name, site, ci, s in (("conv2d_0", "conv2d_0", 512, 1), ("conv2d_01", "conv2d_01.0", 256, 2),
                                  ("conv2d_01", "conv2d_01.1", 256, 2), ("conv2d_02", "conv2d_02", 256, 2)):
            seq = getattr(self, name)
            g = ops.make_geom(bs, h.shape[1], h.shape[2], ci, 256, 3, s, 1, 1)
            y = ops.conv2d_fwd(h, self._unfolded("train:" + name, (seq[0],)), seq[0].bias.detach(), g, True)   # Conv -> ReLU
            st = self._bn_stats(seq[2], y, 256)
            out = ops.bn_apply(y, 256, st[2], st[3], drop=(ops.DROP_CHANNEL, float(seq[3].p), seed, _SITES[site], g.Ho * g.Wo))
            out = out.view(bs, g.Ho, g.Wo, 256)
            sv[site] = (h, y, st, g, float(seq[3].p))
            feats.append(out)
            h = out
        total = sum(f.shape[1] * f.shape[2] for f in feats[1:]) * k
        sv["total"] = total
        loc = torch.empty((bs, total, 4), device=h5.device, dtype=torch.float32)
        conf = torch.empty((bs, total, 21), device=h5.device, dtype=torch.float32)
        off = 0
        for s, f in zip(("4", "2", "1"), feats[1:]):
            bb, cl = getattr(self, f"conv2d_02_bb{s}"), getattr(self, f"conv2d_02_c{s}")
            wf, _ = self._unfolded("train:head" + s, (bb[0], cl))
            g = ops.make_geom(bs, f.shape[1], f.shape[2], 256, co, 3, 1, 1, 1)
            bias = torch.cat((bb[0].bias.detach(), cl.bias.detach()))
            packed = ops.conv2d_fwd(f, wf, bias, g, False, ld=ld)           # loc channels 0..4k-1 before their BatchNorm
            st = self._bn_stats(bb[1], packed, 4 * k, ld=ld)
            hwn = g.Ho * g.Wo
            out = packed.clone()
            ops.bn_apply(packed, 4 * k, st[2], st[3], drop=(ops.DROP_CHANNEL, float(bb[2].p), seed, _SITES["conv2d_02_bb" + s], hwn),
                         out=out, ld=ld, out_ld=ld)
            ops.heads_scatter(out, ld, loc, conf, bs, hwn, k, off)
            sv["head" + s] = (f, packed, st, g, float(bb[2].p), off)
            off += hwn * k
        self._last_train = {"seed": seed, "bs": bs, "x5": tuple(h5.shape), "maps": [tuple(f.shape[1:3]) for f in feats],
                            "device": h5.device}
        return loc, conf, (sv if save else None)

    def _train_backward(self, sv, dloc, dconf):
        """gradients of the 30 head-section tensors (in _head_params order) from dL/dloc, dL/dconf"""
        k = self.k
        co = 25 * k
        ld = ops.pad32(co)
        seed = sv["seed"]
        grads: Dict[str, torch.Tensor] = {}

        def bn_back(bn, dy, x, st, drop, relu_mask, ld_=None, accumulate=False, want_dx=True):
            c = st.shape[1]
            if not accumulate:
                grads[id(bn.weight)] = torch.empty(c, device=dy.device)
                grads[id(bn.bias)] = torch.empty(c, device=dy.device)
            dx, _ = ops.bn_train_bwd(dy, x, c, st[0], st[1], bn.weight.detach(), drop, relu_mask, dgamma=grads[id(bn.weight)],
                                     dbeta=grads[id(bn.bias)], accumulate=accumulate, dx=dy if want_dx else None, want_dx=want_dx,
                                     ld_dy=ld_, ld_x=ld_, ld_dx=ld_)
            return dx

        def head(s, into: Optional[torch.Tensor]):
            """head s's gradient: its parameters, and its input's gradient added to `into` (or returned)"""
            f, packed, st, g, p, off = sv["head" + s]
            bb, cl = getattr(self, f"conv2d_02_bb{s}"), getattr(self, f"conv2d_02_c{s}")
            bs, hwn = g.N, g.Ho * g.Wo
            dy = ops.heads_gather(dloc, dconf, ld, bs, hwn, k, off)
            bn_back(bb[1], dy, packed, st, (ops.DROP_CHANNEL, p, seed, _SITES["conv2d_02_bb" + s], hwn), False, ld_=ld)
            dw, db = ops.conv2d_wgrad(f, dy, g, ld, True)
            a4 = 4 * k
            grads[id(bb[0].weight)], grads[id(cl.weight)] = dw[:a4], dw[a4:]
            grads[id(bb[0].bias)], grads[id(cl.bias)] = db[:a4], db[a4:]
            _, wb = self._unfolded("train:head" + s, (bb[0], cl))
            return ops.conv2d_dgrad(dy, wb, g, into, None, into is not None)

        def block(name, site, dy, first_use=True, want_dx=True):
            seq = getattr(self, name)
            xin, y, st, g, p = sv[site]
            dyr = dy.reshape(-1, 256)
            bn_back(seq[2], dyr, y, st, (ops.DROP_CHANNEL, p, seed, _SITES[site], g.Ho * g.Wo), True, accumulate=not first_use)
            dw, db = ops.conv2d_wgrad(xin, dyr, g, 256, True)
            if first_use:
                grads[id(seq[0].weight)], grads[id(seq[0].bias)] = dw, db
            else:
                grads[id(seq[0].weight)] = grads[id(seq[0].weight)] + dw
                grads[id(seq[0].bias)] = grads[id(seq[0].bias)] + db
            if not want_dx:
                return None
            wb = self._cache.get("train:ihwo:" + name)
            sig = (seq[0].weight.data_ptr(), seq[0].weight._version)
            if wb is None or wb[0] != sig:
                wb = (sig, ops.weight_ihwo(seq[0].weight.detach().contiguous()))
                self._cache["train:ihwo:" + name] = wb
            return ops.conv2d_dgrad(dyr, wb[1], g)

        dx9 = head("1", None)
        dx8 = block("conv2d_02", "conv2d_02", dx9)
        head("2", dx8)
        dx7 = block("conv2d_01", "conv2d_01.1", dx8)
        head("4", dx7)
        dx6 = block("conv2d_01", "conv2d_01.0", dx7, first_use=False)
        block("conv2d_0", "conv2d_0", dx6, want_dx=False)
        return [grads[id(p)] for p in self._head_params()]

    def dropout_masks(self) -> Dict[str, torch.Tensor]:
        """Testing aid: the Dropout / Dropout2d keep masks of the last train-mode forward, regenerated on the device by the same
        generator the forward used (nothing is stored).  "drop": (bs,512,h,w) of nn.Dropout on x5e; "conv2d_0", "conv2d_01.0",
        "conv2d_01.1" (the two uses of conv2d_01), "conv2d_02", "conv2d_02_bb4/2/1": (bs,C) of each Dropout2d.  Reads the modules'
        current `p`, so call it before changing one."""
        lt = getattr(self, "_last_train", None)
        if lt is None:
            raise RuntimeError("dropout_masks(): no train-mode forward has run yet")
        bs, seed, dev = lt["bs"], lt["seed"], lt["device"]
        _, h, w, c = lt["x5"]
        out = {"drop": ops.dropout_mask(bs * h * w * c, float(self.drop.p), seed, _SITES["drop"], dev).view(bs, h, w, c).permute(0, 3, 1, 2)}
        for name, site in (("conv2d_0", "conv2d_0"), ("conv2d_01", "conv2d_01.0"), ("conv2d_01", "conv2d_01.1"), ("conv2d_02", "conv2d_02")):
            out[site] = ops.dropout_mask(bs * 256, float(getattr(self, name)[3].p), seed, _SITES[site], dev).view(bs, 256)
        for s in ("4", "2", "1"):
            bb = getattr(self, f"conv2d_02_bb{s}")
            out["conv2d_02_bb" + s] = ops.dropout_mask(bs * 4 * self.k, float(bb[2].p), seed, _SITES["conv2d_02_bb" + s], dev).view(bs, 4 * self.k)
        return out

    @property
    def last_dropout_seed(self) -> Optional[int]:
        """the 64-bit key the last train-mode forward drew from torch's default generator (testing aid)"""
        lt = getattr(self, "_last_train", None)
        return None if lt is None else lt["seed"]

    def forward(self, x):
        if x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32:
            raise ValueError(f"SSD_resnet34 expects float32 (bs,3,H,W) NCHW input, got {tuple(x.shape)} {x.dtype}")
        if not x.is_cuda:
            raise RuntimeError("SSD_resnet34 runs on the gfx950 HIP kernels only, in train and in eval mode: move the model and the "
                               "input to the GPU (there is no CPU fallback)")
        if self.conv_dtype not in ("f32", "bf16"):
            raise ValueError("conv_dtype must be 'f32' or 'bf16'")
        if self.training:
            return self._train_forward(x)
        bf16 = self.conv_dtype == "bf16"
        W = self._prepared()
        x = x.contiguous()
        bs = x.shape[0]

        def conv(h, key, ci, co, k, s, pad, relu, out=None, accumulate=False, ld=None):
            g = ops.make_geom(bs, h.shape[1], h.shape[2], ci, co, k, s, pad, 1)
            return ops.conv2d_fwd(h, W[key][0], W[key][1], g, relu, ld=ld, out=out, bf16=bf16, accumulate=accumulate)

        with torch.no_grad():
            col = ops.im2col_nchw3(x, 7, 2, 3)                                     # seq1: conv 7x7/s2 + BN + ReLU
            g = ops.make_geom(bs, col.shape[1], col.shape[2], col.shape[3], 64, 1, 1, 0, 1)
            h = ops.conv2d_fwd(col, W["stem"][0], W["stem"][1], g, True, bf16=bf16)
            h, _ = ops.maxpool_fwd(h, 3, 2, 1, False, want_argmax=False)           # seq2[0]
            cin = 64
            for li, (c, nblk, stride) in enumerate(_STAGES, start=1):              # seq2[1], seq3, seq4, seq5
                for bi in range(nblk):
                    p = f"layer{li}.{bi}."
                    s = stride if bi == 0 else 1
                    o = conv(h, p + "conv1", cin, c, 3, s, 1, True)
                    idt = conv(h, p + "down", cin, c, 1, s, 0, False) if (p + "down") in W else h
                    h = conv(o, p + "conv2", c, c, 3, 1, 1, True, out=idt, accumulate=True)    # relu(bn2(conv2) + identity)
                    cin = c
            # Model.py:88 relu (h is already >= 0) and dropout (identity in eval)
            feats = []
            for name, ci, s in (("conv2d_0", 512, 1), ("conv2d_01", 256, 2), ("conv2d_01", 256, 2), ("conv2d_02", 256, 2)):
                h = conv(h, name, ci, 256, 3, s, 1, True)
                h = ops.channel_affine(h, W[name][2], W[name][3], out=h)
                feats.append(h)
            k = self.k
            co = 25 * k
            total = sum(f.shape[1] * f.shape[2] for f in feats[1:]) * k
            loc = torch.empty((bs, total, 4), device=x.device, dtype=torch.float32)
            conf = torch.empty((bs, total, 21), device=x.device, dtype=torch.float32)
            off = 0
            for s, f in zip(("4", "2", "1"), feats[1:]):
                packed = conv(f, "head" + s, 256, co, 3, 1, 1, False, ld=ops.pad32(co))
                hw = f.shape[1] * f.shape[2]
                ops.heads_scatter(packed, ops.pad32(co), loc, conf, bs, hw, k, off)
                off += hw * k
        return loc, conf


class _HeadSection(torch.autograd.Function):
    """Model.py:89-126 in train mode as one autograd node: inputs x5e (no history: the trunk is frozen) and the 30 trainable
    tensors; outputs (loc, conf).  Saves the head-section activations and per-site statistics and seed -- nothing of the trunk --
    and regenerates the dropout masks in the backward."""

    @staticmethod
    def forward(ctx, net, h5, seed, *params):
        loc, conf, sv = net._train_heads(h5, seed, save=True)
        ctx.net = net
        ctx.sv = sv
        return loc, conf

    @staticmethod
    def backward(ctx, dloc, dconf):
        net, sv = ctx.net, ctx.sv
        if sv is None:
            raise RuntimeError("SSD_resnet34 train backward: the saved state was already freed (backward called twice?)")
        ctx.sv = None
        shape = (sv["x5"].shape[0], sv["total"])
        dloc = torch.zeros(shape + (4,), device=sv["x5"].device) if dloc is None else dloc.contiguous()
        dconf = torch.zeros(shape + (21,), device=sv["x5"].device) if dconf is None else dconf.contiguous()
        grads = net._train_backward(sv, dloc, dconf)
        return (None, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[3:]))

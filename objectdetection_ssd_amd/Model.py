"""`Model.SSD_300` with the reference's constructor, attribute / parameter names and
`forward(x) -> (loc (bs,8732,4), conf (bs,8732,21))` contract (reference
Model.py:128-235; `SSD_300(n_classes=K)` gives conf rows of K + 1 columns), computed by the gfx950 kernels of libssd_gfx950.so.

The module tree exists to own the `nn.Parameter`s under the reference's
state-dict names (so `train.py`'s optimizer groups, `.to(device)`,
`state_dict()` and checkpoints keep working); none of the `nn.Conv2d` /
`nn.MaxPool2d` modules is ever called.  `forward` hands the parameters to
`_Engine`, which runs the network as a flat list of NHWC ops through the C ABI
and, under autograd, supplies an explicit backward (dgrad / wgrad / pool /
L2-norm kernels) through one `torch.autograd.Function`.
"""
from __future__ import annotations

import math
import numbers
from collections import namedtuple
from dataclasses import dataclass, replace
from typing import Callable, Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import ops
from .Util import ANCHORS_PER_CELL, ANCHORS_PER_CELL_512, subsampling

N_CLASSES = 21            # width of `conf` of the default model: 20 VOC classes + background (the last column)
MAX_FOREGROUND = 255      # SSD_300(n_classes=...) range: 1 .. 255 foreground classes, conf rows of 2 .. 256 columns
_VGG_CFG = (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M")


class _VGG16(nn.Module):
    """Layer list of VGG-16 'D' (what `torchvision.models.vgg16()` builds and reference
    Model.py:131-157 slices by index).  Pretrained weights are a network download in
    the reference; here the layers are initialised like torchvision's untrained model
    and `load_state_dict` accepts the torchvision key names (`features.N.weight`, ...)."""

    def __init__(self):
        super().__init__()
        layers: List[nn.Module] = []
        cin = 3
        for v in _VGG_CFG:
            if v == "M":
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            else:
                layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        self.features = nn.Sequential(*layers)
        self.avgpool = nn.AdaptiveAvgPool2d((7, 7))
        self.classifier = nn.Sequential(nn.Linear(512 * 7 * 7, 4096), nn.ReLU(True), nn.Dropout(),
                                        nn.Linear(4096, 4096), nn.ReLU(True), nn.Dropout(), nn.Linear(4096, 1000))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.constant_(m.bias, 0)


# ------------------------------------------------------------------------------------------
# op list
# ------------------------------------------------------------------------------------------
def _conv(p, x, y, ci, co, k=3, s=1, pad=1, dil=1, relu=True):
    return dict(op="conv", p=p, x=x, y=y, ci=ci, co=co, k=k, s=s, pad=pad, dil=dil, relu=relu)


def _pool(x, y, k=2, s=2, pad=0, ceil=False):
    return dict(op="pool", x=x, y=y, k=k, s=s, pad=pad, ceil=ceil)


def _head(p, x, scale, ci, anchors=ANCHORS_PER_CELL):
    return dict(op="head", p=p, x=x, scale=scale, ci=ci, a=anchors[scale])


# aux blocks (name, cin, mid, cout, stride, pad) after fc7
_AUX_300 = (("seq8", 1024, 256, 512, 2, 1), ("seq9", 512, 128, 256, 2, 1), ("seq10", 256, 128, 256, 1, 0), ("seq11", 256, 128, 256, 1, 0))
_AUX_512 = (("seq8", 1024, 256, 512, 2, 1), ("seq9", 512, 128, 256, 2, 1), ("seq10", 256, 128, 256, 2, 1), ("seq11", 256, 128, 256, 2, 1),
            ("seq12", 256, 128, 256, 2, 1))


def build_ops(variant: int = 300) -> List[dict]:
    """SSD300 as a flat op list (reference Model.py:203-235).  Order matters only where a
    tensor has two consumers: in reverse order the consumer that cannot accumulate
    (L2-norm backward) must deliver its gradient first."""
    if variant not in (300, 512):
        raise ValueError("variant must be 300 or 512")
    anchors = ANCHORS_PER_CELL if variant == 300 else ANCHORS_PER_CELL_512
    f = "model.features."
    o = [dict(op="conv_first", p=f + "0", x="x", y="a1_1"),
         _conv(f + "2", "a1_1", "a1_2", 64, 64), _pool("a1_2", "p1"),
         _conv(f + "5", "p1", "a2_1", 64, 128), _conv(f + "7", "a2_1", "a2_2", 128, 128), _pool("a2_2", "p2"),
         _conv(f + "10", "p2", "a3_1", 128, 256), _conv(f + "12", "a3_1", "a3_2", 256, 256),
         _conv(f + "14", "a3_2", "a3_3", 256, 256), _pool("a3_3", "p3", ceil=True),            # Model.py:137
         _conv(f + "17", "p3", "a4_1", 256, 512), _conv(f + "19", "a4_1", "a4_2", 512, 512),
         _conv(f + "21", "a4_2", "a4_3", 512, 512),
         _pool("a4_3", "p4"),
         dict(op="l2norm", p="rescaling_conv_4_3", x="a4_3", y="n4_3"),                         # Model.py:206-209
         _head("c_4", "n4_3", 0, 512, anchors),
         _conv(f + "24", "p4", "a5_1", 512, 512), _conv(f + "26", "a5_1", "a5_2", 512, 512),
         _conv(f + "28", "a5_2", "a5_3", 512, 512), _pool("a5_3", "p5", k=3, s=1, pad=1, ceil=True),   # Model.py:142
         _conv("conv_fc6", "p5", "a6", 512, 1024, k=3, pad=4, dil=4),                            # Model.py:149
         _conv("conv_fc7", "a6", "a7", 1024, 1024, k=1, pad=0),
         _head("c_7", "a7", 1, 1024, anchors)]
    prev = "a7"
    for i, (name, cin, mid, cout, s, pad) in enumerate(_AUX_300 if variant == 300 else _AUX_512):
        n = 8 + i
        o.append(_conv(f"{name}.0", prev, f"a{n}a", cin, mid, k=1, pad=0))
        o.append(_conv(f"{name}.2", f"a{n}a", f"a{n}", mid, cout, k=3, s=s, pad=pad))
        o.append(_head(f"c_{n}", f"a{n}", 2 + i, cout, anchors))
        prev = f"a{n}"
    return o


def param_names(op_list: List[dict]) -> List[str]:
    names = []
    for op in op_list:
        if op["op"] in ("conv", "conv_first"):
            names += [op["p"] + ".weight", op["p"] + ".bias"]
        elif op["op"] == "l2norm":
            names.append(op["p"])
        elif op["op"] == "head":
            names += [op["p"] + "_bb.weight", op["p"] + "_bb.bias", op["p"] + "_cl.weight", op["p"] + "_cl.bias"]
    return names


def _cat_flat(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """cat((a, b)) of two 1-D parameters -- without a copy when b starts where a ends in one storage (ddp.py lays the loc and conf
    biases of a head side by side in its flat parameter buffer)."""
    if (a.dim() == 1 and b.dim() == 1 and a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr() and a.storage_offset() + a.numel() == b.storage_offset()):
        return torch.as_strided(a, (a.numel() + b.numel(),), (1,), a.storage_offset())
    return torch.cat((a, b))


@dataclass(frozen=True)
class _Layer:
    """A `conv` or `head` op as the engine's one convolution-layer path sees it, built once per op.  A head is a 3x3 / pad 1 convolution
    without ReLU whose filter is two parameter tensors stacked (loc rows, then conf rows) and whose output rows are padded to 32."""
    key: str                      # op["p"]: weight-cache key and profile label
    weights: Tuple[str, ...]      # parameter names: one filter, or a head's (_bb, _cl) pair ...
    biases: Tuple[str, ...]
    rows0: int                    # ... whose first tensor has this many output rows
    x: str
    y: Optional[str]              # the activation a conv produces; a head's output goes to the packed head list
    co: int
    co_pad: int                   # leading dimension of the output and of an f32 dy (conv: co; head: pad32(co))
    ld16: int                     # leading dimension of a bf16 dy (conv: co; head: pad64(co))
    conv: Tuple[int, int, int, int, int]      # ci, kernel size, stride, padding, dilation
    relu: bool
    head: bool
    first_dx: bool                # the last reader of its input: in the backward the first to deliver that input's gradient

    def geom(self, bs: int, h: int, w: int):
        return ops.make_geom(bs, h, w, self.conv[0], self.co, *self.conv[1:])

    def filter(self, P) -> tuple:
        return tuple(P[n] for n in self.weights)

    def bias(self, P) -> torch.Tensor:
        b = [P[n].detach() for n in self.biases]
        return b[0] if len(b) == 1 else _cat_flat(*b)

    def wanted(self, need) -> bool:
        return any(need[n] for n in self.weights + self.biases)

    def hand(self, grads, dw, db) -> None:
        """The layer's (dw, db) to its parameters' entries of the gradient table: a head's rows split into loc and conf."""
        if len(self.weights) == 1:
            grads[self.weights[0]], grads[self.biases[0]] = dw, db
        else:
            r = self.rows0
            grads[self.weights[0]], grads[self.weights[1]] = dw[:r], dw[r:]
            grads[self.biases[0]], grads[self.biases[1]] = db[:r], db[r:]


def _stacked(tensors) -> torch.Tensor:
    """The filter of a layer as one OIHW tensor (a head's loc and conf rows stacked)."""
    return tensors[0] if len(tensors) == 1 else torch.cat(list(tensors), 0)


@dataclass
class _Filter:
    """One layer's filter re-laid in one layout family (`_FAMILIES`): what the weight cache holds."""
    sig: tuple                                  # (data_ptr, _version) per source tensor (+ limb-GEMM form, adjoint flag: Winograd)
    fwd: torch.Tensor                           # the forward's layout
    bwd: Optional[torch.Tensor] = None          # the data gradient's layout (`layout`: built on first request)
    fwd_limbs: Optional[torch.Tensor] = None    # `layout`, f32x3 and bf16-operand modes: the bf16 limb planes of fwd / bwd
    bwd_limbs: Optional[torch.Tensor] = None
    oihw: Optional[torch.Tensor] = None         # `layout`, built per layer: the stacked OIHW source a later bwd is made from


@dataclass(frozen=True)
class _Family:
    """One filter layout family: how its record is built for one layer, and how the batched weight table builds the same."""
    slot: str                                   # family part of the cache key (the two Winograd forms share one slot per layer)
    job: int                                    # kind number of its `ssd_weights_prepare` job
    alloc: Callable                             # (co, ci, taps, co_pad, device) -> (fwd, bwd or None): the job's output buffers
    build: Callable                             # (engine, layer, contiguous stacked OIHW filter, adj) -> (fwd, bwd or None), per layer
    adj: bool = False                           # Winograd: bwd in the adjoint form
    job_fields: Callable = lambda co, bwd: {}   # what its job sets besides the common fields
    lazy: Optional[Callable] = None             # (engine, layer, record, need_bwd): fields filled on request, at every lookup


def _build_wino(eng, L, w, adj):
    uf, ub = ops.wino_weights(w, L.co_pad, want_bwd=not adj, mo=eng.WINO_TILE)
    return uf, ops.wino_adj_weights(w, L.co_pad) if adj else ub


def _layout_on_request(eng, L, rec, need_bwd):
    if need_bwd and rec.bwd is None:
        rec.bwd = ops.weight_ihwo(rec.oihw, L.co_pad)
    if eng.x3 or (eng.bf16 and not eng.bf16_tensors):         # pre-split limb planes of the layouts in use
        if rec.fwd_limbs is None:
            rec.fwd_limbs = ops.weight_split3(rec.fwd)
        if need_bwd and rec.bwd_limbs is None:
            rec.bwd_limbs = ops.weight_split3(rec.bwd)


# Keyed by what `_Engine._table_kind` answers, plus conv1_1's own family.  A new family is a row here and an answer there.
_FAMILIES: Dict[str, _Family] = {
    "first": _Family("first", 2, lambda co, ci, taps, co_pad, dev: (ops.first_rows_alloc(co, dev), None),       # conv1_1: [64][32] rows
                     lambda eng, L, w, adj: (ops.first_weight_rows(w), None)),
    "layout": _Family("layout", 1,                             # direct kernels: OHWI [co_pad][T][Ci] / IHWO [Ci][T][co_pad]
                      lambda co, ci, taps, co_pad, dev: tuple(ops.layout_filter_alloc(ci, taps, co_pad, dev, bwd=b) for b in (False, True)),
                      lambda eng, L, w, adj: (ops.weight_ohwi(w, L.co_pad), None), lazy=_layout_on_request),
    "wino": _Family("wino", 0,                                 # Winograd domain: U_fwd [P][Co][Ci], U_bwd [P][Ci][co_pad] of the rotated filter
                    lambda co, ci, taps, co_pad, dev: (ops.wino_filter_alloc(4, co, ci, dev), ops.wino_filter_alloc(4, ci, co_pad, dev)),
                    _build_wino),
    "x31": _Family("x31", 4,                                   # limb planes of a 1x1 filter and of its transpose
                   lambda co, ci, taps, co_pad, dev: (ops.x3_filter_alloc(co, ci, dev), ops.x3_filter_alloc(ci, co_pad, dev)),
                   lambda eng, L, w, adj: ops.conv1x1_weights_x3(w, L.co_pad)),
    "b16": _Family("b16", 3,                                   # bf16 OHWI / IHWO copies of a 3x3 filter; the job's row counts are the buffers'
                   lambda co, ci, taps, co_pad, dev: tuple(ops.bf16_filter_alloc(co, ci, dev, bwd=b) for b in (False, True)),
                   lambda eng, L, w, adj: ops.weights_bf16(w), job_fields=lambda co, bwd: dict(co_pad=co, pad1=int(bwd.shape[2]))),
}
# ... U_bwd instead the forward transform laid out [Ci][co_pad], for the adjoint data gradient
_FAMILIES["wino_adj"] = replace(_FAMILIES["wino"], adj=True, job_fields=lambda co, bwd: dict(adj=True))

# A training forward's batched weight table: what it was built for, the `ops.WeightTable`, per job (family name, layer, fwd buffer, bwd or None)
_TableFill = namedtuple("_TableFill", "sig table entries")


class _FilterCache(dict):
    """The engine's re-laid filters: (family slot, layer key) -> `_Filter`.  `clear()` drops the records; the weight table `fill`,
    whose buffers persist across steps, stays."""
    fill: Optional[_TableFill] = None

    @staticmethod
    def sig(fam: _Family, L: _Layer, P) -> tuple:
        sig = tuple((t.data_ptr(), t._version) for t in L.filter(P))
        return sig + (ops.wino_x3(4, 256), fam.adj) if fam.slot == "wino" else sig      # + the GEMM form the filters were laid out for

    def lookup(self, fam: _Family, L: _Layer, P, build: Callable) -> _Filter:
        """The layer's record in this family if it was made from what `sig` sees now; else build(sig, the layer's contiguous stacked
        OIHW filter), stored in its place."""
        sig, at = self.sig(fam, L, P), (fam.slot, L.key)
        rec = self.get(at)
        if rec is None or rec.sig != sig:
            rec = self[at] = build(sig, _stacked(L.filter(P)).detach().contiguous())
        return rec

    def tensors(self) -> list:
        """Every tensor of every record (what a captured graph that read them must keep alive)."""
        return [t for r in self.values() for t in (r.fwd, r.bwd, r.fwd_limbs, r.bwd_limbs, r.oihw) if t is not None]

    def kinds(self) -> Dict[str, str]:
        """{layer key: family name} of the last table filling (kept, like the table, across `clear()`)."""
        return {} if self.fill is None else {L.key: name for name, L, _, _ in self.fill.entries}


# What `_Engine._path` answers for one layer:
#   kind        "b16" (csrc/conv_bf16.hip on bf16 tensors) | "wino" (Winograd F(4x4) / F(2x2)) | "x31" (1x1 limb GEMMs) | "direct" (igemm)
#   cast16      b16: the input is an f32 tensor and the layer (a head) runs on a bf16 copy of it; its dx goes back as f32
#   adj         wino, training: the backward filter is laid out for the adjoint data gradient
#   keep        wino, training: the forward keeps its F(4x4) input planes for the Winograd weight gradient
#   bits        wino, training: the input transform also leaves the ReLU mask of its input as bits
#   pool        wino: the 2x2 / stride-2 pool op fused into the output transform, or None
#   wino_wgrad  the weight gradient runs in the Winograd domain (else: the fused direct kernels, or the path's own)
_Path = namedtuple("_Path", "kind cast16 adj keep bits pool wino_wgrad", defaults=(False, False, False, False, None, False))


class _Elided:
    """Stands in the activation table for a tensor that a fused kernel consumed without writing it: shape only.  In the backward it
    takes the ReLU-mask slot of its pool, which then gates by the pooled output (`maxpool_bwd(..., y_gate=)`)."""

    dtype = torch.float32

    def __init__(self, shape):
        self.shape = tuple(shape)


class _SinkDict(dict):
    """Gradient table of one backward pass that tells a listener about every entry as soon as it exists (ddp.py starts the
    all-reduce of a bucket when its last gradient has been computed, while the rest of the backward is still running).

    The listener is only ever called with the CALLER's stream current and with the producing kernel ordered before that stream's
    position: gradients produced on the engine's side stream are held (`hold()`) until the caller's stream has waited for the side
    stream's event (`release()`), so a collective the listener starts can never read a gradient that is still being written."""

    def __init__(self, sink):
        super().__init__()
        self._sink = sink
        self._held = None

    def __setitem__(self, name, tensor):
        super().__setitem__(name, tensor)
        if self._held is not None:
            self._held.append((name, tensor))
        else:
            self._sink(name, tensor)

    def hold(self):
        if self._held is None:
            self._held = []

    def release(self):
        held, self._held = self._held or [], None
        for name, tensor in held:
            self._sink(name, tensor)


class _Engine:
    """Runs the op list on the current HIP stream.  Holds only caches (re-laid-out weights)."""

    def __init__(self, variant: int = 300, n_conf: int = N_CLASSES):
        ops_ = build_ops(variant)
        self.n_conf = n_conf                      # width of the conf rows (foreground classes + background)
        self.names = param_names(ops_)            # parameter order of the autograd Function: the reference's forward order
        # Schedule: [backbone ... seq8] then [L2-norm, c_4, c_7: big MFMA-bound head convolutions] then [c_8, seq9 ... c_11: a dozen tiny
        # maps (10x10 ... 1x1) whose ~60 launches per direction are latency-bound].  The last group runs on a second HIP stream beside
        # the middle one, forward and backward: it depends only on a8, and nothing but its own ops reads what it produces.
        late = [o for o in ops_ if o["op"] == "l2norm" or (o["op"] == "head" and o["p"] in ("c_4", "c_7"))]
        k8 = next(i for i, o in enumerate(ops_) if o["op"] == "conv" and o["y"] == "a8")
        side = [o for i, o in enumerate(ops_) if i > k8 and o not in late]
        early = [o for o in ops_ if o not in late and o not in side]
        self.ops = early + late + side
        self._side_ids = {id(o) for o in side}
        self._late_first = id(late[0])
        self.defer_tail_wgrad = True              # backward: the side group's weight gradients after its data-gradient chain, behind the join
        self.overlap_tail = True                  # False: everything on the caller's stream (bit-identical; interleaved A/B: 26.09 -> 25.85 ms)
        self._side_stream = None
        # Backward: the Winograd weight-gradient GEMMs (MFMA-bound, nothing waits for them) on their own stream beside the chain
        # dy transform -> dgrad GEMM -> output transform -> next layer's dy transform, whose transforms are HBM-bound.  Opt-in: measured
        # +-0.2 ms (the GEMMs end up beside other GEMMs, the transform kernels leave no room on the CUs), and the planes that cross the
        # streams (GBs per layer, held by record_stream until the other stream has passed) make torch's caching allocator reserve
        # 180 GB instead of 19.
        self.overlap_wgrad = False
        self._wgrad_stream = None
        self.batch_weights = True     # training forward: all ~56 filter transforms / re-layouts of the step in ONE launch (ops.WeightTable)
        self._wcache = _FilterCache()
        self.consumers: Dict[str, int] = {}
        for op in self.ops:
            self.consumers[op["x"]] = self.consumers.get(op["x"], 0) + 1
        self.relu_out = {op["y"] for op in self.ops if op["op"] == "conv_first" or (op["op"] == "conv" and op["relu"])}
        # conv -> ReLU -> MaxPool2d(2, 2) where nothing else reads the convolution (conv1_2, conv2_2, conv3_3): one fused pass
        self.pool_after: Dict[str, dict] = {}
        for op in self.ops:
            readers = [o for o in self.ops if o["x"] == op["y"]] if op["op"] == "conv" else []
            if (len(readers) == 1 and readers[0]["op"] == "pool" and (readers[0]["k"], readers[0]["s"], readers[0]["pad"]) == (2, 2, 0)
                    and op["relu"] and op["co"] % 4 == 0):
                self.pool_after[op["y"]] = readers[0]
        self._conv_of = {o["y"]: o for o in self.ops if o["op"] == "conv"}      # producer of an activation, where that is a convolution
        self.layers: Dict[str, _Layer] = {}       # op["p"] -> description of every conv / head op
        for op in self.ops:
            if op["op"] not in ("conv", "head"):
                continue
            p, head = op["p"], op["op"] == "head"
            co = op["a"] * (4 + n_conf) if head else op["co"]
            self.layers[p] = _Layer(
                key=p, x=op["x"], y=None if head else op["y"], head=head, relu=not head and op["relu"],
                weights=(p + "_bb.weight", p + "_cl.weight") if head else (p + ".weight",),
                biases=(p + "_bb.bias", p + "_cl.bias") if head else (p + ".bias",),
                rows0=4 * op["a"] if head else co, co=co, co_pad=ops.pad32(co) if head else co, ld16=ops.pad64(co) if head else co,
                conv=(op["ci"], 3, 1, 1, 1) if head else (op["ci"], op["k"], op["s"], op["pad"], op["dil"]),
                first_dx=[o for o in self.ops if o["x"] == op["x"]][-1] is op)
        p = self.ops[0]["p"]          # conv_first has a path of its own; the weight cache sees it as one more layer
        self._first = _Layer(key=p, x="x", y=self.ops[0]["y"], head=False, relu=True, weights=(p + ".weight",), biases=(p + ".bias",),
                             rows0=64, co=64, co_pad=64, ld16=64, conv=(3, 3, 1, 1, 1), first_dx=True)
        self.grad_sink = None     # callable(name, gradient): called during backward the moment a parameter's gradient is ready
        self.grad_out = None      # callable(names) -> flat f32 tensor or None: where the gradient of these consecutive parameters is to be written
        self.sink_owns_grads = False   # True (ddp.py): gradients live in the listener's buffer, autograd is handed None for them
        self.sink_early = False        # True: the listener acts on a gradient at once (overlapped all-reduce), so side-stream gradients are joined early
        self._test_side_delay = None   # tests: callable run on the side stream in front of the deferred weight gradients
        self.grad_tap = None           # tests: dict that receives every activation's finished gradient tensor (name -> dX as the backward stored it)
        self.dual_dy = True       # backward: one pass over dy writes the planes of the weight gradient AND of the data gradient
        self.keep_planes = True   # training forward keeps the F(4x4) input planes of the layers whose weight gradient is Winograd
        self.fuse_pool = True     # Winograd F(4x4) layers in pool_after write the pooled map + argmax only ...
        self.lazy_pool_grad = True     # ... and in the backward their dy pass reads the pooled gradient: the pool's dx is never written
        self.first_fused = True        # conv1_1 forward and weight gradient straight from the NCHW batch (csrc/conv_first.hip), no im2col rows
        self.wino_dilated = True       # fc6 (3x3, dilation 4) in the Winograd domain too: 49 tiles x 36 products per image instead of 361 x 9
        self.relu_bits = True     # training forward: the input transform also leaves the ReLU mask of its input as bits for the dgrad epilogue
        # Round 4: data gradient of the F(4x4) layers with >= 256 output channels in the ADJOINT Winograd form -- it multiplies the planes
        # A dy A^T the weight gradient already has (no second plane set B^T dy B), and between two such layers of one resolution
        # (conv3_3 -> 3_2 -> 3_1, conv4_3 -> 4_2 -> 4_1, conv5_3 -> 5_2 -> 5_1) the gradient tensor itself is never written: the output
        # transform of the upper layer's data gradient writes the lower layer's dy planes (csrc/winograd.hip wino4_adj_out_kernel)
        self.adjoint_dgrad = True
        # Round 4 experiment (SSD_EXPERIMENTAL builds): conv1_1 writes conv1_2's Winograd input planes (+ ReLU bits) itself; its 64-channel
        # activation -- read by nothing else -- is never stored (csrc/conv_first.hip conv_first_wino_kernel; bit-identical planes).  Measured
        # SLOWER than the two kernels it replaces (0.96 vs 0.25 + 0.52 ms; step 20.16 vs 19.97): off
        self.first_wino = False
        self.adjoint_chain = True      # False: every adjoint data gradient is written out as a tensor (A/B aid)
        self.prof = None          # bench.py: list collecting (label, kernel tag, flops, start event, end event)
        self.bf16 = False         # True: forward / dgrad / fused-wgrad convolutions multiply bf16-rounded operands (f32 accumulate)
        # bf16 mode: the VGG trunk (conv1_1 ... pool5, the L2-norm and the c_4 head's input) keeps its activations and gradients in bf16 in
        # HBM -- written once by the producing kernel -- and runs csrc/conv_bf16.hip (LDS-DMA halo kernel), the bf16-input nine-tap weight
        # gradient and the bf16 pools / L2-norm; fc6 onwards (19x19 maps and smaller) stays on the f32-tensor bf16-operand kernels.
        # False: the round-2 form (every tensor f32 in HBM, operands rounded on their way into LDS).
        self.bf16_tensors = True
        self.x3 = False           # True: forward / dgrad convolutions form f32 products from three bf16 limbs per operand
        self.wino = True          # f32 mode: Winograd F(4x4,3x3) (WINO_TILE) for the 3x3 / stride-1 layers with >= WINO_MIN_CI input channels

    def _timed(self, label, tag, flops, fn):
        """Run fn(); when profiling, bracket it with HIP events on the current stream."""
        if self.prof is None:
            return fn()
        executed = flops
        if isinstance(flops, tuple):          # (direct-convolution FLOPs, FLOPs the Winograd GEMMs execute)
            flops, executed = flops
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        self.prof.append((label, tag, flops, e0, e1, executed))
        return out

    def schedule_key(self) -> tuple:
        """Every setting that decides which kernels a step runs, or in what form (dtype mode, Winograd and its thresholds, the fused
        and adjoint forms, the library's limb-GEMM switch).  The training weight table is keyed by it, and so is a captured train
        step (ddp.GraphedTrainStep): a flag flipped between two steps rebuilds the one and re-captures the other.  Stream placement
        (`overlap_tail`, `defer_tail_wgrad`) is not in it: it changes where the kernels run, not which."""
        return (self.bf16, self.bf16_tensors, self.x3, self.wino, self.WINO_TILE, self.WINO_MIN_CI, self.WINO_MIN_HW,
                self.WINO_WGRAD_MAX_HW, self.WINO_WGRAD_MIN_CI, self.X31_MIN_PIXELS, ops.wino_x3(4, 256), self.adjoint_dgrad,
                self.adjoint_chain, self.keep_planes, self.dual_dy, self.fuse_pool, self.lazy_pool_grad, self.relu_bits, self.wino_dilated,
                self.first_fused, self.first_wino, self.overlap_wgrad, self.batch_weights)

    def uses_weight_table(self) -> bool:
        """A training forward lays out all its filters through the batched weight table (`_prepare_weights_batched`)."""
        return self.batch_weights and not self.x3 and (not self.bf16 or self.bf16_tensors)

    # -- weights ----------------------------------------------------------------------------
    def _filter(self, what: str, L: _Layer, P, need_bwd: bool = False) -> _Filter:
        """THE lookup of a layer's re-laid filter in the family `what` (a name of `_FAMILIES`): the cached record while its signature
        holds (`_FilterCache.sig`), else built for this layer alone.  need_bwd: the caller reads the data gradient's layout."""
        fam = _FAMILIES[what]
        rec = self._wcache.lookup(fam, L, P, lambda sig, w: _Filter(sig, *fam.build(self, L, w, fam.adj), oihw=w if fam.lazy else None))
        if fam.lazy:
            fam.lazy(self, L, rec, need_bwd)
        return rec

    WINO_TILE = 4                 # forward / dgrad output tile: F(4x4,3x3) (36 multiplies per 16 outputs; ~1e-5 of the output scale) or 2
    WINO_WGRAD_MAX_HW = 512       # Winograd weight gradient on maps up to this size and from this many input channels.  Steps measured in
    WINO_WGRAD_MIN_CI = 64        # the train step: (80, 256) 985 -> (150, 128) 1018 images/s; once the forward planes were kept and one pass
                                  # over dy fed both gradients, the 64-channel layers paid too: + conv2_1 +0.7 %, + conv1_2 +3.8 %
    WINO_MIN_HW = 8               # maps below this (heads c_9 .. c_11: 5x5, 3x3, 1x1) take the direct kernel: one launch instead of five
    WINO_MIN_CI = 64              # measured in the step with F(4x4): 256 -> 836, 128 -> 872, 64 -> 879 images/s (F(2x2): only >= 256 paid)

    def _wino_ok(self, g) -> bool:
        # dilation d = padding (fc6, Model.py:149): d x d plain 3x3 convolutions on the sub-lattices of the map, F(4x4) tiles on each
        dil_ok = g.dil == 1 or (self.wino_dilated and self.WINO_TILE == 4 and 2 <= g.dil <= 4)
        return (self.wino and not self.bf16 and not self.x3 and g.R == 3 and g.S == 3 and g.stride == 1 and dil_ok and g.pad == g.dil
                and g.Ci % 32 == 0 and g.Ci >= self.WINO_MIN_CI and g.H >= self.WINO_MIN_HW)

    X31_MIN_PIXELS = 8192         # 1x1 layers on the limb GEMMs from this many output pixels (fc7, seq8.0 at batch 32: 11 552; below, the
                                  # 128 x 128 tiles leave most CUs idle and the split-K f32 kernel wins)

    def _x31_ok(self, g) -> bool:
        """f32 mode: this 1x1 / stride-1 convolution runs the three-limb GEMM kernels (forward, data gradient, weight gradient)."""
        return (self.wino and not self.bf16 and not self.x3 and ops.wino_x3(4, 256) and g.R == 1 and g.S == 1 and g.stride == 1 and g.pad == 0
                and g.Ci % 32 == 0 and g.Ci >= 256 and g.Co % 32 == 0 and g.Co >= 128 and g.N * g.H * g.W >= self.X31_MIN_PIXELS)

    def _wino_wgrad_ok(self, g, head: bool) -> bool:
        """Weight gradient of this layer in the Winograd domain (else: the fused direct kernels)."""
        return (self._wino_ok(g) and g.H <= self.WINO_WGRAD_MAX_HW and g.Ci >= self.WINO_WGRAD_MIN_CI
                and (g.H >= 19 if head else g.Co % 4 == 0))

    def _adj_ok(self, g) -> bool:
        """This convolution's data gradient takes the adjoint Winograd form (needs the kept forward planes: its weight gradient is the
        Winograd one and shares the dy planes; reduction long enough for the plane GEMM kernels, i.e. not the fused K <= 128 kernel)."""
        return (self.adjoint_dgrad and self.keep_planes and self.dual_dy and not self.overlap_wgrad and self.WINO_TILE == 4 and self._wino_ok(g) and g.dil == 1
                and self._wino_wgrad_ok(g, False) and g.Co % 32 == 0 and 256 <= g.Co <= 1024 and g.Ci % 4 == 0)

    def _first_wino_ok(self, op, bs, x) -> bool:
        """conv1_1's output goes straight into the input planes of the layer behind it: that layer is its only reader and an F(4x4) one."""
        if not (self.first_wino and ops.has_experimental() and self.wino and self.WINO_TILE == 4 and self.consumers.get(op["y"], 0) == 1):
            return False
        nxt = next((o for o in self.ops if o["op"] == "conv" and o["x"] == op["y"]), None)
        if nxt is None or nxt["ci"] != 64:
            return False
        g = ops.make_geom(bs, x.shape[2], x.shape[3], nxt["ci"], nxt["co"], nxt["k"], nxt["s"], nxt["pad"], nxt["dil"])
        return self._wino_ok(g) and g.dil == 1 and g.Co % 4 == 0 and not ops.wino_uses_full(g, 0)

    def _t16(self, g) -> bool:
        """bf16-tensor mode: this convolution, given a bf16 input, runs csrc/conv_bf16.hip (3x3 / stride 1 / pad 1, Ci a multiple of 64)."""
        return self.bf16 and self.bf16_tensors and g.R == 3 and g.S == 3 and g.stride == 1 and g.dil == 1 and g.pad == 1 and g.Ci % 64 == 0

    def _head16(self, L: _Layer, g) -> bool:
        """bf16-tensor mode: this head, although its input is an f32 tensor, runs csrc/conv_bf16.hip on a bf16 copy of it -- where the map is
        large enough to pay (19x19) and the head is the FIRST to deliver its input's gradient (so that gradient needs neither += nor a
        ReLU mask from the kernel, which writes it as f32)."""
        return L.head and L.first_dx and self._t16(g) and g.H >= 16

    def _path(self, L: _Layer, g, x_is_b16: bool, save: bool = True) -> _Path:
        """THE dispatch decision of a conv / head layer: which kernel family it runs on, given its geometry and whether its input is held
        in bf16, and the sub-decisions that go with the family (the fields of `_Path`).  The forward records the answer in `aux`, the
        backward reads it back, the weight table (`_plan`) lays out the filters it names: nothing else looks at the predicates."""
        if self._t16(g) and (x_is_b16 or self._head16(L, g)):
            return _Path("b16", cast16=not x_is_b16)
        if self._wino_ok(g):
            t4 = self.WINO_TILE == 4
            wino_wgrad = self._wino_wgrad_ok(g, L.head)
            # training: the transformed input stays for the weight gradient, which multiplies the same planes
            keep = save and self.keep_planes and t4 and wino_wgrad
            if L.head:                                  # no ReLU in front of a head's dx, no pool behind it, no adjoint form
                return _Path("wino", keep=keep, wino_wgrad=wino_wgrad)
            # the mask is only ever applied to a post-ReLU input (deliver() in the backward): pool outputs and the image are not gated here
            bits = keep and self.relu_bits and self.dual_dy and L.x in self.relu_out and g.Co % 32 == 0
            pool = self.pool_after.get(L.y) if (self.fuse_pool and t4) else None
            return _Path("wino", adj=save and self._adj_ok(g), keep=keep, bits=bits, pool=pool, wino_wgrad=wino_wgrad)
        if self._x31_ok(g):
            return _Path("x31")
        return _Path("direct")

    def _plan(self, bs: int, h: int, w: int, save: bool = True):
        """(op, layer, geometry, path) of every conv / head op for a batch of bs images of h x w, without running anything: the map sizes
        follow from the ops in front, and a tensor is held in bf16 where the path of its producer says so."""
        hw, b16 = {"x": (h, w)}, {"x": False}
        for op in self.ops:
            kind = op["op"]
            if kind in ("conv", "head"):
                L = self.layers[op["p"]]
                g = L.geom(bs, *hw[op["x"]])
                path = self._path(L, g, b16[op["x"]], save)
                if kind == "conv":
                    hw[op["y"]], b16[op["y"]] = (g.Ho, g.Wo), path.kind == "b16"
                yield op, L, g, path
            elif kind == "pool":
                hw[op["y"]] = tuple(ops.pool_out(n, op["k"], op["s"], op["pad"], op["ceil"]) for n in hw[op["x"]])
                b16[op["y"]] = b16[op["x"]]
            else:                                       # conv_first (bf16 out in the bf16-tensor mode), l2norm
                hw[op["y"]] = hw[op["x"]]
                b16[op["y"]] = (self.bf16 and self.bf16_tensors) if kind == "conv_first" else b16[op["x"]]

    def _table_kind(self, path: _Path) -> Optional[str]:
        """What the batched weight table lays out for a layer on this path; None: nothing (F(2x2), a tuning aid, is transformed per layer)."""
        if path.kind == "wino":
            return None if self.WINO_TILE != 4 else "wino_adj" if path.adj else "wino"
        return {"b16": "b16", "x31": "x31", "direct": "layout"}[path.kind]

    def _prepare_weights_batched(self, x: torch.Tensor, P: Dict[str, torch.Tensor]) -> None:
        """Fill the weight cache for a training step with one launch.  The output buffers persist across steps (rewritten in place, on the
        caller's stream, after the previous step's last use); the job table is rebuilt only when a parameter's storage or the input
        size changes."""
        sig = (x.shape[2], x.shape[3]) + self.schedule_key() + tuple(P[n].data_ptr() for n in self.names)
        fill = self._wcache.fill
        if fill is None or fill.sig != sig:
            jobs, entries = [], []
            layers = [("first", self._first, 3, 9)] + [(self._table_kind(path), L, g.Ci, g.R * g.S)
                                                       for _, L, g, path in self._plan(x.shape[0], x.shape[2], x.shape[3])]
            for what, L, ci, taps in (row for row in layers if row[0] is not None):
                fam, tensors = _FAMILIES[what], L.filter(P)
                co = sum(t.shape[0] for t in tensors)
                fwd, bwd = fam.alloc(co, ci, taps, L.co_pad, x.device)
                jobs.append(dict(dict(kind=fam.job, w0=tensors[0].detach(), w1=tensors[1].detach() if len(tensors) > 1 else None,
                                      co0=tensors[0].shape[0], co=co, ci=ci, taps=taps, co_pad=L.co_pad, out_fwd=fwd, out_bwd=bwd),
                                 **fam.job_fields(co, bwd)))
                entries.append((what, L, fwd, bwd))
            fill = self._wcache.fill = _TableFill(sig, ops.WeightTable(jobs, x.device), entries)
        fill.table.run()
        for what, L, fwd, bwd in fill.entries:            # the records `_filter` would have built
            fam = _FAMILIES[what]
            self._wcache[(fam.slot, L.key)] = _Filter(self._wcache.sig(fam, L, P), fwd, bwd)

    # -- forward ----------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, P: Dict[str, torch.Tensor], save: bool):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"SSD_300 expects (bs,3,H,W) NCHW input, got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise ValueError("SSD_300 expects float32 input")
        if not x.is_cuda:
            raise RuntimeError("SSD_300 runs on the gfx950 HIP kernels only: move the model and the input to the GPU "
                               "(there is no CPU fallback)")
        x = x.contiguous()
        bs = x.shape[0]
        if save:
            # A training forward re-lays every weight: the parameters change each step anyway, and the cache key
            # (data_ptr, _version) cannot see writes through `.data` (p.data.mul_(), dist.broadcast(p.data), EMA swaps).
            # The backward of this step reads what this forward stored.
            self._wcache.clear()
            if self.uses_weight_table():
                self._prepare_weights_batched(x, P)
        T = {"x": x}
        aux = {}
        heads = []
        main = torch.cuda.current_stream(x.device)
        overlap = self.overlap_tail and bool(self._side_ids)
        if overlap and self._side_stream is None:
            self._side_stream = torch.cuda.Stream(device=x.device)
        side, fork = self._side_stream, None
        side_ctx = [None]              # the stream context of the side group, left in `finally`: an exception must not leave the side stream current
        try:
            self._forward_ops(x, P, save, T, aux, heads, main, side, side_ctx, overlap, bs)
        finally:
            if side_ctx[0] is not None:
                side_ctx[0].__exit__(None, None, None)
        if side_ctx[0] is not None:
            for op, packed, _ in heads:
                if id(op) in self._side_ids:
                    packed.record_stream(main)
            main.wait_event(side.record_event())
        heads.sort(key=lambda h: h[0]["scale"])                   # prior order: c_4, c_7, c_8, ... (Model.py:235)
        P_total = sum(g.Ho * g.Wo * op["a"] for op, _, g in heads)
        loc = torch.empty((bs, P_total, 4), device=x.device, dtype=torch.float32)
        conf = torch.empty((bs, P_total, self.n_conf), device=x.device, dtype=torch.float32)
        off = 0
        offs = {}
        for op, packed, g in heads:
            ops.heads_scatter(packed, ops.pad32(g.Co), loc, conf, bs, g.Ho * g.Wo, op["a"], off)
            offs[op["p"]] = (off, g)
            off += g.Ho * g.Wo * op["a"]
        saved = dict(T=T, aux=aux, offs=offs, bs=bs) if save else None
        return loc, conf, saved

    def _forward_ops(self, x, P, save, T, aux, heads, main, side, side_ctx, overlap, bs):
        fork = None
        for op in self.ops:
            kind = op["op"]
            if overlap and id(op) == self._late_first:
                fork = main.record_event()                        # a8 (and everything before it) is enqueued
            if overlap and side_ctx[0] is None and id(op) in self._side_ids:
                side.wait_event(fork)
                T[op["x"]].record_stream(side)
                side_ctx[0] = torch.cuda.stream(side)
                side_ctx[0].__enter__()
            if kind == "conv_first":
                g = ops.make_geom(bs, x.shape[2], x.shape[3], 32, 64, 1, 1, 0, 1)
                rows, bias = self._filter("first", self._first, P).fwd, self._first.bias(P)
                flops1 = 2.0 * bs * g.Ho * g.Wo * 64 * 27
                if self.bf16 and self.bf16_tensors:
                    # bf16-tensor mode: operands rounded to bf16 inside the kernel, bf16 NHWC out; the weight gradient reads x itself
                    T[op["y"]] = self._timed("fwd " + op["p"], "conv_first_fwd_kernel", flops1,
                                             lambda: ops.conv1_first_fwd_bf16(x, rows, bias, True))
                    col = None
                elif (self.first_fused and not self.bf16 and not self.x3 and self._first_wino_ok(op, bs, x)
                      and (not save or (self.relu_bits and self.dual_dy and self.keep_planes))):
                    # ... and, where its only reader is a Winograd layer, straight into that layer's input planes: no activation tensor at all
                    pre = self._timed("fwd " + op["p"], "conv_first_fwd_kernel", flops1,
                                      lambda: ops.conv1_first_wino_fwd(x, rows, bias, want_bits=save and self.relu_bits))
                    T[op["y"]] = _Elided((bs, x.shape[2], x.shape[3], 64))
                    aux["preplanes:" + op["y"]] = pre
                    col = None
                elif self.first_fused and not self.bf16 and not self.x3:
                    # one kernel from the NCHW batch: halo tile in LDS, K = 27 on the MFMA, bias + ReLU; the weight gradient's rows ride along
                    T[op["y"]], col = self._timed("fwd " + op["p"], "conv_first_fwd_kernel", flops1,
                                                  lambda: ops.conv1_first_fwd(x, rows, bias, True, want_col=False))
                else:
                    # conv1_1 as im2col (K = 27 -> 32) + the 1x1 MFMA convolution
                    col = ops.im2col_first(x)
                    T[op["y"]] = self._timed("fwd " + op["p"], ops.igemm_tile(g, 0, self.bf16, self.x3) if self.prof is not None else "", flops1,
                                             lambda: ops.conv2d_fwd(col, rows, bias, g, True, bf16=self.bf16))
                T["x_col"] = col
                aux[op["y"]] = g
            elif kind in ("conv", "head"):
                L = self.layers[op["p"]]
                xin = T[op["x"]]
                g = L.geom(bs, xin.shape[1], xin.shape[2])
                path = aux["path:" + L.key] = self._path(L, g, xin.dtype == torch.bfloat16, save)
                y = self._conv_forward(L, g, path, xin, P, save, T, aux)
                if L.head:
                    heads.append((op, y, g))
                else:
                    T[op["y"]], aux[op["y"]] = y, g
            elif kind == "pool":
                if op["y"] in T:                                  # produced by the convolution before it
                    continue
                y, am = ops.maxpool_fwd(T[op["x"]], op["k"], op["s"], op["pad"], op["ceil"], want_argmax=save)
                T[op["y"]] = y
                aux[op["y"]] = am
            elif kind == "l2norm":
                T[op["y"]] = ops.l2norm_fwd(T[op["x"]], P[op["p"]].detach().reshape(-1))

    def _conv_forward(self, L: _Layer, g, path: _Path, xin, P, save, T, aux):
        """Forward of one convolution layer, trunk or head, on the path `_path` chose -> its output (N, Ho, Wo, L.co_pad), or the `_Elided`
        stand-in where the pool behind it was fused (the pooled map and its argmax are then stored under the pool's name)."""
        bias, label = L.bias(P), "fwd " + L.key
        if path.kind == "b16":
            if path.cast16:
                # a head on an f32 tensor outside the bf16 trunk (c_7 on fc7's output): one cast, then the LDS-DMA kernel
                xin = T[L.x + ":b16"] = ops.cast_bf16(xin)
            wf16 = self._filter("b16", L, P).fwd
            if not L.head:
                return self._timed(label, "conv3x3_bf16_kernel", ops.conv_flops(g), lambda: ops.conv3x3_bf16(xin, wf16, bias, L.co, L.relu))
            # a head's rows go to the scatter as f32 with its leading dimension
            out = torch.empty((g.N, g.H, g.W, L.co_pad), device=xin.device, dtype=torch.float32)      # pad columns are never read
            return self._timed(label, "conv3x3_bf16_kernel", ops.conv_flops(g),
                               lambda: ops.conv3x3_bf16(xin, wf16, bias, (L.co + 3) // 4 * 4, False, out=out, out_f32=True, ldo=L.co_pad))
        if xin.dtype == torch.bfloat16:
            # boundary of the bf16 trunk (pool5 -> fc6): the kernels below take f32 tensors; a copy another reader made is reused
            xin = T[L.x + ":f32"] = T.get(L.x + ":f32") if T.get(L.x + ":f32") is not None else ops.cast_f32(xin)
        if path.kind == "wino":
            uf = self._filter("wino_adj" if path.adj else "wino", L, P).fwd
            pl, keep, wb = path.pool, path.keep, path.bits
            pre = aux.pop("preplanes:" + L.x, None)
            if pre is not None:
                # the producer of this layer's input left the input planes (and the ReLU bits): GEMMs + output transform only
                planes, pbits = pre
                if pl is not None:
                    yp, am = self._timed(label, "winograd_3x3", ops.wino_flops(g),
                                         lambda: ops.conv2d_fwd_wino_from_planes(planes, uf, bias, g, True, pool_ceil=pl["ceil"], want_argmax=save))
                    y = _Elided((g.N, g.H, g.W, L.co))
                    T[pl["y"]], aux[pl["y"]] = yp, am
                else:
                    y = self._timed(label, "winograd_3x3", ops.wino_flops(g), lambda: ops.conv2d_fwd_wino_from_planes(planes, uf, bias, g, L.relu))
                if keep:
                    aux["planes:" + L.key] = planes
                if wb and pbits is not None:
                    aux["bits:" + L.key] = pbits
                return y
            if pl is not None:
                res = self._timed(label, "winograd_3x3", ops.wino_flops(g),
                                  lambda: ops.conv2d_fwd_wino_pool(xin, uf, bias, g, pl["ceil"], want_argmax=save, keep_planes=keep, want_bits=wb))
                T[pl["y"]], aux[pl["y"]] = res[0], res[1]
                if keep:
                    aux["planes:" + L.key] = res[2]
                if wb:
                    aux["bits:" + L.key] = res[3]
                return _Elided((g.N, g.H, g.W, L.co))      # never materialised: its only reader is the pool
            res = self._timed(label, "winograd_3x3", ops.wino_flops(g),
                              lambda: ops.conv2d_fwd_wino(xin, uf, bias, g, L.relu, ld=L.co_pad, keep_planes=keep, want_bits=wb))
            if keep:
                aux["planes:" + L.key] = res[1]
            if wb:
                aux["bits:" + L.key] = res[2]
            return res[0] if keep else res
        if path.kind == "x31":
            w3f = self._filter("x31", L, P).fwd
            return self._timed(label, "gemm_planes_x3_kernel (1x1)", ops.conv_flops(g), lambda: ops.conv1x1_fwd_x3(xin, w3f, bias, g, L.relu))
        w = self._filter("layout", L, P)          # (bf16 mode: plane 0 of the limbs feeds the halo-tile kernel)
        return self._timed(label, ops.igemm_tile(g, 0, self.bf16, self.x3) if self.prof is not None else "", ops.conv_flops(g),
                           lambda: ops.conv2d_fwd_x3(xin, w.fwd_limbs, bias, g, L.relu, ld=L.co_pad) if self.x3 else
                           ops.conv2d_fwd(xin, w.fwd, bias, g, L.relu, ld=L.co_pad, bf16=self.bf16, w3=w.fwd_limbs if self.bf16 else None))

    def _wgrad_gemm_async(self, main, Y, kept, part, g, ldy, assign):
        """Second half of a Winograd weight gradient on the weight-gradient stream: waits for what `main` has enqueued so far (the dy
        transform), multiplies, and hands (dw, db) to `assign` inside the stream context."""
        ws = self._wgrad_stream
        ws.wait_event(main.record_event())
        for t in (Y, kept, part):
            t.record_stream(ws)
        with torch.cuda.stream(ws):
            dw, db = ops.wino_wgrad_gemm(Y, kept, part, g, ldy)
            dw.record_stream(main)
            db.record_stream(main)
            assign(dw, db)

    # -- backward ---------------------------------------------------------------------------
    def backward(self, saved, dloc: torch.Tensor, dconf: torch.Tensor, P: Dict[str, torch.Tensor], need: Dict[str, bool]):
        dloc = dloc.contiguous()
        dconf = dconf.contiguous()
        G: Dict[str, torch.Tensor] = {}
        arrived: Dict[str, int] = {}
        grads: Dict[str, torch.Tensor] = _SinkDict(self.grad_sink) if self.grad_sink is not None else {}
        side_ctx = [None]              # left in `finally`: an exception must not leave the side stream current
        try:
            return self._backward_ops(saved, dloc, dconf, P, need, G, arrived, grads, side_ctx)
        finally:
            if side_ctx[0] is not None:
                side_ctx[0].__exit__(None, None, None)

    def _gout(self, *names):
        """Where the gradient of these consecutive parameters is to be written (a flat view of the listener's buffer), or None."""
        return None if self.grad_out is None else self.grad_out(names)

    def _backward_ops(self, saved, dloc, dconf, P, need, G, arrived, grads, side_ctx):
        T, aux, offs, bs = saved["T"], saved["aux"], saved["offs"], saved["bs"]

        def deliver(name, fn):
            """fn(dx, accumulate, mask) -> dx; mask only when this is the last contribution to a post-ReLU tensor."""
            k = arrived.get(name, 0)
            last = k + 1 == self.consumers[name]
            mask = T[name] if (last and name in self.relu_out) else None
            G[name] = fn(G.get(name), k > 0, mask)
            arrived[name] = k + 1
            if self.grad_tap is not None and torch.is_tensor(G[name]):
                if last:
                    self.grad_tap[name] = G[name]
                else:                                        # a partial sum, as stored before the next reader adds to it in place
                    self.grad_tap[f"{name}:{k + 1}"] = G[name].clone()

        main = torch.cuda.current_stream(dloc.device)
        # (with a gradient listener every gradient is reported on the caller's stream: no third stream then)
        async_wgrad = self.overlap_wgrad and self.prof is None and self.dual_dy and self.WINO_TILE == 4 and self.grad_sink is None
        if async_wgrad and self._wgrad_stream is None:
            self._wgrad_stream = torch.cuda.Stream(device=dloc.device)
        wgrad_used = False
        overlap = self.overlap_tail and bool(self._side_ids) and self._side_stream is not None
        side, joined = self._side_stream, not overlap
        held = isinstance(grads, _SinkDict)
        if overlap:                                               # the reversed list starts with the side group
            side.wait_event(main.record_event())
            dloc.record_stream(side)
            dconf.record_stream(side)
            side_ctx[0] = torch.cuda.stream(side)
            side_ctx[0].__enter__()
            if held:
                grads.hold()                                      # the listener hears of side-stream gradients once the caller's stream has waited for them
        join_event = side_done = None
        # The side group's weight gradients are not on the path to a8's gradient (the only thing the caller's stream needs from the group):
        # they are enqueued AFTER the group's data-gradient chain, behind the join event.
        deferred = []
        defer = self.defer_tail_wgrad and self.prof is None

        def conv_backward(L, g, path, dy):
            """Weight and data gradient of one convolution layer, trunk or head, on the path its forward recorded.  dy: a tensor with rows
            of L.co_pad (b16: L.ld16) columns, or (trunk only) a `PooledGrad` / `AdjPlanesGrad` that stands for one."""
            nonlocal wgrad_used
            name, xin, need_w = L.key, T[L.x], L.wanted(need)

            def gout():
                """where the gradient listener, if any, wants this layer's dw and db written"""
                return dict(dw_out=self._gout(*L.weights), db_out=self._gout(*L.biases))
            if path.kind == "b16":
                # bf16 trunk: nine-tap bf16 weight gradient, LDS-DMA data gradient
                f32_dx = path.cast16                      # the head ran on a bf16 copy of an f32 tensor: its dx goes back as f32
                if f32_dx:
                    xin = T[L.x + ":b16"]
                if need_w:
                    L.hand(grads, *self._timed("wgrad " + name, "wgrad3x3_bf16_kernel", ops.conv_flops(g),
                                               lambda: ops.conv3x3_wgrad_bf16t(xin, dy, g, L.ld16, True, **gout())))
                wb16 = self._filter("b16", L, P).bwd

                def dgrad16(dx, acc, mask):
                    if f32_dx and (acc or mask is not None or dx is not None):
                        raise RuntimeError("a head on a bf16 copy must be the first to deliver its input's gradient")
                    return self._timed("dgrad " + name, "conv3x3_bf16_kernel", ops.conv_flops(g),
                                       lambda: ops.conv3x3_bf16(dy, wb16, None, g.Ci, False, flip=True, out=dx, out_f32=f32_dx, relu_mask=mask,
                                                                accumulate=acc))
                deliver(L.x, dgrad16)
                return
            to_bf16 = xin.dtype == torch.bfloat16         # boundary of the bf16 trunk: this layer ran on the f32 copy, its dx goes back as bf16
            if to_bf16:
                xin = T[L.x + ":f32"]
            full = path.kind == "wino" and ops.wino_uses_full(g, 1)      # the library runs this data gradient as one kernel that reads dy itself
            kept_planes = aux.get("planes:" + name) is not None
            # dy rows the plane GEMMs of both gradients can share.  One condition for both kinds: a trunk layer's co_pad is its Co, so
            # this reads Co % 32 == 0 and Co <= 1024; a head's co_pad = pad32(co) is a multiple of 32 by construction, so for it only
            # co_pad <= 1024 decides (SSD300 / SSD512, conf widths 2 .. 256: 32 .. 1568).
            wide = L.co_pad % 32 == 0 and L.co_pad <= 1024
            if isinstance(dy, ops.PooledGrad):
                # dy exists only behind its pool; the Winograd dy pass of this layer can form it on the fly when that pass feeds
                # both the weight gradient and the data gradient -- otherwise it is scattered to memory after all
                if not (need_w and path.wino_wgrad and self.WINO_TILE == 4 and self.dual_dy and kept_planes and wide and not full):
                    dy = dy.materialize()
            # (an adjoint layout implies the Winograd path, hence f32 mode: never the bf16 trunk's boundary)
            adj = path.adj and kept_planes and not (async_wgrad and side_ctx[0] is None) and not full
            if isinstance(dy, ops.AdjPlanesGrad) and not adj:
                dy = dy.materialize()
            if adj:
                # Adjoint Winograd form: ONE set of dy planes (A dy A^T) feeds the weight gradient's TN GEMMs and the data gradient's
                # plane GEMMs; where dy itself is the adjoint data gradient of the layer above (same map, this layer its only reader)
                # the planes come straight from that layer's product planes and dy is never a tensor.
                kept = aux.pop("planes:" + name)

                def dy_planes():
                    if isinstance(dy, ops.AdjPlanesGrad):
                        return ops.wino_adj_output_to_planes(dy.md, dy.g, g, dy.relu_mask, dy.bits, want_bias=need_w)
                    Yp, _, part = ops.wino_dy_transform(dy, g, g.Co, False, need_w)
                    return Yp, part
                if need_w:
                    def wg_adj():
                        Yp, part = dy_planes()
                        dw_, db_ = ops.wino_wgrad_gemm(Yp, kept, part, g, g.Co, **gout())
                        return Yp, dw_, db_
                    Y, dw, db = self._timed("wgrad " + name, "winograd_3x3", ops.wino_flops(g), wg_adj)
                    L.hand(grads, dw, db)
                else:
                    Y, _ = dy_planes()
                del kept
                uadj = self._filter("wino_adj", L, P).bwd
                bits = aux.pop("bits:" + name, None)
                below = self._conv_of.get(L.x) if self.adjoint_chain else None
                gb = aux.get(L.x) if below is not None else None
                chain = (below is not None and gb is not None and self.consumers[L.x] == 1 and L.x in self.relu_out
                         and aux["path:" + below["p"]].adj and aux.get("planes:" + below["p"]) is not None and gb.Co == g.Ci
                         and (gb.N, gb.H, gb.W) == (g.N, g.H, g.W) and T[L.x].dtype == torch.float32)

                def dgrad_adj(dx, acc, mask):
                    md = ops.wino_dgrad_adj_gemm(Y, uadj, g, g.Co)
                    use_bits = bits if mask is not None else None
                    fmask = None if use_bits is not None else mask
                    if chain and dx is None and not acc and mask is not None:
                        return ops.AdjPlanesGrad(md, g, fmask, use_bits)         # the layer below reads the planes, not a tensor
                    return ops.wino_adj_output(md, g, dx, relu_mask=fmask, bits=use_bits, accumulate=acc)
                deliver(L.x, lambda dx, acc, mask: self._timed("dgrad " + name, "winograd_3x3", ops.wino_flops(g),
                                                               lambda: dgrad_adj(dx, acc, mask)))
                return
            dyp = None
            if need_w:
                if path.wino_wgrad and async_wgrad and side_ctx[0] is None and kept_planes and wide:
                    kept = aux.pop("planes:" + name)
                    # the one-kernel data gradient reads dy itself: no B^T dy B planes to write (a head's data gradient always takes them)
                    Y, dyp, part = ops.wino_dy_transform(dy, g, L.co_pad, L.head or not full, True)
                    self._wgrad_gemm_async(main, Y, kept, part, g, L.co_pad, lambda dw, db: L.hand(grads, dw, db))
                    wgrad_used = True
                elif path.wino_wgrad:
                    kept = aux.pop("planes:" + name, None)
                    # one pass over dy feeds the weight and the data gradient (trunk: where the data gradient runs on planes at all)
                    dual = kept is not None and self.dual_dy and (L.head or (g.Co % 32 == 0 and not full))
                    res = self._timed("wgrad " + name, "winograd_3x3", ops.wino_flops(g),
                                      lambda: ops.conv2d_wgrad_wino(xin, dy, g, L.co_pad, True, mo=self.WINO_TILE, planes=kept,
                                                                    dgrad_planes=dual, **gout()))
                    L.hand(grads, res[0], res[1])
                    dyp = res[2] if dual else None
                else:
                    def wg():
                        if path.kind == "x31":
                            L.hand(grads, *self._timed("wgrad " + name, "gemm_tn_x3_kernel (1x1)", ops.conv_flops(g),
                                                       lambda: ops.conv1x1_wgrad_x3(xin, dy, g, L.co_pad, True, **gout())))
                            return
                        L.hand(grads, *self._timed("wgrad " + name, ops.wgrad_tile(g, self.bf16) if self.prof is not None else "", ops.conv_flops(g),
                                                   lambda: ops.conv2d_wgrad(xin, dy, g, L.co_pad, True, bf16=self.bf16, **gout())))
                    if side_ctx[0] is not None and defer:
                        deferred.append(wg)
                    else:
                        wg()
            if path.kind == "wino":
                if path.adj:
                    raise RuntimeError(f"{name}: its filter planes are laid out for the adjoint data gradient, which needs the forward's kept planes "
                                       "(the engine's keep_planes / dual_dy / adjoint_dgrad switches must not change between a forward and its backward)")
                ub = self._filter("wino", L, P).bwd
                bits = aux.pop("bits:" + name, None) if (dyp is not None or full or isinstance(T[L.x], _Elided)) else None

                def dgrad_rot(dx, acc, mask):
                    if isinstance(mask, _Elided):            # the gated activation was never stored (conv1_1 -> planes): only its bits exist
                        if bits is None:
                            raise RuntimeError(f"{name}: its input was not stored and no ReLU bits were kept for its data gradient")
                        mask_t = None
                    else:
                        mask_t = mask
                    return ops.conv2d_dgrad_wino(None if isinstance(dy, ops.PooledGrad) else dy, ub, g, dx, mask_t, acc, planes=dyp,
                                                 bits=bits if mask is not None else None)
                deliver(L.x, lambda dx, acc, mask: self._timed("dgrad " + name, "winograd_3x3", ops.wino_flops(g),
                                                               lambda: dgrad_rot(dx, acc, mask)))
                return
            if path.kind == "x31" and not to_bf16:
                w3b = self._filter("x31", L, P).bwd
                deliver(L.x, lambda dx, acc, mask: self._timed(
                    "dgrad " + name, "gemm_planes_x3_kernel (1x1)", ops.conv_flops(g),
                    lambda: ops.conv1x1_dgrad_x3(dy, w3b, g, dx, mask, acc)))
                return
            w = self._filter("layout", L, P, need_bwd=True)
            w3 = w.bwd_limbs if self.bf16 else None
            if to_bf16:
                def boundary(dx, acc, mask):
                    if acc or mask is not None or dx is not None:
                        raise RuntimeError("the bf16 trunk's boundary tensor must have one consumer and no ReLU of its own")
                    d32 = self._timed("dgrad " + name, ops.igemm_tile(g, 1, self.bf16, self.x3) if self.prof is not None else "", ops.conv_flops(g),
                                      lambda: ops.conv2d_dgrad(dy, w.bwd, g, None, None, False, bf16=self.bf16, w3=w3))
                    return ops.cast_bf16(d32)
                deliver(L.x, boundary)
                return
            deliver(L.x, lambda dx, acc, mask: self._timed(
                "dgrad " + name, ops.igemm_tile(g, 1, self.bf16, self.x3) if self.prof is not None else "", ops.conv_flops(g),
                lambda: ops.conv2d_dgrad_x3(dy, w.bwd_limbs, g, dx, mask, acc) if self.x3 else
                ops.conv2d_dgrad(dy, w.bwd, g, dx, mask, acc, bf16=self.bf16, w3=w3)))

        for op in reversed(self.ops):
            kind = op["op"]
            if side_ctx[0] is not None and id(op) not in self._side_ids:   # the side group is enqueued: back to the caller's stream
                join_event = side.record_event()                           # every data gradient the caller's stream will read exists
                for t in G.values():
                    t.record_stream(main)
                if self._test_side_delay is not None:
                    self._test_side_delay()
                for wg in deferred:                                        # the side group's weight gradients: nothing waits for them
                    wg()
                deferred.clear()
                side_ctx[0].__exit__(None, None, None)
                side_ctx[0] = None
                side_done = side.record_event()
                for t in grads.values():
                    t.record_stream(main)
                if held and self.sink_early:
                    # the listener starts a collective the moment a bucket is complete: order the side stream's gradients before the
                    # caller's stream first (a listener that only collects hears of them at the end of the backward, below)
                    main.wait_event(side_done)
                    side_done = None
                    grads.release()
            if not joined and side_ctx[0] is None and kind in ("conv", "pool", "conv_first"):      # first op that needs what the side group produced (a8's gradient)
                main.wait_event(join_event)
                joined = True
            if kind == "head":
                L = self.layers[op["p"]]
                off, g = offs[L.key]
                path = aux["path:" + L.key]
                # its dy is gathered from the loss gradients: packed bf16 rows (K of the data gradient padded to 64) on the bf16 path
                if path.kind == "b16":
                    dy = ops.heads_gather_bf16(dloc, dconf, L.ld16, bs, g.Ho * g.Wo, op["a"], off).view(bs, g.Ho, g.Wo, L.ld16)
                else:
                    dy = ops.heads_gather(dloc, dconf, L.co_pad, bs, g.Ho * g.Wo, op["a"], off)
                conv_backward(L, g, path, dy)
            elif kind == "conv":
                L = self.layers[op["p"]]
                conv_backward(L, aux[op["y"]], aux["path:" + L.key], G.pop(op["y"]))
            elif kind == "pool":
                dy = G.pop(op["y"])
                xin = T[op["x"]]
                am = aux[op["y"]]
                yout = T[op["y"]]
                deliver(op["x"], lambda dx, acc, mask: (
                    # behind a fused conv -> ReLU -> pool layer: that layer's dy pass reads (dy, argmax, gate) itself
                    ops.PooledGrad(dy, am, yout, xin.shape)
                    if (self.lazy_pool_grad and isinstance(xin, _Elided) and mask is not None and not acc and dx is None
                        and (op["k"], op["s"], op["pad"]) == (2, 2, 0)) else
                    ops.maxpool_bwd(dy, am, tuple(xin.shape), op["k"], op["s"], op["pad"], dx, y_gate=yout)
                    if (mask is not None and not acc) else          # sole consumer of a ReLU output: gate by the pooled output
                    ops.maxpool_bwd(dy, am, tuple(xin.shape), op["k"], op["s"], op["pad"], dx, mask, acc)))
            elif kind == "l2norm":
                dy = G.pop(op["y"])
                xin = T[op["x"]]
                gamma = P[op["p"]].detach().reshape(-1)
                box = {}

                def run(dx, acc, mask, xin=xin, gamma=gamma, dy=dy, box=box):
                    if acc or mask is not None:
                        raise RuntimeError("L2-norm backward must deliver the first, non-final gradient of its input")
                    dx, box["dg"] = ops.l2norm_bwd(xin, gamma, dy, dg_out=self._gout(op["p"]))
                    return dx
                deliver(op["x"], run)
                grads[op["p"]] = box["dg"].reshape(P[op["p"]].shape)
            elif kind == "conv_first":
                dy = G.pop(op["y"])
                if need[op["p"] + ".weight"] or need[op["p"] + ".bias"]:
                    g = aux[op["y"]]
                    col = T["x_col"]
                    if col is None:                                    # the one-kernel forward left no [pixel][32] rows: gradient from x itself
                        dw, db = self._timed("wgrad " + op["p"], "conv_first_wgrad_kernel", 2.0 * dy.numel() * 27,
                                             lambda: (ops.conv1_first_wgrad_bf16 if dy.dtype == torch.bfloat16 else ops.conv1_first_wgrad)(T["x"], dy, True))
                    else:
                        dw, db = self._timed("wgrad " + op["p"], ops.wgrad_tile(g, self.bf16) if self.prof is not None else "", 2.0 * dy.numel() * 27,
                                             lambda: ops.conv2d_wgrad(col, dy, g, g.Co, True))
                    grads[op["p"] + ".weight"], grads[op["p"] + ".bias"] = ops.first_weight_grad(dw), db
        if not joined:
            main.wait_event(join_event)
        if side_done is not None:
            main.wait_event(side_done)
        if wgrad_used:
            main.wait_event(self._wgrad_stream.record_event())
        if held:
            grads.release()
        return grads


class _SSD300Function(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, engine, *params):
        P = dict(zip(engine.names, params))
        loc, conf, saved = engine.forward(x, P, save=True)
        ctx.engine = engine
        ctx.saved = saved
        ctx.params = params
        return loc, conf

    @staticmethod
    def backward(ctx, dloc, dconf):
        eng = ctx.engine
        P = dict(zip(eng.names, ctx.params))
        need = {n: bool(f) for n, f in zip(eng.names, ctx.needs_input_grad[2:])}
        grads = eng.backward(ctx.saved, dloc, dconf, P, need)
        ctx.saved = None
        if eng.sink_owns_grads and eng.grad_sink is not None:
            # ddp.py: every gradient already sits in the flat buffer the all-reduce reads (the parameters' .grad are views of it);
            # handing the views to autograd would make it clone 105 MB into fresh .grad tensors
            return (None, None) + (None,) * len(eng.names)
        return (None, None) + tuple(grads.get(n) if need[n] else None for n in eng.names)


def _check_n_classes(n_classes) -> int:
    if isinstance(n_classes, bool) or not isinstance(n_classes, numbers.Integral):
        raise ValueError(f"n_classes must be an integer, got {n_classes!r}")
    if not 1 <= int(n_classes) <= MAX_FOREGROUND:
        raise ValueError(f"n_classes must be in 1..{MAX_FOREGROUND} (foreground classes; background is added), got {n_classes}")
    return int(n_classes)


class SSD_300(nn.Module):
    """Drop-in for reference Model.py:128-235 (same no-argument constructor, same parameter names).
    `n_classes` (keyword only): the number of FOREGROUND classes, 1..255; `conf` has n_classes + 1 columns, background last.
    The default 20 is the reference's VOC model; any other value changes only the output channels of the `c_*_cl` heads."""
    _VARIANT = 300

    def __init__(self, *, n_classes: int = 20):
        super().__init__()
        self.n_classes = _check_n_classes(n_classes)
        n_conf = self.n_classes + 1
        self.model = _VGG16()                                              # Model.py:131 (no download here)
        self.rescaling_conv_4_3 = nn.Parameter(torch.full((1, 512, 1, 1), 20.))   # Model.py:132-133
        feats = self.model.features
        self.conv_4_3 = nn.Sequential(*feats[0:16], nn.MaxPool2d(2, 2, 0, 1, ceil_mode=True), *feats[17:23])
        self.seq5 = nn.Sequential(*feats[23:30], nn.MaxPool2d(3, 1, 1, 1, ceil_mode=True))
        # fc6 / fc7 as convolutions by sub-sampling the classifier weights (Model.py:145-161)
        cls0, cls3 = self.model.classifier[0], self.model.classifier[3]
        self.fc6 = subsampling(cls0.weight.detach().view(4096, 512, 7, 7), [4, None, 3, 3])
        self.fc6_b = subsampling(cls0.bias.detach(), [4])
        self.fc7 = subsampling(cls3.weight.detach().view(4096, 4096, 1, 1), [4, 4, None, None])
        self.fc7_b = subsampling(cls3.bias.detach(), [4])
        self.conv_fc6 = nn.Conv2d(512, 1024, 3, padding=4, dilation=4)
        self.conv_fc6.weight = nn.Parameter(self.fc6.clone())
        self.conv_fc6.bias = nn.Parameter(self.fc6_b.clone())
        self.conv_fc7 = nn.Conv2d(1024, 1024, 1)
        self.conv_fc7.weight = nn.Parameter(self.fc7.clone())
        self.conv_fc7.bias = nn.Parameter(self.fc7_b.clone())
        self.seq7 = nn.Sequential(self.conv_fc6, nn.ReLU(), self.conv_fc7, nn.ReLU())
        self.seq8 = nn.Sequential(nn.Conv2d(1024, 256, 1), nn.ReLU(), nn.Conv2d(256, 512, 3, 2, padding=1), nn.ReLU())
        self.seq9 = nn.Sequential(nn.Conv2d(512, 128, 1), nn.ReLU(), nn.Conv2d(128, 256, 3, 2, padding=1), nn.ReLU())
        aux = _AUX_300 if self._VARIANT == 300 else _AUX_512
        for name, cin, mid, cout, stride, pad in aux[2:]:
            setattr(self, name, nn.Sequential(nn.Conv2d(cin, mid, 1), nn.ReLU(), nn.Conv2d(mid, cout, 3, stride, padding=pad), nn.ReLU()))
        anchors = ANCHORS_PER_CELL if self._VARIANT == 300 else ANCHORS_PER_CELL_512
        self._aux_names = tuple(a[0] for a in aux)
        self._head_names = ("c_4", "c_7") + tuple(f"c_{8 + i}" for i in range(len(aux)))
        for name, cin, a in zip(self._head_names, (512, 1024, 512) + (256,) * (len(aux) - 1), anchors):
            setattr(self, name + "_bb", nn.Conv2d(cin, 4 * a, 3, padding=1))
            setattr(self, name + "_cl", nn.Conv2d(cin, n_conf * a, 3, padding=1))
        self.initialization()
        self._engine = _Engine(self._VARIANT, n_conf)

    @property
    def conv_dtype(self) -> str:
        """"f32" (default: exact-f32 MFMA, the reference's precision) or "bf16" (BASELINE configs[2]: forward and
        data-gradient convolutions on the bf16 MFMA with f32 accumulation; weight gradients, loss and everything
        else stay f32)."""
        return "bf16" if self._engine.bf16 else ("f32x3" if self._engine.x3 else "f32")

    @conv_dtype.setter
    def conv_dtype(self, value: str) -> None:
        """"f32x3": forward / dgrad products formed from three exact bf16 limbs per f32 operand (six bf16 MFMAs per
        block, f32 accumulate, sign-dithered against the bf16 MFMA's truncation): f32-accurate -- kernel errors within 2x of the exact-f32
        MFMA kernels', and the whole step within the direct engine's decision-pinned bar (1e-5)."""
        if value not in ("f32", "bf16", "f32x3"):
            raise ValueError("conv_dtype must be 'f32', 'f32x3' or 'bf16'")
        self._engine.bf16 = value == "bf16"
        self._engine.x3 = value == "f32x3"
        self._engine._wcache.clear()

    @property
    def winograd(self) -> bool:
        """f32 mode: Winograd F(4x4,3x3) for forward / dgrad of the 3x3 stride-1 layers and the deep weight gradients (default on:
        ~1e-5 of the output scale from the direct sum, 1.5x the step rate).  False = exact-f32 MFMA direct kernels everywhere."""
        return self._engine.wino

    @winograd.setter
    def winograd(self, value: bool) -> None:
        self._engine.wino = bool(value)
        self._engine._wcache.clear()

    def invalidate_weight_cache(self) -> None:
        """Drop the re-laid (OHWI / IHWO / Winograd-domain) copies of the weights.  A training forward always rebuilds them;
        an inference forward reuses them while every parameter's `(data_ptr, _version)` is unchanged.  In-place updates through
        autograd-visible ops (`p.mul_()`, `p.copy_()` under `no_grad`, optimizers, `load_state_dict`, `.to()`) change that key;
        writes through `p.data` (`p.data.copy_()`, `dist.broadcast(p.data, 0)`, EMA weight swaps) do NOT -- call this after
        them before the next `.eval()` forward (and re-capture any `graphed_forward`)."""
        self._engine._wcache.clear()

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        if hasattr(self, "_engine"):
            self._engine._wcache.clear()
        return out

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._engine._wcache.clear()
        return out

    def get_norm(self):
        return torch.norm(self.fc6) + torch.norm(self.fc6_b) + torch.norm(self.fc7) + torch.norm(self.fc7_b)

    def initialization(self):
        """Xavier-uniform weights / zero biases for the aux and head convolutions (Model.py:190-200)."""
        for name in self._aux_names:
            seq = getattr(self, name)
            self.initialize(seq[0])
            self.initialize(seq[2])
        for name in self._head_names:
            self.initialize(getattr(self, name + "_bb"))
            self.initialize(getattr(self, name + "_cl"))

    def initialize(self, c):
        nn.init.xavier_uniform_(c.weight)
        nn.init.constant_(c.bias, 0.)

    def init_conf_prior(self, prior_prob: float = 0.01) -> None:
        """Start for a sigmoid (focal) classification head, Lin et al. 2017 section 4.1: the bias of every foreground conf column of
        every head becomes -log((1 - prior_prob) / prior_prob), so each prior starts with sigmoid score prior_prob instead of 0.5
        (8732 x n_classes negatives at 0.5 swamp the few positives and the first steps diverge); the background column's bias
        becomes 0.  Values only: no parameter is added, renamed or re-laid (channel a * (n_classes + 1) + c is anchor a, column c)."""
        if not 0.0 < float(prior_prob) < 1.0:
            raise ValueError(f"prior_prob must be in (0, 1), got {prior_prob!r}")
        b = -math.log((1.0 - float(prior_prob)) / float(prior_prob))
        n_conf = self.n_classes + 1
        with torch.no_grad():
            for name in self._head_names:
                bias = getattr(self, name + "_cl").bias
                bias.view(-1, n_conf)[:, :-1] = b
                bias.view(-1, n_conf)[:, -1] = 0.0
        self._engine._wcache.clear()

    def graphed_forward(self, example_input: torch.Tensor) -> "GraphedForward":
        """Capture the inference forward for this input shape into a HIP graph (see GraphedForward)."""
        return GraphedForward(self, example_input)

    def _forward_params(self) -> Dict[str, torch.Tensor]:
        named = dict(self.named_parameters())
        return {n: named[n] for n in self._engine.names}

    def forward(self, x):
        P = self._forward_params()
        eng = self._engine
        if torch.is_grad_enabled() and any(p.requires_grad for p in P.values()):
            return _SSD300Function.apply(x, eng, *[P[n] for n in eng.names])
        loc, conf, _ = eng.forward(x, P, save=False)
        return loc, conf


class GraphedForward:
    """Inference forward of a fixed input shape captured once into a HIP graph and replayed: at small batches the
    ~80 kernel launches of a forward cost more host time than GPU time, the replay is one launch.  Every kernel of the
    path only enqueues on the stream it is given (no allocation, no synchronisation inside the library), so the capture
    needs nothing special.  `__call__(x)` copies x into the static input and returns the static (loc, conf) tensors, which
    the next call overwrites.

    What a replay holds: the graph runs on a copy of the parameters taken at capture (biases and the L2-norm scale are read
    from it directly, the filters through layouts made from it and kept out of the engine's weight cache), on those layouts,
    and on the workspaces the capture used (`ops.capture_workspaces`; the capture runs on a stream of its own).  This object keeps all of them alive for its own
    lifetime -- one more copy of the parameters, of their layouts and of the scratch buffers than the eager path holds -- so
    eager calls on the same net (other batch sizes, training steps, `invalidate_weight_cache()`, `load_state_dict`) may
    replace the engine's caches without freeing memory the replay reads.  What it does not notice: ANY change of the
    parameters after the capture (optimizer steps, writes through `.data`, `load_state_dict`) -- a replay returns the outputs
    of the weights at capture.  Capture again (`net.graphed_forward(x)`) after the parameters change."""

    def __init__(self, net: "SSD_300", example: torch.Tensor):
        self.net = net
        self.x = example.detach().clone().contiguous()
        eng = net._engine
        P = {n: p.detach().clone() for n, p in net._forward_params().items()}
        self._stream = torch.cuda.Stream(device=self.x.device)
        s = self._stream
        # The copy's layouts go into a cache of their own, never into the engine's: entries keyed on (data_ptr, _version) of the
        # copy would outlive it there, and a later copy allocated at the same addresses (version 0 again) would hit them.
        shared, eng._wcache = eng._wcache, _FilterCache()
        try:
            s.wait_stream(torch.cuda.current_stream(self.x.device))
            with torch.no_grad(), torch.cuda.stream(s):       # warm-up: weight layouts, workspaces, allocator pools
                for _ in range(2):
                    eng.forward(self.x, P, save=False)
            torch.cuda.current_stream(self.x.device).wait_stream(s)
            self.graph = torch.cuda.CUDAGraph()
            with ops.capture_workspaces() as ws, torch.no_grad(), torch.cuda.graph(self.graph, stream=s):
                self.loc, self.conf, _ = eng.forward(self.x, P, save=False)
            layouts = eng._wcache.tensors()
        finally:
            eng._wcache = shared
        self._held = (P, ws, layouts)          # what the replay reads besides its own pool: the parameter copy, its layouts, the workspaces

    def __call__(self, x: torch.Tensor):
        if tuple(x.shape) != tuple(self.x.shape) or x.dtype != self.x.dtype:
            raise ValueError(f"graph captured for {tuple(self.x.shape)} {self.x.dtype}, got {tuple(x.shape)} {x.dtype}")
        self.x.copy_(x, non_blocking=True)
        self.graph.replay()
        return self.loc, self.conf


class SSD_512(SSD_300):
    """Build-defined SSD512 (NOT in the reference): 512x512 input, seven maps
    64/32/16/8/4/2/1 (every aux block 1x1 -> 3x3 stride 2 pad 1, plus `seq12` / `c_12_*`), 24564 priors
    (`Util.create_priors_ssd512`).  Same kernels, same parameter naming scheme; parity is against the oracle's own
    restatement only -- there is no reference implementation to compare with."""
    _VARIANT = 512


from .ModelResnet import SSD_resnet34  # noqa: E402,F401  (reference Model.py:12-126 lives in the same module)

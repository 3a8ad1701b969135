"""torch-tensor front ends of the C ABI (device memory + streams are torch's; the
arithmetic is libssd_gfx950.so's).  Every wrapper validates what the kernels
assume (device, dtype, contiguity, shapes) before enqueueing -- a wrong shape
must never reach a hand-written kernel.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import List, Optional, Tuple

import torch

from . import _lib
from ._lib import ConvGeom, check


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


_current_device = torch.cuda.current_device


def _req(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: the gfx950 path needs a device tensor (got {t.device}); there is no CPU fallback")
    if t.device.index != _current_device():
        # the kernels are enqueued on the CURRENT device's stream (`_stream()`): a tensor of another GPU would be a foreign pointer there
        raise RuntimeError(f"{name}: tensor lives on {t.device} but the current device is cuda:{_current_device()}; run the call under "
                           f"`torch.cuda.device({t.device.index})` (one process per GPU: `torch.cuda.set_device(local_rank)`)")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    return t


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _grad_dst(dst: Optional[torch.Tensor], shape, device, name: str) -> torch.Tensor:
    """Destination of a parameter gradient: a fresh tensor, or the caller's buffer (ddp.py hands out views of its flat gradient
    buffer, so the kernel writes the gradient where the all-reduce reads it)."""
    if dst is None:
        return torch.empty(shape, device=device, dtype=torch.float32)
    _req(dst, name)
    n = 1
    for d in shape:
        n *= d
    if dst.numel() != n or dst.device != device:
        raise ValueError(f"{name}: destination has {dst.numel()} elements on {dst.device}, the gradient has {n} on {device}")
    return dst.view(shape)


def conv_out_hw(h: int, w: int, k: int, stride: int, pad: int, dil: int) -> Tuple[int, int]:
    return ((h + 2 * pad - dil * (k - 1) - 1) // stride + 1, (w + 2 * pad - dil * (k - 1) - 1) // stride + 1)


def make_geom(n, h, w, ci, co, k, stride, pad, dil) -> ConvGeom:
    ho, wo = conv_out_hw(h, w, k, stride, pad, dil)
    return ConvGeom(n, h, w, ci, ho, wo, co, k, k, stride, pad, dil)


def pad32(c: int) -> int:
    return (c + 31) // 32 * 32


def igemm_tile(g: ConvGeom, direction: int, bf16: bool = False, x3: bool = False) -> str:
    """Name prefix of the kernel the library picks for this geometry (bench.py groups per-launch timings by it)."""
    if (x3 or bf16) and g.R == 3 and g.S == 3 and g.stride == 1 and g.dil == 1 and g.pad == 1 and (direction == 1 or g.Ci % 32 == 0):
        ho, wo = (g.Ho, g.Wo) if direction == 0 else (g.H, g.W)
        if ho >= 30 and wo >= (64 if x3 else 30):
            return "conv3x3_halo_kernel"
    if x3:
        return "igemm_x3_kernel"
    if bf16:
        return "igemm_bf16_kernel"
    bm, bn = C.c_int(0), C.c_int(0)
    check(_lib.load().ssd_conv2d_igemm_tile(C.byref(g), direction, C.byref(bm), C.byref(bn)), "igemm_tile")
    return f"igemm_kernel<{bm.value}, {bn.value}"


def wgrad_tile(g: ConvGeom, bf16: bool = False) -> str:
    if bf16 and g.stride == 1 and g.R == g.S and ((g.R == 3 and g.pad == g.dil and g.dil in (1, 4)) or (g.R == 1 and g.pad == 0)):
        return "wgrad3x3_bf16_kernel"                   # the bf16 patch kernel (csrc/conv_wgrad.hip plan_wgrad)
    bt, ns = C.c_int(0), C.c_int(0)
    check(_lib.load().ssd_conv2d_wgrad_tile(C.byref(g), C.byref(bt), C.byref(ns)), "wgrad_tile")
    return "wgrad3x3_kernel" if bt.value == 3 else f"wgrad_kernel<{bt.value}"


def conv_flops(g: ConvGeom) -> float:
    """algorithmic FLOPs of one pass (fwd, dgrad or wgrad all cost 2*M*Co*K)"""
    return 2.0 * g.N * g.Ho * g.Wo * g.Co * g.R * g.S * g.Ci


def wino_tiles(g: ConvGeom) -> int:
    """4x4 output tiles of the F(4x4,3x3) form of a 3x3 / stride-1 convolution with padding = dilation D: the D x D sub-lattices of the
    map are tiled one by one (csrc/winograd.hip, struct Lat); D = 1 is the plain ceil(H/4) x ceil(W/4) grid."""
    d = g.dil
    th = sum((((g.H - a + d - 1) // d) + 3) // 4 for a in range(d) if a < g.H)
    tw = sum((((g.W - a + d - 1) // d) + 3) // 4 for a in range(d) if a < g.W)
    return g.N * th * tw


def wino_flops(g: ConvGeom):
    """(direct-convolution FLOPs, FLOPs the 36 batched GEMMs of the F(4x4,3x3) form execute: 36 multiplies per 4x4 output tile
    instead of 144, on the tile grid padded to multiples of 4, output channels padded to 32)"""
    return conv_flops(g), 2.0 * 36 * wino_tiles(g) * pad32(g.Co) * g.Ci


# ---- weights ---------------------------------------------------------------------------
def layout_filter_alloc(ci: int, taps: int, co_pad: int, device, bwd: bool = False) -> torch.Tensor:
    """Destination of a filter in the direct kernels' layout: OHWI (co_pad, taps, ci) or, bwd, IHWO (ci, taps, co_pad), f32.  The
    transforms write every element, the rows past the filter's own as zeros."""
    return torch.empty((ci, taps, co_pad) if bwd else (co_pad, taps, ci), device=device, dtype=torch.float32)


def weight_ohwi(w_oihw: torch.Tensor, co_pad: Optional[int] = None) -> torch.Tensor:
    _req(w_oihw, "weight")
    co, ci, r, s = w_oihw.shape
    co_pad = co if co_pad is None else co_pad
    out = layout_filter_alloc(ci, r * s, co_pad, w_oihw.device)
    check(_lib.load().ssd_weight_oihw_to_ohwi(w_oihw.data_ptr(), out.data_ptr(), co, ci, r, s, co_pad, _stream()), "weight_ohwi")
    return out


def weight_ihwo(w_oihw: torch.Tensor, co_pad: Optional[int] = None) -> torch.Tensor:
    _req(w_oihw, "weight")
    co, ci, r, s = w_oihw.shape
    co_pad = pad32(co) if co_pad is None else co_pad
    out = layout_filter_alloc(ci, r * s, co_pad, w_oihw.device, bwd=True)
    check(_lib.load().ssd_weight_oihw_to_ihwo(w_oihw.data_ptr(), out.data_ptr(), co, ci, r, s, co_pad, _stream()), "weight_ihwo")
    return out


def weight_split3(w_layout: torch.Tensor) -> torch.Tensor:
    """f32 weights in a kernel layout (OHWI / IHWO) -> (3, *shape) bf16 limb planes hi, mid, lo with hi+mid+lo == w exactly"""
    _req(w_layout, "w_layout")
    out = torch.empty((3,) + tuple(w_layout.shape), device=w_layout.device, dtype=torch.bfloat16)
    check(_lib.load().ssd_weight_split_bf16x3(w_layout.data_ptr(), out.data_ptr(), w_layout.numel(), _stream()), "weight_split3")
    return out


# ---- convolution -----------------------------------------------------------------------
def _filter(w: torch.Tensor, name: str, limbs: bool):
    """(rows, taps, channels) of a filter in a kernel layout (OHWI / IHWO), given in f32 or, limbs, as its weight_split3 planes"""
    _req(w, name, torch.bfloat16 if limbs else torch.float32)
    if w.dim() != (4 if limbs else 3) or (limbs and w.shape[0] != 3):
        raise ValueError(f"{name} shape does not match geometry")
    return tuple(w.shape[-3:])


def _fwd_core(x, w, name, limbs, bias, g, ld, out, accumulate):
    """What every direct forward settles before its library call: the operands against the geometry, and the destination
    (N,Ho,Wo,ld) -- the caller's, or a fresh one whose columns Co..ld-1 are zero.  -> (out, ld)"""
    _req(x, "x")
    rows, taps, ci = _filter(w, name, limbs)
    if tuple(x.shape) != (g.N, g.H, g.W, g.Ci):
        raise ValueError(f"x shape {tuple(x.shape)} != geometry {(g.N, g.H, g.W, g.Ci)}")
    if rows < g.Co or taps != g.R * g.S or ci != g.Ci:
        raise ValueError(f"{name} shape does not match geometry")
    if bias is not None:
        _req(bias, "bias")
        if bias.numel() != g.Co:
            raise ValueError("bias length")
    ld = g.Co if ld is None else ld
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs an existing out")
        alloc = torch.empty if ld == g.Co else torch.zeros
        return alloc((g.N, g.Ho, g.Wo, ld), device=x.device, dtype=torch.float32), ld
    _req(out, "out")
    if out.numel() != g.N * g.Ho * g.Wo * ld:
        raise ValueError("out size")
    return out, ld


def _dgrad_core(dy, w, name, limbs, g, dx, relu_mask, accumulate):
    """What every direct data gradient settles before its library call: the operands against the geometry, dx (N,H,W,Ci) -- the
    caller's, or a fresh one -- and the ReLU mask.  -> (dx, co_pad)"""
    _req(dy, "dy")
    ci, taps, co_pad = _filter(w, name, limbs)
    if dy.numel() != g.N * g.Ho * g.Wo * co_pad:
        raise ValueError(f"dy has {dy.numel()} elements, geometry wants {g.N * g.Ho * g.Wo * co_pad}")
    if ci != g.Ci or taps != g.R * g.S or co_pad % 32 != 0 or co_pad < g.Co:
        raise ValueError(f"{name} shape does not match geometry")
    if dx is None:
        if accumulate:
            raise ValueError("accumulate needs an existing dx")
        dx = torch.empty((g.N, g.H, g.W, g.Ci), device=dy.device, dtype=torch.float32)
    _req(dx, "dx")
    if dx.numel() != g.N * g.H * g.W * g.Ci:
        raise ValueError("dx size")
    if relu_mask is not None:
        _req(relu_mask, "relu_mask")
        if relu_mask.numel() != dx.numel():
            raise ValueError("relu_mask size")
    return dx, co_pad


def _igemm_ws(g: ConvGeom, direction: int, device):
    """(pointer, bytes) of the split-K workspace of the _ws entry points: (None, 0) except for small grids with a deep K loop"""
    nbytes = _lib.load().ssd_conv2d_igemm_workspace(C.byref(g), direction)
    ws = workspace(nbytes, device, "igemm") if nbytes else None
    return _ptr(ws), ws.numel() if ws is not None else 0


def conv2d_fwd_x3(x: torch.Tensor, w3_ohwi: torch.Tensor, bias: Optional[torch.Tensor], g: ConvGeom, relu: bool,
                  ld: Optional[int] = None) -> torch.Tensor:
    out, ld = _fwd_core(x, w3_ohwi, "w3_ohwi", True, bias, g, ld, None, False)
    check(_lib.load().ssd_conv2d_fwd_x3(x.data_ptr(), w3_ohwi.data_ptr(), int(w3_ohwi.shape[1]), _ptr(bias), out.data_ptr(), ld,
                                        C.byref(g), int(relu), _stream()), "conv2d_fwd_x3")
    return out


def conv2d_dgrad_x3(dy: torch.Tensor, w3_ihwo: torch.Tensor, g: ConvGeom, dx: Optional[torch.Tensor] = None,
                    relu_mask: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    dx, co_pad = _dgrad_core(dy, w3_ihwo, "w3_ihwo", True, g, dx, relu_mask, accumulate)
    check(_lib.load().ssd_conv2d_dgrad_x3(dy.data_ptr(), co_pad, w3_ihwo.data_ptr(), co_pad, dx.data_ptr(), _ptr(relu_mask),
                                          int(accumulate), C.byref(g), _stream()), "conv2d_dgrad_x3")
    return dx


def conv2d_fwd(x: torch.Tensor, w_ohwi: torch.Tensor, bias: Optional[torch.Tensor], g: ConvGeom, relu: bool,
               ld: Optional[int] = None, out: Optional[torch.Tensor] = None, bf16: bool = False,
               w3: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """x (N,H,W,Ci) -> (N,Ho,Wo,ld) (ld defaults to Co; columns Co..ld-1 are left untouched).
    bf16 with `w3` (weight_split3 of w_ohwi): 3x3/s1/p1 layers on large maps take the halo-tile kernel.
    accumulate: out += conv (+ bias), then ReLU: the residual tail of a ResNet BasicBlock."""
    out, ld = _fwd_core(x, w_ohwi, "w_ohwi", False, bias, g, ld, out, accumulate)
    lib = _lib.load()
    args = (x.data_ptr(), w_ohwi.data_ptr(), _ptr(bias), out.data_ptr(), ld, C.byref(g), int(relu))
    if accumulate:
        check((lib.ssd_conv2d_fwd_accum_bf16 if bf16 else lib.ssd_conv2d_fwd_accum)(*args, _stream()), "conv2d_fwd_accum")
        return out
    if bf16 and w3 is not None and g.Ci % 32 == 0:
        _req(w3, "w3", torch.bfloat16)
        if tuple(w3.shape) != (3,) + tuple(w_ohwi.shape):
            raise ValueError("w3 must be weight_split3(w_ohwi)")
        rc = lib.ssd_conv3x3_halo_fwd_bf16(x.data_ptr(), w3.data_ptr(), int(w3.shape[1]), _ptr(bias), out.data_ptr(), ld,
                                           C.byref(g), int(relu), _stream())
        if rc <= 0:
            check(rc, "conv3x3_halo_fwd_bf16")
            return out
    fn, what = (lib.ssd_conv2d_fwd_bf16_ws, "conv2d_fwd_bf16") if bf16 else (lib.ssd_conv2d_fwd_ws, "conv2d_fwd")
    check(fn(*args, *_igemm_ws(g, 0, x.device), _stream()), what)
    return out


def conv2d_dgrad(dy: torch.Tensor, w_ihwo: torch.Tensor, g: ConvGeom, dx: Optional[torch.Tensor] = None,
                 relu_mask: Optional[torch.Tensor] = None, accumulate: bool = False, bf16: bool = False,
                 w3: Optional[torch.Tensor] = None) -> torch.Tensor:
    dx, co_pad = _dgrad_core(dy, w_ihwo, "w_ihwo", False, g, dx, relu_mask, accumulate)
    lib = _lib.load()
    if bf16 and w3 is not None and g.Ci % 4 == 0:
        _req(w3, "w3", torch.bfloat16)
        if tuple(w3.shape) != (3,) + tuple(w_ihwo.shape):
            raise ValueError("w3 must be weight_split3(w_ihwo)")
        rc = lib.ssd_conv3x3_halo_dgrad_bf16(dy.data_ptr(), co_pad, w3.data_ptr(), co_pad, dx.data_ptr(), _ptr(relu_mask),
                                             int(accumulate), C.byref(g), _stream())
        if rc <= 0:
            check(rc, "conv3x3_halo_dgrad_bf16")
            return dx
    fn, what = (lib.ssd_conv2d_dgrad_bf16_ws, "conv2d_dgrad_bf16") if bf16 else (lib.ssd_conv2d_dgrad_ws, "conv2d_dgrad")
    check(fn(dy.data_ptr(), co_pad, w_ihwo.data_ptr(), co_pad, dx.data_ptr(), _ptr(relu_mask), int(accumulate), C.byref(g),
             *_igemm_ws(g, 1, dy.device), _stream()), what)
    return dx


def conv3x3_bf16(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], n_out: int, relu: bool, flip: bool = False,
                 out: Optional[torch.Tensor] = None, out_f32: bool = False, ldo: Optional[int] = None,
                 relu_mask: Optional[torch.Tensor] = None, accumulate: bool = False, K: Optional[int] = None) -> torch.Tensor:
    """3x3 / stride 1 / pad 1 convolution on bf16 tensors (csrc/conv_bf16.hip).  x (N,H,W,ldx) bf16; w (rows, 9, K) bf16 -- the
    OHWI copy of the weights for the forward, the IHWO copy with flip=True for the data gradient (x is then dy);
    -> out (N,H,W,ldo) bf16 (f32 with out_f32), columns 0..n_out-1 written: [accumulate: out +] conv (+ bias) -> [relu] -> [mask > 0]."""
    _req(x, "x", torch.bfloat16); _req(w, "w", torch.bfloat16)
    if x.dim() != 4 or w.dim() != 3 or w.shape[1] != 9:
        raise ValueError("conv3x3_bf16: x (N,H,W,ldx), w (rows,9,K)")
    n, h, wd, ldx = x.shape
    K = int(w.shape[2]) if K is None else K
    if K != w.shape[2] or K % 64 != 0 or K > ldx or n_out % 4 != 0:
        raise ValueError("conv3x3_bf16: K must be the weights' row length, a multiple of 64 and <= ldx; n_out % 4 == 0")
    ldo = n_out if ldo is None else ldo
    odt = torch.float32 if out_f32 else torch.bfloat16
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs an existing out")
        out = torch.empty((n, h, wd, ldo), device=x.device, dtype=odt) if ldo == n_out else torch.zeros((n, h, wd, ldo), device=x.device, dtype=odt)
    else:
        _req(out, "out", odt)
        if out.numel() != n * h * wd * ldo:
            raise ValueError("conv3x3_bf16: out size")
    if bias is not None:
        _req(bias, "bias")
        if bias.numel() < min(n_out, int(w.shape[0])):
            raise ValueError("conv3x3_bf16: bias needs one entry per weight row")
    if relu_mask is not None:
        _req(relu_mask, "relu_mask", torch.bfloat16)
        if relu_mask.numel() != out.numel() or out_f32:
            raise ValueError("conv3x3_bf16: relu_mask must have the layout of a bf16 out")
    check(_lib.load().ssd_conv3x3_bf16(x.data_ptr(), ldx, w.data_ptr(), int(w.shape[0]), K, _ptr(bias), out.data_ptr(), ldo, n_out,
                                       int(out_f32), _ptr(relu_mask), int(accumulate), int(relu), int(flip), n, h, wd, _stream()),
          "conv3x3_bf16")
    return out


def pad64(c: int) -> int:
    return (c + 63) // 64 * 64


def bf16_filter_alloc(co: int, ci: int, device, bwd: bool = False) -> torch.Tensor:
    """Destination of a 3x3 filter for csrc/conv_bf16.hip: OHWI (co, 9, ci) or, bwd, IHWO (ci, 9, pad64(co)) zero-filled, bf16."""
    if bwd:
        return torch.zeros((ci, 9, pad64(co)), device=device, dtype=torch.bfloat16)
    return torch.empty((co, 9, ci), device=device, dtype=torch.bfloat16)


def weights_bf16(w_oihw: torch.Tensor):
    """(Co,Ci,3,3) f32 -> the bf16 OHWI and IHWO copies of `bf16_filter_alloc` (per-layer form of the kind-3 weight job)."""
    co, ci = int(w_oihw.shape[0]), int(w_oihw.shape[1])
    wf, wb = bf16_filter_alloc(co, ci, w_oihw.device), bf16_filter_alloc(co, ci, w_oihw.device, bwd=True)
    wf.copy_(w_oihw.permute(0, 2, 3, 1).reshape(co, 9, ci))
    wb[:, :, :co] = w_oihw.permute(1, 2, 3, 0).reshape(ci, 9, co)
    return wf, wb


def cast_bf16(x: torch.Tensor) -> torch.Tensor:
    """f32 -> bf16 (round to nearest even), same shape; numel % 8 == 0"""
    _req(x, "x")
    y = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    check(_lib.load().ssd_cast_f32_bf16(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "cast_f32_bf16")
    return y


def cast_f32(x: torch.Tensor) -> torch.Tensor:
    _req(x, "x", torch.bfloat16)
    y = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    check(_lib.load().ssd_cast_bf16_f32(x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "cast_bf16_f32")
    return y


def conv1_first_fwd_bf16(x_nchw: torch.Tensor, w_rows: torch.Tensor, bias: Optional[torch.Tensor], relu: bool = True) -> torch.Tensor:
    """conv1_1 in the bf16-tensor mode: f32 NCHW image -> bf16 NHWC (N,H,W,64); operands rounded to bf16, f32 accumulate."""
    _req(x_nchw, "x"); _req(w_rows, "w_rows")
    n, c, h, w = x_nchw.shape
    if c != 3 or w_rows.numel() != 64 * 32:
        raise ValueError("conv1_first_fwd_bf16 expects 3 input channels and (64, 32) filter rows")
    if bias is not None:
        _req(bias, "bias")
    y = torch.empty((n, h, w, 64), device=x_nchw.device, dtype=torch.bfloat16)
    check(_lib.load().ssd_conv1_first_fwd_bf16(x_nchw.data_ptr(), w_rows.data_ptr(), _ptr(bias), y.data_ptr(), n, h, w, int(relu), _stream()),
          "conv1_first_fwd_bf16")
    return y


def conv1_first_wgrad_bf16(x_nchw: torch.Tensor, dy: torch.Tensor, want_bias: bool = True):
    """conv1_1 weight / bias gradient from the f32 NCHW image and the bf16 NHWC dy -> (dw rows (64,32,1,1), dbias or None), f32."""
    _req(x_nchw, "x"); _req(dy, "dy", torch.bfloat16)
    n, c, h, w = x_nchw.shape
    if c != 3 or tuple(dy.shape) != (n, h, w, 64):
        raise ValueError("conv1_first_wgrad_bf16: x (N,3,H,W) and dy (N,H,W,64)")
    lib = _lib.load()
    ws = workspace(lib.ssd_conv1_first_wgrad_workspace(n, h, w), x_nchw.device, "first_wgrad")
    dw = torch.empty((64, 32, 1, 1), device=x_nchw.device, dtype=torch.float32)
    db = torch.empty((64,), device=x_nchw.device, dtype=torch.float32) if want_bias else None
    check(lib.ssd_conv1_first_wgrad_bf16(x_nchw.data_ptr(), dy.data_ptr(), dw.data_ptr(), _ptr(db), n, h, w, ws.data_ptr(), ws.numel(), _stream()),
          "conv1_first_wgrad_bf16")
    return dw, db


def conv3x3_wgrad_bf16t(x: torch.Tensor, dy: torch.Tensor, g: ConvGeom, ldy: int, want_bias: bool = True,
                        dw_out: Optional[torch.Tensor] = None, db_out: Optional[torch.Tensor] = None):
    """Weight gradient of a 3x3 / s1 / p1 layer from bf16 x (N,H,W,Ci) and bf16 dy (N,H,W,ldy) -> (dw (Co,Ci,3,3), dbias) f32."""
    _req(x, "x", torch.bfloat16); _req(dy, "dy", torch.bfloat16)
    if tuple(x.shape) != (g.N, g.H, g.W, g.Ci) or dy.numel() != g.N * g.Ho * g.Wo * ldy or ldy < g.Co:
        raise ValueError("conv3x3_wgrad_bf16t: shapes do not match the geometry")
    lib = _lib.load()
    ws = workspace(lib.ssd_conv2d_wgrad_workspace(C.byref(g)), x.device)
    dw = _grad_dst(dw_out, (g.Co, g.Ci, 3, 3), x.device, "dw_out")
    db = _grad_dst(db_out, (g.Co,), x.device, "db_out") if want_bias else None
    check(lib.ssd_conv3x3_wgrad_bf16t(x.data_ptr(), dy.data_ptr(), ldy, dw.data_ptr(), _ptr(db), C.byref(g), ws.data_ptr(), ws.numel(), _stream()),
          "conv3x3_wgrad_bf16t")
    return dw, db


def heads_gather_bf16(dloc: torch.Tensor, dconf: torch.Tensor, ld: int, n: int, hw: int, a: int, prior_off: int) -> torch.Tensor:
    _req(dloc, "dloc"); _req(dconf, "dconf")
    p, ncls = dconf.shape[1], dconf.shape[2]
    if tuple(dloc.shape) != (n, p, 4) or dconf.shape[0] != n:
        raise ValueError("heads_gather shapes")
    packed = torch.empty((n * hw, ld), device=dloc.device, dtype=torch.bfloat16)
    check(_lib.load().ssd_heads_gather_bf16(dloc.data_ptr(), dconf.data_ptr(), packed.data_ptr(), ld, n, hw, a, prior_off, p, ncls, _stream()),
          "heads_gather_bf16")
    return packed


_ws_cache = {}
_ws_capture: Optional[dict] = None      # set by `capture_workspaces`: id -> every workspace handed out meanwhile


def workspace(nbytes: int, device, tag: str = "ws") -> torch.Tensor:
    """Grow-only scratch buffer per (device, stream, tag); contents are dead between calls.  A larger request replaces (and frees) the
    buffer of its key: a captured graph that baked in the old one must hold it itself (`capture_workspaces`)."""
    key = (str(device), _stream(), tag)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), device=device, dtype=torch.uint8)
        _ws_cache[key] = buf
    if _ws_capture is not None:
        _ws_capture[id(buf)] = buf
    return buf


@contextlib.contextmanager
def capture_workspaces():
    """Yields a list that, when the block ends, holds every workspace `workspace()` handed out inside it (on any stream): the buffers
    a graph captured in the block has baked in.  The graph's owner keeps the list for the graph's lifetime, so that a later, larger
    eager call that regrows a workspace does not free memory a replay still reads and writes."""
    global _ws_capture
    prev, _ws_capture = _ws_capture, {}
    held: List[torch.Tensor] = []
    try:
        yield held
    finally:
        mine, _ws_capture = _ws_capture, prev
        held.extend(mine.values())
        if prev is not None:
            prev.update(mine)


def conv2d_wgrad(x: torch.Tensor, dy: torch.Tensor, g: ConvGeom, ldy: int, want_bias: bool = True, bf16: bool = False,
                 dw_out: Optional[torch.Tensor] = None, db_out: Optional[torch.Tensor] = None):
    """-> (dw (Co,Ci,R,S) OIHW, dbias (Co,) or None); dw_out / db_out: write the gradients there (same element counts)."""
    _req(x, "x"); _req(dy, "dy")
    if tuple(x.shape) != (g.N, g.H, g.W, g.Ci):
        raise ValueError("x shape does not match geometry")
    if dy.numel() != g.N * g.Ho * g.Wo * ldy or ldy < g.Co:
        raise ValueError("dy size does not match geometry")
    lib = _lib.load()
    nbytes = lib.ssd_conv2d_wgrad_workspace(C.byref(g))
    ws = workspace(nbytes, x.device)
    dw = _grad_dst(dw_out, (g.Co, g.Ci, g.R, g.S), x.device, "dw_out")
    db = _grad_dst(db_out, (g.Co,), x.device, "db_out") if want_bias else None
    fn = lib.ssd_conv2d_wgrad_bf16 if bf16 else lib.ssd_conv2d_wgrad
    check(fn(x.data_ptr(), dy.data_ptr(), ldy, dw.data_ptr(), _ptr(db), C.byref(g), ws.data_ptr(), ws.numel(), _stream()),
          "conv2d_wgrad")
    return dw, db


def im2col_first(x_nchw: torch.Tensor) -> torch.Tensor:
    """(N,3,H,W) NCHW -> (N,H,W,32) rows of the 27 taps (k = (r*3+s)*3 + c) + 5 zero columns."""
    _req(x_nchw, "x")
    n, c, h, w = x_nchw.shape
    if c != 3:
        raise ValueError("im2col_first expects 3 input channels")
    out = torch.empty((n, h, w, 32), device=x_nchw.device, dtype=torch.float32)
    check(_lib.load().ssd_im2col_first(x_nchw.data_ptr(), out.data_ptr(), n, h, w, _stream()), "im2col_first")
    return out


def conv1_first_fwd(x_nchw: torch.Tensor, w_rows: torch.Tensor, bias: Optional[torch.Tensor], relu: bool = True, want_col: bool = False):
    """conv1_1 (3 -> 64 channels, 3x3, pad 1) + bias + ReLU from the NCHW batch in one kernel -> (y (N,H,W,64) NHWC, col or None);
    w_rows = `first_weight_rows(weight)`; want_col: also the (N,H,W,32) rows of `im2col_first` (the weight gradient's operand)."""
    _req(x_nchw, "x"); _req(w_rows, "w_rows")
    n, c, h, w = x_nchw.shape
    if c != 3 or w_rows.numel() != 64 * 32:
        raise ValueError("conv1_first_fwd expects 3 input channels and (64, 32) filter rows")
    if bias is not None:
        _req(bias, "bias")
        if bias.numel() != 64:
            raise ValueError("conv1_first_fwd: 64 biases")
    y = torch.empty((n, h, w, 64), device=x_nchw.device, dtype=torch.float32)
    col = torch.empty((n, h, w, 32), device=x_nchw.device, dtype=torch.float32) if want_col else None
    check(_lib.load().ssd_conv1_first_fwd(x_nchw.data_ptr(), w_rows.data_ptr(), _ptr(bias), y.data_ptr(), _ptr(col), n, h, w, int(relu), _stream()),
          "conv1_first_fwd")
    return y, col


def has_experimental() -> bool:
    """the library was built with SSD_EXPERIMENTAL=1 (the kernels that measured no better than the shipped ones)"""
    return bool(_lib.load().ssd_has_experimental())


def conv1_first_wino_fwd(x_nchw: torch.Tensor, w_rows: torch.Tensor, bias: Optional[torch.Tensor], want_bits: bool = True):
    """conv1_1 + bias + ReLU left as the F(4x4) input planes of the 64 -> 64 convolution behind it -> (planes (36, tiles, 64), ReLU bit
    words (tiles, 16) int64 or None): what `conv1_first_fwd` + that layer's input transform would have produced, bit for bit, without the
    activation tensor in between."""
    _req(x_nchw, "x"); _req(w_rows, "w_rows")
    n, c, h, w = x_nchw.shape
    if c != 3 or w_rows.numel() != 64 * 32:
        raise ValueError("conv1_first_wino_fwd expects 3 input channels and (64, 32) filter rows")
    if bias is not None:
        _req(bias, "bias")
        if bias.numel() != 64:
            raise ValueError("conv1_first_wino_fwd: 64 biases")
    tiles = n * ((h + 3) // 4) * ((w + 3) // 4)
    planes = torch.empty((36, tiles, 64), device=x_nchw.device, dtype=torch.float32)
    bits = torch.empty((tiles, 16), device=x_nchw.device, dtype=torch.int64) if want_bits else None
    check(_lib.load().ssd_conv1_first_wino_fwd(x_nchw.data_ptr(), w_rows.data_ptr(), _ptr(bias), planes.data_ptr(), _ptr(bits), n, h, w, _stream()),
          "conv1_first_wino_fwd")
    return planes, bits


def conv1_first_wgrad(x_nchw: torch.Tensor, dy: torch.Tensor, want_bias: bool = True):
    """Weight / bias gradient of conv1_1 from the NCHW input: -> (dw (64,32,1,1) rows for `first_weight_grad`, dbias (64,) or None)."""
    _req(x_nchw, "x"); _req(dy, "dy")
    n, c, h, w = x_nchw.shape
    if c != 3 or tuple(dy.shape) != (n, h, w, 64):
        raise ValueError("conv1_first_wgrad: x (N,3,H,W) and dy (N,H,W,64)")
    lib = _lib.load()
    ws = workspace(lib.ssd_conv1_first_wgrad_workspace(n, h, w), x_nchw.device, "first_wgrad")
    dw = torch.empty((64, 32, 1, 1), device=x_nchw.device, dtype=torch.float32)
    db = torch.empty((64,), device=x_nchw.device, dtype=torch.float32) if want_bias else None
    check(lib.ssd_conv1_first_wgrad(x_nchw.data_ptr(), dy.data_ptr(), dw.data_ptr(), _ptr(db), n, h, w, ws.data_ptr(), ws.numel(), _stream()),
          "conv1_first_wgrad")
    return dw, db


def im2col_nchw3(x_nchw: torch.Tensor, k: int, stride: int, pad: int, kpad: Optional[int] = None) -> torch.Tensor:
    """(N,3,H,W) -> (N,Ho,Wo,Kpad) rows with k = (r*k+s)*3 + c, zero-padded to a multiple of 32 (ResNet-34 stem)."""
    _req(x_nchw, "x")
    if x_nchw.dim() != 4 or x_nchw.shape[1] != 3:
        raise ValueError("im2col_nchw3 expects (N,3,H,W)")
    n, _, h, w = x_nchw.shape
    ho, wo = conv_out_hw(h, w, k, stride, pad, 1)
    kpad = pad32(k * k * 3) if kpad is None else kpad
    out = torch.empty((n, ho, wo, kpad), device=x_nchw.device, dtype=torch.float32)
    check(_lib.load().ssd_im2col_nchw3(x_nchw.data_ptr(), out.data_ptr(), n, h, w, k, k, stride, pad, ho, wo, kpad, _stream()),
          "im2col_nchw3")
    return out


def stem_weight_rows(w_oihw: torch.Tensor, kpad: Optional[int] = None) -> torch.Tensor:
    """(Co,3,R,S) -> (Co,1,Kpad) rows in im2col_nchw3's column order (the 1x1 OHWI layout)."""
    co, ci, r, s_ = w_oihw.shape
    kpad = pad32(r * s_ * ci) if kpad is None else kpad
    rows = torch.zeros((co, 1, kpad), device=w_oihw.device, dtype=torch.float32)
    rows[:, 0, :r * s_ * ci] = w_oihw.detach().permute(0, 2, 3, 1).reshape(co, -1)
    return rows


def channel_affine(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, relu: bool = False,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[..., c] = x[..., c] * scale[c] + shift[c] over NHWC rows (eval-mode BatchNorm after a ReLU)."""
    _req(x, "x"); _req(scale, "scale"); _req(shift, "shift")
    c = x.shape[-1]
    if scale.numel() != c or shift.numel() != c or c % 4 != 0:
        raise ValueError("scale / shift must have one entry per channel, C % 4 == 0")
    out = torch.empty_like(x) if out is None else out
    check(_lib.load().ssd_channel_affine(x.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(), x.numel() // c, c,
                                         int(relu), _stream()), "channel_affine")
    return out


# ---- BatchNorm in training mode / dropout (csrc/batchnorm.hip) --------------------------------------------------------------------
DROP_NONE, DROP_ELEMENT, DROP_CHANNEL = 0, 1, 2


def _bn_rows(x: torch.Tensor, c: int, ld: Optional[int], name: str) -> Tuple[int, int]:
    """(M, ld) of x seen as [M][ld] rows whose first c columns are the channels"""
    _req(x, name)
    ld = c if ld is None else ld
    if c <= 0 or c % 4 != 0 or ld < c or ld % 4 != 0 or x.numel() % ld != 0:
        raise ValueError(f"{name}: {x.numel()} elements are not rows of ld = {ld} holding C = {c} channels (C % 4 == 0, ld % 4 == 0)")
    return x.numel() // ld, ld


def _drop_args(drop) -> Tuple[int, float, int, int, int]:
    """drop = None or (mode, p, seed, site, hw) -> the C arguments"""
    if drop is None:
        return DROP_NONE, 0.0, 0, 0, 1
    mode, p, seed, site, hw = drop
    if mode not in (DROP_NONE, DROP_ELEMENT, DROP_CHANNEL) or not 0.0 <= p <= 1.0:
        raise ValueError(f"dropout mode {mode} / p {p}")
    return int(mode), float(p), int(seed) & (2 ** 64 - 1), int(site), int(hw)


def _per_channel(t: Optional[torch.Tensor], c: int, name: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    _req(t, name)
    if t.numel() != c:
        raise ValueError(f"{name}: {t.numel()} entries for {c} channels")
    return t


def bn_train_stats(x: torch.Tensor, c: int, gamma: Optional[torch.Tensor], beta: Optional[torch.Tensor], eps: float, momentum: float,
                   running_mean: Optional[torch.Tensor] = None, running_var: Optional[torch.Tensor] = None,
                   num_batches_tracked: Optional[torch.Tensor] = None, ld: Optional[int] = None) -> torch.Tensor:
    """Training-mode BatchNorm statistics of the first c columns of x's [M][ld] rows -> (4, c): mean, invstd, scale, shift.
    Updates the running buffers in place (when given) on the device."""
    m, ld = _bn_rows(x, c, ld, "x")
    if m < 2:
        raise ValueError(f"Expected more than 1 value per channel when training, got {m} rows of {c} channels")
    for t, n in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        _per_channel(t, c, n)
    if num_batches_tracked is not None:
        _req(num_batches_tracked, "num_batches_tracked", torch.int64)
    out = torch.empty((4, c), device=x.device, dtype=torch.float32)
    lib = _lib.load()
    nbytes = lib.ssd_bn_workspace(m, c)
    ws = workspace(nbytes, x.device, "bn")
    check(lib.ssd_bn_train_stats(x.data_ptr(), ld, m, c, _ptr(gamma), _ptr(beta), float(eps), float(momentum), _ptr(running_mean),
                                 _ptr(running_var), _ptr(num_batches_tracked), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                 out[3].data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "bn_train_stats")
    return out


def bn_apply(x: torch.Tensor, c: int, scale: torch.Tensor, shift: torch.Tensor, relu: bool = False, res: Optional[torch.Tensor] = None,
             res_scale: Optional[torch.Tensor] = None, res_shift: Optional[torch.Tensor] = None, drop=None,
             out: Optional[torch.Tensor] = None, ld: Optional[int] = None, res_ld: Optional[int] = None,
             out_ld: Optional[int] = None) -> torch.Tensor:
    """out = drop(act(x*scale + shift [+ res*res_scale + res_shift | + res])) over the first c columns; out may be x.
    drop = None or (mode, p, seed, site, hw) with mode DROP_ELEMENT / DROP_CHANNEL."""
    m, ld = _bn_rows(x, c, ld, "x")
    _per_channel(scale, c, "scale"); _per_channel(shift, c, "shift")
    if res is not None:
        mr, res_ld = _bn_rows(res, c, res_ld, "res")
        if mr != m:
            raise ValueError("res rows")
    if (res_scale is None) != (res_shift is None) or (res_scale is not None and res is None):
        raise ValueError("res_scale and res_shift go together, with res")
    _per_channel(res_scale, c, "res_scale"); _per_channel(res_shift, c, "res_shift")
    if out is None:
        out = torch.empty((m, c), device=x.device, dtype=torch.float32) if out_ld is None else \
            torch.zeros((m, out_ld), device=x.device, dtype=torch.float32)
    mo, out_ld = _bn_rows(out, c, out_ld, "out")
    if mo != m:
        raise ValueError("out rows")
    mode, p, seed, site, hw = _drop_args(drop)
    if mode == DROP_CHANNEL and m % hw != 0:
        raise ValueError("rows are not a whole number of samples")
    check(_lib.load().ssd_bn_apply(x.data_ptr(), ld, m, c, scale.data_ptr(), shift.data_ptr(), _ptr(res), res_ld or 0, _ptr(res_scale),
                                   _ptr(res_shift), int(relu), mode, p, seed, site, hw, out.data_ptr(), out_ld, _stream()), "bn_apply")
    return out


def bn_train_bwd(dy: torch.Tensor, x: torch.Tensor, c: int, mean: torch.Tensor, invstd: torch.Tensor, gamma: Optional[torch.Tensor],
                 drop=None, relu_mask: bool = False, dgamma: Optional[torch.Tensor] = None, dbeta: Optional[torch.Tensor] = None,
                 accumulate: bool = False, dx: Optional[torch.Tensor] = None, want_dx: bool = True, ld_dy: Optional[int] = None,
                 ld_x: Optional[int] = None, ld_dx: Optional[int] = None):
    """Backward of drop(BN_train(x)) (after a ReLU when relu_mask) -> (dx or None, sums (2, c): sum g, sum g*xhat).
    dx may be dy (in place); dgamma / dbeta are written, or added to when accumulate."""
    m, ld_dy = _bn_rows(dy, c, ld_dy, "dy")
    mx, ld_x = _bn_rows(x, c, ld_x, "x")
    if mx != m:
        raise ValueError("x rows")
    if m < 2:
        raise ValueError("BatchNorm backward needs more than 1 value per channel")
    for t, n in ((mean, "mean"), (invstd, "invstd"), (gamma, "gamma"), (dgamma, "dgamma"), (dbeta, "dbeta")):
        _per_channel(t, c, n)
    if want_dx:
        if dx is None:
            dx = torch.empty((m, c), device=dy.device, dtype=torch.float32) if ld_dx is None else \
                torch.zeros((m, ld_dx), device=dy.device, dtype=torch.float32)
        md, ld_dx = _bn_rows(dx, c, ld_dx, "dx")
        if md != m:
            raise ValueError("dx rows")
    else:
        dx, ld_dx = None, 0
    mode, p, seed, site, hw = _drop_args(drop)
    if mode == DROP_CHANNEL and m % hw != 0:
        raise ValueError("rows are not a whole number of samples")
    sums = torch.empty((2, c), device=dy.device, dtype=torch.float32)
    lib = _lib.load()
    ws = workspace(lib.ssd_bn_workspace(m, c), dy.device, "bn")
    check(lib.ssd_bn_train_bwd(dy.data_ptr(), ld_dy, x.data_ptr(), ld_x, m, c, mean.data_ptr(), invstd.data_ptr(), _ptr(gamma), mode, p,
                               seed, site, hw, int(relu_mask), sums.data_ptr(), _ptr(dgamma), _ptr(dbeta), int(accumulate), _ptr(dx),
                               ld_dx, ws.data_ptr(), ws.numel(), _stream()), "bn_train_bwd")
    return dx, sums


def dropout_mask(n: int, p: float, seed: int, site: int, device) -> torch.Tensor:
    """bool keep flags of dropout indices 0..n-1 of (seed, site): the generator of bn_apply, materialised (n % 4 == 0)"""
    out = torch.empty((n,), device=device, dtype=torch.uint8)
    _, p, seed, site, _ = _drop_args((DROP_ELEMENT, p, seed, site, 1))
    check(_lib.load().ssd_dropout_mask(out.data_ptr(), n, p, seed, site, _stream()), "dropout_mask")
    return out.bool()


def first_rows_alloc(co: int, device) -> torch.Tensor:
    """Destination of conv1_1's filter rows: (co, 1, 32) f32, zero-filled (27 taps, padded to the GEMM's K = 32)."""
    return torch.zeros((co, 1, 32), device=device, dtype=torch.float32)


def first_weight_rows(w_oihw: torch.Tensor) -> torch.Tensor:
    """(Co,3,3,3) OIHW -> (Co,1,32): rows ordered like im2col_first's columns, zero padded."""
    co = w_oihw.shape[0]
    out = first_rows_alloc(co, w_oihw.device)
    out.view(co, 32)[:, :27] = w_oihw.detach().permute(0, 2, 3, 1).reshape(co, 27)      # [co][(r,s),c]
    return out


def first_weight_grad(dw_rows: torch.Tensor) -> torch.Tensor:
    """inverse of first_weight_rows for the gradient: (Co,32,1,1) -> (Co,3,3,3) OIHW"""
    co = dw_rows.shape[0]
    return dw_rows.reshape(co, 32)[:, :27].reshape(co, 3, 3, 3).permute(0, 3, 1, 2).contiguous()


# ---- pooling / norm ----------------------------------------------------------------------
def pool_out(h: int, k: int, stride: int, pad: int, ceil_mode: bool) -> int:
    num = h + 2 * pad - k
    o = (-(-num // stride) if ceil_mode else num // stride) + 1
    if ceil_mode and (o - 1) * stride >= h + pad:      # torch: last window must start inside the input or left pad
        o -= 1
    return o


def maxpool_fwd(x: torch.Tensor, k: int, stride: int, pad: int, ceil_mode: bool, want_argmax: bool = True):
    """NHWC max pool -> (y, argmax codes or None); a bf16 x takes the bf16-tensor kernels (csrc/elementwise_bf16.hip)."""
    n, h, w, c = x.shape
    ho, wo = pool_out(h, k, stride, pad, ceil_mode), pool_out(w, k, stride, pad, ceil_mode)
    if x.dtype == torch.bfloat16:
        _req(x, "x", torch.bfloat16)
        y = torch.empty((n, ho, wo, c), device=x.device, dtype=torch.bfloat16)
        am = torch.empty((n, ho, wo, c), device=x.device, dtype=torch.uint8) if want_argmax else None
        check(_lib.load().ssd_maxpool_fwd_bf16(x.data_ptr(), y.data_ptr(), _ptr(am), n, h, w, c, k, stride, pad, ho, wo, _stream()),
              "maxpool_fwd_bf16")
        return y, am
    _req(x, "x")
    y = torch.empty((n, ho, wo, c), device=x.device, dtype=torch.float32)
    am = torch.empty((n, ho, wo, c), device=x.device, dtype=torch.uint8) if want_argmax else None
    check(_lib.load().ssd_maxpool_fwd(x.data_ptr(), y.data_ptr(), _ptr(am), n, h, w, c, k, stride, pad, ho, wo, _stream()),
          "maxpool_fwd")
    return y, am


def maxpool_bwd(dy: torch.Tensor, argmax: torch.Tensor, in_shape, k: int, stride: int, pad: int,
                dx: Optional[torch.Tensor] = None, relu_mask: Optional[torch.Tensor] = None, accumulate: bool = False,
                y_gate: Optional[torch.Tensor] = None):
    """y_gate: the pooled OUTPUT; with it (and no accumulate / relu_mask) the ReLU mask of the pool's input is applied as
    y > 0 per window, which reads a quarter of the bytes of relu_mask = x."""
    n, h, w, c = in_shape
    _, ho, wo, c2 = dy.shape
    if dy.dtype == torch.bfloat16:
        _req(dy, "dy", torch.bfloat16); _req(argmax, "argmax", torch.uint8)
        if c2 != c or tuple(argmax.shape) != tuple(dy.shape):
            raise ValueError("maxpool_bwd shapes")
        if y_gate is not None and (accumulate or relu_mask is not None):
            raise ValueError("y_gate replaces relu_mask and cannot accumulate")
        for t, nm in ((y_gate, "y_gate"), (relu_mask, "relu_mask")):
            if t is not None:
                _req(t, nm, torch.bfloat16)
        if y_gate is not None and tuple(y_gate.shape) != tuple(dy.shape):
            raise ValueError("y_gate must be the pooled output")
        if dx is None:
            if accumulate:
                raise ValueError("accumulate needs an existing dx")
            dx = torch.empty((n, h, w, c), device=dy.device, dtype=torch.bfloat16)
        _req(dx, "dx", torch.bfloat16)
        if dx.numel() != n * h * w * c or (relu_mask is not None and relu_mask.numel() != dx.numel()):
            raise ValueError("dx / relu_mask size")
        check(_lib.load().ssd_maxpool_bwd_bf16(dy.data_ptr(), argmax.data_ptr(), dx.data_ptr(), _ptr(relu_mask), _ptr(y_gate), int(accumulate),
                                               n, h, w, c, k, stride, pad, ho, wo, _stream()), "maxpool_bwd_bf16")
        return dx
    _req(dy, "dy"); _req(argmax, "argmax", torch.uint8)
    if c2 != c or tuple(argmax.shape) != tuple(dy.shape):
        raise ValueError("maxpool_bwd shapes")
    if y_gate is not None:
        if accumulate or relu_mask is not None:
            raise ValueError("y_gate replaces relu_mask and cannot accumulate")
        _req(y_gate, "y_gate")
        if tuple(y_gate.shape) != tuple(dy.shape):
            raise ValueError("y_gate must be the pooled output")
        dx = torch.empty((n, h, w, c), device=dy.device, dtype=torch.float32) if dx is None else dx
        _req(dx, "dx")
        if dx.numel() != n * h * w * c:
            raise ValueError("dx size")
        check(_lib.load().ssd_maxpool_bwd_gated(dy.data_ptr(), argmax.data_ptr(), y_gate.data_ptr(), dx.data_ptr(), n, h, w, c, k, stride,
                                                pad, ho, wo, _stream()), "maxpool_bwd_gated")
        return dx
    if dx is None:
        if accumulate:
            raise ValueError("accumulate needs an existing dx")
        dx = torch.empty((n, h, w, c), device=dy.device, dtype=torch.float32)
    _req(dx, "dx")
    if dx.numel() != n * h * w * c:
        raise ValueError("dx size")
    if relu_mask is not None:
        _req(relu_mask, "relu_mask")
        if relu_mask.numel() != dx.numel():
            raise ValueError("relu_mask size")
    check(_lib.load().ssd_maxpool_bwd(dy.data_ptr(), argmax.data_ptr(), dx.data_ptr(), _ptr(relu_mask), int(accumulate),
                                      n, h, w, c, k, stride, pad, ho, wo, _stream()), "maxpool_bwd")
    return dx


def l2norm_fwd(x: torch.Tensor, gamma: torch.Tensor) -> torch.Tensor:
    _req(x, "x", x.dtype if x.dtype == torch.bfloat16 else torch.float32); _req(gamma, "gamma")
    c = x.shape[-1]
    if gamma.numel() != c:
        raise ValueError("gamma length")
    if x.dtype == torch.bfloat16:
        y = torch.empty_like(x)
        check(_lib.load().ssd_l2norm_fwd_bf16(x.data_ptr(), gamma.data_ptr(), y.data_ptr(), x.numel() // c, c, _stream()), "l2norm_fwd_bf16")
        return y
    y = torch.empty_like(x)
    check(_lib.load().ssd_l2norm_fwd(x.data_ptr(), gamma.data_ptr(), y.data_ptr(), x.numel() // c, c, _stream()), "l2norm_fwd")
    return y


def l2norm_bwd(x: torch.Tensor, gamma: torch.Tensor, dy: torch.Tensor, dx: Optional[torch.Tensor] = None,
               dg_out: Optional[torch.Tensor] = None):
    c = x.shape[-1]
    m = x.numel() // c
    if x.dtype == torch.bfloat16:
        _req(x, "x", torch.bfloat16); _req(gamma, "gamma"); _req(dy, "dy", torch.bfloat16)
        if dy.numel() != x.numel():
            raise ValueError("dy size")
        lib = _lib.load()
        ws = workspace(lib.ssd_l2norm_bwd_bf16_workspace(m, c), x.device)
        dx = torch.empty_like(x) if dx is None else _req(dx, "dx", torch.bfloat16)
        dg = _grad_dst(dg_out, (c,), x.device, "dg_out")
        check(lib.ssd_l2norm_bwd_bf16(x.data_ptr(), gamma.data_ptr(), dy.data_ptr(), dx.data_ptr(), dg.data_ptr(), m, c, ws.data_ptr(),
                                      ws.numel(), _stream()), "l2norm_bwd_bf16")
        return dx, dg
    _req(x, "x"); _req(gamma, "gamma"); _req(dy, "dy")
    if dy.numel() != x.numel():
        raise ValueError("dy size")
    lib = _lib.load()
    ws = workspace(lib.ssd_l2norm_bwd_workspace(m, c), x.device)
    dx = torch.empty_like(x) if dx is None else _req(dx, "dx")
    dg = _grad_dst(dg_out, (c,), x.device, "dg_out")
    check(lib.ssd_l2norm_bwd(x.data_ptr(), gamma.data_ptr(), dy.data_ptr(), dx.data_ptr(), dg.data_ptr(), m, c,
                             ws.data_ptr(), ws.numel(), _stream()), "l2norm_bwd")
    return dx, dg


# ---- heads ---------------------------------------------------------------------------------
def heads_scatter(packed: torch.Tensor, ld: int, loc: torch.Tensor, conf: torch.Tensor, n: int, hw: int, a: int,
                  prior_off: int) -> None:
    _req(packed, "packed"); _req(loc, "loc"); _req(conf, "conf")
    p, ncls = conf.shape[1], conf.shape[2]
    if packed.numel() != n * hw * ld or tuple(loc.shape) != (n, p, 4) or conf.shape[0] != n:
        raise ValueError("heads_scatter shapes")
    check(_lib.load().ssd_heads_scatter(packed.data_ptr(), ld, loc.data_ptr(), conf.data_ptr(), n, hw, a, prior_off, p, ncls,
                                        _stream()), "heads_scatter")


def heads_gather(dloc: torch.Tensor, dconf: torch.Tensor, ld: int, n: int, hw: int, a: int, prior_off: int) -> torch.Tensor:
    _req(dloc, "dloc"); _req(dconf, "dconf")
    p, ncls = dconf.shape[1], dconf.shape[2]
    if tuple(dloc.shape) != (n, p, 4) or dconf.shape[0] != n:
        raise ValueError("heads_gather shapes")
    packed = torch.empty((n * hw, ld), device=dloc.device, dtype=torch.float32)
    check(_lib.load().ssd_heads_gather(dloc.data_ptr(), dconf.data_ptr(), packed.data_ptr(), ld, n, hw, a, prior_off, p, ncls,
                                       _stream()), "heads_gather")
    return packed


# ---- loss / decode ----------------------------------------------------------------------------
IGNORE_OVERLAPS = {"iou": 0, "ioa": 1}


def ignore_overlap_mode(overlap):
    """0 / 1 for "iou" / "ioa" (the `overlap_mode` of the C ABI); ValueError for anything else."""
    try:
        return IGNORE_OVERLAPS[overlap]
    except (KeyError, TypeError):
        raise ValueError(f"ignore_overlap must be 'iou' or 'ioa', not {overlap!r}") from None


LOC_LOSSES = {"l1": 0, "iou": 1, "giou": 2, "diou": 3, "ciou": 4}


def loc_loss_mode(name):
    """0 .. 4 for "l1" / "iou" / "giou" / "diou" / "ciou" (the `loc_mode` of the C ABI); ValueError for anything else."""
    try:
        return LOC_LOSSES[name]
    except (KeyError, TypeError):
        raise ValueError(f"loc_loss must be one of {', '.join(map(repr, LOC_LOSSES))}, not {name!r}") from None


CONF_LOSSES = {"ce": 0, "focal": 1}


def conf_loss_mode(name):
    """0 / 1 for "ce" / "focal" (the `conf_mode` of the C ABI); ValueError for anything else."""
    try:
        return CONF_LOSSES[name]
    except (KeyError, TypeError):
        raise ValueError(f"conf_loss must be one of {', '.join(map(repr, CONF_LOSSES))}, not {name!r}") from None


def focal_params(focal_alpha, focal_gamma):
    """(alpha, gamma) as floats: alpha in [0, 1] or negative (no alpha weighting), gamma >= 0 and finite; ValueError otherwise."""
    try:
        alpha, gamma = float(focal_alpha), float(focal_gamma)
    except (TypeError, ValueError):
        raise ValueError(f"focal_alpha / focal_gamma must be numbers, not {focal_alpha!r} / {focal_gamma!r}") from None
    if not alpha <= 1.0:
        raise ValueError(f"focal_alpha must be in [0, 1], or negative for no weighting, not {focal_alpha!r}")
    if not 0.0 <= gamma < float("inf"):
        raise ValueError(f"focal_gamma must be >= 0 and finite, not {focal_gamma!r}")
    return alpha, gamma


MATCHES = {"iou": 0, "atss": 1}


def match_mode(name):
    """0 / 1 for "iou" / "atss" (the `match_mode` of the C ABI); ValueError for anything else."""
    try:
        return MATCHES[name]
    except (KeyError, TypeError):
        raise ValueError(f"match must be one of {', '.join(map(repr, MATCHES))}, not {name!r}") from None


def atss_topk_value(atss_topk):
    """atss_topk as an int in 1 .. 32; ValueError otherwise."""
    if isinstance(atss_topk, bool) or not isinstance(atss_topk, int) or not 1 <= atss_topk <= 32:
        raise ValueError(f"atss_topk must be an integer in 1 .. 32, not {atss_topk!r}")
    return atss_topk


def atss_levels(prior_levels, n_priors):
    """prior_levels = (cells, anchors), two equally long sequences of 1 .. 8 positive ints with sum(cells * anchors) == n_priors
    (`Util.prior_levels`) -> two ctypes int arrays for the C ABI; ValueError otherwise."""
    try:
        cells, anchors = prior_levels
        cells, anchors = [int(v) for v in cells], [int(v) for v in anchors]
    except (TypeError, ValueError):
        raise ValueError(f"prior_levels must be (cells, anchors), two sequences of ints, not {prior_levels!r}") from None
    if len(cells) != len(anchors) or not 1 <= len(cells) <= 8:
        raise ValueError(f"prior_levels must describe 1 .. 8 levels, cells and anchors equally long, not {prior_levels!r}")
    if min(cells) < 1 or min(anchors) < 1 or sum(c * a for c, a in zip(cells, anchors)) != n_priors:
        raise ValueError(f"prior_levels {prior_levels!r} does not sum to the {n_priors} priors")
    arr = C.c_int * len(cells)
    return arr(*cells), arr(*anchors)


def multibox_loss(loc, conf, gt_boxes, gt_classes, img_start, priors_cxcywh, priors_xyxy, iou_threshold=0.5,
                  neg_pos_ratio=3, norm_mode=0, want_grads=True, loc_loss="l1", conf_loss="ce", focal_alpha=0.25, focal_gamma=2.0,
                  match="iou", atss_topk=9, prior_levels=None, ignore_boxes=None, ignore_start=None, ignore_threshold=0.5,
                  ignore_overlap="iou"):
    """-> dict(losses (3,), obj (bs,P) i32, cls (bs,P) i32, dloc, dconf).  `ssd_multibox_loss_box` serves every option; the call without any goes
    to `ssd_multibox_loss`, the same host path.
    ignore_boxes (n_ign, 4) fractional xyxy with ignore_start (bs + 1,) int32 prefix offsets (both on the device; n_ign may be 0):
    the loss with ignore regions -- a prior that is not positive and overlaps an ignore box of its image by >= ignore_threshold
    ("iou", or "ioa" = intersection over the prior's area) is neither mined nor given a gradient; the dict then has "ign" (bs,P)
    uint8 too.  None: no ignore regions.
    loc_loss: "l1" (the reference's term), or "iou" / "giou" / "diou" / "ciou": the predicted box of each positive is decoded
    (exponent clamped to +-log(1000 / 16)) and losses[0] is the per-positive mean (norm_mode 1: sum) of 1 - IoU plus the mode's
    penalty, dloc its gradient; everything else is unchanged.  "ciou" needs ground-truth boxes of positive height; "iou" gives no
    gradient where the two boxes do not overlap.
    conf_loss: "ce" (the reference's softmax cross entropy with hard-negative mining), or "focal": columns 0 .. C-2 are
    one-against-all logits and losses[1] is the sum over every prior that is not ignored and every foreground column of
    alpha_t (1 - p_t)^focal_gamma BCE (torchvision's `sigmoid_focal_loss`; focal_alpha < 0: no alpha weighting), divided by n_pos
    (norm_mode 1: the sum); dconf its gradient, zero in the background column; nothing is mined and neg_pos_ratio is not read
    (`ssd_multibox_loss_focal`).  Matching, losses[0], losses[2], dloc and "ign" are those of "ce".
    match: "iou" (the reference's rule: IoU >= iou_threshold against the prior's best box, plus one forced prior per box), or "atss"
    (`ssd_multibox_loss_atss`): per box the priors of the atss_topk (1 .. 32) nearest cells of every level are
    candidates, those with IoU >= mean + std of the candidates' IoUs and their centre inside the box are its positives, a prior wanted
    by several boxes goes to the largest IoU.  It needs prior_levels = (cells, anchors) per pyramid level (`Util.prior_levels`);
    iou_threshold is not read, nothing is forced: a box may get no prior and an image no positive (a batch without any positive
    divides by n_pos = 0 in norm_mode 0, as every entry does).  Everything behind the assignment is unchanged."""
    mode = ignore_overlap_mode(ignore_overlap)
    mmode = match_mode(match)
    topk = atss_topk_value(atss_topk)
    if mmode and prior_levels is None:
        raise ValueError('multibox_loss: match="atss" needs prior_levels (Util.prior_levels)')
    loc_mode = loc_loss_mode(loc_loss)
    conf_mode = conf_loss_mode(conf_loss)
    alpha, gamma = focal_params(focal_alpha, focal_gamma)
    if (ignore_boxes is None) != (ignore_start is None):
        raise ValueError("multibox_loss: ignore_boxes and ignore_start go together")
    _req(loc, "loc"); _req(conf, "conf"); _req(gt_boxes, "gt_boxes"); _req(gt_classes, "gt_classes")
    _req(img_start, "img_start", torch.int32); _req(priors_cxcywh, "priors"); _req(priors_xyxy, "priors_xyxy")
    bs, p, ncls = conf.shape
    n_gt = gt_boxes.shape[0]
    if tuple(loc.shape) != (bs, p, 4) or tuple(gt_boxes.shape) != (n_gt, 4) or gt_classes.numel() != n_gt or \
            img_start.numel() != bs + 1 or tuple(priors_cxcywh.shape) != (p, 4) or tuple(priors_xyxy.shape) != (p, 4):
        raise ValueError("multibox_loss shapes")
    n_ign = 0
    if ignore_boxes is not None:
        _req(ignore_boxes, "ignore_boxes"); _req(ignore_start, "ignore_start", torch.int32)
        n_ign = ignore_boxes.shape[0]
        if tuple(ignore_boxes.shape) != (n_ign, 4) or ignore_start.numel() != bs + 1:
            raise ValueError("multibox_loss ignore shapes")
    levels = atss_levels(prior_levels, p) if mmode else None
    lib = _lib.load()
    dev = loc.device
    ws = workspace((lib.ssd_multibox_loss_atss_workspace if mmode else lib.ssd_multibox_loss_box_workspace)(bs, p, n_gt, n_ign), dev, "loss")
    out = dict(losses=torch.empty((3,), device=dev, dtype=torch.float32),
               obj=torch.empty((bs, p), device=dev, dtype=torch.int32),
               cls=torch.empty((bs, p), device=dev, dtype=torch.int32),
               dloc=torch.empty_like(loc) if want_grads else None,
               dconf=torch.empty_like(conf) if want_grads else None)
    if ignore_boxes is not None:
        out["ign"] = torch.empty((bs, p), device=dev, dtype=torch.uint8)
    head = (loc.data_ptr(), conf.data_ptr(), gt_boxes.data_ptr(), gt_classes.data_ptr(), img_start.data_ptr(), bs, n_gt,
            priors_cxcywh.data_ptr(), priors_xyxy.data_ptr(), p, ncls, float(iou_threshold), int(neg_pos_ratio), int(norm_mode))
    outs = (out["losses"].data_ptr(), out["obj"].data_ptr(), out["cls"].data_ptr())
    tail = (_ptr(out["dloc"]), _ptr(out["dconf"]), ws.data_ptr(), ws.numel(), _stream())
    if mmode != 0:
        check(lib.ssd_multibox_loss_atss(*head, ignore_boxes.data_ptr() if n_ign else None, _ptr(ignore_start), n_ign,
                                         float(ignore_threshold), mode, loc_mode, conf_mode, alpha, gamma, mmode, topk, len(levels[0]),
                                         levels[0], levels[1], *outs, _ptr(out.get("ign")), *tail), "multibox_loss_atss")
    elif conf_mode != 0:
        check(lib.ssd_multibox_loss_focal(*head, ignore_boxes.data_ptr() if n_ign else None, _ptr(ignore_start), n_ign,
                                          float(ignore_threshold), mode, loc_mode, conf_mode, alpha, gamma, *outs, _ptr(out.get("ign")),
                                          *tail), "multibox_loss_focal")
    elif loc_mode == 0 and ignore_boxes is None:              # (the entry the cross-check switch `ssd_tune_set_loss_form` reaches)
        check(lib.ssd_multibox_loss(*head, *outs, *tail), "multibox_loss")
    else:
        check(lib.ssd_multibox_loss_box(*head, ignore_boxes.data_ptr() if n_ign else None, _ptr(ignore_start), n_ign,
                                        float(ignore_threshold), mode, loc_mode, *outs, _ptr(out.get("ign")), *tail),
              "multibox_loss_box" if loc_mode else "multibox_loss_ignore")
    return out


def atss_assign(gt_boxes, img_start, priors_cxcywh, priors_xyxy, prior_levels, atss_topk=9):
    """The assignment pass of `multibox_loss(match="atss")` alone (`ssd_atss_assign`) -> dict(assign (bs,P) i32 global box index or -1,
    n_cand (n_gt,) i32 candidates per box, mean / var (n_gt,) f64 of their IoUs, n_acc (n_gt,) i32 candidates that passed the
    threshold and the centre test, before conflicts)."""
    topk = atss_topk_value(atss_topk)
    _req(gt_boxes, "gt_boxes"); _req(img_start, "img_start", torch.int32); _req(priors_cxcywh, "priors"); _req(priors_xyxy, "priors_xyxy")
    bs, n_gt, p = img_start.numel() - 1, gt_boxes.shape[0], priors_cxcywh.shape[0]
    if bs < 1 or n_gt < 1 or tuple(gt_boxes.shape) != (n_gt, 4) or tuple(priors_cxcywh.shape) != (p, 4) or tuple(priors_xyxy.shape) != (p, 4):
        raise ValueError("atss_assign shapes")
    cells, anchors = atss_levels(prior_levels, p)
    lib = _lib.load()
    dev = gt_boxes.device
    ws = workspace(lib.ssd_atss_assign_workspace(bs, p), dev, "atss")
    out = dict(assign=torch.empty((bs, p), device=dev, dtype=torch.int32), n_cand=torch.empty((n_gt,), device=dev, dtype=torch.int32),
               mean=torch.empty((n_gt,), device=dev, dtype=torch.float64), var=torch.empty((n_gt,), device=dev, dtype=torch.float64),
               n_acc=torch.empty((n_gt,), device=dev, dtype=torch.int32))
    check(lib.ssd_atss_assign(gt_boxes.data_ptr(), img_start.data_ptr(), bs, n_gt, priors_cxcywh.data_ptr(), priors_xyxy.data_ptr(), p, topk,
                              len(cells), cells, anchors, out["assign"].data_ptr(), out["n_cand"].data_ptr(), out["mean"].data_ptr(),
                              out["var"].data_ptr(), out["n_acc"].data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "atss_assign")
    return out


NMS_METHODS = {"hard": 0, "linear": 1, "gaussian": 2}


def nms_method(nms):
    """0 / 1 / 2 for "hard" / "linear" / "gaussian" (the `method` of the C ABI); ValueError for anything else."""
    try:
        return NMS_METHODS[nms]
    except (KeyError, TypeError):
        raise ValueError(f"nms must be 'hard', 'linear' or 'gaussian', not {nms!r}") from None


SCORES = {"softmax": 0, "sigmoid": 1}


def score_mode(score):
    """0 / 1 for "softmax" / "sigmoid" (the `score_mode` of the C ABI); ValueError for anything else."""
    try:
        return SCORES[score]
    except (KeyError, TypeError):
        raise ValueError(f"score must be 'softmax' or 'sigmoid', not {score!r}") from None


def decode_nms(l_, c_, priors_cxcywh, img_w, img_h, top_k=200, min_score=0.2, iou_threshold=0.45, score="softmax", nms="hard",
               sigma=0.5, keep_score=None):
    """-> (boxes (top_k,4), classes (top_k,) i64, probs (top_k,), prior_ids (top_k,) i32, count (1,) i32), all device.
    nms = "linear" / "gaussian": Soft-NMS (probs are the decayed scores; keep_score None = min_score).
    score = "sigmoid": the probability of a class is the sigmoid of its own column (a model trained with conf_loss="focal"); the
    default "softmax" makes the call it has always made."""
    method = nms_method(nms)
    smode = score_mode(score)
    _req(l_, "l_"); _req(c_, "c_"); _req(priors_cxcywh, "priors")
    p, ncls = c_.shape
    if tuple(l_.shape) != (p, 4) or tuple(priors_cxcywh.shape) != (p, 4):
        raise ValueError("decode_nms shapes")
    lib = _lib.load()
    ws = workspace(lib.ssd_decode_nms_workspace(p, ncls), l_.device, "nms")
    dev = l_.device
    boxes = torch.zeros((top_k, 4), device=dev, dtype=torch.float32)
    classes = torch.zeros((top_k,), device=dev, dtype=torch.int64)
    probs = torch.zeros((top_k,), device=dev, dtype=torch.float32)
    ids = torch.zeros((top_k,), device=dev, dtype=torch.int32)
    count = torch.zeros((1,), device=dev, dtype=torch.int32)
    if smode != 0:
        check(lib.ssd_decode_nms_score(l_.data_ptr(), c_.data_ptr(), priors_cxcywh.data_ptr(), p, ncls, float(min_score),
                                       float(iou_threshold), int(top_k), float(img_w), float(img_h), boxes.data_ptr(),
                                       classes.data_ptr(), probs.data_ptr(), ids.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(),
                                       _stream(), method, float(sigma), float(min_score if keep_score is None else keep_score), smode),
              "decode_nms_score")
        return boxes, classes, probs, ids, count
    if method != 0:
        check(lib.ssd_decode_nms_soft(l_.data_ptr(), c_.data_ptr(), priors_cxcywh.data_ptr(), p, ncls, float(min_score),
                                      float(iou_threshold), int(top_k), float(img_w), float(img_h), boxes.data_ptr(),
                                      classes.data_ptr(), probs.data_ptr(), ids.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(),
                                      _stream(), method, float(sigma), float(min_score if keep_score is None else keep_score)),
              "decode_nms_soft")
        return boxes, classes, probs, ids, count
    check(lib.ssd_decode_nms(l_.data_ptr(), c_.data_ptr(), priors_cxcywh.data_ptr(), p, ncls, float(min_score),
                             float(iou_threshold), int(top_k), float(img_w), float(img_h), boxes.data_ptr(), classes.data_ptr(),
                             probs.data_ptr(), ids.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "decode_nms")
    return boxes, classes, probs, ids, count


def decode_nms_batch(l, c, priors_cxcywh, img_wh, top_k=200, min_score=0.2, iou_threshold=0.45, score="softmax", nms="hard",
                     sigma=0.5, keep_score=None):
    """l (B,P,4), c (B,P,C), img_wh (B,2) device floats -> (boxes (B,top_k,4), classes (B,top_k) i64, probs (B,top_k),
    prior_ids (B,top_k) i32, count (B,) i32), all on the device, one launch set, no host sync.
    nms = "linear" / "gaussian": Soft-NMS (probs are the decayed scores; keep_score None = min_score).  score: as in `decode_nms`."""
    method = nms_method(nms)
    smode = score_mode(score)
    _req(l, "l"); _req(c, "c"); _req(priors_cxcywh, "priors"); _req(img_wh, "img_wh")
    b, p, ncls = c.shape
    if tuple(l.shape) != (b, p, 4) or tuple(priors_cxcywh.shape) != (p, 4) or tuple(img_wh.shape) != (b, 2):
        raise ValueError("decode_nms_batch shapes")
    lib = _lib.load()
    ws = workspace(lib.ssd_decode_nms_batch_workspace(b, p, ncls), l.device, "nms")
    dev = l.device
    boxes = torch.zeros((b, top_k, 4), device=dev, dtype=torch.float32)
    classes = torch.zeros((b, top_k), device=dev, dtype=torch.int64)
    probs = torch.zeros((b, top_k), device=dev, dtype=torch.float32)
    ids = torch.zeros((b, top_k), device=dev, dtype=torch.int32)
    count = torch.zeros((b,), device=dev, dtype=torch.int32)
    if smode != 0:
        check(lib.ssd_decode_nms_batch_score(l.data_ptr(), c.data_ptr(), priors_cxcywh.data_ptr(), img_wh.data_ptr(), b, p, ncls,
                                             float(min_score), float(iou_threshold), int(top_k), boxes.data_ptr(), classes.data_ptr(),
                                             probs.data_ptr(), ids.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(), _stream(),
                                             method, float(sigma), float(min_score if keep_score is None else keep_score), smode),
              "decode_nms_batch_score")
        return boxes, classes, probs, ids, count
    if method != 0:
        check(lib.ssd_decode_nms_batch_soft(l.data_ptr(), c.data_ptr(), priors_cxcywh.data_ptr(), img_wh.data_ptr(), b, p, ncls,
                                            float(min_score), float(iou_threshold), int(top_k), boxes.data_ptr(), classes.data_ptr(),
                                            probs.data_ptr(), ids.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(), _stream(),
                                            method, float(sigma), float(min_score if keep_score is None else keep_score)),
              "decode_nms_batch_soft")
        return boxes, classes, probs, ids, count
    check(lib.ssd_decode_nms_batch(l.data_ptr(), c.data_ptr(), priors_cxcywh.data_ptr(), img_wh.data_ptr(), b, p, ncls,
                                   float(min_score), float(iou_threshold), int(top_k), boxes.data_ptr(), classes.data_ptr(),
                                   probs.data_ptr(), ids.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
          "decode_nms_batch")
    return boxes, classes, probs, ids, count


def sgd_momentum_(param, grad, buf, lr, momentum, weight_decay, grad_scale=None, first_step=False):
    _req(param, "param"); _req(grad, "grad"); _req(buf, "buf")
    if grad.numel() != param.numel() or buf.numel() != param.numel():
        raise ValueError("sgd sizes")
    if grad_scale is not None:
        _req(grad_scale, "grad_scale")
    check(_lib.load().ssd_sgd_momentum(param.data_ptr(), grad.data_ptr(), buf.data_ptr(), param.numel(), float(lr), float(momentum),
                                       float(weight_decay), _ptr(grad_scale), int(first_step), _stream()), "sgd_momentum")


GRAD_CLIP_STATE_WORDS = 8      # total_norm, clip_coef, grad_scale (f32) | skip, skipped_steps (int32) | 3 spare: include/ssd_gfx950.h


def _norm_kind(norm_type) -> int:
    if norm_type == 2:
        return 0
    if norm_type == float("inf"):
        return 1
    raise ValueError(f"norm_type must be 2 or inf, got {norm_type!r}")


def grad_norm_slots(n: int) -> int:
    """Partial slots `grad_norm_partials_` writes for a range of n floats (host-side query, no GPU)."""
    return int(_lib.load().ssd_grad_norm_slots(int(n)))


def grad_norm_partials_(grad, partials, slot0, norm_type=2.0) -> int:
    """Per-workgroup partials of sum(g^2) (f64) or max|g| over the contiguous f32 range `grad` (16-byte aligned, a multiple of 4
    floats) into partials[slot0:]; returns the first free slot after them."""
    _req(grad, "grad"); _req(partials, "partials", torch.float64)
    if grad.numel() % 4 or grad.data_ptr() % 16:
        raise ValueError("grad_norm_partials_: the range must be 16-byte aligned and a multiple of 4 floats long (zero pads)")
    slot0 = int(slot0)
    check(_lib.load().ssd_grad_norm_partials(grad.data_ptr(), grad.numel(), _norm_kind(norm_type), partials.data_ptr(), slot0,
                                             partials.numel(), _stream()), "grad_norm_partials")
    return slot0 + grad_norm_slots(grad.numel())


def grad_clip_finalize_(partials, n_slots, norm_type, max_norm, pre_scale, guard, state):
    """partials[:n_slots] -> state (f32[GRAD_CLIP_STATE_WORDS]): total_norm, clip_coef, grad_scale, skip, skipped_steps += skip.
    max_norm None: no clipping (clip_coef = 1); pre_scale: optional 1-element device tensor the norm and the scale are multiplied by."""
    _req(partials, "partials", torch.float64); _req(state, "state")
    n_slots = int(n_slots)
    if not 0 <= n_slots <= partials.numel() or state.numel() < GRAD_CLIP_STATE_WORDS:
        raise ValueError("grad_clip_finalize_: slot count / state size")
    if pre_scale is not None:
        _req(pre_scale, "pre_scale")
    check(_lib.load().ssd_grad_clip_finalize(partials.data_ptr(), n_slots, _norm_kind(norm_type), -1.0 if max_norm is None else float(max_norm),
                                             _ptr(pre_scale), int(bool(guard)), state.data_ptr(), _stream()), "grad_clip_finalize")


def sgd_momentum_guarded_(param, grad, buf, lr, momentum, weight_decay, grad_scale, first_step, skip):
    """`sgd_momentum_` that leaves parameters and momentum untouched when the device flag `skip` (int32) is set."""
    _req(param, "param"); _req(grad, "grad"); _req(buf, "buf"); _req(skip, "skip", torch.int32)
    if grad.numel() != param.numel() or buf.numel() != param.numel():
        raise ValueError("sgd sizes")
    if grad_scale is not None:
        _req(grad_scale, "grad_scale")
    check(_lib.load().ssd_sgd_momentum_guarded(param.data_ptr(), grad.data_ptr(), buf.data_ptr(), param.numel(), float(lr), float(momentum),
                                               float(weight_decay), _ptr(grad_scale), int(first_step), skip.data_ptr(), _stream()),
          "sgd_momentum_guarded")


SCHED_STATE_HEAD = 2           # step (int32), ema_w (f32), then one f32 lr word per parameter group: include/ssd_gfx950.h


def sgd_schedule_advance_(state, lr_table, ema_decay=None, ema_warmup=True, skip=None):
    """One step of the device schedule: state (int32[2 + G]) <- lr words from column min(step, T-1) of lr_table (f32 (G, T)), the EMA
    weight of this step (ema_decay None: 0), step + 1.  skip: optional int32 device flag; when it is set nothing is written."""
    _req(state, "state", torch.int32); _req(lr_table, "lr_table")
    if lr_table.dim() != 2 or lr_table.shape[0] < 1 or lr_table.shape[1] < 1 or state.numel() < SCHED_STATE_HEAD + lr_table.shape[0]:
        raise ValueError("sgd_schedule_advance_: lr_table must be (groups, steps) and state hold 2 + groups words")
    if skip is not None:
        _req(skip, "skip", torch.int32)
    check(_lib.load().ssd_sgd_schedule_advance(state.data_ptr(), lr_table.data_ptr(), int(lr_table.shape[0]), int(lr_table.shape[1]),
                                               -1.0 if ema_decay is None else float(ema_decay), int(bool(ema_warmup)), _ptr(skip),
                                               _stream()), "sgd_schedule_advance")


def sgd_momentum_sched_(param, grad, buf, ema, lr_dev, ema_w_dev, momentum, weight_decay, grad_scale=None, first_step=False, skip=None):
    """`sgd_momentum_` whose learning rate is the device word `lr_dev`, that writes nothing when the device flag `skip` is set, and
    that, given `ema`, moves it towards the new parameters by the device weight `ema_w_dev` in the same pass."""
    _req(param, "param"); _req(grad, "grad"); _req(buf, "buf"); _req(lr_dev, "lr_dev")
    if grad.numel() != param.numel() or buf.numel() != param.numel() or lr_dev.numel() < 1:
        raise ValueError("sgd sizes")
    if ema is not None:
        _req(ema, "ema"); _req(ema_w_dev, "ema_w_dev")
        if ema.numel() != param.numel() or ema_w_dev.numel() < 1:
            raise ValueError("sgd sizes")
    if grad_scale is not None:
        _req(grad_scale, "grad_scale")
    if skip is not None:
        _req(skip, "skip", torch.int32)
    check(_lib.load().ssd_sgd_momentum_sched(param.data_ptr(), grad.data_ptr(), buf.data_ptr(), _ptr(ema), param.numel(), lr_dev.data_ptr(),
                                             _ptr(ema_w_dev) if ema is not None else None, float(momentum), float(weight_decay),
                                             _ptr(grad_scale), int(first_step), _ptr(skip), _stream()), "sgd_momentum_sched")


def swap_f32_(a, b):
    """Exchange the contents of two disjoint f32 ranges of equal length, in place."""
    _req(a, "a"); _req(b, "b")
    if a.numel() != b.numel():
        raise ValueError("swap_f32_: sizes")
    check(_lib.load().ssd_swap_f32(a.data_ptr(), b.data_ptr(), a.numel(), _stream()), "swap_f32")


ADAM_STATE_WORDS = 3           # pow1, pow2 (f64), then step (int32) in the low half of the third 8-byte word: include/ssd_gfx950.h


def adam_state(device, step: int = 0, pow1: float = 1.0, pow2: float = 1.0) -> torch.Tensor:
    """A new Adam state block (f64[ADAM_STATE_WORDS]); `adam_state_step` is the int32 view of its counter."""
    state = torch.tensor([pow1, pow2, 0.0], dtype=torch.float64)
    state.view(torch.int32)[4] = int(step)
    return state.to(device)


def adam_state_step(state) -> torch.Tensor:
    """0-dim int32 view of the block's step counter."""
    return state.view(torch.int32)[4]


def adam_advance_(state, beta1, beta2, skip=None):
    """One step of the Adam state block: step + 1, pow1 * beta1, pow2 * beta2 (one f64 multiply each).  skip: optional int32 device
    flag; when it is set nothing is written."""
    _req(state, "state", torch.float64)
    if state.numel() < ADAM_STATE_WORDS:
        raise ValueError("adam_advance_: state holds 3 f64 words")
    if skip is not None:
        _req(skip, "skip", torch.int32)
    check(_lib.load().ssd_adam_advance(state.data_ptr(), float(beta1), float(beta2), _ptr(skip), _stream()), "adam_advance")


def adam_step_(param, grad, exp_avg, exp_avg_sq, ema, lr, lr_dev, ema_w_dev, state, beta1, beta2, eps, weight_decay, decoupled,
               grad_scale=None, skip=None):
    """One fused Adam (decoupled False: L2 weight decay) or AdamW (True) launch over equally long flat slices, at the host rate `lr`
    (f64) or, given `lr_dev`, at that f32 device word; the bias corrections come from `state`, which `adam_advance_` has advanced for
    this step.  Given `ema`, it moves towards the new parameters by the device weight `ema_w_dev` in the same pass; when the device
    flag `skip` is set nothing is written."""
    _req(param, "param"); _req(grad, "grad"); _req(exp_avg, "exp_avg"); _req(exp_avg_sq, "exp_avg_sq"); _req(state, "state", torch.float64)
    n = param.numel()
    if grad.numel() != n or exp_avg.numel() != n or exp_avg_sq.numel() != n or state.numel() < ADAM_STATE_WORDS:
        raise ValueError("adam sizes")
    if lr_dev is not None:
        _req(lr_dev, "lr_dev")
        if lr_dev.numel() < 1:
            raise ValueError("adam sizes")
    if ema is not None:
        _req(ema, "ema"); _req(ema_w_dev, "ema_w_dev")
        if ema.numel() != n or ema_w_dev.numel() < 1:
            raise ValueError("adam sizes")
    if grad_scale is not None:
        _req(grad_scale, "grad_scale")
    if skip is not None:
        _req(skip, "skip", torch.int32)
    check(_lib.load().ssd_adam_step(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), _ptr(ema), n, float(lr),
                                    _ptr(lr_dev), _ptr(ema_w_dev) if ema is not None else None, state.data_ptr(), float(beta1),
                                    float(beta2), float(eps), float(weight_decay), int(bool(decoupled)), _ptr(grad_scale), _ptr(skip),
                                    _stream()), "adam_step")


def map_eval(det_boxes, det_classes, det_scores, det_start, gt_boxes, gt_classes, gt_start, recall_levels, n_classes=20):
    """Concatenated detections / ground truth (see include/ssd_gfx950.h ssd_map_eval) -> (table (n_classes, n_levels)
    float64, tp (D,) uint8, counts (2, n_classes) int32).  recall_levels: host sequence of floats."""
    import numpy as np
    dev = det_start.device
    D, G, B = int(det_boxes.shape[0]), int(gt_boxes.shape[0]), int(det_start.numel()) - 1
    _req(det_boxes, "det_boxes"); _req(det_scores, "det_scores"); _req(gt_boxes, "gt_boxes")
    _req(det_classes, "det_classes", torch.int32); _req(gt_classes, "gt_classes", torch.int32)
    _req(det_start, "det_start", torch.int32); _req(gt_start, "gt_start", torch.int32)
    if det_classes.numel() != D or det_scores.numel() != D or gt_classes.numel() != G or gt_start.numel() != B + 1 or B < 1:
        raise ValueError("map_eval: inconsistent array lengths")
    lv = np.ascontiguousarray(np.asarray(recall_levels, np.float64))
    tp = torch.zeros(max(D, 1), device=dev, dtype=torch.uint8)
    table = torch.empty((n_classes, lv.size), device=dev, dtype=torch.float64)
    counts = torch.empty((2, n_classes), device=dev, dtype=torch.int32)
    lib = _lib.load()
    ws = workspace(lib.ssd_map_eval_workspace(D, G), dev, "map")
    check(lib.ssd_map_eval(_ptr(det_boxes), _ptr(det_classes), _ptr(det_scores), det_start.data_ptr(), D, _ptr(gt_boxes),
                           _ptr(gt_classes), gt_start.data_ptr(), G, B, n_classes, lv.ctypes.data, int(lv.size), tp.data_ptr(),
                           table.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "map_eval")
    return table, tp[:D], counts


# launches of the evaluator's entry points since import: the matching pass runs once per batch whatever the number of thresholds
launch_counts = {"eval_match": 0, "eval_ap": 0, "coco_match": 0, "coco_ap": 0}


def _det_layout(name, det_boxes, det_classes, det_scores, det_start, det_count, gt_boxes, gt_classes, gt_start, n_gt):
    """The dtype checks the match entries share and the layout of their detections: concatenated (det_start) or padded (det_count)
    -> (B, K, D), K = 0 for concatenated rows."""
    _req(det_boxes, "det_boxes"); _req(det_scores, "det_scores"); _req(gt_boxes, "gt_boxes")
    _req(det_classes, "det_classes", torch.int32); _req(gt_classes, "gt_classes", torch.int32)
    _req(gt_start, "gt_start", torch.int32); _req(n_gt, "n_gt", torch.int32)
    if (det_start is None) == (det_count is None):
        raise ValueError(f"{name}: give det_start (concatenated rows) or det_count (padded rows), not both")
    if det_count is not None:
        _req(det_count, "det_count", torch.int32)
        if det_boxes.dim() != 3 or det_boxes.shape[2] != 4 or det_boxes.shape[1] < 1:
            raise ValueError(f"{name}: padded detections must be (B,K,4) with K >= 1")
        B, K = int(det_boxes.shape[0]), int(det_boxes.shape[1])
        D = B * K
        if tuple(det_classes.shape) != (B, K) or tuple(det_scores.shape) != (B, K) or det_count.numel() != B:
            raise ValueError(f"{name}: inconsistent padded shapes")
    else:
        _req(det_start, "det_start", torch.int32)
        if det_boxes.dim() != 2 or det_boxes.shape[1] != 4:
            raise ValueError(f"{name}: concatenated detections must be (D,4)")
        B, K, D = int(det_start.numel()) - 1, 0, int(det_boxes.shape[0])
        if det_classes.numel() != D or det_scores.numel() != D:
            raise ValueError(f"{name}: inconsistent array lengths")
    return B, K, D


def eval_match(det_boxes, det_classes, det_scores, det_start, det_count, gt_boxes, gt_classes, gt_difficult, gt_start, n_gt,
               thresholds, n_classes):
    """One batch of the detection evaluator (include/ssd_gfx950.h ssd_eval_match).  Detections: concatenated (D,4)/(D,)/(D,) with
    det_start (B+1,) int32 and det_count None, or padded (B,K,4)/(B,K)/(B,K) with det_count (B,) int32 and det_start None; classes
    int32.  Ground truth: (G,4), (G,) int32, optional (G,) uint8 difficult flags, gt_start (B+1,) int32.  n_gt (n_classes,) int32 is
    added to.  thresholds: host sequence of floats.  -> (rec_classes int32, tp int16, ignored int16), one entry per detection row
    (the 16-bit masks are bit patterns: view them as uint16).  Enqueues only; no host synchronisation."""
    import numpy as np
    B, K, D = _det_layout("eval_match", det_boxes, det_classes, det_scores, det_start, det_count, gt_boxes, gt_classes, gt_start, n_gt)
    G = int(gt_boxes.shape[0])
    if B < 1 or gt_boxes.dim() != 2 or gt_boxes.shape[1] != 4 or gt_classes.numel() != G or gt_start.numel() != B + 1 \
            or n_gt.numel() != n_classes:
        raise ValueError("eval_match: inconsistent array lengths")
    if gt_difficult is not None:
        _req(gt_difficult, "gt_difficult", torch.uint8)
        if gt_difficult.numel() != G:
            raise ValueError("eval_match: gt_difficult must have one flag per ground-truth box")
    dev = gt_start.device
    thr = np.ascontiguousarray(np.asarray(thresholds, np.float32))
    rec = torch.empty(max(D, 1), device=dev, dtype=torch.int32)
    tp = torch.empty(max(D, 1), device=dev, dtype=torch.int16)
    ign = torch.empty(max(D, 1), device=dev, dtype=torch.int16)
    lib = _lib.load()
    ws = workspace(lib.ssd_eval_match_workspace(G), dev, "eval_match")
    check(lib.ssd_eval_match(_ptr(det_boxes), _ptr(det_classes), _ptr(det_scores), _ptr(det_start), _ptr(det_count), K, D,
                             _ptr(gt_boxes), _ptr(gt_classes), _ptr(gt_difficult), gt_start.data_ptr(), G, B, int(n_classes),
                             thr.ctypes.data, int(thr.size), rec.data_ptr(), tp.data_ptr(), ign.data_ptr(), n_gt.data_ptr(),
                             ws.data_ptr(), ws.numel(), _stream()), "eval_match")
    launch_counts["eval_match"] += 1
    return rec[:D], tp[:D], ign[:D]


def eval_ap(rec_classes, det_scores, tp, ignored, n_gt, n_thresholds, n_levels, n_classes):
    """Per-class order and AP tables of the detection evaluator (include/ssd_gfx950.h ssd_eval_ap) over D detection rows.
    n_levels: 10, 100 or 0 (all-point).  -> (out float64 (T, n_classes, n_levels + 1) or (T, n_classes), n_det (n_classes,) int32)."""
    _req(rec_classes, "rec_classes", torch.int32); _req(det_scores, "det_scores"); _req(n_gt, "n_gt", torch.int32)
    _req(tp, "tp", torch.int16); _req(ignored, "ignored", torch.int16)
    D = int(rec_classes.numel())
    if det_scores.numel() != D or tp.numel() != D or ignored.numel() != D or n_gt.numel() != n_classes:
        raise ValueError("eval_ap: inconsistent array lengths")
    dev = n_gt.device
    shape = (n_thresholds, n_classes, n_levels + 1) if n_levels else (n_thresholds, n_classes)
    out = torch.empty(shape, device=dev, dtype=torch.float64)
    n_det = torch.empty(n_classes, device=dev, dtype=torch.int32)
    lib = _lib.load()
    ws = workspace(lib.ssd_eval_ap_workspace(D), dev, "eval_ap")
    nz = D > 0
    check(lib.ssd_eval_ap(_ptr(rec_classes) if nz else None, _ptr(det_scores) if nz else None, _ptr(tp) if nz else None,
                          _ptr(ignored) if nz else None, D, n_gt.data_ptr(), int(n_classes), int(n_thresholds), int(n_levels),
                          out.data_ptr(), n_det.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "eval_ap")
    launch_counts["eval_ap"] += 1
    return out, n_det


def coco_match(det_boxes, det_classes, det_scores, det_start, det_count, gt_boxes, gt_classes, gt_crowd, gt_area, gt_start, n_gt,
               thresholds, area_lo, area_hi, max_det_last, n_classes):
    """One batch of the COCO evaluator (include/ssd_gfx950.h ssd_coco_match).  Detections and ground truth as `eval_match` takes them;
    gt_crowd: optional (G,) uint8 flags, gt_area: optional (G,) float32 areas (None: the box area).  n_gt (A, n_classes) int32 is added
    to.  thresholds, area_lo, area_hi: host sequences of floats; max_det_last: the largest maxDets value.  -> (rec_classes int32,
    tp int64, ignored int64, rank int32), one entry per detection row; bit a*16 + t of the 64-bit words is area range a at
    threshold t (bit patterns: view them as four uint16).  Enqueues only; no host synchronisation."""
    import numpy as np
    B, K, D = _det_layout("coco_match", det_boxes, det_classes, det_scores, det_start, det_count, gt_boxes, gt_classes, gt_start, n_gt)
    G = int(gt_boxes.shape[0])
    thr = np.ascontiguousarray(np.asarray(thresholds, np.float32))
    lo = np.ascontiguousarray(np.asarray(area_lo, np.float32))
    hi = np.ascontiguousarray(np.asarray(area_hi, np.float32))
    if B < 1 or gt_boxes.dim() != 2 or gt_boxes.shape[1] != 4 or gt_classes.numel() != G or gt_start.numel() != B + 1 \
            or lo.ndim != 1 or lo.shape != hi.shape or n_gt.numel() != lo.size * n_classes:
        raise ValueError("coco_match: inconsistent array lengths")
    if gt_crowd is not None:
        _req(gt_crowd, "gt_crowd", torch.uint8)
        if gt_crowd.numel() != G:
            raise ValueError("coco_match: gt_crowd must have one flag per ground-truth box")
    if gt_area is not None:
        _req(gt_area, "gt_area")
        if gt_area.numel() != G:
            raise ValueError("coco_match: gt_area must have one value per ground-truth box")
    dev = gt_start.device
    rec = torch.empty(max(D, 1), device=dev, dtype=torch.int32)
    tp = torch.empty(max(D, 1), device=dev, dtype=torch.int64)
    ign = torch.empty(max(D, 1), device=dev, dtype=torch.int64)
    rank = torch.empty(max(D, 1), device=dev, dtype=torch.int32)
    lib = _lib.load()
    ws = workspace(lib.ssd_coco_match_workspace(G), dev, "coco_match")
    check(lib.ssd_coco_match(_ptr(det_boxes), _ptr(det_classes), _ptr(det_scores), _ptr(det_start), _ptr(det_count), K, D,
                             _ptr(gt_boxes), _ptr(gt_classes), _ptr(gt_crowd), _ptr(gt_area), gt_start.data_ptr(), G, B, int(n_classes),
                             thr.ctypes.data, int(thr.size), lo.ctypes.data, hi.ctypes.data, int(lo.size), int(max_det_last),
                             rec.data_ptr(), tp.data_ptr(), ign.data_ptr(), rank.data_ptr(), n_gt.data_ptr(), ws.data_ptr(), ws.numel(),
                             _stream()), "coco_match")
    launch_counts["coco_match"] += 1
    return rec[:D], tp[:D], ign[:D], rank[:D]


def coco_ap(rec_classes, det_scores, tp, ignored, rank, n_gt, n_thresholds, n_areas, max_dets, n_classes):
    """Per-class order, 101-level precision tables and true-positive counts of the COCO evaluator (include/ssd_gfx950.h ssd_coco_ap)
    over D detection rows.  max_dets: host sequence of ascending integers.  -> (out float64 (T, A, n_classes, 101), tp_count int32
    (T, A, M, n_classes), n_det (n_classes,) int32)."""
    import numpy as np
    _req(rec_classes, "rec_classes", torch.int32); _req(det_scores, "det_scores"); _req(n_gt, "n_gt", torch.int32)
    _req(tp, "tp", torch.int64); _req(ignored, "ignored", torch.int64); _req(rank, "rank", torch.int32)
    D = int(rec_classes.numel())
    md = np.ascontiguousarray(np.asarray(max_dets, np.int32))
    if det_scores.numel() != D or tp.numel() != D or ignored.numel() != D or rank.numel() != D or md.ndim != 1 \
            or n_gt.numel() != n_areas * n_classes:
        raise ValueError("coco_ap: inconsistent array lengths")
    dev = n_gt.device
    out = torch.empty((n_thresholds, n_areas, n_classes, 101), device=dev, dtype=torch.float64)
    tp_count = torch.empty((n_thresholds, n_areas, int(md.size), n_classes), device=dev, dtype=torch.int32)
    n_det = torch.empty(n_classes, device=dev, dtype=torch.int32)
    lib = _lib.load()
    ws = workspace(lib.ssd_coco_ap_workspace(D), dev, "coco_ap")
    nz = D > 0
    check(lib.ssd_coco_ap(_ptr(rec_classes) if nz else None, _ptr(det_scores) if nz else None, _ptr(tp) if nz else None,
                          _ptr(ignored) if nz else None, _ptr(rank) if nz else None, D, n_gt.data_ptr(), int(n_classes),
                          int(n_thresholds), int(n_areas), md.ctypes.data, int(md.size), out.data_ptr(), tp_count.data_ptr(),
                          n_det.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "coco_ap")
    launch_counts["coco_ap"] += 1
    return out, tp_count, n_det


def preprocess_u8(arena: torch.Tensor, descs, out_hw=(300, 300), mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225),
                  filler=(123, 116, 103)) -> torch.Tensor:
    """arena: uint8 device tensor holding the HWC RGB images; descs: ctypes array of _lib.ImageDesc (host).
    -> (B,3,out_h,out_w) float32: expand / crop / flip geometry, Pillow-exact bilinear resize, /255, (x-mean)/std."""
    import numpy as np
    _req(arena, "arena", torch.uint8)
    B = len(descs)
    oh, ow = out_hw
    for d in descs:
        if d.src_offset < 0 or d.src_offset + d.src_h * d.src_w * 3 > arena.numel():
            raise ValueError("image descriptor points outside the arena")
    lib = _lib.load()
    nbytes = lib.ssd_preprocess_workspace(C.byref(descs), B, oh, ow)
    if nbytes == 0:
        raise ValueError("preprocess_u8: bad geometry (window outside the canvas, empty image, or a down-scale factor above 31)")
    ws = workspace(nbytes, arena.device, "pre")
    raw = np.frombuffer(bytes(descs), dtype=np.uint8)          # bytes() copies: safe to hand to torch
    descs_dev = torch.from_numpy(raw.copy()).to(arena.device, non_blocking=False)
    out = torch.empty((B, 3, oh, ow), device=arena.device, dtype=torch.float32)
    m = (C.c_float * 3)(*mean); s_ = (C.c_float * 3)(*std); f = (C.c_uint8 * 3)(*filler)
    check(lib.ssd_preprocess_u8(arena.data_ptr(), descs_dev.data_ptr(), C.byref(descs), B, oh, ow, C.addressof(m), C.addressof(s_),
                                C.addressof(f), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "preprocess_u8")
    return out


def preprocess_tiles_u8(arena: torch.Tensor, tiles, B: int, out_hw=(300, 300), mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225),
                        filler=(123, 116, 103)) -> torch.Tensor:
    """The resize / normalise pass into destination rectangles (include/ssd_gfx950.h ssd_preprocess_tiles_u8).  arena: uint8 device
    tensor holding the HWC RGB sources; tiles: ctypes array of _lib.TileDesc (host) whose rectangles cover each of the B output images
    exactly once; their reserved[] (where each tile's scratch lies in the workspace) are filled here.  -> (B,3,out_h,out_w) float32."""
    import numpy as np
    _req(arena, "arena", torch.uint8)
    T = len(tiles)
    oh, ow = out_hw
    # struct ssd_tile_desc as a numpy record; a view: the reserved[] written below are the descriptors' own
    v = np.frombuffer(tiles, dtype=np.dtype([("src_offset", "<i8")] + [("src_" + n[0] if n[0] == "reserved" else n[0], "<i4") for n in
                                                                       _lib.ImageDesc._fields_[1:] + _lib.TileDesc._fields_[1:-1]] +
                                            [("reserved", "<i4", (3,))]))
    if ((v["src_offset"] < 0) | (v["src_offset"] + v["src_h"].astype(np.int64) * v["src_w"] * 3 > arena.numel())).any():
        raise ValueError("image descriptor points outside the arena")
    dst_w, dst_h = np.maximum(v["dst_w"], 0).astype(np.int64), np.maximum(v["dst_h"], 0).astype(np.int64)
    rows = np.cumsum(dst_w + dst_h)
    units = np.cumsum((np.maximum(v["crop_h"], 0) * dst_w * 3 + 255) // 256)
    if rows[-1] >= 1 << 31 or units[-1] >= 1 << 31:
        raise ValueError("preprocess_tiles_u8: the tiles' scratch rows do not fit 32-bit offsets")
    v["reserved"][:, 0] = rows - (dst_w + dst_h)
    v["reserved"][:, 1] = units - (np.maximum(v["crop_h"], 0) * dst_w * 3 + 255) // 256
    v["reserved"][:, 2] = 0
    lib = _lib.load()
    nbytes = lib.ssd_preprocess_tiles_workspace(C.byref(tiles), T, B, oh, ow)
    if nbytes == 0:
        raise ValueError("preprocess_tiles_u8: bad geometry (a window outside its canvas, an empty image or rectangle, a crop more than "
                         "31 times its rectangle, or rectangles that do not cover every output image exactly once)")
    ws = workspace(nbytes, arena.device, "pre_tiles")
    tiles_dev = torch.from_numpy(np.frombuffer(bytes(tiles), dtype=np.uint8).copy()).to(arena.device, non_blocking=False)
    out = torch.empty((B, 3, oh, ow), device=arena.device, dtype=torch.float32)
    m = (C.c_float * 3)(*mean); s_ = (C.c_float * 3)(*std); f = (C.c_uint8 * 3)(*filler)
    check(lib.ssd_preprocess_tiles_u8(arena.data_ptr(), tiles_dev.data_ptr(), C.byref(tiles), T, B, oh, ow, C.addressof(m), C.addressof(s_),
                                      C.addressof(f), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "preprocess_tiles_u8")
    return out


def affine_warp(x: torch.Tensor, mats, fill) -> torch.Tensor:
    """Random affine augmentation of a normalised batch (include/ssd_gfx950.h ssd_affine_warp_f32).  x: (B,3,H,W) float32 device tensor;
    mats: (B,6) float32 host array or CPU tensor, per image the coefficients that map an output pixel centre to input coordinates;
    fill: the three normalised filler values every tap outside the image reads.  -> a new (B,3,H,W) float32 tensor; only enqueues."""
    import numpy as np
    _req(x, "x")
    if x.dim() != 4 or x.shape[1] != 3 or x.numel() == 0:
        raise ValueError(f"affine_warp: x must be (B,3,H,W) with B, H, W >= 1, got {tuple(x.shape)}")
    B, _, H, W = x.shape
    if torch.is_tensor(mats):
        if mats.is_cuda:
            raise ValueError("affine_warp: mats is host data (a CPU tensor or an array): the library validates it before it enqueues")
        mats = mats.numpy()
    m = np.asarray(mats)
    if m.dtype != np.float32 or m.shape != (B, 6):
        raise ValueError(f"affine_warp: mats must be float32 of shape ({B}, 6), got {m.dtype} {m.shape}")
    m = np.ascontiguousarray(m)
    if not np.isfinite(m).all():
        raise ValueError("affine_warp: a coefficient is not finite")
    if B > 65535 or H * W >= 1 << 31:
        raise ValueError("affine_warp: at most 65535 images of fewer than 2^31 pixels")
    if len(fill) != 3:
        raise ValueError("affine_warp: fill is three values, one per channel")
    f = (C.c_float * 3)(*(float(v) for v in fill))
    mats_dev = torch.from_numpy(m.copy()).to(x.device, non_blocking=True)
    out = torch.empty_like(x)
    check(_lib.load().ssd_affine_warp_f32(x.data_ptr(), out.data_ptr(), mats_dev.data_ptr(), m.ctypes.data, B, H, W, C.addressof(f),
                                          _stream()), "affine_warp")
    return out


def clock_probe(device) -> torch.Tensor:
    """Enqueue a clock probe on the current stream; returns the (16, 2) int64 tensor it fills (counter, 100 MHz ticks per XCC)."""
    out = torch.zeros((16, 2), device=device, dtype=torch.int64)
    check(_lib.load().ssd_clock_probe(out.data_ptr(), _stream()), "clock_probe")
    return out


def shader_mhz(probe_a: torch.Tensor, probe_b: torch.Tensor) -> float:
    """Average shader clock between two probes (mean over the XCCs both probes landed on)."""
    a, b = probe_a.cpu(), probe_b.cpu()
    ok = (a[:, 1] > 0) & (b[:, 1] > a[:, 1])
    if not bool(ok.any()):
        return float("nan")
    return float((100.0 * (b[ok, 0] - a[ok, 0]).double() / (b[ok, 1] - a[ok, 1]).double()).mean())


def photometric_u8(arena: torch.Tensor, descs, photo) -> None:
    """In place on the arena's source images: photo = ctypes array of _lib.PhotoDesc (one per image, same order as descs)."""
    import numpy as np
    _req(arena, "arena", torch.uint8)
    B = len(descs)
    if len(photo) != B:
        raise ValueError("one photo descriptor per image")
    for d in descs:
        if d.src_offset < 0 or d.src_offset + d.src_h * d.src_w * 3 > arena.numel():
            raise ValueError("image descriptor points outside the arena")
    lib = _lib.load()
    ws = workspace(lib.ssd_photometric_workspace(B), arena.device, "photo")
    d_dev = torch.from_numpy(np.frombuffer(bytes(descs), dtype=np.uint8).copy()).to(arena.device)
    p_dev = torch.from_numpy(np.frombuffer(bytes(photo), dtype=np.uint8).copy()).to(arena.device)
    check(lib.ssd_photometric_u8(arena.data_ptr(), d_dev.data_ptr(), C.byref(descs), p_dev.data_ptr(), C.byref(photo), B, ws.data_ptr(),
                                 ws.numel(), _stream()), "photometric_u8")


JPEG_ENTROPY, JPEG_IDCT, JPEG_COLOUR, JPEG_ALL = 1, 2, 4, 7


def jpeg_fill_desc(d, header, stream_offset: int, dst_offset: int, dst_bytes: int, seg_first: int) -> None:
    """Fill one _lib.JpegDesc from a `Dataset.JpegHeader` (host only; the C entry validates what it is given)."""
    import numpy as np
    d.stream_offset, d.dst_offset, d.dst_bytes = int(stream_offset), int(dst_offset), int(dst_bytes)
    d.stream_bytes = int(header.data_end - header.data_begin)
    d.seg_first, d.n_segments, d.restart_interval = int(seg_first), len(header.seg_offsets), int(header.restart_interval)
    d.width, d.height, d.n_components, d.h_samp, d.v_samp = header.width, header.height, header.n_components, header.h_samp, header.v_samp
    for c in range(header.n_components):
        d.quant_sel[c], d.dc_sel[c], d.ac_sel[c] = header.quant_sel[c], header.dc_sel[c], header.ac_sel[c]
    for t, q in header.quant_tables.items():
        C.memmove(d.quant[t], np.ascontiguousarray(q, np.uint16).ctypes.data, 128)
    for (tc, th), (bits, vals) in header.huff_tables.items():
        t = 2 * tc + th
        if len(bits) != 16 or len(vals) > 256:
            raise ValueError("jpeg: a Huffman table has 16 length counts and at most 256 values")
        d.n_huffval[t] = len(vals)
        C.memmove(d.bits[t], np.ascontiguousarray(bits, np.uint8).ctypes.data, 16)
        C.memmove(d.huffval[t], np.ascontiguousarray(vals, np.uint8).ctypes.data, len(vals))


# The entropy decode gives a restart segment to ONE lane ("segment") or cuts it into subsequences that many lanes decode and repair
# ("split", csrc/jpeg_split.hip).  Both constants are measured (tools/jpeg_decode_bench.py, profiles/jpeg_split_bench.json).
JPEG_SUBSEQUENCE_BYTES = 64          # the default subsequence size of "split": the fastest of 64 / 128 / 256 / 512 on 32 files of 44 KB
JPEG_SPLIT_AUTO_BYTES = 2361         # "auto" takes "split" when the batch's longest segment has more bytes than this: the shortest
#                                      segments of the restart-interval sweep at which "split" beat "segment" by more than the windows spread
JPEG_ENTROPY_MODES = ("segment", "split", "auto")


def _jpeg_longest_segment(descs, segs) -> int:
    longest = 0
    for d in descs:
        first, n = int(d.seg_first), int(d.n_segments)
        if n < 1 or first < 0 or first + n > len(segs):
            raise ValueError("jpeg: a descriptor's segments lie outside seg_offsets")
        ends = [int(segs[first + k + 1]) - 2 for k in range(n - 1)] + [int(d.stream_bytes)]
        longest = max(longest, max(e - int(segs[first + k]) for k, e in enumerate(ends)))
    return longest


def jpeg_entropy_auto(descs, seg_offsets) -> str:
    """What `entropy="auto"` chooses for a batch (host only): "split" when its longest restart segment exceeds
    JPEG_SPLIT_AUTO_BYTES -- files without restart markers, one segment each -- else "segment"."""
    import numpy as np
    segs = np.asarray(seg_offsets, np.int32).reshape(-1)
    return "split" if _jpeg_longest_segment(descs, segs) > JPEG_SPLIT_AUTO_BYTES else "segment"


def jpeg_decode_(arena: torch.Tensor, descs, seg_offsets, stages: int = JPEG_ALL, entropy: str = "auto",
                 subsequence_bytes: Optional[int] = None, stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Decode baseline JPEG streams held in `arena` (uint8, device) into their pixel slots of the same arena, in place
    (include/ssd_gfx950.h ssd_jpeg_decode_u8 / ssd_jpeg_decode_split_u8).  descs: ctypes array of _lib.JpegDesc (host);
    seg_offsets: int32 array, the restart-segment offsets of all images.  entropy: "segment" (one lane per restart segment), "split"
    (many lanes per segment, subsequence_bytes each: a multiple of 4 in 8 .. 4096, default JPEG_SUBSEQUENCE_BYTES) or "auto"
    (`jpeg_entropy_auto`); the pixels and the status do not depend on it.  stats ("split" only): int32 (B, 4) on the device, receives
    subsequences, repair rounds, subsequence walks, 0 per image.  -> status (B,) int32 on the device: 0 = decoded, else the slot is
    zero-filled.  Enqueues only; reading the status is the caller's synchronisation."""
    import numpy as np
    if entropy not in JPEG_ENTROPY_MODES:
        raise ValueError(f"jpeg_decode_: entropy must be one of {JPEG_ENTROPY_MODES}, not {entropy!r}")
    sub = JPEG_SUBSEQUENCE_BYTES if subsequence_bytes is None else subsequence_bytes
    if not isinstance(sub, int) or isinstance(sub, bool) or sub < 8 or sub > 4096 or sub % 4:
        raise ValueError("jpeg_decode_: subsequence_bytes must be a multiple of 4 in 8 .. 4096")
    _req(arena, "arena", torch.uint8)
    if arena.dim() != 1:
        raise ValueError("jpeg_decode_: arena must be 1-D")
    B = len(descs)
    segs = np.ascontiguousarray(np.asarray(seg_offsets, np.int32))
    if B == 0 or segs.ndim != 1 or segs.size == 0:
        raise ValueError("jpeg_decode_: at least one image and one segment")
    if entropy == "auto":
        entropy = jpeg_entropy_auto(descs, segs)
    if stats is not None:
        if entropy != "split":
            raise ValueError("jpeg_decode_: stats are those of entropy='split'")
        _req(stats, "stats", torch.int32)
        if tuple(stats.shape) != (B, 4) or stats.device != arena.device:
            raise ValueError("jpeg_decode_: stats must be (B, 4) int32 on the arena's device")
    lib = _lib.load()
    if entropy == "split":
        nbytes = lib.ssd_jpeg_decode_split_workspace(C.byref(descs), B, segs.ctypes.data, int(segs.size), sub)
    else:
        nbytes = lib.ssd_jpeg_decode_workspace(C.byref(descs), B)
    if nbytes == 0:
        raise ValueError("jpeg_decode_: a descriptor is outside the decoder's scope (see include/ssd_gfx950.h)")
    ws = workspace(nbytes, arena.device, "jpeg")
    d_dev = torch.from_numpy(np.frombuffer(bytes(descs), dtype=np.uint8).copy()).to(arena.device, non_blocking=True)
    s_dev = torch.from_numpy(segs.copy()).to(arena.device, non_blocking=True)
    status = torch.empty(B, device=arena.device, dtype=torch.int32)
    if entropy == "split":
        check(lib.ssd_jpeg_decode_split_u8(arena.data_ptr(), arena.numel(), d_dev.data_ptr(), C.byref(descs), s_dev.data_ptr(),
                                           segs.ctypes.data, int(segs.size), B, status.data_ptr(), ws.data_ptr(), ws.numel(), int(stages),
                                           _stream(), sub, None if stats is None else stats.data_ptr()), "jpeg_decode_split_u8")
    else:
        check(lib.ssd_jpeg_decode_u8(arena.data_ptr(), arena.numel(), d_dev.data_ptr(), C.byref(descs), s_dev.data_ptr(), segs.ctypes.data,
                                     int(segs.size), B, status.data_ptr(), ws.data_ptr(), ws.numel(), int(stages), _stream()), "jpeg_decode_u8")
    return status


# ---- Winograd F(mo x mo, 3x3), mo = 2 or 4 --------------------------------------------------------
def wino_x3(mo: int, K: int) -> bool:
    """True if the F(4x4) plane GEMMs of reduction length K multiply three bf16 limbs per f32 operand (csrc/gemm_x3.hip); the layer's
    transformed filter is then a bf16 limb tensor (`wino_filter_alloc`)."""
    return bool(_lib.load().ssd_wino_uses_x3(mo, K))


def wino_filter_alloc(mo: int, rows: int, K: int, device) -> torch.Tensor:
    """Destination of a transformed filter with `rows` output rows and reduction length K: (P, rows, K) f32, or -- where `wino_x3` --
    the limb planes (P, K/16, 3, pad128(rows), 16) bf16, zero-filled (the padding rows are never written)."""
    P = (mo + 2) ** 2
    if wino_x3(mo, K):
        return torch.zeros((P, K // 16, 3, (rows + 127) // 128 * 128, 16), device=device, dtype=torch.bfloat16)
    return torch.empty((P, rows, K), device=device, dtype=torch.float32)


def _wino_filter(u: torch.Tensor, name: str, rows: int, K: Optional[int]) -> int:
    """Check a transformed filter against its geometry and the library's current GEMM form; returns K."""
    mo = _wino_mo(u)
    if u.dtype == torch.bfloat16:
        _req(u, name, torch.bfloat16)
        k = u.shape[1] * 16
        ok = u.dim() == 5 and tuple(u.shape[2:]) == (3, (rows + 127) // 128 * 128, 16) and (K is None or k == K)
    else:
        _req(u, name)
        k = u.shape[2] if u.dim() == 3 else -1
        ok = u.dim() == 3 and u.shape[1] == rows and (K is None or k == K)
    if not ok:
        raise ValueError(f"{name}: shape does not match the geometry")
    if (u.dtype == torch.bfloat16) != wino_x3(mo, k):
        raise ValueError(f"{name}: transformed under another ssd_tune_set_wino_x3 setting than the one in force")
    return k


def wino_weights(w_oihw: torch.Tensor, co_pad: Optional[int] = None, want_bwd: bool = True, mo: int = 2):
    """(Co,Ci,3,3) -> U_fwd (P,Co,Ci) and, if asked, U_bwd (P,Ci,co_pad), P = (mo+2)^2, for conv2d_fwd_wino / conv2d_dgrad_wino
    (either may be a limb tensor instead: `wino_filter_alloc`)."""
    _req(w_oihw, "weight")
    co, ci, r, s = w_oihw.shape
    if (r, s) != (3, 3) or mo not in (2, 4):
        raise ValueError("Winograd needs 3x3 filters and mo in (2, 4)")
    co_pad = pad32(co) if co_pad is None else co_pad
    uf = wino_filter_alloc(mo, co, ci, w_oihw.device)
    ub = wino_filter_alloc(mo, ci, co_pad, w_oihw.device) if want_bwd else None
    check(_lib.load().ssd_wino_weights(w_oihw.data_ptr(), uf.data_ptr(), _ptr(ub), co, ci, co_pad, mo, _stream()), "wino_weights")
    return uf, ub


def _wino_mo(u: torch.Tensor) -> int:
    if u.shape[0] not in (16, 36):
        raise ValueError("transformed filter must have 16 or 36 planes")
    return 2 if u.shape[0] == 16 else 4


# ---- 1x1 / stride-1 convolutions on the three-limb GEMM kernels (csrc/gemm_x3.hip; fc7, seq8.0) ---------------------------------
def x3_filter_alloc(rows: int, K: int, device) -> torch.Tensor:
    """Limb planes of a [rows][K] filter matrix: (K/16, 3, pad128(rows), 16) bf16, zero-filled (padding rows are never written)."""
    return torch.zeros((K // 16, 3, (rows + 127) // 128 * 128, 16), device=device, dtype=torch.bfloat16)


def conv1x1_weights_x3(w_oihw: torch.Tensor, co_pad: int):
    """(Co,Ci,1,1) -> (limbs of w [Co][Ci], limbs of w^T [Ci][co_pad]) for conv1x1_fwd_x3 / conv1x1_dgrad_x3 (per-layer form of the kind-4
    weight job)."""
    _req(w_oihw, "weight")
    co, ci = int(w_oihw.shape[0]), int(w_oihw.shape[1])
    if tuple(w_oihw.shape[2:]) != (1, 1) or ci % 32 != 0 or co_pad % 32 != 0 or co_pad < co:
        raise ValueError("conv1x1_weights_x3: a 1x1 filter with Ci and co_pad multiples of 32")
    lib = _lib.load()
    wf = x3_filter_alloc(co, ci, w_oihw.device)
    check(lib.ssd_gemm_x3_split_weights(w_oihw.data_ptr(), wf.data_ptr(), co, ci, 1, _stream()), "conv1x1_weights_x3")
    wt = torch.zeros((ci, co_pad), device=w_oihw.device, dtype=torch.float32)
    wt[:, :co] = w_oihw.reshape(co, ci).t()
    wb = x3_filter_alloc(ci, co_pad, w_oihw.device)
    check(lib.ssd_gemm_x3_split_weights(wt.data_ptr(), wb.data_ptr(), ci, co_pad, 1, _stream()), "conv1x1_weights_x3")
    return wf, wb


def _x3_filter(w3: torch.Tensor, name: str, rows: int, K: int) -> None:
    _req(w3, name, torch.bfloat16)
    if tuple(w3.shape) != (K // 16, 3, (rows + 127) // 128 * 128, 16):
        raise ValueError(f"{name}: limb planes do not match the geometry")


def conv1x1_fwd_x3(x: torch.Tensor, w3: torch.Tensor, bias: Optional[torch.Tensor], g: ConvGeom, relu: bool) -> torch.Tensor:
    _req(x, "x")
    if tuple(x.shape) != (g.N, g.H, g.W, g.Ci):
        raise ValueError("conv1x1_fwd_x3: x shape does not match geometry")
    _x3_filter(w3, "w3", g.Co, g.Ci)
    if bias is not None:
        _req(bias, "bias")
    y = torch.empty((g.N, g.H, g.W, g.Co), device=x.device, dtype=torch.float32)
    check(_lib.load().ssd_conv1x1_fwd_x3(x.data_ptr(), w3.data_ptr(), _ptr(bias), y.data_ptr(), g.Co, C.byref(g), int(relu), _stream()), "conv1x1_fwd_x3")
    return y


def conv1x1_dgrad_x3(dy: torch.Tensor, w3t: torch.Tensor, g: ConvGeom, dx: Optional[torch.Tensor] = None, relu_mask: Optional[torch.Tensor] = None,
                     accumulate: bool = False) -> torch.Tensor:
    _req(dy, "dy")
    ldy = dy.shape[-1]
    if dy.numel() != g.N * g.H * g.W * ldy:
        raise ValueError("conv1x1_dgrad_x3: dy size does not match geometry")
    _x3_filter(w3t, "w3t", g.Ci, ldy)
    if dx is None:
        if accumulate:
            raise ValueError("accumulate needs an existing dx")
        dx = torch.empty((g.N, g.H, g.W, g.Ci), device=dy.device, dtype=torch.float32)
    _req(dx, "dx")
    if relu_mask is not None:
        _req(relu_mask, "relu_mask")
    check(_lib.load().ssd_conv1x1_dgrad_x3(dy.data_ptr(), ldy, w3t.data_ptr(), dx.data_ptr(), _ptr(relu_mask), int(accumulate), C.byref(g), _stream()),
          "conv1x1_dgrad_x3")
    return dx


def conv1x1_wgrad_x3(x: torch.Tensor, dy: torch.Tensor, g: ConvGeom, ldy: int, want_bias: bool = True, dw_out: Optional[torch.Tensor] = None,
                     db_out: Optional[torch.Tensor] = None):
    _req(x, "x"); _req(dy, "dy")
    if tuple(x.shape) != (g.N, g.H, g.W, g.Ci) or dy.numel() != g.N * g.H * g.W * ldy or ldy < g.Co:
        raise ValueError("conv1x1_wgrad_x3: shapes do not match geometry")
    lib = _lib.load()
    nbytes = lib.ssd_conv1x1_wgrad_x3_workspace(C.byref(g), ldy)
    if nbytes == 0:
        raise ValueError("conv1x1_wgrad_x3: not a 1x1 / stride 1 geometry")
    ws = workspace(nbytes, x.device)
    dw = _grad_dst(dw_out, (g.Co, g.Ci, 1, 1), x.device, "dw_out")
    db = _grad_dst(db_out, (g.Co,), x.device, "db_out") if want_bias else None
    check(lib.ssd_conv1x1_wgrad_x3(x.data_ptr(), dy.data_ptr(), ldy, dw.data_ptr(), _ptr(db), C.byref(g), ws.data_ptr(), ws.numel(), _stream()),
          "conv1x1_wgrad_x3")
    return dw, db


def wino_planes_shape(g: ConvGeom):
    return (36, wino_tiles(g), g.Ci)


def wino_planes(g: ConvGeom, device) -> torch.Tensor:
    """Buffer for the F(4x4) transformed input of a convolution, [36][tiles][Ci] (include/ssd_gfx950.h ssd_conv3x3_wino_fwd_keep)."""
    return torch.empty((36, wino_tiles(g), g.Ci), device=device, dtype=torch.float32)


def wino_uses_full(g: ConvGeom, direction: int) -> bool:
    """True if the library runs this geometry's F(4x4) forward (0) / data gradient from dy (1) as one kernel from the activation."""
    return bool(_lib.load().ssd_conv3x3_wino_uses_full(C.byref(g), direction))


def wino_relu_bits(g: ConvGeom, device) -> torch.Tensor:
    """Buffer for the ReLU mask of a convolution's INPUT as bits: one int64 word per (tile, channel quad) (include/ssd_gfx950.h
    ssd_conv3x3_wino_fwd_keep_bits)."""
    return torch.empty((wino_tiles(g), g.Ci // 4), device=device, dtype=torch.int64)


def _fwd_wino(name: str, src: torch.Tensor, u_fwd: torch.Tensor, bias: Optional[torch.Tensor], g: ConvGeom, relu: bool, from_planes: bool = False,
              ld: Optional[int] = None, pool_ceil: Optional[bool] = None, want_argmax: bool = True, keep_planes: bool = False,
              want_bits: bool = False):
    """What the three Winograd forward wrappers share once each has checked its own source: filter and bias checks, the workspace,
    the outputs and the call -> (y or pooled y, argmax or None, kept planes or None, bits or None)."""
    _wino_filter(u_fwd, "u_fwd", g.Co, g.Ci)
    if bias is not None:
        _req(bias, "bias")
    lib, dev, mo = _lib.load(), src.device, _wino_mo(u_fwd)
    nbytes = lib.ssd_conv3x3_wino_workspace(C.byref(g), 0, mo)
    if nbytes == 0:
        raise ValueError(f"{name}: not a 3x3 / stride 1 / pad 1 geometry")
    ws = workspace(nbytes, dev, "wino")
    am = None
    if pool_ceil is None:
        ld = g.Co if ld is None else ld
        y = (torch.empty if ld == g.Co else torch.zeros)((g.N, g.H, g.W, ld), device=dev, dtype=torch.float32)
    else:
        ho, wo = pool_out(g.H, 2, 2, 0, pool_ceil), pool_out(g.W, 2, 2, 0, pool_ceil)
        y = torch.empty((g.N, ho, wo, g.Co), device=dev, dtype=torch.float32)
        am = torch.empty((g.N, ho, wo, g.Co), device=dev, dtype=torch.uint8) if want_argmax else None
    planes = wino_planes(g, dev) if keep_planes else None
    bits = wino_relu_bits(g, dev) if want_bits else None
    head, tail = (src.data_ptr(), u_fwd.data_ptr(), _ptr(bias)), (ws.data_ptr(), ws.numel(), _stream())
    if from_planes:
        dst = (y.data_ptr(), ld, None, None, C.byref(g), int(relu), 0) if pool_ceil is None else \
            (None, 0, y.data_ptr(), _ptr(am), C.byref(g), 1, int(pool_ceil))
        status = lib.ssd_conv3x3_wino_fwd_from_planes(*head, *dst, *tail)
    elif pool_ceil is not None:
        status = lib.ssd_conv3x3_wino_fwd_pool_bits(*head, y.data_ptr(), _ptr(am), C.byref(g), int(pool_ceil), _ptr(planes), _ptr(bits), *tail)
    elif keep_planes:
        status = lib.ssd_conv3x3_wino_fwd_keep_bits(*head, y.data_ptr(), ld, C.byref(g), int(relu), planes.data_ptr(), _ptr(bits), *tail)
    else:
        status = lib.ssd_conv3x3_wino_fwd(*head, y.data_ptr(), ld, C.byref(g), int(relu), mo, *tail)
    check(status, name)
    return y, am, planes, bits


def conv2d_fwd_wino(x: torch.Tensor, u_fwd: torch.Tensor, bias: Optional[torch.Tensor], g: ConvGeom, relu: bool,
                    ld: Optional[int] = None, keep_planes: bool = False, want_bits: bool = False):
    """keep_planes: also return the transformed input (F(4x4) only) for `conv2d_wgrad_wino(..., planes=)` -> (y, planes);
    want_bits (with keep_planes): also the bit mask x > 0 for `conv2d_dgrad_wino(..., bits=)` -> (y, planes, bits)."""
    _req(x, "x")
    mo = _wino_mo(u_fwd)
    if tuple(x.shape) != (g.N, g.H, g.W, g.Ci):
        raise ValueError("conv2d_fwd_wino: shapes do not match the geometry")
    if keep_planes and mo != 4:
        raise ValueError("conv2d_fwd_wino: keep_planes needs F(4x4,3x3) filters")
    if want_bits and not keep_planes:
        raise ValueError("conv2d_fwd_wino: want_bits needs keep_planes")
    y, _, planes, bits = _fwd_wino("conv2d_fwd_wino", x, u_fwd, bias, g, relu, ld=ld, keep_planes=keep_planes, want_bits=want_bits)
    if want_bits:
        return y, planes, bits
    return (y, planes) if keep_planes else y


def conv2d_fwd_wino_pool(x: torch.Tensor, u_fwd: torch.Tensor, bias: Optional[torch.Tensor], g: ConvGeom, ceil_mode: bool,
                         want_argmax: bool = True, keep_planes: bool = False, want_bits: bool = False):
    """conv3x3 -> ReLU -> max pool 2x2 / stride 2 in one pass (F(4x4,3x3) filters): (pooled y, argmax or None), the pair
    `conv2d_fwd_wino(relu=True)` + `maxpool_fwd(2, 2, 0)` returns, without the full-resolution activation in between."""
    _req(x, "x")
    if _wino_mo(u_fwd) != 4:
        raise ValueError("conv2d_fwd_wino_pool: needs F(4x4,3x3) filters")
    if tuple(x.shape) != (g.N, g.H, g.W, g.Ci) or g.Co % 4 != 0:
        raise ValueError("conv2d_fwd_wino_pool: shapes do not match the geometry")
    y, am, planes, bits = _fwd_wino("conv2d_fwd_wino_pool", x, u_fwd, bias, g, True, pool_ceil=bool(ceil_mode), want_argmax=want_argmax,
                                    keep_planes=keep_planes, want_bits=want_bits)
    if want_bits:
        return y, am, planes, bits
    return (y, am, planes) if keep_planes else (y, am)


def conv2d_fwd_wino_from_planes(planes: torch.Tensor, u_fwd: torch.Tensor, bias: Optional[torch.Tensor], g: ConvGeom, relu: bool = True,
                                pool_ceil: Optional[bool] = None, want_argmax: bool = True):
    """Forward of an F(4x4) layer whose input planes exist already (`conv1_first_wino_fwd`): plane GEMMs + output transform.
    pool_ceil None -> y (N,H,W,Co); True / False -> (pooled y, argmax or None) of the fused conv -> ReLU -> 2x2 / stride-2 pool."""
    _req(planes, "planes")
    if _wino_mo(u_fwd) != 4 or tuple(planes.shape) != tuple(wino_planes_shape(g)) or g.Co % 4 != 0:
        raise ValueError("conv2d_fwd_wino_from_planes: planes / filters do not match the geometry")
    y, am, _, _ = _fwd_wino("conv2d_fwd_wino_from_planes", planes, u_fwd, bias, g, relu, from_planes=True, pool_ceil=pool_ceil,
                            want_argmax=want_argmax)
    return y if pool_ceil is None else (y, am)


def conv2d_dgrad_wino(dy: Optional[torch.Tensor], u_bwd: torch.Tensor, g: ConvGeom, dx: Optional[torch.Tensor] = None,
                      relu_mask: Optional[torch.Tensor] = None, accumulate: bool = False,
                      planes: Optional[torch.Tensor] = None, bits: Optional[torch.Tensor] = None) -> torch.Tensor:
    """planes: B^T dy B as `conv2d_wgrad_wino(..., dgrad_planes=True)` left it ((36, tiles, Co_pad), F(4x4)); dy is then not read.
    bits (with planes): the ReLU mask as the forward's input transform left it (`conv2d_fwd_wino(..., want_bits=True)`), applied
    instead of relu_mask."""
    mo = _wino_mo(u_bwd)
    co_pad = _wino_filter(u_bwd, "u_bwd", g.Ci, None)
    dev = u_bwd.device
    if planes is not None:
        _req(planes, "planes")
        if mo != 4 or tuple(planes.shape) != (36, wino_planes_shape(g)[1], co_pad):
            raise ValueError("conv2d_dgrad_wino: planes do not match the geometry")
    else:
        _req(dy, "dy")
        if dy.numel() != g.N * g.H * g.W * co_pad:
            raise ValueError("conv2d_dgrad_wino: shapes do not match the geometry")
    if dx is None:
        if accumulate:
            raise ValueError("accumulate needs an existing dx")
        dx = torch.empty((g.N, g.H, g.W, g.Ci), device=dev, dtype=torch.float32)
    _req(dx, "dx")
    if relu_mask is not None:
        _req(relu_mask, "relu_mask")
    lib = _lib.load()
    ws = workspace(lib.ssd_conv3x3_wino_workspace(C.byref(g), 1, mo), dev, "wino")
    if bits is not None:
        _req(bits, "bits", torch.int64)
        if mo != 4 or tuple(bits.shape) != (wino_planes_shape(g)[1], g.Ci // 4) or g.Ci % 4 != 0:
            raise ValueError("conv2d_dgrad_wino: bits need F(4x4) filters and one word per (tile, channel quad)")
    # one argument list: source (dy and its row length, or the planes), filter, dx, mask (the bits win), then the rest
    src = (dy.data_ptr(), co_pad) if planes is None else (planes.data_ptr(),)
    args = (*src, u_bwd.data_ptr(), co_pad, dx.data_ptr(), _ptr(relu_mask) if bits is None else bits.data_ptr(), int(accumulate), C.byref(g),
            *((mo,) if planes is None and bits is None else ()), ws.data_ptr(), ws.numel(), _stream())
    entry = "ssd_conv3x3_wino_dgrad" + ("" if planes is None else "_planes") + ("" if bits is None else "_bits")
    check(getattr(lib, entry)(*args), "conv2d_dgrad_wino")
    return dx


def conv2d_wgrad_wino(x: Optional[torch.Tensor], dy: torch.Tensor, g: ConvGeom, ldy: int, want_bias: bool = True, mo: int = 2,
                      planes: Optional[torch.Tensor] = None, dgrad_planes: bool = False,
                      dw_out: Optional[torch.Tensor] = None, db_out: Optional[torch.Tensor] = None):
    """Winograd F(mo x mo, 3x3) weight gradient, mo = 2 or 4 -> (dw (Co,Ci,3,3) OIHW, dbias (Co,) or None).
    planes: the transformed input the forward kept (`conv2d_fwd_wino(..., keep_planes=True)`); x is then not read.
    dgrad_planes (needs planes): the pass over dy also forms this layer's dgrad input planes -> (dw, dbias, planes_dy (36, tiles, ldy))
    for `conv2d_dgrad_wino(None, ..., planes=planes_dy)`."""
    pooled = isinstance(dy, PooledGrad)
    if pooled and planes is None:
        raise ValueError("conv2d_wgrad_wino: a pooled gradient needs the kept forward planes")
    if not pooled:
        _req(dy, "dy")
    if planes is not None:
        _req(planes, "planes")
        if mo != 4 or tuple(planes.shape) != tuple(wino_planes_shape(g)):
            raise ValueError("conv2d_wgrad_wino: planes do not match the geometry")
    else:
        _req(x, "x")
        if tuple(x.shape) != (g.N, g.H, g.W, g.Ci):
            raise ValueError("conv2d_wgrad_wino: shapes do not match the geometry")
    if not pooled and dy.numel() != g.N * g.H * g.W * ldy:
        raise ValueError("conv2d_wgrad_wino: shapes do not match the geometry")
    lib = _lib.load()
    nbytes = lib.ssd_conv3x3_wino_wgrad_workspace(C.byref(g), ldy, mo)
    if nbytes == 0:
        raise ValueError("conv2d_wgrad_wino: not a 3x3 / stride 1 / pad 1 geometry")
    dev = planes.device if pooled else dy.device
    ws = workspace(nbytes, dev, "wino")
    dw = _grad_dst(dw_out, (g.Co, g.Ci, 3, 3), dev, "dw_out")
    db = _grad_dst(db_out, (g.Co,), dev, "db_out") if want_bias else None
    if dgrad_planes and planes is None:
        raise ValueError("conv2d_wgrad_wino: dgrad_planes needs the kept forward planes")
    pd = torch.empty((36, planes.shape[1], ldy), device=dev, dtype=torch.float32) if dgrad_planes else None
    suffix, src = _dy_source(dy, g, ldy)
    # one argument list: x or its kept planes, the gradient's source, the outputs, then mo (from x) or the dgrad planes (from planes)
    args = ((x if planes is None else planes).data_ptr(), *src, ldy, dw.data_ptr(), _ptr(db), C.byref(g), mo if planes is None else _ptr(pd),
            ws.data_ptr(), ws.numel(), _stream())
    entry = "ssd_conv3x3_wino_wgrad" + ("" if planes is None else "_planes" + suffix)
    check(getattr(lib, entry)(*args), "conv2d_wgrad_wino" + suffix)
    return (dw, db, pd) if dgrad_planes else (dw, db)


def wino_dy_transform(dy: torch.Tensor, g: ConvGeom, ldy: int, dgrad_planes: bool = True, want_bias: bool = True):
    """First half of the F(4x4) weight gradient on kept planes: one pass over dy -> (wgrad_planes (36, tiles, ldy),
    dgrad_planes (36, tiles, ldy) or None, bias_partial or None).  The data gradient only needs dgrad_planes."""
    pooled = isinstance(dy, PooledGrad)
    dev = dy.dpool.device if pooled else _req(dy, "dy").device
    tiles = wino_planes_shape(g)[1]
    if (not pooled and dy.numel() != g.N * g.H * g.W * ldy) or ldy % 4 != 0 or ldy < g.Co:
        raise ValueError("wino_dy_transform: shapes do not match the geometry")
    lib = _lib.load()
    Y = torch.empty((36, tiles, ldy), device=dev, dtype=torch.float32)
    Vd = torch.empty((36, tiles, ldy), device=dev, dtype=torch.float32) if dgrad_planes else None
    part = torch.empty((lib.ssd_wino4_bias_partial_floats(C.byref(g), ldy),), device=dev, dtype=torch.float32) if want_bias else None
    suffix, src = _dy_source(dy, g, ldy)
    check(getattr(lib, "ssd_wino4_dy_transform" + suffix)(*src, ldy, C.byref(g), Y.data_ptr(), _ptr(Vd), _ptr(part), _stream()),
          "wino_dy_transform" + suffix)
    return Y, Vd, part


def wino_adj_weights(w_oihw: torch.Tensor, co_pad: int) -> torch.Tensor:
    """Filter planes of the adjoint-form data gradient (`wino_dgrad_adj_gemm`): the forward transform G g G^T laid out (36, Ci, co_pad)
    -- limb planes where `wino_x3(4, co_pad)`."""
    _req(w_oihw, "w")
    co, ci = int(w_oihw.shape[0]), int(w_oihw.shape[1])
    u = wino_filter_alloc(4, ci, co_pad, w_oihw.device)
    check(_lib.load().ssd_wino_weights_adj(w_oihw.data_ptr(), u.data_ptr(), co, ci, co_pad, _stream()), "wino_weights_adj")
    return u


def wino_dgrad_adj_gemm(y_planes: torch.Tensor, u_adj: torch.Tensor, g: ConvGeom, ldy: int) -> torch.Tensor:
    """The 36 plane GEMMs of the adjoint-form data gradient: (36, tiles, ldy) planes A dy A^T (`wino_dy_transform`'s first result, the
    weight gradient's operand) x the adjoint filter planes -> md (36, tiles, Ci)."""
    _req(y_planes, "y_planes")
    tiles = wino_planes_shape(g)[1]
    if tuple(y_planes.shape) != (36, tiles, ldy) or g.Ci % 4 != 0 or ldy % 32 != 0:
        raise ValueError("wino_dgrad_adj_gemm: planes do not match the geometry")
    _wino_filter(u_adj, "u_adj", g.Ci, ldy)
    md = torch.empty((36, tiles, g.Ci), device=y_planes.device, dtype=torch.float32)
    check(_lib.load().ssd_conv3x3_wino_dgrad_adj_gemm(y_planes.data_ptr(), ldy, u_adj.data_ptr(), md.data_ptr(), C.byref(g), _stream()),
          "wino_dgrad_adj_gemm")
    return md


def _adj_mask_args(g: ConvGeom, tiles: int, relu_mask, bits):
    if bits is not None:
        _req(bits, "bits", torch.int64)
        if tuple(bits.shape) != (tiles, g.Ci // 4):
            raise ValueError("adjoint output: one mask word per (tile, channel quad)")
    if relu_mask is not None:
        _req(relu_mask, "relu_mask")
        if relu_mask.numel() != g.N * g.H * g.W * g.Ci:
            raise ValueError("adjoint output: relu_mask must have dx's shape")


def wino_adj_output(md: torch.Tensor, g: ConvGeom, dx: Optional[torch.Tensor] = None, relu_mask: Optional[torch.Tensor] = None,
                    bits: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """dx (N,H,W,Ci) [+=] the overlap-added 6x6 patches B md B^T, then the ReLU mask (bit words of the forward's input transform, or an
    f32 tensor > 0)."""
    _req(md, "md")
    tiles = wino_planes_shape(g)[1]
    if tuple(md.shape) != (36, tiles, g.Ci):
        raise ValueError("wino_adj_output: planes do not match the geometry")
    _adj_mask_args(g, tiles, relu_mask, bits)
    if dx is None:
        if accumulate:
            raise ValueError("accumulate needs an existing dx")
        dx = torch.empty((g.N, g.H, g.W, g.Ci), device=md.device, dtype=torch.float32)
    _req(dx, "dx")
    if dx.numel() != g.N * g.H * g.W * g.Ci:
        raise ValueError("wino_adj_output: dx shape")
    check(_lib.load().ssd_wino4_adj_output(md.data_ptr(), dx.data_ptr(), _ptr(relu_mask) if bits is None else None, _ptr(bits), int(accumulate),
                                           C.byref(g), _stream()), "wino_adj_output")
    return dx


def wino_adj_output_to_planes(md: torch.Tensor, g: ConvGeom, g_below: ConvGeom, relu_mask: Optional[torch.Tensor] = None,
                              bits: Optional[torch.Tensor] = None, want_bias: bool = True):
    """The chained form: the masked dx block of layer `g` is the dy block of the layer below it -> (planes A dy A^T (36, tiles, g.Ci) of
    `g_below`, its bias partial sums or None), without the gradient tensor in between."""
    _req(md, "md")
    tiles = wino_planes_shape(g)[1]
    if tuple(md.shape) != (36, tiles, g.Ci) or g_below.Co != g.Ci or (g_below.N, g_below.H, g_below.W) != (g.N, g.H, g.W):
        raise ValueError("wino_adj_output_to_planes: the two layers do not chain")
    _adj_mask_args(g, tiles, relu_mask, bits)
    lib = _lib.load()
    Y = torch.empty((36, tiles, g.Ci), device=md.device, dtype=torch.float32)
    part = torch.empty((lib.ssd_wino4_bias_partial_floats(C.byref(g_below), g.Ci),), device=md.device, dtype=torch.float32) if want_bias else None
    check(lib.ssd_wino4_adj_output_to_planes(md.data_ptr(), _ptr(relu_mask) if bits is None else None, _ptr(bits), C.byref(g), C.byref(g_below),
                                             Y.data_ptr(), _ptr(part), _stream()), "wino_adj_output_to_planes")
    return Y, part


class AdjPlanesGrad:
    """A data gradient that exists only as the product planes `md` of the adjoint-form GEMMs of layer `g` (plus the ReLU mask of the
    tensor it is the gradient of): the layer below turns it into its own dy planes (`wino_adj_output_to_planes`) without the tensor
    being written; `materialize()` is the stand-alone output transform for any other reader."""

    def __init__(self, md: torch.Tensor, g: ConvGeom, relu_mask: Optional[torch.Tensor], bits: Optional[torch.Tensor]):
        self.md, self.g, self.relu_mask, self.bits = md, g, relu_mask, bits

    @property
    def shape(self):
        return (self.g.N, self.g.H, self.g.W, self.g.Ci)

    def materialize(self) -> torch.Tensor:
        return wino_adj_output(self.md, self.g, None, self.relu_mask, self.bits, False)


class PooledGrad:
    """A gradient that exists only as the gradient of the 2x2 / stride-2 max pool behind it: (dpool (N,Hp,Wp,C), argmax codes, pooled forward
    output = the ReLU gate).  `wino_dy_transform` / `conv2d_wgrad_wino` take it in place of dy; `materialize()` is the scatter to memory."""

    def __init__(self, dpool: torch.Tensor, argmax: torch.Tensor, y_pooled: torch.Tensor, in_shape):
        _req(dpool, "dpool"); _req(y_pooled, "y_pooled"); _req(argmax, "argmax", torch.uint8)
        if tuple(dpool.shape) != tuple(y_pooled.shape) or tuple(argmax.shape) != tuple(dpool.shape) or dpool.shape[3] != in_shape[3]:
            raise ValueError("PooledGrad: dpool, argmax and the pooled output must have one shape, and the channels of the pool's input")
        self.dpool, self.argmax, self.y_pooled, self.in_shape = dpool, argmax, y_pooled, tuple(in_shape)

    def materialize(self, dx: Optional[torch.Tensor] = None) -> torch.Tensor:
        return maxpool_bwd(self.dpool, self.argmax, self.in_shape, 2, 2, 0, dx, y_gate=self.y_pooled)


def _dy_source(dy, g: ConvGeom, ldy: int):
    """The gradient a weight-gradient entry reads -> (suffix of the entry's name, its leading arguments): a tensor, or a `PooledGrad`
    for the `_pooled` entries."""
    if not isinstance(dy, PooledGrad):
        return "", (dy.data_ptr(),)
    if dy.in_shape != (g.N, g.H, g.W, g.Co) or ldy != g.Co:
        raise ValueError("pooled gradient does not match the geometry")
    return "_pooled", (dy.dpool.data_ptr(), dy.argmax.data_ptr(), dy.y_pooled.data_ptr(), dy.dpool.shape[1], dy.dpool.shape[2])


def wino_wgrad_gemm(wgrad_planes: torch.Tensor, x_planes: torch.Tensor, bias_partial: Optional[torch.Tensor], g: ConvGeom, ldy: int,
                    dw_out: Optional[torch.Tensor] = None, db_out: Optional[torch.Tensor] = None):
    """Second half: the TN GEMMs over the tiles, the inverse transform and the bias gradient -> (dw (Co,Ci,3,3), dbias or None).
    Runs on the CURRENT stream, which may differ from the one `wino_dy_transform` ran on (the caller orders them with an event)."""
    _req(wgrad_planes, "wgrad_planes"); _req(x_planes, "x_planes")
    tiles = wino_planes_shape(g)[1]
    if tuple(wgrad_planes.shape) != (36, tiles, ldy) or tuple(x_planes.shape) != (36, tiles, g.Ci):
        raise ValueError("wino_wgrad_gemm: planes do not match the geometry")
    lib = _lib.load()
    dev = x_planes.device
    ws = workspace(lib.ssd_wino4_wgrad_gemm_workspace(C.byref(g), ldy), dev, "wino_wgrad")
    dw = _grad_dst(dw_out, (g.Co, g.Ci, 3, 3), dev, "dw_out")
    db = _grad_dst(db_out, (g.Co,), dev, "db_out") if bias_partial is not None else None
    check(lib.ssd_wino4_wgrad_gemm(wgrad_planes.data_ptr(), x_planes.data_ptr(), ldy, _ptr(bias_partial), dw.data_ptr(), _ptr(db), C.byref(g),
                                   ws.data_ptr(), ws.numel(), _stream()), "wino_wgrad_gemm")
    return dw, db


class WeightTable:
    """Job table of `ssd_weights_prepare`: every filter transform / re-layout of a training step in one launch.  `jobs` is a list of
    dicts(kind, w0, w1 or None, co0, co, ci, taps, co_pad, out_fwd, out_bwd or None) holding tensors; the table keeps them alive and is
    valid while their storage does not move."""

    def __init__(self, jobs, device):
        import numpy as np
        lib = _lib.load()
        arr = (_lib.WeightJob * len(jobs))()
        starts, total = [], 0
        self.keep = []
        for a, j in zip(arr, jobs):
            for t in (j["w0"], j.get("w1"), j.get("out_fwd"), j.get("out_bwd")):
                if t is not None:
                    _req(t, "weight job tensor", t.dtype if (j["kind"] in (0, 3, 4) and t.dtype == torch.bfloat16) else torch.float32)
                    self.keep.append(t)
            a.w0 = j["w0"].data_ptr()
            a.w1 = j["w1"].data_ptr() if j.get("w1") is not None else j["w0"].data_ptr()
            a.out_fwd = _ptr(j.get("out_fwd"))
            a.out_bwd = _ptr(j.get("out_bwd"))
            a.co0, a.co, a.ci, a.taps, a.co_pad, a.kind = j["co0"], j["co"], j["ci"], j["taps"], j["co_pad"], j["kind"]
            a.pad1 = j.get("pad1", 0)
            if j["kind"] == 0:                 # Winograd filters: which outputs are limb tensors (wino_filter_alloc); bit 2: out_bwd in the adjoint form
                a.pad0 = sum(bit for bit, key in ((1, "out_fwd"), (2, "out_bwd")) if j.get(key) is not None and j[key].dtype == torch.bfloat16)
                if j.get("adj"):
                    a.pad0 |= 4
            nb = lib.ssd_weight_job_blocks(C.byref(a))
            if nb <= 0:
                raise ValueError("bad weight job")
            starts.append(total)
            total += nb
        self.njobs, self.total_blocks = len(jobs), total
        self.jobs_dev = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(device)
        self.starts_dev = torch.tensor(starts, dtype=torch.int32).to(device)

    def run(self) -> None:
        check(_lib.load().ssd_weights_prepare(self.jobs_dev.data_ptr(), self.starts_dev.data_ptr(), self.njobs, self.total_blocks, _stream()),
              "weights_prepare")

"""Exact integer-data tests of the direct convolution kernels: every entry point, the dispatch edges, every bench geometry.

The norm-wise checks of test_gpu_kernels.py (max error <= 1e-4 of max|ref|) cannot see an error confined to a few elements that are
small against the tensor's largest one: one dropped position in the last split of a weight gradient, one tap missing at the border of
the last ragged tile, the last iteration of a persistent kernel.  Here inputs, weights and gradients are small integers, bounded so
that for every output the sum of |terms| is below 2^24 (asserted from each case's own data).  Then every product and every partial
sum is exact in f32, and bf16 operands are exact too (|v| <= 256), in any summation order: split-K partition, tile, MFMA shape and
limb split (hi = v, mid = lo = 0) do not matter.  The correct output is one number, and every kernel is compared with `torch.equal`
against a convolution of the same data (f64, or f32 im2col + GEMM under the same precondition, cross-checked against f64 once).
bf16 outputs are that exact value rounded once to nearest even.  Outputs go into buffers prefilled with a sentinel: padding columns
and a tail past the tensor must come back bit-unchanged.
"""
import ctypes as C
import time

import pytest
import torch
import torch.nn.functional as F

from conv_geometries import bench_geometries, bf16_plan, halo_shape

pytestmark = pytest.mark.gpu

EXACT = 1 << 24
SENT = -1.0e30           # sentinel of every output canvas (finite: a NaN would compare unequal to itself)
TAIL = 1024              # elements of canvas past the end of each tensor


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator(device=_dev()).manual_seed(seed)


def _ints(shape, amp, gen, zero=0.3):
    """integers in [-amp, amp] (f32), a share `zero` of them forced to 0"""
    v = torch.randint(-amp, amp + 1, shape, generator=gen, device=gen.device, dtype=torch.int32).float()
    if zero:
        v[torch.rand(shape, generator=gen, device=gen.device) < zero] = 0
    return v


def _canvas(shape, dtype=torch.float32, fill=None):
    """(view of the tensor, the whole buffer): a tensor of `shape` at the start of a buffer with TAIL more elements, all SENT (or the
    tensor part = `fill`)"""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + TAIL,), SENT, dtype=dtype, device=_dev())
    view = buf[:n].view(shape)
    if fill is not None:
        view.copy_(fill)
    return view, buf


def _tail_ok(buf, n, what):
    t = buf[n:]
    assert bool((t == torch.tensor(SENT, dtype=buf.dtype, device=buf.device)).all()), f"{what}: wrote past the end of its tensor"


def _eq(got, want, what):
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    if torch.equal(got, want):
        return
    bad = (got != want) & ~(torch.isnan(got) & torch.isnan(want))
    nbad = int(bad.sum())
    idx = tuple(int(i) for i in bad.nonzero()[0])
    diff = float((got.double() - want.double()).abs().max())
    raise AssertionError(f"{what}: {nbad} of {got.numel()} elements differ; first at {idx}: got {float(got[idx])}, "
                         f"want {float(want[idx])}; max |diff| {diff:g}")


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def _bound(terms, a, b, extra=0.0):
    """exactness precondition: a sum of `terms` products of factors bounded by a and b, plus `extra`, stays below 2^24"""
    s = float(terms) * a * b + extra
    assert s < EXACT, f"exactness precondition: sum of |terms| may reach {s:g} >= 2^24"


def _ref(x, w, b, dy, s, p, d, dtype=torch.float64):
    """y = conv(x, w) + b, dx, dw, db of one convolution (NCHW, on the device).  f64 is exact for these data whatever the order; f32
    (im2col + GEMM, MIOpen off so no Winograd or FFT algorithm) is exact under the 2^24 precondition (test_reference_is_exact)."""
    with torch.backends.cudnn.flags(enabled=False):
        prev = torch.backends.cuda.matmul.allow_tf32
        torch.backends.cuda.matmul.allow_tf32 = False
        try:
            xx, ww = x.to(dtype), w.to(dtype)
            y = F.conv2d(xx, ww, None if b is None else b.to(dtype), stride=s, padding=p, dilation=d)
            dx = dw = db = None
            if dy is not None:
                dx, dw, db = torch.ops.aten.convolution_backward(dy.to(dtype), xx, ww, [w.shape[0]], [s, s], [p, p], [d, d], False, [0, 0], 1,
                                                                 [True, True, True])
        finally:
            torch.backends.cuda.matmul.allow_tf32 = prev
    f = lambda t: None if t is None else t.float()                 # noqa: E731  (integers below 2^24: exact in f32)
    return f(y), f(dx), f(dw), f(db)


class Case:
    """One convolution with integer data and its exact results (NHWC copies for the kernels)."""

    def __init__(self, geo, seed, amp=None, zero=0.3, ref_dtype=torch.float64):
        from objectdetection_ssd_amd import ops
        n, h, w, ci, co, k, s, p, d = geo
        self.geo, self.n, self.h, self.w, self.ci, self.co, self.k, self.s, self.p, self.d = geo, n, h, w, ci, co, k, s, p, d
        self.g = ops.make_geom(n, h, w, ci, co, k, s, p, d)
        ho, wo = self.g.Ho, self.g.Wo
        m = n * ho * wo
        # amplitudes: x and dy so that the weight gradient's M products stay exact, w so that forward and data gradient do
        axd = max(1, min(8, int((EXACT / 4 / m) ** 0.5)))
        aw = max(1, min(8, int(EXACT / 4 / (max(ci, co) * k * k * axd))))
        if amp is not None:
            axd, aw = amp
        gen = _gen(seed)
        self.x = _ints((n, ci, h, w), axd, gen, zero)
        self.wt = _ints((co, ci, k, k), aw, gen, zero)
        self.b = _ints((co,), 64, gen, 0.1)
        self.dy = _ints((n, co, ho, wo), axd, gen, zero)
        ax, ady, awt = _amax(self.x), _amax(self.dy), _amax(self.wt)
        _bound(ci * k * k, ax, awt, 64 + 64)                    # forward (+ bias, + a residual of |v| <= 64)
        _bound(co * k * k, ady, awt, 64)                         # data gradient (+ an accumulated |v| <= 64)
        _bound(m, ax, ady)                                       # weight gradient
        _bound(m, ady, 1.0)                                      # bias gradient
        assert max(ax, ady, awt) <= 256                          # bf16 operands are exact
        y, dx, dw, db = _ref(self.x, self.wt, None, self.dy, s, p, d, ref_dtype)
        self.y, self.dx, self.dw, self.db = _nhwc(y), _nhwc(dx), dw, db
        self.x_nhwc = _nhwc(self.x)
        self.co_pad = ops.pad32(co)
        dyp = torch.zeros((n, ho, wo, self.co_pad), device=self.x.device)
        dyp[..., :co] = _nhwc(self.dy)
        self.dy_pad = dyp
        self.res = _ints(tuple(self.y.shape), 64, gen, 0.2)     # residual / accumulated dx
        self.prev = _ints(tuple(self.dx.shape), 64, gen, 0.2)
        self.mask = _ints(tuple(self.dx.shape), 2, gen, 0.0)    # ReLU mask: > 0 passes

    @property
    def is3x3s1(self):
        return (self.k, self.s, self.p, self.d) == (3, 1, 1, 1)

    @property
    def numel_y(self):
        return self.y.numel()


# ---- the f32, bf16-operand and f32x3 entry points on one case ----------------------------------------------------------------------
def _fwd(c, what, relu=True, **kw):
    """conv2d_fwd into a canvas of ld = co_pad + 32 columns: columns >= Co and the tail stay SENT"""
    from objectdetection_ssd_amd import ops
    ld = c.co_pad + 32
    out, buf = _canvas((c.n, c.g.Ho, c.g.Wo, ld))
    wf = kw.pop("wf")
    ops.conv2d_fwd(c.x_nhwc, wf, c.b, c.g, relu, ld=ld, out=out, **kw)
    want = c.y + c.b
    _eq(out[..., :c.co], want.relu() if relu else want, what)
    assert bool((out[..., c.co:] == SENT).all()), f"{what}: wrote into the ld padding"
    _tail_ok(buf, out.numel(), what)


def _fwd_accumulate(c, wf, what, bf16=False):
    from objectdetection_ssd_amd import ops
    with pytest.raises(ValueError, match="accumulate needs an existing out"):      # not onto fresh, uninitialised memory
        ops.conv2d_fwd(c.x_nhwc, wf, c.b, c.g, True, bf16=bf16, accumulate=True)
    out, buf = _canvas(tuple(c.y.shape), fill=c.res)
    ops.conv2d_fwd(c.x_nhwc, wf, c.b, c.g, True, out=out, bf16=bf16, accumulate=True)
    _eq(out, (c.res + c.y + c.b).relu(), what)
    _tail_ok(buf, out.numel(), what)


def _dgrad(c, wb, what, **kw):
    """plain data gradient, then += an existing dx under a ReLU mask, both into canvases"""
    from objectdetection_ssd_amd import ops
    dx, buf = _canvas(tuple(c.dx.shape))
    ops.conv2d_dgrad(c.dy_pad, wb, c.g, dx=dx, **kw)
    _eq(dx, c.dx, what)
    _tail_ok(buf, dx.numel(), what)
    dx, buf = _canvas(tuple(c.dx.shape), fill=c.prev)
    ops.conv2d_dgrad(c.dy_pad, wb, c.g, dx=dx, relu_mask=c.mask, accumulate=True, **kw)
    _eq(dx, (c.prev + c.dx) * (c.mask > 0), what + " (accumulate + mask)")
    _tail_ok(buf, dx.numel(), what + " (accumulate + mask)")


def _wgrad(c, what, bf16=False):
    from objectdetection_ssd_amd import ops
    dw, bw = _canvas(tuple(c.dw.shape))
    db, bb = _canvas((c.co,))
    ops.conv2d_wgrad(c.x_nhwc, c.dy_pad, c.g, c.co_pad, True, bf16=bf16, dw_out=dw, db_out=db)
    _eq(dw, c.dw, what)
    _eq(db, c.db, what + " bias")
    _tail_ok(bw, dw.numel(), what)
    _tail_ok(bb, db.numel(), what + " bias")


def _run_f32_direct(c, lib, sweep):
    """f32 igemm forward / data gradient and the weight-gradient kernels; `sweep`: every tile, stage count, split-K form, wgrad tile,
    stage count, split target and patch shape forced in turn (the dispatcher's own choice always runs too)"""
    from objectdetection_ssd_amd import ops
    wf = ops.weight_ohwi(c.wt, c.co_pad)
    wb = ops.weight_ihwo(c.wt, c.co_pad)
    tag = f"{c.geo}"
    _fwd(c, f"f32 fwd relu {tag}", wf=wf)
    _fwd(c, f"f32 fwd {tag}", relu=False, wf=wf)
    _fwd_accumulate(c, wf, f"f32 fwd accumulate {tag}")
    _dgrad(c, wb, f"f32 dgrad {tag}")
    _wgrad(c, f"f32 wgrad {tag}")
    if not sweep:
        return
    try:
        for tile in range(4):
            for nbuf in (1, 2):
                assert lib.ssd_tune_set_igemm(tile, nbuf) == 0
                _fwd(c, f"f32 fwd tile {tile} nbuf {nbuf} {tag}", wf=wf)
                _dgrad(c, wb, f"f32 dgrad tile {tile} nbuf {nbuf} {tag}")
        lib.ssd_tune_set_igemm(-1, -1)
        for ks in (1, 2, 3, 7):
            assert lib.ssd_tune_set_igemm_splitk(ks) == 0
            _fwd(c, f"f32 fwd split-K {ks} {tag}", wf=wf)
            _dgrad(c, wb, f"f32 dgrad split-K {ks} {tag}")
        lib.ssd_tune_set_igemm_splitk(-1)
        for bt, nbuf in ((3, 1), (64, 1), (64, 2), (128, 1), (128, 2)):
            for bpc in (-1, 1, 40):
                lib.ssd_tune_set_wgrad(bt, nbuf, bpc)
                _wgrad(c, f"f32 wgrad bt {bt} nbuf {nbuf} bpc {bpc} {tag}")
        lib.ssd_tune_set_wgrad(-1, -1, -1)
        if c.is3x3s1:
            lib.ssd_tune_set_wgrad(3, 1, -1)
            for shape in (0, 1, 2):
                assert lib.ssd_tune_set_wgrad_patch(shape) == 0
                _wgrad(c, f"f32 fused wgrad patch shape {shape} {tag}")
    finally:
        lib.ssd_tune_set_igemm(-1, -1)
        lib.ssd_tune_set_igemm_splitk(-1)
        lib.ssd_tune_set_wgrad(-1, -1, -1)
        lib.ssd_tune_set_wgrad_patch(-1)


def _run_bf16_operand(c, lib, sweep):
    """bf16-operand igemm (every tile), the halo kernel via w3 (both patch shapes), accumulate, the bf16 weight gradient"""
    from objectdetection_ssd_amd import ops
    wf = ops.weight_ohwi(c.wt, c.co_pad)
    wb = ops.weight_ihwo(c.wt, c.co_pad)
    tag = f"{c.geo}"
    try:
        for tile in ((-1, 0, 1, 2, 3) if sweep else (-1,)):
            assert lib.ssd_tune_set_igemm_bf16(tile) == 0
            assert lib.ssd_tune_set_halo(0 if sweep else -1) == 0
            _fwd(c, f"bf16-operand fwd tile {tile} {tag}", wf=wf, bf16=True)
            _dgrad(c, wb, f"bf16-operand dgrad tile {tile} {tag}", bf16=True)
        lib.ssd_tune_set_igemm_bf16(-1)
        if c.is3x3s1:
            wf3, wb3 = ops.weight_split3(wf), ops.weight_split3(wb)
            for halo in ((-1, 1, 2) if sweep else (-1,)):
                assert lib.ssd_tune_set_halo(halo) == 0
                _fwd(c, f"bf16 halo fwd {halo} {tag}", wf=wf, bf16=True, w3=wf3)
                _dgrad(c, wb, f"bf16 halo dgrad {halo} {tag}", bf16=True, w3=wb3)
        lib.ssd_tune_set_halo(-1)
        _fwd_accumulate(c, ops.weight_ohwi(c.wt), f"bf16-operand fwd accumulate {tag}", bf16=True)
        _wgrad(c, f"bf16-operand wgrad {tag}", bf16=True)
    finally:
        lib.ssd_tune_set_igemm_bf16(-1)
        lib.ssd_tune_set_halo(-1)


def _run_x3(c, lib, sweep):
    """three-limb kernels: conv2d_fwd_x3 / conv2d_dgrad_x3 (every igemm_x3 tile with the halo kernel off, then both halo shapes),
    conv1x1_{fwd,dgrad,wgrad}_x3; every output into a canvas"""
    from objectdetection_ssd_amd import _lib, ops
    tag = f"{c.geo}"
    w3f = ops.weight_split3(ops.weight_ohwi(c.wt, c.co_pad))
    w3b = ops.weight_split3(ops.weight_ihwo(c.wt, c.co_pad))
    assert bool((w3f[1:] == 0).all()) and bool((w3b[1:] == 0).all())      # integers: hi = v, mid = lo = 0

    def run(t):
        ld = c.co_pad + 32
        y, buf = _canvas((c.n, c.g.Ho, c.g.Wo, ld))
        _lib.check(lib.ssd_conv2d_fwd_x3(c.x_nhwc.data_ptr(), w3f.data_ptr(), int(w3f.shape[1]), c.b.data_ptr(), y.data_ptr(), ld,
                                         C.byref(c.g), 1, ops._stream()), "conv2d_fwd_x3")
        _eq(y[..., :c.co], (c.y + c.b).relu(), "x3 fwd " + t)
        assert bool((y[..., c.co:] == SENT).all()), f"x3 fwd {t}: wrote into the ld padding"
        _tail_ok(buf, y.numel(), "x3 fwd " + t)
        dx, buf = _canvas(tuple(c.dx.shape), fill=c.prev)
        ops.conv2d_dgrad_x3(c.dy_pad, w3b, c.g, dx=dx, relu_mask=c.mask, accumulate=True)
        _eq(dx, (c.prev + c.dx) * (c.mask > 0), "x3 dgrad accumulate + mask " + t)
        _tail_ok(buf, dx.numel(), "x3 dgrad accumulate + mask " + t)
        dx, buf = _canvas(tuple(c.dx.shape))
        ops.conv2d_dgrad_x3(c.dy_pad, w3b, c.g, dx=dx)
        _eq(dx, c.dx, "x3 dgrad " + t)
        _tail_ok(buf, dx.numel(), "x3 dgrad " + t)

    try:
        if not sweep:
            run(tag)
        else:
            assert lib.ssd_tune_set_halo(0) == 0
            for tile in (-1, 1, 2, 3):
                assert lib.ssd_tune_set_igemm_x3(tile) == 0
                run(f"tile {tile} {tag}")
            lib.ssd_tune_set_igemm_x3(-1)
            if c.is3x3s1:
                for halo in (1, 2):
                    assert lib.ssd_tune_set_halo(halo) == 0
                    assert halo_shape(c.geo, 0, 3) == halo and halo_shape(c.geo, 1, 3) == halo
                    run(f"halo {halo} {tag}")
    finally:
        lib.ssd_tune_set_igemm_x3(-1)
        lib.ssd_tune_set_halo(-1)
    if c.k == 1 and c.s == 1 and c.p == 0 and c.ci % 32 == 0:
        wf, wbt = ops.conv1x1_weights_x3(c.wt, c.co_pad)
        y, buf = _canvas(tuple(c.y.shape))
        _lib.check(lib.ssd_conv1x1_fwd_x3(c.x_nhwc.data_ptr(), wf.data_ptr(), c.b.data_ptr(), y.data_ptr(), c.co, C.byref(c.g), 1,
                                          ops._stream()), "conv1x1_fwd_x3")
        _eq(y, (c.y + c.b).relu(), f"conv1x1_fwd_x3 {tag}")
        _tail_ok(buf, y.numel(), f"conv1x1_fwd_x3 {tag}")
        dx, buf = _canvas(tuple(c.dx.shape), fill=c.prev)
        ops.conv1x1_dgrad_x3(c.dy_pad, wbt, c.g, dx=dx, relu_mask=c.mask, accumulate=True)
        _eq(dx, (c.prev + c.dx) * (c.mask > 0), f"conv1x1_dgrad_x3 {tag}")
        _tail_ok(buf, dx.numel(), f"conv1x1_dgrad_x3 {tag}")
        dw, bw = _canvas(tuple(c.dw.shape))
        db, bb = _canvas((c.co,))
        ops.conv1x1_wgrad_x3(c.x_nhwc, c.dy_pad, c.g, c.co_pad, True, dw_out=dw, db_out=db)
        _eq(dw, c.dw, f"conv1x1_wgrad_x3 {tag}")
        _eq(db, c.db, f"conv1x1_wgrad_x3 bias {tag}")
        _tail_ok(bw, dw.numel(), f"conv1x1_wgrad_x3 {tag}")
        _tail_ok(bb, db.numel(), f"conv1x1_wgrad_x3 bias {tag}")


# ---- the bf16-tensor kernels ------------------------------------------------------------------------------------------------------
BF16_FORCED = [(-1, -1), (0, 64), (0, 128), (1, 64), (1, 128), (2, 64), (2, 128)]


def _run_conv3x3_bf16(c, lib, forced, mfma=(32,), k64=(1,), n_out=None, f32_out=True):
    """conv3x3_bf16 (csrc/conv_bf16.hip) on bf16 tensors: forward (bias + ReLU, bf16 out, wider ldo), forward with f32 out (the heads),
    flipped-tap data gradient (+= an existing bf16 dx under a bf16 ReLU mask).  Weights (rows = Co, 9, K = Ci) / (Ci, 9, pad64(Co))."""
    from objectdetection_ssd_amd import ops
    assert c.is3x3s1 and c.ci % 64 == 0
    tag = f"{c.geo}"
    n_out = c.co if n_out is None else n_out
    assert n_out % 4 == 0 and n_out >= c.co
    wf16 = c.wt.permute(0, 2, 3, 1).reshape(c.co, 9, c.ci).contiguous().bfloat16()
    kb = ops.pad64(c.co)
    wb16 = torch.zeros((c.ci, 9, kb), device=c.x.device, dtype=torch.bfloat16)
    wb16[:, :, :c.co] = c.wt.permute(1, 2, 3, 0).reshape(c.ci, 9, c.co)
    x16 = c.x_nhwc.bfloat16()
    dy16 = torch.zeros((c.n, c.h, c.w, kb), device=c.x.device, dtype=torch.bfloat16)
    dy16[..., :c.co] = _nhwc(c.dy)
    want = torch.zeros(tuple(c.y.shape[:3]) + (n_out,), device=c.x.device)
    want[..., :c.co] = c.y + c.b                                   # columns co .. n_out - 1: no weight row, no bias -> 0
    prev16, mask16 = c.prev.bfloat16(), c.mask.bfloat16()
    assert torch.equal(prev16.float(), c.prev) and torch.equal(mask16.float(), c.mask)
    dwant = ((c.prev + c.dx) * (c.mask > 0)).bfloat16()
    try:
        for m in mfma:
            assert lib.ssd_tune_set_conv_bf16_mfma(m) == 0
            for on in k64:
                lib.ssd_tune_set_conv_bf16_k64(on)
                for mode, bn in forced:
                    assert lib.ssd_tune_set_conv_bf16(mode, bn) == 0
                    t = f"mode {mode} bn {bn} mfma {m} k64 {on} {tag}"
                    ldo = n_out + 32
                    out, buf = _canvas((c.n, c.h, c.w, ldo), torch.bfloat16)
                    ops.conv3x3_bf16(x16, wf16, c.b, n_out, True, out=out, ldo=ldo)
                    _eq(out[..., :n_out], want.relu().bfloat16(), "conv3x3_bf16 fwd " + t)
                    assert bool((out[..., n_out:] == SENT).all()), f"conv3x3_bf16 fwd {t}: wrote into the ldo padding"
                    _tail_ok(buf, out.numel(), "conv3x3_bf16 fwd " + t)
                    if f32_out:
                        ld = ops.pad32(n_out)
                        out, buf = _canvas((c.n, c.h, c.w, ld))
                        ops.conv3x3_bf16(x16, wf16, c.b, n_out, False, out=out, out_f32=True, ldo=ld)
                        _eq(out[..., :n_out], want, "conv3x3_bf16 fwd f32 out " + t)
                        assert bool((out[..., n_out:] == SENT).all()), f"conv3x3_bf16 fwd f32 out {t}: wrote into the padding"
                        _tail_ok(buf, out.numel(), "conv3x3_bf16 fwd f32 out " + t)
                    dx, buf = _canvas(tuple(c.dx.shape), torch.bfloat16, fill=prev16)
                    ops.conv3x3_bf16(dy16, wb16, None, c.ci, False, flip=True, out=dx, relu_mask=mask16, accumulate=True)
                    _eq(dx, dwant, "conv3x3_bf16 flip dgrad (accumulate + mask) " + t)
                    _tail_ok(buf, dx.numel(), "conv3x3_bf16 flip dgrad " + t)
                    if f32_out:                        # f32 dx, as the head that is the only reader of an f32 tensor takes it
                        dx, buf = _canvas(tuple(c.dx.shape))
                        ops.conv3x3_bf16(dy16, wb16, None, c.ci, False, flip=True, out=dx, out_f32=True)
                        _eq(dx, c.dx, "conv3x3_bf16 flip dgrad f32 out " + t)
                        _tail_ok(buf, dx.numel(), "conv3x3_bf16 flip dgrad f32 out " + t)
                        dx, buf = _canvas(tuple(c.dx.shape), fill=c.prev)
                        ops.conv3x3_bf16(dy16, wb16, None, c.ci, False, flip=True, out=dx, out_f32=True, accumulate=True)
                        _eq(dx, c.prev + c.dx, "conv3x3_bf16 flip dgrad f32 out accumulate " + t)
                        _tail_ok(buf, dx.numel(), "conv3x3_bf16 flip dgrad f32 out accumulate " + t)
    finally:
        lib.ssd_tune_set_conv_bf16(-1, -1)
        lib.ssd_tune_set_conv_bf16_mfma(32)
        lib.ssd_tune_set_conv_bf16_k64(1)


def _run_wgrad_bf16t(c, lib, bpcs=(-1,), ldy=None):
    """ssd_conv3x3_wgrad_bf16t: the bf16-tensor instantiations of the patch weight-gradient kernel (3x3, dilation 4, 1x1) straight
    through the C ABI (the ops wrapper allocates 3x3 filters), into canvases.  ldy: row length of dy (default pad32(Co); the engine's
    heads pass pad64(Co)), columns Co .. ldy - 1 zero."""
    from objectdetection_ssd_amd import _lib, ops
    tag = f"{c.geo}"
    x16 = c.x_nhwc.bfloat16()
    ldy = c.co_pad if ldy is None else ldy
    dy16 = torch.zeros((c.n, c.g.Ho, c.g.Wo, ldy), device=c.x.device, dtype=torch.bfloat16)
    dy16[..., :c.co] = _nhwc(c.dy)
    try:
        for bpc in bpcs:
            lib.ssd_tune_set_wgrad(-1, -1, bpc)
            ws = ops.workspace(lib.ssd_conv2d_wgrad_workspace(C.byref(c.g)), c.x.device)      # (the split count follows bpc)
            dw, bw = _canvas(tuple(c.dw.shape))
            db, bb = _canvas((c.co,))
            _lib.check(lib.ssd_conv3x3_wgrad_bf16t(x16.data_ptr(), dy16.data_ptr(), ldy, dw.data_ptr(), db.data_ptr(), C.byref(c.g),
                                                   ws.data_ptr(), ws.numel(), ops._stream()), "conv3x3_wgrad_bf16t")
            _eq(dw, c.dw, f"wgrad bf16 tensors bpc {bpc} {tag}")
            _eq(db, c.db, f"wgrad bf16 tensors bias bpc {bpc} {tag}")
            _tail_ok(bw, dw.numel(), f"wgrad bf16 tensors {tag}")
            _tail_ok(bb, db.numel(), f"wgrad bf16 tensors bias {tag}")
            _wgrad(c, f"bf16-operand wgrad bpc {bpc} {tag}", bf16=True)
    finally:
        lib.ssd_tune_set_wgrad(-1, -1, -1)


def _bf16_patch_wgrad(c):
    return c.s == 1 and c.k in (1, 3) and ((c.k == 3 and c.p == c.d and c.d in (1, 4)) or (c.k == 1 and c.p == 0))


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def test_reference_is_exact():
    """the f32 reference (im2col + GEMM) equals f64 on data whose forward sums of |terms| may reach 9216 x 40 x 40 = 88 % of 2^24, and f64
    equals int64 arithmetic.  (The large f32-reference cases rest on the a-priori precondition each Case asserts, not on this check.)"""
    geo = (2, 12, 12, 1024, 64, 3, 1, 1, 1)
    c = Case(geo, seed=1, amp=(40, 40), zero=0.0)
    y, dx, dw, db = _ref(c.x, c.wt, None, c.dy, 1, 1, 1, torch.float32)
    _eq(_nhwc(y), c.y, "f32 reference forward")
    _eq(_nhwc(dx), c.dx, "f32 reference data gradient")
    _eq(dw, c.dw, "f32 reference weight gradient")
    _eq(db, c.db, "f32 reference bias gradient")
    # one output of each against integer arithmetic
    wi = c.wt.cpu().long()
    xp = F.pad(c.x.cpu(), (1, 1, 1, 1)).long()
    assert float(c.y[1, 4, 6, 17]) == float((xp[1, :, 4:7, 6:9] * wi[17]).sum())
    assert float(c.dw[5, 7, 0, 2]) == float(sum(int((xp[n, 7, 0:12, 2:14] * c.dy.cpu().long()[n, 5]).sum()) for n in range(2)))
    assert float(c.db[11]) == float(c.dy.cpu().long()[:, 11].sum())


# ---- dispatch edges ---------------------------------------------------------------------------------------------------------------
# n, h, w, ci, co, k, stride, pad, dil
EDGE_CASES = [
    (2, 19, 19, 64, 64, 3, 1, 1, 1),        # M = 722, ragged 64 x 64 tiles
    (1, 38, 38, 128, 256, 3, 1, 1, 1),
    (4, 64, 64, 64, 128, 3, 1, 1, 1),       # 128 x 128 tiles
    (2, 62, 62, 64, 64, 3, 1, 1, 1),        # bf16 flat space: W = 62 (<= 384 rows), Wo = 62
    (2, 63, 63, 64, 128, 3, 1, 1, 1),       # W = 63 (7 pieces), Wo = 63 / 64 halo edge
    (1, 30, 64, 64, 64, 3, 1, 1, 1),        # Ho = 30, Wo = 64: the halo kernels' lower edge (x3 and bf16)
    (1, 29, 64, 64, 64, 3, 1, 1, 1),        # Ho = 29: below it
    (2, 19, 19, 256, 100, 3, 1, 1, 1),      # head Co = 100
    (1, 19, 19, 256, 150, 3, 1, 1, 1),      # head Co = 150
    (1, 10, 10, 128, 340, 3, 1, 1, 1),      # head Co = 340 (81 classes)
    (1, 10, 10, 128, 510, 3, 1, 1, 1),      # head Co = 510
    (2, 10, 10, 128, 256, 3, 2, 1, 1),      # stride 2 -> 5 x 5
    (2, 19, 19, 256, 512, 3, 2, 1, 1),      # stride 2 -> 10 x 10
    (3, 5, 5, 128, 256, 3, 1, 0, 1),        # pad 0 -> 3 x 3
    (2, 3, 3, 128, 256, 3, 1, 0, 1),        # -> 1 x 1
    (2, 1, 1, 256, 128, 3, 1, 1, 1),        # 1 x 1 map, 3 x 3 filter
    (1, 3, 3, 256, 256, 3, 1, 1, 1),        # 3 x 3 map
    (1, 19, 19, 512, 160, 1, 1, 0, 1),      # 1 x 1 filter
    (1, 19, 19, 128, 256, 3, 1, 4, 4),      # dilation 4 (fc6)
    (1, 37, 53, 64, 96, 3, 1, 1, 1),        # odd map, Co = 96
]


@pytest.mark.parametrize("geo", EDGE_CASES)
def test_f32_and_bf16_operand_and_x3_kernels_exact(geo):
    from objectdetection_ssd_amd import _lib
    lib = _lib.load()
    c = Case(geo, seed=sum(geo))
    _run_f32_direct(c, lib, sweep=True)
    _run_bf16_operand(c, lib, sweep=True)
    _run_x3(c, lib, sweep=True)
    if _bf16_patch_wgrad(c):
        _run_wgrad_bf16t(c, lib)
    torch.cuda.synchronize()


# conv3x3_bf16: n, h, w, ci, co, and the automatic plan (position space, N tile, halo pieces, persistent); every forced position space /
# N tile, both MFMA shapes, k64 on and off
BF16T_CASES = [
    ((2, 62, 62, 64, 64), (2, 64, 6, 0)),        # flat_rows 384: the 6-piece flat form
    ((2, 63, 63, 64, 128), (2, 128, 7, 0)),      # 386: 7 pieces, 128-channel tiles
    ((1, 94, 94, 128, 128), (2, 128, 7, 0)),     # 448: the widest flat map
    ((1, 95, 95, 64, 64), (1, 64, 6, 0)),        # 450: patches
    ((1, 127, 128, 64, 64), (1, 64, 6, 0)),      # H = 127: 16 x 16 patches
    ((1, 128, 128, 64, 64), (0, 64, 6, 1)),      # H = W = 128: 8 x 32 patches, the persistent K = 64 kernel
    ((1, 128, 127, 64, 128), (1, 128, 6, 0)),    # W = 127
    ((1, 1, 1, 64, 64), (2, 64, 6, 0)),          # 1 x 1 map
    ((2, 3, 3, 128, 64), (2, 64, 6, 0)),         # 3 x 3 map
    ((3, 10, 10, 64, 128), (2, 64, 6, 0)),       # flat space over three images, 64-channel switch (few blocks)
    ((1, 19, 19, 512, 152), (2, 64, 6, 0)),      # a head's 152 stored columns (150 rows below)
]


@pytest.mark.parametrize("geo,plan", BF16T_CASES)
def test_conv3x3_on_bf16_tensors_exact(geo, plan):
    from objectdetection_ssd_amd import _lib
    lib = _lib.load()
    n, h, w, ci, co = geo
    assert bf16_plan(n, h, w, ci, co) == plan
    c = Case((n, h, w, ci, co, 3, 1, 1, 1), seed=7 * h + w)
    _run_conv3x3_bf16(c, lib, BF16_FORCED, mfma=(32, 16), k64=(1, 0))
    torch.cuda.synchronize()


HEAD_CASES = [(150, 152), (100, 100), (510, 512), (340, 340)]      # weight rows, stored columns


@pytest.mark.parametrize("co,n_out", HEAD_CASES)
def test_conv3x3_bf16_head_columns_exact(co, n_out):
    """heads: `co` weight rows and biases, n_out stored columns (a multiple of 4), f32 out of ld = pad32(n_out) as the engine runs them"""
    from objectdetection_ssd_amd import _lib
    c = Case((2, 19, 19, 256, co, 3, 1, 1, 1), seed=co)
    _run_conv3x3_bf16(c, _lib.load(), [(-1, -1), (2, 64), (2, 128), (1, 128)], n_out=n_out)
    _run_wgrad_bf16t(c, _lib.load(), ldy=(co + 63) // 64 * 64)          # dy rows of pad64(Co), as the heads' weight gradient reads them
    torch.cuda.synchronize()


# persistent K = 64 kernel: 8 x 32 patches over N images, one workgroup per CU (256): tile counts under, at and over multiples of 256
K64_CASES = [(1, 136, 480), (1, 128, 512), (1, 2050, 30), (1, 216, 600), (2, 8, 32), (3, 300, 300)]


@pytest.mark.parametrize("geo", K64_CASES)
def test_persistent_k64_kernel_tile_loop_exact(geo):
    from objectdetection_ssd_amd import _lib
    n, h, w = geo
    lib = _lib.load()
    tiles = n * -(-h // 8) * -(-w // 32)
    c = Case((n, h, w, 64, 64, 3, 1, 1, 1), seed=tiles)
    try:
        lib.ssd_tune_set_conv_bf16(0, 64)
        assert bf16_plan(n, h, w, 64, 64) == (0, 64, 6, 1)           # the persistent kernel
    finally:
        lib.ssd_tune_set_conv_bf16(-1, -1)
    _run_conv3x3_bf16(c, lib, [(0, 64)], mfma=(32, 16), k64=(1,), f32_out=False)
    torch.cuda.synchronize()


# the bf16 patch weight gradient (f32-operand and bf16-tensor instantiations): 3x3, dilation 4, 1x1; the split caps
WGRAD_BF16_CASES = [
    (2, 19, 19, 64, 64, 3, 1, 1, 1),        # few patches: nsplit = npatch / 4
    (8, 128, 128, 64, 64, 3, 1, 1, 1),      # 4096 patches: with bpc 40 both caps are 1024; tap-wise reduction
    (8, 136, 128, 64, 64, 3, 1, 1, 1),      # 4352 patches: bpc 40 stops at the 1024-split cap alone (871 splits of 5 patches)
    (1, 38, 38, 512, 512, 3, 1, 1, 1),      # many reduction blocks: the plain reduction
    (2, 75, 75, 128, 256, 3, 1, 1, 1),
    (1, 19, 19, 256, 150, 3, 1, 1, 1),      # ragged Co
    (2, 19, 19, 128, 256, 3, 1, 4, 4),      # dilation 4
    (2, 19, 19, 256, 512, 1, 1, 0, 1),      # 1 x 1: 128 consecutive pixels per patch
    (3, 10, 10, 128, 64, 1, 1, 0, 1),       # 1 x 1, M = 300 (ragged last patch)
    (1, 1, 1, 128, 64, 3, 1, 1, 1),         # one pixel
]


@pytest.mark.parametrize("geo", WGRAD_BF16_CASES)
def test_bf16_patch_weight_gradient_exact(geo):
    from objectdetection_ssd_amd import _lib
    c = Case(geo, seed=3 + sum(geo))
    _run_wgrad_bf16t(c, _lib.load(), bpcs=(-1, 1, 40))
    torch.cuda.synchronize()


# ---- conv1_1 and the stem ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 300, 300), (1, 37, 70), (3, 5, 5), (2, 4, 129), (32, 300, 300), (16, 512, 512)])
def test_conv1_1_kernels_exact(shape):
    """conv1_first_fwd (persistent, f32 out + its im2col rows), im2col_first + conv1_first_wgrad, and the bf16 forms; every output
    into a canvas"""
    from objectdetection_ssd_amd import _lib, ops
    lib = _lib.load()
    st = ops._stream()
    n, h, w = shape
    c = Case((n, h, w, 3, 64, 3, 1, 1, 1), seed=h + w, ref_dtype=torch.float32 if n * h * w > 10 ** 6 else torch.float64)
    rows = ops.first_weight_rows(c.wt)
    want = (c.y + c.b).relu()
    y, by = _canvas((n, h, w, 64))
    col, bc = _canvas((n, h, w, 32))
    _lib.check(lib.ssd_conv1_first_fwd(c.x.data_ptr(), rows.data_ptr(), c.b.data_ptr(), y.data_ptr(), col.data_ptr(), n, h, w, 1, st), "fwd")
    _eq(y, want, f"conv1_first_fwd {shape}")
    _tail_ok(by, y.numel(), f"conv1_first_fwd {shape}")
    _tail_ok(bc, col.numel(), f"conv1_first_fwd rows {shape}")
    col2, bc2 = _canvas((n, h, w, 32))
    _lib.check(lib.ssd_im2col_first(c.x.data_ptr(), col2.data_ptr(), n, h, w, st), "im2col_first")
    _tail_ok(bc2, col2.numel(), f"im2col_first {shape}")
    _eq(col, col2, f"conv1_first_fwd rows {shape}")
    xp = F.pad(c.x, (1, 1, 1, 1))                        # the rows: tap (r, s), channel c at (r * 3 + s) * 3 + c, five zero columns
    cols = torch.stack([xp[:, ch, r:r + h, s_:s_ + w] for r in range(3) for s_ in range(3) for ch in range(3)], -1)
    _eq(col2[..., :27], cols, f"im2col_first {shape}")
    assert bool((col2[..., 27:] == 0).all())
    y16, by16 = _canvas((n, h, w, 64), torch.bfloat16)
    _lib.check(lib.ssd_conv1_first_fwd_bf16(c.x.data_ptr(), rows.data_ptr(), c.b.data_ptr(), y16.data_ptr(), n, h, w, 1, st), "fwd bf16")
    _eq(y16, want.bfloat16(), f"conv1_first_fwd_bf16 {shape}")
    _tail_ok(by16, y16.numel(), f"conv1_first_fwd_bf16 {shape}")
    dy = _nhwc(c.dy)
    ws = ops.workspace(lib.ssd_conv1_first_wgrad_workspace(n, h, w), c.x.device, "first_wgrad")
    for fn, d, what in ((lib.ssd_conv1_first_wgrad, dy, "conv1_first_wgrad"), (lib.ssd_conv1_first_wgrad_bf16, dy.bfloat16(), "conv1_first_wgrad_bf16")):
        dw, bw = _canvas((64, 32, 1, 1))
        db, bb = _canvas((64,))
        _lib.check(fn(c.x.data_ptr(), d.data_ptr(), dw.data_ptr(), db.data_ptr(), n, h, w, ws.data_ptr(), ws.numel(), st), what)
        _eq(ops.first_weight_grad(dw), c.dw, f"{what} {shape}")
        assert bool((dw.reshape(64, 32)[:, 27:] == 0).all()), what
        _eq(db, c.db, f"{what} bias {shape}")
        _tail_ok(bw, dw.numel(), f"{what} {shape}")
        _tail_ok(bb, db.numel(), f"{what} bias {shape}")
    g = ops.make_geom(n, h, w, 32, 64, 1, 1, 0, 1)
    dw, bw = _canvas((64, 32, 1, 1))
    db, bb = _canvas((64,))
    ops.conv2d_wgrad(col2, dy, g, 64, True, dw_out=dw, db_out=db)
    _eq(ops.first_weight_grad(dw), c.dw, f"im2col_first + conv2d_wgrad {shape}")
    _eq(db, c.db, f"im2col_first + conv2d_wgrad bias {shape}")
    _tail_ok(bw, dw.numel(), f"im2col_first + conv2d_wgrad {shape}")
    _tail_ok(bb, db.numel(), f"im2col_first + conv2d_wgrad bias {shape}")
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(2, 224, 224, 7, 2, 3), (1, 37, 53, 7, 2, 3), (2, 30, 30, 3, 1, 1), (1, 16, 20, 5, 3, 0)])
def test_stem_im2col_and_conv_exact(shape):
    from objectdetection_ssd_amd import ops
    n, h, w, k, s, p = shape
    gen = _gen(k * h)
    x = _ints((n, 3, h, w), 8, gen)
    wt = _ints((64, 3, k, k), 8, gen)
    b = _ints((64,), 64, gen)
    _bound(3 * k * k, 8, 8, 64)
    y = _nhwc(_ref(x, wt, b, None, s, p, 1)[0]).relu()
    col = ops.im2col_nchw3(x, k, s, p)
    g = ops.make_geom(n, col.shape[1], col.shape[2], col.shape[3], 64, 1, 1, 0, 1)
    out, buf = _canvas((n, col.shape[1], col.shape[2], 64))
    ops.conv2d_fwd(col, ops.stem_weight_rows(wt), b, g, True, out=out)
    _eq(out, y, f"stem {shape}")
    _tail_ok(buf, out.numel(), f"stem {shape}")


# ---- every conv geometry a bench step launches ------------------------------------------------------------------------------------
BENCH_RUNS = [(300, 32), (512, 16)]


@pytest.mark.parametrize("variant,bs", BENCH_RUNS)
def test_every_bench_geometry_exact(variant, bs):
    """Each convolution of an SSD300 step at batch 32 / SSD512 at batch 16 (heads with 21 and 81 classes) through every direct entry
    point its modes run there: f32 igemm + weight gradient, bf16-operand igemm / halo / patch weight gradient, the three-limb kernels,
    the bf16-tensor convolution and weight gradient.  One reference per geometry serves all modes: the exact answer is the same."""
    from objectdetection_ssd_amd import _lib
    lib = _lib.load()
    t0 = time.time()
    for geo in bench_geometries(variant, bs, (21, 81)):
        c = Case(geo, seed=sum(geo), ref_dtype=torch.float32)
        _run_f32_direct(c, lib, sweep=False)
        _run_bf16_operand(c, lib, sweep=False)
        _run_x3(c, lib, sweep=False)
        head = c.co % 32 != 0                     # the fused loc + conf heads (a x (4 + classes) rows); every other layer has Co % 64 == 0
        if c.is3x3s1 and c.ci % 64 == 0:
            _run_conv3x3_bf16(c, lib, [(-1, -1)], n_out=(c.co + 3) // 4 * 4)
        if _bf16_patch_wgrad(c):
            _run_wgrad_bf16t(c, lib, ldy=(c.co + 63) // 64 * 64 if head else c.co)      # as the engine passes dy
        del c
        torch.cuda.synchronize()
    print(f"SSD{variant} batch {bs}: {time.time() - t0:.1f} s")

"""The kernels between the convolutions (csrc/elementwise.hip, csrc/elementwise_bf16.hip) bare, against the plain f64 references of
tests/elementwise_ref.py: max pool forward and every backward form, the conv4_3 L2 norm, the head scatter and gather, the f32 <-> bf16
casts and channel_affine -- f32 and bf16, at odd sizes, at sizes over each launch's block cap (the grid-stride loops), with ties, NaN
and +-inf.

Where a result is a selection (pooling, the heads, the casts) or the data make every summation order exact (integer pooling
gradients; L2-norm rows of four +-2^e channels, elementwise_ref.l2norm_exact_data), the kernel must return the one correct number:
`torch.equal`.  General-data L2-norm and channel_affine results are held per element to bounds that scale with the sum of the
absolute terms of that element, so a wrong row with a small norm cannot hide behind the tensor's maximum.  Outputs go into buffers
prefilled with a sentinel, through the C entry points: a tail past each tensor must come back unchanged.
"""
import pytest
import torch

import elementwise_ref as R

pytestmark = pytest.mark.gpu

SENT = -1.0e30           # sentinel of every float canvas (finite: a NaN would compare unequal to itself)
SENT_CODE = 0xEE         # ... and of the argmax canvases (a code is below 225)
TAIL = 1024              # elements of canvas past the end of each tensor
U = R.U
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
_ids = lambda d: "bf16" if d == BF16 else "f32"                                                  # noqa: E731


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _gen(seed):
    return torch.Generator(device=_dev()).manual_seed(seed)


def _lib():
    from objectdetection_ssd_amd import _lib as L, ops
    return L.load(), L.check, ops._stream()


class Canvas:
    """A tensor of `shape` at the start of a buffer with TAIL more elements, all the sentinel (or the tensor part = `fill`)."""

    def __init__(self, shape, dtype=F32, fill=None):
        self.n = 1
        for d in shape:
            self.n *= d
        self.sent = SENT_CODE if dtype == torch.uint8 else SENT
        self.buf = torch.full((self.n + TAIL,), self.sent, dtype=dtype, device=_dev())
        self.t = self.buf[:self.n].view(shape)
        if fill is not None:
            self.t.copy_(fill)

    def ptr(self):
        return self.buf.data_ptr()

    def done(self, what):
        tail = self.buf[self.n:]
        assert bool((tail == torch.tensor(self.sent, dtype=self.buf.dtype, device=self.buf.device)).all()), f"{what}: wrote past the end of its tensor"
        return self.t


def _eq(got, want, what):
    """equal element for element, NaN matching NaN"""
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    want = want.to(got.device)
    if torch.equal(got, want):
        return
    bad = ~R.nan_equal(got, want)
    nbad = int(bad.sum())
    if nbad == 0:
        return
    idx = tuple(int(i) for i in bad.nonzero()[0])
    raise AssertionError(f"{what}: {nbad} of {got.numel()} elements differ; first at {idx}: got {float(got[idx])}, want {float(want[idx])}")


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ---- max pooling ------------------------------------------------------------------------------------------------------------------
def _pool_fwd(x, k, s, p, ho, wo, want_argmax=True):
    """the C entry on an NHWC tensor of either dtype -> (y, argmax codes or None), tails checked"""
    lib, check, st = _lib()
    n, h, w, c = x.shape
    y = Canvas((n, ho, wo, c), x.dtype)
    am = Canvas((n, ho, wo, c), torch.uint8) if want_argmax else None
    fn = lib.ssd_maxpool_fwd_bf16 if x.dtype == BF16 else lib.ssd_maxpool_fwd
    check(fn(x.data_ptr(), y.ptr(), am.ptr() if am else None, n, h, w, c, k, s, p, ho, wo, st), "maxpool_fwd")
    return y.done("pool y"), (am.done("pool argmax") if am else None)


def _pool_bwd(dy, am, in_shape, k, s, p, prev=None, mask=None, gate=None):
    lib, check, st = _lib()
    n, h, w, c = in_shape
    _, ho, wo, _ = dy.shape
    dx = Canvas(in_shape, dy.dtype, fill=prev)
    mp, acc = (None if mask is None else mask.data_ptr()), int(prev is not None)
    if dy.dtype == BF16:
        check(lib.ssd_maxpool_bwd_bf16(dy.data_ptr(), am.data_ptr(), dx.ptr(), mp, None if gate is None else gate.data_ptr(), acc, n, h, w, c, k, s,
                                       p, ho, wo, st), "maxpool_bwd_bf16")
    elif gate is not None:
        assert mask is None and prev is None
        check(lib.ssd_maxpool_bwd_gated(dy.data_ptr(), am.data_ptr(), gate.data_ptr(), dx.ptr(), n, h, w, c, k, s, p, ho, wo, st), "maxpool_bwd_gated")
    else:
        check(lib.ssd_maxpool_bwd(dy.data_ptr(), am.data_ptr(), dx.ptr(), mp, acc, n, h, w, c, k, s, p, ho, wo, st), "maxpool_bwd")
    return dx.done("pool dx")


def _pool_forward_checks(x, k, s, p, ce, dtype, what):
    """x NCHW f32 on the device, its values bf16 values: the forward, with and without codes, against the scan -> (y, am, ref codes)"""
    ref_v, ref_c = R.pool_ref(x.double(), k, s, p, ce)
    ho, wo = ref_v.shape[-2:]
    xk = _nhwc(x).to(dtype)
    assert bool(R.nan_equal(xk.float(), _nhwc(x)).all())
    y, am = _pool_fwd(xk, k, s, p, ho, wo)
    _eq(y, _nhwc(ref_v).to(dtype), f"{what} values")
    _eq(am, _nhwc(ref_c).to(torch.uint8), f"{what} argmax codes")
    y2, _ = _pool_fwd(xk, k, s, p, ho, wo, want_argmax=False)
    _eq(y2, y, f"{what} values without codes")
    return xk, y, am, ref_v, ref_c


def _pool_backward_checks(x, dy, prev, xk, y, am, ref_v, ref_c, k, s, p, dtype, what, forms):
    shape = tuple(xk.shape)
    n, h, w, c = shape
    ho, wo = y.shape[1:3]
    dyk, prevk = _nhwc(dy).to(dtype), _nhwc(prev).to(dtype)
    want = lambda **kw: _nhwc(R.pool_bwd_ref(dy.double(), ref_c, x.shape, k, s, p, **kw)).to(dtype)          # noqa: E731
    if "plain" in forms:
        _eq(_pool_bwd(dyk, am, shape, k, s, p), want(), f"{what} backward, ties routed by the codes")
    if "mask" in forms:
        _eq(_pool_bwd(dyk, am, shape, k, s, p, mask=xk), want(mask=x), f"{what} backward + ReLU mask")
        _eq(_pool_bwd(dyk, am, shape, k, s, p, prev=prevk, mask=xk), want(prev=prev, mask=x), f"{what} backward + mask + accumulate")
        _eq(_pool_bwd(dyk, am, shape, k, s, p, prev=prevk), want(prev=prev), f"{what} backward + accumulate")
    if "gated" in forms:
        got = _pool_bwd(dyk, am, shape, k, s, p, gate=y)
        _eq(got, want(gate=ref_v), f"{what} backward gated by the pooled output")
        if (k, s, p) == (2, 2, 0) and 2 * ho < h:            # floor mode, odd side: the gather form, and no window reaches the last row
            assert float(got[:, h - 1].abs().max()) == 0.0
        if (k, s, p) == (2, 2, 0) and 2 * wo < w:
            assert float(got[:, :, w - 1].abs().max()) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("case", R.pool_cases(), ids=str)
def test_maxpool_forward_and_every_backward_form_are_exact(case, dtype):
    """Integer data full of ties (and a post-ReLU copy, where half of every window is tied at 0): values, codes and every gradient
    are one number.  Over the cases the gated backward takes the 2x2 scatter kernel (ceil mode or an even side) and the gather form
    (floor mode on an odd side)."""
    k, s, p, ce, h, w = case
    gen = _gen(100 + 7 * h + w + k)
    for n, c in ((1, 4), (3, 12), (1, 64), (3, 64)) if dtype == F32 else ((1, 8), (3, 24), (1, 64), (3, 64)):
        for relu in (False, True):
            x, dy, prev = R.pool_int_data(n, c, h, w, k, s, p, ce, gen, relu)
            what = f"pool {case} N={n} C={c} relu={relu}"
            fw = _pool_forward_checks(x, k, s, p, ce, dtype, what)
            _pool_backward_checks(x, dy, prev, *fw, k, s, p, dtype, what, ("plain", "mask", "gated"))


def test_the_pool_cases_take_both_gated_kernels():
    from objectdetection_ssd_amd.ops import pool_out
    scatter = [(c, 2 * pool_out(c[4], 2, 2, 0, c[3]) >= c[4] and 2 * pool_out(c[5], 2, 2, 0, c[3]) >= c[5]) for c in R.pool_cases() if c[:3] == (2, 2, 0)]
    assert any(sc and c[3] and c[4] % 2 for c, sc in scatter), "scatter kernel on a ceil-mode map with an odd side"
    assert any(not sc and not c[3] and c[4] % 2 for c, sc in scatter), "gather form on a floor-mode map with an odd side"


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_maxpool_nan_and_infinities_follow_the_scan(dtype):
    """NaN, +inf and -inf at the first, a middle and the last position of windows, border windows and an all -inf channel included:
    the first maximum wins, a NaN replaces whatever came before it, so the last NaN of a window is the one the code names."""
    for i, (k, s, p, ce) in enumerate(R.POOL_GEOMETRIES):
        gen = _gen(900 + i)
        x, _, _ = R.pool_int_data(2, 24, 7, 10, k, s, p, ce, gen)
        x = R.plant_specials(x, gen)
        assert bool(torch.isnan(x).any()) and bool((x == float("inf")).any()) and bool((x == float("-inf")).any())
        _, y, am, ref_v, ref_c = _pool_forward_checks(x, k, s, p, ce, dtype, f"pool with specials {(k, s, p, ce)}")
        assert bool(torch.isnan(y).any()) and bool((y[:, :, :, 3] == float("-inf")).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_maxpool_grid_stride_loops(dtype):
    """More than 4096 blocks of 256 threads in the forward, the gather backward and the 2x2 scatter backward: every thread loops."""
    n, c, h, w = (3, 256, 150, 150) if dtype == F32 else (6, 256, 150, 150)
    k, s, p, ce = 2, 2, 0, False
    assert n * (h // 2) * (w // 2) * (c // (4 if dtype == F32 else 8)) > 4096 * 256
    x, dy, prev = R.pool_int_data(n, c, h, w, k, s, p, ce, _gen(77), relu=True)
    fw = _pool_forward_checks(x, k, s, p, ce, dtype, "large pool")
    _pool_backward_checks(x, dy, prev, *fw, k, s, p, dtype, "large pool", ("plain", "gated"))


# ---- L2 norm ------------------------------------------------------------------------------------------------------------------------
def _l2_fwd(x, gamma):
    lib, check, st = _lib()
    m = x.shape[0]
    y = Canvas((m, 512), x.dtype)
    fn = lib.ssd_l2norm_fwd_bf16 if x.dtype == BF16 else lib.ssd_l2norm_fwd
    check(fn(x.data_ptr(), gamma.data_ptr(), y.ptr(), m, 512, st), "l2norm_fwd")
    return y.done("l2norm y")


def _l2_bwd(x, gamma, dy):
    lib, check, st = _lib()
    m = x.shape[0]
    dx, dg = Canvas((m, 512), x.dtype), Canvas((512,), F32)
    bf = x.dtype == BF16
    nbytes = (lib.ssd_l2norm_bwd_bf16_workspace if bf else lib.ssd_l2norm_bwd_workspace)(m, 512)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    fn = lib.ssd_l2norm_bwd_bf16 if bf else lib.ssd_l2norm_bwd
    check(fn(x.data_ptr(), gamma.data_ptr(), dy.data_ptr(), dx.ptr(), dg.ptr(), m, 512, ws.data_ptr(), nbytes, st), "l2norm_bwd")
    return dx.done("l2norm dx"), dg.done("l2norm dgamma")


def _rounded(t, dtype):
    """an exact f64 result as the kernel must store it: unchanged in f32 (asserted exact), rounded once to nearest even in bf16"""
    if dtype == BF16:
        return R.bf16_rne(t.cpu())
    assert bool((t.float().double() == t).all())
    return t.float()


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("m", [1, 5, 37, 2051, 8197])
def test_l2norm_on_exact_data(m, dtype):
    """M = 1: one block with idle waves; 5: a ragged last block; 37: fewer than 16 slabs; 2051: over the backward's 512 blocks (rows and
    slab sums loop); 8197: over the forward's 2048 blocks.  y, dx and dgamma are exact whatever the order of the sums."""
    x, gamma, dy = R.l2norm_exact_data(m, _gen(m))
    ref = R.l2norm_ref(x, gamma, dy)
    xk, dyk = x.to(dtype), dy.to(dtype)
    assert torch.equal(xk.float(), x) and torch.equal(dyk.float(), dy)
    _eq(_l2_fwd(xk, gamma).cpu(), _rounded(ref["y"], dtype).cpu(), f"l2norm y, M={m}")
    if dtype == BF16:
        assert torch.equal(R.bf16_rne(ref["y"].cpu()).double(), ref["y"].cpu())                 # +-gamma/2 is a bf16 value
    dx, dg = _l2_bwd(xk, gamma, dyk)
    _eq(dx.cpu(), _rounded(ref["dx"], dtype).cpu(), f"l2norm dx, M={m}")
    _eq(dg, _rounded(ref["dg"], F32), f"l2norm dgamma, M={m}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
def test_l2norm_of_an_all_zero_row_is_nan_like_the_division_without_epsilon(dtype):
    m = 37
    x, gamma, _ = R.l2norm_exact_data(m, _gen(3))
    x[0] = 0
    x[17] = 0
    ref = R.l2norm_ref(x, gamma)["y"]
    assert bool(torch.isnan(ref[[0, 17]]).all()) and int(torch.isnan(ref).sum()) == 2 * 512
    y = _l2_fwd(x.to(dtype), gamma)
    assert bool(torch.isnan(y[[0, 17]]).all())
    _eq(y.cpu(), (R.bf16_rne(ref.cpu()) if dtype == BF16 else ref.float().cpu()), "l2norm y next to zero rows")


def _worst(err, bound):
    """largest err / bound over the elements with a bound, after asserting err == 0 where the bound is 0"""
    zero = bound == 0
    assert float(err[zero].max() if bool(zero.any()) else 0.0) == 0.0
    return float((err[~zero] / bound[~zero]).max())


def test_l2norm_f32_on_general_data_meets_per_element_bounds():
    """Rows whose norms span e^-12 .. e^12, 40 % zeros.  With u = 2^-24: |y - ref| <= 32u |ref|, |dx - ref| <= 32u (|gamma dy|/|x| +
    |x| sum|x dy gamma|/|x|^3), |dgamma - ref| <= (M + 32)u sum_m |dy x|/|x|.  A row's sum of 512 terms is 8 adds per lane and 6 butterfly
    steps (14u), the square root halves that, the formula's own roundings are added and the total doubled; the dgamma bound is the
    order-free bound of a sum of M terms.  A plain numpy f32 evaluation stays at or under 3.3u of each bound."""
    m = 37
    x, gamma, dy = R.l2norm_general_data(m, _gen(41))
    ref = R.l2norm_ref(x, gamma, dy)
    y = _l2_fwd(x, gamma)
    dx, dg = _l2_bwd(x, gamma, dy)
    wy = _worst((y.double() - ref["y"]).abs(), U * ref["y"].abs())
    wdx = _worst((dx.double() - ref["dx"]).abs(), U * ref["dx_abs"])
    wdg = _worst((dg.double() - ref["dg"]).abs(), U * ref["dg_abs"])
    print(f"l2norm f32 general data, error in units of u x bound: y {wy:.2f}, dx {wdx:.2f}, dgamma {wdg:.2f} (bars 32, 32, {m + 32})")
    assert wy <= 32 and wdx <= 32 and wdg <= m + 32, (wy, wdx, wdg)


_bf16_general_cache = []


def _l2norm_bf16_general():
    """the bf16 kernels on general data whose x and dy are bf16 values, once for the tests below: (M, results, f64 reference)"""
    if not _bf16_general_cache:
        m = 37
        x, gamma, dy = R.l2norm_general_data(m, _gen(43))
        xk, dyk = x.to(BF16), dy.to(BF16)
        ref = R.l2norm_ref(xk.double(), gamma, dyk.double())
        dx, dg = _l2_bwd(xk, gamma, dyk)
        _bf16_general_cache.append((m, {"y": _l2_fwd(xk, gamma), "dx": dx, "dg": dg}, ref))
    return _bf16_general_cache[0]


def test_l2norm_bf16_on_general_data_meets_the_f32_bounds_and_one_rounding():
    """The bf16 kernels do at least the f32 kernels' arithmetic and round once at the store, so a stored value is at most the f32
    bound of test_l2norm_f32_on_general_data_meets_per_element_bounds plus half a bf16 ulp (taken at |ref| + that bound, where the value
    before the rounding may lie) from the f64 value.  dgamma stays f32 under the f32 bound."""
    m, got, ref = _l2norm_bf16_general()
    for what, scale in (("y", ref["y"].abs()), ("dx", ref["dx_abs"])):
        err, a = (got[what].double() - ref[what]).abs(), 32 * U * scale
        bound = a + 0.5 * R.bf16_ulp(ref[what].abs() + a)
        print(f"l2norm bf16 general data, {what}: worst error {float((err / bound.clamp_min(1e-300)).max()):.3f} of 32u x bound + ulp/2")
        assert bool((err <= bound).all()), what
    wdg = _worst((got["dg"].double() - ref["dg"]).abs(), U * ref["dg_abs"])
    print(f"l2norm bf16 general data, dgamma error in units of u x bound: {wdg:.2f} (bar {m + 32})")
    assert wdg <= m + 32


def test_l2norm_bf16_on_general_data_is_the_rounded_f64_value():
    """y and dx must lie within one bf16 ulp of the f64 value everywhere and equal its rounding to nearest even on at least 99 % of
    the elements: the f32 arithmetic before the store is some 2^-16 of an ulp off, so only values that close to a rounding boundary
    (about 0.03 %) may land on the other side.

    The case that failed first, kept: the two terms of dx = gamma dy/|x| - x (sum x dy gamma)/|x|^3 cancel, at one of these 18 944
    elements to 1.93e-6 of the sum of their absolute values.  A backward that formed dx in f32 was 0.361 u of that sum from the f64
    value there -- far inside the f32 bar of 32 u -- and still 1.725 bf16 ulp from it (a plain torch f32 evaluation misses one ulp
    on 6 of 200 seeds of these data, by up to 5.2 ulp).  l2norm_bwd_bf16_kernel therefore carries its row sums and dx in f64."""
    m, got, ref = _l2norm_bf16_general()
    fig = {}
    for what, scale in (("y", ref["y"].abs()), ("dx", ref["dx_abs"])):
        want = ref[what]
        ulps = (got[what].double() - want).abs() / R.bf16_ulp(want)
        i = int(ulps.argmax())
        same = float((got[what].cpu() == R.bf16_rne(want.cpu())).double().mean())
        fig[what] = (float(ulps.max()), int((ulps > 1).sum()), same)
        print(f"l2norm bf16 general data, {what}: {100 * same:.3f} % of {want.numel()} equal the rounded f64 value; worst {fig[what][0]:.3f} ulp, "
              f"{fig[what][1]} over one ulp; at the worst element |ref| is {float((want.abs() / scale).flatten()[i]):.3g} of the sum of its "
              f"absolute terms and the error {float(((got[what].double() - want).abs() / (U * scale)).flatten()[i]):.3f} u of that sum")
    for what, (worst, over, same) in fig.items():
        assert worst <= 1.0, f"l2norm bf16 {what}: {over} elements more than one ulp from the f64 value, worst {worst:.3f} ulp"
        assert same >= 0.99, (what, same)


# ---- heads --------------------------------------------------------------------------------------------------------------------------
def _pad(c, q):
    return (c + q - 1) // q * q


def _tie_heavy(shape, gen):
    """randn, a quarter of the elements replaced by exact ties between two neighbouring bf16 values (lower 16 bits 0x8000)"""
    v = torch.randn(shape, generator=gen, device=gen.device)
    tie = (v.view(torch.int32) & -65536) | 0x8000
    return torch.where(torch.rand(shape, generator=gen, device=gen.device) < 0.25, tie.view(F32), v)


def _heads_case(level, ncls, n):
    lib, check, st = _lib()
    hw, a = R.SSD300_LEVELS[level]
    off, P = R.ssd300_prior_offsets()[level], R.SSD300_P
    cw = a * (4 + ncls)
    ld = _pad(cw, 32)
    gen = _gen(1000 * level + 10 * ncls + n)
    what = f"heads level {level} (HW={hw}, A={a}) ncls={ncls} N={n}"
    # scatter: the level's rows, every other row of both tensors and the tails untouched
    packed = torch.randn((n * hw, ld), generator=gen, device=_dev())
    loc, conf = Canvas((n, P, 4)), Canvas((n, P, ncls))
    check(lib.ssd_heads_scatter(packed.data_ptr(), ld, loc.ptr(), conf.ptr(), n, hw, a, off, P, ncls, st), "heads_scatter")
    want_loc, want_conf = torch.full((n, P, 4), SENT, device=_dev()), torch.full((n, P, ncls), SENT, device=_dev())
    want_loc[:, off:off + hw * a], want_conf[:, off:off + hw * a] = R.heads_ref(packed, ld, n, hw, a, ncls)
    _eq(loc.done(what), want_loc, f"{what}: loc after the scatter")
    _eq(conf.done(what), want_conf, f"{what}: conf after the scatter")
    # gather: the inverse below A*(4+ncls), zeros from there to ld; the bf16 form is its rounding
    dloc, dconf = _tie_heavy((n, P, 4), gen), _tie_heavy((n, P, ncls), gen)
    want = R.heads_inverse_ref(dloc[:, off:off + hw * a], dconf[:, off:off + hw * a], ld, n, hw, a, ncls)
    assert ld == cw or float(want[:, cw:].abs().max()) == 0.0
    back = Canvas((n * hw, ld))
    check(lib.ssd_heads_gather(dloc.data_ptr(), dconf.data_ptr(), back.ptr(), ld, n, hw, a, off, P, ncls, st), "heads_gather")
    _eq(back.done(what), want, f"{what}: gather")
    ld16 = _pad(cw, 64)
    want16 = R.heads_inverse_ref(dloc[:, off:off + hw * a], dconf[:, off:off + hw * a], ld16, n, hw, a, ncls)
    back16 = Canvas((n * hw, ld16), BF16)
    check(lib.ssd_heads_gather_bf16(dloc.data_ptr(), dconf.data_ptr(), back16.ptr(), ld16, n, hw, a, off, P, ncls, st), "heads_gather_bf16")
    _eq(back16.done(what).cpu(), R.bf16_rne(want16.cpu()), f"{what}: bf16 gather")
    assert ld16 > cw and float(back16.t[:, cw:].float().abs().max()) == 0.0


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("ncls", [21, 2, 81])
@pytest.mark.parametrize("level", range(6))
def test_heads_scatter_and_gather_at_every_ssd300_level(level, ncls, n):
    _heads_case(level, ncls, n)


def test_heads_scatter_and_gather_over_the_grid_cap():
    hw, a = R.SSD300_LEVELS[0]
    assert 8 * hw * a * 25 == 1155200 > 4096 * 256 and 8 * hw * 128 == 1478656
    _heads_case(0, 21, 8)


# ---- casts --------------------------------------------------------------------------------------------------------------------------
def test_cast_bf16_to_f32_over_all_65536_bit_patterns():
    lib, check, st = _lib()
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    x = bits.view(BF16)
    want = x.float()
    y = Canvas((65536,))
    check(lib.ssd_cast_bf16_f32(x.to(_dev()).data_ptr(), y.ptr(), 65536, st), "cast_bf16_f32")
    got = y.done("cast to f32").cpu()
    same = (got.view(torch.int32) == want.view(torch.int32)) | (torch.isnan(got) & torch.isnan(want))
    assert bool(same.all()), f"{int((~same).sum())} bit patterns differ, first {int(bits[(~same).nonzero()[0]]) & 0xFFFF:#06x}"
    assert int(torch.isnan(want).sum()) == 2 * 127


@pytest.mark.parametrize("n", [8, 8 * (2 ** 20 + 1)])
def test_cast_f32_to_bf16_rounds_to_nearest_even(n):
    """Ties in both directions at every exponent, their f32 neighbours, overflow to inf, +-0, +-inf, f32 subnormals and values that
    round to bf16 subnormals: non-NaN results bit for bit the CPU's round-to-nearest-even, a NaN stays a NaN.  n = 8 is one thread;
    8 (2^20 + 1) is one element vector more than 4096 blocks of 256 threads take in one pass."""
    lib, check, st = _lib()
    vals = R.cast_f32_values()
    if n == 8:
        chunks = vals.view(-1, 8)
    else:
        assert n > 4096 * 256 * 8
        chunks = vals.repeat(-(-n // vals.numel()))[:n].view(1, n)
    for x in chunks:
        want = R.bf16_rne(x)
        y = Canvas((x.numel(),), BF16)
        check(lib.ssd_cast_f32_bf16(x.to(_dev()).data_ptr(), y.ptr(), x.numel(), st), "cast_f32_bf16")
        got = y.done("cast to bf16").cpu()
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan), "a NaN must stay a NaN, and nothing else become one"
        bad = (got.view(torch.int16) != want.view(torch.int16)) & ~nan
        assert not bool(bad.any()), (f"{int(bad.sum())} of {x.numel()} differ from round-to-nearest-even; first: f32 bits "
                                     f"{int(x.view(torch.int32)[bad.nonzero()[0]]) & 0xFFFFFFFF:#010x} -> {int(got.view(torch.int16)[bad.nonzero()[0]]) & 0xFFFF:#06x}, "
                                     f"want {int(want.view(torch.int16)[bad.nonzero()[0]]) & 0xFFFF:#06x}")


# ---- channel_affine -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inplace", [False, True], ids=["out", "inplace"])
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("m,c", [(37, 4), (37, 256), (16400, 256)])
def test_channel_affine_per_element(m, c, relu, inplace):
    """|y - (x a + b)| <= 2^-23 (|x a| + |b|): one rounding of the product and one of the sum, or the single one of a fused multiply-add.
    The ReLU cannot widen it (|max(p, 0) - max(q, 0)| <= |p - q|).  M = 16400 at C = 256 is over 4096 blocks of 256 threads."""
    lib, check, st = _lib()
    assert (m, c) != (16400, 256) or m * c // 4 > 4096 * 256
    gen = _gen(m + c)
    x = torch.randn((m, c), generator=gen, device=_dev())
    a, b = torch.randn(c, generator=gen, device=_dev()), torch.randn(c, generator=gen, device=_dev())
    y = Canvas((m, c), fill=x if inplace else None)
    check(lib.ssd_channel_affine(y.ptr() if inplace else x.data_ptr(), a.data_ptr(), b.data_ptr(), y.ptr(), m, c, int(relu), st), "channel_affine")
    got = y.done("channel_affine").double()
    ref = x.double() * a.double() + b.double()
    bound = 2.0 ** -23 * ((x.double() * a.double()).abs() + b.double().abs())
    if relu:
        ref = ref.clamp_min(0)
        assert bool((got >= 0).all())
    assert bool(((got - ref).abs() <= bound).all()), f"worst {float(((got - ref).abs() / bound).max()):.3f} of the bound"

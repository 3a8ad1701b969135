"""tests/elementwise_ref.py held to torch itself on the CPU: the pool scan against F.max_pool2d's values and indices (ties, NaN, +-inf,
every geometry the kernel tests use), its backward against autograd, the L2 norm against autograd of Model.py:207-209, and the
exact-data generators against their own claim."""
import pytest
import torch
import torch.nn.functional as F

import elementwise_ref as R

NAN, INF = float("nan"), float("inf")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("window,index,value", [
    ([1, 1, 1, 1], 0, 1.0), ([3, 3, 2, 3], 0, 3.0), ([NAN, 1, 2, 3], 0, NAN), ([1, NAN, 5, 0], 1, NAN), ([1, 2, NAN, NAN], 3, NAN),
    ([-INF] * 4, 0, -INF), ([0, 1, 1, 0], 1, 1.0), ([-INF, INF, INF, NAN], 3, NAN)])
def test_the_scan_picks_the_first_maximum_and_the_last_nan(window, index, value):
    x = torch.tensor(window, dtype=torch.float64).view(1, 1, 2, 2)
    v, c = R.pool_ref(x, 2, 2, 0, False)
    tv, ti = F.max_pool2d(x, 2, 2, 0, ceil_mode=False, return_indices=True)
    assert int(c) == index == int(ti)
    assert bool(R.nan_equal(v, torch.tensor(value, dtype=torch.float64)).all()) and bool(R.nan_equal(v, tv).all())


def _pool_inputs(case):
    k, s, p, ce, h, w = case
    gen = _gen(11 + h * 100 + w + k)
    for relu in (False, True):
        x, dy, prev = R.pool_int_data(2, 5, h, w, k, s, p, ce, gen, relu)
        yield x.double(), dy.double(), prev.double(), False
    yield R.plant_specials(x, gen).double(), dy.double(), prev.double(), True


@pytest.mark.parametrize("case", R.pool_cases(), ids=str)
def test_pool_ref_equals_torch_values_indices_and_autograd(case):
    k, s, p, ce, h, w = case
    for x, dy, prev, special in _pool_inputs(case):
        xr = x.clone().requires_grad_(True)
        tv, ti = F.max_pool2d(xr, k, s, p, ceil_mode=ce, return_indices=True)
        v, c = R.pool_ref(x, k, s, p, ce)
        assert v.shape == tv.shape
        assert bool(R.nan_equal(v, tv.detach()).all())
        assert torch.equal(c, R.flat_to_codes(ti, w, k, s, p))
        if special:
            continue                                         # NaN gradients compare with nothing
        tv.backward(dy)
        g = xr.grad
        assert torch.equal(R.pool_bwd_ref(dy, c, x.shape, k, s, p), g)
        assert torch.equal(R.pool_bwd_ref(dy, c, x.shape, k, s, p, mask=x), g * (x > 0))
        assert torch.equal(R.pool_bwd_ref(dy, c, x.shape, k, s, p, prev=prev, mask=x), (g + prev) * (x > 0))
        xr.grad = None
        F.max_pool2d(xr, k, s, p, ceil_mode=ce).backward(dy * (v > 0))
        assert torch.equal(R.pool_bwd_ref(dy, c, x.shape, k, s, p, gate=v), xr.grad)
        if bool((x >= 0).all()):                             # post-ReLU input: the gate by the output is the mask by the input
            assert torch.equal(R.pool_bwd_ref(dy, c, x.shape, k, s, p, gate=v), g * (x > 0))


def test_pool_cases_cover_every_geometry_and_map():
    cases = R.pool_cases()
    assert {c[:4] for c in cases} == set(R.POOL_GEOMETRIES) and {c[4:] for c in cases} == set(R.POOL_MAPS)
    assert [c for c in cases if c[4:] == (1, 1)] == [(3, 1, 1, True, 1, 1)]


def test_l2norm_ref_equals_autograd():
    gen = _gen(5)
    x, gamma, dy = (t.double() for t in R.l2norm_general_data(37, gen))
    x4 = x.t().reshape(1, 512, 37, 1).clone().requires_grad_(True)
    g4 = gamma.view(1, 512, 1, 1).clone().requires_grad_(True)
    y = x4 / x4.pow(2).sum(dim=1, keepdim=True).sqrt() * g4                 # Model.py:207-209
    y.backward(dy.t().reshape(1, 512, 37, 1))
    ref = R.l2norm_ref(x, gamma, dy)
    close = lambda a, b, scale: bool(((a - b).abs() <= 1e-13 * scale).all())            # noqa: E731  (f64 against f64)
    assert close(ref["y"], y.detach()[0, :, :, 0].t(), ref["y"].abs() + 1e-300)
    assert close(ref["dx"], x4.grad[0, :, :, 0].t(), ref["dx_abs"])
    assert close(ref["dg"], g4.grad.view(-1), ref["dg_abs"])


@pytest.mark.parametrize("m", [1, 5, 37, 2051, 8197])
def test_exact_l2norm_data_gives_one_result_in_f32_in_any_order(m):
    gen = _gen(m)
    x, gamma, dy = R.l2norm_exact_data(m, gen)                              # asserts its precondition
    if m >= 2051:
        assert bool((x != 0).any(0).all()), "every channel, so every lane and both vectors of a lane, must be hit"
    ref = R.l2norm_ref(x, gamma, dy)
    perm_c, perm_m = torch.randperm(512, generator=gen), torch.randperm(m, generator=gen)
    xs, gs, ds = x[perm_m][:, perm_c], gamma[perm_c], dy[perm_m][:, perm_c]
    nrm = torch.zeros(m, 1)
    dot = torch.zeros(m, 1)
    for j in range(0, 512, 64):                                             # f32, a summation order of its own
        nrm += (xs[:, j:j + 64] * xs[:, j:j + 64]).sum(1, keepdim=True)
        dot += (xs[:, j:j + 64] * ds[:, j:j + 64] * gs[j:j + 64]).sum(1, keepdim=True)
    inv = 1 / nrm.sqrt()
    y = xs / nrm.sqrt() * gs
    dx = gs * ds * inv - xs * (dot * inv * inv * inv)
    dg = torch.zeros(512)
    for i in range(0, m, 7):
        dg += (ds[i:i + 7] * xs[i:i + 7] * inv[i:i + 7]).sum(0)
    assert y.dtype == dx.dtype == dg.dtype == torch.float32
    assert torch.equal(y.double(), ref["y"][perm_m][:, perm_c])
    assert torch.equal(dx.double(), ref["dx"][perm_m][:, perm_c])
    assert torch.equal(dg.double(), ref["dg"][perm_c])
    assert torch.equal(R.bf16_rne(ref["y"]).double(), ref["y"])             # y = +-gamma/2 is a bf16 value


def test_heads_ref_and_its_inverse():
    offs = R.ssd300_prior_offsets()
    assert offs == [0, 5776, 7942, 8542, 8692, 8728]
    N, HW, A, ncls, ld = 2, 9, 4, 3, 32
    packed = torch.arange(N * HW * ld, dtype=torch.float32).view(N * HW, ld)
    loc, conf = R.heads_ref(packed, ld, N, HW, A, ncls)
    assert loc.shape == (N, HW * A, 4) and conf.shape == (N, HW * A, ncls)
    assert float(loc[1, 2 * A + 1, 2]) == float(packed[HW + 2, 4 * 1 + 2])
    assert float(conf[1, 2 * A + 3, 1]) == float(packed[HW + 2, 4 * A + 3 * ncls + 1])
    back = R.heads_inverse_ref(loc, conf, ld, N, HW, A, ncls)
    want = packed.clone()
    want[:, A * (4 + ncls):] = 0
    assert torch.equal(back, want)


def test_cast_values_hold_the_cases_they_name():
    v = R.cast_f32_values()
    assert v.numel() % 8 == 0 and v.dtype == torch.float32
    r = R.bf16_rne(v)
    bits = lambda *b: R._f32_from_bits(list(b))                                                  # noqa: E731
    rb = lambda *b: R.bf16_rne(bits(*b)).view(torch.int16).tolist()                              # noqa: E731
    assert rb(0x3F808000, 0x3F818000) == [0x3F80, 0x3F82]                   # ties go to the even neighbour, down and up
    assert rb(0x3F807FFF, 0x3F808001) == [0x3F80, 0x3F81]
    assert rb(0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF) == [0x7F7F, 0x7F80, 0x7F80]
    assert rb(0x00008000, 0x00008001, 0x00018000) == [0, 1, 2]             # around the smallest bf16 subnormal
    assert bool(torch.isnan(R.bf16_rne(bits(0x7F80FFFF, 0x7F800001))).all())
    vb = v.view(torch.int32)
    assert bool(torch.isnan(v).any()) and bool(torch.isinf(v).any()) and bool(torch.isinf(r[torch.isfinite(v)]).any())
    assert bool((((vb & 0x7F800000) == 0) & ((vb & 0x007FFFFF) != 0)).any())                    # f32 subnormals
    assert bool(((vb & 0xFFFF) == 0x8000).sum() > 800)                                          # ties
    assert len({int(e) for e in ((vb >> 23) & 0xFF).tolist()}) == 256                           # every exponent

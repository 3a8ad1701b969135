"""The kernels of csrc/batchnorm.hip, called bare through ops.bn_train_stats / bn_apply / bn_train_bwd / dropout_mask and held to
bn_ref.py: the statistics to the per-channel rounding bounds of bn_ref.stats_bars on well- and ill-conditioned data at every edge of
the slab plan, apply and backward to exact equality on integer data (bn_ref.exact_case) with the dropout mask taken from the numpy
Philox restatement, never from the device.  Every tensor a kernel gets carries a NaN sentinel in its pad columns (ld > C): a read
of a pad column poisons a result, and after the call the pad columns of every output must still hold the sentinel's bits.

Every tolerance is exact equality, a bound written out in bn_ref from u = 2^-24, the plan's depth and the data, or -- in the one
chained case -- the error of torch's own CPU f32 autograd on the same data times 5.

Out of scope by construction: the high word of the Philox counter (needs 2^34 dropout indices), (float)M beyond 2^24 rows, and the
walk of blockIdx.y over channel chunks beyond the second (C = 260 has two; more needs nothing the second does not).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_ref as R

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-5, 0.1
SENT = 0x7FC0BAD1                                               # a quiet NaN with a payload
SEED = (0x9E3779B9 << 32) | 0x01234567                          # nonzero high word
_id = lambda s: "x".join(map(str, s))                           # noqa: E731


def sentinel(M, ld):
    return torch.full((M, ld), SENT, dtype=torch.int32).view(torch.float32)


def dev(a, ld=None):
    """(M, C) -> [M][ld] f32 rows on the device, the pad columns holding the sentinel"""
    a = np.asarray(a, np.float32)
    t = sentinel(a.shape[0], ld or a.shape[1])
    t[:, :a.shape[1]] = torch.from_numpy(a)
    return t.cuda()


def vec(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t, C=None):
    return (t if C is None else t[:, :C]).cpu().double().numpy()


def pad_intact(t, C):
    return bool((t[:, C:].view(torch.int32) == SENT).all())


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def hw_of(M):
    """rows per sample of the per-sample dropout cases: a divisor of M (M itself, one sample, for a prime M)"""
    return next((d for d in (49, 17, 7, 5, 3, 2) if M % d == 0 and d < M), M)


# ---- statistics -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("shape", R.STATS_SHAPES, ids=_id)
def test_statistics_within_the_derived_bars(shape, fam):
    from objectdetection_ssd_amd import ops
    M, C, ld = shape
    x = R.family(fam, M, C, 2)
    gamma, beta, rm, rv = R.channel_params(C, 2)
    pl = R.plan(M, C)
    ref = R.stats_ref(x, gamma, beta, EPS, MOM, rm, rv)
    bars = R.stats_bars(x, pl, gamma, beta, EPS, MOM, rm, rv)
    xd = dev(x, ld)
    x0 = xd.clone()
    gd, bd, rmd, rvd = vec(gamma), vec(beta), vec(rm), vec(rv)
    nbt = torch.full((), 41, dtype=torch.int64, device="cuda")
    st = ops.bn_train_stats(xd, C, gd, bd, EPS, MOM, rmd, rvd, nbt, ld=ld)

    def within(pairs, ref, bars, tag):
        worst = {}
        for name, got in pairs:
            err = np.abs(host(got) - getattr(ref, name))
            bar = getattr(bars, name)
            with np.errstate(invalid="ignore", divide="ignore"):
                worst[name] = float(np.where(err == 0, 0.0, err / bar).max())
            assert (err <= bar).all(), (name, int(np.argmax(~(err <= bar))), err.max(), worst)
        print(f"{tag} {_id(shape)} {fam} depth {R.stats_depth(pl)} error/bar", {k: f"{v:.3g}" for k, v in worst.items()})

    within((("mean", st[0]), ("invstd", st[1]), ("scale", st[2]), ("shift", st[3]), ("running_mean", rmd), ("running_var", rvd)),
           ref, bars, "stats")
    assert int(nbt) == 42
    if fam == "constant":
        assert same_bits(st[0], vec(x[0]))
        want = 1.0 / np.sqrt(float(np.float32(EPS)))
        assert (np.abs(host(st[1]) - want) <= 2 * float(np.spacing(np.float32(want)))).all()
    # running buffers and the counter absent: everything else bit-equal, and nothing of theirs touched
    rm1, rv1 = rmd.clone(), rvd.clone()
    st2 = ops.bn_train_stats(xd, C, gd, bd, EPS, MOM, None, None, None, ld=ld)
    assert same_bits(st, st2) and int(nbt) == 42 and same_bits(rmd, rm1) and same_bits(rvd, rv1)
    # a repeat launch from the same buffers: the same bits, the counter up by one again
    rm2, rv2 = vec(rm), vec(rv)
    st3 = ops.bn_train_stats(xd, C, gd, bd, EPS, MOM, rm2, rv2, nbt, ld=ld)
    assert same_bits(st, st3) and same_bits(rm2, rmd) and same_bits(rv2, rvd) and int(nbt) == 43
    # gamma / beta absent: 1 / 0
    st4 = ops.bn_train_stats(xd, C, None, None, EPS, MOM, None, None, None, ld=ld)
    assert same_bits(st4[:2], st[:2])
    within((("scale", st4[2]), ("shift", st4[3])), R.stats_ref(x, None, None, EPS, MOM, None, None),
           R.stats_bars(x, pl, None, None, EPS, MOM, None, None), "no-affine")
    assert same_bits(xd, x0)


# ---- apply ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def exact(M, C, mode, p, HW):
    return R.exact_case(M, C, SEED, mode, p, 3, HW)


APPLY_SHAPES = [(5, 4, 4, 5), (147, 12, 96, 49), (8193, 512, 512, 3)]      # M, C, ld, HW; the last: 1,048,704 vectors, a second trip
RES_FORMS = (None, "id", "scaled")


def run_apply(ops, c, xd, C, lds, relu, form, drop, dv, out=None):
    ldx, ldr, ldy = lds
    out = sentinel(xd.shape[0], ldy).cuda() if out is None else out
    res = None if form is None else dv["res"]
    return ops.bn_apply(xd, C, dv["scale"], dv["shift"], relu=relu, res=res, res_scale=dv["res_scale"] if form == "scaled" else None,
                        res_shift=dv["res_shift"] if form == "scaled" else None, drop=drop, out=out, ld=ldx, res_ld=ldr, out_ld=ldy)


def ref_apply(c, relu, form, factor):
    kw = {} if form is None else {"res": c["res"]} if form == "id" else {k: c[k] for k in ("res", "res_scale", "res_shift")}
    return R.apply_ref(c["x"], c["scale"], c["shift"], relu=relu, factor=factor, **kw)


def apply_devs(c, lds):
    return {"res": dev(c["res"], lds[1]), **{k: vec(c[k]) for k in ("scale", "shift", "res_scale", "res_shift")}}


# every mode with both factors at the small shapes; the large shape takes each mode once
APPLY_CASES = [(s, m, p) for s in APPLY_SHAPES for m, p in ((0, 0.0), (1, 0.5), (2, 0.75), (1, 0.75), (2, 0.5))
               if s[0] <= 4096 or (m, p) in ((0, 0.0), (1, 0.5), (2, 0.75))]


@pytest.mark.parametrize("shape,mode,p", APPLY_CASES, ids=lambda v: _id(v) if isinstance(v, tuple) else str(v))
def test_apply_is_exact_on_integer_data(shape, mode, p):
    from objectdetection_ssd_amd import ops
    M, C, ld, HW = shape
    big = M > 4096
    c = exact(M, C, mode, p, HW)
    lds = (ld, ld + 4, ld + 8)
    xd, dv = dev(c["x"], lds[0]), apply_devs(c, lds)
    forms = [(True, "scaled"), (False, "id"), (True, None)] if big else [(r, f) for r in (False, True) for f in RES_FORMS]
    for relu, form in forms:
        out = run_apply(ops, c, xd, C, lds, relu, form, c["drop"], dv)
        assert np.array_equal(host(out, C), ref_apply(c, relu, form, c["factor"])), (relu, form)
        assert pad_intact(out, C)
    # in place (y is x, with a residual and dropout): the bits of the out-of-place call
    xi = xd.clone()
    run_apply(ops, c, xi, C, (ld, ld + 4, ld), True, "scaled", c["drop"], dv, out=xi)
    ref = run_apply(ops, c, xd, C, lds, True, "scaled", c["drop"], dv)
    assert same_bits(xi[:, :C], ref[:, :C]) and pad_intact(xi, C) and pad_intact(dv["res"], C)


@pytest.mark.parametrize("shape", APPLY_SHAPES, ids=_id)
def test_apply_at_p_0_and_p_1(shape):
    from objectdetection_ssd_amd import ops
    M, C, ld, HW = shape
    c = exact(M, C, 0, 0.0, HW)
    lds = (ld, ld + 4, ld + 8)
    xd, dv = dev(c["x"], lds[0]), apply_devs(c, lds)
    for relu, form in ((False, "scaled"), (True, "id")):
        plain = run_apply(ops, c, xd, C, lds, relu, form, None, dv)
        assert np.array_equal(host(plain, C), ref_apply(c, relu, form, None))
        for mode in (1, 2):
            keep_all = run_apply(ops, c, xd, C, lds, relu, form, (mode, 0.0, SEED, 3, HW), dv)
            assert same_bits(keep_all, plain)
            drop_all = run_apply(ops, c, xd, C, lds, relu, form, (mode, 1.0, SEED, 3, HW), dv)
            assert not drop_all[:, :C].any() and pad_intact(drop_all, C)


def test_apply_on_randn_data_within_four_roundings():
    """relu(x*scale + shift + res) * factor rounds four times at most (product, two sums, factor; 1/(1-p) is formed on the host and
    is bn_ref.drop_scale exactly), each by at most u times the sum of the magnitudes of the terms"""
    from objectdetection_ssd_amd import ops
    M, C, HW = 147, 12, 49
    lds = (96, 100, 104)
    rng = np.random.default_rng(11)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)                              # noqa: E731
    c = {"x": f(M, C) * 2 + 0.5, "res": f(M, C), "scale": f(C), "shift": f(C), "res_scale": f(C), "res_shift": f(C)}
    xd, dv = dev(c["x"], lds[0]), apply_devs(c, lds)
    for mode in (1, 2):
        factor = R.drop_factor(mode, 0.3, SEED, 6, M, C, HW)
        out = run_apply(ops, c, xd, C, lds, True, "id", (mode, 0.3, SEED, 6, HW), dv)
        ref, mag = R.apply_ref(c["x"], c["scale"], c["shift"], res=c["res"], relu=True, factor=factor, terms=True)
        err = np.abs(host(out, C) - ref)
        print("apply randn: largest error / bar", float((err / np.maximum(4 * R.U * mag, 1e-300)).max()))
        assert (err <= 4 * R.U * mag).all() and pad_intact(out, C)
        assert ((host(out, C) == 0) >= (factor == 0)).all()


# ---- backward ---------------------------------------------------------------------------------------------------------------------
BWD_SHAPES = [s for s in R.STATS_SHAPES if s[0] != 66563] + [(8193, 512, 512), (1024, 12, 32)]


def run_bwd(ops, dyd, xd, C, dv, lds, drop, relu_mask, gamma=True, dg=None, db=None, accumulate=False, dx=None, want_dx=True):
    ld_dy, ld_x, ld_dx = lds
    if want_dx and dx is None:
        dx = sentinel(xd.shape[0], ld_dx).cuda()
    return ops.bn_train_bwd(dyd, xd, C, dv["mean"], dv["invstd"], dv["gamma"] if gamma else None, drop, relu_mask, dg, db, accumulate,
                            dx=dx, want_dx=want_dx, ld_dy=ld_dy, ld_x=ld_x, ld_dx=ld_dx if want_dx else None)


@pytest.mark.parametrize("mode,p", [(0, 0.0), (1, 0.5), (2, 0.75)])
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=_id)
def test_backward_sums_exact_and_dx_exact_or_within_its_bar(shape, mode, p):
    from objectdetection_ssd_amd import ops
    M, C, ld = shape
    c = exact(M, C, mode, p, hw_of(M))
    pow2 = M & (M - 1) == 0
    lds = (ld + 4, ld, ld + 8)
    dyd, xd = dev(c["dy"], lds[0]), dev(c["x"], lds[1])
    dy0 = dyd.clone()
    dv = {k: vec(c[k]) for k in ("mean", "invstd", "gamma")}
    nan = lambda: torch.full((C,), float("nan"), device="cuda")                            # noqa: E731

    def check_dx(dx, gamma, relu_mask):
        _, _, want = R.bwd_ref(c["dy"], c["x"], c["mean"], c["invstd"], gamma, c["factor"], relu_mask)
        got = host(dx, C)
        if pow2:
            assert np.array_equal(got, want)
        else:
            assert (np.abs(got - want) <= R.dx_bar(c["dy"], c["x"], c["mean"], c["invstd"], gamma, c["factor"])).all()
            if relu_mask:
                assert not got[~(c["x"] > 0)].any()
        assert pad_intact(dx, C)

    sg, sgx, _ = R.bwd_ref(c["dy"], c["x"], c["mean"], c["invstd"], c["gamma"], c["factor"])
    kept = {}
    for relu_mask in (False, True):
        dg, db = nan(), nan()
        dx, sums = run_bwd(ops, dyd, xd, C, dv, lds, c["drop"], relu_mask, dg=dg, db=db)
        assert np.array_equal(host(sums), np.stack([sg, sgx])), relu_mask
        assert np.array_equal(host(db), sg) and np.array_equal(host(dg), sgx)
        check_dx(dx, c["gamma"], relu_mask)
        kept[relu_mask] = (dx, sums)
    dx1, sums1 = kept[True]
    # gamma absent: 1
    dxg, sums = run_bwd(ops, dyd, xd, C, dv, lds, c["drop"], True, gamma=False)
    assert same_bits(sums, sums1)
    check_dx(dxg, None, True)
    # accumulate onto integers; no dx wanted: the same sums
    rng = np.random.default_rng(C)
    g0, b0 = rng.integers(-100, 101, C).astype(np.float64), rng.integers(-100, 101, C).astype(np.float64)
    assert R.is_f32(g0 + sgx) and R.is_f32(b0 + sg)
    dg, db = vec(g0), vec(b0)
    none, sums = run_bwd(ops, dyd, xd, C, dv, lds, c["drop"], True, dg=dg, db=db, accumulate=True, want_dx=False)
    assert none is None and same_bits(sums, sums1)
    assert np.array_equal(host(dg), g0 + sgx) and np.array_equal(host(db), b0 + sg)
    assert same_bits(dyd, dy0)
    # dx written over dy: the bits of the out-of-place call
    dxa, sums = run_bwd(ops, dyd, xd, C, dv, (lds[0], lds[1], lds[0]), c["drop"], True, dx=dyd)
    assert dxa is dyd and same_bits(sums, sums1) and same_bits(dyd[:, :C], dx1[:, :C]) and pad_intact(dyd, C)


def test_chained_stats_apply_backward_against_f64_autograd():
    """the kernels' own mean and invstd feed the backward; dx per channel against f64 autograd of F.batch_norm, held to 5 times the
    error of torch's CPU f32 autograd on the same data, the yardstick and margin of test_resnet34_train.py"""
    from objectdetection_ssd_amd import ops
    M, C, ld = 1367, 12, 32
    rng = np.random.default_rng(21)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)                              # noqa: E731
    x, dy = f(M, C) * 2 + 0.5, f(M, C)
    gamma, beta = (rng.random(C) + 0.5).astype(np.float32), f(C) * 0.1

    def autograd(dtype):
        xs, g, b = (torch.from_numpy(v).to(dtype).requires_grad_(True) for v in (x, gamma, beta))
        y = F.batch_norm(xs, None, None, g, b, True, MOM, EPS)
        (y * torch.from_numpy(dy).to(dtype)).sum().backward()
        return [t.detach().double().numpy() for t in (y, xs.grad, g.grad, b.grad)]

    y64, dx64, dg64, db64 = autograd(torch.float64)
    y32, dx32, dg32, db32 = autograd(torch.float32)
    xd, dyd = dev(x, ld), dev(dy, ld + 4)
    st = ops.bn_train_stats(xd, C, vec(gamma), vec(beta), EPS, MOM, None, None, None, ld=ld)
    y = ops.bn_apply(xd, C, st[2], st[3], out=sentinel(M, ld + 8).cuda(), ld=ld, out_ld=ld + 8)
    dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    dx, _ = ops.bn_train_bwd(dyd, xd, C, st[0], st[1], vec(gamma), None, False, dg, db, dx=sentinel(M, ld + 12).cuda(), ld_dy=ld + 4,
                             ld_x=ld, ld_dx=ld + 12)
    err, e32 = np.abs(host(dx, C) - dx64).max(0), np.abs(dx32 - dx64).max(0)
    print(f"chained dx: kernel error per channel {err}\n  torch f32 error {e32}\n  largest ratio {float((err / e32).max()):.3g}")
    assert (err <= 5 * e32).all()
    # one number per channel: a single channel's f32 error can be zero by chance, so the yardstick is the largest over the channels
    for name, got, ref, t32 in (("dgamma", host(dg), dg64, dg32), ("dbeta", host(db), db64, db32)):
        err, e32 = np.abs(got - ref), float(np.abs(t32 - ref).max())
        print(f"chained {name}: kernel error per channel {err}\n  largest torch f32 error {e32:.3g}, ratio {float(err.max()) / e32:.3g}")
        assert (err <= 5 * e32).all(), name
    assert pad_intact(y, C) and pad_intact(dx, C) and np.isfinite(host(y, C)).all()


# ---- the generator, materialised --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 4 * 1048576 + 20])            # one vector; 1,048,581 vectors: the first 5 threads take a second trip
def test_dropout_mask_equals_the_numpy_philox(n):
    from objectdetection_ssd_amd import ops
    for seed, site in ((SEED, 0), (SEED, 7), ((0xDEADBEEF << 32) | 0xCAFEF00D, 7)):
        for p in (0.0, 0.3, 1.0):
            got = ops.dropout_mask(n, p, seed, site, "cuda")
            assert got.shape == (n,) and got.dtype == torch.bool
            want = R.philox_keep(seed, site, n, p)
            assert np.array_equal(got.cpu().numpy(), want), (hex(seed), site, p)
            assert want.all() if p == 0 else not want.any() if p == 1 else abs(want.mean() - 0.7) < 5 * (0.21 / n) ** 0.5 or n == 4

"""The two F(4x4) transform kernels that WRITE planes -- wino4_input_kernel (B^T d B of the activation, + the ReLU bit words) and
wino4_dy_kernel (A dy A^T, optionally B^T dy B, optionally the bias partial sums; from dy or from a pooled gradient) -- request a thread's
whole patch up front through a buffer descriptor (csrc/winograd.hip).  What a thread computes did not change, so the checks are exact:

  * small-integer data (|x| <= 64) keeps every sum exact in f32 (largest |value| 64 * 10 * 10 < 2^24), and the planes must EQUAL the
    numpy restatement of the transforms below: maps with partial tiles on both edges and a one-tile map, 4 and 64 channels, a head-like
    row (Co = 100 in rows of 128), one dilated geometry, pooled sources in floor and ceil shape, planes / bias partials on and off;
  * with the block cap lowered so that every thread takes a second trip through its grid-stride loop, the same bits as without;
  * on randn data, the f64 transforms within the forward bound of the linear combination, computed in f64 from the inputs.

The forward wrapper takes channel counts that are multiples of 32 only (the plane GEMMs' rule), so the input planes and bit words are
checked at 32 and 64 channels; 4 and 8 channels run through the dy pass, whose dgrad planes are the same B^T d B."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BT = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]],
              np.float64)
AT = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64)


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _lattice_rows(size, d):
    """Image rows of the six patch rows of every tile row (-1: outside), tile rows numbered through the sub-lattices 0 .. d-1."""
    rows = []
    for off in range(min(d, size)):
        n_lat = (size - off + d - 1) // d
        for t in range((n_lat + 3) // 4):
            lat = [4 * t - 1 + a for a in range(6)]
            rows.append([d * l + off if l >= 0 and d * l + off < size else -1 for l in lat])
    return np.array(rows)


def _patches(x, d=1):
    """x (N,H,W,C) -> the 6x6 patches of all tiles, (tiles, 6, 6, C) f64, zeros outside the map; tiles ordered (n, th, tw)."""
    n, h, w, c = x.shape
    rh, rw = _lattice_rows(h, d), _lattice_rows(w, d)
    xp = np.zeros((n, h + 1, w + 1, c), np.float64)           # row / column -1 of the index arrays lands on the zero border
    xp[:, :h, :w] = x
    p = xp[:, rh[:, None, :, None], rw[None, :, None, :]]     # (n, TH, TW, 6, 6, c)
    return p.reshape(-1, 6, 6, c)


def _planes(p, left, right):
    """p (tiles, r, s, C) -> planes [a*6+b][tile][c] = sum over r, s of left[a][r] p[r][s] right[b][s], in f64."""
    out = np.einsum("ar,trsc,bs->abtc", left, p, right)
    return out.reshape(36, p.shape[0], p.shape[3])


def input_planes(x, d=1):
    return _planes(_patches(x, d), BT, BT)                    # B^T d B


def dy_planes(dy, d=1):
    return _planes(_patches(dy, d)[:, 1:5, 1:5], AT.T, AT.T)  # A dy A^T of the 4x4 block = the patch's interior


def relu_words(x, d=1):
    """One word per (tile, channel quad): bit (a*4+b)*4+e = interior element (a, b), channel 4*quad+e, > 0."""
    p = _patches(x, d)[:, 1:5, 1:5] > 0                       # (tiles, 4, 4, C)
    t, c = p.shape[0], p.shape[3]
    bits = p.reshape(t, 16, c // 4, 4).transpose(0, 2, 1, 3).reshape(t, c // 4, 64).astype(np.uint64)
    return (bits << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64).view(np.int64)


def unpool(dpool, codes, gate, h, w):
    """The gradient a 2x2 / stride-2 max pool hands its input: the gated pooled gradient at the window position the code names."""
    n, hp, wp, c = dpool.shape
    dy = np.zeros((n, 2 * hp, 2 * wp, c), np.float64)
    g = np.where(gate > 0, dpool, 0.0)
    for code in range(4):
        dy[:, code // 2::2, code % 2::2] = np.where(codes == code, g, 0.0)
    return dy[:, :h, :w]


def _ints(rng, shape, lim=64):
    return rng.integers(-lim, lim + 1, size=shape).astype(np.float32)


def _pooled_source(rng, n, h, w, c, hp, wp, ints=True):
    """(dpool, codes, gate) with all four codes and gates of both signs; at a ragged edge a code stays inside the map, as a pool leaves it."""
    dpool = _ints(rng, (n, hp, wp, c)) if ints else rng.standard_normal((n, hp, wp, c)).astype(np.float32)
    gate = _ints(rng, (n, hp, wp, c), 3)
    codes = rng.integers(0, 4, size=(n, hp, wp, c)).astype(np.uint8)
    if 2 * hp > h:
        codes[:, -1] &= 1
    if 2 * wp > w:
        codes[:, :, -1] &= 2
    assert set(np.unique(codes)) == {0, 1, 2, 3} and (gate > 0).any() and (gate <= 0).any()
    return dpool, codes, gate


def _bias_blocks(tiles, c4):
    """Blocks of a dy pass with bias partial sums: its threads in blocks of 256 (whole periods of the channel quads: c4 divides 256 here)."""
    assert 256 % c4 == 0
    return max(1, (tiles * c4 + 255) // 256)


def _run_dy(src, g, ldy, vd, bias):
    from objectdetection_ssd_amd import ops
    Y, Vd, part = ops.wino_dy_transform(src, g, ldy, vd, bias)
    torch.cuda.synchronize()
    return Y.cpu().numpy(), None if Vd is None else Vd.cpu().numpy(), None if part is None else part.cpu().numpy()


def _check_dy_exact(src, dy_np, g, ldy, co, d=1):
    """All four (dgrad planes, bias) forms of the pass against the restatement of dy_np (N,H,W,ldy), exactly."""
    y_ref, v_ref = dy_planes(dy_np, d), input_planes(dy_np, d)
    tiles = y_ref.shape[1]
    for vd in (True, False):
        for bias in (True, False):
            Y, Vd, part = _run_dy(src, g, ldy, vd, bias)
            assert np.array_equal(Y, y_ref.astype(np.float32)), f"A dy A^T (dgrad planes {vd}, bias {bias})"
            assert (Vd is not None) == vd and (part is not None) == bias
            if vd:
                assert np.array_equal(Vd, v_ref.astype(np.float32)), f"B^T dy B (bias {bias})"
            if bias:
                blocks, ldp = _bias_blocks(tiles, ldy // 4), (co + 3) // 4 * 4
                sums = part[:blocks * ldp].reshape(blocks, ldp)[:, :co].astype(np.float64).sum(0)
                assert np.array_equal(sums, dy_np[..., :co].sum((0, 1, 2))), f"bias partial sums (dgrad planes {vd})"


MAPS = [(4, 4), (5, 7), (10, 10), (7, 7)]


@pytest.mark.parametrize("c", [32, 64])
@pytest.mark.parametrize("hw", MAPS)
def test_input_planes_and_relu_words_equal_the_restatement(hw, c):
    from objectdetection_ssd_amd import ops
    dev = _dev()
    (h, w), n = hw, 2
    rng = np.random.default_rng(h * 100 + w + c)
    x = _ints(rng, (n, h, w, c))
    g = ops.make_geom(n, h, w, c, 32, 3, 1, 1, 1)
    uf, _ = ops.wino_weights(torch.zeros(32, c, 3, 3, device=dev), want_bwd=False, mo=4)
    _, planes, bits = ops.conv2d_fwd_wino(torch.from_numpy(x).to(dev), uf, None, g, False, keep_planes=True, want_bits=True)
    assert np.array_equal(planes.cpu().numpy(), input_planes(x).astype(np.float32))
    assert np.array_equal(bits.cpu().numpy(), relu_words(x))


def test_input_planes_on_the_sub_lattices_of_a_dilated_map():
    from objectdetection_ssd_amd import ops
    dev = _dev()
    n, h, w, c, d = 2, 19, 19, 32, 4                          # fc6's geometry
    x = _ints(np.random.default_rng(19), (n, h, w, c))
    g = ops.make_geom(n, h, w, c, 32, 3, 1, d, d)
    uf, _ = ops.wino_weights(torch.zeros(32, c, 3, 3, device=dev), want_bwd=False, mo=4)
    _, planes, bits = ops.conv2d_fwd_wino(torch.from_numpy(x).to(dev), uf, None, g, False, keep_planes=True, want_bits=True)
    assert planes.shape[1] == n * _lattice_rows(h, d).shape[0] * _lattice_rows(w, d).shape[0]
    assert np.array_equal(planes.cpu().numpy(), input_planes(x, d).astype(np.float32))
    assert np.array_equal(bits.cpu().numpy(), relu_words(x, d))


@pytest.mark.parametrize("c", [4, 64])
@pytest.mark.parametrize("hw", MAPS)
def test_dy_planes_and_bias_partials_equal_the_restatement(hw, c):
    from objectdetection_ssd_amd import ops
    (h, w), n = hw, 2
    dy = _ints(np.random.default_rng(h * 100 + w + c + 1), (n, h, w, c))
    g = ops.make_geom(n, h, w, 32, c, 3, 1, 1, 1)
    _check_dy_exact(torch.from_numpy(dy).to(_dev()), dy, g, c, c)


def test_dy_pass_on_a_head_like_row():
    """Co = 100 in rows of 128: the pass transforms all 128 columns, the partial sums cover the 100."""
    from objectdetection_ssd_amd import ops
    n, h, w, co, ld = 2, 5, 7, 100, 128
    dy = _ints(np.random.default_rng(100), (n, h, w, ld))
    _check_dy_exact(torch.from_numpy(dy).to(_dev()), dy, ops.make_geom(n, h, w, 32, co, 3, 1, 1, 1), ld, co)


def test_dy_pass_on_the_sub_lattices_of_a_dilated_map():
    from objectdetection_ssd_amd import ops
    n, h, w, c, d = 2, 19, 19, 8, 4
    dy = _ints(np.random.default_rng(8), (n, h, w, c))
    _check_dy_exact(torch.from_numpy(dy).to(_dev()), dy, ops.make_geom(n, h, w, 32, c, 3, 1, d, d), c, c, d)


@pytest.mark.parametrize("c", [4, 64])
@pytest.mark.parametrize("hw,hp", [((10, 10), (5, 5)), ((7, 7), (4, 4))])
def test_dy_pass_from_a_pooled_gradient_equals_the_restatement(hw, hp, c):
    """Hp = H/2 and Hp = (H+1)/2 (ceil mode: the last cells hang over the map's edge)."""
    from objectdetection_ssd_amd import ops
    dev = _dev()
    (h, w), n = hw, 2
    dpool, codes, gate = _pooled_source(np.random.default_rng(h + c), n, h, w, c, *hp)
    src = ops.PooledGrad(torch.from_numpy(dpool).to(dev), torch.from_numpy(codes).to(dev), torch.from_numpy(gate).to(dev), (n, h, w, c))
    _check_dy_exact(src, unpool(dpool, codes, gate, h, w), ops.make_geom(n, h, w, 32, c, 3, 1, 1, 1), c, c)


def test_every_thread_loops_and_the_bits_stay():
    """2 x 40 x 40 x 512 is 25 600 (tile, channel quad) pairs; under a cap of 64 blocks 16 384 threads share them."""
    from objectdetection_ssd_amd import _lib, ops
    dev = _dev()
    n, h, w, c = 2, 40, 40, 512
    rng = np.random.default_rng(512)
    x = torch.from_numpy(_ints(rng, (n, h, w, c))).to(dev)
    dpool, codes, gate = _pooled_source(rng, n, h, w, c, 20, 20)
    pooled = ops.PooledGrad(torch.from_numpy(dpool).to(dev), torch.from_numpy(codes).to(dev), torch.from_numpy(gate).to(dev), (n, h, w, c))
    g = ops.make_geom(n, h, w, c, 32, 3, 1, 1, 1)
    gd = ops.make_geom(n, h, w, 32, c, 3, 1, 1, 1)
    uf, _ = ops.wino_weights(torch.zeros(32, c, 3, 3, device=dev), want_bwd=False, mo=4)

    def run():
        out = list(ops.conv2d_fwd_wino(x, uf, None, g, False, keep_planes=True, want_bits=True)[1:])
        for src in (x, pooled):
            for vd in (True, False):
                Y, Vd, part = ops.wino_dy_transform(src, gd, c, vd, True)
                out += [Y, part] + ([Vd] if vd else [])
        torch.cuda.synchronize()
        return out

    lib = _lib.load()
    try:
        _lib.check(lib.ssd_tune_set_wino_xform_blocks(64), "tune")
        capped = run()
    finally:
        _lib.check(lib.ssd_tune_set_wino_xform_blocks(8192), "tune")
    free = run()
    tiles, c4 = n * 10 * 10, c // 4
    for k, (a, b) in enumerate(zip(capped, free)):
        if a.dim() == 1:                                      # bias partials: 64 rows against 100, the same exact column sums
            sa, sb = (t[:r * c].reshape(r, c).double().sum(0) for t, r in ((a, 64), (b, _bias_blocks(tiles, c4))))
            assert torch.equal(sa, sb), f"output {k}: bias partial sums"
        else:
            assert torch.equal(a, b), f"output {k}"
    assert torch.equal(free[0], torch.from_numpy(input_planes(x.cpu().numpy()).astype(np.float32)).to(dev))


@functools.lru_cache(maxsize=None)
def _float_case(h, w):
    rng = np.random.default_rng(h * 10 + w)
    n, c = 2, 64
    x = rng.standard_normal((n, h, w, c)).astype(np.float32)
    hp, wp = (h + 1) // 2, (w + 1) // 2
    return x, _pooled_source(rng, n, h, w, c, hp, wp, ints=False)


def _within_forward_bound(got, p, left, right, what):
    """|got - exact| <= n * 2^-24 * sum |c| |x| per output, n = 12 roundings on the longest path (two stages of at most four fused
    multiply-adds, and headroom); exact and bound in f64 from the f32 inputs p (tiles, r, s, C)."""
    exact, mag = _planes(p, left, right), _planes(np.abs(p), np.abs(left), np.abs(right))
    err = np.abs(got.astype(np.float64) - exact)
    worst = float((err / np.maximum(mag, 1e-300)).max())
    print(f"{what}: max err / sum|c||x| = {worst:.3e} (bound {12 * 2.0 ** -24:.3e})")
    assert (err <= 12 * 2.0 ** -24 * mag).all(), what


@pytest.mark.parametrize("hw", [(5, 7), (10, 10)])
def test_float_planes_within_the_forward_bound_of_the_f64_transforms(hw):
    from objectdetection_ssd_amd import ops
    dev = _dev()
    (h, w), n, c = hw, 2, 64
    x, (dpool, codes, gate) = _float_case(h, w)
    g = ops.make_geom(n, h, w, c, 32, 3, 1, 1, 1)
    uf, _ = ops.wino_weights(torch.zeros(32, c, 3, 3, device=dev), want_bwd=False, mo=4)
    _, planes = ops.conv2d_fwd_wino(torch.from_numpy(x).to(dev), uf, None, g, False, keep_planes=True)
    _within_forward_bound(planes.cpu().numpy(), _patches(x), BT, BT, "B^T d B")
    gd = ops.make_geom(n, h, w, 32, c, 3, 1, 1, 1)
    pooled = ops.PooledGrad(torch.from_numpy(dpool).to(dev), torch.from_numpy(codes).to(dev), torch.from_numpy(gate).to(dev), (n, h, w, c))
    for name, src, dy in (("dy", torch.from_numpy(x).to(dev), x), ("pooled dy", pooled, unpool(dpool, codes, gate, h, w))):
        Y, Vd, _ = _run_dy(src, gd, c, True, False)
        _within_forward_bound(Y, _patches(dy)[:, 1:5, 1:5], AT.T, AT.T, f"A dy A^T ({name})")
        _within_forward_bound(Vd, _patches(dy), BT, BT, f"B^T dy B ({name})")

"""What tests/test_photometric_kernels_gpu.py leans on, checked without a GPU: the properties tests/photometric_cases.py builds its
images for, and the oracle's photometric_apply against Pillow itself on the regimes those cases add -- ImageEnhance.Color over all
2^24 colours, ImageEnhance.Contrast and ImageEnhance.Brightness on every pivot and tie image at every alpha of the cases, the
blend's edges 0.0 and the float32 next above 1.0 among them."""
import numpy as np
import pytest

import photometric_cases as PC
import ssd_oracle as O


def test_every_pivot_is_reached_with_all_values_present():
    imgs = PC.pivot_images()
    assert len(imgs) == 256
    for m, a in enumerate(imgs):
        assert (a[..., 0] == a[..., 1]).all() and (a[..., 0] == a[..., 2]).all()
        lum = O.rgb_to_l(a)
        assert np.array_equal(lum, a[..., 0])
        assert int(float(lum.astype(np.int64).sum()) / float(lum.size) + 0.5) == m
        if 1 <= m <= 254:
            assert np.array_equal(np.unique(a), np.arange(256)), m
    assert sum(a.shape[0] * a.shape[1] for a in imgs) < 1 << 20          # the whole batch stays small
    case = PC.pivots(PC.CONTRAST, 0.5)
    assert len(case.images) == 256 and all(o == ((PC.CONTRAST, 0.5),) for o in case.ops)


def test_ties_fall_as_stated():
    pairs = PC.tie_images()
    assert [a.shape[0] for a, _ in pairs] == [1000, 1000, 600, 600]
    k = PC.TIE_K
    for i, (a, p) in enumerate(pairs):
        n = a.shape[0] * a.shape[1]
        assert n > PC.BLOCK_CAP_PX
        s = int(O.rgb_to_l(a).astype(np.int64).sum())
        assert np.array_equal(np.unique(a), [k, k + 1])
        if i % 2 == 0:
            assert 2 * s == 2 * n * k + n and p == k + 1 and PC.pivot(a) == k + 1          # exactly k + 1/2
        else:
            assert 2 * s == 2 * n * k + n - 2 and p == k and PC.pivot(a) == k              # one count below it
    exp = PC.ties(0.5).expected()
    for i, e in enumerate(exp):                                       # the two pivots give different images
        assert np.array_equal(np.unique(e), [100, 101] if i % 2 == 0 else [100]), i


def test_mixed_batch_covers_what_it_claims():
    case = PC.mixed()
    px = [a.shape[0] * a.shape[1] for a in case.images]
    for n in (1, 7, 257, 1023, 1024, 1025, 511 * 513, 512 * 512, 512 * 513):
        assert n in px
    assert [a.shape[:2] for a in case.images].count((1, 7)) == 1 and [a.shape[:2] for a in case.images].count((7, 1)) == 1
    assert 511 * 513 < PC.BLOCK_CAP_PX == 512 * 512 < 512 * 513
    assert (511 * 513 + 1023) // 1024 == 256 and (512 * 512 + 1023) // 1024 == 256 and (512 * 513 + 1023) // 1024 == 257
    assert {len(o) for o in case.ops} == {0, 1, 2, 3, 4}
    assert {(k, s) for o in case.ops for s, (k, _) in enumerate(o)} == {(k, s) for k in range(4) for s in range(4)}
    contrast_at = [tuple(s for s, (k, _) in enumerate(o) if k == PC.CONTRAST) for o in case.ops]
    assert {c[0] for c in contrast_at if len(c) == 1} == {0, 1, 2, 3} and any(len(c) == 2 for c in contrast_at)
    assert px[[len(o) for o in case.ops].index(0)] == 1 and any(len(o) == 0 and n == 512 * 512 for o, n in zip(case.ops, px))
    for a, o, e in zip(case.images, case.ops, case.expected()):
        if not o:
            assert np.array_equal(a, e)
    assert any((a[..., 0] == a[..., 1]).all() and (a[..., 0] == a[..., 2]).all() and a.shape[0] > 1 for a in case.images)
    assert any(a.shape[0] > 1 and int(a.max()) - int(a.min()) < 16 for a in case.images)


def test_cube_holds_every_colour_once():
    a = PC.cube_image()
    assert a.shape == (4096, 4096, 3) and a.shape[0] * a.shape[1] == 64 * 256 * 1024
    flat = a.reshape(-1, 3).astype(np.uint32)
    assert np.array_equal((flat[:, 0] << 16) | (flat[:, 1] << 8) | flat[:, 2], np.arange(1 << 24, dtype=np.uint32))
    assert [O.hue_delta_u8(f) for k, f in PC.CUBE_OPS if k == PC.HUE] == [7, 238]


def test_layout_guards_and_descriptors():
    case = PC.mixed()
    host, descs, photo, slots = PC.layout(case)
    outside = PC.outside_mask(host.size, slots)
    assert (host[outside] == PC.PATTERN).all()
    end = 0
    for d, p, a, o, (so, h, w) in zip(descs, photo, case.images, case.ops, slots):
        assert so % 2 == 1 and so - end >= PC.GUARD and (h, w) == a.shape[:2]
        end = so + a.size
        assert np.array_equal(host[so:end].reshape(a.shape), a)
        assert (d.src_offset, d.src_h, d.src_w, d.crop_h, d.crop_w, d.canvas_h, d.canvas_w) == (so, h, w, h, w, h, w)
        assert p.n_ops == len(o)
        for k, (kind, f) in enumerate(o):
            assert p.kind[k] == kind and p.alpha[k] == np.float32(f)
            assert p.hue_delta[k] == ((int(f * 255) & 0xFF) if kind == PC.HUE else 0)
    assert host.size - end >= PC.GUARD


@pytest.mark.parametrize("factor", [0.5, 1.5, 0.999])
def test_oracle_saturation_equals_pillow_on_every_colour(factor):
    from PIL import Image, ImageEnhance
    cube = PC.cube_image()
    for q in range(4):                                                # 2^22 colours at a time
        a = cube[q * 1024:(q + 1) * 1024]
        ref = np.asarray(ImageEnhance.Color(Image.fromarray(a)).enhance(factor))
        assert np.array_equal(O.photometric_apply(a, [(PC.SATURATION, factor)]), ref), (factor, q)


@pytest.mark.parametrize("alpha", PC.ALPHAS)
def test_oracle_contrast_and_brightness_equal_pillow_on_pivots_and_ties(alpha):
    """ImageEnhance takes any factor; Image.blend interpolates on [0, 1] and clips outside it.  0.0 and the float32 next above 1.0
    are the edges of that choice: Pillow's own answer is the expected value there as everywhere."""
    from PIL import Image, ImageEnhance
    for m, a in enumerate(PC.pivot_images() + [t for t, _ in PC.tie_images()]):
        im = Image.fromarray(a)
        assert np.array_equal(O.photometric_apply(a, [(PC.CONTRAST, alpha)]), np.asarray(ImageEnhance.Contrast(im).enhance(alpha))), (m, alpha)
        assert np.array_equal(O.photometric_apply(a, [(PC.BRIGHTNESS, alpha)]), np.asarray(ImageEnhance.Brightness(im).enhance(alpha))), (m, alpha)

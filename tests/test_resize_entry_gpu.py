"""ssd_preprocess_u8 (csrc/preprocess.hip, the batch entry) taken bare through ops.preprocess_u8 with small outputs: every axis ratio
up to the 31:1 tap bound against Pillow itself, the batch-wide tap stride / max_in_h / [B][2][out_max] bookkeeping against one-image
calls, canvas / crop / flip geometry against the oracle's composition, and the refusal above 31:1.  Every comparison is an equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import resize_cases as RC
import ssd_oracle as O

pytestmark = pytest.mark.gpu

FILLER = tuple(int(v) for v in O.mean_filler_u8())


def _run(items, out_hw):
    from objectdetection_ssd_amd import ops
    host, descs = RC.layout(items)
    arena = torch.from_numpy(host.copy()).cuda()
    out = ops.preprocess_u8(arena, descs, out_hw, O.IMAGENET_MEAN, O.IMAGENET_STD, FILLER)
    assert tuple(out.shape) == (len(items), 3) + tuple(out_hw) and out.dtype == torch.float32
    res = out.cpu().numpy()
    assert np.array_equal(arena.cpu().numpy(), host)                  # the sources are read only
    return res


def _diff(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} of {got.size} values differ; first at {bad[0].tolist()}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"


@pytest.mark.parametrize("src,out_hw", RC.RATIOS, ids=[f"{s[0]}x{s[1]}_to_{o[0]}x{o[1]}" for s, o in RC.RATIOS])
def test_ratios_equal_pillow(src, out_hw):
    img = RC.image(11, *src)
    got = _run([RC.Item(img)], out_hw)[0]
    want = RC.pillow(img, out_hw)
    assert np.array_equal(got, want), _diff(got, want)
    assert np.array_equal(RC.oracle(RC.Item(img), out_hw), want)


def test_ratio_cases_reach_the_tap_bound():
    ks = {RC.ksize(s[axis], o[axis]) for s, o in RC.RATIOS for axis in (0, 1)}
    assert ks == {3, 5, 7, 11, 63} and RC.ksize(248, 8) == 63 and RC.ksize(249, 8) == 65


def test_batch_wide_strides_equal_one_image_calls():
    """The ks = 63 image, a ks = 3 image (57 zero coefficients behind its taps), the tallest crop and a one-row crop in one batch: the
    shared tap stride and max_in_h give every image what a call of its own gives it, which is the oracle's."""
    items = [RC.Item(RC.image(20 + i, h, w)) for i, (h, w) in enumerate(RC.STRIDE_SHAPES)]
    ks = [max(RC.ksize(h, RC.STRIDE_OUT[0]), RC.ksize(w, RC.STRIDE_OUT[1])) for h, w in RC.STRIDE_SHAPES]
    assert ks[0] == 63 and ks[1] == 3 and max(h for h, _ in RC.STRIDE_SHAPES) == RC.STRIDE_SHAPES[2][0] and RC.STRIDE_SHAPES[3][0] == 1
    alone = [_run([it], RC.STRIDE_OUT)[0] for it in items]
    for it, a in zip(items, alone):
        want = RC.oracle(it, RC.STRIDE_OUT)
        assert np.array_equal(a, want), (it.img.shape, _diff(a, want))
    batch = _run(items, RC.STRIDE_OUT)
    flipped = _run(items[::-1], RC.STRIDE_OUT)[::-1]                   # the same images in the other order
    for it, a, b, f in zip(items, alone, batch, flipped):
        assert np.array_equal(b, a), (it.img.shape, _diff(b, a))
        assert np.array_equal(f, a), (it.img.shape, _diff(f, a))
    assert np.array_equal(batch, _run(items, RC.STRIDE_OUT))           # and repeats bitwise


@pytest.mark.parametrize("out_hw", RC.NONSQUARE_OUTS, ids=[f"{h}x{w}" for h, w in RC.NONSQUARE_OUTS])
def test_non_square_outputs(out_hw):
    """out_max = max(out_h, out_w) strides the coefficient rows of both axes."""
    items = [RC.Item(RC.image(30 + i, h, w)) for i, (h, w) in enumerate(RC.NONSQUARE_SHAPES)]
    got = _run(items, out_hw)
    for i, it in enumerate(items):
        want = RC.oracle(it, out_hw)
        assert np.array_equal(got[i], want), (it.img.shape, _diff(got[i], want))
        assert np.array_equal(want, RC.pillow(it.img, out_hw))


def test_geometry_equals_the_composition():
    """Windows wholly in the filler, over each side and two corners of the source, 1 x 1 crops, flips of odd and even widths."""
    items = RC.geometry_items()
    got = _run(items, RC.GEOM_OUT)
    for i, it in enumerate(items):
        want = RC.oracle(it, RC.GEOM_OUT)
        assert np.array_equal(got[i], want), (it.canvas, it.crop, it.flip, _diff(got[i], want))
    in_filler = RC.oracle(items[0], RC.GEOM_OUT)
    for c in range(3):                                               # a window in the filler is the normalised filler
        assert (in_filler[c] == in_filler[c, 0, 0]).all()


def test_refusal_above_31_to_1():
    """A 249 -> 8 axis has support 31.125: the workspace query answers 0, ops.preprocess_u8 raises, and the C entry, handed an ample
    workspace, refuses before any kernel runs: its output buffer keeps what it held."""
    from objectdetection_ssd_amd import _lib, ops
    lib = _lib.load()
    for shape in ((249, 8), (8, 249)):
        items = [RC.Item(RC.image(40, 8, 8)), RC.Item(RC.image(41, *shape))]
        host, descs = RC.layout(items)
        arena = torch.from_numpy(host.copy()).cuda()
        with pytest.raises(ValueError):
            ops.preprocess_u8(arena, descs, (8, 8), O.IMAGENET_MEAN, O.IMAGENET_STD, FILLER)
        assert lib.ssd_preprocess_workspace(C.byref(descs), 2, 8, 8) == 0
        assert lib.ssd_preprocess_workspace(C.byref(descs), 1, 8, 8) > 0          # the first image alone is fine
        out = torch.full((2, 3, 8, 8), -7.0, device="cuda")
        ws = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device="cuda")
        d_dev = torch.from_numpy(np.frombuffer(bytes(descs), dtype=np.uint8).copy()).cuda()
        m = (C.c_float * 3)(*O.IMAGENET_MEAN); s = (C.c_float * 3)(*O.IMAGENET_STD); f = (C.c_uint8 * 3)(*FILLER)
        status = lib.ssd_preprocess_u8(arena.data_ptr(), d_dev.data_ptr(), C.byref(descs), 2, 8, 8, C.addressof(m), C.addressof(s),
                                       C.addressof(f), out.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert status == -1                                          # SSD_ERR_BAD_SHAPE
        assert bool((out == -7.0).all()) and bool((ws == 0x5A).all())
        assert np.array_equal(arena.cpu().numpy(), host)

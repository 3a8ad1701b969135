"""The greedy NMS kernel and the cross-class top-k of the default decode, each alone on made-up inputs (ssd_nms_sorted,
ssd_topk_emit_sorted: the production launchers, nothing forced) against the numpy reference (tests/hard_nms_ref.py), bit for bit: the
rule is +, -, x, /, min and max in f32, the top-k compares bit patterns, so there is no tolerance to set.  Every greedy case
computes from ssd_nms_plan whether its largest class is resolved in 64- or 32-row chunks and asserts the mode it means to test.
Then a few decodes end to end (Losses.inference_batch against O.decode_nms) in regimes random logits do not reach, on inputs whose
reference decisions have the margins the other decode tests ask for (asserted first, on the reference alone)."""
import ctypes

import numpy as np
import pytest
import torch

import hard_nms_ref as H
import soft_nms_ref as S
import ssd_oracle as O
from nms_cases import lattice_image, lattice_pair, near_threshold_pairs, pack, random_class, tied_image, undertrained_image

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _lib():
    from objectdetection_ssd_amd import _lib
    return _lib.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- the greedy kernel, bare ---------------------------------------------------------------------------------------------------
def chunk_rows(B, C1, P, n):
    """rows per chunk for a class of n candidates in a (B, C1, P) launch, and the launch's block size -- from the library's plan"""
    t, w = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _lib().ssd_nms_plan(B, C1, P, ctypes.byref(t), ctypes.byref(w)) == 0
    return (64 if 64 * ((n + 63) // 64) <= w.value else 32), t.value


def run_nms(s_boxes, s_prob, cnt, thr):
    B, C1, P = s_prob.shape
    d_boxes, d_prob, d_cnt = _t(s_boxes), _t(s_prob), _t(cnt)
    kept_pos = torch.full((B, C1, P), -1, device=DEV, dtype=torch.int32)
    kept_prob = torch.full((B, C1, P), -1.0, device=DEV, dtype=torch.float32)
    kept_cnt = torch.full((B, C1 + 1), -1, device=DEV, dtype=torch.int32)
    rc = _lib().ssd_nms_sorted(d_boxes.data_ptr(), d_prob.data_ptr(), d_cnt.data_ptr(), B, C1, P, thr, kept_pos.data_ptr(),
                               kept_prob.data_ptr(), kept_cnt.data_ptr(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return kept_pos.cpu().numpy(), kept_prob.cpu().numpy(), kept_cnt.cpu().numpy()


def check_nms(classes, B, C1, P, thr=0.45, rows=None, threads=None, refs=None):
    """classes[b][c] = (boxes, scores) -> the kernel's output equals greedy_nms_sorted for every (image, class): count, positions,
    the probability bits of the kept positions, sentinels past the count (the input slots past a class's count are poisoned by
    pack()).  rows / threads: the chunk mode of the largest class and the block size this case is meant to run in.
    -> survivors per (image, class)"""
    n_max = max(len(classes[b][c][1]) for b in range(B) for c in range(C1))
    mode = chunk_rows(B, C1, P, n_max)
    if rows is not None:
        assert mode[0] == rows, (mode, n_max)
    if threads is not None:
        assert mode[1] == threads, mode
    s_boxes, s_prob, cnt = pack(classes, B, C1, P)
    kp, kq, kc = run_nms(s_boxes, s_prob, cnt, thr)
    assert (kc[:, C1] == -1).all()                                  # the (C1 + 1)-th counter of an image is not the kernel's
    kept = np.zeros((B, C1), np.int64)
    for b in range(B):
        for c in range(C1):
            bx, sc = classes[b][c]
            ref = refs[b][c] if refs is not None else H.greedy_nms_sorted(bx, sc, thr)
            k = ref.shape[0]
            kept[b, c] = k
            assert kc[b, c] == k, (b, c, int(kc[b, c]), k)
            assert np.array_equal(kp[b, c, :k], ref), (b, c, np.nonzero(kp[b, c, :k] != ref)[0][:8])
            assert np.array_equal(kq[b, c, :k].view(np.uint32), np.asarray(sc, np.float32)[ref].view(np.uint32)), (b, c)
            assert (kp[b, c, k:] == -1).all() and (kq[b, c, k:] == -1.0).all(), (b, c)      # nothing written past the survivors
    return kept


def among_small_classes(rng, cls, B, C1, b0, c0):
    """cls at (b0, c0), every other (image, class) with 0 - 3 candidates"""
    return [[cls if (b, c) == (b0, c0) else random_class(rng, int(rng.integers(0, 4)), size=(0.3, 0.6)) for c in range(C1)]
            for b in range(B)]


SWEEP = [0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2049]


@pytest.mark.parametrize("n", SWEEP)
def test_bare_greedy_at_each_size(n):
    """P = 2112, scores quantised to 1/64 (ties): the wide launch (one class, 1024 threads: the compaction loops in steps of 1024) and
    the batch launch (7 x 20 classes, 512 threads; the swept class among classes of 0 - 3 candidates); 64-row chunks in both"""
    rng = np.random.default_rng(300 + n)
    cls = random_class(rng, n, quantum=1 / 64)
    kept = check_nms([[cls]], 1, 1, 2112, rows=64, threads=1024)
    assert (kept[0, 0] > 0) == (n > 0) and (n < 100 or kept[0, 0] < n)
    b0, c0 = n % 7, (3 * n) % 20
    kept = check_nms(among_small_classes(rng, cls, 7, 20, b0, c0), 7, 20, 2112, rows=64, threads=512)
    assert (kept[b0, c0] > 0) == (n > 0)


BATCH_32 = [4608, 4609, 4640, 4641, 6000, 8732]


@pytest.mark.parametrize("size", [(0.05, 0.3), (0.3, 0.6)])
def test_bare_greedy_32_row_chunks_in_a_batch(size):
    """B = 7, C1 = 20, P = 8732 (512 threads, chunk_words 4608): one class per image with 4608 candidates -- the last size in 64-row
    chunks -- 4609 (the first in 32-row chunks), 4640 / 4641 (32-row chunks end with a full chunk / with one row in a chunk that
    starts at bit 32 of its word), 6000 and 8732 (ragged / every slot).  Small boxes leave hundreds of survivors; large boxes a
    few, so most rows are already removed when their chunk starts."""
    rng = np.random.default_rng(41 if size[0] < 0.1 else 42)
    B, C1, P = 7, 20, 8732
    assert [chunk_rows(B, C1, P, n)[0] for n in BATCH_32] == [64, 32, 32, 32, 32, 32]
    classes = [[random_class(rng, int(rng.integers(0, 4)), size=(0.3, 0.6)) for _ in range(C1)] for _ in range(B)]
    where = {}
    for b, n in enumerate(BATCH_32):
        where[b] = (3 * b + 1) % C1
        classes[b][where[b]] = random_class(rng, n, size=size, quantum=1 / 1024)
    kept = check_nms(classes, B, C1, P, rows=32, threads=512)
    k = [int(kept[b, where[b]]) for b in range(len(BATCH_32))]
    print("survivors", k)
    assert all(100 < v < 3000 for v in k) if size[0] < 0.1 else all(5 < v < 100 for v in k)


@pytest.mark.parametrize("n", [17536, 17537, 20000])
def test_bare_greedy_32_row_chunks_single_image(n):
    """B = 1, C1 = 20, P = 24564 (1024 threads, chunk_words at the LDS cap, 17536): 17536 candidates still run 64-row chunks, 17537
    and 20000 run 32-row chunks"""
    rng = np.random.default_rng(n)
    B, C1, P = 1, 20, 24564
    classes = among_small_classes(rng, random_class(rng, n, size=(0.05, 0.3), quantum=1 / 4096), B, C1, 0, 13)
    kept = check_nms(classes, B, C1, P, rows=64 if n == 17536 else 32, threads=1024)
    print("survivors", int(kept[0, 13]))
    assert 100 < kept[0, 13] < 3000


def lattice_class(width, shift, interleaved):
    """64 lattice pairs (IoU exactly 0.5 or 0.25) in separate 8 x 8-cell tiles of the 64 x 64 lattice; partners next to each other
    (rows 2k, 2k + 1) or 64 rows apart (the second box in the next word)"""
    pairs = [lattice_pair(width, shift, x0=8 * (k % 8), y0=8 * (k // 8)) for k in range(64)]
    boxes = np.concatenate(pairs) if interleaved else np.concatenate([np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])])
    return boxes.astype(np.float32), np.linspace(0.9, 0.3, 128).astype(np.float32)


@pytest.mark.parametrize("width,shift,iou", [(3, 1, 0.5), (5, 3, 0.25)])
def test_bare_greedy_exact_equality_is_suppression(width, shift, iou):
    """IoU == thr exactly, every term representable: suppressed (>=); with thr one ulp above, kept"""
    above = float(np.nextafter(np.float32(iou), np.float32(2)))
    for interleaved in (True, False):
        boxes, sc = lattice_class(width, shift, interleaved)
        first = np.arange(0, 128, 2) if interleaved else np.arange(64)
        assert H.greedy_nms_sorted(boxes, sc, iou).tolist() == first.tolist()
        assert H.greedy_nms_sorted(boxes, sc, above).tolist() == list(range(128))
        for thr in (iou, above):
            check_nms([[(boxes, sc)]], 1, 1, 128, thr=thr)
            check_nms(among_small_classes(np.random.default_rng(1), (boxes, sc), 7, 20, 2, 9), 7, 20, 200, thr=thr, threads=512)


@pytest.mark.parametrize("thr", [0.45, 0.5, 0.1])
def test_bare_greedy_exact_division_decides(thr):
    """pairs whose inter / union lies within 1e-5 * thr of thr, on both sides: the kernel's fast comparison cannot decide them, the
    IEEE division must -- and must round as the reference's"""
    boxes = near_threshold_pairs(np.random.default_rng(int(thr * 100)), 144, thr)
    sc = np.linspace(0.95, 0.25, boxes.shape[0]).astype(np.float32)
    iou = np.asarray([S.iou_one_to_many(boxes[2 * k], boxes[2 * k + 1:2 * k + 2])[0] for k in range(144)], np.float64)
    near = np.abs(iou - float(np.float32(thr))) <= 1e-5 * thr
    hit = iou[near] >= float(np.float32(thr))
    print(f"thr {thr}: {int(near.sum())} pairs within 1e-5 thr, {int(hit.sum())} suppressed, nearest {np.min(np.abs(iou - np.float32(thr))):.2e}")
    assert near.sum() >= 64 and hit.sum() >= 8 and (~hit).sum() >= 8
    kept = check_nms([[(boxes, sc)]], 1, 1, 320, thr=thr, threads=1024)
    assert kept[0, 0] == 144 + int((iou < float(np.float32(thr))).sum())
    check_nms(among_small_classes(np.random.default_rng(2), (boxes, sc), 7, 20, 6, 19), 7, 20, 320, thr=thr, threads=512)


def degenerate_class(rng, n=200):
    boxes, scores = random_class(rng, n, size=(0.1, 0.4))
    boxes[5] = [0.4, 0.4, 0.4, 0.4]; boxes[6] = [0.4, 0.4, 0.4, 0.4]                      # empty, twice at one point (0 / 0)
    boxes[17] = [0.3, 0.2, 0.3, 0.9]                                                         # zero width
    boxes[40] = [0.6, 0.6, 0.2, 0.2]                                                         # inverted in both axes: area > 0
    boxes[41] = [0.6, 0.2, 0.2, 0.6]; boxes[42] = [0.6, 0.2, 0.2, 0.6]                      # inverted in x: negative area, twice
    boxes[70] = [0.2, 0.2, 0.2, 0.2]; boxes[199] = [0.7, 0.1, 0.7, 0.1]
    return boxes, scores


def test_bare_greedy_identical_and_degenerate_boxes():
    rng = np.random.default_rng(11)
    n = 200
    _, scores = random_class(rng, n)
    same = np.tile(np.asarray([[0.2, 0.3, 0.6, 0.8]], np.float32), (n, 1))
    assert check_nms([[(same, scores)]], 1, 1, 256, thr=1.0)[0, 0] == 1                      # a / ((a + a) - a) = 1 exactly, >= 1.0
    assert check_nms([[(same, scores)]], 1, 1, 256, thr=float(np.nextafter(np.float32(1), np.float32(2))))[0, 0] == n
    empty = np.tile(np.asarray([[0.4, 0.4, 0.4, 0.4]], np.float32), (n, 1))
    empty[100:] = [0.3, 0.2, 0.3, 0.9]
    for thr in (0.45, 0.0):
        assert check_nms([[(empty, scores)]], 1, 1, 256, thr=thr)[0, 0] == n                 # 0 / 0 = NaN: never >=, not even >= 0
    boxes, scores = degenerate_class(rng)
    ref = H.greedy_nms_sorted(boxes, scores, 0.45)
    assert {5, 6, 17, 70, 199} <= set(ref.tolist())                                          # IoU 0 or NaN with everything
    for thr in (0.45, 1e-30, 0.0):
        check_nms([[(boxes, scores)]], 1, 1, 256, thr=thr)
    check_nms(among_small_classes(rng, (boxes, scores), 7, 20, 0, 0), 7, 20, 256, threads=512)


@pytest.mark.parametrize("thr", [0.0, 1e-30, 1.0, 1.5, -0.1])
def test_bare_greedy_threshold_edges(thr):
    """the threshold goes to the kernel as the decode passes it, unchecked; iou >= thr in f32 is the answer.  At 0 and below every
    comparison takes the exact path (and IoU = 0 of disjoint boxes suppresses)."""
    rng = np.random.default_rng(23)
    cls = [[random_class(rng, int(rng.integers(0, 90)) * (c != 2), size=(0.2, 0.5)) for c in range(5)] for _ in range(3)]
    cls[1][4] = random_class(rng, 700, size=(0.05, 0.3), quantum=1 / 64)
    for dup, of in ((10, 3), (333, 300), (699, 64)):                   # three exact copies: IoU = 1, the only pairs that reach thr = 1
        cls[1][4][0][dup] = cls[1][4][0][of]
    cls[2][0] = degenerate_class(rng)
    kept = check_nms(cls, 3, 5, 704, thr=thr)
    k = int(kept[1, 4])
    if thr <= 0:
        assert k == 1
    elif thr >= 1:
        assert k == (700 if thr > 1 else 697)
    else:
        assert 1 < k < 697


def test_bare_greedy_non_finite_coordinates():
    """NaN coordinates, infinite extents (an overflowed exp(g / 5) times the prior's size) and both, in the first, a middle and the
    last chunk: ordinary inputs -- counts and indices stay in range -- whose IoU is NaN (never >=) or, for an infinite box against a
    finite one, 0"""
    nan, inf = np.float32("nan"), np.float32("inf")
    odd = [[nan, 0.1, 0.5, 0.5], [-inf, 0.2, inf, 0.6], [-inf, -inf, inf, inf], [nan, -inf, nan, inf], [0.1, 0.1, 0.5, nan],
           [0.3, -inf, 0.5, inf]]
    for n, P, B, C1, rows in ((300, 320, 1, 1, 64), (300, 320, 7, 20, 64), (4700, 8732, 7, 20, 32)):
        rng = np.random.default_rng(n + B)
        boxes, scores = random_class(rng, n, size=(0.1, 0.4) if n == 300 else (0.2, 0.5))
        last = (n - 1) // rows * rows
        mid = (n // 2) // rows * rows
        spots = [0, 3, 5, mid + 1, mid + rows - 1, mid + 2, last, n - 1, n - 2]
        for i, p in enumerate(spots):
            boxes[p] = odd[i % len(odd)]
        with np.errstate(all="ignore"):
            ref = H.greedy_nms_sorted(boxes, scores, 0.45)
        assert {0, 5, n - 1} <= set(ref.tolist())                        # NaN boxes survive whatever surrounds them
        classes = among_small_classes(rng, (boxes, scores), B, C1, B - 1, C1 - 1)
        for thr in (0.45, 0.0):
            check_nms(classes, B, C1, P, thr=thr, rows=rows)


def test_bare_greedy_255_classes_and_per_image_offsets():
    rng = np.random.default_rng(7)
    cls = [[random_class(rng, int(rng.integers(0, 4)), size=(0.3, 0.6)) for _ in range(255)]]
    assert check_nms(cls, 1, 255, 130, threads=512).sum() > 100
    cls = [[random_class(rng, int(rng.integers(0, 130)) * (c != 2), size=(0.2, 0.5)) for c in range(5)] for _ in range(3)]
    assert len({tuple(len(x[1]) for x in row) for row in cls}) == 3
    assert check_nms(cls, 3, 5, 130, threads=1024).sum() > 30
    cls = [[random_class(rng, int(rng.integers(0, 130)), size=(0.2, 0.5)) for c in range(255)] for _ in range(2)]
    assert check_nms(cls, 2, 255, 130, threads=512).sum() > 1000


# ---- the top-k, bare -------------------------------------------------------------------------------------------------------------
def split_total(rng, total, C1, P, empty=()):
    """total survivors over C1 classes, at most P each, none in `empty`"""
    w = rng.uniform(0.2, 1.0, C1)
    w[list(empty)] = 0
    cnt = np.minimum(np.floor(total * w / w.sum()).astype(np.int64), P)
    open_ = [c for c in range(C1) if c not in set(empty)]
    while cnt.sum() < total:
        c = open_[int(rng.integers(0, len(open_)))]
        if cnt[c] < P:
            cnt[c] += min(P - cnt[c], total - cnt.sum(), max(1, (total - cnt.sum()) // 4))
    assert cnt.sum() == total and cnt.max() <= P
    return cnt


def topk_image(rng, counts, P, prob_bits):
    """One image of survivors: random boxes and prior ids in every slot, per class a random increasing subset of the P positions and
    probabilities (from prob_bits(total) -> uint32 bit patterns of positive floats) descending inside the class, as NMS leaves
    them.  The slots past a class's count are poisoned: position 0 and probability 2.0, which would win every top-k."""
    C1 = len(counts)
    s_boxes = rng.uniform(0, 1, (C1, P, 4)).astype(np.float32)
    s_idx = rng.integers(0, 100000, (C1, P)).astype(np.int32)
    kept_pos = np.zeros((C1, P), np.int32)
    kept_prob = np.full((C1, P), 2.0, np.float32)
    bits = np.asarray(prob_bits(int(np.sum(counts))), np.uint32)
    o = 0
    for c, k in enumerate(counts):
        kept_pos[c, :k] = np.sort(rng.choice(P, k, replace=False))
        kept_prob[c, :k] = -np.sort(-bits[o:o + k].view(np.float32))
        o += k
    cnt = np.zeros(C1 + 1, np.int32)
    cnt[:C1] = counts
    cnt[C1] = 12345                                                    # not a class: must not be read
    return s_boxes, s_idx, kept_pos, kept_prob, cnt


def uniform_bits(rng):
    return lambda n: rng.uniform(0.01, 1.0, n).astype(np.float32).view(np.uint32)


def run_topk(arrs, wh, top_k):
    """arrs: s_boxes (B,C1,P,4), s_idx, kept_pos, kept_prob (B,C1,P), kept_cnt (B,C1+1) -> the kernel's outputs, preset to sentinels"""
    B, C1, P = arrs[1].shape
    d = [_t(a) for a in arrs]
    d_wh = _t(np.asarray(wh, np.float32).reshape(B, 2))
    boxes = torch.full((B, top_k, 4), -1.0, device=DEV, dtype=torch.float32)
    classes = torch.full((B, top_k), -1, device=DEV, dtype=torch.int64)
    probs = torch.full((B, top_k), -1.0, device=DEV, dtype=torch.float32)
    ids = torch.full((B, top_k), -1, device=DEV, dtype=torch.int32)
    count = torch.full((B,), -7, device=DEV, dtype=torch.int32)
    half = (B * C1 * P * 4 + 255) // 256 * 256
    ws = torch.empty(2 * half, device=DEV, dtype=torch.uint8)
    rc = _lib().ssd_topk_emit_sorted(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), d_wh.data_ptr(),
                                     B, C1, P, top_k, boxes.data_ptr(), classes.data_ptr(), probs.data_ptr(), ids.data_ptr(),
                                     count.data_ptr(), ws.data_ptr(), 2 * half, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (boxes, classes, probs, ids, count))


def check_topk(images, wh, top_k):
    """images: per image the tuple of topk_image -> every output of the kernel equals topk_emit_ref exactly, slots past count keep
    their sentinel.  -> counts"""
    B = len(images)
    C1, P = images[0][1].shape
    gb, gc, gp, gi, gn = run_topk([np.stack([im[i] for im in images]) for i in range(5)], wh, top_k)
    for b, im in enumerate(images):
        rb, rc_, rp, ri = H.topk_emit_ref(*im, top_k, *np.asarray(wh, np.float32).reshape(B, 2)[b])
        k = rb.shape[0]
        assert k == min(int(im[4][:C1].sum()), top_k) and gn[b] == k, (b, int(gn[b]), k)
        assert np.array_equal(gc[b, :k], rc_), (b, np.nonzero(gc[b, :k] != rc_)[0][:8])
        assert np.array_equal(gp[b, :k].view(np.uint32), rp.view(np.uint32)), b
        assert np.array_equal(gi[b, :k], ri), (b, np.nonzero(gi[b, :k] != ri)[0][:8])
        assert np.array_equal(gb[b, :k].view(np.uint32), rb.view(np.uint32)), b
        assert (gb[b, k:] == -1).all() and (gc[b, k:] == -1).all() and (gp[b, k:] == -1).all() and (gi[b, k:] == -1).all(), b
    return gn


@pytest.mark.parametrize("top_k", [1, 200, 4096])
def test_bare_topk_totals_around_the_cut(top_k):
    """six images in one launch: total = 0, 1, top_k - 1, top_k, top_k + 1, 10 top_k (40 960 at top_k = 4096: beyond the 16 384
    probabilities the block keeps in LDS)"""
    rng = np.random.default_rng(top_k)
    C1, P = 20, 2560
    totals = [0, 1, top_k - 1, top_k, top_k + 1, 10 * top_k]
    images = [topk_image(rng, split_total(rng, t, C1, P, empty=(0, 7) if t > 1 else ()), P, uniform_bits(rng)) for t in totals]
    n = check_topk(images, [(300, 300)] * 6, top_k)
    assert n.tolist() == [min(t, top_k) for t in totals]


def test_bare_topk_ties():
    """top_k = 200 of about 2000: all probabilities one bit pattern (the first 200 in class-major order); 8 values (the cut inside a
    tie group that spans classes); values that differ in the lowest byte only, in the highest byte only, in one middle byte only
    (each radix pass decides alone); and the value 1.0, more often than top_k and less often"""
    rng = np.random.default_rng(5)
    C1, P, top_k = 20, 256, 200
    one = np.float32(1.0).view(np.uint32)
    makers = [
        lambda n: np.full(n, np.float32(0.5).view(np.uint32), np.uint32),
        lambda n: (np.float32(0.125) * rng.integers(1, 9, n).astype(np.float32)).view(np.uint32),
        lambda n: (np.uint32(0x3F000000) + rng.integers(0, 256, n).astype(np.uint32)),
        lambda n: ((rng.integers(0x30, 0x3F, n).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00123456)),
        lambda n: (np.uint32(0x3E000012) | (rng.integers(0, 256, n).astype(np.uint32) << np.uint32(8))),
        lambda n: (np.uint32(0x3E120034) | (rng.integers(0, 128, n).astype(np.uint32) << np.uint32(16))),
        lambda n: np.where(rng.uniform(0, 1, n) < 0.3, one, rng.uniform(0.5, 1.0, n).astype(np.float32).view(np.uint32)).astype(np.uint32),
        lambda n: np.where(rng.uniform(0, 1, n) < 0.03, one, rng.uniform(0.5, 1.0, n).astype(np.float32).view(np.uint32)).astype(np.uint32),
    ]
    images = [topk_image(rng, split_total(rng, 2000 + 17 * i, C1, P, empty=(3,)), P, mk) for i, mk in enumerate(makers)]
    # conditions, on the reference: the cut of the 8-value image falls inside a tie group that spans several classes
    _, rc, rp, _ = H.topk_emit_ref(*images[1], top_k, 1.0, 1.0)
    im = images[1]
    group = [c for c in range(C1) if (im[3][c, :im[4][c]] == rp[-1]).any()]
    taken = int((rp == rp[-1]).sum())
    assert len(group) > 3 and 0 < taken < sum(int((im[3][c, :im[4][c]] == rp[-1]).sum()) for c in group)
    assert len(set(rc[rp == rp[-1]].tolist())) > 1
    _, rc, rp, _ = H.topk_emit_ref(*images[0], top_k, 1.0, 1.0)
    assert (np.diff(rc) >= 0).all() and rc[0] == 0                                    # all tied: class-major order
    assert check_topk(images, [(300, 300)] * len(images), top_k).tolist() == [top_k] * len(images)


def test_bare_topk_beyond_the_lds_capacity():
    """C1 = 20, P = 1024: 900 kept per class (18 000 probabilities: read back from global memory), 16 384 (the last total that
    stays in LDS), 16 385 (the first that does not), and 18 000 again with probabilities quantised to 1/256 (ties on that path)"""
    rng = np.random.default_rng(6)
    C1, P, top_k = 20, 1024, 200
    quant = lambda n: (np.float32(1 / 256) * rng.integers(1, 257, n).astype(np.float32)).view(np.uint32)
    images = [topk_image(rng, np.full(C1, 900), P, uniform_bits(rng)),
              topk_image(rng, split_total(rng, 16384, C1, P), P, uniform_bits(rng)),
              topk_image(rng, split_total(rng, 16385, C1, P, empty=(0, 19)), P, uniform_bits(rng)),
              topk_image(rng, np.full(C1, 900), P, quant)]
    assert [int(im[4][:C1].sum()) for im in images] == [18000, 16384, 16385, 18000]
    check_topk(images, [(300, 300), (500, 375), (640, 480), (1, 1)], top_k)
    check_topk(images, [(300, 300), (500, 375), (640, 480), (1, 1)], 4096)


@pytest.mark.parametrize("C1", [1, 20, 255])
def test_bare_topk_class_counts(C1):
    """classes without survivors at the front, in the middle and at the end; totals above and below top_k"""
    rng = np.random.default_rng(C1)
    P, top_k = (512, 200) if C1 == 1 else (64, 200)
    if C1 == 1:
        images = [topk_image(rng, np.asarray([k]), P, uniform_bits(rng)) for k in (400, 0, 200, 512)]
    else:
        gaps = [(0, 1, 2), (C1 // 2, C1 // 2 + 1), (C1 - 1,), (0, C1 // 3, C1 - 2, C1 - 1)]
        images = []
        for e in gaps:
            cnt = rng.integers(0, P + 1, C1)
            cnt[list(e)] = 0
            images.append(topk_image(rng, cnt, P, uniform_bits(rng)))
        few = np.zeros(C1, np.int64)
        few[[C1 // 4, C1 // 2, C1 - 2]] = [5, 64, 1]                  # 70 survivors in three classes: emitted as they are
        images.append(topk_image(rng, few, P, uniform_bits(rng)))
    n = check_topk(images, [(300, 300)] * len(images), top_k)
    assert (n == top_k).any() and (n < top_k).any()


def test_bare_topk_several_images():
    """three images of different sizes in one launch, the middle one without survivors: count 0, outputs untouched"""
    rng = np.random.default_rng(8)
    C1, P, top_k = 20, 300, 200
    images = [topk_image(rng, split_total(rng, t, C1, P), P, uniform_bits(rng)) for t in (900, 0, 150)]
    assert check_topk(images, [(500, 375), (300, 300), (1920.5, 1080.25)], top_k).tolist() == [200, 0, 150]


# ---- end to end --------------------------------------------------------------------------------------------------------------------
IOU_MARGIN, SCORE_MARGIN, GAP = 2e-6, 2e-6, 1e-7         # the conventions of test_decode_at_ssd512_prior_count (tests/test_gpu_path.py)
RTOL = 1e-5


def _e2e(images, top_k, min_score=0.2, what=""):
    """images (l_, c_) -> Losses.inference_batch against O.decode_nms, image by image: prior ids and classes exactly, probabilities
    within 1e-5, boxes as the other decode tests.  Conditions first, on the reference alone (hard_nms_ref.decode_hard_nms, asserted
    equal to the oracle): every IoU comparison made 2e-6 from the threshold, every probability 2e-6 from min_score, distinct
    neighbouring candidates of a class 1e-7 apart.  -> the references' info dicts"""
    from objectdetection_ssd_amd import Losses
    refs, infos = [], []
    for l_, c_ in images:
        ref = O.decode_nms(l_, c_, 300, 300, top_k=top_k, min_score=min_score)
        mine = H.decode_hard_nms(l_, c_, 300, 300, top_k=top_k, min_score=min_score)
        assert all(np.array_equal(a, b) for a, b in zip(ref, mine[:4]))
        info = mine[4]
        print(what, {k: v for k, v in info.items() if k != "per_class"})
        assert info["iou_margin"] >= IOU_MARGIN and info["score_margin"] >= SCORE_MARGIN and info["gaps"] >= GAP, info
        refs.append(ref); infos.append(info)
    B = len(images)
    res = Losses.inference_batch(_t(np.stack([i[0] for i in images])), _t(np.stack([i[1] for i in images])), [(300, 300)] * B,
                                 top_k=top_k, min_score=min_score)
    for b, (o, (rb, rc, rp, ri)) in enumerate(zip(res, refs)):
        if rb.shape[0] == 0:
            assert o == ([], [], [])
            continue
        gb, gc, gp = (x.cpu().numpy() for x in o)
        assert gb.shape[0] == rb.shape[0], (what, b)
        assert np.array_equal(Losses.inference_batch.last_prior_ids[b].cpu().numpy(), ri), (what, b)
        assert np.array_equal(gc, rc), (what, b)
        np.testing.assert_allclose(gp, rp, rtol=RTOL, atol=0)
        np.testing.assert_allclose(gb, rb, rtol=1e-5, atol=1e-3)
    return infos


UNDERTRAINED_SEEDS = (100, 102, 103, 0, 104, 105, 106)       # image 3: the dense class; searched on the CPU for the margins


def test_decode_of_an_undertrained_net_runs_32_row_chunks():
    """B = 7; image 3 has one class with logit +6 on 6000 random priors, random l: production dispatch (B = 7, C1 = 20, 512 threads)
    resolves that class in 32-row chunks, on decoded boxes; about 1800 of them survive, so the radix select runs as well"""
    images = [undertrained_image(s, 6000 if i == 3 else 0) for i, s in enumerate(UNDERTRAINED_SEEDS)]
    infos = _e2e(images, 200, what="undertrained")
    n = infos[3]["max_candidates"]
    assert n > 4608 and chunk_rows(7, 20, 8732, n) == (32, 512)
    assert infos[3]["total"] > 1000 and all(chunk_rows(7, 20, 8732, i["max_candidates"])[0] == 64 for i in infos[:3] + infos[4:])


def test_decode_with_more_survivors_than_the_topk_keeps_in_lds():
    """COCO-style min_score = 0.01 on l = standard_normal * 0.05: more than 16 384 boxes survive NMS, so the top-k reads its
    probabilities from global memory.  Every prior is a candidate of 5 classes, probabilities on a lattice 3e-6 apart (the
    cross-class order has a relative margin of 2e-5)."""
    infos = _e2e([lattice_image(0)], 200, min_score=0.01, what="beyond kp_cap")
    assert all(i["total"] > 16384 for i in infos), [i["total"] for i in infos]


def test_decode_with_cross_class_ties_at_the_cut():
    """logit rows from 4 vectors with equal foreground entries: equal probabilities inside and across classes; with top_k = 50 the
    cut falls inside a tie group that spans classes (class-major order, lower prior index first inside a class)"""
    seeds = (1, 2, 3)
    images = [tied_image(s) for s in seeds]
    for l_, c_ in images:
        _, rc, rp, _, info = H.decode_hard_nms(l_, c_, 300, 300, top_k=50)
        ties = rp == rp[-1]
        all_p = H.decode_hard_nms(l_, c_, 300, 300, top_k=10 ** 6)[2]
        assert info["total"] > 50 and len(set(rc[ties].tolist())) > 1 and int(ties.sum()) < int((all_p == rp[-1]).sum())
    _e2e(images, 50, what="ties")

"""Synthetic per-class candidates for the bare NMS kernels (tests/test_soft_nms_gpu.py, tests/test_hard_nms_gpu.py): boxes and
sorted scores of one class, and their packing into the kernels' (image, class, slot) layout."""
import numpy as np


def random_class(rng, n, lo=0.05, size=(0.05, 0.3), quantum=None):
    """n boxes (centres uniform in the unit square) and n descending scores; quantum: scores rounded to multiples of it (ties)."""
    c = rng.uniform(0, 1, (n, 2))
    wh = rng.uniform(size[0], size[1], (n, 2))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    s = rng.uniform(lo, 1.0, n)
    if quantum:
        s = np.maximum(np.round(s / quantum), 1) * quantum
    return boxes, -np.sort(-s.astype(np.float32))


def pack(classes, B, C1, P):
    """classes[b][c] = (boxes (n,4), scores (n,)) -> s_boxes (B,C1,P,4), s_prob (B,C1,P), cand_cnt (B,C1+1); the slots past a
    class's count are filled with values that would change the result if they were read as candidates"""
    s_boxes = np.full((B, C1, P, 4), 0.5, np.float32)
    s_boxes[..., 2:] = 0.9
    s_prob = np.full((B, C1, P), 2.0, np.float32)
    cnt = np.zeros((B, C1 + 1), np.int32)
    for b in range(B):
        for c in range(C1):
            bx, sc = classes[b][c]
            n = sc.shape[0]
            s_boxes[b, c, :n], s_prob[b, c, :n], cnt[b, c] = bx, sc, n
    return s_boxes, s_prob, cnt


def lattice_pair(width, shift, x0=8, y0=8, height=4):
    """Two boxes on the 1/64 lattice, `width` x `height` cells, the second shifted right by `shift` cells: every coordinate, extent,
    area, intersection and union is a small integer over a power of two -- exact in f32 -- and so is the quotient for
    (width, shift) = (3, 1): 2 / 4 = 0.5 and (5, 3): 2 / 8 = 0.25."""
    q = np.float32(1 / 64)
    a = np.asarray([x0, y0, x0 + width, y0 + height], np.float32) * q
    b = np.asarray([x0 + shift, y0, x0 + shift + width, y0 + height], np.float32) * q
    return np.stack([a, b])


def near_threshold_pairs(rng, n_pairs, thr):
    """2 * n_pairs boxes: pair k = a random box and a copy shifted right so that IoU is about thr, its right edge then moved by
    -8 .. +8 ulps: inter / union lands within a few 1e-7 of thr, on either side.  The pairs lie in separate cells of a grid, so
    only partners overlap.  -> boxes (2 n, 4) with the partners interleaved (rows 2k, 2k + 1)."""
    side = int(np.ceil(np.sqrt(n_pairs)))
    cell = 1.0 / side
    out = []
    for k in range(n_pairs):
        x0, y0 = (k % side) * cell, (k // side) * cell
        w, h = rng.uniform(0.25, 0.4) * cell, rng.uniform(0.3, 0.8) * cell
        s = w * (1 - thr) / (1 + thr)                        # IoU of two w-wide boxes shifted by s: (w - s) / (w + s)
        a = np.asarray([x0, y0, x0 + w, y0 + h], np.float32)
        b = np.asarray([x0 + s, y0, x0 + s + w, y0 + h], np.float32)
        b[2] = np.nextafter(b[2], np.float32(2.0 if k % 2 else -2.0))        # start on one side, walk ulps
        for _ in range(int(rng.integers(0, 9))):
            b[2] = np.nextafter(b[2], np.float32(2.0 if k % 2 else -2.0))
        out += [a, b]
    return np.stack(out).astype(np.float32)


# ---- end-to-end images whose probabilities are separated by construction -------------------------------------------------------
# The device's softmax and expf differ from torch's by a few ulps, so an end-to-end comparison needs every decision of the reference
# to have a margin.  Thousands of random probabilities in one class always hold a pair closer than that, so these images place
# their probabilities on a lattice (logits = log of the wanted probabilities), every candidate on a slot of its own.
def lattice_image(seed, m=5, lo=0.02, hi=0.15, scale=0.05, P=8732, C=21):
    """Every prior is a candidate of m random classes, the P * m probabilities evenly spaced over [lo, hi) in random assignment
    (3e-6 apart for the defaults), all other foreground probabilities ~1e-13; l = standard_normal * scale."""
    rng = np.random.default_rng(seed)
    l_ = rng.standard_normal((P, 4), dtype=np.float32) * np.float32(scale)
    c_ = np.full((P, C), -30.0, np.float32)
    q = lo + (hi - lo) * rng.permutation(P * m).reshape(P, m) / (P * m)
    for p in range(P):
        c_[p, rng.choice(C - 1, m, replace=False)] = np.log(q[p])
        c_[p, C - 1] = np.log(1 - q[p].sum())
    return l_, c_


def undertrained_image(seed, n_dense=6000, cls=5, P=8732, C=21):
    """An under-trained net: class `cls` has logit +6 on n_dense random priors (n_dense = 0: none), whose background logits are
    chosen so that the class's probabilities are evenly spaced over [0.3, 0.95) in random assignment; 300 more random priors carry
    standard_normal * 3 rows; everything else is strong background.  l = standard_normal * 0.5."""
    rng = np.random.default_rng(seed)
    l_ = rng.standard_normal((P, 4), dtype=np.float32) * np.float32(0.5)
    c_ = np.full((P, C), -8.0, np.float32)
    c_[:, C - 1] = 8.0
    perm = rng.permutation(P)
    dense, fg = perm[:n_dense], perm[n_dense:n_dense + 300]
    c_[fg] = rng.standard_normal((fg.size, C), dtype=np.float32) * np.float32(3.0)
    if n_dense:
        q = 0.3 + 0.65 * rng.permutation(n_dense) / n_dense
        c_[dense] = -30.0
        c_[dense, cls] = 6.0
        c_[dense, C - 1] = 6.0 + np.log(1 / q - 1)             # p = 1 / (1 + exp(bg - 6))
    return l_, c_


def tied_image(seed, n_fg=120, P=8732, C=21):
    """Cross-class ties: n_fg random priors carry one of 4 logit vectors, each with several EQUAL foreground entries (so one row
    gives the same probability to several classes, and equal rows give equal probabilities within a class): probabilities
    0.21 / 0.24 / 0.27 / 0.30, in 4 / 3 / 3 / 2 classes.  l = standard_normal * 0.5."""
    rng = np.random.default_rng(seed)
    l_ = rng.standard_normal((P, 4), dtype=np.float32) * np.float32(0.5)
    c_ = np.full((P, C), -8.0, np.float32)
    c_[:, C - 1] = 8.0
    vec = np.full((4, C), -30.0, np.float32)
    for v, (p, classes) in enumerate(((0.21, (0, 3, 7, 19)), (0.24, (1, 3, 12)), (0.27, (0, 5, 19)), (0.30, (2, 7)))):
        vec[v, list(classes)] = np.log(p)
        vec[v, C - 1] = np.log(1 - p * len(classes))
    fg = rng.choice(P, n_fg, replace=False)
    c_[fg] = vec[rng.integers(0, 4, n_fg)]
    return l_, c_

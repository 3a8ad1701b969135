"""Checker and inputs for the first two stages of the decode alone (csrc/nms.hip: decode_compact_kernel, rank_scatter_kernel, through
ssd_decode_sorted), in numpy alone -- no kernel of the package runs here.

`check` takes the inputs of one launch and the five arrays it filled, and holds them to an f64 restatement of the decode:

  boxes       every prior's box is written.  The centre is g_c * p_wh / 10 + p_c in f32 (exact IEEE under the build's flags, so numpy
              gives the device's bits); the corners are centre -/+ extent / 2 with the SAME f32 half extent, so their midpoint is the
              centre up to the two final roundings: |mid - centre| <= (spacing(lo) + spacing(hi)) / 4.  The extent is held to an f64
              exp(g / 5) * p_wh before the cancellation: |corner - (centre -/+ extent64 / 2)| <= 1e-5 * (|centre| + extent64).
  set         cand_cnt[c] and the set s_idx[c, :n] equal {p : softmax64(c_)[p, c] >= float(float32(min_score))} exactly.  The
              precondition, asserted first on the reference alone: every foreground f64 probability is at least `margin` (SCORE_MARGIN
              = 2e-6) from the cut.  margin = 0 is for cuts whose decisions no rounding can change, and the caller says why:
              min_score <= 0 or > 1 (every non-NaN probability is on one side) and rows whose probabilities are exact in f32 and f64.
  order       on the device's own bits: s_prob[c, :n] non-increasing, equal bit patterns in ascending s_idx, no prior twice.
  values      s_prob[c, r] within 1e-5 (relative) of the f64 softmax at (s_idx[c, r], c).
  scatter     s_boxes[c, r] bit-equal to boxes[s_idx[c, r]]; cand_cnt[b, C1] == 0; every slot past n still holds its poison.
  oracle      hard_nms_ref.sorted_candidates (the oracle's decode, torch's f32 softmax): in every class whose reference neighbours
              are bit-equal or at least GAP = 1e-7 apart, s_idx equals the reference order exactly.

NaN probabilities (a row with a NaN or +inf logit, a row of -inf) are candidates of no class: NaN >= cut is false, as in torch.
Every tolerance-compared input keeps its logit spread within 60, so that every probability is a normal f32.
"""
import numpy as np

import hard_nms_ref as H
import ssd_oracle as O

SCORE_MARGIN, GAP, RTOL = 2e-6, 1e-7, 1e-5               # the conventions of tests/test_hard_nms_gpu.py

# What the output arrays hold before a launch, as nms_cases.pack chooses its fill: values that would change a later stage if read.
POISON_BOX = np.asarray([0.5, 0.5, 0.9, 0.9], np.float32)  # a box with an area, overlapping most others: would suppress
POISON_PROB = np.float32(2.0)                              # above every probability: would win every top-k
POISON_IDX = np.int32(-7)                                  # no prior: would be emitted as an id
POISON_CNT = np.int32(100003)                              # a counter the clear missed: past every array
POISON_ALL_BOXES = np.float32(-3.0)                        # boxes (B,P,4) is written everywhere


def block_priors(C):
    """priors per block of decode_compact for C classes (include/ssd_gfx950.h): as many of 256 / 128 / 64 rows of C | 1 floats as
    fit 48 KB"""
    S = C | 1
    return 256 if 256 * S * 4 <= 48 * 1024 else (128 if 128 * S * 4 <= 48 * 1024 else 64)


def sweep_sizes(C):
    """the prior counts of the shape sweep, relative to the block size: below one wave, around one wave, around one block, two blocks
    and one prior, two blocks, one wave and one lane"""
    nt = block_priors(C)
    return sorted({1, 63, 64, 65, nt - 1, nt, nt + 1, 2 * nt + 1, 2 * nt + 65})


def poisoned_outputs(B, P, C1):
    boxes = np.full((B, P, 4), POISON_ALL_BOXES, np.float32)
    s_boxes = np.tile(POISON_BOX, (B, C1, P, 1))
    s_prob = np.full((B, C1, P), POISON_PROB, np.float32)
    s_idx = np.full((B, C1, P), POISON_IDX, np.int32)
    cnt = np.full((B, C1 + 1), POISON_CNT, np.int32)
    return boxes, s_boxes, s_prob, s_idx, cnt


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
P_MAX = 2 * 256 + 65
# The shape sweep: both sides of both block-size switches (47 | 48, 95 | 96), both parities of the LDS row stride on each side, and
# one, two and three rounds of 32 classes, with rounds of exactly 32 (C = 33, 65) and of one class (34, 66).
SWEEP_C = (2, 3, 4, 21, 22, 33, 34, 47, 48, 65, 66, 95, 96, 97, 255, 256)
# Seeds whose three images keep every f64 foreground probability SCORE_MARGIN from min_score = 0.2 at P_MAX priors: the first of
# 1000 C + 0 .. 7 that does, searched on the reference alone (tests/test_decode_sort_cpu.py asserts it).  Of the 8 seeds of a class
# count, 8 meet the margin for C = 2, 3, 22, 33, 34, 48, 65, 95, 97, 256 and 7 for C = 4, 21, 47, 66, 96, 255.
SWEEP_SEED = {C: 1000 * C for C in SWEEP_C}


def random_priors(rng, P):
    """a valid prior set that is not an SSD table: centres in (0, 1), sizes in (0.05, 0.9)"""
    return np.concatenate([rng.uniform(0.01, 0.99, (P, 2)), rng.uniform(0.05, 0.9, (P, 2))], 1).astype(np.float32)


def random_offsets(rng, P):
    """N(0, 0.25), the size components of a few priors at +-10: exp(g / 5) spans e^-2 .. e^2"""
    l_ = (rng.standard_normal((P, 4)) * 0.5).astype(np.float32)
    k = max(1, P // 16)
    at = rng.choice(P, k, replace=False)
    l_[at, 2] = rng.choice([-10.0, 10.0], k)
    l_[at, 3] = rng.choice([-10.0, 10.0], k)
    return l_


def sweep_image(C, seed, b):
    """image b of the sweep for C classes: P_MAX priors, rows N(0, 9); a case of P priors takes the first P, so a margin that holds at
    P_MAX holds at every P"""
    rng = np.random.default_rng([seed, b])
    c_ = (rng.standard_normal((P_MAX, C)) * 3.0).astype(np.float32)
    return random_offsets(rng, P_MAX), c_


def sweep_case(C, seed, P, B=3):
    """-> l_ (B,P,4), c_ (B,P,C), priors (P,4)"""
    ims = [sweep_image(C, seed, b) for b in range(B)]
    pri = random_priors(np.random.default_rng([seed, 99]), P_MAX)
    return np.stack([i[0][:P] for i in ims]), np.stack([i[1][:P] for i in ims]), pri[:P].copy()


def softmax64(c_):
    x = np.asarray(c_, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(x - np.max(x, axis=-1, keepdims=True))      # a NaN or +inf logit, or a row of -inf: NaN in the whole row
        return e / np.sum(e, axis=-1, keepdims=True)


def score_margin(c_, min_score):
    """smallest |p - cut| over the foreground f64 probabilities that are numbers"""
    p = softmax64(c_)[..., :-1]
    d = np.abs(p - float(np.float32(min_score)))
    return float(np.min(d[np.isfinite(d)])) if np.isfinite(d).any() else np.inf


def strong_class_image(rng, n, cls, P, C, min_score_zero=False):
    """nms_cases.undertrained_image at any size: class `cls` has logit +6 on exactly n random priors whose background logits spread
    its probabilities evenly over [0.3, 0.95); every other class has the same on 0 - 3 of the priors that are left (while any are);
    everything else is strong background.  No prior is a candidate of two classes."""
    l_ = random_offsets(rng, P)
    c_ = np.full((P, C), -8.0, np.float32)
    c_[:, C - 1] = 8.0
    perm = rng.permutation(P)

    def place(at, c, q):
        c_[at] = -30.0
        c_[at, c] = 6.0
        c_[at, C - 1] = (6.0 + np.log(1 / q - 1)).astype(np.float32)         # p = 1 / (1 + exp(bg - 6))

    if n:
        place(perm[:n], cls, 0.3 + 0.65 * rng.permutation(n) / n)
    o = n
    for c in range(C - 1):
        k = min(int(rng.integers(0, 4)), P - o) if c != cls else 0
        if k:
            place(perm[o:o + k], c, rng.uniform(0.3, 0.95, k))
        o += k
    return l_, c_


def tied_rows_image(rng, P, C, n_fg=None):
    """nms_cases.tied_image at any size: n_fg (default: all) random priors carry one of 4 logit vectors with several equal foreground
    entries -- equal probabilities within a class and across classes"""
    l_ = random_offsets(rng, P)
    c_ = np.full((P, C), -8.0, np.float32)
    c_[:, C - 1] = 8.0
    vec = np.full((4, C), -30.0, np.float32)
    for v, (p, classes) in enumerate(((0.21, (0, 3, 7, 19)), (0.24, (1, 3, 12)), (0.27, (0, 5, 19)), (0.30, (2, 7)))):
        vec[v, list(classes)] = np.log(p)
        vec[v, C - 1] = np.log(1 - p * len(classes))
    fg = rng.choice(P, P if n_fg is None else n_fg, replace=False)
    c_[fg] = vec[rng.integers(0, 4, fg.size)]
    return l_, c_


# ---- the reference's own output, in the device's layout ------------------------------------------------------------------------
def reference_outputs(l_, c_, pri, min_score):
    """the oracle's decode up to the sorted candidates (hard_nms_ref.sorted_candidates) written into poisoned arrays"""
    B, P, C = c_.shape
    out = poisoned_outputs(B, P, C - 1)
    boxes, s_boxes, s_prob, s_idx, cnt = out
    for b in range(B):
        boxes[b] = O.xywh_to_xyxy(O.decode_offsets(l_[b], pri))
        cands, _ = H.sorted_candidates(l_[b], c_[b], min_score, pri)
        cnt[b] = 0
        for c, (bx, pc, order) in enumerate(cands):
            n = order.size
            s_boxes[b, c, :n], s_prob[b, c, :n], s_idx[b, c, :n], cnt[b, c] = bx, pc, order, n
    return out


# ---- the checker -----------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_boxes(l_, pri, boxes):
    """one image -> largest corner error in units of its bar"""
    g, p = np.asarray(l_, np.float32), np.asarray(pri, np.float32)
    assert np.isfinite(boxes).all(), "boxes: not every prior's box was written as a number"
    ref = O.decode_offsets(g, p)
    ctr = ref[:, :2].astype(np.float64)                          # exact f32 operations: the device's bits
    lo, hi = boxes[:, :2], boxes[:, 2:]
    mid = (lo.astype(np.float64) + hi.astype(np.float64)) / 2
    slack = (np.spacing(np.abs(lo)).astype(np.float64) + np.spacing(np.abs(hi)).astype(np.float64)) / 4
    bad = np.abs(mid - ctr) > slack
    assert not bad.any(), f"boxes: centre of prior {np.nonzero(bad)[0][:4]} is not the f32 centre: off by {np.abs(mid - ctr)[bad][:4]}"
    ext = np.exp(g[:, 2:].astype(np.float64) / 5) * p[:, 2:].astype(np.float64)
    bar = RTOL * (np.abs(ctr) + ext)
    err = np.maximum(np.abs(lo - (ctr - ext / 2)), np.abs(hi - (ctr + ext / 2))) / bar
    assert err.max() <= 1.0, f"boxes: corner of prior {int(np.argmax(err.max(1)))} is {err.max():.3g} bars from the f64 decode"
    return float(err.max())


def check(l_, c_, pri, min_score, outputs, margin=SCORE_MARGIN, oracle=True):
    """l_ (B,P,4), c_ (B,P,C), pri (P,4); outputs = (boxes, s_boxes, s_prob, s_idx, cand_cnt) as numpy arrays, pre-filled by
    poisoned_outputs.  Raises AssertionError at the first violation.  -> dict: prob_err (largest relative probability error against
    f64), box_err (largest corner error in bars), candidates (per image and class), compared / classes (classes with candidates whose
    order was compared with the oracle / all of them), score_margin."""
    boxes, s_boxes, s_prob, s_idx, cnt = outputs
    B, P, C = c_.shape
    C1 = C - 1
    assert boxes.shape == (B, P, 4) and s_boxes.shape == (B, C1, P, 4) and s_prob.shape == s_idx.shape == (B, C1, P) and cnt.shape == (B, C1 + 1)
    cut = float(np.float32(min_score))
    info = dict(prob_err=0.0, box_err=0.0, compared=0, classes=0, candidates=np.zeros((B, C1), np.int64))
    # the precondition, on the reference alone
    info["score_margin"] = score_margin(c_, min_score)
    assert info["score_margin"] >= margin, f"precondition: a reference probability lies {info['score_margin']:.3g} from the cut"
    for b in range(B):
        where = f"image {b}"
        info["box_err"] = max(info["box_err"], check_boxes(l_[b], pri, boxes[b]))
        p64 = softmax64(c_[b])
        with np.errstate(invalid="ignore"):
            ref_mask = (p64[:, :C1] >= cut).T                                     # (C1, P); NaN >= cut is False
        n = cnt[b, :C1].astype(np.int64)
        info["candidates"][b] = n
        assert cnt[b, C1] == 0, f"scatter: {where}: the spare counter holds {int(cnt[b, C1])}"
        ref_n = ref_mask.sum(1)
        bad = np.nonzero(n != ref_n)[0]
        assert bad.size == 0, f"set: {where} class {bad[:4]}: count {n[bad][:4]}, reference {ref_n[bad][:4]}"
        valid = np.arange(P)[None, :] < n[:, None]
        ci, ri = np.nonzero(valid)
        pi = s_idx[b][ci, ri].astype(np.int64)
        assert ((pi >= 0) & (pi < P)).all(), f"set: {where}: a prior id outside 0 .. P - 1"
        times = np.bincount(ci * P + pi, minlength=C1 * P).reshape(C1, P)
        assert times.max(initial=0) <= 1, f"order: {where} class {np.nonzero(times.max(1) > 1)[0][:4]}: a prior appears twice"
        bad = np.nonzero(((times > 0) != ref_mask).any(1))[0]
        assert bad.size == 0, f"set: {where} class {bad[:4]}: the candidates are not the reference's"
        # order, on the device's own bits
        pr, ix = s_prob[b], s_idx[b]
        pair = valid[:, 1:]
        with np.errstate(invalid="ignore"):
            rising = pair & ~(pr[:, :-1] >= pr[:, 1:])
        assert not rising.any(), f"order: {where} class {np.nonzero(rising.any(1))[0][:4]}: probabilities not in descending order"
        tie = pair & (_bits(pr)[:, :-1] == _bits(pr)[:, 1:]) & ~(ix[:, :-1] < ix[:, 1:])
        assert not tie.any(), f"order: {where} class {np.nonzero(tie.any(1))[0][:4]}: equal probabilities not in ascending prior order"
        # values
        want = p64[pi, ci]
        err = np.abs(pr[ci, ri].astype(np.float64) - want)
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(want > 0, err / want, np.where(err == 0, 0.0, np.inf))
        if rel.size:
            k = int(np.argmax(rel))
            assert rel[k] <= RTOL, f"values: {where} class {ci[k]} slot {ri[k]}: {pr[ci[k], ri[k]]!r} is {rel[k]:.3g} (relative) from {want[k]!r}"
            info["prob_err"] = max(info["prob_err"], float(rel[k]))
        # scatter
        same = (_bits(s_boxes[b])[ci, ri] == _bits(boxes[b])[pi]).all(1)
        assert same.all(), f"scatter: {where} class {ci[~same][:4]} slot {ri[~same][:4]}: not the box of its prior"
        rest = ~valid
        assert (_bits(s_boxes[b])[rest] == _bits(POISON_BOX)).all(), f"scatter: {where}: a box slot past the count was written"
        assert (_bits(pr)[rest] == _bits(POISON_PROB)).all(), f"scatter: {where}: a probability slot past the count was written"
        assert (ix[rest] == POISON_IDX).all(), f"scatter: {where}: a prior-id slot past the count was written"
        # the oracle's order, where its own probabilities decide it
        if oracle:
            cands, _ = H.sorted_candidates(l_[b], c_[b], min_score, pri)
            for c, (_, pc, order) in enumerate(cands):
                if order.size == 0:
                    continue
                info["classes"] += 1
                d = -np.diff(pc.astype(np.float64))
                if order.size != n[c] or not ((d == 0) | (d >= GAP)).all():
                    continue
                info["compared"] += 1
                assert np.array_equal(ix[c, :n[c]], order), \
                    f"oracle: {where} class {c}: order differs at slot {np.nonzero(ix[c, :n[c]] != order)[0][:4]}"
    return info

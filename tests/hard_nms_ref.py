"""CPU reference of the greedy NMS rule and of the cross-class top-k of the decode (csrc/nms.hip: nms_kernel, topk_emit_kernel), in
numpy alone -- no kernel of the package runs here.

(a) `greedy_nms_sorted`: one class in sorted order; a kept box suppresses every later box with IoU >= thr.  IoU is
    soft_nms_ref.iou_one_to_many -- the contraction-free f32 sequence of oracle/ssd_oracle.py:iou_matrix, one vectorised row per KEPT
    box -- so every operation is a correctly rounded f32 operation and the device must reproduce the keep list bit for bit.  A NaN IoU
    (0 / 0 of empty boxes, a NaN coordinate, inf - inf) is not >= thr: such a pair never suppresses.
(b) `topk_emit_ref`: the survivors of all classes concatenated class-major; all of them if at most top_k, else a stable sort by
    descending probability bits (ties keep their class-major order) cut at top_k; boxes times (w, h, w, h) in f32.
(c) `decode_hard_nms`: one image from (l_, c_) through (a) and (b) -- O.decode_nms restated on these two functions, with the
    margins of the decisions it took, for end-to-end comparisons that must allow the device's softmax and expf a few ulps.
"""
import numpy as np
import torch

import ssd_oracle as O
from soft_nms_ref import iou_one_to_many


def greedy_nms_sorted(boxes, scores, thr, with_margin=False):
    """boxes (n,4) xyxy f32 and scores (n,) of one class in sorted order -> kept positions (k,) int32, ascending.
    with_margin: also the smallest |IoU - thr| over the comparisons that were made (inf for none)."""
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
    n = boxes.shape[0]
    assert np.asarray(scores).reshape(-1).shape[0] == n
    thr = np.float32(thr)
    removed = np.zeros(n, bool)
    kept = []
    margin = np.inf
    for i in range(n):
        if removed[i]:
            continue
        kept.append(i)
        rest = np.nonzero(~removed[i + 1:])[0] + (i + 1)
        if rest.size == 0:
            continue
        iou = iou_one_to_many(boxes[i], boxes[rest])
        with np.errstate(invalid="ignore"):
            removed[rest[iou >= thr]] = True                 # NaN >= thr is False
        if with_margin:
            fin = iou[np.isfinite(iou)].astype(np.float64)
            if fin.size:
                margin = min(margin, float(np.min(np.abs(fin - float(thr)))))
    kept = np.asarray(kept, np.int32)
    return (kept, margin) if with_margin else kept


def topk_emit_ref(s_boxes, s_idx, kept_pos, kept_prob, kept_cnt, top_k, w, h):
    """One image.  s_boxes (C1,P,4), s_idx (C1,P), kept_pos (C1,P), kept_prob (C1,P) f32, kept_cnt (>= C1,) ->
    (boxes (K,4) f32 pixels, classes (K,) int64, probs (K,) f32, prior_ids (K,) int32), K = min(total, top_k)."""
    C1 = s_idx.shape[0]
    cls, pos, prob = [], [], []
    for c in range(C1):
        k = int(kept_cnt[c])
        cls.append(np.full(k, c, np.int64)); pos.append(np.asarray(kept_pos[c, :k], np.int64)); prob.append(np.asarray(kept_prob[c, :k], np.float32))
    cls, pos, prob = np.concatenate(cls), np.concatenate(pos), np.concatenate(prob)
    if cls.shape[0] > top_k:
        o = np.argsort(-prob.view(np.uint32).astype(np.int64), kind="stable")[:top_k]
        cls, pos, prob = cls[o], pos[o], prob[o]
    scale = np.asarray([w, h, w, h], np.float32)[None]
    boxes = (np.asarray(s_boxes, np.float32)[cls, pos].reshape(-1, 4) * scale).astype(np.float32)
    return boxes, cls, prob, np.asarray(s_idx)[cls, pos].astype(np.int32).reshape(-1)


def sorted_candidates(l_, c_, min_score=0.2, pri_cxcywh=None):
    """The oracle's decode up to the sorted candidates: per class (boxes (n,4) xyxy, probs (n,), prior ids (n,)) in descending order
    of probability, lower prior index first on ties; and the f32 softmax (P,C)."""
    l_ = np.asarray(l_, np.float32)
    c_ = np.asarray(c_, np.float32)
    if pri_cxcywh is None:
        pri_cxcywh = O.create_priors_ssd300() if c_.shape[0] == 8732 else O.create_priors_ssd512()
    bx = O.xywh_to_xyxy(O.decode_offsets(l_, pri_cxcywh))
    probs = torch.softmax(torch.from_numpy(c_), dim=1).numpy()
    out = []
    for c in range(c_.shape[1] - 1):
        pc = probs[:, c]
        cand = np.nonzero(pc >= np.float32(min_score))[0]
        order = cand[np.argsort(-pc[cand], kind="stable")]
        out.append((bx[order], pc[order], order))
    return out, probs


def decode_hard_nms(l_, c_, w, h, top_k=200, min_score=0.2, iou_threshold=0.45, pri_cxcywh=None):
    """(boxes, classes, probs, prior ids) as O.decode_nms, and a dict: iou_margin (smallest |IoU - thr| over the comparisons made),
    score_margin (smallest |prob - min_score| over all foreground probabilities, f64), gaps (the distinct nonzero differences
    between neighbouring candidate probabilities inside a class: their minimum), max_candidates (largest class), total (survivors
    before the top-k), per_class (survivors of each class)."""
    cands, probs = sorted_candidates(l_, c_, min_score, pri_cxcywh)
    C1 = len(cands)
    P = probs.shape[0]
    s_boxes = np.zeros((C1, P, 4), np.float32)
    s_idx = np.zeros((C1, P), np.int32)
    kept_pos = np.zeros((C1, P), np.int32)
    kept_prob = np.zeros((C1, P), np.float32)
    kept_cnt = np.zeros(C1, np.int32)
    info = dict(iou_margin=np.inf, gaps=np.inf, max_candidates=0)
    p64 = probs[:, :C1].astype(np.float64)
    info["score_margin"] = float(np.min(np.abs(p64 - float(np.float32(min_score)))))
    for c, (bx, pc, order) in enumerate(cands):
        n = order.size
        info["max_candidates"] = max(info["max_candidates"], n)
        if n == 0:
            continue
        kept, m = greedy_nms_sorted(bx, pc, iou_threshold, with_margin=True)
        info["iou_margin"] = min(info["iou_margin"], m)
        d = -np.diff(pc.astype(np.float64))
        if (d > 0).any():
            info["gaps"] = min(info["gaps"], float(d[d > 0].min()))
        s_boxes[c, :n], s_idx[c, :n] = bx, order
        kept_pos[c, :kept.size], kept_prob[c, :kept.size], kept_cnt[c] = kept, pc[kept], kept.size
    info["total"] = int(kept_cnt.sum())
    info["per_class"] = kept_cnt.copy()
    b, k, p, i = topk_emit_ref(s_boxes, s_idx, kept_pos, kept_prob, kept_cnt, top_k, w, h)
    return b, k, p, i.astype(np.int64), info

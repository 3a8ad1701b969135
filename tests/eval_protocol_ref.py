"""CPU restatement of the detection evaluator's protocol (Util.DetectionEvaluator: VOC 'difficult' objects, IoU-threshold sweep,
11-point / 101-point / all-point AP with integer recall).  IoU is the oracle's (oracle/ssd_oracle.py iou_matrix); everything else
is written the long way round: one full matching run per threshold with its own claimed array -- deliberately NOT the kernels'
one-pass bitmask form -- and plain numpy over the sorted lists for the AP.
tests/test_eval_protocol_cpu.py ties it to the reference's get_map through the golden vectors."""
import numpy as np

import ssd_oracle as O

LEVELS = {"11point": 10, "101point": 100, "all": 0}


def level_reached(cum_tp, n_gt, k, L):
    """Recall cum_tp / n_gt >= k / L, decided in 64-bit integers (cum_tp: scalar or array)."""
    return np.asarray(cum_tp, np.int64) * np.int64(L) >= np.int64(k) * np.int64(n_gt)


def ap_from_sorted(tp, ignored, n_gt, interpolation):
    """AP of one class at one threshold from its detections in descending (score, lower index first) order: `tp` / `ignored`
    boolean per detection, `n_gt` non-difficult objects.  NaN when n_gt == 0."""
    if n_gt == 0:
        return np.float64(np.nan)
    tp = np.asarray(tp, bool)[~np.asarray(ignored, bool)]                # the ignored detections leave the list
    cum_tp = np.cumsum(tp.astype(np.int64))
    cum_fp = np.cumsum((~tp).astype(np.int64))
    prec = cum_tp / (cum_tp + cum_fp)                                    # int64 / int64 -> float64, one correctly rounded division
    L = LEVELS[interpolation]
    if L:
        table = np.zeros(L + 1, np.float64)
        for k in range(L + 1):
            m = level_reached(cum_tp, n_gt, k, L)
            if m.any():
                table[k] = prec[m].max()
        return np.float64(np.mean(table))
    env = np.maximum.accumulate(prec[::-1])[::-1] if prec.size else prec # running maximum from the end
    return np.float64(env[tp].sum() / n_gt)


def _flat(items, dtype, width):
    parts = [np.asarray(a, dtype).reshape((-1, width) if width else (-1,)) for a in items]
    img = [np.full(len(p), i, np.int64) for i, p in enumerate(parts)]
    if not parts:
        return np.zeros((0, width) if width else (0,), dtype), np.zeros(0, np.int64)
    return np.concatenate(parts), np.concatenate(img)


def match(det_boxes, det_classes, det_scores, gt_boxes, gt_classes, gt_difficult=None, n_classes=20, thresholds=(0.5,)):
    """Rules 1-4.  Per-image lists as Util.get_map takes them (+ optional per-image 0/1 difficult flags) -> dict(tp, ignored uint16
    (D,), bit t = thresholds[t]; n_gt, n_det int64 (n_classes,); classes, scores: the concatenated detections)."""
    db, di = _flat(det_boxes, np.float32, 4)
    dc, _ = _flat([np.asarray(c).astype(np.int64) for c in det_classes], np.int64, 0)
    ds, _ = _flat(det_scores, np.float32, 0)
    gb, gi = _flat(gt_boxes, np.float32, 4)
    gc, _ = _flat([np.asarray(c).astype(np.int64) for c in gt_classes], np.int64, 0)
    gd = np.zeros(gb.shape[0], bool) if gt_difficult is None else _flat(gt_difficult, np.int64, 0)[0].astype(bool)
    D, G, T = db.shape[0], gb.shape[0], len(thresholds)
    thr32 = [np.float32(t) for t in thresholds]
    n_img = len(det_boxes)
    gt_of = [np.nonzero(gi == i)[0] for i in range(n_img)]
    det_of = [np.nonzero(di == i)[0] for i in range(n_img)]

    # rules 1-2: the best box of a detection and its IoU do not depend on the threshold
    best = np.full(D, -1, np.int64)             # global ground-truth index; -1 = no candidates or a NaN among their IoUs
    best_v = np.zeros(D, np.float32)
    for i in range(n_img):
        for d in det_of[i]:
            cand = gt_of[i][gc[gt_of[i]] == dc[d]]
            if cand.size == 0:
                continue
            iou = O.iou_matrix(db[d:d + 1], gb[cand])[0]
            if np.isnan(iou).any():
                continue
            k = int(np.argmax(iou))             # first index on ties
            best[d], best_v[d] = cand[k], iou[k]

    # rule 3, one whole run per threshold
    tp = np.zeros(D, np.uint16)
    ign = np.zeros(D, np.uint16)
    for t in range(T):
        claimed = np.zeros(G, bool)
        for i in range(n_img):
            sel = det_of[i]
            for cls in np.unique(dc[sel]):
                if not 0 <= cls < n_classes:
                    continue
                s = sel[dc[sel] == cls]
                for d in s[np.lexsort((s, -ds[s].astype(np.float64)))]:     # score descending, flat index ascending
                    g = best[d]
                    if g < 0 or not best_v[d] > thr32[t]:
                        continue                                             # false positive
                    if gd[g]:
                        ign[d] |= np.uint16(1 << t)
                    elif not claimed[g]:
                        claimed[g] = True
                        tp[d] |= np.uint16(1 << t)

    n_gt = np.asarray([int(((gc == c) & ~gd).sum()) for c in range(n_classes)], np.int64)
    n_det = np.asarray([int((dc == c).sum()) for c in range(n_classes)], np.int64)
    return dict(tp=tp, ignored=ign, n_gt=n_gt, n_det=n_det, classes=dc, scores=ds, n_thresholds=T)


def average_precisions(m, interpolation):
    """Rules 5-8 on the result of `match` -> ap float64 (T, n_classes), NaN where a class has no non-difficult ground truth."""
    tp, ign, dc, ds, n_gt = m["tp"], m["ignored"], m["classes"], m["scores"], m["n_gt"]
    T = m["n_thresholds"]
    ap = np.full((T, len(n_gt)), np.nan, np.float64)
    for c in range(len(n_gt)):
        s = np.nonzero(dc == c)[0]
        order = s[np.lexsort((s, -ds[s].astype(np.float64)))]        # score descending, flat index ascending
        for t in range(T):
            ap[t, c] = ap_from_sorted((tp[order] >> t) & 1, (ign[order] >> t) & 1, int(n_gt[c]), interpolation)
    return ap


def evaluate(det_boxes, det_classes, det_scores, gt_boxes, gt_classes, gt_difficult=None, n_classes=20, thresholds=(0.5,),
             interpolation="11point"):
    """`match` + `average_precisions`: the dict of `match` with ap float64 (T, n_classes)."""
    m = match(det_boxes, det_classes, det_scores, gt_boxes, gt_classes, gt_difficult, n_classes, thresholds)
    m["ap"] = average_precisions(m, interpolation)
    return m

"""CPU reference of the Soft-NMS rule (Bodla et al. 2017), in numpy alone -- no kernel of the package runs here.

(a) `soft_nms_sorted`: the rule operation for operation in IEEE f32 (np.float32 arrays, np.maximum / np.minimum, separate multiply
    and subtract, expf = np.exp on float32).  Every operation of the linear rule is a correctly rounded f32 operation, so the device
    must reproduce it bit for bit; the gaussian rule differs from the device through expf alone.  (np.maximum propagates a NaN
    coordinate where the device's fmaxf drops it; a box with a NaN coordinate has a NaN area either way, so IoU is NaN in both.)
(b) the margin: the smallest relative distance of any decision taken in (a) from flipping -- the picked score against the runner-up
    at every pick, every score against keep_score where the two are compared, IoU against iou_threshold (linear), and in (c) every
    probability against min_score.  A comparison between device and reference that allows rounding differences (gaussian, end to
    end) is only meaningful on inputs whose margin is far above those differences.
(c) `decode_soft_nms`: one image from (l_, c_), the Soft-NMS counterpart of class_count_ref.decode_nms.
"""
import numpy as np
import torch

import ssd_oracle as O

LINEAR, GAUSSIAN = 1, 2
METHODS = {"linear": LINEAR, "gaussian": GAUSSIAN}
_F0, _F1 = np.float32(0), np.float32(1)


def iou_one_to_many(a, b):
    """a (4,), b (m,4) xyxy f32 -> (m,) f32: inter / ((area_a + area_b) - inter), 0/0 = NaN."""
    lx, ly = np.maximum(a[0], b[:, 0]), np.maximum(a[1], b[:, 1])
    hx, hy = np.minimum(a[2], b[:, 2]), np.minimum(a[3], b[:, 3])
    dx, dy = np.maximum(hx - lx, _F0), np.maximum(hy - ly, _F0)
    inter = dx * dy
    a1 = (a[2] - a[0]) * (a[3] - a[1])
    a2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    with np.errstate(all="ignore"):
        return inter / ((a1 + a2) - inter)


def _rel(x, ref):
    """smallest |x - ref| / ref over x (float64), inf for no x"""
    x = np.asarray(x, np.float64).reshape(-1)
    return float(np.min(np.abs(x - float(ref)) / float(ref))) if x.size else np.inf


def soft_nms_sorted(boxes, scores, method, iou_threshold, sigma, keep_score, max_picks):
    """boxes (n,4) xyxy and scores (n,) of one class in sorted order (descending score).
    -> (positions (k,) int32 in pick order, decayed scores (k,) f32, margin)."""
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 4)
    s = np.array(scores, np.float32).reshape(-1)
    n = s.shape[0]
    thr, sig, keep = np.float32(iou_threshold), np.float32(sigma), np.float32(keep_score)
    live = np.ones(n, bool)
    pos, out = [], []
    margin = _rel(s, keep)
    with np.errstate(all="ignore"):
        for _ in range(min(n, int(max_picks))):
            idx = np.nonzero(live)[0]
            if idx.size == 0:
                break
            sl = s[idx]
            t = int(np.argmax(sl))                            # first maximum: the lower sorted position on ties
            j, top = int(idx[t]), sl[t]
            if idx.size > 1:
                second = np.delete(sl, t).max()
                margin = min(margin, (float(top) - float(second)) / float(top))
            margin = min(margin, _rel(top, keep))
            if top < keep:
                break
            pos.append(j)
            out.append(top)
            live[j] = False
            rest = idx[idx != j]
            if rest.size == 0:
                continue
            iou = iou_one_to_many(boxes[j], boxes[rest])
            fin = np.isfinite(iou)
            if method == LINEAR:
                w = np.where(iou > thr, _F1 - iou, _F1).astype(np.float32)
                if thr > 0:
                    margin = min(margin, _rel(iou[fin], thr))
            elif method == GAUSSIAN:
                w = np.exp(-(iou * iou) / sig).astype(np.float32)
            else:
                raise ValueError("method")
            w = np.where(fin, w, _F1).astype(np.float32)
            s2 = (s[rest] * w).astype(np.float32)
            s[rest] = s2
            margin = min(margin, _rel(s2, keep))
            live[rest[s2 < keep]] = False
    return np.asarray(pos, np.int32), np.asarray(out, np.float32), margin


def decode_soft_nms(l_, c_, w, h, top_k=200, min_score=0.2, iou_threshold=0.45, nms="linear", sigma=0.5, keep_score=None,
                    pri_cxcywh=None):
    """One image, as class_count_ref.decode_nms: (boxes (K,4) pixels, classes (K,) int64, decayed scores (K,), prior ids (K,)) and
    a dict: margin (all decisions of the rule and of the candidate selection), order_margin (smallest relative gap between
    neighbours in the cross-class descending sort, inf where all picks are emitted class-major), total (picks before the top-k)."""
    l_ = np.asarray(l_, np.float32)
    c_ = np.asarray(c_, np.float32)
    C = c_.shape[1]
    method = METHODS[nms]
    keep = min_score if keep_score is None else keep_score
    if pri_cxcywh is None:
        pri_cxcywh = O.create_priors_ssd300() if c_.shape[0] == 8732 else O.create_priors_ssd512()
    boxes_cxcywh = O.decode_offsets(l_, pri_cxcywh)
    probs = torch.softmax(torch.from_numpy(c_), dim=1).numpy()
    margin = _rel(probs[:, :C - 1], np.float32(min_score))
    kb, kc, kp, ki = [], [], [], []
    for c in range(C - 1):
        pc = probs[:, c]
        cand = np.nonzero(pc >= np.float32(min_score))[0]
        if cand.size == 0:
            continue
        order = cand[np.argsort(-pc[cand], kind="stable")]
        bx = O.xywh_to_xyxy(boxes_cxcywh[order])
        pos, sc, m = soft_nms_sorted(bx, pc[order], method, iou_threshold, sigma, keep, top_k)
        margin = min(margin, m)
        kb.append(bx[pos]); kp.append(sc); ki.append(order[pos])
        kc.append(np.full(pos.size, c, np.int64))
    info = dict(margin=margin, order_margin=np.inf, total=0)
    if not kb:
        z = np.zeros
        return z((0, 4), np.float32), z((0,), np.int64), z((0,), np.float32), z((0,), np.int64), info
    kb, kc, kp, ki = np.concatenate(kb), np.concatenate(kc), np.concatenate(kp), np.concatenate(ki)
    info["total"] = int(kb.shape[0])
    if kb.shape[0] > top_k:
        full = np.argsort(-kp, kind="stable")
        srt = kp[full].astype(np.float64)
        # the order of the first top_k and the cut after them (the decision between entry top_k - 1 and entry top_k)
        info["order_margin"] = float(np.min((srt[:top_k] - srt[1:top_k + 1]) / srt[:top_k]))
        o = full[:top_k]
        kb, kc, kp, ki = kb[o], kc[o], kp[o], ki[o]
    return (kb * np.asarray([w, h, w, h], np.float32)[None]).astype(np.float32), kc, kp.astype(np.float32), ki, info


def disjoint_inputs(C, seed, n_classes_used=3):
    """(l_, c_) of one SSD300 image whose candidates cannot overlap: zero offsets (boxes = priors), everything strong background
    except the 0.1 x 0.1 square priors of every fifth cell of the 38 x 38 map (centres 0.13 apart), with random foreground rows."""
    rng = np.random.default_rng(seed)
    l_ = np.zeros((8732, 4), np.float32)
    c_ = np.full((8732, C), -8.0, np.float32)
    c_[:, C - 1] = 8.0
    cells = [(i * 38 + j) * 4 for i in range(0, 38, 5) for j in range(0, 38, 5)]
    for p in cells:
        c_[p] = -8.0
        c_[p, rng.integers(0, min(n_classes_used, C - 1))] = rng.uniform(-7.0, 2.0)      # probabilities on both sides of min_score
    return l_, c_

"""CPU restatement of the class-count-dependent parts of the reference for ANY conf width C = n_classes + 1 (background = the
last column, C - 1): matching and MultiBox loss (Losses.py:136-199), decode + per-class NMS + top-k (Losses.py:11-98), get_map
(Util.py:783-885) and the SSD300 / SSD512 heads.  The oracle (oracle/ssd_oracle.py) hard-codes VOC's 20 + 1; this module uses its
class-independent pieces (priors, IoU, encode / decode, the trunk) and restates the rest with C as a parameter.
tests/test_class_count_cpu.py ties it to the reference at C = 21 through the golden vectors."""
import numpy as np
import torch

import ssd_oracle as O


# ---- matching + loss (Losses.py:136-199) ---------------------------------------------------------------------------------------
def match_priors(boxes, classes, pri_xyxy, C):
    """obj (bs,P) global GT index, cls (bs,P) int64 with background C - 1, overlap (bs,P), all boxes, image starts."""
    bs = len(boxes)
    counts = [int(np.asarray(b).shape[0]) for b in boxes]
    if any(c == 0 for c in counts):
        raise ValueError("every image needs at least one ground-truth box")
    start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    allb = np.concatenate([np.asarray(b, np.float32).reshape(-1, 4) for b in boxes], 0)
    allc = np.concatenate([np.asarray(c, np.float32).reshape(-1) for c in classes], 0)
    iou = O.iou_matrix(allb, pri_xyxy)
    P = pri_xyxy.shape[0]
    obj = np.zeros((bs, P), np.int64)
    overlap = np.zeros((bs, P), np.float32)
    prior_for_obj = np.argmax(iou, axis=1)                  # best prior per box, first index on ties
    for i in range(bs):
        s, e = start[i], start[i + 1]
        obj[i] = np.argmax(iou[s:e], axis=0) + s            # best box per prior, first index on ties
        overlap[i] = iou[s:e].max(axis=0)
        for k in range(s, e):                               # forced matches in GT order: the last box wins
            obj[i, prior_for_obj[k]] = k
            overlap[i, prior_for_obj[k]] = np.float32(1.)
    cls = allc[obj].astype(np.float32)
    cls[overlap < np.float32(0.5)] = C - 1
    return obj, cls.astype(np.int64), overlap, allb, start


def multibox_loss(loc, conf, boxes, classes, pri_cxcywh=None, neg_pos_ratio=3):
    """The loss of Losses.py:136-199 at conf width C = conf.shape[-1].  Selection (matching, hard negatives) from the f32 cross
    entropy as torch computes it; losses and gradients also in float64 (`*_64`) for tolerance checks."""
    loc = np.asarray(loc, np.float32)
    conf = np.asarray(conf, np.float32)
    bs, P, C = conf.shape
    if pri_cxcywh is None:
        pri_cxcywh = O.create_priors_ssd300() if P == 8732 else O.create_priors_ssd512()
    obj, cls, overlap, allb, _ = match_priors(boxes, classes, O.xywh_to_xyxy(pri_cxcywh), C)
    pos = cls != C - 1
    n_pos = int(pos.sum())
    g = O.encode_offsets(O.xyxy_to_xywh(allb)[obj][pos], np.broadcast_to(pri_cxcywh[None], (bs, P, 4))[pos])
    diff = loc[pos] - g
    logp = torch.log_softmax(torch.from_numpy(conf.reshape(-1, C)), dim=-1).numpy().reshape(bs, P, C)
    cce = -np.take_along_axis(logp, cls[..., None], axis=2)[..., 0]
    neg = cce.copy()
    neg[pos] = 0.
    k = neg_pos_ratio * pos.sum(axis=1)
    order = np.argsort(-neg, axis=1, kind="stable")         # descending, lower prior index first among equal values
    hn = np.zeros_like(pos)
    for i in range(bs):
        hn[i, order[i, :min(int(k[i]), P)]] = True
    logp64 = torch.log_softmax(torch.from_numpy(conf.reshape(-1, C)).double(), dim=-1).numpy().reshape(bs, P, C)
    cce64 = -np.take_along_axis(logp64, cls[..., None], axis=2)[..., 0]
    loc_loss = np.abs(diff.astype(np.float64)).sum() / (n_pos * 4)
    # a quota past the negatives spills onto positives, which count as 0 there (Losses.py:190: cce1[pos_ancs] = 0. before the sort)
    conf_loss = (cce64[hn & ~pos].sum() + cce64[pos].sum()) / n_pos
    dloc = np.zeros(loc.shape, np.float64)
    dloc[pos] = np.sign(diff) / (n_pos * 4)
    onehot = np.zeros((bs, P, C), np.float64)
    np.put_along_axis(onehot, cls[..., None], 1.0, axis=2)
    dconf = (np.exp(logp64) - onehot) * (pos | hn)[..., None] / n_pos
    return dict(obj=obj, cls=cls, pos=pos, hn=hn, n_pos=n_pos, cce=cce, enc=g, loc_loss=loc_loss, conf_loss=conf_loss, dloc=dloc,
                dconf=dconf)


# ---- decode + NMS + top-k (Losses.py:11-98) -----------------------------------------------------------------------------------
def decode_nms(l_, c_, w, h, top_k=200, min_score=0.2, iou_threshold=0.45, pri_cxcywh=None):
    """One image: (boxes (K,4) pixels, classes (K,) int64 in 0 .. C-2, probs (K,), prior ids (K,))."""
    l_ = np.asarray(l_, np.float32)
    c_ = np.asarray(c_, np.float32)
    C = c_.shape[1]
    if pri_cxcywh is None:
        pri_cxcywh = O.create_priors_ssd300() if c_.shape[0] == 8732 else O.create_priors_ssd512()
    boxes_cxcywh = O.decode_offsets(l_, pri_cxcywh)
    probs = torch.softmax(torch.from_numpy(c_), dim=1).numpy()
    kb, kc, kp, ki = [], [], [], []
    for c in range(C - 1):                                  # never the background
        pc = probs[:, c]
        cand = np.nonzero(pc >= np.float32(min_score))[0]
        if cand.size == 0:
            continue
        order = cand[np.argsort(-pc[cand], kind="stable")]
        bx = O.xywh_to_xyxy(boxes_cxcywh[order])
        n = order.size
        suppressed = np.zeros(n, bool)
        for i in range(n):                                  # greedy, row by row (no n x n matrix: the all-candidates case has 8 732)
            if suppressed[i]:
                continue
            rest = np.arange(i + 1, n)[~suppressed[i + 1:]]
            if rest.size:
                suppressed[rest[O.iou_matrix(bx[i:i + 1], bx[rest])[0] >= np.float32(iou_threshold)]] = True
        keep = ~suppressed
        kb.append(bx[keep]); kp.append(pc[order][keep]); ki.append(order[keep])
        kc.append(np.full(int(keep.sum()), c, np.int64))
    if not kb:
        z = np.zeros
        return z((0, 4), np.float32), z((0,), np.int64), z((0,), np.float32), z((0,), np.int64)
    kb, kc, kp, ki = np.concatenate(kb), np.concatenate(kc), np.concatenate(kp), np.concatenate(ki)
    if kb.shape[0] > top_k:
        o = np.argsort(-kp, kind="stable")[:top_k]
        kb, kc, kp, ki = kb[o], kc[o], kp[o], ki[o]
    return (kb * np.asarray([w, h, w, h], np.float32)[None]).astype(np.float32), kc, kp.astype(np.float32), ki


# ---- get_map (Util.py:783-885) ------------------------------------------------------------------------------------------------
def get_map(det_boxes, det_classes, det_scores, gt_boxes, gt_classes, n_classes=20):
    """{class: AP} for range(n_classes); the matching and precision / recall rules of O.get_map."""
    db = np.concatenate([np.asarray(b, np.float32).reshape(-1, 4) for b in det_boxes])
    dc = np.concatenate([np.asarray(c).reshape(-1).astype(np.int64) for c in det_classes])
    ds = np.concatenate([np.asarray(s, np.float32).reshape(-1) for s in det_scores])
    di = np.concatenate([np.full(len(np.asarray(b).reshape(-1, 4)), i, np.int64) for i, b in enumerate(det_boxes)])
    gb = np.concatenate([np.asarray(b, np.float32).reshape(-1, 4) for b in gt_boxes])
    gc = np.concatenate([np.asarray(c).reshape(-1).astype(np.int64) for c in gt_classes])
    gi = np.concatenate([np.full(len(np.asarray(b).reshape(-1, 4)), i, np.int64) for i, b in enumerate(gt_boxes)])
    avail = np.ones(gb.shape[0], bool)
    thr = O.ap_recall_thresholds()
    table = np.zeros((n_classes, 11), np.float64)
    for cls in range(n_classes):
        sel = np.nonzero(dc == cls)[0]
        if sel.size == 0:
            continue
        order = sel[np.lexsort((sel, -ds[sel].astype(np.float64)))]
        n_gt = int((gc == cls).sum())
        tps = []
        for d in order:
            cand = np.nonzero((gi == di[d]) & (gc == cls))[0]
            hit = False
            if cand.size:
                iou = O.iou_matrix(db[d:d + 1], gb[cand])[0]
                best = -1 if np.isnan(iou).any() else int(np.argmax(iou))
                if best >= 0 and iou[best] > np.float32(0.5) and avail[cand[best]]:
                    hit = True
                    avail[cand[best]] = False
            tps.append(1.0 if hit else 0.0)
        tps = np.asarray(tps, np.float64)
        cum_tp, cum_fp = tps.cumsum(), (1.0 - tps).cumsum()
        prec = cum_tp / (cum_tp + cum_fp)
        with np.errstate(divide="ignore", invalid="ignore"):
            rec = np.float64(np.float32(1.0) / np.float32(n_gt)) * cum_tp
        for t in range(11):
            m = rec >= thr[t]
            if m.any():
                table[cls, t] = prec[m].max()
    return {cls: np.float64(table[cls].mean()) for cls in range(n_classes)}


# ---- the network with C-wide conf heads --------------------------------------------------------------------------------------
def heads(variant=300):
    return O.HEADS if variant == 300 else O.HEADS_512


def random_params(n_conf, seed=0, variant=300):
    """O.ssd300_random_params with the conf heads drawn at width n_conf * anchors (same draw rule: torch default init of a conv)."""
    params = O.ssd300_random_params(seed, variant)
    g = torch.Generator().manual_seed(seed + 1000 * n_conf)
    for name, cin, a in heads(variant):
        bound = 1.0 / np.sqrt(cin * 9)
        params[f"{name}_cl.weight"] = (torch.rand((n_conf * a, cin, 3, 3), generator=g) * 2 - 1) * bound
        params[f"{name}_cl.bias"] = (torch.rand((n_conf * a,), generator=g) * 2 - 1) * bound
    return params


def ssd_forward(x, params, n_conf, variant=300, operand_round=None, decisions=None, store_round=False):
    """loc (bs,P,4), conf (bs,P,n_conf): the oracle's trunk (run with 21-wide stand-ins for the conf heads, whose outputs are
    dropped) and the heads restated at width n_conf, NHWC-flattened and concatenated in the order of Model.py:212-235."""
    import torch.nn.functional as F
    trunk = dict(params)
    for name, cin, a in heads(variant):
        trunk[f"{name}_cl.weight"] = torch.zeros((21 * a, cin, 3, 3), dtype=x.dtype)
        trunk[f"{name}_cl.bias"] = torch.zeros((21 * a,), dtype=x.dtype)
    loc, _, srcs = O.ssd300_forward(x, trunk, return_features=True, variant=variant, operand_round=operand_round,
                                    decisions=decisions, store_round=store_round)
    conv2d = F.conv2d if operand_round is None else O._conv_bf16_operands()
    bs, confs = x.shape[0], []
    for (name, _, _), s in zip(heads(variant), srcs):
        hk = {"dy_bf16": True} if (store_round and name in ("c_4", "c_7")) else {}
        cl = conv2d(s, params[f"{name}_cl.weight"], params[f"{name}_cl.bias"], padding=1, **hk)
        confs.append(cl.permute(0, 2, 3, 1).reshape(bs, -1, n_conf))
    return loc, torch.cat(confs, 1)


def conf_ce_loss_torch(loc, conf, boxes, classes, neg_select, pri_cxcywh=None):
    """Differentiable (loc_loss, conf_loss) at width C = conf.shape[-1] with the hard negatives given (decision-pinned form)."""
    import torch.nn.functional as F
    bs, P, C = conf.shape
    if pri_cxcywh is None:
        pri_cxcywh = O.create_priors_ssd300() if P == 8732 else O.create_priors_ssd512()
    obj, cls, _, allb, _ = match_priors([np.asarray(b) for b in boxes], [np.asarray(c) for c in classes], O.xywh_to_xyxy(pri_cxcywh), C)
    pos_np = cls != C - 1
    g = O.encode_offsets(O.xyxy_to_xywh(allb)[obj][pos_np], np.broadcast_to(pri_cxcywh[None], (bs, P, 4))[pos_np])
    pos = torch.from_numpy(pos_np)
    loc_loss = (loc[pos] - torch.from_numpy(g).to(loc.dtype)).abs().mean()
    cce = F.cross_entropy(conf.reshape(-1, C), torch.from_numpy(cls).reshape(-1), reduction="none").view(bs, P)
    sel = torch.as_tensor(neg_select, dtype=torch.bool)
    conf_loss = (cce[sel].sum() + cce[pos].sum()) / pos.sum().to(cce.dtype)
    return loc_loss, conf_loss

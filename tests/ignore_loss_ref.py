"""CPU restatement of the MultiBox loss with ignore regions (ssd_multibox_loss_ignore).

Per image: the ground truth as in class_count_ref.multibox_loss, plus a possibly empty list of ignore boxes (fractional xyxy).
  1. matching is class_count_ref.match_priors: ignore boxes take no part, a positive prior stays positive
  2. a prior is ignored when it is not positive and some ignore box of its image overlaps it by >= ignore_threshold;
     "iou": ssd_oracle.iou_matrix (the matching's f32 op sequence), "ioa": the same intersection / the prior's own unclipped area,
     IEEE divide.  A NaN overlap is not >= anything: that box ignores nothing
  3. the reference's `cce1[pos_ancs] = 0.` becomes `cce1[pos_ancs | ignored] = 0.`; ranking, quota min(ratio * n_pos, P) and the
     tie rule (lower index first) are unchanged; the rows with a conf gradient are pos | (hn & ~ignored)
Overlaps, masks and the selection in f32 as the device computes them; losses and gradients in f64."""
import numpy as np
import torch

import class_count_ref as R
import ssd_oracle as O


def overlap_matrix(ign_boxes, pri_xyxy, mode):
    """(m, P) f32 overlap of every ignore box with every prior: "iou" or "ioa" (intersection over the prior's area)."""
    a = np.asarray(ign_boxes, np.float32).reshape(-1, 4)
    b = np.asarray(pri_xyxy, np.float32)
    if mode == "iou":
        return O.iou_matrix(a, b)
    if mode != "ioa":
        raise ValueError(mode)
    lo = np.maximum(a[:, None, :2], b[None, :, :2])
    hi = np.minimum(a[:, None, 2:], b[None, :, 2:])
    d = np.maximum(hi - lo, np.float32(0))
    inter = d[:, :, 0] * d[:, :, 1]
    area_p = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    with np.errstate(invalid="ignore", divide="ignore"):
        return (inter / area_p[None, :]).astype(np.float32)


def ignored_mask(ignore, pri_xyxy, pos, threshold=0.5, mode="iou"):
    """(bs, P) bool: not positive, and some ignore box of the image reaches the threshold."""
    ign = np.zeros(pos.shape, bool)
    thr = np.float32(threshold)
    for i, boxes in enumerate(ignore):
        boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
        if boxes.shape[0]:
            with np.errstate(invalid="ignore"):
                ign[i] = (overlap_matrix(boxes, pri_xyxy, mode) >= thr).any(axis=0)
    return ign & ~pos


def multibox_loss(loc, conf, boxes, classes, ignore=None, pri_cxcywh=None, neg_pos_ratio=3, ignore_threshold=0.5, ignore_overlap="iou"):
    """class_count_ref.multibox_loss's result with `ign` (bs, P) bool added; ignore = list of (m_i, 4) arrays, m_i >= 0 (None: none)."""
    loc = np.asarray(loc, np.float32)
    conf = np.asarray(conf, np.float32)
    bs, P, C = conf.shape
    if pri_cxcywh is None:
        pri_cxcywh = O.create_priors_ssd300() if P == 8732 else O.create_priors_ssd512()
    if ignore is None:
        ignore = [np.zeros((0, 4), np.float32)] * bs
    if len(ignore) != bs:
        raise ValueError("one ignore list per image")
    pri_xyxy = O.xywh_to_xyxy(pri_cxcywh)
    obj, cls, _, allb, _ = R.match_priors(boxes, classes, pri_xyxy, C)
    pos = cls != C - 1
    ign = ignored_mask(ignore, pri_xyxy, pos, ignore_threshold, ignore_overlap)
    n_pos = int(pos.sum())
    enc = O.encode_offsets(O.xyxy_to_xywh(allb)[obj][pos], np.broadcast_to(pri_cxcywh[None], (bs, P, 4))[pos])
    diff = loc[pos] - enc
    flat = torch.from_numpy(conf.reshape(-1, C))
    logp = torch.log_softmax(flat, dim=-1).numpy().reshape(bs, P, C)
    cce = -np.take_along_axis(logp, cls[..., None], axis=2)[..., 0]
    ranked = cce.copy()
    ranked[pos | ign] = 0.
    quota = neg_pos_ratio * pos.sum(axis=1)
    order = np.argsort(-ranked, axis=1, kind="stable")
    hn = np.zeros_like(pos)
    for i in range(bs):
        hn[i, order[i, :min(int(quota[i]), P)]] = True
    sel = pos | (hn & ~ign)
    logp64 = torch.log_softmax(flat.double(), dim=-1).numpy().reshape(bs, P, C)
    cce64 = -np.take_along_axis(logp64, cls[..., None], axis=2)[..., 0]
    loc_loss = np.abs(diff.astype(np.float64)).sum() / (n_pos * 4)
    conf_loss = (cce64[hn & ~pos & ~ign].sum() + cce64[pos].sum()) / n_pos
    dloc = np.zeros(loc.shape, np.float64)
    dloc[pos] = np.sign(diff) / (n_pos * 4)
    onehot = np.zeros((bs, P, C), np.float64)
    np.put_along_axis(onehot, cls[..., None], 1.0, axis=2)
    dconf = (np.exp(logp64) - onehot) * sel[..., None] / n_pos
    return dict(obj=obj, cls=cls, pos=pos, hn=hn, ign=ign, sel=sel, n_pos=n_pos, cce=cce, ranked=ranked, enc=enc, loc_loss=loc_loss,
                conf_loss=conf_loss, dloc=dloc, dconf=dconf)

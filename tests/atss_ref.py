"""CPU restatement of the ATSS matching of the MultiBox loss (ssd_multibox_loss_atss, match_mode 1), in numpy, and
the loss given that assignment.

levels = (cells, anchors): grid cells and priors per cell of every pyramid level; the priors are stored level after level, cell after
cell, the priors of a cell contiguous.  For box g = (x1, y1, x2, y2) of image i:
  1. candidates: in every level the min(topk, cells) cells whose centre (cx, cy of the cell's first prior) is nearest to
     ((x1 + x2) / 2, (y1 + y2) / 2), squared float32 distance dx dx + dy dy; nearest first, equal distances -> lower cell, NaN last --
     as the kernel does it: the smallest (distance bits, cell) above the last one taken.  All priors of a chosen cell, in the order
     (level, rank of the cell, prior of the cell)
  2. IoU of every candidate with g in iou_xyxy's float32 op sequence (fmax / fmin: a NaN operand gives the other one); float64 mean and
     unbiased variance in the kernel's order: partial sum j of 64 takes candidates j, j + 64, ... in turn, then a butterfly (xor 32, 16,
     .. 1) adds the partial sums; the variance of fewer than two candidates is 0
  3. accepted: d = float64(iou) - mean, d >= 0 and d d >= var (no square root), and x1 < pcx < x2, y1 < pcy < y2 of the prior's own centre
  4. a prior accepted by several boxes of its image goes to the largest (IoU bits, -box index)
A prior with a box is positive with that box's class and regression target, every other prior is background; nothing is forced.

`textbook` is the independent form tests/test_atss_cpu.py compares with: a full stable sort of the distances and torch's float32
mean() + std() as the threshold.

The loss given the assignment is tests/ignore_loss_ref.py's from its step 2 on (`ignored_mask` is that file's), with loc_side of
tests/box_loss_ref.py and conf_side of tests/focal_loss_ref.py for the other terms."""
import numpy as np
import torch

import box_loss_ref as BR
import focal_loss_ref as FR
import ignore_loss_ref as IR
import ssd_oracle as O

F = np.float32


def level_offsets(levels):
    """first prior of every level (and P at the end)"""
    cells, anchors = levels
    return np.concatenate([[0], np.cumsum([c * a for c, a in zip(cells, anchors)])]).astype(np.int64)


def iou_f32(g, b):
    """iou_xyxy: box g (4,) against priors b (n, 4), float32 throughout"""
    g, b = np.asarray(g, F), np.asarray(b, F)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        lx, ly = np.fmax(g[0], b[:, 0]), np.fmax(g[1], b[:, 1])
        hx, hy = np.fmin(g[2], b[:, 2]), np.fmin(g[3], b[:, 3])
        dx, dy = np.fmax(hx - lx, F(0)), np.fmax(hy - ly, F(0))
        inter = dx * dy
        area_a = (g[2] - g[0]) * (g[3] - g[1])
        area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        uni = (area_a + area_b) - inter
        return (inter / uni).astype(F)


def distances(g, pri_cxcywh, first, cells, anch):
    """squared float32 distance of the level's cell centres to the centre of box g"""
    g = np.asarray(g, F)
    with np.errstate(invalid="ignore", over="ignore"):
        gcx, gcy = (g[0] + g[2]) / F(2), (g[1] + g[3]) / F(2)
        c = pri_cxcywh[first + np.arange(cells) * anch]
        dx, dy = c[:, 0] - gcx, c[:, 1] - gcy
        return (dx * dx + dy * dy).astype(F)


def nearest_cells(d, k):
    """the kernel's rounds: k times the smallest (distance bits, cell) above the last one taken"""
    bits = np.where(np.isnan(d), np.uint32(0xFFFFFFFF), np.ascontiguousarray(d, F).view(np.uint32)).astype(np.uint64)
    key = (bits << np.uint64(32)) | np.arange(d.shape[0], dtype=np.uint64)
    out, prev = [], None
    for _ in range(min(k, d.shape[0])):
        best = key.min() if prev is None else key[key > prev].min()
        out.append(int(best & np.uint64(0xFFFFFFFF)))
        prev = best
    return out


def candidates(g, pri_cxcywh, levels, topk, pick=nearest_cells):
    """prior indices of the candidates of box g, in the kernel's order; and the chosen cells per level"""
    cells, anchors = levels
    off = level_offsets(levels)
    idx, chosen = [], []
    for l, (nc, an) in enumerate(zip(cells, anchors)):
        cs = pick(distances(g, pri_cxcywh, off[l], nc, an), topk)
        chosen.append(cs)
        for c in cs:
            idx.extend(range(off[l] + c * an, off[l] + (c + 1) * an))
    return np.asarray(idx, np.int64), chosen


def _ordered_sum(v):
    """float64 sum of v in the kernel's order"""
    n = v.shape[0]
    rows = (n + 63) // 64
    m = np.zeros(rows * 64, np.float64)
    m[:n] = v
    part = np.zeros(64, np.float64)
    for r in m.reshape(rows, 64):
        part = part + r
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[lane ^ o]
    return part[0]


def statistics(iou):
    """(mean, var) of the candidates' float32 IoUs, float64, the kernel's order of operations"""
    v = np.asarray(iou, F).astype(np.float64)
    n = v.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        mean = _ordered_sum(v) / np.float64(n)
        d = v - mean
        var = _ordered_sum(d * d) / np.float64(n - 1) if n > 1 else np.float64(0)
    return mean, var


def inside(g, pri_cxcywh, idx):
    g = np.asarray(g, F)
    with np.errstate(invalid="ignore"):
        pcx, pcy = pri_cxcywh[idx, 0], pri_cxcywh[idx, 1]
        return (g[0] < pcx) & (pcx < g[2]) & (g[1] < pcy) & (pcy < g[3])


def assign(boxes, pri_cxcywh, levels, topk=9):
    """boxes: one (n_i, 4) array per image -> dict(assign (bs, P) int32 global box index or -1; per box n_cand, mean, var, n_acc,
    cand (prior indices), accepted (bool per candidate), iou (float32 per candidate), cells (chosen cells per level))"""
    pri_cxcywh = np.asarray(pri_cxcywh, F)
    pri_xyxy = O.xywh_to_xyxy(pri_cxcywh)
    P = pri_cxcywh.shape[0]
    if level_offsets(levels)[-1] != P:
        raise ValueError("levels do not sum to P")
    out = dict(assign=np.full((len(boxes), P), -1, np.int32), n_cand=[], mean=[], var=[], n_acc=[], cand=[], accepted=[], iou=[], cells=[])
    k = 0
    for i, bx in enumerate(boxes):
        keys = np.zeros(P, np.uint64)
        for g in np.asarray(bx, F).reshape(-1, 4):
            idx, chosen = candidates(g, pri_cxcywh, levels, topk)
            iou = iou_f32(g, pri_xyxy[idx])
            mean, var = statistics(iou)
            with np.errstate(invalid="ignore", over="ignore"):
                d = iou.astype(np.float64) - mean
                ok = (d >= 0) & (d * d >= var) & inside(g, pri_cxcywh, idx)
            key = (iou.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(0xFFFFFFFF - k)
            np.maximum.at(keys, idx[ok], key[ok])
            for name, v in (("n_cand", idx.shape[0]), ("mean", mean), ("var", var), ("n_acc", int(ok.sum())), ("cand", idx), ("accepted", ok),
                            ("iou", iou), ("cells", chosen)):
                out[name].append(v)
            k += 1
        has = keys != 0
        out["assign"][i, has] = (np.uint64(0xFFFFFFFF) - (keys[has] & np.uint64(0xFFFFFFFF))).astype(np.int32)
    for name, dt in (("n_cand", np.int32), ("mean", np.float64), ("var", np.float64), ("n_acc", np.int32)):
        out[name] = np.asarray(out[name], dt)
    return out


def sorted_cells(d, k):
    """textbook: a full stable sort of the distances (numpy puts NaN last)"""
    return [int(c) for c in np.argsort(d, kind="stable")[:min(k, d.shape[0])]]


def textbook(boxes, pri_cxcywh, levels, topk=9):
    """The independent form: candidates by a full sort, threshold = torch float32 mean() + std() of the candidates' IoUs, accepted =
    iou >= threshold and the centre inside, conflicts by the largest IoU then the lower box.  -> dict(assign, thr (per box, float32),
    cand, iou)"""
    pri_cxcywh = np.asarray(pri_cxcywh, F)
    pri_xyxy = O.xywh_to_xyxy(pri_cxcywh)
    P = pri_cxcywh.shape[0]
    out = dict(assign=np.full((len(boxes), P), -1, np.int32), thr=[], cand=[], iou=[])
    k = 0
    for i, bx in enumerate(boxes):
        best = np.full(P, -np.inf, np.float64)
        for g in np.asarray(bx, F).reshape(-1, 4):
            idx, _ = candidates(g, pri_cxcywh, levels, topk, pick=sorted_cells)
            iou = iou_f32(g, pri_xyxy[idx])
            t = torch.tensor(iou)
            thr = (t.mean() + (t.std() if iou.shape[0] > 1 else 0.0)).numpy().astype(F)
            with np.errstate(invalid="ignore"):
                ok = (iou >= thr) & inside(g, pri_cxcywh, idx)
                take = ok & (iou.astype(np.float64) > best[idx])          # boxes in order: an equal IoU leaves the lower box
            out["assign"][i, idx[take]] = k
            best[idx[take]] = iou[take]
            out["thr"].append(thr)
            out["cand"].append(idx)
            out["iou"].append(iou)
            k += 1
    out["thr"] = np.asarray(out["thr"], F)
    return out


def class_index(v, C):
    """the kernels' clamp of a label into the row"""
    v = np.asarray(v, F)
    with np.errstate(invalid="ignore"):
        return np.where(v >= 0, np.where(v < C - 1, np.nan_to_num(v).astype(np.int64), C - 1), 0).astype(np.int64)


def multibox_loss(loc, conf, boxes, classes, pri_cxcywh, levels, topk=9, ignore=None, neg_pos_ratio=3, ignore_threshold=0.5,
                  ignore_overlap="iou"):
    """ignore_loss_ref.multibox_loss's result (cross entropy with mining, L1 term, norm_mode 0) with the ATSS assignment in the
    matching's place, plus `allb`, `assignment` and `sel_img` (the mined rows, positives not among them)"""
    loc, conf = np.asarray(loc, F), np.asarray(conf, F)
    pri_cxcywh = np.asarray(pri_cxcywh, F)
    bs, P, C = conf.shape
    if ignore is None:
        ignore = [np.zeros((0, 4), F)] * bs
    asg = assign(boxes, pri_cxcywh, levels, topk)
    allb = np.concatenate([np.asarray(b, F).reshape(-1, 4) for b in boxes], 0)
    allc = np.concatenate([np.asarray(c, F).reshape(-1) for c in classes], 0)
    pos = asg["assign"] >= 0
    obj = np.where(pos, asg["assign"], 0).astype(np.int64)
    cls = np.where(pos, class_index(allc, C)[obj], C - 1)
    ign = IR.ignored_mask(ignore, O.xywh_to_xyxy(pri_cxcywh), pos, ignore_threshold, ignore_overlap)
    n_pos = int(pos.sum())
    enc = O.encode_offsets(O.xyxy_to_xywh(allb)[obj][pos], np.broadcast_to(pri_cxcywh[None], (bs, P, 4))[pos])
    diff = loc[pos] - enc
    flat = torch.tensor(conf.reshape(-1, C))
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
    return dict(obj=obj, cls=cls, pos=pos, hn=hn, ign=ign, sel=sel, n_pos=n_pos, loc_loss=loc_loss, conf_loss=conf_loss, dloc=dloc,
                dconf=dconf, allb=allb, assignment=asg)


def box_side(loc, pri_cxcywh, base, mode, dtype=torch.float64, norm_mode=0):
    """box_loss_ref.loc_side on the assignment of `base`"""
    return BR.loc_side(loc, pri_cxcywh, base["allb"], base["pos"], base["obj"], mode, dtype, norm_mode)


def focal_side(conf, base, alpha, gamma, dtype=torch.float64, norm_mode=0):
    """focal_loss_ref.conf_side on the assignment of `base`"""
    return FR.conf_side(conf, base["cls"], base["ign"], base["n_pos"], alpha, gamma, dtype, norm_mode)

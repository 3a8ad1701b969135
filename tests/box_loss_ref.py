"""CPU restatement of the box-overlap localisation terms of the MultiBox loss (ssd_multibox_loss_box, loc_mode 1 .. 4; DESIGN.md
section 4l), in torch, parametrised by dtype, gradients by autograd.

For a positive prior (pcx, pcy, pw, ph) with offsets l = loc[i, p] and matched box g = (gx1, gy1, gx2, gy2):
    T  = log(1000 / 16)
    cx = l0 pw / 10 + pcx,  cy = l1 ph / 10 + pcy,  w = exp(clamp(l2 / 5, -T, T)) pw,  h = exp(clamp(l3 / 5, -T, T)) ph
    (x1, y1, x2, y2) = (cx - w/2, cy - h/2, cx + w/2, cy + h/2);  gw = gx2 - gx1, gh = gy2 - gy1
    inter = max(min(x2, gx2) - max(x1, gx1), 0) max(min(y2, gy2) - max(y1, gy1), 0)
    union = w h + gw gh - inter;  iou = inter / (union + eps), eps = 1e-7
    cw = max(x2, gx2) - min(x1, gx1);  ch = max(y2, gy2) - min(y1, gy1)
    "iou" : L = 1 - iou
    "giou": L = 1 - iou + (cw ch - union) / (cw ch + eps)
    "diou": L = 1 - iou + rho2 / (cw^2 + ch^2 + eps),  rho2 = (cx - (gx1 + gx2) / 2)^2 + (cy - (gy1 + gy2) / 2)^2
    "ciou": L = diou + alpha v,  v = 4 / pi^2 (atan(gw / gh) - atan(w / h))^2,  alpha = v / (1 - iou + v + eps), constant in the gradient
loc_loss = sum of L over the positives / n_pos (norm_mode 0) or the sum (norm_mode 1); dloc is its gradient.  Matching and the conf
side are tests/ignore_loss_ref.py's (which is tests/class_count_ref.py's where there is no ignore box).

Three deliberately wrong variants (tests/test_box_loss_cpu.py shows that the GPU bar tells each from the right one):
    "alpha_grad"   alpha takes part in the gradient
    "no_clamp"     the exponent is not clamped
    "diou_as_giou" "diou" with GIoU's penalty

`python tests/box_loss_ref.py` measures, for every case of tests/box_loss_cases.py and every mode, the distance of the float32 restatement
from the float64 one and writes tests/golden/box_loss_ref_distance.json."""
import json
import math
import os
import sys

import numpy as np
import torch

_ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")
if _ORACLE not in sys.path:                  # (`python tests/box_loss_ref.py` runs without tests/conftest.py)
    sys.path.insert(0, _ORACLE)

import ignore_loss_ref as IR
import ssd_oracle as O

T = math.log(1000.0 / 16.0)
EPS = 1e-7
MODES = ("iou", "giou", "diou", "ciou")
VARIANTS = ("alpha_grad", "no_clamp", "diou_as_giou")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_loss_ref_distance.json")


def decode(l, pri, clamp=True):
    """(n, 4) offsets against (n, 4) cxcywh priors -> cx, cy, w, h"""
    t2, t3 = l[:, 2] / 5, l[:, 3] / 5
    if clamp:
        t2, t3 = torch.clamp(t2, -T, T), torch.clamp(t3, -T, T)
    return l[:, 0] * pri[:, 2] / 10 + pri[:, 0], l[:, 1] * pri[:, 3] / 10 + pri[:, 1], torch.exp(t2) * pri[:, 2], torch.exp(t3) * pri[:, 3]


def geometry(l, pri, g, clamp=True):
    cx, cy, w, h = decode(l, pri, clamp)
    x1, y1, x2, y2 = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
    gx1, gy1, gx2, gy2 = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
    iw = torch.minimum(x2, gx2) - torch.maximum(x1, gx1)
    ih = torch.minimum(y2, gy2) - torch.maximum(y1, gy1)
    return dict(cx=cx, cy=cy, w=w, h=h, x1=x1, y1=y1, x2=x2, y2=y2, gx1=gx1, gy1=gy1, gx2=gx2, gy2=gy2, gw=gx2 - gx1, gh=gy2 - gy1, iw=iw, ih=ih)


def aspect_v(q):
    """CIoU's v of geometry q"""
    return (4 / math.pi ** 2) * (torch.atan(q["gw"] / q["gh"]) - torch.atan(q["w"] / q["h"])) ** 2


def per_positive(l, pri, g, mode, variant=None, alpha=None):
    """L of every row: l, pri (cxcywh), g (xyxy) are (n, 4) tensors of one dtype.  alpha: "ciou" with these values in alpha's place."""
    if mode not in MODES or variant not in (None,) + VARIANTS:
        raise ValueError((mode, variant))
    q = geometry(l, pri, g, clamp=variant != "no_clamp")
    inter = torch.clamp(q["iw"], min=0) * torch.clamp(q["ih"], min=0)
    union = q["w"] * q["h"] + q["gw"] * q["gh"] - inter
    iou = inter / (union + EPS)
    cw = torch.maximum(q["x2"], q["gx2"]) - torch.minimum(q["x1"], q["gx1"])
    ch = torch.maximum(q["y2"], q["gy2"]) - torch.minimum(q["y1"], q["gy1"])
    L = 1 - iou
    if mode == "giou" or (mode == "diou" and variant == "diou_as_giou"):
        return L + (cw * ch - union) / (cw * ch + EPS)
    if mode == "iou":
        return L
    rho2 = (q["cx"] - (q["gx1"] + q["gx2"]) / 2) ** 2 + (q["cy"] - (q["gy1"] + q["gy2"]) / 2) ** 2
    L = L + rho2 / (cw ** 2 + ch ** 2 + EPS)
    if mode == "diou":
        return L
    v = aspect_v(q)
    if alpha is None:
        alpha = v / (1 - iou + v + EPS)
        if variant != "alpha_grad":
            alpha = alpha.detach()
    return L + alpha * v


def ciou_alpha(l, pri, g):
    """alpha of "ciou" per row, as the constant it is in the gradient"""
    with torch.no_grad():
        q = geometry(l, pri, g)
        inter = torch.clamp(q["iw"], min=0) * torch.clamp(q["ih"], min=0)
        iou = inter / (q["w"] * q["h"] + q["gw"] * q["gh"] - inter + EPS)
        v = aspect_v(q)
        return v / (1 - iou + v + EPS)


def alpha_v(l, pri, g):
    """alpha * v of "ciou" per row (float64 tensors): how alive the aspect term is"""
    with torch.no_grad():
        return per_positive(l, pri, g, "ciou") - per_positive(l, pri, g, "diou")


def kink_distance(l, pri, g):
    """Per row (float64 tensors): the smallest of |x1 - gx1|, |x2 - gx2|, |y1 - gy1|, |y2 - gy2|, the two unclamped intersection
    extents' magnitudes and | |l/5| - T | of l2, l3 -- the places where min, max or clamp change branch."""
    q = geometry(l, pri, g)
    terms = [(q["x1"] - q["gx1"]).abs(), (q["x2"] - q["gx2"]).abs(), (q["y1"] - q["gy1"]).abs(), (q["y2"] - q["gy2"]).abs(),
             q["iw"].abs(), q["ih"].abs(), ((l[:, 2] / 5).abs() - T).abs(), ((l[:, 3] / 5).abs() - T).abs()]
    return torch.stack(terms, 1).min(1)[0]


def loc_side(loc, pri_cxcywh, allb, pos, obj, mode, dtype=torch.float64, norm_mode=0, variant=None):
    """loss_sum (the sum of L over the positives), loc_loss and dloc (bs, P, 4) of it, computed in `dtype`, returned as float64"""
    bs, P = pos.shape
    l = torch.tensor(np.asarray(loc, np.float32)[pos], dtype=dtype, requires_grad=True)
    pri = torch.tensor(np.broadcast_to(np.asarray(pri_cxcywh, np.float32)[None], (bs, P, 4))[pos], dtype=dtype)
    g = torch.tensor(np.asarray(allb, np.float32)[obj[pos]], dtype=dtype)
    L = per_positive(l, pri, g, mode, variant)
    total = L.sum()
    n_pos = int(pos.sum())
    value = total / n_pos if norm_mode == 0 else total
    value.backward()
    dloc = np.zeros((bs, P, 4), np.float64)
    dloc[pos] = l.grad.double().numpy()
    return dict(loss_sum=float(total.detach().double()), loc_loss=float(value.detach().double()), dloc=dloc, L=L.detach().double().numpy())


def multibox_loss(loc, conf, boxes, classes, mode, ignore=None, pri_cxcywh=None, neg_pos_ratio=3, ignore_threshold=0.5, ignore_overlap="iou",
                  dtype=torch.float64, norm_mode=0, variant=None, base=None):
    """ignore_loss_ref.multibox_loss's result (matching and the conf side: norm_mode 0) with loc_loss / dloc replaced by the box term's
    and `loss_sum`, `L` added.  base: that result, where the caller has it already."""
    if base is None:
        base = IR.multibox_loss(loc, conf, boxes, classes, ignore, pri_cxcywh, neg_pos_ratio, ignore_threshold, ignore_overlap)
    if pri_cxcywh is None:
        P = np.asarray(conf).shape[1]
        pri_cxcywh = O.create_priors_ssd300() if P == 8732 else O.create_priors_ssd512()
    allb = np.concatenate([np.asarray(b, np.float32).reshape(-1, 4) for b in boxes], 0)
    out = dict(base)
    out.update(loc_side(loc, pri_cxcywh, allb, base["pos"], base["obj"], mode, dtype, norm_mode, variant))
    return out


def distance(case, base, mode):
    """d32 of a case and mode: max |float32 restatement - float64| / max |float64| of dloc, and the same of the loss sum"""
    allb = np.concatenate([np.asarray(b, np.float32).reshape(-1, 4) for b in case.boxes], 0)
    a = loc_side(case.loc, case.priors_cxcywh, allb, base["pos"], base["obj"], mode, torch.float32)
    b = loc_side(case.loc, case.priors_cxcywh, allb, base["pos"], base["obj"], mode, torch.float64)
    big = np.abs(b["dloc"]).max()
    d = float(np.abs(a["dloc"] - b["dloc"]).max() / big) if big > 0 else float(np.abs(a["dloc"]).max())
    return dict(dloc=d, loss=abs(a["loss_sum"] - b["loss_sum"]) / abs(b["loss_sum"]))


if __name__ == "__main__":
    import box_loss_cases as BC
    out = {"what": "max |dloc(float32 restatement) - dloc(float64)| / max |dloc(float64)| and |loss sum difference| / |loss sum| of "
                   "tests/box_loss_ref.py on every case of tests/box_loss_cases.py and mode, CPU; written by `python tests/box_loss_ref.py`; "
                   "tests/test_box_loss_cpu.py holds a re-measurement to 2x these, tests/test_box_loss_gpu.py takes its dloc bar from them",
           "torch": torch.__version__.split("+")[0], "d32": {}}
    for case_id in BC.CASE_IDS:
        case, base = BC.case_and_reference(case_id)
        for mode in BC.modes_of(case_id):
            out["d32"][f"{case_id}|{mode}"] = distance(case, base, mode)
            print(case_id, mode, out["d32"][f"{case_id}|{mode}"])
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=2)
        f.write("\n")

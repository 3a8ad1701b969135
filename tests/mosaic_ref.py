"""numpy restatement of the mosaic augmentation (Dataset.MultiImageMultiBBoxDataset(mosaic=...), Bochkovskiy et al. 2020, section 3.3):
the draws with python's `random` in the order the dataset documents, the box arithmetic in float32, and the pixels -- each tile is
`oracle.ssd_oracle.preprocess_image` of its source at the tile's size, pasted at the tile's rectangle.  numpy only: nothing of the
package is imported here."""
import random

import numpy as np

import ssd_oracle as O

F = np.float32


def rectangles(cx, cy, H, W):
    """(top, left, h, w) of the tiles top-left, top-right, bottom-left, bottom-right around the centre (cx, cy)"""
    return ((0, 0, cy, cx), (0, cx, cy, W - cx), (cy, 0, H - cy, cx), (cy, cx, H - cy, W - cx))


def photometric_draws(rng=random):
    """reference Util.py:752-780: shuffle, then per op a coin and a factor"""
    order = [0, 1, 2, 3]
    rng.shuffle(order)
    out = []
    for kind in order:
        if rng.random() < 0.5:
            out.append((kind, rng.uniform(-18 / 255., 18 / 255.) if kind == 3 else rng.uniform(0.5, 1.5)))
    return tuple(out)


def _iou(cb, boxes):
    lo = np.maximum(cb[None, :2], boxes[:, :2])
    hi = np.minimum(cb[None, 2:], boxes[:, 2:])
    wh = np.maximum(hi - lo, F(0))
    inter = wh[:, 0] * wh[:, 1]
    a1 = (cb[2] - cb[0]) * (cb[3] - cb[1])
    a2 = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    return inter / (a1 + a2 - inter)


def plan_without_expand(width, height, boxes, labels, photometric=True, rng=random):
    """The reference's `transform` draw order (Util.py:566-607) run by hand with the expand coin and its three draws removed:
    photometric, random_crop, flip.  -> (photo, canvas, crop, flip, boxes, labels); float32 arithmetic throughout."""
    boxes = np.array(boxes, F).reshape(-1, 4)
    labels = np.array(labels)
    photo = photometric_draws(rng) if photometric else ()
    ch, cw = height, width
    crop = (0, 0, ch, cw)
    done = False
    while not done:
        min_overlap = rng.choice([0., .1, .3, .5, .7, .9, None])
        if min_overlap is None:
            break
        for _ in range(50):
            scale_h = rng.uniform(0.3, 1)
            scale_w = rng.uniform(0.3, 1)
            new_h, new_w = int(scale_h * ch), int(scale_w * cw)
            if not 0.5 < new_h / new_w < 2:
                continue
            left = rng.randint(0, cw - new_w)
            right = left + new_w
            top = rng.randint(0, ch - new_h)
            bottom = top + new_h
            cb = np.array([left, top, right, bottom], F)
            if float(_iou(cb, boxes).max()) < min_overlap:
                continue
            centers = (boxes[:, :2] + boxes[:, 2:]) / F(2)
            inside = (centers[:, 0] > left) & (centers[:, 0] < right) & (centers[:, 1] > top) & (centers[:, 1] < bottom)
            if not inside.any():
                continue
            boxes, labels = boxes[inside], labels[inside]
            boxes[:, :2] = np.maximum(boxes[:, :2], cb[:2]) - cb[:2]
            boxes[:, 2:] = np.minimum(boxes[:, 2:], cb[2:]) - cb[:2]
            crop = (top, left, new_h, new_w)
            done = True
            break
    flip = False
    if rng.random() < .5:
        flip = True
        img_w = F(crop[3])
        x0 = img_w - boxes[:, 0] - F(1)
        x2 = img_w - boxes[:, 2] - F(1)
        boxes = np.stack((x2, boxes[:, 1], x0, boxes[:, 3]), 1)
    return photo, (height, width, 0, 0), crop, flip, boxes, labels


def carry(boxes, crop_hw, rect, H, W):
    """boxes in a tile's crop frame (pixels) -> fractions of the (H, W) mosaic: divide by the crop size, clamp to [0, 1], scale to the
    rectangle, shift by its corner, divide by the frame -- float32, in this order"""
    ch, cw = crop_hw
    top, left, h, w = rect
    s = np.clip(np.asarray(boxes, F).reshape(-1, 4) / np.array([cw, ch, cw, ch], F), F(0), F(1))
    return (s * np.array([w, h, w, h], F) + np.array([left, top, left, top], F)) / np.array([W, H, W, H], F)


def select(boxes, H, W, min_box):
    """mask of the boxes at least min_box output pixels wide and high; the largest one (first on ties) where none is"""
    keep = ((boxes[:, 2] - boxes[:, 0]) * F(W) >= F(min_box)) & ((boxes[:, 3] - boxes[:, 1]) * F(H) >= F(min_box))
    if not keep.any():
        keep[int(np.argmax((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])))] = True
    return keep


def map_regions(canvas, crop, flip, boxes):
    """ignore boxes through a plan: shift by the placement, intersect with the crop window, drop what has no area, mirror"""
    boxes = np.array(boxes, F).reshape(-1, 4)
    ch, cw, top, left = canvas
    boxes = boxes + np.array([left, top, left, top], F)
    ct, cl, crop_h, crop_w = crop
    if (ct, cl, crop_h, crop_w) != (0, 0, ch, cw):
        cb = np.array([cl, ct, cl + crop_w, ct + crop_h], F)
        boxes[:, :2] = np.maximum(boxes[:, :2], cb[:2]) - cb[:2]
        boxes[:, 2:] = np.minimum(boxes[:, 2:], cb[2:]) - cb[:2]
    boxes = boxes[(boxes[:, 2] > boxes[:, 0]) & (boxes[:, 3] > boxes[:, 1])]
    if flip:
        x0 = F(crop_w) - boxes[:, 0] - F(1)
        x2 = F(crop_w) - boxes[:, 2] - F(1)
        boxes = np.stack((x2, boxes[:, 1], x0, boxes[:, 3]), 1)
    return boxes


def sample(index, sizes, boxes, labels, ignore=None, center=(0.25, 0.75), min_box=2.0, out_hw=(300, 300), rng=random):
    """One mosaic sample AFTER the coin `random() < mosaic` came up true.  sizes[i] = (h, w), boxes[i], labels[i] (class numbers) and
    ignore[i] of every image of the dataset.  -> dict(members, rects, plans [(photo, canvas, crop, flip)], boxes, labels, ignore)"""
    H, W = out_hw
    lo, hi = center
    members = [index] + [rng.randrange(len(sizes)) for _ in range(3)]
    cx = rng.randint(int(lo * W), int(hi * W))
    cy = rng.randint(int(lo * H), int(hi * H))
    rects = rectangles(cx, cy, H, W)
    plans, bs, ls, igs = [], [], [], []
    for i, rect in zip(members, rects):
        h, w = sizes[i]
        photo, canvas, crop, flip, b, l = plan_without_expand(w, h, boxes[i], labels[i], rng=rng)
        plans.append((photo, canvas, crop, flip))
        bs.append(carry(b, crop[2:], rect, H, W)); ls.append(l)
        if ignore is not None:
            igs.append(carry(map_regions(canvas, crop, flip, ignore[i]), crop[2:], rect, H, W))
    bs, ls = np.concatenate(bs), np.concatenate(ls)
    keep = select(bs, H, W, min_box)
    out = {"members": members, "rects": rects, "plans": plans, "boxes": bs[keep], "labels": ls[keep], "all_boxes": bs, "ignore": None}
    if ignore is not None:
        ig = np.concatenate(igs)
        out["ignore"] = ig[(ig[:, 2] > ig[:, 0]) & (ig[:, 3] > ig[:, 1])]
    return out


def compose(sources, plans, rects, out_hw):
    """(3, H, W) float32: tile k = preprocess_image(sources[k], h, w, canvas, crop, flip) pasted at rects[k]; plans[k] =
    (canvas, crop, flip).  Every element must be written exactly once."""
    H, W = out_hw
    out = np.full((3, H, W), np.nan, F)
    hits = np.zeros((H, W), np.int32)
    for img, (canvas, crop, flip), (top, left, h, w) in zip(sources, plans, rects):
        out[:, top:top + h, left:left + w] = O.preprocess_image(img, h, w, canvas=canvas, crop=crop, flip=flip)
        hits[top:top + h, left:left + w] += 1
    assert (hits == 1).all(), "the rectangles do not tile the frame"
    return out

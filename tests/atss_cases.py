"""The cases of tests/test_atss_cpu.py and tests/test_atss_gpu.py: four prior sets, the boxes that exercise the rule's edges, and the
reference results, computed once per process.

Prior sets (cells per level x priors per cell):
    "g5321"  grids (5, 3, 2, 1) x (4, 6, 6, 4), P = 182: one 256 block, a level of fewer cells than topk = 9, a level of one cell
    "g8421"  grids (8, 4, 2, 1) x (4, 6, 6, 4), P = 380: crosses a 256 block, not a multiple of 64; every cell centre a dyadic number
    "ssd300" create_priors_ssd300, P = 8732
    "ssd512" create_priors_ssd512, P = 24564 (4096 cells in level 0, seven levels)
The two small sets are built as create_priors_ssd300 builds its own (ratios 1, 2, 1/2 (+ 3, 1/3) and the extra square after 1).

Boxes of image 0 of every set, in this order: centre exactly on a cell corner of the dyadic grids (0.5, 0.5: four equidistant cells in
every level with an even grid), centre exactly on a prior centre of grid 8 (0.4375, 0.4375), two identical boxes, a box too small to
hold a prior centre, a zero-width box, a box with a NaN coordinate, then random boxes (sides 0.02 .. 0.9).  The assignment batches
give "g8421" and "ssd300" a second image of 130 random boxes (past the 128 kept in LDS).  The loss batches add an image whose only box
is the too-small one: an image without a positive beside images that have some.

`python tests/atss_cases.py --record` writes tests/golden/atss_ref_distance.json (numbers only): the distance of the float32
restatements of the "ciou" and focal terms from the float64 ones on the loss batches."""
import json
import os
import sys
from collections import namedtuple
from math import sqrt

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.join(os.path.dirname(_HERE), "oracle")):      # (`python tests/atss_cases.py` runs without tests/conftest.py)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import atss_ref as AR
import ssd_oracle as O

F = np.float32
GOLDEN = os.path.join(_HERE, "golden", "atss_ref_distance.json")
SETS = ("g5321", "g8421", "ssd300", "ssd512")
TOPKS = (1, 9, 32)
CLASS_COUNTS = (21, 81)
FOCAL = (0.25, 2.0)             # (alpha, gamma) of the focal runs
NEG_POS_RATIO = 3
_RATIOS = {4: (1., 2., .5), 6: (1., 2., 3., .5, .333)}
_cache = {}

LossCase = namedtuple("LossCase", "loc conf boxes classes priors_cxcywh levels ignore")


def small_priors(grids, anchors):
    """create_priors_ssd300's construction on other grids: (P, 4) float32 cx, cy, w, h"""
    scales = np.linspace(0.15, 0.9, len(grids))
    out = []
    for k, (g, a) in enumerate(zip(grids, anchors)):
        s = scales[k]
        extra = sqrt(s * scales[k + 1]) if k + 1 < len(grids) else 1.
        for row in range(g):
            for col in range(g):
                for r in _RATIOS[a]:
                    out.append([(col + 0.5) / g, (row + 0.5) / g, s * sqrt(r), s / sqrt(r)])
                    if r == 1.:
                        out.append([(col + 0.5) / g, (row + 0.5) / g, extra, extra])
    return np.clip(np.asarray(out, np.float64).astype(F), 0, 1)


def prior_set(name):
    """(priors_cxcywh (P, 4) float32, levels = (cells, anchors))"""
    if name not in _cache:
        if name == "ssd300":
            pri, levels = O.create_priors_ssd300(), (tuple(g * g for g in (38, 19, 10, 5, 3, 1)), (4, 6, 6, 6, 4, 4))
        elif name == "ssd512":
            pri, levels = O.create_priors_ssd512(), (tuple(g * g for g in (64, 32, 16, 8, 4, 2, 1)), (4, 6, 6, 6, 6, 4, 4))
        else:
            grids = {"g5321": (5, 3, 2, 1), "g8421": (8, 4, 2, 1)}[name]
            pri, levels = small_priors(grids, (4, 6, 6, 4)), (tuple(g * g for g in grids), (4, 6, 6, 4))
        pri = np.ascontiguousarray(pri, F)
        pri.setflags(write=False)
        _cache[name] = (pri, levels)
    return _cache[name]


SPECIAL = np.asarray([[0.25, 0.3125, 0.75, 0.6875],            # centre (0.5, 0.5): a cell corner of every even grid
                      [0.3125, 0.3125, 0.5625, 0.5625],        # centre (0.4375, 0.4375): a prior centre of grid 8
                      [0.1, 0.15, 0.45, 0.6],                  # two identical boxes: the lower index keeps every prior
                      [0.1, 0.15, 0.45, 0.6],
                      [0.51, 0.51, 0.5102, 0.5103],            # no prior centre inside
                      [0.3, 0.2, 0.3, 0.7],                    # zero width
                      [np.nan, 0.2, 0.6, 0.7]], F)             # a NaN coordinate
TINY = SPECIAL[4:5]


def random_boxes(rng, n):
    w, h = rng.uniform(0.02, 0.9, n), rng.uniform(0.02, 0.9, n)
    x1, y1 = rng.uniform(0, 1 - w), rng.uniform(0, 1 - h)
    return np.stack([x1, y1, x1 + w, y1 + h], 1).astype(F)


def near_priors(rng, pri, n):
    """n ignore boxes: random priors, 5 % larger about their centre (IoU 0.9 with that prior, high with its neighbours)"""
    c = pri[rng.choice(pri.shape[0], n, replace=False)].astype(np.float64)
    half = c[:, 2:] * 0.525
    return np.concatenate([c[:, :2] - half, c[:, :2] + half], 1).astype(F)


def assign_boxes(name):
    """the batch of the assignment tests: one (n_i, 4) array per image"""
    rng = np.random.default_rng([SETS.index(name), 20261])
    out = [np.concatenate([SPECIAL, random_boxes(rng, 9)])]
    if name in ("g8421", "ssd300"):
        out.append(random_boxes(rng, 130))
    return out


def assignment(name, topk):
    """atss_ref.assign of the set's batch, computed once per process; callers must not write into it"""
    key = ("assign", name, topk)
    if key not in _cache:
        pri, levels = prior_set(name)
        _cache[key] = AR.assign(assign_boxes(name), pri, levels, topk)
    return _cache[key]


def loss_case(name, C):
    """the batch of the loss tests (topk 9): image 0 as in the assignment batch, image 1 without a positive, image 2 random boxes"""
    key = ("case", name, C)
    if key not in _cache:
        pri, levels = prior_set(name)
        rng = np.random.default_rng([SETS.index(name), C, 20262])
        boxes = [np.concatenate([SPECIAL, random_boxes(rng, 9)]), TINY.copy(), random_boxes(rng, 6)]
        if name == "ssd512":
            boxes = boxes[:2]
        bs, P = len(boxes), pri.shape[0]
        classes = [rng.integers(0, C - 1, b.shape[0]).astype(F) for b in boxes]
        loc = (rng.standard_normal((bs, P, 4)) * 0.5).astype(F)
        conf = (rng.standard_normal((bs, P, C)) * 2).astype(F)
        ignore = [near_priors(rng, pri, 3) for _ in range(bs)]
        for a in (loc, conf):
            a.setflags(write=False)
        _cache[key] = LossCase(loc, conf, boxes, classes, pri, levels, ignore)
    return _cache[key]


def loss_reference(name, C, with_ignore):
    """atss_ref.multibox_loss of the loss batch, computed once per process; callers must not write into it"""
    key = ("ref", name, C, with_ignore)
    if key not in _cache:
        c = loss_case(name, C)
        _cache[key] = AR.multibox_loss(c.loc, c.conf, c.boxes, c.classes, c.priors_cxcywh, c.levels, 9, c.ignore if with_ignore else None,
                                       NEG_POS_RATIO)
    return _cache[key]


def measure(sets=SETS):
    """d32 of the "ciou" and focal terms on every loss batch of these prior sets: the content of the fixture"""
    import torch
    out = {}
    for name in sets:
        for C in CLASS_COUNTS:
            c = loss_case(name, C)
            for with_ignore in (False, True):
                base = loss_reference(name, C, with_ignore)
                a, b = (AR.focal_side(c.conf, base, *FOCAL, dtype=dt) for dt in (torch.float32, torch.float64))
                out[f"{name}|C{C}|{'ign' if with_ignore else 'plain'}|focal"] = float(np.abs(a["dconf"] - b["dconf"]).max() / np.abs(b["dconf"]).max())
            a, b = (AR.box_side(c.loc, c.priors_cxcywh, base, "ciou", dtype=dt) for dt in (torch.float32, torch.float64))
            out[f"{name}|C{C}|ciou"] = float(np.abs(a["dloc"] - b["dloc"]).max() / np.abs(b["dloc"]).max())
    return out


def d32(key):
    if "gold" not in _cache:
        with open(GOLDEN) as f:
            _cache["gold"] = json.load(f)["d32"]
    return _cache["gold"][key]


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/atss_cases.py --record")
    m = measure()
    for k, v in m.items():
        print(k, v)
    with open(GOLDEN, "w") as f:
        json.dump({"what": "max |float32 restatement - float64| / max |float64| of dconf (focal, alpha 0.25, gamma 2) and dloc (ciou) of "
                           "tests/atss_ref.py on the loss batches of tests/atss_cases.py, CPU; written by `python tests/atss_cases.py --record`",
                   "d32": m}, f, indent=2)
        f.write("\n")

"""The cases of tests/test_focal_loss_gpu.py: geometry, loc, conf and boxes of tests/loss_regimes.make (tests/ignore_loss_cases.make for
those with ignore boxes) as they are, and the reference result of the matching (tests/ignore_loss_ref.py), computed once per process.
The `trained`, `tie_groups` and `many_boxes` regimes carry saturated rows with gaps of 40 .. 60 already.

One more regime, `extreme`, on top of `trained`: every fifth prior of an image and every second positive get, in every column with
probability 1/2 and in the positive's target column always, a logit drawn from {0, +-30, +-88, +-104, +-1e4} -- beyond where expf
under- and overflows in float32 -- so the term and its gradient must stay finite where a naive sigmoid / log would not.

`python tests/focal_loss_cases.py --record` writes tests/golden/focal_loss_ref_distance.json (numbers only)."""
import json
import os
import sys
from collections import namedtuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.join(os.path.dirname(_HERE), "oracle")):      # (`python tests/focal_loss_cases.py` runs without tests/conftest.py)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import focal_loss_ref as FR
import ignore_loss_cases as IC
import ignore_loss_ref as IR
import loss_regimes as LR

FocalCase = namedtuple("FocalCase", "loc conf boxes classes priors_cxcywh neg_pos_ratio ignore threshold overlap loc_loss")

EXTREME = np.asarray([0, 30, -30, 88, -88, 104, -104, 1e4, -1e4], np.float32)

# id: (source, loc_loss, extreme).  source = (regime, P, C, bs, seed of loss_regimes.make) or the id of a case of ignore_loss_cases
SPEC = {
    "trained-P777-C21-bs3": (("trained", 777, 21, 3, 401), "l1", False),
    "tie_groups-P1000-C81-bs1-ciou": (("tie_groups", 1000, 81, 1, 402), "ciou", False),
    "many_boxes-P1000-C21-bs3-ciou": (("many_boxes", 1000, 21, 3, 403), "ciou", False),
    "many_boxes-P777-C81-bs3": (("many_boxes", 777, 81, 3, 404), "l1", False),
    "tie_groups-P777-C21-bs1": (("tie_groups", 777, 21, 1, 405), "l1", False),
    "trained-P777-C21-bs3-ignore": ("trained-P777-C21-bs3-iou-0first", "l1", False),
    "trained-P1000-C81-bs3-ignore": ("trained-P1000-C81-bs3-ioa-0last", "l1", False),
    "trained-P8732-C21-bs2-ignore": ("trained-P8732-C21-bs2-iou-ssd_priors", "l1", False),
    "extreme-P777-C21-bs3": (("trained", 777, 21, 3, 406), "l1", True),
    "extreme-P1000-C81-bs1": (("trained", 1000, 81, 1, 407), "l1", True),
}
CASE_IDS = list(SPEC)
P8732_ID = "trained-P8732-C21-bs2-ignore"
IGNORE_IDS = [c for c in SPEC if isinstance(SPEC[c][0], str)]
_cache = {}


def _extreme_rows(conf, cls, seed):
    bs, P, C = conf.shape
    rng = np.random.default_rng([seed, 4242])
    conf = conf.copy()
    for i in range(bs):
        pos = np.nonzero(cls[i] != C - 1)[0]
        rows = np.union1d(np.arange(0, P, 5), pos[::2])
        draw = rng.choice(EXTREME, (rows.shape[0], C))
        take = rng.random((rows.shape[0], C)) < 0.5
        tc = cls[i, rows]
        take[tc != C - 1, tc[tc != C - 1]] = True
        conf[i, rows] = np.where(take, draw, conf[i, rows])
    return conf


def make(case_id):
    """-> (case, ignore_loss_ref.multibox_loss's result: the matching)"""
    source, loc_loss, extreme = SPEC[case_id]
    if isinstance(source, str):
        src = IC.make(source)
        ignore, thr, overlap = src.ignore, src.threshold, src.overlap
    else:
        src = LR.make(*source)
        ignore, thr, overlap = None, 0.5, "iou"
    boxes, classes = [np.asarray(b, np.float32) for b in src.boxes], [np.asarray(c, np.float32) for c in src.classes]
    conf = src.conf
    if extreme:
        pre = IR.multibox_loss(src.loc, conf, boxes, classes, ignore, src.priors_cxcywh, src.neg_pos_ratio, thr, overlap)
        conf = _extreme_rows(conf, pre["cls"], source[4])
    base = IR.multibox_loss(src.loc, conf, boxes, classes, ignore, src.priors_cxcywh, src.neg_pos_ratio, thr, overlap)
    return FocalCase(src.loc, conf, boxes, classes, src.priors_cxcywh, src.neg_pos_ratio, ignore, thr, overlap, loc_loss), base


def case_and_reference(case_id):
    """(FocalCase, matching), computed once per process and shared: callers must not write into either."""
    if case_id not in _cache:
        case, base = make(case_id)
        for v in [case.loc, case.conf, case.priors_cxcywh] + [a for a in base.values() if isinstance(a, np.ndarray)]:
            v.setflags(write=False)
        _cache[case_id] = (case, base)
    return _cache[case_id]


def reference(case_id, alpha, gamma, norm_mode=0, dtype=None):
    """the focal term of a case: focal_loss_ref.conf_side's dict (float64 unless dtype is given), computed once per process"""
    import torch
    key = (case_id, alpha, gamma, norm_mode, dtype)
    if key not in _cache:
        case, base = case_and_reference(case_id)
        _cache[key] = FR.conf_side(case.conf, base["cls"], base["ign"], base["n_pos"], alpha, gamma, dtype or torch.float64, norm_mode)
        _cache[key]["dconf"].setflags(write=False)
    return _cache[key]


def measure():
    """d32 of every case x parameter set: the content of the fixture"""
    out = {}
    for case_id in CASE_IDS:
        case, base = case_and_reference(case_id)
        for alpha, gamma in FR.PARAMS:
            out[f"{case_id}|{FR.param_id(alpha, gamma)}"] = FR.distance(case, base, alpha, gamma)
    return out


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/focal_loss_cases.py --record")
    d32 = measure()
    for k, v in d32.items():
        print(k, v)
    with open(FR.GOLDEN, "w") as f:
        json.dump({"d32": d32}, f, indent=2)
        f.write("\n")

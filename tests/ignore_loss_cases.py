"""The cases of tests/test_ignore_loss_gpu.py: inputs of tests/loss_regimes.py plus ignore boxes per image, and the reference result
(tests/ignore_loss_ref.py) of each, computed once per process.  tests/test_ignore_loss_cpu.py holds every case to the condition
that lets the selection be compared bit for bit: after the ignored priors are zeroed, each image's k-th and (k+1)-th largest ranked
values are bit-equal or >= 1e-4 apart (loss_regimes.boundary_ok).

Ignore boxes come from loss_regimes._boxes, the generator of the ground truth.  A half-trained network scores the priors over an
unlabelled object high -- that is what the ignore set is for -- so every second would-be-ignored prior gets a `hard` conf row here
with the background logit lowered by 8 (CE > 9): without the ignore path those rows are mined, with it they must not be."""
from collections import namedtuple

import numpy as np

import ignore_loss_ref as IR
import loss_regimes as LR
import ssd_oracle as O

IgnoreCase = namedtuple("IgnoreCase", "loc conf boxes classes priors_cxcywh neg_pos_ratio ignore threshold overlap")

SG = 128             # ignore (and GT) boxes of an image the first kernel keeps in LDS; the rest it reads from memory
COVER = np.asarray([[-1., -1., 2., 2.]], np.float32)          # covers the unit square and every prior: ioa is exactly 1


# id: (regime, P, C, bs, seed, overlap, threshold, per-image ignore lists: an int = that many drawn boxes, or a tag)
SPEC = {
    "trained-P777-C21-bs3-iou-0first": ("trained", 777, 21, 3, 1, "iou", 0.5, [0, 1, 5]),
    "trained-P1000-C81-bs3-ioa-0last": ("trained", 1000, 81, 3, 2, "ioa", 0.5, [5, 1, 0]),
    "tie_groups-P1000-C21-bs3-iou-thr0.3": ("tie_groups", 1000, 21, 3, 3, "iou", 0.3, [1, 5, 0]),
    "tie_groups-P777-C81-bs1-ioa-thr0.7": ("tie_groups", 777, 81, 1, 4, "ioa", 0.7, [5]),
    "k_exceeds_nonzero-P777-C21-bs1-iou-130boxes": ("k_exceeds_nonzero", 777, 21, 1, 20, "iou", 0.5, ["late"]),
    "k_exceeds_nonzero-P1000-C81-bs3-ioa": ("k_exceeds_nonzero", 1000, 81, 3, 6, "ioa", 0.5, [0, 5, 1]),
    "tie_groups-P1000-C21-bs1-iou-equals_gt": ("tie_groups", 1000, 21, 1, 7, "iou", 0.5, ["gt+1"]),
    "trained-P777-C81-bs3-ioa-cover": ("trained", 777, 81, 3, 8, "ioa", 0.5, ["cover", "cover+5", "cover"]),
    "trained-P777-C21-bs1-ioa-cover": ("trained", 777, 21, 1, 9, "ioa", 0.5, ["cover"]),
    "trained-P777-C21-bs1-ioa-zero_area": ("trained", 777, 21, 1, 10, "ioa", 0.5, ["zero+1"]),
    "trained-P1000-C81-bs1-iou-zero_area": ("trained", 1000, 81, 1, 11, "iou", 0.5, ["zero+1"]),
    "trained-P8732-C21-bs2-iou-ssd_priors": ("trained", 8732, 21, 2, 12, "iou", 0.5, [2, 0]),
}
CASE_IDS = list(SPEC)
N_IGN_ZERO_IDS = ("trained-P777-C21-bs3-iou-0first", "tie_groups-P777-C81-bs1-ioa-thr0.7")      # also run with every list emptied
_cache = {}


def _ignore_lists(rng, spec, boxes):
    out = []
    for i, what in enumerate(spec):
        if isinstance(what, int):
            out.append(LR._boxes(rng, what) if what else np.zeros((0, 4), np.float32))
            continue
        if what == "late":          # more boxes than are staged: one ordinary box, SG - 1 too small for any prior, two ordinary ones past SG
            tiny = LR._boxes(rng, SG - 1, smin=0.008, srange=0.004)
            out.append(np.concatenate([LR._boxes(rng, 1), tiny, LR._boxes(rng, 2)]).astype(np.float32))
            continue
        head, _, extra = what.partition("+")
        drawn = LR._boxes(rng, int(extra)) if extra else np.zeros((0, 4), np.float32)
        if head == "gt":
            first = np.asarray(boxes[i], np.float32).copy()
        elif head == "cover":
            first = COVER
        else:                                                   # "zero": no area (x1 == x2, y1 == y2), inside the image
            first = np.asarray([[0.4, 0.3, 0.4, 0.3]], np.float32)
        out.append(np.concatenate([first, drawn]).astype(np.float32))
    return out


def make(case_id):
    regime, P, C, bs, seed, overlap, thr, spec = SPEC[case_id]
    priors = O.create_priors_ssd300() if P == 8732 else None
    base = LR.make(regime, P, C, bs, 1000 + seed, priors=priors)
    rng = np.random.default_rng([seed, P, C])
    ignore = _ignore_lists(rng, spec, base.boxes)
    pri_xyxy = O.xywh_to_xyxy(base.priors_cxcywh)
    _, cls, _, _, _ = LR.R.match_priors(base.boxes, base.classes, pri_xyxy, C)
    pos = cls != C - 1
    ign = IR.ignored_mask(ignore, pri_xyxy, pos, thr, overlap)
    for attempt in range(50):
        r2 = np.random.default_rng([seed, P, C, attempt])
        conf = base.conf.copy()
        for i in range(bs):
            at = np.nonzero(ign[i])[0][::2]
            rows = LR._hard(r2, at.shape[0], C)
            rows[:, C - 1] -= np.float32(8)                     # background 8 lower: these rows lead the ranking unless they are ignored
            conf[i, at] = rows
        ranked = LR.ce_f32(conf, cls)
        ranked[pos | ign] = 0
        if all(LR.boundary_ok(ranked[i], min(base.neg_pos_ratio * int(pos[i].sum()), P)) for i in range(bs)) and \
                not ((ranked > 0) & (ranked < 1e-2)).any():
            return IgnoreCase(base.loc, conf, base.boxes, base.classes, base.priors_cxcywh, base.neg_pos_ratio, ignore, thr, overlap)
    raise RuntimeError(f"{case_id}: no draw met the boundary condition")


def reference(case, ignore=None):
    return IR.multibox_loss(case.loc, case.conf, case.boxes, case.classes, case.ignore if ignore is None else ignore, case.priors_cxcywh,
                            case.neg_pos_ratio, case.threshold, case.overlap)


def case_and_reference(case_id):
    """(IgnoreCase, reference result), computed once per process and shared: callers must not write into either."""
    if case_id not in _cache:
        case = make(case_id)
        ref = reference(case)
        for v in [case.loc, case.conf, case.priors_cxcywh] + [a for a in ref.values() if isinstance(a, np.ndarray)]:
            v.setflags(write=False)
        _cache[case_id] = (case, ref)
    return _cache[case_id]

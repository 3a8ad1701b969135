"""The cases of tests/test_box_loss_gpu.py: geometry, conf and boxes of tests/loss_regimes.py (tests/ignore_loss_cases.py for those with
ignore boxes), `loc` replaced per regime, and the reference result of the matching and the conf side (tests/ignore_loss_ref.py),
computed once per process.

With enc = the encoded matched box of each positive, the `loc` regimes are (non-positive rows keep N(0, 1)):
    noise     N(0, 1)
    near      enc + N(0, 0.5)
    far       enc +- 60 on l0, l1: no overlap with the matched box
    aspect    enc + (0, 0, +6, -6): the CIoU term is alive (accepted only if alpha * v >= 0.05 on at least half of the positives)
    inside    enc + (0, 0, -4, -4)
    around    enc + (0, 0, +4, +4)
    clamped   enc + N(0, 0.5), with l2 = 40 and l3 = -1000 on every third positive
The gradient of a row changes branch where two corners meet, where an intersection extent passes zero and where an exponent meets the
clamp (box_loss_ref.kink_distance).  A positive row within 1e-4 of such a place has its noise drawn again -- the regimes without
noise get N(0, 0.05) on such a row only --, and a case is accepted only when no positive row is left there: every positive row is
compared, none is left out."""
from collections import namedtuple

import numpy as np
import torch

import box_loss_ref as BR
import ignore_loss_cases as IC
import ignore_loss_ref as IR
import loss_regimes as LR

BoxCase = namedtuple("BoxCase", "loc conf boxes classes priors_cxcywh neg_pos_ratio ignore threshold overlap")

KINK = 1e-4
SG = 128             # GT boxes of an image the per-image kernel keeps in LDS; a positive of a later box reads it from memory
ZERO_AREA = np.asarray([0.4, 0.3, 0.4, 0.3], np.float32)

# id: (source, loc regime, seed).  source = (regime, P, C, bs, seed of loss_regimes.make) or the id of a case of ignore_loss_cases
SPEC = {
    "trained-P777-C21-bs3-noise": (("trained", 777, 21, 3, 301), "noise", 1),
    "trained-P1000-C81-bs1-near": (("trained", 1000, 81, 1, 302), "near", 2),
    "tie_groups-P1000-C21-bs3-far": (("tie_groups", 1000, 21, 3, 303), "far", 3),
    "trained-P777-C81-bs3-aspect": (("trained", 777, 81, 3, 304), "aspect", 4),
    "tie_groups-P1000-C21-bs1-inside": (("tie_groups", 1000, 21, 1, 305), "inside", 5),
    "tie_groups-P777-C81-bs1-around": (("tie_groups", 777, 81, 1, 306), "around", 6),
    "many_boxes-P1000-C81-bs3-noise": (("many_boxes", 1000, 81, 3, 307), "noise", 7),
    "many_boxes-P777-C21-bs3-near": (("many_boxes", 777, 21, 3, 308), "near", 8),
    "trained-P1000-C21-bs3-clamped": (("trained", 1000, 21, 3, 309), "clamped", 9),
    "trained-P777-C21-bs3-clamped": (("trained", 777, 21, 3, 320), "clamped", 15),
    "tie_groups-P777-C81-bs3-clamped": (("tie_groups", 777, 81, 3, 310), "clamped", 10),
    "trained-P777-C21-bs1-noise-zero_area": (("trained", 777, 21, 1, 311), "noise", 11),
    "trained-P777-C21-bs3-near-ignore": ("trained-P777-C21-bs3-iou-0first", "near", 12),
    "trained-P1000-C81-bs3-noise-ignore": ("trained-P1000-C81-bs3-ioa-0last", "noise", 13),
    "trained-P8732-C21-bs2-near-ignore": ("trained-P8732-C21-bs2-iou-ssd_priors", "near", 14),
}
CASE_IDS = list(SPEC)
FAR_ID, CLAMPED_IDS, P8732_ID = "tie_groups-P1000-C21-bs3-far", [c for c in SPEC if "clamped" in c], "trained-P8732-C21-bs2-near-ignore"
_cache = {}


def modes_of(case_id):
    """"ciou" needs ground-truth boxes of positive height"""
    return BR.MODES[:3] if "zero_area" in case_id else BR.MODES


def clamped_rows(n):
    return np.arange(n) % 3 == 0


def _draw(regime, rng, enc, n, jitter=False):
    """(n, 4) float32 offsets of the positives"""
    if regime == "noise":
        return rng.standard_normal((n, 4)).astype(np.float32)
    if regime in ("near", "clamped"):
        out = enc + rng.normal(0, 0.5, (n, 4))
        if regime == "clamped":
            third = clamped_rows(n)
            out[third, 2], out[third, 3] = 40.0, -1000.0
        return out.astype(np.float32)
    add = {"far": None, "aspect": (0, 0, 6, -6), "inside": (0, 0, -4, -4), "around": (0, 0, 4, 4)}[regime]
    if add is None:
        add = np.zeros((n, 4))
        add[:, :2] = 60.0 * rng.choice([-1.0, 1.0], (n, 2))
    out = enc + np.asarray(add, np.float64)
    if jitter:
        out = out + rng.normal(0, 0.05, (n, 4))
    return out.astype(np.float32)


def positive_rows(case, base):
    """(l, pri, g) float64 tensors of the positives of a case, in row-major order of (image, prior)"""
    pos = base["pos"]
    bs, P = pos.shape
    allb = np.concatenate([np.asarray(b, np.float32).reshape(-1, 4) for b in case.boxes], 0)
    t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64)
    return t(case.loc[pos]), t(np.broadcast_to(case.priors_cxcywh[None], (bs, P, 4))[pos]), t(allb[base["obj"][pos]])


ALIVE, ALIVE_SHARE = 0.05, 0.5


def aspect_alive(case, base):
    """share of the positives of a case whose CIoU aspect term alpha * v is at least ALIVE"""
    return float((BR.alpha_v(*positive_rows(case, base)).numpy() >= ALIVE).mean())


def make(case_id):
    """-> (case, matching and conf side, re-draws it took).  An `aspect` case whose ground truth leaves the aspect term alive on fewer
    than half of the positives (boxes about as wide as high, or wider) is not accepted: the next ground truth is drawn."""
    source, regime, seed = SPEC[case_id]
    if regime != "aspect":
        return _make(case_id, source)
    for k in range(20):
        out = _make(case_id, source[:4] + (source[4] + 1000 * k,))
        if aspect_alive(out[0], out[1]) >= ALIVE_SHARE:
            return out
    raise RuntimeError(f"{case_id}: no ground truth with alpha * v >= {ALIVE} on half of the positives")


def _make(case_id, source):
    _, regime, seed = SPEC[case_id]
    if isinstance(source, str):
        src = IC.make(source)
        ignore, thr, overlap = src.ignore, src.threshold, src.overlap
    else:
        src = LR.make(*source)
        ignore, thr, overlap = None, 0.5, "iou"
    boxes, classes = [np.asarray(b, np.float32) for b in src.boxes], [np.asarray(c, np.float32) for c in src.classes]
    if "zero_area" in case_id:            # a box without area: IoU 0 with every prior, its forced match makes prior 0 a positive
        boxes[0] = np.concatenate([boxes[0], ZERO_AREA[None]])
        classes[0] = np.concatenate([classes[0], np.zeros(1, np.float32)])
    with np.errstate(divide="ignore"):        # (the encoding of the box without area, which no regime used with it reads)
        base = IR.multibox_loss(src.loc, src.conf, boxes, classes, ignore, src.priors_cxcywh, src.neg_pos_ratio, thr, overlap)
    pos = base["pos"]
    n = int(pos.sum())
    rng = np.random.default_rng([seed, 77])
    enc = base["enc"].astype(np.float64)
    rows = _draw(regime, rng, enc, n)
    loc = np.array(src.loc, np.float32)
    for attempt in range(50):
        loc[pos] = rows
        case = BoxCase(loc, src.conf, boxes, classes, src.priors_cxcywh, src.neg_pos_ratio, ignore, thr, overlap)
        near = (BR.kink_distance(*positive_rows(case, base)) < KINK).numpy()
        if not near.any():
            return case, base, int(attempt)
        again = _draw(regime, np.random.default_rng([seed, 77, attempt]), enc, n, jitter=True)
        rows[near] = again[near]             # (a clamped row stays clamped: _draw sets its l2, l3 again)
    raise RuntimeError(f"{case_id}: positives left within {KINK} of a kink")


def case_and_reference(case_id):
    """(BoxCase, result of ignore_loss_ref.multibox_loss: matching and the conf side), computed once per process and shared: callers
    must not write into either."""
    if case_id not in _cache:
        case, base, _ = make(case_id)
        for v in [case.loc, case.conf, case.priors_cxcywh] + [a for a in base.values() if isinstance(a, np.ndarray)]:
            v.setflags(write=False)
        _cache[case_id] = (case, base)
    return _cache[case_id]


def reference(case_id, mode, norm_mode=0, dtype=torch.float64, variant=None):
    """the box term of a case in `dtype`: box_loss_ref.loc_side's dict"""
    case, base = case_and_reference(case_id)
    allb = np.concatenate([np.asarray(b, np.float32).reshape(-1, 4) for b in case.boxes], 0)
    return BR.loc_side(case.loc, case.priors_cxcywh, allb, base["pos"], base["obj"], mode, dtype, norm_mode, variant)

"""Which status ssd_multibox_loss_atss (csrc/loss.hip) and ssd_atss_assign (csrc/atss.hip) return for a defective call: the header's
order -- SSD_ERR_NULL, then SSD_ERR_BAD_SHAPE, then SSD_ERR_ALIGN, then SSD_ERR_WORKSPACE; where several defects meet, the first of
these classes is returned.  The level description is host memory that the entries read before anything else, so it is real here (a
NULL one is a defect of the first class); every device pointer is made up: all checks run before any launch."""
import ctypes
import itertools

import pytest
import torch

OK_PTR, ODD_PTR = 0x10000, 0x10004
OK, BAD_SHAPE, WORKSPACE, NULL, LAUNCH, ALIGN = 0, -1, -2, -3, -4, -5
CLASSES = ["null", "shape", "align", "ws"]
STATUS = {"null": NULL, "shape": BAD_SHAPE, "align": ALIGN, "ws": WORKSPACE}
NAN = float("nan")
P = 182


def _ints(*v):
    return (ctypes.c_int * len(v))(*v)


CELLS, ANCHORS = _ints(25, 9, 4, 1), _ints(4, 6, 6, 4)          # sums to P = 182
SHORT = _ints(25, 9, 4, 2)                                      # 186
ZERO = _ints(25, 9, 4, 0)

_LEVELS = [("topk", 9), ("n_levels", 4), ("level_cells", CELLS), ("level_anchors", ANCHORS)]
ARGS = {
    "ssd_multibox_loss_atss": [("loc", OK_PTR), ("conf", OK_PTR), ("gt_boxes", OK_PTR), ("gt_classes", OK_PTR), ("img_start", OK_PTR), ("bs", 2),
                               ("n_gt", 5), ("priors_cxcywh", OK_PTR), ("priors_xyxy", OK_PTR), ("P", P), ("n_classes", 21),
                               ("iou_threshold", 0.5), ("neg_pos_ratio", 3), ("norm_mode", 0), ("ign_boxes", OK_PTR), ("ign_start", OK_PTR),
                               ("n_ign", 3), ("ignore_threshold", 0.5), ("overlap_mode", 0), ("loc_mode", 0), ("conf_mode", 0),
                               ("focal_alpha", 0.25), ("focal_gamma", 2.0), ("match_mode", 1)] + _LEVELS +
                              [("losses", OK_PTR), ("obj", OK_PTR), ("cls", OK_PTR), ("ign", OK_PTR), ("dloc", OK_PTR), ("dconf", OK_PTR),
                               ("workspace", OK_PTR), ("ws_bytes", 0), ("stream", None)],
    "ssd_atss_assign": [("gt_boxes", OK_PTR), ("img_start", OK_PTR), ("bs", 2), ("n_gt", 5), ("priors_cxcywh", OK_PTR), ("priors_xyxy", OK_PTR),
                        ("P", P)] + _LEVELS + [("assign", OK_PTR), ("n_cand", OK_PTR), ("mean", OK_PTR), ("var", OK_PTR), ("n_acc", OK_PTR),
                                               ("workspace", OK_PTR), ("ws_bytes", 0), ("stream", None)],
}


def _each(cls, name, *values):
    return [(f"{name}={v}", {name: v}, cls) for v in values]


def _nulls(*names):
    return [(f"null:{n}", {n: None}, "null") for n in names]


def _odd(*names):
    return [(f"odd:{n}", {n: ODD_PTR}, "align") for n in names]


_LEVEL_DEFECTS = (_nulls("level_cells", "level_anchors") + _each("shape", "topk", 0, -1, 33) + _each("shape", "n_levels", 0, 9, 3) +
                  [("levels-sum", {"level_cells": SHORT}, "shape"), ("level-empty", {"level_cells": ZERO}, "shape")])
DEFECTS = {
    "ssd_multibox_loss_atss": _nulls("loc", "conf", "gt_boxes", "gt_classes", "img_start", "priors_cxcywh", "priors_xyxy", "losses", "obj", "cls",
                                     "workspace", "ign", "dloc") + _LEVEL_DEFECTS +
    _each("shape", "bs", 0) + _each("shape", "n_gt", 1) + _each("shape", "P", 0, 36001) + _each("shape", "n_classes", 1, 257) +
    _each("shape", "norm_mode", 2) + _each("shape", "loc_mode", 5) + _each("shape", "conf_mode", 2) + _each("shape", "match_mode", -1, 2) +
    _each("shape", "focal_alpha", 1.5, NAN) + _each("shape", "focal_gamma", -1.0) + _each("shape", "overlap_mode", 2) +
    _odd("loc", "priors_cxcywh", "priors_xyxy", "dloc", "workspace", "ign_boxes") + [("ws-1", {"ws_bytes": -1}, "ws")],
    "ssd_atss_assign": _nulls("gt_boxes", "img_start", "priors_cxcywh", "priors_xyxy", "assign", "workspace") + _LEVEL_DEFECTS +
    _each("shape", "bs", 0) + _each("shape", "n_gt", 0) + _each("shape", "P", 0, 36001) + _odd("priors_xyxy", "workspace") +
    [("ws-1", {"ws_bytes": -1}, "ws")],
}
# what is no defect: no ignore regions, forward only, the per-box outputs absent; match_mode 0 does not look at the level description
VALID = {
    "ssd_multibox_loss_atss": [{}, {"ign_start": None, "ign": None, "ign_boxes": None}, {"dloc": None, "dconf": None}, {"conf_mode": 1, "loc_mode": 4},
                               {"match_mode": 0, "level_cells": None, "level_anchors": None, "topk": 0, "n_levels": 0}, {"topk": 1}, {"topk": 32},
                               {"iou_threshold": NAN}],
    "ssd_atss_assign": [{}, {"n_cand": None, "mean": None, "var": None, "n_acc": None}, {"topk": 32}, {"priors_cxcywh": ODD_PTR}],
}


def cases(entry):
    """every single defect, and every pair that does not set one argument twice, with the status of the earlier class"""
    d = DEFECTS[entry]
    assert len({la for la, _, _ in d}) == len(d), entry
    out = [(la, ch, STATUS[cls]) for la, ch, cls in d]
    for (la, ca, sa), (lb, cb, sb) in itertools.combinations(d, 2):
        if set(ca) & set(cb):
            continue
        if "P" in ca or "P" in cb:
            continue                                   # (another P changes whether the levels sum to it: not a pair of independent defects)
        out.append((f"{la}+{lb}", {**ca, **cb}, STATUS[min(sa, sb, key=CLASSES.index)]))
    return out


def call(lib, entry, changes):
    v = {**dict(ARGS[entry]), **{k: c for k, c in changes.items() if k != "ws_bytes"}}
    if entry == "ssd_atss_assign":
        need = lib.ssd_atss_assign_workspace(2, P)
    else:
        need = lib.ssd_multibox_loss_atss_workspace(2, P, 5, 3) if v["match_mode"] == 1 else lib.ssd_multibox_loss_focal_workspace(2, P, 5, 3)
    assert need > 0
    v["ws_bytes"] = need + changes.get("ws_bytes", 0)
    return getattr(lib, entry)(*[v[name] for name, _ in ARGS[entry]])


@pytest.fixture(scope="module")
def lib():
    """Every defective call is refused before anything is enqueued, so the made-up pointers are never dereferenced; where a GPU is
    present the tests still do not run, so that no made-up pointer can ever reach a launch on a shared machine."""
    if torch.cuda.is_available():
        pytest.skip("made-up pointers: only where no launch can succeed")
    from objectdetection_ssd_amd import _lib
    return _lib.load()


def test_the_tables_match_the_signatures():
    from objectdetection_ssd_amd import _lib
    for e in ARGS:
        assert len(ARGS[e]) == len(_lib.SIGNATURES[e][1]), e
    assert set(ARGS) == set(DEFECTS) == set(VALID)


@pytest.mark.parametrize("entry", list(ARGS))
def test_every_defect_and_pair_returns_the_status_of_the_header_order(lib, entry):
    got = [(la, call(lib, entry, ch), want) for la, ch, want in cases(entry)]
    wrong = [g for g in got if g[1] != g[2]]
    assert not wrong, f"{entry}: {len(wrong)} of {len(got)} statuses differ (defects, got, pinned): {wrong[:20]}"


@pytest.mark.parametrize("entry", list(ARGS))
def test_what_is_no_defect_is_accepted(lib, entry):
    """past every check the entry launches; without a device that is SSD_ERR_LAUNCH, never one of the refusals"""
    got = [(ch, call(lib, entry, ch)) for ch in VALID[entry]]
    assert all(st in (OK, LAUNCH) for _, st in got), got


def test_the_workspace_of_match_mode_1_holds_the_keys(lib):
    for bs, p, n_gt in ((2, P, 5), (32, 8732, 100), (1, 24564, 7)):
        base = lib.ssd_multibox_loss_focal_workspace(bs, p, n_gt, 0)
        keys = lib.ssd_atss_assign_workspace(bs, p)
        assert keys == (8 * bs * p + 255) // 256 * 256 and lib.ssd_multibox_loss_atss_workspace(bs, p, n_gt, 0) == base + keys
    assert lib.ssd_atss_assign_workspace(0, P) == 0 and lib.ssd_multibox_loss_atss_workspace(2, 0, 5, 0) == 0
    # match_mode 0 asks for no more than ssd_multibox_loss_focal does
    assert call(lib, "ssd_multibox_loss_atss", {"match_mode": 0}) in (OK, LAUNCH)

"""COCO evaluator on the device (Util.CocoEvaluator / evaluate_coco, csrc/map_eval.hip) against the protocol restatement
(tests/coco_protocol_ref.py).  Every comparison is bit-exact, NaN positions included: the overlaps are reproducible float32, each
precision is one division of two integers, and the means are the same numpy calls on both sides."""
import numpy as np
import pytest
import torch

import coco_protocol_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SMALL = dict(thresholds=(0.5,), area_ranges=(("all", 0, 1e10),), max_dets=(100,))
DEFAULT = dict(thresholds=R.IOU_THRESHOLDS, area_ranges=R.AREA_RANGES, max_dets=R.MAX_DETS)
ALL_CROWD, EMPTY, LONG_IMAGE, NO_OBJECTS = 3, 7, 10, 5
_sets, _refs = {}, {}


def make_set(n_classes, n_img=120, seed=321):
    """Seeded set in pixels, in the manner of test_eval_protocol_gpu.make_set: objects 8..300 pixels on a side (all three sized ranges
    are populated), about 10 % crowd, class 3 all crowd, class 7 without objects, duplicated objects; for about a third of the objects
    an area below the box's (a mask's), which moves some across a range bound; up to 120 detections per image scattered around the
    objects, a tenth of them exact copies, scores on a 50-value grid, every seventh image without detections, image 5 without
    objects, detections of classes outside the range, image 10 with 150 detections of a single class."""
    if (n_classes, n_img, seed) in _sets:
        return _sets[(n_classes, n_img, seed)]
    rng = np.random.default_rng(seed + n_classes)
    gt_b, gt_c, gt_w, gt_a = [], [], [], []
    for i in range(n_img):
        n = 1 + min(int(rng.poisson(2.0)), 9)
        xy = rng.uniform(0, 340, (n, 2))
        wh = np.exp(rng.uniform(np.log(8), np.log(300), (n, 2)))
        b = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        c = rng.integers(0, n_classes, n).astype(np.int64)
        if i % 3 == 0:                                                     # a duplicate of the first box, same class
            b, c = np.concatenate([b, b[:1]]), np.concatenate([c, c[:1]])
        c[c == EMPTY] = EMPTY + 1
        w = (rng.uniform(size=len(c)) < .1) | (c == ALL_CROWD)
        a = R.box_area(b)
        a = np.where(rng.uniform(size=len(c)) < .35, a * rng.uniform(.3, .9, len(c)).astype(np.float32), a).astype(np.float32)
        gt_b.append(b); gt_c.append(c); gt_w.append(w.astype(np.uint8)); gt_a.append(a)
    gt_b[NO_OBJECTS], gt_c[NO_OBJECTS] = np.zeros((0, 4), np.float32), np.zeros(0, np.int64)
    gt_w[NO_OBJECTS], gt_a[NO_OBJECTS] = np.zeros(0, np.uint8), np.zeros(0, np.float32)
    det_b, det_c, det_s = [], [], []
    for i in range(n_img):
        n = int(rng.integers(0, 121)) if i % 7 else 0
        if i == LONG_IMAGE:
            n = 150
        src_b, src_c = (gt_b[i], gt_c[i]) if len(gt_b[i]) else (gt_b[0], gt_c[0])     # image 5 has detections and no objects
        k = rng.integers(0, len(src_b), n)
        size = np.tile(src_b[k][:, 2:] - src_b[k][:, :2], 2)
        b = src_b[k] + (rng.normal(0, .07, (n, 4)) * size).astype(np.float32)
        b = np.stack([np.minimum(b[:, 0], b[:, 2]), np.minimum(b[:, 1], b[:, 3]),
                      np.maximum(b[:, 0], b[:, 2]) + np.float32(1), np.maximum(b[:, 1], b[:, 3]) + np.float32(1)], 1).astype(np.float32)
        exact = rng.uniform(size=n) < .1
        b[exact] = src_b[k][exact]                                       # exact copies: overlap 1 with a box and with its duplicate
        c = np.where(rng.uniform(size=n) < .8, src_c[k], rng.integers(0, n_classes + 2, n)).astype(np.int64)
        if i == LONG_IMAGE:
            c[:] = src_c[0]
        det_b.append(b); det_c.append(c)
        det_s.append((rng.integers(1, 50, n) / np.float32(50)).astype(np.float32))
    out = (det_b, det_c, det_s, gt_b, gt_c, gt_w, gt_a)
    _sets[(n_classes, n_img, seed)] = out
    return out


def ref(n_classes, cfg_name, n_img=120):
    """The restatement's result, computed once per configuration and never changed."""
    key = (n_classes, cfg_name, n_img)
    if key not in _refs:
        _refs[key] = R.evaluate(*make_set(n_classes, n_img), n_classes=n_classes, **(DEFAULT if cfg_name == "default" else SMALL))
    return _refs[key]


def _t(parts):
    return [torch.from_numpy(np.ascontiguousarray(p)).to(DEV) for p in parts]


def _kw(cfg):
    return dict(iou_thresholds=cfg["thresholds"], area_ranges=cfg["area_ranges"], max_dets=cfg["max_dets"])


def check_against_ref(res, m):
    for k in ("tp", "ignored"):
        assert res[k].dtype == torch.uint16 and res[k].is_cuda and tuple(res[k].shape) == m[k].shape
        assert np.array_equal(res[k].cpu().numpy(), m[k]), k
    assert res["rank"].dtype == torch.int32 and res["rank"].is_cuda and np.array_equal(res["rank"].cpu().numpy(), m["rank"])
    for k in ("n_gt", "n_det", "tp_count"):
        assert res[k].dtype == np.int64 and np.array_equal(res[k], m[k]), k
    for k in ("precision", "ap", "recall"):
        assert res[k].dtype == np.float64 and res[k].shape == m[k].shape
        assert res[k].tobytes() == m[k].tobytes(), k                         # NaN positions and payloads included
    assert list(res["stats"]) == list(m["stats"])
    for k in m["stats"]:
        assert np.array_equal(np.float64(res["stats"][k]), m["stats"][k], equal_nan=True), (k, res["stats"][k], m["stats"][k])


def test_the_seeded_set_does_what_it_is_meant_to():
    """Asserted on the restatement's output, so that the comparisons below cover what they claim."""
    det_b, det_c, det_s, gt_b, gt_c, gt_w, gt_a = make_set(80)
    m = ref(80, "default")
    tp, ign = m["tp"], m["ignored"]
    # in "all" nothing is outside the range, so an ignored detection there was matched to a crowd region
    assert (ign[:, 0] != 0).any()
    # a detection whose class has no object in its image is unmatched everywhere: ignored in a sized range = by its own area
    img = np.concatenate([np.full(len(b), i) for i, b in enumerate(det_b)])
    dc = np.concatenate(det_c)
    lonely = np.asarray([0 <= dc[d] < 80 and not (gt_c[img[d]] == dc[d]).any() for d in range(len(dc))])
    assert lonely.sum() > 50
    for a in (1, 2, 3):
        assert (ign[lonely, a] == 0x3FF).any() and (ign[lonely, a] == 0).any()
        assert ((tp[:, 0] & 1) & (ign[:, a] & 1)).any()                      # true positive in "all", ignored in the sized range
    assert not tp[lonely].any() and not ign[lonely, 0].any()
    assert (m["rank"] >= 100).any() and m["rank"].max() == 149 and (m["rank"] == -1).any()
    # an object whose sized range its area decides, not its box
    box_a, area = R.box_area(np.concatenate(gt_b)), np.concatenate(gt_a)
    assert any((((box_a < lo) | (box_a > hi)) != ((area < lo) | (area > hi))).any() for _, lo, hi in R.AREA_RANGES[1:])
    assert .05 < np.concatenate(gt_w).mean() < .2
    assert (m["n_gt"][:, ALL_CROWD] == 0).all() and (m["n_gt"][:, EMPTY] == 0).all() and m["n_det"][ALL_CROWD] > 0
    assert np.isnan(m["ap"][:, :, ALL_CROWD]).all() and np.isnan(m["ap"][:, :, EMPTY]).all()
    assert (m["n_gt"][1:].sum(1) > 20).all()
    assert 0.02 < m["stats"]["AP"] < 0.98
    assert all(not np.isnan(v) for v in m["stats"].values())
    assert m["stats"]["AR_1"] < m["stats"]["AR_10"] <= m["stats"]["AR_100"]


@pytest.mark.parametrize("n_classes,cfg_name", [(80, "default"), (20, "small")])
def test_seeded_set_vs_restatement(n_classes, cfg_name):
    from objectdetection_ssd_amd import Util
    cfg = DEFAULT if cfg_name == "default" else SMALL
    res = Util.evaluate_coco(*[_t(a) for a in make_set(n_classes)], n_classes=n_classes, **_kw(cfg))
    assert res["iou_thresholds"] == cfg["thresholds"] and res["max_dets"] == cfg["max_dets"]
    assert [n for n, _, _ in res["area_ranges"]] == [n for n, _, _ in cfg["area_ranges"]]
    m = ref(n_classes, cfg_name)
    check_against_ref(res, m)
    assert 0.02 < res["stats"]["AP"] < 0.98


@pytest.mark.parametrize("name", sorted(R.HAND_CASES))
def test_hand_cases_on_the_device(name):
    from objectdetection_ssd_amd import Util
    case = R.HAND_CASES[name]
    lists, cfg = R.hand_case_inputs(case)
    res = Util.evaluate_coco(*[_t(a) for a in lists], n_classes=1, **_kw(cfg))
    R.check_hand_case(case, res["tp"].cpu().numpy(), res["ignored"].cpu().numpy(), res["n_gt"], res["ap"], res["recall"])
    assert res["rank"].cpu().tolist() == list(range(len(case["det"])))


def _padded(det_b, det_c, det_s, gt_b, K=200):
    """(B,K,4), (B,K) int64, (B,K), count from the lists; rows past the count hold an object-sized box of a valid class with score
    1.0, so that a kernel that reads them changes the result."""
    B = len(det_b)
    boxes = np.tile(np.asarray([10, 10, 60, 60], np.float32), (B, K, 1))
    classes = np.full((B, K), 1, np.int64)
    scores = np.ones((B, K), np.float32)
    count = np.zeros(B, np.int32)
    for i in range(B):
        n = len(det_b[i])
        if len(gt_b[i]):
            boxes[i, n:] = gt_b[i][0]
        boxes[i, :n], classes[i, :n], scores[i, :n], count[i] = det_b[i], det_c[i], det_s[i], n
    return [torch.from_numpy(a).to(DEV) for a in (boxes, classes, scores, count)]


def _same(r, first):
    for k in ("tp", "ignored"):
        assert torch.equal(r[k].view(torch.int16), first[k].view(torch.int16)), k
    assert torch.equal(r["rank"], first["rank"])
    for k in ("ap", "precision", "recall", "tp_count", "n_gt", "n_det"):
        assert r[k].tobytes() == first[k].tobytes(), k
    assert {k: np.float64(v).tobytes() for k, v in r["stats"].items()} == {k: np.float64(v).tobytes() for k, v in first["stats"].items()}


def test_batch_split_and_input_layout_do_not_change_a_bit():
    from objectdetection_ssd_amd import Util
    n_img = 120
    data = make_set(80)
    lists = [_t(a) for a in data]
    results = []
    for step in (n_img, 32, 1):
        ev = Util.CocoEvaluator(80)
        for s in range(0, n_img, step):
            ev.add_batch(*[a[s:s + step] for a in lists[:3]], None, *[a[s:s + step] for a in lists[3:]])
        results.append(ev.compute())
    for step in (n_img, 32):                                               # padded tensors (K = 200), lists of ground truth
        ev = Util.CocoEvaluator(80)
        for s in range(0, n_img, step):
            pb, pc, ps, cnt = _padded(*[a[s:s + step] for a in data[:4]])
            ev.add_batch(pb, pc, ps, cnt, *[a[s:s + step] for a in lists[3:]])
        results.append(ev.compute())
    check_against_ref(results[0], ref(80, "default"))
    for r in results[1:]:
        _same(r, results[0])


def test_both_sides_of_the_register_path_limits():
    """The matching kernel keeps an image of at most 256 rows and 64 boxes in registers and walks longer ones through the
    workspace: images on either side of both limits, as lists and as padded tensors, against the restatement."""
    from objectdetection_ssd_amd import Util
    rng = np.random.default_rng(78)
    shapes = [(256, 64), (257, 64), (256, 65), (257, 65), (40, 6)]
    cfg = dict(thresholds=(0.5, 0.6, 0.75, 0.9), area_ranges=R.AREA_RANGES, max_dets=(10, 200))
    gt_b, gt_c, gt_w, gt_a, det_b, det_c, det_s = [], [], [], [], [], [], []
    for n, g in shapes:
        xy = rng.uniform(0, 300, (g, 2)); wh = np.exp(rng.uniform(np.log(10), np.log(200), (g, 2)))
        b = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        b[g // 2] = b[0]                                                   # a duplicate: overlap ties
        c = rng.integers(0, 2, g).astype(np.int64)
        c[g // 2] = c[0]
        gt_b.append(b); gt_c.append(c); gt_w.append((rng.uniform(size=g) < .15).astype(np.uint8))
        gt_a.append((R.box_area(b) * rng.uniform(.4, 1., g).astype(np.float32)).astype(np.float32))
        k = rng.integers(0, g, n)
        size = np.tile(b[k][:, 2:] - b[k][:, :2], 2)
        det_b.append((b[k] + rng.normal(0, .04, (n, 4)) * size).astype(np.float32))
        det_c.append(np.where(rng.uniform(size=n) < .9, c[k], rng.integers(0, 3, n)).astype(np.int64))
        det_s.append((rng.integers(1, 20, n) / np.float32(20)).astype(np.float32))
    m = R.evaluate(det_b, det_c, det_s, gt_b, gt_c, gt_w, gt_a, n_classes=2, **cfg)
    assert m["tp"].any() and m["ignored"][:, 0].any() and (m["rank"] > 100).any()
    assert all(((m["tp"][:, a] >> t) & 1).any() for a in range(4) for t in range(4))
    res = Util.evaluate_coco(_t(det_b), _t(det_c), _t(det_s), _t(gt_b), _t(gt_c), _t(gt_w), _t(gt_a), n_classes=2, **_kw(cfg))
    check_against_ref(res, m)
    ev = Util.CocoEvaluator(2, **_kw(cfg))
    pb, pc, ps, cnt = _padded(det_b, det_c, det_s, gt_b, K=300)
    ev.add_batch(pb, pc, ps, cnt, _t(gt_b), _t(gt_c), _t(gt_w), _t(gt_a))
    check_against_ref(ev.compute(), m)


def test_degenerate_boxes():
    """A zero-area detection on a zero-area object: the overlap is 0/0 = NaN, which never matches, so the detection is unmatched at
    every threshold and claims nothing -- a false positive in every area range that holds area 0 ("all" and "small" of the
    defaults, and all four ranges of the second configuration).  In "medium" and "large" rule 6 makes an unmatched detection of
    area 0 ignored.  The ordinary detection after it still gets the ordinary object."""
    from objectdetection_ssd_amd import Util
    gt_b = [np.asarray([[5, 5, 5, 5], [20, 20, 40, 40]], np.float32)]
    det_b = [np.asarray([[5, 5, 5, 5], [20, 20, 40, 40]], np.float32)]
    zeros, sc = [np.zeros(2, np.int64)], [np.asarray([.9, .8], np.float32)]
    wide = (("all", 0, 1e10), ("b", 0, 1), ("c", 0, 500), ("d", 0, 1e5))
    for ranges, fp_in in ((R.AREA_RANGES, (0, 1)), (wide, (0, 1, 2, 3))):
        m = R.evaluate(det_b, zeros, sc, gt_b, zeros, None, None, 1, R.IOU_THRESHOLDS, ranges, R.MAX_DETS)
        res = Util.evaluate_coco(_t(det_b), _t(zeros), _t(sc), _t(gt_b), _t(zeros), n_classes=1, area_ranges=ranges)
        check_against_ref(res, m)
        tp, ign = res["tp"].cpu().numpy(), res["ignored"].cpu().numpy()
        assert not tp[0].any()
        for a in range(4):
            assert ign[0, a] == (0 if a in fp_in else 0x3FF)
        assert tp[1, 0] == 0x3FF and res["n_gt"][0, 0] == 2 and res["tp_count"][:, 0, -1, 0].tolist() == [1] * 10


def _packed(n_classes, n_img=32):
    det_b, det_c, det_s, gt_b, gt_c, gt_w, gt_a = [a[:n_img] for a in make_set(n_classes)]
    pb, pc, ps, cnt = _padded(det_b, det_c, det_s, gt_b)
    gb = torch.from_numpy(np.concatenate(gt_b)).to(DEV)
    gc = torch.from_numpy(np.concatenate(gt_c)).to(DEV, torch.int32)
    gw = torch.from_numpy(np.concatenate(gt_w)).to(DEV)
    ga = torch.from_numpy(np.concatenate(gt_a)).to(DEV)
    off = torch.tensor(np.cumsum([0] + [len(b) for b in gt_b]), dtype=torch.int32, device=DEV)
    return (pb, pc.to(torch.int32), ps, cnt), (gb, gc, gw, ga, off), (det_b, det_c, det_s, gt_b, gt_c, gt_w, gt_a)


def test_matching_is_launched_once_per_batch_whatever_the_configuration():
    from objectdetection_ssd_amd import Util, ops
    det, (gb, gc, gw, ga, off), _ = _packed(20)
    ten_four_three = dict(iou_thresholds=R.IOU_THRESHOLDS, area_ranges=R.AREA_RANGES, max_dets=R.MAX_DETS)
    for kw in (_kw(SMALL), ten_four_three):
        before = dict(ops.launch_counts)
        ev = Util.CocoEvaluator(20, **kw)
        for _ in range(3):
            ev.add_batch(*det, gb, gc, gw, ga, gt_offsets=off)
            assert ops.launch_counts["coco_match"] - before["coco_match"] == _ + 1
        ev.compute()
        assert ops.launch_counts["coco_match"] - before["coco_match"] == 3
        assert ops.launch_counts["coco_ap"] - before["coco_ap"] == 1
        assert ops.launch_counts["eval_match"] == before["eval_match"] and ops.launch_counts["eval_ap"] == before["eval_ap"]


def test_add_batch_does_not_wait_for_the_device():
    """Padded device detections and packed device ground truth under torch.cuda.set_sync_debug_mode("error"): any synchronising call
    inside add_batch raises.  The result is the restatement's."""
    from objectdetection_ssd_amd import Util
    det, (gb, gc, gw, ga, off), lists = _packed(80)
    ev = Util.CocoEvaluator(80)
    ev.add_batch(*det, gb, gc, gw, ga, gt_offsets=off)                      # first use: workspaces are allocated here
    ev.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev.add_batch(*det, gb, gc, gw, ga, gt_offsets=off)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    check_against_ref(ev.compute(), R.evaluate(*lists, n_classes=80, **DEFAULT))


def test_reset_repeated_compute_and_adding_after_compute():
    from objectdetection_ssd_amd import Util
    lists = [_t(a) for a in make_set(80)]
    part = lambda lo, hi: ([a[lo:hi] for a in lists[:3]], [a[lo:hi] for a in lists[3:]])      # noqa: E731
    ev = Util.CocoEvaluator(80)
    with pytest.raises(RuntimeError, match="no batch"):
        ev.compute()
    d, g = part(0, 40)
    ev.add_batch(*d, None, *g)                                             # something to forget
    ev.reset()
    with pytest.raises(RuntimeError, match="no batch"):
        ev.compute()
    d, g = part(0, 70)
    ev.add_batch(*d, None, *g)
    first, again = ev.compute(), ev.compute()
    _same(again, first)
    assert first["tp"].shape[0] < ref(80, "default")["tp"].shape[0]
    d, g = part(70, 120)
    ev.add_batch(*d, None, *g)                                             # adding after compute()
    check_against_ref(ev.compute(), ref(80, "default"))

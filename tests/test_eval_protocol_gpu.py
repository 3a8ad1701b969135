"""Detection evaluator on the device (Util.DetectionEvaluator / evaluate_detections, csrc/map_eval.hip) against the protocol
restatement (tests/eval_protocol_ref.py).  Bars: true-positive / ignored masks and the counts bit-exact; "11point" / "101point" AP
bit-exact, NaN positions included (each table entry is a maximum of correctly rounded integer quotients and the mean is the same
numpy call on both sides); "all" AP within n_tp * 2**-52 per class, n_tp that class's true positives (a sum of n_tp terms <= 1 taken
in a different order, divided by n_gt >= n_tp) -- derived, not measured."""
import os

import numpy as np
import pytest
import torch

import eval_protocol_ref as R
import ssd_oracle as O
from test_oracle_golden import _map_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWEEP = tuple(0.5 + 0.05 * k for k in range(10))
_sets, _refs = {}, {}


def make_set(n_classes, n_img=600, seed=123):
    """Seeded set in the manner of test_get_map_large_with_ties_vs_oracle: up to 200 detections per image scattered around the
    ground truth, scores on a 50-value grid (ties are common), every seventh image without detections, one image without ground
    truth, duplicated ground-truth boxes (IoU ties), about 15 % difficult objects, class 3 all difficult, class 7 without objects,
    some detections of classes outside the range."""
    if (n_classes, n_img, seed) in _sets:
        return _sets[(n_classes, n_img, seed)]
    rng = np.random.default_rng(seed + n_classes)
    gt_b, gt_c, gt_d = [], [], []
    for i in range(n_img):
        n = 1 + min(int(rng.poisson(2.0)), 9)
        x1 = rng.uniform(0, .6, n); y1 = rng.uniform(0, .6, n)
        w = rng.uniform(.08, .6, n); h = rng.uniform(.08, .6, n)
        b = np.stack([x1, y1, np.minimum(x1 + w, 1.), np.minimum(y1 + h, 1.)], 1).astype(np.float32)
        c = rng.integers(0, n_classes, n).astype(np.int64)
        if i % 3 == 0:                                                     # a duplicate of the first box, same class
            b, c = np.concatenate([b, b[:1]]), np.concatenate([c, c[:1]])
        c[c == 7] = 8
        d = (rng.uniform(size=len(c)) < .15) | (c == 3)
        gt_b.append(b); gt_c.append(c); gt_d.append(d.astype(np.uint8))
    gt_b[5], gt_c[5], gt_d[5] = np.zeros((0, 4), np.float32), np.zeros(0, np.int64), np.zeros(0, np.uint8)
    det_b, det_c, det_s = [], [], []
    for i in range(n_img):
        n = int(rng.integers(0, 201)) if i % 7 else 0
        src_b, src_c = (gt_b[i], gt_c[i]) if len(gt_b[i]) else (gt_b[0], gt_c[0])     # image 5 has detections and no objects
        k = rng.integers(0, len(src_b), n)
        b = src_b[k] + rng.normal(0, .04, (n, 4)).astype(np.float32)
        b = np.stack([np.minimum(b[:, 0], b[:, 2]), np.minimum(b[:, 1], b[:, 3]),
                      np.maximum(b[:, 0], b[:, 2]) + np.float32(.01), np.maximum(b[:, 1], b[:, 3]) + np.float32(.01)], 1).astype(np.float32)
        exact = rng.uniform(size=n) < .1
        b[exact] = src_b[k][exact]                                       # exact copies: IoU 1 with a box and with its duplicate
        c = np.where(rng.uniform(size=n) < .8, src_c[k], rng.integers(0, n_classes + 2, n)).astype(np.int64)
        det_b.append(b); det_c.append(c)
        det_s.append((rng.integers(1, 50, n) / np.float32(50)).astype(np.float32))
    out = (det_b, det_c, det_s, gt_b, gt_c, gt_d)
    _sets[(n_classes, n_img, seed)] = out
    return out


def ref_match(n_classes, thresholds, difficult=True, n_img=600):
    key = (n_classes, thresholds, difficult, n_img)
    if key not in _refs:
        det_b, det_c, det_s, gt_b, gt_c, gt_d = make_set(n_classes, n_img)
        _refs[key] = R.match(det_b, det_c, det_s, gt_b, gt_c, gt_d if difficult else None, n_classes, thresholds)
    return _refs[key]


def _t(parts, dtype=None):
    return [torch.from_numpy(np.ascontiguousarray(p)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(p)).to(DEV, dtype)
            for p in parts]


def check_against_ref(res, m, interpolation):
    tp, ign = res["tp"].cpu().numpy(), res["ignored"].cpu().numpy()
    assert res["tp"].dtype == torch.uint16 and res["ignored"].dtype == torch.uint16 and res["tp"].is_cuda
    assert np.array_equal(tp, m["tp"]) and np.array_equal(ign, m["ignored"])
    assert res["n_gt"].dtype == np.int64 and np.array_equal(res["n_gt"], m["n_gt"])
    assert res["n_det"].dtype == np.int64 and np.array_equal(res["n_det"], m["n_det"])
    ap_ref = R.average_precisions(m, interpolation)
    ap = res["ap"]
    assert ap.dtype == np.float64 and ap.shape == ap_ref.shape
    assert np.array_equal(np.isnan(ap), np.isnan(ap_ref))
    if interpolation == "all":
        worst = 0.0
        for t in range(ap.shape[0]):
            for c in range(ap.shape[1]):
                n_tp = int((((m["tp"] >> t) & 1).astype(bool) & (m["classes"] == c)).sum())
                assert n_tp < 4096
                if not np.isnan(ap_ref[t, c]):
                    worst = max(worst, abs(ap[t, c] - ap_ref[t, c]) / (max(n_tp, 1) * 2.0 ** -52))
                    assert abs(ap[t, c] - ap_ref[t, c]) <= n_tp * 2.0 ** -52, (t, c, ap[t, c], ap_ref[t, c])
        print(f"all-point AP: largest |diff| / (n_tp * 2**-52) = {worst:.3f}")
    else:
        assert np.array_equal(ap, ap_ref, equal_nan=True)
    with np.errstate(all="ignore"):
        mean_ref = np.asarray([np.nanmean(ap[t]) for t in range(ap.shape[0])])
    assert np.array_equal(res["mean_ap"], mean_ref, equal_nan=True)
    assert res["mean_ap_over_thresholds"] == np.mean(mean_ref)


@pytest.mark.parametrize("thresholds", [(0.5,), (0.5, 0.75), SWEEP], ids=["t50", "t50_75", "sweep"])
@pytest.mark.parametrize("n_classes", [20, 80])
def test_random_sets_vs_restatement(n_classes, thresholds):
    from objectdetection_ssd_amd import Util
    det_b, det_c, det_s, gt_b, gt_c, gt_d = make_set(n_classes)
    m = ref_match(n_classes, thresholds)
    assert m["n_gt"][3] == 0 and m["n_gt"][7] == 0 and m["ignored"].any() and m["tp"].any()
    for interpolation in ("11point", "101point", "all"):
        res = Util.evaluate_detections(_t(det_b), _t(det_c), _t(det_s), _t(gt_b), _t(gt_c), _t(gt_d), n_classes=n_classes,
                                       iou_thresholds=thresholds, interpolation=interpolation)
        assert res["iou_thresholds"] == thresholds and res["interpolation"] == interpolation
        check_against_ref(res, m, interpolation)
        assert np.isnan(res["ap"][:, 3]).all() and np.isnan(res["ap"][:, 7]).all()
        assert 0.02 < res["mean_ap"][0] < 0.98


def test_hand_example_on_the_device():
    from objectdetection_ssd_amd import Util
    gt = [np.asarray([[0, 0, 10, 10], [20, 20, 30, 30], [40, 40, 50, 50]], np.float32)]
    det = [np.asarray([[0, 0, 10, 9], [40, 40, 50, 50], [20, 20, 30, 29]], np.float32)]
    cls, sc = [np.zeros(3, np.int64)], [np.asarray([.9, .8, .7], np.float32)]
    for interpolation, want in (("all", 0.8333333333333333), ("11point", 0.8484848484848484), ("101point", 0.8349834983498351)):
        res = Util.evaluate_detections(_t(det), _t(cls), _t(sc), [torch.from_numpy(gt[0][:2])], [torch.zeros(2)],
                                       n_classes=1, interpolation=interpolation)
        assert res["tp"].cpu().tolist() == [1, 0, 1] and res["ap"][0, 0] == want
        res = Util.evaluate_detections(_t(det), _t(cls), _t(sc), _t(gt), [torch.zeros(3)], [torch.tensor([0, 0, 1])],
                                       n_classes=1, interpolation=interpolation)
        assert res["tp"].cpu().tolist() == [1, 0, 1] and res["ignored"].cpu().tolist() == [0, 1, 0] and res["ap"][0, 0] == 1.0
        assert res["n_gt"].tolist() == [2] and res["n_det"].tolist() == [3]


def test_nan_iou_makes_a_false_positive_at_every_threshold():
    """Rule 2's NaN branch.  Image 0: a zero-area object and a zero-area detection of the same class elsewhere in the image (IoU =
    0/0 = NaN) next to an ordinary object that detection misses anyway: false positive at every threshold, while the ordinary
    detection of the class (no zero area on its side, so no NaN) keeps its match.  Image 1: an object with a NaN coordinate makes
    every detection of its class a false positive, even the one that sits exactly on the class's other object; the detection of
    another class is untouched."""
    from objectdetection_ssd_amd import Util
    nan = np.float32("nan")
    gt_b = [np.asarray([[.5, .5, .5, .5], [.1, .1, .4, .4]], np.float32), np.asarray([[.1, .1, nan, .4], [.5, .5, .9, .9], [.1, .1, .4, .4]], np.float32)]
    gt_c = [np.asarray([0, 0]), np.asarray([1, 1, 2])]
    det_b = [np.asarray([[.8, .8, .8, .8], [.1, .1, .4, .41]], np.float32), np.asarray([[.5, .5, .9, .9], [.1, .1, .4, .4]], np.float32)]
    det_c = [np.asarray([0, 0]), np.asarray([1, 2])]
    det_s = [np.asarray([.9, .8], np.float32), np.asarray([.9, .8], np.float32)]
    m = R.match(det_b, det_c, det_s, gt_b, gt_c, None, 3, SWEEP)
    assert m["tp"].tolist() == [0, 0x3FF, 0, 0x3FF]                         # the restatement's own reading of the case
    res = Util.evaluate_detections(_t(det_b), _t(det_c), _t(det_s), _t(gt_b), _t(gt_c), n_classes=3, iou_thresholds=SWEEP)
    assert res["tp"].cpu().tolist() == m["tp"].tolist() and not res["ignored"].cpu().numpy().any()
    check_against_ref(res, m, "11point")


def _flat_dev(parts, dtype):
    start = torch.tensor(np.cumsum([0] + [len(p) for p in parts]), dtype=torch.int32, device=DEV)
    return torch.from_numpy(np.concatenate(parts)).to(DEV, dtype).contiguous(), start


def _map_eval_tp(det_b, det_c, det_s, gt_b, gt_c, n_classes):
    from objectdetection_ssd_amd import ops
    db, dstart = _flat_dev(det_b, torch.float32)
    dc, _ = _flat_dev(det_c, torch.int32)
    ds, _ = _flat_dev(det_s, torch.float32)
    gb, gstart = _flat_dev(gt_b, torch.float32)
    gc, _ = _flat_dev(gt_c, torch.int32)
    _, tp, counts = ops.map_eval(db, dc, ds, dstart, gb, gc, gstart, O.ap_recall_thresholds(), n_classes)
    return tp, counts


@pytest.mark.parametrize("ci", range(4))
def test_bit0_equals_map_eval_on_the_golden_cases(gold_dir, ci):
    from objectdetection_ssd_amd import Util
    z = np.load(os.path.join(gold_dir, "map.npz"))
    (det_b, det_c, det_s, gt_b, gt_c), _ = _map_case(z, ci)
    tp_old, counts = _map_eval_tp(det_b, det_c, det_s, gt_b, gt_c, 20)
    res = Util.evaluate_detections(_t(det_b), _t(det_c), _t(det_s), _t(gt_b), _t(gt_c))
    assert torch.equal(res["tp"].view(torch.int16).to(torch.uint8), tp_old)
    assert res["n_gt"].tolist() == counts[1].tolist() and res["n_det"].tolist() == counts[0].tolist()


def test_bit0_equals_map_eval_on_the_large_set():
    from objectdetection_ssd_amd import Util
    det_b, det_c, det_s, gt_b, gt_c, _ = make_set(20)
    tp_old, counts = _map_eval_tp(det_b, det_c, det_s, gt_b, gt_c, 20)
    res = Util.evaluate_detections(_t(det_b), _t(det_c), _t(det_s), _t(gt_b), _t(gt_c))
    assert int(tp_old.sum()) > 1000
    assert torch.equal(res["tp"].view(torch.int16).to(torch.uint8), tp_old)
    assert res["n_gt"].tolist() == counts[1].tolist() and res["n_det"].tolist() == counts[0].tolist()


def _map_eval_vs_oracle(det_b, det_c, det_s, gt_b, gt_c, n_classes):
    """ops.map_eval on per-image lists: TP flags, table and both count rows bit for bit against the CPU oracle (whose table has 20
    rows: the classes past n_classes must be empty) and numpy.  -> (tp, table) of the oracle."""
    from objectdetection_ssd_amd import ops
    _, tp_ref, table_ref = O.get_map(det_b, det_c, det_s, gt_b, gt_c, return_details=True)
    db, dstart = _flat_dev([np.asarray(b, np.float32).reshape(-1, 4) for b in det_b], torch.float32)
    dc, _ = _flat_dev(det_c, torch.int32)
    ds, _ = _flat_dev(det_s, torch.float32)
    gb, gstart = _flat_dev([np.asarray(b, np.float32).reshape(-1, 4) for b in gt_b], torch.float32)
    gc, _ = _flat_dev(gt_c, torch.int32)
    table, tp, counts = ops.map_eval(db, dc, ds, dstart, gb, gc, gstart, O.ap_recall_thresholds(), n_classes)
    assert tp.dtype == torch.uint8 and np.array_equal(tp.cpu().numpy(), tp_ref)
    assert not table_ref[n_classes:].any() and np.array_equal(table.cpu().numpy(), table_ref[:n_classes])
    dcat, gcat = np.concatenate(det_c), np.concatenate(gt_c)
    assert counts[0].tolist() == [int((dcat == c).sum()) for c in range(n_classes)]
    assert counts[1].tolist() == [int((gcat == c).sum()) for c in range(n_classes)]
    return tp_ref, table_ref


def test_map_eval_on_both_sides_of_the_register_path_limits_vs_oracle():
    """get_map's core shares the evaluator's matching kernel: the images on either side of the register path's limits, without the
    difficult flags, against the oracle."""
    det_b, det_c, det_s, gt_b, gt_c, _ = _images_around_the_register_path_limits()
    tp_ref, table_ref = _map_eval_vs_oracle(det_b, det_c, det_s, gt_b, gt_c, 20)
    assert tp_ref.size == 1429 and int(tp_ref.sum()) == 297 and 0 < tp_ref.sum() < tp_ref.size
    assert int(table_ref.any(axis=1).sum()) == 3
    assert np.array_equal(tp_ref, R.match(det_b, det_c, det_s, gt_b, gt_c, None, 20, (0.5,))["tp"] & 1)


def test_map_eval_nan_iou_makes_a_false_positive():
    """The case of test_nan_iou_makes_a_false_positive_at_every_threshold through get_map's core."""
    nan = np.float32("nan")
    gt_b = [np.asarray([[.5, .5, .5, .5], [.1, .1, .4, .4]], np.float32), np.asarray([[.1, .1, nan, .4], [.5, .5, .9, .9], [.1, .1, .4, .4]], np.float32)]
    gt_c = [np.asarray([0, 0]), np.asarray([1, 1, 2])]
    det_b = [np.asarray([[.8, .8, .8, .8], [.1, .1, .4, .41]], np.float32), np.asarray([[.5, .5, .9, .9], [.1, .1, .4, .4]], np.float32)]
    det_c = [np.asarray([0, 0]), np.asarray([1, 2])]
    det_s = [np.asarray([.9, .8], np.float32), np.asarray([.9, .8], np.float32)]
    tp_ref, _ = _map_eval_vs_oracle(det_b, det_c, det_s, gt_b, gt_c, 3)
    assert tp_ref.tolist() == [0, 1, 0, 1]


@pytest.mark.parametrize("side", ["no_detections", "no_ground_truth"])
def test_map_eval_with_an_empty_side(side):
    """D = 0 with three objects, one of a class out of range; G = 0 with three detections: no true positive, a table of zeros."""
    box = np.asarray([[.1, .1, .4, .4], [.5, .5, .9, .9], [.2, .2, .6, .7]], np.float32)
    none_b, none_c, none_s = np.zeros((0, 4), np.float32), np.zeros(0, np.int64), np.zeros(0, np.float32)
    if side == "no_detections":
        args = ([none_b, none_b], [none_c, none_c], [none_s, none_s], [box[:2], box[2:]], [np.asarray([1, 25]), np.asarray([1])])
    else:
        args = ([box[:2], box[2:]], [np.asarray([1, 4]), np.asarray([1])], [np.asarray([.9, .8], np.float32), np.asarray([.7], np.float32)],
                [none_b, none_b], [none_c, none_c])
    tp_ref, table_ref = _map_eval_vs_oracle(*args, 20)
    assert not tp_ref.any() and not table_ref.any()


def _padded(det_b, det_c, det_s, gt_b, K=200):
    """(B,K,4), (B,K) int64, (B,K), count from the lists; rows past the count hold a ground-truth-sized box of a valid class with
    score 1.0, so that a kernel that reads them changes the result."""
    B = len(det_b)
    boxes = np.tile(np.asarray([.1, .1, .5, .5], np.float32), (B, K, 1))
    classes = np.full((B, K), 1, np.int64)
    scores = np.ones((B, K), np.float32)
    count = np.zeros(B, np.int32)
    for i in range(B):
        n = len(det_b[i])
        if len(gt_b[i]):
            boxes[i, n:] = gt_b[i][0]
        boxes[i, :n], classes[i, :n], scores[i, :n], count[i] = det_b[i], det_c[i], det_s[i], n
    return [torch.from_numpy(a).to(DEV) for a in (boxes, classes, scores, count)]


@pytest.mark.parametrize("interpolation", ["101point", "all"])
def test_batch_split_and_input_layout_do_not_change_a_bit(interpolation):
    from objectdetection_ssd_amd import Util
    n_img = 150
    det_b, det_c, det_s, gt_b, gt_c, gt_d = make_set(20, n_img)
    lists = [_t(a) for a in (det_b, det_c, det_s, gt_b, gt_c, gt_d)]
    results = []
    for step in (n_img, 32, 1):
        ev = Util.DetectionEvaluator(20, SWEEP, interpolation)
        for s in range(0, n_img, step):
            db, dc, ds, gb, gc, gd = [a[s:s + step] for a in lists]
            ev.add_batch(db, dc, ds, None, gb, gc, gd)
        results.append(ev.compute())
    for step in (n_img, 32):                                               # padded tensors, lists of ground truth
        ev = Util.DetectionEvaluator(20, SWEEP, interpolation)
        for s in range(0, n_img, step):
            pb, pc, ps, cnt = _padded(det_b[s:s + step], det_c[s:s + step], det_s[s:s + step], gt_b[s:s + step])
            ev.add_batch(pb, pc, ps, cnt, lists[3][s:s + step], lists[4][s:s + step], lists[5][s:s + step])
        results.append(ev.compute())
    check_against_ref(results[0], ref_match(20, SWEEP, True, n_img), interpolation)
    for r in results[1:]:
        assert torch.equal(r["tp"].view(torch.int16), results[0]["tp"].view(torch.int16))
        assert torch.equal(r["ignored"].view(torch.int16), results[0]["ignored"].view(torch.int16))
        assert r["ap"].tobytes() == results[0]["ap"].tobytes()
        assert np.array_equal(r["n_gt"], results[0]["n_gt"]) and np.array_equal(r["n_det"], results[0]["n_det"])


def _images_around_the_register_path_limits():
    """Seven images on either side of both limits of the matching kernel's register path (256 detections, 64 objects)."""
    rng = np.random.default_rng(77)
    shapes = [(300, 70), (300, 5), (50, 70), (256, 64), (257, 64), (256, 65), (10, 3)]
    gt_b, gt_c, gt_d, det_b, det_c, det_s = [], [], [], [], [], []
    for n, g in shapes:
        xy = rng.uniform(0, .7, (g, 2)); wh = rng.uniform(.1, .3, (g, 2))
        b = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        b[g // 2] = b[0]                                                   # a duplicate: IoU ties
        c = rng.integers(0, 3, g).astype(np.int64)
        c[g // 2] = c[0]
        gt_b.append(b); gt_c.append(c); gt_d.append((rng.uniform(size=g) < .2).astype(np.uint8))
        k = rng.integers(0, g, n)
        det_b.append((b[k] + rng.normal(0, .015, (n, 4))).astype(np.float32))
        det_c.append(np.where(rng.uniform(size=n) < .9, c[k], rng.integers(0, 4, n)).astype(np.int64))
        det_s.append((rng.integers(1, 20, n) / np.float32(20)).astype(np.float32))
    return det_b, det_c, det_s, gt_b, gt_c, gt_d


def test_images_too_long_for_the_register_path():
    """The matching kernel keeps an image of at most 256 detections and 64 objects in registers and walks longer ones in memory:
    images on either side of both limits, as lists and as padded tensors, against the restatement."""
    from objectdetection_ssd_amd import Util
    det_b, det_c, det_s, gt_b, gt_c, gt_d = _images_around_the_register_path_limits()
    m = R.match(det_b, det_c, det_s, gt_b, gt_c, gt_d, 3, SWEEP)
    assert m["tp"].any() and m["ignored"].any()
    res = Util.evaluate_detections(_t(det_b), _t(det_c), _t(det_s), _t(gt_b), _t(gt_c), _t(gt_d), n_classes=3, iou_thresholds=SWEEP,
                                   interpolation="101point")
    check_against_ref(res, m, "101point")
    ev = Util.DetectionEvaluator(3, SWEEP, "101point")
    pb, pc, ps, cnt = _padded(det_b, det_c, det_s, gt_b, K=300)
    ev.add_batch(pb, pc, ps, cnt, _t(gt_b), _t(gt_c), _t(gt_d))
    check_against_ref(ev.compute(), m, "101point")


def test_matching_is_launched_once_per_batch_whatever_the_number_of_thresholds():
    from objectdetection_ssd_amd import Util, ops
    det_b, det_c, det_s, gt_b, gt_c, gt_d = make_set(20, 150)
    lists = [_t(a) for a in (det_b, det_c, det_s, gt_b, gt_c, gt_d)]
    for thresholds in ((0.5,), SWEEP):
        before = dict(ops.launch_counts)
        ev = Util.DetectionEvaluator(20, thresholds, "all")
        for s in range(0, 150, 50):
            ev.add_batch(*[a[s:s + 50] for a in lists[:3]], None, *[a[s:s + 50] for a in lists[3:]])
        ev.compute()
        assert ops.launch_counts["eval_match"] - before["eval_match"] == 3
        assert ops.launch_counts["eval_ap"] - before["eval_ap"] == 1


def test_reset_and_repeated_compute():
    from objectdetection_ssd_amd import Util
    det_b, det_c, det_s, gt_b, gt_c, gt_d = make_set(20, 150)
    lists = [_t(a) for a in (det_b, det_c, det_s, gt_b, gt_c, gt_d)]
    ev = Util.DetectionEvaluator(20, (0.5, 0.75), "all")
    with pytest.raises(RuntimeError, match="no batch"):
        ev.compute()
    ev.add_batch(*[a[:40] for a in lists[:3]], None, *[a[:40] for a in lists[3:]])      # something to forget
    ev.reset()
    ev.add_batch(*lists[:3], None, *lists[3:])
    a, b = ev.compute(), ev.compute()
    fresh = Util.evaluate_detections(*lists, n_classes=20, iou_thresholds=(0.5, 0.75), interpolation="all")
    for r in (b, fresh):
        assert r["ap"].tobytes() == a["ap"].tobytes() and np.array_equal(r["n_gt"], a["n_gt"]) and np.array_equal(r["n_det"], a["n_det"])
        assert torch.equal(r["tp"].view(torch.int16), a["tp"].view(torch.int16))
        assert torch.equal(r["ignored"].view(torch.int16), a["ignored"].view(torch.int16))
    check_against_ref(a, ref_match(20, (0.5, 0.75), True, 150), "all")


def test_end_to_end_from_the_network_without_a_host_sync():
    """SSD_300().eval() on a seeded batch -> inference_batch_padded -> add_batch with packed device ground truth -> compute(), equal
    to the restatement fed the same detections copied to the host.  The add_batch call runs under
    torch.cuda.set_sync_debug_mode("error"): any synchronising call inside it raises."""
    from objectdetection_ssd_amd import Losses, Model, Util
    torch.manual_seed(11)
    net = Model.SSD_300().to(DEV).eval()
    B = 4
    x = torch.randn(B, 3, 300, 300, generator=torch.Generator().manual_seed(12)).to(DEV)
    with torch.no_grad():
        loc, conf = net(x)
    sizes = torch.ones(B, 2, device=DEV)                                  # decode to fractions, the ground truth's coordinates
    boxes, classes, probs, _, count = Losses.inference_batch_padded(loc, conf, sizes, top_k=200, min_score=0.02)
    cnt = count.cpu().numpy()
    assert cnt.sum() > 0
    hb, hc, hs = boxes.cpu().numpy(), classes.cpu().numpy(), probs.cpu().numpy()
    det_b = [hb[i, :cnt[i]] for i in range(B)]
    det_c = [hc[i, :cnt[i]] for i in range(B)]
    det_s = [hs[i, :cnt[i]] for i in range(B)]
    rng = np.random.default_rng(13)
    gt_b, gt_c, gt_d = [], [], []
    for i in range(B):                                                     # objects on some of the detections, so matches exist
        pick = rng.integers(0, cnt[i], min(5, cnt[i])) if cnt[i] else np.zeros(0, np.int64)
        gt_b.append(np.concatenate([det_b[i][pick], np.asarray([[.2, .2, .7, .8]], np.float32)]))
        gt_c.append(np.concatenate([det_c[i][pick], [0]]).astype(np.int64))
        gt_d.append((rng.uniform(size=len(pick) + 1) < .3).astype(np.uint8))
    gb = torch.from_numpy(np.concatenate(gt_b)).to(DEV)
    gc = torch.from_numpy(np.concatenate(gt_c)).to(DEV, torch.int32)
    gd = torch.from_numpy(np.concatenate(gt_d)).to(DEV)
    off = torch.tensor(np.cumsum([0] + [len(b) for b in gt_b]), dtype=torch.int32, device=DEV)
    ev = Util.DetectionEvaluator(20, SWEEP, "all")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev.add_batch(boxes, classes, probs, count, gb, gc, gd, gt_offsets=off)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    res = ev.compute()
    m = R.match(det_b, det_c, det_s, gt_b, gt_c, gt_d, 20, SWEEP)
    assert m["tp"].any()
    check_against_ref(res, m, "all")

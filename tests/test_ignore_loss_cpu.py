"""Ignore regions in the MultiBox loss, the parts that need no GPU: the restatement tests/ignore_loss_ref.py on hand-worked cases,
against tests/class_count_ref.py where there is no ignore box and against torch autograd; the host surface of the new entry (symbols,
refusals, ValueErrors); `Dataset.map_regions` and `keep_difficult="ignore"`; and the condition every case of
tests/test_ignore_loss_gpu.py must meet for its selection to be compared bit for bit."""
import os
import random
import types

import numpy as np
import pytest
import torch

import class_count_ref as R
import ignore_loss_cases as IC
import ignore_loss_ref as IR
import loss_regimes as LR
import ssd_oracle as O


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def _xyxy_to_cxcywh(b):
    b = np.asarray(b, np.float64)
    return np.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1).astype(np.float32)


# prior 0 is the ground-truth box (positive); against the ignore box (0.6, 0.6, 0.8, 0.8): prior 1 equals it (IoU = IoA = 1), prior 2
# overlaps it by 0.04 of its own 0.09 (IoU = IoA = 0.444), prior 3 lies inside it (IoU 0.25, IoA 1)
HAND_PRIORS = _xyxy_to_cxcywh([[0.1, 0.1, 0.3, 0.3], [0.6, 0.6, 0.8, 0.8], [0.6, 0.6, 0.9, 0.9], [0.65, 0.65, 0.75, 0.75]])
HAND_GT = [np.asarray([[0.1, 0.1, 0.3, 0.3]], np.float32)]
HAND_IGN = [np.asarray([[0.6, 0.6, 0.8, 0.8]], np.float32)]
# background = column 2; CE against it: prior 1 > prior 2 > prior 3 > 0
HAND_CONF = np.asarray([[[2., 0., 0.], [6., 0., 0.], [4., 0., 0.], [2., 0., 0.]]], np.float32)
HAND_LOC = np.asarray([[[.5, -.5, .25, 0.], [1., 1., 1., 1.], [2., 2., 2., 2.], [3., 3., 3., 3.]]], np.float32)


def _hand(ratio, ignore=HAND_IGN, **kw):
    return IR.multibox_loss(HAND_LOC, HAND_CONF, HAND_GT, [np.zeros(1, np.float32)], ignore, HAND_PRIORS, neg_pos_ratio=ratio, **kw)


def _ce64(row, c):
    row = np.asarray(row, np.float64)
    return float(np.log(np.exp(row).sum()) - row[c])


@pytest.mark.parametrize("overlap,threshold,ign,hn", [
    (None, 0.5, [], [1]),                              # no ignore box: the highest CE is mined
    ("iou", 0.5, [1], [2]),                            # it is ignored: the next one is
    ("iou", 0.4, [1, 2], [3]),
    ("iou", 0.2, [1, 2, 3], [0]),                      # all ignored: every value is 0, the lowest index fills the quota -- the positive
    ("ioa", 0.5, [1, 3], [2]),
    ("ioa", 0.4, [1, 2, 3], [0]),
    ("ioa", 1.0, [3], [1]),                            # >= : an overlap equal to the threshold ignores (prior 3 lies inside the box: its
                                                       # intersection is its area, bit for bit; prior 1's corners are rounded, just below 1)
])
def test_hand_worked_case_quota_one(overlap, threshold, ign, hn):
    kw = {} if overlap is None else dict(ignore_threshold=threshold, ignore_overlap=overlap)
    out = _hand(1, [np.zeros((0, 4), np.float32)] if overlap is None else HAND_IGN, **kw)
    assert out["pos"].tolist() == [[True, False, False, False]] and out["n_pos"] == 1
    assert np.nonzero(out["ign"][0])[0].tolist() == ign
    assert np.nonzero(out["hn"][0])[0].tolist() == hn
    sel = sorted({0} | (set(hn) - set(ign)))
    assert np.nonzero(out["sel"][0])[0].tolist() == sel
    want = _ce64(HAND_CONF[0, 0], 0) + sum(_ce64(HAND_CONF[0, p], 2) for p in sel if p != 0)
    assert abs(out["conf_loss"] - want) < 1e-12
    assert np.array_equal((out["dconf"] != 0).any(-1)[0], np.isin(np.arange(4), sel))
    assert not out["dloc"][0, 1:].any() and out["dloc"][0, 0].any()


def test_hand_worked_case_quota_over_everything():
    """quota min(4 * 1, P) = 4: every prior is in the quota, the ignored one among them -- and still without loss or gradient"""
    out = _hand(4)
    assert out["hn"].all() and out["ign"].tolist() == [[False, True, False, False]]
    assert out["sel"].tolist() == [[True, False, True, True]]
    assert not out["dconf"][0, 1].any() and not out["dloc"][0, 1].any()
    want = _ce64(HAND_CONF[0, 0], 0) + _ce64(HAND_CONF[0, 2], 2) + _ce64(HAND_CONF[0, 3], 2)
    assert abs(out["conf_loss"] - want) < 1e-12


def test_a_positive_stays_positive_inside_an_ignore_box_and_nan_ignores_nothing():
    out = _hand(1, [np.asarray([[0.1, 0.1, 0.3, 0.3], [0., 0., 1., 1.]], np.float32)], ignore_threshold=0.01)
    assert out["pos"][0, 0] and not out["ign"][0, 0] and out["ign"][0, 1:].all()
    # a zero-area prior against a zero-area box: 0 / 0 in both measures
    pri = np.asarray([[0.5, 0.5, 0.5, 0.5], [0.2, 0.2, 0.3, 0.3]], np.float32)
    box = np.asarray([[0.5, 0.5, 0.5, 0.5]], np.float32)
    for mode in ("iou", "ioa"):
        assert np.isnan(IR.overlap_matrix(box, pri, mode)[0, 0])
        assert not IR.ignored_mask([box], pri, np.zeros((1, 2), bool), 0.0, mode)[0, 0]
    with pytest.raises(ValueError):
        IR.overlap_matrix(box, pri, "giou")


def test_without_ignore_boxes_it_is_the_plain_restatement_bit_for_bit():
    case = LR.make("trained", 777, 21, 3, 3)
    plain = R.multibox_loss(case.loc, case.conf, case.boxes, case.classes, case.priors_cxcywh, case.neg_pos_ratio)
    for ignore in (None, [np.zeros((0, 4), np.float32)] * 3):
        mine = IR.multibox_loss(case.loc, case.conf, case.boxes, case.classes, ignore, case.priors_cxcywh, case.neg_pos_ratio)
        assert not mine["ign"].any()
        for k, v in plain.items():
            if isinstance(v, np.ndarray):
                assert v.dtype == mine[k].dtype and np.array_equal(v.view(np.uint8), np.ascontiguousarray(mine[k]).view(np.uint8)), k
            else:
                assert v == mine[k], k


def test_gradients_equal_autograd_of_the_loss_written_in_torch():
    """rule 3 in torch, f64: cce[pos | ignored] = 0 before the ranking, the loss over the quota's rows; its autograd gradients"""
    case, ref = IC.case_and_reference("trained-P777-C21-bs3-iou-0first")
    bs, P, C = case.conf.shape
    pos, ign, cls = torch.tensor(ref["pos"]), torch.tensor(ref["ign"]), torch.tensor(ref["cls"])
    assert ref["ign"].any()
    loc = torch.tensor(case.loc, dtype=torch.float64, requires_grad=True)
    conf = torch.tensor(case.conf, dtype=torch.float64, requires_grad=True)
    cce = torch.nn.functional.cross_entropy(conf.reshape(-1, C), cls.reshape(-1), reduction="none").view(bs, P)
    cce1 = cce.detach().float().clone()                               # the f32 values decide, as in the reference
    cce1[pos | ign] = 0.
    conf_loss = cce[pos].sum()
    for i in range(bs):
        k = min(case.neg_pos_ratio * int(pos[i].sum()), P)
        idx = torch.sort(cce1[i], descending=True, stable=True)[1][:k]
        conf_loss = conf_loss + (cce[i][idx] * (~pos[i][idx] & ~ign[i][idx])).sum()
    conf_loss = conf_loss / pos.sum()
    loc_loss = (loc[pos] - torch.tensor(ref["enc"], dtype=torch.float64)).abs().mean()
    (loc_loss + conf_loss).backward()
    # (the restatement takes loc - g in f32, as the reference does: 2^-24 relative per term)
    assert abs(float(loc_loss) - ref["loc_loss"]) <= 1e-7 * abs(ref["loc_loss"])
    assert abs(float(conf_loss) - ref["conf_loss"]) <= 1e-9 * abs(ref["conf_loss"])      # (f32-decided ranking, f64 sums on both sides)
    # (the restatement's dloc is class_count_ref's: sign / (4 n_pos) formed in f32, 2^-24 relative)
    assert np.abs(loc.grad.numpy() - ref["dloc"]).max() <= 1e-7 * np.abs(ref["dloc"]).max()
    assert np.array_equal(np.sign(loc.grad.numpy()), np.sign(ref["dloc"]))
    assert np.abs(conf.grad.numpy() - ref["dconf"]).max() <= 1e-12 * np.abs(ref["dconf"]).max()
    assert np.array_equal((conf.grad.numpy() != 0).any(-1), ref["sel"])


# ---- the cases of the GPU test -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", IC.CASE_IDS)
def test_every_gpu_case_is_boundary_safe_and_reaches_what_it_is_named_after(case_id):
    case, ref = IC.case_and_reference(case_id)
    bs, P, C = case.conf.shape
    ranked = ref["ranked"].astype(np.float32)
    ranked = np.where(ranked > 0, ranked, np.float32(0))
    for i in range(bs):
        k = min(case.neg_pos_ratio * int(ref["pos"][i].sum()), P)
        assert LR.boundary_ok(ranked[i], k), (case_id, i)
        assert int(ref["hn"][i].sum()) == k
    assert not ((ranked > 0) & (ranked < 1e-2)).any()
    assert P % 64 and P % 256 and C in (21, 81) and bs in (1, 2, 3)
    plain = R.multibox_loss(case.loc, case.conf, case.boxes, case.classes, case.priors_cxcywh, case.neg_pos_ratio)
    assert np.array_equal(plain["cls"], ref["cls"])                                  # matching takes no notice of ignore boxes
    assert (ref["ign"] & plain["hn"]).any(), "no ignored prior that the plain loss would have mined"
    assert not (ref["ign"] & ref["pos"]).any()
    counts = [len(b) for b in case.ignore]
    for i in range(bs):
        assert (counts[i] == 0) <= (not ref["ign"][i].any())
    if "0first" in case_id:
        assert counts[0] == 0 and sorted(counts) == [0, 1, 5]
    if "0last" in case_id:
        assert counts[-1] == 0 and sorted(counts) == [0, 1, 5]
    if "130boxes" in case_id:
        late = IR.ignored_mask([case.ignore[0][IC.SG:]], O.xywh_to_xyxy(case.priors_cxcywh), ref["pos"], case.threshold, case.overlap)
        early = IR.ignored_mask([case.ignore[0][:IC.SG]], O.xywh_to_xyxy(case.priors_cxcywh), ref["pos"], case.threshold, case.overlap)
        assert counts[0] > IC.SG and (late & ~early).any() and early.any(), "no prior ignored by a box past the staged ones alone"
    if "k_exceeds_nonzero" in case_id:
        assert any(min(case.neg_pos_ratio * int(ref["pos"][i].sum()), P) > int((ranked[i] > 0).sum()) for i in range(bs))
    if case_id == "k_exceeds_nonzero-P1000-C81-bs3-ioa":
        assert (ref["ign"] & ref["hn"]).any()                                        # ignored priors inside the quota
    if "equals_gt" in case_id:
        assert np.array_equal(case.ignore[0][:len(case.boxes[0])], case.boxes[0]) and ref["pos"].any()
        iou = O.iou_matrix(case.ignore[0][:len(case.boxes[0])], O.xywh_to_xyxy(case.priors_cxcywh))
        assert (ref["pos"][0] & (iou.max(0) >= 0.5)).any()                           # a positive under the ignore box, still positive
    if "cover" in case_id:
        assert np.array_equal(ref["ign"], ~ref["pos"]) and np.array_equal(ref["sel"], ref["pos"])
    if "zero_area" in case_id:
        b = case.ignore[0][0]
        assert b[0] == b[2] and b[1] == b[3]
        assert not IR.ignored_mask([case.ignore[0][:1]], O.xywh_to_xyxy(case.priors_cxcywh), ref["pos"], case.threshold, case.overlap).any()


def test_the_cases_cover_what_the_kernels_distinguish():
    specs = list(IC.SPEC.values())
    assert {s[1] for s in specs} >= {777, 1000, 8732} and {s[2] for s in specs} == {21, 81} and {s[3] for s in specs} >= {1, 3}
    assert {s[0] for s in specs} == {"trained", "tie_groups", "k_exceeds_nonzero"}
    assert {s[5] for s in specs} == {"iou", "ioa"} and {s[6] for s in specs} - {0.5}
    for C in (21, 81):                                                               # both kernel families see both measures
        assert {s[5] for s in specs if s[2] == C} == {"iou", "ioa"}
    assert set(IC.N_IGN_ZERO_IDS) <= set(IC.CASE_IDS) and {IC.SPEC[c][2] for c in IC.N_IGN_ZERO_IDS} == {21, 81}


# ---- host surface ------------------------------------------------------------------------------------------------------------------
NEW = ("ssd_multibox_loss_ignore_workspace", "ssd_multibox_loss_ignore")


def test_the_new_symbols_are_declared_bound_and_exported():
    from objectdetection_ssd_amd import _lib
    with open(os.path.join(os.path.dirname(_lib.PKG), "include", "ssd_gfx950.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name in NEW:
        assert f" {name}(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    plain, ign = _lib.SIGNATURES["ssd_multibox_loss"][1], _lib.SIGNATURES["ssd_multibox_loss_ignore"][1]
    assert len(ign) == len(plain) + 6 and ign[:14] == plain[:14] and ign[-3:] == plain[-3:]
    assert lib.ssd_abi_version() == 1
    assert lib.ssd_multibox_loss_ignore_workspace(32, 8732, 90, 64) == lib.ssd_multibox_loss_workspace(32, 8732, 90) > 0
    assert lib.ssd_multibox_loss_ignore_workspace(32, 8732, 90, 0) == lib.ssd_multibox_loss_workspace(32, 8732, 90)
    assert lib.ssd_multibox_loss_ignore_workspace(32, 8732, 90, -1) == 0 and lib.ssd_multibox_loss_ignore_workspace(0, 8732, 90, 1) == 0


OK_PTR, ODD_PTR = 0x10000, 0x10004
OK, BAD_SHAPE, WORKSPACE, NULL, ALIGN = 0, -1, -2, -3, -5
ARGS = ["loc", "conf", "gt_boxes", "gt_classes", "img_start", "bs", "n_gt", "priors_cxcywh", "priors_xyxy", "P", "n_classes",
        "iou_threshold", "neg_pos_ratio", "norm_mode", "ign_boxes", "ign_start", "n_ign", "ignore_threshold", "overlap_mode", "losses",
        "obj", "cls", "ign", "dloc", "dconf", "workspace", "workspace_bytes", "stream"]
VALID = dict(bs=2, n_gt=3, P=100, n_classes=21, iou_threshold=0.5, neg_pos_ratio=3, norm_mode=0, n_ign=4, ignore_threshold=0.5,
             overlap_mode=1, stream=None)
REFUSALS = [
    ("null:ign_start", dict(ign_start=None), NULL), ("null:ign", dict(ign=None), NULL), ("null:loc", dict(loc=None), NULL),
    ("null:workspace", dict(workspace=None), NULL), ("null:ign_boxes with boxes", dict(ign_boxes=None), NULL),
    ("one gradient only", dict(dloc=None), NULL),
    ("n_ign -1", dict(n_ign=-1), BAD_SHAPE), ("n_ign -1, no boxes", dict(n_ign=-1, ign_boxes=None), BAD_SHAPE),
    ("mode 2", dict(overlap_mode=2), BAD_SHAPE), ("mode -1", dict(overlap_mode=-1), BAD_SHAPE), ("bs 0", dict(bs=0), BAD_SHAPE),
    ("C 257", dict(n_classes=257), BAD_SHAPE), ("norm_mode 2", dict(norm_mode=2), BAD_SHAPE),
    ("odd:ign_boxes", dict(ign_boxes=ODD_PTR), ALIGN), ("odd:loc", dict(loc=ODD_PTR), ALIGN),
    ("workspace one byte short", dict(workspace_bytes=-1), WORKSPACE),
    # where several apply: null, then shape, then alignment, then workspace
    ("null + shape", dict(ign=None, overlap_mode=5), NULL), ("shape + align", dict(n_ign=-1, loc=ODD_PTR), BAD_SHAPE),
    ("shape + workspace", dict(overlap_mode=2, workspace_bytes=-1), BAD_SHAPE), ("align + workspace", dict(ign_boxes=ODD_PTR, workspace_bytes=-1), ALIGN),
]


@pytest.mark.parametrize("label,changes,want", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_new_entry_refuses_defective_arguments_with_the_stated_status(label, changes, want):
    """Every case is refused before anything is enqueued, so the made-up pointers are never dereferenced; where a GPU is present the
    test does not run (tests/test_elementwise_status_cpu.py: a tuple some change made acceptable must never reach a launch)."""
    if torch.cuda.is_available():
        pytest.skip("made-up pointers: only where no launch can succeed")
    from objectdetection_ssd_amd import _lib
    lib = _lib.load()
    v = dict(VALID)
    v["workspace_bytes"] = lib.ssd_multibox_loss_ignore_workspace(v["bs"], v["P"], v["n_gt"], v["n_ign"])
    for k, val in changes.items():
        v[k] = v["workspace_bytes"] + val if k == "workspace_bytes" else val
    args = [v[a] if a in v else OK_PTR for a in ARGS]
    assert len(args) == len(_lib.SIGNATURES["ssd_multibox_loss_ignore"][1])
    assert lib.ssd_multibox_loss_ignore(*args) == want, label


def test_value_errors_of_the_python_surface():
    from objectdetection_ssd_amd import Losses, ops
    from objectdetection_ssd_amd.ddp import GraphedTrainStep
    z = torch.zeros
    loss_args = (z(1, 8732, 4), z(1, 8732, 21), z(1, 4), z(1), z(2, dtype=torch.int32), z(8732, 4), z(8732, 4))
    with pytest.raises(ValueError):
        ops.multibox_loss(*loss_args, ignore_boxes=z(0, 4), ignore_start=z(2, dtype=torch.int32), ignore_overlap="giou")
    with pytest.raises(ValueError):
        ops.multibox_loss(*loss_args, ignore_boxes=z(0, 4))                         # boxes without their offsets
    assert ops.ignore_overlap_mode("iou") == 0 and ops.ignore_overlap_mode("ioa") == 1
    out = (z(2, 8732, 4), z(2, 8732, 21))
    cl, bx = [z(1), z(1)], [torch.tensor([[.1, .1, .5, .5]])] * 2
    with pytest.raises(ValueError):
        Losses.ssd(out, cl, bx, ignore_bboxs=[z(0, 4)] * 2, ignore_overlap="IoU")
    with pytest.raises(ValueError):
        Losses.ssd(out, cl, bx, ignore_overlap=None)                                # also without ignore boxes
    with pytest.raises(ValueError):
        Losses.ssd(out, cl, bx, ignore_bboxs=[z(0, 4)] * 3)                         # not one list per image
    with pytest.raises(RuntimeError):
        Losses.ssd(out, cl, bx, ignore_bboxs=[z(0, 4)] * 2)                         # host tensors: no CPU fallback, as without ignore boxes
    import inspect
    for fn, names in ((ops.multibox_loss, ["ignore_boxes", "ignore_start", "ignore_threshold", "ignore_overlap"]),
                      (Losses.ssd, ["ignore_bboxs", "ignore_threshold", "ignore_overlap"]),
                      (GraphedTrainStep.__init__, ["max_ignore_per_image"])):
        params = list(inspect.signature(fn).parameters.values())
        assert [p.name for p in params[-len(names):]] == names
    assert inspect.signature(ops.multibox_loss).parameters["ignore_threshold"].default == 0.5
    assert inspect.signature(GraphedTrainStep.__init__).parameters["max_ignore_per_image"].default == 0
    assert list(inspect.signature(GraphedTrainStep.__call__).parameters)[1:] == ["x", "classes", "boxes", "ignore"]
    trainer = types.SimpleNamespace(grad_dtype=torch.float32, world=1, overlap=True)
    net = types.SimpleNamespace(_engine=types.SimpleNamespace(sink_early=True))
    step = GraphedTrainStep(net, trainer)
    with pytest.raises(ValueError):
        step(z(2, 3, 300, 300), cl, bx, [z(0, 4)] * 2)                              # no capacity for ignore boxes
    with pytest.raises(ValueError):
        GraphedTrainStep(net, trainer, max_ignore_per_image=-1)


# ---- Dataset -----------------------------------------------------------------------------------------------------------------------
W, H = 200, 160
BOXES = [[20., 30., 120., 130.], [10., 10., 60., 50.], [100., 20., 190., 90.], [150., 100., 195., 155.], [90., 60., 110., 80.]]
DIFFICULT = [0, 1, 0, 1, 1]


def _files(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(3)
    paths = []
    for i in range(2):
        p = str(tmp_path / f"i{i}.jpg")
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(p, "JPEG", quality=85)
        paths.append(p)
    n = len(paths)
    return paths, [BOXES] * n, [["dog", "cat", "car", "bus", "person"]] * n, [DIFFICULT] * n, list(range(n))


def test_map_regions_is_plan_transforms_box_arithmetic():
    """Every ground-truth box that survives the drawn crop comes out of map_regions with the bits plan_transform gave it; a box that
    misses the crop window is dropped; expand, crop and flip are each reached (and each without the others)."""
    from objectdetection_ssd_amd import Dataset
    boxes = torch.tensor(BOXES)
    seen = dict(expand=0, crop=0, flip=0, dropped=0, clipped=0, plain=0)
    for seed in range(200):
        plan, new_boxes, new_labels = Dataset.plan_transform(W, H, boxes, torch.arange(len(BOXES)), rng=random.Random(seed))
        ch, cw, top, left = plan.canvas
        ct, cl, crop_h, crop_w = plan.crop
        cropped = (ct, cl, crop_h, crop_w) != (0, 0, ch, cw)
        seen["expand"] += plan.canvas != (H, W, 0, 0); seen["crop"] += cropped; seen["flip"] += plan.flip
        seen["plain"] += plan.canvas == (H, W, 0, 0) and not cropped and not plan.flip
        for j, k in enumerate(new_labels.tolist()):
            one = Dataset.map_regions(plan, boxes[k:k + 1])
            assert one.shape == (1, 4) and one.dtype == torch.float32
            assert np.array_equal(one[0].numpy().view(np.uint32), new_boxes[j].numpy().view(np.uint32)), (seed, k)
        all_of_them = Dataset.map_regions(plan, boxes)
        kept = 0
        for k, (x1, y1, x2, y2) in enumerate(BOXES):
            x1, x2, y1, y2 = x1 + left, x2 + left, y1 + top, y2 + top                # on the canvas (integers: exact)
            misses = cropped and (x2 <= cl or x1 >= cl + crop_w or y2 <= ct or y1 >= ct + crop_h)
            one = Dataset.map_regions(plan, boxes[k:k + 1])
            assert one.shape[0] == (0 if misses else 1), (seed, k)
            seen["dropped"] += misses
            if not misses:
                assert torch.equal(one[0], all_of_them[kept])                        # order kept
                kept += 1
                assert 0 <= one[0, 0] if not plan.flip else True
                if cropped:
                    assert one[0, 2] - one[0, 0] <= crop_w and one[0, 3] - one[0, 1] <= crop_h
                    seen["clipped"] += bool(k not in new_labels.tolist())            # kept by what is left of it, not by its centre
        assert all_of_them.shape[0] == kept
        if plan.flip and kept:                                                        # the reference's mirror: x -> w - x - 1, ends swapped
            unflipped = Dataset.map_regions(Dataset.GeomPlan(plan.src_h, plan.src_w, plan.canvas, plan.crop, False), boxes)
            assert torch.equal(all_of_them[:, 0], crop_w - unflipped[:, 2] - 1) and torch.equal(all_of_them[:, 2], crop_w - unflipped[:, 0] - 1)
            assert torch.equal(all_of_them[:, 1::2], unflipped[:, 1::2])
    assert all(v > 0 for v in seen.values()), seen
    # no area left, or none to begin with: dropped
    assert Dataset.map_regions(Dataset.identity_plan(H, W), torch.tensor([[5., 5., 5., 9.], [3., 4., 8., 9.]])).tolist() == [[3., 4., 8., 9.]]
    assert Dataset.map_regions(Dataset.identity_plan(H, W), torch.zeros((0, 4))).shape == (0, 4)


@pytest.mark.parametrize("decode", ["host", "device"])
def test_keep_difficult_ignore_returns_the_items_of_false_plus_the_mapped_difficult_boxes(tmp_path, decode):
    from objectdetection_ssd_amd import Dataset
    args = _files(tmp_path)
    plain = Dataset.MultiImageMultiBBoxDataset(*args, decode=decode)
    ign = Dataset.MultiImageMultiBBoxDataset(*args, keep_difficult="ignore", decode=decode)
    hard = torch.tensor(BOXES)[torch.tensor(DIFFICULT) == 1]
    some_dropped = some_kept = 0
    for test_mode in (True, False):
        plain.isTest = ign.isTest = test_mode
        for seed in range(30):
            i = seed % len(plain)
            random.seed(500 + seed)
            a = plain[i]
            state_a = random.getstate()
            random.seed(500 + seed)
            b = ign[i]
            assert random.getstate() == state_a                                      # ignore boxes take part in no draw
            assert len(a) == 4 and len(b) == 5
            assert type(b[0]) is (Dataset.EncodedImage if decode == "device" else Dataset.RawImage) and type(a[0]) is type(b[0])
            assert a[0].plan == b[0].plan and a[0].size == b[0].size
            assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3]
            w, h = b[0].size
            want = Dataset.map_regions(b[0].plan, hard) / torch.FloatTensor([w, h, w, h]).unsqueeze(0)
            assert b[4].dtype == torch.float32 and torch.equal(b[4], want)
            if test_mode:
                assert torch.equal(b[4], hard / torch.FloatTensor([W, H, W, H]).unsqueeze(0))
            else:
                some_dropped += b[4].shape[0] < hard.shape[0]
                some_kept += b[4].shape[0] > 0
    assert some_dropped and some_kept
    for kd in (False, True):                                                          # the reference's 4-tuple, unchanged
        ds = Dataset.MultiImageMultiBBoxDataset(*args, isTest=True, keep_difficult=kd, decode=decode)
        item = ds[0]
        assert len(item) == 4 and item[1].numel() == (5 if kd else 2)


def test_collate_passes_the_fifth_list_through(tmp_path):
    from objectdetection_ssd_amd import Dataset
    args = _files(tmp_path)
    ign = Dataset.MultiImageMultiBBoxDataset(*args, isTest=True, keep_difficult="ignore")
    out = Dataset.collate_fn([ign[0], ign[1]])
    assert len(out) == 5 and isinstance(out[0], Dataset.RawBatch) and out[3] == [0, 1]
    assert all(isinstance(v, list) and len(v) == 2 for v in out[1:])
    assert torch.equal(out[4][0], ign[0][4]) and out[4][0].shape == (3, 4)
    plain = Dataset.MultiImageMultiBBoxDataset(*args, isTest=True)
    assert len(Dataset.collate_fn([plain[0], plain[1]])) == 4

"""ssd_multibox_loss_ignore (csrc/loss.hip) against tests/ignore_loss_ref.py on the cases of tests/ignore_loss_cases.py: the ignored
mask, the matching and the rows with a gradient bit for bit, losses and gradients to the bars of tests/test_loss_regimes_gpu.py (the
same kernels), in both norm modes; the entry with no ignore box equals ssd_multibox_loss in every bit, and leaves it as it was."""
import numpy as np
import pytest
import torch

import ignore_loss_cases as IC
import ssd_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_device_args = {}


def _starts(lists):
    return np.concatenate([[0], np.cumsum([len(b) for b in lists])]).astype(np.int32)


def _args(case_id):
    """the case on the device, uploaded once: (loc, conf, gt_boxes, gt_classes, img_start, priors_cxcywh, priors_xyxy), (ign_boxes, ign_start)"""
    if case_id not in _device_args:
        case, _ = IC.case_and_reference(case_id)
        host = (case.loc, case.conf, np.concatenate(case.boxes), np.concatenate(case.classes), _starts(case.boxes), case.priors_cxcywh,
                O.xywh_to_xyxy(case.priors_cxcywh))
        ign = (np.concatenate(case.ignore).astype(np.float32).reshape(-1, 4), _starts(case.ignore))
        _device_args[case_id] = tuple(torch.tensor(a).to(DEV) for a in host), tuple(torch.tensor(a).to(DEV) for a in ign)
    return _device_args[case_id]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _host(o):
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}


def _check_against_reference(case_id, norm_mode, loc_loss, conf_loss, n_pos, obj, cls, ign, dloc, dconf):
    case, ref = IC.case_and_reference(case_id)
    pos, hn = ref["pos"], ref["hn"]
    assert np.array_equal(ign.astype(bool), ref["ign"]) and set(np.unique(ign)) <= {0, 1}
    assert np.array_equal(cls, ref["cls"])
    assert np.array_equal(obj[pos], ref["obj"][pos])
    assert np.array_equal((dconf != 0).any(-1), pos | (hn & ~ref["ign"]))      # the rows with a gradient, bit-exact
    assert not dconf[ref["ign"]].any() and not dloc[ref["ign"]].any()            # an ignored prior: both rows exactly zero
    assert n_pos == ref["n_pos"]
    scale = 1.0 if norm_mode == 0 else float(ref["n_pos"])                     # norm_mode 1 leaves the division by n_pos to the caller
    want_loc, want_conf = ref["loc_loss"] * scale, ref["conf_loss"] * scale
    print(f"{case_id} norm_mode {norm_mode}: loc_loss {loc_loss:.8g} (ref {want_loc:.8g}) conf_loss {conf_loss:.8g} (ref {want_conf:.8g}) "
          f"ignored {ref['ign'].sum(1)} of them in the quota {(ref['ign'] & hn).sum(1)}")
    assert abs(loc_loss - want_loc) <= 1e-4 * max(1.0, abs(want_loc))
    assert abs(conf_loss - want_conf) <= 1e-4 * max(1.0, abs(want_conf))
    factor = np.float32(0.25) * (np.float32(1) / np.float32(ref["n_pos"]) if norm_mode == 0 else np.float32(1))
    assert np.array_equal(_bits(dloc), _bits(np.sign(ref["dloc"]).astype(np.float32) * factor))
    want = ref["dconf"] * scale
    err = np.abs(dconf - want).max()
    print(f"  dconf: max |err| {err:.3e} of max |ref| {np.abs(want).max():.3e}")
    assert err <= 1e-5 * np.abs(want).max()


def _run(case_id, norm_mode, want_grads=True, ignore=True, empty=False):
    from objectdetection_ssd_amd import ops
    case, _ = IC.case_and_reference(case_id)
    args, (ib, ist) = _args(case_id)
    kw = {}
    if ignore:
        if empty:
            ib, ist = torch.zeros((0, 4), device=DEV), torch.zeros_like(ist)
        kw = dict(ignore_boxes=ib, ignore_start=ist, ignore_threshold=case.threshold, ignore_overlap=case.overlap)
    return _host(ops.multibox_loss(*args, iou_threshold=0.5, neg_pos_ratio=case.neg_pos_ratio, norm_mode=norm_mode, want_grads=want_grads,
                                   **kw))


@pytest.mark.parametrize("norm_mode", [0, 1])
@pytest.mark.parametrize("case_id", IC.CASE_IDS)
def test_ignore_loss_equals_the_restatement(case_id, norm_mode):
    before = _run(case_id, norm_mode, ignore=False)                            # the existing entry, before and after the new one
    a = _run(case_id, norm_mode)
    b = _run(case_id, norm_mode)
    fwd = _run(case_id, norm_mode, want_grads=False)
    after = _run(case_id, norm_mode, ignore=False)
    _check_against_reference(case_id, norm_mode, float(a["losses"][0]), float(a["losses"][1]), int(a["losses"][2]), a["obj"], a["cls"],
                             a["ign"], a["dloc"], a["dconf"])
    for k in ("losses", "dloc", "dconf"):                                       # two launches, the same bits
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(a["obj"], b["obj"]) and np.array_equal(a["cls"], b["cls"]) and np.array_equal(a["ign"], b["ign"])
    assert fwd["dloc"] is None and fwd["dconf"] is None                         # forward only: the same losses and masks
    assert np.array_equal(_bits(fwd["losses"]), _bits(a["losses"]))
    assert np.array_equal(fwd["cls"], a["cls"]) and np.array_equal(fwd["ign"], a["ign"])
    assert "ign" not in before and set(before) == set(after)
    for k in ("losses", "dloc", "dconf"):
        assert np.array_equal(_bits(before[k]), _bits(after[k])), k
    assert np.array_equal(before["obj"], after["obj"]) and np.array_equal(before["cls"], after["cls"])


@pytest.mark.parametrize("case_id", [c for c in IC.CASE_IDS if "cover" in c])
def test_a_box_over_everything_leaves_the_positives_alone(case_id):
    """"ioa" with a box that contains every prior: every non-positive is ignored, the rows with a gradient are the positives, the conf
    loss is their cross entropy."""
    _, ref = IC.case_and_reference(case_id)
    o = _run(case_id, 1)
    pos = ref["pos"]
    assert np.array_equal(o["ign"].astype(bool), ~pos)
    assert np.array_equal((o["dconf"] != 0).any(-1), pos)
    want = -np.take_along_axis(torch.log_softmax(torch.tensor(IC.case_and_reference(case_id)[0].conf).double(), -1).numpy(),
                               ref["cls"][..., None], axis=2)[..., 0][pos].sum()
    assert abs(float(o["losses"][1]) - want) <= 1e-4 * max(1.0, abs(want))


def test_an_ignore_box_equal_to_a_ground_truth_box_keeps_its_positives():
    case_id = "tie_groups-P1000-C21-bs1-iou-equals_gt"
    case, ref = IC.case_and_reference(case_id)
    assert np.array_equal(case.ignore[0][:len(case.boxes[0])], case.boxes[0])
    o = _run(case_id, 0)
    plain = _run(case_id, 0, ignore=False)
    assert np.array_equal(o["cls"], plain["cls"]) and np.array_equal(o["obj"], plain["obj"])      # matching unchanged
    assert ref["pos"].any() and not o["ign"][ref["pos"]].any()
    assert np.array_equal(_bits(o["dloc"]), _bits(plain["dloc"]))                                  # the loc side too


@pytest.mark.parametrize("norm_mode", [0, 1])
@pytest.mark.parametrize("case_id", IC.N_IGN_ZERO_IDS)
def test_no_ignore_box_equals_the_plain_entry_bit_for_bit(case_id, norm_mode):
    plain = _run(case_id, norm_mode, ignore=False)
    zero = _run(case_id, norm_mode, empty=True)
    assert not zero["ign"].any()
    for k in ("losses", "dloc", "dconf"):
        assert np.array_equal(_bits(plain[k]), _bits(zero[k])), k
    assert np.array_equal(plain["obj"], zero["obj"]) and np.array_equal(plain["cls"], zero["cls"])
    fwd = _run(case_id, norm_mode, want_grads=False, empty=True)
    assert np.array_equal(_bits(fwd["losses"]), _bits(plain["losses"]))


@pytest.mark.parametrize("norm_mode", [0, 1])
def test_ignore_regions_through_the_public_loss(norm_mode):
    """Losses.ssd(..., ignore_bboxs=...) + backward(): the gradients of the ops call, last_match["ignored"] set."""
    from objectdetection_ssd_amd import Losses
    case_id = "trained-P8732-C21-bs2-iou-ssd_priors"
    case, ref = IC.case_and_reference(case_id)
    assert case.neg_pos_ratio == Losses.NEG_POS_RATIO
    (loc, conf, *_), _ = _args(case_id)
    lt, ct = loc.clone().requires_grad_(True), conf.clone().requires_grad_(True)
    l1, l2, n_pos = Losses.ssd((lt, ct), [torch.tensor(c).to(DEV) for c in case.classes], [torch.tensor(b).to(DEV) for b in case.boxes],
                               norm_mode=norm_mode, with_n_pos=True, ignore_bboxs=[torch.tensor(b) for b in case.ignore],
                               ignore_threshold=case.threshold, ignore_overlap=case.overlap)
    (l1 + l2).backward()
    torch.cuda.synchronize()
    m = Losses.last_match
    assert np.array_equal(m["ignored"].cpu().numpy().astype(bool), ref["ign"]) and ref["ign"].any()
    o = _run(case_id, norm_mode)
    assert np.array_equal(_bits(lt.grad.cpu().numpy()), _bits(o["dloc"])) and np.array_equal(_bits(ct.grad.cpu().numpy()), _bits(o["dconf"]))
    assert np.array_equal(_bits(np.asarray([l1.item(), l2.item(), n_pos.item()])), _bits(o["losses"]))
    Losses.ssd((loc, conf), [torch.tensor(c).to(DEV) for c in case.classes], [torch.tensor(b).to(DEV) for b in case.boxes])
    assert "ignored" not in Losses.last_match                                   # a call without ignore boxes: the plain entry

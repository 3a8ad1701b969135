"""csrc/loss.hip against tests/class_count_ref.py::multibox_loss in the regimes of tests/loss_regimes.py (saturated background rows
with CE exactly 0, quotas past the non-zero values / the negatives / P, tie groups across ranking slices and waves, one / four histogram
bins, logits up to 1e4, more than 128 boxes in an image): matching, the selected set and n_pos bit-exact, losses and gradients to the
project's bars, in both loss forms and both norm modes.  tests/test_loss_regimes_cpu.py shows, on the reference alone, that the cases
allow a bit-exact comparison of the selection and that each regime reaches what it is named after."""
import numpy as np
import pytest
import torch

import loss_regimes as LR
import ssd_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_device_args = {}


def _args(case_id):
    """the case on the device, uploaded once: loc, conf, gt_boxes, gt_classes, img_start, priors_cxcywh, priors_xyxy"""
    if case_id not in _device_args:
        case, _ = LR.case_and_reference(case_id)
        start = np.concatenate([[0], np.cumsum([len(b) for b in case.boxes])]).astype(np.int32)
        host = (case.loc, case.conf, np.concatenate(case.boxes), np.concatenate(case.classes), start, case.priors_cxcywh,
                O.xywh_to_xyxy(case.priors_cxcywh))
        _device_args[case_id] = tuple(torch.tensor(a).to(DEV) for a in host)
    return _device_args[case_id]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_against_reference(case_id, norm_mode, loc_loss, conf_loss, n_pos, obj, cls, dloc, dconf):
    case, ref = LR.case_and_reference(case_id)
    pos, hn = ref["pos"], ref["hn"]
    assert np.array_equal(cls, ref["cls"])
    assert np.array_equal(obj[pos], ref["obj"][pos])
    assert np.array_equal((dconf != 0).any(-1), pos | hn)                      # the selected set, bit-exact (positives included)
    assert n_pos == ref["n_pos"]
    scale = 1.0 if norm_mode == 0 else float(ref["n_pos"])                     # norm_mode 1 leaves the division by n_pos to the caller
    want_loc, want_conf = ref["loc_loss"] * scale, ref["conf_loss"] * scale
    print(f"{case_id} norm_mode {norm_mode}: loc_loss {loc_loss:.8g} (ref {want_loc:.8g}) conf_loss {conf_loss:.8g} (ref {want_conf:.8g})")
    assert abs(loc_loss - want_loc) <= 1e-4 * max(1.0, abs(want_loc))
    assert abs(conf_loss - want_conf) <= 1e-4 * max(1.0, abs(want_conf))
    # dloc is a sign pattern times one f32 factor: (1 / n_pos) * 0.25, or 0.25 in norm_mode 1
    factor = np.float32(0.25) * (np.float32(1) / np.float32(ref["n_pos"]) if norm_mode == 0 else np.float32(1))
    assert np.array_equal(_bits(dloc), _bits(np.sign(ref["dloc"]).astype(np.float32) * factor))
    want = ref["dconf"] * scale
    err = np.abs(dconf - want).max()
    print(f"  dconf: max |err| {err:.3e} of max |ref| {np.abs(want).max():.3e}")
    assert err <= 1e-5 * np.abs(want).max()
    # The bar above cannot see the e^-40-sized entries of selected saturated rows: those elementwise.  torch's f32 CPU softmax deviates
    # from the f64 reference by at most 1.985e-6 (relative) on these entries over all cases (LR.SOFTMAX_F32_DEV = 2.0e-6, held by the CPU
    # test); the device's expf is another implementation: 4 x that.
    m = LR.small_entries(case, ref)
    if m.any():
        rel = (np.abs(dconf - want)[m] / np.abs(want)[m]).max()
        print(f"  {int(m.sum())} small entries: max relative error {rel:.3e}")
        assert rel <= 4 * LR.SOFTMAX_F32_DEV


@pytest.mark.parametrize("norm_mode", [0, 1])
@pytest.mark.parametrize("form", [0, 1], ids=["four_launch", "three_launch"])
@pytest.mark.parametrize("case_id", LR.CASE_IDS)
def test_loss_regime_equals_the_restatement(case_id, form, norm_mode):
    from objectdetection_ssd_amd import _lib, ops
    case, _ = LR.case_and_reference(case_id)
    args = _args(case_id)
    lib = _lib.load()
    try:
        _lib.check(lib.ssd_tune_set_loss_form(form), "tune")
        runs = []
        for _ in range(2):
            o = ops.multibox_loss(*args, iou_threshold=0.5, neg_pos_ratio=case.neg_pos_ratio, norm_mode=norm_mode)
            torch.cuda.synchronize()
            runs.append({k: v.cpu().numpy() for k, v in o.items()})
        fwd = ops.multibox_loss(*args, iou_threshold=0.5, neg_pos_ratio=case.neg_pos_ratio, norm_mode=norm_mode, want_grads=False)
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.ssd_tune_set_loss_form(1), "tune")
    a, b = runs
    _check_against_reference(case_id, norm_mode, float(a["losses"][0]), float(a["losses"][1]), int(a["losses"][2]), a["obj"], a["cls"],
                             a["dloc"], a["dconf"])
    for k in ("losses", "dloc", "dconf"):                                       # two launches, the same bits
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(a["obj"], b["obj"]) and np.array_equal(a["cls"], b["cls"])
    assert fwd["dloc"] is None and fwd["dconf"] is None                         # forward only: the same losses and classes
    assert np.array_equal(_bits(fwd["losses"].cpu().numpy()), _bits(a["losses"])) and np.array_equal(fwd["cls"].cpu().numpy(), a["cls"])


PUBLIC_CASES = [c for c in LR.CASE_IDS if "ssd_priors" in c]


@pytest.mark.parametrize("norm_mode", [0, 1])
@pytest.mark.parametrize("form", [0, 1], ids=["four_launch", "three_launch"])
@pytest.mark.parametrize("case_id", PUBLIC_CASES)
def test_trained_regime_through_the_public_loss(case_id, form, norm_mode):
    """Losses.ssd + backward() (the autograd wrapper, its own prior sets, last_match) on the `trained` cases at the prior counts it knows."""
    from objectdetection_ssd_amd import Losses, _lib
    case, _ = LR.case_and_reference(case_id)
    assert len(PUBLIC_CASES) == 3 and case.neg_pos_ratio == Losses.NEG_POS_RATIO
    loc, conf = _args(case_id)[:2]
    lt, ct = loc.clone().requires_grad_(True), conf.clone().requires_grad_(True)
    lib = _lib.load()
    try:
        _lib.check(lib.ssd_tune_set_loss_form(form), "tune")
        l1, l2, n_pos = Losses.ssd((lt, ct), [torch.tensor(c).to(DEV) for c in case.classes], [torch.tensor(b).to(DEV) for b in case.boxes],
                                   norm_mode=norm_mode, with_n_pos=True)
        (l1 + l2).backward()
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.ssd_tune_set_loss_form(1), "tune")
    m = Losses.last_match
    assert int(m["n_pos"].item()) == int(n_pos.item())
    _check_against_reference(case_id, norm_mode, l1.item(), l2.item(), int(n_pos.item()), m["obj"].cpu().numpy(), m["cls"].cpu().numpy(),
                             lt.grad.cpu().numpy(), ct.grad.cpu().numpy())

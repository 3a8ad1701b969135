"""ssd_multibox_loss_focal (csrc/loss.hip) on the cases of tests/focal_loss_cases.py, every case x (alpha, gamma) in both norm modes: what
the classification term must not touch (matching, ignore bytes, the loc side, n_pos) bit-equal to the cross-entropy call on the same
inputs; the exact zeros of dconf (the background column, ignored rows); every output finite; dconf against the float64 restatement
tests/focal_loss_ref.py to 8 x max(d32, 2^-23) of max |ref| over the whole tensor, d32 = the recorded distance of the float32
restatement for that case and parameter set (tests/golden/focal_loss_ref_distance.json); conf_loss to 1e-4 max(1, |ref|); two calls the
same bits; conf_mode 0 through the new entry bit-equal to the existing entries; and the public path `Losses.ssd(..., conf_loss="focal")`.

Measured on gfx950 (err / bar, the largest over the cases of a parameter set): see DESIGN.md section 4m."""
import json

import numpy as np
import pytest
import torch

import focal_loss_cases as FC
import focal_loss_ref as FR
import ssd_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_device_args = {}
_gold = {}
_ce = {}


def _starts(lists):
    return np.concatenate([[0], np.cumsum([len(b) for b in lists])]).astype(np.int32)


def _args(case_id):
    """the case on the device, uploaded once: (loc, conf, gt_boxes, gt_classes, img_start, priors_cxcywh, priors_xyxy), (ign_boxes, ign_start)"""
    if case_id not in _device_args:
        case, _ = FC.case_and_reference(case_id)
        host = (case.loc, case.conf, np.concatenate(case.boxes), np.concatenate(case.classes), _starts(case.boxes), case.priors_cxcywh,
                O.xywh_to_xyxy(case.priors_cxcywh))
        lists = case.ignore if case.ignore is not None else [np.zeros((0, 4), np.float32)] * case.conf.shape[0]
        ign = (np.concatenate(lists).astype(np.float32).reshape(-1, 4), _starts(lists))
        _device_args[case_id] = tuple(torch.tensor(a).to(DEV) for a in host), tuple(torch.tensor(a).to(DEV) for a in ign)
    return _device_args[case_id]


def _d32(case_id, alpha, gamma):
    if not _gold:
        with open(FR.GOLDEN) as f:
            _gold.update(json.load(f)["d32"])
    return _gold[f"{case_id}|{FR.param_id(alpha, gamma)}"]["dconf"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _host(o):
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}


def _run(case_id, norm_mode, focal=None, want_grads=True, ignore=None, loc_loss=None):
    """focal None: the cross-entropy call; (alpha, gamma): the focal one.  ignore None: as the case has it"""
    from objectdetection_ssd_amd import ops
    case, _ = FC.case_and_reference(case_id)
    args, (ib, ist) = _args(case_id)
    if ignore is None:
        ignore = case.ignore is not None
    kw = dict(ignore_boxes=ib, ignore_start=ist, ignore_threshold=case.threshold, ignore_overlap=case.overlap) if ignore else {}
    if focal is not None:
        kw.update(conf_loss="focal", focal_alpha=focal[0], focal_gamma=focal[1])
    return _host(ops.multibox_loss(*args, iou_threshold=0.5, neg_pos_ratio=case.neg_pos_ratio, norm_mode=norm_mode, want_grads=want_grads,
                                   loc_loss=case.loc_loss if loc_loss is None else loc_loss, **kw))


def _same_bits(a, b, keys=("losses", "dloc", "dconf")):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(a["obj"], b["obj"]) and np.array_equal(a["cls"], b["cls"]) and ("ign" in a) == ("ign" in b)
    if "ign" in a:
        assert np.array_equal(a["ign"], b["ign"])


CASES_PARAMS = [(c, p) for c in FC.CASE_IDS for p in FR.PARAMS]


@pytest.mark.parametrize("norm_mode", [0, 1])
@pytest.mark.parametrize("case_id,params", CASES_PARAMS, ids=[f"{c}-{FR.param_id(*p)}" for c, p in CASES_PARAMS])
def test_focal_loss_equals_the_restatement(case_id, params, norm_mode):
    case, base = FC.case_and_reference(case_id)
    alpha, gamma = params
    C = case.conf.shape[2]
    ce = _run(case_id, norm_mode)                                  # the cross-entropy entries, before and after
    plain = _run(case_id, norm_mode, ignore=False, loc_loss="l1")
    a = _run(case_id, norm_mode, params)
    b = _run(case_id, norm_mode, params)
    fwd = _run(case_id, norm_mode, params, want_grads=False)
    ce_after = _run(case_id, norm_mode)
    plain_after = _run(case_id, norm_mode, ignore=False, loc_loss="l1")

    # what the term must not touch: bit-equal to the cross-entropy call with the same loc_loss and ignore arguments
    assert np.array_equal(a["cls"], ce["cls"]) and np.array_equal(a["obj"], ce["obj"]) and ("ign" in a) == (case.ignore is not None)
    if "ign" in a:
        assert np.array_equal(a["ign"], ce["ign"]) and np.array_equal(a["ign"].astype(bool), base["ign"])
    assert np.array_equal(_bits(a["losses"][[0, 2]]), _bits(ce["losses"][[0, 2]])) and np.array_equal(_bits(a["dloc"]), _bits(ce["dloc"]))
    assert np.array_equal(a["cls"], base["cls"]) and int(a["losses"][2]) == base["n_pos"]

    # exact zeros (all bits) and finiteness
    dconf = a["dconf"]
    assert not _bits(dconf[..., C - 1]).any() and not _bits(dconf[base["ign"]]).any()
    assert np.isfinite(dconf).all() and np.isfinite(a["losses"]).all() and np.isfinite(a["dloc"]).all()

    # dconf and conf_loss against the float64 restatement: the whole tensor, no element left out
    ref = FC.reference(case_id, alpha, gamma, norm_mode)
    big = np.abs(ref["dconf"]).max()
    bar = 8 * max(_d32(case_id, alpha, gamma), 2.0 ** -23)
    err = np.abs(dconf - ref["dconf"]).max()
    conf_loss = float(a["losses"][1])
    print(f"{case_id} alpha {alpha} gamma {gamma} norm_mode {norm_mode}: dconf max |err| {err:.3e} of max |ref| {big:.3e}: {err / big:.3e} against "
          f"the bar {bar:.3e} ({err / big / bar:.3f} of it); conf_loss {conf_loss:.8g} (ref {ref['conf_loss']:.8g}, "
          f"{abs(conf_loss - ref['conf_loss']) / max(1.0, abs(ref['conf_loss'])):.2e} of 1e-4)")
    assert big > 0 and err <= bar * big
    assert abs(conf_loss - ref["conf_loss"]) <= 1e-4 * max(1.0, abs(ref["conf_loss"]))

    # repeatability and paths
    _same_bits(a, b)
    assert fwd["dloc"] is None and fwd["dconf"] is None and np.array_equal(_bits(fwd["losses"]), _bits(a["losses"]))
    assert np.array_equal(fwd["cls"], a["cls"]) and np.array_equal(fwd["obj"], a["obj"])
    _same_bits(ce, ce_after)
    _same_bits(plain, plain_after)
    assert "ign" not in plain


def _raw_entry(case_id, norm_mode, with_ignore, entry, loc_mode=0, conf_mode=0, alpha=0.25, gamma=2.0):
    """A C entry called directly: "focal" (ssd_multibox_loss_focal), "box", "ignore" or "plain"; the ignore pointers given or NULL"""
    from objectdetection_ssd_amd import _lib, ops
    case, _ = FC.case_and_reference(case_id)
    (loc, conf, gt, gcl, start, pri, pri_xyxy), (ib, ist) = _args(case_id)
    bs, p, ncls = conf.shape
    lib = _lib.load()
    n_ign = ib.shape[0] if with_ignore else 0
    ws = ops.workspace(lib.ssd_multibox_loss_focal_workspace(bs, p, gt.shape[0], n_ign), loc.device, "loss")
    losses = torch.empty((3,), device=DEV)
    obj, cls = torch.empty((bs, p), device=DEV, dtype=torch.int32), torch.empty((bs, p), device=DEV, dtype=torch.int32)
    ign = torch.empty((bs, p), device=DEV, dtype=torch.uint8) if with_ignore else None
    dloc, dconf = torch.empty_like(loc), torch.empty_like(conf)
    head = (loc.data_ptr(), conf.data_ptr(), gt.data_ptr(), gcl.data_ptr(), start.data_ptr(), bs, gt.shape[0], pri.data_ptr(),
            pri_xyxy.data_ptr(), p, ncls, 0.5, case.neg_pos_ratio, norm_mode)
    ignore = (ib.data_ptr() if n_ign else None, ist.data_ptr() if with_ignore else None, n_ign, float(case.threshold),
              ops.ignore_overlap_mode(case.overlap))
    outs = (losses.data_ptr(), obj.data_ptr(), cls.data_ptr())
    tail = (dloc.data_ptr(), dconf.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    ign_ptr = None if ign is None else ign.data_ptr()
    if entry == "focal":
        ops.check(lib.ssd_multibox_loss_focal(*head, *ignore, loc_mode, conf_mode, alpha, gamma, *outs, ign_ptr, *tail), "multibox_loss_focal")
    elif entry == "box":
        ops.check(lib.ssd_multibox_loss_box(*head, *ignore, loc_mode, *outs, ign_ptr, *tail), "multibox_loss_box")
    elif entry == "ignore":
        ops.check(lib.ssd_multibox_loss_ignore(*head, *ignore, *outs, ign_ptr, *tail), "multibox_loss_ignore")
    else:
        ops.check(lib.ssd_multibox_loss(*head, *outs, *tail), "multibox_loss")
    out = dict(losses=losses, obj=obj, cls=cls, dloc=dloc, dconf=dconf)
    if ign is not None:
        out["ign"] = ign
    return _host(out)


@pytest.mark.parametrize("norm_mode", [0, 1])
@pytest.mark.parametrize("case_id", ["trained-P777-C21-bs3-ignore", "trained-P1000-C81-bs3-ignore", "many_boxes-P777-C81-bs3",
                                     "extreme-P777-C21-bs3", FC.P8732_ID])
def test_conf_mode_0_through_the_new_entry_is_the_existing_entries_bit_for_bit(case_id, norm_mode):
    for with_ignore in (False, True):
        for loc_mode, loc_loss in ((0, "l1"), (4, "ciou")):
            f0 = _raw_entry(case_id, norm_mode, with_ignore, "focal", loc_mode, 0, alpha=0.9, gamma=0.5)      # (parameters conf_mode 0 does not read)
            _same_bits(f0, _raw_entry(case_id, norm_mode, with_ignore, "box", loc_mode))
            _same_bits(f0, _run(case_id, norm_mode, ignore=with_ignore, loc_loss=loc_loss))
        _same_bits(_raw_entry(case_id, norm_mode, with_ignore, "focal"), _raw_entry(case_id, norm_mode, with_ignore, "ignore" if with_ignore else "plain"))
        # and the raw call is the one ops makes for the focal term
        _same_bits(_raw_entry(case_id, norm_mode, with_ignore, "focal", 4, 1, -1.0, 1.5), _run(case_id, norm_mode, (-1.0, 1.5), ignore=with_ignore, loc_loss="ciou"))


@pytest.mark.parametrize("norm_mode", [0, 1])
@pytest.mark.parametrize("case_id", ["trained-P777-C21-bs3-ignore", "extreme-P1000-C81-bs1", FC.P8732_ID])
def test_the_dense_pass_alone_is_the_dense_pass_of_the_call(case_id, norm_mode):
    """ssd_focal_dense on the reference's classes and ignore mask: conf_loss and dconf of the whole call, bit for bit; without dconf the
    same conf_loss"""
    from objectdetection_ssd_amd import _lib, ops
    case, base = FC.case_and_reference(case_id)
    alpha, gamma = 0.25, 2.0
    whole = _run(case_id, norm_mode, (alpha, gamma))
    conf = _args(case_id)[0][1]
    bs, p, ncls = conf.shape
    lib = _lib.load()
    cls = torch.tensor(base["cls"].astype(np.int32)).to(DEV)
    ign = torch.tensor(base["ign"].astype(np.uint8)).to(DEV) if case.ignore is not None else None
    ws = torch.empty(lib.ssd_focal_dense_workspace(bs, p), device=DEV, dtype=torch.uint8)
    for with_grad in (True, False):
        loss, dconf = torch.full((1,), -1.0, device=DEV), torch.full_like(conf, -1.0)
        ops.check(lib.ssd_focal_dense(conf.data_ptr(), cls.data_ptr(), None if ign is None else ign.data_ptr(), bs, p, ncls, float(base["n_pos"]),
                                      norm_mode, alpha, gamma, loss.data_ptr(), dconf.data_ptr() if with_grad else None, ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream().cuda_stream), "focal_dense")
        torch.cuda.synchronize()
        assert np.array_equal(_bits(loss.cpu().numpy()), _bits(whole["losses"][1:2]))
        if with_grad:
            assert np.array_equal(_bits(dconf.cpu().numpy()), _bits(whole["dconf"]))
        else:
            assert (dconf == -1.0).all()


@pytest.mark.parametrize("with_ignore", [False, True])
@pytest.mark.parametrize("norm_mode", [0, 1])
def test_focal_loss_through_the_public_loss(norm_mode, with_ignore):
    """Losses.ssd(..., conf_loss="focal") + backward(): the gradients and losses of the ops call; a following default call is today's"""
    from objectdetection_ssd_amd import Losses
    case_id = FC.P8732_ID
    case, base = FC.case_and_reference(case_id)
    assert case.neg_pos_ratio == Losses.NEG_POS_RATIO
    (loc, conf, *_), _ = _args(case_id)
    lt, ct = loc.clone().requires_grad_(True), conf.clone().requires_grad_(True)
    cl, bx = [torch.tensor(c).to(DEV) for c in case.classes], [torch.tensor(b).to(DEV) for b in case.boxes]
    kw = dict(ignore_bboxs=[torch.tensor(b) for b in case.ignore], ignore_threshold=case.threshold, ignore_overlap=case.overlap) if with_ignore else {}
    l1, l2, n_pos = Losses.ssd((lt, ct), cl, bx, norm_mode=norm_mode, with_n_pos=True, conf_loss="focal", focal_alpha=0.75, focal_gamma=5.0, **kw)
    (l1 + l2).backward()
    torch.cuda.synchronize()
    assert set(Losses.last_match) == ({"obj", "cls", "n_pos", "ignored"} if with_ignore else {"obj", "cls", "n_pos"})
    o = _run(case_id, norm_mode, (0.75, 5.0), ignore=with_ignore)
    assert np.array_equal(_bits(lt.grad.cpu().numpy()), _bits(o["dloc"])) and np.array_equal(_bits(ct.grad.cpu().numpy()), _bits(o["dconf"]))
    assert np.array_equal(_bits(np.asarray([l1.item(), l2.item(), n_pos.item()])), _bits(o["losses"]))
    negatives = ~base["pos"] & ~base["ign"] if with_ignore else ~base["pos"]
    assert o["dconf"][negatives].any() and o["dconf"][base["pos"]].any()
    d1, d2 = Losses.ssd((loc, conf), cl, bx, norm_mode=norm_mode)                    # the default: the plain entry, as today
    torch.cuda.synchronize()
    m = Losses.last_match
    plain = _run(case_id, norm_mode, ignore=False)
    assert set(m) == {"obj", "cls", "n_pos"} and np.array_equal(m["obj"].cpu().numpy(), plain["obj"]) and np.array_equal(m["cls"].cpu().numpy(), plain["cls"])
    assert np.array_equal(_bits(np.asarray([d1.item(), d2.item()])), _bits(plain["losses"][:2]))
    with pytest.raises(ValueError):
        Losses.ssd((loc, conf), cl, bx, conf_loss="focal", focal_gamma=-1.0)

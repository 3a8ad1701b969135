"""ssd_multibox_loss_box (csrc/loss.hip) on the cases of tests/box_loss_cases.py, every case x mode in both norm modes: what the mode
must not touch (matching, mining, ignore regions, the conf side) bit-equal to the existing entries on the same inputs; the exact zeros
of dloc; dloc against the float64 restatement tests/box_loss_ref.py to 8 x max(d32, 2^-23) of max |ref|, d32 = the recorded distance of
the float32 restatement for that case and mode (tests/golden/box_loss_ref_distance.json); loc_loss to 1e-4 max(1, |ref|); loc_mode 0
through the new entry bit-equal to the two existing entries; and the public path `Losses.ssd(..., loc_loss=...)`."""
import json

import numpy as np
import pytest
import torch

import box_loss_cases as BC
import box_loss_ref as BR
import ssd_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_device_args = {}
_gold = {}


def _starts(lists):
    return np.concatenate([[0], np.cumsum([len(b) for b in lists])]).astype(np.int32)


def _args(case_id):
    """the case on the device, uploaded once: (loc, conf, gt_boxes, gt_classes, img_start, priors_cxcywh, priors_xyxy), (ign_boxes, ign_start)
    -- the latter of the case's ignore boxes, or of none"""
    if case_id not in _device_args:
        case, _ = BC.case_and_reference(case_id)
        host = (case.loc, case.conf, np.concatenate(case.boxes), np.concatenate(case.classes), _starts(case.boxes), case.priors_cxcywh,
                O.xywh_to_xyxy(case.priors_cxcywh))
        lists = case.ignore if case.ignore is not None else [np.zeros((0, 4), np.float32)] * case.conf.shape[0]
        ign = (np.concatenate(lists).astype(np.float32).reshape(-1, 4), _starts(lists))
        _device_args[case_id] = tuple(torch.tensor(a).to(DEV) for a in host), tuple(torch.tensor(a).to(DEV) for a in ign)
    return _device_args[case_id]


def _d32(case_id, mode):
    if not _gold:
        with open(BR.GOLDEN) as f:
            _gold.update(json.load(f)["d32"])
    return _gold[f"{case_id}|{mode}"]["dloc"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _host(o):
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}


def _run(case_id, norm_mode, loc_loss="l1", want_grads=True, ignore=None):
    """ignore None: as the case has it; True: the entry with ignore regions (of the case's boxes, or of none); False: without"""
    from objectdetection_ssd_amd import ops
    case, _ = BC.case_and_reference(case_id)
    args, (ib, ist) = _args(case_id)
    if ignore is None:
        ignore = case.ignore is not None
    kw = dict(ignore_boxes=ib, ignore_start=ist, ignore_threshold=case.threshold, ignore_overlap=case.overlap) if ignore else {}
    return _host(ops.multibox_loss(*args, iou_threshold=0.5, neg_pos_ratio=case.neg_pos_ratio, norm_mode=norm_mode, want_grads=want_grads,
                                   loc_loss=loc_loss, **kw))


def _same_bits(a, b, keys=("losses", "dloc", "dconf")):
    for k in keys:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(a["obj"], b["obj"]) and np.array_equal(a["cls"], b["cls"]) and ("ign" in a) == ("ign" in b)
    if "ign" in a:
        assert np.array_equal(a["ign"], b["ign"])


def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


CASES_MODES = [(c, m) for c in BC.CASE_IDS for m in BC.modes_of(c)]


@pytest.mark.parametrize("norm_mode", [0, 1])
@pytest.mark.parametrize("case_id,mode", CASES_MODES, ids=[f"{c}-{m}" for c, m in CASES_MODES])
def test_box_loss_equals_the_restatement(case_id, mode, norm_mode):
    case, base = BC.case_and_reference(case_id)
    pos = base["pos"]
    before = [_run(case_id, norm_mode, ignore=False), _run(case_id, norm_mode, ignore=True)]       # the existing entries, before and after
    a = _run(case_id, norm_mode, mode)
    b = _run(case_id, norm_mode, mode)
    fwd = _run(case_id, norm_mode, mode, want_grads=False)
    after = [_run(case_id, norm_mode, ignore=False), _run(case_id, norm_mode, ignore=True)]
    l1 = before[1] if case.ignore is not None else before[0]

    # what the mode must not touch: bit-equal to the L1 call on the same inputs
    assert np.array_equal(a["cls"], l1["cls"]) and np.array_equal(a["obj"], l1["obj"]) and ("ign" in a) == (case.ignore is not None)
    if "ign" in a:
        assert np.array_equal(a["ign"], l1["ign"]) and np.array_equal(a["ign"].astype(bool), base["ign"])
    assert np.array_equal(_bits(a["losses"][1:]), _bits(l1["losses"][1:])) and np.array_equal(_bits(a["dconf"]), _bits(l1["dconf"]))
    assert np.array_equal(a["cls"], base["cls"]) and int(a["losses"][2]) == base["n_pos"]

    # exact zeros
    dloc = a["dloc"]
    assert not dloc[~pos].any()
    if "clamped" in case_id:
        third = BC.clamped_rows(base["n_pos"])
        assert third.any() and not dloc[pos][third, 2:].any() and dloc[pos][~third, 2:].any()
    n_pos = base["n_pos"]
    loc_loss = float(a["losses"][0])
    if case_id == BC.FAR_ID and mode == "iou":
        assert not dloc.any()
        assert _ulps(loc_loss, n_pos if norm_mode == 1 else 1.0) <= 1

    # dloc and loc_loss against the float64 restatement
    ref = BC.reference(case_id, mode, norm_mode)
    big = np.abs(ref["dloc"]).max()
    bar = 8 * max(_d32(case_id, mode), 2.0 ** -23)
    err = np.abs(dloc - ref["dloc"]).max()
    print(f"{case_id} {mode} norm_mode {norm_mode}: dloc max |err| {err:.3e} of max |ref| {big:.3e}: {err / big if big else 0:.3e} against the bar "
          f"{bar:.3e} ({(err / big if big else 0) / bar:.3f} of it); loc_loss {loc_loss:.8g} (ref {ref['loc_loss']:.8g})")
    assert np.isfinite(dloc).all() and err <= bar * big
    assert abs(loc_loss - ref["loc_loss"]) <= 1e-4 * max(1.0, abs(ref["loc_loss"]))

    # repeatability and paths
    _same_bits(a, b)
    assert fwd["dloc"] is None and fwd["dconf"] is None and np.array_equal(_bits(fwd["losses"]), _bits(a["losses"]))
    assert np.array_equal(fwd["cls"], a["cls"]) and np.array_equal(fwd["obj"], a["obj"])
    for x, y in zip(before, after):
        _same_bits(x, y)
    assert "ign" not in before[0] and "ign" in before[1]


def _raw_entry(case_id, norm_mode, with_ignore, loc_mode=None):
    """A C entry called directly.  loc_mode 0 .. 4: ssd_multibox_loss_box (the entry ops.multibox_loss calls whenever an option is set), the
    ignore pointers given or NULL.  loc_mode None: the entries without a loc_mode, ssd_multibox_loss_ignore or ssd_multibox_loss."""
    from objectdetection_ssd_amd import _lib, ops
    case, _ = BC.case_and_reference(case_id)
    (loc, conf, gt, gcl, start, pri, pri_xyxy), (ib, ist) = _args(case_id)
    bs, p, ncls = conf.shape
    lib = _lib.load()
    n_ign = ib.shape[0] if with_ignore else 0
    ws = ops.workspace(lib.ssd_multibox_loss_box_workspace(bs, p, gt.shape[0], n_ign), loc.device, "loss")
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
    if loc_mode is not None:
        ops.check(lib.ssd_multibox_loss_box(*head, *ignore, loc_mode, *outs, ign_ptr, *tail), "multibox_loss_box")
    elif with_ignore:
        ops.check(lib.ssd_multibox_loss_ignore(*head, *ignore, *outs, ign_ptr, *tail), "multibox_loss_ignore")
    else:
        ops.check(lib.ssd_multibox_loss(*head, *outs, *tail), "multibox_loss")
    out = dict(losses=losses, obj=obj, cls=cls, dloc=dloc, dconf=dconf)
    if ign is not None:
        out["ign"] = ign
    return _host(out)


@pytest.mark.parametrize("norm_mode", [0, 1])
@pytest.mark.parametrize("case_id", ["trained-P777-C21-bs3-near-ignore", "trained-P1000-C81-bs3-noise-ignore", "many_boxes-P1000-C81-bs3-noise",
                                     "many_boxes-P777-C21-bs3-near", "trained-P8732-C21-bs2-near-ignore"])
def test_loc_mode_0_through_the_new_entry_is_the_existing_entries_bit_for_bit(case_id, norm_mode):
    for with_ignore in (False, True):
        box0 = _raw_entry(case_id, norm_mode, with_ignore, 0)
        _same_bits(box0, _raw_entry(case_id, norm_mode, with_ignore))
        _same_bits(box0, _run(case_id, norm_mode, ignore=with_ignore))
    # and the raw call is the one ops makes for a box mode
    _same_bits(_raw_entry(case_id, norm_mode, True, 3), _run(case_id, norm_mode, "diou", ignore=True))
    _same_bits(_raw_entry(case_id, norm_mode, False, 3), _run(case_id, norm_mode, "diou", ignore=False))


@pytest.mark.parametrize("with_ignore", [False, True])
@pytest.mark.parametrize("norm_mode", [0, 1])
def test_box_loss_through_the_public_loss(norm_mode, with_ignore):
    """Losses.ssd(..., loc_loss="ciou") + backward(): the gradients and losses of the ops call; a following default call is today's"""
    from objectdetection_ssd_amd import Losses
    case_id = BC.P8732_ID
    case, base = BC.case_and_reference(case_id)
    assert case.neg_pos_ratio == Losses.NEG_POS_RATIO
    (loc, conf, *_), _ = _args(case_id)
    lt, ct = loc.clone().requires_grad_(True), conf.clone().requires_grad_(True)
    cl, bx = [torch.tensor(c).to(DEV) for c in case.classes], [torch.tensor(b).to(DEV) for b in case.boxes]
    kw = dict(ignore_bboxs=[torch.tensor(b) for b in case.ignore], ignore_threshold=case.threshold, ignore_overlap=case.overlap) if with_ignore else {}
    l1, l2, n_pos = Losses.ssd((lt, ct), cl, bx, norm_mode=norm_mode, with_n_pos=True, loc_loss="ciou", **kw)
    (l1 + l2).backward()
    torch.cuda.synchronize()
    assert ("ignored" in Losses.last_match) == with_ignore
    o = _run(case_id, norm_mode, "ciou", ignore=with_ignore)
    assert np.array_equal(_bits(lt.grad.cpu().numpy()), _bits(o["dloc"])) and np.array_equal(_bits(ct.grad.cpu().numpy()), _bits(o["dconf"]))
    assert np.array_equal(_bits(np.asarray([l1.item(), l2.item(), n_pos.item()])), _bits(o["losses"]))
    assert o["dloc"][base["pos"]].any()
    d1, d2 = Losses.ssd((loc, conf), cl, bx, norm_mode=norm_mode)                    # the default: the plain L1 entry, as today
    torch.cuda.synchronize()
    m = Losses.last_match
    plain = _run(case_id, norm_mode, ignore=False)
    assert set(m) == {"obj", "cls", "n_pos"} and np.array_equal(m["obj"].cpu().numpy(), plain["obj"]) and np.array_equal(m["cls"].cpu().numpy(), plain["cls"])
    assert np.array_equal(_bits(np.asarray([d1.item(), d2.item()])), _bits(plain["losses"][:2]))

"""ATSS matching on the device (csrc/atss.hip, ssd_multibox_loss_atss in csrc/loss.hip) against tests/atss_ref.py on the cases of
tests/atss_cases.py.

1. ssd_atss_assign bare: assignment, candidate and accepted counts equal, mean and variance equal in their float64 bits (two NaNs
   are equal whatever their payload: the box with a NaN coordinate).
2. ops.multibox_loss(match="atss"), C = 21 (narrow L1) and 81 (wide L1), cross entropy and focal x ignore boxes or none x "l1" and
   "ciou" x both norm modes: cls everywhere and obj at the positives exact; the rest to the bars of the tests of those quantities --
   losses to 1e-4 max(1, |ref|), the rows with a conf gradient exact and dconf to 1e-5 max |ref| (tests/test_ignore_loss_gpu.py), the
   L1 dloc bit for bit (same), the "ciou" dloc and the focal dconf to 8 x max(d32, 2^-23) of max |ref| with d32 recorded in
   tests/golden/atss_ref_distance.json (tests/test_box_loss_gpu.py, tests/test_focal_loss_gpu.py).  Image 1 of every batch has no
   positive: every output finite, no row of it mined (sel all zero: its cross-entropy dconf rows and its dloc rows are zero).
3. match_mode 0 through the new entry bit-equal to the three older ones; two ATSS calls the same bits; the ATSS call on a workspace
   full of 0xFF bytes and on one full of zeros the same bits (L2 reads forced matches out of the workspace).
4. Losses.ssd(match="atss") + backward() gives the gradients of 2.

Measured on gfx950 (the largest over all cases): no prior, count or statistics bit differs in 1; in 2 the "ciou" dloc reaches 0.16 and
the focal dconf 0.21 of their bars, the cross-entropy dconf 2.9e-7 of max |ref| against 1e-5; see DESIGN.md section 4n."""
import numpy as np
import pytest
import torch

import atss_cases as AC
import ssd_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_dev = {}


def _t(a):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV)


def _starts(lists):
    return np.concatenate([[0], np.cumsum([len(b) for b in lists])]).astype(np.int32)


def _priors(name):
    if name not in _dev:
        pri, levels = AC.prior_set(name)
        _dev[name] = (_t(pri), _t(np.ascontiguousarray(O.xywh_to_xyxy(pri), np.float32)), levels)
    return _dev[name]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _host(o):
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in o.items()}


def _same_f64(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


@pytest.mark.parametrize("topk", AC.TOPKS)
@pytest.mark.parametrize("name", AC.SETS)
def test_the_assignment_pass_is_the_restatement(name, topk):
    from objectdetection_ssd_amd import ops
    pri, pri_xyxy, levels = _priors(name)
    boxes = AC.assign_boxes(name)
    ref = AC.assignment(name, topk)
    args = (_t(np.concatenate(boxes)), _t(_starts(boxes)), pri, pri_xyxy, levels)
    a = _host(ops.atss_assign(*args, atss_topk=topk))
    b = _host(ops.atss_assign(*args, atss_topk=topk))
    print(f"{name} topk {topk}: candidates {ref['n_cand'][0]}, accepted per box {ref['n_acc'].min()} .. {ref['n_acc'].max()}, positives per "
          f"image {(ref['assign'] >= 0).sum(1)}, differing priors {(a['assign'] != ref['assign']).sum()}")
    assert np.array_equal(a["n_cand"], ref["n_cand"])
    assert _same_f64(a["mean"], ref["mean"]) and _same_f64(a["var"], ref["var"])
    assert np.array_equal(a["n_acc"], ref["n_acc"])
    assert np.array_equal(a["assign"], ref["assign"])
    assert (ref["assign"] >= 0).any() and (ref["n_acc"] == 0).any()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=k in ("mean", "var")), k


def _loss_args(name, C):
    key = ("loss", name, C)
    if key not in _dev:
        c = AC.loss_case(name, C)
        pri, pri_xyxy, _ = _priors(name)
        _dev[key] = ((_t(c.loc), _t(c.conf), _t(np.concatenate(c.boxes)), _t(np.concatenate(c.classes)), _t(_starts(c.boxes)), pri, pri_xyxy),
                     (_t(np.concatenate(c.ignore)), _t(_starts(c.ignore))))
    return _dev[key]


def _run(name, C, norm_mode, focal=False, ignore=False, loc_loss="l1", match="atss", want_grads=True):
    from objectdetection_ssd_amd import ops
    args, (ib, ist) = _loss_args(name, C)
    kw = dict(ignore_boxes=ib, ignore_start=ist) if ignore else {}
    if focal:
        kw.update(conf_loss="focal", focal_alpha=AC.FOCAL[0], focal_gamma=AC.FOCAL[1])
    if match == "atss":
        kw.update(match="atss", atss_topk=9, prior_levels=AC.prior_set(name)[1])
    return _host(ops.multibox_loss(*args, iou_threshold=0.5, neg_pos_ratio=AC.NEG_POS_RATIO, norm_mode=norm_mode, want_grads=want_grads,
                                   loc_loss=loc_loss, **kw))


@pytest.mark.parametrize("C", AC.CLASS_COUNTS)
@pytest.mark.parametrize("name", AC.SETS)
def test_the_loss_on_the_assignment_is_the_restatement(name, C):
    import atss_ref as AR
    case = AC.loss_case(name, C)
    for ignore in (False, True):
        ref = AC.loss_reference(name, C, ignore)
        pos, n_pos = ref["pos"], ref["n_pos"]
        assert not pos[1].any() and pos[0].any() and n_pos > 0
        for norm_mode in (0, 1):
            scale = 1.0 if norm_mode == 0 else float(n_pos)
            for loc_loss in ("l1", "ciou"):
                box = AR.box_side(case.loc, case.priors_cxcywh, ref, "ciou", norm_mode=norm_mode) if loc_loss == "ciou" else None
                for focal in (False, True):
                    o = _run(name, C, norm_mode, focal, ignore, loc_loss)
                    tag = f"{name} C{C} {'ign' if ignore else 'plain'} norm {norm_mode} {loc_loss} {'focal' if focal else 'ce'}"
                    # the assignment
                    assert np.array_equal(o["cls"], ref["cls"]), tag
                    assert np.array_equal(o["obj"][pos], ref["obj"][pos]), tag
                    assert float(o["losses"][2]) == n_pos, tag
                    assert ("ign" in o) == ignore
                    if ignore:
                        assert np.array_equal(o["ign"].astype(bool), ref["ign"]), tag
                    assert all(np.isfinite(o[k]).all() for k in ("losses", "dloc", "dconf")), tag
                    assert not o["dloc"][~pos].any() and not o["dloc"][1].any(), tag
                    loc_v, conf_v = float(o["losses"][0]), float(o["losses"][1])
                    # the loc side
                    if loc_loss == "l1":
                        want = ref["loc_loss"] * scale
                        factor = np.float32(0.25) * (np.float32(1) / np.float32(n_pos) if norm_mode == 0 else np.float32(1))
                        assert np.array_equal(_bits(o["dloc"]), _bits(np.sign(ref["dloc"]).astype(np.float32) * factor)), tag
                    else:
                        want = box["loc_loss"]
                        big = np.abs(box["dloc"]).max()
                        bar = 8 * max(AC.d32(f"{name}|C{C}|ciou"), 2.0 ** -23)
                        err = np.abs(o["dloc"] - box["dloc"]).max()
                        print(f"{tag}: dloc max |err| / max |ref| {err / big:.3e} against the bar {bar:.3e} ({err / big / bar:.3f} of it)")
                        assert big > 0 and err <= bar * big, tag
                    assert abs(loc_v - want) <= 1e-4 * max(1.0, abs(want)), (tag, loc_v, want)
                    # the conf side
                    if focal:
                        fr = AR.focal_side(case.conf, ref, *AC.FOCAL, norm_mode=norm_mode)
                        big = np.abs(fr["dconf"]).max()
                        bar = 8 * max(AC.d32(f"{name}|C{C}|{'ign' if ignore else 'plain'}|focal"), 2.0 ** -23)
                        err = np.abs(o["dconf"] - fr["dconf"]).max()
                        print(f"{tag}: dconf max |err| / max |ref| {err / big:.3e} against the bar {bar:.3e} ({err / big / bar:.3f} of it); "
                              f"conf_loss {conf_v:.8g} (ref {fr['conf_loss']:.8g})")
                        assert big > 0 and err <= bar * big, tag
                        assert abs(conf_v - fr["conf_loss"]) <= 1e-4 * max(1.0, abs(fr["conf_loss"])), tag
                        assert not _bits(o["dconf"][..., C - 1]).any() and not _bits(o["dconf"][ref["ign"]]).any(), tag
                    else:
                        want = ref["conf_loss"] * scale
                        assert np.array_equal((o["dconf"] != 0).any(-1), ref["sel"]), tag      # the rows with a gradient: positives + mined
                        assert not o["dconf"][1].any(), tag                                       # the image without a positive: sel all zero
                        wd = ref["dconf"] * scale
                        err = np.abs(o["dconf"] - wd).max()
                        print(f"{tag}: dconf max |err| {err:.3e} of max |ref| {np.abs(wd).max():.3e}; conf_loss {conf_v:.8g} (ref {want:.8g})")
                        assert err <= 1e-5 * np.abs(wd).max(), tag
                        assert abs(conf_v - want) <= 1e-4 * max(1.0, abs(want)), (tag, conf_v, want)


def _raw(name, C, norm_mode, with_ignore, entry, loc_mode=0, conf_mode=0, match_mode=0, fill=None):
    """A C entry called directly on a workspace of its own: "atss", "focal", "box" or "plain"; fill: the byte the workspace holds"""
    from objectdetection_ssd_amd import _lib, ops
    (loc, conf, gt, gcl, start, pri, pri_xyxy), (ib, ist) = _loss_args(name, C)
    bs, p, ncls = conf.shape
    lib = _lib.load()
    n_ign = ib.shape[0] if with_ignore else 0
    nbytes = lib.ssd_multibox_loss_atss_workspace(bs, p, gt.shape[0], n_ign)
    assert nbytes > lib.ssd_multibox_loss_focal_workspace(bs, p, gt.shape[0], n_ign)
    ws = torch.full((nbytes,), 0 if fill is None else fill, device=DEV, dtype=torch.uint8)
    losses = torch.empty((3,), device=DEV)
    obj, cls = torch.empty((bs, p), device=DEV, dtype=torch.int32), torch.empty((bs, p), device=DEV, dtype=torch.int32)
    ign = torch.empty((bs, p), device=DEV, dtype=torch.uint8) if with_ignore else None
    dloc, dconf = torch.empty_like(loc), torch.empty_like(conf)
    head = (loc.data_ptr(), conf.data_ptr(), gt.data_ptr(), gcl.data_ptr(), start.data_ptr(), bs, gt.shape[0], pri.data_ptr(),
            pri_xyxy.data_ptr(), p, ncls, 0.5, AC.NEG_POS_RATIO, norm_mode)
    ignore = (ib.data_ptr() if n_ign else None, ist.data_ptr() if with_ignore else None, n_ign, 0.5, 0)
    outs = (losses.data_ptr(), obj.data_ptr(), cls.data_ptr())
    tail = (dloc.data_ptr(), dconf.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    ign_ptr = None if ign is None else ign.data_ptr()
    if entry == "atss":
        cells, anchors = ops.atss_levels(AC.prior_set(name)[1], p)
        ops.check(lib.ssd_multibox_loss_atss(*head, *ignore, loc_mode, conf_mode, *AC.FOCAL, match_mode, 9, len(cells), cells, anchors, *outs,
                                             ign_ptr, *tail), "multibox_loss_atss")
    elif entry == "focal":
        ops.check(lib.ssd_multibox_loss_focal(*head, *ignore, loc_mode, conf_mode, *AC.FOCAL, *outs, ign_ptr, *tail), "multibox_loss_focal")
    elif entry == "box":
        ops.check(lib.ssd_multibox_loss_box(*head, *ignore, loc_mode, *outs, ign_ptr, *tail), "multibox_loss_box")
    else:
        ops.check(lib.ssd_multibox_loss(*head, *outs, *tail), "multibox_loss")
    out = dict(losses=losses, obj=obj, cls=cls, dloc=dloc, dconf=dconf)
    if ign is not None:
        out["ign"] = ign
    return _host(out)


def _same_bits(a, b, obj_at=None):
    for k in ("losses", "dloc", "dconf"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k
    assert np.array_equal(a["cls"], b["cls"]) and ("ign" in a) == ("ign" in b)
    if obj_at is None:
        assert np.array_equal(a["obj"], b["obj"])
    else:
        assert np.array_equal(a["obj"][obj_at], b["obj"][obj_at])
    if "ign" in a:
        assert np.array_equal(a["ign"], b["ign"])


@pytest.mark.parametrize("norm_mode", [0, 1])
@pytest.mark.parametrize("name,C", [("g8421", 21), ("g5321", 81), ("ssd300", 21)])
def test_match_mode_0_is_the_existing_entries_and_atss_is_repeatable_on_any_workspace(name, C, norm_mode):
    for with_ignore in (False, True):
        for loc_mode in (0, 4):
            for conf_mode in (0, 1):
                m0 = _raw(name, C, norm_mode, with_ignore, "atss", loc_mode, conf_mode, 0, fill=0xFF)
                _same_bits(m0, _raw(name, C, norm_mode, with_ignore, "focal", loc_mode, conf_mode))
                if conf_mode == 0:
                    _same_bits(m0, _raw(name, C, norm_mode, with_ignore, "box", loc_mode))
                    if loc_mode == 0 and not with_ignore:
                        _same_bits(m0, _raw(name, C, norm_mode, False, "plain"))
                zeros = _raw(name, C, norm_mode, with_ignore, "atss", loc_mode, conf_mode, 1, fill=0)
                ones = _raw(name, C, norm_mode, with_ignore, "atss", loc_mode, conf_mode, 1, fill=0xFF)
                again = _raw(name, C, norm_mode, with_ignore, "atss", loc_mode, conf_mode, 1, fill=0xFF)
                pos = zeros["cls"] != C - 1
                _same_bits(zeros, ones, obj_at=pos)
                _same_bits(ones, again)
                assert not np.array_equal(zeros["cls"], m0["cls"])             # the rule is not the IoU rule
                # and the raw call is the one ops makes
                _same_bits(ones, _run(name, C, norm_mode, conf_mode == 1, with_ignore, "ciou" if loc_mode else "l1"))


@pytest.mark.parametrize("focal", [False, True])
@pytest.mark.parametrize("norm_mode", [0, 1])
def test_atss_through_the_public_loss(norm_mode, focal):
    """Losses.ssd(..., match="atss") + backward(): the gradients and losses of the ops call; a following default call is the plain one"""
    from objectdetection_ssd_amd import Losses
    name, C = "ssd300", 21
    case = AC.loss_case(name, C)
    (loc, conf, *_), _ = _loss_args(name, C)
    lt, ct = loc.clone().requires_grad_(True), conf.clone().requires_grad_(True)
    cl, bx = [_t(c) for c in case.classes], [_t(b) for b in case.boxes]
    kw = dict(conf_loss="focal", focal_alpha=AC.FOCAL[0], focal_gamma=AC.FOCAL[1]) if focal else {}
    l1, l2, n_pos = Losses.ssd((lt, ct), cl, bx, norm_mode=norm_mode, with_n_pos=True, loc_loss="ciou", match="atss", atss_topk=9, **kw)
    (l1 + l2).backward()
    torch.cuda.synchronize()
    o = _run(name, C, norm_mode, focal, False, "ciou")
    assert np.array_equal(_bits(lt.grad.cpu().numpy()), _bits(o["dloc"])) and np.array_equal(_bits(ct.grad.cpu().numpy()), _bits(o["dconf"]))
    assert np.array_equal(_bits(np.asarray([l1.item(), l2.item(), n_pos.item()])), _bits(o["losses"]))
    assert np.array_equal(Losses.last_match["cls"].cpu().numpy(), o["cls"]) and o["dloc"].any() and o["dconf"].any()
    d1, d2 = Losses.ssd((loc, conf), cl, bx, norm_mode=norm_mode)                    # the default: the plain entry, as ever
    torch.cuda.synchronize()
    plain = _run(name, C, norm_mode, match="iou")
    assert np.array_equal(Losses.last_match["cls"].cpu().numpy(), plain["cls"])
    assert np.array_equal(_bits(np.asarray([d1.item(), d2.item()])), _bits(plain["losses"][:2]))
    with pytest.raises(ValueError):
        Losses.ssd((loc, conf), cl, bx, match="nearest")
    with pytest.raises(ValueError):
        Losses.ssd((loc, conf), cl, bx, match="atss", atss_topk=0)

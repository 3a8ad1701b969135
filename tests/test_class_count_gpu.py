"""Configurable class count on the GPU: MultiBox loss (incl. the wide-row kernels past C = 64), decode + NMS, get_map, the SSD300
heads at 81 columns (f32 and bf16), the train step against a decision-pinned f64 restatement, the graphed and data-parallel
steps, and SSD512 -- all against tests/class_count_ref.py, the C-general restatement of the reference."""
import os

import numpy as np
import pytest
import torch

import class_count_ref as R
import ssd_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _gt(rng, bs, C):
    boxes, classes = [], []
    for _ in range(bs):
        n = 1 + min(int(rng.poisson(1.4)), 7)
        x1 = rng.uniform(0, .6, n); y1 = rng.uniform(0, .6, n)
        w = rng.uniform(.08, .6, n); h = rng.uniform(.08, .6, n)
        boxes.append(np.stack([x1, y1, np.minimum(x1 + w, 1.), np.minimum(y1 + h, 1.)], 1).astype(np.float32))
        classes.append(rng.integers(0, C - 1, n).astype(np.float32))
    return boxes, classes


def _loss_case(C, degenerate, gold_dir):
    rng = np.random.default_rng(1000 + C)
    bs = 8
    boxes, classes = _gt(rng, bs, C)
    if degenerate:                   # the reference's degenerate ground truth (zero-area / zero-height boxes) in the first images
        z = np.load(os.path.join(gold_dir, "degenerate.npz"))
        for ci in range(int(z["n_cases"])):
            p = f"c{ci}_"
            counts = z[p + "counts"]
            off = np.concatenate([[0], np.cumsum(counts)])
            boxes[ci] = z[p + "boxes"][off[0]:off[1]]
            classes[ci] = (z[p + "classes"][off[0]:off[1]] % (C - 1)).astype(np.float32)
    loc = rng.standard_normal((bs, 8732, 4), dtype=np.float32)
    conf = rng.standard_normal((bs, 8732, C), dtype=np.float32) * np.float32(2.0)
    return boxes, classes, loc, conf


def _gpu_loss(loc, conf, boxes, classes):
    from objectdetection_ssd_amd import Losses
    lt, ct = _t(loc).requires_grad_(True), _t(conf).requires_grad_(True)
    l1, l2 = Losses.ssd((lt, ct), [_t(c) for c in classes], [_t(b) for b in boxes])
    (l1 + l2).backward()
    torch.cuda.synchronize()
    m = Losses.last_match
    return (l1.item(), l2.item(), m["obj"].cpu().numpy(), m["cls"].cpu().numpy(), lt.grad.cpu().numpy(), ct.grad.cpu().numpy())


@pytest.mark.parametrize("degenerate", [False, True])
@pytest.mark.parametrize("C", [2, 21, 65, 81, 256])
def test_loss_at_class_count_vs_restatement(gold_dir, C, degenerate):
    boxes, classes, loc, conf = _loss_case(C, degenerate, gold_dir)
    l1, l2, obj, cls, dloc, dconf = _gpu_loss(loc, conf, boxes, classes)
    ref = R.multibox_loss(loc, conf, boxes, classes)
    assert np.array_equal(cls, ref["cls"])
    assert np.array_equal(obj[ref["pos"]], ref["obj"][ref["pos"]])
    hn = (cls == C - 1) & (np.abs(dconf).max(-1) > 0)
    assert np.array_equal(hn, ref["hn"])                                        # the hard-negative set, bit-exact
    if degenerate:
        assert np.isinf(l1) and np.isinf(ref["loc_loss"])
        assert np.isfinite(dloc).all() and np.isfinite(dconf).all()
    else:
        assert abs(l1 - ref["loc_loss"]) <= 1e-4 * max(1.0, abs(ref["loc_loss"]))
    assert abs(l2 - ref["conf_loss"]) <= 1e-4 * max(1.0, abs(ref["conf_loss"]))
    assert np.abs(dloc - ref["dloc"]).max() <= 1e-5 * np.abs(ref["dloc"]).max()
    assert np.abs(dconf - ref["dconf"]).max() <= 1e-5 * np.abs(ref["dconf"]).max()
    again = _gpu_loss(loc, conf, boxes, classes)                                 # bitwise reproducible
    assert again[0] == l1 or (np.isinf(l1) and np.isinf(again[0]))
    assert again[1] == l2
    for a, b in zip(again[2:], (obj, cls, dloc, dconf)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("C", [81, 256])
def test_wide_loss_ignores_out_of_range_labels_without_faulting(C):
    """labels outside 0 .. C-2 are the caller's error: unspecified values, but the kernels stay inside their tensors"""
    from objectdetection_ssd_amd import Losses
    rng = np.random.default_rng(C)
    boxes, classes = _gt(rng, 2, C)
    classes[0][0], classes[1][0] = np.float32(1e6), np.float32(-7)
    loc = _t(rng.standard_normal((2, 8732, 4), dtype=np.float32))
    conf = _t(rng.standard_normal((2, 8732, C), dtype=np.float32))
    l1, l2 = Losses.ssd((loc, conf), [_t(c) for c in classes], [_t(b) for b in boxes])
    torch.cuda.synchronize()
    assert np.isfinite(l2.item())


def _nms_inputs(C, B, seed):
    rng = np.random.default_rng(seed)
    l = rng.standard_normal((B, 8732, 4), dtype=np.float32) * np.float32(0.5)
    scale = np.float32(3.0)          # wide rows: ~10 000 candidates per image, the best ones near 0.995 -- not saturated at 1
    c = rng.standard_normal((B, 8732, C), dtype=np.float32) * scale
    return l, c


def _same_detections(gi, gc, gp, ri, rc, rp, what):
    """The kept (class, prior id) set bit-exact; the emitted order too, except that two detections whose probabilities lie within
    1e-6 of each other may trade places in the cross-class top-k sort: the device and torch's CPU softmax sum the C exponentials in
    different orders (measured up to 6 ulps apart at C = 160), which decides the order of such near-ties."""
    assert sorted(zip(gc.tolist(), gi.tolist())) == sorted(zip(rc.tolist(), ri.tolist())), what
    for i in np.nonzero((gi != ri) | (gc != rc))[0]:
        assert abs(float(gp[i]) - float(rp[i])) <= 1e-6 * float(rp[i]), (what, i, gp[i], rp[i])


@pytest.mark.parametrize("B", [1, 32])
@pytest.mark.parametrize("C", [2, 81, 160, 256])
def test_decode_nms_at_class_count_keep_sets_bit_exact(C, B):
    from objectdetection_ssd_amd import Losses
    l, c = _nms_inputs(C, B, 7 * C + B)
    if B == 1:
        out = Losses.inference(_t(l[0]), _t(c[0]), (300, 300), toDraw=False)
        got = [(out, Losses.inference.last_prior_ids)]
    else:
        res = Losses.inference_batch(_t(l), _t(c), [(300, 300)] * B)
        got = list(zip(res, Losses.inference_batch.last_prior_ids))
    n_det = 0
    for b, (o, ids) in enumerate(got):
        rb, rc, rp, ri = R.decode_nms(l[b], c[b], 300, 300)
        if rb.shape[0] == 0:
            assert o == ([], [], [])
            continue
        n_det += rb.shape[0]
        gi, gc, gp = ids.cpu().numpy(), o[1].cpu().numpy(), o[2].cpu().numpy()
        _same_detections(gi, gc, gp, ri, rc, rp, b)
        np.testing.assert_allclose(np.sort(gp), np.sort(rp), rtol=1e-5)
    assert n_det > 0


@pytest.mark.parametrize("C", [2, 81, 256])
def test_decode_nms_all_candidates_at_class_count(C):
    """every prior a candidate of one class (the worst case of the candidate lists): the restatement's keep set, in every image of a
    batch too"""
    from objectdetection_ssd_amd import Losses
    l_ = torch.zeros(8732, 4, device=DEV)
    c_ = torch.full((8732, C), -10.0, device=DEV)
    col = min(3, C - 2)
    c_[:, col] = 10.0
    boxes, classes, probs = Losses.inference(l_, c_, (300, 300), toDraw=False)
    ob, oc, op_, oi = R.decode_nms(l_.cpu().numpy(), c_.cpu().numpy(), 300, 300)
    assert np.array_equal(Losses.inference.last_prior_ids.cpu().numpy(), oi)
    assert np.array_equal(classes.cpu().numpy(), oc) and set(oc.tolist()) == {col}
    got = Losses.inference_batch(l_[None].repeat(32, 1, 1), c_[None].repeat(32, 1, 1), [(300, 300)] * 32)
    for i, ids in enumerate(Losses.inference_batch.last_prior_ids):
        assert np.array_equal(ids.cpu().numpy(), oi) and np.array_equal(got[i][1].cpu().numpy(), oc)


def test_draw_hook_gets_integer_ids_beyond_voc():
    from objectdetection_ssd_amd import Losses
    seen = []
    old = Losses.draw_hook
    Losses.draw_hook = lambda idx, boxes, labels, probs: seen.append(labels)
    try:
        for C in (21, 81):
            l_ = torch.zeros(8732, 4, device=DEV)
            c_ = torch.full((8732, C), -10.0, device=DEV)
            c_[:, 3] = 10.0
            Losses.inference(l_, c_, (300, 300), toDraw=True)
    finally:
        Losses.draw_hook = old
    assert len(seen) == 2 and set(seen[0]) == {"boat"} and set(seen[1]) == {3}


def test_get_map_with_80_classes_bit_exact():
    from objectdetection_ssd_amd import Util
    rng = np.random.default_rng(80)
    det_b, det_c, det_s, gt_b, gt_c = [], [], [], [], []
    for _ in range(12):
        ng = int(rng.integers(1, 12))
        g = rng.uniform(0, 200, (ng, 2)).astype(np.float32)
        gb = np.concatenate([g, g + rng.uniform(20, 100, (ng, 2)).astype(np.float32)], 1)
        gc = rng.integers(0, 80, ng)
        nd = int(rng.integers(0, 40))
        pick = rng.integers(0, ng, nd)
        db = (gb[pick] + rng.normal(0, 8, (nd, 4))).astype(np.float32)
        dc = np.where(rng.uniform(size=nd) < 0.8, gc[pick], rng.integers(0, 80, nd))
        det_b.append(db); det_c.append(dc); det_s.append(rng.uniform(0, 1, nd).astype(np.float32))
        gt_b.append(gb); gt_c.append(gc)
    ref = R.get_map(det_b, det_c, det_s, gt_b, gt_c, n_classes=80)
    got = Util.get_map([_t(b) for b in det_b], [torch.from_numpy(c) for c in det_c], [_t(s) for s in det_s],
                       [_t(b) for b in gt_b], [torch.from_numpy(c) for c in gt_c], n_classes=80)
    assert sorted(got) == list(range(80))
    assert all(got[k] == ref[k] for k in range(80)), [(k, got[k], ref[k]) for k in range(80) if got[k] != ref[k]]
    assert sum(v > 0 for v in ref.values()) > 20


# ---- the network at 81 columns ---------------------------------------------------------------------------------------------------
def _net(n_classes, params, variant=300):
    from objectdetection_ssd_amd import Model
    net = (Model.SSD_300 if variant == 300 else Model.SSD_512)(n_classes=n_classes)
    named = dict(net.named_parameters())
    with torch.no_grad():
        for k, v in params.items():
            named[k].copy_(v)
    return net.to(DEV)


@pytest.fixture(scope="module")
def net81():
    params = R.random_params(81, seed=3)
    return _net(80, params), params


@pytest.mark.parametrize("conv_dtype", ["f32", "f32x3", "bf16"])
@pytest.mark.parametrize("winograd", [True, False])
def test_ssd300_80_classes_forward_vs_restatement(net81, conv_dtype, winograd):
    import grad_measure as M
    net, params = net81
    x = np.random.default_rng(81).standard_normal((2, 3, 300, 300), dtype=np.float32)
    net.eval()
    net.conv_dtype, net.winograd = conv_dtype, winograd
    try:
        with torch.no_grad():
            loc, conf = net(_t(x))
    finally:
        net.conv_dtype, net.winograd = "f32", True
    assert loc.shape == (2, 8732, 4) and conf.shape == (2, 8732, 81)
    with torch.no_grad():
        lo, co = R.ssd_forward(torch.from_numpy(x), params, 81, operand_round="bf16" if conv_dtype == "bf16" else None,
                               store_round=conv_dtype == "bf16" and net._engine.bf16_tensors)
    e_loc = float((loc.cpu() - lo).abs().max()) / max(1.0, float(lo.abs().max()))
    e_conf = float((conf.cpu() - co).abs().max()) / max(1.0, float(co.abs().max()))
    if conv_dtype == "bf16":                     # the bars of test_bf16_conv_mode_config3
        table = M.load_bars()
        noise = table["bf16_mode_noise"]
        assert e_loc <= min(2 * table["bf16_oracle_out"]["loc"], 1.5 * noise["loc"]), e_loc
        assert e_conf <= min(2 * table["bf16_oracle_out"]["conf"], 1.5 * noise["conf"]), e_conf
    else:
        assert e_loc <= 1e-4 and e_conf <= 1e-4, (e_loc, e_conf)


def _decisions(net, x, classes, boxes):
    """grad_measure.gpu_decisions with the background at C - 1"""
    import grad_measure as M
    from objectdetection_ssd_amd import Losses, ops
    from objectdetection_ssd_amd.Model import _Elided
    net.train()
    eng = net._engine
    with torch.no_grad():
        loc, conf, saved = eng.forward(x, net._forward_params(), save=True)
    T, aux = saved["T"], saved["aux"]
    relu, pool = {}, {}
    for op in eng.ops:
        if op["op"] in ("conv", "conv_first") and op["y"] in eng.relu_out:
            relu[op["y"]] = M._relu_mask_of(eng, T, aux, op)
        elif op["op"] == "pool":
            gate = (T[op["y"]] > 0).permute(0, 3, 1, 2).cpu() if isinstance(T[op["x"]], _Elided) else None
            pool[op["y"]] = (aux[op["y"]].permute(0, 3, 1, 2).cpu(), gate)
    gt, cls_t, img_start = Losses._pack_targets(classes, boxes, loc.device)
    pri, pri_xyxy = Losses._priors_on(loc.device, loc.shape[1])
    out = ops.multibox_loss(loc.contiguous(), conf.contiguous(), gt, cls_t, img_start, pri, pri_xyxy, Losses.IOU_THRESHOLD,
                            Losses.NEG_POS_RATIO, 0, want_grads=True)
    torch.cuda.synchronize()
    neg = (out["cls"] == conf.shape[-1] - 1) & (out["dconf"].abs().amax(-1) > 0)
    return {"relu": relu, "pool": pool}, neg.cpu()


@pytest.mark.parametrize("engine", ["direct", "wino"])
def test_train_step_81_gradients_vs_decision_pinned_f64(net81, engine):
    """all 71 gradients within the fixed bar of test_train_step_gradients_vs_decision_pinned_f64_oracle"""
    import grad_measure as M
    net, params = net81
    x, boxes, classes = M.f64_case()
    classes = [(c * 4 + 3) % 80 for c in classes]                 # spread over the 80 classes
    xd, cl, bx = _t(x), [_t(c) for c in classes], [_t(b) for b in boxes]
    M.set_engine(net, engine)
    try:
        decisions, neg = _decisions(net, xd, cl, bx)
        _, _, l1, l2, grads = M.train_step(net, xd, cl, bx)
    finally:
        M.set_engine(net, "wino")
    P = {k: v.detach().clone().double().requires_grad_(True) for k, v in params.items()}
    loc, conf = R.ssd_forward(torch.from_numpy(x).double(), P, 81, decisions=decisions)
    a1, a2 = R.conf_ce_loss_torch(loc, conf, boxes, classes, neg)
    (a1 + a2).backward()
    assert abs(l1 - float(a1)) <= 1e-4 * max(1, float(a1)) and abs(l2 - float(a2)) <= 1e-4 * max(1, float(a2))
    assert len(grads) == 71
    rows = sorted(((M.rel_l2(grads[k], P[k].grad), k) for k in P), reverse=True)
    print(f"C = 81 decision-pinned f64 distance [{engine}]: worst " + ", ".join(f"{k} {v:.2e}" for v, k in rows[:6]))
    bad = [(k, v) for v, k in rows if v > M.PINNED_BAR[engine]]
    assert not bad, bad


def _sgd_groups(named):
    biases, others = [], []
    for n, p in named:
        (biases if n.endswith(".bias") else others).append(p)
    return biases, others


def test_flat_sgd_data_parallel_81_equals_torch_sgd():
    from objectdetection_ssd_amd import Losses
    from objectdetection_ssd_amd.ddp import FlatSGDDataParallel
    lr, bs = 1e-4, 2
    params = R.random_params(81, seed=6)
    x = _t(np.random.default_rng(41).standard_normal((bs, 3, 300, 300), dtype=np.float32))
    boxes, classes = _gt(np.random.default_rng(42), bs, 81)
    cl, bx = [_t(c) for c in classes], [_t(b) for b in boxes]
    a, b = _net(80, params).train(), _net(80, params).train()
    biases, others = _sgd_groups(a.named_parameters())
    opt = torch.optim.SGD([{"params": biases, "lr": 2 * lr}, {"params": others}], lr=lr, momentum=0.9, weight_decay=5e-4)
    dp = FlatSGDDataParallel(b, lr=lr, momentum=0.9, weight_decay=5e-4)
    for _ in range(2):
        opt.zero_grad()
        l1, l2 = Losses.ssd(a(x), cl, bx)
        (l1 + l2).backward()
        opt.step()
        dp.zero_grad()
        m1, m2, n_pos = Losses.ssd(b(x), cl, bx, norm_mode=1, with_n_pos=True)
        (m1 + m2).backward()
        dp.reduce_and_step(n_pos)
    na, nb = dict(a.named_parameters()), dict(b.named_parameters())
    for k in a._engine.names:
        ref = na[k].detach()
        err = float((nb[k].detach() - ref).abs().max())
        assert err <= 2e-5 * max(1.0, float(ref.abs().max())), (k, err)


@pytest.mark.parametrize("conv_dtype", ["f32", "bf16"])
def test_graphed_train_step_81_is_bitwise_the_eager_step(conv_dtype):
    from objectdetection_ssd_amd import Losses
    from objectdetection_ssd_amd.ddp import FlatSGDDataParallel, GraphedTrainStep
    lr, bs = 1e-3, 2
    params = R.random_params(81, seed=8)
    nets, trs = [], []
    for _ in range(2):
        n = _net(80, params).train()
        n.conv_dtype = conv_dtype
        nets.append(n)
        trs.append(FlatSGDDataParallel(n, lr=lr, momentum=0.9, weight_decay=5e-4))
    gstep = GraphedTrainStep(nets[1], trs[1], max_boxes_per_image=8, warmup=2)
    for it in range(3):
        x = _t(np.random.default_rng(100 + it).standard_normal((bs, 3, 300, 300), dtype=np.float32))
        boxes, classes = _gt(np.random.default_rng(200 + it), bs, 81)
        cl, bx = [_t(c) for c in classes], [_t(b) for b in boxes]
        trs[0].zero_grad()
        l1, l2, n_pos = Losses.ssd(nets[0](x), cl, bx, norm_mode=1, with_n_pos=True)
        (l1 + l2).backward()
        trs[0].reduce_and_step(n_pos)
        g1, g2, gn = gstep(x, cl, bx)
        torch.cuda.synchronize()
        assert float(g1) == float(l1) and float(g2) == float(l2) and float(gn) == float(n_pos), it
        assert torch.equal(trs[0].flat_param, trs[1].flat_param), f"weights differ after step {it}"
        assert torch.equal(trs[0].flat_mom, trs[1].flat_mom), it


def test_graphed_inference_81_replays_the_eager_forward(net81):
    net, _ = net81
    net.eval()
    x = _t(np.random.default_rng(9).standard_normal((2, 3, 300, 300), dtype=np.float32))
    with torch.no_grad():
        loc, conf = net(x)
    g = net.graphed_forward(x)
    gl, gc = g(x)
    torch.cuda.synchronize()
    assert torch.equal(gl, loc) and torch.equal(gc, conf) and gc.shape[-1] == 81


def test_ssd512_81_train_step_runs_finite():
    from objectdetection_ssd_amd import Losses
    params = R.random_params(81, seed=12, variant=512)
    net = _net(80, params, variant=512).train()
    x = _t(np.random.default_rng(12).standard_normal((2, 3, 512, 512), dtype=np.float32))
    boxes, classes = _gt(np.random.default_rng(13), 2, 81)
    loc, conf = net(x)
    assert loc.shape == (2, 24564, 4) and conf.shape == (2, 24564, 81)
    l1, l2 = Losses.ssd((loc, conf), [_t(c) for c in classes], [_t(b) for b in boxes])
    (l1 + l2).backward()
    torch.cuda.synchronize()
    assert np.isfinite(l1.item()) and np.isfinite(l2.item())
    for k, p in net.named_parameters():
        if k in net._engine.names:
            assert p.grad is not None and torch.isfinite(p.grad).all(), k

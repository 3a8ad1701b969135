"""The decision-pinned f64 oracle (tests/grad_measure.py) at the shapes bench.py times.  The batch-2 checks in test_gpu_path.py do not
reach what depends on the grid size: the three-limb 1x1 GEMMs of fc7 / seq8.0 (from `_Engine.X31_MIN_PIXELS` output pixels), the
split-K and K-slice counts picked from the resident workgroups, the bf16 tile and split rules, SSD512's Winograd c_9 head, its
512 x 512 conv1_x layers and stride-2 aux blocks.  Each test runs the engine with its default flags, follows the HIP step's own
decisions (and, in the bf16-tensor mode, its stored values) in an f64 evaluation of the oracle on the host -- in chunks of images,
each normalised by the whole batch's positive count -- and holds every gradient to the same fixed bars as the batch-2 tests."""
import os
import resource
import time

import numpy as np
import pytest
import torch

import grad_measure as M
import ssd_oracle as O

pytestmark = pytest.mark.gpu
DEV = M.DEV


def _net(variant):
    from objectdetection_ssd_amd import Model
    if variant == 300:
        z = np.load(os.path.join(M.ROOT, "tests", "golden", "network.npz"))
        params, net = O.ssd300_random_params(int(z["param_seed"])), Model.SSD_300()
    else:
        params, net = O.ssd300_random_params(8, variant=512), Model.SSD_512()
    named = dict(net.named_parameters())
    with torch.no_grad():
        for k, v in params.items():
            named[k].copy_(v)
    return net.to(DEV), params


def _timing(label, x, t0):
    print(f"{label}: f64 evaluation of {x.shape[0]} images {time.time() - t0:.1f} s on {torch.get_num_threads()} threads, "
          f"peak RSS of the process {resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20:.2f} GB")


def _same_forward(decisions, loc, conf):
    """the forward that exported the decisions made the choices of the step whose gradients are compared: bitwise the same outputs"""
    assert torch.equal(decisions["out"][0], loc) and torch.equal(decisions["out"][1], conf)


def _check_outputs(out, loc, conf, l1, l2, a1, a2):
    lo, co = out["loc"], out["conf"]
    assert float((loc.cpu().double() - lo).abs().max()) <= 1e-4 * max(1.0, float(lo.abs().max()))
    assert float((conf.cpu().double() - co).abs().max()) <= 1e-4 * max(1.0, float(co.abs().max()))
    assert abs(l1 - a1) <= 1e-4 * max(1, a1) and abs(l2 - a2) <= 1e-4 * max(1, a2), (l1, a1, l2, a2)


def _check_grads(label, grads, g64, bar, n):
    assert len(g64) == n and set(g64) == set(grads)
    rows = sorted(((M.rel_l2(grads[k], g64[k]), k) for k in g64), reverse=True)
    print(f"{label}: worst " + ", ".join(f"{k} {v:.2e}" for v, k in rows[:6]) + f"; median {rows[len(rows) // 2][0]:.2e}")
    bad = [(k, v) for v, k in rows if v > bar]
    assert not bad, bad


def _check_report(pinned):
    rep = pinned["report"]
    assert len(rep) >= 2 * len(pinned["fwd"]) - 2, sorted(rep)
    worst = sorted(((v, k) for k, v in rep.items()), reverse=True)
    print("rounding-pinned layer distances (spacings): " + ", ".join(f"{k} {v:.3f}" for v, k in worst[:8]))
    assert "a4_3:1" in pinned["bwd"] and "a4_3:1:bwd" in rep
    bad = [(k, v) for k, v in rep.items() if v > (0.51 if k.split(":")[0] in pinned["bf16"] else 1.0)]
    assert not bad, bad


def _f32_pinned(variant, x, cl, bx, conv_dtype, want_kinds, bar, label):
    net, params = _net(variant)
    net.conv_dtype = conv_dtype
    decisions, neg = M.gpu_decisions(net, x, cl, bx)
    kinds = M.weight_kinds(net) if net._engine.uses_weight_table() else {}
    for layer, kind in want_kinds.items():
        assert kinds.get(layer) == kind, (layer, kinds.get(layer))
    loc, conf, l1, l2, grads = M.train_step(net, x, cl, bx)
    _same_forward(decisions, loc, conf)
    out, t0 = {}, time.time()
    a1, a2, g64 = M.f64_pinned_grads(params, decisions, neg, case=(x, bx, cl), variant=variant, outputs=out)
    _timing(label, x, t0)
    _check_outputs(out, loc, conf, l1, l2, a1, a2)
    _check_grads(label, grads, g64, bar, 71 if variant == 300 else 79)


def _bf16_pinned(variant, x, cl, bx, label):
    net, params = _net(variant)
    assert net._engine.bf16_tensors
    decisions, neg, pinned, (l1, l2), grads = M.gpu_pinned_step(net, x, cl, bx, "bf16")
    # the heads whose bias gradient the oracle sums from a bf16 dy are those the engine ran on the bf16-tensor kernels
    assert M.bf16_tensor_heads(net) == set(O.BF16_TENSOR_HEADS)
    M.set_engine(net, "wino", "bf16")
    try:
        loc, conf, _, _, step_grads = M.train_step(net, x, cl, bx)
    finally:
        M.set_engine(net, "wino", "f32")
    _same_forward(decisions, loc, conf)
    # ... and the gradients compared below are bitwise those of the step as bench.py runs it (the autograd path, no gradient tap)
    assert set(step_grads) == set(grads)
    assert all(torch.equal(step_grads[k].cpu(), grads[k]) for k in grads), [k for k in grads if not torch.equal(step_grads[k].cpu(), grads[k])]
    assert {"a1_1", "a1_2", "p1", "a4_3", "n4_3", "p5"} <= pinned["bf16"] and "a6" in pinned["fwd"] and "a6" not in pinned["bf16"]
    out, t0 = {}, time.time()
    a1, a2, g64 = M.f64_rounding_pinned_grads(params, decisions, neg, pinned, case=(x, bx, cl), variant=variant, outputs=out)
    _timing(label, x, t0)
    _check_report(pinned)
    # bf16 operands: loc / conf of the step against the oracle that followed its stored values
    _check_outputs(out, loc, conf, l1, l2, a1, a2)
    _check_grads(label, grads, g64, M.BF16_PINNED_BAR, 71 if variant == 300 else 79)


def test_ssd300_f32_step_at_bench_batch_vs_decision_pinned_f64():
    """bench.py's headline step (SSD300, f32, default engine) on its batch of 32: fc7 and seq8.0 on the three-limb 1x1 GEMMs, which the
    batch-2 test never reaches; all 71 gradients within PINNED_BAR["wino"]"""
    x, cl, bx = M.bench_batch()
    _f32_pinned(300, x, cl, bx, "f32", {"conv_fc7": "x31", "seq8.0": "x31"}, M.PINNED_BAR["wino"],
                "decision-pinned f64 distance [SSD300 f32, batch 32]")


def test_ssd300_bf16_step_at_bench_batch_vs_rounding_pinned_f64():
    """`--conv-dtype bf16` on bench.py's batch of 32, decision- and rounding-pinned: every layer within half a bf16 spacing of what the
    kernel stored (one spacing on f32 tensors), all 71 gradients within BF16_PINNED_BAR"""
    x, cl, bx = M.bench_batch()
    _bf16_pinned(300, x, cl, bx, "rounding-pinned bf16 gradient distance [SSD300, batch 32]")


def test_ssd512_f32_step_at_its_batch_vs_decision_pinned_f64():
    """`--variant 512 --batch 16`: the c_9 head (8x8) on Winograd, fc7 / seq8.0 on the three-limb GEMMs; all 79 gradients within
    PINNED_BAR["wino"]"""
    x, cl, bx = M.bench_batch(16, hw=512)
    _f32_pinned(512, x, cl, bx, "f32", {"c_9": "wino", "conv_fc7": "x31", "seq8.0": "x31"}, M.PINNED_BAR["wino"],
                "decision-pinned f64 distance [SSD512 f32, batch 16]")


def test_ssd512_bf16_step_vs_rounding_pinned_f64():
    """`--variant 512 --conv-dtype bf16` (no other test runs this mode), batch 2, decision- and rounding-pinned: the bars of the SSD300
    bf16 test"""
    x, cl, bx = M.bench_batch(2, hw=512)
    _bf16_pinned(512, x, cl, bx, "rounding-pinned bf16 gradient distance [SSD512, batch 2]")



def test_f32x3_step_vs_decision_pinned_f64():
    """`--conv-dtype f32x3` (three bf16 limbs per operand) on the f64 case, decision-pinned: all 71 gradients within PINNED_BAR["direct"],
    the bar of the exact-f32 direct engine -- each limb kernel is within 2x of the f32 MFMA kernel at kernel level, and the sign dither
    keeps the bf16 MFMA's truncation from adding up along the data-gradient chain (test_limb_conv_errors_carry_no_signed_bias)"""
    x, boxes, classes = M.f64_case()
    _f32_pinned(300, M._t(x), [M._t(c) for c in classes], [M._t(b) for b in boxes], "f32x3", {}, M.PINNED_BAR["direct"],
                "decision-pinned f64 distance [f32x3, batch 2]")

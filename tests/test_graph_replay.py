"""The two HIP-graph paths -- `ddp.GraphedTrainStep` and `Model.GraphedForward` -- replayed under the conditions a training loop
creates: eager calls on the same net between replays (other batch sizes, a weight table rebuilt by a flipped flag, a changed
parameter), schedule flags flipped between steps, and momentum 0.

A graph records raw device pointers.  Every lifetime test here takes weak references to what the graph could have baked in and
asserts that all of it is still alive BEFORE the next replay, so a lost buffer fails an assertion and is never replayed into.
Nothing here calls `torch.cuda.empty_cache()`.
"""
import gc
import weakref

import numpy as np
import pytest
import torch

import ssd_oracle as O
from helpers import synth_gt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BS = 2            # the captured batch
BIG = 4           # the eager calls in between: doubles the tail's split-K / weight-gradient workspaces (> the 1 MB floor)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _load_params(net, params):
    named = dict(net.named_parameters())
    with torch.no_grad():
        for k, v in params.items():
            named[k].copy_(v)


def _batch(seed, bs=BS):
    x = _t(np.random.default_rng(100 + seed).standard_normal((bs, 3, 300, 300), dtype=np.float32))
    boxes, classes = synth_gt(np.random.default_rng(200 + seed), bs)
    return x, [_t(c) for c in classes], [_t(b) for b in boxes]


def _pair(conv_dtype="f32", momentum=0.9, weight_decay=5e-4, two_streams=True):
    """Two nets with the same weights, each with its data-parallel optimizer: net 0 steps eagerly, net 1 through the graph."""
    from objectdetection_ssd_amd import Model
    from objectdetection_ssd_amd.ddp import FlatSGDDataParallel, GraphedTrainStep
    params = O.ssd300_random_params(8)
    nets, trs = [], []
    for _ in range(2):
        n = Model.SSD_300()
        _load_params(n, params)
        n = n.to(DEV).train()
        n.conv_dtype = conv_dtype
        nets.append(n)
        trs.append(FlatSGDDataParallel(n, lr=1e-4, momentum=momentum, weight_decay=weight_decay))   # 1e-3 diverges by step 7
    gstep = GraphedTrainStep(nets[1], trs[1], max_boxes_per_image=8, warmup=2, two_streams=two_streams)
    return nets, trs, gstep


def _lockstep(nets, trs, gstep, seed):
    """One eager step of the twin, then one step of the graph on the same batch -- no synchronisation before the graph's step --
    and the two must agree bit for bit: loss sums, positive count, weights, momentum."""
    from objectdetection_ssd_amd import Losses
    x, cl, bx = _batch(seed)
    trs[0].zero_grad()
    l1, l2, n_pos = Losses.ssd(nets[0](x), cl, bx, norm_mode=1, with_n_pos=True)
    (l1 + l2).backward()
    trs[0].reduce_and_step(n_pos)
    g1, g2, gn = gstep(x, cl, bx)
    torch.cuda.synchronize()
    assert np.isfinite(float(l1)) and np.isfinite(float(l2)), f"the eager step diverged at step {seed}"
    assert float(g1) == float(l1) and float(g2) == float(l2) and float(gn) == float(n_pos), (seed, float(g1), float(l1))
    assert torch.equal(trs[0].flat_param, trs[1].flat_param), f"weights differ after step {seed}"
    assert torch.equal(trs[0].flat_mom, trs[1].flat_mom), f"momentum differs after step {seed}"
    assert trs[0].steps == trs[1].steps


def _train_fwd_bwd(net, tr, seed, bs):
    """An eager forward + backward on the net (gradients land in the trainer's flat buffer), no SGD step."""
    from objectdetection_ssd_amd import Losses
    x, cl, bx = _batch(seed, bs)
    tr.zero_grad()
    l1, l2, _ = Losses.ssd(net(x), cl, bx, norm_mode=1, with_n_pos=True)
    (l1 + l2).backward()
    tr.zero_grad()


def _ws_refs(streams):
    """Weak references to the workspaces cached for these streams: key -> weakref."""
    from objectdetection_ssd_amd import ops
    keys = {s.cuda_stream for s in streams if s is not None}
    return {k: weakref.ref(buf) for k, buf in ops._ws_cache.items() if k[1] in keys}


def _replaced(refs):
    """Keys whose cached workspace is no longer the one referenced (regrown since, or gone)."""
    from objectdetection_ssd_amd import ops
    return [k for k, r in refs.items() if ops._ws_cache.get(k) is not r()]


@pytest.mark.parametrize("conv_dtype,two_streams", [("f32", True), ("f32", False), ("bf16", True)])
def test_graphed_train_step_survives_eager_work_on_its_own_net(conv_dtype, two_streams):
    """Between replays, net 1 runs an eval forward at twice the captured batch, a training forward under a flipped weight-table
    flag (flipped back before the replay, so the graph is NOT re-captured), and a training forward + backward at twice the batch.
    Those regrow the side stream's workspaces and replace the engine's weight table; the graph must still own the ones it baked
    in, and the following replays must stay bitwise equal to the eager twin."""
    nets, trs, gstep = _pair(conv_dtype, two_streams=two_streams)
    eng = nets[1]._engine
    for it in range(gstep.warmup + 2):                         # warm-up, capture + replay, one more replay
        _lockstep(nets, trs, gstep, it)
    graph = gstep.graph
    assert graph is not None
    # everything the graph could have baked in: its stream's workspaces (and, with two streams, the tail's), the weight table
    streams = [gstep._stream] + ([eng._side_stream, eng._wgrad_stream] if two_streams else [])
    ws = _ws_refs(streams)
    assert ws, "no workspace cached for the capture's streams"
    table = weakref.ref(eng._wcache.fill.table)
    kept = [weakref.ref(t) for t in eng._wcache.fill.table.keep]

    with torch.no_grad():                                      # 1: eval forward at the larger batch
        nets[1](_batch(50, BIG)[0])
    eng.adjoint_dgrad = not eng.adjoint_dgrad                  # 2: a training forward under another weight-table key
    loc, conf = nets[1](_batch(51)[0])
    del loc, conf
    eng.adjoint_dgrad = not eng.adjoint_dgrad
    for net, tr in zip(nets, trs):                             # 3: forward + backward at the larger batch, on both nets
        _train_fwd_bwd(net, tr, 52, BIG)

    if two_streams:
        assert _replaced(ws), "no side-stream workspace was regrown: the test no longer exercises the hazard"
    assert eng._wcache.fill.table is not table(), "the weight table was not replaced: the test no longer exercises the hazard"
    gc.collect()
    dead = [k for k, r in ws.items() if r() is None]
    assert not dead, f"workspaces the graph replays with were freed: {dead}"
    assert table() is not None, "the weight table the graph replays with was freed"
    assert all(r() is not None for r in kept), "buffers of the captured weight table were freed"

    for it in range(3):
        _lockstep(nets, trs, gstep, 10 + it)
    assert gstep.graph is graph, "the graph was captured again: the replays above did not test the captured buffers"


def test_graphed_forward_survives_eager_work_and_returns_the_weights_at_capture():
    """GraphedForward replays from the workspaces of its capture and from weights of its own (a copy of the parameters and its
    layouts, which no eager call can reach).  Eager calls at another batch, an invalidated cache, changed parameters and a second
    capture at another batch must neither free the workspaces nor change what the first graph returns: the outputs of the weights
    at capture, bit for bit.  The capture leaves the engine's weight cache as it found it.  A fresh capture follows the new weights."""
    from objectdetection_ssd_amd import Model
    net = Model.SSD_300()
    _load_params(net, O.ssd300_random_params(8))
    net = net.to(DEV).eval()
    eng = net._engine
    x2, x4 = _batch(60)[0], _batch(61, BIG)[0]
    with torch.no_grad():
        ref0 = tuple(t.clone() for t in net(x2))
    before = dict(eng._wcache)
    gf = net.graphed_forward(x2)
    assert eng._wcache.keys() == before.keys() and all(eng._wcache[k] is v for k, v in before.items()), \
        "the capture changed the engine's weight cache"
    # taken the moment the capture is done: the workspaces of the streams the capture ran on -- its own (torch's shared capture
    # stream for a GraphedForward without one) and the side stream of the tail group.  (Not every stream's: torch hands out
    # pooled streams, so other streams may carry other tests' buffers.)
    cap = getattr(gf, "_stream", None) or torch.cuda.graphs.graph.default_capture_stream
    ws = _ws_refs([cap, eng._side_stream])
    assert ws
    a, b = gf(x2)
    assert torch.equal(a, ref0[0]) and torch.equal(b, ref0[1])

    with torch.no_grad():
        net(x4)
        net.invalidate_weight_cache()
        net(x4)
        for p in net._forward_params().values():            # through .data: invisible to the cache key, hence the invalidation
            p.data.mul_(0.97)
        net.invalidate_weight_cache()
    gf4 = net.graphed_forward(x4)

    assert _replaced(ws), "no workspace of the first capture was regrown: the test no longer exercises the hazard"
    gc.collect()
    dead = [k for k, r in ws.items() if r() is None]
    assert not dead, f"workspaces the first graph replays with were freed: {dead}"

    a, b = gf(x2)
    assert torch.equal(a, ref0[0]) and torch.equal(b, ref0[1]), "the replay did not return the outputs of the weights at capture"
    with torch.no_grad():
        ref1 = tuple(t.clone() for t in net(x2))
        ref4 = tuple(t.clone() for t in net(x4))
    assert not torch.equal(ref1[1], ref0[1])
    gf2 = net.graphed_forward(x2)
    a, b = gf2(x2)
    assert torch.equal(a, ref1[0]) and torch.equal(b, ref1[1])
    a, b = gf4(x4)
    assert torch.equal(a, ref4[0]) and torch.equal(b, ref4[1])


def test_graphed_forward_captured_again_after_an_in_place_update_follows_it():
    """A graph dropped, the parameters updated in place under no_grad (`p.copy_()`: an update the weight cache's key sees), and the
    forward captured again at the same shape: the new graph must compute the new weights, bit for bit the eager forward -- not
    filters laid out for the first capture's parameter copy, whose memory the second copy may reuse."""
    from objectdetection_ssd_amd import Model
    net = Model.SSD_300()
    _load_params(net, O.ssd300_random_params(8))
    net = net.to(DEV).eval()
    x = _batch(70)[0]
    gf = net.graphed_forward(x)
    conf0 = gf(x)[1].clone()
    del gf
    gc.collect()
    with torch.no_grad():
        for p in net._forward_params().values():
            p.copy_(p * 0.97)
    gf = net.graphed_forward(x)
    a, b = gf(x)
    with torch.no_grad():
        ref = net(x)
    assert not torch.equal(ref[1], conf0)
    assert torch.equal(a, ref[0]) and torch.equal(b, ref[1]), "the second capture did not compute the updated weights"


def test_graphed_train_step_recaptures_when_a_schedule_flag_flips():
    """`adjoint_dgrad` and `lazy_pool_grad` change which kernels the step runs.  Flipping them on both nets must re-capture the graph
    (not replay the old schedule), and the step must stay bitwise equal to the eager twin -- and again when they are flipped back."""
    nets, trs, gstep = _pair()
    for it in range(gstep.warmup + 2):
        _lockstep(nets, trs, gstep, it)
    for flip in (1, 2):
        old = gstep.graph
        for net in nets:
            net._engine.adjoint_dgrad = not net._engine.adjoint_dgrad
            net._engine.lazy_pool_grad = not net._engine.lazy_pool_grad
        _lockstep(nets, trs, gstep, 20 + flip)
        assert gstep.graph is not None and gstep.graph is not old, f"flip {flip}: the old schedule was replayed"
        _lockstep(nets, trs, gstep, 30 + flip)
    assert nets[1]._engine.adjoint_dgrad and nets[1]._engine.lazy_pool_grad


@pytest.mark.parametrize("weight_decay", [0.0, 5e-4])
def test_graphed_train_step_is_captured_with_momentum_zero(weight_decay):
    """With momentum 0 no momentum buffer ever comes into being; the step must be captured after the warm-up all the same (not run
    eagerly for ever) and stay bitwise equal to the eager step."""
    nets, trs, gstep = _pair(momentum=0.0, weight_decay=weight_decay)
    for it in range(4):
        _lockstep(nets, trs, gstep, it)
        if gstep._calls >= gstep.warmup + 1:
            assert gstep.graph is not None, f"call {gstep._calls}: momentum 0 left the step eager"
    assert trs[1].steps == 4

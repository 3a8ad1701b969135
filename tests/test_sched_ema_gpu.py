"""Device-resident learning-rate schedule and weight EMA on the device: the three kernels through `ops`, `optim.SGD` against a twin
whose rates are set on the host, the guard, checkpoints, `ddp.FlatSGDDataParallel` under `ddp.GraphedTrainStep` on SSD_300 and
`ema_weights()`.

Everything is compared bit for bit: the rates are table lookups, the EMA weight is an f64 expression of IEEE operations rounded
once, the parameter / momentum arithmetic is the existing SGD kernel's and the EMA update is three separately rounded f32
operations that tests/sched_ema_ref.py restates in numpy."""
import copy

import numpy as np
import pytest
import torch

import sched_ema_ref as R
import ssd_oracle as O
from helpers import synth_gt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# The SGD kernel launches min(ceil(units / 256), 2048) workgroups of 256 threads, units = 16-byte groups of 4 floats in the vector
# form and floats in the scalar form: one pass of the full grid covers 2048 * 256 * 4 = 2,097,152 floats (vector) or 524,288
# (scalar).  The long lengths take every thread through the loop once and one more thread (vector) / five more (scalar) twice.
VEC_PASS = 2048 * 256 * 4
SCALAR_PASS = 2048 * 256
# (n, offset of the range inside its 16-byte aligned allocation): offset 4 keeps the 16-byte alignment, offset 1 leaves a range
# that is only 4-byte aligned and takes the scalar loop
RANGES = [(4, 4), (1028, 4), (4100, 4), (VEC_PASS + 4, 4), (1027, 1), (4100, 1), (SCALAR_PASS + 5, 1)]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---- ssd_sgd_schedule_advance ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warmup", [True, False])
def test_advance_follows_the_table_clamps_past_its_end_and_holds_still_when_skipped(warmup):
    from objectdetection_ssd_amd import ops
    G, T, steps, decay = 2, 20, 25, 0.999
    factors = R.cosine(T - 1, warmup_steps=3)
    assert len(factors) == T
    rows = np.stack([R.table_row(2e-3, factors), R.table_row(1e-3, factors)])
    table = _t(rows)
    state = torch.zeros(2 + G + 2, device=DEV, dtype=torch.int32)
    state[2 + G:] = 0x5A5A5A5A                                       # words behind the block: never written
    seen = []
    for _ in range(steps):
        ops.sgd_schedule_advance_(state, table, decay, warmup)
        seen.append(state.clone())
    skip = torch.ones(1, device=DEV, dtype=torch.int32)
    ops.sgd_schedule_advance_(state, table, decay, warmup, skip)
    held = state.clone()
    skip.zero_()
    ops.sgd_schedule_advance_(state, table, decay, warmup, skip)
    torch.cuda.synchronize()
    for t, st in enumerate(seen):
        f = st.view(torch.float32).cpu().numpy()
        assert int(st[0]) == t + 1
        assert f[2:2 + G].tobytes() == rows[:, min(t, T - 1)].tobytes(), t
        assert f[1:2].tobytes() == R.ema_w(t, decay, warmup).tobytes(), (t, f[1], R.ema_w(t, decay, warmup))
        assert st[2 + G:].tolist() == [0x5A5A5A5A] * 2
    assert torch.equal(held, seen[-1]), "a skipped advance wrote the block"
    assert int(state[0]) == steps + 1                                # skip word 0: the step is taken
    # no EMA: weight 0
    ops.sgd_schedule_advance_(state, table, None, warmup)
    assert float(state.view(torch.float32)[1]) == 0.0 and int(state[0]) == steps + 2


# ---- ssd_sgd_momentum_sched --------------------------------------------------------------------------------------------------------
MOM, WD, DECAY = 0.9, 5e-4, 0.9
_REF = {}


def _reference(n, off):
    """Inputs of one (n, offset) case and the twin's results after each of three steps, stepped by the existing `ops.sgd_momentum_`
    with the same f32 rates passed from the host -- computed once, shared, never written again."""
    from objectdetection_ssd_amd import ops
    key = (n, off)
    if key not in _REF:
        rng = np.random.default_rng(n * 7 + off)
        p0, e0 = rng.standard_normal(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32)
        grads = [rng.standard_normal(n, dtype=np.float32) for _ in range(3)]
        lrs = [np.float32(v) for v in (1e-2, 3.3e-3, 7.7e-4)]
        scale = torch.tensor([0.37], device=DEV)
        p, b = _t(p0), torch.zeros(n, device=DEV)
        after = []
        for k in range(3):
            ops.sgd_momentum_(p, _t(grads[k]), b, float(lrs[k]), MOM, WD, scale, k == 0)
            after.append((p.clone(), b.clone()))
        e, emas = e0, []
        for k in range(3):
            e = R.ema_update(e, after[k][0].cpu().numpy(), R.ema_w(k, DECAY))
            emas.append(e)
        _REF[key] = dict(p0=p0, e0=e0, grads=grads, lrs=lrs, scale=scale, after=after, emas=emas)
    return _REF[key]


def _framed(host, n, off):
    """The values inside a larger allocation with a recognisable frame around them -> (whole buffer, the range)."""
    whole = torch.full((off + n + 8,), -77.0, device=DEV)
    whole[off:off + n] = _t(host)
    return whole, whole[off:off + n]


def _frame_intact(whole, n, off):
    return bool((whole[:off] == -77.0).all()) and bool((whole[off + n:] == -77.0).all())


@pytest.mark.parametrize("n,off", RANGES, ids=[f"n{n}-off{o}" for n, o in RANGES])
def test_sgd_momentum_sched_is_bitwise_the_existing_kernel_and_the_restated_ema(n, off):
    from objectdetection_ssd_amd import ops
    ref = _reference(n, off)
    (Pw, p), (Bw, b), (Ew, e) = _framed(ref["p0"], n, off), _framed(np.zeros(n, np.float32), n, off), _framed(ref["e0"], n, off)
    assert p.data_ptr() % 16 == (0 if off % 4 == 0 else 4 * off % 16)
    lr, w = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    for k in range(3):
        Gw, g = _framed(ref["grads"][k], n, off)
        lr.fill_(float(ref["lrs"][k]))
        w.fill_(float(R.ema_w(k, DECAY)))
        ops.sgd_momentum_sched_(p, g, b, e, lr, w, MOM, WD, ref["scale"], k == 0, None)
        assert _same(p, ref["after"][k][0]), f"step {k}: parameters differ from the existing kernel's"
        assert _same(b, ref["after"][k][1]), f"step {k}: momentum differs from the existing kernel's"
        assert e.cpu().numpy().tobytes() == ref["emas"][k].tobytes(), f"step {k}: EMA differs from the restatement"
    assert all(_frame_intact(x, n, off) for x in (Pw, Bw, Ew, Gw)), "written outside the range"
    # skip set: nothing at all is written; ema = NULL: the EMA buffer is untouched and the step is still the existing kernel's
    keep = (Pw.clone(), Bw.clone(), Ew.clone())
    one = torch.ones(1, device=DEV, dtype=torch.int32)
    ops.sgd_momentum_sched_(p, g, b, e, lr, w, MOM, WD, ref["scale"], False, one)
    ops.sgd_momentum_sched_(p, g, b, None, lr, None, MOM, WD, ref["scale"], True, one)
    assert _same(Pw, keep[0]) and _same(Bw, keep[1]) and _same(Ew, keep[2]), "a skipped launch wrote"
    # ema = NULL: parameters and momentum live in ONE allocation, each directly followed by a copy of the EMA values that the launch is
    # not given -- [frame | p | e | b | e | frame] -- so a store that strays past either range, or an EMA update that runs all the same,
    # lands in them
    whole = torch.full((off + 4 * n + 8,), -77.0, device=DEV)
    p, e1, b, e2 = (whole[off + i * n:off + (i + 1) * n] for i in range(4))
    p.copy_(_t(ref["p0"])); b.zero_(); e1.copy_(_t(ref["e0"])); e2.copy_(_t(ref["e0"]))
    zero = torch.zeros(1, device=DEV, dtype=torch.int32)
    for k in range(3):
        lr.fill_(float(ref["lrs"][k]))
        ops.sgd_momentum_sched_(p, _framed(ref["grads"][k], n, off)[1], b, None, lr, None, MOM, WD, ref["scale"], k == 0, zero if k else None)
    assert _same(p, ref["after"][2][0]) and _same(b, ref["after"][2][1])
    assert e1.cpu().numpy().tobytes() == ref["e0"].tobytes() and e2.cpu().numpy().tobytes() == ref["e0"].tobytes(), "ema = NULL wrote next door"
    assert _frame_intact(whole, 4 * n, off)


@pytest.mark.parametrize("n,off", [(4, 4), (4100, 4), (VEC_PASS + 4, 4), (1027, 1)])
def test_swap(n, off):
    from objectdetection_ssd_amd import ops
    rng = np.random.default_rng(n)
    a0, b0 = rng.standard_normal(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32)
    (Aw, a), (Bw, b) = _framed(a0, n, off), _framed(b0, n, off)
    ops.swap_f32_(a, b)
    assert a.cpu().numpy().tobytes() == b0.tobytes() and b.cpu().numpy().tobytes() == a0.tobytes()
    assert _frame_intact(Aw, n, off) and _frame_intact(Bw, n, off)
    with pytest.raises(RuntimeError):
        ops.swap_f32_(Aw[:8], Aw[4:12])                              # overlapping ranges are refused


# ---- optim.SGD ---------------------------------------------------------------------------------------------------------------------
class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Conv2d(3, 5, 3)          # 135 + 5 params: slots are padded to multiples of 4
        self.b = torch.nn.Conv2d(5, 7, 1)
        self.g = torch.nn.Parameter(torch.ones(1, 6, 1, 1))


LR = 1e-2
FACTORS = R.cosine(10, warmup_steps=3)             # warm-up 3 + cosine 10: the table ends at step 10, steps 11 and 12 hold its last entry


def _schedule():
    from objectdetection_ssd_amd.optim import LRSchedule
    return LRSchedule.cosine(10, warmup_steps=3)


def _tiny_opt(**kw):
    from objectdetection_ssd_amd.optim import SGD
    torch.manual_seed(4)
    net = _Tiny().to(DEV)
    named = list(net.named_parameters())
    biases = [p for n, p in named if n.endswith(".bias")]
    rest = [p for n, p in named if not n.endswith(".bias")]
    opt = SGD([{"params": biases, "lr": 2 * LR}, {"params": rest}], lr=LR, momentum=0.9, weight_decay=5e-4, **kw)
    return net, biases + rest, opt


def _tiny_grads(ps, step, poison=False):
    g = torch.Generator().manual_seed(900 + step)
    for i, p in enumerate(ps):
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
        if poison and i == 2:
            p.grad.view(-1)[3] = float("inf")


@pytest.mark.parametrize("guard", [False, True])
def test_scheduled_sgd_is_bitwise_a_twin_whose_rates_the_host_sets(guard):
    """12 steps of two groups (biases at 2x lr).  The twin has no schedule: its groups' lr are set before each step to the
    restatement's f32 values.  With the guard, step 4 carries one Inf gradient element: counter, rates and EMA hold still."""
    kw = dict(skip_nonfinite=True) if guard else {}
    _, pa, ref = _tiny_opt(**kw)
    _, pb, opt = _tiny_opt(schedule=_schedule(), ema_decay=0.9, **kw)
    assert FACTORS.tobytes() == opt.schedule.factors.tobytes()
    rows = [R.table_row(2 * LR, FACTORS), R.table_row(LR, FACTORS)]
    emas = [p.detach().cpu().numpy().copy() for p in pb]
    taken = 0
    for step in range(12):
        bad = guard and step == 4
        _tiny_grads(pa, step, bad)
        _tiny_grads(pb, step, bad)
        for g, row in zip(ref.param_groups, rows):
            g["lr"] = float(R.lr_at(row, taken))
        if bad:
            before = (opt._sched_state.clone(), [e.clone() for e in opt.ema_parameters()], [p.detach().clone() for p in pb])
        ref.step()
        opt.step()
        assert [g["lr"] for g in opt.param_groups] == [2 * LR, LR], "the groups' lr must stay the base rates"
        if bad:
            assert torch.equal(opt._sched_state, before[0]), "a skipped step advanced the counter, the rate or the EMA weight"
            assert all(_same(a, b) for a, b in zip(opt.ema_parameters(), before[1])), "a skipped step moved the EMA"
            assert all(_same(a, b) for a, b in zip(pb, before[2])) and int(opt.skipped_steps) == 1
            continue
        assert opt.current_lr.cpu().numpy().tobytes() == np.array([R.lr_at(r, taken) for r in rows], np.float32).tobytes(), step
        assert np.float32(opt.ema_weight.item()).tobytes() == R.ema_w(taken, 0.9).tobytes()
        taken += 1
        assert int(opt.step_count) == taken
        for i, (a, b) in enumerate(zip(pa, pb)):
            assert _same(a, b), (step, "parameter", i)
            assert _same(ref.state[a]["momentum_buffer"], opt.state[b]["momentum_buffer"]), (step, "momentum", i)
            emas[i] = R.ema_update(emas[i], b.detach().cpu().numpy(), R.ema_w(taken - 1, 0.9))
            assert opt.state[b]["ema"].cpu().numpy().tobytes() == emas[i].tobytes(), (step, "ema", i)
    assert taken == (11 if guard else 12) and (int(opt.skipped_steps) == 1 if guard else opt.skipped_steps is None)
    assert all(a.data_ptr() == opt.state[p]["ema"].data_ptr() for a, p in zip(opt.ema_parameters(), pb))


def test_ema_alone_steps_at_the_base_rates():
    """Only the EMA on: the table is the one column of base rates, parameters and momentum are those of the plain optimizer."""
    _, pa, ref = _tiny_opt()
    _, pb, opt = _tiny_opt(ema_decay=0.99, ema_warmup=False)
    # the average starts as a copy of the parameters AT THE FIRST STEP: asked for earlier, it is copied again then, because the
    # parameters may have been loaded in between (here: scaled)
    early = [e.clone() for e in opt.ema_parameters()]
    assert all(_same(e, p) for e, p in zip(early, pb))
    with torch.no_grad():
        for p in pa + pb:
            p.mul_(1.5)
    start = [p.detach().cpu().numpy().copy() for p in pb]
    for step in range(3):
        _tiny_grads(pa, step)
        _tiny_grads(pb, step)
        ref.step()
        opt.step()
        assert opt.current_lr.cpu().numpy().tobytes() == np.array([2 * LR, LR], np.float32).tobytes()
        assert np.float32(opt.ema_weight.item()).tobytes() == R.ema_w(step, 0.99, False).tobytes()
        assert all(_same(a, b) for a, b in zip(pa, pb))
        if step == 0:
            for i, (e, p) in enumerate(zip(opt.ema_parameters(), pb)):
                want = R.ema_update(start[i], p.detach().cpu().numpy(), R.ema_w(0, 0.99, False))
                assert e.cpu().numpy().tobytes() == want.tobytes(), ("the EMA did not start from the parameters of the first step", i)
    assert tuple(opt._sched_table.shape) == (2, 1) and ref.current_lr is None


def test_checkpoint_resumes_bitwise():
    """state_dict() at step 5 into a fresh optimizer over a copy of the parameters: three more steps equal the uninterrupted run in
    parameters, momentum, EMA and counter."""
    _, pa, oa = _tiny_opt(schedule=_schedule(), ema_decay=0.9)
    for step in range(5):
        _tiny_grads(pa, step)
        oa.step()
    sd = copy.deepcopy(oa.state_dict())                               # (as torch.save / torch.load would hand it over)
    assert [g["sched_step"] for g in sd["param_groups"]] == [5, 5] and all("ema" in s for s in sd["state"].values())
    _, pb, ob = _tiny_opt(schedule=_schedule(), ema_decay=0.9)
    with torch.no_grad():
        for a, b in zip(pa, pb):
            b.copy_(a)
    ob.load_state_dict(sd)
    for step in range(5, 8):
        _tiny_grads(pa, step)
        _tiny_grads(pb, step)
        oa.step()
        ob.step()
        assert int(ob.step_count) == int(oa.step_count) == step + 1
        assert _same(oa.current_lr, ob.current_lr)
        for i, (a, b) in enumerate(zip(pa, pb)):
            assert _same(a, b), (step, "parameter", i)
            assert _same(oa.state[a]["momentum_buffer"], ob.state[b]["momentum_buffer"]), (step, "momentum", i)
            assert _same(oa.state[a]["ema"], ob.state[b]["ema"]), (step, "ema", i)


# ---- FlatSGDDataParallel + GraphedTrainStep, SSD_300 ---------------------------------------------------------------------------------
BS = 2
_PARAMS = []
_STREAM_OWNERS = []           # engines and graph steps built here: each takes streams from torch's pool


@pytest.fixture(scope="module", autouse=True)
def _leave_streams_and_workspaces_as_found():
    """As tests/test_grad_clip_gpu.py does: the SSD_300 tests take streams from torch's pool (32 per device, round-robin) and grow
    the scratch buffers `ops.workspace` caches per stream handle; the lifetime tests of tests/test_graph_replay.py depend on both.
    This module hands back the workspace cache as it was and the pool at the position it had."""
    import gc
    from objectdetection_ssd_amd import ops
    before = dict(ops._ws_cache)
    yield
    torch.cuda.synchronize()
    taken = 0
    for o in _STREAM_OWNERS:
        taken += sum(getattr(o, a, None) is not None for a in ("_side_stream", "_wgrad_stream", "_stream"))
    del _STREAM_OWNERS[:]
    ops._ws_cache.clear()
    ops._ws_cache.update(before)
    gc.collect()
    for _ in range(-taken % 32):
        torch.cuda.Stream(device=DEV)


def _load_params(net, params):
    named = dict(net.named_parameters())
    with torch.no_grad():
        for k, v in params.items():
            named[k].copy_(v)


def _batch(seed, bs=BS):
    x = _t(np.random.default_rng(100 + seed).standard_normal((bs, 3, 300, 300), dtype=np.float32))
    boxes, classes = synth_gt(np.random.default_rng(200 + seed), bs)
    return x, [_t(c) for c in classes], [_t(b) for b in boxes]


def _trainer(**kw):
    from objectdetection_ssd_amd import Model
    from objectdetection_ssd_amd.ddp import FlatSGDDataParallel
    if not _PARAMS:
        _PARAMS.append(O.ssd300_random_params(8))
    net = Model.SSD_300()
    _load_params(net, _PARAMS[0])
    net = net.to(DEV).train()
    _STREAM_OWNERS.append(net._engine)
    return net, FlatSGDDataParallel(net, lr=1e-4, momentum=0.9, weight_decay=5e-4, **kw)     # 1e-3 diverges within a few steps


def test_graphed_step_under_a_per_step_schedule_is_captured_once():
    """SSD300, batch 2, warm-up 3 + cosine 8 with the EMA, 7 calls (two eager warm-up steps, the capture, four replays): the graph
    object never changes, and parameters, momentum, EMA, counter and rates are bitwise those of an eager twin with the same settings."""
    from objectdetection_ssd_amd import Losses
    from objectdetection_ssd_amd.ddp import GraphedTrainStep
    from objectdetection_ssd_amd.optim import LRSchedule
    factors = R.cosine(8, warmup_steps=3)
    rows = [R.table_row(2e-4, factors), R.table_row(1e-4, factors)]          # group 0 = biases at 2x lr
    (n0, t0), (n1, t1) = (_trainer(schedule=LRSchedule.cosine(8, warmup_steps=3), ema_decay=0.9) for _ in range(2))
    gstep = GraphedTrainStep(n1, t1, max_boxes_per_image=8, warmup=2)
    _STREAM_OWNERS.append(gstep)
    graph = None
    for call in range(7):
        x, cl, bx = _batch(call)
        t0.zero_grad()
        l1, l2, n_pos = Losses.ssd(n0(x), cl, bx, norm_mode=1, with_n_pos=True)
        (l1 + l2).backward()
        t0.reduce_and_step(n_pos)
        gstep(x, cl, bx)
        torch.cuda.synchronize()
        assert np.isfinite(float(l1.detach())) and np.isfinite(float(l2.detach())), f"the eager step diverged at call {call}"
        if call >= gstep.warmup:
            assert gstep.graph is not None
            graph = graph or gstep.graph
            assert gstep.graph is graph, f"call {call}: the step was captured again under the schedule"
        else:
            assert gstep.graph is None
        want = np.array([R.lr_at(r, call) for r in rows], np.float32)
        assert t1.current_lr.cpu().numpy().tobytes() == want.tobytes(), (call, t1.current_lr, want)
        assert np.float32(t1.ema_weight.item()).tobytes() == R.ema_w(call, 0.9).tobytes()
        assert int(t1.step_count) == int(t0.step_count) == call + 1 and t0.steps == t1.steps == call + 1
        assert torch.equal(t0._sched_state, t1._sched_state)
        assert _same(t0.flat_param, t1.flat_param), f"weights differ after call {call}"
        assert _same(t0.flat_mom, t1.flat_mom), f"momentum differs after call {call}"
        assert _same(t0.flat_ema, t1.flat_ema), f"EMA differs after call {call}"
    assert [g["lr"] for g in t1.param_groups] == [2e-4, 1e-4]
    assert not torch.equal(t1.flat_ema, t1.flat_param)
    print(f"kernel nodes of the captured step with schedule and EMA: {gstep.kernel_nodes}")


def test_ema_weights_swaps_in_place_and_invalidates_the_weight_cache():
    from objectdetection_ssd_amd import Losses, Model
    net, tr = _trainer(ema_decay=0.9, ema_warmup=False)
    for step in range(2):
        x, cl, bx = _batch(40 + step)
        tr.zero_grad()
        l1, l2, n_pos = Losses.ssd(net(x), cl, bx, norm_mode=1, with_n_pos=True)
        (l1 + l2).backward()
        tr.reduce_and_step(n_pos)
    assert not torch.equal(tr.flat_ema, tr.flat_param)
    x = _batch(50)[0]
    net.eval()
    par, ema = tr.flat_param.clone(), tr.flat_ema.clone()
    with torch.no_grad():
        before = tuple(t.clone() for t in net(x))
    # a second net whose parameters were loaded from ema_parameters()
    other = Model.SSD_300()
    _load_params(other, _PARAMS[0])
    other = other.to(DEV).eval()
    _STREAM_OWNERS.append(other._engine)
    named = dict(other.named_parameters())
    with torch.no_grad():
        for name, e in zip(tr.names, tr.ema_parameters()):
            named[name].copy_(e)
        want = tuple(t.clone() for t in other(x))
        with tr.ema_weights():
            assert _same(tr.flat_param, ema) and _same(tr.flat_ema, par)
            inside = tuple(t.clone() for t in net(x))
        assert _same(tr.flat_param, par) and _same(tr.flat_ema, ema), "parameters and EMA are not what they were before entry"
        after = tuple(t.clone() for t in net(x))
    assert not _same(before[1], want[1]), "the averaged weights give the same outputs: the comparison proves nothing"
    assert _same(inside[0], want[0]) and _same(inside[1], want[1]), "the forward inside ema_weights() is not the averaged net's"
    assert _same(after[0], before[0]) and _same(after[1], before[1]), "a stale weight cache survived the exit"

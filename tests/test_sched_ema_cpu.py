"""Device-resident learning-rate schedule and weight EMA, the parts that need no GPU: the numpy restatement (tests/sched_ema_ref.py)
and `optim.LRSchedule` against torch's own schedulers and `AveragedModel`, the exported symbols, argument checking of both
optimizers, the state-dict layout, and the data-parallel bookkeeping at world 2 under gloo with torch stand-ins for the GPU-only
`ops` wrappers (as tests/test_grad_clip_cpu.py does)."""
import os
import re
import socket
import types
import warnings

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn
from torch.optim import lr_scheduler as L

import sched_ema_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ssd_sgd_schedule_advance", "ssd_sgd_momentum_sched", "ssd_swap_f32")
BASE_LR = 1e-3
STEPS = 40


# ---- the restatement against torch -----------------------------------------------------------------------------------------------
def _cases():
    from objectdetection_ssd_amd.optim import LRSchedule
    return {
        "multistep": (lambda o: L.MultiStepLR(o, [8, 12]), R.multistep([8, 12]), LRSchedule.multistep([8, 12]), STEPS),
        # torch's CosineAnnealingLR does not stop at T_max: it climbs the cosine again (period 2 * T_max).  The schedule here is
        # defined to HOLD its last factor past the end of the table, so torch is the reference up to and including T_max = 20 and
        # the held value -- torch's own value at T_max, 0.0 -- is asserted for steps 21 .. 40 (where torch itself goes from 6.2e-6 at
        # step 21 back up to the base rate 1e-3 at step 40).
        "cosine": (lambda o: L.CosineAnnealingLR(o, T_max=20), R.cosine(20), LRSchedule.cosine(20), 20),
        "poly": (lambda o: L.PolynomialLR(o, total_iters=20, power=2.0), R.poly(20, 2.0), LRSchedule.poly(20, 2.0), STEPS),
        "warmup": (lambda o: L.LinearLR(o, 0.1, 1.0, 5), R.constant(5), LRSchedule.constant(warmup_steps=5), STEPS),
        "warmup+multistep": (lambda o: L.ChainedScheduler([L.LinearLR(o, 0.1, 1.0, 5), L.MultiStepLR(o, [8, 12])]),
                             R.multistep([8, 12], warmup_steps=5), LRSchedule.multistep([8, 12], warmup_steps=5), STEPS),
    }


def _torch_lrs(make):
    p = nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=BASE_LR)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sched = make(opt)
        out = []
        for _ in range(STEPS + 1):
            out.append(np.float32(sched.get_last_lr()[0]))
            opt.step()
            sched.step()
    return out


@pytest.mark.parametrize("name", ["multistep", "cosine", "poly", "warmup", "warmup+multistep"])
def test_schedules_are_torchs_within_one_f32_ulp(name):
    """Both sides are f64 closed forms rounded once to f32: they can differ only at a rounding boundary, so the bar is 1 ulp."""
    make, factors, sched, torch_until = _cases()[name]
    row = R.table_row(BASE_LR, factors)
    assert sched.table([BASE_LR, 2 * BASE_LR])[0].tobytes() == row.tobytes(), "optim.LRSchedule and the restatement disagree"
    assert sched.table([BASE_LR, 2 * BASE_LR])[1].tobytes() == R.table_row(2 * BASE_LR, factors).tobytes()
    ref = _torch_lrs(make)
    worst = 0
    for t in range(STEPS + 1):
        want = ref[min(t, torch_until)]
        got = R.lr_at(row, t)
        assert float(got) == float(np.float32(np.float64(BASE_LR) * sched.factor(t)))
        worst = max(worst, R.ulps(got, want))
    print(f"{name}: worst distance to torch over {STEPS + 1} steps: {worst} ulp")
    assert worst <= 1


def test_ema_restatement_against_averaged_model():
    """20 updates of a 64 x 64 weight at decay 0.9.  Per update the two differ by at most one rounding (torch's lerp may fuse the
    multiply-add), and the geometric sum at decay 0.9 multiplies that by at most 10: 10 * 2^-23 of the largest value."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    g = torch.Generator().manual_seed(5)
    lin = nn.Linear(64, 64, bias=False)
    avg = AveragedModel(lin, multi_avg_fn=get_ema_multi_avg_fn(0.9))
    avg.update_parameters(lin)                                      # the first call copies
    e = lin.weight.detach().numpy().copy()
    w = R.ema_w(0, 0.9, warmup=False)
    assert w == np.float32(1.0 - 0.9)
    for _ in range(20):
        with torch.no_grad():
            lin.weight.copy_(torch.randn(64, 64, generator=g))
        avg.update_parameters(lin)
        e = R.ema_update(e, lin.weight.detach().numpy(), w)
    want = avg.module.weight.detach().numpy()
    rel = float(np.max(np.abs(e - want)) / np.max(np.abs(want)))
    print(f"EMA restatement against AveragedModel: relative difference {rel:.3g}")
    assert rel <= 10 * 2.0 ** -23


def test_ema_weight_restatement_against_values_worked_by_hand():
    """The GPU tests hold the advance kernel to `R.ema_w` bit for bit; this pins `R.ema_w` itself to exact fractions worked by hand and
    to the weight `get_ema_multi_avg_fn` hands to lerp."""
    from torch.optim.swa_utils import get_ema_multi_avg_fn
    assert float(R.ema_w(0, 0.9)) == float(np.float32(0.9))          # d_0 = min(0.9, 1/10)
    assert float(R.ema_w(5, 0.9999)) == float(np.float32(0.6))       # d_5 = 6/15
    assert float(R.ema_w(2, 0.5)) == 0.75                            # d_2 = min(0.5, 3/12) = 0.25
    assert float(R.ema_w(2, 0.125)) == 0.875 and float(R.ema_w(2, 0.5, warmup=False)) == 0.5
    assert R.ema_w(3, None) == 0.0
    e, p = torch.zeros(1), torch.ones(1)
    get_ema_multi_avg_fn(0.99)([e], [p], 1)                         # torch: e.lerp_(p, 1 - decay) -> e holds float32(1 - 0.99)
    assert float(e) == float(R.ema_w(10 ** 6, 0.99)) == float(R.ema_w(0, 0.99, warmup=False))


# ---- exports and arguments -------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    from objectdetection_ssd_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ssd_gfx950.h")).read()
    declared = set(re.findall(r"\b(ssd_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.ssd_abi_version() == 1
    # host-side argument checks (nothing is launched): NULL pointers, an empty table, overlapping swap ranges, n == 0
    assert lib.ssd_sgd_schedule_advance(None, None, 1, 1, 0.9, 1, None, None) == -3
    assert lib.ssd_sgd_schedule_advance(16, 32, 0, 4, 0.9, 1, None, None) == -1
    assert lib.ssd_sgd_schedule_advance(16, 32, 2, 0, 0.9, 1, None, None) == -1
    assert lib.ssd_sgd_momentum_sched(16, 32, None, None, 4, 64, None, 0.9, 0.0, None, 0, None, None) == -3
    assert lib.ssd_sgd_momentum_sched(16, 32, 48, 80, 4, 64, None, 0.9, 0.0, None, 0, None, None) == -3      # ema without its weight
    assert lib.ssd_sgd_momentum_sched(16, 32, 48, None, 0, 64, None, 0.9, 0.0, None, 0, None, None) == 0
    assert lib.ssd_swap_f32(None, 16, 4, None) == -3 and lib.ssd_swap_f32(16, 32, 0, None) == 0
    assert lib.ssd_swap_f32(16, 24, 4, None) == -1


class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Conv2d(3, 5, 3)          # 135 + 5 params: slots are padded to multiples of 4
        self.b = nn.Conv2d(5, 7, 1)
        self.g = nn.Parameter(torch.ones(1, 6, 1, 1))
        self._engine = types.SimpleNamespace(names=["a.weight", "a.bias", "b.weight", "b.bias", "g"], _wcache={"x": 1})


BAD = [dict(ema_decay=0.0), dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=1.5), dict(ema_decay=float("nan")),
       dict(ema_decay="0.9"), dict(ema_decay=True), dict(schedule="cosine"), dict(schedule=[1.0, 0.5]), dict(schedule=3),
       dict(ema_warmup=1), dict(ema_warmup=None)]


@pytest.mark.parametrize("kw", BAD, ids=[f"{k}={v!r}" for d in BAD for k, v in d.items()])
def test_bad_schedule_and_ema_arguments_are_refused_by_both_optimizers(kw):
    from objectdetection_ssd_amd import optim
    from objectdetection_ssd_amd.ddp import FlatSGDDataParallel
    with pytest.raises(ValueError):
        optim.SGD([nn.Parameter(torch.zeros(3))], lr=0.1, **kw)
    with pytest.raises(ValueError):
        FlatSGDDataParallel(_Tiny(), lr=0.1, **kw)
    o = optim.SGD([nn.Parameter(torch.zeros(3))], lr=0.1)
    setattr(o, *next(iter(kw.items())))                              # plain attributes: a bad value set later is refused at the step
    with pytest.raises(ValueError):
        o.step()


def test_an_empty_or_malformed_table_is_refused():
    from objectdetection_ssd_amd.optim import LRSchedule
    for bad in ([], [[]], [1.0, float("nan")], [1.0, -0.5], [float("inf")], "abc"):
        with pytest.raises(ValueError):
            LRSchedule(bad)
    with pytest.raises(ValueError):
        LRSchedule.cosine(0)
    with pytest.raises(ValueError):
        LRSchedule.constant(warmup_steps=-1)
    s = LRSchedule([1.0, 0.5, 0.25])
    assert len(s) == 3 and s.factor(1) == 0.5 and s.factor(99) == 0.25 and s.table([0.1]).shape == (1, 3)


def test_state_dict_loads_into_torchs_sgd_and_carries_the_counter():
    from objectdetection_ssd_amd import optim
    from objectdetection_ssd_amd.ddp import FlatSGDDataParallel
    p = nn.Parameter(torch.zeros(3))
    sched = optim.LRSchedule.cosine(10, warmup_steps=3)
    o = optim.SGD([p], lr=0.1, momentum=0.9, schedule=sched, ema_decay=0.9)
    assert (o.schedule, o.ema_decay, o.ema_warmup) == (sched, 0.9, True)
    assert o.current_lr is None and o.step_count is None and o.ema_weight is None          # no step yet
    sd = o.state_dict()
    assert [g["sched_step"] for g in sd["param_groups"]] == [0] and sd["param_groups"][0]["lr"] == 0.1
    plain = torch.optim.SGD([nn.Parameter(torch.zeros(3))], lr=0.5, momentum=0.9)
    plain.load_state_dict(sd)                                                                # torch accepts the extra group key
    assert plain.param_groups[0]["lr"] == 0.1
    sd["param_groups"][0]["sched_step"] = 7
    o2 = optim.SGD([nn.Parameter(torch.zeros(3))], lr=0.1, momentum=0.9, schedule=sched, ema_decay=0.9)
    o2.load_state_dict(sd)
    assert "sched_step" not in o2.param_groups[0] and o2.state_dict()["param_groups"][0]["sched_step"] == 7
    # with the feature off the layouts are those of before
    assert "sched_step" not in optim.SGD([p], lr=0.1).state_dict()["param_groups"][0]
    t = FlatSGDDataParallel(_Tiny(), lr=0.1)
    assert t.flat_ema is None and t.current_lr is None and all("sched_step" not in g for g in t.state_dict()["param_groups"])
    # the data-parallel optimizer: state block and table exist from the constructor on (CPU tensors here); the EMA does not -- it
    # starts as a copy of the parameters at the first step, which a broadcast or a loaded model may precede
    t = FlatSGDDataParallel(_Tiny(), lr=0.1, schedule=sched, ema_decay=0.9)
    assert t.flat_ema is None and "ema" not in str(t.state_dict()["state"])
    early = list(t.ema_parameters())                                # asked for before the first step: a copy of the parameters now
    assert torch.equal(t.flat_ema, t.flat_param) and t.flat_ema.data_ptr() != t.flat_param.data_ptr()
    with torch.no_grad():
        t.flat_param.mul_(3.0)                                      # the parameters are loaded afterwards ...
    t._sched_prepare()                                              # ... and the first step starts the average from THEM
    assert torch.equal(t.flat_ema, t.flat_param) and early[0].data_ptr() == t.flat_ema.data_ptr()
    with torch.no_grad():
        t.flat_param.mul_(0.5)
    t._sched_prepare()                                              # later steps leave it alone
    assert not torch.equal(t.flat_ema, t.flat_param)
    assert int(t.step_count) == 0 and tuple(t._sched_table.shape) == (2, len(sched))
    assert t._sched_table[0].numpy().tobytes() == R.table_row(0.2, sched.factors).tobytes()      # group 0 = biases at 2x lr
    assert t._sched_table[1].numpy().tobytes() == R.table_row(0.1, sched.factors).tobytes()
    sd = t.state_dict()
    assert [g["sched_step"] for g in sd["param_groups"]] == [0, 0] and set(sd) == {"state", "param_groups", "flat_steps"}
    assert all(torch.equal(sd["state"][i]["ema"], e) for i, e in enumerate(list(t.ema_parameters())[3:] + list(t.ema_parameters())[:3]))
    # a checkpoint without averages (written with the EMA off) loaded into a trainer that has them: state_dict() still carries the EMA
    bare = FlatSGDDataParallel(_Tiny(), lr=0.1).state_dict()
    t.load_state_dict(bare)
    sd = t.state_dict()
    assert all(sd["state"][i]["ema"].data_ptr() == e.data_ptr() for i, e in enumerate(t.ema_views[3:] + t.ema_views[:3]))
    ptr = t._sched_table.data_ptr()
    t.lr = 0.05                                                     # a new base rate: the table is rewritten in place at the next step
    t._sched_prepare()
    assert t._sched_table.data_ptr() == ptr and t._sched_table[1].numpy().tobytes() == R.table_row(0.05, sched.factors).tobytes()


# ---- world 2 under gloo ----------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _install_standins(ops, log):
    """TEST stand-ins for the GPU-only wrappers, on CPU tensors."""
    def slots(n):
        return 1 if n else 0

    def partials_(grad, partials, slot0, norm_type=2.0):
        log.append(("norm",))
        g = grad.double()
        partials[slot0] = (g * g).sum()
        return slot0 + 1

    def finalize_(partials, n_slots, norm_type, max_norm, pre_scale, guard, state):
        log.append(("finalize",))
        pre = pre_scale.reshape(()).clone()
        total = (partials[:n_slots].sum().sqrt() * pre.double()).float()
        skip = int(bool(guard) and not bool(torch.isfinite(total)))
        state[0], state[1], state[2] = total, 1.0, pre
        ist = state.view(torch.int32)
        ist[3] = skip
        ist[4] += skip

    def advance_(state, lr_table, ema_decay=None, ema_warmup=True, skip=None):
        log.append(("advance", None if skip is None else int(skip)))
        if skip is not None and int(skip) != 0:
            return
        t, (G, T) = int(state[0]), lr_table.shape
        f = state.view(torch.float32)
        f[2:2 + G] = lr_table[:, min(t, T - 1)]
        f[1] = float(R.ema_w(t, ema_decay, ema_warmup))
        state[0] = t + 1

    def sched_(param, grad, buf, ema, lr_dev, ema_w_dev, momentum, weight_decay, grad_scale=None, first_step=False, skip=None):
        log.append(("sgd", float(lr_dev[0]), None if skip is None else int(skip)))
        if skip is not None and int(skip) != 0:
            return
        g = (grad * grad_scale if grad_scale is not None else grad.clone()) + weight_decay * param
        if first_step:
            buf.copy_(g)
        else:
            buf.mul_(momentum).add_(g)
        param.sub_(lr_dev[0] * buf)
        if ema is not None:
            ema.add_(ema_w_dev[0] * (param - ema))

    def refuse(*a, **k):
        raise AssertionError("with the schedule on, the step must go through sgd_momentum_sched_")

    ops.grad_norm_slots, ops.grad_norm_partials_, ops.grad_clip_finalize_ = slots, partials_, finalize_
    ops.sgd_schedule_advance_, ops.sgd_momentum_sched_ = advance_, sched_
    ops.sgd_momentum_guarded_ = ops.sgd_momentum_ = refuse


def _sched_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from objectdetection_ssd_amd import ddp
        from objectdetection_ssd_amd.optim import LRSchedule
        log = []
        _install_standins(ddp.ops, log)
        torch.manual_seed(rank)                                       # every rank its own initial weights: the broadcast matters
        tr = ddp.FlatSGDDataParallel(_Tiny(), lr=0.1, skip_nonfinite=True, schedule=LRSchedule.cosine(6, warmup_steps=2), ema_decay=0.9)
        mine = tr.flat_param.clone()
        tr.broadcast_parameters(0)
        assert tr.flat_ema is None and (rank == 0) == torch.equal(mine, tr.flat_param)
        out = []
        for step in range(4):
            tr.zero_grad()
            g = torch.Generator().manual_seed(1000 * step + rank)
            for p in tr.params:
                p.grad = torch.randn(p.shape, generator=g)
            if step == 2 and rank == 1:
                tr.params[0].grad.view(-1)[5] = float("inf")       # one rank's overflow reaches every rank through the sum
            tr.reduce_gradients(torch.tensor(3.0 + rank))
            start = tr.flat_param.clone()
            before = (start, tr.flat_ema.clone() if step else None, tr._sched_state.clone())
            del log[:]
            tr.step()
            # the norm and its finalise, ONE advance given the guard's skip word, then the two launches at the block's rates
            assert [e[0] for e in log] == ["norm", "finalize", "advance", "sgd", "sgd"], log
            skipped = int(step == 2)
            assert log[2] == ("advance", skipped) and log[3][2] == skipped and log[4][2] == skipped, log
            lrs = tr.current_lr.clone().numpy()
            assert log[3][1] == float(lrs[1]) and log[4][1] == float(lrs[0]), log     # weights at lr[1], biases at lr[0]
            out.append(dict(count=int(tr.step_count), lrs=lrs, ema_w=float(tr.ema_weight), skipped=int(tr.skipped_steps),
                            par=tr.flat_param.clone().numpy(), ema=tr.flat_ema.clone().numpy(),
                            e0=start.numpy(),
                            still=step > 0 and torch.equal(before[0], tr.flat_param) and torch.equal(before[1], tr.flat_ema)
                            and torch.equal(before[2], tr._sched_state)))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_scheduled_data_parallel_step_world2():
    """Both ranks issue advance and then the SGD launches, hold the same counter, rates and averages, and a step that ONE rank's
    non-finite gradient skips advances nothing on either."""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_sched_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = sorted([q.get(timeout=240) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    a, b = out[0][1], out[1][1]
    factors = R.cosine(6, warmup_steps=2)
    rows = [R.table_row(0.2, factors), R.table_row(0.1, factors)]
    taken = 0
    for step, (x, y) in enumerate(zip(a, b)):
        assert x["count"] == y["count"] and np.array_equal(x["lrs"], y["lrs"]) and x["ema_w"] == y["ema_w"], step
        assert np.array_equal(x["par"], y["par"]) and np.array_equal(x["ema"], y["ema"]), step
        if step == 2:
            assert x["still"] and y["still"] and x["skipped"] == y["skipped"] == 1 and x["count"] == taken
            continue
        assert not x["still"] and x["count"] == taken + 1
        assert [np.float32(v) for v in x["lrs"]] == [R.lr_at(r, taken) for r in rows], (step, x["lrs"])
        assert np.float32(x["ema_w"]) == R.ema_w(taken, 0.9, True)
        if step == 0:                                               # the average started from the BROADCAST parameters, on both ranks
            assert np.allclose(x["ema"], x["e0"] + x["ema_w"] * (x["par"] - x["e0"]), rtol=0, atol=1e-6)
        taken += 1
    assert taken == 3 and a[-1]["skipped"] == 1

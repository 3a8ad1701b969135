"""The launch sequence of `optim.SGD.step()`: which `ops` wrapper runs, in which order, over which ranges of a group's flat buffers and
with which device words, in each of the five modes (plain, clip, schedule, schedule + EMA + guard, schedule + clip).  The data-parallel
trainer's sequence is pinned on CPU tensors (tests/test_grad_clip_cpu.py, tests/test_sched_ema_cpu.py); `optim.SGD` refuses CPU
tensors, so its sequence is pinned here, with recorders that log a call and then run the real wrapper.

The model is that of tests/test_grad_clip_gpu.py: (1,) (6,) (3,) in group 0, (7, 5) (1000,) in group 1 at twice the base rate, and
the (6,) parameter has a gradient at step 0 only.  Slots are padded to 16 bytes: 4, 8, 4 floats in group 0 (16 in all), 36, 1000 in
group 1 (1036).  Step 0 starts every momentum buffer: one launch per group with `first_step` set.  Steps 1 and 2 leave the (6,)
parameter out: group 0 is the two runs [0:4] and [12:16]."""
import inspect

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1,), (6,), (3,), (7, 5), (1000,)]
GROUP0 = 3                                             # parameters in group 0
MID = 1
LR, MOMENTUM, WD = 1e-2, 0.9, 5e-4
STEPS = 3
WRAPPERS = ("grad_norm_partials_", "grad_clip_finalize_", "sgd_schedule_advance_", "sgd_momentum_", "sgd_momentum_guarded_",
            "sgd_momentum_sched_")
# (group, offset from the group's first parameter, length, first_step), in launch order
RANGES_STEP0 = [(0, 0, 16, True), (1, 0, 1036, True)]
RANGES_LATER = [(0, 0, 4, False), (0, 12, 4, False), (1, 0, 1036, False)]


def _modes():
    from objectdetection_ssd_amd.optim import LRSchedule
    sched = LRSchedule.cosine(10, warmup_steps=3)
    return {
        "plain": dict(),
        "clip": dict(max_grad_norm=1.0),
        "sched": dict(schedule=sched),
        "sched+ema+guard": dict(schedule=sched, ema_decay=0.9, skip_nonfinite=True),
        "sched+clip": dict(schedule=sched, max_grad_norm=1.0),
    }


@pytest.fixture
def log(monkeypatch):
    """Every call of the six wrappers as (name, arguments by parameter name, defaults filled in); the real wrapper then runs."""
    from objectdetection_ssd_amd import ops
    calls = []

    def recorder(name, orig):
        sig = inspect.signature(orig)

        def wrapped(*a, **k):
            bound = sig.bind(*a, **k)
            bound.apply_defaults()
            calls.append((name, dict(bound.arguments)))
            return orig(*a, **k)
        return wrapped

    for name in WRAPPERS:
        monkeypatch.setattr(ops, name, recorder(name, getattr(ops, name)))
    return calls


def _set_grads(ps, step):
    g = torch.Generator().manual_seed(500 + step)
    for i, p in enumerate(ps):
        t = torch.randn(p.shape, generator=g)
        p.grad = None if (i == MID and step > 0) else t.to(DEV)


def _check_sgd_call(a, ps, want, opt):
    """One SGD launch against (group, offset, length, first_step): the range of the parameter buffer, equally long gradient and
    momentum slices, the group's momentum and weight decay."""
    gi, off, length, first = want
    base = ps[0] if gi == 0 else ps[GROUP0]                # the group's first parameter sits at offset 0 of its flat buffer
    assert (a["param"].data_ptr() - base.data_ptr(), a["param"].numel()) == (4 * off, length), (want, a["param"].shape)
    assert a["grad"].numel() == length and a["buf"].numel() == length and a["param"].dtype == torch.float32
    assert bool(a["first_step"]) == first, want
    assert (a["momentum"], a["weight_decay"]) == (opt.param_groups[gi]["momentum"], opt.param_groups[gi]["weight_decay"])


@pytest.mark.parametrize("mode", ["plain", "clip", "sched", "sched+ema+guard", "sched+clip"])
def test_launch_sequence_of_a_step(mode, log):
    from objectdetection_ssd_amd.optim import SGD
    kw = _modes()[mode]
    clip = "max_grad_norm" in kw or kw.get("skip_nonfinite", False)
    sched = "schedule" in kw
    ps = [torch.nn.Parameter(torch.randn(s, generator=torch.Generator().manual_seed(10 + i)).to(DEV)) for i, s in enumerate(SHAPES)]
    opt = SGD([{"params": ps[:GROUP0]}, {"params": ps[GROUP0:], "lr": 2 * LR}], lr=LR, momentum=MOMENTUM, weight_decay=WD, **kw)
    for step in range(STEPS):
        _set_grads(ps, step)
        del log[:]
        opt.step()
        torch.cuda.synchronize()
        ranges = RANGES_STEP0 if step == 0 else RANGES_LATER
        calls = list(log)
        print(mode, step, [(n, {k: (tuple(v.shape) if torch.is_tensor(v) else v) for k, v in a.items()}) for n, a in calls])
        norm_grads = []
        if clip:
            # one partials launch per range, filling slots 0, 1 (, 2); one finalise over them
            for slot0, want in enumerate(ranges):
                name, a = calls.pop(0)
                assert name == "grad_norm_partials_" and a["grad"].numel() == want[2] and a["slot0"] == slot0, (step, name, want)
                assert a["norm_type"] == 2.0
                norm_grads.append(a["grad"].data_ptr())
            name, a = calls.pop(0)
            assert name == "grad_clip_finalize_" and a["n_slots"] == len(ranges) and a["pre_scale"] is None, (step, name, a)
            assert a["max_norm"] == kw.get("max_grad_norm") and a["guard"] == kw.get("skip_nonfinite", False)
        if sched:
            # ONE advance; it is held still by the skip word only when the guard is on
            name, a = calls.pop(0)
            assert name == "sgd_schedule_advance_", (step, name)
            assert (a["skip"] is not None) == kw.get("skip_nonfinite", False), (step, a["skip"])
            assert a["ema_decay"] == kw.get("ema_decay") and a["ema_warmup"] is True
        sgd = "sgd_momentum_sched_" if sched else "sgd_momentum_guarded_" if clip else "sgd_momentum_"
        assert [n for n, _ in calls] == [sgd] * len(ranges), (step, [n for n, _ in calls])
        for i, ((_, a), want) in enumerate(zip(calls, ranges)):
            _check_sgd_call(a, ps, want, opt)
            if clip:
                assert a["grad"].data_ptr() == norm_grads[i], "the norm read another range than the step"
                assert a["grad_scale"] is not None and a["skip"] is not None
                assert a["skip"].dtype == torch.int32 and a["grad_scale"].data_ptr() == opt.clip_coef.data_ptr() + 4
            else:
                assert a["grad_scale"] is None and a.get("skip") is None
            if sched:
                gi = want[0]
                assert a["lr_dev"].data_ptr() == opt.current_lr[gi:gi + 1].data_ptr()
                assert float(a["lr_dev"][0]) == float(opt.current_lr[gi])
                assert a["ema_w_dev"].data_ptr() == opt.ema_weight.data_ptr()
                if "ema_decay" in kw:
                    assert a["ema"] is not None and a["ema"].numel() == want[2]
                else:
                    assert a["ema"] is None
            else:
                assert a["lr"] == opt.param_groups[want[0]]["lr"] == (LR, 2 * LR)[want[0]]
    if sched:
        assert int(opt.step_count) == STEPS
    if clip:
        assert int(opt.skipped_steps) == 0

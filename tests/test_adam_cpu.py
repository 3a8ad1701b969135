"""Fused Adam / AdamW, the parts that need no GPU: the numpy restatement (tests/adam_ref.py) against torch.optim.Adam / AdamW on CPU
tensors, constructor and refusals of `optim.Adam` / `optim.AdamW`, the state-dict layout of an optimizer that has not stepped, the
launch sequence of `FlatSGDDataParallel(optimizer="adamw")` on CPU tensors with recording stand-ins for the GPU-only wrappers, and
the status codes of both C entries for defective calls (nothing is launched)."""
import inspect
import json
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

import adam_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "adam_ref_distance.json")
F32 = np.float32
SIZES = (1, 7, 1000, 4099)
HYPER = (dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8), dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-6))
STEPS = 12


# ---- the restatement against torch -----------------------------------------------------------------------------------------------
def _against_torch(cls, n, hyper, wd):
    """12 free-running steps of torch's optimizer; at every step the restatement takes ONE step from torch's state.
    -> (largest parameter distance in ulps, step sizes that differ as f32)."""
    lr, betas, eps = hyper["lr"], hyper["betas"], hyper["eps"]
    gen = torch.Generator().manual_seed(17 * n + int(wd * 1000))
    p = nn.Parameter(torch.randn(n, generator=gen))
    opt = cls([p], weight_decay=wd, foreach=False, **hyper)
    state, m, v = R.State(), np.zeros(n, F32), np.zeros(n, F32)
    worst = differ = 0
    for t in range(STEPS):
        grad = torch.randn(n, generator=gen) * (0.1 + t)
        p.grad = grad.clone()
        before = p.detach().numpy().copy()
        opt.step()
        state.advance(*betas)
        assert state.step == t + 1 == int(opt.state[p]["step"])
        # torch forms its step size and bias correction from beta ** t; the running products differ from that in the last f64 bits
        differ += int(F32(-(lr / (1 - betas[0] ** (t + 1)))) != R.step_size(lr, state.pow1))
        differ += int(F32((1 - betas[1] ** (t + 1)) ** 0.5) != R.bc2_sqrt(state.pow2))
        new, m, v, _ = R.step(before, grad.numpy(), m, v, state, lr=lr, betas=betas, eps=eps, weight_decay=wd,
                              decoupled=cls is torch.optim.AdamW)
        assert m.tobytes() == opt.state[p]["exp_avg"].numpy().tobytes(), f"exp_avg differs at step {t}"
        assert v.tobytes() == opt.state[p]["exp_avg_sq"].numpy().tobytes(), f"exp_avg_sq differs at step {t}"
        worst = max(worst, R.ulps(new, p.detach().numpy()))
    return worst, differ


def test_restatement_against_torch_adam_and_adamw():
    """Both moments bit-equal to torch's after every step; the parameter within the recorded one-step distance (its cause is in the
    golden file's note), no step size that differs as f32."""
    golden = json.load(open(GOLDEN))
    worst = differ = cases = 0
    for cls in (torch.optim.Adam, torch.optim.AdamW):
        for n in SIZES:
            for hyper in HYPER:
                for wd in (0.0, 0.01):
                    w, d = _against_torch(cls, n, hyper, wd)
                    worst, differ, cases = max(worst, w), differ + d, cases + 1
    print(f"{cases} cases x {STEPS} steps: parameter at most {worst} ulp from torch's after one step; {differ} step sizes differ as f32")
    assert cases == golden["cases"] and STEPS == golden["steps"]
    assert worst <= golden["param_one_step_ulps"]
    assert differ == golden["step_sizes_differing_as_f32"] == 0


def test_state_block_restatement():
    s = R.State()
    for t in range(5):
        s.advance(0.9, 0.999)
    assert s.step == 5 and float(s.pow1) == 0.9 * 0.9 * 0.9 * 0.9 * 0.9 and float(s.pow2) == ((((0.999 * 0.999) * 0.999) * 0.999) * 0.999)
    assert s.advance(0.9, 0.999, skip=1).step == 5
    w = s.words()
    assert w.nbytes == 24 and w.view(np.int32)[4] == 5 and w.view(np.int32)[5] == 0 and w[0] == s.pow1 and w[1] == s.pow2
    again = R.State.at(5, 0.9, 0.999)
    assert again.words().tobytes() == w.tobytes()


# ---- constructor and refusals ----------------------------------------------------------------------------------------------------
BAD = [dict(amsgrad=True), dict(maximize=True), dict(differentiable=True), dict(betas=(1.0, 0.999)), dict(betas=(0.9, 1.0)),
       dict(betas=(-0.1, 0.999)), dict(betas=(0.9, float("nan"))), dict(lr=-1e-3), dict(eps=-1e-8), dict(weight_decay=-0.1)]


@pytest.mark.parametrize("kw", BAD, ids=[f"{k}={v!r}" for d in BAD for k, v in d.items()])
@pytest.mark.parametrize("name", ["Adam", "AdamW"])
def test_unsupported_and_bad_arguments_are_refused(name, kw):
    from objectdetection_ssd_amd import optim
    with pytest.raises(ValueError):
        getattr(optim, name)([nn.Parameter(torch.zeros(3))], **kw)


def test_trainer_refuses_bad_adam_arguments():
    from objectdetection_ssd_amd.ddp import FlatSGDDataParallel
    for kw in (dict(optimizer="rmsprop"), dict(optimizer="adamw", betas=(0.9, 1.0)), dict(optimizer="adam", eps=-1.0)):
        with pytest.raises(ValueError):
            FlatSGDDataParallel(_Tiny(), lr=0.1, **kw)


def test_groups_with_different_betas_are_refused_at_the_step():
    from objectdetection_ssd_amd import optim
    a, b = nn.Parameter(torch.zeros(3)), nn.Parameter(torch.zeros(3))
    o = optim.AdamW([{"params": [a]}, {"params": [b], "betas": (0.8, 0.999)}], lr=0.1)
    with pytest.raises(ValueError, match="same betas"):
        o.step()


@pytest.mark.parametrize("name", ["Adam", "AdamW"])
def test_signatures_start_with_torchs_parameter_names(name):
    from objectdetection_ssd_amd import optim
    mine = list(inspect.signature(getattr(optim, name).__init__).parameters.values())
    theirs = list(inspect.signature(getattr(torch.optim, name).__init__).parameters.values())
    assert [(p.name, p.kind) for p in mine[:len(theirs)]] == [(p.name, p.kind) for p in theirs]
    assert [p.default for p in mine[2:len(theirs)]] == [p.default for p in theirs[2:]]
    assert [p.name for p in mine[len(theirs):]] == ["max_grad_norm", "norm_type", "skip_nonfinite", "schedule", "ema_decay", "ema_warmup"]
    sgd = inspect.signature(optim.SGD.__init__).parameters
    assert all(p.kind is p.KEYWORD_ONLY and p.default == sgd[p.name].default for p in mine[len(theirs):])


# ---- state dict, before any step -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Adam", "AdamW"])
def test_state_dict_layout_of_an_optimizer_that_has_not_stepped(name):
    from objectdetection_ssd_amd import optim
    ps = [nn.Parameter(torch.zeros(3)), nn.Parameter(torch.zeros(2, 2))]
    kw = dict(lr=0.01, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.1)
    mine, theirs = getattr(optim, name)(ps, **kw), getattr(torch.optim, name)(ps, **kw)
    a, b = mine.state_dict(), theirs.state_dict()
    assert a["state"] == b["state"] == {} and list(a) == list(b)
    assert [list(g) for g in a["param_groups"]] == [list(g) for g in b["param_groups"]]
    assert a["param_groups"] == b["param_groups"]
    assert isinstance(mine, torch.optim.Optimizer) and mine.adam_steps is None
    # torch's own checkpoint loads, and its step count becomes the optimizer's one counter
    for p in ps:
        p.grad = torch.ones_like(p)
    theirs.step()
    theirs.step()
    mine.load_state_dict(theirs.state_dict())
    assert mine._adam_start == (2, 0.8 * 0.8, 0.99 * 0.99) and mine._adam_step_host() == 2
    back = mine.state_dict()
    assert all(float(st["step"]) == 2.0 and st["step"].dtype == torch.float32 and st["step"].dim() == 0 for st in back["state"].values())
    assert {k: (v.dtype, v.shape) for k, v in back["state"][1].items()} == {k: (v.dtype, v.shape) for k, v in theirs.state_dict()["state"][1].items()}
    getattr(torch.optim, name)(ps, **kw).load_state_dict(back)                     # ... and the other way round
    uneven = theirs.state_dict()
    uneven["state"][1]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError, match="disagree"):
        mine.load_state_dict(uneven)
    # with the schedule on, the counter of the schedule travels as optim.SGD carries it
    sched = getattr(optim, name)(ps, schedule=optim.LRSchedule.cosine(10), **kw).state_dict()
    assert [g["sched_step"] for g in sched["param_groups"]] == [0]


# ---- the trainer's launch sequence on CPU tensors --------------------------------------------------------------------------------
class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Conv2d(3, 5, 3)          # 135 + 5 params: slots are padded to multiples of 4
        self.b = nn.Conv2d(5, 7, 1)
        self.g = nn.Parameter(torch.ones(1, 6, 1, 1))
        self._engine = types.SimpleNamespace(names=["a.weight", "a.bias", "b.weight", "b.bias", "g"], _wcache={"x": 1})


def _install_standins(ops, log):
    """TEST stand-ins for the GPU-only wrappers, on CPU tensors: they record the launches; the Adam launch is the restatement."""
    def partials_(grad, partials, slot0, norm_type=2.0):
        log.append(("norm", grad.numel()))
        partials[slot0] = (grad.double() ** 2).sum()
        return slot0 + 1

    def finalize_(partials, n_slots, norm_type, max_norm, pre_scale, guard, state):
        log.append(("finalize",))
        pre = pre_scale.reshape(()).clone()
        total = (partials[:n_slots].sum().sqrt() * pre.double()).float()
        skip = int(bool(guard) and not bool(torch.isfinite(total)))
        coef = 1.0 if max_norm is None else min(1.0, max_norm / (float(total) + 1e-6))
        state[0], state[1], state[2] = total, coef, pre * coef
        ist = state.view(torch.int32)
        ist[3] = skip
        ist[4] += skip

    def sched_advance_(state, lr_table, ema_decay=None, ema_warmup=True, skip=None):
        log.append(("sched_advance", None if skip is None else int(skip)))
        if skip is not None and int(skip) != 0:
            return
        t, (G, T) = int(state[0]), lr_table.shape
        f = state.view(torch.float32)
        f[2:2 + G] = lr_table[:, min(t, T - 1)]
        f[1] = 0.0 if ema_decay is None else 1.0 - min(ema_decay, (1 + t) / (10 + t)) if ema_warmup else 1.0 - ema_decay
        state[0] = t + 1

    def adam_advance_(state, beta1, beta2, skip=None):
        log.append(("adam_advance", beta1, beta2, None if skip is None else int(skip)))
        if skip is not None and int(skip) != 0:
            return
        state[0] *= beta1
        state[1] *= beta2
        state.view(torch.int32)[4] += 1

    def adam_step_(param, grad, exp_avg, exp_avg_sq, ema, lr, lr_dev, ema_w_dev, state, beta1, beta2, eps, weight_decay, decoupled,
                   grad_scale=None, skip=None):
        log.append(dict(kind="adam", n=param.numel(), off=(param.data_ptr() - param._base.data_ptr()) // 4, lr=lr,
                        lr_dev=None if lr_dev is None else float(lr_dev[0]), ema=ema is not None, decoupled=decoupled, eps=eps,
                        wd=weight_decay, scale=None if grad_scale is None else float(grad_scale[0]),
                        skip=None if skip is None else int(skip)))
        assert grad.numel() == exp_avg.numel() == exp_avg_sq.numel() == param.numel()
        if skip is not None and int(skip) != 0:
            return
        st = R.State(int(state.view(torch.int32)[4]), float(state[0]), float(state[1]))
        p, m, v, e = R.step(param.numpy(), grad.numpy(), exp_avg.numpy(), exp_avg_sq.numpy(), st,
                            lr=lr if lr_dev is None else lr_dev.numpy()[0], betas=(beta1, beta2), eps=eps, weight_decay=weight_decay,
                            decoupled=decoupled, grad_scale=None if grad_scale is None else grad_scale.numpy()[0],
                            ema=None if ema is None else ema.numpy(), ema_w=None if ema is None else ema_w_dev.numpy()[0])
        param.copy_(torch.from_numpy(p)); exp_avg.copy_(torch.from_numpy(m)); exp_avg_sq.copy_(torch.from_numpy(v))
        if ema is not None:
            ema.copy_(torch.from_numpy(e))

    def refuse(*a, **k):
        raise AssertionError("an Adam trainer must not launch SGD")

    ops.grad_norm_slots, ops.grad_norm_partials_, ops.grad_clip_finalize_ = (lambda n: 1 if n else 0), partials_, finalize_
    ops.sgd_schedule_advance_, ops.adam_advance_, ops.adam_step_ = sched_advance_, adam_advance_, adam_step_
    ops.sgd_momentum_sched_ = ops.sgd_momentum_guarded_ = ops.sgd_momentum_ = refuse


MODES = {"plain": {}, "clip": dict(max_grad_norm=0.5),
         "sched+ema+guard": dict(skip_nonfinite=True, ema_decay=0.9, schedule="cosine")}


@pytest.mark.parametrize("mode", list(MODES))
def test_adamw_trainer_launch_sequence_on_cpu_tensors(mode, monkeypatch):
    from objectdetection_ssd_amd import ddp, optim
    log = []
    for name in ("grad_norm_slots", "grad_norm_partials_", "grad_clip_finalize_", "sgd_schedule_advance_", "adam_advance_", "adam_step_",
                 "sgd_momentum_sched_", "sgd_momentum_guarded_", "sgd_momentum_"):
        monkeypatch.setattr(ddp.ops, name, getattr(ddp.ops, name))                 # (put back after the test)
    _install_standins(ddp.ops, log)
    kw = dict(MODES[mode])
    if "schedule" in kw:
        kw["schedule"] = optim.LRSchedule.cosine(6, warmup_steps=2)
    torch.manual_seed(3)
    tr = ddp.FlatSGDDataParallel(_Tiny(), lr=0.01, weight_decay=0.01, optimizer="adamw", betas=(0.8, 0.99), eps=1e-6, **kw)
    assert tr.optimizer_kind == "adamw" and tr.flat_sq is not None and tr.flat_sq.numel() == tr.n
    assert list(tr.param_groups[0]) == list(torch.optim.AdamW([nn.Parameter(torch.zeros(1))]).param_groups[0])
    assert tr.state_dict()["state"] == {}
    guard, sched = "skip_nonfinite" in kw, "schedule" in kw
    for step in range(3):
        tr.zero_grad()
        gen = torch.Generator().manual_seed(step)
        for p in tr.params:
            p.grad = torch.randn(p.shape, generator=gen)
        if guard and step == 1:
            tr.params[0].grad.view(-1)[5] = float("nan")
        tr.reduce_gradients(torch.tensor(4.0))
        before = [t.clone() for t in (tr.flat_param, tr.flat_mom, tr.flat_sq, tr._adam_state)]
        del log[:]
        tr.step()
        kinds = [e["kind"] if isinstance(e, dict) else e[0] for e in log]
        want = (["norm", "finalize"] if mode != "plain" else []) + (["sched_advance"] if sched else []) + ["adam_advance", "adam", "adam"]
        assert kinds == want, log
        skipped = int(guard and step == 1)
        adv = log[kinds.index("adam_advance")]
        assert adv == ("adam_advance", 0.8, 0.99, skipped if guard else None), adv     # ONE advance, its skip word only under the guard
        w, b = log[-2], log[-1]
        assert (w["off"], w["n"]) == (0, tr.n_w) and (b["off"], b["n"]) == (tr.n_w, tr.n - tr.n_w)
        assert w["decoupled"] and b["decoupled"] and w["eps"] == 1e-6 and w["wd"] == 0.01 and (w["lr"], b["lr"]) == (0.01, 0.02)
        assert w["ema"] == b["ema"] == ("ema_decay" in kw)
        assert w["skip"] == b["skip"] == (skipped if mode != "plain" else None)
        if sched:
            lrs = tr.current_lr.numpy()
            assert (w["lr_dev"], b["lr_dev"]) == (float(lrs[1]), float(lrs[0]))
        else:
            assert w["lr_dev"] is None and b["lr_dev"] is None
        assert w["scale"] == (0.25 if mode == "plain" else float(tr._clip_state[2]))     # pre_scale = 1 / n_pos, times the clip
        same = all(torch.equal(x, y) for x, y in zip(before, (tr.flat_param, tr.flat_mom, tr.flat_sq, tr._adam_state)))
        assert same == bool(skipped)
    taken = 2 if guard else 3
    assert int(tr.adam_steps) == taken and tr.steps == 3
    # state_dict carries both moments as views of the flat buffers, and the one counter as every parameter's step
    sd = tr.state_dict()
    order = [3, 4, 0, 1, 2]                                                            # group 0 = biases, group 1 = weights
    for i, k in enumerate(order):
        st = sd["state"][i]
        assert float(st["step"]) == taken and st["step"].dtype == torch.float32
        assert st["exp_avg"].data_ptr() == tr.mom_views[k].data_ptr() and st["exp_avg_sq"].data_ptr() == tr.sq_views[k].data_ptr()
    # ... loads into a fresh trainer, which continues with the same block, and into torch's AdamW over the same groups
    torch.manual_seed(3)
    tr2 = ddp.FlatSGDDataParallel(_Tiny(), lr=0.01, weight_decay=0.01, optimizer="adamw", betas=(0.8, 0.99), eps=1e-6, **kw)
    tr2.load_state_dict(sd)
    assert torch.equal(tr2.flat_mom, tr.flat_mom) and torch.equal(tr2.flat_sq, tr.flat_sq)
    assert tr2._adam_state.numpy().tobytes() == tr._adam_state.numpy().tobytes() == R.State.at(taken, 0.8, 0.99).words().tobytes()
    torch.optim.AdamW([{"params": tr.params[3:], "lr": 0.02}, {"params": tr.params[:3]}], lr=0.01).load_state_dict(sd)
    tr.close()
    tr2.close()


# ---- status codes, nothing is launched --------------------------------------------------------------------------------------------
OK, BAD_SHAPE, NULL, ALIGN = 0, -1, -3, -5


def _step_args(**over):
    a = dict(param=0x1000, grad=0x2000, exp_avg=0x3000, exp_avg_sq=0x4000, ema=None, n=0, lr=1e-3, lr_dev=None, ema_w_dev=None,
             state=0x5000, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, decoupled=1, grad_scale_dev=None, skip_dev=None,
             stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


def test_symbols_are_declared_bound_and_exported():
    from objectdetection_ssd_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ssd_gfx950.h")).read()
    declared = set(re.findall(r"\b(ssd_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name, n_args in (("ssd_adam_advance", 5), ("ssd_adam_step", 18)):
        assert name in declared and hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == n_args, name
    assert lib.ssd_abi_version() == 1


def test_status_codes_of_both_entries():
    """n == 0 in every call of ssd_adam_step, so even the valid ones launch nothing; ssd_adam_advance is only called defectively."""
    from objectdetection_ssd_amd import _lib
    lib = _lib.load()
    step = lib.ssd_adam_step
    assert step(*_step_args()) == OK
    assert step(*_step_args(ema=0x6000, ema_w_dev=0x7000, lr_dev=0x7010, grad_scale_dev=0x7020, skip_dev=0x7030)) == OK
    for name in ("param", "grad", "exp_avg", "exp_avg_sq", "state"):
        assert step(*_step_args(**{name: None})) == NULL, name
    assert step(*_step_args(ema=0x6000)) == NULL                                    # the EMA without its weight
    for name in ("param", "grad", "exp_avg", "exp_avg_sq", "state"):
        assert step(*_step_args(**{name: 0x1004 if name != "state" else 0x5004})) == (ALIGN if name == "state" else OK), name
        assert step(*_step_args(**{name: 0x1002})) == ALIGN, name
    assert step(*_step_args(ema=0x6002, ema_w_dev=0x7000)) == ALIGN and step(*_step_args(skip_dev=0x7002)) == ALIGN
    for bad in (dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=float("nan")), dict(eps=-1e-8), dict(weight_decay=-0.1),
                dict(lr=-1.0)):
        assert step(*_step_args(**bad)) == BAD_SHAPE, bad
        assert step(*_step_args(param=None, **bad)) == NULL, bad                    # NULL comes first ...
        assert step(*_step_args(grad=0x2002, **bad)) == BAD_SHAPE, bad              # ... and the values before the alignment
    assert step(*_step_args(lr=-1.0, lr_dev=0x7010)) == OK                          # the host rate is not read then
    adv = lib.ssd_adam_advance
    assert adv(None, 0.9, 0.999, None, None) == NULL
    assert adv(0x5000, 1.0, 0.999, None, None) == BAD_SHAPE and adv(0x5000, 0.9, -0.5, None, None) == BAD_SHAPE
    assert adv(None, 1.0, 0.999, None, None) == NULL and adv(0x5004, 1.5, 0.999, None, None) == BAD_SHAPE
    assert adv(0x5004, 0.9, 0.999, None, None) == ALIGN and adv(0x5000, 0.9, 0.999, 0x7002, None) == ALIGN

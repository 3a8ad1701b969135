"""`torch.optim.SGD` for the step that follows the hot path, as one fused launch per parameter group.

The reference builds its optimizer as (train.py:44-55)

    torch.optim.SGD(params=[{'params': biases, 'lr': 2*lr}, {'params': not_biases}], lr=lr, momentum=0.9, weight_decay=5e-4)

and `train_function.py` then uses `.zero_grad()`, `.step()`, `.param_groups[*]['lr']`, `.state_dict()` and
`.load_state_dict()` (train_function.py:8-9,27-30,76,95,116).  `SGD` here keeps all of that -- same constructor, same
param-group keys, same `state[p]['momentum_buffer']` entries, so checkpoints move between the two -- and runs
`ssd_sgd_momentum` (include/ssd_gfx950.h) once per group on flat storage: each group's parameters and momentum buffers
are re-seated as views of one buffer the first time `step()` sees them, gradients are gathered with one foreach copy.
The kernel reproduces torch's rounding sequence, so the parameters after k steps are bit-identical to torch.optim.SGD's.

This module is also where the pieces that `SGD` shares with `ddp.FlatSGDDataParallel` exist once: `FlatLayout` (the slot rule of a
flat buffer), `FlatStore` (the flat parameter / gradient / momentum / EMA buffers of one layout, their views and the EMA's life
cycle; `SGD` / `Adam` keep one per parameter group, the trainer one over all its parameters), `FusedStepMixin._step_controls` (the order
inside a step: clip norm and finalise, ONE schedule advance, and the device words the SGD launches then read) and `launch_sgd`
(the choice between the plain, guarded and scheduled SGD wrappers).  What differs stays with each optimizer: how gradients reach the
flat buffer, which ranges are launched, and the momentum bookkeeping.

Only what the reference uses is implemented: `dampening`, `nesterov`, `maximize` must stay at their defaults.  GPU only,
like the rest of the package.

Gradient clipping and the non-finite step guard (`max_grad_norm`, `norm_type`, `skip_nonfinite`) are what a user of that loop
adds with `torch.nn.utils.clip_grad_norm_` between `backward()` and `step()`: here they are one norm pass per launch range, one
finalise launch and the guarded form of the same SGD kernel, and nothing comes back to the host (`GradClipMixin`).

A per-iteration learning-rate schedule (`LRSchedule`: warm-up, multistep, cosine, polynomial) and an exponential moving average of
the weights (`ema_decay`) live on the device too (`SchedEmaMixin`): the rate is a device word the SGD launch reads, a device step
counter indexes a table of rates built on the host, and the average is updated in the pass SGD makes anyway.

`Adam` and `AdamW` are torch's optimizers of those names on the same stores, controls and launch order (`FlatGroupOptimizer` is what
the three share): `ssd_adam_step` per run, the first moments in the stores' `mom` buffers, the second in `sq`, and ONE device step
counter with the running products beta1^t, beta2^t per optimizer (`AdamStateMixin`), where torch counts per parameter.
"""
from __future__ import annotations

import contextlib
import math
from typing import List

import numpy as np
import torch

from . import ops


def check_clip_settings(max_grad_norm, norm_type, skip_nonfinite) -> None:
    if max_grad_norm is not None:
        if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float)) or not max_grad_norm > 0:
            raise ValueError(f"max_grad_norm must be None or a positive number, got {max_grad_norm!r}")
    if isinstance(norm_type, bool) or not isinstance(norm_type, (int, float)) or not (norm_type == 2 or norm_type == math.inf):
        raise ValueError(f"norm_type must be 2 or float('inf'), got {norm_type!r}")
    if not isinstance(skip_nonfinite, bool):
        raise ValueError(f"skip_nonfinite must be a bool, got {skip_nonfinite!r}")


class GradClipMixin:
    """Settings, device state and launches of gradient-norm clipping and the non-finite step guard, shared by `optim.SGD` and
    `ddp.FlatSGDDataParallel`.  The settings are plain attributes (`max_grad_norm`, `norm_type`, `skip_nonfinite`), read at every
    step; the state block (include/ssd_gfx950.h, ssd_grad_clip_finalize) lives on the device and `grad_norm` / `clip_coef` /
    `skipped_steps` are views of it: reading them is the caller's synchronisation, the step itself never synchronises."""

    def _init_clip(self, max_grad_norm, norm_type, skip_nonfinite) -> None:
        check_clip_settings(max_grad_norm, norm_type, skip_nonfinite)
        self.max_grad_norm, self.norm_type, self.skip_nonfinite = max_grad_norm, norm_type, skip_nonfinite
        self._clip_state = None
        self._clip_partials = None

    def _clip_on(self) -> bool:
        check_clip_settings(self.max_grad_norm, self.norm_type, self.skip_nonfinite)
        return self.max_grad_norm is not None or self.skip_nonfinite

    def _clip_settings(self):
        return (self.max_grad_norm, float(self.norm_type), self.skip_nonfinite)

    def _clip_buffers(self, dev, slots: int) -> None:
        if self._clip_state is None or self._clip_state.device != dev:
            self._clip_state = torch.zeros(ops.GRAD_CLIP_STATE_WORDS, device=dev, dtype=torch.float32)
        if self._clip_partials is None or self._clip_partials.device != dev or self._clip_partials.numel() < slots:
            self._clip_partials = torch.zeros(max(slots, 1), device=dev, dtype=torch.float64)

    @property
    def grad_norm(self):
        """0-dim f32 device tensor: the global gradient norm of the last clipped / guarded step (None before the first)."""
        return None if self._clip_state is None else self._clip_state[0]

    @property
    def clip_coef(self):
        """0-dim f32 device tensor: min(1, max_grad_norm / (grad_norm + 1e-6)) of the last step."""
        return None if self._clip_state is None else self._clip_state[1]

    @property
    def skipped_steps(self):
        """0-dim int32 device tensor: steps the guard has skipped so far."""
        return None if self._clip_state is None else self._clip_state.view(torch.int32)[4]


class LRSchedule:
    """A per-step learning-rate schedule as a table of factors: step t runs at `group['lr'] * factors[min(t, T-1)]` -- past the end the
    last factor holds.  The factors are f64; group g's row of the device table is `float32(float64(group['lr']) * factors[t])`, one
    rounding.  `param_groups[g]['lr']` stays the BASE rate (writing a new base rebuilds the table at the next step).  The factors are
    copied and read-only: an optimizer and a captured step key their table by the identity of this object, so another schedule is
    another `LRSchedule`.

    The constructors are the closed forms of torch's schedulers times a linear warm-up: factor(t) = warm(t) * decay(t),
    warm(t) = warmup_start + (1 - warmup_start) * t / warmup_steps for t < warmup_steps, else 1 (torch's LinearLR)."""

    def __init__(self, factors) -> None:
        try:
            f = np.array(factors, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError) as e:
            raise ValueError(f"LRSchedule: factors must be a sequence of numbers ({e})") from None
        if f.size == 0:
            raise ValueError("LRSchedule: an empty table")
        if not np.all(np.isfinite(f)) or np.any(f < 0):
            raise ValueError("LRSchedule: factors must be finite and non-negative")
        f.setflags(write=False)
        self.factors = f

    def __len__(self) -> int:
        return int(self.factors.size)

    def factor(self, t: int) -> float:
        return float(self.factors[min(max(int(t), 0), self.factors.size - 1)])

    def table(self, base_lrs) -> np.ndarray:
        """(groups, T) f32: the rows the device reads."""
        return np.stack([(np.float64(lr) * self.factors).astype(np.float32) for lr in base_lrs])

    @staticmethod
    def _warm(t: int, warmup_steps: int, warmup_start: float) -> float:
        if t >= warmup_steps:
            return 1.0
        return warmup_start + (1.0 - warmup_start) * t / warmup_steps

    @classmethod
    def _build(cls, decay, steps: int, warmup_steps: int, warmup_start: float) -> "LRSchedule":
        if isinstance(warmup_steps, bool) or not isinstance(warmup_steps, int) or warmup_steps < 0:
            raise ValueError(f"LRSchedule: warmup_steps must be a non-negative integer, got {warmup_steps!r}")
        if not 0.0 < float(warmup_start) <= 1.0:
            raise ValueError(f"LRSchedule: warmup_start must be in (0, 1], got {warmup_start!r}")
        steps = max(int(steps), warmup_steps)
        return cls([cls._warm(t, warmup_steps, float(warmup_start)) * decay(t) for t in range(steps + 1)])

    @classmethod
    def constant(cls, warmup_steps: int = 0, warmup_start: float = 0.1) -> "LRSchedule":
        return cls._build(lambda t: 1.0, 0, warmup_steps, warmup_start)

    @classmethod
    def multistep(cls, milestones, gamma: float = 0.1, total_steps=None, warmup_steps: int = 0, warmup_start: float = 0.1) -> "LRSchedule":
        """torch's MultiStepLR: the factor is multiplied by `gamma` at every milestone (once per occurrence)."""
        ms = sorted(int(m) for m in milestones)
        if any(m < 0 for m in ms):
            raise ValueError("LRSchedule.multistep: milestones must be non-negative")
        acc, out = 1.0, []
        last = max(ms + [0])
        for t in range(last + 1):
            for _ in range(ms.count(t)):
                acc = acc * gamma
            out.append(acc)
        return cls._build(lambda t: out[min(t, last)], last if total_steps is None else total_steps, warmup_steps, warmup_start)

    @classmethod
    def cosine(cls, total_steps: int, min_factor: float = 0.0, warmup_steps: int = 0, warmup_start: float = 0.1) -> "LRSchedule":
        """torch's CosineAnnealingLR(T_max=total_steps, eta_min=min_factor * lr) up to total_steps; then `min_factor` holds."""
        if int(total_steps) < 1:
            raise ValueError("LRSchedule.cosine: total_steps must be positive")
        T = int(total_steps)
        return cls._build(lambda t: min_factor + (1.0 - min_factor) * 0.5 * (1.0 + math.cos(math.pi * min(t, T) / T)), T, warmup_steps,
                          warmup_start)

    @classmethod
    def poly(cls, total_steps: int, power: float = 1.0, warmup_steps: int = 0, warmup_start: float = 0.1) -> "LRSchedule":
        """torch's PolynomialLR(total_iters=total_steps, power)."""
        if int(total_steps) < 1:
            raise ValueError("LRSchedule.poly: total_steps must be positive")
        T = int(total_steps)
        return cls._build(lambda t: (1.0 - min(t, T) / T) ** power, T, warmup_steps, warmup_start)


def check_sched_settings(schedule, ema_decay, ema_warmup) -> None:
    if schedule is not None and not isinstance(schedule, LRSchedule):
        raise ValueError(f"schedule must be None or an LRSchedule, got {type(schedule).__name__}")
    if schedule is not None and len(schedule) == 0:
        raise ValueError("schedule: an empty table")
    if ema_decay is not None:
        if isinstance(ema_decay, bool) or not isinstance(ema_decay, (int, float)) or not 0.0 < ema_decay < 1.0:
            raise ValueError(f"ema_decay must be None or a number in (0, 1), got {ema_decay!r}")
    if not isinstance(ema_warmup, bool):
        raise ValueError(f"ema_warmup must be a bool, got {ema_warmup!r}")


class SchedEmaMixin:
    """Settings, device state and launches of the device-resident learning-rate schedule and the weight EMA, shared by `optim.SGD` and
    `ddp.FlatSGDDataParallel`.  `schedule`, `ema_decay` and `ema_warmup` are plain attributes read at every step.  The state block
    (include/ssd_gfx950.h, ssd_sgd_schedule_advance: step counter, EMA weight, one lr word per group) lives on the device;
    `current_lr`, `step_count` and `ema_weight` are views of it and never synchronise."""

    def _init_sched(self, schedule, ema_decay, ema_warmup) -> None:
        check_sched_settings(schedule, ema_decay, ema_warmup)
        self.schedule, self.ema_decay, self.ema_warmup = schedule, ema_decay, ema_warmup
        self._sched_state = None          # int32[2 + G]
        self._sched_table = None          # f32 (G, T)
        self._sched_key = None            # (schedule, base lrs) the table was built from
        self._sched_step0 = 0             # counter a restored checkpoint starts from, until the block exists

    def _sched_on(self) -> bool:
        check_sched_settings(self.schedule, self.ema_decay, self.ema_warmup)
        return self.schedule is not None or self.ema_decay is not None

    def _sched_settings(self):
        return (self.schedule, self.ema_decay, self.ema_warmup)

    def _sched_buffers(self, dev) -> None:
        """The state block and the table of rates, built or rebuilt outside any capture: a new base lr or another schedule object is
        written INTO the table's storage when the shape allows, so a captured step keeps reading the right memory."""
        G = len(self.param_groups)
        if self._sched_state is None or self._sched_state.device != dev or self._sched_state.numel() != ops.SCHED_STATE_HEAD + G:
            old = self._sched_state
            self._sched_state = torch.zeros(ops.SCHED_STATE_HEAD + G, device=dev, dtype=torch.int32)
            if old is not None:                                    # (a parameter group was added: the counter goes on)
                self._sched_state[0:1].copy_(old[0:1])
            elif self._sched_step0:
                self._sched_state[0:1].fill_(self._sched_step0)
            self._sched_key = None
        base = tuple(float(g["lr"]) for g in self.param_groups)
        key = (self.schedule, base)
        if self._sched_key is None or self._sched_key[0] is not key[0] or self._sched_key[1] != key[1]:
            sch = self.schedule if self.schedule is not None else LRSchedule([1.0])      # the EMA alone: the one-column table of base lrs
            host = torch.from_numpy(sch.table(base))
            if self._sched_table is not None and self._sched_table.device == dev and self._sched_table.shape == host.shape:
                self._sched_table.copy_(host)
            else:
                self._sched_table = host.to(dev)
            self._sched_key = key

    def _sched_step_host(self) -> int:
        """The counter, read back: the one synchronisation (checkpoints)."""
        return int(self._sched_state[0].item()) if self._sched_state is not None else int(self._sched_step0)

    def _sched_stamp(self, sd):
        """state_dict(): with the feature on every param group carries `sched_step`, the device counter."""
        if self._sched_on():
            step = self._sched_step_host()
            for g in sd["param_groups"]:
                g["sched_step"] = step
        return sd

    def _sched_unstamp(self) -> None:
        """load_state_dict(): take `sched_step` out of the restored groups and into the device counter."""
        steps = [g.pop("sched_step", None) for g in self.param_groups]
        steps = [s for s in steps if s is not None]
        if steps:
            self._sched_step0 = int(steps[0])
            if self._sched_state is not None:
                self._sched_state[0:1].fill_(self._sched_step0)

    @property
    def current_lr(self):
        """f32[G] device tensor: the rate each group's last step ran at (None before the first step with the feature on)."""
        return None if self._sched_state is None else self._sched_state.view(torch.float32)[ops.SCHED_STATE_HEAD:]

    @property
    def step_count(self):
        """0-dim int32 device tensor: optimizer steps actually taken (skipped steps do not count)."""
        return None if self._sched_state is None else self._sched_state[0]

    @property
    def ema_weight(self):
        """0-dim f32 device tensor: 1 - decay of the last step, the weight the EMA moved towards the new parameters by."""
        return None if self._sched_state is None else self._sched_state.view(torch.float32)[1]


class FusedStepMixin(GradClipMixin, SchedEmaMixin):
    """What both optimizers run between the gradients and the SGD launches."""

    def _step_controls(self, ranges, pre_scale=None):
        """The device words this step's SGD launches read -> (grad_scale, skip, lr_words, ema_w); each is None when its feature is off
        (grad_scale is then `pre_scale`).  Order: with clipping or the guard on, the norm of the flat f32 gradient `ranges` (one
        partials launch each) times `pre_scale` and one finalise; with the schedule or the EMA on, ONE advance, given the skip word
        only when the guard is on, so a skipped step advances neither the counter nor the EMA.  The buffers exist already
        (`_clip_buffers`, `_sched_buffers`: never inside a capture)."""
        grad_scale, skip, lr_words, ema_w = pre_scale, None, None, None
        if self._clip_on():
            s = 0
            for r in ranges:
                s = ops.grad_norm_partials_(r, self._clip_partials, s, self.norm_type)
            ops.grad_clip_finalize_(self._clip_partials, s, self.norm_type, self.max_grad_norm, pre_scale, self.skip_nonfinite,
                                    self._clip_state)
            grad_scale, skip = self._clip_state[2:3], self._clip_state.view(torch.int32)[3:4]
        if self._sched_on():
            ops.sgd_schedule_advance_(self._sched_state, self._sched_table, self.ema_decay, self.ema_warmup,
                                      skip if self.skip_nonfinite else None)
            f = self._sched_state.view(torch.float32)
            lr_words, ema_w = f[ops.SCHED_STATE_HEAD:], f[1:2]          # f32[G], f32[1]
        return grad_scale, skip, lr_words, ema_w


def launch_sgd(param, grad, buf, *, lr, lr_dev, ema, ema_w, momentum, weight_decay, grad_scale, first, skip) -> None:
    """One fused SGD launch over equally long flat slices: the only caller of the three wrappers.  With the device rate `lr_dev` the
    scheduled form (which also updates `ema`, if given, by the device weight `ema_w`); else, with the device flag `skip`, the guarded
    form at the host rate `lr`; else the plain one."""
    if lr_dev is not None:
        ops.sgd_momentum_sched_(param, grad, buf, ema, lr_dev, ema_w, momentum, weight_decay, grad_scale, first, skip)
    elif skip is not None:
        ops.sgd_momentum_guarded_(param, grad, buf, lr, momentum, weight_decay, grad_scale, first, skip)
    else:
        ops.sgd_momentum_(param, grad, buf, lr, momentum, weight_decay, grad_scale, first)


class FlatLayout:
    """Where each parameter sits in a flat f32 buffer.  Every parameter starts 16-byte aligned: its slot is its size rounded up to a
    multiple of 4 floats, and `offsets` (one more entry than there are parameters) are the running sums of the slots."""

    def __init__(self, params) -> None:
        self.shapes = [p.shape for p in params]
        self.sizes = [p.numel() for p in params]
        self.slots = [(s + 3) // 4 * 4 for s in self.sizes]
        self.offsets = [0]
        for s in self.slots:
            self.offsets.append(self.offsets[-1] + s)
        self.total = self.offsets[-1]

    def views(self, flat) -> list:
        """One view of `flat` per parameter, in its shape."""
        return [flat[o:o + sz].view(shape) for o, sz, shape in zip(self.offsets, self.sizes, self.shapes)]

    def span(self, lo: int, hi: int) -> slice:
        """The floats of parameters lo .. hi-1, the last one's pad included."""
        return slice(self.offsets[lo], self.offsets[hi])


class FlatStore:
    """The flat `param`, `grad`, `mom` and (once asked for) `ema` buffers of one `FlatLayout`, and their per-parameter views.  The
    parameters are seated in `param` (`p.data` become its views); `grad` has `tail` more words behind the last slot.  `mom` is SGD's
    momentum buffer or Adam's `exp_avg`; a store built with `sq_key` also has `sq`, Adam's `exp_avg_sq`."""

    def __init__(self, params, layout: FlatLayout, tail: int = 0, mom_key: str = "momentum_buffer", sq_key=None) -> None:
        dev = params[0].device
        self.params, self.layout = list(params), layout
        self.mom_key, self.sq_key = mom_key, sq_key                # the `state[p]` entries that `mom` and `sq` are the storage of
        self.param = torch.zeros(layout.total, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(layout.total + tail, device=dev, dtype=torch.float32)
        self.mom = torch.zeros(layout.total, device=dev, dtype=torch.float32)
        self.grad_views, self.mom_views = layout.views(self.grad), layout.views(self.mom)
        self.sq = self.sq_views = None                             # Adam's second moment: only a store given `sq_key` has one
        if sq_key is not None:
            self.sq = torch.zeros(layout.total, device=dev, dtype=torch.float32)
            self.sq_views = layout.views(self.sq)
        self.ema = self.ema_views = None                           # the weight EMA, with the parameters' layout (`make_ema`)
        self.ema_live = False                                      # a step has updated it, or a checkpoint brought it
        with torch.no_grad():
            for p, view in zip(self.params, layout.views(self.param)):
                view.copy_(p.data)
                p.data = view
        self.ptrs = [p.data_ptr() for p in self.params]

    def seated(self, params) -> bool:
        return len(params) == len(self.ptrs) and all(p.data_ptr() == q for p, q in zip(params, self.ptrs))

    def adopt(self, state) -> None:
        """Take over what a checkpoint (or the store these parameters lived in before) left in the optimizer's `state`: momentum
        buffers (or Adam's moments) are copied into `mom` (and `sq`) and replaced by their views, and so are the averages, if there
        are any."""
        with torch.no_grad():
            for key, views in ((self.mom_key, self.mom_views), (self.sq_key, self.sq_views)):
                if key is None:
                    continue
                for p, mv in zip(self.params, views):
                    have = state.get(p, {}).get(key)
                    if have is not None:
                        mv.copy_(have.to(mv.device, torch.float32).reshape(mv.shape))
                        state[p][key] = mv
        emas = [state.get(p, {}).get("ema") for p in self.params]
        if self.ema is not None or any(e is not None for e in emas):
            self.make_ema(state, emas)

    def make_ema(self, state, restored=None) -> None:
        """The EMA buffer: a copy of the parameters, except where `restored` (one entry per parameter, or None) brings an average;
        `state[p]['ema']` become its views."""
        with torch.no_grad():
            if self.ema is None:
                self.ema = self.param.clone()
                self.ema_views = self.layout.views(self.ema)
            for i, (p, ev) in enumerate(zip(self.params, self.ema_views)):
                if restored is not None and restored[i] is not None:
                    ev.copy_(restored[i].to(ev.device, torch.float32).reshape(ev.shape))
                    self.ema_live = True
                state[p]["ema"] = ev

    def start_ema(self, state) -> None:
        """Called by the step that is about to update the EMA: the average starts as a copy of the parameters AT THE FIRST STEP, so a
        buffer that `ema_parameters()` / `ema_weights()` made earlier is copied again -- the parameters may have been loaded since."""
        if self.ema is None:
            self.make_ema(state)
        elif not self.ema_live:
            self.ema.copy_(self.param)
        self.ema_live = True


class AdamStateMixin:
    """The Adam state block of `optim.Adam` / `optim.AdamW` and of `ddp.FlatSGDDataParallel(optimizer="adam" | "adamw")`: ONE step
    counter and ONE pair of running products beta1^t, beta2^t per optimizer, on the device (include/ssd_gfx950.h, ssd_adam_advance).
    `adam_steps` is a view of the counter and never synchronises."""

    def _init_adam(self) -> None:
        self._adam_state = None           # f64[3]: pow1, pow2, step
        self._adam_start = (0, 1.0, 1.0)  # what a restored checkpoint starts the block from, until it exists

    @staticmethod
    def _adam_betas(groups):
        """The one pair of betas of all groups: the running products are per optimizer, as the counter is."""
        betas = {(float(g["betas"][0]), float(g["betas"][1])) for g in groups}
        if len(betas) != 1:
            raise ValueError(f"Adam: every parameter group must have the same betas (one step counter and one pair of running "
                             f"products per optimizer), got {sorted(betas)}")
        b1, b2 = next(iter(betas))
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"Adam: betas must be in [0, 1), got {(b1, b2)}")
        return b1, b2

    def _adam_buffers(self, dev) -> None:
        """The block, made outside any capture."""
        if self._adam_state is None or self._adam_state.device != dev:
            if self._adam_state is not None:
                words = self._adam_state.cpu()
                self._adam_start = (int(words.view(torch.int32)[4]), float(words[0]), float(words[1]))
            self._adam_state = ops.adam_state(dev, *self._adam_start)

    def _adam_restore(self, t: int, beta1: float, beta2: float) -> None:
        """A checkpoint's step count: the products are rebuilt by the t multiplications the device would have done (Python floats
        are IEEE f64), and written INTO the block when it exists, so a captured step keeps reading the right memory."""
        pow1 = pow2 = 1.0
        for _ in range(int(t)):
            pow1, pow2 = pow1 * beta1, pow2 * beta2
        self._adam_start = (int(t), pow1, pow2)
        if self._adam_state is not None:
            self._adam_state.copy_(ops.adam_state("cpu", *self._adam_start))

    def _adam_step_host(self) -> int:
        """The counter, read back: the one synchronisation (checkpoints)."""
        return int(ops.adam_state_step(self._adam_state).item()) if self._adam_state is not None else int(self._adam_start[0])

    @property
    def adam_steps(self):
        """0-dim int32 device tensor: Adam steps actually taken (skipped steps do not count); None before the first step."""
        return None if self._adam_state is None else ops.adam_state_step(self._adam_state)


def check_adam_settings(name, lr, betas, eps, weight_decay, amsgrad, maximize, differentiable) -> None:
    if amsgrad or maximize or differentiable:
        raise ValueError(f"{name}: amsgrad / maximize / differentiable are not implemented")
    if isinstance(lr, torch.Tensor) or not lr >= 0.0:
        raise ValueError(f"{name}: lr must be a non-negative number, got {lr!r}")
    if len(betas) != 2 or not all(0.0 <= float(b) < 1.0 for b in betas):
        raise ValueError(f"{name}: betas must be two numbers in [0, 1), got {betas!r}")
    if not eps >= 0.0 or not weight_decay >= 0.0:
        raise ValueError(f"{name}: eps and weight_decay must be non-negative")


class FlatGroupOptimizer(FusedStepMixin, torch.optim.Optimizer):
    """What `SGD`, `Adam` and `AdamW` share: one `FlatStore` per parameter group, seated the first time a step (or the EMA's
    accessors) sees the group, the EMA's accessors, and how a step turns the groups' gradients into launch ranges (`_gather`) and
    the device words the launches read (`_controls`).  A subclass names the `state[p]` entries its store's `mom` / `sq` buffers
    are (`_MOM_KEY`, `_SQ_KEY`) and writes `step()`."""

    _MOM_KEY, _SQ_KEY = "momentum_buffer", None

    def __init__(self, params, defaults, max_grad_norm, norm_type, skip_nonfinite, schedule, ema_decay, ema_warmup) -> None:
        self._init_clip(max_grad_norm, norm_type, skip_nonfinite)
        self._init_sched(schedule, ema_decay, ema_warmup)
        super().__init__(params, defaults)
        self._buffers: List[FlatStore | None] = [None] * len(self.param_groups)       # one store per parameter group

    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        if hasattr(self, "_buffers"):
            self._buffers.append(None)

    def _seat_all(self) -> None:
        for gi, group in enumerate(self.param_groups):
            if group["params"]:
                buf = self._group_buffers(gi, group["params"])
                if buf.ema is None:
                    buf.make_ema(self.state)

    def ema_parameters(self):
        """The averaged weights, one tensor per parameter in `param_groups` order: views of the flat EMA buffers (a copy of the
        parameters until the first step with `ema_decay` set)."""
        self._seat_all()
        for group in self.param_groups:
            for p in group["params"]:
                yield self.state[p]["ema"]

    @contextlib.contextmanager
    def ema_weights(self):
        """Evaluate with the averaged weights: parameters and EMA change places, in place, on entry and again on exit."""
        self._seat_all()
        self._swap_ema()
        try:
            yield self
        finally:
            self._swap_ema()

    def _swap_ema(self) -> None:
        for buf, group in zip(self._buffers, self.param_groups):
            if buf is None:
                continue
            ops.swap_f32_(buf.param, buf.ema)
            for p in group["params"]:
                torch.autograd.graph.increment_version(p)         # as a step does: invalidate re-laid weight caches

    def _group_buffers(self, gi: int, params) -> FlatStore:
        buf = self._buffers[gi]
        if buf is None or not buf.seated(params):                 # first step, or the caller moved / replaced the tensors
            for p in params:
                if p.dtype != torch.float32 or p.device.type != "cuda" or not p.is_contiguous():
                    raise ValueError(f"{type(self).__name__}: parameters must be contiguous float32 tensors on the GPU")
            buf = self._buffers[gi] = FlatStore(params, FlatLayout(params), mom_key=self._MOM_KEY, sq_key=self._SQ_KEY)
            buf.adopt(self.state)                                 # restored momentum / moment and EMA buffers
        return buf

    def _gather(self, fresh_of=None):
        """-> [(gi, group, store, runs)] for every group with a gradient, the gradients copied into the stores' flat buffers.
        Parameters without a gradient are skipped, as torch skips them: maximal runs [lo, hi, fresh] of neighbouring parameters in
        the same situation are one launch (the whole group, in the reference's loop); `fresh_of(group, p)` tells the situations
        apart (SGD: the momentum buffer starts at this step), None: there is one."""
        pending = []
        for gi, group in enumerate(self.param_groups):
            params = group["params"]
            if not params:
                continue
            buf = self._group_buffers(gi, params)
            runs, cur = [], None
            for i, p in enumerate(params):
                if p.grad is None:
                    cur = None
                    continue
                if p.grad.is_sparse:
                    raise ValueError(f"{type(self).__name__}: sparse gradients are not supported")
                fresh = bool(fresh_of(group, p)) if fresh_of is not None else False
                if cur is not None and cur[2] == fresh:
                    cur[1] = i + 1
                else:
                    cur = [i, i + 1, fresh]
                    runs.append(cur)
            have = [i for i, p in enumerate(params) if p.grad is not None]
            if not have:
                continue
            torch._foreach_copy_([buf.grad_views[i] for i in have], [params[i].grad for i in have])
            pending.append((gi, group, buf, runs))
        return pending

    def _controls(self, pending):
        """ONE norm over the runs the launches cover (slots of parameters without a gradient hold stale data and are in no run),
        then ONE schedule advance -> `_step_controls`' device words."""
        ranges = [buf.grad[buf.layout.span(lo, hi)] for _, _, buf, runs in pending for lo, hi, _ in runs]
        if self._clip_on():
            self._clip_buffers(ranges[0].device, sum(ops.grad_norm_slots(r.numel()) for r in ranges))
        if self._sched_on():
            self._sched_buffers(ranges[0].device)
        return self._step_controls(ranges)


class SGD(FlatGroupOptimizer):
    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0,
                 nesterov: bool = False, *, maximize: bool = False, foreach=None, differentiable: bool = False, fused=None,
                 max_grad_norm=None, norm_type=2.0, skip_nonfinite: bool = False, schedule=None, ema_decay=None,
                 ema_warmup: bool = True):
        """max_grad_norm: clip the GLOBAL norm (`norm_type` 2 or inf) of every gradient of every group to it, as
        `torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm, norm_type)` before `step()` does.  skip_nonfinite: a step whose
        gradient norm is Inf or NaN changes neither parameters nor momentum and counts into `skipped_steps`.

        schedule: an `LRSchedule`; step t runs group g at float32(group['lr'] * schedule.factors[t]) read from a device table, the
        groups' 'lr' stay the base rates.  ema_decay (in (0, 1)): keep an exponential moving average of every parameter,
        e += (1 - d_t) * (p - e) after each step, d_t = min(ema_decay, (1 + t) / (10 + t)) with `ema_warmup`, else ema_decay;
        `state[p]['ema']`, `ema_parameters()` and `ema_weights()` reach it.  A parameter takes part in the steps it has a gradient in."""
        check_clip_settings(max_grad_norm, norm_type, skip_nonfinite)
        check_sched_settings(schedule, ema_decay, ema_warmup)
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError("SGD: lr, momentum and weight_decay must be non-negative")
        if dampening != 0.0 or nesterov or maximize or differentiable:
            raise ValueError("SGD: dampening / nesterov / maximize / differentiable are not part of the reference's step "
                             "(train.py:53-55) and are not implemented")
        defaults = dict(lr=lr, momentum=momentum, dampening=0.0, weight_decay=weight_decay, nesterov=False, maximize=False,
                        foreach=foreach, differentiable=False, fused=fused)
        super().__init__(params, defaults, max_grad_norm, norm_type, skip_nonfinite, schedule, ema_decay, ema_warmup)

    def state_dict(self):
        """torch's layout; with the schedule or the EMA on, every group also carries `sched_step`, the device step counter (reading it
        is the one synchronisation), and `state[p]['ema']` travels with the momentum buffers."""
        return self._sched_stamp(super().state_dict())

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        self._buffers = [None] * len(self.param_groups)           # restored momentum and EMA buffers are re-seated at the next step
        self._sched_unstamp()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        sched = self._sched_on()
        self._clip_on()
        for group in self.param_groups:
            if group["dampening"] != 0 or group["nesterov"] or group.get("maximize", False):
                raise ValueError("SGD: dampening / nesterov / maximize are not implemented")
        # torch starts a momentum buffer at the first gradient it sees: such parameters are launches of their own
        pending = self._gather(lambda group, p: group["momentum"] != 0 and self.state[p].get("momentum_buffer") is None)
        if not pending:
            return loss
        grad_scale, skip, lr_words, ema_w = self._controls(pending)
        for gi, group, buf, runs in pending:
            lr, mom, wd = float(group["lr"]), float(group["momentum"]), float(group["weight_decay"])
            if self.ema_decay is not None:
                buf.start_ema(self.state)
            for lo, hi, fresh in runs:
                span = buf.layout.span(lo, hi)
                # momentum 0: torch keeps no buffer and steps with the gradient itself = the "first step" form of the kernel
                launch_sgd(buf.param[span], buf.grad[span], buf.mom[span], lr=lr, lr_dev=lr_words[gi:gi + 1] if sched else None,
                           ema=buf.ema[span] if self.ema_decay is not None else None, ema_w=ema_w, momentum=mom, weight_decay=wd,
                           grad_scale=grad_scale, first=fresh or mom == 0.0, skip=skip)
                for i in range(lo, hi):
                    p = buf.params[i]
                    if mom != 0.0 and fresh:
                        # (a skipped first step leaves the buffer at zero: momentum * 0 + g is the first-step form in value)
                        self.state[p]["momentum_buffer"] = buf.mom_views[i]
                    torch.autograd.graph.increment_version(p)     # written outside autograd: invalidate re-laid weight caches
        return loss


class Adam(AdamStateMixin, FlatGroupOptimizer):
    """`torch.optim.Adam` (L2 weight decay; `decoupled_weight_decay=True` makes it AdamW) on the flat stores and the step sequence
    of `optim.SGD`: `ssd_adam_step` (include/ssd_gfx950.h) once per run of neighbouring parameters with a gradient, the first
    moments in the stores' `mom` buffers, the second in `sq`.  Same constructor and param-group keys as torch's, same
    `state[p] = {'step', 'exp_avg', 'exp_avg_sq'}` entries, so checkpoints move between the two; `exp_avg` and `exp_avg_sq`
    follow torch's rounding sequence bit for bit (foreach=False), the parameter follows the sequence documented in the header.

    The one deliberate departure from torch: the step counter is ONE device word per optimizer, not one per parameter.  A parameter
    without a gradient is left out of that step's launches and its moments stay untouched, as in torch, but when it takes part again
    its bias correction follows the optimizer's counter, where torch's would follow the number of steps that parameter itself has
    taken.  For the same reason every group has the same betas, and `load_state_dict` refuses per-parameter steps that disagree.
    `state[p]['step']` is brought up to date by `state_dict()`, which reads the counter back (the one synchronisation).

    max_grad_norm / norm_type / skip_nonfinite / schedule / ema_decay / ema_warmup: exactly as in `optim.SGD`; a skipped step
    advances neither counter.  Without a schedule and without the EMA the step size comes from the f64 `group['lr']`, as torch's
    does; with either it comes from the f32 device word of the schedule block."""

    _MOM_KEY, _SQ_KEY = "exp_avg", "exp_avg_sq"
    _DECOUPLED = False

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 amsgrad: bool = False, *, foreach=None, maximize: bool = False, capturable: bool = False,
                 differentiable: bool = False, fused=None, decoupled_weight_decay: bool = False, max_grad_norm=None, norm_type=2.0,
                 skip_nonfinite: bool = False, schedule=None, ema_decay=None, ema_warmup: bool = True):
        name = type(self).__name__
        check_clip_settings(max_grad_norm, norm_type, skip_nonfinite)
        check_sched_settings(schedule, ema_decay, ema_warmup)
        check_adam_settings(name, lr, betas, eps, weight_decay, amsgrad, maximize, differentiable)
        self._init_adam()
        defaults = dict(lr=lr, betas=(betas[0], betas[1]), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=foreach, capturable=capturable, differentiable=False, fused=fused,
                        decoupled_weight_decay=bool(decoupled_weight_decay) or self._DECOUPLED)
        super().__init__(params, defaults, max_grad_norm, norm_type, skip_nonfinite, schedule, ema_decay, ema_warmup)

    def state_dict(self):
        """torch's layout: `state[p] = {'step' (0-dim f32, the optimizer's counter), 'exp_avg', 'exp_avg_sq'}` plus `'ema'` when
        there is one, torch's param-group keys, and `sched_step` with the schedule or the EMA on, as `optim.SGD` carries it."""
        t = self._adam_step_host()
        for st in self.state.values():
            if "exp_avg" in st:
                st["step"] = torch.tensor(float(t), dtype=torch.float32)
        return self._sched_stamp(super().state_dict())

    def load_state_dict(self, state_dict) -> None:
        """Both moments are re-seated into the stores at the next step; the running products are rebuilt from the step count by the
        multiplications the device would have done, so a resumed run continues bit for bit."""
        steps = {float(st["step"]) for st in state_dict["state"].values() if "step" in st}
        if len(steps) > 1:
            raise ValueError(f"{type(self).__name__}.load_state_dict: the parameters' step counts disagree ({sorted(steps)}); the "
                             "step counter here is one per optimizer")
        t = steps.pop() if steps else 0.0
        if t != int(t) or t < 0:
            raise ValueError(f"{type(self).__name__}.load_state_dict: step count {t!r}")
        super().load_state_dict(state_dict)
        self._buffers = [None] * len(self.param_groups)
        self._sched_unstamp()
        self._adam_restore(int(t), *self._adam_betas(self.param_groups))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        sched = self._sched_on()
        self._clip_on()
        for group in self.param_groups:
            check_adam_settings(type(self).__name__, group["lr"], group["betas"], group["eps"], group["weight_decay"],
                                group.get("amsgrad", False), group.get("maximize", False), group.get("differentiable", False))
        beta1, beta2 = self._adam_betas(self.param_groups)
        pending = self._gather()
        if not pending:
            return loss
        grad_scale, skip, lr_words, ema_w = self._controls(pending)
        self._adam_buffers(pending[0][2].param.device)
        ops.adam_advance_(self._adam_state, beta1, beta2, skip if self.skip_nonfinite else None)
        for gi, group, buf, runs in pending:
            if self.ema_decay is not None:
                buf.start_ema(self.state)
            for lo, hi, _ in runs:
                span = buf.layout.span(lo, hi)
                ops.adam_step_(buf.param[span], buf.grad[span], buf.mom[span], buf.sq[span],
                               buf.ema[span] if self.ema_decay is not None else None, float(group["lr"]),
                               lr_words[gi:gi + 1] if sched else None, ema_w, self._adam_state, beta1, beta2, float(group["eps"]),
                               float(group["weight_decay"]), bool(group.get("decoupled_weight_decay", self._DECOUPLED)), grad_scale, skip)
                for i in range(lo, hi):
                    p = buf.params[i]
                    st = self.state[p]
                    if "exp_avg" not in st:                       # torch's entries; zero moments are Adam's own start
                        st["step"] = torch.tensor(0.0, dtype=torch.float32)
                        st["exp_avg"], st["exp_avg_sq"] = buf.mom_views[i], buf.sq_views[i]
                    torch.autograd.graph.increment_version(p)     # written outside autograd: invalidate re-laid weight caches
        return loss


class AdamW(Adam):
    """`torch.optim.AdamW`: `optim.Adam` with decoupled weight decay, p <- p * float32(1 - lr * weight_decay) before the step."""

    _DECOUPLED = True

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False, *, maximize: bool = False, foreach=None, capturable: bool = False,
                 differentiable: bool = False, fused=None, max_grad_norm=None, norm_type=2.0, skip_nonfinite: bool = False,
                 schedule=None, ema_decay=None, ema_warmup: bool = True):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize, capturable=capturable,
                         differentiable=differentiable, fused=fused, decoupled_weight_decay=True, max_grad_norm=max_grad_norm,
                         norm_type=norm_type, skip_nonfinite=skip_nonfinite, schedule=schedule, ema_decay=ema_decay,
                         ema_warmup=ema_warmup)

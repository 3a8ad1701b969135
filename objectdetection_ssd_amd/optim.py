"""`torch.optim.SGD` for the step that follows the hot path, as one fused launch per parameter group.

The reference builds its optimizer as (train.py:44-55)

    torch.optim.SGD(params=[{'params': biases, 'lr': 2*lr}, {'params': not_biases}], lr=lr, momentum=0.9, weight_decay=5e-4)

and `train_function.py` then uses `.zero_grad()`, `.step()`, `.param_groups[*]['lr']`, `.state_dict()` and
`.load_state_dict()` (train_function.py:8-9,27-30,76,95,116).  `SGD` here keeps all of that -- same constructor, same
param-group keys, same `state[p]['momentum_buffer']` entries, so checkpoints move between the two -- and runs
`ssd_sgd_momentum` (include/ssd_gfx950.h) once per group on flat storage: each group's parameters and momentum buffers
are re-seated as views of one buffer the first time `step()` sees them, gradients are gathered with one foreach copy.
The kernel reproduces torch's rounding sequence, so the parameters after k steps are bit-identical to torch.optim.SGD's.

Only what the reference uses is implemented: `dampening`, `nesterov`, `maximize` must stay at their defaults.  GPU only,
like the rest of the package.

Gradient clipping and the non-finite step guard (`max_grad_norm`, `norm_type`, `skip_nonfinite`) are what a user of that loop
adds with `torch.nn.utils.clip_grad_norm_` between `backward()` and `step()`: here they are one norm pass per launch range, one
finalise launch and the guarded form of the same SGD kernel, and nothing comes back to the host (`GradClipMixin`).
"""
from __future__ import annotations

import math
from typing import List

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

    def _clip_run(self, ranges, pre_scale):
        """Norm of the flat f32 ranges (one partials launch each), one finalise -> (grad_scale, skip): the device words the guarded
        SGD launches read."""
        s = 0
        for r in ranges:
            s = ops.grad_norm_partials_(r, self._clip_partials, s, self.norm_type)
        ops.grad_clip_finalize_(self._clip_partials, s, self.norm_type, self.max_grad_norm, pre_scale, self.skip_nonfinite,
                                self._clip_state)
        return self._clip_state[2:3], self._clip_state.view(torch.int32)[3:4]

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


class _GroupBuffers:
    """Flat storage of one parameter group."""

    def __init__(self, params: List[torch.nn.Parameter], state) -> None:
        dev = params[0].device
        sizes = [p.numel() for p in params]
        slots = [(s + 3) // 4 * 4 for s in sizes]                  # every parameter starts 16-byte aligned
        self.offsets, off = [], 0
        for s in slots:
            self.offsets.append(off)
            off += s
        self.total = off
        self.sizes = sizes
        self.param = torch.zeros(off, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(off, device=dev, dtype=torch.float32)
        self.mom = torch.zeros(off, device=dev, dtype=torch.float32)
        self.grad_views = []
        with torch.no_grad():
            for p, o, sz in zip(params, self.offsets, sizes):
                view = self.param[o:o + sz].view_as(p)
                view.copy_(p.data)
                p.data = view
                self.grad_views.append(self.grad[o:o + sz].view_as(p))
                st = state.get(p)
                if st is not None and st.get("momentum_buffer") is not None:
                    mv = self.mom[o:o + sz].view_as(p)
                    mv.copy_(st["momentum_buffer"])
                    st["momentum_buffer"] = mv
        self.ptrs = [p.data_ptr() for p in params]

    def seated(self, params) -> bool:
        return len(params) == len(self.ptrs) and all(p.data_ptr() == q for p, q in zip(params, self.ptrs))


class SGD(GradClipMixin, torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0, weight_decay: float = 0.0,
                 nesterov: bool = False, *, maximize: bool = False, foreach=None, differentiable: bool = False, fused=None,
                 max_grad_norm=None, norm_type=2.0, skip_nonfinite: bool = False):
        """max_grad_norm: clip the GLOBAL norm (`norm_type` 2 or inf) of every gradient of every group to it, as
        `torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm, norm_type)` before `step()` does.  skip_nonfinite: a step whose
        gradient norm is Inf or NaN changes neither parameters nor momentum and counts into `skipped_steps`."""
        self._init_clip(max_grad_norm, norm_type, skip_nonfinite)
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError("SGD: lr, momentum and weight_decay must be non-negative")
        if dampening != 0.0 or nesterov or maximize or differentiable:
            raise ValueError("SGD: dampening / nesterov / maximize / differentiable are not part of the reference's step "
                             "(train.py:53-55) and are not implemented")
        defaults = dict(lr=lr, momentum=momentum, dampening=0.0, weight_decay=weight_decay, nesterov=False, maximize=False,
                        foreach=foreach, differentiable=False, fused=fused)
        super().__init__(params, defaults)
        self._buffers: List[_GroupBuffers | None] = [None] * len(self.param_groups)

    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        if hasattr(self, "_buffers"):
            self._buffers.append(None)

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        self._buffers = [None] * len(self.param_groups)           # restored momentum buffers are re-seated at the next step

    def _group_buffers(self, gi: int, params) -> _GroupBuffers:
        buf = self._buffers[gi]
        if buf is None or not buf.seated(params):                 # first step, or the caller moved / replaced the tensors
            for p in params:
                if p.dtype != torch.float32 or p.device.type != "cuda" or not p.is_contiguous():
                    raise ValueError("SGD: parameters must be contiguous float32 tensors on the GPU")
            buf = self._buffers[gi] = _GroupBuffers(params, self.state)
        return buf

    def _launch_runs(self, buf, params, runs, lr, mom, wd, grad_scale, skip) -> None:
        for lo, hi, fresh in runs:
            a = buf.offsets[lo]
            b = buf.offsets[hi - 1] + (buf.sizes[hi - 1] + 3) // 4 * 4
            # momentum 0: torch keeps no buffer and steps with the gradient itself = the "first step" form of the kernel
            if skip is None:
                ops.sgd_momentum_(buf.param[a:b], buf.grad[a:b], buf.mom[a:b], lr, mom, wd, None, fresh or mom == 0.0)
            else:
                ops.sgd_momentum_guarded_(buf.param[a:b], buf.grad[a:b], buf.mom[a:b], lr, mom, wd, grad_scale, fresh or mom == 0.0, skip)
            for i in range(lo, hi):
                p = params[i]
                if mom != 0.0 and fresh:
                    # (a skipped first step leaves the buffer at zero: momentum * 0 + g is the first-step form in value)
                    o, sz = buf.offsets[i], buf.sizes[i]
                    self.state[p]["momentum_buffer"] = buf.mom[o:o + sz].view_as(p)
                torch.autograd.graph.increment_version(p)     # written outside autograd: invalidate re-laid weight caches

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        clip = self._clip_on()
        pending = []                                              # clipping: every group's runs wait for the one global norm
        for gi, group in enumerate(self.param_groups):
            if group["dampening"] != 0 or group["nesterov"] or group.get("maximize", False):
                raise ValueError("SGD: dampening / nesterov / maximize are not implemented")
            params = group["params"]
            if not params:
                continue
            buf = self._group_buffers(gi, params)
            lr, mom, wd = float(group["lr"]), float(group["momentum"]), float(group["weight_decay"])
            # torch skips parameters without a gradient and starts a momentum buffer at the first gradient it sees: maximal runs of
            # neighbouring parameters in the same situation are one launch (the whole group, in the reference's loop)
            runs, cur = [], None
            for i, p in enumerate(params):
                if p.grad is None:
                    cur = None
                    continue
                if p.grad.is_sparse:
                    raise ValueError("SGD: sparse gradients are not supported")
                fresh = mom != 0.0 and self.state[p].get("momentum_buffer") is None
                if cur is not None and cur[2] == fresh:
                    cur[1] = i + 1
                else:
                    cur = [i, i + 1, fresh]
                    runs.append(cur)
            have = [i for i, p in enumerate(params) if p.grad is not None]
            if not have:
                continue
            torch._foreach_copy_([buf.grad_views[i] for i in have], [params[i].grad for i in have])
            if clip:
                pending.append((buf, params, runs, lr, mom, wd))
            else:
                self._launch_runs(buf, params, runs, lr, mom, wd, None, None)
        if pending:
            # ONE norm over the runs the SGD launches cover: slots of parameters without a gradient hold stale data and are in no run
            ranges = []
            for buf, _, runs, *_ in pending:
                for lo, hi, _ in runs:
                    ranges.append(buf.grad[buf.offsets[lo]:buf.offsets[hi - 1] + (buf.sizes[hi - 1] + 3) // 4 * 4])
            self._clip_buffers(ranges[0].device, sum(ops.grad_norm_slots(r.numel()) for r in ranges))
            grad_scale, skip = self._clip_run(ranges, None)
            for work in pending:
                self._launch_runs(*work, grad_scale, skip)
        return loss

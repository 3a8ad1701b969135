"""numpy restatement of the device-resident learning-rate schedule and the weight EMA (include/ssd_gfx950.h,
ssd_sgd_schedule_advance / ssd_sgd_momentum_sched): the f64 factor tables, the f32 table rows the device reads, the EMA weight
of a step and the three-rounding EMA update.  Written from the formulas, not from optim.LRSchedule; held against torch's own
schedulers and AveragedModel on CPU tensors in tests/test_sched_ema_cpu.py."""
import math

import numpy as np

F32 = np.float32


def warm(t, warmup_steps=0, warmup_start=0.1):
    """Linear warm-up factor (torch's LinearLR(start_factor, 1.0, warmup_steps) in closed form)."""
    if t >= warmup_steps:
        return 1.0
    return warmup_start + (1.0 - warmup_start) * t / warmup_steps


def _table(decay, steps, warmup_steps, warmup_start):
    steps = max(steps, warmup_steps)
    return np.array([warm(t, warmup_steps, warmup_start) * decay(t) for t in range(steps + 1)], np.float64)


def constant(warmup_steps=0, warmup_start=0.1):
    return _table(lambda t: 1.0, 0, warmup_steps, warmup_start)


def multistep(milestones, gamma=0.1, total_steps=None, warmup_steps=0, warmup_start=0.1):
    """MultiStepLR: one multiplication by gamma per milestone reached."""
    ms = sorted(milestones)
    last = max(ms + [0])

    def decay(t):
        f = 1.0
        for m in ms:
            if m <= t:
                f = f * gamma
        return f
    return _table(decay, last if total_steps is None else total_steps, warmup_steps, warmup_start)


def cosine(total_steps, min_factor=0.0, warmup_steps=0, warmup_start=0.1):
    """CosineAnnealingLR(T_max=total_steps) in closed form up to total_steps; the table ends there, so min_factor holds afterwards."""
    return _table(lambda t: min_factor + (1.0 - min_factor) * 0.5 * (1.0 + math.cos(math.pi * min(t, total_steps) / total_steps)),
                  total_steps, warmup_steps, warmup_start)


def poly(total_steps, power=1.0, warmup_steps=0, warmup_start=0.1):
    """PolynomialLR(total_iters=total_steps, power) in closed form."""
    return _table(lambda t: (1.0 - min(t, total_steps) / total_steps) ** power, total_steps, warmup_steps, warmup_start)


def table_row(base_lr, factors):
    """Group row of the device table: float32(float64(base_lr) * factors[t]), one rounding."""
    return (np.float64(base_lr) * np.asarray(factors, np.float64)).astype(F32)


def lr_at(row, t):
    """The rate of step t: past the end of the table the last entry holds."""
    return F32(row[min(t, len(row) - 1)])


def ema_w(t, decay, warmup=True):
    """EMA weight of step t: 1 - d_t in f64 (add, subtract, divide only), rounded once to f32.  decay None: no EMA, weight 0."""
    if decay is None:
        return F32(0.0)
    d = np.float64(decay)
    if warmup:
        d = min(d, (np.float64(1.0) + np.float64(t)) / (np.float64(10.0) + np.float64(t)))
    return F32(np.float64(1.0) - d)


def ema_update(e, p, w):
    """e + w * (p - e) in f32, three separately rounded operations."""
    e, p, w = np.asarray(e, F32), np.asarray(p, F32), F32(w)
    d = (p - e).astype(F32)
    m = (w * d).astype(F32)
    return (e + m).astype(F32)


def ulps(a, b):
    """Distance of two finite f32 values in units in the last place (0 = the same bits, up to the sign of zero)."""
    def key(v):
        i = int(np.asarray(v, F32).reshape(1).view(np.int32)[0])
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return abs(key(a) - key(b))

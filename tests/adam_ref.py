"""numpy restatement of the fused Adam / AdamW step (include/ssd_gfx950.h, ssd_adam_advance / ssd_adam_step): the state block with
its running products, and one step over flat f32 arrays in the documented rounding sequence.  Every fused multiply-add is formed as
an f64 product (exact for f32 factors) plus the addend in f64, rounded once to f32.  Written from the formulas, not from the
package; held against torch.optim.Adam / AdamW on CPU tensors in tests/test_adam_cpu.py, and the only source of expected values of
the GPU tests."""
import numpy as np

F32 = np.float32
F64 = np.float64


def fma(a, b, c):
    """a * b + c with one rounding to f32: the product of two f32 is exact in f64."""
    return (np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64) + np.asarray(c, F32).astype(F64)).astype(F32)


class State:
    """The Adam state block: step counter and the running products beta1^t, beta2^t (f64, one IEEE multiply per step)."""

    def __init__(self, step=0, pow1=1.0, pow2=1.0):
        self.step, self.pow1, self.pow2 = int(step), F64(pow1), F64(pow2)

    @classmethod
    def at(cls, t, beta1, beta2):
        """The block after t advances from the start: what a restored checkpoint rebuilds."""
        s = cls()
        for _ in range(int(t)):
            s.advance(beta1, beta2)
        return s

    def advance(self, beta1, beta2, skip=0):
        if skip:
            return self
        self.step += 1
        self.pow1 = F64(self.pow1 * F64(beta1))
        self.pow2 = F64(self.pow2 * F64(beta2))
        return self

    def words(self):
        """The block as the device holds it: 3 x 8 bytes."""
        out = np.zeros(3, F64)
        out[0], out[1] = self.pow1, self.pow2
        out.view(np.int32)[4] = self.step
        return out


def step_size(lr, pow1):
    """f32(-(lr / (1 - pow1))): f64 throughout, one rounding."""
    return F32(-(F64(lr) / (F64(1.0) - F64(pow1))))


def bc2_sqrt(pow2):
    return F32(np.sqrt(F64(1.0) - F64(pow2)))


def step(p, g, m, v, state, *, lr, betas, eps, weight_decay, decoupled, grad_scale=None, ema=None, ema_w=None, skip=0):
    """One launch: -> (p, m, v, ema) as new arrays.  `lr` is the f64 host rate or an f32 device word (np.float32), which widens
    exactly; `state` has been advanced for this step.  skip: everything comes back unchanged."""
    p, g, m, v = (np.array(a, F32) for a in (p, g, m, v))
    e = None if ema is None else np.array(ema, F32)
    if skip:
        return p, m, v, e
    beta1, beta2 = F64(betas[0]), F64(betas[1])
    rate, wd = F64(lr), F64(weight_decay)
    omb1, omb2, b2 = F32(F64(1.0) - beta1), F32(F64(1.0) - beta2), F32(beta2)
    with np.errstate(all="ignore"):
        if grad_scale is not None:
            g = (g * F32(grad_scale)).astype(F32)
        if wd != 0:
            if decoupled:
                p = (p * F32(F64(1.0) - rate * wd)).astype(F32)
            else:
                g = fma(F32(wd), p, g)
        m = fma(omb1, (g - m).astype(F32), m)
        v = fma((omb2 * g).astype(F32), g, (v * b2).astype(F32))
        den = ((np.sqrt(v).astype(F32) / bc2_sqrt(state.pow2)).astype(F32) + F32(eps)).astype(F32)
        p = (p + ((step_size(rate, state.pow1) * m).astype(F32) / den).astype(F32)).astype(F32)
        if e is not None:
            d = (p - e).astype(F32)
            e = (e + (F32(ema_w) * d).astype(F32)).astype(F32)
    return p, m, v, e


def ulps(a, b):
    """Largest distance of two finite f32 arrays in units in the last place (0 = the same bits, up to the sign of zero)."""
    def key(x):
        i = np.asarray(x, F32).reshape(-1).view(np.int32).astype(np.int64)
        return np.where(i >= 0, i, -(i & 0x7FFFFFFF))
    d = np.abs(key(a) - key(b))
    return int(d.max()) if d.size else 0

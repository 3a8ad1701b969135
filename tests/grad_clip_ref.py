"""numpy restatement of gradient-norm clipping and the non-finite step guard (include/ssd_gfx950.h, ssd_grad_clip_finalize):
the global norm in f64, torch.nn.utils.clip_grad_norm_'s f32 coefficient sequence, the scale handed to the SGD kernel and the
skip decision.  Held against torch itself on CPU tensors in tests/test_grad_clip_cpu.py."""
import numpy as np

F32 = np.float32


def total_norm(arrays, norm_type=2.0, pre_scale=None):
    """f32 global norm of a list of arrays.  L2: the squares and their sum in f64 (an f32 squared is exact there), the root and the
    optional pre_scale in f64, ONE rounding to f32.  inf: max |g| (NaN if any element is NaN), times pre_scale in f32."""
    flat = [np.asarray(a, F32).reshape(-1) for a in arrays]
    with np.errstate(all="ignore"):
        if norm_type == 2:
            s = np.float64(0.0)
            for a in flat:
                a64 = a.astype(np.float64)
                s = s + np.sum(a64 * a64, dtype=np.float64)
            t = np.sqrt(s)
            if pre_scale is not None:
                t = t * np.float64(F32(pre_scale))
            return F32(t)
        if norm_type == float("inf"):
            m = F32(0.0)
            for a in flat:
                if a.size:
                    if np.isnan(a).any():
                        m = F32(np.nan)
                        break
                    m = max(m, F32(np.max(np.abs(a))))
            return m if pre_scale is None else F32(m * F32(pre_scale))
    raise ValueError(norm_type)


def clip_coef(norm, max_norm):
    """clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1.0), every step in f32; clamp keeps a NaN.  None: no clipping.
    torch evaluates number / tensor as tensor.reciprocal() * number, so the quotient is rounded twice: 1 / (norm + 1e-6), then
    times max_norm."""
    if max_norm is None:
        return F32(1.0)
    with np.errstate(all="ignore"):
        c = F32(F32(F32(1.0) / F32(F32(norm) + F32(1e-6))) * F32(max_norm))
    return F32(1.0) if c > F32(1.0) else c


def grad_scale(coef, pre_scale=None):
    with np.errstate(all="ignore"):
        return F32(coef) if pre_scale is None else F32(F32(pre_scale) * F32(coef))


def skips(norm, guard):
    return bool(guard) and not bool(np.isfinite(F32(norm)))


def ulps(a, b):
    """Distance of two finite f32 values in units in the last place (0 = the same bits, up to the sign of zero)."""
    def key(v):
        i = int(np.asarray(v, F32).reshape(1).view(np.int32)[0])
        return i if i >= 0 else -(i & 0x7FFFFFFF)
    return abs(key(a) - key(b))

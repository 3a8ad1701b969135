"""Plain numpy references for csrc/batchnorm.hip: the slab plan, the Philox4x32-10 dropout generator, f64 statistics / apply / backward,
the per-channel rounding bounds of the statistics, and integer data on which every f32 operation of apply and backward is exact.

Nothing here runs on a GPU or imports the package; the functions restate what the header comments of batchnorm.hip promise.
"""
import collections
import math

import numpy as np

U = 2.0 ** -24                       # unit roundoff of f32
THREADS, MAX_SLABS = 256, 1024

Plan = collections.namedtuple("Plan", "cgb lanes chunks rows nslab bytes")


def plan(M, C):
    """plan_for(M, C) restated, plus the workspace bytes: {mean, M2} (or the two sums) per slab and channel"""
    cg = C // 4
    cgb = min(cg, 64)
    lanes = THREADS // cgb
    chunks = -(-cg // cgb)
    rows = max(-(-M // MAX_SLABS), lanes * 16)
    nslab = -(-M // rows)
    return Plan(cgb, lanes, chunks, rows, nslab, nslab * C * 2 * 4)


# ---- dropout ----------------------------------------------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """numpy uint64 restatement of Philox4x32-10: ctr (4, n), key (2,) -> (4, n) uint32 words"""
    M = 0xFFFFFFFF
    c = [v.astype(np.uint64) for v in ctr]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(M)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(M)
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(0x9E3779B9)) & np.uint64(M)
        k1 = (k1 + np.uint64(0xBB67AE85)) & np.uint64(M)
    return c


def philox_keep(seed, site, n, p):
    """keep flags of dropout indices 0..n-1: word (i & 3) of philox({lo(i >> 2), hi(i >> 2), site, 0}, {lo(seed), hi(seed)}),
    kept iff (word >> 8) * 2^-24 < 1 - p, the difference taken in f32"""
    nq = -(-n // 4)
    q = np.arange(nq, dtype=np.uint64)                          # one Philox call serves the four indices 4q .. 4q+3
    ctr = [q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), np.full(nq, site, np.uint64), np.zeros(nq, np.uint64)]
    words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    w = np.stack(words, axis=1).reshape(-1)[:n]
    u = (w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return u < float(np.float32(1.0) - np.float32(p))


def drop_scale(p):
    """1/(1-p) as the entry forms it: p, 1 - p and the quotient each rounded to f32; 0 at p = 1"""
    p = np.float32(p)
    return float(np.float32(1.0) / (np.float32(1.0) - p)) if p < 1 else 0.0


def drop_factor(mode, p, seed, site, M, C, HW):
    """(M, C) f64 factors, 0 or 1/(1-p) (all 0 at p = 1, all 1 for mode 0).  Elementwise dropout (mode 1) indexes by row*C + c, per-sample
    dropout (mode 2) by (row // HW)*C + c."""
    if mode == 0:
        return np.ones((M, C))
    if mode == 1:
        keep = philox_keep(seed, site, M * C, p).reshape(M, C)
    else:
        assert mode == 2 and HW > 0 and M % HW == 0
        keep = np.repeat(philox_keep(seed, site, (M // HW) * C, p).reshape(M // HW, C), HW, axis=0)
    return keep.astype(np.float64) * drop_scale(p)


# ---- statistics -------------------------------------------------------------------------------------------------------------------
Stats = collections.namedtuple("Stats", "mean var M2 invstd scale shift running_mean running_var")


def _f32(v):
    return float(np.float32(v))


def stats_ref(x, gamma, beta, eps, momentum, rm, rv):
    """f64 training statistics of x (M, C).  eps and momentum are the f32 values the entry receives."""
    x = np.asarray(x, np.float64)
    M = x.shape[0]
    eps, momentum = _f32(eps), _f32(momentum)
    mean = x.mean(0)
    M2 = ((x - mean) ** 2).sum(0)
    var = M2 / M
    invstd = 1.0 / np.sqrt(var + eps)
    g = np.ones_like(mean) if gamma is None else np.asarray(gamma, np.float64)
    b = np.zeros_like(mean) if beta is None else np.asarray(beta, np.float64)
    scale = g * invstd
    shift = b - mean * scale
    new_rm = None if rm is None else (1.0 - momentum) * np.asarray(rm, np.float64) + momentum * mean
    new_rv = None if rv is None else (1.0 - momentum) * np.asarray(rv, np.float64) + momentum * (M2 / (M - 1))
    return Stats(mean, var, M2, invstd, scale, shift, new_rm, new_rv)


def stats_depth(pl):
    """the longest chain of dependent updates and merges: Welford steps of one thread, lane merges, strided slab merges, tree"""
    return -(-pl.rows // pl.lanes) + pl.lanes + -(-pl.nslab // 64) + 6


def stats_bars(x, pl, gamma=None, beta=None, eps=1e-5, momentum=0.1, rm=None, rv=None):
    """Per-channel first-order worst-case bounds on |f32 result - stats_ref| for every output of ssd_bn_train_stats, same fields as
    Stats.  Each chain step rounds at most a few times relative to max|x| (mean) or to M2 + max|x| * sum|x - mean| (M2); each later
    step adds the propagated bound and 4u of the magnitude of that step's own terms."""
    x = np.asarray(x, np.float64)
    M = x.shape[0]
    momentum = _f32(momentum)
    r = stats_ref(x, gamma, beta, eps, momentum, rm, rv)
    depth = stats_depth(pl)
    amax = np.abs(x).max(0)
    b_mean = depth * U * amax
    b_M2 = depth * U * (r.M2 + amax * np.abs(x - r.mean).sum(0))
    b_var = b_M2 / M + 4 * U * r.var
    b_invstd = 0.5 * r.invstd ** 3 * b_var + 4 * U * r.invstd
    g = np.ones_like(r.mean) if gamma is None else np.abs(np.asarray(gamma, np.float64))
    b = np.zeros_like(r.mean) if beta is None else np.abs(np.asarray(beta, np.float64))
    b_scale = g * b_invstd + 4 * U * np.abs(r.scale)
    b_shift = np.abs(r.scale) * b_mean + np.abs(r.mean) * b_scale + 4 * U * (b + np.abs(r.mean * r.scale))
    b_rm = None if rm is None else momentum * b_mean + 4 * U * ((1 - momentum) * np.abs(rm) + momentum * np.abs(r.mean))
    b_rv = None if rv is None else momentum * b_M2 / (M - 1) + 4 * U * ((1 - momentum) * np.abs(rv) + momentum * r.M2 / (M - 1))
    return Stats(b_mean, b_var, b_M2, b_invstd, b_scale, b_shift, b_rm, b_rv)


# ---- apply and backward -----------------------------------------------------------------------------------------------------------
def _note(trace, *vs):
    if trace is not None:
        trace.extend(vs)


def apply_ref(x, scale, shift, res=None, res_scale=None, res_shift=None, relu=False, factor=None, trace=None, terms=False):
    """y = drop(act(x*scale + shift [+ res*res_scale + res_shift | + res])) in f64; `factor` is drop_factor's (M, C) array or None.
    trace (a list) receives every intermediate; terms=True also returns the sum of the magnitudes of the terms of each element."""
    x = np.asarray(x, np.float64)
    a = x * scale
    o = a + shift
    mag = np.abs(a) + np.abs(shift)
    _note(trace, a, o)
    if res is not None:
        res = np.asarray(res, np.float64)
        if res_scale is not None:
            ra = res * res_scale
            rb = ra + res_shift
            mag = mag + np.abs(ra) + np.abs(res_shift)
            _note(trace, ra, rb)
        else:
            rb = res
            mag = mag + np.abs(res)
        o = o + rb
        _note(trace, o)
    if relu:
        o = np.where(o < 0, 0.0, o)
    if factor is not None:
        o = o * factor
        mag = mag * factor
        _note(trace, o)
    return (o, mag) if terms else o


def bwd_ref(dy, x, mean, invstd, gamma=None, factor=None, relu_mask=False, trace=None, trace_dx=True):
    """(sum g, sum g*xhat, dx) in f64, g = dy * factor, xhat = (x - mean)*invstd,
    dx = gamma*invstd * (g - sum_g/M - xhat * sum_gxhat/M), zero where not x > 0 when relu_mask.  mean and invstd are inputs."""
    dy, x = np.asarray(dy, np.float64), np.asarray(x, np.float64)
    M = x.shape[0]
    g = dy if factor is None else dy * factor
    xc = x - mean
    xh = xc * invstd
    gx = g * xh
    sg, sgx = g.sum(0), gx.sum(0)
    _note(trace, g, xc, xh, gx, sg, sgx)
    ga = np.ones_like(sg) if gamma is None else np.asarray(gamma, np.float64)
    t1, t2 = sg / M, sgx / M
    t3 = xh * t2
    t4 = g - t1
    t5 = t4 - t3
    k = ga * invstd
    dx = k * t5
    if trace_dx:
        _note(trace, t1, t2, t3, t4, t5, k, dx)
    if relu_mask:
        dx = np.where(x > 0, dx, 0.0)
    return sg, sgx, dx


def dx_bar(dy, x, mean, invstd, gamma=None, factor=None):
    """|dx - bwd_ref| per element when M is no power of two: the rounding of 1/M and four dependent operations,
    8u * |gamma*invstd| * (|g| + |sum_g|/M + |xhat*sum_gxhat|/M)"""
    dy, x = np.asarray(dy, np.float64), np.asarray(x, np.float64)
    M = x.shape[0]
    g = dy if factor is None else dy * factor
    xh = (x - mean) * invstd
    sg, sgx = g.sum(0), (g * xh).sum(0)
    ga = 1.0 if gamma is None else np.abs(np.asarray(gamma, np.float64))
    return 8 * U * ga * np.abs(invstd) * (np.abs(g) + np.abs(sg) / M + np.abs(xh * sgx) / M)


def is_f32(v):
    v = np.asarray(v, np.float64)
    return bool(np.all(v.astype(np.float32).astype(np.float64) == v))


def check_exact(case):
    """Raises ValueError unless every f32 operation of apply (all three residual forms) and of backward is exact on `case`: each
    intermediate of the f64 computation equals its own f32 rounding -- the two sums included and, when M is a power of two, every
    term of dx -- and the magnitudes of the terms of either sum add up to less than 2^24 units, so any partial sum in any order is an
    integer number of units below 2^24 (a unit is 1 for sum g, invstd for sum g*xhat)."""
    c = case
    M = c["x"].shape[0]
    trace = [c[k] for k in ("x", "res", "dy", "scale", "shift", "res_scale", "res_shift", "gamma", "mean", "invstd", "factor")]
    for kw in ({}, {"res": c["res"]}, {"res": c["res"], "res_scale": c["res_scale"], "res_shift": c["res_shift"]}):
        apply_ref(c["x"], c["scale"], c["shift"], factor=c["factor"], trace=trace, **kw)
    pow2 = M & (M - 1) == 0
    for gamma in (c["gamma"], None):
        bwd_ref(c["dy"], c["x"], c["mean"], c["invstd"], gamma, c["factor"], trace=trace, trace_dx=pow2)
    if not all(is_f32(v) for v in trace):
        raise ValueError("exact_case: an intermediate is not an f32 number")
    m, e = np.frexp(c["invstd"])
    if not np.all(m == 0.5):
        raise ValueError("exact_case: invstd is no power of two")
    g = np.abs(c["dy"] * c["factor"])
    if g.sum(0).max() >= 2 ** 24 or (g * np.abs(c["x"] - c["mean"])).sum(0).max() >= 2 ** 24:
        raise ValueError("exact_case: a sum can reach 2^24 units")


def exact_case(M, C, seed, mode=0, p=0.5, site=0, HW=1, amp=8):
    """Integer data for ssd_bn_apply and ssd_bn_train_bwd: x (with zeros of both signs), res, dy in [-amp, amp]; scale, res_scale and
    gamma in +-{1, 2}; shift, res_shift and mean in [-3, 3]; invstd in {1/2, 1, 2}; p in {0, 0.5, 0.75, 1} (factor 1, 2, 4, 0).
    f64 arrays, checked by check_exact."""
    if mode != 0 and p not in (0.0, 0.5, 0.75, 1.0):
        raise ValueError("exact_case: 1/(1-p) must be a power of two")
    rng = np.random.default_rng(seed)
    ints = lambda lo, hi, shape: rng.integers(lo, hi + 1, shape).astype(np.float64)        # noqa: E731
    sign2 = lambda shape: rng.choice([-2.0, -1.0, 1.0, 2.0], shape)                        # noqa: E731
    x = ints(-amp, amp, (M, C))
    x[(x == 0) & (rng.random((M, C)) < 0.5)] = -0.0
    case = {"x": x, "res": ints(-amp, amp, (M, C)), "dy": ints(-amp, amp, (M, C)), "scale": sign2(C), "shift": ints(-3, 3, C),
            "res_scale": sign2(C), "res_shift": ints(-3, 3, C), "gamma": sign2(C), "mean": ints(-3, 3, C),
            "invstd": rng.choice([0.5, 1.0, 2.0], C), "factor": drop_factor(mode, p, seed, site, M, C, HW),
            "drop": None if mode == 0 else (mode, p, seed, site, HW)}
    check_exact(case)
    return case


# ---- the shapes and data families of the statistics tests -------------------------------------------------------------------------
STATS_SHAPES = [(2, 4, 4), (1360, 12, 32), (1361, 12, 32), (1367, 12, 32), (600, 28, 28), (4096, 256, 256), (4097, 260, 288),
                (66563, 256, 256), (147, 512, 512)]
FAMILIES = ["randn", "offset", "near-one", "scales", "constant"]


def family(name, M, C, seed):
    """(M, C) f32 data: randn*2 + 0.5;  4096 + k*2^-11, k an integer in -64..64 (each value exact in f32);  1 + 1e-3*randn;  channels of
    scale 1e-3, 1 and 1e3 in turn;  constant channels"""
    rng = np.random.default_rng([seed, M, C, FAMILIES.index(name)])
    if name == "randn":
        x = rng.standard_normal((M, C)) * 2.0 + 0.5
    elif name == "offset":
        x = 4096.0 + rng.integers(-64, 65, (M, C)) * 2.0 ** -11
    elif name == "near-one":
        x = 1.0 + 1e-3 * rng.standard_normal((M, C))
    elif name == "scales":
        x = rng.standard_normal((M, C)) * np.array([1e-3, 1.0, 1e3])[np.arange(C) % 3]
    else:
        x = np.broadcast_to(np.array([1000.5, -3.25, 0.1, 70001.0, 0.0, 1e-3, -12345.678])[np.arange(C) % 7], (M, C))
    return np.ascontiguousarray(x, dtype=np.float32)


def channel_params(C, seed):
    """gamma, beta, running_mean, running_var (f32) of a statistics case"""
    rng = np.random.default_rng([seed, C, 77])
    f = lambda v: v.astype(np.float32)                                                     # noqa: E731
    return f(rng.random(C) + 0.5), f(rng.standard_normal(C) * 0.1), f(rng.standard_normal(C) * 0.1), f(rng.random(C) + 0.5)

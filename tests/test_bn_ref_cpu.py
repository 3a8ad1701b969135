"""bn_ref.py can tell a right BatchNorm statistics kernel from a wrong one, shown without a GPU.

`emulate` is an f32 numpy restatement of the order batchnorm.hip documents (Welford per thread over its interleaved rows, Chan merges of
the lanes in lane order, of the slabs strided over 64 threads, then a 64-wide tree); `naive` is the sum x^2 - M*mean^2 form.  Both are
test code, neither is the kernel.  The emulation has to stay within bn_ref.stats_bars on every shape and data family the GPU test
uses; the naive form, a wrong lane count and a variance over M - 1 have to break them.

Largest emulation error / bar seen over all shapes and families (how loose the first-order worst-case bars are; nothing asserts it):
0.098 for mean, 0.054 for M2 and var, 0.21 for invstd and scale, 0.076 for shift; 0.55 for the running statistics, whose bars are mostly
the 4u of their own three roundings (run with -s for every case's figures).  The naive form sits at 1e4 to 2.5e5 times bar_M2 on the
offset family and on a zero bar (NaN invstd) on constant channels; the wrong lane count at 29 to 4.6e4 times bar_mean.
"""
import numpy as np
import pytest

import bn_ref as R

EPS, MOM = 1e-5, 0.1
f32 = np.float32


def _merge(n, mean, m2, nb, meanb, m2b):
    """chan_merge on f32 arrays; where nb == 0 nothing changes"""
    with np.errstate(invalid="ignore", divide="ignore"):
        t = n + nb
        d = meanb - mean
        f = nb / t
        mean2 = mean + d * f
        m22 = m2 + (m2b + d * d * n * f)
    skip = nb == 0
    return np.where(skip, n, t), np.where(skip, mean, mean2), np.where(skip, m2, m22)


def emulate_mean_m2(x, pl, wrong_lanes=False):
    """(mean, M2) per channel in the documented order, every operation rounded to f32"""
    M, C = x.shape
    rows, lanes, nslab = pl.rows, pl.lanes, pl.nslab
    steps = -(-rows // lanes)
    rows_s = np.minimum(rows, M - np.arange(nslab) * rows)                                  # rows of each slab
    off = np.arange(steps)[:, None] * lanes + np.arange(lanes)[None, :]                    # (steps, lanes) row within the slab
    valid = off[None] < rows_s[:, None, None]
    idx = np.minimum(np.arange(nslab)[:, None, None] * rows + off[None], M - 1)
    mean = np.zeros((nslab, lanes, C), f32)
    m2 = np.zeros((nslab, lanes, C), f32)
    for k in range(steps):                                                                  # Welford, one row per thread and step
        v = x[idx[:, k]]
        ok = valid[:, k][:, :, None]
        inv = f32(1) / f32(k + 1)
        d = v - mean
        mean_n = mean + d * inv
        m2_n = m2 + d * (v - mean_n)
        mean, m2 = np.where(ok, mean_n, mean), np.where(ok, m2_n, m2)
    count = (lambda l: rows_s // lanes) if wrong_lanes else (lambda l: np.where(rows_s > l, (rows_s - l + lanes - 1) // lanes, 0))
    n = count(0).astype(f32)[:, None]
    sm, s2 = mean[:, 0], m2[:, 0]
    for l in range(1, lanes):                                                               # lanes, in lane order
        nl = count(l).astype(f32)[:, None]
        _, sm, s2 = _merge(n, sm, s2, nl, mean[:, l], m2[:, l])
        n = n + nl
    trips = -(-nslab // 64)
    pad = trips * 64 - nslab
    pn = np.concatenate([rows_s.astype(f32), np.zeros(pad, f32)]).reshape(trips, 64, 1)
    pm = np.concatenate([sm, np.zeros((pad, C), f32)]).reshape(trips, 64, C)
    p2 = np.concatenate([s2, np.zeros((pad, C), f32)]).reshape(trips, 64, C)
    n, mu, q = np.zeros((64, 1), f32), np.zeros((64, C), f32), np.zeros((64, C), f32)
    for t in range(trips):                                                                  # slabs, strided over the 64 threads
        n, mu, q = _merge(n, mu, q, pn[t], pm[t], p2[t])
    w = 32
    while w > 0:                                                                            # the tree
        a, am, a2 = _merge(n[:w], mu[:w], q[:w], n[w:2 * w], mu[w:2 * w], q[w:2 * w])
        n, mu, q = a, am, a2
        w //= 2
    assert n[0, 0] == M
    return mu[0], q[0]


def naive_mean_m2(x):
    M = f32(x.shape[0])
    mean = x.sum(0, dtype=f32) / M
    return mean, (x * x).sum(0, dtype=f32) - M * mean * mean


def finish(mean, m2, M, gamma, beta, rm, rv, divide_by=None):
    """bn_finalize_kernel's last step in f32 -> bn_ref.Stats"""
    with np.errstate(invalid="ignore", divide="ignore"):
        var = m2 / f32(divide_by or M)
        invstd = f32(1) / np.sqrt(var + f32(EPS))
        scale = gamma * invstd
        shift = beta - mean * scale
        nrm = (f32(1) - f32(MOM)) * rm + f32(MOM) * mean
        nrv = (f32(1) - f32(MOM)) * rv + f32(MOM) * (m2 / f32(M - 1))
    return R.Stats(mean, var, m2, invstd, scale, shift, nrm, nrv)


def ratios(got, bars, ref):
    """largest |got - ref| / bar per field; inf where a value is NaN or an error sits on a zero bar"""
    out = {}
    for name in R.Stats._fields:
        err = np.abs(getattr(got, name).astype(np.float64) - getattr(ref, name))
        bar = getattr(bars, name)
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(err == 0, 0.0, err / bar)
        out[name] = float(np.inf if np.isnan(r).any() else r.max())
    return out


_cache = {}


def case(shape, fam):
    key = (shape, fam)
    if key not in _cache:
        _cache.clear()                                          # one case at a time: the largest is 68 MB in f32
        M, C, _ = shape
        x = R.family(fam, M, C, 1)
        gamma, beta, rm, rv = R.channel_params(C, 1)
        pl = R.plan(M, C)
        _cache[key] = (x, pl, (gamma, beta, rm, rv), R.stats_ref(x, gamma, beta, EPS, MOM, rm, rv),
                       R.stats_bars(x, pl, gamma, beta, EPS, MOM, rm, rv))
    return _cache[key]


def test_plan_restates_what_the_shapes_were_chosen_for():
    P = {s[:2]: R.plan(*s[:2]) for s in R.STATS_SHAPES}
    assert (P[2, 4].lanes, P[2, 4].nslab) == (256, 1)
    assert (P[1360, 12].cgb, P[1360, 12].lanes, P[1360, 12].rows, P[1360, 12].nslab) == (3, 85, 1360, 1)
    assert P[1361, 12].nslab == 2 and 1361 - P[1361, 12].rows == 1
    assert P[1367, 12].nslab == 2 and 1367 - P[1367, 12].rows == 7 < P[1367, 12].lanes
    assert (P[600, 28].cgb, P[600, 28].lanes) == (7, 36) and 256 - 7 * 36 == 4
    assert P[4096, 256].nslab == 64
    assert (P[4097, 260].nslab, P[4097, 260].chunks, P[4097, 260].rows) == (65, 2, 64) and 260 // 4 - 64 == 1
    p = P[66563, 256]
    assert (p.rows, p.lanes, p.nslab) == (66, 4, 1009) and p.rows > p.lanes * 16 and p.rows % p.lanes and 66563 - 1008 * 66 == 35
    assert all(pl.bytes == pl.nslab * C * 8 for (M, C), pl in P.items())


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("shape", R.STATS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_documented_order_stays_within_the_bars(shape, fam):
    x, pl, (gamma, beta, rm, rv), ref, bars = case(shape, fam)
    mean, m2 = emulate_mean_m2(x, pl)
    r = ratios(finish(mean, m2, x.shape[0], gamma, beta, rm, rv), bars, ref)
    print("emulation/bar", shape, fam, {k: f"{v:.3g}" for k, v in r.items()})
    assert max(r.values()) <= 1.0, r
    if fam == "constant":
        assert np.array_equal(mean, x[0]) and not m2.any()


@pytest.mark.parametrize("fam", ["offset", "constant"])
@pytest.mark.parametrize("shape", [s for s in R.STATS_SHAPES if s[0] >= 147], ids=lambda s: "x".join(map(str, s)))
def test_the_naive_variance_breaks_the_m2_bar(shape, fam):
    x, pl, (gamma, beta, rm, rv), ref, bars = case(shape, fam)
    mean, m2 = naive_mean_m2(x)
    r = ratios(finish(mean, m2, x.shape[0], gamma, beta, rm, rv), bars, ref)
    print("naive/bar", shape, fam, {k: f"{v:.3g}" for k, v in r.items()})
    assert r["M2"] > 1.0 and r["running_var"] > 1.0 and r["invstd"] > 1.0, r


# the shapes with a slab whose row count is no multiple of `lanes`, beyond a single leftover row (which lane 0 owns either way)
@pytest.mark.parametrize("shape", [(2, 4, 4), (1367, 12, 32), (66563, 256, 256), (147, 512, 512)], ids=lambda s: "x".join(map(str, s)))
def test_a_wrong_lane_count_breaks_the_bars(shape):
    x, pl, (gamma, beta, rm, rv), ref, bars = case(shape, "randn")
    mean, m2 = emulate_mean_m2(x, pl, wrong_lanes=True)
    r = ratios(finish(mean, m2, x.shape[0], gamma, beta, rm, rv), bars, ref)
    print("wrong lanes/bar", shape, {k: f"{v:.3g}" for k, v in r.items()})
    assert r["mean"] > 1.0 and r["invstd"] > 1.0 and r["shift"] > 1.0, r


# invstd moves by 1/(2M) relative; the bar is some 5 * depth * u, so the two can be told apart up to M of a few thousand
@pytest.mark.parametrize("shape", [s for s in R.STATS_SHAPES if s[0] <= 4097], ids=lambda s: "x".join(map(str, s)))
def test_a_variance_over_m_minus_1_breaks_the_bars(shape):
    x, pl, (gamma, beta, rm, rv), ref, bars = case(shape, "randn")
    mean, m2 = emulate_mean_m2(x, pl)
    r = ratios(finish(mean, m2, x.shape[0], gamma, beta, rm, rv, divide_by=x.shape[0] - 1), bars, ref)
    assert r["invstd"] > 1.0 and r["scale"] > 1.0 and r["mean"] <= 1.0 and r["running_var"] <= 1.0, r


# ---- exact cases ------------------------------------------------------------------------------------------------------------------
def test_exact_case_checks_itself():
    for M, C, mode, p, HW in ((5, 4, 0, 0.0, 1), (147, 12, 2, 0.75, 49), (1024, 12, 1, 0.5, 1), (4096, 256, 2, 0.75, 64)):
        c = R.exact_case(M, C, 3, mode, p, 2, HW)
        assert set(np.unique(c["factor"])) <= {0.0, 1.0 / (1.0 - p)}
        zeros = c["x"][c["x"] == 0]
        assert M < 147 or (np.signbit(zeros).any() and not np.signbit(zeros).all())
    with pytest.raises(ValueError, match="2\\^24"):
        R.exact_case(5000, 4, 3, amp=256)                       # every product fits, sum |g| * |x - mean| passes 2^24
    with pytest.raises(ValueError, match="f32 number"):
        R.exact_case(64, 4, 3, amp=2 ** 13)                     # g * (x - mean) needs more than 24 bits
    with pytest.raises(ValueError, match="power of two"):
        R.exact_case(64, 4, 3, mode=1, p=0.3)
    c = R.exact_case(1024, 12, 3)
    c["invstd"] = c["invstd"] * 3.0
    with pytest.raises(ValueError):
        R.check_exact(c)


# ---- Philox -----------------------------------------------------------------------------------------------------------------------
def _philox_int(ctr, key):
    """Philox4x32-10 on Python integers, from the paper: per round one 32x32 -> 64 product per counter pair, then the key bumps"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return [c0, c1, c2, c3]


KAT = [  # Random123's known-answer vectors for philox4x32-10: counter, key, output
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


def test_philox_reproduces_the_known_answers():
    for ctr, key, want in KAT:
        got = R.philox4x32_10([np.array([v], np.uint64) for v in ctr], key)
        assert [int(g[0]) for g in got] == want
        assert _philox_int(ctr, key) == want
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 2 ** 32, (4, 50), dtype=np.uint64)
    key = [int(v) for v in rng.integers(0, 2 ** 32, 2, dtype=np.uint64)]
    got = np.stack(R.philox4x32_10(list(ctr), key))
    assert all([int(v) for v in got[:, i]] == _philox_int([int(v) for v in ctr[:, i]], key) for i in range(50))


def test_philox_keep_draws_the_documented_word_of_the_documented_counter():
    seed, site, p = (0xDEADBEEF << 32) | 0x12345678, 5, 0.3
    keep = R.philox_keep(seed, site, 40, p)
    for i in (0, 1, 6, 39):
        w = _philox_int([i >> 2, 0, site, 0], [seed & 0xFFFFFFFF, seed >> 32])[i & 3]
        assert keep[i] == ((w >> 8) * 2.0 ** -24 < float(f32(1) - f32(p)))
    assert R.philox_keep(seed, site, 64, 0.0).all() and not R.philox_keep(seed, site, 64, 1.0).any()


@pytest.mark.parametrize("p", [0.3, 0.5, 0.75])
def test_drop_factor_has_mean_one(p):
    M, C, HW = 4096, 64, 16
    for mode, draws in ((1, M * C), (2, M // HW * C)):
        f = R.drop_factor(mode, p, 1234567 << 20, 3, M, C, HW)
        assert set(np.unique(f)) == {0.0, R.drop_scale(p)}
        sigma = np.sqrt(p / (1 - p) / draws)                    # a factor is 1/(1-p) with probability 1-p, else 0
        assert abs(f.mean() - 1.0) < 5 * sigma
        if mode == 2:
            assert np.array_equal(f.reshape(M // HW, HW, C), np.repeat(f[::HW, None], HW, axis=1))
    assert not R.drop_factor(1, 1.0, 9, 0, 8, 4, 1).any() and (R.drop_factor(2, 0.0, 9, 0, 8, 4, 2) == 1).all()
    flat = R.philox_keep(9, 1, 8 * 12, p)
    assert np.array_equal(R.drop_factor(1, p, 9, 1, 8, 12, 1) != 0, flat.reshape(8, 12))
    assert np.array_equal(R.drop_factor(2, p, 9, 1, 8, 12, 4) != 0, np.repeat(flat[:24].reshape(2, 12), 4, axis=0))

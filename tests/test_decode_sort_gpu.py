"""The first two stages of the decode alone -- decode_compact_kernel and rank_scatter_kernel through ssd_decode_sorted, the decode's own
launch function with nothing forced -- held to the f64 checker of tests/decode_sort_ref.py: every box, the exact candidate set of
every class, the order on the device's own bits, every probability within 1e-5 of f64, every scattered box, every slot the kernels
must leave alone.  The shapes are the ones at which these kernels decide something: both sides of both block-size switches and both
parities of the LDS row stride, one to three rounds of 32 classes, prior counts around a wave and around the block, rank tiles of
256 / 257 / 512 candidates, tied keys, the score cut at equality, rows that are not numbers; then the bare entries chained against
the whole decode.

Two tolerances, both 1e-5 (boxes before the cancellation, probabilities against f64); everything else is exact.  Every
tolerance-compared case keeps its logit spread within 60, so that every probability is a normal f32: what the device does with a
subnormal probability is not pinned here.  The output arrays and the key workspace are freshly poisoned before every launch."""
import ctypes

import numpy as np
import pytest
import torch

import decode_sort_ref as D

pytestmark = pytest.mark.gpu

DEV = "cuda"
MIN_SCORE = 0.2


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _lib():
    from objectdetection_ssd_amd import _lib
    return _lib.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def launch(l_, c_, pri, min_score, clear=0):
    """one ssd_decode_sorted launch into freshly poisoned arrays -> the five device tensors (boxes, s_boxes, s_prob, s_idx, cand_cnt)"""
    B, P, C = c_.shape
    lib = _lib()
    d_in = [_t(l_), _t(c_), _t(pri)]
    out = [_t(a) for a in D.poisoned_outputs(B, P, C - 1)]
    need = lib.ssd_decode_sorted_workspace(B, P, C)
    assert need == (B * (C - 1) * P * 8 + 255) // 256 * 256
    ws = torch.full((need,), 0xFF, device=DEV, dtype=torch.uint8)          # stale keys that would outrank every candidate
    rc = lib.ssd_decode_sorted(d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), B, P, C, float(min_score), out[0].data_ptr(),
                               out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), out[4].data_ptr(), ws.data_ptr(), need, _stream(), clear)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def run(l_, c_, pri, min_score, clear=0):
    return tuple(x.cpu().numpy() for x in launch(l_, c_, pri, min_score, clear))


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


# ---- shape sweep ---------------------------------------------------------------------------------------------------------------------
BLOCK = {2: 256, 3: 256, 4: 256, 21: 256, 22: 256, 33: 256, 34: 256, 47: 256, 48: 128, 65: 128, 66: 128, 95: 128, 96: 64, 97: 64,
         255: 64, 256: 64}


@pytest.mark.parametrize("C", D.SWEEP_C)
def test_shape_sweep(C):
    """B = 3, rows N(0, 9), offsets N(0, 0.25) with exp(g / 5) up to e^+-2 on a few priors, random priors, min_score 0.2; every prior
    count of decode_sort_ref.sweep_sizes for this C's block size.  The second launch clears the counters with the kernel and must
    give the first one's bits."""
    nt = D.block_priors(C)
    assert nt == BLOCK[C]
    sizes = D.sweep_sizes(C)
    assert sizes[0] == 1 and sizes[-1] == 2 * nt + 65 and {63, 64, 65, nt - 1, nt, nt + 1, 2 * nt + 1} <= set(sizes)
    prob_err = box_err = 0.0
    classes = 0
    for P in sizes:
        l_, c_, pri = D.sweep_case(C, D.SWEEP_SEED[C], P)
        out = run(l_, c_, pri, MIN_SCORE, clear=0)
        info = D.check(l_, c_, pri, MIN_SCORE, out)
        assert info["compared"] == info["classes"], (P, info["compared"], info["classes"])    # a property of the reference alone
        assert same_bits(out, run(l_, c_, pri, MIN_SCORE, clear=1)), P
        prob_err, box_err, classes = max(prob_err, info["prob_err"]), max(box_err, info["box_err"]), classes + info["classes"]
        if P == sizes[-1]:
            assert info["candidates"].sum() > P // 2 and (info["candidates"] > 0).sum() >= min(C - 1, 20)
    print(f"sweep C {C}: block {nt}, P {sizes}, {classes} classes with candidates, prob err {prob_err:.3g} (relative, against f64), "
          f"box err {box_err:.3g} bars")


# ---- rank-tile boundaries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 511, 512, 513, 1100])
def test_rank_tile_boundaries(n):
    """P = 1100, C = 21, B = 2: one class per image has exactly n candidates at random positions -- no tile, one tile short by one,
    exactly one, one and one more, two, all P -- among classes of 0 - 3 candidates; blocks of rank_scatter past a class's count exit"""
    rng = np.random.default_rng(7000 + n)
    P, C = 1100, 21
    swept = (5, 13)
    ims = [D.strong_class_image(rng, n, cls, P, C) for cls in swept]
    l_, c_, pri = np.stack([i[0] for i in ims]), np.stack([i[1] for i in ims]), D.random_priors(rng, P)
    out = run(l_, c_, pri, MIN_SCORE)
    info = D.check(l_, c_, pri, MIN_SCORE, out)
    for b, cls in enumerate(swept):
        assert out[4][b, cls] == n
        assert np.delete(info["candidates"][b], cls).max() <= 3
    assert info["compared"] == info["classes"]
    if n == P:
        # every class full.  The cut 0 needs no margin: p >= 0 holds for every probability that is a number, however it was rounded
        out = run(l_, c_, pri, 0.0, clear=1)
        info = D.check(l_, c_, pri, 0.0, out, margin=0.0)
        assert (out[4][:, :C - 1] == P).all()
        assert float((c_.max(-1) - c_.min(-1)).max()) < 60


# ---- ties ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_group", [False, True])
def test_tied_keys_order_by_prior_and_repeat_bitwise(one_group):
    """C = 21, P = 700, two identical images.  Rows from 4 logit vectors: hundreds of keys with one high half in a class, the same
    probability in several classes; or every row the same vector: n = P, one tie group.  Inside a tie group the order is the prior
    index (the low half of the key); the slots the candidates took in keys[] differ from launch to launch, the outputs do not."""
    rng = np.random.default_rng(11 + one_group)
    P, C = 700, 21
    l1, c1 = D.tied_rows_image(rng, P, C, n_fg=600)
    if one_group:
        c1[:] = c1[np.nonzero(c1[:, 0] > -8.0)[0][0]]                   # the vector with classes 0, 3, 7, 19 or 0, 5, 19
    l_, c_, pri = np.stack([l1, l1]), np.stack([c1, c1]), D.random_priors(rng, P)
    first = run(l_, c_, pri, MIN_SCORE)
    info = D.check(l_, c_, pri, MIN_SCORE, first)
    assert info["compared"] == info["classes"] > 0
    n = first[4][0, :C - 1]
    assert np.array_equal(first[4][0], first[4][1])
    assert all(np.array_equal(a[0].view(np.uint32), a[1].view(np.uint32)) for a in first[:4])       # both images alike
    ties = 0
    for c in np.nonzero(n)[0]:
        bits = first[2][0, c, :n[c]].view(np.uint32)
        ties += int((bits[1:] == bits[:-1]).sum())
        if one_group:
            assert n[c] == P and np.array_equal(first[3][0, c], np.arange(P)) and len(set(bits.tolist())) == 1
    assert ties > 500
    for k in range(4):
        assert same_bits(first, run(l_, c_, pri, MIN_SCORE, clear=k % 2)), k


# ---- the score cut at equality -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 4, 256])
def test_exact_cut(C):
    """all-zero rows: every probability is exactly 1 / C, on the device, in torch and in f64 (exp(0) = 1, a power-of-two sum), so the
    checker's set needs no margin.  min_score = 1 / C: every prior is a candidate of every class (>= at equality); one ulp above:
    none, and nothing is written; 0: all; 1.5: none."""
    P, B = 2 * D.block_priors(C) + 65, 2
    rng = np.random.default_rng(C)
    l_ = np.stack([D.random_offsets(rng, P) for _ in range(B)])
    c_, pri = np.zeros((B, P, C), np.float32), D.random_priors(rng, P)
    q = np.float32(1.0) / np.float32(C)
    assert float(q) * C == 1.0
    for min_score, full in ((float(q), True), (float(np.nextafter(q, np.float32(1))), False), (0.0, True), (1.5, False)):
        out = run(l_, c_, pri, min_score, clear=int(full))
        D.check(l_, c_, pri, min_score, out, margin=0.0)
        assert (out[4][:, :C - 1] == (P if full else 0)).all(), min_score
        if full:
            assert (out[3] == np.arange(P, dtype=np.int32)).all() and (out[2].view(np.uint32) == q.view(np.uint32)).all()
        else:
            assert (out[3] == D.POISON_IDX).all() and (out[2] == D.POISON_PROB).all() and (out[1] == D.POISON_BOX).all()


# ---- rows that are not numbers -------------------------------------------------------------------------------------------------------
def test_non_finite_rows():
    """P = 300, C = 21 (one full block and a partial one).  Among N(0, 9) rows: a row with a NaN logit at prior 0 (lane 0 of wave 0), a
    row with +inf at prior 127 (lane 63 of wave 1), a row of -inf at prior 70, and at prior 260 (second block) a row with -inf on some
    classes, probability 0 there.  The first three are candidates of nothing at min_score 0.2 and at 0 -- NaN >= cut is false, as in
    torch; the fourth follows the reference (at cut 0 its zeros are candidates: 0 >= 0); every other prior of those waves is what
    the reference says; every box is decoded."""
    P, C = 300, 21
    l_, c_, pri = D.sweep_case(C, D.SWEEP_SEED[C], P, B=2)
    c_ = c_.copy()
    nan, inf = np.float32("nan"), np.float32("inf")
    c_[0, 0, 4] = nan
    c_[0, 127, 9] = inf
    c_[0, 70, :] = -inf
    c_[0, 260, :] = np.linspace(-0.5, 0.5, C, dtype=np.float32)
    c_[0, 260, [1, 2, 17]] = -inf
    c_[0, 260, 6] = 3.0                                                   # (a candidate of class 6: about half of its mass)
    c_[1, 299, 20] = nan                                                  # the last prior of the other image, a NaN background logit
    ref = D.softmax64(c_)
    assert np.isnan(ref[0, [0, 127, 70]]).all() and np.isnan(ref[1, 299]).all() and np.isfinite(ref).sum() == ref.size - 4 * C
    assert (ref[0, 260, [1, 2, 17]] == 0).all() and ref[0, 260, 6] > 0.3
    for min_score in (MIN_SCORE, 0.0):
        out = run(l_, c_, pri, min_score)
        # cut 0: no margin needed, p >= 0 holds for every probability that is a number
        info = D.check(l_, c_, pri, min_score, out, margin=D.SCORE_MARGIN if min_score else 0.0)
        n = out[4][:, :C - 1]
        listed = [set(out[3][b, c, :n[b, c]].tolist()) for b in range(2) for c in range(C - 1)]
        assert not any({0, 127, 70} & s for s in listed[:C - 1]) and not any(299 in s for s in listed[C - 1:])
        if min_score == 0.0:
            assert (n[0] == P - 3).all() and (n[1] == P - 1).all()
            for c in (1, 2, 17):
                assert out[3][0, c, P - 4] == 260 and out[2][0, c, P - 4] == 0        # probability 0: the last candidate
        else:
            assert 260 in listed[6] and info["candidates"].sum() > 200


# ---- the bare entries chained, against the whole decode ----------------------------------------------------------------------------
def chain(l_, c_, pri, wh, top_k, thr, soft):
    """ssd_decode_sorted -> ssd_nms_sorted or ssd_soft_nms_sorted (linear) -> ssd_topk_emit_sorted"""
    lib = _lib()
    B, P, C = c_.shape
    C1 = C - 1
    boxes, s_boxes, s_prob, s_idx, cnt = launch(l_, c_, pri, MIN_SCORE, clear=int(soft))
    kept_pos = torch.full((B, C1, P), -1, device=DEV, dtype=torch.int32)
    kept_prob = torch.full((B, C1, P), -1.0, device=DEV, dtype=torch.float32)
    kept_cnt = torch.full((B, C1 + 1), -1, device=DEV, dtype=torch.int32)
    if soft:
        rc = lib.ssd_soft_nms_sorted(s_boxes.data_ptr(), s_prob.data_ptr(), cnt.data_ptr(), B, C1, P, 1, thr, 0.5, MIN_SCORE, top_k,
                                     kept_pos.data_ptr(), kept_prob.data_ptr(), kept_cnt.data_ptr(), _stream())
    else:
        rc = lib.ssd_nms_sorted(s_boxes.data_ptr(), s_prob.data_ptr(), cnt.data_ptr(), B, C1, P, thr, kept_pos.data_ptr(),
                                kept_prob.data_ptr(), kept_cnt.data_ptr(), _stream())
    assert rc == 0, rc
    d_wh = _t(wh)
    return emit_outputs(lambda o, ws, nbytes: lib.ssd_topk_emit_sorted(
        s_boxes.data_ptr(), s_idx.data_ptr(), kept_pos.data_ptr(), kept_prob.data_ptr(), kept_cnt.data_ptr(), d_wh.data_ptr(), B, C1, P,
        top_k, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), ws.data_ptr(), nbytes, _stream()),
        B, top_k, 2 * ((B * C1 * P * 4 + 255) // 256 * 256))


def emit_outputs(call, B, top_k, ws_bytes):
    o = [torch.full((B, top_k, 4), -1.0, device=DEV, dtype=torch.float32), torch.full((B, top_k), -1, device=DEV, dtype=torch.int64),
         torch.full((B, top_k), -1.0, device=DEV, dtype=torch.float32), torch.full((B, top_k), -1, device=DEV, dtype=torch.int32),
         torch.full((B,), -7, device=DEV, dtype=torch.int32)]
    ws = torch.empty(ws_bytes, device=DEV, dtype=torch.uint8)
    rc = call(o, ws, ws_bytes)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in o]


def whole(l_, c_, pri, wh, top_k, thr, soft):
    lib = _lib()
    B, P, C = c_.shape
    d = [_t(l_), _t(c_), _t(pri), _t(wh)]
    head = lambda o, ws, nbytes: (d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), B, P, C, MIN_SCORE, thr, top_k,
                                  o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), ws.data_ptr(), nbytes,
                                  _stream())
    if soft:
        return emit_outputs(lambda o, ws, nbytes: lib.ssd_decode_nms_batch_soft(*head(o, ws, nbytes), 1, 0.5, MIN_SCORE), B, top_k,
                            lib.ssd_decode_nms_batch_workspace(B, P, C))
    return emit_outputs(lambda o, ws, nbytes: lib.ssd_decode_nms_batch(*head(o, ws, nbytes)), B, top_k,
                        lib.ssd_decode_nms_batch_workspace(B, P, C))


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("C", [21, 48, 96, 256])
def test_chained_bare_entries_equal_the_decode(C, soft):
    """the sweep's inputs at P = 2 NT + 65: count, boxes, classes, probabilities and prior ids of the chain are the decode's, bit for
    bit -- the greedy keep sets and the arg-max picks depend on the sorted arrays alone, and the top-k orders by probability bits,
    class and sorted position.  The Soft-NMS chain clears the counters with the kernel, as its decode does."""
    P = 2 * D.block_priors(C) + 65
    l_, c_, pri = D.sweep_case(C, D.SWEEP_SEED[C], P)
    wh = np.asarray([(300, 300), (500, 375), (640, 480)], np.float32)
    top_k = 200
    got, ref = chain(l_, c_, pri, wh, top_k, 0.45, soft), whole(l_, c_, pri, wh, top_k, 0.45, soft)
    assert np.array_equal(got[4], ref[4]) and (ref[4] > 0).all() and (ref[4] <= top_k).all()
    print(f"chain C {C} soft {soft}: counts {ref[4].tolist()}")
    for b in range(3):
        k = int(ref[4][b])
        assert np.array_equal(got[1][b, :k], ref[1][b, :k]) and np.array_equal(got[3][b, :k], ref[3][b, :k]), b
        assert np.array_equal(got[2][b, :k].view(np.uint32), ref[2][b, :k].view(np.uint32)), b
        assert np.array_equal(got[0][b, :k].view(np.uint32), ref[0][b, :k].view(np.uint32)), b
        assert (got[1][b, k:] == -1).all() and (got[3][b, k:] == -1).all()

"""Soft-NMS on the GPU against the numpy reference (tests/soft_nms_ref.py): the bare kernel bit for bit under the linear rule (every
operation a correctly rounded f32 operation) and within the decode tolerance under the gaussian rule (expf), then the rule through
Losses.inference / inference_batch / inference_batch_padded, the hard rule's regression, and graph capture.

Comparisons that allow rounding differences -- gaussian, and everything end to end, where the device's softmax differs from torch's
by a few ulps -- are made on inputs whose reference margin (soft_nms_ref: the relative distance of the nearest decision from
flipping) is at least 1e-4, ten times the decode tolerance rtol = 1e-5; the margin is asserted first, on the reference alone.  Where
more than top_k picks compete, the cross-class sort's nearest neighbours are asserted 1e-5 apart as well: ten times the 1e-6 by
which device and reference probabilities were found to differ (tests/test_class_count_gpu.py), each gaussian factor adding about
an ulp."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import soft_nms_ref as S
from nms_cases import pack, random_class

pytestmark = pytest.mark.gpu

DEV = "cuda"
MARGIN, ORDER_MARGIN, RTOL = 1e-4, 1e-5, 1e-5


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the bare kernel ---------------------------------------------------------------------------------------------------------
def run_bare(s_boxes, s_prob, cnt, method, thr, sigma, keep, max_picks):
    from objectdetection_ssd_amd import _lib
    lib = _lib.load()
    B, C1, P = s_prob.shape
    d_boxes, d_prob, d_cnt = _t(s_boxes), _t(s_prob), _t(cnt)
    kept_pos = torch.full((B, C1, P), -1, device=DEV, dtype=torch.int32)
    kept_prob = torch.full((B, C1, P), -1.0, device=DEV, dtype=torch.float32)
    kept_cnt = torch.full((B, C1 + 1), -1, device=DEV, dtype=torch.int32)
    rc = lib.ssd_soft_nms_sorted(d_boxes.data_ptr(), d_prob.data_ptr(), d_cnt.data_ptr(), B, C1, P, method, thr, sigma, keep, max_picks,
                                 kept_pos.data_ptr(), kept_prob.data_ptr(), kept_cnt.data_ptr(),
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return kept_pos.cpu().numpy(), kept_prob.cpu().numpy(), kept_cnt.cpu().numpy()


def check_bare(classes, B, C1, P, method, thr=0.45, sigma=0.5, keep=0.2, max_picks=200, exact=True, min_margin=None):
    s_boxes, s_prob, cnt = pack(classes, B, C1, P)
    refs = [[S.soft_nms_sorted(*classes[b][c], method, thr, sigma, keep, max_picks) for c in range(C1)] for b in range(B)]
    if min_margin is not None:                                  # a condition of the test, on the reference alone
        m = min(r[2] for row in refs for r in row)
        print(f"reference margin {m:.3e}")
        assert m >= min_margin, m
    kp, kq, kc = run_bare(s_boxes, s_prob, cnt, method, thr, sigma, keep, max_picks)
    picks = 0
    for b in range(B):
        for c in range(C1):
            pos, sc, _ = refs[b][c]
            k = pos.shape[0]
            picks += k
            assert kc[b, c] == k, (b, c, kc[b, c], k)
            assert np.array_equal(kp[b, c, :k], pos), (b, c)
            if exact:
                assert np.array_equal(kq[b, c, :k].view(np.uint32), sc.view(np.uint32)), (b, c)
            else:
                np.testing.assert_allclose(kq[b, c, :k], sc, rtol=RTOL, atol=0)
            assert (kp[b, c, k:] == -1).all() and (kq[b, c, k:] == -1.0).all()          # nothing written past the picks
    return picks


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 511, 512, 513, 1025])
def test_bare_linear_bit_exact_at_each_size(n):
    rng = np.random.default_rng(100 + n)
    picks = check_bare([[random_class(rng, n, quantum=1 / 64)]], 1, 1, 1100, S.LINEAR)     # quantised scores: ties between candidates
    assert (picks > 0) == (n > 0)


def test_bare_linear_stops_at_max_picks():
    n = 300
    g = np.arange(n)
    lo = np.stack([(g % 20) * 0.05, (g // 20) * 0.05], 1)
    boxes = np.concatenate([lo, lo + 0.04], 1).astype(np.float32)                           # a 20 x 15 grid of disjoint boxes
    scores = np.linspace(0.95, 0.3, n).astype(np.float32)
    assert check_bare([[(boxes, scores)]], 1, 1, 1100, S.LINEAR, max_picks=200) == 200


def test_bare_linear_255_classes_and_per_image_offsets():
    rng = np.random.default_rng(7)
    cls = [[random_class(rng, int(rng.integers(0, 4)), size=(0.3, 0.6)) for _ in range(255)]]
    assert check_bare(cls, 1, 255, 130, S.LINEAR) > 100
    cls = [[random_class(rng, int(rng.integers(0, 90)) * (c != 2), size=(0.2, 0.5)) for c in range(5)] for _ in range(3)]
    assert len({tuple(len(x[1]) for x in row) for row in cls}) == 3
    assert check_bare(cls, 3, 5, 100, S.LINEAR) > 30
    assert check_bare(cls, 3, 5, 100, S.LINEAR, thr=0.0, keep=0.3) > 10
    assert check_bare(cls, 3, 5, 100, S.LINEAR, keep=1e-6, max_picks=7) > 10


def test_bare_linear_identical_boxes_and_degenerate_boxes():
    rng = np.random.default_rng(11)
    n = 200
    _, scores = random_class(rng, n)
    same = np.tile(np.asarray([[0.2, 0.3, 0.6, 0.8]], np.float32), (n, 1))
    assert check_bare([[(same, scores)]], 1, 1, 256, S.LINEAR) == 1                          # IoU = 1 exactly: every other score becomes 0
    boxes, scores = random_class(rng, n, size=(0.1, 0.4))
    nan = np.float32("nan")
    boxes[5] = [0.4, 0.4, 0.4, 0.4]; boxes[6] = [0.4, 0.4, 0.4, 0.4]                      # empty, twice at one point (0 / 0)
    boxes[17] = [0.3, 0.2, 0.3, 0.9]                                                         # zero width
    boxes[30] = [nan, 0.1, 0.5, 0.5]; boxes[31] = [0.1, 0.1, 0.5, nan]; boxes[0] = [0.2, nan, 0.7, 0.7]
    boxes[40] = [0.6, 0.6, 0.2, 0.2]                                                         # inverted: negative extents
    for method in (S.LINEAR, S.GAUSSIAN):
        pos, sc, _ = S.soft_nms_sorted(boxes, scores, method, 0.45, 0.5, 0.2, 200)
        assert {0, 5, 6, 17, 30, 31} <= set(pos.tolist())                                    # never decayed: w = 1
        for j in (0, 5, 6, 17, 30, 31):
            assert sc[pos.tolist().index(j)] == scores[j]
    check_bare([[(boxes, scores)]], 1, 1, 256, S.LINEAR)


@pytest.mark.parametrize("P", [8732, 24564])
def test_bare_linear_dense_single_class(P):
    rng = np.random.default_rng(P)
    assert check_bare([[random_class(rng, P, size=(0.05, 0.5))]], 1, 1, P, S.LINEAR) == 200


GAUSS_SEEDS = {0.5: 15, 0.1: 2}         # sigma -> seed with reference margin >= 1e-4 (searched on the CPU)


def gaussian_classes(seed):
    rng = np.random.default_rng(seed)
    return [[random_class(rng, int(rng.integers(20, 140)), lo=0.25, size=(0.1, 0.45)) for _ in range(4)] for _ in range(2)]


@pytest.mark.parametrize("sigma", sorted(GAUSS_SEEDS))
def test_bare_gaussian_with_margin(sigma):
    picks = check_bare(gaussian_classes(GAUSS_SEEDS[sigma]), 2, 4, 150, S.GAUSSIAN, sigma=sigma, exact=False, min_margin=MARGIN)
    assert picks > 100


def test_bare_gaussian_dense_invariants():
    n, keep, top_k = 8732, 0.2, 200
    rng = np.random.default_rng(5)
    boxes, scores = random_class(rng, n, size=(0.05, 0.5))
    kp, kq, kc = run_bare(*pack([[(boxes, scores)]], 1, 1, n), S.GAUSSIAN, 0.45, 0.5, keep, top_k)
    k = int(kc[0, 0])
    # kept_cnt = min(top_k, picks the rule can make): on this input the reference reaches the limit with scores far above keep_score
    pos, sc, _ = S.soft_nms_sorted(boxes, scores, S.GAUSSIAN, 0.45, 0.5, keep, top_k)
    assert pos.shape[0] == top_k and sc[-1] > 1.5 * keep
    assert k == top_k
    q = kq[0, 0, :k]
    assert (np.diff(q) <= 0).all() and (q >= np.float32(keep)).all() and q[0] == scores[0]
    p = kp[0, 0, :k]
    assert len(set(p.tolist())) == k and (p >= 0).all() and (p < n).all()


# ---- end to end --------------------------------------------------------------------------------------------------------------
def e2e_image(C, seed):
    """Sparse candidates: every prior strong background (-8, +8 on the last column) except 400 (60 at C = 2) random priors with
    standard_normal * 3 rows; l = standard_normal * 0.5."""
    rng = np.random.default_rng(seed)
    l_ = rng.standard_normal((8732, 4), dtype=np.float32) * np.float32(0.5)
    c_ = np.full((8732, C), -8.0, np.float32)
    c_[:, C - 1] = 8.0
    fg = rng.choice(8732, 60 if C == 2 else 400, replace=False)
    c_[fg] = rng.standard_normal((fg.size, C), dtype=np.float32) * np.float32(3.0)
    return l_, c_


# (C, rule) -> per-image seeds and top_k, searched on the CPU with the reference: margin >= 1e-4, order margin >= 1e-5
# (margins found: 1.1e-4 .. 2.1e-3; order margins 1.3e-5 .. 3.4e-5).  C = 21: about 500 picks compete for top_k = 200 (radix
# select); C = 81 with top_k = 600 and C = 2: everything is emitted, class-major.
E2E = {
    (2, "linear"): ((7, 8, 12), 200), (2, "gaussian"): ((2, 6, 7), 200),
    (21, "linear"): ((0, 2, 3), 200), (21, "gaussian"): ((10, 12, 16), 200),
    (81, "linear"): ((2, 3, 4), 600), (81, "gaussian"): ((2, 3, 6), 600),
}


@functools.lru_cache(maxsize=None)
def e2e_reference(C, nms, seed, top_k):
    l_, c_ = e2e_image(C, seed)
    return (l_, c_) + S.decode_soft_nms(l_, c_, 300, 300, top_k=top_k, nms=nms)


def _compare(got, ids, ref, what):
    rb, rc, rp, ri, info = ref
    print(f"{what}: reference margin {info['margin']:.3e}, order margin {info['order_margin']:.3e}, total {info['total']}")
    assert info["margin"] >= MARGIN and info["order_margin"] >= ORDER_MARGIN, (what, info)
    gb, gc, gp = (x.cpu().numpy() for x in got)
    assert gb.shape[0] == rb.shape[0], what
    assert np.array_equal(ids.cpu().numpy(), ri) and np.array_equal(gc, rc), what
    np.testing.assert_allclose(gp, rp, rtol=RTOL, atol=0)
    np.testing.assert_allclose(gb, rb, rtol=1e-5, atol=1e-3)       # pixels at 300: the hard path's tests ask no more of the boxes
    return info["total"]


@pytest.mark.parametrize("nms", ["linear", "gaussian"])
@pytest.mark.parametrize("C,B", [(21, 1), (21, 3), (81, 1), (81, 3), (2, 1)])
def test_inference_soft_end_to_end(C, B, nms):
    from objectdetection_ssd_amd import Losses
    seeds, top_k = E2E[C, nms]
    refs = [e2e_reference(C, nms, s, top_k) for s in seeds[:B]]
    if B == 1:
        out = Losses.inference(_t(refs[0][0]), _t(refs[0][1]), (300, 300), top_k=top_k, toDraw=False, nms=nms)
        got = [(out, Losses.inference.last_prior_ids)]
    else:
        res = Losses.inference_batch(_t(np.stack([r[0] for r in refs])), _t(np.stack([r[1] for r in refs])), [(300, 300)] * B,
                                     top_k=top_k, nms=nms)
        got = list(zip(res, Losses.inference_batch.last_prior_ids))
    for b, ((o, ids), r) in enumerate(zip(got, refs)):
        assert _compare(o, ids, r[2:], (C, B, nms, b)) > 0


def test_both_sides_of_top_k_occur():
    below = above = 0
    for (C, nms), (seeds, top_k) in E2E.items():
        for s in seeds:
            total = e2e_reference(C, nms, s, top_k)[-1]["total"]
            below += total <= top_k
            above += total > top_k
    assert below > 0 and above > 0, (below, above)


def test_coco_style_setting_keeps_decayed_boxes():
    """min_score 0.01, keep_score 0.001: keep_score below min_score, far more candidates than picks"""
    from objectdetection_ssd_amd import Losses
    l_, c_ = e2e_image(21, 1)
    kw = dict(top_k=200, min_score=0.01, iou_threshold=0.45, nms="gaussian", sigma=0.5, keep_score=0.001)
    rb, rc, rp, ri, info = S.decode_soft_nms(l_, c_, 300, 300, **kw)
    boxes, classes, probs = Losses.inference(_t(l_), _t(c_), (300, 300), toDraw=False, **kw)
    assert boxes.shape[0] == rb.shape[0] == 200 and info["total"] > 200
    # No margin at this density (~1e-7), so near-ties may trade places; the gaussian rule is continuous in the scores, so the sorted
    # scores still agree.  Tolerance: a score carries at most top_k = 200 factors, each an expf (<= 2 ulps) and a product (1/2 ulp)
    # on either side: 200 x 2.5 x 2^-23 = 6e-5.
    np.testing.assert_allclose(np.sort(probs.cpu().numpy()), np.sort(rp), rtol=6e-5, atol=0)
    assert float(probs.min()) >= 0.001 and (np.diff(probs.cpu().numpy()) <= 0).all()


def _padded_inputs(B=3):
    """three images of the C = 81 cases: fewer picks than top_k = 600, so the padded rows end in zeros"""
    seeds, top_k = E2E[81, "linear"]
    imgs = [e2e_image(81, s) for s in seeds[:B]]
    return (_t(np.stack([i[0] for i in imgs])), _t(np.stack([i[1] for i in imgs])), torch.tensor([[300., 300.]] * B, device=DEV),
            top_k)


def test_padded_form_equals_list_form_and_pads_with_zeros():
    from objectdetection_ssd_amd import Losses
    l, c, wh, top_k = _padded_inputs()
    boxes, classes, probs, ids, count = Losses.inference_batch_padded(l, c, wh, top_k=top_k, nms="linear")
    res = Losses.inference_batch(l, c, wh, top_k=top_k, nms="linear")
    assert tuple(boxes.shape) == (3, top_k, 4) and count.dtype == torch.int32
    for b, k in enumerate(count.tolist()):
        assert 0 < k < top_k
        assert torch.equal(boxes[b, :k], res[b][0]) and torch.equal(classes[b, :k], res[b][1]) and torch.equal(probs[b, :k], res[b][2])
        assert torch.equal(ids[b, :k], Losses.inference_batch.last_prior_ids[b])
        assert not boxes[b, k:].any() and not classes[b, k:].any() and not probs[b, k:].any() and not ids[b, k:].any()


def test_hard_keyword_is_bitwise_the_call_without_it():
    from objectdetection_ssd_amd import Losses
    rng = np.random.default_rng(3)
    l = _t(rng.standard_normal((3, 8732, 4), dtype=np.float32) * np.float32(0.5))
    c = _t(rng.standard_normal((3, 8732, 21), dtype=np.float32) * np.float32(3.0))
    wh = torch.tensor([[300., 300.], [500., 375.], [640., 480.]], device=DEV)
    plain = Losses.inference_batch_padded(l, c, wh)
    keyed = Losses.inference_batch_padded(l, c, wh, nms="hard", sigma=0.3, keep_score=0.5)
    assert int(plain[4].sum()) > 0
    for a, b in zip(plain, keyed):
        assert a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize("nms", ["linear", "gaussian"])
def test_disjoint_boxes_soft_equals_hard_bitwise(nms):
    from objectdetection_ssd_amd import Losses
    imgs = [S.disjoint_inputs(21, s) for s in (5, 6)]
    l, c = _t(np.stack([i[0] for i in imgs])), _t(np.stack([i[1] for i in imgs]))
    wh = torch.tensor([[300., 300.]] * 2, device=DEV)
    hard = Losses.inference_batch_padded(l, c, wh)
    soft = Losses.inference_batch_padded(l, c, wh, nms=nms)
    assert int(hard[4].min()) > 10
    for a, b in zip(hard, soft):
        assert torch.equal(a, b)


def test_padded_gaussian_decode_replays_from_a_graph():
    from objectdetection_ssd_amd import Losses
    l, c, wh, top_k = _padded_inputs()
    eager = [x.clone() for x in Losses.inference_batch_padded(l, c, wh, top_k=top_k, nms="gaussian")]
    assert int(eager[4].min()) > 0
    torch.cuda.synchronize()
    from objectdetection_ssd_amd import ops
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        Losses.inference_batch_padded(l, c, wh, top_k=top_k, nms="gaussian")              # warm-up on the capture stream (its workspace)
        st.synchronize()
        graph = torch.cuda.CUDAGraph()
        with ops.capture_workspaces() as held, torch.cuda.graph(graph, stream=st):
            out = Losses.inference_batch_padded(l, c, wh, top_k=top_k, nms="gaussian")
    torch.cuda.synchronize()
    assert held
    for _ in range(2):
        for x in out:
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, out):
            assert torch.equal(a, b)

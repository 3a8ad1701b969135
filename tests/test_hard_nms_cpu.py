"""The greedy-NMS / top-k reference (tests/hard_nms_ref.py) without a GPU: it reproduces the oracle's decode on the golden cases, agrees
with the Soft-NMS reference where the two rules coincide, gives the hand-written keep lists at exact-equality IoUs and threshold
edges; and the host-side launch plan of the greedy kernel (ssd_nms_plan) and the argument checks of the bare entry points."""
import ctypes
import os

import numpy as np
import pytest

import hard_nms_ref as H
import soft_nms_ref as S
import ssd_oracle as O
from helpers import nms_case
from nms_cases import lattice_pair, near_threshold_pairs, random_class

OK_PTR, ODD_PTR = 0x10000, 0x10004


@pytest.mark.parametrize("ni", range(6))
def test_reference_reproduces_the_golden_decodes(gold_dir, ni):
    """oracle decode up to the sorted candidates, then greedy_nms_sorted, then topk_emit_ref == O.decode_nms, exactly"""
    z = np.load(os.path.join(gold_dir, "nms.npz"))
    l_, c_, top_k, p = nms_case(z, ni)
    w, h = [int(v) for v in z["img_wh"]]
    ob, oc, op_, oi = O.decode_nms(l_, c_, w, h, top_k=top_k)
    b, c, pr, i, info = H.decode_hard_nms(l_, c_, w, h, top_k=top_k)
    assert b.shape == ob.shape == z[p + "boxes"].shape
    assert np.array_equal(b.view(np.uint32), ob.view(np.uint32)) and np.array_equal(c, oc) and np.array_equal(i, oi)
    assert np.array_equal(pr.view(np.uint32), op_.view(np.uint32))
    assert (info["total"] == 0) == (ni == 5)


def test_both_sides_of_top_k_occur_among_the_golden_cases(gold_dir):
    z = np.load(os.path.join(gold_dir, "nms.npz"))
    sides = set()
    for ni in range(6):
        l_, c_, top_k, _ = nms_case(z, ni)
        sides.add(H.decode_hard_nms(l_, c_, 300, 300, top_k=top_k)[4]["total"] > top_k)
    assert sides == {False, True}


def test_disjoint_boxes_equal_the_soft_rule():
    n = 300
    g = np.arange(n)
    lo = np.stack([(g % 20) * 0.05, (g // 20) * 0.05], 1)
    boxes = np.concatenate([lo, lo + 0.04], 1).astype(np.float32)          # a 20 x 15 grid of disjoint boxes
    scores = np.linspace(0.95, 0.3, n).astype(np.float32)
    kept = H.greedy_nms_sorted(boxes, scores, 0.45)
    for method in (S.LINEAR, S.GAUSSIAN):
        pos, sc, _ = S.soft_nms_sorted(boxes, scores, method, 0.45, 0.5, 0.2, n)
        assert np.array_equal(kept, pos) and np.array_equal(sc, scores)
    assert kept.tolist() == list(range(n))


def test_against_the_matrix_form_on_random_boxes():
    """the row-per-kept-box form against the oracle's own loop over the full IoU matrix"""
    rng = np.random.default_rng(4)
    for n, size in ((1, (0.1, 0.3)), (2, (0.5, 0.9)), (257, (0.05, 0.3)), (700, (0.3, 0.6))):
        boxes, scores = random_class(rng, n, size=size)
        iou = O.iou_matrix(boxes, boxes)
        sup = np.zeros(n, bool)
        for i in range(n):
            if sup[i]:
                continue
            sup |= iou[i] >= np.float32(0.45)
            sup[i] = False
        assert np.array_equal(H.greedy_nms_sorted(boxes, scores, 0.45), np.nonzero(~sup)[0])
    assert H.greedy_nms_sorted(np.zeros((0, 4), np.float32), np.zeros(0, np.float32), 0.45).shape == (0,)


def test_hand_cases_exact_equality_and_threshold_edges():
    up = lambda v: np.nextafter(np.float32(v), np.float32(2))
    sc2 = np.asarray([0.9, 0.8], np.float32)
    for (width, shift), iou in (((3, 1), 0.5), ((5, 3), 0.25)):
        pair = lattice_pair(width, shift)
        assert S.iou_one_to_many(pair[0], pair[1:])[0] == np.float32(iou)      # exactly
        assert H.greedy_nms_sorted(pair, sc2, iou).tolist() == [0]              # >= : suppressed at equality
        assert H.greedy_nms_sorted(pair, sc2, up(iou)).tolist() == [0, 1]       # one ulp above: not
    # A, B (IoU with A = 0.5), C disjoint, D = A again
    boxes = np.asarray([[0, 0, 1, 1], [0, 0, 1, 0.5], [2, 2, 3, 3], [0, 0, 1, 1]], np.float32)
    sc = np.asarray([0.9, 0.8, 0.7, 0.6], np.float32)
    assert H.greedy_nms_sorted(boxes, sc, 0.45).tolist() == [0, 2]
    assert H.greedy_nms_sorted(boxes, sc, 0.5).tolist() == [0, 2]
    assert H.greedy_nms_sorted(boxes, sc, 0.6).tolist() == [0, 1, 2]              # D falls to A (IoU 1), B stays
    assert H.greedy_nms_sorted(boxes, sc, 1.0).tolist() == [0, 1, 2]              # IoU = 1 exactly is >= 1
    assert H.greedy_nms_sorted(boxes, sc, 1.5).tolist() == [0, 1, 2, 3]           # nothing reaches 1.5
    assert H.greedy_nms_sorted(boxes, sc, 0.0).tolist() == [0]                    # IoU 0 >= 0: disjoint boxes fall too
    assert H.greedy_nms_sorted(boxes, sc, -0.1).tolist() == [0]
    assert H.greedy_nms_sorted(boxes, sc, 1e-30).tolist() == [0, 2]               # any overlap, but not none
    # suppression is by KEPT boxes only: B (suppressed by A) does not suppress E, which overlaps B alone
    chain = np.asarray([[0, 0, 1, 1], [0.5, 0, 1.5, 1], [1.05, 0, 2.05, 1]], np.float32)   # IoU(A,B) = 1/3, IoU(B,E) = 0.29, IoU(A,E) = 0
    assert H.greedy_nms_sorted(chain, sc[:3], 0.25).tolist() == [0, 2]
    # two empty boxes at one point: 0 / 0 = NaN, not >= anything; a NaN coordinate: NaN with every box.  An empty box against a
    # box with an area, and the inverted box (both extents negative: area +0.16, never an intersection) give IoU 0: kept at any
    # positive threshold, suppressed at thr = 0 -- where only the NaN pairs survive
    nan = np.float32("nan")
    odd = np.asarray([[0.5, 0.5, 0.5, 0.5], [0.5, 0.5, 0.5, 0.5], [0, nan, 1, 1], [0, 0, 1, 1], [0.6, 0.6, 0.2, 0.2]], np.float32)
    so = np.linspace(0.9, 0.5, 5).astype(np.float32)
    assert np.isnan(S.iou_one_to_many(odd[0], odd[1:2])[0]) and S.iou_one_to_many(odd[0], odd[3:4])[0] == 0
    assert H.greedy_nms_sorted(odd, so, 0.45).tolist() == [0, 1, 2, 3, 4]
    assert H.greedy_nms_sorted(odd, so, 1e-30).tolist() == [0, 1, 2, 3, 4]
    assert H.greedy_nms_sorted(odd, so, 0.0).tolist() == [0, 1, 2]


def test_near_threshold_pairs_take_both_outcomes():
    """the construction the GPU test relies on: IoU within 1e-5 * thr of thr, both outcomes"""
    thr = 0.45
    boxes = near_threshold_pairs(np.random.default_rng(9), 100, thr)
    iou = np.asarray([S.iou_one_to_many(boxes[2 * k], boxes[2 * k + 1:2 * k + 2])[0] for k in range(100)], np.float64)
    near = np.abs(iou - np.float32(thr)) <= 1e-5 * thr
    assert near.sum() >= 64
    hit = iou[near] >= np.float32(thr)
    assert hit.any() and (~hit).any()
    kept = H.greedy_nms_sorted(boxes, np.linspace(0.9, 0.3, 200).astype(np.float32), thr)
    assert set(np.arange(0, 200, 2)) <= set(kept.tolist())
    assert [(2 * k + 1) not in set(kept.tolist()) for k in range(100)] == (iou >= np.float32(thr)).tolist()


def test_topk_emit_reference_on_a_hand_case():
    P, C1 = 6, 3
    s_boxes = np.arange(C1 * P * 4, dtype=np.float32).reshape(C1, P, 4) / 128
    s_idx = np.arange(C1 * P, dtype=np.int32).reshape(C1, P) + 100
    kept_pos = np.asarray([[0, 2, 5, 0, 0, 0], [0] * 6, [1, 3, 0, 0, 0, 0]], np.int32)
    kept_prob = np.asarray([[0.75, 0.5, 0.5, 0, 0, 0], [0] * 6, [0.5, 0.25, 0, 0, 0, 0]], np.float32)
    kept_cnt = np.asarray([3, 0, 2, 77], np.int32)                               # (a fourth entry, the kernels' stride, is ignored)
    b, c, p, i = H.topk_emit_ref(s_boxes, s_idx, kept_pos, kept_prob, kept_cnt, 5, 10.0, 20.0)
    assert c.tolist() == [0, 0, 0, 2, 2] and i.tolist() == [100, 102, 105, 113, 115]          # total <= top_k: class-major, unsorted
    assert np.array_equal(b[1], s_boxes[0, 2] * np.asarray([10, 20, 10, 20], np.float32))
    b, c, p, i = H.topk_emit_ref(s_boxes, s_idx, kept_pos, kept_prob, kept_cnt, 3, 10.0, 20.0)
    assert p.tolist() == [0.75, 0.5, 0.5] and c.tolist() == [0, 0, 0]                          # the tie at 0.5: class-major, class 2 loses
    b, c, p, i = H.topk_emit_ref(s_boxes, s_idx, kept_pos, kept_prob, kept_cnt, 4, 10.0, 20.0)
    assert p.tolist() == [0.75, 0.5, 0.5, 0.5] and c.tolist() == [0, 0, 0, 2] and i.tolist() == [100, 102, 105, 113]
    b, c, p, i = H.topk_emit_ref(s_boxes, s_idx, kept_pos, kept_prob, np.zeros(4, np.int32), 4, 10.0, 20.0)
    assert b.shape == (0, 4) and c.shape == p.shape == i.shape == (0,)


# ---- the library's host side ---------------------------------------------------------------------------------------------------
def plan(B, C1, P):
    from objectdetection_ssd_amd import _lib
    lib = _lib.load()
    t, w = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = lib.ssd_nms_plan(B, C1, P, ctypes.byref(t), ctypes.byref(w))
    return rc, t.value, w.value


def test_plan_values_of_the_benchmarked_configurations():
    assert plan(1, 20, 8732) == (0, 1024, 8768)
    assert plan(32, 20, 8732) == (0, 512, 4608)
    assert plan(1, 20, 24564) == (0, 1024, 17536)
    assert plan(32, 20, 24564) == (0, 512, 12288)
    # the block size follows C1 * B <= 128; chunk_words always holds 32 rows of all ceil(P / 64) column words
    assert plan(6, 20, 8732)[1] == 1024 and plan(7, 20, 8732)[1:] == (512, 4608)
    assert plan(1, 128, 8732)[1] == 1024 and plan(1, 129, 8732)[1] == 512
    assert plan(1, 1, 1) == (0, 1024, 64) and plan(7, 20, 2112) == (0, 512, 4608) and plan(1, 1, 2112) == (0, 1024, 2112)
    for B, C1, P in ((1, 20, 8732), (32, 20, 8732), (1, 20, 24564), (32, 20, 24564), (32, 255, 34752), (1, 1, 34752)):
        rc, t, w = plan(B, C1, P)
        nwcap = (P + 63) // 64
        assert rc == 0 and w >= 32 * nwcap and (nwcap + w) * 8 <= 140 * 1024


def test_plan_refuses_what_the_launcher_refuses():
    # 32 rows x ceil(P / 64) words beside the removed-bitset exceed 140 KB from P = 34 753 on (544 column words)
    assert plan(1, 20, 34752)[0] == 0 and plan(32, 20, 34752)[0] == 0
    assert plan(1, 20, 34753)[0] == -1 and plan(32, 20, 34753)[0] == -1 and plan(1, 20, 100000)[0] == -1
    for B, C1, P in ((0, 20, 8732), (65536, 20, 8732), (1, 0, 8732), (1, 256, 8732), (1, 20, 0), (1, 20, 100001)):
        assert plan(B, C1, P)[0] == -1, (B, C1, P)
    from objectdetection_ssd_amd import _lib
    lib = _lib.load()
    t = ctypes.c_int(0)
    assert lib.ssd_nms_plan(1, 20, 8732, None, ctypes.byref(t)) == -3 and lib.ssd_nms_plan(1, 20, 8732, ctypes.byref(t), None) == -3


def test_bare_entry_points_validate_before_launching():
    """nothing is enqueued for a refused call, so the made-up pointer values are never dereferenced"""
    from objectdetection_ssd_amd import _lib
    lib = _lib.load()
    for name in ("ssd_nms_plan", "ssd_nms_sorted", "ssd_topk_emit_sorted", "ssd_decode_sorted", "ssd_decode_sorted_workspace"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    P = OK_PTR

    # the keys: 8 bytes per (image, class, prior), rounded up to 256
    assert lib.ssd_decode_sorted_workspace(2, 8732, 21) == 2 * 20 * 8732 * 8 == 2794240 and 2794240 % 256 == 0
    assert lib.ssd_decode_sorted_workspace(1, 1, 2) == 256 and lib.ssd_decode_sorted_workspace(3, 577, 256) == (3 * 255 * 577 * 8 + 255) // 256 * 256
    assert lib.ssd_decode_sorted_workspace(0, 8732, 21) == lib.ssd_decode_sorted_workspace(1, 0, 21) == lib.ssd_decode_sorted_workspace(1, 8732, 1) == 0
    dneed = lib.ssd_decode_sorted_workspace(2, 8732, 21)

    def dec(B=2, n=8732, C=21, ws_bytes=dneed, clear=0, **ptr):
        a = dict(l=P, c=P, pri=P, boxes=P, s_boxes=P, s_prob=P, s_idx=P, cnt=P, ws=P)
        a.update(ptr)
        return lib.ssd_decode_sorted(a["l"], a["c"], a["pri"], B, n, C, 0.2, a["boxes"], a["s_boxes"], a["s_prob"], a["s_idx"], a["cnt"],
                                     a["ws"], ws_bytes, None, clear)

    for name in ("l", "c", "pri", "boxes", "s_boxes", "s_prob", "s_idx", "cnt", "ws"):
        assert dec(**{name: None}) == -3, name
    for kw in (dict(B=0), dict(B=65536), dict(n=0), dict(n=100001), dict(C=1), dict(C=257), dict(clear=2), dict(clear=-1)):
        assert dec(**kw) == -1, kw
    for name in ("l", "pri", "boxes", "s_boxes", "ws"):
        assert dec(**{name: ODD_PTR}) == -5, name
    for name in ("c", "s_prob", "s_idx", "cnt"):                        # read and written four bytes at a time: any float address
        assert dec(**{name: ODD_PTR}, ws_bytes=dneed - 1) == -2, name
    assert dec(ws_bytes=dneed - 1) == -2 and dec(ws_bytes=dneed - 1, clear=1) == -2
    assert dec(B=3, ws_bytes=dneed) == -2 and dec(C=22, ws_bytes=dneed) == -2
    assert dec(ws=None, ws_bytes=0) == -3 and dec(B=0, ws_bytes=0) == -1 and dec(l=ODD_PTR, ws_bytes=0) == -5     # in that order

    def nms(B=1, C1=20, n=8732, boxes=P, prob=P, cnt=P, kpos=P, kprob=P, kcnt=P):
        return lib.ssd_nms_sorted(boxes, prob, cnt, B, C1, n, 0.45, kpos, kprob, kcnt, None)

    for kw in (dict(boxes=None), dict(prob=None), dict(cnt=None), dict(kpos=None), dict(kprob=None), dict(kcnt=None)):
        assert nms(**kw) == -3, kw
    for kw in (dict(B=0), dict(B=65536), dict(C1=0), dict(C1=256), dict(n=0), dict(n=100001), dict(n=34753)):
        assert nms(**kw) == -1, kw
    assert nms(boxes=ODD_PTR) == -5

    K = 2 * 20 * 8732
    need = 2 * ((K * 4 + 255) // 256 * 256)

    def topk(B=2, C1=20, n=8732, top_k=200, ws_bytes=need, **ptr):
        a = dict(s_boxes=P, s_idx=P, kept_pos=P, kept_prob=P, kept_cnt=P, wh=P, boxes=P, classes=P, probs=P, ids=P, count=P, ws=P)
        a.update(ptr)
        return lib.ssd_topk_emit_sorted(a["s_boxes"], a["s_idx"], a["kept_pos"], a["kept_prob"], a["kept_cnt"], a["wh"], B, C1, n, top_k,
                                        a["boxes"], a["classes"], a["probs"], a["ids"], a["count"], a["ws"], ws_bytes, None)

    for name in ("s_boxes", "s_idx", "kept_pos", "kept_prob", "kept_cnt", "wh", "boxes", "classes", "probs", "ids", "count", "ws"):
        assert topk(**{name: None}) == -3, name
    for kw in (dict(B=0), dict(C1=0), dict(C1=256), dict(n=0), dict(n=100001), dict(top_k=0), dict(top_k=4097)):
        assert topk(**kw) == -1, kw
    for name in ("s_boxes", "boxes", "ws"):
        assert topk(**{name: ODD_PTR}) == -5, name
    assert topk(ws_bytes=need - 1) == -2

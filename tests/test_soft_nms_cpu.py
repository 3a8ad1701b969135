"""Soft-NMS without a GPU: the numpy reference (tests/soft_nms_ref.py) on cases worked out by hand, the C ABI's exports and argument
checks (nothing is enqueued for a refused call, so made-up pointer values are never dereferenced), and the keyword checks of Losses."""
import numpy as np
import pytest
import torch

import class_count_ref as R
import soft_nms_ref as S

OK_PTR, ODD_PTR = 0x10000, 0x10004


def test_hand_case_linear_and_gaussian():
    boxes = np.asarray([[0, 0, 1, 1], [0, 0, 1, 0.5], [2, 2, 3, 3]], np.float32)          # A, B (IoU with A = 0.5), C disjoint
    scores = np.asarray([0.9, 0.8, 0.7], np.float32)
    pos, sc, _ = S.soft_nms_sorted(boxes, scores, S.LINEAR, 0.45, 0.5, 0.2, 200)
    assert pos.tolist() == [0, 2, 1]
    assert sc.tolist() == [np.float32(0.9), np.float32(0.7), np.float32(0.8) * np.float32(0.5)]
    pos, sc, _ = S.soft_nms_sorted(boxes, scores, S.GAUSSIAN, 0.45, 0.5, 0.2, 200)
    assert pos.tolist() == [0, 2, 1]
    assert sc[0] == np.float32(0.9) and sc[1] == np.float32(0.7)
    np.testing.assert_allclose(sc[2], 0.8 * np.exp(-0.5), rtol=1e-6)
    # a higher keep_score drops B once it has decayed to 0.4; the pick limit cuts the list
    pos, sc, _ = S.soft_nms_sorted(boxes, scores, S.LINEAR, 0.45, 0.5, 0.5, 200)
    assert pos.tolist() == [0, 2]
    pos, sc, _ = S.soft_nms_sorted(boxes, scores, S.LINEAR, 0.45, 0.5, 0.2, 1)
    assert pos.tolist() == [0]
    # IoU 0.5 is not beyond a threshold of 0.5: no decay, sorted order
    pos, sc, _ = S.soft_nms_sorted(boxes, scores, S.LINEAR, 0.5, 0.5, 0.2, 200)
    assert pos.tolist() == [0, 1, 2] and sc.tolist() == scores.tolist()


def test_margin_reports_the_nearest_decision():
    boxes = np.asarray([[0, 0, 1, 1], [0, 0, 1, 0.5], [2, 2, 3, 3]], np.float32)
    scores = np.asarray([0.9, 0.8, 0.7], np.float32)
    _, _, m = S.soft_nms_sorted(boxes, scores, S.LINEAR, 0.45, 0.5, 0.2, 200)
    assert m == pytest.approx(1 / 9, rel=1e-5)                     # 0.9 against the runner-up 0.8, and IoU 0.5 against 0.45
    _, _, m = S.soft_nms_sorted(boxes, scores, S.LINEAR, 0.4999, 0.5, 0.2, 200)
    assert m == pytest.approx(0.0001 / 0.4999, rel=1e-2)
    _, _, m = S.soft_nms_sorted(boxes, np.asarray([0.9, 0.9, 0.7], np.float32), S.GAUSSIAN, 0.45, 0.5, 0.2, 200)
    assert m == 0.0                                                # a tie for the pick


def test_non_finite_iou_means_no_decay():
    nan = np.float32("nan")
    boxes = np.asarray([[0.5, 0.5, 0.5, 0.5], [0.5, 0.5, 0.5, 0.5], [0, nan, 1, 1], [0, 0, 1, 1]], np.float32)    # two empty boxes at one point: 0 / 0
    scores = np.asarray([0.9, 0.8, 0.7, 0.6], np.float32)
    for method in (S.LINEAR, S.GAUSSIAN):
        pos, sc, _ = S.soft_nms_sorted(boxes, scores, method, 0.45, 0.5, 0.2, 200)
        assert pos.tolist() == [0, 1, 2, 3] and sc.tolist() == scores.tolist()


@pytest.mark.parametrize("nms", ["linear", "gaussian"])
def test_disjoint_boxes_equal_the_hard_rule_exactly(nms):
    l_, c_ = S.disjoint_inputs(21, 5)
    hb, hc, hp, hi = R.decode_nms(l_, c_, 300, 300)
    sb, sc, sp, si, info = S.decode_soft_nms(l_, c_, 300, 300, nms=nms)
    assert hb.shape[0] > 10 and info["total"] == hb.shape[0]
    assert np.array_equal(hb, sb) and np.array_equal(hc, sc) and np.array_equal(hp, sp) and np.array_equal(hi, si)


def test_identical_boxes_under_linear_leave_one_survivor_per_class():
    l_ = np.zeros((8732, 4), np.float32)
    c_ = np.full((8732, 5), -8.0, np.float32)
    c_[:, 4] = 8.0
    pri = np.tile(np.asarray([[0.5, 0.5, 0.2, 0.3]], np.float32), (8732, 1))       # every prior the same box
    rng = np.random.default_rng(3)
    for p in rng.choice(8732, 40, replace=False):
        c_[p] = -8.0
        c_[p, rng.integers(0, 3)] = rng.uniform(0.0, 3.0)
    sb, sc, sp, si, info = S.decode_soft_nms(l_, c_, 300, 300, nms="linear", pri_cxcywh=pri)
    assert sorted(sc.tolist()) == [0, 1, 2]                        # IoU = 1: every other score is multiplied by 0
    probs = torch.softmax(torch.from_numpy(c_), dim=1).numpy()
    for c, p, i in zip(sc, sp, si):
        assert p == probs[:, c].max() and i == int(np.argmax(probs[:, c]))


def test_new_symbols_are_exported():
    from objectdetection_ssd_amd import _lib
    lib = _lib.load()
    for name in ("ssd_decode_nms_soft", "ssd_decode_nms_batch_soft", "ssd_soft_nms_sorted"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.ssd_abi_version() == 1


def test_soft_entry_points_validate_before_launching():
    from objectdetection_ssd_amd import _lib
    lib = _lib.load()
    P = OK_PTR
    f = lib.ssd_soft_nms_sorted

    def bare(method=1, thr=0.45, sigma=0.5, keep=0.2, picks=200, B=1, C1=20, n=8732, boxes=P, prob=P, cnt=P, kpos=P, kprob=P, kcnt=P):
        return f(boxes, prob, cnt, B, C1, n, method, thr, sigma, keep, picks, kpos, kprob, kcnt, None)

    for kw in (dict(boxes=None), dict(prob=None), dict(cnt=None), dict(kpos=None), dict(kprob=None), dict(kcnt=None)):
        assert bare(**kw) == -3, kw
    for kw in (dict(method=0), dict(method=3), dict(method=-1), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")),
               dict(keep=0.0), dict(keep=1e-7), dict(keep=1.5), dict(keep=float("nan")), dict(thr=-0.1), dict(thr=1.1),
               dict(thr=float("nan")), dict(picks=0), dict(picks=4097), dict(B=0), dict(C1=0), dict(C1=256), dict(n=0),
               dict(n=40705)):                                      # 4 * P bytes of live scores beside the fixed part: P <= 40 704
        assert bare(**kw) == -1, kw
    assert bare(boxes=ODD_PTR) == -5

    ws = lib.ssd_decode_nms_batch_workspace(2, 8732, 21)
    fb = lib.ssd_decode_nms_batch_soft

    def batch(method=2, sigma=0.5, keep=0.2, thr=0.45, l=P, ws_bytes=ws, workspace=P, n=8732):
        return fb(l, P, P, P, 2, n, 21, 0.2, thr, 200, P, P, P, P, P, workspace, ws_bytes, None, method, sigma, keep)

    assert batch(l=None) == -3 and batch(workspace=None) == -3
    for kw in (dict(method=0), dict(method=3), dict(sigma=0.0), dict(keep=0.0), dict(keep=2.0), dict(thr=1.5), dict(n=40705)):
        assert batch(**kw) == -1, kw
    assert batch(l=ODD_PTR) == -5
    assert batch(ws_bytes=ws - 1) == -2

    ws1 = lib.ssd_decode_nms_workspace(8732, 21)
    f1 = lib.ssd_decode_nms_soft

    def single(method=1, sigma=0.5, keep=0.2, workspace=P, ws_bytes=ws1):
        return f1(P, P, P, 8732, 21, 0.2, 0.45, 200, 300.0, 300.0, P, P, P, P, P, workspace, ws_bytes, None, method, sigma, keep)

    assert single(workspace=None) == -3
    for kw in (dict(method=0), dict(method=5), dict(sigma=-0.5), dict(keep=1e-9)):
        assert single(**kw) == -1, kw
    assert single(ws_bytes=ws1 - 1) == -2


@pytest.mark.parametrize("fn", ["inference", "inference_batch", "inference_batch_padded"])
def test_unknown_rule_is_a_value_error_before_any_device_work(fn):
    from objectdetection_ssd_amd import Losses
    l_, c_ = torch.zeros(8732, 4), torch.zeros(8732, 21)           # host tensors: a device call would raise RuntimeError instead
    for bad in ("soft", "Hard", None, 1):
        with pytest.raises(ValueError, match="nms must be"):
            if fn == "inference":
                Losses.inference(l_, c_, (300, 300), toDraw=False, nms=bad)
            else:
                getattr(Losses, fn)(l_[None], c_[None], [(300, 300)], nms=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Losses.inference(l_, c_, (300, 300), toDraw=False, nms="gaussian")


def test_keywords_are_appended_with_their_defaults():
    import inspect
    from objectdetection_ssd_amd import Losses
    for fn in (Losses.inference, Losses.inference_batch, Losses.inference_batch_padded):
        names = list(inspect.signature(fn).parameters)
        assert names[-3:] == ["nms", "sigma", "keep_score"], names
        d = {k: v.default for k, v in inspect.signature(fn).parameters.items()}
        assert (d["nms"], d["sigma"], d["keep_score"]) == ("hard", 0.5, None)
    assert list(inspect.signature(Losses.inference).parameters)[:8] == ["l_", "c_", "index", "top_k", "phase", "toDraw", "min_score",
                                                                       "iou_threshold"]

"""Sigmoid scores in the decode without a GPU: the cases of tests/sigmoid_decode_ref.py meet their own precondition, the recorded
float32 distance is a fresh measurement, `ops.score_mode`, and the status answers of the *_score entries (returned before anything is
enqueued)."""
import json

import numpy as np
import pytest

import sigmoid_decode_ref as S

OK_PTR, ODD_PTR = 0x10000, 0x10004
BAD_SHAPE, WORKSPACE, NULL, ALIGN = -1, -2, -3, -5


@pytest.mark.parametrize("case_id", list(S.CASES))
def test_cases_and_fixture(case_id):
    l_, c_, pri = S.case(case_id)
    P, C, _ = S.CASES[case_id]
    assert c_.shape == (S.B, P, C) and l_.shape == (S.B, P, 4) and pri.shape == (P, 4)
    assert not S.near_cut(c_).any()
    cand = S.sigmoid64(c_)[..., :-1] >= float(np.float32(S.MIN_SCORE))
    assert cand.any(axis=1).all() and not cand.all()                       # every class of every image has candidates, and not every prior
    with open(S.GOLDEN) as f:
        gold = json.load(f)["d32"]
    assert set(gold) == set(S.CASES) and gold[case_id] == S.distance(case_id) and 0 < gold[case_id] < 2.0 ** -22


def test_score_mode_names():
    from objectdetection_ssd_amd import ops
    assert ops.score_mode("softmax") == 0 and ops.score_mode("sigmoid") == 1
    for bad in ("Sigmoid", "logistic", None, 1, ["sigmoid"]):
        with pytest.raises(ValueError):
            ops.score_mode(bad)


def test_status_answers_of_the_score_entries():
    from objectdetection_ssd_amd import _lib
    lib = _lib.load()
    B, P, C, top_k = 2, 777, 21, 200
    need = lib.ssd_decode_nms_batch_workspace(B, P, C)
    ptrs = [OK_PTR] * 6

    def batch(l_=OK_PTR, ws_bytes=need, method=0, sigma=0.5, keep=0.2, score_mode=1, c_=OK_PTR):
        return lib.ssd_decode_nms_batch_score(l_, c_, OK_PTR, OK_PTR, B, P, C, 0.2, 0.45, top_k, *ptrs[:5], OK_PTR, ws_bytes, None, method, sigma,
                                              keep, score_mode)

    assert batch(score_mode=2) == BAD_SHAPE and batch(score_mode=-1) == BAD_SHAPE and batch(method=3) == BAD_SHAPE and batch(method=-1) == BAD_SHAPE
    assert batch(method=2, sigma=0.0) == BAD_SHAPE and batch(method=1, keep=0.0) == BAD_SHAPE
    assert batch(c_=None) == NULL and batch(l_=ODD_PTR) == ALIGN and batch(ws_bytes=need - 1) == WORKSPACE
    assert batch(score_mode=2, c_=None) == BAD_SHAPE               # the entry's own arguments first, then the decode's order
    need1 = lib.ssd_decode_nms_workspace(P, C)

    def single(ws=OK_PTR, ws_bytes=need1, method=0, score_mode=1):
        return lib.ssd_decode_nms_score(OK_PTR, OK_PTR, OK_PTR, P, C, 0.2, 0.45, top_k, 300.0, 300.0, *ptrs[:5], ws, ws_bytes, None, method, 0.5,
                                        0.2, score_mode)

    assert single(score_mode=2) == BAD_SHAPE and single(method=3) == BAD_SHAPE and single(ws=None) == NULL and single(ws_bytes=need1 - 1) == WORKSPACE
    needs = lib.ssd_decode_sorted_workspace(B, P, C)

    def bare(c_=OK_PTR, boxes=OK_PTR, ws_bytes=needs, clear=0, score_mode=1):
        return lib.ssd_decode_sorted_score(OK_PTR, c_, OK_PTR, B, P, C, 0.2, boxes, OK_PTR, OK_PTR, OK_PTR, OK_PTR, OK_PTR, ws_bytes, None, clear,
                                           score_mode)

    assert bare(score_mode=2) == BAD_SHAPE and bare(clear=2) == BAD_SHAPE and bare(c_=None) == NULL and bare(boxes=ODD_PTR) == ALIGN
    assert bare(ws_bytes=needs - 1) == WORKSPACE

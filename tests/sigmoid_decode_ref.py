"""Inputs and an f64 restatement for the decode's first stage with sigmoid scores (csrc/nms.hip: decode_compact_kernel<., true> through
ssd_decode_sorted_score, score_mode 1), in numpy and torch alone -- no kernel of the package runs here.

The probability of class c in 0 .. C-2 at prior p is sigmoid(c_[p, c]); column C-1 takes no part.  Inputs are drawn as
tests/decode_sort_ref.py draws its sweep (rows N(0, 9), its offsets and priors); a logit whose f64 score lies within MARGIN = 1e-5
(relative) of min_score is drawn again until none is left, so the candidate set is decided by no rounding.

`python tests/sigmoid_decode_ref.py --record` writes tests/golden/sigmoid_decode_ref_distance.json: per case the largest relative
distance of torch's float32 sigmoid from the float64 one over the candidates (numbers only)."""
import json
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.join(os.path.dirname(_HERE), "oracle")):      # (`python tests/sigmoid_decode_ref.py` runs without tests/conftest.py)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import decode_sort_ref as D

GOLDEN = os.path.join(_HERE, "golden", "sigmoid_decode_ref_distance.json")
MIN_SCORE, MARGIN = 0.2, 1e-5
CASES = {"P777-C21": (777, 21, 11), "P1000-C21": (1000, 21, 12), "P1000-C81": (1000, 81, 13), "P777-C256": (777, 256, 14)}      # (P, C, seed)
B = 2
_cache = {}


def sigmoid64(c_):
    return torch.sigmoid(torch.tensor(np.asarray(c_, np.float32), dtype=torch.float64)).numpy()


def near_cut(c_, min_score=MIN_SCORE):
    cut = float(np.float32(min_score))
    return np.abs(sigmoid64(c_)[..., :-1] - cut) <= MARGIN * cut


def case(case_id):
    """-> l_ (B,P,4), c_ (B,P,C), priors (P,4); computed once per process, callers must not write into them"""
    if case_id not in _cache:
        P, C, seed = CASES[case_id]
        rng = np.random.default_rng([seed, P, C])
        l_ = np.stack([D.random_offsets(rng, P) for _ in range(B)])
        c_ = (rng.standard_normal((B, P, C)) * 3.0).astype(np.float32)
        for _ in range(100):
            near = near_cut(c_)
            if not near.any():
                break
            c_[..., :-1][near] = (rng.standard_normal(int(near.sum())) * 3.0).astype(np.float32)
        else:
            raise RuntimeError(f"{case_id}: scores left within {MARGIN} of the cut")
        pri = D.random_priors(rng, P)
        for a in (l_, c_, pri):
            a.setflags(write=False)
        _cache[case_id] = (l_, c_, pri)
    return _cache[case_id]


def distance(case_id):
    """d32: max over the candidates of |sigmoid32 - sigmoid64| / sigmoid64"""
    _, c_, _ = case(case_id)
    p64 = sigmoid64(c_)[..., :-1]
    p32 = torch.sigmoid(torch.tensor(c_[..., :-1])).numpy().astype(np.float64)
    cand = p64 >= float(np.float32(MIN_SCORE))
    return float((np.abs(p32 - p64) / p64)[cand].max())


def check(c_, min_score, outputs, bar):
    """c_ (B,P,C); outputs = (boxes, s_boxes, s_prob, s_idx, cand_cnt) filled from decode_sort_ref.poisoned_outputs.  The candidate sets
    are the f64 ones exactly; every score is within `bar` (relative) of the f64 one; two candidates of a class whose f64 scores differ
    by more than `bar` (relative) stand in the f64 order; equal device bits stand in ascending prior order; slots past the count are
    untouched.  -> largest relative score error"""
    boxes, s_boxes, s_prob, s_idx, cnt = outputs
    nb, P, C = c_.shape
    C1 = C - 1
    cut = float(np.float32(min_score))
    assert not near_cut(c_, min_score).any(), "precondition: an f64 score lies within the margin of the cut"
    p64 = sigmoid64(c_)
    worst = 0.0
    for b in range(nb):
        ref_mask = (p64[b, :, :C1] >= cut).T
        n = cnt[b, :C1].astype(np.int64)
        assert cnt[b, C1] == 0 and np.array_equal(n, ref_mask.sum(1)), f"image {b}: counts {n[:6]}, reference {ref_mask.sum(1)[:6]}"
        for c in range(C1):
            ix, pr = s_idx[b, c, :n[c]].astype(np.int64), s_prob[b, c, :n[c]]
            got = np.zeros(P, bool)
            assert ((ix >= 0) & (ix < P)).all() and np.unique(ix).size == ix.size
            got[ix] = True
            assert np.array_equal(got, ref_mask[c]), f"image {b} class {c}: the candidates are not the reference's"
            assert (s_idx[b, c, n[c]:] == D.POISON_IDX).all() and (s_prob[b, c, n[c]:] == D.POISON_PROB).all()
            if n[c] == 0:
                continue
            want = p64[b, ix, c]
            rel = np.abs(pr.astype(np.float64) - want) / want
            worst = max(worst, float(rel.max()))
            assert rel.max() <= bar, f"image {b} class {c}: a score is {rel.max():.3g} (relative) from the f64 one, bar {bar:.3g}"
            assert (np.diff(pr) <= 0).all(), f"image {b} class {c}: device scores not in descending order"
            tie = (np.diff(pr.view(np.uint32)) == 0) & (np.diff(ix) <= 0)
            assert not tie.any(), f"image {b} class {c}: equal scores not in ascending prior order"
            before = np.minimum.accumulate(want)[:-1]             # the smallest f64 score in front of each slot
            assert not (before < want[1:] * (1 - bar)).any(), f"image {b} class {c}: two scores further apart than the bar stand in the wrong order"
            same = (s_boxes[b, c, :n[c]].view(np.uint32) == boxes[b, ix].view(np.uint32)).all()
            assert same, f"image {b} class {c}: a sorted box is not the box of its prior"
    return worst


if __name__ == "__main__":
    if "--record" not in sys.argv:
        sys.exit("usage: python tests/sigmoid_decode_ref.py --record")
    d32 = {k: distance(k) for k in CASES}
    print(d32)
    with open(GOLDEN, "w") as f:
        json.dump({"d32": d32}, f, indent=2)
        f.write("\n")

"""The checker of the decode's first two stages (tests/decode_sort_ref.py) without a GPU: it accepts the reference's own output and
rejects that output with one thing wrong at a time; the inputs of the GPU tests (tests/test_decode_sort_gpu.py) meet the margins
those tests assert first."""
import numpy as np
import pytest

import decode_sort_ref as D

MIN_SCORE = 0.2


@pytest.fixture(scope="module")
def case():
    """B = 2, P = 200, C = 21: 90 priors carry one of four logit vectors (tied probabilities within and across classes), 90 carry
    N(0, 9) rows, the rest is background -> inputs, the reference's output, and in image 1 a class with a tied and an untied pair of
    neighbours"""
    rng = np.random.default_rng(5)
    B, P, C = 2, 200, 21
    ls, cs = [], []
    for b in range(B):
        l_, c_ = D.tied_rows_image(rng, P, C, n_fg=90)
        free = np.nonzero(c_[:, 0] == -8.0)[0]
        at = rng.choice(free, 90, replace=False)
        c_[at] = (rng.standard_normal((90, C)) * 3.0).astype(np.float32)
        ls.append(l_); cs.append(c_)
    l_, c_, pri = np.stack(ls), np.stack(cs), D.random_priors(rng, P)
    out = D.reference_outputs(l_, c_, pri, MIN_SCORE)
    bits = out[2][1].view(np.uint32)
    n = out[4][1]
    for c in range(C - 1):
        same = bits[c, :n[c] - 1] == bits[c, 1:n[c]]
        if n[c] >= 6 and same.any() and (~same).any():
            return (l_, c_, pri), out, (1, c, int(np.nonzero(same)[0][0]), int(np.nonzero(~same)[0][0]))
    raise AssertionError("no class with a tied and an untied pair")


def corrupted(out):
    return tuple(a.copy() for a in out)


def check(case, out, **kw):
    l_, c_, pri = case[0]
    return D.check(l_, c_, pri, MIN_SCORE, out, **kw)


def swap(out, b, c, r, arrays=(1, 2, 3)):
    for i in arrays:
        out[i][b, c, [r, r + 1]] = out[i][b, c, [r + 1, r]]


def test_the_reference_output_passes(case):
    info = check(case, case[1])
    print(info)
    assert info["compared"] == info["classes"] > 10 and info["candidates"].max() > 20
    assert info["prob_err"] < 2e-6 and info["box_err"] < 0.1            # torch's f32 softmax and numpy's f32 exp against f64
    assert info["score_margin"] >= D.SCORE_MARGIN


def test_tied_neighbours_swapped(case):
    out = corrupted(case[1])
    b, c, tied, _ = case[2]
    swap(out, b, c, tied)
    assert out[2][b, c, tied] == out[2][b, c, tied + 1] and out[3][b, c, tied] > out[3][b, c, tied + 1]
    with pytest.raises(AssertionError, match="order: image 1 .*ascending prior order"):
        check(case, out)


def test_untied_neighbours_swapped(case):
    out = corrupted(case[1])
    b, c, _, untied = case[2]
    swap(out, b, c, untied)
    with pytest.raises(AssertionError, match="order: image 1 .*descending order"):
        check(case, out)


def test_untied_neighbours_swapped_by_prior_only(case):
    """probabilities left in order, the prior ids and boxes of two neighbours exchanged: each probability now belongs to the other"""
    out = corrupted(case[1])
    b, c, _, untied = case[2]
    swap(out, b, c, untied, arrays=(1, 3))
    with pytest.raises(AssertionError, match="values: image 1|oracle: image 1"):
        check(case, out)


def test_candidate_dropped_with_the_count_decremented(case):
    out = corrupted(case[1])
    b, c, _, r = case[2]
    n = int(out[4][b, c])
    for i, poison in ((1, D.POISON_BOX), (2, D.POISON_PROB), (3, D.POISON_IDX)):
        out[i][b, c, r:n - 1] = out[i][b, c, r + 1:n]
        out[i][b, c, n - 1] = poison
    out[4][b, c] = n - 1
    with pytest.raises(AssertionError, match="set: image 1"):
        check(case, out)


def test_candidate_duplicated(case):
    out = corrupted(case[1])
    b, c, _, r = case[2]
    for i in (1, 2, 3):
        out[i][b, c, r + 1] = out[i][b, c, r]
    with pytest.raises(AssertionError, match="order: image 1 .*appears twice"):
        check(case, out)


def test_probability_off_by_3e_5(case):
    out = corrupted(case[1])
    b, c, _, r = case[2]
    n = int(out[4][b, c])
    out[2][b, c, n - 1] *= np.float32(1 - 3e-5)                          # the last: still in descending order
    with pytest.raises(AssertionError, match="values: image 1"):
        check(case, out)
    out = corrupted(case[1])
    out[2][b, c, 0] *= np.float32(1 + 3e-5)                              # the first, upwards
    with pytest.raises(AssertionError, match="values: image 1"):
        check(case, out)


def test_sorted_box_of_the_neighbouring_prior(case):
    out = corrupted(case[1])
    b, c, _, r = case[2]
    p = int(out[3][b, c, r])
    out[1][b, c, r] = out[0][b, p + 1 if p + 1 < out[0].shape[1] else p - 1]
    with pytest.raises(AssertionError, match="scatter: image 1 .*not the box of its prior"):
        check(case, out)


@pytest.mark.parametrize("which", [1, 2, 3])
def test_slot_past_the_count_overwritten(case, which):
    out = corrupted(case[1])
    b, c, _, _ = case[2]
    n = int(out[4][b, c])
    out[which][b, c, n] = out[which][b, c, n - 1]
    with pytest.raises(AssertionError, match="scatter: image 1: a .* slot past the count"):
        check(case, out)


def test_spare_counter_set(case):
    out = corrupted(case[1])
    out[4][0, -1] = 1
    with pytest.raises(AssertionError, match="scatter: image 0: the spare counter"):
        check(case, out)


def test_box_errors_are_caught(case):
    """beyond the issue's list: a centre one ulp off where the corners' rounding cannot hide it, an extent 3e-5 off, a box never
    written"""
    (l_, c_, pri), ref, _ = case
    out = corrupted(ref)
    lo, hi = out[0][0, :, 0], out[0][0, :, 2]
    sp = lambda v: np.spacing(np.abs(v))
    p = int(np.argmax(sp(lo) + sp(hi) < 2 * sp((lo + hi) / 2)))          # both corners one ulp of the centre up: the midpoint leaves the slack
    assert sp(lo[p]) + sp(hi[p]) < 2 * sp((lo[p] + hi[p]) / 2)
    step = sp((lo[p] + hi[p]) / 2)
    out[0][0, p, 0] += step; out[0][0, p, 2] += step
    with pytest.raises(AssertionError, match="boxes: centre"):
        D.check_boxes(l_[0], pri, out[0][0])
    out = corrupted(ref)
    w = out[0][0, 7, 2] - out[0][0, 7, 0]
    out[0][0, 7, 2] += np.float32(3e-5) * w * (1 + abs(out[0][0, 7, 0]) / w)                  # only the high corner: the midpoint moves too
    with pytest.raises(AssertionError, match="boxes: "):
        D.check_boxes(l_[0], pri, out[0][0])
    out = corrupted(ref)
    out[0][1, 3] = np.nan
    with pytest.raises(AssertionError, match="boxes: not every prior"):
        check(case, out)


def test_margin_precondition_is_asserted_first(case):
    (l_, c_, pri), ref, _ = case
    c2 = c_.copy()
    c2[0, 0, :] = -30.0
    c2[0, 0, 3], c2[0, 0, 20] = np.log(0.2), np.log(0.8)                 # a probability on the cut, to rounding
    with pytest.raises(AssertionError, match="precondition"):
        D.check(l_, c2, pri, MIN_SCORE, ref)


# ---- the inputs of the GPU tests -------------------------------------------------------------------------------------------------
SWEEP_C, SWEEP_SEED = D.SWEEP_C, D.SWEEP_SEED


def test_block_size_rule():
    assert [D.block_priors(C) for C in (2, 21, 46, 47, 48, 49, 94, 95, 96, 97, 256)] == [256, 256, 256, 256, 128, 128, 128, 128, 64, 64, 64]
    assert D.sweep_sizes(21) == [1, 63, 64, 65, 255, 256, 257, 513, 577] and D.sweep_sizes(48) == [1, 63, 64, 65, 127, 128, 129, 257, 321]
    assert D.sweep_sizes(256) == [1, 63, 64, 65, 129, 193]
    assert max(D.sweep_sizes(C)[-1] for C in SWEEP_C) == D.P_MAX


@pytest.mark.parametrize("C", SWEEP_C)
def test_sweep_seeds_meet_the_score_margin(C):
    """at P_MAX, so at every prefix; and the logit spread stays within 60 (normal f32 probabilities)"""
    _, c_, _ = D.sweep_case(C, SWEEP_SEED[C], D.P_MAX)
    assert D.score_margin(c_, MIN_SCORE) >= D.SCORE_MARGIN
    assert float((c_.max(-1) - c_.min(-1)).max()) < 60


def test_reference_passes_on_a_sweep_case_with_three_class_rounds():
    l_, c_, pri = D.sweep_case(66, SWEEP_SEED[66], 321)
    info = D.check(l_, c_, pri, MIN_SCORE, D.reference_outputs(l_, c_, pri, MIN_SCORE))
    assert info["compared"] > 100

"""The conditions under which tests/test_loss_regimes_gpu.py may compare the hard-negative selection of csrc/loss.hip bit for bit
with tests/class_count_ref.py, checked on the reference alone for every case of tests/loss_regimes.py, together with what each regime
claims to reach.  Every test prints the facts it asserted (pytest -s): per image the quota k, the counts of non-zero CE values and of
negatives, the k-th / (k+1)-th values, and the extent of the tie group at the boundary in ranking slices and waves.

Which case reaches which branch of the selection (from these facts, not from instrumenting the kernel):
  bin-0 fallback of the first radix pass     k > #nonzero: all_saturated, k_exceeds_nonzero, k_exceeds_negatives (every image), most
                                             images of trained / many_boxes
  a whole wave in one histogram bin          all_saturated and all_equal (every wave, every pass), one_bin (first pass: 64 consecutive
                                             priors with one non-zero top byte, asserted)
  exactly four bins in a wave                four_bins, second pass (64 consecutive priors whose second bytes take exactly four values,
                                             asserted; 48 distinct CE values in four second-byte buckets under top byte 0x40)
  nearly all values under one top byte       one_bin, four_bins, all_equal (all negatives), trained (all but ~6 % in bin 0)
  ties across slices and waves               tie_groups (a group of 52 .. 288 bit-equal values at stride 4 .. 6 over the whole image with
                                             the boundary inside, taken and left members in different waves on both sides), all_equal,
                                             and the zeros of the k > #nonzero cases; P = 777 and 1000: CH = 1, threads P .. 1023 hold
                                             empty slices; 2500: CH = 3; 4133: CH = 5 with a last slice of 3
  k >= P - n_pos, positives selected, T = 0  k_exceeds_negatives (k_raw > negatives), its clamp cases (k_raw > P, k = P), many_boxes
  more than 128 boxes in an image            many_boxes (130 and 200 boxes; ordinary and forced matches owned by boxes >= 128, asserted)
  large log-sum-exp, wrong positives         large_magnitude (CE up to ~1e4, C = 21 / 81 / 256), trained (positive CE 30 .. 100)"""
import numpy as np
import pytest
import torch

import class_count_ref as R
import loss_regimes as LR
import ssd_oracle as O


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ranked(ref, i):
    neg = ref["cce"][i].astype(np.float32)
    return np.where(~ref["pos"][i] & (neg > 0), neg, np.float32(0))


@pytest.mark.parametrize("case_id", LR.CASE_IDS)
def test_selection_conditions_hold_on_the_reference(case_id):
    case, ref = LR.case_and_reference(case_id)
    bs, P, C = case.conf.shape
    pos, hn = ref["pos"], ref["hn"]
    assert all(0 <= c <= C - 2 for cl in case.classes for c in cl)
    assert np.abs(case.conf).max() <= 1e4 and np.isfinite(case.conf).all()
    neg_ce = ref["cce"][~pos]
    assert ((neg_ce == 0) | (neg_ce >= 1e-2)).all()                          # exactly zero or far from it
    for i in range(bs):
        v = _ranked(ref, i)
        k = min(case.neg_pos_ratio * int(pos[i].sum()), P)
        assert int(hn[i].sum()) == k
        if k < P:
            order = np.argsort(-v, kind="stable")
            a, b = order[k - 1], order[k]
            if _bits(v[a]) == _bits(v[b]):
                # equal by construction, not by accident: both exactly zero, or the same row bit for bit
                assert v[a] == 0 or (not pos[i, a] and not pos[i, b] and np.array_equal(_bits(case.conf[i, a]), _bits(case.conf[i, b])))
            else:
                assert v[a] - v[b] >= 1e-4 * v[a], (v[a], v[b])
    # every selected row shows in dconf (the only way the selection is visible through ops.multibox_loss)
    assert np.array_equal((ref["dconf"].astype(np.float32) != 0).any(-1), pos | hn)
    # torch's f32 softmax on the e^-40-sized entries stays within the figure the GPU test's tolerance is built on
    m = LR.small_entries(case, ref)
    if m.any():
        s32 = torch.softmax(torch.tensor(case.conf), -1).numpy().astype(np.float64)
        s64 = torch.softmax(torch.tensor(case.conf).double(), -1).numpy()
        dev = (np.abs(s32 - s64)[m] / s64[m]).max()
        print(f"{case_id}: {int(m.sum())} small entries, f32 softmax deviation {dev:.3e}")
        assert dev <= LR.SOFTMAX_F32_DEV


@pytest.mark.parametrize("case_id", LR.CASE_IDS)
def test_each_regime_reaches_what_its_name_says(case_id):
    case, ref = LR.case_and_reference(case_id)
    regime = LR.CASES[LR.CASE_IDS.index(case_id)][1]
    clamp = "clamp" in case_id
    bs, P, C = case.conf.shape
    facts = [LR.image_facts(ref, i, case.neg_pos_ratio) for i in range(bs)]
    for i, f in enumerate(facts):
        print(f"{case_id} image {i}: k={f['k']} (ratio*n_pos={f['k_raw']}) nonzero={f['nonzero']} negatives={f['negatives']} "
              f"kth={f['kth']:.7g} next={f['next']} CH={f['CH']} tie group: {f['group_size']} values, {f['group_taken']} taken, "
              f"slices {f['group_slices']}, waves {f['group_waves']}, last taken {f['last_taken']}, first left {f['first_left']}")
    wave = lambda f, p: p // (f["CH"] * 64)
    top = lambda v: _bits(v) >> 24
    second = lambda v: (_bits(v) >> 16) & 255
    if regime == "all_saturated":
        assert all(f["nonzero"] == 0 and f["kth"] == 0 and 0 < f["k"] < f["negatives"] for f in facts)
    if regime == "k_exceeds_nonzero":
        assert all(0 < f["nonzero"] < f["k"] < f["negatives"] for f in facts)
    if regime == "trained":
        # ~94 % of the negatives at exactly zero, confidently wrong positives
        assert all(0.9 <= 1 - f["nonzero"] / f["negatives"] <= 0.97 for f in facts)
        assert (ref["cce"][ref["pos"]] >= 30).sum() >= 1
    if regime == "k_exceeds_negatives":
        if clamp:
            assert all(f["k_raw"] > P and f["k"] == P for f in facts)
        else:
            assert all(f["negatives"] < f["k_raw"] <= P for f in facts)
        assert all((ref["hn"][i] & ref["pos"][i]).any() for i in range(bs))   # the quota spills onto positives
    if regime in ("tie_groups", "all_equal"):
        for f in facts:
            assert f["kth"] > 0 and f["next"] is not None and _bits(np.float32(f["kth"])) == _bits(np.float32(f["next"]))
            assert f["group_taken"] > 0 and f["group_left"] > 0
            if regime == "all_equal":
                assert f["group_size"] == f["negatives"] == f["nonzero"]
            else:
                # taken and left members on both sides of slice and wave borders
                assert f["group_waves"][0] < wave(f, f["last_taken"]) and wave(f, f["first_left"]) < f["group_waves"][1]
                assert f["group_slices"][0] < f["last_taken"] // f["CH"] <= f["first_left"] // f["CH"] < f["group_slices"][1]
                assert 50 <= f["group_size"] < f["nonzero"]
        if regime == "tie_groups":
            for i in range(bs):                                               # 4 .. 6 distinct non-zero values, interleaved
                v = _ranked(ref, i)
                assert 4 <= np.unique(v[v > 0]).shape[0] <= 6
    if regime in ("one_bin", "four_bins"):
        for i, f in enumerate(facts):
            v = _ranked(ref, i)
            nz = v > 0
            assert f["nonzero"] == f["negatives"] and np.unique(top(v[nz])).tolist() == [0x40]
            full = [w for w in range(P // 64) if nz[64 * w:64 * w + 64].all()]
            assert full                                                       # a whole wave of the histogram loop in one first-pass bin
            if regime == "four_bins":
                assert np.unique(second(v[nz])).shape[0] == 4 and np.unique(v[nz]).shape[0] >= 40
                assert any(np.unique(second(v[64 * w:64 * w + 64])).shape[0] == 4 for w in full)
            else:
                assert np.unique(second(v[nz])).shape[0] > 64
    if regime == "large_magnitude":
        assert np.abs(case.conf).max() >= 5e3 and (case.conf > 100).any() and (case.conf < -100).any()
        assert ref["cce"][ref["pos"]].max() >= 100 and all(f["kth"] >= 100 and f["nonzero"] == f["negatives"] for f in facts)
    if regime == "many_boxes":
        counts = [len(b) for b in case.boxes]
        assert counts[:2] == [130, 200] and all(1 <= c <= 3 for c in counts[2:])
        pri_xyxy = O.xywh_to_xyxy(case.priors_cxcywh)
        start = np.concatenate([[0], np.cumsum(counts)])
        for i in (0, 1):
            b = case.boxes[i]
            assert np.array_equal(_bits(b[127]), _bits(b[128]))
            best_prior = O.iou_matrix(b, pri_xyxy).argmax(1)
            assert best_prior[127] == best_prior[128] and ref["obj"][i, best_prior[128]] - start[i] >= 128     # the last of the two wins
            forced, ordinary = LR.late_box_matches(b, case.priors_cxcywh, ref["obj"][i] - start[i], ref["pos"][i])
            print(f"{case_id} image {i}: positives owned by boxes >= 128: {forced} only through a forced match, {ordinary} ordinary")
            assert forced > 0 and ordinary > 0


@pytest.mark.parametrize("case_id", LR.CASE_IDS)
def test_reference_gradients_equal_f64_autograd(case_id):
    """dloc / dconf of the restatement against autograd through conf_ce_loss_torch in f64 with the reference's hard negatives given:
    1e-6 of the largest entry, and 1e-6 elementwise where no cancellation is involved (off the class column)."""
    case, ref = LR.case_and_reference(case_id)
    loc = torch.tensor(case.loc).double().requires_grad_(True)
    conf = torch.tensor(case.conf).double().requires_grad_(True)
    l1, l2 = R.conf_ce_loss_torch(loc, conf, case.boxes, case.classes, ref["hn"] & ~ref["pos"], case.priors_cxcywh)
    (l1 + l2).backward()
    assert abs(l1.item() - ref["loc_loss"]) <= 1e-6 * max(1.0, abs(ref["loc_loss"]))     # (the reference rounds loc - g to f32)
    assert abs(l2.item() - ref["conf_loss"]) <= 1e-9 * max(1.0, abs(ref["conf_loss"]))
    for name, got in (("dloc", loc.grad.numpy()), ("dconf", conf.grad.numpy())):
        assert np.abs(got - ref[name]).max() <= 1e-6 * np.abs(ref[name]).max(), name
    off = np.ones(case.conf.shape, bool)
    np.put_along_axis(off, ref["cls"][..., None], False, axis=2)
    got, want = conf.grad.numpy()[off], ref["dconf"][off]
    normal = np.abs(want) >= 1e-300                                            # (f64 denormals carry fewer digits)
    assert (np.abs(got - want)[normal] <= 1e-6 * np.abs(want)[normal]).all() and np.abs(got[~normal]).max(initial=0) < 1e-299

"""Seeded MultiBox-loss inputs in the regimes a trained network produces (and a few no network does), for comparing
ops.multibox_loss with tests/class_count_ref.py::multibox_loss where the hard-negative selection must agree bit for bit.

Rows of `conf` come from templates, so that every negative cross entropy (against the background column C - 1) is one of
  saturated   background logit b, every other logit in [b - 60, b - 40]: sum exp = 1 + (<= 255 e^-40) == 1.0f, CE exactly +0.0 in any
              correct f32 implementation; the softmax entries e^-40 .. e^-60 (/ n_pos) stay normal f32, so a selected row has dconf != 0
  hard        others ~ b + N(0, 3) with one column >= b + 1: CE >= log(1 + e) > 1
  duplicated  one hard row copied bit for bit to many priors: exactly tied CE
  targeted    a hard row built to a given CE value t: the mass e^t - 1 split over up to three columns
and a case is accepted only if, on the reference's f32 CE, each image's k-th and (k+1)-th largest negative values are bit-equal or
at least 1e-4 apart (relative); otherwise the logits are drawn again (next sub-seed).  The selection of such a case does not depend
on the last bits of expf / logf.

make(regime, P, C, bs, seed, priors=None, clamp=False) -> Case(loc, conf, boxes, classes, priors_cxcywh, neg_pos_ratio): plain numpy, no GPU.
Priors as tests/test_gpu_kernels.py::_loss_inputs draws them (random centres, wh in [0.03, 0.53]) unless `priors` is given."""
from collections import namedtuple

import numpy as np
import torch

import class_count_ref as R
import ssd_oracle as O

Case = namedtuple("Case", "loc conf boxes classes priors_cxcywh neg_pos_ratio")

NT = 1024            # threads of the per-image selection kernel: thread t ranks the slice [t * CH, (t + 1) * CH), CH = ceil(P / NT)
GAP_LO, GAP_HI = 40.0, 60.0


def ce_f32(conf, cls):
    """(bs, P) f32 cross entropy as the reference computes it (torch log_softmax on the CPU)."""
    bs, P, C = conf.shape
    logp = torch.log_softmax(torch.from_numpy(np.ascontiguousarray(conf, np.float32).reshape(-1, C)), dim=-1).numpy().reshape(bs, P, C)
    return -np.take_along_axis(logp, cls[..., None], axis=2)[..., 0]


# ---- geometry ------------------------------------------------------------------------------------------------------------------
def _priors(rng, P):
    cxcy = rng.random((P, 2), dtype=np.float32)
    wh = rng.random((P, 2), dtype=np.float32) * np.float32(0.5) + np.float32(0.03)
    return np.concatenate([cxcy, wh], 1)


def _boxes(rng, n, smin=0.05, srange=0.4):
    c = rng.random((n, 2), dtype=np.float32) * np.float32(0.6) + np.float32(0.2)
    s = rng.random((n, 2), dtype=np.float32) * np.float32(srange) + np.float32(smin)
    return np.concatenate([c - s / 2, c + s / 2], 1).astype(np.float32)


def _match(boxes, classes, pri, C):
    obj, cls, _, _, start = R.match_priors(boxes, classes, O.xywh_to_xyxy(pri), C)
    return obj, cls, start


# ---- row templates (background = column C - 1) ------------------------------------------------------------------------------------
def _saturated(rng, n, C, top=None):
    """n rows whose column `top` (default: the background) is GAP_LO .. GAP_HI above every other column."""
    b = rng.uniform(-4, 4, n)
    rows = b[:, None] - rng.uniform(GAP_LO, GAP_HI, (n, C))
    col = np.full(n, C - 1) if top is None else np.asarray(top)
    rows[np.arange(n), col] = b
    return rows.astype(np.float32)


def _hard(rng, n, C):
    b = rng.uniform(-4, 4, n)
    rows = b[:, None] + rng.normal(0, 3, (n, C))
    rows[np.arange(n), rng.integers(0, C - 1, n)] = b + 1 + np.abs(rng.normal(0, 3, n))
    rows[:, C - 1] = b
    return rows.astype(np.float32)


def _targeted(rng, t, C):
    """rows with CE against the background = t (to f32 rounding): e^t - 1 split over up to three columns, the rest saturated."""
    t = np.asarray(t, np.float64)
    n = t.shape[0]
    rows = _saturated(rng, n, C).astype(np.float64)
    b = rows[:, C - 1]
    live = min(3, C - 1)
    w = rng.dirichlet(np.full(live, 4.0), n)
    for r in range(n):
        cols = rng.choice(C - 1, live, replace=False)
        rows[r, cols] = b[r] + np.log(np.expm1(t[r])) + np.log(w[r])
    return rows.astype(np.float32)


def _positive_rows(rng, cls, C, wrong_share, scale=None):
    """rows for positives of class cls: `wrong_share` of them confidently wrong (true-class logit 30 .. 100 below the maximum, which
    sits on another column), the rest split between confidently right (saturated on the true class) and soft (true class 3 above
    N(0, 3) others).  scale (large_magnitude): every row wrong, multiplied by scale[i]; every second one a near miss (true class within 2 of
    the maximum after scaling), so that every positive keeps a non-zero gradient."""
    n = cls.shape[0]
    rows = np.empty((n, C), np.float64)
    kind = rng.random(n)
    wrong_col = (cls + 1 + rng.integers(0, C - 1, n)) % C
    for r in range(n):
        c = int(cls[r])
        if scale is not None or kind[r] < wrong_share:
            row = _saturated(rng, 1, C, top=[wrong_col[r]])[0].astype(np.float64)
            row[c] = row[wrong_col[r]] - rng.uniform(30, 100)
            if scale is not None:
                row *= scale[r]
                if r % 2 == 1:
                    row[c] = row[wrong_col[r]] - rng.uniform(0, 2)
        elif kind[r] < wrong_share + (1 - wrong_share) / 2:
            row = _saturated(rng, 1, C, top=[c])[0]
        else:
            row = rng.normal(0, 3, C)
            row[c] = row.max() + 3
        rows[r] = row
    return rows.astype(np.float32)


def _second_byte_targets(rng, per_bucket=12):
    """CE targets with top byte 0x40 (values in [2, 8)) and exactly four distinct second bytes; in each bucket `per_bucket` values
    in the middle 60 %, 0.05 bucket widths (~4e-4 relative) apart."""
    sbs = np.sort(rng.choice(np.arange(2, 254), 4, replace=False))
    out = []
    for sb in sbs:
        lo = np.array([(0x40 << 24) | (int(sb) << 16)], np.uint32).view(np.float32)[0]
        hi = np.array([(0x40 << 24) | ((int(sb) + 1) << 16)], np.uint32).view(np.float32)[0]
        out.append(float(lo) + (float(hi) - float(lo)) * (0.2 + 0.05 * np.arange(per_bucket)))
    return np.concatenate(out)


# ---- regimes: fill the negatives of one image -----------------------------------------------------------------------------------
def _fill_negatives(regime, rng, neg, k, C):
    """(len(neg), C) rows for the negative priors `neg` (ascending indices) of one image whose quota is k."""
    N = neg.shape[0]
    rows = _saturated(rng, N, C)
    if regime in ("trained", "many_boxes"):
        hard = rng.random(N) < 0.06
        rows[hard] = _hard(rng, int(hard.sum()), C)
    elif regime == "all_saturated":
        pass
    elif regime == "k_exceeds_nonzero":
        if not 1 < k < N:
            raise ValueError("k_exceeds_nonzero needs 1 < k < #negatives")
        at = rng.choice(N, max(1, k // 2), replace=False)
        rows[at] = _hard(rng, at.shape[0], C)
    elif regime == "k_exceeds_negatives":
        hard = rng.random(N) < 0.5
        rows[hard] = _hard(rng, int(hard.sum()), C)
    elif regime == "tie_groups":
        tg = 1 + int(rng.integers(0, 2))                       # the boundary falls into the (tg + 1)-th largest group
        m = int(k / (tg + 0.5))
        G = min(4 + int(rng.integers(0, 3)), N // m)
        if G < tg + 2 or not tg * m < k < (tg + 1) * m:
            raise ValueError(f"tie_groups: k={k} N={N} m={m} G={G}")
        at = np.floor(np.linspace(0, N - 1, G * m)).astype(np.int64)          # spread over the whole image, group g at stride G
        rows[at] = _hard(rng, G, C)[np.arange(G * m) % G]
    elif regime == "all_equal":
        rows[:] = _hard(rng, 1, C)
    elif regime == "one_bin":
        T = min(N, 400)
        tmpl = _targeted(rng, np.exp(np.linspace(np.log(2.2), np.log(7.5), T)), C)
        rows = tmpl[rng.integers(0, T, N)]
    elif regime == "four_bins":
        tmpl = _targeted(rng, _second_byte_targets(rng), C)
        which = rng.integers(0, tmpl.shape[0], N)
        which[:tmpl.shape[0]] = np.arange(tmpl.shape[0])      # every target present
        rows = tmpl[which]
    elif regime == "large_magnitude":
        s = 10.0 ** rng.uniform(0.5, 2.7, N)
        rows = np.clip(_hard(rng, N, C).astype(np.float64) * s[:, None], -1e4, 1e4).astype(np.float32)
    else:
        raise ValueError(regime)
    return rows


def _ground_truth(regime, rng, bs, P, C, pri, ratio, clamp):
    def draw(n):
        return _boxes(rng, n), rng.integers(0, C - 1, n).astype(np.float32)

    boxes, classes = [], []
    if regime == "many_boxes":
        counts = [130, 200] + [1 + int(rng.integers(0, 3)) for _ in range(bs - 2)]
        for i, n in enumerate(counts):
            b, c = draw(n)
            if n > 128:
                tiny = np.arange(133, n, 9)                     # boxes too small for any IoU >= 0.5: positives only through their forced match
                b[tiny] = _boxes(rng, tiny.shape[0], smin=0.008, srange=0.004)
                b[128] = b[127]                                 # the same box on both sides of the 128 boxes kept in LDS
                if n > 170:
                    b[170] = b[60]                              # and a pair with one box in LDS, one in memory
            boxes.append(b); classes.append(c)
        return boxes, classes
    for i in range(bs):
        if regime == "tie_groups":
            n = 12 + int(rng.integers(0, 9))
        elif regime == "k_exceeds_negatives":
            n = 8
        else:
            n = 1 + int(rng.integers(0, 3))
        b, c = draw(n)
        if regime == "k_exceeds_negatives":
            while True:                                          # more boxes until the quota passes the negatives (clamp: all priors)
                _, cls, _ = _match([b], [c], pri, C)
                n_pos = int((cls != C - 1).sum())
                if ratio * n_pos > (P if clamp else P - n_pos):
                    break
                if b.shape[0] > 400:
                    raise ValueError("k_exceeds_negatives: not reached with 400 boxes")
                b2, c2 = draw(2)
                b, c = np.concatenate([b, b2]), np.concatenate([c, c2])
        boxes.append(b); classes.append(c)
    return boxes, classes


def late_box_matches(boxes, pri, obj, pos):
    """One image (obj = local box index per prior): how many positives owned by boxes 128 .. are (forced, ordinary): positive only
    through the box's forced match (another box, or none, would have had the prior), or by the plain arg-max with IoU >= 0.5 at a
    prior that is not the box's forced one."""
    iou = O.iou_matrix(boxes, O.xywh_to_xyxy(pri))
    nat_obj, nat_ov, best_prior = iou.argmax(0), iou.max(0), iou.argmax(1)
    late = pos & (obj >= 128)
    forced = late & ((nat_obj != obj) | (nat_ov < np.float32(0.5)))
    ordinary = late & (nat_obj == obj) & (nat_ov >= np.float32(0.5)) & (best_prior[obj] != np.arange(pos.shape[0]))
    return int(forced.sum()), int(ordinary.sum())


def boundary_ok(neg_ce, k):
    """k-th and (k+1)-th largest of one image's values: bit-equal or >= 1e-4 apart, relative."""
    P = neg_ce.shape[0]
    if k <= 0 or k >= P:
        return True
    srt = np.sort(neg_ce)[::-1]
    a, b = srt[k - 1], srt[k]
    return a.view(np.uint32) == b.view(np.uint32) or (a - b) >= 1e-4 * a


def make(regime, P, C, bs, seed, priors=None, clamp=False):
    rng = np.random.default_rng([seed, P, C, bs])
    pri = _priors(rng, P) if priors is None else np.asarray(priors, np.float32)
    ratio = 3
    if regime == "k_exceeds_negatives":
        ratio = 8 if clamp else 4 + seed % 5                 # clamp: ratio * n_pos > P, the quota is cut to P
    for _ in range(20):
        boxes, classes = _ground_truth(regime, rng, bs, P, C, pri, ratio, clamp)
        obj, cls, start = _match(boxes, classes, pri, C)
        if regime != "many_boxes" or all(min(late_box_matches(boxes[i], pri, obj[i] - start[i], cls[i] != C - 1)) > 0 for i in (0, 1)):
            break
    else:
        raise RuntimeError(f"many_boxes P={P} seed={seed}: no boxes >= 128 with both a forced and an ordinary match")
    pos = cls != C - 1
    loc = rng.standard_normal((bs, P, 4), dtype=np.float32)
    for attempt in range(50):
        r2 = np.random.default_rng([seed, P, C, bs, attempt])
        conf = np.empty((bs, P, C), np.float32)
        for i in range(bs):
            neg = np.nonzero(~pos[i])[0]
            k = min(ratio * int(pos[i].sum()), P)
            conf[i, neg] = _fill_negatives(regime, r2, neg, k, C)
            pc = cls[i, pos[i]]
            if regime == "all_equal":
                conf[i, pos[i]] = conf[i, neg[0]]
            elif regime == "large_magnitude":
                conf[i, pos[i]] = np.clip(_positive_rows(r2, pc, C, 1.0, scale=10.0 ** r2.uniform(0.5, 2.0, pc.shape[0])), -1e4, 1e4)
            else:
                conf[i, pos[i]] = _positive_rows(r2, pc, C, 0.4 if regime in ("trained", "many_boxes") else 0.2)
        ce = ce_f32(conf, cls)
        ce[pos] = 0
        if all(boundary_ok(ce[i], min(ratio * int(pos[i].sum()), P)) for i in range(bs)) and not ((ce > 0) & (ce < 1e-2)).any():
            return Case(loc, conf, boxes, classes, pri, ratio)
    raise RuntimeError(f"{regime} P={P} C={C} bs={bs} seed={seed}: no draw met the conditions")


# ---- what a case reaches, from the reference alone -----------------------------------------------------------------------------------
def image_facts(ref, i, ratio):
    """Facts of image i of a case from the reference's result `ref` (class_count_ref.multibox_loss): quota, counts, the boundary
    values and the tie group at the boundary with its extent in ranking slices (CH priors) and waves (64 slices)."""
    pos, hn = ref["pos"][i], ref["hn"][i]
    P = pos.shape[0]
    neg = ref["cce"][i].astype(np.float32)
    neg = np.where(~pos & (neg > 0), neg, np.float32(0))                        # what is ranked: positives and -0.0 are +0.0
    n_pos = int(pos.sum())
    k_raw = ratio * n_pos
    k = min(k_raw, P)
    order = np.argsort(-neg, kind="stable")
    kth = neg[order[k - 1]]
    nxt = neg[order[k]] if k < P else None
    CH = -(-P // NT)
    group = np.nonzero(neg.view(np.uint32) == kth.view(np.uint32))[0]            # everything equal to the k-th value (positives are 0)
    f = dict(P=P, n_pos=n_pos, k_raw=k_raw, k=k, negatives=P - n_pos, nonzero=int((neg > 0).sum()), kth=float(kth),
             next=None if nxt is None else float(nxt), CH=CH, group_size=int(group.shape[0]),
             group_taken=int(hn[group].sum()), group_left=int((~hn[group]).sum()))
    if group.shape[0]:
        f["group_slices"] = (int(group[0] // CH), int(group[-1] // CH))
        f["group_waves"] = (int(group[0] // (CH * 64)), int(group[-1] // (CH * 64)))
        tk, lf = group[hn[group]], group[~hn[group]]
        f["last_taken"] = int(tk[-1]) if tk.shape[0] else None
        f["first_left"] = int(lf[0]) if lf.shape[0] else None
    return f


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
PS = (777, 1000, 2500, 4133)
CS = (5, 21, 64, 81, 256)


def _cases():
    out = []

    def add(regime, P, C, bs, seed, **opts):
        tag = "".join(f"-{k}" for k, v in opts.items() if v is True)
        out.append((f"{regime}{tag}-P{P}-C{C}-bs{bs}", regime, P, C, bs, seed, opts))

    # every class width of both kernel families, each with a different P
    for ri, regime in enumerate(("trained", "k_exceeds_nonzero", "tie_groups", "many_boxes")):
        for ci, C in enumerate(CS):
            bs = 3 if regime == "many_boxes" else (1, 3)[(ci + ri // 2) % 2]
            add(regime, PS[(ci + ri) % 4], C, bs, 11 * ri + ci)
    for j, P in enumerate(PS):                                   # the ranking depends on P alone: every P at C = 21 as well
        if not any(c[1] == "tie_groups" and c[2] == P and c[3] == 21 for c in out):
            add("tie_groups", P, 21, (3, 1)[j % 2], 50 + j)
    for ri, regime in enumerate(("all_saturated", "k_exceeds_negatives", "all_equal", "one_bin", "four_bins", "large_magnitude")):
        for j, P in enumerate(PS):
            add(regime, P, 21, (1, 3)[(j + ri) % 2], 100 + 10 * ri + j)
    add("k_exceeds_negatives", 777, 21, 1, 170, clamp=True)
    add("k_exceeds_negatives", 2500, 21, 3, 171, clamp=True)
    add("large_magnitude", 1000, 81, 3, 180)                    # the wide kernels' log-sum-exp at large magnitudes
    add("large_magnitude", 777, 256, 1, 181)
    add("trained", 8732, 21, 2, 190, ssd_priors=True)
    add("trained", 24564, 21, 1, 191, ssd_priors=True)
    add("trained", 8732, 81, 2, 192, ssd_priors=True)
    return out


CASES = _cases()
CASE_IDS = [c[0] for c in CASES]
_cache = {}


def case_and_reference(case_id):
    """(Case, reference result) of a named case, computed once per process and shared: callers must not write into either."""
    if case_id not in _cache:
        _, regime, P, C, bs, seed, opts = CASES[CASE_IDS.index(case_id)]
        opts = dict(opts)
        priors = None
        if opts.pop("ssd_priors", False):
            priors = O.create_priors_ssd300() if P == 8732 else O.create_priors_ssd512()
        case = make(regime, P, C, bs, seed, priors=priors, **opts)
        ref = R.multibox_loss(case.loc, case.conf, case.boxes, case.classes, case.priors_cxcywh, case.neg_pos_ratio)
        for v in list(case[:2]) + [case.priors_cxcywh] + [a for a in ref.values() if isinstance(a, np.ndarray)]:
            v.setflags(write=False)
        _cache[case_id] = (case, ref)
    return _cache[case_id]


# ---- the e^-40-sized gradient entries of selected saturated rows ---------------------------------------------------------------------
# Worst relative deviation of torch's f32 CPU softmax from the f64 softmax on these entries, over all CASES: 1.985e-6 (measured;
# tests/test_loss_regimes_cpu.py holds every case to it).  It is the rounding of x - max at |x - max| in [32, 64): half an ulp, 2^-19.
SOFTMAX_F32_DEV = 2.0e-6


def small_entries(case, ref):
    """(bs, P, C) mask: in the selected rows (positives and hard negatives) whose largest logit is >= 39 above every other, the columns
    other than that largest one and the row's class whose f64 softmax is >= 1e-30 (normal in f32 also after the division by n_pos).
    These are the entries a max-abs bar on dconf cannot see."""
    conf = case.conf
    srt = np.sort(conf, -1)
    rows = (ref["pos"] | ref["hn"]) & (srt[..., -1] - srt[..., -2] >= 39)
    m = np.broadcast_to(rows[..., None], conf.shape).copy()
    np.put_along_axis(m, conf.argmax(-1)[..., None], False, axis=2)
    np.put_along_axis(m, ref["cls"][..., None], False, axis=2)
    sm = torch.softmax(torch.tensor(conf, dtype=torch.float64), -1).numpy()
    return m & (sm >= 1e-30)

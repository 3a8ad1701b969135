// Average precision over a set of images, on the device: get_map (Util.py:783-885, the reference's 11-point AP), the detection
// evaluator (Util.DetectionEvaluator: VOC 'difficult' objects, an IoU-threshold sweep, 11- / 101- / all-point AP) and the COCO
// evaluator (Util.CocoEvaluator: crowd regions, area ranges, maxDets, AP and AR).  All three run the same four stages.
//
//   prep     per batch: tp / ignored words (and the rank) of every detection row := 0, its record class (-2 = padding row past
//            count[b], -1 = class outside [0, n_classes)), the claimed word of every object := 0; the objects that count per class
//            += (integer atomics: order-independent).  The detection side is one routine, the counting is the protocol's.
//   match    one wave per (image, class) -- matching never crosses images or classes.  That image's detections of the class are
//            visited in descending (score, lower flat index first) order, by repeated wave-max of a 64-bit key below the previous
//            one.  The usual image (at most 64 * MATCH_SLOTS rows, at most 64 objects) is staged into registers once, keys and boxes
//            in MATCH_SLOTS slots per lane and one object per lane, and the loop then touches memory only to store its flags; a
//            longer image is walked in memory.  Selection, staging and the broadcast of the selected box are shared; how a
//            detection is settled is the protocol's.
//   order    detections per class (LDS histogram), stable compaction of each class's rows with their keys (eight rows per thread),
//            rank inside the class = number of larger keys (unique keys; the class's keys stream through LDS): the per-class
//            descending order is a scatter of the tp / ignored words (and the rank).
//   ap       block per class (and threshold, and area range): scan of the TP / kept bits in sorted order by ballots and popcounts.
//
// The rules of the protocols:
//   VOC (get_map and the detection evaluator; eval_match_kernel, W = one byte / sixteen bits per row).  The best-IoU box among ALL
//            boxes of the class in the image (wave arg-max, first index on ties, Util.py:852-854; a NaN IoU among them -- torch.max
//            propagates it -- makes a false positive) does not depend on the threshold, so all thresholds are settled at once:
//            above = bits of the thresholds below the IoU; difficult box -> ignored = above; else tp = above & ~claimed[box],
//            claimed[box] |= above.  get_map is the one threshold 0.5 without difficult flags: bit 0 is its TP byte (:855-859).
//   COCO     lane a*16 + t owns the claimed set of pair (area range a, threshold t); every object lane computes its overlap with the
//            selected detection once, and the state lanes walk the class's objects: candidates are the objects unclaimed at (a, t)
//            plus every crowd object with overlap >= thr; the best non-ignored candidate, else the best ignored one, later object on
//            ties.  Two ballots give the detection's tp / ignored words (bit index = lane).  rank = position in the visiting order;
//            ranks >= max_dets[-1] only get their rank.
//   AP       the evaluators: the ignored rows removed; precision = cumTP / kept position (one division of two integers); level k of
//            L reached iff cumTP * L >= k * n_gt in 64-bit integers; or the backward envelope pass for all-point AP; COCO counts the
//            true positives with rank < m per maxDets value in the same pass.  get_map (map_ap_kernel) keeps the reference's
//            recall = float64(float32(1 / n_gt)) * cumTP in double (`numpy / long tensor` goes through Tensor.__rtruediv__ =
//            reciprocal() * other with a float32 reciprocal); max precision at recall >= each level (0 where none); the mean over
//            the levels is host side everywhere.
// IoU is the same contraction-free f32 sequence as the matcher's and the NMS's (Util.py:252-301).
#include <climits>

#include "common.h"
#pragma clang fp contract(off)

namespace {

constexpr int MAX_LEVELS = 16;
constexpr int MAX_THRESHOLDS = 16;
constexpr int MAX_EVAL_LEVELS = 100;
constexpr int MAX_AREAS = 4;
constexpr int MAX_MAXDETS = 4;
constexpr int MATCH_SLOTS = 4;
constexpr int BUCKET_ROWS = 8;
constexpr int RANK_TILE = 2048;

struct LevelArgs {
    double level[MAX_LEVELS];
};
struct ThresholdArgs {
    float thr[MAX_THRESHOLDS];
};
struct CocoArgs {
    float thr[MAX_THRESHOLDS];
    float lo[MAX_AREAS];
    float hi[MAX_AREAS];
};
struct MaxDetArgs {
    int m[MAX_MAXDETS];
};

__device__ __forceinline__ float iou_boxes(const f32x4 a, const f32x4 b) {
    const float lx = fmaxf(a[0], b[0]), ly = fmaxf(a[1], b[1]);
    const float hx = fminf(a[2], b[2]), hy = fminf(a[3], b[3]);
    const float dx = fmaxf(hx - lx, 0.f), dy = fmaxf(hy - ly, 0.f);
    const float inter = dx * dy;
    const float a1 = (a[2] - a[0]) * (a[3] - a[1]);
    const float a2 = (b[2] - b[0]) * (b[3] - b[1]);
    return inter / ((a1 + a2) - inter);
}

__device__ __forceinline__ float box_area(const f32x4 b) { return (b[2] - b[0]) * (b[3] - b[1]); }

// crowd region b: intersection over the detection's area, iou_boxes' own expressions
__device__ __forceinline__ float crowd_overlap(const f32x4 a, const f32x4 b) {
    const float lx = fmaxf(a[0], b[0]), ly = fmaxf(a[1], b[1]);
    const float hx = fminf(a[2], b[2]), hy = fminf(a[3], b[3]);
    const float dx = fmaxf(hx - lx, 0.f), dy = fmaxf(hy - ly, 0.f);
    const float inter = dx * dy;
    const float a1 = (a[2] - a[0]) * (a[3] - a[1]);
    return inter / a1;
}

__device__ __forceinline__ f32x4 load_box(const float* boxes, int i) { return *reinterpret_cast<const f32x4*>(boxes + (size_t)i * 4); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// monotone map float -> uint32 (larger float = larger integer)
__device__ __forceinline__ uint32_t ordered_bits(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// Larger key = visited earlier: the score, then the lower flat index.  Never 0, so 0 stands for "no row".
__device__ __forceinline__ uint64_t det_key(float score, int flat_index) {
    return ((uint64_t)ordered_bits(score) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)flat_index);
}
__device__ __forceinline__ int key_row(uint64_t key) { return (int)(0xFFFFFFFFu - (uint32_t)key); }
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
        const uint64_t w = ((uint64_t)hi << 32) | lo;
        v = w > v ? w : v;
    }
    return v;
}

__global__ void zero_counts_kernel(int32_t* counts, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) counts[i] = 0;
}

// ---- prep ----------------------------------------------------------------------------------------------------------------------
// The detection side, row i of D.  rec_classes, ignored and rank are optional outputs.
template <typename W>
__device__ __forceinline__ void prep_det_row(int i, const int32_t* __restrict__ det_classes, const int32_t* __restrict__ det_count,
                                             int K, int n_classes, int32_t* __restrict__ rec_classes, W* __restrict__ tp,
                                             W* __restrict__ ignored, int32_t* __restrict__ rank) {
    tp[i] = 0;
    if (ignored) ignored[i] = 0;
    if (rank) rank[i] = -1;                                                         // stays -1 outside every (image, class) list
    if (rec_classes) {
        const bool row = !det_count || (i % K) < clampi(det_count[i / K], 0, K);
        const int c = row ? det_classes[i] : -1;                                    // padding rows are never read
        rec_classes[i] = !row ? -2 : ((c >= 0 && c < n_classes) ? c : -1);
    }
}

// VOC: n_gt[c] += the objects of class c that are not difficult
template <typename W>
__global__ void eval_prep_kernel(const int32_t* __restrict__ det_classes, const int32_t* __restrict__ det_count, int K, int D,
                                 const int32_t* __restrict__ gt_classes, const uint8_t* __restrict__ gt_difficult, int G, int n_classes,
                                 int32_t* __restrict__ rec_classes, W* __restrict__ tp, W* __restrict__ ignored,
                                 W* __restrict__ claimed, int32_t* __restrict__ n_gt) {
    const int n = D > G ? D : G;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (i < G) {
            claimed[i] = 0;
            const int c = gt_classes[i];
            if (c >= 0 && c < n_classes && !(gt_difficult && gt_difficult[i])) atomicAdd(&n_gt[c], 1);
        }
        if (i < D) prep_det_row<W>(i, det_classes, det_count, K, n_classes, rec_classes, tp, ignored, nullptr);
    }
}

// COCO: n_gt[a][c] += the objects of class c that are neither crowd nor outside area range a
__global__ void coco_prep_kernel(const int32_t* __restrict__ det_classes, const int32_t* __restrict__ det_count, int K, int D,
                                 const float* __restrict__ gt_boxes, const int32_t* __restrict__ gt_classes,
                                 const uint8_t* __restrict__ gt_crowd, const float* __restrict__ gt_area, int G, int n_classes,
                                 const CocoArgs ca, int n_areas, int32_t* __restrict__ rec_classes, uint64_t* __restrict__ tp,
                                 uint64_t* __restrict__ ignored, int32_t* __restrict__ rank, uint64_t* __restrict__ claimed,
                                 int32_t* __restrict__ n_gt) {
    const int n = D > G ? D : G;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (i < G) {
            claimed[i] = 0ull;
            const int c = gt_classes[i];
            if (c >= 0 && c < n_classes && !(gt_crowd && gt_crowd[i])) {
                const float area = gt_area ? gt_area[i] : box_area(load_box(gt_boxes, i));
#pragma unroll
                for (int a = 0; a < MAX_AREAS; ++a)
                    if (a < n_areas && !(area < ca.lo[a] || area > ca.hi[a])) atomicAdd(&n_gt[a * n_classes + c], 1);
            }
        }
        if (i < D) prep_det_row<uint64_t>(i, det_classes, det_count, K, n_classes, rec_classes, tp, ignored, rank);
    }
}

// ---- match: what the protocols share -----------------------------------------------------------------------------------------------
// Rows of image b: [det_start[b], det_start[b+1]) of the concatenated layout, or [b*K, b*K + count[b]) of the padded one; its
// objects [gt_start[b], gt_start[b+1]).  Everything is clamped to the arrays.
struct ImageRows {
    int ds, de, gs, ge;
};
__device__ __forceinline__ ImageRows image_rows(int b, const int32_t* __restrict__ det_start, const int32_t* __restrict__ det_count,
                                                int K, int D, const int32_t* __restrict__ gt_start, int G) {
    ImageRows r;
    if (det_count) {
        r.ds = b * K;
        r.de = r.ds + clampi(det_count[b], 0, K);
    } else {
        r.ds = clampi(det_start[b], 0, D);
        r.de = clampi(det_start[b + 1], r.ds, D);
    }
    r.gs = clampi(gt_start[b], 0, G);
    r.ge = clampi(gt_start[b + 1], r.gs, G);
    return r;
}
// The register path: the selection loop then touches memory only to store its flags.  The dependent loads of the memory walk make
// a batch of 32 images cost as much as its longest (image, class) list times seven round trips.
__device__ __forceinline__ bool fits_registers(const ImageRows& r) { return r.de - r.ds <= 64 * MATCH_SLOTS && r.ge - r.gs <= 64; }

// Keys and boxes of the image's detections of class c, row ds + s*64 + lane in slot s (key 0: no such row).  Plain arrays, not a
// struct: as a struct the slots go to scratch memory.
__device__ __forceinline__ void stage_slots(uint64_t (&key)[MATCH_SLOTS], f32x4 (&dbox)[MATCH_SLOTS], const float* __restrict__ det_boxes,
                                            const int32_t* __restrict__ det_classes, const float* __restrict__ det_scores, int ds, int de,
                                            int c, int lane) {
#pragma unroll
    for (int s = 0; s < MATCH_SLOTS; ++s) {
        const int i = ds + s * 64 + lane;
        key[s] = 0;
        dbox[s] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (i < de && det_classes[i] == c) {
            key[s] = det_key(det_scores[i], i);
            dbox[s] = load_box(det_boxes, i);
        }
    }
}
// The largest key below prev (uniform; 0: no detection of this class left), over the slots ...
__device__ __forceinline__ uint64_t next_key(const uint64_t (&key)[MATCH_SLOTS], uint64_t prev) {
    uint64_t best = 0;
#pragma unroll
    for (int s = 0; s < MATCH_SLOTS; ++s)
        if (key[s] < prev && key[s] > best) best = key[s];
    return wave_max_u64(best);
}
// ... and over memory.
__device__ __forceinline__ uint64_t next_key(const int32_t* __restrict__ det_classes, const float* __restrict__ det_scores, int ds,
                                             int de, int c, int lane, uint64_t prev) {
    uint64_t best = 0;
    for (int i = ds + lane; i < de; i += 64) {
        if (det_classes[i] == c) {
            const uint64_t k = det_key(det_scores[i], i);
            if (k < prev && k > best) best = k;
        }
    }
    return wave_max_u64(best);
}
// The box of the selected row d on every lane, from its slot and lane.
__device__ __forceinline__ f32x4 slot_box(const f32x4 (&dbox)[MATCH_SLOTS], int d, int ds) {
    const int slot = (d - ds) >> 6, src = (d - ds) & 63;                            // uniform
    f32x4 sel = dbox[0];
#pragma unroll
    for (int s = 1; s < MATCH_SLOTS; ++s) {
        const f32x4 other = dbox[s];                    // read unconditionally: a conditional read turns into an indexed one,
        sel = slot == s ? other : sel;                  // and an indexed array leaves the registers
    }
    f32x4 box;
#pragma unroll
    for (int j = 0; j < 4; ++j) box[j] = __shfl(sel[j], src, 64);
    return box;
}

// ---- match: the VOC rule -------------------------------------------------------------------------------------------------------
// Wave arg-max of the lanes' (v_best, g_best) candidates (-1, INT_MAX: none), first index on ties.  False if any lane saw a NaN.
__device__ __forceinline__ bool best_iou(float& v_best, int& g_best, bool nan) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v_best, o, 64);
        const int og = __shfl_xor(g_best, o, 64);
        if (ov > v_best || (ov == v_best && og < g_best)) { v_best = ov; g_best = og; }
    }
    return __ballot(nan) == 0ull;
}
__device__ __forceinline__ uint32_t thresholds_below(float v, const ThresholdArgs& th, int n_thr) {
    uint32_t above = 0;
    for (int t = 0; t < n_thr; ++t) above |= (v > th.thr[t]) ? (1u << t) : 0u;
    return above;
}

// W = uint16_t: the detection evaluator.  W = uint8_t: get_map (one threshold, gt_difficult and ignored null).  The claimed words
// of an (image, class) pair are touched by its one wave only: by the lane that owns the object on the register path, by lane 0 on
// the memory path.
template <typename W>
__global__ __launch_bounds__(256) void eval_match_kernel(const float* __restrict__ det_boxes, const int32_t* __restrict__ det_classes,
                                                         const float* __restrict__ det_scores, const int32_t* __restrict__ det_start,
                                                         const int32_t* __restrict__ det_count, int K, int D,
                                                         const float* __restrict__ gt_boxes, const int32_t* __restrict__ gt_classes,
                                                         const uint8_t* __restrict__ gt_difficult, const int32_t* __restrict__ gt_start,
                                                         int G, int B, int n_classes, const ThresholdArgs th, int n_thr,
                                                         W* __restrict__ claimed, W* __restrict__ tp, W* __restrict__ ignored) {
    const int lane = threadIdx.x & 63;
    const long pair = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= (long)B * n_classes) return;                 // whole wave leaves together
    const int b = (int)(pair / n_classes), c = (int)(pair % n_classes);
    const ImageRows r = image_rows(b, det_start, det_count, K, D, gt_start, G);
    if (fits_registers(r)) {
        uint64_t key[MATCH_SLOTS];
        f32x4 dbox[MATCH_SLOTS];
        stage_slots(key, dbox, det_boxes, det_classes, det_scores, r.ds, r.de, c, lane);
        const int g_mine = r.gs + lane;
        const bool has = g_mine < r.ge && gt_classes[g_mine] == c;
        const f32x4 gbox = has ? load_box(gt_boxes, g_mine) : f32x4{0.f, 0.f, 0.f, 0.f};
        const bool difficult = has && gt_difficult && gt_difficult[g_mine];
        uint32_t claimed_mine = 0;
        for (uint64_t prev = ~0ull, sel; (sel = next_key(key, prev)) != 0; prev = sel) {
            const int d = key_row(sel);
            const f32x4 box = slot_box(dbox, d, r.ds);
            const float v = has ? iou_boxes(box, gbox) : -1.f;
            float v_best = -1.f;
            int g_best = INT_MAX;
            if (has && v > -1.f) { v_best = v; g_best = g_mine; }
            if (best_iou(v_best, g_best, has && v != v) && g_best == g_mine) {      // the lane that owns the best box settles it
                const uint32_t above = thresholds_below(v_best, th, n_thr);
                if (above) {
                    if (difficult) {
                        ignored[d] = (W)above;
                    } else {
                        tp[d] = (W)(above & ~claimed_mine);
                        claimed_mine |= above;
                    }
                }
            }
        }
        return;
    }
    for (uint64_t prev = ~0ull, sel; (sel = next_key(det_classes, det_scores, r.ds, r.de, c, lane, prev)) != 0; prev = sel) {
        const int d = key_row(sel);
        const f32x4 box = load_box(det_boxes, d);
        float v_best = -1.f;
        int g_best = INT_MAX;
        bool nan = false;
        for (int g = r.gs + lane; g < r.ge; g += 64) {
            if (gt_classes[g] == c) {
                const float v = iou_boxes(box, load_box(gt_boxes, g));
                nan |= (v != v);
                if (v > v_best) { v_best = v; g_best = g; }     // ascending g per lane: strict > keeps the first
            }
        }
        if (best_iou(v_best, g_best, nan) && lane == 0 && g_best != INT_MAX) {
            const uint32_t above = thresholds_below(v_best, th, n_thr);
            if (above) {
                if (gt_difficult && gt_difficult[g_best]) {
                    ignored[d] = (W)above;                     // neither TP nor FP; the box is never claimed
                } else {
                    const uint32_t cl = claimed[g_best];
                    tp[d] = (W)(above & ~cl);
                    claimed[g_best] = (W)(cl | above);
                }
            }
        }
    }
}

// ---- match: the COCO rule ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void coco_match_kernel(const float* __restrict__ det_boxes, const int32_t* __restrict__ det_classes,
                                                         const float* __restrict__ det_scores, const int32_t* __restrict__ det_start,
                                                         const int32_t* __restrict__ det_count, int K, int D,
                                                         const float* __restrict__ gt_boxes, const int32_t* __restrict__ gt_classes,
                                                         const uint8_t* __restrict__ gt_crowd, const float* __restrict__ gt_area,
                                                         const int32_t* __restrict__ gt_start, int G, int B, int n_classes,
                                                         const CocoArgs ca, int n_thr, int n_areas, int max_det, uint64_t* claimed,
                                                         uint64_t* __restrict__ tp, uint64_t* __restrict__ ignored,
                                                         int32_t* __restrict__ rank) {
    const int lane = threadIdx.x & 63;
    const long pair = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pair >= (long)B * n_classes) return;                 // whole wave leaves together
    const int b = (int)(pair / n_classes), c = (int)(pair % n_classes);
    const ImageRows rows = image_rows(b, det_start, det_count, K, D, gt_start, G);
    // this lane's (area range, threshold) pair; a lane without one gets a threshold nothing reaches
    const int my_a = lane >> 4, my_t = lane & 15;
    const bool state = my_a < n_areas && my_t < n_thr;
    float my_thr = __int_as_float(0x7F800000), my_lo = 0.f, my_hi = 0.f;
#pragma unroll
    for (int t = 0; t < MAX_THRESHOLDS; ++t)
        if (state && my_t == t) my_thr = ca.thr[t];
#pragma unroll
    for (int a = 0; a < MAX_AREAS; ++a)
        if (my_a == a) { my_lo = ca.lo[a]; my_hi = ca.hi[a]; }
    int r = 0;                                                 // rank of the detection being visited (uniform)
    if (fits_registers(rows)) {
        uint64_t key[MATCH_SLOTS];
        f32x4 dbox[MATCH_SLOTS];
        stage_slots(key, dbox, det_boxes, det_classes, det_scores, rows.ds, rows.de, c, lane);
        const int g_mine = rows.gs + lane;
        const bool has = g_mine < rows.ge && gt_classes[g_mine] == c;
        const f32x4 gbox = has ? load_box(gt_boxes, g_mine) : f32x4{0.f, 0.f, 0.f, 0.f};
        const bool crowd = has && gt_crowd && gt_crowd[g_mine];
        const float area = has ? (gt_area ? gt_area[g_mine] : box_area(gbox)) : 0.f;
        const uint64_t cls_mask = __ballot(has), crowd_mask = __ballot(crowd);
        uint64_t ign_mask = 0;                                 // the objects ignored in this lane's area range
#pragma unroll
        for (int a = 0; a < MAX_AREAS; ++a) {
            const uint64_t m = __ballot(has && (crowd || area < ca.lo[a] || area > ca.hi[a]));
            if (my_a == a) ign_mask = m;
        }
        uint64_t claimed_mine = 0;                             // the objects claimed at this lane's (a, t)
        for (uint64_t prev = ~0ull, sel; (sel = next_key(key, prev)) != 0; prev = sel, ++r) {
            const int d = key_row(sel);
            if (r < max_det) {
                const f32x4 box = slot_box(dbox, d, rows.ds);
                const float ov = !has ? -1.f : (crowd ? crowd_overlap(box, gbox) : iou_boxes(box, gbox));
                const float darea = box_area(box);
                float v_ni = my_thr, v_ig = my_thr;            // `>=` from the threshold up: the later object wins ties, NaN never
                int g_ni = -1, g_ig = -1;
                for (uint64_t m = cls_mask; m != 0ull; m &= m - 1ull) {             // uniform walk over the class's objects
                    const int g = __ffsll((unsigned long long)m) - 1;
                    const float o = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ov), g));
                    const uint64_t bit = 1ull << g;
                    const bool avail = (claimed_mine & bit) == 0ull || (crowd_mask & bit) != 0ull;
                    const bool ig = (ign_mask & bit) != 0ull;
                    if (avail && !ig && o >= v_ni) { v_ni = o; g_ni = g; }
                    if (avail && ig && o >= v_ig) { v_ig = o; g_ig = g; }
                }
                const int hit = g_ni >= 0 ? g_ni : g_ig;
                if (hit >= 0) claimed_mine |= 1ull << hit;
                const uint64_t tp_word = __ballot(state && g_ni >= 0);
                const uint64_t ign_word = __ballot(state && g_ni < 0 && (g_ig >= 0 || darea < my_lo || darea > my_hi));
                if (lane == 0) {
                    tp[d] = tp_word;
                    ignored[d] = ign_word;
                }
            }
            if (lane == 0) rank[d] = r;
        }
        return;
    }
    // Memory path: every state lane walks the image's objects itself; the claimed words live in the workspace, bit = lane.  A word
    // is written by lane 0 alone, completed by the fence before any lane reads it again, and read past the vector L1.
    for (uint64_t prev = ~0ull, sel; (sel = next_key(det_classes, det_scores, rows.ds, rows.de, c, lane, prev)) != 0; prev = sel, ++r) {
        const int d = key_row(sel);
        if (r < max_det) {
            const f32x4 box = load_box(det_boxes, d);
            const float darea = box_area(box);
            float v_ni = my_thr, v_ig = my_thr;
            int g_ni = -1, g_ig = -1;
            for (int g = rows.gs; g < rows.ge; ++g) {          // uniform
                if (gt_classes[g] != c) continue;
                const f32x4 gbox = load_box(gt_boxes, g);
                const bool crowd = gt_crowd && gt_crowd[g];
                const float area = gt_area ? gt_area[g] : box_area(gbox);
                const float o = crowd ? crowd_overlap(box, gbox) : iou_boxes(box, gbox);
                const uint64_t cl = __hip_atomic_load(&claimed[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const bool avail = ((cl >> lane) & 1ull) == 0ull || crowd;
                const bool ig = crowd || area < my_lo || area > my_hi;
                if (avail && !ig && o >= v_ni) { v_ni = o; g_ni = g; }
                if (avail && ig && o >= v_ig) { v_ig = o; g_ig = g; }
            }
            const int hit = g_ni >= 0 ? g_ni : g_ig;
            uint64_t pending = __ballot(state && hit >= 0);
            while (pending != 0ull) {                          // one round per distinct object hit
                const int g = __shfl(hit, __ffsll((unsigned long long)pending) - 1, 64);
                const uint64_t m = __ballot(state && hit == g);
                if (lane == 0) {
                    const uint64_t cl = __hip_atomic_load(&claimed[g], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&claimed[g], cl | m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
                pending &= ~m;
            }
            __threadfence();
            const uint64_t tp_word = __ballot(state && g_ni >= 0);
            const uint64_t ign_word = __ballot(state && g_ni < 0 && (g_ig >= 0 || darea < my_lo || darea > my_hi));
            if (lane == 0) {
                tp[d] = tp_word;
                ignored[d] = ign_word;
            }
        }
        if (lane == 0) rank[d] = r;
    }
}

// ---- order ---------------------------------------------------------------------------------------------------------------------
// Detections per class through a per-block LDS histogram: a million rows on twenty global counters serialise otherwise.
__global__ __launch_bounds__(256) void eval_count_kernel(const int32_t* __restrict__ det_classes, int D, int n_classes,
                                                         int32_t* __restrict__ counts) {
    __shared__ int hist[256];
    hist[threadIdx.x] = 0;
    __syncthreads();
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < D; i += gridDim.x * blockDim.x) {
        const int c = det_classes[i];
        if (c >= 0 && c < n_classes) atomicAdd(&hist[c], 1);
    }
    __syncthreads();
    if ((int)threadIdx.x < n_classes && hist[threadIdx.x] != 0) atomicAdd(&counts[threadIdx.x], hist[threadIdx.x]);
}

// Block per class: stable compaction of the class's rows and their keys, BUCKET_ROWS consecutive rows per thread.
__global__ __launch_bounds__(256) void eval_bucket_kernel(const int32_t* __restrict__ det_classes, const float* __restrict__ det_scores,
                                                          int D, const int32_t* __restrict__ counts, int32_t* __restrict__ list,
                                                          uint64_t* __restrict__ keys) {
    __shared__ int wave_cnt[4];
    const int c = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int off = 0;
    for (int k = 0; k < c; ++k) off += counts[k];
    int base = 0;
    for (int i0 = 0; i0 < D; i0 += 256 * BUCKET_ROWS) {
        const int first = i0 + threadIdx.x * BUCKET_ROWS;
        uint32_t mask = 0;
#pragma unroll
        for (int j = 0; j < BUCKET_ROWS; ++j)
            if (first + j < D && det_classes[first + j] == c) mask |= 1u << j;
        const int cnt = __popc(mask);
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int w = __shfl_up(incl, o, 64);
            if (lane >= o) incl += w;
        }
        if (lane == 63) wave_cnt[wv] = incl;
        __syncthreads();
        int before = 0;
        for (int k = 0; k < wv; ++k) before += wave_cnt[k];
        const int total = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        int pos = off + base + before + incl - cnt;
#pragma unroll
        for (int j = 0; j < BUCKET_ROWS; ++j) {
            if (mask & (1u << j)) {
                list[pos] = first + j;
                keys[pos] = det_key(det_scores[first + j], first + j);
                ++pos;
            }
        }
        base += total;
        __syncthreads();
    }
}

// A block owns 256 consecutive positions of the bucketed list and, for each class that reaches into them, streams that class's
// keys through an LDS tile; every thread counts the keys above its own (keys are unique: the count is its rank) and scatters its
// row's words to that position.  W = uint8_t: get_map's TP bytes (ignored null).  W = uint16_t: the evaluator's threshold masks.
// W = uint64_t with WITH_RANK: the COCO evaluator's (area range, threshold) words and the rank inside the (image, class) list.
template <typename W, bool WITH_RANK>
__global__ __launch_bounds__(256) void eval_rank_kernel(const int32_t* __restrict__ counts, int n_classes, const int32_t* __restrict__ list,
                                                        const uint64_t* __restrict__ keys, const W* __restrict__ tp,
                                                        const W* __restrict__ ignored, const int32_t* __restrict__ det_rank,
                                                        W* __restrict__ sorted_tp, W* __restrict__ sorted_ign,
                                                        int32_t* __restrict__ sorted_rank) {
    __shared__ uint64_t tile[RANK_TILE];
    const int p0 = blockIdx.x * 256, p = p0 + threadIdx.x;
    int hi = 0;
    for (int c = 0; c < n_classes; ++c) {                                           // every branch on lo / hi is block-uniform
        const int lo = hi;
        hi = lo + counts[c];
        if (hi <= p0 || hi == lo) continue;
        if (lo >= p0 + 256) break;
        const bool mine = p >= lo && p < hi;
        const uint64_t key = mine ? keys[p] : ~0ull;
        int rank = 0;
        for (int t0 = lo; t0 < hi; t0 += RANK_TILE) {
            const int m = hi - t0 < RANK_TILE ? hi - t0 : RANK_TILE;
            const int m4 = (m + 3) & ~3;
            __syncthreads();
            for (int k = threadIdx.x; k < m4; k += 256) tile[k] = k < m ? keys[t0 + k] : 0ull;
            __syncthreads();
            for (int k = 0; k < m4; k += 4) {
                rank += tile[k] > key ? 1 : 0;
                rank += tile[k + 1] > key ? 1 : 0;
                rank += tile[k + 2] > key ? 1 : 0;
                rank += tile[k + 3] > key ? 1 : 0;
            }
        }
        if (mine) {
            const int i = list[p];
            sorted_tp[lo + rank] = tp[i];
            if (ignored) sorted_ign[lo + rank] = ignored[i];
            if (WITH_RANK) sorted_rank[lo + rank] = det_rank[i];
        }
    }
}

// ---- ap ------------------------------------------------------------------------------------------------------------------------
// For each of N flags, given as this wave's ballot, over the 256 threads of the block: the set flags in the waves before this one
// and in the whole block.  Both barriers are inside: the LDS words are free again on return.
template <int N>
__device__ __forceinline__ void block_counts(int (*wave_cnt)[4], const uint64_t (&bal)[N], int (&before)[N], int (&total)[N]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int f = 0; f < N; ++f) wave_cnt[f][wv] = __popcll(bal[f]);
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < N; ++f) {
        before[f] = 0;
        for (int k = 0; k < wv; ++k) before[f] += wave_cnt[f][k];
        total[f] = wave_cnt[f][0] + wave_cnt[f][1] + wave_cnt[f][2] + wave_cnt[f][3];
    }
    __syncthreads();
}
__device__ __forceinline__ uint64_t lanes_upto(int lane) { return (lane == 63) ? ~0ull : ((1ull << (lane + 1)) - 1ull); }

// get_map's table[class][level] (the header comment's AP paragraph).
__global__ __launch_bounds__(256) void map_ap_kernel(const int32_t* __restrict__ counts, int n_classes, const uint8_t* __restrict__ sorted_tp,
                                                     const LevelArgs lv, int n_levels, double* __restrict__ table) {
    __shared__ int wave_cnt[1][4];
    __shared__ double red[4][MAX_LEVELS];
    const int c = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int off = 0;
    for (int k = 0; k < c; ++k) off += counts[k];
    const int n = counts[c], n_gt = counts[n_classes + c];
    const double rinv = (double)(1.0f / (float)n_gt);          // reciprocal() of a long tensor is float32; n_gt = 0 -> inf
    double best[MAX_LEVELS];
#pragma unroll
    for (int t = 0; t < MAX_LEVELS; ++t) best[t] = -1.0;       // -1 = no position reached the level yet
    int run_tp = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const uint64_t bal[1] = {__ballot(i < n && sorted_tp[off + i] != 0)};
        int before[1], total[1];
        block_counts<1>(wave_cnt, bal, before, total);
        if (i < n) {
            const int cum_tp = run_tp + before[0] + __popcll(bal[0] & lanes_upto(lane));
            const double prec = (double)cum_tp / (double)(i + 1);      // cumTP + cumFP == position, exactly
            const double rec = rinv * (double)cum_tp;                  // inf * 0 = NaN: compares false
#pragma unroll
            for (int t = 0; t < MAX_LEVELS; ++t)
                if (t < n_levels && rec >= lv.level[t] && prec > best[t]) best[t] = prec;
        }
        run_tp += total[0];
    }
#pragma unroll
    for (int t = 0; t < MAX_LEVELS; ++t) {
        double v = best[t];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double w = __shfl_xor(v, o, 64);
            v = w > v ? w : v;
        }
        if (lane == 0) red[wv][t] = v;
    }
    __syncthreads();
    if (threadIdx.x < n_levels) {
        double v = red[0][threadIdx.x];
        for (int k = 1; k < 4; ++k) v = red[k][threadIdx.x] > v ? red[k][threadIdx.x] : v;
        table[(size_t)c * n_levels + threadIdx.x] = v < 0.0 ? 0.0 : v;
    }
}

// The evaluators' forward pass over the n sorted rows of a class at one bit of the words: a row takes part iff live(i); it is a true
// positive iff its tp bit is set (on_tp(i) is then called), kept iff its ignored bit is clear.  For L > 0 levels:
// out_row[k] = max precision = cumTP / kept position over the positions that reach level k, 0 if none.  Only true-positive positions
// can hold a maximum: a false positive has the cumTP (so the levels) of the true positive before it and a lower precision, or
// cumTP = 0 and precision 0, the default.  -> the true positives and the kept rows of the class.
struct ScanTotals {
    int tp, kept;
};
template <typename W, typename Live, typename OnTp>
__device__ __forceinline__ ScanTotals level_scan(const W* __restrict__ sorted_tp, const W* __restrict__ sorted_ign, int n, W bit, int n_gt,
                                                 int L, int (*wave_cnt)[4], unsigned long long* lvl, double* __restrict__ out_row,
                                                 Live live, OnTp on_tp) {
    const int lane = threadIdx.x & 63;
    for (int k = threadIdx.x; k <= MAX_EVAL_LEVELS; k += 256) lvl[k] = 0ull;       // bits of +0.0
    __syncthreads();
    ScanTotals run{0, 0};
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const bool in = i < n && live(i);
        const bool is_tp = in && (sorted_tp[i] & bit) != 0;
        const bool kept = in && (sorted_ign[i] & bit) == 0;
        const uint64_t bal[2] = {__ballot(is_tp), __ballot(kept)};
        int before[2], total[2];
        block_counts<2>(wave_cnt, bal, before, total);
        if (is_tp) on_tp(i);
        if (L > 0 && is_tp && n_gt > 0) {
            const int cum_tp = run.tp + before[0] + __popcll(bal[0] & lanes_upto(lane));
            const int pos = run.kept + before[1] + __popcll(bal[1] & lanes_upto(lane));     // cumTP + cumFP, exactly
            const double prec = (double)cum_tp / (double)pos;
            long long k = (long long)cum_tp * L / n_gt;                             // highest level with cumTP * L >= k * n_gt
            if (k > L) k = L;
            atomicMax(&lvl[k], (unsigned long long)__double_as_longlong(prec));     // non-negative doubles order as integers
        }
        run.tp += total[0];
        run.kept += total[1];
    }
    if (L > 0) {
        __syncthreads();
        if (threadIdx.x <= L) {
            unsigned long long v = 0ull;
            for (int k = threadIdx.x; k <= L; ++k) v = lvl[k] > v ? lvl[k] : v;     // reaching level k reaches every lower one
            out_row[threadIdx.x] = __longlong_as_double((long long)v);
        }
    }
    return run;
}

// L > 0: out[(t * n_classes + c) * (L + 1) + k], the level table.
// L == 0: out[t * n_classes + c] = (sum over the true positives of the precision envelope) / n_gt  (0 when n_gt == 0: the host
// writes NaN there).
__global__ __launch_bounds__(256) void eval_ap_kernel(const int32_t* __restrict__ counts, const int32_t* __restrict__ n_gt_all,
                                                      int n_classes, const uint16_t* __restrict__ sorted_tp,
                                                      const uint16_t* __restrict__ sorted_ign, int L, double* __restrict__ out) {
    __shared__ int wave_cnt[2][4];
    __shared__ unsigned long long lvl[MAX_EVAL_LEVELS + 1];
    __shared__ double wave_max[4];
    __shared__ double wave_sum[4];
    const int c = blockIdx.x, t = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint16_t bit = (uint16_t)(1u << t);
    int off = 0;
    for (int k = 0; k < c; ++k) off += counts[k];
    const int n = counts[c], n_gt = n_gt_all[c];
    sorted_tp += off;
    sorted_ign += off;
    const ScanTotals run = level_scan(sorted_tp, sorted_ign, n, bit, n_gt, L, wave_cnt, lvl, out + ((size_t)t * n_classes + c) * (L + 1),
                                      [](int) { return true; }, [](int) {});
    if (L > 0) return;
    // backward: envelope = running maximum of precision from the end; sum it over the true positives
    double carry = 0.0, sum = 0.0;
    int after_tp = 0, after_kept = 0;                                              // in the chunks behind this one
    for (int i0 = ((n - 1) / 256) * 256; n > 0 && i0 >= 0; i0 -= 256) {
        const int i = i0 + threadIdx.x;
        const bool is_tp = i < n && (sorted_tp[i] & bit) != 0;
        const bool kept = i < n && (sorted_ign[i] & bit) == 0;
        const uint64_t bal[2] = {__ballot(is_tp), __ballot(kept)};
        int before[2], total[2];
        block_counts<2>(wave_cnt, bal, before, total);
        const uint64_t above = ~lanes_upto(lane);                                  // lanes after this one
        double v = 0.0;
        if (is_tp) {
            const int behind_tp = total[0] - before[0] - __popcll(bal[0]), behind_k = total[1] - before[1] - __popcll(bal[1]);
            const int cum_tp = run.tp - (after_tp + behind_tp + __popcll(bal[0] & above));
            const int pos = run.kept - (after_kept + behind_k + __popcll(bal[1] & above));
            v = (double)cum_tp / (double)pos;
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {                                          // inclusive max-scan towards lane 0
            const double w = __shfl_down(v, o, 64);
            if (lane + o < 64) v = w > v ? w : v;
        }
        if (lane == 0) wave_max[wv] = v;
        __syncthreads();
        double env = v > carry ? v : carry;
        double chunk = carry;
        for (int k = 0; k < 4; ++k) {
            if (k > wv) env = wave_max[k] > env ? wave_max[k] : env;
            chunk = wave_max[k] > chunk ? wave_max[k] : chunk;
        }
        if (is_tp) sum += env;
        carry = chunk;
        after_tp += total[0];
        after_kept += total[1];
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) wave_sum[wv] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
        out[(size_t)t * n_classes + c] = n_gt > 0 ? s / (double)n_gt : 0.0;
    }
}

// out[((t * A + a) * n_classes + c) * 101 + k], the level table over the rows with 0 <= rank < max_dets[-1];
// tp_count[((t * A + a) * M + m) * n_classes + c] = true positives with rank < max_dets[m].
__global__ __launch_bounds__(256) void coco_ap_kernel(const int32_t* __restrict__ counts, const int32_t* __restrict__ n_gt_all,
                                                      int n_classes, int n_thr, int n_areas, const uint64_t* __restrict__ sorted_tp,
                                                      const uint64_t* __restrict__ sorted_ign, const int32_t* __restrict__ sorted_rank,
                                                      const MaxDetArgs md, int n_md, int max_last, double* __restrict__ out,
                                                      int32_t* __restrict__ tp_count) {
    constexpr int L = MAX_EVAL_LEVELS;
    __shared__ int wave_cnt[2][4];
    __shared__ int wave_md[4][MAX_MAXDETS];
    __shared__ unsigned long long lvl[L + 1];
    const int c = blockIdx.x, a = blockIdx.y / n_thr, t = blockIdx.y % n_thr, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int off = 0;
    for (int k = 0; k < c; ++k) off += counts[k];
    const size_t ta = (size_t)t * n_areas + a;
    int rk = 0;                                                                    // the rank of this thread's row of the chunk
    int below[MAX_MAXDETS] = {0, 0, 0, 0};
    level_scan(sorted_tp + off, sorted_ign + off, counts[c], (uint64_t)1 << (a * 16 + t), n_gt_all[a * n_classes + c], L, wave_cnt, lvl,
               out + (ta * n_classes + c) * (L + 1),
               [&](int i) {
                   rk = sorted_rank[off + i];
                   return rk >= 0 && rk < max_last;
               },
               [&](int) {
#pragma unroll
                   for (int m = 0; m < MAX_MAXDETS; ++m) below[m] += (m < n_md && rk < md.m[m]) ? 1 : 0;
               });
#pragma unroll
    for (int m = 0; m < MAX_MAXDETS; ++m) {
        int v = below[m];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) wave_md[wv][m] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < n_md)
        tp_count[(ta * n_md + threadIdx.x) * n_classes + c] =
            wave_md[0][threadIdx.x] + wave_md[1][threadIdx.x] + wave_md[2][threadIdx.x] + wave_md[3][threadIdx.x];
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t at_least_one(int n) { return (size_t)(n > 0 ? n : 1); }

// The order stage's workspace over D rows of `word`-byte tp / ignored words.
struct OrderWs {
    uint64_t* keys;
    int32_t* list;
    void* sorted_tp;
    void* sorted_ign;
    int32_t* sorted_rank;                                      // with_rank only
    size_t bytes;
};
OrderWs carve(void* base, int D, size_t word, bool with_rank) {
    OrderWs w;
    size_t o = 0;
    char* b = static_cast<char*>(base);
    w.keys = reinterpret_cast<uint64_t*>(b + o); o += align256(at_least_one(D) * 8);
    w.list = reinterpret_cast<int32_t*>(b + o); o += align256(at_least_one(D) * 4);
    w.sorted_tp = b + o; o += align256(at_least_one(D) * word);
    w.sorted_ign = b + o; o += align256(at_least_one(D) * word);
    w.sorted_rank = reinterpret_cast<int32_t*>(b + o); o += with_rank ? align256(at_least_one(D) * 4) : 0;
    w.bytes = o;
    return w;
}
// The match stage's workspace: one claimed word per object.
size_t claimed_bytes(int G, size_t word) { return align256(at_least_one(G) * word); }

// n_thresholds ascending values in (0, 1) -> dst
bool copy_thresholds(const float* host, int n, float* dst) {
    for (int t = 0; t < n; ++t) {
        const float v = host[t];
        if (!(v > 0.f && v < 1.f) || (t > 0 && !(v > host[t - 1]))) return false;
        dst[t] = v;
    }
    return true;
}

// What the evaluators' match entries check alike, between their own null checks and their own shape checks.
int check_match_args(const float* det_boxes, const int32_t* det_classes, const float* det_scores, const int32_t* det_start,
                     const int32_t* det_count, int K, int D, const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_start,
                     int G, int B, int n_classes, int n_thresholds, const float* thresholds_host, const int32_t* n_gt) {
    if (!gt_start || !thresholds_host || !n_gt || (!det_start == !det_count)) return SSD_ERR_NULL;
    if ((D > 0 && (!det_boxes || !det_classes || !det_scores)) || (G > 0 && (!gt_boxes || !gt_classes))) return SSD_ERR_NULL;
    if (D < 0 || D > (1 << 30) || G < 0 || G > (1 << 30) || B <= 0 || n_classes <= 0 || n_classes > 256 || n_thresholds <= 0 ||
        n_thresholds > MAX_THRESHOLDS)
        return SSD_ERR_BAD_SHAPE;
    if (det_count && (K <= 0 || (long)B * K != (long)D)) return SSD_ERR_BAD_SHAPE;
    if ((long)B * n_classes >= (1L << 31)) return SSD_ERR_BAD_SHAPE;
    return SSD_OK;
}

inline unsigned stride_blocks(int n, int cap) { return (unsigned)(ssd_cdiv(n, 256) > cap ? cap : ssd_cdiv(n, 256)); }
inline unsigned pair_blocks(int B, int n_classes) { return (unsigned)(((long)B * n_classes + 3) / 4); }

// The order stage: n_det[c] = rows of class c; the rows' words (and ranks) scattered into the per-class descending order.
template <typename W, bool WITH_RANK>
int order_rows(hipStream_t st, const int32_t* classes, const float* scores, int D, int n_classes, int32_t* n_det, const W* tp,
               const W* ignored, const int32_t* rank, const OrderWs& w) {
    if (D <= 0) return SSD_OK;
    hipLaunchKernelGGL(eval_count_kernel, dim3(stride_blocks(D, 1024)), dim3(256), 0, st, classes, D, n_classes, n_det);
    SSD_CHECK_LAUNCH();
    hipLaunchKernelGGL(eval_bucket_kernel, dim3(n_classes), dim3(256), 0, st, classes, scores, D, n_det, w.list, w.keys);
    SSD_CHECK_LAUNCH();
    hipLaunchKernelGGL(HIP_KERNEL_NAME(eval_rank_kernel<W, WITH_RANK>), dim3(ssd_cdiv(D, 256)), dim3(256), 0, st, n_det, n_classes, w.list,
                       w.keys, tp, ignored, rank, static_cast<W*>(w.sorted_tp), static_cast<W*>(w.sorted_ign), w.sorted_rank);
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}

// VOC prep and match of one batch.
template <typename W>
int voc_match(hipStream_t st, const float* det_boxes, const int32_t* det_classes, const float* det_scores, const int32_t* det_start,
              const int32_t* det_count, int K, int D, const float* gt_boxes, const int32_t* gt_classes, const uint8_t* gt_difficult,
              const int32_t* gt_start, int G, int B, int n_classes, const ThresholdArgs& th, int n_thresholds, int32_t* rec_classes,
              W* tp, W* ignored, int32_t* n_gt, W* claimed) {
    if (D > 0 || G > 0) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(eval_prep_kernel<W>), dim3(stride_blocks(D > G ? D : G, 1024)), dim3(256), 0, st, det_classes,
                           det_count, K > 0 ? K : 1, D, gt_classes, gt_difficult, G, n_classes, rec_classes, tp, ignored, claimed, n_gt);
        SSD_CHECK_LAUNCH();
    }
    if (D > 0) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(eval_match_kernel<W>), dim3(pair_blocks(B, n_classes)), dim3(256), 0, st, det_boxes, det_classes,
                           det_scores, det_start, det_count, K, D, gt_boxes, gt_classes, gt_difficult, gt_start, G, B, n_classes, th,
                           n_thresholds, claimed, tp, ignored);
        SSD_CHECK_LAUNCH();
    }
    return SSD_OK;
}

}  // namespace

// get_map: the VOC stages at the one threshold 0.5 with byte words.  The workspace is the order stage's (its sorted ignored bytes
// stay unused) followed by the claimed bytes.
extern "C" size_t ssd_map_eval_workspace(int D, int G) {
    if (D < 0 || G < 0) return 0;
    return carve(nullptr, D, 1, false).bytes + claimed_bytes(G, 1);
}

extern "C" int ssd_map_eval(const float* det_boxes, const int32_t* det_classes, const float* det_scores, const int32_t* det_start,
                            int D, const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_start, int G, int B,
                            int n_classes, const double* recall_levels_host, int n_levels, uint8_t* tp, double* table,
                            int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (!det_start || !gt_start || !recall_levels_host || !table || !counts) return SSD_ERR_NULL;
    if ((D > 0 && (!det_boxes || !det_classes || !det_scores || !tp)) || (G > 0 && (!gt_boxes || !gt_classes))) return SSD_ERR_NULL;
    if (D < 0 || G < 0 || B <= 0 || n_classes <= 0 || n_classes > 256 || n_levels <= 0 || n_levels > MAX_LEVELS) return SSD_ERR_BAD_SHAPE;
    if ((long)B * n_classes >= (1L << 31)) return SSD_ERR_BAD_SHAPE;
    if (!workspace || workspace_bytes < ssd_map_eval_workspace(D, G)) return SSD_ERR_WORKSPACE;
    if (!ssd_aligned16(workspace) || (D > 0 && !ssd_aligned16(det_boxes)) || (G > 0 && !ssd_aligned16(gt_boxes))) return SSD_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const OrderWs w = carve(workspace, D, 1, false);
    uint8_t* claimed = static_cast<uint8_t*>(workspace) + w.bytes;
    LevelArgs lv{};
    for (int t = 0; t < n_levels; ++t) lv.level[t] = recall_levels_host[t];
    ThresholdArgs th{};
    th.thr[0] = 0.5f;
    hipLaunchKernelGGL(zero_counts_kernel, dim3(ssd_cdiv(2 * n_classes, 256)), dim3(256), 0, st, counts, 2 * n_classes);
    SSD_CHECK_LAUNCH();
    // counts[n_classes + c] is prep's object count; the detection classes feed the order stage as they are: it range-checks them
    int err = voc_match<uint8_t>(st, det_boxes, det_classes, det_scores, det_start, nullptr, 0, D, gt_boxes, gt_classes, nullptr, gt_start,
                                 G, B, n_classes, th, 1, nullptr, tp, nullptr, counts + n_classes, claimed);
    if (err != SSD_OK) return err;
    err = order_rows<uint8_t, false>(st, det_classes, det_scores, D, n_classes, counts, tp, nullptr, nullptr, w);
    if (err != SSD_OK) return err;
    hipLaunchKernelGGL(map_ap_kernel, dim3(n_classes), dim3(256), 0, st, counts, n_classes, static_cast<const uint8_t*>(w.sorted_tp), lv,
                       n_levels, table);
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}

extern "C" size_t ssd_eval_match_workspace(int G) {
    if (G < 0) return 0;
    return claimed_bytes(G, 2);
}

extern "C" int ssd_eval_match(const float* det_boxes, const int32_t* det_classes, const float* det_scores, const int32_t* det_start,
                              const int32_t* det_count, int K, int D, const float* gt_boxes, const int32_t* gt_classes,
                              const uint8_t* gt_difficult, const int32_t* gt_start, int G, int B, int n_classes,
                              const float* thresholds_host, int n_thresholds, int32_t* rec_classes, uint16_t* tp, uint16_t* ignored,
                              int32_t* n_gt, void* workspace, size_t workspace_bytes, void* stream) {
    if (D > 0 && (!rec_classes || !tp || !ignored)) return SSD_ERR_NULL;
    const int err = check_match_args(det_boxes, det_classes, det_scores, det_start, det_count, K, D, gt_boxes, gt_classes, gt_start, G, B,
                                     n_classes, n_thresholds, thresholds_host, n_gt);
    if (err != SSD_OK) return err;
    ThresholdArgs th{};
    if (!copy_thresholds(thresholds_host, n_thresholds, th.thr)) return SSD_ERR_BAD_SHAPE;
    if (!workspace || workspace_bytes < ssd_eval_match_workspace(G)) return SSD_ERR_WORKSPACE;
    if ((D > 0 && !ssd_aligned16(det_boxes)) || (G > 0 && !ssd_aligned16(gt_boxes))) return SSD_ERR_ALIGN;
    return voc_match<uint16_t>((hipStream_t)stream, det_boxes, det_classes, det_scores, det_start, det_count, K, D, gt_boxes, gt_classes,
                               gt_difficult, gt_start, G, B, n_classes, th, n_thresholds, rec_classes, tp, ignored, n_gt,
                               static_cast<uint16_t*>(workspace));
}

extern "C" size_t ssd_eval_ap_workspace(int D) {
    if (D < 0) return 0;
    return carve(nullptr, D, 2, false).bytes;
}

extern "C" int ssd_eval_ap(const int32_t* rec_classes, const float* det_scores, const uint16_t* tp, const uint16_t* ignored, int D,
                           const int32_t* n_gt, int n_classes, int n_thresholds, int n_levels, double* out, int32_t* n_det,
                           void* workspace, size_t workspace_bytes, void* stream) {
    if (!n_gt || !out || !n_det) return SSD_ERR_NULL;
    if (D > 0 && (!rec_classes || !det_scores || !tp || !ignored)) return SSD_ERR_NULL;
    if (D < 0 || D > (1 << 30) || n_classes <= 0 || n_classes > 256 || n_thresholds <= 0 || n_thresholds > MAX_THRESHOLDS) return SSD_ERR_BAD_SHAPE;
    if (n_levels != 0 && n_levels != 10 && n_levels != 100) return SSD_ERR_BAD_SHAPE;
    if (!workspace || workspace_bytes < ssd_eval_ap_workspace(D)) return SSD_ERR_WORKSPACE;
    if (!ssd_aligned16(workspace)) return SSD_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const OrderWs w = carve(workspace, D, 2, false);
    hipLaunchKernelGGL(zero_counts_kernel, dim3(1), dim3(256), 0, st, n_det, n_classes);
    SSD_CHECK_LAUNCH();
    const int err = order_rows<uint16_t, false>(st, rec_classes, det_scores, D, n_classes, n_det, tp, ignored, nullptr, w);
    if (err != SSD_OK) return err;
    hipLaunchKernelGGL(eval_ap_kernel, dim3(n_classes, n_thresholds), dim3(256), 0, st, n_det, n_gt, n_classes,
                       static_cast<const uint16_t*>(w.sorted_tp), static_cast<const uint16_t*>(w.sorted_ign), n_levels, out);
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}

extern "C" size_t ssd_coco_match_workspace(int G) {
    if (G < 0) return 0;
    return claimed_bytes(G, 8);
}

extern "C" int ssd_coco_match(const float* det_boxes, const int32_t* det_classes, const float* det_scores, const int32_t* det_start,
                              const int32_t* det_count, int K, int D, const float* gt_boxes, const int32_t* gt_classes,
                              const uint8_t* gt_crowd, const float* gt_area, const int32_t* gt_start, int G, int B, int n_classes,
                              const float* thresholds_host, int n_thresholds, const float* area_lo_host, const float* area_hi_host,
                              int n_areas, int max_det_last, int32_t* rec_classes, uint64_t* tp, uint64_t* ignored, int32_t* rank,
                              int32_t* n_gt, void* workspace, size_t workspace_bytes, void* stream) {
    if (!area_lo_host || !area_hi_host || (D > 0 && (!rec_classes || !tp || !ignored || !rank))) return SSD_ERR_NULL;
    const int err = check_match_args(det_boxes, det_classes, det_scores, det_start, det_count, K, D, gt_boxes, gt_classes, gt_start, G, B,
                                     n_classes, n_thresholds, thresholds_host, n_gt);
    if (err != SSD_OK) return err;
    if (n_areas <= 0 || n_areas > MAX_AREAS || max_det_last <= 0 || max_det_last > 65535) return SSD_ERR_BAD_SHAPE;
    CocoArgs ca{};
    if (!copy_thresholds(thresholds_host, n_thresholds, ca.thr)) return SSD_ERR_BAD_SHAPE;
    for (int a = 0; a < n_areas; ++a) {
        if (!(area_lo_host[a] <= area_hi_host[a])) return SSD_ERR_BAD_SHAPE;
        ca.lo[a] = area_lo_host[a];
        ca.hi[a] = area_hi_host[a];
    }
    if (!workspace || workspace_bytes < ssd_coco_match_workspace(G)) return SSD_ERR_WORKSPACE;
    if (!ssd_aligned16(workspace) || (D > 0 && !ssd_aligned16(det_boxes)) || (G > 0 && !ssd_aligned16(gt_boxes))) return SSD_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    uint64_t* claimed = static_cast<uint64_t*>(workspace);
    if (D > 0 || G > 0) {
        hipLaunchKernelGGL(coco_prep_kernel, dim3(stride_blocks(D > G ? D : G, 1024)), dim3(256), 0, st, det_classes, det_count,
                           K > 0 ? K : 1, D, gt_boxes, gt_classes, gt_crowd, gt_area, G, n_classes, ca, n_areas, rec_classes, tp, ignored,
                           rank, claimed, n_gt);
        SSD_CHECK_LAUNCH();
    }
    if (D > 0) {
        hipLaunchKernelGGL(coco_match_kernel, dim3(pair_blocks(B, n_classes)), dim3(256), 0, st, det_boxes, det_classes, det_scores,
                           det_start, det_count, K, D, gt_boxes, gt_classes, gt_crowd, gt_area, gt_start, G, B, n_classes, ca, n_thresholds,
                           n_areas, max_det_last, claimed, tp, ignored, rank);
        SSD_CHECK_LAUNCH();
    }
    return SSD_OK;
}

extern "C" size_t ssd_coco_ap_workspace(int D) {
    if (D < 0) return 0;
    return carve(nullptr, D, 8, true).bytes;
}

extern "C" int ssd_coco_ap(const int32_t* rec_classes, const float* det_scores, const uint64_t* tp, const uint64_t* ignored,
                           const int32_t* rank, int D, const int32_t* n_gt, int n_classes, int n_thresholds, int n_areas,
                           const int32_t* max_dets_host, int n_max_dets, double* out, int32_t* tp_count, int32_t* n_det,
                           void* workspace, size_t workspace_bytes, void* stream) {
    if (!n_gt || !out || !tp_count || !n_det || !max_dets_host) return SSD_ERR_NULL;
    if (D > 0 && (!rec_classes || !det_scores || !tp || !ignored || !rank)) return SSD_ERR_NULL;
    if (D < 0 || D > (1 << 30) || n_classes <= 0 || n_classes > 256 || n_thresholds <= 0 || n_thresholds > MAX_THRESHOLDS ||
        n_areas <= 0 || n_areas > MAX_AREAS || n_max_dets <= 0 || n_max_dets > MAX_MAXDETS)
        return SSD_ERR_BAD_SHAPE;
    MaxDetArgs md{};
    for (int m = 0; m < n_max_dets; ++m) {
        const int v = max_dets_host[m];
        if (v <= 0 || v > 65535 || (m > 0 && v <= max_dets_host[m - 1])) return SSD_ERR_BAD_SHAPE;
        md.m[m] = v;
    }
    if (!workspace || workspace_bytes < ssd_coco_ap_workspace(D)) return SSD_ERR_WORKSPACE;
    if (!ssd_aligned16(workspace)) return SSD_ERR_ALIGN;
    hipStream_t st = (hipStream_t)stream;
    const OrderWs w = carve(workspace, D, 8, true);
    hipLaunchKernelGGL(zero_counts_kernel, dim3(1), dim3(256), 0, st, n_det, n_classes);
    SSD_CHECK_LAUNCH();
    const int err = order_rows<uint64_t, true>(st, rec_classes, det_scores, D, n_classes, n_det, tp, ignored, rank, w);
    if (err != SSD_OK) return err;
    hipLaunchKernelGGL(coco_ap_kernel, dim3(n_classes, n_areas * n_thresholds), dim3(256), 0, st, n_det, n_gt, n_classes, n_thresholds,
                       n_areas, static_cast<const uint64_t*>(w.sorted_tp), static_cast<const uint64_t*>(w.sorted_ign), w.sorted_rank, md,
                       n_max_dets, md.m[n_max_dets - 1], out, tp_count);
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}

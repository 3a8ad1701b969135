// MultiBox matching + loss + gradients (Losses.py:119-199; Util.py:57-63,98-102,252-301).
//
// THREE launches (round 4; no host round trip, no IoU matrix in memory):
//   L1 loss_prior_kernel   wide, a wave per 64 consecutive priors of an image: IoU against the image's boxes (kept in LDS) -> the
//                          prior's best box (first index on ties) AND, per box, the wave's best prior (torch.max's order: NaN above
//                          numbers, first index on ties; Util.py:252-301, Losses.py:160-163); log-softmax CE against the background
//                          class from conf rows staged through LDS by coalesced loads (a lane reading its own 84-byte row makes every
//                          load instruction touch 42 lines)
//   L2 loss_image_kernel   one workgroup per IMAGE, what needs the whole image and little arithmetic: best prior of each box over
//                          L1's per-wave results, forced matches in GT order (last wins, Losses.py:164-167), threshold -> class, CE
//                          and L1 term of the (few) positives, then the k-th largest negative CE by radix select on the float bits
//                          (CE >= 0) over the image's values in LDS -- bins scanned by one wave, histogram atomics aggregated per
//                          wave (the top bytes of CE values are nearly all equal) --, sum of the top k, selection mask (lower index
//                          first among equal values)
//   L3 finalize_kernel     losses and d(loss)/d(loc|conf), wide; conf rows are read for the selected priors only and dconf leaves
//                          through LDS as whole lines
// One workgroup per image for ALL of it was built and measured first (two launches): 124 us against 107 for K1-K3 -- 8 732 priors x ~1 000
// instructions of IoU divisions and exponentials are VALU-bound on ONE CU (57 us) whatever the memory side does; so the arithmetic
// stays wide and only the reductions are per image.
// The FOUR-launch form of rounds 1-3 (K1 best_prior_per_gt, K2 match_ce, K3 hard_negative, then L3) stays as the in-library
// cross-check (ssd_tune_set_loss_form(0); tests/test_gpu_kernels.py compares the two forms: obj / cls / selection identical, sums
// to rounding).
// All sums are reduced in a fixed order (no float atomics): results are bitwise reproducible.
//
// Wide rows (64 < C <= 256: COCO's 81 classes, own label sets): L1 and L3 above stage whole rows of 64 / 256 priors in LDS, 64 x 256 and
// 256 x 256 floats at C = 256 -- more than a CU holds.  Their wide forms stage nothing per class:
//   L1w loss_prior_wide_kernel   the same matching; the cross entropy walks the wave's 64 rows one at a time with the lanes across the
//                                classes (four per lane, every load a whole coalesced row), max and sum of exp by butterfly (fixed order)
//   L3w finalize_wide_kernel     64 priors per block: (max, 1/sum exp, class) of the selected rows by a wave per row, then the block's
//                                64 x C dconf floats leave as ONE flat coalesced stream (consecutive threads, consecutive floats)
// L2 (one workgroup per image, radix select) does not depend on C and is shared.  C <= 64 keeps L1 / L3 as they are.
//
// Ignore regions (ssd_multibox_loss_ignore: VOC `difficult` objects, COCO crowd regions).  L1, L1w and L2 are templates on IGN; the
// IGN = false instances are the kernels above, unchanged.  With IGN, L1 / L1w stage the image's ignore boxes beside its GT boxes (the
// first SG in LDS, more from memory) and write one byte per prior: some ignore box overlaps it by >= the threshold (IoU, or
// intersection over the prior's own area).  L2, which alone knows the positives (forced matches), keeps the byte for non-positives only,
// gives those priors the mining value 0 where the positives get theirs (the reference's cce1[pos] = 0 becomes cce1[pos | ign] = 0)
// and leaves their selection bit clear: L3 / L3w, which read nothing but cls and sel, then skip them -- the same kernels for both entries.
//
// Box-overlap localisation terms (ssd_multibox_loss_box: IoU, GIoU, DIoU, CIoU on the decoded prediction).  L2, L3 and L3w are templates
// on BOX; the BOX = false instances are the kernels above, unchanged.  With BOX, L2 sums box_term()'s loss over the positives where it
// summed the four absolute differences, and L3 / L3w write box_term()'s gradient where they wrote +-1/4: one device function for the
// decode, the four losses and their gradients, so the two finalize kernels cannot drift apart.
//
// ATSS matching (ssd_multibox_loss_atss, match_mode 1).  The assignment pass of atss.hip runs in front and leaves
// one 64-bit key per prior; L1 and L1w are templates on ATSS, whose instances read the key where the others run match_wave (no IoU
// loop), answer L2's threshold test with +-inf and fill every box's slots of partv / parti with "nothing", so that L2 -- the same
// kernel -- finds no forced match whatever the workspace held.  The ATSS = false instances are the kernels above, unchanged.
//
// Class labels index conf rows: every kernel reads them through class_index(), which keeps any value (negative, >= C - 1, NaN)
// inside the row.  Labels outside 0 .. C-2 are the caller's error and give unspecified losses, but no access outside the tensors.
//
// The IoU arithmetic must equal the reference's f32 op sequence bit for bit
// (sub, max, min, mul, add, sub, IEEE divide): this file is compiled with
// -ffp-contract=off and the pragma below keeps a*b+c from being fused.
#include "common.h"
#include "atss.h"
#include <cfloat>
#pragma clang fp contract(off)

namespace {

constexpr int LB = 256;       // threads per block in K2/K4
constexpr int HB = 1024;      // threads per block in K3

__device__ __forceinline__ float iou_xyxy(float ax1, float ay1, float ax2, float ay2, float area_a, float bx1, float by1,
                                          float bx2, float by2, float area_b) {
    const float lx = fmaxf(ax1, bx1), ly = fmaxf(ay1, by1);
    const float hx = fminf(ax2, bx2), hy = fminf(ay2, by2);
    const float dx = fmaxf(hx - lx, 0.f), dy = fmaxf(hy - ly, 0.f);
    const float inter = dx * dy;
    const float uni = (area_a + area_b) - inter;          // Util.py:299: a1 + a2 - inter, left to right
    return inter / uni;                                   // no epsilon (Util.py:301)
}

// ground-truth label -> conf column, clamped into 0 .. C-1 (NaN -> 0); the identity (int)v for the valid labels 0 .. C-2
__device__ __forceinline__ int class_index(float v, int C) { return v >= 0.f ? (v < (float)(C - 1) ? (int)v : C - 1) : 0; }

// torch.max(dim) update rule: take v when it is larger, or when it is NaN and best is not.
__device__ __forceinline__ bool better(float v, float best) { return v > best || (v != v && best == best); }

__global__ __launch_bounds__(256) void best_prior_per_gt_kernel(const float* __restrict__ gt, const float* __restrict__ pri_xyxy,
                                                                int P, int32_t* __restrict__ best_prior) {
    const int k = blockIdx.x;
    const float ax1 = gt[k * 4 + 0], ay1 = gt[k * 4 + 1], ax2 = gt[k * 4 + 2], ay2 = gt[k * 4 + 3];
    const float area_a = (ax2 - ax1) * (ay2 - ay1);
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int p = threadIdx.x; p < P; p += 256) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(pri_xyxy + (size_t)p * 4);
        const float area_b = (b[2] - b[0]) * (b[3] - b[1]);
        const float v = iou_xyxy(ax1, ay1, ax2, ay2, area_a, b[0], b[1], b[2], b[3], area_b);
        if (idx == 0x7fffffff || better(v, best)) { best = v; idx = p; }
    }
    // combine: larger value wins, NaN beats numbers, equal values -> smaller index
    __shared__ float sv[256];
    __shared__ int si[256];
    sv[threadIdx.x] = best;
    si[threadIdx.x] = idx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            const float v2 = sv[threadIdx.x + o];
            const int i2 = si[threadIdx.x + o];
            const float v1 = sv[threadIdx.x];
            const int i1 = si[threadIdx.x];
            bool take;
            if (i2 == 0x7fffffff) take = false;
            else if (i1 == 0x7fffffff) take = true;
            else if (v1 != v1 || v2 != v2) take = (v2 != v2) && (v1 == v1 || i2 < i1);
            else take = v2 > v1 || (v2 == v1 && i2 < i1);
            if (take) { sv[threadIdx.x] = v2; si[threadIdx.x] = i2; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) best_prior[k] = si[0];
}

struct MatchArgs {
    const float* loc; const float* conf; const float* gt; const float* gt_cls; const int32_t* img_start;
    const int32_t* best_prior; const float* pri; const float* pri_xyxy;
    int32_t* obj; int32_t* cls; float* neg; float* part;
    int P, C, NB; float thr;
};

// encode of the matched GT against the prior (Util.py:57-63 xyxy_to_xywh then Util.py:98-102)
__device__ __forceinline__ void encode_gt(const float* __restrict__ gt, int k, const f32x4 pr, float g[4]) {
    const float x1 = gt[k * 4 + 0], y1 = gt[k * 4 + 1], x2 = gt[k * 4 + 2], y2 = gt[k * 4 + 3];
    const float cx = (x2 + x1) / 2.f, cy = (y2 + y1) / 2.f, w = x2 - x1, h = y2 - y1;
    g[0] = (cx - pr[0]) / (pr[2] / 10.f);
    g[1] = (cy - pr[1]) / (pr[3] / 10.f);
    g[2] = logf(w / pr[2]) * 5.f;
    g[3] = logf(h / pr[3]) * 5.f;
}

// Box-overlap localisation terms (ssd_multibox_loss_box, loc_mode 1 .. 4 = IoU, GIoU, DIoU, CIoU): decode of the
// predicted box (Util.gcxgcy_to_cxcy, the exponent clamped to +-log(1000 / 16)), the loss of one positive and its gradient with respect
// to the four offsets, in ONE function for the per-image kernel (which keeps the loss) and both finalize kernels (which keep the
// gradient).  `mode` is wave-uniform.  A clamped coordinate has gradient exactly +0; CIoU's alpha is a constant of the gradient.
// Where two corners are equal (a kink of min / max) the gradient is one of the two one-sided ones.
constexpr float BOX_T = 4.135166556742356f;      // log(1000 / 16)
constexpr float BOX_EPS = 1e-7f;
struct BoxTerm { float loss; float d[4]; };

__device__ __forceinline__ f32x4 load_box(const float* __restrict__ gt, int k) {
    const f32x4 g = {gt[k * 4 + 0], gt[k * 4 + 1], gt[k * 4 + 2], gt[k * 4 + 3]};
    return g;
}

__device__ __forceinline__ BoxTerm box_term(int mode, const f32x4 l, const f32x4 pr, const f32x4 g) {
    const float gx1 = g[0], gy1 = g[1], gx2 = g[2], gy2 = g[3];
    const float cx = l[0] * pr[2] / 10.f + pr[0], cy = l[1] * pr[3] / 10.f + pr[1];
    const float t2 = l[2] / 5.f, t3 = l[3] / 5.f;
    const bool free_w = t2 >= -BOX_T && t2 <= BOX_T, free_h = t3 >= -BOX_T && t3 <= BOX_T;
    const float w = expf(fminf(fmaxf(t2, -BOX_T), BOX_T)) * pr[2], h = expf(fminf(fmaxf(t3, -BOX_T), BOX_T)) * pr[3];
    const float x1 = cx - w / 2.f, y1 = cy - h / 2.f, x2 = cx + w / 2.f, y2 = cy + h / 2.f;
    const float gw = gx2 - gx1, gh = gy2 - gy1;
    const float iw = fminf(x2, gx2) - fmaxf(x1, gx1), ih = fminf(y2, gy2) - fmaxf(y1, gy1);
    const float iwc = fmaxf(iw, 0.f), ihc = fmaxf(ih, 0.f);
    const float inter = iwc * ihc;
    const float uni = w * h + gw * gh - inter;
    const float ue = uni + BOX_EPS;
    const float iou = inter / ue;
    const float cw = fmaxf(x2, gx2) - fminf(x1, gx1), ch = fmaxf(y2, gy2) - fminf(y1, gy1);
    float loss = 1.f - iou;
    // d(loss) / d(inter) with the union held, d / d(union), d / d(cw | ch), and what reaches cx, cy, w, h without passing a corner
    const float g_int = -1.f / ue;
    float g_uni = inter / (ue * ue);
    float g_cw = 0.f, g_ch = 0.f, g_cx = 0.f, g_cy = 0.f, g_w = 0.f, g_h = 0.f;
    if (mode == 2) {
        const float hull = cw * ch, he = hull + BOX_EPS;
        loss += (hull - uni) / he;
        g_uni -= 1.f / he;
        const float g_hull = ue / (he * he);
        g_cw = g_hull * ch;
        g_ch = g_hull * cw;
    } else if (mode >= 3) {
        const float dx = cx - (gx1 + gx2) / 2.f, dy = cy - (gy1 + gy2) / 2.f;
        const float rho2 = dx * dx + dy * dy, ce = cw * cw + ch * ch + BOX_EPS;
        loss += rho2 / ce;
        g_cx = 2.f * dx / ce;
        g_cy = 2.f * dy / ce;
        const float g_c2 = -rho2 / (ce * ce);
        g_cw = g_c2 * 2.f * cw;
        g_ch = g_c2 * 2.f * ch;
        if (mode == 4) {
            constexpr float K = 0.4052847345693511f;       // 4 / pi^2
            const float da = atanf(gw / gh) - atanf(w / h);
            const float v = K * da * da;
            const float alpha = v / (1.f - iou + v + BOX_EPS);
            loss += alpha * v;
            const float sv = alpha * 2.f * K * da / (w * w + h * h);      // alpha * dv/dw = -sv * h, alpha * dv/dh = sv * w
            g_w = -sv * h;
            g_h = sv * w;
        }
    }
    const float gi = g_int - g_uni;                        // the intersection also lowers the union
    const float ox = iw > 0.f ? gi * ihc : 0.f, oy = ih > 0.f ? gi * iwc : 0.f;
    const float d_x1 = (x1 > gx1 ? -ox : 0.f) + (x1 < gx1 ? -g_cw : 0.f);
    const float d_x2 = (x2 < gx2 ? ox : 0.f) + (x2 > gx2 ? g_cw : 0.f);
    const float d_y1 = (y1 > gy1 ? -oy : 0.f) + (y1 < gy1 ? -g_ch : 0.f);
    const float d_y2 = (y2 < gy2 ? oy : 0.f) + (y2 > gy2 ? g_ch : 0.f);
    BoxTerm o;
    o.loss = loss;
    o.d[0] = (d_x1 + d_x2 + g_cx) * (pr[2] / 10.f);
    o.d[1] = (d_y1 + d_y2 + g_cy) * (pr[3] / 10.f);
    o.d[2] = free_w ? ((d_x2 - d_x1) / 2.f + g_uni * h + g_w) * (w / 5.f) : 0.f;
    o.d[3] = free_h ? ((d_y2 - d_y1) / 2.f + g_uni * w + g_h) * (h / 5.f) : 0.f;
    return o;
}

__device__ __forceinline__ float block_sum_256(float v, float* sm) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

__global__ __launch_bounds__(LB) void match_ce_kernel(const MatchArgs a) {
    __shared__ float red[4];
    const int i = blockIdx.y;
    const int p = blockIdx.x * LB + threadIdx.x;
    const int s = a.img_start[i], e = a.img_start[i + 1];
    float my_pos = 0.f, my_ce = 0.f, my_l1 = 0.f;
    if (p < a.P) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(a.pri_xyxy + (size_t)p * 4);
        const float area_b = (b[2] - b[0]) * (b[3] - b[1]);
        float best = 0.f;
        int idx = s;
        for (int k = s; k < e; ++k) {
            const float ax1 = a.gt[k * 4 + 0], ay1 = a.gt[k * 4 + 1], ax2 = a.gt[k * 4 + 2], ay2 = a.gt[k * 4 + 3];
            const float area_a = (ax2 - ax1) * (ay2 - ay1);
            const float v = iou_xyxy(ax1, ay1, ax2, ay2, area_a, b[0], b[1], b[2], b[3], area_b);
            if (k == s || better(v, best)) { best = v; idx = k; }
        }
        for (int k = s; k < e; ++k)            // Losses.py:164-167: sequential writes, last GT wins
            if (a.best_prior[k] == p) { idx = k; best = 1.f; }
        const int bg = a.C - 1;
        const int c = best < a.thr ? bg : class_index(a.gt_cls[idx], a.C);
        const bool pos = c != bg;
        const size_t ip = (size_t)i * a.P + p;
        a.obj[ip] = idx;
        a.cls[ip] = c;
        // cross entropy, torch log_softmax order: (x - max) - log(sum exp(x - max))
        const float* x = a.conf + ip * a.C;
        float m = x[0];
        for (int q = 1; q < a.C; ++q) m = fmaxf(m, x[q]);
        float se = 0.f;
        for (int q = 0; q < a.C; ++q) se += expf(x[q] - m);
        const float ce = -((x[c] - m) - logf(se));
        a.neg[ip] = pos ? 0.f : ce;
        if (pos) {
            my_pos = 1.f;
            my_ce = ce;
            const f32x4 pr = *reinterpret_cast<const f32x4*>(a.pri + (size_t)p * 4);
            float g[4];
            encode_gt(a.gt, idx, pr, g);
            const f32x4 l = *reinterpret_cast<const f32x4*>(a.loc + ip * 4);
            my_l1 = (fabsf(l[0] - g[0]) + fabsf(l[1] - g[1])) + (fabsf(l[2] - g[2]) + fabsf(l[3] - g[3]));
        }
    }
    const float t_pos = block_sum_256(my_pos, red);
    const float t_ce = block_sum_256(my_ce, red);
    const float t_l1 = block_sum_256(my_l1, red);
    if (threadIdx.x == 0) {
        float* o = a.part + ((size_t)i * a.NB + blockIdx.x) * 3;
        o[0] = t_pos; o[1] = t_ce; o[2] = t_l1;
    }
}

// ---- K3 --------------------------------------------------------------------------------
__global__ __launch_bounds__(HB) void hard_negative_kernel(const float* __restrict__ neg, const float* __restrict__ part,
                                                           uint8_t* __restrict__ sel, float* __restrict__ stats, int P,
                                                           int NB, int ratio) {
    extern __shared__ __attribute__((aligned(16))) uint32_t vals[];      // P values of this image
    __shared__ int hist[256];
    __shared__ float fred[HB / 64];
    __shared__ int ired[HB / 64];
    __shared__ int s_bcast[4];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // per-image totals from K2's per-block partials (fixed order)
    if (tid == 0) {
        float npos = 0.f, ce = 0.f, l1 = 0.f;
        for (int b = 0; b < NB; ++b) {
            const float* q = part + ((size_t)i * NB + b) * 3;
            npos += q[0]; ce += q[1]; l1 += q[2];
        }
        stats[i * 4 + 0] = npos; stats[i * 4 + 1] = ce; stats[i * 4 + 2] = l1;
        s_bcast[0] = (int)npos;
    }
    for (int p = tid; p < P; p += HB) {
        const float v = neg[(size_t)i * P + p];
        vals[p] = __float_as_uint(v > 0.f ? v : 0.f);       // also maps -0.0 and NaN to +0.0
    }
    __syncthreads();
    long kk = (long)ratio * s_bcast[0];
    const int k = kk > P ? P : (int)kk;
    if (k <= 0) {
        for (int p = tid; p < P; p += HB) sel[(size_t)i * P + p] = 0;
        if (tid == 0) stats[i * 4 + 3] = 0.f;
        return;
    }
    // radix select of the k-th largest bit pattern, 8 bits per pass from the top
    uint32_t prefix = 0, mask = 0;
    int remaining = k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int b = tid; b < 256; b += HB) hist[b] = 0;
        __syncthreads();
        for (int p = tid; p < P; p += HB) {
            const uint32_t u = vals[p];
            if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int rem = remaining, d = 255;
            for (; d > 0; --d) {
                if (hist[d] >= rem) break;
                rem -= hist[d];
            }
            s_bcast[1] = d;
            s_bcast[2] = rem;
        }
        __syncthreads();
        prefix |= (uint32_t)s_bcast[1] << shift;
        mask |= 255u << shift;
        remaining = s_bcast[2];
        __syncthreads();
    }
    const uint32_t T = prefix;            // k-th largest value; take `remaining` of the elements equal to it
    // ordered pass: thread t owns the contiguous slice [t*CH, (t+1)*CH)
    const int CH = (P + HB - 1) / HB;
    const int p0 = tid * CH, p1 = min(P, p0 + CH);
    float sum_gt = 0.f;
    int n_eq = 0;
    for (int p = p0; p < p1; ++p) {
        const uint32_t u = vals[p];
        if (u > T) sum_gt += __uint_as_float(u);
        n_eq += (u == T);
    }
    // exclusive prefix of n_eq over threads (wave scan + scan of wave totals)
    int incl = n_eq;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) ired[wave] = incl;
    const float wsum = wave_sum(sum_gt);
    if (lane == 0) fred[wave] = wsum;
    __syncthreads();
    int wave_off = 0;
    for (int w = 0; w < wave; ++w) wave_off += ired[w];
    int rank = wave_off + incl - n_eq;     // number of equal elements before this thread's slice
    for (int p = p0; p < p1; ++p) {
        const uint32_t u = vals[p];
        uint8_t s = 0;
        if (u > T) s = 1;
        else if (u == T) { s = rank < remaining ? 1 : 0; ++rank; }
        sel[(size_t)i * P + p] = s;
    }
    if (tid == 0) {
        float tot = 0.f;
        for (int w = 0; w < HB / 64; ++w) tot += fred[w];
        stats[i * 4 + 3] = tot + (float)remaining * __uint_as_float(T);
    }
}


// ---- L1: one workgroup per image ----------------------------------------------------------------------------------------
// (value, index) under torch.max's order: NaN above every number, equal values -> smaller index; 0x7fffffff = nothing yet
__device__ __forceinline__ bool arg_takes(float v2, int i2, float v1, int i1) {
    if (i2 == 0x7fffffff) return false;
    if (i1 == 0x7fffffff) return true;
    if (v1 != v1 || v2 != v2) return (v2 != v2) && (v1 == v1 || i2 < i1);
    return v2 > v1 || (v2 == v1 && i2 < i1);
}

struct ImageArgs {
    const float* loc; const float* conf; const float* gt; const float* gt_cls; const int32_t* img_start;
    const float* pri; const float* pri_xyxy;
    float* partv; int32_t* parti;                     // [n_gt][NPW]: per GT box, the best prior of each 64-prior wave of L1
    float* bestv; float* cebg;                        // [bs][P]: IoU of the prior's best box (unforced); CE against the class that box gives it
    int32_t* best_prior; int32_t* obj; int32_t* cls; uint8_t* sel; float* stats;
    int P, C, ratio, NPW; float thr;
    int loc_mode;                                     // loss_image_kernel<., true>: 1 .. 4 = IoU, GIoU, DIoU, CIoU (box_term)
    const unsigned long long* akey = nullptr;         // ATSS instances of L1 / L1w: [bs][P] keys of the assignment pass (atss.hip)
};

constexpr int SG = 128;        // GT boxes of an image kept in LDS (more are read from memory: correct, slower)

// Ignore regions of the batch: boxes [ign_start[i], ign_start[i + 1]) belong to image i; ign[bs][P] is the output byte per prior.
struct IgnArgs {
    const float* boxes; const int32_t* start; uint8_t* ign;
    float thr; int mode;                              // mode 0: IoU, 1: intersection over the prior's area
};

// L1 / L1w with IGN: the first SG ignore boxes of image i into LDS (before the block's barrier)
__device__ __forceinline__ void stage_ignore(const IgnArgs& g, int i, int tid, f32x4* si_box, float* si_area) {
    const int s = g.start[i], e = g.start[i + 1];
    const int ns = e - s < SG ? e - s : SG;
    for (int t = tid; t < ns; t += 256) {
        const f32x4 g4 = *reinterpret_cast<const f32x4*>(g.boxes + (size_t)(s + t) * 4);
        si_box[t] = g4;
        si_area[t] = (g4[2] - g4[0]) * (g4[3] - g4[1]);
    }
}

// does some ignore box of image i overlap prior b by >= thr?  The IoU is iou_xyxy's op sequence with the ignore box in the GT box's
// place; mode 1 divides the same intersection by the prior's own (unclipped) area.  A NaN overlap compares false.
__device__ __forceinline__ bool ignore_hit(const IgnArgs& g, const f32x4* si_box, const float* si_area, int i, const f32x4 b) {
    const int s = g.start[i], e = g.start[i + 1];
    const float area_b = (b[2] - b[0]) * (b[3] - b[1]);
    bool hit = false;
    for (int k = s; k < e; ++k) {
        f32x4 g4;
        float area_a;
        if (k - s < SG) {
            g4 = si_box[k - s];
            area_a = si_area[k - s];
        } else {
            g4 = *reinterpret_cast<const f32x4*>(g.boxes + (size_t)k * 4);
            area_a = (g4[2] - g4[0]) * (g4[3] - g4[1]);
        }
        const float lx = fmaxf(g4[0], b[0]), ly = fmaxf(g4[1], b[1]);
        const float hx = fminf(g4[2], b[2]), hy = fminf(g4[3], b[3]);
        const float dx = fmaxf(hx - lx, 0.f), dy = fmaxf(hy - ly, 0.f);
        const float inter = dx * dy;
        const float v = g.mode == 0 ? inter / ((area_a + area_b) - inter) : inter / area_b;
        hit = hit || v >= g.thr;
    }
    return hit;
}

// L1 / L1w: IoU of prior p (lane of a wave owning 64 consecutive priors) against the image's boxes [s, e) -> the prior's best box
// (first index on ties) in (best, idx); and, per box, the wave's best prior into partv / parti[k][slot]
__device__ __forceinline__ void match_wave(const ImageArgs& a, const f32x4* sg_box, const float* sg_area, int s, int e, int p, bool live,
                                           int lane, int slot, float& best, int& idx) {
    f32x4 b = {0.f, 0.f, 0.f, 0.f};
    if (live) b = *reinterpret_cast<const f32x4*>(a.pri_xyxy + (size_t)p * 4);
    const float area_b = (b[2] - b[0]) * (b[3] - b[1]);
    best = 0.f;
    idx = s;
    for (int k = s; k < e; ++k) {
        float v;
        if (k - s < SG) {
            const f32x4 g4 = sg_box[k - s];
            v = iou_xyxy(g4[0], g4[1], g4[2], g4[3], sg_area[k - s], b[0], b[1], b[2], b[3], area_b);
        } else {
            const float ax1 = a.gt[k * 4 + 0], ay1 = a.gt[k * 4 + 1], ax2 = a.gt[k * 4 + 2], ay2 = a.gt[k * 4 + 3];
            v = iou_xyxy(ax1, ay1, ax2, ay2, (ax2 - ax1) * (ay2 - ay1), b[0], b[1], b[2], b[3], area_b);
        }
        if (k == s || better(v, best)) { best = v; idx = k; }
        // this wave's best prior for box k (first index on ties, NaN above numbers: torch.max's rule)
        float wvv = v;
        int wii = live ? p : 0x7fffffff;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(wvv, o, 64);
            const int i2 = __shfl_xor(wii, o, 64);
            if (arg_takes(v2, i2, wvv, wii)) { wvv = v2; wii = i2; }
        }
        if (lane == 0) {
            a.partv[(size_t)k * a.NPW + slot] = wvv;
            a.parti[(size_t)k * a.NPW + slot] = wii;
        }
    }
}

// L1 / L1w with ATSS (ssd_multibox_loss_atss, match_mode 1): the prior's box is the one the assignment pass gave it (atss.hip: the low
// word of its key is 0xFFFFFFFF - box), no IoU is computed.  (best, idx) are what L2 reads: +inf with the box, or -inf, against the
// threshold 0.5 the host puts in place of the caller's.  There are no forced matches, and L2 finds them in partv / parti of a workspace
// that may hold anything: this wave writes "nothing" (0x7fffffff) for every box of the image into its slot.
__device__ __forceinline__ void match_assigned(const ImageArgs& a, int i, int s, int e, int p, bool live, int lane, int slot, float& best,
                                               int& idx) {
    for (int k = s + lane; k < e; k += 64) {
        a.partv[(size_t)k * a.NPW + slot] = 0.f;
        a.parti[(size_t)k * a.NPW + slot] = 0x7fffffff;
    }
    const unsigned long long key = live ? a.akey[(size_t)i * a.P + p] : 0ull;
    idx = key != 0ull ? (int)(0xFFFFFFFFu - (uint32_t)key) : s;
    best = key != 0ull ? INFINITY : -INFINITY;
}

// A conf row of C <= 256 floats across one wave: lane l holds columns l, l + 64, l + 128, l + 192 (-inf past the end).  Returns the
// row's max and sum of exp(x - max) (butterflies: the same value in every lane, the same bits on every run).
struct RowStats { float m, se; };
__device__ __forceinline__ void load_row_wave(const float* __restrict__ x, int C, int lane, float v[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = lane + 64 * j;
        v[j] = q < C ? x[q] : -INFINITY;
    }
}
__device__ __forceinline__ RowStats row_stats_wave(const float v[4], int C, int lane) {
    float m = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float e4 = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (lane + 64 * j < C) e4 += expf(v[j] - m);
    return RowStats{m, wave_sum(e4)};
}
__device__ __forceinline__ float col_wave(const float v[4], int c) {         // column c (wave-uniform) of the row, in every lane
    const int j = c >> 6;
    const float vj = j == 0 ? v[0] : (j == 1 ? v[1] : (j == 2 ? v[2] : v[3]));
    return __shfl(vj, c & 63, 64);
}

// L1: grid (ceil(P / 256), bs), 256 threads; a wave owns 64 consecutive priors of image blockIdx.y
// ATSS: match_assigned in match_wave's place (no box is staged); false is the kernel as it was.
template <bool IGN, bool ATSS = false>
__global__ __launch_bounds__(256) void loss_prior_kernel(const ImageArgs a, const IgnArgs g) {
    extern __shared__ __attribute__((aligned(16))) float stage_all[];       // [4][64 * C] conf rows
    __shared__ f32x4 sg_box[ATSS ? 1 : SG];
    __shared__ float sg_area[ATSS ? 1 : SG];
    __shared__ int sg_cls[SG];
    __shared__ f32x4 si_box[IGN ? SG : 1];
    __shared__ float si_area[IGN ? SG : 1];
    const int i = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = a.img_start[i], e = a.img_start[i + 1];
    const int P = a.P, C = a.C;
    const int ns = e - s < SG ? e - s : SG;
    for (int t = tid; t < ns; t += 256) {
        if constexpr (!ATSS) {
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(a.gt + (size_t)(s + t) * 4);
            sg_box[t] = g4;
            sg_area[t] = (g4[2] - g4[0]) * (g4[3] - g4[1]);
        }
        sg_cls[t] = class_index(a.gt_cls[s + t], C);
    }
    if (IGN) stage_ignore(g, i, tid, si_box, si_area);
    const int pb = blockIdx.x * 256 + wave * 64;          // this wave's first prior
    const int rows = P - pb < 64 ? P - pb : 64;           // (<= 0: a wave past the end; it still reports "nothing" for every box)
    float* const st = stage_all + (size_t)wave * 64 * C;
    if (rows > 0) {
        const int nfl = rows * C;
        const float* src = a.conf + ((size_t)i * P + pb) * C;
        for (int t = lane; t < nfl; t += 64) st[t] = src[t];
    }
    __syncthreads();                                      // boxes staged (and this wave's rows written)
    const int p = pb + lane;
    const bool live = lane < rows;
    float best;
    int idx;
    if constexpr (ATSS) match_assigned(a, i, s, e, p, live, lane, blockIdx.x * 4 + wave, best, idx);
    else match_wave(a, sg_box, sg_area, s, e, p, live, lane, blockIdx.x * 4 + wave, best, idx);
    if (live) {
        const size_t ip = (size_t)i * P + p;
        // cross entropy against the class the prior has unless a box claims it in L2 (Losses.py:164-167: those few are redone there);
        // torch log_softmax order: (x - max) - log(sum exp(x - max))
        const int c = best < a.thr ? C - 1 : (idx - s < SG ? sg_cls[idx - s] : class_index(a.gt_cls[idx], C));
        const float* x = st + lane * C;
        float m = x[0];
        for (int q = 1; q < C; ++q) m = fmaxf(m, x[q]);
        float se = 0.f;
        for (int q = 0; q < C; ++q) se += expf(x[q] - m);
        a.cebg[ip] = -((x[c] - m) - logf(se));
        a.bestv[ip] = best;
        a.obj[ip] = idx;
        if (IGN) g.ign[ip] = ignore_hit(g, si_box, si_area, i, *reinterpret_cast<const f32x4*>(a.pri_xyxy + (size_t)p * 4)) ? 1 : 0;
    }
}

// L1w (64 < C <= 256): L1 without the row staging; grid (ceil(P / 256), bs), 256 threads, a wave per 64 consecutive priors.
// FOCAL (conf_mode 1, any C): the matching alone -- no conf row is read, cebg is not written; false is the kernel as it was.
// ATSS: as in L1.
template <bool IGN, bool FOCAL = false, bool ATSS = false>
__global__ __launch_bounds__(256) void loss_prior_wide_kernel(const ImageArgs a, const IgnArgs g) {
    __shared__ f32x4 sg_box[ATSS ? 1 : SG];
    __shared__ float sg_area[ATSS ? 1 : SG];
    __shared__ int sg_cls[SG];
    __shared__ f32x4 si_box[IGN ? SG : 1];
    __shared__ float si_area[IGN ? SG : 1];
    const int i = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = a.img_start[i], e = a.img_start[i + 1];
    const int P = a.P, C = a.C;
    const int ns = e - s < SG ? e - s : SG;
    for (int t = tid; t < ns; t += 256) {
        if constexpr (!ATSS) {
            const f32x4 g4 = *reinterpret_cast<const f32x4*>(a.gt + (size_t)(s + t) * 4);
            sg_box[t] = g4;
            sg_area[t] = (g4[2] - g4[0]) * (g4[3] - g4[1]);
        }
        sg_cls[t] = class_index(a.gt_cls[s + t], C);
    }
    if (IGN) stage_ignore(g, i, tid, si_box, si_area);
    __syncthreads();
    const int pb = blockIdx.x * 256 + wave * 64;
    const int rows = P - pb < 64 ? P - pb : 64;
    const int p = pb + lane;
    const bool live = lane < rows;
    float best;
    int idx;
    if constexpr (ATSS) match_assigned(a, i, s, e, p, live, lane, blockIdx.x * 4 + wave, best, idx);
    else match_wave(a, sg_box, sg_area, s, e, p, live, lane, blockIdx.x * 4 + wave, best, idx);
    const int c = !live || best < a.thr ? C - 1 : (idx - s < SG ? sg_cls[idx - s] : class_index(a.gt_cls[idx], C));
    // cross entropy (torch log_softmax order: (x - max) - log(sum exp(x - max))), a row at a time, two rows' loads in flight
    float ce = 0.f;
    const float* src = a.conf + ((size_t)i * P + pb) * C;
    for (int r = 0; !FOCAL && r < rows; r += 2) {         // (rows <= 0: a wave past the end does nothing here)
        float v0[4], v1[4];
        load_row_wave(src + (size_t)r * C, C, lane, v0);
        const bool two = r + 1 < rows;
        if (two) load_row_wave(src + (size_t)(r + 1) * C, C, lane, v1);
        {
            const RowStats st = row_stats_wave(v0, C, lane);
            const float xc = col_wave(v0, __shfl(c, r, 64));
            const float cr = -((xc - st.m) - logf(st.se));
            if (lane == r) ce = cr;
        }
        if (two) {
            const RowStats st = row_stats_wave(v1, C, lane);
            const float xc = col_wave(v1, __shfl(c, r + 1, 64));
            const float cr = -((xc - st.m) - logf(st.se));
            if (lane == r + 1) ce = cr;
        }
    }
    if (live) {
        const size_t ip = (size_t)i * P + p;
        if (!FOCAL) a.cebg[ip] = ce;
        a.bestv[ip] = best;
        a.obj[ip] = idx;
        if (IGN) g.ign[ip] = ignore_hit(g, si_box, si_area, i, *reinterpret_cast<const f32x4*>(a.pri_xyxy + (size_t)p * 4)) ? 1 : 0;
    }
}

// L2: one workgroup of 1024 threads per image.  IGN: the bytes L1 wrote stay set for non-positives only; those get the mining value 0
// like the positives and never a selection bit (one bit per prior in LDS behind vals carries that to the last pass).
// BOX: the localisation term of a positive is box_term's (stats[2] = the sum of the per-positive losses); false is the L1 kernel, unchanged.
// FOCAL (conf_mode 1): forced matches, classes, the ignore bytes, n_pos and the loc term as ever, then it returns: no cross entropy,
// nothing in LDS per prior, no radix select (stats[1] = stats[3] = 0, sel is left unwritten and unread).
template <bool IGN, bool BOX, bool FOCAL = false>
__global__ __launch_bounds__(1024) void loss_image_kernel(const ImageArgs a, const IgnArgs g) {
    constexpr int NW = 16, NT = 1024;
    extern __shared__ __attribute__((aligned(16))) uint32_t vals[];            // [P] negative CE bits of this image (IGN: + [ceil(P / 32)] ignored bits)
    __shared__ float fred[3][NW];
    __shared__ int ired[NW];
    __shared__ int hist[256];
    __shared__ int s_bcast[4];
    __shared__ int sg_cls[SG], sg_bp[SG];
    __shared__ f32x4 sg_box[SG];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = a.img_start[i], e = a.img_start[i + 1];
    const int P = a.P, C = a.C;
    const int ns = e - s < SG ? e - s : SG;
    for (int t = tid; t < ns; t += NT) {
        sg_cls[t] = class_index(a.gt_cls[s + t], C);
        sg_box[t] = *reinterpret_cast<const f32x4*>(a.gt + (size_t)(s + t) * 4);
    }
    uint32_t* const ibits = vals + P;
    if (IGN && !FOCAL)
        for (int t = tid; t < (P + 31) / 32; t += NT) ibits[t] = 0u;           // (the barrier below orders this before the atomicOr's)
    // ---- best prior of each box: a wave per box over the NPW per-wave results of L1 ----
    for (int k = s + wave; k < e; k += NW) {
        float v = 0.f;
        int ix = 0x7fffffff;
        for (int t = lane; t < a.NPW; t += 64) {
            const float v2 = a.partv[(size_t)k * a.NPW + t];
            const int i2 = a.parti[(size_t)k * a.NPW + t];
            if (arg_takes(v2, i2, v, ix)) { v = v2; ix = i2; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(v, o, 64);
            const int i2 = __shfl_xor(ix, o, 64);
            if (arg_takes(v2, i2, v, ix)) { v = v2; ix = i2; }
        }
        if (lane == 0) {
            if (k - s < SG) sg_bp[k - s] = ix;
            a.best_prior[k] = ix;
        }
    }
    __syncthreads();

    // ---- per prior: forced matches, class, L1 term of the positives.  UP priors per thread in flight: everything a prior may need is
    // requested up front (measured with in-kernel clock stamps: a wave's nine priors in a row, each waiting for its own loads and the positives re-reading their conf row, were 50-70 us per image; this form 12-24) ----
    float my_pos = 0.f, my_ce = 0.f, my_l1 = 0.f;
    const int bg = C - 1;
    constexpr int UP = 3;
    for (int p0 = tid; p0 < P; p0 += UP * NT) {
        float bv[UP], cev[UP];
        int ob[UP];
        uint8_t ig[UP];
        f32x4 lc[UP], prr[UP];
#pragma unroll
        for (int u = 0; u < UP; ++u) {
            const int p = p0 + u * NT;
            const size_t ip = (size_t)i * P + (p < P ? p : 0);
            bv[u] = a.bestv[ip];
            ob[u] = a.obj[ip];
            cev[u] = FOCAL ? 0.f : a.cebg[ip];
            ig[u] = IGN ? g.ign[ip] : (uint8_t)0;
            lc[u] = *reinterpret_cast<const f32x4*>(a.loc + ip * 4);
            prr[u] = *reinterpret_cast<const f32x4*>(a.pri + (size_t)(p < P ? p : 0) * 4);
        }
#pragma unroll
        for (int u = 0; u < UP; ++u) {
            const int p = p0 + u * NT;
            if (p < P) {
                const size_t ip = (size_t)i * P + p;
                float best = bv[u];
                int idx = ob[u];
                bool forced = false;
                for (int k = 0; k < ns; ++k)                   // Losses.py:164-167: sequential writes, last GT wins
                    if (sg_bp[k] == p) { idx = s + k; best = 1.f; forced = true; }
                for (int k = s + ns; k < e; ++k)
                    if (a.best_prior[k] == p) { idx = k; best = 1.f; forced = true; }
                const int c = best < a.thr ? bg : (idx - s < SG ? sg_cls[idx - s] : class_index(a.gt_cls[idx], C));
                const bool pos = c != bg;
                a.obj[ip] = idx;
                a.cls[ip] = c;
                float ce = cev[u];
                if (!FOCAL && forced) {                         // (at most one prior per box: its class may have changed, the lane reads its row)
                    const float* x = a.conf + ip * C;
                    float m = x[0];
                    for (int q = 1; q < C; ++q) m = fmaxf(m, x[q]);
                    float se = 0.f;
                    for (int q = 0; q < C; ++q) se += expf(x[q] - m);
                    ce = -((x[c] - m) - logf(se));
                }
                float nv = ce;
                if (pos) {
                    nv = 0.f;
                    my_pos += 1.f;
                    my_ce += ce;
                    if (BOX) {
                        my_l1 += box_term(a.loc_mode, lc[u], prr[u], idx - s < SG ? sg_box[idx - s] : load_box(a.gt, idx)).loss;
                    } else {
                        float g[4];
                        if (idx - s < SG) {
                            const f32x4 g4 = sg_box[idx - s];
                            const float gb[4] = {g4[0], g4[1], g4[2], g4[3]};
                            encode_gt(gb, 0, prr[u], g);
                        } else {
                            encode_gt(a.gt, idx, prr[u], g);
                        }
                        const f32x4 l = lc[u];
                        my_l1 += (fabsf(l[0] - g[0]) + fabsf(l[1] - g[1])) + (fabsf(l[2] - g[2]) + fabsf(l[3] - g[3]));
                    }
                }
                if (IGN) {
                    const bool ignored = !pos && ig[u] != 0;
                    if (!FOCAL && ignored) {
                        nv = 0.f;
                        atomicOr(&ibits[p >> 5], 1u << (p & 31));
                    }
                    if (pos && ig[u] != 0) g.ign[ip] = 0;       // a positive stays positive inside an ignore box
                }
                if (!FOCAL) vals[p] = __float_as_uint(nv > 0.f ? nv : 0.f);      // also maps -0.0 and NaN to +0.0
            }
        }
    }
    {
        const float t0 = wave_sum(my_pos), t1 = wave_sum(my_ce), t2 = wave_sum(my_l1);
        if (lane == 0) { fred[0][wave] = t0; fred[1][wave] = t1; fred[2][wave] = t2; }
    }
    __syncthreads();                                       // vals complete, wave sums written
    if (tid == 0) {
        float npos = 0.f, ce = 0.f, l1 = 0.f;
        for (int w = 0; w < NW; ++w) { npos += fred[0][w]; ce += fred[1][w]; l1 += fred[2][w]; }
        a.stats[i * 4 + 0] = npos; a.stats[i * 4 + 1] = ce; a.stats[i * 4 + 2] = l1;
        s_bcast[0] = (int)npos;
        if (FOCAL) a.stats[i * 4 + 3] = 0.f;
    }
    if (FOCAL) return;                                     // nothing is mined: every prior that is not ignored is in the dense pass
    __syncthreads();

    // ---- C: hard negatives ----
    const long kk = (long)a.ratio * s_bcast[0];
    const int k = kk > P ? P : (int)kk;
    if (k <= 0) {
        for (int p = tid; p < P; p += NT) a.sel[(size_t)i * P + p] = 0;
        if (tid == 0) a.stats[i * 4 + 3] = 0.f;
        return;
    }
    uint32_t prefix = 0, mask = 0;
    int remaining = k;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int b = tid; b < 256; b += NT) hist[b] = 0;
        __syncthreads();
        for (int p0 = 0; p0 < P; p0 += NT) {               // uniform trip count: the ballots below need whole waves
            const int p = p0 + tid;
            const uint32_t u = p < P ? vals[p] : 0u;
            bool act = p < P && (u & mask) == prefix;
            const int bin = (int)((u >> shift) & 255u);
            // equal bins of a wave add once (the upper bytes of CE values are nearly all equal: plain atomics would serialise)
            for (int it = 0; it < 4; ++it) {
                const unsigned long long am = __ballot(act);
                if (am == 0ull) break;
                const int leader = __ffsll((long long)am) - 1;
                const int lb = __shfl(bin, leader, 64);
                const bool same = act && bin == lb;
                const unsigned long long sm = __ballot(same);
                if (lane == leader) atomicAdd(&hist[lb], __popcll(sm));
                act = act && !same;
            }
            if (act) atomicAdd(&hist[bin], 1);
        }
        __syncthreads();
        if (wave == 0) {
            // lane l owns bins 255 - 4 l ... 252 - 4 l (descending); walk down from bin 255 until the count reaches `remaining`
            int c4[4], tot = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { c4[j] = hist[255 - (4 * lane + j)]; tot += c4[j]; }
            int incl = tot;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            int run = incl - tot, d = -1, rem = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int bin = 255 - (4 * lane + j);
                if (d < 0 && bin > 0 && run + c4[j] >= remaining) { d = bin; rem = remaining - run; }
                if (d < 0 && bin > 0) run += c4[j];
            }
            const unsigned long long fm = __ballot(d >= 0);
            if (fm != 0ull) {
                const int first = __ffsll((long long)fm) - 1;
                if (lane == first) { s_bcast[1] = d; s_bcast[2] = rem; }
            } else if (lane == 63) {                       // not reached above bin 0: bin 0 takes what is left (lane 63's run = the count of bins 255 .. 1)
                s_bcast[1] = 0;
                s_bcast[2] = remaining - run;
            }
        }
        __syncthreads();
        prefix |= (uint32_t)s_bcast[1] << shift;
        mask |= 255u << shift;
        remaining = s_bcast[2];
        // (no barrier here: wave 0 writes s_bcast again only behind the next pass's second barrier, which every thread reaches after this read)
    }
    const uint32_t T = prefix;            // k-th largest value; take `remaining` of the elements equal to it
    const int CH = (P + NT - 1) / NT;
    const int p0 = tid * CH, p1 = min(P, p0 + CH);
    float sum_gt = 0.f;
    int n_eq = 0;
    for (int p = p0; p < p1; ++p) {
        const uint32_t u = vals[p];
        if (u > T) sum_gt += __uint_as_float(u);
        n_eq += (u == T);
    }
    int incl = n_eq;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) ired[wave] = incl;
    const float wsum = wave_sum(sum_gt);
    if (lane == 0) fred[0][wave] = wsum;
    __syncthreads();
    int wave_off = 0;
    for (int w = 0; w < wave; ++w) wave_off += ired[w];
    int rank = wave_off + incl - n_eq;     // number of equal elements before this thread's slice
    for (int p = p0; p < p1; ++p) {
        const uint32_t u = vals[p];
        uint8_t sl = 0;
        if (u > T) sl = 1;
        else if (u == T) { sl = rank < remaining ? 1 : 0; ++rank; }
        if (IGN && ((ibits[p >> 5] >> (p & 31)) & 1u)) sl = 0;             // (after the rank: the tie rule counts them as it always did)
        a.sel[(size_t)i * P + p] = sl;
    }
    if (tid == 0) {
        float tot = 0.f;
        for (int w = 0; w < NW; ++w) tot += fred[0][w];
        a.stats[i * 4 + 3] = tot + (float)remaining * __uint_as_float(T);
    }
}

struct FinalArgs {
    const float* loc; const float* conf; const float* gt; const float* pri;
    const int32_t* obj; const int32_t* cls; const uint8_t* sel; const float* stats;
    float* losses; float* dloc; float* dconf;
    int P, C, bs, norm_mode;
    int loc_mode;                                     // finalize kernels <true>: as ImageArgs::loc_mode
    float* npos_out = nullptr;                        // finalize_kernel<., true>: n_pos of the batch for the dense pass, one float
};

// BOX (both finalize kernels): loc_loss is the per-positive mean (or sum) of box_term's loss and dloc its gradient; false is the L1 form
// FOCAL (finalize_kernel, any C, no dynamic LDS): losses[0], losses[2] and dloc only; losses[1] and dconf are the dense pass's.
template <bool BOX, bool FOCAL = false>
__global__ __launch_bounds__(LB) void finalize_kernel(const FinalArgs a) {
    __shared__ float tot[4];
    if (threadIdx.x == 0) {
        float npos = 0.f, ce = 0.f, l1 = 0.f, hn = 0.f;
        for (int i = 0; i < a.bs; ++i) {
            npos += a.stats[i * 4 + 0]; ce += a.stats[i * 4 + 1]; l1 += a.stats[i * 4 + 2]; hn += a.stats[i * 4 + 3];
        }
        tot[0] = npos; tot[1] = ce; tot[2] = l1; tot[3] = hn;
    }
    __syncthreads();
    const float npos = tot[0];
    const float inv = a.norm_mode == 0 ? 1.f / npos : 1.f;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        if (BOX) a.losses[0] = a.norm_mode == 0 ? tot[2] / npos : tot[2];
        else a.losses[0] = a.norm_mode == 0 ? tot[2] / (npos * 4.f) : tot[2] / 4.f;     // nn.L1Loss mean over n_pos*4
        if (!FOCAL) a.losses[1] = a.norm_mode == 0 ? (tot[3] + tot[1]) / npos : (tot[3] + tot[1]);
        if (FOCAL) *a.npos_out = npos;
        a.losses[2] = npos;
    }
    if (a.dloc == nullptr || a.dconf == nullptr) return;
    extern __shared__ __attribute__((aligned(16))) float fstage[];       // [LB][C]: dconf rows of this block's priors
    const int i = blockIdx.y;
    const int pb = blockIdx.x * LB;
    const int p = pb + threadIdx.x;
    const int rows = a.P - pb < LB ? a.P - pb : LB;
    const size_t ip = (size_t)i * a.P + p;
    if (p < a.P) {
        const int c = a.cls[ip];
        const bool pos = c != a.C - 1;
        if constexpr (!FOCAL) {                     // (FOCAL: dconf is the dense pass's, nothing is staged)
            const bool on = pos || a.sel[ip] != 0;
            float* dc = fstage + threadIdx.x * a.C;
            if (on) {                               // (few rows: the conf row is read by its own lane)
                const float* x = a.conf + ip * a.C;
                float m = x[0];
                for (int q = 1; q < a.C; ++q) m = fmaxf(m, x[q]);
                float se = 0.f;
                for (int q = 0; q < a.C; ++q) se += expf(x[q] - m);
                const float r = 1.f / se;
                for (int q = 0; q < a.C; ++q) dc[q] = (expf(x[q] - m) * r - (q == c ? 1.f : 0.f)) * inv;
            } else {
                for (int q = 0; q < a.C; ++q) dc[q] = 0.f;
            }
        }
        f32x4 dl = {0.f, 0.f, 0.f, 0.f};
        if (pos) {
            const f32x4 pr = *reinterpret_cast<const f32x4*>(a.pri + (size_t)p * 4);
            const f32x4 l = *reinterpret_cast<const f32x4*>(a.loc + ip * 4);
            if (BOX) {
                const BoxTerm bt = box_term(a.loc_mode, l, pr, load_box(a.gt, a.obj[ip]));
#pragma unroll
                for (int q = 0; q < 4; ++q) dl[q] = bt.d[q] * inv;
            } else {
                float g[4];
                encode_gt(a.gt, a.obj[ip], pr, g);
                const float sc = inv * 0.25f;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float d = l[q] - g[q];
                    dl[q] = d > 0.f ? sc : (d < 0.f ? -sc : 0.f);
                }
            }
        }
        *reinterpret_cast<f32x4*>(a.dloc + ip * 4) = dl;
    }
    if (FOCAL) return;
    __syncthreads();
    float* const dst = a.dconf + ((size_t)i * a.P + pb) * a.C;
    const int nfl = rows * a.C;
    for (int t = threadIdx.x; t < nfl; t += LB) dst[t] = fstage[t];
}

// L3w (64 < C <= 256): grid (ceil(P / 64), bs), 256 threads; block = 64 consecutive priors of image blockIdx.y
constexpr int RW = 64;
template <bool BOX>
__global__ __launch_bounds__(LB) void finalize_wide_kernel(const FinalArgs a) {
    __shared__ float tot[4];
    __shared__ float s_m[RW], s_r[RW];
    __shared__ int s_c[RW];                         // class of the row, -1 = row not selected (all-zero gradient)
    if (threadIdx.x == 0) {
        float npos = 0.f, ce = 0.f, l1 = 0.f, hn = 0.f;
        for (int i = 0; i < a.bs; ++i) {
            npos += a.stats[i * 4 + 0]; ce += a.stats[i * 4 + 1]; l1 += a.stats[i * 4 + 2]; hn += a.stats[i * 4 + 3];
        }
        tot[0] = npos; tot[1] = ce; tot[2] = l1; tot[3] = hn;
    }
    __syncthreads();
    const float npos = tot[0];
    const float inv = a.norm_mode == 0 ? 1.f / npos : 1.f;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        if (BOX) a.losses[0] = a.norm_mode == 0 ? tot[2] / npos : tot[2];
        else a.losses[0] = a.norm_mode == 0 ? tot[2] / (npos * 4.f) : tot[2] / 4.f;
        a.losses[1] = a.norm_mode == 0 ? (tot[3] + tot[1]) / npos : (tot[3] + tot[1]);
        a.losses[2] = npos;
    }
    if (a.dloc == nullptr || a.dconf == nullptr) return;
    const int i = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pb = blockIdx.x * RW;
    const int rows = a.P - pb < RW ? a.P - pb : RW;
    const int C = a.C;
    const float* const src = a.conf + ((size_t)i * a.P + pb) * C;
    // (max, 1 / sum exp, class) of the selected rows: a wave per row (row index wave-uniform)
    for (int r = wave; r < rows; r += LB / 64) {
        const size_t ip = (size_t)i * a.P + pb + r;
        const int c = a.cls[ip];
        const bool on = c != C - 1 || a.sel[ip] != 0;
        if (on) {
            float v[4];
            load_row_wave(src + (size_t)r * C, C, lane, v);
            const RowStats st = row_stats_wave(v, C, lane);
            if (lane == 0) { s_m[r] = st.m; s_r[r] = 1.f / st.se; s_c[r] = c; }
        } else if (lane == 0) {
            s_c[r] = -1;
        }
    }
    if (tid < rows) {
        const int p = pb + tid;
        const size_t ip = (size_t)i * a.P + p;
        f32x4 dl = {0.f, 0.f, 0.f, 0.f};
        if (a.cls[ip] != C - 1) {
            const f32x4 pr = *reinterpret_cast<const f32x4*>(a.pri + (size_t)p * 4);
            const f32x4 l = *reinterpret_cast<const f32x4*>(a.loc + ip * 4);
            if (BOX) {
                const BoxTerm bt = box_term(a.loc_mode, l, pr, load_box(a.gt, a.obj[ip]));
#pragma unroll
                for (int q = 0; q < 4; ++q) dl[q] = bt.d[q] * inv;
            } else {
                float g[4];
                encode_gt(a.gt, a.obj[ip], pr, g);
                const float sc = inv * 0.25f;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float d = l[q] - g[q];
                    dl[q] = d > 0.f ? sc : (d < 0.f ? -sc : 0.f);
                }
            }
        }
        *reinterpret_cast<f32x4*>(a.dloc + ip * 4) = dl;
    }
    __syncthreads();
    // the block's rows x C floats of dconf as one contiguous stream; conf is read only where the row is selected
    float* const dst = a.dconf + ((size_t)i * a.P + pb) * C;
    const int nfl = rows * C;
    for (int t = tid; t < nfl; t += LB) {
        const int r = t / C, q = t - r * C;
        const int c = s_c[r];
        float d = 0.f;
        if (c >= 0) d = (expf(src[t] - s_m[r]) * s_r[r] - (q == c ? 1.f : 0.f)) * inv;
        dst[t] = d;
    }
}

// ---- Sigmoid focal classification (ssd_multibox_loss_focal, conf_mode 1) ------------------------------------
// One element of the term: logit x of a foreground column, target (the prior's class is this column), alpha (< 0: no weighting) and
// gamma >= 0.  With z = x for a target and -x otherwise,
//     FL = a_t * exp(-gamma * softplus(z)) * softplus(-z)                      (= a_t * (1 - p_t)^gamma * BCE-with-logits)
//     dFL/dx = s * a_t * exp(-gamma * softplus(z)) * (-gamma * sigmoid(z) * softplus(-z) - sigmoid(-z)),     s = +1 / -1
// softplus(u) = max(u, 0) + log1p(exp(-|u|)): both softplus values and both sigmoids come from the one exp(-|x|), nothing overflows
// for a finite x, the two terms of the bracket have the same sign (no cancellation) and gamma = 0 gives a factor of exactly 1.
// The loss and its gradient live in ONE function, as box_term() does for the loc side.
// Arithmetic: the dense pass runs this 7 million times per call, and with libm's expf / log1pf / IEEE division it was 5 x the time of
// moving its bytes.  The two exponentials, the logarithm and the reciprocal are the hardware's (v_exp_f32, v_log_f32, v_rcp_f32: 1 ulp
// each; the exponent's scaling by log2(e) adds |u| * 6e-8 relative to exp(u), which is an absolute error below 3e-8 because
// |u| exp(-|u|) <= 0.37); log1p(e) is e - e^2 / 2 below e = 2^-12, where 1 + e would round e away.
struct FocalTerm { float loss, grad; };
__device__ __forceinline__ FocalTerm focal_term(float x, bool target, float alpha, float gamma) {
    const float z = target ? x : -x;
    const float e = __expf(-fabsf(z));
    const float l1p = e < 0x1p-12f ? e * (1.f - 0.5f * e) : __logf(1.f + e);
    const float sp_z = fmaxf(z, 0.f) + l1p, sp_nz = fmaxf(-z, 0.f) + l1p;       // softplus(z), softplus(-z)
    const float r = __builtin_amdgcn_rcpf(1.f + e);
    const float sg_z = z >= 0.f ? r : e * r, sg_nz = z >= 0.f ? e * r : r;     // sigmoid(z), sigmoid(-z)
    const float a_t = alpha < 0.f ? 1.f : (target ? alpha : 1.f - alpha);
    const float w = a_t * __expf(-gamma * sp_z);
    const float d = w * (-gamma * sg_z * sp_nz - sg_nz);
    return FocalTerm{w * sp_nz, target ? d : -d};
}

struct FocalArgs {
    const float* conf; const int32_t* cls; const uint8_t* ign; const float* n_pos_dev;
    float* dconf; float* part; float* conf_loss;     // conf_loss: where the value goes (losses + 1 of the loss call)
    int P, C, bs, norm_mode, NBR; float alpha, gamma;
    float n_pos;                                     // n_pos_dev == nullptr (ssd_focal_dense): the divisor, given by the caller
};

// n_pos of the batch: the float finalize_kernel<., true> left (the sum its losses[2] is), or the caller's
__device__ __forceinline__ float focal_n_pos(const FocalArgs& a) { return a.n_pos_dev ? *a.n_pos_dev : a.n_pos; }

// L4 focal_dense_kernel: grid (ceil(P / 128), bs), 256 threads; a block owns 128 consecutive priors of image blockIdx.y, whose 128 x C
// logits are one contiguous stream: consecutive threads read consecutive floats and write the same floats of dconf (whole lines both
// ways, four requests per thread in flight), the (row, column) of an element stepped from one division per thread, its class from 128
// ints in LDS -- nothing per class, any C.  Column C-1 and the rows of ignored priors get +0.0 and add nothing.  The block's sum
// leaves in a fixed order (thread, wave butterfly, four waves) to part[blockIdx.y * NBR + blockIdx.x]; dconf == nullptr: the sum only.
constexpr int FR = 128;
__global__ __launch_bounds__(LB) void focal_dense_kernel(const FocalArgs a) {
    __shared__ float s_inv;
    __shared__ float red[4];
    __shared__ int s_c[FR];                         // class of the row; -1 = ignored prior
    const int i = blockIdx.y, tid = threadIdx.x;
    const int pb = blockIdx.x * FR;
    const int rows = a.P - pb < FR ? a.P - pb : FR;
    const int C = a.C;
    if (tid == 0) s_inv = a.norm_mode == 0 ? 1.f / focal_n_pos(a) : 1.f;
    if (tid < rows) {
        const size_t ip = (size_t)i * a.P + pb + tid;
        s_c[tid] = (a.ign != nullptr && a.ign[ip] != 0) ? -1 : a.cls[ip];
    }
    __syncthreads();
    const float inv = s_inv;
    const size_t base = ((size_t)i * a.P + pb) * C;
    const float* const src = a.conf + base;
    float* const dst = a.dconf ? a.dconf + base : nullptr;
    const int nfl = rows * C;
    float sum = 0.f;
    constexpr int UF = 4;
    const int dr = LB / C, dq = LB - dr * C;               // 256 elements on: dr rows and dq columns
    int r = tid / C, q = tid - r * C;
    for (int t0 = tid; t0 < nfl; t0 += UF * LB) {
        float x[UF];
#pragma unroll
        for (int u = 0; u < UF; ++u) {
            const int t = t0 + u * LB;
            x[u] = t < nfl ? src[t] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < UF; ++u) {
            const int t = t0 + u * LB;
            if (t < nfl) {                                 // (then r < rows)
                const int c = s_c[r];
                float d = 0.f;
                if (c >= 0 && q != C - 1) {
                    const FocalTerm ft = focal_term(x[u], q == c, a.alpha, a.gamma);
                    sum += ft.loss;
                    d = ft.grad * inv;
                }
                if (dst) dst[t] = d;
            }
            q += dq;
            r += dr;
            if (q >= C) { q -= C; ++r; }
        }
    }
    const float tot = block_sum_256(sum, red);
    if (tid == 0) a.part[(size_t)i * a.NBR + blockIdx.x] = tot;
}

// L5 focal_sum_kernel: one block; the bs * NBR partials of L4 in a fixed order (thread t takes t, t + 256, ...) -> losses[1]
__global__ __launch_bounds__(LB) void focal_sum_kernel(const FocalArgs a) {
    __shared__ float red[4];
    const int n = a.bs * a.NBR;
    float sum = 0.f;
    for (int t = threadIdx.x; t < n; t += LB) sum += a.part[t];
    const float tot = block_sum_256(sum, red);
    if (threadIdx.x == 0) *a.conf_loss = a.norm_mode == 0 ? tot / focal_n_pos(a) : tot;
}

int g_loss_form = 1;      // 1 = three launches (L1 wide, L2 per image, L3), 0 = the four-launch form (ssd_tune_set_loss_form)

struct LossWs {
    int32_t* best_prior; float* neg; float* part; uint8_t* sel; float* stats; float* partv; int32_t* parti; float* bestv; size_t bytes;
};
LossWs carve(void* ws, int bs, int P, int n_gt) {
    const int NB = ssd_cdiv(P, LB);
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    char* b = reinterpret_cast<char*>(ws);
    size_t o = 0;
    LossWs w;
    w.best_prior = reinterpret_cast<int32_t*>(b + o); o += up((size_t)n_gt * 4);
    w.neg = reinterpret_cast<float*>(b + o); o += up((size_t)bs * P * 4);
    w.part = reinterpret_cast<float*>(b + o); o += up((size_t)bs * NB * 3 * 4);
    w.sel = reinterpret_cast<uint8_t*>(b + o); o += up((size_t)bs * P);
    w.stats = reinterpret_cast<float*>(b + o); o += up((size_t)bs * 4 * 4);
    w.partv = reinterpret_cast<float*>(b + o); o += up((size_t)n_gt * NB * 4 * 4);
    w.parti = reinterpret_cast<int32_t*>(b + o); o += up((size_t)n_gt * NB * 4 * 4);
    w.bestv = reinterpret_cast<float*>(b + o); o += up((size_t)bs * P * 4);
    w.bytes = o;
    return w;
}

// L1 (or L1w) and L2 of the three-launch form; IGN = false, BOX = false is what ssd_multibox_loss has always launched
// ATSS picks the instances of L1 / L1w that read the assignment (L2 is the same kernel); false launches what it always did
template <bool IGN, bool BOX, bool ATSS = false>
int launch_prior_image(const ImageArgs& ia, const IgnArgs& ga, int bs, int NB, hipStream_t st, bool focal) {
    if (focal) {                                    // the matching-only instances: nothing staged per class or per prior, any C
        hipLaunchKernelGGL((loss_prior_wide_kernel<IGN, true, ATSS>), dim3(NB, bs), dim3(256), 0, st, ia, ga);
        SSD_CHECK_LAUNCH();
        hipLaunchKernelGGL((loss_image_kernel<IGN, BOX, true>), dim3(bs), dim3(1024), 0, st, ia, ga);
        SSD_CHECK_LAUNCH();
        return SSD_OK;
    }
    const bool wide_rows = ia.C > 64;               // L1w / L3w: nothing staged per class
    const size_t l1_lds = wide_rows ? 0 : (size_t)4 * 64 * ia.C * 4;
    const size_t l2_lds = (size_t)ia.P * 4 + (IGN ? (size_t)ssd_cdiv(ia.P, 32) * 4 : 0);
    static std::atomic<unsigned long long> raised_l12{0};     // one bit per device (common.h); one word per instance of this template
    int dev;
    if ((l1_lds > 48 * 1024 || l2_lds > 48 * 1024) && ssd_attr_needed(raised_l12, dev)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(loss_prior_kernel<IGN, ATSS>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) !=
                hipSuccess ||
            hipFuncSetAttribute(reinterpret_cast<const void*>(loss_image_kernel<IGN, BOX>), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024) !=
                hipSuccess)
            return SSD_ERR_LAUNCH;
        ssd_attr_done(raised_l12, dev);
    }
    if (wide_rows)
        hipLaunchKernelGGL((loss_prior_wide_kernel<IGN, false, ATSS>), dim3(NB, bs), dim3(256), 0, st, ia, ga);
    else
        hipLaunchKernelGGL((loss_prior_kernel<IGN, ATSS>), dim3(NB, bs), dim3(256), l1_lds, st, ia, ga);
    SSD_CHECK_LAUNCH();
    hipLaunchKernelGGL((loss_image_kernel<IGN, BOX>), dim3(bs), dim3(1024), l2_lds, st, ia, ga);
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}

// L3 (or L3w): shared by the entries; BOX = false is what they have always launched
template <bool BOX>
int launch_finalize(const FinalArgs& fa, hipStream_t st, bool focal = false) {
    const int NB = ssd_cdiv(fa.P, LB);
    const bool grads = fa.dloc != nullptr;
    if (focal) {
        hipLaunchKernelGGL((finalize_kernel<BOX, true>), grads ? dim3(NB, fa.bs) : dim3(1, 1), dim3(LB), 0, st, fa);
        SSD_CHECK_LAUNCH();
        return SSD_OK;
    }
    if (fa.C > 64) {
        hipLaunchKernelGGL(finalize_wide_kernel<BOX>, grads ? dim3(ssd_cdiv(fa.P, RW), fa.bs) : dim3(1, 1), dim3(LB), 0, st, fa);
        SSD_CHECK_LAUNCH();
        return SSD_OK;
    }
    const size_t fin_lds = grads ? (size_t)LB * fa.C * 4 : 0;
    if (fin_lds > 48 * 1024) {
        static std::atomic<unsigned long long> raised_fin{0};
        int dev;
        if (ssd_attr_needed(raised_fin, dev)) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(finalize_kernel<BOX>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024) !=
                hipSuccess)
                return SSD_ERR_LAUNCH;
            ssd_attr_done(raised_fin, dev);
        }
    }
    hipLaunchKernelGGL(finalize_kernel<BOX>, grads ? dim3(NB, fa.bs) : dim3(1, 1), dim3(LB), fin_lds, st, fa);
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}

// Everything an entry receives: ssd_multibox_loss_box's parameters in their order, plus with_ign ahead of the ignore arguments.
// An entry without ignore regions leaves with_ign false (the ignore fields are then read by nothing); one without a choice of
// localisation term leaves loc_mode 0.
struct LossCall {
    const float* loc; const float* conf; const float* gt_boxes; const float* gt_classes; const int32_t* img_start;
    int bs, n_gt;
    const float* priors_cxcywh; const float* priors_xyxy;
    int P, n_classes; float iou_threshold; int neg_pos_ratio, norm_mode;
    bool with_ign; const float* ign_boxes; const int32_t* ign_start; int n_ign; float ignore_threshold; int overlap_mode;
    int loc_mode;
    int conf_mode = 0; float focal_alpha = 0.25f, focal_gamma = 2.f;      // ssd_multibox_loss_focal: 1 = sigmoid focal classification
    int match_mode = 0; int level_status = SSD_OK; AtssLevels levels{};   // ssd_multibox_loss_atss: 1 = ATSS; ssd_internal_atss_levels' verdict
    float* losses; int32_t* obj; int32_t* cls; uint8_t* ign; float* dloc; float* dconf;
    void* workspace; size_t workspace_bytes; hipStream_t stream;
};

// alpha in [0, 1] or negative (no weighting), gamma >= 0 and finite; a NaN fails
bool focal_params_ok(float alpha, float gamma) { return alpha <= 1.f && gamma >= 0.f && gamma <= FLT_MAX; }

// The status of a call in the header's order: null, shape, alignment, workspace
int check_loss_call(const LossCall& c) {
    if (!c.loc || !c.conf || !c.gt_boxes || !c.gt_classes || !c.img_start || !c.priors_cxcywh || !c.priors_xyxy || !c.losses || !c.obj ||
        !c.cls || !c.workspace)
        return SSD_ERR_NULL;
    if ((c.dloc == nullptr) != (c.dconf == nullptr)) return SSD_ERR_NULL;
    if (c.with_ign && (!c.ign_start || !c.ign || (c.n_ign > 0 && !c.ign_boxes))) return SSD_ERR_NULL;
    if (c.match_mode != 0 && c.level_status == SSD_ERR_NULL) return SSD_ERR_NULL;
    if (c.bs <= 0 || c.n_gt < c.bs || c.P <= 0 || c.P > 36000 || c.n_classes < 2 || c.n_classes > 256 || c.neg_pos_ratio < 0 ||
        (c.norm_mode != 0 && c.norm_mode != 1) || c.loc_mode < 0 || c.loc_mode > 4)
        return SSD_ERR_BAD_SHAPE;
    if ((c.conf_mode != 0 && c.conf_mode != 1) || !focal_params_ok(c.focal_alpha, c.focal_gamma)) return SSD_ERR_BAD_SHAPE;
    if (c.with_ign && (c.n_ign < 0 || (c.overlap_mode != 0 && c.overlap_mode != 1))) return SSD_ERR_BAD_SHAPE;
    if ((c.match_mode != 0 && c.match_mode != 1) || (c.match_mode == 1 && c.level_status != SSD_OK)) return SSD_ERR_BAD_SHAPE;
    if (!ssd_aligned16(c.loc) || !ssd_aligned16(c.priors_cxcywh) || !ssd_aligned16(c.priors_xyxy) || (c.dloc && !ssd_aligned16(c.dloc)) ||
        !ssd_aligned16(c.workspace))
        return SSD_ERR_ALIGN;
    if (c.with_ign && c.n_ign > 0 && !ssd_aligned16(c.ign_boxes)) return SSD_ERR_ALIGN;
    if (c.workspace_bytes < carve(nullptr, c.bs, c.P, c.n_gt).bytes + (c.match_mode == 1 ? ssd_internal_atss_key_bytes(c.bs, c.P) : 0))
        return SSD_ERR_WORKSPACE;
    return SSD_OK;
}

// L4 and L5, one place for the loss call and for ssd_focal_dense
int launch_focal_dense(const FocalArgs& za, hipStream_t st) {
    hipLaunchKernelGGL(focal_dense_kernel, dim3(za.NBR, za.bs), dim3(LB), 0, st, za);
    SSD_CHECK_LAUNCH();
    hipLaunchKernelGGL(focal_sum_kernel, dim3(1), dim3(LB), 0, st, za);
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}

// The three launches of a checked call.  with_ign picks the IGN instances of L1 / L1w / L2, loc_mode != 0 the BOX instances of L2 and
// L3 / L3w: without either these are the kernels of the plain loss.
int run_loss(const LossCall& c) {
    const LossWs w = carve(c.workspace, c.bs, c.P, c.n_gt);
    const int NB = ssd_cdiv(c.P, LB);
    // match_mode 1: the keys lie behind what every entry has; L1 / L1w answer L2's threshold test with +-inf, against 0.5 whatever
    // the caller left in iou_threshold
    const bool atss = c.match_mode == 1;
    unsigned long long* const keys = atss ? reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(c.workspace) + w.bytes) : nullptr;
    if (atss) {
        const int rk = ssd_internal_atss_keys(c.gt_boxes, c.img_start, c.bs, c.n_gt, c.priors_cxcywh, c.priors_xyxy, c.P, c.levels, keys,
                                              nullptr, nullptr, nullptr, nullptr, c.stream);
        if (rk != SSD_OK) return rk;
    }
    const ImageArgs ia{c.loc, c.conf, c.gt_boxes, c.gt_classes, c.img_start, c.priors_cxcywh, c.priors_xyxy, w.partv, w.parti, w.bestv,
                       w.neg, w.best_prior, c.obj, c.cls, w.sel, w.stats, c.P, c.n_classes, c.neg_pos_ratio, NB * 4,
                       atss ? 0.5f : c.iou_threshold, c.loc_mode, keys};
    const IgnArgs ga = c.with_ign ? IgnArgs{c.ign_boxes, c.ign_start, c.ign, c.ignore_threshold, c.overlap_mode}
                                  : IgnArgs{nullptr, nullptr, nullptr, 0.f, 0};
    const FinalArgs fa{c.loc, c.conf, c.gt_boxes, c.priors_cxcywh, c.obj, c.cls, w.sel, w.stats, c.losses, c.dloc, c.dconf, c.P,
                       c.n_classes, c.bs, c.norm_mode, c.loc_mode, w.part};
    const bool box = c.loc_mode != 0, focal = c.conf_mode != 0;
    int rc;
    if (atss) {
        if (c.with_ign)
            rc = box ? launch_prior_image<true, true, true>(ia, ga, c.bs, NB, c.stream, focal)
                     : launch_prior_image<true, false, true>(ia, ga, c.bs, NB, c.stream, focal);
        else
            rc = box ? launch_prior_image<false, true, true>(ia, ga, c.bs, NB, c.stream, focal)
                     : launch_prior_image<false, false, true>(ia, ga, c.bs, NB, c.stream, focal);
    } else if (c.with_ign)
        rc = box ? launch_prior_image<true, true>(ia, ga, c.bs, NB, c.stream, focal)
                 : launch_prior_image<true, false>(ia, ga, c.bs, NB, c.stream, focal);
    else
        rc = box ? launch_prior_image<false, true>(ia, ga, c.bs, NB, c.stream, focal)
                 : launch_prior_image<false, false>(ia, ga, c.bs, NB, c.stream, focal);
    if (rc != SSD_OK) return rc;
    rc = box ? launch_finalize<true>(fa, c.stream, focal) : launch_finalize<false>(fa, c.stream, focal);
    if (rc != SSD_OK || !focal) return rc;
    // conf_mode 1: the dense pass (conf_loss partials, dconf) and the fixed-order sum; the partials lie where the cross entropy of
    // the mined form lay (bs * ceil(P / 128) of its bs * P floats) and n_pos in the first float of the four-launch form's partials, so
    // the workspace is the one every entry has
    return launch_focal_dense(FocalArgs{c.conf, c.cls, c.with_ign ? c.ign : nullptr, w.part, c.dconf, w.neg, c.losses + 1, c.P, c.n_classes, c.bs,
                                        c.norm_mode, ssd_cdiv(c.P, FR), c.focal_alpha, c.focal_gamma, 0.f},
                              c.stream);
}

// The four-launch form of rounds 1-3 (K1 - K3, then L3), the cross-check ssd_tune_set_loss_form(0) selects.  It has neither ignore
// regions nor box terms and is reached from ssd_multibox_loss alone.
int run_loss_four_launch(const LossCall& c) {
    hipStream_t st = c.stream;
    const LossWs w = carve(c.workspace, c.bs, c.P, c.n_gt);
    const int NB = ssd_cdiv(c.P, LB);
    hipLaunchKernelGGL(best_prior_per_gt_kernel, dim3(c.n_gt), dim3(256), 0, st, c.gt_boxes, c.priors_xyxy, c.P, w.best_prior);
    SSD_CHECK_LAUNCH();
    MatchArgs ma{c.loc, c.conf, c.gt_boxes, c.gt_classes, c.img_start, w.best_prior, c.priors_cxcywh, c.priors_xyxy,
                 c.obj, c.cls, w.neg, w.part, c.P, c.n_classes, NB, c.iou_threshold};
    hipLaunchKernelGGL(match_ce_kernel, dim3(NB, c.bs), dim3(LB), 0, st, ma);
    SSD_CHECK_LAUNCH();
    const size_t hn_lds = (size_t)c.P * sizeof(uint32_t);
    if (hn_lds > 48 * 1024) {
        static std::atomic<unsigned long long> raised{0};     // one bit per device (common.h)
        int dev;
        if (ssd_attr_needed(raised, dev)) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(hard_negative_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    150 * 1024) != hipSuccess)
                return SSD_ERR_LAUNCH;
            ssd_attr_done(raised, dev);
        }
    }
    hipLaunchKernelGGL(hard_negative_kernel, dim3(c.bs), dim3(HB), hn_lds, st, w.neg, w.part, w.sel, w.stats, c.P, NB, c.neg_pos_ratio);
    SSD_CHECK_LAUNCH();
    return launch_finalize<false>(FinalArgs{c.loc, c.conf, c.gt_boxes, c.priors_cxcywh, c.obj, c.cls, w.sel, w.stats, c.losses, c.dloc, c.dconf,
                                            c.P, c.n_classes, c.bs, c.norm_mode},
                                  st);
}

}  // namespace

// Cross-check aid: 1 = the three-launch form (default), 0 = the four-launch form of rounds 1-3.
extern "C" int ssd_tune_set_loss_form(int three_launch) {
    g_loss_form = three_launch ? 1 : 0;
    return SSD_OK;
}

// One workspace for the three entries: the ignore byte per prior is the caller's `ign`, nothing is kept per ignore box or per loc_mode.
extern "C" size_t ssd_multibox_loss_workspace(int bs, int P, int n_gt) {
    if (bs <= 0 || P <= 0 || n_gt <= 0) return 0;
    return carve(nullptr, bs, P, n_gt).bytes;
}

extern "C" size_t ssd_multibox_loss_ignore_workspace(int bs, int P, int n_gt, int n_ign) {
    if (n_ign < 0) return 0;
    return ssd_multibox_loss_workspace(bs, P, n_gt);
}

extern "C" size_t ssd_multibox_loss_box_workspace(int bs, int P, int n_gt, int n_ign) {
    return ssd_multibox_loss_ignore_workspace(bs, P, n_gt, n_ign);
}

extern "C" size_t ssd_multibox_loss_focal_workspace(int bs, int P, int n_gt, int n_ign) {
    return ssd_multibox_loss_ignore_workspace(bs, P, n_gt, n_ign);
}

// The plain loss: no ignore regions, L1 localisation term.  The one entry ssd_tune_set_loss_form reaches.
extern "C" int ssd_multibox_loss(const float* loc, const float* conf, const float* gt_boxes, const float* gt_classes,
                                 const int32_t* img_start, int bs, int n_gt, const float* priors_cxcywh,
                                 const float* priors_xyxy, int P, int n_classes, float iou_threshold, int neg_pos_ratio,
                                 int norm_mode, float* losses, int32_t* obj, int32_t* cls, float* dloc, float* dconf,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    const LossCall c{.loc = loc, .conf = conf, .gt_boxes = gt_boxes, .gt_classes = gt_classes, .img_start = img_start, .bs = bs, .n_gt = n_gt,
                     .priors_cxcywh = priors_cxcywh, .priors_xyxy = priors_xyxy, .P = P, .n_classes = n_classes,
                     .iou_threshold = iou_threshold, .neg_pos_ratio = neg_pos_ratio, .norm_mode = norm_mode, .with_ign = false,
                     .loc_mode = 0, .losses = losses, .obj = obj, .cls = cls, .dloc = dloc, .dconf = dconf, .workspace = workspace,
                     .workspace_bytes = workspace_bytes, .stream = (hipStream_t)stream};
    const int bad = check_loss_call(c);
    if (bad != SSD_OK) return bad;
    return g_loss_form != 0 ? run_loss(c) : run_loss_four_launch(c);
}

// The loss with ignore regions (always: a null ign_start or ign is an error here), L1 localisation term
extern "C" int ssd_multibox_loss_ignore(const float* loc, const float* conf, const float* gt_boxes, const float* gt_classes,
                                        const int32_t* img_start, int bs, int n_gt, const float* priors_cxcywh,
                                        const float* priors_xyxy, int P, int n_classes, float iou_threshold, int neg_pos_ratio,
                                        int norm_mode, const float* ign_boxes, const int32_t* ign_start, int n_ign,
                                        float ignore_threshold, int overlap_mode, float* losses, int32_t* obj, int32_t* cls,
                                        uint8_t* ign, float* dloc, float* dconf, void* workspace, size_t workspace_bytes, void* stream) {
    const LossCall c{.loc = loc, .conf = conf, .gt_boxes = gt_boxes, .gt_classes = gt_classes, .img_start = img_start, .bs = bs, .n_gt = n_gt,
                     .priors_cxcywh = priors_cxcywh, .priors_xyxy = priors_xyxy, .P = P, .n_classes = n_classes,
                     .iou_threshold = iou_threshold, .neg_pos_ratio = neg_pos_ratio, .norm_mode = norm_mode, .with_ign = true,
                     .ign_boxes = ign_boxes, .ign_start = ign_start, .n_ign = n_ign, .ignore_threshold = ignore_threshold,
                     .overlap_mode = overlap_mode, .loc_mode = 0, .losses = losses, .obj = obj, .cls = cls, .ign = ign, .dloc = dloc,
                     .dconf = dconf, .workspace = workspace, .workspace_bytes = workspace_bytes, .stream = (hipStream_t)stream};
    const int bad = check_loss_call(c);
    return bad != SSD_OK ? bad : run_loss(c);
}

// The loss with a choice of localisation term; ignore regions where ign_start is given
extern "C" int ssd_multibox_loss_box(const float* loc, const float* conf, const float* gt_boxes, const float* gt_classes,
                                     const int32_t* img_start, int bs, int n_gt, const float* priors_cxcywh, const float* priors_xyxy,
                                     int P, int n_classes, float iou_threshold, int neg_pos_ratio, int norm_mode, const float* ign_boxes,
                                     const int32_t* ign_start, int n_ign, float ignore_threshold, int overlap_mode, int loc_mode,
                                     float* losses, int32_t* obj, int32_t* cls, uint8_t* ign, float* dloc, float* dconf, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    const LossCall c{.loc = loc, .conf = conf, .gt_boxes = gt_boxes, .gt_classes = gt_classes, .img_start = img_start, .bs = bs, .n_gt = n_gt,
                     .priors_cxcywh = priors_cxcywh, .priors_xyxy = priors_xyxy, .P = P, .n_classes = n_classes,
                     .iou_threshold = iou_threshold, .neg_pos_ratio = neg_pos_ratio, .norm_mode = norm_mode, .with_ign = ign_start != nullptr,
                     .ign_boxes = ign_boxes, .ign_start = ign_start, .n_ign = n_ign, .ignore_threshold = ignore_threshold,
                     .overlap_mode = overlap_mode, .loc_mode = loc_mode, .losses = losses, .obj = obj, .cls = cls, .ign = ign, .dloc = dloc,
                     .dconf = dconf, .workspace = workspace, .workspace_bytes = workspace_bytes, .stream = (hipStream_t)stream};
    const int bad = check_loss_call(c);
    return bad != SSD_OK ? bad : run_loss(c);
}

// The loss with a choice of classification term beside ssd_multibox_loss_box's options: conf_mode 0 is that entry, launch for launch;
// conf_mode 1 the sigmoid focal term (neg_pos_ratio is then not read)
extern "C" int ssd_multibox_loss_focal(const float* loc, const float* conf, const float* gt_boxes, const float* gt_classes,
                                       const int32_t* img_start, int bs, int n_gt, const float* priors_cxcywh, const float* priors_xyxy,
                                       int P, int n_classes, float iou_threshold, int neg_pos_ratio, int norm_mode, const float* ign_boxes,
                                       const int32_t* ign_start, int n_ign, float ignore_threshold, int overlap_mode, int loc_mode,
                                       int conf_mode, float focal_alpha, float focal_gamma, float* losses, int32_t* obj, int32_t* cls,
                                       uint8_t* ign, float* dloc, float* dconf, void* workspace, size_t workspace_bytes, void* stream) {
    const LossCall c{.loc = loc, .conf = conf, .gt_boxes = gt_boxes, .gt_classes = gt_classes, .img_start = img_start, .bs = bs, .n_gt = n_gt,
                     .priors_cxcywh = priors_cxcywh, .priors_xyxy = priors_xyxy, .P = P, .n_classes = n_classes,
                     .iou_threshold = iou_threshold, .neg_pos_ratio = conf_mode == 1 && neg_pos_ratio < 0 ? 0 : neg_pos_ratio,
                     .norm_mode = norm_mode, .with_ign = ign_start != nullptr, .ign_boxes = ign_boxes, .ign_start = ign_start, .n_ign = n_ign,
                     .ignore_threshold = ignore_threshold, .overlap_mode = overlap_mode, .loc_mode = loc_mode, .conf_mode = conf_mode,
                     .focal_alpha = focal_alpha, .focal_gamma = focal_gamma, .losses = losses, .obj = obj, .cls = cls, .ign = ign,
                     .dloc = dloc, .dconf = dconf, .workspace = workspace, .workspace_bytes = workspace_bytes, .stream = (hipStream_t)stream};
    const int bad = check_loss_call(c);
    return bad != SSD_OK ? bad : run_loss(c);
}

// The loss with a choice of matching rule beside ssd_multibox_loss_focal's options: match_mode 0 is that entry, launch for launch;
// match_mode 1 runs the ATSS assignment pass (atss.hip) in front and the instances of L1 / L1w that read it
extern "C" size_t ssd_multibox_loss_atss_workspace(int bs, int P, int n_gt, int n_ign) {
    const size_t base = ssd_multibox_loss_ignore_workspace(bs, P, n_gt, n_ign);
    return base ? base + ssd_internal_atss_key_bytes(bs, P) : 0;
}

extern "C" int ssd_multibox_loss_atss(const float* loc, const float* conf, const float* gt_boxes, const float* gt_classes,
                                      const int32_t* img_start, int bs, int n_gt, const float* priors_cxcywh, const float* priors_xyxy,
                                      int P, int n_classes, float iou_threshold, int neg_pos_ratio, int norm_mode, const float* ign_boxes,
                                      const int32_t* ign_start, int n_ign, float ignore_threshold, int overlap_mode, int loc_mode,
                                      int conf_mode, float focal_alpha, float focal_gamma, int match_mode, int topk, int n_levels,
                                      const int* level_cells, const int* level_anchors, float* losses, int32_t* obj, int32_t* cls,
                                      uint8_t* ign, float* dloc, float* dconf, void* workspace, size_t workspace_bytes, void* stream) {
    LossCall c{.loc = loc, .conf = conf, .gt_boxes = gt_boxes, .gt_classes = gt_classes, .img_start = img_start, .bs = bs, .n_gt = n_gt,
               .priors_cxcywh = priors_cxcywh, .priors_xyxy = priors_xyxy, .P = P, .n_classes = n_classes,
               .iou_threshold = iou_threshold, .neg_pos_ratio = conf_mode == 1 && neg_pos_ratio < 0 ? 0 : neg_pos_ratio,
               .norm_mode = norm_mode, .with_ign = ign_start != nullptr, .ign_boxes = ign_boxes, .ign_start = ign_start, .n_ign = n_ign,
               .ignore_threshold = ignore_threshold, .overlap_mode = overlap_mode, .loc_mode = loc_mode, .conf_mode = conf_mode,
               .focal_alpha = focal_alpha, .focal_gamma = focal_gamma, .match_mode = match_mode, .losses = losses, .obj = obj, .cls = cls,
               .ign = ign, .dloc = dloc, .dconf = dconf, .workspace = workspace, .workspace_bytes = workspace_bytes,
               .stream = (hipStream_t)stream};
    if (match_mode != 0) c.level_status = ssd_internal_atss_levels(P, topk, n_levels, level_cells, level_anchors, c.levels);
    const int bad = check_loss_call(c);
    return bad != SSD_OK ? bad : run_loss(c);
}

// The dense pass of conf_mode 1 alone (L4 and L5, launched as the loss launches them), for tests and tools: cls (bs, P) int32 classes
// (C-1 = background), ign (bs, P) bytes or NULL, n_pos the divisor of norm_mode 0.  conf_loss[0] receives the value of losses[1];
// dconf may be NULL.  workspace: 4 * bs * ceil(P / 128) bytes rounded up to a multiple of 256, 16-byte aligned.
extern "C" size_t ssd_focal_dense_workspace(int bs, int P) {
    if (bs <= 0 || P <= 0) return 0;
    return ((size_t)bs * ssd_cdiv(P, FR) * 4 + 255) / 256 * 256;
}

extern "C" int ssd_focal_dense(const float* conf, const int32_t* cls, const uint8_t* ign, int bs, int P, int n_classes, float n_pos,
                               int norm_mode, float focal_alpha, float focal_gamma, float* conf_loss, float* dconf, void* workspace,
                               size_t workspace_bytes, void* stream) {
    if (!conf || !cls || !conf_loss || !workspace) return SSD_ERR_NULL;
    if (bs <= 0 || P <= 0 || P > 36000 || n_classes < 2 || n_classes > 256 || (norm_mode != 0 && norm_mode != 1) || !(n_pos > 0.f) ||
        !focal_params_ok(focal_alpha, focal_gamma))
        return SSD_ERR_BAD_SHAPE;
    if (!ssd_aligned16(workspace)) return SSD_ERR_ALIGN;
    if (workspace_bytes < ssd_focal_dense_workspace(bs, P)) return SSD_ERR_WORKSPACE;
    return launch_focal_dense(FocalArgs{conf, cls, ign, nullptr, dconf, reinterpret_cast<float*>(workspace), conf_loss, P, n_classes, bs,
                                        norm_mode, ssd_cdiv(P, FR), focal_alpha, focal_gamma, n_pos},
                              (hipStream_t)stream);
}

// ATSS matching for the MultiBox loss (Zhang et al., CVPR 2020): which priors are the positives of a box.
//
// atss_assign_kernel   one workgroup of 512 threads per ground-truth box:
//   A  squared f32 distance of every cell centre (the cell's first prior) to the box centre, all levels, as sortable bits in LDS
//      (NaN -> 0xFFFFFFFF: last)
//   B  a wave per level: min(topk, cells) rounds of "smallest (distance bits, cell) above the last one taken" over the level's
//      slice of LDS, a 64-bit wave arg-min by shuffles per round -- nearest first, equal distances -> lower cell, no marking
//   C  IoU of every candidate (level, rank of the cell, prior of the cell) with the box into LDS, over the distances
//   D  f64 mean and unbiased variance: lane j adds candidates j, j + 64, ... in order, the 64 partial sums by a butterfly (xor 32 .. 1);
//      every wave does it for itself (the same bits in every lane of every wave, no barrier)
//   E  d = iou - mean: d >= 0 && d * d >= var, and the prior's centre strictly inside the box -> a 64-bit integer atomicMax of
//      (IoU bits << 32) | (0xFFFFFFFF - box) into keys[image][prior]: the largest IoU wins, equal -> the lower box, in any order
// The keys are zeroed by a memset node in front (0 = no box).  No float atomics; NaNs compare false everywhere, so a box with a NaN
// or without width is nobody's match, and every index stays inside the level description, which the host checked against P.
//
// The IoU is loss.hip's f32 op sequence (sub, max, min, mul, add, sub, IEEE divide) and the distance is mul, mul, add: this file is
// compiled with -ffp-contract=off and the pragma below keeps a*b+c from being fused, in f32 and in f64.
#include "atss.h"
#pragma clang fp contract(off)

namespace {

constexpr int AB = 512;       // threads of the assignment pass: a wave per level

struct AtssArgs {
    const float* gt; const int32_t* img_start; const float* pri; const float* pri_xyxy;
    unsigned long long* keys; int32_t* n_cand; double* mean; double* var; int32_t* n_acc;
    int bs, P; AtssLevels lv;
};

// loss.hip's iou_xyxy, the box in the first place
__device__ __forceinline__ float atss_iou(float ax1, float ay1, float ax2, float ay2, float area_a, float bx1, float by1, float bx2,
                                          float by2, float area_b) {
    const float lx = fmaxf(ax1, bx1), ly = fmaxf(ay1, by1);
    const float hx = fminf(ax2, bx2), hy = fminf(ay2, by2);
    const float dx = fmaxf(hx - lx, 0.f), dy = fmaxf(hy - ly, 0.f);
    const float inter = dx * dy;
    const float uni = (area_a + area_b) - inter;
    return inter / uni;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(AB) void atss_assign_kernel(const AtssArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn[];      // [max(cells of all levels, candidates)]
    __shared__ int s_cell[ATSS_MAX_LEVELS][ATSS_MAX_TOPK];               // the chosen cells of each level, nearest first
    __shared__ int s_coff[ATSS_MAX_LEVELS + 1], s_poff[ATSS_MAX_LEVELS + 1], s_noff[ATSS_MAX_LEVELS + 1];     // first cell / prior / candidate
    __shared__ int s_acc;
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nl = a.lv.n_levels, topk = a.lv.topk;
    // rows of gt_boxes outside [img_start[0], img_start[bs]) belong to no image (a captured step keeps spare rows): nobody's match
    if (k < a.img_start[0] || k >= a.img_start[a.bs]) {
        if (tid == 0) {
            if (a.n_cand) a.n_cand[k] = 0;
            if (a.mean) a.mean[k] = 0.0;
            if (a.var) a.var[k] = 0.0;
            if (a.n_acc) a.n_acc[k] = 0;
        }
        return;
    }
    if (tid == 0) {
        int co = 0, po = 0, no = 0;
        for (int l = 0; l < nl; ++l) {
            s_coff[l] = co; s_poff[l] = po; s_noff[l] = no;
            const int cells = a.lv.cells[l], anch = a.lv.anchors[l];
            co += cells;
            po += cells * anch;
            no += (cells < topk ? cells : topk) * anch;
        }
        s_coff[nl] = co; s_poff[nl] = po; s_noff[nl] = no;
        s_acc = 0;
    }
    // the image of box k: the last i with img_start[i] <= k (inside 0 .. bs-1 whatever img_start holds)
    int i = 0;
    for (int hi = a.bs; hi - i > 1;) {
        const int mid = (i + hi) >> 1;
        if (a.img_start[mid] <= k) i = mid; else hi = mid;
    }
    const float x1 = a.gt[k * 4 + 0], y1 = a.gt[k * 4 + 1], x2 = a.gt[k * 4 + 2], y2 = a.gt[k * 4 + 3];
    const float gcx = (x1 + x2) / 2.f, gcy = (y1 + y2) / 2.f;
    const float area_g = (x2 - x1) * (y2 - y1);
    __syncthreads();

    // ---- A: distance bits of every cell ----
    const int ncell = s_coff[nl];
    for (int c = tid; c < ncell; c += AB) {
        int l = 0;
        while (l + 1 < nl && c >= s_coff[l + 1]) ++l;
        const size_t p = (size_t)s_poff[l] + (size_t)(c - s_coff[l]) * a.lv.anchors[l];
        const float dx = a.pri[p * 4 + 0] - gcx, dy = a.pri[p * 4 + 1] - gcy;
        const float d = dx * dx + dy * dy;
        dyn[c] = d != d ? 0xFFFFFFFFu : __float_as_uint(d);
    }
    __syncthreads();

    // ---- B: a wave per level, nearest cells first ----
    if (wave < nl) {
        const int cells = a.lv.cells[wave];
        const int nsel = cells < topk ? cells : topk;
        const uint32_t* const dk = dyn + s_coff[wave];
        unsigned long long prev = 0ull;
        for (int r = 0; r < nsel; ++r) {
            unsigned long long best = ~0ull;                             // (no cell has this key: a cell index is below 2^31)
#pragma unroll 8
            for (int c = lane; c < cells; c += 64) {                    // (unrolled: the LDS reads of a round are in flight together)
                const unsigned long long key = ((unsigned long long)dk[c] << 32) | (uint32_t)c;
                if ((r == 0 || key > prev) && key < best) best = key;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long b2 = __shfl_xor(best, o, 64);
                if (b2 < best) best = b2;
            }
            prev = best;
            if (lane == 0) s_cell[wave][r] = (int)(uint32_t)best;
        }
    }
    __syncthreads();

    // ---- C: candidate IoUs (over the distances, which nobody reads any more) ----
    const int ncand = s_noff[nl];
    for (int c = tid; c < ncand; c += AB) {
        int l = 0;
        while (l + 1 < nl && c >= s_noff[l + 1]) ++l;
        const int anch = a.lv.anchors[l];
        const int q = c - s_noff[l], r = q / anch, an = q - r * anch;
        const size_t p = (size_t)s_poff[l] + (size_t)s_cell[l][r] * anch + an;
        const f32x4 b = *reinterpret_cast<const f32x4*>(a.pri_xyxy + p * 4);
        const float area_b = (b[2] - b[0]) * (b[3] - b[1]);
        dyn[c] = __float_as_uint(atss_iou(x1, y1, x2, y2, area_g, b[0], b[1], b[2], b[3], area_b));
    }
    __syncthreads();

    // ---- D: mean and unbiased variance, every wave for itself ----
    double sum = 0.0;
    for (int c = lane; c < ncand; c += 64) sum += (double)__uint_as_float(dyn[c]);
    const double mean = wave_sum_f64(sum) / (double)ncand;
    double sq = 0.0;
    for (int c = lane; c < ncand; c += 64) {
        const double d = (double)__uint_as_float(dyn[c]) - mean;
        sq += d * d;
    }
    sq = wave_sum_f64(sq);
    const double var = ncand > 1 ? sq / (double)(ncand - 1) : 0.0;

    // ---- E: the accept test and the conflict rule ----
    for (int c0 = 0; c0 < ncand; c0 += AB) {                             // uniform trip count: the ballot needs whole waves
        const int c = c0 + tid;
        bool ok = false;
        if (c < ncand) {
            int l = 0;
            while (l + 1 < nl && c >= s_noff[l + 1]) ++l;
            const int anch = a.lv.anchors[l];
            const int q = c - s_noff[l], r = q / anch, an = q - r * anch;
            const size_t p = (size_t)s_poff[l] + (size_t)s_cell[l][r] * anch + an;
            const uint32_t bits = dyn[c];
            const double d = (double)__uint_as_float(bits) - mean;
            const float pcx = a.pri[p * 4 + 0], pcy = a.pri[p * 4 + 1];
            ok = d >= 0.0 && d * d >= var && x1 < pcx && pcx < x2 && y1 < pcy && pcy < y2;
            if (ok) atomicMax(a.keys + (size_t)i * a.P + p, ((unsigned long long)bits << 32) | (0xFFFFFFFFu - (uint32_t)k));
        }
        const unsigned long long m = __ballot(ok);
        if (lane == 0 && m != 0ull) atomicAdd(&s_acc, __popcll(m));
    }
    __syncthreads();
    if (tid == 0) {
        if (a.n_cand) a.n_cand[k] = ncand;
        if (a.mean) a.mean[k] = mean;
        if (a.var) a.var[k] = var;
        if (a.n_acc) a.n_acc[k] = s_acc;
    }
}

// keys -> box index or -1 (the bare entry's output)
__global__ __launch_bounds__(256) void atss_unpack_kernel(const unsigned long long* __restrict__ keys, int32_t* __restrict__ assign, int n) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < n) {
        const unsigned long long key = keys[t];
        assign[t] = key != 0ull ? (int32_t)(0xFFFFFFFFu - (uint32_t)key) : -1;
    }
}

}  // namespace

int ssd_internal_atss_levels(int P, int topk, int n_levels, const int* level_cells, const int* level_anchors, AtssLevels& out) {
    if (!level_cells || !level_anchors) return SSD_ERR_NULL;
    if (topk < 1 || topk > ATSS_MAX_TOPK || n_levels < 1 || n_levels > ATSS_MAX_LEVELS) return SSD_ERR_BAD_SHAPE;
    out = AtssLevels{};
    out.n_levels = n_levels;
    out.topk = topk;
    long long sum = 0;
    for (int l = 0; l < n_levels; ++l) {
        if (level_cells[l] < 1 || level_anchors[l] < 1) return SSD_ERR_BAD_SHAPE;
        out.cells[l] = level_cells[l];
        out.anchors[l] = level_anchors[l];
        sum += (long long)level_cells[l] * level_anchors[l];
        if (sum > P) return SSD_ERR_BAD_SHAPE;
    }
    return sum == P ? SSD_OK : SSD_ERR_BAD_SHAPE;
}

size_t ssd_internal_atss_key_bytes(int bs, int P) { return ((size_t)bs * P * 8 + 255) / 256 * 256; }

int ssd_internal_atss_keys(const float* gt, const int32_t* img_start, int bs, int n_gt, const float* pri, const float* pri_xyxy, int P,
                           const AtssLevels& lv, unsigned long long* keys, int32_t* n_cand, double* mean, double* var, int32_t* n_acc,
                           hipStream_t st) {
    int ncell = 0, ncand = 0;
    for (int l = 0; l < lv.n_levels; ++l) {
        ncell += lv.cells[l];
        ncand += (lv.cells[l] < lv.topk ? lv.cells[l] : lv.topk) * lv.anchors[l];
    }
    const size_t lds = (size_t)(ncell > ncand ? ncell : ncand) * 4;      // <= 4 P: both count distinct priors
    if (lds > 48 * 1024) {
        static std::atomic<unsigned long long> raised{0};                // one bit per device (common.h)
        int dev;
        if (ssd_attr_needed(raised, dev)) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(atss_assign_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    150 * 1024) != hipSuccess)
                return SSD_ERR_LAUNCH;
            ssd_attr_done(raised, dev);
        }
    }
    if (hipMemsetAsync(keys, 0, (size_t)bs * P * 8, st) != hipSuccess) return SSD_ERR_LAUNCH;
    hipLaunchKernelGGL(atss_assign_kernel, dim3(n_gt), dim3(AB), lds, st,
                       AtssArgs{gt, img_start, pri, pri_xyxy, keys, n_cand, mean, var, n_acc, bs, P, lv});
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}

extern "C" size_t ssd_atss_assign_workspace(int bs, int P) {
    if (bs <= 0 || P <= 0) return 0;
    return ssd_internal_atss_key_bytes(bs, P);
}

extern "C" int ssd_atss_assign(const float* gt_boxes, const int32_t* img_start, int bs, int n_gt, const float* priors_cxcywh,
                               const float* priors_xyxy, int P, int topk, int n_levels, const int* level_cells, const int* level_anchors,
                               int32_t* assign, int32_t* n_cand, double* mean, double* var, int32_t* n_acc, void* workspace,
                               size_t workspace_bytes, void* stream) {
    if (!gt_boxes || !img_start || !priors_cxcywh || !priors_xyxy || !assign || !workspace || !level_cells || !level_anchors)
        return SSD_ERR_NULL;
    if (bs <= 0 || n_gt <= 0 || P <= 0 || P > 36000) return SSD_ERR_BAD_SHAPE;
    AtssLevels lv;
    const int bad = ssd_internal_atss_levels(P, topk, n_levels, level_cells, level_anchors, lv);
    if (bad != SSD_OK) return bad;
    if (!ssd_aligned16(priors_xyxy) || !ssd_aligned16(workspace)) return SSD_ERR_ALIGN;
    if (workspace_bytes < ssd_internal_atss_key_bytes(bs, P)) return SSD_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(workspace);
    const int rc = ssd_internal_atss_keys(gt_boxes, img_start, bs, n_gt, priors_cxcywh, priors_xyxy, P, lv, keys, n_cand, mean, var, n_acc, st);
    if (rc != SSD_OK) return rc;
    hipLaunchKernelGGL(atss_unpack_kernel, dim3(ssd_cdiv(bs * P, 256)), dim3(256), 0, st, keys, assign, bs * P);
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}

// BatchNorm2d in training mode and Dropout / Dropout2d for SSD_resnet34's train forward and backward (reference Model.py:56-126 +
// torchvision BasicBlock): batch statistics, the normalise pass with its ReLU / residual / dropout variants, the backward of the
// head-section BatchNorms, and the counter-based dropout generator.
//
// All tensors are NHWC f32 rows [M][ld] of which the first C columns are the channels (the packed head buffer keeps its loc
// channels 0..4k-1 inside ld = pad32(25k)).  Every reduction is a fixed-order slab reduction -- no float atomics -- so a result is
// bitwise reproducible from run to run.
#include "common.h"

namespace {

// ---------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11).  Dropout element `idx` of site `site` draws word (idx & 3) of
// philox(counter = {lo32(idx >> 2), hi32(idx >> 2), site, 0}, key = {lo32(seed), hi32(seed)}) and is KEPT iff
// (word >> 8) * 2^-24 < 1 - p.  idx = row * C + c for elementwise Dropout (row = n*H*W + h*W + w, NHWC order) and n * C + c for
// Dropout2d, so the four channels of one 16-byte vector share one Philox call.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 philox4x32_10(uint4 ctr, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, ctr.x), lo0 = 0xD2511F53u * ctr.x;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, ctr.z), lo1 = 0xCD9E8D57u * ctr.z;
        ctr = make_uint4(hi1 ^ ctr.y ^ k0, lo1, hi0 ^ ctr.w ^ k1, lo0);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return ctr;
}

// keep flags of the four indices 4*q .. 4*q+3
__device__ __forceinline__ void dropout_keep4(uint64_t seed, int site, uint64_t q, float keep_p, bool keep[4]) {
    const uint4 r = philox4x32_10(make_uint4((uint32_t)q, (uint32_t)(q >> 32), (uint32_t)site, 0u), (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) keep[e] = (float)(w[e] >> 8) * 0x1p-24f < keep_p;
}

struct Drop {               // dropout of one site: mode 0 none, 1 elementwise (idx = row*C + c), 2 per (sample, channel) (idx = n*C + c)
    uint64_t seed;
    int site, mode, HW;
    float keep_p, scale;    // 1 - p, and 1/(1-p) (0 when p == 1: torch returns zeros)
};

// factor (0 or 1/(1-p)) of the four channels c4*4 .. c4*4+3 of row r
__device__ __forceinline__ void drop_factor4(const Drop& d, size_t r, int C, int c4, float f[4]) {
    if (d.mode == 0) {
        f[0] = f[1] = f[2] = f[3] = 1.f;
        return;
    }
    const uint64_t u = d.mode == 1 ? (uint64_t)r : (uint64_t)(r / (size_t)d.HW);
    bool k[4];
    dropout_keep4(d.seed, d.site, u * (uint64_t)(C / 4) + (uint64_t)c4, d.keep_p, k);
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = k[e] ? d.scale : 0.f;
}

// ---------------------------------------------------------------------------------------
// slab plan: a function of (M, C) only, so the reduction order -- and the result bits -- never depend on the device.
// A block covers up to 64 channel vectors (256 channels; blockIdx.y walks further chunks) and `lanes` interleaved rows of one slab.
// ---------------------------------------------------------------------------------------
constexpr int kThreads = 256;
constexpr int kMaxSlabs = 1024;

struct Plan {
    int cgb, lanes, chunks;
    size_t rows;            // rows per slab
    int nslab;
};

inline Plan plan_for(size_t M, int C) {
    Plan p;
    const int cg = C / 4;
    p.cgb = cg < 64 ? cg : 64;
    p.lanes = kThreads / p.cgb;
    p.chunks = (cg + p.cgb - 1) / p.cgb;
    size_t r = (M + kMaxSlabs - 1) / kMaxSlabs;
    const size_t rmin = (size_t)p.lanes * 16;
    p.rows = r > rmin ? r : rmin;
    p.nslab = (int)((M + p.rows - 1) / p.rows);
    return p;
}

__device__ __forceinline__ void chan_merge(float& n, float& mean, float& m2, float nb, float meanb, float m2b) {
    if (nb == 0.f) return;
    const float t = n + nb;
    const float d = meanb - mean;
    const float f = nb / t;
    mean += d * f;
    m2 += m2b + d * d * n * f;
    n = t;
}

// Per slab and channel: mean and M2 (sum of squared deviations) of the slab's rows.  Welford per thread over its rows, then the
// lanes merged by Chan's formula in lane order through LDS.  part[(slab*C + c)*2 + {0,1}] = {mean, M2}.
__global__ __launch_bounds__(kThreads) void bn_stats_kernel(const float* __restrict__ x, int ldx, size_t M, int C, int cgb, int lanes,
                                                            size_t rows_per_slab, float* __restrict__ part) {
    __shared__ float s_mean[kThreads * 4], s_m2[kThreads * 4];
    const int tid = threadIdx.x;
    const int cgl = tid % cgb, lane = tid / cgb;
    const int c4 = blockIdx.y * cgb + cgl;
    const bool active = lane < lanes && c4 < C / 4;
    const size_t r0 = (size_t)blockIdx.x * rows_per_slab;
    const size_t r1 = r0 + rows_per_slab < M ? r0 + rows_per_slab : M;
    float mean[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) {
        int k = 0;
        for (size_t r = r0 + lane; r < r1; r += lanes) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + r * (size_t)ldx + 4 * c4);
            const float inv = 1.f / (float)(++k);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = v[e] - mean[e];
                mean[e] += d * inv;
                m2[e] += d * (v[e] - mean[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        s_mean[tid * 4 + e] = mean[e];
        s_m2[tid * 4 + e] = m2[e];
    }
    __syncthreads();
    if (lane == 0 && c4 < C / 4) {
        const size_t rows = r1 - r0;
        float n = (float)((rows + lanes - 1) / lanes);
        for (int l = 1; l < lanes; ++l) {
            const size_t nl = rows > (size_t)l ? (rows - l + lanes - 1) / lanes : 0;
            const int t = l * cgb + cgl;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float nn = n;
                chan_merge(nn, mean[e], m2[e], (float)nl, s_mean[t * 4 + e], s_m2[t * 4 + e]);
            }
            n += (float)nl;
        }
        float* o = part + ((size_t)blockIdx.x * C + 4 * c4) * 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[2 * e] = mean[e];
            o[2 * e + 1] = m2[e];
        }
    }
}

// One block (64 threads) per channel: slabs merged strided per thread, then a fixed LDS tree.  Writes the batch mean / invstd of the
// normalisation, scale = gamma*invstd, shift = beta - mean*scale, and updates the running statistics (unbiased variance) and
// num_batches_tracked like torch's BatchNorm2d.train().
__global__ __launch_bounds__(64) void bn_finalize_kernel(const float* __restrict__ part, size_t M, int C, size_t rows_per_slab, int nslab,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                         float momentum, float* __restrict__ running_mean, float* __restrict__ running_var,
                                                         int64_t* __restrict__ num_batches_tracked, float* __restrict__ mean_out,
                                                         float* __restrict__ invstd_out, float* __restrict__ scale_out,
                                                         float* __restrict__ shift_out) {
    __shared__ float s_n[64], s_mean[64], s_m2[64];
    const int c = blockIdx.x, t = threadIdx.x;
    float n = 0.f, mean = 0.f, m2 = 0.f;
    for (int s = t; s < nslab; s += 64) {
        const size_t r0 = (size_t)s * rows_per_slab;
        const size_t rows = M - r0 < rows_per_slab ? M - r0 : rows_per_slab;
        const float* p = part + ((size_t)s * C + c) * 2;
        chan_merge(n, mean, m2, (float)rows, p[0], p[1]);     // from n = 0 this takes the slab's mean and M2 exactly
    }
    s_n[t] = n; s_mean[t] = mean; s_m2[t] = m2;
    __syncthreads();
    for (int w = 32; w > 0; w >>= 1) {
        if (t < w) {
            float a = s_n[t], am = s_mean[t], a2 = s_m2[t];
            chan_merge(a, am, a2, s_n[t + w], s_mean[t + w], s_m2[t + w]);
            s_n[t] = a; s_mean[t] = am; s_m2[t] = a2;
        }
        __syncthreads();
    }
    if (t == 0) {
        const float mu = s_mean[0], q = s_m2[0];
        const float var = q / (float)M;
        const float invstd = 1.f / sqrtf(var + eps);
        const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
        const float sc = g * invstd;
        mean_out[c] = mu;
        invstd_out[c] = invstd;
        scale_out[c] = sc;
        shift_out[c] = b - mu * sc;
        if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mu;
        if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (q / (float)(M - 1));
        if (c == 0 && num_batches_tracked) num_batches_tracked[0] += 1;
    }
}

// y = drop( act( x*scale + shift [+ res*res_scale + res_shift | + res] ) ),  act = ReLU or identity.  x may alias y.
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* x, int ldx, size_t M, int C, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, const float* res, int ldr,
                                                       const float* __restrict__ res_scale, const float* __restrict__ res_shift, int relu,
                                                       Drop d, float* y, int ldy) {
    const int C4 = C / 4;
    const size_t total = M * (size_t)C4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = i / C4;
        const int c4 = (int)(i % C4);
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + r * (size_t)ldx + 4 * c4);
        const f32x4 a = reinterpret_cast<const f32x4*>(scale)[c4], b = reinterpret_cast<const f32x4*>(shift)[c4];
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = v[e] * a[e] + b[e];
        if (res) {
            const f32x4 rv = *reinterpret_cast<const f32x4*>(res + r * (size_t)ldr + 4 * c4);
            if (res_scale) {
                const f32x4 ra = reinterpret_cast<const f32x4*>(res_scale)[c4], rb = reinterpret_cast<const f32x4*>(res_shift)[c4];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] += rv[e] * ra[e] + rb[e];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] += rv[e];
            }
        }
        if (relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = o[e] < 0.f ? 0.f : o[e];
        }
        float f[4];
        drop_factor4(d, r, C, c4, f);
        if (d.mode != 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] *= f[e];
        }
        *reinterpret_cast<f32x4*>(y + r * (size_t)ldy + 4 * c4) = o;
    }
}

// Backward, pass 1: per slab and channel, sum of g and of g*xhat, with g = dy * dropout factor and xhat = (x - mean)*invstd.
// Same slab plan and fixed lane order as bn_stats_kernel.  part[(slab*C + c)*2 + {0,1}] = {sum g, sum g*xhat}.
__global__ __launch_bounds__(kThreads) void bn_bwd_reduce_kernel(const float* __restrict__ dy, int ldd, const float* __restrict__ x, int ldx,
                                                                 size_t M, int C, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                 Drop d, int cgb, int lanes, size_t rows_per_slab, float* __restrict__ part) {
    __shared__ float s_g[kThreads * 4], s_gx[kThreads * 4];
    const int tid = threadIdx.x;
    const int cgl = tid % cgb, lane = tid / cgb;
    const int c4 = blockIdx.y * cgb + cgl;
    const bool active = lane < lanes && c4 < C / 4;
    const size_t r0 = (size_t)blockIdx.x * rows_per_slab;
    const size_t r1 = r0 + rows_per_slab < M ? r0 + rows_per_slab : M;
    float sg[4] = {0.f, 0.f, 0.f, 0.f}, sgx[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) {
        const f32x4 mu = reinterpret_cast<const f32x4*>(mean)[c4], is = reinterpret_cast<const f32x4*>(invstd)[c4];
        for (size_t r = r0 + lane; r < r1; r += lanes) {
            const f32x4 gv = *reinterpret_cast<const f32x4*>(dy + r * (size_t)ldd + 4 * c4);
            const f32x4 xv = *reinterpret_cast<const f32x4*>(x + r * (size_t)ldx + 4 * c4);
            float f[4];
            drop_factor4(d, r, C, c4, f);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float g = gv[e] * f[e];
                sg[e] += g;
                sgx[e] += g * ((xv[e] - mu[e]) * is[e]);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        s_g[tid * 4 + e] = sg[e];
        s_gx[tid * 4 + e] = sgx[e];
    }
    __syncthreads();
    if (lane == 0 && c4 < C / 4) {
        for (int l = 1; l < lanes; ++l) {
            const int t = l * cgb + cgl;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sg[e] += s_g[t * 4 + e];
                sgx[e] += s_gx[t * 4 + e];
            }
        }
        float* o = part + ((size_t)blockIdx.x * C + 4 * c4) * 2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[2 * e] = sg[e];
            o[2 * e + 1] = sgx[e];
        }
    }
}

// Backward, pass 2: one block per channel sums the slabs in a fixed order.  sums[c] = sum g (= dbeta), sums[C + c] = sum g*xhat
// (= dgamma); dgamma / dbeta (optional) are written, or added to when `accumulate`.
__global__ __launch_bounds__(64) void bn_bwd_finalize_kernel(const float* __restrict__ part, int C, int nslab, float* __restrict__ sums,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate) {
    __shared__ float s_g[64], s_gx[64];
    const int c = blockIdx.x, t = threadIdx.x;
    float g = 0.f, gx = 0.f;
    for (int s = t; s < nslab; s += 64) {
        const float* p = part + ((size_t)s * C + c) * 2;
        g += p[0];
        gx += p[1];
    }
    s_g[t] = g; s_gx[t] = gx;
    __syncthreads();
    for (int w = 32; w > 0; w >>= 1) {
        if (t < w) {
            s_g[t] += s_g[t + w];
            s_gx[t] += s_gx[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        sums[c] = s_g[0];
        sums[C + c] = s_gx[0];
        if (dbeta) dbeta[c] = accumulate ? dbeta[c] + s_g[0] : s_g[0];
        if (dgamma) dgamma[c] = accumulate ? dgamma[c] + s_gx[0] : s_gx[0];
    }
}

// Backward, pass 3: dx = gamma*invstd * (g - sum_g/M - xhat * sum_gxhat/M), then zeroed where x <= 0 when the BatchNorm follows a
// ReLU (x is the post-ReLU activation).  dx may alias dy.
__global__ __launch_bounds__(256) void bn_bwd_dx_kernel(const float* dy, int ldd, const float* __restrict__ x, int ldx, size_t M, int C,
                                                        const float* __restrict__ mean, const float* __restrict__ invstd,
                                                        const float* __restrict__ gamma, const float* __restrict__ sums, Drop d, int relu_mask,
                                                        float* dx, int lddx) {
    const int C4 = C / 4;
    const size_t total = M * (size_t)C4;
    const float invm = 1.f / (float)M;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = i / C4;
        const int c4 = (int)(i % C4);
        const f32x4 gv = *reinterpret_cast<const f32x4*>(dy + r * (size_t)ldd + 4 * c4);
        const f32x4 xv = *reinterpret_cast<const f32x4*>(x + r * (size_t)ldx + 4 * c4);
        const f32x4 mu = reinterpret_cast<const f32x4*>(mean)[c4], is = reinterpret_cast<const f32x4*>(invstd)[c4];
        const f32x4 ga = gamma ? reinterpret_cast<const f32x4*>(gamma)[c4] : f32x4{1.f, 1.f, 1.f, 1.f};
        const f32x4 sg = reinterpret_cast<const f32x4*>(sums)[c4], sgx = reinterpret_cast<const f32x4*>(sums + C)[c4];
        float f[4];
        drop_factor4(d, r, C, c4, f);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float xh = (xv[e] - mu[e]) * is[e];
            o[e] = ga[e] * is[e] * (gv[e] * f[e] - sg[e] * invm - xh * (sgx[e] * invm));
            if (relu_mask && !(xv[e] > 0.f)) o[e] = 0.f;
        }
        *reinterpret_cast<f32x4*>(dx + r * (size_t)lddx + 4 * c4) = o;
    }
}

// out[i] = keep flag of dropout index i (the testing aid behind SSD_resnet34.dropout_masks()), n % 4 == 0
__global__ __launch_bounds__(256) void dropout_mask_kernel(uint8_t* __restrict__ out, size_t n4, Drop d) {
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < n4; q += (size_t)gridDim.x * 256) {
        bool k[4];
        dropout_keep4(d.seed, d.site, q, d.keep_p, k);
        uchar4 o = make_uchar4(k[0], k[1], k[2], k[3]);
        reinterpret_cast<uchar4*>(out)[q] = o;
    }
}

inline int grid_for(size_t total, int block = 256, int cap = 4096) {
    size_t b = (total + block - 1) / block;
    return (int)(b > (size_t)cap ? cap : (b == 0 ? 1 : b));
}

inline int make_drop(Drop& d, int mode, float p, uint64_t seed, int site, int HW) {
    if (mode < 0 || mode > 2 || !(p >= 0.f && p <= 1.f) || site < 0 || (mode == 2 && HW <= 0)) return SSD_ERR_BAD_SHAPE;
    d.seed = seed;
    d.site = site;
    d.mode = mode;
    d.HW = HW > 0 ? HW : 1;
    d.keep_p = 1.f - p;
    d.scale = p < 1.f ? 1.f / (1.f - p) : 0.f;
    return SSD_OK;
}

inline bool rows_ok(const float* p, int ld, int C) { return p && ld >= C && ld % 4 == 0 && ssd_aligned16(p); }

}  // namespace

extern "C" size_t ssd_bn_workspace(size_t M, int C) {
    if (M == 0 || C <= 0 || C % 4 != 0) return 0;
    const Plan p = plan_for(M, C);
    return (size_t)p.nslab * C * 2 * sizeof(float);
}

extern "C" int ssd_bn_train_stats(const float* x, int ldx, size_t M, int C, const float* gamma, const float* beta, float eps,
                                  float momentum, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                                  float* mean, float* invstd, float* scale, float* shift, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    if (!x || !mean || !invstd || !scale || !shift || !workspace) return SSD_ERR_NULL;
    if (M < 2 || C <= 0 || C % 4 != 0 || ldx < C || ldx % 4 != 0 || !(eps > 0.f)) return SSD_ERR_BAD_SHAPE;
    if (!ssd_aligned16(x) || !ssd_aligned16(workspace)) return SSD_ERR_ALIGN;
    if (workspace_bytes < ssd_bn_workspace(M, C)) return SSD_ERR_WORKSPACE;
    const Plan p = plan_for(M, C);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(bn_stats_kernel, dim3(p.nslab, p.chunks), dim3(kThreads), 0, (hipStream_t)stream, x, ldx, M, C, p.cgb, p.lanes,
                       p.rows, part);
    SSD_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(C), dim3(64), 0, (hipStream_t)stream, part, M, C, p.rows, p.nslab, gamma, beta, eps,
                       momentum, running_mean, running_var, num_batches_tracked, mean, invstd, scale, shift);
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}

extern "C" int ssd_bn_apply(const float* x, int ldx, size_t M, int C, const float* scale, const float* shift, const float* res, int ldr,
                            const float* res_scale, const float* res_shift, int relu, int drop_mode, float p, uint64_t seed, int site,
                            int HW, float* y, int ldy, void* stream) {
    if (!x || !scale || !shift || !y) return SSD_ERR_NULL;
    if (M == 0 || C <= 0 || C % 4 != 0 || ldx < C || ldx % 4 != 0 || ldy < C || ldy % 4 != 0) return SSD_ERR_BAD_SHAPE;
    if (res && (ldr < C || ldr % 4 != 0)) return SSD_ERR_BAD_SHAPE;
    if ((res_scale == nullptr) != (res_shift == nullptr) || (res_scale && !res)) return SSD_ERR_BAD_SHAPE;
    if (!ssd_aligned16(x) || !ssd_aligned16(y) || !ssd_aligned16(scale) || !ssd_aligned16(shift)) return SSD_ERR_ALIGN;
    if ((res && !ssd_aligned16(res)) || (res_scale && (!ssd_aligned16(res_scale) || !ssd_aligned16(res_shift)))) return SSD_ERR_ALIGN;
    Drop d;
    const int st = make_drop(d, drop_mode, p, seed, site, HW);
    if (st != SSD_OK) return st;
    if (drop_mode == 2 && M % (size_t)HW != 0) return SSD_ERR_BAD_SHAPE;
    hipLaunchKernelGGL(bn_apply_kernel, dim3(grid_for(M * (size_t)(C / 4))), dim3(256), 0, (hipStream_t)stream, x, ldx, M, C, scale, shift,
                       res, ldr, res_scale, res_shift, relu, d, y, ldy);
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}

extern "C" int ssd_bn_train_bwd(const float* dy, int ldd, const float* x, int ldx, size_t M, int C, const float* mean, const float* invstd,
                                const float* gamma, int drop_mode, float p, uint64_t seed, int site, int HW, int relu_mask, float* sums,
                                float* dgamma, float* dbeta, int accumulate, float* dx, int lddx, void* workspace, size_t workspace_bytes,
                                void* stream) {
    if (!dy || !x || !mean || !invstd || !sums || !workspace) return SSD_ERR_NULL;
    if (M < 2 || C <= 0 || C % 4 != 0 || !rows_ok(dy, ldd, C) || !rows_ok(x, ldx, C)) return SSD_ERR_BAD_SHAPE;
    if (dx && !rows_ok(dx, lddx, C)) return SSD_ERR_BAD_SHAPE;
    if (!ssd_aligned16(mean) || !ssd_aligned16(invstd) || !ssd_aligned16(sums) || !ssd_aligned16(workspace) ||
        (gamma && !ssd_aligned16(gamma)))
        return SSD_ERR_ALIGN;
    if (workspace_bytes < ssd_bn_workspace(M, C)) return SSD_ERR_WORKSPACE;
    Drop d;
    const int st = make_drop(d, drop_mode, p, seed, site, HW);
    if (st != SSD_OK) return st;
    if (drop_mode == 2 && M % (size_t)HW != 0) return SSD_ERR_BAD_SHAPE;
    const Plan pl = plan_for(M, C);
    float* part = static_cast<float*>(workspace);
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(pl.nslab, pl.chunks), dim3(kThreads), 0, (hipStream_t)stream, dy, ldd, x, ldx, M, C, mean,
                       invstd, d, pl.cgb, pl.lanes, pl.rows, part);
    SSD_CHECK_LAUNCH();
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(64), 0, (hipStream_t)stream, part, C, pl.nslab, sums, dgamma, dbeta, accumulate);
    SSD_CHECK_LAUNCH();
    if (dx) {
        hipLaunchKernelGGL(bn_bwd_dx_kernel, dim3(grid_for(M * (size_t)(C / 4))), dim3(256), 0, (hipStream_t)stream, dy, ldd, x, ldx, M, C,
                           mean, invstd, gamma, sums, d, relu_mask, dx, lddx);
        SSD_CHECK_LAUNCH();
    }
    return SSD_OK;
}

extern "C" int ssd_dropout_mask(uint8_t* out, size_t n, float p, uint64_t seed, int site, void* stream) {
    if (!out) return SSD_ERR_NULL;
    if (n == 0 || n % 4 != 0) return SSD_ERR_BAD_SHAPE;
    if (((uintptr_t)out & 3u) != 0) return SSD_ERR_ALIGN;
    Drop d;
    const int st = make_drop(d, 1, p, seed, site, 1);
    if (st != SSD_OK) return st;
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, out, n / 4, d);
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}

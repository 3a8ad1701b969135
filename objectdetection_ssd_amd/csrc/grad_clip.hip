// Global gradient norm of the flat f32 gradient buffers, the clip coefficient of torch.nn.utils.clip_grad_norm_ and the non-finite
// step guard, all on the device: one streaming pass per contiguous range (per-workgroup partials), one single-workgroup finalise.
// The fused SGD step (elementwise.hip) consumes the resulting `grad_scale` and `skip` words; nothing here comes back to the host.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NORM_THREADS = 256;
constexpr int NORM_UNROLL = 4;        // independent 16-byte loads a thread has in flight
constexpr int NORM_MAX_BLOCKS = 1024; // 4 workgroups (16 waves) per CU on 256 CUs; one pass of the full grid covers 4,194,304 floats

// The grid depends on n alone, every thread walks a fixed set of elements in a fixed order, and the partials of a workgroup are
// combined by a fixed butterfly + a fixed 4-term sum: no floating-point atomics, the same bits on every run.
inline int norm_blocks(size_t n) {
    const size_t per = (size_t)NORM_THREADS * NORM_UNROLL * 4;
    const size_t b = (n + per - 1) / per;
    return (int)(b > (size_t)NORM_MAX_BLOCKS ? NORM_MAX_BLOCKS : b);
}

template <int KIND>
struct NormAcc {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;       // KIND 0: sums of squares (an f32 squared is exact in f64)
    float m = 0.f;                                       // KIND 1: max |g| ...
    int bad = 0;                                         // ... and whether a NaN was seen (fmaxf drops NaNs)
    __device__ __forceinline__ void add(const f32x4 v) {
        if (KIND == 0) {
            const double a = (double)v[0], b = (double)v[1], c = (double)v[2], d = (double)v[3];
            s0 += a * a;
            s1 += b * b;
            s2 += c * c;
            s3 += d * d;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float t = __builtin_fabsf(v[e]);
                bad |= (t != t) ? 1 : 0;
                m = __builtin_fmaxf(m, t);
            }
        }
    }
};

// partial of one workgroup -> out[blockIdx.x]: the sum of squares, or max |g| widened to f64 (NaN if the range holds a NaN)
template <int KIND>
__global__ __launch_bounds__(NORM_THREADS) void norm_partials_kernel(const f32x4* __restrict__ g, size_t n4, double* __restrict__ out) {
    const size_t stride = (size_t)gridDim.x * NORM_THREADS;
    size_t i = (size_t)blockIdx.x * NORM_THREADS + threadIdx.x;
    NormAcc<KIND> acc;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const f32x4 a = g[i], b = g[i + stride], c = g[i + 2 * stride], d = g[i + 3 * stride];
        acc.add(a);
        acc.add(b);
        acc.add(c);
        acc.add(d);
    }
    for (; i < n4; i += stride) acc.add(g[i]);

    __shared__ double sh[NORM_THREADS / 64];
    __shared__ int sh_bad[NORM_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double s;
    int bad = acc.bad;
    if (KIND == 0) {
        s = (acc.s0 + acc.s1) + (acc.s2 + acc.s3);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    } else {
        float m = acc.m;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            m = __builtin_fmaxf(m, __shfl_xor(m, o, 64));
            bad |= __shfl_xor(bad, o, 64);
        }
        s = (double)m;
    }
    if (lane == 0) {
        sh[wave] = s;
        sh_bad[wave] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double r;
        if (KIND == 0) {
            r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
        } else {
            r = __builtin_fmax(__builtin_fmax(sh[0], sh[1]), __builtin_fmax(sh[2], sh[3]));
            if (sh_bad[0] | sh_bad[1] | sh_bad[2] | sh_bad[3]) r = __builtin_nan("");
        }
        out[blockIdx.x] = r;
    }
}

// One workgroup: thread t folds slots t, t+256, ... in index order, a fixed tree folds the 256 threads; thread 0 does the scalar part.
__global__ __launch_bounds__(256) void clip_finalize_kernel(const double* __restrict__ partials, int n_slots, int kind, float max_norm,
                                                            const float* __restrict__ pre_scale, int guard, float* __restrict__ state) {
    __shared__ double sh[256];
    __shared__ int sh_bad[256];
    const int t = threadIdx.x;
    double acc = 0.0;
    int bad = 0;
    for (int i = t; i < n_slots; i += 256) {
        const double v = partials[i];
        if (kind == 0) {
            acc += v;
        } else {
            bad |= (v != v) ? 1 : 0;
            acc = __builtin_fmax(acc, v);
        }
    }
    sh[t] = acc;
    sh_bad[t] = bad;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            if (kind == 0) sh[t] = sh[t] + sh[t + o];
            else sh[t] = __builtin_fmax(sh[t], sh[t + o]);
            sh_bad[t] |= sh_bad[t + o];
        }
        __syncthreads();
    }
    if (t != 0) return;
    const float pre = pre_scale ? *pre_scale : 1.f;
    float total;
    if (kind == 0) {
        total = (float)(__builtin_sqrt(sh[0]) * (double)pre);
    } else {
        const float mx = sh_bad[0] ? __builtin_nanf("") : (float)sh[0];
        total = pre_scale ? mx * pre : mx;
    }
    // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6); clamp(clip_coef, max=1.0).  A number divided by a
    // tensor is, in torch, the tensor's reciprocal times the number: two roundings, reproduced here; clamp keeps a NaN.
    float coef = 1.f;
    if (max_norm >= 0.f) {
        const float c = (1.f / (total + 1e-6f)) * max_norm;
        coef = c > 1.f ? 1.f : c;
    }
    const float scale = pre_scale ? pre * coef : coef;
    const int skip = (guard && !(__builtin_fabsf(total) <= 3.402823466e38f)) ? 1 : 0;      // not finite: Inf or NaN
    int* istate = reinterpret_cast<int*>(state);
    state[0] = total;
    state[1] = coef;
    state[2] = scale;
    istate[3] = skip;
    istate[4] = istate[4] + skip;
}

}  // namespace

extern "C" int ssd_grad_norm_slots(size_t n) { return norm_blocks(n); }

extern "C" int ssd_grad_norm_partials(const float* grad, size_t n, int norm_kind, double* partials, int slot0, int slot_capacity,
                                      void* stream) {
    if (!grad || !partials) return SSD_ERR_NULL;
    if ((norm_kind != 0 && norm_kind != 1) || (n & 3) != 0 || slot0 < 0) return SSD_ERR_BAD_SHAPE;
    if (!ssd_aligned16(grad) || (reinterpret_cast<uintptr_t>(partials) & 7u) != 0) return SSD_ERR_ALIGN;
    const int blocks = norm_blocks(n);
    if ((long long)slot0 + blocks > (long long)slot_capacity) return SSD_ERR_WORKSPACE;
    if (n == 0) return SSD_OK;
    const f32x4* g4 = reinterpret_cast<const f32x4*>(grad);
    if (norm_kind == 0)
        hipLaunchKernelGGL((norm_partials_kernel<0>), dim3(blocks), dim3(NORM_THREADS), 0, (hipStream_t)stream, g4, n / 4, partials + slot0);
    else
        hipLaunchKernelGGL((norm_partials_kernel<1>), dim3(blocks), dim3(NORM_THREADS), 0, (hipStream_t)stream, g4, n / 4, partials + slot0);
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}

extern "C" int ssd_grad_clip_finalize(const double* partials, int n_slots, int norm_kind, float max_norm, const float* pre_scale_dev,
                                      int guard, float* state, void* stream) {
    if (!partials || !state) return SSD_ERR_NULL;
    if ((norm_kind != 0 && norm_kind != 1) || n_slots < 0 || max_norm != max_norm) return SSD_ERR_BAD_SHAPE;
    if ((reinterpret_cast<uintptr_t>(partials) & 7u) != 0 || (reinterpret_cast<uintptr_t>(state) & 3u) != 0) return SSD_ERR_ALIGN;
    hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n_slots, norm_kind, max_norm,
                       pre_scale_dev, guard != 0 ? 1 : 0, state);
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}

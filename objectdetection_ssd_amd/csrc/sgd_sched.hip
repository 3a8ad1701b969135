// Device-resident learning-rate schedule and weight EMA of the fused SGD step.  The learning rate is a device word the SGD launch
// reads, a device step counter indexes a host-built table of rates, and the exponential moving average of the weights is updated in
// the pass over the parameters that SGD already makes.  Nothing here depends on a host value that changes from step to step, so a
// captured train step (ddp.GraphedTrainStep) replays under any per-iteration schedule.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SCHED_THREADS = 256;
constexpr int SCHED_MAX_BLOCKS = 2048;   // 8 workgroups (32 waves) per CU on 256 CUs: the whole grid is resident, the rest is grid-stride

// One pass of the full grid covers SCHED_MAX_BLOCKS * SCHED_THREADS units: 16-byte units (4 floats) in the vector kernels, floats in
// the scalar ones.
inline int sched_blocks(size_t units) {
    const size_t b = (units + SCHED_THREADS - 1) / SCHED_THREADS;
    return (int)(b > (size_t)SCHED_MAX_BLOCKS ? SCHED_MAX_BLOCKS : (b ? b : 1));
}

// state: [0] step (int32) | [1] ema_w (f32) | [2 .. 2+G) lr[g] (f32).  One workgroup; every thread reads the counter before thread 0
// replaces it.
__global__ __launch_bounds__(SCHED_THREADS) void schedule_advance_kernel(int* __restrict__ state, const float* __restrict__ lr_table, int G,
                                                                         int T, double ema_decay, int ema_warmup,
                                                                         const int* __restrict__ skip) {
    if (skip && *skip != 0) return;
    const int t = state[0];
    __syncthreads();
    const int col = t < 0 ? 0 : (t < T - 1 ? t : T - 1);
    float* fstate = reinterpret_cast<float*>(state);
    for (int g = threadIdx.x; g < G; g += SCHED_THREADS) fstate[2 + g] = lr_table[(size_t)g * T + col];
    if (threadIdx.x != 0) return;
    float w = 0.f;
    if (ema_decay >= 0.0) {
        double d = ema_decay;
        if (ema_warmup) {
            const double r = (1.0 + (double)t) / (10.0 + (double)t);
            d = r < d ? r : d;
        }
        w = (float)(1.0 - d);
    }
    fstate[1] = w;
    state[0] = t + 1;
}

// torch.optim.SGD's rounding sequence, exactly that of sgd_kernel (elementwise.hip); then, with EMA, three separately rounded f32
// operations on the parameter just formed.
template <bool EMA>
__device__ __forceinline__ void sgd_element(float& w, const float g, float& b, float& e, const float sc, const bool scaled,
                                            const float neg_lr, const float mom, const float wd, const int first, const float ema_w) {
    const float gs = scaled ? g * sc : g;
    const float d = wd != 0.f ? __builtin_fmaf(wd, w, gs) : gs;
    float nb = d;
    if (!first) {
        const float mb = mom * b;
        nb = mb + d;
    }
    b = nb;
    w = __builtin_fmaf(neg_lr, nb, w);
    if (EMA) {
        const float diff = w - e;
        const float m = ema_w * diff;
        e = e + m;
    }
}

// VEC: the ranges are 16-byte aligned and a multiple of 4 floats long, `n` counts 16-byte units.  Seven dword streams per element
// with EMA (p, g, buf, e in; p, buf, e out), five without; on the first step the momentum buffer is not read.
// Gradient, momentum and EMA are touched once per step and by nothing else before the next one: their vector accesses are
// non-temporal, so they do not push the parameters -- which the next forward reads first -- out of the caches.  On the 105 MB
// buffers streamed from HBM that was 9 % faster than plain accesses throughout and 4 % faster than all seven streams non-temporal.
template <bool VEC, bool EMA>
__global__ __launch_bounds__(SCHED_THREADS) void sgd_sched_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                                  float* __restrict__ ema, size_t n, const float* __restrict__ lr_dev,
                                                                  const float* __restrict__ ema_w_dev, float mom, float wd,
                                                                  const float* __restrict__ scale, int first, const int* __restrict__ skip) {
    if (skip && *skip != 0) return;
    const float sc = scale ? *scale : 1.f;
    const bool scaled = scale != nullptr;
    const float neg_lr = -(*lr_dev);
    const float ema_w = EMA ? *ema_w_dev : 0.f;
    const size_t stride = (size_t)gridDim.x * SCHED_THREADS;
    for (size_t i = (size_t)blockIdx.x * SCHED_THREADS + threadIdx.x; i < n; i += stride) {
        if (VEC) {
            f32x4* p4 = reinterpret_cast<f32x4*>(p);
            f32x4* b4 = reinterpret_cast<f32x4*>(buf);
            f32x4* e4 = reinterpret_cast<f32x4*>(ema);
            f32x4 w = p4[i];
            const f32x4 gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g) + i);
            f32x4 b = {0.f, 0.f, 0.f, 0.f}, e = {0.f, 0.f, 0.f, 0.f};
            if (!first) b = __builtin_nontemporal_load(b4 + i);
            if (EMA) e = __builtin_nontemporal_load(e4 + i);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float wk = w[k], bk = b[k], ek = e[k];
                sgd_element<EMA>(wk, gv[k], bk, ek, sc, scaled, neg_lr, mom, wd, first, ema_w);
                w[k] = wk;
                b[k] = bk;
                e[k] = ek;
            }
            __builtin_nontemporal_store(b, b4 + i);
            p4[i] = w;
            if (EMA) __builtin_nontemporal_store(e, e4 + i);
        } else {
            float w = p[i], b = first ? 0.f : buf[i], e = EMA ? ema[i] : 0.f;
            sgd_element<EMA>(w, g[i], b, e, sc, scaled, neg_lr, mom, wd, first, ema_w);
            buf[i] = b;
            p[i] = w;
            if (EMA) ema[i] = e;
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(SCHED_THREADS) void swap_kernel(float* __restrict__ a, float* __restrict__ b, size_t n) {
    const size_t stride = (size_t)gridDim.x * SCHED_THREADS;
    for (size_t i = (size_t)blockIdx.x * SCHED_THREADS + threadIdx.x; i < n; i += stride) {
        if (VEC) {
            f32x4* a4 = reinterpret_cast<f32x4*>(a);
            f32x4* b4 = reinterpret_cast<f32x4*>(b);
            const f32x4 x = a4[i], y = b4[i];
            a4[i] = y;
            b4[i] = x;
        } else {
            const float x = a[i], y = b[i];
            a[i] = y;
            b[i] = x;
        }
    }
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace

extern "C" int ssd_sgd_schedule_advance(void* state, const float* lr_table, int G, int T, double ema_decay, int ema_warmup,
                                        const int* skip_dev, void* stream) {
    if (!state || !lr_table) return SSD_ERR_NULL;
    if (G <= 0 || T <= 0 || ema_decay != ema_decay || ema_decay >= 1.0) return SSD_ERR_BAD_SHAPE;
    if (!aligned4(state) || !aligned4(lr_table) || !aligned4(skip_dev)) return SSD_ERR_ALIGN;
    hipLaunchKernelGGL(schedule_advance_kernel, dim3(1), dim3(SCHED_THREADS), 0, (hipStream_t)stream, static_cast<int*>(state), lr_table, G, T,
                       ema_decay, ema_warmup != 0 ? 1 : 0, skip_dev);
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}

extern "C" int ssd_sgd_momentum_sched(float* param, const float* grad, float* buf, float* ema, size_t n, const float* lr_dev,
                                      const float* ema_w_dev, float momentum, float weight_decay, const float* grad_scale_dev,
                                      int first_step, const int* skip_dev, void* stream) {
    if (!param || !grad || !buf || !lr_dev || (ema && !ema_w_dev)) return SSD_ERR_NULL;
    if (!aligned4(param) || !aligned4(grad) || !aligned4(buf) || !aligned4(ema)) return SSD_ERR_ALIGN;
    if (n == 0) return SSD_OK;
    const bool vec = (n & 3) == 0 && ssd_aligned16(param) && ssd_aligned16(grad) && ssd_aligned16(buf) && ssd_aligned16(ema);
    const size_t units = vec ? n / 4 : n;
    const dim3 grid(sched_blocks(units)), block(SCHED_THREADS);
    hipStream_t st = (hipStream_t)stream;
    const int first = first_step != 0 ? 1 : 0;
#define SSD_SCHED_LAUNCH(V, E)                                                                                                          \
    hipLaunchKernelGGL((sgd_sched_kernel<V, E>), grid, block, 0, st, param, grad, buf, ema, units, lr_dev, ema_w_dev, momentum, weight_decay, \
                       grad_scale_dev, first, skip_dev)
    if (vec) {
        if (ema) SSD_SCHED_LAUNCH(true, true);
        else SSD_SCHED_LAUNCH(true, false);
    } else {
        if (ema) SSD_SCHED_LAUNCH(false, true);
        else SSD_SCHED_LAUNCH(false, false);
    }
#undef SSD_SCHED_LAUNCH
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}

extern "C" int ssd_swap_f32(float* a, float* b, size_t n, void* stream) {
    if (!a || !b) return SSD_ERR_NULL;
    if (!aligned4(a) || !aligned4(b)) return SSD_ERR_ALIGN;
    if (n == 0) return SSD_OK;
    const uintptr_t ua = reinterpret_cast<uintptr_t>(a), ub = reinterpret_cast<uintptr_t>(b);
    if ((ua <= ub ? ub - ua : ua - ub) < n * sizeof(float)) return SSD_ERR_BAD_SHAPE;       // the ranges overlap
    const bool vec = (n & 3) == 0 && ssd_aligned16(a) && ssd_aligned16(b);
    const size_t units = vec ? n / 4 : n;
    if (vec) hipLaunchKernelGGL((swap_kernel<true>), dim3(sched_blocks(units)), dim3(SCHED_THREADS), 0, (hipStream_t)stream, a, b, units);
    else hipLaunchKernelGGL((swap_kernel<false>), dim3(sched_blocks(units)), dim3(SCHED_THREADS), 0, (hipStream_t)stream, a, b, units);
    SSD_CHECK_LAUNCH();
    return SSD_OK;
}
